"""float64 numpy yardsticks of the reconstruction-evaluation kernels and tools (csrc/nearest.hip, csrc/mesh_depth.hip,
evennicer_slam_amd/eval_recon.py): brute-force nearest neighbour, a Moeller-Trumbore ray caster that also reports how close
each ray passes to a triangle edge, point-to-point ICP with cKDTree, and the frustum test and culling rule of the
reference's tools (check_proj, cull_mesh.py) in float32 numpy."""
import numpy as np
from scipy.spatial import cKDTree


def nearest(query, ref, block=512):
    """(dist float64 [M], idx int64 [M]): np.sqrt(((q - r) ** 2).sum(-1)) over all pairs, argmin (the first minimum)"""
    q, r = np.asarray(query, np.float64), np.asarray(ref, np.float64)
    dist, idx = np.empty(len(q)), np.empty(len(q), np.int64)
    for lo in range(0, len(q), block):
        d = np.sqrt(((q[lo:lo + block, None, :] - r[None, :, :]) ** 2).sum(-1))
        idx[lo:lo + block] = d.argmin(1)
        dist[lo:lo + block] = d[np.arange(d.shape[0]), idx[lo:lo + block]]
    return dist, idx


def pixel_rays(c2w, cam):
    """(origin [3], directions [H,W,3]) of a camera-to-world matrix: direction ((i - cx) / fx, -(j - cy) / fy, -1) rotated"""
    c2w = np.asarray(c2w, np.float64)
    j, i = np.meshgrid(np.arange(cam['H'], dtype=np.float64), np.arange(cam['W'], dtype=np.float64), indexing='ij')
    d = np.stack([(i - cam['cx']) / cam['fx'], -(j - cam['cy']) / cam['fy'], -np.ones_like(i)], -1)
    return c2w[:3, 3], d @ c2w[:3, :3].T


def ray_cast(vertices, faces, c2w, cam, z_near=0.0, z_far=20.0):
    """(depth float64 [H,W], margin float64 [H,W]) by Moeller-Trumbore in world space: depth is the smallest ray parameter t,
    z_near < t <= z_far, with barycentric u >= 0, v >= 0, u + v <= 1 over the non-degenerate triangles (both sides), 0 where
    there is none; margin is, per pixel, the smallest min(|u|, |v|, |1 - u - v|) over all non-degenerate triangles with t > 0
    (how close the ray passes to the line of an edge of a triangle in front of it)."""
    v, f = np.asarray(vertices, np.float64), np.asarray(faces)
    o, d = pixel_rays(c2w, cam)
    depth = np.full(d.shape[:2], np.inf)
    margin = np.full(d.shape[:2], np.inf)
    for a, b, c in f:
        e1, e2 = v[b] - v[a], v[c] - v[a]
        p = np.cross(d, e2)
        det = p @ e1
        ok = det != 0.0
        with np.errstate(divide='ignore', invalid='ignore'):
            s = o - v[a]
            bu = (p @ s) / det
            q = np.cross(s, e1)
            bv = (d @ q) / det
            t = (q @ e2) / det
        front = ok & (t > 0)
        m = np.minimum(np.minimum(np.abs(bu), np.abs(bv)), np.abs(1.0 - bu - bv))
        margin = np.where(front, np.minimum(margin, m), margin)
        hit = ok & (bu >= 0) & (bv >= 0) & (bu + bv <= 1) & (t > z_near) & (t <= z_far)
        depth = np.where(hit, np.minimum(depth, t), depth)
    return np.where(np.isfinite(depth), depth, 0.0), margin


def kabsch(s, d):
    """4x4: the least-squares rigid motion of the paired points s -> d (SVD, reflection guard)"""
    mu_s, mu_d = s.mean(0), d.mean(0)
    U, _, Vt = np.linalg.svd((s - mu_s).T @ (d - mu_d))
    D = np.diag([1.0, 1.0, 1.0 if np.linalg.det(Vt.T @ U.T) >= 0 else -1.0])
    T = np.eye(4)
    T[:3, :3] = Vt.T @ D @ U.T
    T[:3, 3] = mu_d - T[:3, :3] @ mu_s
    return T


def icp(src, dst, threshold=0.1, max_iter=30, tol=1e-6):
    """(4x4, iterations, fitness, rmse): Open3D's point-to-point registration_icp from the identity, with cKDTree"""
    src, dst = np.array(src, np.float64), np.asarray(dst, np.float64)
    tree = cKDTree(dst)

    def match(p):
        d, i = tree.query(p)
        ok = d < threshold
        n = int(ok.sum())
        return ok, i, n / len(p), float(np.sqrt((d[ok] ** 2).sum() / n)) if n else 0.0

    T = np.eye(4)
    ok, idx, fit, rmse = match(src)
    it = 0
    while it < max_iter and ok.any():
        step = kabsch(src[ok], dst[idx[ok]])
        T = step @ T
        src = src @ step[:3, :3].T + step[:3, 3]
        it += 1
        ok, idx, fit2, rmse2 = match(src)
        done = abs(fit2 - fit) < tol and abs(rmse2 - rmse) < tol
        fit, rmse = fit2, rmse2
        if done:
            break
    return T, it, fit, rmse


def check_proj(points, cam, c2w):
    """bool [P]: which points one camera of the reference's check_proj / cull_mesh.py has in its frustum, in float32 numpy, one
    component at a time: the world-to-camera matrix (inverted in the dtype c2w comes in, then float32) applied to the float32
    points, the x axis turned round, the pinhole projection with 1e-5 added to the depth term before the division, and the
    open image rectangle for points that are not behind the camera.  c2w is the camera-to-world matrix in this project's axes
    (the camera looks down -z)."""
    f32 = np.float32
    m = np.linalg.inv(np.asarray(c2w)).astype(f32)
    x, y, z = np.asarray(points, np.float64).astype(f32).T
    right, up, back = (m[r, 0] * x + m[r, 1] * y + m[r, 2] * z + m[r, 3] for r in range(3))
    right = -right
    depth = back + f32(1e-5)
    with np.errstate(divide='ignore', invalid='ignore'):
        u = (f32(cam['fx']) * right + f32(cam['cx']) * back) / depth
        v = (f32(cam['fy']) * up + f32(cam['cy']) * back) / depth
    return (depth <= 0) & (u > 0) & (u < cam['W']) & (v > 0) & (v < cam['H'])


def cull_faces(vertices, faces, c2w_list, cam):
    """the faces the reference's cull_mesh.py keeps: a face goes when every one of its vertices is outside every frustum"""
    unseen = np.ones(len(vertices), bool)
    for c2w in c2w_list:
        unseen &= ~check_proj(vertices, cam, c2w)
    faces = np.asarray(faces)
    return faces[~unseen[faces].all(axis=1)]
