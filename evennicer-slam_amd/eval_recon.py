"""Reconstruction metrics of the reference's src/tools/eval_recon.py and the mesh culling of its src/tools/cull_mesh.py:
accuracy, completion and completion ratio of surface samples after an ICP alignment, and the depth L1 of random views.

Point sets are numpy arrays (the scipy.spatial.cKDTree route, as the reference) or float64 tensors on a HIP device (the
exact nearest-neighbour kernel, functional.nearest).  Distances are in the units of the points (metres for the reference).
On a CPU device everything but the depth renderer has a host route; `calc_2d_metric` needs a HIP device.

Two documented differences from the reference tool: the depth renderer's near plane is z_near = 0 (Open3D derives its near
plane from the scene's bounding box), and the box the random views are drawn from is an argument (`view_box` gives the
axis-aligned box of the ground-truth mesh; the reference fits an oriented box with trimesh.bounds.oriented_bounds)."""
import numpy as np
import torch
from scipy.spatial import cKDTree as KDTree


def _on_hip(*ts):
    return all(torch.is_tensor(t) and t.is_cuda for t in ts)


def _np(t):
    return t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)


def _nearest_distances(query, ref):
    """distances of `query` to `ref`: a float64 tensor through functional.nearest for HIP tensors, else numpy through cKDTree"""
    if _on_hip(query, ref):
        from . import functional as EF
        return EF.nearest(query.double(), ref.double())[0]
    distances, _ = KDTree(_np(ref)).query(_np(query))
    return distances


def completion_ratio(gt_points, rec_points, dist_th=0.05):
    """Fraction of the ground-truth points within dist_th of a reconstructed point."""
    if _on_hip(gt_points, rec_points):
        return float((_nearest_distances(gt_points, rec_points) < dist_th).double().mean())
    distances, _ = KDTree(rec_points).query(gt_points)
    return float(np.mean((distances < dist_th).astype(np.float64)))


def accuracy(gt_points, rec_points):
    """Mean distance of the reconstructed points to the ground truth."""
    if _on_hip(gt_points, rec_points):
        return float(_nearest_distances(rec_points, gt_points).mean())
    distances, _ = KDTree(gt_points).query(rec_points)
    return float(np.mean(distances))


def completion(gt_points, rec_points):
    """Mean distance of the ground-truth points to the reconstruction."""
    if _on_hip(gt_points, rec_points):
        return float(_nearest_distances(gt_points, rec_points).mean())
    distances, _ = KDTree(rec_points).query(gt_points)
    return float(np.mean(distances))


# ---- meshes -----------------------------------------------------------------------------------------------------------------
_PLY_TYPES = {'char': 'i1', 'int8': 'i1', 'uchar': 'u1', 'uint8': 'u1', 'short': 'i2', 'int16': 'i2', 'ushort': 'u2',
              'uint16': 'u2', 'int': 'i4', 'int32': 'i4', 'uint': 'u4', 'uint32': 'u4', 'float': 'f4', 'float32': 'f4',
              'double': 'f8', 'float64': 'f8'}


def _split_polygons(counts, flat):
    """int32 [F',3]: triangles as they are, quads (a, b, c, d) as (a, b, c) and (a, c, d), in file order"""
    counts = np.asarray(counts, np.int64)
    if ((counts != 3) & (counts != 4)).any():
        bad = int(counts[(counts != 3) & (counts != 4)][0])
        raise ValueError(f"load_mesh reads triangles and quads only (the file has a face with {bad} vertices)")
    start = np.concatenate([[0], np.cumsum(counts)[:-1]])
    n_out = counts - 2
    first = np.repeat(start, n_out)                                 # index of vertex a of each output triangle
    k = np.arange(int(n_out.sum())) - np.repeat(np.cumsum(n_out) - n_out, n_out)       # 0, or 0 and 1 for a quad
    flat = np.asarray(flat)
    return np.stack([flat[first], flat[first + 1 + k], flat[first + 2 + k]], 1).astype(np.int32)


def load_mesh(path):
    """(vertices float64 [V,3], faces int32 [F,3], colours uint8 [V,3] or None) of a PLY file, read by its header:
    binary_little_endian or ascii, any scalar vertex properties (x, y, z and red, green, blue are kept), a face element
    whose one property is a list with a uchar count and int32 / uint32 indices.  Quads are split into two triangles; any
    other polygon, a big-endian file or another layout raises ValueError.  Elements after the faces are ignored."""
    with open(path, "rb") as fh:
        data = fh.read()
    if not data.startswith(b"ply"):
        raise ValueError(f"{path} is not a PLY file")
    try:
        end = data.index(b"end_header")
        end = data.index(b"\n", end) + 1
    except ValueError:
        raise ValueError(f"{path}: the PLY header has no end_header line") from None
    fmt, elements = None, []
    for line in data[:end].decode("ascii", "replace").splitlines():
        w = line.split()
        if not w or w[0] in ("ply", "comment", "obj_info", "end_header"):
            continue
        if w[0] == "format":
            fmt = w[1]
        elif w[0] == "element":
            elements.append((w[1], int(w[2]), []))
        elif w[0] == "property" and elements:
            elements[-1][2].append(w[1:])
        else:
            raise ValueError(f"{path}: unexpected header line {line!r}")
    if fmt not in ("binary_little_endian", "ascii"):
        raise ValueError(f"{path}: format {fmt!r} is not supported (binary_little_endian and ascii are)")
    if len(elements) < 1 or elements[0][0] != "vertex" or (len(elements) > 1 and elements[1][0] != "face"):
        raise ValueError(f"{path}: expected the elements vertex and face, in this order "
                         f"(got {[e[0] for e in elements]})")
    _, V, vprops = elements[0]
    if any(p[0] == "list" or p[0] not in _PLY_TYPES for p in vprops):
        raise ValueError(f"{path}: the vertex element has a property that is not a scalar")
    names = [p[1] for p in vprops]
    if not all(a in names for a in "xyz"):
        raise ValueError(f"{path}: the vertex element lacks x, y or z")
    F, fprops = (elements[1][1], elements[1][2]) if len(elements) > 1 else (0, [])
    if F:
        if len(fprops) != 1 or fprops[0][0] != "list" or _PLY_TYPES.get(fprops[0][1]) != 'u1' or \
                _PLY_TYPES.get(fprops[0][2]) not in ('i4', 'u4'):
            raise ValueError(f"{path}: the face element must be one list property with a uchar count and int or uint indices "
                             f"(got {fprops})")
    if fmt == "binary_little_endian":
        vt = np.dtype([(p[1], '<' + _PLY_TYPES[p[0]]) for p in vprops])
        if len(data) < end + V * vt.itemsize:
            raise ValueError(f"{path}: the file ends inside the vertex data")
        vrec = np.frombuffer(data, dtype=vt, count=V, offset=end)
        cols = {n: vrec[n] for n in names}
        off = end + V * vt.itemsize
        counts = flat = np.zeros(0, np.int64)
        if F:
            it = '<' + _PLY_TYPES[fprops[0][2]]
            if off >= len(data):
                raise ValueError(f"{path}: the file ends inside the face data")
            n0 = data[off]
            ft = np.dtype([('n', 'u1'), ('i', it, (n0,))])
            frec = np.frombuffer(data, dtype=ft, count=F, offset=off) if len(data) >= off + F * ft.itemsize else None
            if frec is not None and (frec['n'] == n0).all():            # one polygon size throughout: no loop
                counts, flat = np.full(F, n0, np.int64), frec['i'].reshape(-1)
            else:
                counts, chunks = np.empty(F, np.int64), []
                for f in range(F):
                    if off >= len(data):
                        raise ValueError(f"{path}: the file ends inside the face data")
                    n = data[off]
                    counts[f] = n
                    chunks.append(np.frombuffer(data, dtype=it, count=n, offset=off + 1))
                    off += 1 + 4 * n
                flat = np.concatenate(chunks)
    else:
        tokens = data[end:].split()
        nv = len(vprops)
        if len(tokens) < V * nv:
            raise ValueError(f"{path}: the file ends inside the vertex data")
        table = np.array(tokens[:V * nv], dtype=np.float64).reshape(V, nv)
        cols = {n: table[:, k] for k, n in enumerate(names)}
        counts, chunks, pos = np.empty(F, np.int64), [], V * nv
        for f in range(F):
            if pos >= len(tokens):
                raise ValueError(f"{path}: the file ends inside the face data")
            n = int(tokens[pos])
            counts[f] = n
            chunks.append(np.array(tokens[pos + 1:pos + 1 + n], dtype=np.int64))
            pos += 1 + n
        flat = np.concatenate(chunks) if chunks else np.zeros(0, np.int64)
    vertices = np.stack([np.asarray(cols[a], np.float64) for a in "xyz"], 1)
    faces = _split_polygons(counts, flat) if F else np.zeros((0, 3), np.int32)
    if F and (faces.min() < 0 or faces.max() >= V):
        raise ValueError(f"{path}: a face refers to a vertex outside [0, {V})")
    colors = None
    if all(c in names for c in ("red", "green", "blue")):
        colors = np.stack([np.asarray(cols[c]).astype(np.uint8) for c in ("red", "green", "blue")], 1)
    return vertices, faces, colors


def _as_mesh(mesh, device):
    """(vertices float64 [V,3], faces int64 [F,3]) tensors on `device` of a path or a (vertices, faces[, ...]) pair"""
    if isinstance(mesh, (str, bytes)) or hasattr(mesh, '__fspath__'):
        mesh = load_mesh(mesh)
    v, f = mesh[0], mesh[1]
    v = torch.as_tensor(_np(v) if not torch.is_tensor(v) else v).to(device=device, dtype=torch.float64)
    f = torch.as_tensor(_np(f) if not torch.is_tensor(f) else f).to(device=device, dtype=torch.int64)
    return v, f


def sample_surface(vertices, faces, n, seed=0, device=None):
    """(points float64 [n,3], face index int64 [n]): n points spread uniformly by area over a triangle mesh (the reference's
    trimesh.sample.sample_surface): a face per draw by a search of the cumulative face areas, uniform barycentric coordinates
    with the reflection u + v > 1 -> (1 - u, 1 - v).  Float64 torch on `device` (default: where the vertices are), seeded."""
    if device is None:
        device = vertices.device if torch.is_tensor(vertices) else 'cpu'
    v, f = _as_mesh((vertices, faces), device)
    if f.shape[0] == 0:
        raise ValueError("sample_surface needs at least one face")
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    cum = torch.cumsum(0.5 * torch.linalg.norm(torch.linalg.cross(b - a, c - a), dim=1), 0)
    g = torch.Generator(device=v.device).manual_seed(int(seed))
    r = torch.rand(int(n), 3, generator=g, dtype=torch.float64, device=v.device)
    pick = torch.searchsorted(cum, r[:, 0] * cum[-1], right=True).clamp_(max=f.shape[0] - 1)
    u, w = r[:, 1], r[:, 2]
    flip = u + w > 1.0
    u, w = torch.where(flip, 1.0 - u, u), torch.where(flip, 1.0 - w, w)
    p = a[pick] + u[:, None] * (b[pick] - a[pick]) + w[:, None] * (c[pick] - a[pick])
    return p, pick


# ---- alignment --------------------------------------------------------------------------------------------------------------
def kabsch(mu_s, mu_d, cov):
    """4x4 float64 numpy: the rotation and translation that move the source onto the destination in the least-squares sense,
    from the centroids and cov = sum (s - mu_s)(d - mu_d)^T, with the reflection guard (host, 3x3 SVD)."""
    U, _, Vt = np.linalg.svd(cov)
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(Vt.T @ U.T)) or 1.0])
    R = Vt.T @ D @ U.T
    T = np.eye(4)
    T[:3, :3] = R
    T[:3, 3] = mu_d - R @ mu_s
    return T


def align_icp(src_points, dst_points, threshold=0.1, max_iter=30, tol=1e-6):
    """(4x4 float64 numpy matrix, iterations, fitness, inlier RMSE): point-to-point ICP of src onto dst from the identity, as
    the reference's Open3D registration_icp call: correspondences are the nearest destination point of every source point
    when it is closer than `threshold`; fitness = correspondences / source points, RMSE over the correspondences; the
    iteration stops when both change by less than `tol`, or after max_iter updates.  HIP tensors: the search is
    functional.nearest (the grid over dst is built once), centroids and the covariance are float64 sums on the device, the
    3x3 SVD runs on the host.  Numpy arrays or CPU tensors: the same with cKDTree."""
    on_hip = _on_hip(src_points, dst_points)
    if on_hip:
        from . import functional as EF
        src, dst = src_points.detach().double().contiguous().clone(), dst_points.detach().double().contiguous()
        index = EF.NearestIndex(dst)
    else:
        src, dst = torch.from_numpy(_np(src_points).astype(np.float64)), torch.from_numpy(_np(dst_points).astype(np.float64))
        tree = KDTree(dst.numpy())

    def correspondences(p):
        if on_hip:
            d, i = index.query(p, max_dist=threshold)
            ok = i >= 0
            i = i.long()
        else:
            d, i = tree.query(p.numpy())
            d, i = torch.from_numpy(d), torch.from_numpy(i)
            ok = d < threshold
        n = int(ok.sum())
        d_ok = torch.where(ok, d, torch.zeros_like(d))
        rmse = float(torch.sqrt((d_ok * d_ok).sum() / n)) if n else 0.0
        return ok, i, n / max(len(p), 1), rmse

    T = np.eye(4)
    ok, idx, fitness, rmse = correspondences(src)
    it = 0
    while it < max_iter and bool(ok.any()):
        s, d = src[ok], dst[idx[ok]]
        mu_s, mu_d = s.mean(0), d.mean(0)
        # nine plain sums: a [3,N] x [N,3] float64 product through the BLAS took 22 ms at 1 M points, the sums take well under 1
        cov = ((s - mu_s)[:, :, None] * (d - mu_d)[:, None, :]).sum(0)
        step = kabsch(mu_s.cpu().numpy(), mu_d.cpu().numpy(), cov.cpu().numpy())
        T = step @ T
        st = torch.from_numpy(step).to(src.device)
        src = src @ st[:3, :3].T + st[:3, 3]
        it += 1
        ok, idx, f2, r2 = correspondences(src)
        converged = abs(f2 - fitness) < tol and abs(r2 - rmse) < tol
        fitness, rmse = f2, r2
        if converged:
            break
    return T, it, fitness, rmse


def _transform(v, T):
    T = torch.as_tensor(T, dtype=torch.float64, device=v.device)
    return v @ T[:3, :3].T + T[:3, 3]


def calc_3d_metric(rec_mesh, gt_mesh, align=True, n=200000, seed=0, device='cuda:0', return_points=False):
    """dict with 'accuracy' (cm), 'completion' (cm), 'completion_ratio' (%, at 5 cm) and 'transform' (4x4): the reference's
    calc_3d_metric.  Meshes are PLY paths or (vertices, faces) pairs.  As in the reference the ICP alignment runs on the
    mesh VERTICES (reconstruction onto ground truth) and the metrics on n surface samples of each mesh (seeds `seed` and
    `seed + 1`).  On a CPU device the searches go through cKDTree."""
    dev = torch.device(device)
    rv, rf = _as_mesh(rec_mesh, dev)
    gv, gf = _as_mesh(gt_mesh, dev)
    T, info = np.eye(4), None
    if align:
        T, it, fitness, rmse = align_icp(rv, gv)
        info = dict(iterations=it, fitness=fitness, rmse=rmse)
        rv = _transform(rv, T)
    rec = sample_surface(rv, rf, n, seed=seed)[0]
    gt = sample_surface(gv, gf, n, seed=seed + 1)[0]
    if dev.type != 'cuda':
        rec, gt = rec.numpy(), gt.numpy()
    out = {'accuracy': accuracy(gt, rec) * 100, 'completion': completion(gt, rec) * 100,
           'completion_ratio': completion_ratio(gt, rec) * 100, 'transform': T, 'icp': info}
    if return_points:
        out['rec_points'], out['gt_points'] = rec, gt
    return out


# ---- views ------------------------------------------------------------------------------------------------------------------
EVAL_CAM = dict(H=500, W=500, fx=300.0, fy=300.0, cx=249.5, cy=249.5)      # the reference's calc_2d_metric camera


def view_matrices(forward, up, position):
    """float64 [B,4,4] camera-to-world matrices in this project's axes (the camera looks down -z, y up in the image) of B
    cameras at `position` [B,3] whose optical axes point along `forward` [B,3]: the frame the reference's viewmatrix builds
    (optical axis, right = up x axis, down = axis x right, all of unit length) with its y and z columns negated, as its
    check_proj negates them before projecting."""
    unit = lambda a: a / np.linalg.norm(a, axis=-1, keepdims=True)          # noqa: E731
    axis = unit(np.asarray(forward, np.float64))
    right = unit(np.cross(np.asarray(up, np.float64), axis))
    down = unit(np.cross(axis, right))
    c2w = np.tile(np.eye(4), (len(axis), 1, 1))
    c2w[:, :3, 0], c2w[:, :3, 1], c2w[:, :3, 2], c2w[:, :3, 3] = right, -down, -axis, position
    return c2w


def view_box(vertices):
    """(extents [3], transform [4,4]) of the box the reference draws its camera origins from, built on the AXIS-ALIGNED
    bounding box of the ground-truth vertices (the reference fits an oriented box, which is not rebuilt here) with the
    reference's factors: the extents shrink to (0.3, 0.7, 0.7) and the box is lifted by 0.4 along z."""
    v = _np(vertices).astype(np.float64)
    lo, hi = v.min(0), v.max(0)
    transform = np.eye(4)
    transform[:3, 3] = 0.5 * (lo + hi)
    transform[2, 3] += 0.4
    return (hi - lo) * np.array([0.3, 0.7, 0.7]), transform


def _seen_counts(points32, w2c, cam, z_eps=1e-5):
    """int64 numpy [K]: points (float32 [P,3] tensor) inside each camera's frustum, the test of the reference's check_proj
    and cull_mesh.py.  functional.visibility's mask is  z < 0 and 0 < u < W and 0 < v < H;  the reference's is  0 <= -z  with
    the same image test.  They differ only at z == 0, where u and v are +-inf or NaN and both masks are false: the masks are
    identical.  CPU tensors take a torch loop of the same float32 statements."""
    if points32.is_cuda:
        from . import functional as EF
        _, counts = EF.visibility(points32, w2c, cam, edge_seen=0, z_eps=z_eps, want_classes=False, want_counts=True)
        return counts.cpu().numpy().astype(np.int64)
    return np.array([int(_seen_mask_host(points32, w, cam, z_eps).sum()) for w in w2c], np.int64)


def _seen_mask_host(points32, w2c, cam, z_eps=1e-5):
    w = torch.as_tensor(np.asarray(w2c)[:3], dtype=torch.float32)
    c = points32 @ w[:, :3].T + w[:, 3]
    c0, c1, c2 = -c[:, 0], c[:, 1], c[:, 2]
    z = c2 + np.float32(z_eps)
    u = (np.float32(cam['fx']) * c0 + np.float32(cam['cx']) * c2) / z
    v = (np.float32(cam['fy']) * c1 + np.float32(cam['cy']) * c2) / z
    return (z < 0) & (u > 0) & (u < cam['W']) & (v > 0) & (v < cam['H'])


def sample_views(extents, transform, n, unseen_points, cam=None, seed=0, device='cuda:0', batch=64, max_batches=10000):
    """(c2w float64 numpy [n,4,4], stats): n random views that see none of `unseen_points`, the reference's rejection
    sampling: a uniform origin in the box `extents` (centred, then moved by `transform`), a target drawn uniformly in
    +-10000 per axis and rounded to 0.01, up = (0, 0, -1), the reference's viewmatrix.  Candidates are drawn `batch` at a
    time from np.random.default_rng(seed); one visibility call per batch counts the unseen points each candidate sees, and
    the first n candidates with count 0 are kept, in order.  The matrices returned are in this project's axes (the camera
    looks down -z: the reference's matrix with its y and z columns negated, as its check_proj does before projecting).
    stats: candidates drawn up to the last one kept, and how many of them were rejected."""
    from . import functional as EF
    cam = cam or EVAL_CAM
    rng = np.random.default_rng(seed)
    pts = torch.as_tensor(_np(unseen_points), dtype=torch.float64).to(device).float().reshape(-1, 3)
    extents, transform = np.asarray(extents, np.float64), np.asarray(transform, np.float64)
    kept, tried = [], 0
    for _ in range(max_batches):
        if len(kept) >= n:
            break
        origin = (rng.random((batch, 3)) - 0.5) * extents @ transform[:3, :3].T + transform[:3, 3]
        target = np.round(rng.uniform(-10000.0, 10000.0, (batch, 3)), 2)
        c2w = view_matrices(target - origin, (0.0, 0.0, -1.0), origin)
        counts = _seen_counts(pts, EF.world_to_camera(list(c2w)), cam) if len(pts) else np.zeros(batch, np.int64)
        for b in range(batch):
            if len(kept) < n:
                tried += 1
                if counts[b] == 0:
                    kept.append(c2w[b])
    if len(kept) < n:
        raise RuntimeError(f"sample_views: only {len(kept)} of {n} views see none of the unseen points after "
                           f"{max_batches * batch} candidates")
    return np.stack(kept) if n else np.zeros((0, 4, 4)), dict(candidates=tried, rejected=tried - len(kept))


def calc_2d_metric(rec_mesh, gt_mesh, unseen_points, extents, transform, align=True, n_imgs=1000, seed=0, cam=None,
                   device='cuda:0', batch=8, z_near=0.0, z_far=20.0):
    """dict with 'depth_l1' (cm): the reference's calc_2d_metric -- the mean over n_imgs random views (sample_views) of the
    mean absolute difference of the depth images of the two meshes (functional.mesh_depth, `batch` views per call; a pixel
    without a hit holds 0 in either image, as in the reference's depth buffer).  Also 'transform', 'c2w' (the views) and the
    statistics of the view sampling.  Needs a HIP device."""
    dev = torch.device(device)
    if dev.type != 'cuda':
        raise NotImplementedError("calc_2d_metric needs a HIP device")
    from . import functional as EF
    cam = cam or EVAL_CAM
    rv, rf = _as_mesh(rec_mesh, dev)
    gv, gf = _as_mesh(gt_mesh, dev)
    T = np.eye(4)
    if align:
        T = align_icp(rv, gv)[0]
        rv = _transform(rv, T)
    c2w, stats = sample_views(extents, transform, n_imgs, unseen_points, cam=cam, seed=seed, device=dev)
    w2c = EF.world_to_camera(list(c2w))
    rf, gf = rf.int(), gf.int()
    errors = []
    for lo in range(0, n_imgs, batch):
        w = w2c[lo:lo + batch]
        d_gt = EF.mesh_depth(gv, gf, w, cam, z_near=z_near, z_far=z_far)
        d_rec = EF.mesh_depth(rv, rf, w, cam, z_near=z_near, z_far=z_far)
        errors.append((d_gt - d_rec).abs().double().mean(dim=(1, 2)))
    l1 = float(torch.cat(errors).mean()) * 100 if errors else float('nan')
    return {'depth_l1': l1, 'transform': T, 'c2w': c2w, **stats}


def cull_mesh(vertices, faces, c2w_list, cam, device=None):
    """faces int32 numpy [F',3]: the faces that survive the reference's cull_mesh.py -- a face goes when all of its vertices
    are outside every camera's frustum (the projection test of `_seen_counts`: float32, z_eps = 1e-5, no edge).  The
    vertices stay as they are, as in the reference.  c2w_list holds camera-to-world matrices in this project's axes (the
    camera looks down -z; tools/cull_mesh.py negates the y and z columns of a trajectory file's matrices as the reference's
    loader does).  HIP device: one functional.visibility call; CPU: a torch loop over the cameras."""
    from . import functional as EF
    if device is None:
        device = vertices.device if torch.is_tensor(vertices) else 'cpu'
    v = torch.as_tensor(_np(vertices) if not torch.is_tensor(vertices) else vertices).to(device).float()
    f = _np(faces).astype(np.int32).reshape(-1, 3)
    w2c = EF.world_to_camera(list(c2w_list))
    if v.is_cuda:
        classes, _ = EF.visibility(v.contiguous(), w2c, cam, edge_seen=0, z_eps=1e-5)
        seen = (classes == 1).cpu().numpy()
    else:
        seen = np.zeros(len(v), bool)
        for w in w2c:
            seen |= _seen_mask_host(v, w, cam).numpy()
    return f[seen[f].any(axis=1)] if len(f) else f
