"""float64 numpy yardstick of the scene rasteriser (csrc/scene_raster.hip, functional.scene_raster / vertex_normals): the
triangle test of mesh_depth.hip with culling, the point squares, the (float32 depth, id) lexicographic minimum, Open3D's
vertex normals summed in ascending face order and the resolve arithmetic, one pixel grid at a time and with no pixel boxes.
Beside the images it reports its own margins: how close a deciding quantity came to the value at which the answer changes."""
import numpy as np

NONE = np.uint64(0xFFFFFFFFFFFFFFFF)
POINT = 0x80000000


def cross(a, b):
    """a x b over the last axis, each component one product minus one product (the kernel's order)"""
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1],
                     a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def to_camera(m, p):
    """[..., 3]: ((m_r0 x + m_r1 y) + m_r2 z) + m_r3 for the rows r of the 3 x 4 matrix m"""
    x, y, z = p[..., 0], p[..., 1], p[..., 2]
    return np.stack([((m[r, 0] * x + m[r, 1] * y) + m[r, 2] * z) + m[r, 3] for r in range(3)], -1)


def vertex_normals(vertices, faces):
    """float64 [V,3]: the face normals (b - a) x (c - a) added to their three vertices face by face in ascending order, then
    divided by the length; zero stays zero; a face with an index outside the vertices is dropped"""
    v, f = np.asarray(vertices, np.float64), np.asarray(faces)
    n = np.zeros_like(v)
    for a, b, c in f:
        if min(a, b, c) < 0 or max(a, b, c) >= len(v):
            continue
        fn = cross(v[b] - v[a], v[c] - v[a])
        for i in (a, b, c):
            n[i] = n[i] + fn
    ln = np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2])
    ok = ln > 0
    n[ok] = n[ok] / ln[ok, None]
    return n


def point_squares(points, m, cam, point_size, z_near, z_far):
    """(ok bool [P], z [P], first column [P], first row [P], margin): ok marks the points with z_near < z <= z_far; margin is
    the smallest distance of u - point_size / 2 or w - point_size / 2 from an integer over those points"""
    c = to_camera(m, np.asarray(points, np.float64).reshape(-1, 3))
    z = -c[:, 2]
    ok = (z > z_near) & (z <= z_far)
    with np.errstate(divide='ignore', invalid='ignore'):
        u = (cam['cx'] + cam['fx'] * (c[:, 0] / z)) - 0.5 * point_size
        w = (cam['cy'] - cam['fy'] * (c[:, 1] / z)) - 0.5 * point_size
    both = np.concatenate([u[ok], w[ok]])
    margin = float(np.abs(both - np.rint(both)).min()) if both.size else np.inf
    return ok, z, np.ceil(u), np.ceil(w), margin


def raster(vertices, faces, w2c, cam, colors=None, normals=None, points=None, point_colors=None, point_size=4, cull=1,
           z_near=0.0, z_far=1000.0, ambient=0.35, background=(255, 255, 255)):
    """One view (w2c: the 3 x 4 or 4 x 4 world-to-camera matrix).  A dict with rgb uint8 [H,W,3], depth float32 [H,W], id int32
    [H,W] (face index, -2 - p for point p, -1 for nothing) and the margins
      edge    the smallest |s_i / S| over the pixels of every kept triangle with t > 0
      gap     the smallest (t' - t) / t between the winner and the nearest candidate with another depth
      round   the smallest distance of 255 c shade from a half-integer over the face pixels
      point   point_squares' margin"""
    v, f = np.asarray(vertices, np.float64).reshape(-1, 3), np.asarray(faces).reshape(-1, 3)
    m = np.asarray(w2c, np.float64)[:3]
    H, W = cam['H'], cam['W']
    jj, ii = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing='ij')
    dx, dy = (ii - cam['cx']) / cam['fx'], -(jj - cam['cy']) / cam['fy']
    keys, depths, edge = [], [], np.inf

    def edge_fns(p):
        n0, n1, n2 = cross(p[1], p[2]), cross(p[2], p[0]), cross(p[0], p[1])
        return [(dx * n[0] + dy * n[1]) - n[2] for n in (n0, n1, n2)], (p[0, 0] * n0[0] + p[0, 1] * n0[1]) + p[0, 2] * n0[2]

    for fi, (a, b, c) in enumerate(f):
        if min(a, b, c) < 0 or max(a, b, c) >= len(v):
            continue
        if not cross(v[b] - v[a], v[c] - v[a]).any():                       # a repeated vertex
            continue
        (s0, s1, s2), det = edge_fns(to_camera(m, v[[a, b, c]]))
        if det == 0.0 or not np.isfinite(det) or (cull == 1 and not det > 0) or (cull == 2 and not det < 0):
            continue
        S = (s0 + s1) + s2
        with np.errstate(divide='ignore', invalid='ignore'):
            t = det / S
            front = (S != 0.0) & (t > 0)
            bary = np.minimum(np.minimum(np.abs(s0 / S), np.abs(s1 / S)), np.abs(s2 / S))
        if front.any():
            edge = min(edge, float(bary[front].min()))
        inside = ((s0 >= 0) & (s1 >= 0) & (s2 >= 0)) | ((s0 <= 0) & (s1 <= 0) & (s2 <= 0))
        hit = inside & (S != 0.0) & (t > z_near) & (t <= z_far)
        if not hit.any():
            continue
        bits = np.where(hit, t, 0.0).astype(np.float32).view(np.uint32).astype(np.uint64)
        keys.append(np.where(hit, (bits << np.uint64(32)) | np.uint64(fi), NONE))
        depths.append(np.where(hit, t, np.inf))
    pmargin = np.inf
    if points is not None and len(points):
        ok, z, a0, b0, pmargin = point_squares(points, m, cam, point_size, z_near, z_far)
        for pi in np.nonzero(ok)[0]:
            sq = (ii >= a0[pi]) & (ii < a0[pi] + point_size) & (jj >= b0[pi]) & (jj < b0[pi] + point_size)
            if not sq.any():
                continue
            bits = np.uint64(np.float32(z[pi]).view(np.uint32))
            keys.append(np.where(sq, (bits << np.uint64(32)) | np.uint64(POINT | int(pi)), NONE))
            depths.append(np.where(sq, z[pi], np.inf))
    rgb = np.empty((H, W, 3), np.uint8)
    rgb[:] = np.asarray(background, np.uint8)
    out = dict(rgb=rgb, depth=np.zeros((H, W), np.float32), id=np.full((H, W), -1, np.int32), edge=edge, gap=np.inf,
               round=np.inf, point=pmargin)
    if not keys:
        return out
    key = np.min(np.stack(keys), axis=0)
    got = key != NONE
    prim = (key & np.uint64(0xFFFFFFFF)).astype(np.int64)
    out['depth'] = np.where(got, (key >> np.uint64(32)).astype(np.uint32).view(np.float32), np.float32(0))
    is_pt = got & (prim >= POINT)
    out['id'] = np.where(got, np.where(is_pt, -2 - (prim - POINT), prim), -1).astype(np.int32)
    # the winner's float64 depth and the nearest other depth
    d = np.sort(np.stack(depths), axis=0)
    first = d[0]
    with np.errstate(invalid='ignore'):
        other = np.where(d > first[None], d, np.inf).min(axis=0)
        gap = (other - first) / first
    if got.any() and np.isfinite(gap[got]).any():
        out['gap'] = float(gap[got][np.isfinite(gap[got])].min())
    if is_pt.any():
        rgb[is_pt] = np.asarray(point_colors, np.uint8)[prim[is_pt] - POINT]
    nrm = None if normals is None else np.asarray(normals, np.float64)
    col = None if colors is None else np.asarray(colors, np.uint8).astype(np.float64) / 255.0
    for fi in np.unique(prim[got & ~is_pt]):
        px = got & ~is_pt & (prim == fi)
        a, b, c = f[fi]
        (s0, s1, s2), _ = edge_fns(to_camera(m, v[[a, b, c]]))
        S = (s0 + s1) + s2
        b0, b1, b2 = (s0 / S)[px], (s1 / S)[px], (s2 / S)[px]
        n = np.zeros((len(b0), 3))
        if nrm is not None:
            n = (b0[:, None] * nrm[a] + b1[:, None] * nrm[b]) + b2[:, None] * nrm[c]
        zero = ~n.any(axis=1)
        n[zero] = cross(v[b] - v[a], v[c] - v[a])
        dw = np.stack([(m[0, r] * dx[px] + m[1, r] * dy[px]) - m[2, r] for r in range(3)], -1)
        dot = (n[:, 0] * dw[:, 0] + n[:, 1] * dw[:, 1]) + n[:, 2] * dw[:, 2]
        ln = np.sqrt((n * n).sum(1)) * np.sqrt((dw * dw).sum(1))
        shade = ambient + (1.0 - ambient) * np.where(ln > 0, np.abs(dot) / np.where(ln > 0, ln, 1.0), 0.0)
        cc = np.full((len(b0), 3), 0.7) if col is None else (b0[:, None] * col[a] + b1[:, None] * col[b]) + b2[:, None] * col[c]
        x = (255.0 * cc) * shade[:, None]
        out['round'] = min(out['round'], float(np.abs((x - np.floor(x)) - 0.5).min()))
        rgb[px] = np.clip(np.floor(x + 0.5), 0, 255).astype(np.uint8)
    return out
