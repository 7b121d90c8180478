"""float64 numpy yardstick of enslam_visibility (csrc/visibility.hip): the seen / forecast / unseen classes of
Mesher.point_masks and the per-camera counts of Mapper.keyframe_selection_overlap, plus, per point, whether any tested
quantity of any camera lies within a relative margin of its threshold (such points are excluded from exact comparisons:
a float32 comparison may fall on either side there).

Scales of the margin, per tested quantity: W for u against the seen edges, H for v, 1000 for u and v against the forecast
edges, the limit for the projected depth against it (the per-camera depth limit or the largest depth sample), 2.4 for the
projected depth against sample -/+ 2.4, and 1 for z against 0."""
import numpy as np

MARGIN = 1e-5
CAM = dict(H=48, W=64, fx=50.0, fy=50.0, cx=31.5, cy=23.5)      # the tiny camera of the fixtures


def world_to_camera(c2w):
    """float64 [K,3,4] from camera-to-world matrices [K,4,4] of any float dtype"""
    return np.stack([np.linalg.inv(np.asarray(m, np.float64))[:3] for m in c2w]) if len(c2w) else np.zeros((0, 3, 4))


def lattice_points(axes):
    """float64 [nx*ny*nz, 3] of float32 axes, x slowest and z fastest (Mesher.lattice_volume's order)"""
    ax = [np.asarray(a, np.float32).astype(np.float64) for a in axes]
    g = np.meshgrid(*ax, indexing='ij')
    return np.stack([a.reshape(-1) for a in g], 1)


def axes_from_spec(spec):
    """float32 axes from rows (lo, hi, n): np.linspace in float64 rounded to float32, as the Mesher forms its lattice"""
    return [np.linspace(float(lo), float(hi), int(n)).astype(np.float32) for lo, hi, n in spec]


def project(points, w2c, cam, z_eps):
    """u, v, z, pd (each float64 [P]) of one camera: cam = R p + t, cam.x *= -1, uvz = K cam, z = uvz.z + z_eps"""
    p = np.asarray(points, np.float64)
    c = p @ w2c[:, :3].T + w2c[:, 3]
    c0, c1, c2 = -c[:, 0], c[:, 1], c[:, 2]
    z = c2 + z_eps
    with np.errstate(divide='ignore', invalid='ignore'):
        u = (cam['fx'] * c0 + cam['cx'] * c2) / z
        v = (cam['fy'] * c1 + cam['cy'] * c2) / z
    return u, v, z, -c2


def bilinear_zero_padded(img, u, v):
    """F.grid_sample(img, (u, v) in pixels, bilinear, padding_mode='zeros', align_corners=True) in float64"""
    H, W = img.shape
    img = np.asarray(img, np.float64)
    x0, y0 = np.floor(u), np.floor(v)
    out = np.zeros_like(u)
    for dx in (0, 1):
        for dy in (0, 1):
            xi, yi = x0 + dx, y0 + dy
            wgt = (1 - np.abs(u - xi)) * (1 - np.abs(v - yi))
            ok = (xi >= 0) & (xi <= W - 1) & (yi >= 0) & (yi <= H - 1) & np.isfinite(u) & np.isfinite(v)
            xs, ys = np.where(ok, xi, 0).astype(np.int64), np.where(ok, yi, 0).astype(np.int64)
            out += np.where(ok, img[ys, xs] * wgt, 0.0)
    return out


def _close(value, threshold, scale, margin):
    with np.errstate(invalid='ignore'):
        return np.abs(value - threshold) <= margin * scale


def classify(points, w2c, cam, edge_seen=0, edge_forecast=-1000, z_eps=1e-8, limit=None, depth=None, chunk=None,
             margin=MARGIN):
    """classes uint8 [P] (0 unseen, 1 seen, 2 forecast), counts int64 [K] of the points passing each camera's seen test,
    near bool [P] (some tested quantity of some camera within the margin of its threshold) and near_k bool [K,P] (the same
    restricted to the quantities of camera k's SEEN test, which is what a count depends on).  With `depth`, the largest
    sample per camera is taken per `chunk` points, as the reference's per-chunk torch.max."""
    p = np.asarray(points, np.float64).reshape(-1, 3)
    P, K = p.shape[0], len(w2c)
    H, W = cam['H'], cam['W']
    chunk = P if not chunk else int(chunk)
    classes = np.zeros(P, np.uint8)
    counts = np.zeros(K, np.int64)
    near = np.zeros(P, bool)
    near_k = np.zeros((K, P), bool)
    for lo in range(0, P, max(chunk, 1)):
        sl = slice(lo, min(lo + chunk, P))
        seen = np.zeros(sl.stop - lo, bool)
        fore = np.zeros_like(seen)
        for k in range(K):
            u, v, z, pd = project(p[sl], w2c[k], cam, z_eps)
            with np.errstate(invalid='ignore'):
                front = z < 0
                s = front & (u < W - edge_seen) & (u > edge_seen) & (v < H - edge_seen) & (v > edge_seen)
                f = front & (u < W - edge_forecast) & (u > edge_forecast) & (v < H - edge_forecast) & (v > edge_forecast)
            ns = _close(z, 0.0, 1.0, margin) | _close(u, edge_seen, W, margin) | _close(u, W - edge_seen, W, margin) | \
                _close(v, edge_seen, H, margin) | _close(v, H - edge_seen, H, margin)
            nf = _close(u, edge_forecast, 1000.0, margin) | _close(u, W - edge_forecast, 1000.0, margin) | \
                _close(v, edge_forecast, 1000.0, margin) | _close(v, H - edge_forecast, 1000.0, margin)
            if limit is not None:
                lim = float(limit[k])
                with np.errstate(invalid='ignore'):
                    s &= pd < lim
                    f &= pd < lim
                ns |= _close(pd, lim, abs(lim), margin)
            if depth is not None:
                d = bilinear_zero_padded(depth[k], u, v)
                dmax = float(np.max(d))
                with np.errstate(invalid='ignore'):
                    s &= (pd < d + 2.4) & (d - 2.4 < pd)
                    f &= pd < dmax
                ns |= _close(pd, d + 2.4, 2.4, margin) | _close(pd, d - 2.4, 2.4, margin)
                nf |= _close(pd, dmax, abs(dmax), margin)
            seen |= s
            fore |= f
            counts[k] += int(s.sum())
            near[sl] |= ns | nf
            near_k[k, sl] = ns
        classes[sl] = np.where(seen, 1, np.where(fore, 2, 0))
    return classes, counts, near, near_k


# ---- the reference fixture (tests/golden/make_golden_visibility.py) ---------------------------------------------------------
VARIANTS = {'plain': dict(depth_test=False, all_frames=False), 'depth': dict(depth_test=True, all_frames=False),
            'all': dict(depth_test=False, all_frames=True)}


def load_fixture():
    import os
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'tiny_visibility.npz')
    return dict(np.load(path))


def fixture_classes(fx, name, variant, n):
    """uint8 [n] classes the reference's point_masks returned for point set `name` ('lattice' / 'scatter')"""
    seen = np.unpackbits(fx[f'{name}_{variant}_seen'])[:n].astype(bool)
    fore = np.unpackbits(fx[f'{name}_{variant}_forecast'])[:n].astype(bool)
    return np.where(seen, 1, np.where(fore, 2, 0)).astype(np.uint8)


def fixture_points(fx, name):
    """(float64 points [P,3], chunk) of a point set of the fixture"""
    if name == 'lattice':
        return lattice_points(axes_from_spec(fx['lattice_spec'])), int(fx['lattice_chunk'])
    return fx['scatter'].astype(np.float64), int(fx['scatter_chunk'])


def fixture_views(fx, variant):
    """(w2c, limit, depth) as Mesher.point_masks sets them up for a variant: the keyframes with 1.1 x their largest depth
    (float32 product, as torch forms it) or with their depth images, or every frame with neither"""
    w2c = world_to_camera(fx['c2w'])
    v = VARIANTS[variant]
    if v['all_frames']:
        return w2c, None, None
    if v['depth_test']:
        return w2c, None, fx['depth']
    return w2c, (fx['depth'].reshape(len(w2c), -1).max(1) * np.float32(1.1)).astype(np.float32), None
