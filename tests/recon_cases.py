"""Meshes, cameras and point sets of the reconstruction-evaluation tests (tests/test_hip_recon.py, tests/test_recon_cpu.py)."""
import numpy as np

from evennicer_slam_amd.synthetic import BoxRoom, look_at

CAM = dict(H=48, W=64, fx=50.0, fy=50.0, cx=31.5, cy=23.5)
ROOM_ARGS = ([-2, -1.5, -1.2], [2.2, 1.7, 1.3], [0.3, -1.5, -0.6], [1.1, -0.4, 0.2])
VIEWS = (((-1, 0.5, 0.1), (1, -1, -0.3)), ((1.5, 1, 0.8), (-1, -1, -1)), ((0, 0, 0), (0.7, -1, -0.2)))


def room():
    return BoxRoom(*ROOM_ARGS)


def view_poses():
    """float64 [3,4,4] camera-to-world matrices of the three test views"""
    return np.stack([look_at(e, t).numpy() for e, t in VIEWS])


# corner k of a box: bit 0 -> x, bit 1 -> y, bit 2 -> z.  Each face as a quad whose right-hand normal points OUT of the box.
_QUADS = ((0, 4, 6, 2), (1, 3, 7, 5), (0, 1, 5, 4), (2, 6, 7, 3), (0, 2, 3, 1), (4, 5, 7, 6))


def _box(lo, hi, outward):
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    v = np.array([[hi[a] if k >> a & 1 else lo[a] for a in range(3)] for k in range(8)])
    f = []
    for a, b, c, d in _QUADS:
        f += [(a, b, c), (a, c, d)] if outward else [(a, c, b), (a, d, c)]
    return v, np.array(f, np.int32)


def box_room_mesh(r=None):
    """(vertices float64 [16,3], faces int32 [24,3]) of a BoxRoom: the room's six walls facing inward, the box's six faces
    facing outward, two triangles each"""
    r = r or room()
    rv, rf = _box(r.room_lo.numpy(), r.room_hi.numpy(), outward=False)
    bv, bf = _box(r.box_lo.numpy(), r.box_hi.numpy(), outward=True)
    return np.concatenate([rv, bv]), np.concatenate([rf, bf + 8]).astype(np.int32)


def triangle_soup(seed, n=300):
    """(vertices float64 [3n+3,3], faces int32 [n+1,3]) in camera space (the camera at the origin looks down -z): centres
    uniform in [-4,4] x [-3,3] x [-9,1.5], vertex offsets normal with a scale drawn from {0.05, 0.2, 0.6} per triangle; the
    first four triangles have scale 4.0, triangle 4 is pushed 40 m away, and one degenerate triangle (a repeated vertex)
    is appended."""
    rng = np.random.default_rng(seed)
    centre = rng.uniform([-4, -3, -9], [4, 3, 1.5], (n, 3))
    scale = rng.choice([0.05, 0.2, 0.6], n)
    scale[:4] = 4.0
    v = centre[:, None, :] + rng.normal(size=(n, 3, 3)) * scale[:, None, None]
    v[4, :, 2] -= 40.0
    a, b = rng.uniform([-1, -1, -4], [1, 1, -2], (2, 3))
    v = np.concatenate([v.reshape(-1, 3), np.stack([a, a, b])])
    return v, np.arange(3 * n + 3, dtype=np.int32).reshape(-1, 3)


def rigid(angle_deg, axis, translation):
    """float64 [4,4]: the rotation by angle_deg about `axis` (Rodrigues), then the translation"""
    k = np.asarray(axis, np.float64)
    k = k / np.linalg.norm(k)
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    a = np.radians(angle_deg)
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * (K @ K)
    T[:3, 3] = translation
    return T


ICP_TRUTH = rigid(2.0, (1, 2, 3), (0.03, -0.02, 0.025))


def icp_case(other_seed=None, n=20000):
    """(source, destination) float64 [n,3]: destination = n surface samples of the room (seed 1), source = the same samples
    (or, with other_seed, other samples of the same surface) moved by the inverse of ICP_TRUTH"""
    r = room()
    dst = r.sample_surface(n, seed=1).numpy()
    base = dst if other_seed is None else r.sample_surface(n, seed=other_seed).numpy()
    inv = np.linalg.inv(ICP_TRUTH)
    return base @ inv[:3, :3].T + inv[:3, 3], dst


VIEW_CENTRE = np.array([-0.5, 0.3, 0.1])       # inside the room, outside the box: where the 2-D metric's test views sit
VIEW_SEED = 0                                   # with this seed sample_views rejects at least one of its first candidates


def box_top_points(n=500, seed=0):
    """float64 [n,3] points on the top face of the room's box: the "unseen" set of the view-sampling tests"""
    r = room()
    lo, hi = r.box_lo.numpy(), r.box_hi.numpy()
    p = np.random.default_rng(seed).uniform(lo, hi, (n, 3))
    p[:, 2] = hi[2]
    return p


# two cameras for the culling tests: one sees the box and two walls, one looks into a corner of the ceiling
CULL_POSES = [look_at((-1, 0.5, 0.1), (1, -1, -0.3)).numpy(), look_at((1.5, 1, 0.8), (1.5, 1.6, 1.2)).numpy()]


def check_samples(v, f, pts, pick, n):
    """the properties the issue pins: on the triangle to 1e-12, per-face counts within 5 sigma of the area share"""
    a, b, c = v[f[pick, 0]], v[f[pick, 1]], v[f[pick, 2]]
    e1, e2, d = b - a, c - a, pts - a
    nrm = np.cross(e1, e2)
    assert np.abs((d * nrm).sum(1) / np.linalg.norm(nrm, axis=1)).max() <= 1e-12
    g11, g12, g22 = (e1 * e1).sum(1), (e1 * e2).sum(1), (e2 * e2).sum(1)
    r1, r2 = (d * e1).sum(1), (d * e2).sum(1)
    det = g11 * g22 - g12 * g12
    u, w = (g22 * r1 - g12 * r2) / det, (g11 * r2 - g12 * r1) / det
    assert u.min() >= -1e-12 and w.min() >= -1e-12 and (u + w).max() <= 1 + 1e-12
    area = 0.5 * np.linalg.norm(np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]]), axis=1)
    share = area / area.sum()
    counts = np.bincount(pick, minlength=len(f))
    assert (np.abs(counts - n * share) <= 5 * np.sqrt(n * share * (1 - share))).all()
