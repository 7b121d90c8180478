"""Seeded cases of the depth forecast (enslam_depth_forecast) and the conditions each has to meet, asserted here on the
yardstick (tests/depth_forecast_numpy.py) when the module is imported.

Shapes are the smallest at which csrc/depth_forecast.hip can still go wrong: one thread per source pixel and one per target
pixel in workgroups of 256, so 1 x 1, 1 x 300 (a second, partly filled workgroup on both sides), a hand-worked 5 x 7, and
45 x 61 = 2745 source pixels (eleven workgroups, the last partly filled) onto 7 x 9 (non-integer spacings 7.33 and 7.5) and
onto itself.  Every case is run with fill = 0 and fill = 1.

THE EXPECTATION is bit equality: the kernel, the numpy route and the yardstick perform the same IEEE float64 operations in the
same order, and float64 +, -, *, /, floor and the conversion to float32 are correctly rounded everywhere."""
import math

import numpy as np

from tests import depth_forecast_numpy as Y

CAM_1 = dict(fx=1.0, fy=1.0, cx=0.0, cy=0.0)
CAM_ROW = dict(fx=120.0, fy=120.0, cx=149.5, cy=0.0)
CAM_57 = dict(fx=4.0, fy=4.0, cx=3.0, cy=2.0)
CAM_4561 = dict(fx=50.0, fy=50.0, cx=30.0, cy=22.0)


def identity():
    return np.eye(4)[:3].copy()


def translation(tx, ty, tz):
    """The TARGET camera sits at (tx, ty, tz) in source-camera coordinates, same orientation: q = p - t."""
    m = identity()
    m[:, 3] = (-tx, -ty, -tz)
    return m


def rotation_y(angle, t=(0.0, 0.0, 0.0)):
    """The target camera is the source camera turned by `angle` about its y axis (up), then moved to t: q = R^T (p - t)."""
    c, s = math.cos(angle), math.sin(angle)
    R = np.array([[c, 0.0, s], [0.0, 1.0, 0.0], [-s, 0.0, c]])
    m = np.zeros((3, 4))
    m[:, :3] = R.T
    m[:, 3] = -R.T @ np.asarray(t, dtype=np.float64)
    return m


def poison(depth, rng):
    """Zeros, a NaN, an infinity and a negative value at seeded places; returns the places."""
    H, W = depth.shape
    flat = rng.choice(H * W, size=min(6, H * W), replace=False)
    vals = [0.0, 0.0, float('nan'), float('inf'), -1.5, float('-inf')][:len(flat)]
    for f, v in zip(flat, vals):
        depth[f // W, f % W] = v
    return [(int(f // W), int(f % W)) for f in flat]


def bands(H, W, lo, hi, near, far):
    """Fronto-parallel far surface with a near band over the columns lo..hi-1."""
    d = np.full((H, W), far, dtype=np.float32)
    d[:, lo:hi] = near
    return d


def rough(H, W, seed, base=2.0, amp=0.5):
    rng = np.random.default_rng(seed)
    return (base + amp * rng.random((H, W))).astype(np.float32), rng


def _cases():
    out = []

    def add(name, depth, cam, M, size, radius, z_near=0.0):
        out.append(dict(name=name, depth=np.ascontiguousarray(depth, dtype=np.float32), cam=cam, M=np.ascontiguousarray(M),
                        size=size, radius=float(radius), z_near=float(z_near)))

    add('1x1', np.array([[1.25]], dtype=np.float32), CAM_1, translation(0.0, 0.0, -0.5), (1, 1), 0.5)
    d, rng = rough(1, 300, 1)
    d[0, [3, 77, 200, 299]] = [0.0, np.nan, np.inf, -2.0]
    add('1x300_identity', d, CAM_ROW, identity(), (1, 300), 0.5)
    add('1x300_shift', d, CAM_ROW, translation(0.05, 0.0, -0.1), (1, 300), 0.5)
    # hand-worked: a plane at depth 2, the camera moves 1 towards it: every point doubles its distance from the principal
    # point (3, 2) -- u = 2 i - 3, v = 2 j - 2 -- and lands at depth 1 (tests/test_depth_forecast_cpu.py works it out)
    add('5x7_plane', np.full((5, 7), 2.0, dtype=np.float32), CAM_57, translation(0.0, 0.0, -1.0), (5, 7), 0.25)
    add('5x7_to_3x4', np.full((5, 7), 2.0, dtype=np.float32), CAM_57, translation(0.0, 0.0, -1.0), (3, 4), 1.0)
    d, rng = rough(5, 7, 2)
    poison(d, rng)
    add('5x7_to_1x4', d, CAM_57, translation(0.01, 0.02, 0.0), (1, 4), 0.75)
    d, rng = rough(45, 61, 3)
    poison(d, rng)
    add('45x61_identity', d, CAM_4561, identity(), (45, 61), 0.5)
    add('45x61_identity_7x9', d, CAM_4561, identity(), (7, 9), 1.5)
    add('45x61_plane_towards', np.full((45, 61), 3.0, dtype=np.float32), CAM_4561, translation(0.0, 0.0, -0.7), (45, 61), 0.5)
    d, rng = rough(45, 61, 4)
    poison(d, rng)
    add('45x61_rotation', d, CAM_4561, rotation_y(0.35, (0.02, -0.01, 0.03)), (45, 61), 0.5)
    add('45x61_rotation_7x9', d, CAM_4561, rotation_y(-0.35, (0.02, -0.01, 0.03)), (7, 9), 2.0)
    # the camera moves forward past the near band: it ends behind z_near
    d = bands(45, 61, 20, 40, 1.0, 3.0)
    poison(d, np.random.default_rng(5))
    add('45x61_behind', d, CAM_4561, translation(0.0, 0.0, -1.2), (45, 61), 0.5, z_near=0.05)
    # the camera moves right by 0.1: the near band (depth 1) moves 5 pixels to the left, the far surface (depth 3) 1.67 -- the
    # band covers far points on its left (two surfaces vote for one pixel) and uncovers three columns on its right
    d = bands(45, 61, 20, 40, 1.0, 3.0)
    add('45x61_occlusion', d, CAM_4561, translation(0.1, 0.0, 0.0), (45, 61), 0.5)
    d = bands(45, 61, 20, 40, 1.0, 3.0) + (0.05 * np.random.default_rng(6).random((45, 61))).astype(np.float32)
    poison(d, np.random.default_rng(7))
    add('45x61_occlusion_7x9', d, CAM_4561, translation(0.1, 0.02, -0.05), (7, 9), 3.75)
    return out


CASES = _cases()
BY_NAME = {c['name']: c for c in CASES}
FILLS = (0, 1)

_EXPECTED = {}


def expected(case, fill):
    """The yardstick's image of a case, computed once and shared (read-only)."""
    key = (case['name'], int(fill))
    if key not in _EXPECTED:
        img = Y.forecast(case['depth'], case['cam'], case['M'], case['size'][0], case['size'][1], case['radius'], case['z_near'],
                         int(fill))
        img.setflags(write=False)
        _EXPECTED[key] = img
    return _EXPECTED[key]


def case_votes(case):
    return Y.votes(case['depth'], case['cam'], case['M'], case['size'][0], case['size'][1], case['radius'], case['z_near'])


def _check_conditions():
    shapes = {(c['depth'].shape, c['size']) for c in CASES}
    for need in (((1, 1), (1, 1)), ((1, 300), (1, 300)), ((5, 7), (5, 7)), ((5, 7), (3, 4)), ((45, 61), (7, 9)),
                 ((45, 61), (45, 61))):
        assert need in shapes, need
    assert any(c['size'][0] == 1 and c['size'][1] > 1 and c['depth'].shape[0] > 1 for c in CASES)
    everything = np.concatenate([c['depth'].reshape(-1) for c in CASES])
    assert (everything == 0).any() and np.isnan(everything).any() and np.isposinf(everything).any() and (everything < 0).any()
    # identity keeps every valid pixel where it is
    c = BY_NAME['45x61_identity']
    valid = np.isfinite(c['depth']) & (c['depth'] > 0)
    assert valid.sum() == len(case_votes(c)) and not valid.all()
    # the rotation moves part of the image out of view: valid points without a vote, and target columns without any
    c = BY_NAME['45x61_rotation']
    v = case_votes(c)
    assert 0 < sum(len(z) for z in v.values()) < 0.9 * 45 * 61
    cols = {io for (_jo, io) in v}
    assert cols and len(cols) < 61
    # part of the scene ends behind z_near: the near band (20 columns of 61) casts no vote, the far surface does
    c = BY_NAME['45x61_behind']
    v = case_votes(c)
    n = sum(len(z) for z in v.values())
    assert 0 < n <= 41 * 45 and all(float(z) > 1.0 for zs in v.values() for z in zs)
    # occlusion: at least one target pixel receives votes from both surfaces, and the nearer one wins
    for name in ('45x61_occlusion', '45x61_occlusion_7x9'):
        c = BY_NAME[name]
        both = [(t, zs) for t, zs in case_votes(c).items() if min(zs) < 1.5 and max(zs) > 2.5]
        assert both, name
        img = expected(c, 0)
        assert all(img[t] == min(zs) for t, zs in both)
    # disocclusion: empty pixels of which some are filled and some stay 0
    c = BY_NAME['45x61_occlusion']
    a, b = expected(c, 0), expected(c, 1)
    assert ((a == 0) & (b > 0)).any() and ((a == 0) & (b == 0)).any()
    assert (b[(a == 0) & (b > 0)] > 2.5).any()               # a filled hole beside the background shows the background
    # one block is passed on both sides
    assert BY_NAME['1x300_identity']['depth'].size > 256 and 45 * 61 > 10 * 256 and 45 * 61 % 256 != 0


_check_conditions()
