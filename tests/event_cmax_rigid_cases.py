"""Seeded cases of the rigid-motion model of event motion compensation (enslam_event_cmax_rigid_eval), the conditions each has to
meet, and the planted stream of its recovery test.  THE TOLERANCE RULE is tests/event_cmax_cases.py's, unchanged: everything up
to J and all FOUR counters have the bound 0; mu, f and the six gradient components use bounds() of that file on the case's own
yardstick (tests/event_cmax_rigid_numpy.py).  bounds() and quant_bounds() are generic in the number of parameters.

Shapes are the smallest at which the kernels can still go wrong: 1 x 1 under a blur wider than the image; 45 x 61 (2745 pixels:
ten full blocks and one of 185) with N = 0, 1, 255, 256, 257, 700 in shuffled, time and pixel order; 8 x 9 with N = 65537 (257
partials x 6 interleaved columns, two second-level blocks, two values left to add); 20000 events on one pixel of 5 x 7 (the
integer atomics under full contention); a hand-worked 5 x 7 case whose calibration, depths, times and velocities are binary
fractions, so that every x', y' is exact; and a planted 9 x 12 case with one event per rule.

The random cases draw the depth in [0.5, 4] with 5 % invalid pixels (0.0, -1.0, NaN, +inf in turn), theta within +-1 rad / s
and +-1 unit / s, t in [0, 0.1] around t_ref = 0.05.  Their seeds were chosen on the yardstick so that, for N >= 255, some
events drop for depth, some for the warp, and more than 80 % vote (on 8 x 9 that takes a slow motion: at +-1 most of so small an
image would leave it)."""
import numpy as np

from tests import event_cmax_cases as CC
from tests import event_cmax_rigid_numpy as YR

MODEL = 'rigid'
P = 6


def _case(name, H, W, N, seed, signed=False, k=9, order='shuffled', kind='random'):
    return dict(name=name, H=H, W=W, N=N, model=MODEL, seed=seed, signed=signed, k=k, order=order, kind=kind)


CASES = [
    _case('1x1_k3_wider', 1, 1, 5, 1, k=3, signed=True),
    _case('hand_5x7', 5, 7, 6, 0, k=1, kind='hand'),
    _case('45x61_N0', 45, 61, 0, 2),
    _case('45x61_N1', 45, 61, 1, 3, signed=True, k=3),
    _case('45x61_N255', 45, 61, 255, 4, order='pixel'),
    _case('45x61_N256', 45, 61, 256, 5, order='time', k=1),
    _case('45x61_N257', 45, 61, 257, 6, signed=True, k=3, order='time'),
    _case('45x61_N700_pixel', 45, 61, 700, 7, signed=True, order='pixel'),
    _case('45x61_N700', 45, 61, 700, 8),
    _case('8x9_N65537', 8, 9, 65537, 83, k=3),
    _case('5x7_one_pixel', 5, 7, 20000, 47, k=3, kind='one_pixel'),
    _case('planted_9x12', 9, 12, 12, 11, k=3, kind='planted'),
]
# the planted events of 'planted_9x12' by index: fx = fy = 2, theta = (0, 0, 0, 2, -1, 0), t_ref = 0, so that x' = x + 4 t rho and
# y' = y - 2 t rho exactly
PLANTED = dict(lattice=0, last_column=1, depth_zero=2, depth_negative=3, depth_nan=4, depth_inf=5, depth_subnormal=6, depth_tiny=7,
               x_past_W=8, y_at_H=9, nan_t=10, nan_t_on_bad_depth=11)
SUBNORMAL = np.float32(1e-42)
TINY = np.float32(2.0 ** -10)
HAND_THETA = [0.5, -0.25, 0.5, 1.0, -0.5, 2.0]


def calib(case):
    H, W = case['H'], case['W']
    if case['kind'] in ('hand', 'planted'):
        return (2.0, 2.0, 3.0, 2.0)
    if H == 1 and W == 1:
        return (80.0, 80.0, 0.0, 0.0)
    return (80.0, 80.0, (W - 1) / 2.0, (H - 1) / 2.0)


def depth_image(case):
    """float32 [H, W] from the case's seed alone"""
    H, W = case['H'], case['W']
    if case['kind'] == 'hand':
        d = np.full((H, W), 2.0, dtype=np.float32)
        d[0, 4], d[4, 2], d[1, 0], d[3, 5] = 1.0, 4.0, 0.5, 1.0
        return d
    if case['kind'] == 'planted':
        d = np.ones((H, W), dtype=np.float32)
        d[1, 1], d[1, 2], d[1, 3], d[1, 4], d[1, 5], d[1, 6] = 0.0, -1.0, np.nan, np.inf, SUBNORMAL, TINY
        return d
    rng = np.random.default_rng(2000 + case['seed'])
    d = rng.uniform(0.5, 4.0, (H, W)).astype(np.float32)
    bad = np.nonzero(rng.random((H, W)).reshape(-1) < 0.05)[0]
    d.reshape(-1)[bad] = np.array([0.0, -1.0, np.nan, np.inf], dtype=np.float32)[np.arange(bad.size) % 4]
    if case['kind'] == 'one_pixel':
        d[2, 3] = 1.5
    if H == 1 and W == 1:
        d[0, 0] = 2.0
    return d


def stream(case):
    """(t float64, x uint16, y uint16, p uint8) from the case's seed alone"""
    H, W = case['H'], case['W']
    if case['kind'] == 'hand':
        # on the lattice at the principal point; the same pixel an eighth of a second later; a near pixel (z = 1) in the top
        # row; a far one (z = 4) in the last row; the left band (z = 1 / 2); before t_ref (z = 1)
        t = [0.0, 0.125, 0.125, 0.25, 0.125, -0.0625]
        x = [3, 3, 4, 2, 0, 5]
        y = [2, 2, 0, 4, 1, 3]
        p = [1, 1, 0, 1, 1, 0]
    elif case['kind'] == 'planted':
        nan = float('nan')
        t = [0.5, 0.5, 0.25, 0.25, 0.25, 0.25, 0.5, 0.5, 0.0, 0.0, nan, nan]
        x = [5, 9, 1, 2, 3, 4, 5, 6, 65535, 2, 3, 1]
        y = [3, 4, 1, 1, 1, 1, 1, 1, H - 1, H, 3, 1]
        p = [1, 0, 1, 0, 1, 0, 1, 0, 1, 0, 1, 0]
    else:
        return CC.stream(case)
    return (np.asarray(t, dtype=np.float64), np.asarray(x).astype(np.uint16), np.asarray(y).astype(np.uint16), np.asarray(p).astype(np.uint8))


def motion(case):
    """(theta, t_ref) of the case"""
    if case['kind'] == 'hand':
        return list(HAND_THETA), 0.0
    if case['kind'] == 'planted':
        return [0.0, 0.0, 0.0, 2.0, -1.0, 0.0], 0.0
    if case['H'] == 1 and case['W'] == 1:
        return [0.02, -0.03, 0.5, 0.01, -0.02, 0.3], 0.05
    return np.random.default_rng(1000 + case['seed']).uniform(-1.0, 1.0, P).tolist(), 0.05


def arguments(case):
    """the keyword arguments the yardstick takes beside the stream; the routes take model='rigid' on top"""
    theta, t_ref = motion(case)
    return dict(H=case['H'], W=case['W'], calib=calib(case), theta=theta, t_ref=t_ref, taps=CC.taps_of(case['k']), signed=case['signed'],
                depth=depth_image(case))


_REF = {}


def reference(case, variant=None):
    """the yardstick of the case, computed once and shared (never written to)"""
    key = (case['name'], variant)
    if key not in _REF:
        _REF[key] = YR.cmax(*stream(case), variant=variant, **arguments(case))
    return _REF[key]


def check_conditions(case, ref):
    """what the case was built to exercise, asserted on the yardstick"""
    t, x, y, p = stream(case)
    H, W, N = case['H'], case['W'], case['N']
    d = depth_image(case)
    assert d.dtype == np.float32 and d.shape == (H, W)
    assert len(t) == N and int(ref['dropped'].sum()) + int(ref['voted'].sum()) == N and ref['dropped'].shape == (4,)
    theta, _ = motion(case)
    assert len(theta) == P and (case['kind'] in ('hand', 'planted') or all(abs(v) <= 1.0 for v in theta))
    if case['order'] == 'time':
        assert np.all(np.diff(t) >= 0)
    if case['order'] == 'pixel':
        pix = y.astype(np.int64) * W + x
        assert np.all(np.diff(pix) >= 0) and N > 1 and np.any(np.diff(t) < 0)
    if case['order'] == 'shuffled' and case['kind'] == 'random' and N > 100:
        assert np.any(np.diff(t) < 0) and np.any(np.diff(y.astype(np.int64) * W + x) < 0)
    if case['k'] // 2 >= min(H, W):
        assert case['name'].endswith('wider')
    if case['kind'] == 'random' and H > 1:
        ok = np.isfinite(d) & (d > 0)
        assert 0.5 <= d[ok].min() and d[ok].max() <= 4.0 and 0 < (~ok).sum() <= 0.1 * H * W
    if case['kind'] == 'one_pixel':
        assert len(set(zip(x.tolist(), y.tolist()))) == 1 and int(ref['voted'].sum()) > 19000
        assert int(np.abs(ref['iwe']).max()) > 2000 * YR.TWO32          # well past what 32 bits could hold
    if case['kind'] == 'random' and N >= 255 and H > 1:
        assert ref['dropped'][3] > 0 and ref['dropped'][2] > 0 and ref['voted'].sum() > 0.8 * N
        band = ref['voted'] & ((ref['xw'] < 0) | (ref['yw'] < 0) | (ref['xw'] > W - 1) | (ref['yw'] > H - 1))
        assert band.any()                                                 # votes with corners outside
    if case['name'] == '8x9_N65537':
        assert -(-N // 256) == 257 and -(-257 // 256) == 2               # two second-level blocks, two values left to add
    if case['kind'] == 'planted':
        i = PLANTED
        xw, yw, v = ref['xw'], ref['yw'], ref['voted']
        assert (xw[i['lattice']], yw[i['lattice']]) == (7.0, 2.0) and v[i['lattice']] and ref['iwe'][2, 7] == YR.TWO32
        assert (xw[i['last_column']], yw[i['last_column']]) == (W - 1.0, 3.0) and v[i['last_column']] and ref['iwe'][3, W - 1] == YR.TWO32
        for name in ('depth_zero', 'depth_negative', 'depth_nan', 'depth_inf'):
            assert not v[i[name]] and np.isnan(xw[i[name]])               # dropped before the warp
        assert 0 < float(SUBNORMAL) < float(np.finfo(np.float32).tiny)
        assert not v[i['depth_subnormal']] and not (abs(xw[i['depth_subnormal']]) < 1e30)      # non-finite or absurdly far
        assert not v[i['depth_tiny']] and xw[i['depth_tiny']] == 6.0 + 2048.0
        # read before the sensor check, the depth of this event would be looked up far outside the image
        assert int(y[i['x_past_W']]) * W + int(x[i['x_past_W']]) >= H * W and int(y[i['x_past_W']]) < H
        assert not v[i['x_past_W']] and not v[i['y_at_H']] and not v[i['nan_t']] and not v[i['nan_t_on_bad_depth']]
        assert ref['dropped'].tolist() == [2, 2, 2, 4] and int(v.sum()) == 2


# ---- the planted stream of the recovery test ----------------------------------------------------------------------------------
REC_TRUTH = [0.3, -0.5, 0.8, 0.5, -0.3, 0.4]
REC_SEEDS = (0, 1, 2)
# |theta_hat - theta_true| / |theta_true| per component from theta0 = truth (1 +- 0.2), as the CPU route of estimate_motion gave
# it with the reference time in the middle of the window (a record, not a bar: with six parameters and a warp of a few pixels
# the components trade against each other -- seed 1 misses w_x and v_y by as much as their size -- while the warp as a whole,
# which the test bars, moves nearer the truth's: 0.27 / 0.53 / 0.32 pixels off against 0.63 / 0.66 / 0.64 for theta0)
REC_RECORD = {0: (0.0012, 0.026, 0.035, 0.22, 0.0061, 0.23), 1: (0.91, 0.26, 0.19, 0.61, 1.9, 0.023),
              2: (0.37, 0.079, 0.23, 0.063, 0.83, 0.04)}       # 48 - 59 evaluations each (23 - 40 accepted steps)


def rec_depth():
    """the slanted plane z = 2.5 + 3 u + 1.2 v the planted points lie on, as the camera sees it at the start of the window:
    depths between 1 and 4"""
    fx, fy, cx, cy = CC.REC_CALIB
    u = (np.arange(CC.REC_W, dtype=np.float64)[None, :] - cx) / fx
    v = (np.arange(CC.REC_H, dtype=np.float64)[:, None] - cy) / fy
    return (2.5 + 3.0 * u + 1.2 * v).astype(np.float32)


def planted_stream(seed):
    """200 seeded 3-D points on the plane of rec_depth (depths 1 - 4), seen by a camera that goes through the real poses
    c2w0 @ relative_motion(REC_TRUTH, t) for 0.1 s in 400 sub-steps; a point emits an event at the end of a sub-step in which
    its ROUNDED pixel changed, as tests/event_cmax_cases.py's planted_stream does.  Returns (t, x, y, p)."""
    from evennicer_slam_amd.event_cmax import relative_motion
    rng = np.random.default_rng(seed)
    fx, fy, cx, cy = CC.REC_CALIB
    n = CC.REC_POINTS
    px, py = rng.uniform(0, CC.REC_W - 1, n), rng.uniform(0, CC.REC_H - 1, n)
    pol = rng.integers(0, 2, n)
    u, v = (px - cx) / fx, (py - cy) / fy
    z = 2.5 + 3.0 * u + 1.2 * v
    assert z.min() > 1.0 and z.max() < 4.0
    c2w0 = relative_motion([0.2, -0.1, 0.3, 1.0, 2.0, -0.5], 1.0).numpy()              # any pose
    cam = np.stack([u * z, -v * z, -z, np.ones(n)])                                     # the project's camera looks down -z, y up
    world = c2w0 @ cam
    h = CC.REC_WINDOW / CC.REC_SUBSTEPS
    ts, xs, ys, ps = [], [], [], []
    last = (np.rint(px).astype(np.int64), np.rint(py).astype(np.int64))
    for s in range(1, CC.REC_SUBSTEPS + 1):
        c = np.linalg.inv(c2w0 @ relative_motion(REC_TRUTH, s * h).numpy()) @ world
        qx, qy = cx + fx * (c[0] / -c[2]), cy + fy * (-c[1] / -c[2])
        now = (np.rint(qx).astype(np.int64), np.rint(qy).astype(np.int64))
        moved = ((now[0] != last[0]) | (now[1] != last[1])) & (now[0] >= 0) & (now[0] < CC.REC_W) & (now[1] >= 0) & (now[1] < CC.REC_H)
        for j in np.nonzero(moved)[0]:
            ts.append(s * h)
            xs.append(now[0][j])
            ys.append(now[1][j])
            ps.append(pol[j])
        last = now
    return (np.array(ts, dtype=np.float64), np.array(xs).astype(np.uint16), np.array(ys).astype(np.uint16), np.array(ps).astype(np.uint8))


def rec_theta0(seed):
    """the truth with each component perturbed by a seeded +-20 %"""
    sign = np.random.default_rng(500 + seed).integers(0, 2, P) * 2 - 1
    return [float(a * (1.0 + 0.2 * s)) for a, s in zip(REC_TRUTH, sign)]


def field(theta, dt):
    """[H, W, 2]: the pixels the model moves each pixel of rec_depth over dt, first order: (fx du dt, fy dv dt)"""
    fx, fy, cx, cy = CC.REC_CALIB
    rho = 1.0 / rec_depth().astype(np.float64)
    u = (np.arange(CC.REC_W, dtype=np.float64)[None, :] - cx) / fx + 0 * rho
    v = (np.arange(CC.REC_H, dtype=np.float64)[:, None] - cy) / fy + 0 * rho
    wx, wy, wz, vx, vy, vz = theta
    du = u * v * wx - (1 + u * u) * wy + v * wz + rho * (u * vz - vx)
    dv = (1 + v * v) * wx - u * v * wy - u * wz + rho * (v * vz - vy)
    return np.stack([fx * du * dt, fy * dv * dt], axis=-1)


def component_errors(theta):
    return [abs(a - b) / abs(b) for a, b in zip(theta, REC_TRUTH)]
