"""Seeded cases of event motion compensation (enslam_event_cmax_eval), the conditions each has to meet, the tolerance rule, and
the planted streams of the recovery tests.

Shapes are the smallest at which csrc/event_cmax.hip can still go wrong: one thread per event and per pixel in workgroups of
256 (N = 0, 1, 255, 256, 257; 45 x 61 = 2745 pixels = 10 full blocks and one of 185), a second tree level above 256 partials and
the ascending rest above 65536 elements (N = 65537: 257 partials, two second-level blocks), one pixel taking every vote (20000
events: the integer atomics under full contention), a 1 x 1 and a 1 x 300 sensor with a blur wider than the image, and planted
events on the lattice, on the last column, in (-1, 0) and far outside.

THE TOLERANCE RULE.  u = 2^-53.  The yardstick (tests/event_cmax_numpy.py) performs the header's operations in the header's
order, so everything up to J -- the votes, the counters, the blur -- has the bound 0: equal integers, equal bits.  The two
differ only where the header says SUM: the route adds in the stated tree, the yardstick with math.fsum (correctly rounded).
  SUM    a value of the tree passes through 8 + 8 halving levels and at most L = ceil(n / 65536) ascending adds, each one
         rounding: |tree - exact| <= DEPTH(n) u sum|v|, DEPTH(n) = 16 + max(L, 1), to first order in u (a factor 1.01 covers the
         rest), and the yardstick's own rounding of the exact sum adds u |sum|.
  mu     SUM(J) / (H W): E_mu = (DEPTH + 2) u sum|J| / (H W)                                    (the division is one more u)
  C      J - mu with the route's own mu: E_C = E_mu + u max|C|
  f      SUM(C C) / (H W): the squares differ by 2 |C| E_C + E_C^2 + u C^2, the sum by DEPTH u sum C^2:
         E_f = (2 E_C sum|C| + H W E_C^2 + (DEPTH + 3) u sum C^2) / (H W)
  D      G C: the taps are positive and sum to at most 1, so an input error passes through at most unchanged, and the 2 k
         multiply-adds of the two passes each round a partial sum of at most max|C|: E_D = E_C + 4 k u max|C|
  Gx     at most four products D_c dw_c with sum_c |dw_c| = 2, four adds: E_G = 2 E_D + 16 u max|D|
  g_k    s (Gx (mx Bu_k) + Gy (my Bv_k)): E_g = E_G (|mx Bu_k| + |my Bv_k|) + 4 u (|Gx mx Bu_k| + |Gy my Bv_k|), per event
  grad   (2 / (H W)) SUM(g_k): E_grad_k = (2 / (H W)) (sum_e E_g + (DEPTH(N) + 3) u sum_e |g_k|)
Every bound is a multiple of u times an absolute sum, evaluated on the yardstick of the case; none is fitted to a device.

The unquantised statement (cmax_torch) against the quantised one: a vote differs from its weight by at most 2^-33 (half a unit
of the fixed point), so a pixel of I, and of J (taps sum to at most 1), by at most V 2^-33 with V the number of votes (<= 4 N):
E_q = 4 N 2^-33 bounds the error of I, J, mu, C and D alike (C by twice that).  QUANT_* below follow the same chain as above."""
import math

import numpy as np

from tests import event_cmax_numpy as Y

U = 2.0 ** -53
SLACK = 1.01
SIGMA = 1.5


def taps_of(k):
    from evennicer_slam_amd.event_cmax import blur_taps
    return blur_taps(SIGMA, k)


def _case(name, H, W, N, model, seed, signed=False, k=9, order='shuffled', kind='random'):
    return dict(name=name, H=H, W=W, N=N, model=model, seed=seed, signed=signed, k=k, order=order, kind=kind)


CASES = [
    _case('1x1_k1', 1, 1, 5, 'flow', 1, k=1),
    _case('1x1_k3_wider', 1, 1, 5, 'rotation', 2, k=3, signed=True),
    _case('1x300_k9_wider', 1, 300, 257, 'rotation', 3, k=9, order='time'),
    _case('hand_5x7', 5, 7, 6, 'flow', 0, k=1, kind='hand'),
    _case('45x61_N0', 45, 61, 0, 'rotation', 4),
    _case('45x61_N1', 45, 61, 1, 'flow', 5, signed=True, k=3),
    _case('45x61_N255', 45, 61, 255, 'rotation', 6, order='pixel'),
    _case('45x61_N256', 45, 61, 256, 'flow', 7, order='time', k=1),
    _case('45x61_N257', 45, 61, 257, 'rotation', 8, signed=True, k=3, order='time'),
    _case('45x61_flow_k9', 45, 61, 700, 'flow', 9, signed=True, order='pixel'),
    _case('45x61_rot_k9', 45, 61, 700, 'rotation', 10),
    _case('8x9_N65537', 8, 9, 65537, 'flow', 11, k=3),
    _case('5x7_one_pixel', 5, 7, 20000, 'rotation', 12, k=3, kind='one_pixel'),
    _case('planted_9x12', 9, 12, 10, 'flow', 13, k=3, kind='planted'),
]
# the planted events of 'planted_9x12' by index: x' = x - 4 t, y' = y + 2 t exactly (fx = fy = 2, theta = (4, -2), t_ref = 0)
PLANTED = dict(lattice=0, half_lattice=1, last_column=2, left_band=3, top_band=4, far=5, nan_t=6, inf_t=7, x_at_W=8, y_at_H=9)


def calib(case):
    H, W = case['H'], case['W']
    if case['kind'] in ('hand', 'planted'):
        return (2.0, 2.0, 3.0, 2.0)
    if H == 1 and W == 1:
        return (80.0, 80.0, 0.0, 0.0)
    return (80.0, 80.0, (W - 1) / 2.0, (H - 1) / 2.0)


def stream(case):
    """(t float64, x uint16, y uint16, p uint8) from the case's seed alone"""
    rng = np.random.default_rng(case['seed'])
    H, W, N = case['H'], case['W'], case['N']
    if case['kind'] == 'hand':
        # x' = x - 4 t, y' = y + 2 t: on the lattice; (3.5, 0.25); (1.5, 4.25) over the last row; (-0.5, 1.25) in the left band;
        # (5.25, 2.875) before t_ref; on the last column and row
        t = [0.0, 0.125, 0.125, 0.125, -0.0625, 0.0]
        x = [3, 4, 2, 0, 5, 6]
        y = [2, 0, 4, 1, 3, 4]
        p = [1, 1, 0, 1, 0, 1]
    elif case['kind'] == 'planted':
        t = [0.5, 0.25, -0.25, 0.125, -0.25, 100.0, float('nan'), float('inf'), 0.0, 0.0]
        x = [5, 5, W - 2, 0, 4, 6, 3, 3, W, 2]
        y = [3, 3, 4, 5, 0, 4, 3, 3, 2, H]
        p = [1, 0, 1, 1, 0, 1, 1, 0, 1, 0]
    elif case['kind'] == 'one_pixel':
        t, x, y, p = rng.uniform(0.0, 0.1, N), np.full(N, 3), np.full(N, 2), rng.integers(0, 2, N)
    else:
        t, x, y, p = rng.uniform(0.0, 0.1, N), rng.integers(0, W, N), rng.integers(0, H, N), rng.integers(0, 2, N)
    t, x, y, p = np.asarray(t, dtype=np.float64), np.asarray(x), np.asarray(y), np.asarray(p)
    if case['order'] == 'time' or case['order'] == 'pixel':
        o = np.argsort(t, kind='stable')
        t, x, y, p = t[o], x[o], y[o], p[o]
    if case['order'] == 'pixel':
        o = np.argsort(y * W + x, kind='stable')
        t, x, y, p = t[o], x[o], y[o], p[o]
    return t, x.astype(np.uint16), y.astype(np.uint16), p.astype(np.uint8)


def motion(case):
    """(theta, t_ref) of the case"""
    if case['kind'] in ('hand', 'planted'):
        return [4.0, -2.0], 0.0
    rng = np.random.default_rng(1000 + case['seed'])
    if case['H'] == 1 and case['W'] == 1:
        return ([3.0, -2.0] if case['model'] == 'flow' else [0.02, -0.03, 0.5]), 0.05
    if case['model'] == 'flow':
        return rng.uniform(-100.0, 100.0, 2).tolist(), 0.05
    return rng.uniform(-1.0, 1.0, 3).tolist(), 0.05


def arguments(case):
    """the keyword arguments every route and the yardstick take, beside the stream"""
    theta, t_ref = motion(case)
    return dict(H=case['H'], W=case['W'], calib=calib(case), model=case['model'], theta=theta, t_ref=t_ref, taps=taps_of(case['k']),
                signed=case['signed'])


_REF = {}


def reference(case, variant=None):
    """the yardstick of the case, computed once and shared (never written to)"""
    key = (case['name'], variant)
    if key not in _REF:
        _REF[key] = Y.cmax(*stream(case), variant=variant, **arguments(case))
    return _REF[key]


def check_conditions(case, ref):
    """what the case was built to exercise, asserted on the yardstick"""
    t, x, y, p = stream(case)
    H, W, N = case['H'], case['W'], case['N']
    assert len(t) == N and int(ref['dropped'].sum()) + int(ref['voted'].sum()) == N
    if case['order'] == 'time':
        assert np.all(np.diff(t) >= 0)
    if case['order'] == 'pixel':
        pix = y.astype(np.int64) * W + x
        assert np.all(np.diff(pix) >= 0) and N > 1 and np.any(np.diff(t) < 0)
    if case['order'] == 'shuffled' and case['kind'] == 'random' and N > 100:
        assert np.any(np.diff(t) < 0) and np.any(np.diff(y.astype(np.int64) * W + x) < 0)
    if case['k'] // 2 >= min(H, W):
        assert case['name'].endswith('wider')
    if case['kind'] == 'one_pixel':
        assert len(set(zip(x.tolist(), y.tolist()))) == 1 and int(ref['voted'].sum()) > 19000
        assert int(np.abs(ref['iwe']).max()) > 2000 * Y.TWO32          # well past what 32 bits could hold
    if case['kind'] == 'random' and N >= 255 and H > 1:
        assert ref['dropped'][2] > 0 and ref['voted'].sum() > 0.8 * N    # some events leave the image, most stay
        band = ref['voted'] & ((ref['xw'] < 0) | (ref['yw'] < 0) | (ref['xw'] > W - 1) | (ref['yw'] > H - 1))
        assert band.any()                                                 # votes with corners outside
    if case['name'] == '8x9_N65537':
        assert -(-N // 256) == 257 and -(-257 // 256) == 2               # two second-level blocks, two values left to add
    if case['kind'] == 'planted':
        i = PLANTED
        xw, yw, v = ref['xw'], ref['yw'], ref['voted']
        assert (xw[i['lattice']], yw[i['lattice']]) == (3.0, 4.0) and v[i['lattice']]
        assert (xw[i['half_lattice']], yw[i['half_lattice']]) == (4.0, 3.5) and v[i['half_lattice']]
        assert xw[i['last_column']] == W - 1 and v[i['last_column']]
        assert -1 < xw[i['left_band']] < 0 and v[i['left_band']]
        assert -1 < yw[i['top_band']] < 0 and v[i['top_band']]
        assert xw[i['far']] == 6 - 400.0 and not v[i['far']]
        assert not v[i['nan_t']] and not v[i['inf_t']] and not v[i['x_at_W']] and not v[i['y_at_H']]
        assert ref['dropped'].tolist() == [2, 2, 1]
        # the lattice event puts its whole unit on one pixel and nothing else there is touched by it
        assert ref['iwe'][4, 3] >= Y.TWO32


def depth(n):
    return 16 + max(-(-n // 65536), 1)


def bounds(case, ref):
    """dict(mu, f, grad [P]): the absolute bounds of the rule above on the yardstick `ref` of `case`"""
    npix = case['H'] * case['W']
    amax = lambda a: float(np.abs(a).max()) if np.size(a) else 0.0
    dp = depth(npix)
    e_mu = SLACK * (dp + 2) * U * float(np.abs(ref['J']).sum()) / npix
    e_c = e_mu + U * amax(ref['C'])
    e_f = SLACK * (2 * e_c * float(np.abs(ref['C']).sum()) + npix * e_c ** 2 + (dp + 3) * U * float((ref['C'] ** 2).sum())) / npix
    e_d = e_c + 4 * case['k'] * U * amax(ref['C'])
    e_G = 2 * e_d + 16 * U * amax(ref['D'])
    dn = depth(max(case['N'], 1))
    e_grad = []
    for k in range(ref['g'].shape[1]):
        e_g = e_G * (ref['lev_x'][:, k] + ref['lev_y'][:, k]) + 4 * U * (np.abs(ref['Gx']) * ref['lev_x'][:, k] + np.abs(ref['Gy']) * ref['lev_y'][:, k])
        e_g = np.where(ref['voted'], e_g, 0.0)
        e_grad.append(SLACK * (2.0 / npix) * (float(e_g.sum()) + (dn + 3) * U * float(np.abs(ref['g'][:, k]).sum())))
    return dict(mu=e_mu, f=e_f, grad=np.array(e_grad))


def quant_bounds(case, ref):
    """dict(f, grad [P]): how far the unquantised statement may be from the quantised yardstick (the rule's last paragraph)"""
    npix = case['H'] * case['W']
    e_q = 4 * case['N'] * 2.0 ** -33
    e_c = 2 * e_q
    e_f = (2 * e_c * float(np.abs(ref['C']).sum()) + npix * e_c ** 2) / npix
    e_G = 2 * e_c
    e_grad = [(2.0 / npix) * float(np.where(ref['voted'], e_G * (ref['lev_x'][:, k] + ref['lev_y'][:, k]), 0.0).sum())
              for k in range(ref['g'].shape[1])]
    return dict(f=e_f, grad=np.array(e_grad))


# ---- the planted streams of the recovery tests ------------------------------------------------------------------------------
REC_H, REC_W, REC_F = 45, 61, 80.0
REC_CALIB = (REC_F, REC_F, (REC_W - 1) / 2.0, (REC_H - 1) / 2.0)
REC_TRUTH = {'flow': [80.0, -50.0], 'rotation': [0.3, -0.5, 0.8]}
REC_WINDOW, REC_SUBSTEPS, REC_POINTS, REC_K = 0.1, 400, 200, 9
REC_SEEDS = (0, 1, 2)
# |theta_hat - theta_true| / |theta_true| per component, as the CPU route of estimate_motion gave it (a record, not a bar: roll,
# the third component of 'rotation', is barely observable on 45 x 61 pixels)
REC_RECORD = {
    ('flow', 0): (0.0001, 0.048), ('flow', 1): (0.015, 0.086), ('flow', 2): (0.010, 0.0033),
    ('rotation', 0): (0.072, 0.025, 0.067), ('rotation', 1): (0.053, 0.031, 0.0041), ('rotation', 2): (0.020, 0.012, 0.078),
}       # 21 - 34 evaluations each (12 - 17 accepted steps)


def planted_stream(model, seed):
    """200 seeded points on 45 x 61 carried by the model's own flow for 0.1 s in 400 sub-steps; a point emits an event at the
    end of a sub-step in which its ROUNDED pixel changed (events at pixel crossings, not at every step: steady emission makes
    false maxima).  Returns (t, x, y, p)."""
    rng = np.random.default_rng(seed)
    fx, fy, cx, cy = REC_CALIB
    px, py = rng.uniform(0, REC_W - 1, REC_POINTS), rng.uniform(0, REC_H - 1, REC_POINTS)
    pol = rng.integers(0, 2, REC_POINTS)
    th = REC_TRUTH[model]
    h = REC_WINDOW / REC_SUBSTEPS
    ts, xs, ys, ps = [], [], [], []
    last = (np.rint(px).astype(np.int64), np.rint(py).astype(np.int64))
    for s in range(1, REC_SUBSTEPS + 1):
        if model == 'flow':
            vx, vy = np.full(REC_POINTS, th[0]), np.full(REC_POINTS, th[1])
        else:
            u, v = (px - cx) / fx, (py - cy) / fy
            vx = fx * (u * v * th[0] - (1 + u * u) * th[1] + v * th[2])
            vy = fy * ((1 + v * v) * th[0] - u * v * th[1] - u * th[2])
        px, py = px + h * vx, py + h * vy
        now = (np.rint(px).astype(np.int64), np.rint(py).astype(np.int64))
        moved = ((now[0] != last[0]) | (now[1] != last[1])) & (now[0] >= 0) & (now[0] < REC_W) & (now[1] >= 0) & (now[1] < REC_H)
        for j in np.nonzero(moved)[0]:
            ts.append(s * h)
            xs.append(now[0][j])
            ys.append(now[1][j])
            ps.append(pol[j])
        last = now
    return (np.array(ts, dtype=np.float64), np.array(xs).astype(np.uint16), np.array(ys).astype(np.uint16), np.array(ps).astype(np.uint8))


def component_errors(model, theta):
    return [abs(a - b) / abs(b) for a, b in zip(theta, REC_TRUTH[model])]


def fraction(err, ref):
    m = float(np.abs(ref).max()) if np.size(ref) else 0.0
    return float(err) / m if m > 0 else (0.0 if err == 0 else math.inf)
