"""Cases of the time-stamped event streams (csrc/event_stream.hip, event_stream.py), shared by tests/test_event_stream_cpu.py
and tests/test_hip_event_stream.py; the yardstick is tests/event_stream_numpy.py.

Simulator cases: the image cases and the analytic cases of tests/event_sim_cases.py, unchanged (1 x 1, 1 x 300, 37 x 53 and the
45 x 61 camera; K 1, 4 and 5; the 345-event pixel, the no-change pixel, the exact-threshold pixel, per-pixel thresholds).
Interval i of a case runs from t_a = 10 + 0.05 i to t_b = 10 + 0.05 (i + 1).

Accumulator cases: a 37 x 53 sensor, N in {0, 1, 255, 256, 257, 70 001} (one thread per event in workgroups of 256: none,
one, one short of a workgroup, a full one, one more, and some 270 workgroups) times B in {1, 2, 65}, edges 10 + 0.05 j.  Every
stream starts with planted events, as far as N reaches: exactly on edges[B] (kept, last bin), exactly on edges[0] (dropped),
exactly on an interior edge (belongs to the bin that ENDS there; B >= 2), one before and one after the range, and one with
x = W, y = 0 -- out of the sensor, but a flat index formed without the check still lies inside the buffer (it is pixel
(1, 0)), so a missing check shows as a wrong count, not as a stray store.  The rest is seeded: times uniform from 0.02 s
before the range to 0.02 s after it, 2 % of the events with x = W and y < H - 1.  The large streams also hold 300 positive
events of pixel (3, 5) inside bin 0: more than uint8 holds.  `shuffled` is a seeded permutation of each stream.
x = 65535 appears in `far_out_case` only, for the CPU tests.

Tolerance of a time stamp where the device's own log (and sin) decides the levels -- RGB images without host levels, the
analytic room.  DERIVED, not chosen:
  * Level error.  The margin rule of tests/event_sim_cases.py protects a count against a level perturbation of up to
    MARGIN * C (MARGIN = 1e-9: "generous against the ~1e-13 by which a few ulps of float64 sin / log and of the ray geometry can
    move L").  The same estimate is used here: every level, and with it R (a first level plus exact multiples of C), is off by
    at most delta = MARGIN * C.
  * Through f = (X - L_prev) / (L_s - L_prev) with |f| <= 1 at a crossing: numerator and denominator are each off by at most
    2 delta, so |df| <= (2 delta + |f| 2 delta) / |L_s - L_prev| <= 4 delta / |L_s - L_prev|.
  * The limit to [0, 1] caps |df| at 1 whatever the denominator: one sub-step's length, (t_b - t_a) / K, in time.
  * t = t_a + ((s - 1 + f) / K) (t_b - t_a) adds three roundings: 4 ulp of t_b covers them.
  tol(event) = min(1, 4 MARGIN C / |L_s - L_prev|) * (t_b - t_a) / K + 4 ulp(t_b)
with C and L_s - L_prev of that event taken from the yardstick.  tests/test_event_stream_cpu.py prints the largest value over
all device-log cases: 9.26e-9 s (an event whose sub-step moved the level by little), the median over the cases' medians
being 1.4e-11 s; the rounding term alone is 7.1e-15 s.  Pixels left out: the existing rule and its 0.1 % cap (MARGIN, MAX_LEFT_OUT) for the analytic
cases, LOG_PATH_MAX_DIFF_SHARE for the in-kernel log of RGB images; the CPU test asserts that the yardstick alone stays within
the cap."""
import numpy as np

from tests import event_sim_cases as C
from tests import event_sim_numpy as Y
from tests import event_stream_numpy as YS
from tests.viz_cases import CAM

T0, DT = 10.0, 0.05


def stamps(i):
    """(t_a, t_b) of interval i"""
    return T0 + DT * i, T0 + DT * (i + 1)


def time_tolerance(den, c, K, t_a, t_b):
    """the derived bound above, per event (arrays)"""
    with np.errstate(divide='ignore', invalid='ignore'):
        df = np.minimum(1.0, 4.0 * C.MARGIN * np.asarray(c) / np.abs(np.asarray(den)))
    df = np.where(np.isnan(df), 1.0, df)
    return df * ((t_b - t_a) / K) + 4.0 * np.spacing(t_b)


def compare_streams(ref, got, shape, keep=None):
    """A stream `got` = (t, x, y, p) (numpy, pixel-major) against the yardstick's step `ref` where bit equality is not claimed:
    pixels whose number of events differs are counted (`differ`, among the pixels of `keep` [H,W] bool), the events of all
    other kept pixels are compared one by one: same polarity (`polarity_ok`), and |t - t_ref| as a multiple of that event's
    `time_tolerance` (`worst`; `max_err` in seconds, `max_tol` the largest tolerance applied, `compared` events)."""
    H, W = shape
    t, x, y, p = got
    flat_g = y.astype(np.int64) * W + x.astype(np.int64)
    flat_r = ref['y'].astype(np.int64) * W + ref['x'].astype(np.int64)
    assert bool(np.all(np.diff(flat_g) >= 0)), "the stream is not pixel-major"
    cg, cr = np.bincount(flat_g, minlength=H * W), np.bincount(flat_r, minlength=H * W)
    kept = np.ones(H * W, dtype=bool) if keep is None else np.asarray(keep).reshape(-1)
    good = (cg == cr) & kept
    mg, mr = good[flat_g], good[flat_r]
    err = np.abs(t[mg] - ref['t'][mr])
    tol = time_tolerance(ref['den'][mr], ref['c'][mr], ref['K'], *ref['stamps'])
    return dict(differ=int(((cg != cr) & kept).sum()), max_count_diff=int(np.abs(cg - cr)[kept].max()) if kept.any() else 0,
                polarity_ok=bool(np.array_equal(p[mg], ref['p'][mr])), compared=int(err.size),
                worst=float((err / tol).max()) if err.size else 0.0, max_err=float(err.max()) if err.size else 0.0,
                max_tol=float(tol.max()) if err.size else 0.0)


_image_cache, _analytic_cache = {}, {}


def image_stream_reference(name, c_pos=None, c_neg=None):
    """The yardstick's run of one image case, once per process (read-only): per interval the dict of YS.step_levels plus
    `stamps`.  c_pos / c_neg: the per-pixel maps of the simulator under test for the *_maps cases (an input of both sides)."""
    if name not in _image_cache:
        c = C.image_cases()[name]
        cp = c['c_pos'] if c_pos is None else np.asarray(c_pos)
        cn = c['c_neg'] if c_neg is None else np.asarray(c_neg)
        sensor = Y.Sensor(Y.level_of_image(c['images'][0], C.EPS), cp, cn)
        steps = []
        for i, (prev, cur) in enumerate(zip(c['images'][:-1], c['images'][1:])):
            step = YS.step_levels(sensor, YS.image_levels(prev, cur, c['K'], C.EPS), *stamps(i))
            step['stamps'] = stamps(i)
            steps.append(step)
        _image_cache[name] = steps
    return _image_cache[name]


def analytic_stream_reference(name):
    """The yardstick's run of one analytic case, once per process (read-only): per interval the dict of YS.step_levels plus
    `stamps`, `poses` (float64 [K+1,4,4]: the previous frame's pose, then the sub-step poses of C.analytic_reference) and
    `left_out` (the cumulative margin-rule mask of C.analytic_reference)."""
    if name not in _analytic_cache:
        c, base, room, frames = C.ANALYTIC[name], C.analytic_reference(name), Y.Room(C.demo_room()), C.analytic_poses(name)
        sensor = Y.Sensor(base['first'], c['c'], c['c'])
        steps = []
        for i, sub in enumerate(base['sub_poses']):
            poses = np.concatenate([np.asarray(frames[i], dtype=np.float64)[None], sub], axis=0)
            step = YS.step_levels(sensor, YS.scene_levels(room, poses, CAM, C.EPS), *stamps(i))
            step.update(stamps=stamps(i), poses=poses, left_out=base['steps'][i]['left_out'])
            assert np.array_equal(step['events'], base['steps'][i]['events']) and np.array_equal(step['ref'], base['steps'][i]['ref'])
            steps.append(step)
        _analytic_cache[name] = steps
    return _analytic_cache[name]


# ---- accumulator -------------------------------------------------------------------------------------------------------------
ACC_H, ACC_W = 37, 53
ACC_N = (0, 1, 255, 256, 257, 70001)
ACC_B = (1, 2, 65)
SATURATING_PIXEL = (3, 5)           # (y, x)

_acc = {}


def edges_of(B):
    return np.array([T0 + DT * j for j in range(B + 1)], dtype=np.float64)


def _stream(N, B, seed):
    H, W = ACC_H, ACC_W
    e = edges_of(B)
    rng = np.random.default_rng(seed)
    t = rng.uniform(e[0] - 0.02, e[-1] + 0.02, N)
    x = rng.integers(0, W, N)
    y = rng.integers(0, H, N)
    p = rng.integers(0, 2, N)
    out = rng.random(N) < 0.02
    x[out], y[out] = W, rng.integers(0, H - 1, int(out.sum()))
    planted = [(e[-1], 7, 2, 1), (e[0], 7, 2, 0)]
    if B >= 2:
        planted.append((e[1], 8, 2, 1))
    planted += [(e[0] - 0.5, 9, 2, 1), (e[-1] + 0.5, 9, 2, 0), (0.5 * (e[0] + e[1]), W, 0, 1)]
    for k, (tt, xx, yy, pp) in enumerate(planted[:N]):
        t[k], x[k], y[k], p[k] = tt, xx, yy, pp
    if N >= 1000:
        k0 = len(planted)
        t[k0:k0 + 300] = np.linspace(e[0] + 0.001, e[1] - 0.001, 300)
        y[k0:k0 + 300], x[k0:k0 + 300], p[k0:k0 + 300] = SATURATING_PIXEL[0], SATURATING_PIXEL[1], 1
    return t.astype(np.float64), x.astype(np.uint16), y.astype(np.uint16), p.astype(np.uint8)


def accumulate_cases():
    """name -> dict(t, x, y, p, shuffled (a permutation), edges, H, W, B, N); built once, read-only"""
    if not _acc:
        seed = 500
        for N in ACC_N:
            for B in ACC_B:
                seed += 1
                t, x, y, p = _stream(N, B, seed)
                _acc[f"N{N}_B{B}"] = dict(t=t, x=x, y=y, p=p, shuffled=np.random.default_rng(seed + 1000).permutation(N),
                                          edges=edges_of(B), H=ACC_H, W=ACC_W, B=B, N=N)
    return _acc


_acc_ref = {}


def accumulate_reference(name):
    """the yardstick's (counts uint8, unsaturated int64, dropped_time, dropped_sensor) of one case, once per process"""
    if name not in _acc_ref:
        c = accumulate_cases()[name]
        _acc_ref[name] = YS.accumulate(c['t'], c['x'], c['y'], c['p'], c['edges'], c['H'], c['W'])
    return _acc_ref[name]


def far_out_case():
    """CPU only: coordinates far outside the sensor (x = 65535, y = 65535) among valid events"""
    t = np.array([10.01, 10.02, 10.03, 10.04], dtype=np.float64)
    x = np.array([1, 65535, 2, 3], dtype=np.uint16)
    y = np.array([1, 1, 65535, 3], dtype=np.uint16)
    p = np.array([1, 1, 0, 0], dtype=np.uint8)
    return dict(t=t, x=x, y=y, p=p, edges=edges_of(1), H=ACC_H, W=ACC_W)
