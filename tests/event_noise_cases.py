"""Cases of the noisy event sensor (csrc/event_noise.hip, event_sim.EventNoise), shared by tests/test_event_noise_cpu.py and
tests/test_hip_event_noise.py; the yardstick is tests/event_noise_numpy.py.

Sensor cases: the image cases of tests/event_sim_cases.py at C = 0.02 (1 x 1, 1 x 300, 37 x 53; K 1 and 5; grey, RGB and the
`_maps` cases) and its analytic cases (45 x 61; K 1 and 4), with `stamps(i)` of tests/event_stream_cases.py (0.05 s
intervals), crossed with the noise settings

    off         all parameters zero
    refr_short  rho = 2e-3 s
    refr_long   rho = 0.03 s: longer than a sub-step (0.01 s at K = 5) and reaching into the next interval
    shot        r = 8 Hz: q = 0.08 at K = 5, 0.4 at K = 1
    leak        lambda = 31 Hz: 1.55 thresholds per interval
    all         rho = 2e-3 s, lambda = 31 Hz, r = 8 Hz, seed 0x9E3779B97F4A7C15 (both key words non-zero)

Two settings were moved from the first proposal, the conditions staying as they were:
    refr_short  rho = 1e-3 s suppressed 6.8 % (37x53_rgb_K1) and 7.0 % (37x53_rgb_K5) of the candidates, below the 10 % asked
                for; at 2e-3 s the smallest share over the image cases is 14.9 % (37x53_rgb_K1), the largest 92.9 % (1 x 1)
    leak        lambda = 30 Hz is exactly 1.5 thresholds per 0.05 s interval: the third of the pixels that does not change
                reaches d / C = 3 (up to rounding) after two intervals, an event boundary that an ulp decides -- 12 % of
                the pixels of a 37 x 53 case.  At 31 Hz no multiple of a sub-step's leak within a case is that close to an
                integer.

Conditions, asserted and printed by tests/test_event_noise_cpu.py::test_case_conditions on every image case (the analytic
cases fire one to three events per pixel and interval; their figures are printed):
    refr_*     suppresses at least 10 % of the candidates
    refr_long  suppresses at least one candidate through a t_last carried from the previous interval
    shot       has at least one pixel where a noise event falls between two signal events of the same sub-step
    leak       makes the planted no-change pixel (flat index 1; images with more than one pixel) emit positive events

Where the device's own log / sin decides the levels (RGB images without host levels, the analytic room) a pixel is LEFT OUT
of the comparison, for the rest of its case, once one of these holds in the yardstick's run:
    * analytic cases: the margin rule of tests/event_sim_cases.py fires (MARGIN) -- the margin of d / C taken along the noisy
      sensor's own L_ref, which the leak moves, and the geometric margin.  RGB images keep their existing rule instead: at
      most LOG_PATH_MAX_DIFF_SHARE of the pixels may differ in count;
    * some candidate has |(t - t_last) - rho| <= 2 tol, tol the larger `time_tolerance` (tests/event_stream_cases.py, the
      derived bound) of the candidate and of the event that set t_last: within that the device's decision may differ.  This
      holds for rho = 0 as well: the filter then asks that times do not descend, and they can -- under leak an up event may
      fire while the level moves away from the crossing (L_s < L_prev), where f_k descends with k and the later candidate is
      suppressed -- so a near-tie is as undecided there as a near-rho gap is elsewhere;
    * a noise candidate lies within 2 tol of a signal candidate of its sub-step: the merge order may differ.
A time that no level enters is computed by the same operations on the same numbers on both sides and is the same float64:
its tolerance is zero, and a decision between two such times cannot differ.  A noise candidate's time comes from integers
alone: it is one.  IMAGE_DEN_ZERO: on the image
route a level is a function of the pixel's own bytes, so L_s - L_prev = 0 in the yardstick means equal bytes and the same
zero in every implementation; the quotient is then infinite or not a number on both sides, f is 0 or 1 exactly, and such a
candidate (the leak's events on an unchanged pixel) is such a time too, not uncertain by the whole sub-step that
`time_tolerance` gives a vanishing denominator.  On the analytic route the bound stays as derived.  FIRM_LIMIT: `time_tolerance` bounds the
change of f by df = min(1, 4 MARGIN C / |L_s - L_prev|); a candidate whose f before the limit lies below -df or above 1 + df is
limited to the same 0 or 1 on both sides, so its time is such a time as well (the leak's crossings that lie
behind the level the sub-step starts from, and the exact ties at sub-step and frame boundaries they produce).
At most MAX_LEFT_OUT = 0.1 % of a case's pixels may be left out; the CPU test asserts that for every case and setting (none
is, at these settings and seeds)."""
import numpy as np

from tests import event_noise_numpy as YN
from tests import event_sim_cases as C
from tests import event_sim_numpy as Y
from tests import event_stream_cases as SC
from tests import event_stream_numpy as YS
from tests.viz_cases import CAM

ALL_SEED = 0x9E3779B97F4A7C15
SETTINGS = {
    "off": dict(refractory=0.0, leak_rate=0.0, shot_rate=0.0, seed=0),
    "refr_short": dict(refractory=2e-3, leak_rate=0.0, shot_rate=0.0, seed=0),
    "refr_long": dict(refractory=0.03, leak_rate=0.0, shot_rate=0.0, seed=0),
    "shot": dict(refractory=0.0, leak_rate=0.0, shot_rate=8.0, seed=7),
    "leak": dict(refractory=0.0, leak_rate=31.0, shot_rate=0.0, seed=0),
    "all": dict(refractory=2e-3, leak_rate=31.0, shot_rate=8.0, seed=ALL_SEED),
}
NO_CHANGE_PIXEL = 1                 # flat index of the planted pixel whose grey value never changes

IMAGE_NAMES = sorted(n for n in C.image_cases() if not n.endswith('_exact'))
ANALYTIC_NAMES = sorted(C.ANALYTIC)

stamps = SC.stamps

_cache = {}


def _finish(step, stamps_i, left, geo_margin=None):
    """adds `stamps`, and `left_out`, the cumulative mask of the rules above, to one yardstick step"""
    step['stamps'] = stamps_i
    H, W = step['margin'].shape
    out = np.zeros((H, W), dtype=bool)
    if geo_margin is not None:
        out = (step['margin'] < C.MARGIN) | (geo_margin < C.MARGIN)
    cand = step['candidates']
    if cand.shape[0]:
        K, (t_a, t_b) = step['K'], stamps_i
        den, den_last = cand[:, 7].copy(), cand[:, 9].copy()
        if geo_margin is None:                                  # image route: see IMAGE_DEN_ZERO above
            den[den == 0.0], den_last[den_last == 0.0] = np.inf, np.inf
        for d, c, raw in ((den, cand[:, 8], cand[:, 11]), (den_last, cand[:, 10], cand[:, 12])):    # FIRM_LIMIT above
            with np.errstate(divide='ignore', invalid='ignore'):
                df = np.minimum(1.0, 4.0 * C.MARGIN * c / np.abs(d))
                d[(raw < -df) | (raw > 1.0 + df)] = np.inf
        # a time that no level enters (den = inf) is the same float64 on both sides: the same operations on the same numbers
        tol = np.maximum(np.where(np.isinf(den), 0.0, SC.time_tolerance(den, cand[:, 8], K, t_a, t_b)),
                         np.where(np.isinf(den_last), 0.0, SC.time_tolerance(den_last, cand[:, 10], K, t_a, t_b)))
        with np.errstate(invalid='ignore'):
            close = (tol > 0.0) & (np.abs((cand[:, 2] - cand[:, 6]) - step['rho']) <= 2.0 * tol)
        # neighbours in merged order, one of them noise and one signal, same pixel and sub-step
        same = (cand[1:, 0] == cand[:-1, 0]) & (cand[1:, 1] == cand[:-1, 1]) & (cand[1:, 4] != cand[:-1, 4])
        own = np.where(np.isinf(den), 0.0, SC.time_tolerance(den, cand[:, 8], K, t_a, t_b))
        pair = np.maximum(own[1:], own[:-1])
        near = same & (pair > 0.0) & (np.abs(cand[1:, 2] - cand[:-1, 2]) <= 2.0 * pair)
        flagged = np.concatenate([cand[close, 0], cand[1:][near, 0]]).astype(np.int64)
        out.reshape(-1)[flagged] = True
        step['flagged'] = (int(close.sum()), int(near.sum()))
    step['left_out'] = left | out
    return step['left_out']


def image_noise_reference(name, setting, c_pos=None, c_neg=None):
    """The yardstick's run of one image case under one noise setting, once per process (read-only): per interval the dict of
    YN.step_levels plus `stamps`, `rho` and `left_out`.  c_pos / c_neg: the per-pixel maps of the simulator under test for the
    *_maps cases (an input of both sides)."""
    key = ('image', name, setting)
    if key not in _cache:
        c, n = C.image_cases()[name], SETTINGS[setting]
        cp = c['c_pos'] if c_pos is None else np.asarray(c_pos)
        cn = c['c_neg'] if c_neg is None else np.asarray(c_neg)
        sensor = YN.NoisySensor(Y.level_of_image(c['images'][0], C.EPS), cp, cn, **n)
        steps, left = [], np.zeros(c['shape'], dtype=bool)
        for i, (prev, cur) in enumerate(zip(c['images'][:-1], c['images'][1:])):
            step = YN.step_levels(sensor, YS.image_levels(prev, cur, c['K'], C.EPS), *stamps(i))
            step['rho'] = n['refractory']
            left = _finish(step, stamps(i), left)
            steps.append(step)
        _cache[key] = steps
    return _cache[key]


def analytic_noise_reference(name, setting):
    """The yardstick's run of one analytic case under one noise setting, once per process (read-only): per interval the dict
    of YN.step_levels plus `stamps`, `rho`, `poses` (float64 [K+1,4,4], the previous frame's first) and `left_out`."""
    key = ('analytic', name, setting)
    if key not in _cache:
        c, n, base, room, frames = C.ANALYTIC[name], SETTINGS[setting], C.analytic_reference(name), Y.Room(C.demo_room()), C.analytic_poses(name)
        sensor = YN.NoisySensor(base['first'], c['c'], c['c'], **n)
        steps, left = [], np.zeros((CAM['H'], CAM['W']), dtype=bool)
        for i, sub in enumerate(base['sub_poses']):
            poses = np.concatenate([np.asarray(frames[i], dtype=np.float64)[None], sub], axis=0)
            step = YN.step_levels(sensor, YS.scene_levels(room, poses, CAM, C.EPS), *stamps(i))
            step['rho'], step['poses'] = n['refractory'], poses
            left = _finish(step, stamps(i), left, base['steps'][i]['geo_margin'])
            steps.append(step)
        _cache[key] = steps
    return _cache[key]


def conditions(steps):
    """the figures the conditions above are about, over all intervals of one reference run"""
    cand = np.concatenate([s['candidates'] for s in steps], axis=0)
    suppressed = cand[:, 5] == 0
    carried = 0
    between = set()
    for s in steps:
        c = s['candidates']
        if not c.shape[0]:
            continue
        carried += int(((c[:, 5] == 0) & (c[:, 6] < s['stamps'][0])).sum())          # suppressed by an event of an earlier interval
        # a noise candidate with a signal candidate of the same pixel and sub-step on either side
        mid = (c[1:-1, 4] == 1) & (c[:-2, 4] == 0) & (c[2:, 4] == 0)
        for col in (0, 1):
            mid = mid & (c[1:-1, col] == c[:-2, col]) & (c[1:-1, col] == c[2:, col])
        between |= set(c[1:-1][mid, 0].astype(np.int64).tolist())
    quiet = sum(int(s['events'].reshape(-1, 2)[NO_CHANGE_PIXEL, 1]) for s in steps) if steps[0]['events'].shape[0] * steps[0]['events'].shape[1] > 1 else 0
    return dict(candidates=int(cand.shape[0]), suppressed=int(suppressed.sum()),
                suppressed_share=float(suppressed.mean()) if cand.shape[0] else 0.0, carried=carried,
                noise_between_signal=len(between), quiet_pixel_positive=quiet,
                left_out=int(steps[-1]['left_out'].sum()))
