"""Seeded cases of the event-camera simulator at the launch edges of csrc/event_sim.hip (64 x 4 pixel tiles, 256 threads), not
at workload sizes.  Shared by tests/test_event_sim_cpu.py and tests/test_hip_event_sim.py; the yardstick is
tests/event_sim_numpy.py.

Image cases: 1 x 1; 1 x 300 (one row, wider than a block's 64 columns: five column tiles, the last one partial); 37 x 53 (a
multiple of neither the wave nor the tile, ten row tiles).  K in {1, 5}, grey and RGB, four images = three consecutive
intervals with the state carried, scalar thresholds and per-pixel ones (sigma_c = 0.6 around 0.02: a good part of the
draws hits the 0.01 floor).  Every sequence plants, from flat pixel 0 on (as far as the image has pixels):
    0  black -> white -> black -> white   at C = 0.02 the change of 6.9088 is 345 thresholds: saturation, both polarities
    1  no change at all
    2  grey 100 -> 105 -> 100 -> 105      C_POS_EXACT is this step's d EXACTLY (both levels lie within a factor two of each
                                          other, so L_b - L_a and L_a + (L_b - L_a) are exact): one event, not zero
    3  a multi-crossing step: grey 40 -> 90
the rest is a seeded random image whose pixels change by a random amount in [-60, 60] per interval, a third of them not at
all.

Analytic cases: the 45 x 61 camera of tests/viz_cases.py, the demo room (synthetic.write_demo_sequence's), four consecutive
poses of synthetic.trajectory = three intervals with the state carried, K in {1, 4}.  'arc' is the demo's motion scaled up,
'silhouette' a faster one whose every interval moves the box's outline across pixels (asserted in the CPU test).

Thresholds of the analytic cases, tuned so that in EVERY interval the share of pixels with at least one event lies between
1 % and 50 % (tests/test_event_sim_cpu.py::test_analytic_case_conditions asserts and prints it): arc C = 0.04 gives 6.4 %,
14.0 %, 21.6 % over its three intervals, silhouette C = 0.1 gives 1.2 %, 15.0 %, 24.0 % (K = 4; K = 1 within 0.1 % of that).
The shares grow along a case because the trajectory's yaw grows and sub-threshold changes are carried in the state.

Margin rule.  An analytic pixel is LEFT OUT of the count comparison, for the rest of its case, once its smallest margin --
the distance of d / C from an event boundary, or the smallest relative gap of a geometric decision (t1 vs t2, t1 vs 0, t1 vs
t_wall) -- falls below MARGIN = 1e-9.  That bound is generous against the ~1e-13 by which a few ulps of float64 sin / log and
of the ray geometry can move L; it is an ESTIMATE from the precision of the formats, not a measurement.  At most
MAX_LEFT_OUT = 0.1 % of a case's pixels may be left out (none is, at these seeds).

Bounds of the frame outputs against the yardstick: colour 1e-12, depth 1 float32 ulp, L_ref 1e-9.  For the record, the
yardstick against synthetic.BoxRoom.render on the CPU over all analytic frames (test_analytic_case_conditions prints them):
colour 6.2e-16 at most (BoxRoom's matrix products sum in another order), depth equal bit for bit."""
import numpy as np

from tests import event_sim_numpy as Y
from tests.viz_cases import CAM

EPS = 1e-3
MARGIN = 1e-9
MAX_LEFT_OUT = 1e-3
COLOR_TOL, LREF_TOL = 1e-12, 1e-9
LOG_PATH_MAX_DIFF_SHARE = 1e-3      # in-kernel log against the yardstick: pixels whose count differs (by 1 at most)

_T = Y.table(EPS)
C_POS_EXACT = float(_T[105] - _T[100])
assert float(_T[100] + C_POS_EXACT) == float(_T[105])

IMAGE_SHAPES = [(1, 1), (1, 300), (37, 53)]


def _sequence(shape, channels, seed):
    """four uint8 images [H,W] or [H,W,3]"""
    rng = np.random.default_rng(seed)
    H, W = shape
    full = (H, W) if channels == 1 else (H, W, 3)
    imgs = [rng.integers(0, 256, full).astype(np.int64)]
    for _ in range(3):
        step = rng.integers(-60, 61, full)
        step[rng.random((H, W)) < 1.0 / 3.0] = 0
        imgs.append(np.clip(imgs[-1] + step, 0, 255))
    imgs = [im.astype(np.uint8).reshape(H * W, -1) for im in imgs]
    planted = [(0, 255, 0, 255), (77, 77, 77, 77), (100, 105, 100, 105), (40, 90, 90, 200)]
    for k, values in enumerate(planted[:H * W]):
        for im, v in zip(imgs, values):
            im[k, :] = v
    return [im.reshape(full) for im in imgs]


_cases = {}


def image_cases():
    """name -> dict(shape, channels, K, c_pos, c_neg, sigma_c, seed, images); built once, treat as read-only"""
    if _cases:
        return _cases
    cases, seed = _cases, 100
    for shape in IMAGE_SHAPES:
        for channels in (1, 3):
            for K in (1, 5):
                seed += 1
                name = f"{shape[0]}x{shape[1]}_{'grey' if channels == 1 else 'rgb'}_K{K}"
                cases[name] = dict(shape=shape, channels=channels, K=K, c_pos=0.02, c_neg=0.02, sigma_c=0.0, seed=seed,
                                   images=_sequence(shape, channels, seed))
    # the exact-threshold pixel decides with C_pos = its own d; the per-pixel thresholds; unequal polarities
    cases["37x53_grey_K1_exact"] = dict(cases["37x53_grey_K1"], c_pos=C_POS_EXACT, c_neg=0.05)
    cases["37x53_grey_K5_exact"] = dict(cases["37x53_grey_K5"], c_pos=C_POS_EXACT, c_neg=0.05)
    cases["37x53_grey_K5_maps"] = dict(cases["37x53_grey_K5"], sigma_c=0.6)
    cases["37x53_rgb_K5_maps"] = dict(cases["37x53_rgb_K5"], sigma_c=0.6)
    cases["1x300_grey_K1_maps"] = dict(cases["1x300_grey_K1"], sigma_c=0.6)
    return cases


ANALYTIC = {
    "arc_K1": dict(K=1, step=0.02, yaw_deg=0.4, c=0.04),
    "arc_K4": dict(K=4, step=0.02, yaw_deg=0.4, c=0.04),
    "silhouette_K1": dict(K=1, step=0.05, yaw_deg=2.0, c=0.1),
    "silhouette_K4": dict(K=4, step=0.05, yaw_deg=2.0, c=0.1),
}
ANALYTIC_FRAMES = 4


def demo_room():
    from evennicer_slam_amd.scene import scene_bound
    from evennicer_slam_amd.synthetic import BoxRoom
    return BoxRoom.for_bound(scene_bound([[-1.0, 1.1], [-0.9, 0.8], [-0.7, 0.6]], 1.0, 0.32), margin=0.12, seed=1)


def analytic_poses(name):
    """the case's frames: float64 [4,4] camera-to-world each"""
    from evennicer_slam_amd.synthetic import trajectory
    c = ANALYTIC[name]
    return [p.double().numpy() for p in trajectory(demo_room(), ANALYTIC_FRAMES, step=c['step'], yaw_deg=c['yaw_deg'])]


_analytic_cache = {}


def analytic_reference(name):
    """The yardstick's run of one analytic case, computed once per process and shared (treat as read-only): dict with
    `first` (L_ref after the first frame), `sub_poses` (per interval float64 [K,4,4], from the library's
    interpolate_poses: the poses are an INPUT of both sides) and `steps`, per interval the dict of Y.step_scene plus `ref`
    (L_ref after it) and `left_out` (the cumulative margin-rule mask)."""
    if name not in _analytic_cache:
        from evennicer_slam_amd.event_sim import interpolate_poses
        c, room, poses = ANALYTIC[name], Y.Room(demo_room()), analytic_poses(name)
        sensor = Y.Sensor(Y.first_scene_level(room, poses[0], CAM, EPS), c['c'], c['c'])
        out = dict(first=sensor.ref.copy(), sub_poses=[], steps=[])
        left = np.zeros((CAM['H'], CAM['W']), dtype=bool)
        for a, b in zip(poses[:-1], poses[1:]):
            sub = interpolate_poses(a, b, c['K'])
            step = Y.step_scene(sensor, room, sub, CAM, EPS)
            left = left | (np.minimum(step['count_margin'], step['geo_margin']) < MARGIN)
            step['ref'], step['left_out'] = sensor.ref.copy(), left.copy()
            out['sub_poses'].append(sub)
            out['steps'].append(step)
        _analytic_cache[name] = out
    return _analytic_cache[name]


_image_cache = {}


def image_reference(name, c_pos=None, c_neg=None):
    """The yardstick's run of one image case (once per process): list per interval of (events, L_ref after it); `first` state
    is the level of image 0.  c_pos / c_neg: the per-pixel maps of the simulator under test for the *_maps cases (thresholds
    are an input of both sides)."""
    key = name
    if key not in _image_cache:
        c = image_cases()[name]
        cp = c['c_pos'] if c_pos is None else np.asarray(c_pos)
        cn = c['c_neg'] if c_neg is None else np.asarray(c_neg)
        sensor = Y.Sensor(Y.level_of_image(c['images'][0], EPS), cp, cn)
        steps = []
        for prev, cur in zip(c['images'][:-1], c['images'][1:]):
            ev = Y.step_images(sensor, prev, cur, c['K'], EPS)
            steps.append((ev, sensor.ref.copy()))
        _image_cache[key] = steps
    return _image_cache[key]
