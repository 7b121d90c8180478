"""No GPU: the rigid-motion model of event motion compensation (event_cmax.py 'rigid', enslam_event_cmax_rigid_eval) and the
tracker's opt-in pose prior built on it.

The yardstick (tests/event_cmax_rigid_numpy.py) on hand-worked pixels and one hand-worked gradient; the numpy route against it
on every case of tests/event_cmax_rigid_cases.py -- image and all four counters EQUAL, J equal, mu, f and the six gradient
components inside the bound of tests/event_cmax_cases.py; the gradient formula against torch autograd on the unquantised
statement; the bound bracketed by three deliberately wrong models; the reduction to 'rotation'; relative_motion and
camera_velocity; recovery of a planted motion; every refusal of both new entries without a launch; the tools' flags;
BaseDataset.event_slice; the prior on CPU tensors."""
import ctypes
import importlib.util
import json
import math
import os
import re
import types

import numpy as np
import pytest
import torch

from tests import event_cmax_cases as CC
from tests import event_cmax_numpy as Y
from tests import event_cmax_rigid_cases as RC
from tests import event_cmax_rigid_numpy as YR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPORTS = ("enslam_event_cmax_rigid_workspace", "enslam_event_cmax_rigid_eval")
_CASES = {c['name']: c for c in RC.CASES}
NAMES = [c['name'] for c in RC.CASES]


def _route(case, **over):
    from evennicer_slam_amd import event_cmax as M
    kw = dict(RC.arguments(case), model='rigid')
    kw.update(over)
    return M.cmax_numpy(*RC.stream(case), **kw)


# ---- the yardstick by hand -----------------------------------------------------------------------------------------------------
def test_hand_worked_pixels():
    """5 x 7, fx = fy = 2, (cx, cy) = (3, 2), theta = (1/2, -1/4, 1/2, 1, -1/2, 2), t_ref = 0; depth 2 except where noted.
    Event 1, (3, 2) at t = 1/8: u = v = 0, rho = 1/2, du = 1/4 + (1/2)(0 - 1) = -1/4, dv = 1/2 + (1/2)(0 + 1/2) = 3/4,
    mx = my = -1/4: (3 + 1/16, 2 - 3/16).  Event 2, (4, 0) at t = 1/8, z = 1: u = 1/2, v = -1, uv = -1/2, pu = 5/4, pv = 2;
    du = ((-1/4 + 5/16) - 1/2) + (1 - 1) = -7/16, dv = ((1 - 1/8) - 1/4) + (-2 + 1/2) = -7/8: (4 + 7/64, 7/32).  The others
    likewise; every operand is a short binary fraction, so every x', y' and every weight is exact."""
    case = _CASES['hand_5x7']
    ref = RC.reference(case)
    RC.check_conditions(case, ref)
    pos = [(3.0, 2.0), (3.0625, 1.8125), (4.109375, 0.21875), (1.96875, 3.125), (1.765625, 0.859375), (5.25, 3.21875)]
    assert list(zip(ref['xw'].tolist(), ref['yw'].tolist())) == pos
    want = [[0, 141557760, 462422016, 0, 2988441600, 367001600, 0],
            [0, 865075200, 2825912320, 754974720, 887095296, 102760448, 0],
            [0, 0, 0, 7566524416, 218103808, 0, 0],
            [0, 117440512, 3640655872, 0, 0, 2516582400, 838860800],
            [0, 16777216, 520093696, 0, 0, 704643072, 234881024]]
    assert ref['iwe'].tolist() == want
    # the same integers from the positions alone, in exact arithmetic
    from fractions import Fraction as F
    img = [[F(0)] * 7 for _ in range(5)]
    for xw, yw in pos:
        x0, y0 = math.floor(xw), math.floor(yw)
        a, b = F(xw) - x0, F(yw) - y0
        for c, w in enumerate(((1 - a) * (1 - b), a * (1 - b), (1 - a) * b, a * b)):
            px, py = x0 + (c & 1), y0 + (c >> 1)
            if 0 <= px < 7 and 0 <= py < 5:
                img[py][px] += w * Y.TWO32
    assert [[int(v) for v in row] for row in img] == want and all(v.denominator == 1 for row in img for v in row)
    assert ref['dropped'].tolist() == [0, 0, 0, 0] and ref['voted'].all()
    assert int(ref['iwe'].sum()) == 6 * Y.TWO32                            # nothing fell off the image
    signed = YR.cmax(*RC.stream(case), **dict(RC.arguments(case), signed=True))
    assert signed['iwe'][0, 4] == -want[0][4] and signed['iwe'][3, 5] == -want[3][5] and signed['iwe'][2, 3] == want[2][3]


def test_hand_worked_gradient():
    """1 x 2 pixels, fx = fy = 1, one event at the origin (u = v = 0) one second after t_ref at depth 2, theta = (0, 0, 0, 1/2,
    0, 0): du = -rho v_x = -1/4, x' = 1/4, I = (3/4, 1/4), mu = 1/2, C = D = (1/4, -1/4), f = 1/16; Gx = -1/2, Gy = -1/8,
    mx = my = -1, Bu = (0, -1, 0, -1/2, 0, 0), Bv = (1, 0, -0, 0, -1/2, 0): g = (1/8, -1/2, 0, -1/4, -1/16, 0), 2 / (H W) = 1.
    By hand: x' = w_y + v_x / 2 and f = (1/2 - x')^2, so df / dw_y = -1/2 and df / dv_x = -1/4."""
    from evennicer_slam_amd import event_cmax as M
    depth = np.full((1, 2), 2.0, dtype=np.float32)
    args = dict(H=1, W=2, calib=(1.0, 1.0, 0.0, 0.0), theta=[0.0, 0.0, 0.0, 0.5, 0.0, 0.0], t_ref=0.0, taps=[1.0], depth=depth)
    s = (np.array([1.0]), np.array([0], dtype=np.uint16), np.array([0], dtype=np.uint16), np.array([1], dtype=np.uint8))
    ref = YR.cmax(*s, **args)
    assert ref['J'].tolist() == [[0.75, 0.25]] and ref['mu'] == 0.5 and ref['f'] == 0.0625
    assert (ref['Gx'][0], ref['Gy'][0]) == (-0.5, -0.125) and ref['grad'].tolist() == [0.125, -0.5, 0.0, -0.25, -0.0625, 0.0]
    iwe, J, stats, dropped = M.cmax_numpy(*s, model='rigid', **args)
    assert stats.tolist() == [0.5, 0.0625, 0.125, -0.5, 0.0, -0.25, -0.0625, 0.0] and iwe.tolist() == [[3 << 30, 1 << 30]]
    assert dropped.tolist() == [0, 0, 0, 0]


# ---- the numpy route against the yardstick -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_numpy_route_against_the_yardstick(name):
    case = _CASES[name]
    ref = RC.reference(case)
    RC.check_conditions(case, ref)
    iwe, J, stats, dropped = _route(case)
    assert iwe.dtype == np.int64 and np.array_equal(iwe, ref['iwe'])                    # equal integers, no event left out
    assert dropped.shape == (4,) and dropped.tolist() == ref['dropped'].tolist()
    assert np.array_equal(J.view(np.int64), ref['J'].view(np.int64))
    assert stats.shape == (2 + RC.P,)
    b = CC.bounds(case, ref)
    errs = dict(mu=abs(stats[0] - ref['mu']), f=abs(stats[1] - ref['f']), grad=np.abs(stats[2:] - ref['grad']))
    print(name, {k: (np.asarray(errs[k]).tolist(), np.asarray(b[k]).tolist()) for k in errs})
    assert errs['mu'] <= b['mu'] and errs['f'] <= b['f'] and np.all(errs['grad'] <= b['grad']), (errs, b)
    iwe2, J2, stats2, dropped2 = _route(case, want_grad=False)
    assert np.array_equal(iwe2, iwe) and np.array_equal(stats2[:2].view(np.int64), stats[:2].view(np.int64)) and not stats2[2:].any()
    # a CPU tensor is the same image
    iwe3, _, stats3, _ = _route(case, depth=torch.from_numpy(RC.depth_image(case)))
    assert np.array_equal(iwe3, iwe) and np.array_equal(stats3.view(np.int64), stats.view(np.int64))


GRAD_CASES = ['45x61_N257', '45x61_N700_pixel', '45x61_N700', 'planted_9x12', 'hand_5x7']


@pytest.mark.parametrize("name", GRAD_CASES)
def test_gradient_formula_against_autograd(name):
    case = _CASES[name]
    ref = RC.reference(case)
    kw = RC.arguments(case)
    frac = np.stack([ref['xw'] - np.floor(ref['xw']), ref['yw'] - np.floor(ref['yw'])])[:, ref['voted']]
    if case['kind'] == 'random':
        assert np.all(frac > 0)                                         # no event on a kink of the bilinear vote
    theta = torch.tensor(kw['theta'], dtype=torch.float64, requires_grad=True)
    f = YR.cmax_torch(*RC.stream(case), **dict(kw, theta=theta))
    (g,) = torch.autograd.grad(f, theta)
    q, b = CC.quant_bounds(case, ref), CC.bounds(case, ref)
    assert abs(float(f.detach()) - ref['f']) <= q['f'] + b['f']
    if case['kind'] == 'random':
        assert g.shape == (6,) and np.all(np.abs(g.numpy() - ref['grad']) <= q['grad'] + b['grad']), (g.numpy(), ref['grad'], q['grad'])
        assert np.all(q['grad'] + b['grad'] < 1e-2 * np.abs(ref['grad']).max())          # the bound still tells right from wrong


@pytest.mark.parametrize("variant", ['v_sign', 'rho_on_rotation', 'depth_at_warp'])
def test_wrong_models_leave_the_bound(variant):
    """the bound brackets: each wrong statement of the model misses the route's image, and its gradient by more than a
    thousand bounds"""
    for name in ('45x61_N700_pixel', '45x61_N700'):
        case = _CASES[name]
        good, wrong = RC.reference(case), RC.reference(case, variant=variant)
        iwe, _, stats, _ = _route(case)
        b = CC.bounds(case, good)
        assert np.array_equal(iwe, good['iwe']) and not np.array_equal(iwe, wrong['iwe'])
        assert np.all(np.abs(stats[2:] - good['grad']) <= b['grad']) and abs(stats[1] - good['f']) <= b['f']
        assert abs(stats[1] - wrong['f']) > 1000 * b['f'], (variant, name)
        assert np.abs(stats[2:] - wrong['grad']).max() > 1000 * b['grad'].max(), (variant, name)


def test_without_translation_the_image_is_the_rotation_models():
    """v = 0 and every depth valid: rho multiplies an exact zero, and the rigid IWE is the 'rotation' IWE integer for integer"""
    from evennicer_slam_amd import event_cmax as M
    for name in ('45x61_N700', '45x61_N257', '8x9_N65537'):
        case = _CASES[name]
        kw = RC.arguments(case)
        depth = np.where(np.isfinite(kw['depth']) & (kw['depth'] > 0), kw['depth'], np.float32(1.25)).astype(np.float32)
        theta = kw['theta'][:3] + [0.0, 0.0, 0.0]
        common = dict(H=kw['H'], W=kw['W'], calib=kw['calib'], t_ref=kw['t_ref'], taps=kw['taps'], signed=kw['signed'])
        rig = M.cmax_numpy(*RC.stream(case), model='rigid', theta=theta, depth=depth, **common)
        rot = M.cmax_numpy(*RC.stream(case), model='rotation', theta=theta[:3], **common)
        assert np.array_equal(rig[0], rot[0]) and rig[3].tolist() == rot[3].tolist() + [0]
        assert np.array_equal(rig[2][:5].view(np.int64), rot[2].view(np.int64))          # mu, f and the rotation's own gradient


# ---- relative_motion, camera_velocity --------------------------------------------------------------------------------------
THETAS = (((0.3, -0.5, 0.8, 0.5, -0.3, 0.4), 0.1), ((0.0, 0.0, 0.0, 1.0, 2.0, -3.0), 0.5), ((2.0, 1.0, -3.0, -1.0, 0.5, 2.0), 0.7),
          ((1e-9, 0.0, 0.0, 1.0, 0.0, 0.0), 1e-6), ((0.0, 0.0, 0.0, 0.0, 0.0, 0.0), 1.0))


def test_relative_motion_and_camera_velocity_are_inverses():
    from evennicer_slam_amd import event_cmax as M
    rng = np.random.default_rng(0)
    for theta, dt in THETAS:
        D = M.relative_motion(theta, dt)
        assert D.dtype == torch.float64 and tuple(D.shape) == (4, 4) and torch.equal(D[3], torch.tensor([0.0, 0.0, 0.0, 1.0], dtype=torch.float64))
        # the SE(3) exponential of the twist in the project's frame: y and z of w and of v flip
        w = torch.tensor([theta[0], -theta[1], -theta[2]], dtype=torch.float64) * dt
        v = torch.tensor([theta[3], -theta[4], -theta[5]], dtype=torch.float64) * dt
        X = torch.zeros((4, 4), dtype=torch.float64)
        X[:3, :3] = torch.tensor([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]], dtype=torch.float64)
        X[:3, 3] = v
        assert torch.allclose(D, torch.linalg.matrix_exp(X), rtol=0, atol=1e-13)
        base = M.relative_motion(rng.uniform(-1, 1, 6).tolist(), 1.0)                  # any pose
        back = M.camera_velocity(base, base @ D, dt)
        assert np.allclose(back, theta, rtol=1e-8, atol=1e-9 * max(1.0, 1.0 / dt) * 1e-3), (theta, back)
        # without translation: relative_rotation, and angular_velocity on the way back
        R = M.relative_motion(list(theta[:3]) + [0.0, 0.0, 0.0], dt)
        assert torch.equal(R, M.relative_rotation(theta[:3], dt))
    with pytest.raises(M.EnslamError):
        M.relative_motion([0.1, 0.2, 0.3], 1.0)


def test_relative_motion_moves_pixels_the_way_the_warp_assumes():
    """Seeded 3-D points seen from c2w and from c2w @ relative_motion(theta, dt): their projected displacement over dt agrees
    with the model's (fx du, fy dv) to second order -- halving dt divides the error of the velocity by about 2 (of the
    displacement by about 4): the signs and the frames of the warp and of the pose delta agree."""
    from evennicer_slam_amd import event_cmax as M
    fx, fy, cx, cy = 80.0, 75.0, 30.0, 22.0
    theta = [0.3, -0.5, 0.8, 0.5, -0.3, 0.4]
    rng = np.random.default_rng(3)
    c2w = M.relative_motion(rng.uniform(-1, 1, 6).tolist(), 1.0).numpy()
    px, py, z = rng.uniform(0, 60, 50), rng.uniform(0, 44, 50), rng.uniform(1.0, 4.0, 50)
    u, v = (px - cx) / fx, (py - cy) / fy
    world = c2w @ np.stack([u * z, -v * z, -z, np.ones(50)])
    du = u * v * theta[0] - (1 + u * u) * theta[1] + v * theta[2] + (u * theta[5] - theta[3]) / z
    dv = (1 + v * v) * theta[0] - u * v * theta[1] - u * theta[2] + (v * theta[5] - theta[4]) / z
    errs = []
    for dt in (4e-3, 2e-3, 1e-3):
        c = np.linalg.inv(c2w @ M.relative_motion(theta, dt).numpy()) @ world
        qx, qy = cx + fx * (c[0] / -c[2]), cy + fy * (-c[1] / -c[2])
        err = np.hypot((qx - px) - fx * du * dt, (qy - py) - fy * dv * dt)             # pixels
        errs.append(float(err.max()))
        assert float(np.hypot(qx - px, qy - py).max()) > 100 * errs[-1]                 # a small part of the displacement itself
    assert 3.5 < errs[0] / errs[1] < 4.5 and 3.5 < errs[1] / errs[2] < 4.5, errs
    # the yardstick's own warp is that field: an event dt after t_ref is taken back by (fx du, fy dv) dt
    for j in range(5):
        xi, yi = int(round(px[j])), int(round(py[j]))
        xw, yw = YR.warp(theta, (fx, fy, cx, cy), 0.0, 1e-3, xi, yi, float(z[j]))[:2]
        uu, vv = (xi - cx) / fx, (yi - cy) / fy
        du_j = uu * vv * theta[0] - (1 + uu * uu) * theta[1] + vv * theta[2] + (uu * theta[5] - theta[3]) / z[j]
        assert xw - xi == pytest.approx(-1e-3 * fx * du_j, rel=1e-9) and yw != yi


# ---- recovery ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", RC.REC_SEEDS)
def test_recovery_on_a_planted_motion(seed):
    """theta0 = truth (1 +- 0.2) per component; the reference time is the middle of the window, as in the other recovery tests.
    The bars: every accepted step raises f, and the estimate's warp is nearer the truth's than theta0's was -- the mean over the
    sensor of the distance between the two end-of-window displacements."""
    from evennicer_slam_amd import event_cmax as M
    from evennicer_slam_amd.event_stream import EventStream
    s = RC.planted_stream(seed)
    depth = RC.rec_depth()
    assert len(s[0]) > 500 and 1.0 < float(depth.min()) and float(depth.max()) < 4.0
    theta0 = RC.rec_theta0(seed)
    assert all(abs(abs(a / b) - 1.0) == pytest.approx(0.2) for a, b in zip(theta0, RC.REC_TRUTH))
    stream = EventStream(*s)
    kw = dict(H=CC.REC_H, W=CC.REC_W, sigma=CC.SIGMA, ksize=CC.REC_K, t_ref=CC.REC_WINDOW / 2)
    res = M.estimate_motion(stream, CC.REC_CALIB, 'rigid', theta0=theta0, depth=torch.from_numpy(depth), **kw)
    trace = res['trace']
    assert res['thetas'][0] == theta0 and len(trace) == len(res['thetas']) > 3
    assert all(b > a for a, b in zip(trace, trace[1:]))
    ykw = dict(H=CC.REC_H, W=CC.REC_W, calib=CC.REC_CALIB, t_ref=CC.REC_WINDOW / 2, taps=CC.taps_of(CC.REC_K), depth=depth)
    assert YR.cmax(*s, theta=theta0, **ykw)['f'] == pytest.approx(trace[0], rel=1e-12)
    assert YR.cmax(*s, theta=res['theta'], **ykw)['f'] == pytest.approx(trace[-1], rel=1e-12)
    truth = RC.field(RC.REC_TRUTH, CC.REC_WINDOW)
    off = lambda th: float(np.linalg.norm(RC.field(th, CC.REC_WINDOW) - truth, axis=-1).mean())     # noqa: E731
    errors = RC.component_errors(res['theta'])
    print(seed, 'evals', res['evals'], 'steps', len(trace) - 1, 'pixels off', off(res['theta']), 'from', off(theta0), 'errors', errors,
          'recorded', RC.REC_RECORD[seed])
    assert off(res['theta']) < off(theta0)
    f, grad = M.contrast(stream, CC.REC_CALIB, 'rigid', res['theta'], CC.REC_H, CC.REC_W, t_ref=kw['t_ref'], ksize=CC.REC_K, depth=depth)
    assert f == trace[-1] and grad.shape == (6,)
    img, blurred, dropped = M.warp_image(stream, CC.REC_CALIB, 'rigid', res['theta'], CC.REC_H, CC.REC_W, t_ref=kw['t_ref'], ksize=CC.REC_K,
                                         depth=depth, with_dropped=True)
    assert set(dropped) == set(M.DROPPED_RIGID) and float(blurred.var(unbiased=False)) == pytest.approx(f, rel=1e-9)


# ---- ABI, refusals ------------------------------------------------------------------------------------------------------------
def test_abi_exports():
    import evennicer_slam_amd as E
    from evennicer_slam_amd import event_cmax as M
    from evennicer_slam_amd import functional as EF
    header = open(os.path.join(ROOT, "include", "enslam_hip.h")).read()
    handle = E._lib.lib()
    for name in EXPORTS:
        assert name in E._lib.EXPORTS and re.search(r"\b%s\s*\(" % name, header) and hasattr(handle, name), name
    assert re.search(r"#define ENSLAM_CMAX_DROP_DEPTH 3\b", header) and M.DROPPED_RIGID.index('depth') == 3
    assert M.MODELS['rigid'] == EF.EVENT_CMAX_RIGID == 6 and M.DROPPED == ('time', 'sensor', 'warp')


def check_refusals(t, x, y, p, depth, N, H, W, ws, ws_bytes, iwe, blurred, stats, dropped):
    """Every refusal of enslam_event_cmax_rigid_eval returns its code; nothing is launched (the GPU test looks at the buffers).
    The pointers only have to be non-NULL and 8-byte aligned: a refusal comes before any of them is used."""
    from evennicer_slam_amd import _lib as L
    lib = L.lib()
    EINVAL, EUNSUPPORTED = -1, -3
    nan, inf = float('nan'), float('inf')

    def call(n=N, hh=H, ww=W, cal=(80.0, 80.0, 3.0, 2.0), theta=(0.1, 0.2, 0.3, 0.4, 0.5, 0.6), t_ref=0.0, k=3, taps=None, ptrs=None,
             nbytes=ws_bytes):
        q = dict(t=t, x=x, y=y, p=p, depth=depth, ws=ws, iwe=iwe, blurred=blurred, stats=stats, dropped=dropped,
                 theta=(ctypes.c_double * 6)(*theta), taps=(ctypes.c_double * 64)(*(taps or [1.0 / max(k, 1)] * max(k, 1))))
        q.update(ptrs or {})
        return lib.enslam_event_cmax_rigid_eval(q['t'], q['x'], q['y'], q['p'], n, hh, ww, cal[0], cal[1], cal[2], cal[3], q['depth'],
                                                q['theta'], t_ref, 0, k, q['taps'], q['ws'], nbytes, q['iwe'], q['blurred'], q['stats'],
                                                q['dropped'], 1, None)

    for name in ('t', 'x', 'y', 'p', 'depth', 'ws', 'iwe', 'stats', 'dropped', 'theta', 'taps'):
        assert call(ptrs={name: None}) == EINVAL, name
    assert call(n=-1) == EINVAL and call(hh=0) == EINVAL and call(ww=-3) == EINVAL
    for bad in (nan, inf, -inf):
        for i in range(6):
            theta = [0.1, 0.2, 0.3, 0.4, 0.5, 0.6]
            theta[i] = bad
            assert call(theta=theta) == EINVAL, (i, bad)
        assert call(t_ref=bad) == EINVAL and call(taps=[0.25, bad, 0.25]) == EINVAL
        for i in range(4):
            cal = [80.0, 80.0, 3.0, 2.0]
            cal[i] = bad
            assert call(cal=cal) == EINVAL
    assert call(cal=(0.0, 80.0, 3.0, 2.0)) == EINVAL and call(cal=(80.0, -0.0, 3.0, 2.0)) == EINVAL
    assert call(k=0) == EINVAL and call(k=4) == EINVAL and call(k=-3) == EINVAL and call(k=32) == EINVAL
    assert call(k=33) == EUNSUPPORTED
    need = ctypes.c_int64(-1)
    assert lib.enslam_event_cmax_rigid_workspace(H, W, N, ctypes.byref(need)) == 0 and 0 < need.value <= ws_bytes
    assert call(nbytes=need.value - 8) == EINVAL and call(nbytes=0) == EINVAL and call(nbytes=-need.value) == EINVAL
    for name, base in (('ws', ws), ('iwe', iwe), ('blurred', blurred), ('stats', stats), ('dropped', dropped)):
        assert call(ptrs={name: base + 4}) == EINVAL, name
    assert call(n=1 << 31) == EUNSUPPORTED and call(hh=65537) == EUNSUPPORTED and call(ww=65537) == EUNSUPPORTED
    assert call(hh=65536, ww=8192) == EUNSUPPORTED                                     # more than 2^28 pixels
    n = ctypes.c_int64(-1)
    assert lib.enslam_event_cmax_rigid_workspace(H, W, N, None) == EINVAL
    for args, code in (((0, W, N), EINVAL), ((H, W, -1), EINVAL), ((H, W, 1 << 31), EUNSUPPORTED), ((65537, 1, N), EUNSUPPORTED),
                       ((32768, 16384, N), EUNSUPPORTED)):
        assert lib.enslam_event_cmax_rigid_workspace(*args, ctypes.byref(n)) == code and n.value == -1, args
    # the existing formula with P = 6
    assert lib.enslam_event_cmax_rigid_workspace(45, 61, 700, ctypes.byref(n)) == 0 and n.value == (3 * 2745 + 3 * 6) * 8
    assert lib.enslam_event_cmax_rigid_workspace(5, 7, 20000, ctypes.byref(n)) == 0 and n.value == (3 * 35 + 79 * 6) * 8
    # ... and the old pair still stops at three parameters
    for P in (4, 5, 6):
        assert lib.enslam_event_cmax_workspace(H, W, N, P, ctypes.byref(n)) == EINVAL


def test_every_refusal_has_its_code_and_its_error_class():
    from evennicer_slam_amd import _lib as L
    from evennicer_slam_amd import event_cmax as M
    from evennicer_slam_amd import functional as EF
    from evennicer_slam_amd.event_stream import EventStream
    host = (ctypes.c_double * 8192)()
    a = ctypes.addressof(host)
    assert a % 8 == 0
    check_refusals(a, a, a, a, a, 10, 5, 7, a, 8192 * 8, a, a, a, a)
    case = _CASES['hand_5x7']
    s = RC.stream(case)
    ok = dict(RC.arguments(case), model='rigid')
    d = ok['depth']
    nan = float('nan')
    for bad in (dict(depth=None), dict(depth=d.astype(np.float64)), dict(depth=d[:4]), dict(depth=d.reshape(-1)), dict(depth=d.tolist()),
                dict(depth=torch.from_numpy(d).double()), dict(theta=[0.1, 0.2, 0.3]), dict(theta=[0.1, 0.2, 0.3, 0.4, nan, 0.6]),
                dict(model='rotation', theta=[0.1, 0.2, 0.3]), dict(model='flow', theta=[1.0, 2.0]), dict(calib=(0.0, 2.0, 3.0, 2.0)),
                dict(taps=[0.5, 0.5]), dict(H=0), dict(t_ref=float('inf'))):
        with pytest.raises(L.EnslamError):
            M.cmax_numpy(*s, **dict(ok, **bad))
    stream = EventStream(*s)
    kw = dict(H=5, W=7, t_ref=0.0, ksize=1)
    for fn in (M.estimate_motion, ):
        with pytest.raises(L.EnslamError):
            fn(stream, ok['calib'], 'rigid', **kw)                       # no depth
        with pytest.raises(L.EnslamError):
            fn(stream, ok['calib'], 'rotation', depth=d, **kw)           # a depth nobody asked for
    for model, theta, depth in (('rigid', ok['theta'], None), ('rotation', [0.1, 0.2, 0.3], d), ('flow', [1.0, 2.0], torch.from_numpy(d))):
        with pytest.raises(L.EnslamError):
            M.contrast(stream, ok['calib'], model, theta, 5, 7, t_ref=0.0, ksize=1, depth=depth)
        with pytest.raises(L.EnslamError):
            M.warp_image(stream, ok['calib'], model, theta, 5, 7, t_ref=0.0, ksize=1, depth=depth)
    with pytest.raises(L.EnslamError):                                  # the device entry point takes device tensors only
        EF.event_cmax_eval(*(torch.from_numpy(v) for v in s), 5, 7, ok['calib'], 'rigid', ok['theta'], 0.0, [1.0], depth=torch.from_numpy(d))


# ---- tools ------------------------------------------------------------------------------------------------------------------------
def _tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_tools_flags(capsys, tmp_path):
    from evennicer_slam_amd.event_stream import EventStream
    tool = _tool("event_motion")
    with pytest.raises(SystemExit) as e:
        tool.main(['--help'])
    text = capsys.readouterr().out
    assert e.value.code == 0 and all(flag in text for flag in ('rigid', '--depth DEPTH', '--depth-scale'))
    for bad in (['--stream', 'x.npz', '--size', '5', '7', '--calib', '1', '1', '0', '0', '--fps', '30', '--model', 'rigid'],
                ['--stream', 'x.npz', '--size', '5', '7', '--calib', '1', '1', '0', '0', '--fps', '30', '--depth', 'd.npy'],
                ['--demo', '3', '--depth', 'd.npy'], ['--demo', '3', '--model', 'affine']):
        with pytest.raises(SystemExit) as e:
            tool.main(bad)
        assert e.value.code == 2, bad
    capsys.readouterr()
    # a stream file and a depth file through the tool on the CPU route: .npy, and the same image as a 16-bit png
    from PIL import Image
    s = EventStream(*RC.planted_stream(0))
    path = str(tmp_path / 'events.npz')
    s.save(path)
    np.save(str(tmp_path / 'depth.npy'), RC.rec_depth())
    Image.fromarray(np.round(RC.rec_depth().astype(np.float64) * 1000.0).astype(np.uint16)).save(str(tmp_path / 'depth.png'))
    stamps = tmp_path / 'stamps.txt'
    stamps.write_text("0.0\n0.1\n")
    common = ['--stream', path, '--size', str(CC.REC_H), str(CC.REC_W), '--calib'] + [repr(v) for v in CC.REC_CALIB] + \
             ['--stamps', str(stamps), '--model', 'rigid', '--device', 'cpu', '--iters', '3']
    out = tool.main(common + ['--depth', str(tmp_path / 'depth.npy')])
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert line['intervals'] == 1 and line['model'] == 'rigid' and len(out['rows'][0]['theta']) == 6 and out['rows'][0]['events'] == len(s)
    assert out['rows'][0]['contrast_after'] > out['rows'][0]['contrast_before']
    png = tool.main(common + ['--depth', str(tmp_path / 'depth.png'), '--depth-scale', '1000'])
    assert np.allclose(png['rows'][0]['theta'], out['rows'][0]['theta'], rtol=0.2, atol=0.05)      # millimetre rounding of the depth
    capsys.readouterr()
    with pytest.raises(SystemExit):
        tool.main(common[:4] + ['7', '9'] + common[6:] + ['--depth', str(tmp_path / 'depth.npy')])   # a depth of another size
    bench = open(os.path.join(ROOT, "tools", "bench_event_cmax.py")).read()
    assert "_rigid'] = row" in bench and 'DROPPED_RIGID' in bench and bench.count('device_below_numpy=') == 2
    runner = _tool("run_slam")
    ap_text = open(os.path.join(ROOT, "tools", "run_slam.py")).read()
    assert "add_argument('--motion-prior', choices=('const_speed', 'cmax')" in ap_text
    cfg = runner.apply_schedule_arguments({}, types.SimpleNamespace(schedule=None, rgbd_every=None, depth_on_event_frames=None, motion_prior='cmax'))
    assert cfg['tracking'] == {'motion_prior': 'cmax'}
    assert 'tracking' not in runner.apply_schedule_arguments({}, types.SimpleNamespace(schedule=None, rgbd_every=None, depth_on_event_frames=None,
                                                                                       motion_prior=None))
    synth = _tool("run_synthetic_slam")
    assert synth.parse_args(['7', '--events', 'simulate', '--motion-prior', 'cmax'])[1]['motion_prior'] == 'cmax'
    assert 'motion_prior' not in synth.parse_args(['7'])[1]
    for bad in (['--motion-prior', 'cmax'], ['--events', 'simulate', '--motion-prior', 'gyro']):
        with pytest.raises(SystemExit):
            synth.parse_args(bad)


# ---- event_slice and the prior on CPU tensors ------------------------------------------------------------------------------------
N_FRAMES = 5
CAM = dict(H=60, W=80, fx=70.0, fy=70.0, cx=39.5, cy=29.5)
_SEQ = {}


def demo_sequence(root, device='cpu'):
    """(cfg, dataset, poses, streams, stamps): five frames of the analytic room at a step and a threshold that give a few
    hundred events per interval, simulated with time stamps; written once per process and device"""
    if device not in _SEQ:
        from evennicer_slam_amd import datasets as D
        from evennicer_slam_amd.event_sim import EventSimulator
        from evennicer_slam_amd.event_stream import EventStream
        from evennicer_slam_amd.synthetic import demo_config, write_demo_sequence
        root = str(root)
        stamps, streams = [i / 30.0 for i in range(N_FRAMES)], []
        sim = EventSimulator(CAM['H'], CAM['W'], c_pos=0.1, c_neg=0.1, device=device)
        (inp, evf), poses = write_demo_sequence(os.path.join(root, 'data'), N_FRAMES, CAM, step=0.04, yaw_deg=2.0, events='simulate', sim=sim,
                                                stamps=stamps, streams=streams)
        EventStream.concatenate(streams).save(os.path.join(root, 'events.npz'))
        with open(os.path.join(root, 'stamps.txt'), 'w') as f:
            f.write(''.join(f'{v!r}\n' for v in stamps))
        cfg = demo_config(inp, evf, CAM, device=device)
        cfg['data'] = dict(cfg['data'], event_stream=os.path.join(root, 'events.npz'), frame_stamps=os.path.join(root, 'stamps.txt'))
        cfg['tracking'] = dict(cfg['tracking'], iters=0, cmax_min_events=100)
        ds = D.get_dataset(cfg, types.SimpleNamespace(input_folder=None, event_folder=None), 1, device=device)
        _SEQ[device] = (cfg, ds, poses, [s.to('cpu') for s in streams], stamps)
    return _SEQ[device]


def with_prior(cfg, prior, **more):
    out = dict(cfg)
    out['tracking'] = dict(cfg['tracking'], motion_prior=prior, **more)
    return out


def test_event_slice_is_the_interval_of_the_stamps(tmp_path_factory):
    from evennicer_slam_amd.event_stream import EventStream
    cfg, ds, poses, streams, stamps = demo_sequence(tmp_path_factory.mktemp('seq'))
    whole = EventStream.concatenate(streams).time_sorted()
    t = whole.t.numpy()
    total = 0
    for idx in range(1, N_FRAMES):
        part, t0, t1 = ds.event_slice(idx)
        assert (t0, t1) == (stamps[idx - 1], stamps[idx]) and part.device.type == 'cpu'
        mask = (t > t0) & (t <= t1)                                     # the bin rule: an event at a frame's time ends its interval
        assert len(part) == int(mask.sum()) > 100
        for got, want in zip(part.numpy(), whole.numpy()):
            assert np.array_equal(got, want[mask])
        total += len(part)
    assert total == int(((t > stamps[0]) & (t <= stamps[-1])).sum())
    for bad in (0, N_FRAMES, -1):
        with pytest.raises(IndexError):
            ds.event_slice(bad)


def recomposed(slam, ds, idx, min_events=None):
    """the initial pose of frame idx from estimate_motion and relative_motion, as the harness is specified to compose it"""
    from evennicer_slam_amd import event_cmax as M
    from evennicer_slam_amd import functional as EF
    stream, t0, t1 = ds.event_slice(idx)
    pre = slam.estimate_c2w_list[idx - 1].double()
    theta0 = [0.0] * 6
    if idx >= 2:
        theta0 = M.camera_velocity(slam.estimate_c2w_list[idx - 2], slam.estimate_c2w_list[idx - 1], t0 - ds.event_slice(idx - 1)[1])
    src, depth = slam._last_rgbd
    m = EF.relative_camera_matrix(slam.estimate_c2w_list[src], pre)
    d = EF.depth_forecast(depth.float().contiguous(), slam.cam, m, (slam.H, slam.W), radius=slam.forecast_radius, z_near=0.0,
                          fill=slam.forecast_fill)
    res = M.estimate_motion(stream, (slam.fx, slam.fy, slam.cx, slam.cy), 'rigid', slam.H, slam.W, theta0=theta0, t_ref=t0, depth=d,
                            iters=slam.cmax_iters)
    return (pre @ M.relative_motion(res['theta'], t1 - t0)).float(), res


def const_speed(slam, idx, device='cpu'):
    """today's initial pose, as slam.track has computed it since the reference (on the harness's device)"""
    pre = slam.estimate_c2w_list[idx - 1].to(device).float()
    return (pre @ slam.estimate_c2w_list[idx - 2].to(device).float().inverse()) @ pre if idx >= 2 else pre


def test_the_prior_on_cpu_tensors(tmp_path_factory, monkeypatch):
    from evennicer_slam_amd import event_cmax as M
    from evennicer_slam_amd.slam import SLAM
    root = tmp_path_factory.mktemp('prior')
    cfg, ds, poses, streams, stamps = demo_sequence(tmp_path_factory.mktemp('seq'))

    def harness(c, tag):
        slam = SLAM(c, ds, str(root / tag), device='cpu')
        for i in range(N_FRAMES):
            slam.estimate_c2w_list[i] = ds[i][-1]
        slam._last_rgbd = (0, ds[0][2])
        return slam

    track = lambda slam, idx: slam.track(idx, None, None, None, None, None, rgbd=False)          # noqa: E731  (no loss: est itself)
    plain, default = harness(with_prior(cfg, 'const_speed'), 'plain'), harness(cfg, 'default')
    slam = harness(with_prior(cfg, 'cmax'), 'cmax')
    assert default.motion_prior == 'const_speed' and slam.cmax_min_events == 100 and default.cmax_iters == 10
    for idx in (1, 2, 3):
        want = torch.eye(4)
        want[:3] = const_speed(plain, idx)[:3]
        assert torch.equal(track(plain, idx), want) and torch.equal(track(default, idx), want)
    assert plain.motion_prior_stats == dict(cmax=0, few_events=0, no_depth=0, not_finite=0, no_rise=0, seconds=0.0)
    used = 0
    for idx in (2, 3, 4):
        before = dict(slam.motion_prior_stats)
        got = track(slam, idx)
        est, res = recomposed(slam, ds, idx)
        if res['trace'][-1] > res['trace'][0]:
            assert torch.equal(got[:3], est[:3]) and slam.motion_prior_stats['cmax'] == before['cmax'] + 1
            assert not torch.equal(got[:3], const_speed(slam, idx)[:3])
            used += 1
        else:
            assert torch.equal(got[:3], const_speed(slam, idx)[:3]) and slam.motion_prior_stats['no_rise'] == before['no_rise'] + 1
    assert used >= 2 and slam.motion_prior_stats['seconds'] > 0.0
    # the fallbacks, each counted and each the constant-speed pose
    def falls_back(s, cause, idx=3):
        before = dict(s.motion_prior_stats)
        got = track(s, idx)
        assert torch.equal(got[:3], const_speed(s, idx)[:3])
        after = s.motion_prior_stats
        assert after[cause] == before[cause] + 1 and all(after[k] == before[k] for k in after if k not in (cause, 'seconds')), (cause, after)

    few = harness(with_prior(cfg, 'cmax', cmax_min_events=10 ** 9), 'few')
    falls_back(few, 'few_events')
    flat = harness(with_prior(cfg, 'cmax', cmax_iters=0), 'flat')        # no step taken: the contrast cannot have risen
    falls_back(flat, 'no_rise')
    blind = harness(with_prior(cfg, 'cmax'), 'blind')
    blind._last_rgbd = None
    falls_back(blind, 'no_depth')
    poisoned = harness(with_prior(cfg, 'cmax'), 'poisoned')
    real = M.estimate_motion
    monkeypatch.setattr(M, 'estimate_motion', lambda *a, **k: dict(real(*a, **k), theta=[0.0, float('nan'), 0.0, 0.0, 0.0, 0.0]))
    falls_back(poisoned, 'not_finite')
    monkeypatch.undo()
    # construction refuses what the prior cannot work with
    bare = dict(cfg, data={k: v for k, v in cfg['data'].items() if k not in ('event_stream', 'frame_stamps')})
    from evennicer_slam_amd import datasets as D
    ds_png = D.get_dataset(bare, types.SimpleNamespace(input_folder=None, event_folder=None), 1, device='cpu')
    with pytest.raises(ValueError, match='event_stream'):
        SLAM(with_prior(bare, 'cmax'), ds_png, str(root / 'bare'), device='cpu')
    SLAM(with_prior(bare, 'const_speed'), ds_png, str(root / 'bare_ok'), device='cpu')
    with pytest.raises(ValueError, match='motion_prior'):
        SLAM(with_prior(cfg, 'gyro'), ds, str(root / 'gyro'), device='cpu')
    cropped = dict(with_prior(cfg, 'cmax'), cam=dict(cfg['cam'], crop_edge=2))
    with pytest.raises(ValueError, match='uncropped'):
        SLAM(cropped, ds, str(root / 'cropped'), device='cpu')
    with pytest.raises(ValueError):
        ds_png.event_slice(1)
