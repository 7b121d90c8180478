"""No GPU: event motion compensation by contrast maximisation (evennicer_slam_amd/event_cmax.py, enslam_event_cmax_eval).

The yardstick (tests/event_cmax_numpy.py, one event at a time, Python ints, math.fsum) on hand-worked pixels and one hand-worked
gradient; the numpy route cmax_numpy against it on every case of tests/event_cmax_cases.py -- image and counters EQUAL, J equal
(its operations are fixed one by one), mu, f and the gradient inside the bound derived there; the gradient formula against
torch autograd on the unquantised statement; the bound bracketed by three deliberately wrong variants; recovery of a planted
flow and a planted rotation; relative_rotation; the tools' flags; the ABI exports and every refusal, without a launch."""
import ctypes
import importlib.util
import json
import math
import os
import re

import numpy as np
import pytest
import torch

from tests import event_cmax_cases as CC
from tests import event_cmax_numpy as Y

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPORTS = ("enslam_event_cmax_workspace", "enslam_event_cmax_eval")
_CASES = {c['name']: c for c in CC.CASES}
NAMES = [c['name'] for c in CC.CASES]


def _route(case, **over):
    from evennicer_slam_amd import event_cmax as M
    kw = CC.arguments(case)
    kw.update(over)
    return M.cmax_numpy(*CC.stream(case), **kw)


# ---- the yardstick by hand ---------------------------------------------------------------------------------------------------
def test_hand_worked_pixels():
    """5 x 7, fx = fy = 2, flow (4, -2), t_ref = 0: x' = x - 4 t, y' = y + 2 t, every weight a dyadic fraction"""
    case = _CASES['hand_5x7']
    ref = CC.reference(case)
    want = np.zeros((5, 7))
    want[2, 3] += 1.0                                                   # (3, 2) at t = 0: on the lattice
    want[0, 3] += 0.375; want[0, 4] += 0.375; want[1, 3] += 0.125; want[1, 4] += 0.125      # (3.5, 0.25)   # noqa: E702
    want[4, 1] += 0.375; want[4, 2] += 0.375                            # (1.5, 4.25): the lower corners are below the image
    want[1, 0] += 0.375; want[2, 0] += 0.125                            # (-0.5, 1.25): the left corners are outside
    want[2, 5] += 0.09375; want[2, 6] += 0.03125; want[3, 5] += 0.65625; want[3, 6] += 0.21875    # (5.25, 2.875)   # noqa: E702
    want[4, 6] += 1.0                                                   # the last column and row
    assert np.array_equal(ref['iwe'], (want * Y.TWO32).astype(np.int64))
    assert ref['dropped'].tolist() == [0, 0, 0] and ref['voted'].all()
    assert np.array_equal(ref['J'], want)                               # k = 1: no blur
    assert ref['mu'] == 5.25 / 35 and ref['f'] == pytest.approx(float(((want - 0.15) ** 2).mean()), rel=1e-14)
    # signed votes: the two events of polarity 0 flip
    signed = Y.cmax(*CC.stream(case), **dict(CC.arguments(case), signed=True))
    assert signed['iwe'][4, 1] == -int(0.375 * Y.TWO32) and signed['iwe'][3, 5] == -int(0.65625 * Y.TWO32) and signed['iwe'][2, 3] == Y.TWO32


def test_hand_worked_gradient():
    """1 x 2 pixels, fx = fy = 1, one event at the origin one second after t_ref, flow (-1/4, 0): x' = 1/4, I = (3/4, 1/4),
    mu = 1/2, C = (1/4, -1/4), f = 1/16.  Gx = -1/4 - 1/4, Gy = -(3/4)/4 + (1/4)/4 = -1/8 (the corners below are outside);
    mx = my = -1: g = (1/2, 1/8), and 2 / (H W) = 1.  By hand: f = (1/2 - a)^2 with a = -theta_0, df/dtheta_0 = 2 (1/2 - 1/4)."""
    from evennicer_slam_amd import event_cmax as M
    args = dict(H=1, W=2, calib=(1.0, 1.0, 0.0, 0.0), model='flow', theta=[-0.25, 0.0], t_ref=0.0, taps=[1.0])
    s = (np.array([1.0]), np.array([0], dtype=np.uint16), np.array([0], dtype=np.uint16), np.array([1], dtype=np.uint8))
    ref = Y.cmax(*s, **args)
    assert ref['J'].tolist() == [[0.75, 0.25]] and ref['mu'] == 0.5 and ref['f'] == 0.0625
    assert (ref['Gx'][0], ref['Gy'][0]) == (-0.5, -0.125) and ref['grad'].tolist() == [0.5, 0.125]
    iwe, J, stats, dropped = M.cmax_numpy(*s, **args)
    assert stats.tolist() == [0.5, 0.0625, 0.5, 0.125] and iwe.tolist() == [[3 << 30, 1 << 30]] and dropped.tolist() == [0, 0, 0]


def test_tree_sum_is_the_stated_order():
    from evennicer_slam_amd.event_cmax import tree_sum
    rng = np.random.default_rng(0)
    for n in (0, 1, 255, 256, 257, 65536, 65537, 140000):
        v = rng.standard_normal(n) * 10.0 ** rng.integers(-8, 8, n)
        pad = np.concatenate([v, np.zeros(-n % 256)])
        lvl = []
        for level in range(2):                                          # the tree, one block at a time, in plain Python floats
            lvl = []
            for b in range(len(pad) // 256):
                w = pad[b * 256:(b + 1) * 256].tolist()
                s = 128
                while s >= 1:
                    for i in range(s):
                        w[i] = w[i] + w[i + s]
                    s //= 2
                lvl.append(w[0])
            pad = np.concatenate([np.array(lvl), np.zeros(-len(lvl) % 256)])
        acc = 0.0
        for x in lvl:
            acc = acc + x
        assert tree_sum(v) == acc
        assert abs(acc - math.fsum(v.tolist())) <= CC.SLACK * CC.depth(max(n, 1)) * CC.U * float(np.abs(v).sum())


# ---- the numpy route against the yardstick ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_numpy_route_against_the_yardstick(name):
    case = _CASES[name]
    ref = CC.reference(case)
    CC.check_conditions(case, ref)
    iwe, J, stats, dropped = _route(case)
    assert iwe.dtype == np.int64 and np.array_equal(iwe, ref['iwe'])                    # equal integers, no event left out
    assert dropped.tolist() == ref['dropped'].tolist()
    assert np.array_equal(J.view(np.int64), ref['J'].view(np.int64))                    # the blur is fixed operation by operation
    b = CC.bounds(case, ref)
    errs = dict(mu=abs(stats[0] - ref['mu']), f=abs(stats[1] - ref['f']), grad=np.abs(stats[2:] - ref['grad']))
    print(name, {k: (np.asarray(errs[k]).tolist(), np.asarray(b[k]).tolist()) for k in errs})
    assert errs['mu'] <= b['mu'] and errs['f'] <= b['f'] and np.all(errs['grad'] <= b['grad']), (errs, b)
    # without the gradient: the same image and moments, zeros behind them
    iwe2, J2, stats2, dropped2 = _route(case, want_grad=False)
    assert np.array_equal(iwe2, iwe) and np.array_equal(stats2[:2].view(np.int64), stats[:2].view(np.int64)) and not stats2[2:].any()


def test_the_image_does_not_depend_on_the_order_of_the_stream():
    from evennicer_slam_amd import event_cmax as M
    case = _CASES['45x61_rot_k9']
    t, x, y, p = CC.stream(case)
    o = np.argsort(t, kind='stable')
    a = M.cmax_numpy(t, x, y, p, **CC.arguments(case))
    b = M.cmax_numpy(t[o], x[o], y[o], p[o], **CC.arguments(case))
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2][:2], b[2][:2]) and np.array_equal(a[3], b[3])
    assert np.all(np.abs(a[2][2:] - b[2][2:]) <= 2 * CC.bounds(case, CC.reference(case))['grad'])      # the event sum has an order


# ---- the gradient formula against autograd ---------------------------------------------------------------------------------
GRAD_CASES = ['1x300_k9_wider', '45x61_N257', '45x61_flow_k9', '45x61_rot_k9', 'planted_9x12', 'hand_5x7']


@pytest.mark.parametrize("name", GRAD_CASES)
def test_gradient_formula_against_autograd(name):
    case = _CASES[name]
    ref = CC.reference(case)
    kw = CC.arguments(case)
    # events exactly on the lattice sit on a kink of the bilinear vote, where autograd's one-sided choice is its own
    frac = np.stack([ref['xw'] - np.floor(ref['xw']), ref['yw'] - np.floor(ref['yw'])])[:, ref['voted']]
    if case['kind'] == 'random':
        assert np.all(frac > 0)
    theta = torch.tensor(kw['theta'], dtype=torch.float64, requires_grad=True)
    f = Y.cmax_torch(*CC.stream(case), **dict(kw, theta=theta))
    (g,) = torch.autograd.grad(f, theta)
    q = CC.quant_bounds(case, ref)
    b = CC.bounds(case, ref)
    assert abs(float(f.detach()) - ref['f']) <= q['f'] + b['f']
    if case['kind'] == 'random':
        assert np.all(np.abs(g.numpy() - ref['grad']) <= q['grad'] + b['grad']), (g.numpy(), ref['grad'], q['grad'])
        # ... and the bound (E_q puts every vote of the stream on one pixel, so it is a crude one) still separates a right
        # formula from a wrong one: under a hundredth of the gradient, and the wrong sign of one d w / d x' misses it
        assert np.all(q['grad'] + b['grad'] < 1e-2 * np.abs(ref['grad']).max())
        wrong = CC.reference(case, variant='dw_sign')['grad']
        assert np.abs(g.numpy() - wrong).max() > 10 * (q['grad'] + b['grad']).max()


@pytest.mark.parametrize("variant", ['dw_sign', 'one_pass', 'no_scale'])
def test_wrong_variants_leave_the_bound(variant):
    """the bound brackets: each wrong statement misses the route's gradient by more than a thousand bounds"""
    for name in ('45x61_flow_k9', '45x61_rot_k9'):
        case = _CASES[name]
        good, wrong = CC.reference(case), CC.reference(case, variant=variant)
        stats = _route(case)[2]
        b = CC.bounds(case, good)['grad']
        assert np.all(np.abs(stats[2:] - good['grad']) <= b)
        assert np.abs(stats[2:] - wrong['grad']).max() > 1000 * b.max(), (variant, name)


def test_central_differences_agree_with_the_gradient():
    from evennicer_slam_amd import event_cmax as M
    for name in ('45x61_flow_k9', '45x61_rot_k9'):
        case = _CASES[name]
        kw = CC.arguments(case)
        s = CC.stream(case)
        grad = M.cmax_numpy(*s, **kw)[2][2:]
        for k in range(len(kw['theta'])):
            # a step that moves the events by about 1e-4 pixels: far above the 2^-32 grain of the fixed-point votes (a smaller
            # step differentiates the rounding), far below the pixel lattice where the bilinear vote has its kinks
            h = 2e-3 if case['model'] == 'flow' else 2e-5
            up, dn = list(kw['theta']), list(kw['theta'])
            up[k] += h
            dn[k] -= h
            fd = (M.cmax_numpy(*s, **dict(kw, theta=up, want_grad=False))[2][1] - M.cmax_numpy(*s, **dict(kw, theta=dn, want_grad=False))[2][1]) / (2 * h)
            assert fd == pytest.approx(grad[k], rel=1e-4, abs=1e-9 * np.abs(grad).max()), (name, k)


# ---- recovery ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", ['flow', 'rotation'])
@pytest.mark.parametrize("seed", CC.REC_SEEDS)
def test_recovery_on_planted_streams(model, seed):
    from evennicer_slam_amd import event_cmax as M
    from evennicer_slam_amd.event_stream import EventStream
    s = CC.planted_stream(model, seed)
    taps = CC.taps_of(CC.REC_K)
    truth, zero = CC.REC_TRUTH[model], [0.0] * len(CC.REC_TRUTH[model])
    ykw = dict(H=CC.REC_H, W=CC.REC_W, calib=CC.REC_CALIB, model=model, t_ref=CC.REC_WINDOW / 2, taps=taps)
    f_true, f_zero = Y.cmax(*s, theta=truth, **ykw)['f'], Y.cmax(*s, theta=zero, **ykw)['f']
    assert len(s[0]) > 500 and f_true > f_zero                                          # the case's condition, on the yardstick
    stream = EventStream(*s)
    res = M.estimate_motion(stream, CC.REC_CALIB, model, H=CC.REC_H, W=CC.REC_W, sigma=CC.SIGMA, ksize=CC.REC_K, t_ref=CC.REC_WINDOW / 2)
    trace = res['trace']
    assert res['thetas'][0] == zero and len(trace) == len(res['thetas']) > 3 and trace[0] == pytest.approx(f_zero, rel=1e-12)
    assert all(b > a for a, b in zip(trace, trace[1:]))                                 # every accepted step raises f
    assert res['evals'] >= len(trace) and res['evals'] < 100
    f_hat = Y.cmax(*s, theta=res['theta'], **ykw)['f']
    assert f_hat == pytest.approx(trace[-1], rel=1e-12) and f_hat >= f_true
    print(model, seed, 'evals', res['evals'], 'errors', CC.component_errors(model, res['theta']), 'recorded', CC.REC_RECORD[(model, seed)])
    # default t_ref: the middle of the stream's own window
    assert M.default_t_ref(stream) == 0.5 * (float(s[0].min()) + float(s[0].max()))
    f, grad = M.contrast(stream, CC.REC_CALIB, model, res['theta'], CC.REC_H, CC.REC_W, t_ref=CC.REC_WINDOW / 2, ksize=CC.REC_K)
    assert f == trace[-1] and grad.shape == (len(truth),)


def test_warp_image_compensates():
    from evennicer_slam_amd import event_cmax as M
    from evennicer_slam_amd.event_stream import EventStream
    stream = EventStream(*CC.planted_stream('flow', 0))
    kw = dict(H=CC.REC_H, W=CC.REC_W, t_ref=0.05, ksize=CC.REC_K)
    raw, raw_b = M.warp_image(stream, CC.REC_CALIB, 'flow', [0.0, 0.0], **kw)
    comp, comp_b, dropped = M.warp_image(stream, CC.REC_CALIB, 'flow', CC.REC_TRUTH['flow'], with_dropped=True, **kw)
    assert raw.dtype == torch.float64 and tuple(raw.shape) == tuple(comp_b.shape) == (CC.REC_H, CC.REC_W)
    assert float(raw.sum()) == len(stream) and set(dropped) == set(M.DROPPED)           # on the lattice every vote is a whole unit
    assert float(comp_b.var(unbiased=False)) > 1.3 * float(raw_b.var(unbiased=False))   # sharper
    assert float(comp.max()) > float(raw.max())


# ---- relative_rotation ---------------------------------------------------------------------------------------------------------
def test_relative_rotation_against_a_matrix_exponential():
    from evennicer_slam_amd import event_cmax as M
    for omega, dt in (((0.3, -0.5, 0.8), 0.1), ((0.0, 0.0, 0.0), 1.0), ((2.0, 1.0, -3.0), 0.7), ((1e-9, 0.0, 0.0), 1e-6)):
        D = M.relative_rotation(omega, dt)
        w = torch.tensor([omega[0], -omega[1], -omega[2]], dtype=torch.float64) * dt    # y and z flip into the project's frame
        K = torch.tensor([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]], dtype=torch.float64)
        assert D.dtype == torch.float64 and tuple(D.shape) == (4, 4)
        assert torch.allclose(D[:3, :3], torch.linalg.matrix_exp(K), rtol=0, atol=1e-14)
        assert torch.equal(D[3], torch.tensor([0.0, 0.0, 0.0, 1.0], dtype=torch.float64)) and not D[:3, 3].any()
        back = M.angular_velocity(torch.eye(4, dtype=torch.float64), D, dt)
        assert np.allclose(back, omega, rtol=1e-9, atol=1e-12)


def test_relative_rotation_moves_pixels_the_way_the_warp_assumes():
    """A static point seen by a camera that turns by relative_rotation(omega, dt) moves in the image, to first order, by the
    rotation model's own flow: the signs and the frame conventions of the two agree."""
    from evennicer_slam_amd import event_cmax as M
    fx, fy, cx, cy = 80.0, 75.0, 30.0, 22.0
    omega, dt = (0.3, -0.5, 0.8), 1e-4
    D = M.relative_rotation(omega, dt).numpy()
    for px, py in ((10.0, 5.0), (30.0, 22.0), (55.0, 40.0)):
        u, v = (px - cx) / fx, (py - cy) / fy
        X = np.array([u, -v, -1.0, 1.0]) * 2.5                              # the project's camera looks down -z, y up
        X[3] = 1.0
        Xn = np.linalg.inv(D) @ X                                           # the point in the turned camera
        un, vn = Xn[0] / -Xn[2], -Xn[1] / -Xn[2]
        _, _, _, _, Bu, Bv = Y.warp('rotation', omega, (fx, fy, cx, cy), 0.0, 0.0, px, py)
        du, dv = sum(b * w for b, w in zip(Bu, omega)), sum(b * w for b, w in zip(Bv, omega))
        assert (un - u) / dt == pytest.approx(du, rel=1e-3, abs=1e-6) and (vn - v) / dt == pytest.approx(dv, rel=1e-3, abs=1e-6)


# ---- tools, ABI, refusals ------------------------------------------------------------------------------------------------------
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
    assert e.value.code == 0 and all(flag in text for flag in ('--stream', '--calib', '--stamps', '--demo', '--images', '--model {rotation,flow}'))
    for bad in ([], ['--stream', 'x.npz', '--demo', '3'], ['--stream', 'x.npz'], ['--demo', '1'], ['--demo', '3', '--images']):
        with pytest.raises(SystemExit) as e:
            tool.main(bad)
        assert e.value.code == 2, bad
    capsys.readouterr()
    # a stream file through the tool on the CPU route: two intervals of the planted flow
    s = EventStream(*CC.planted_stream('flow', 0))
    path, out_dir = str(tmp_path / 'events.npz'), str(tmp_path / 'out')
    s.save(path)
    stamps = tmp_path / 'stamps.txt'
    stamps.write_text("0.0\n0.05\n0.1\n")
    out = tool.main(['--stream', path, '--size', str(CC.REC_H), str(CC.REC_W), '--calib'] + [repr(v) for v in CC.REC_CALIB] +
                    ['--stamps', str(stamps), '--model', 'flow', '--device', 'cpu', '--out', out_dir, '--images'])
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert line['intervals'] == 2 and len(out['rows']) == 2 and sum(r['events'] for r in out['rows']) == len(s)
    for r in out['rows']:
        assert r['contrast_after'] > r['contrast_before'] and r['steps'] >= 1 and r['theta'][0] > 0 > r['theta'][1]
    assert sorted(os.listdir(out_dir)) == ['interval00000_compensated.png', 'interval00000_raw.png', 'interval00001_compensated.png',
                                           'interval00001_raw.png', 'theta.json']
    bench = open(os.path.join(ROOT, "tools", "bench_event_cmax.py")).read()
    assert all(re.search(r"add_argument\('%s'" % f, bench) for f in ('--repeat', '--estimate-repeat', '--no-numpy'))
    assert 'vote_atomic_gbytes_per_s' in bench and 'device_below_numpy' in bench


def test_abi_exports():
    import evennicer_slam_amd as E
    header = open(os.path.join(ROOT, "include", "enslam_hip.h")).read()
    handle = E._lib.lib()
    for name in EXPORTS:
        assert name in E._lib.EXPORTS and re.search(r"\b%s\s*\(" % name, header) and hasattr(handle, name), name
    from evennicer_slam_amd import functional as EF
    for macro, value in (('ENSLAM_CMAX_FLOW', EF.EVENT_CMAX_MODELS['flow'][0]), ('ENSLAM_CMAX_ROTATION', EF.EVENT_CMAX_MODELS['rotation'][0]),
                         ('ENSLAM_CMAX_MAX_KSIZE', EF.EVENT_CMAX_MAX_KSIZE)):
        assert re.search(r"#define %s %d\b" % (macro, value), header), macro


def check_refusals(t, x, y, p, N, H, W, ws, ws_bytes, iwe, blurred, stats, dropped):
    """Every refusal of enslam_event_cmax_eval returns its code; nothing is launched (the GPU test looks at the buffers).  The
    pointers only have to be non-NULL and 8-byte aligned: a refusal comes before any of them is used."""
    from evennicer_slam_amd import _lib as L
    lib = L.lib()
    EINVAL, EUNSUPPORTED = -1, -3
    nan, inf = float('nan'), float('inf')

    def call(n=N, hh=H, ww=W, cal=(80.0, 80.0, 3.0, 2.0), model=1, theta=(0.1, 0.2, 0.3), t_ref=0.0, k=3, taps=None, ptrs=None,
             nbytes=ws_bytes):
        q = dict(t=t, x=x, y=y, p=p, ws=ws, iwe=iwe, blurred=blurred, stats=stats, dropped=dropped, theta=(ctypes.c_double * 3)(*theta),
                 taps=(ctypes.c_double * 64)(*(taps or [1.0 / max(k, 1)] * max(k, 1))))
        q.update(ptrs or {})
        return lib.enslam_event_cmax_eval(q['t'], q['x'], q['y'], q['p'], n, hh, ww, cal[0], cal[1], cal[2], cal[3], model, q['theta'],
                                          t_ref, 0, k, q['taps'], q['ws'], nbytes, q['iwe'], q['blurred'], q['stats'], q['dropped'], 1, None)

    for name in ('t', 'x', 'y', 'p', 'ws', 'iwe', 'stats', 'dropped', 'theta', 'taps'):
        assert call(ptrs={name: None}) == EINVAL, name
    assert call(n=-1) == EINVAL and call(hh=0) == EINVAL and call(ww=-3) == EINVAL
    for bad in (nan, inf, -inf):
        assert call(theta=(0.1, bad, 0.3)) == EINVAL and call(t_ref=bad) == EINVAL and call(taps=[0.25, bad, 0.25]) == EINVAL
        for i in range(4):
            cal = [80.0, 80.0, 3.0, 2.0]
            cal[i] = bad
            assert call(cal=cal) == EINVAL
    assert call(cal=(0.0, 80.0, 3.0, 2.0)) == EINVAL and call(cal=(80.0, -0.0, 3.0, 2.0)) == EINVAL
    assert call(model=2) == EINVAL and call(model=-1) == EINVAL
    assert call(k=0) == EINVAL and call(k=4) == EINVAL and call(k=-3) == EINVAL and call(k=32) == EINVAL
    assert call(k=33) == EUNSUPPORTED
    need = ctypes.c_int64(-1)
    assert lib.enslam_event_cmax_workspace(H, W, N, 3, ctypes.byref(need)) == 0 and 0 < need.value <= ws_bytes
    assert call(nbytes=need.value - 8) == EINVAL and call(nbytes=0) == EINVAL and call(nbytes=-need.value) == EINVAL
    for name, base in (('ws', ws), ('iwe', iwe), ('blurred', blurred), ('stats', stats), ('dropped', dropped)):
        assert call(ptrs={name: base + 4}) == EINVAL, name
    assert call(n=1 << 31) == EUNSUPPORTED and call(hh=65537) == EUNSUPPORTED and call(ww=65537) == EUNSUPPORTED
    assert call(hh=65536, ww=8192) == EUNSUPPORTED                                     # more than 2^28 pixels
    n = ctypes.c_int64(-1)
    assert lib.enslam_event_cmax_workspace(H, W, N, 3, None) == EINVAL
    for args, code in (((0, W, N, 3), EINVAL), ((H, W, -1, 3), EINVAL), ((H, W, N, 1), EINVAL), ((H, W, N, 4), EINVAL),
                       ((H, W, 1 << 31, 3), EUNSUPPORTED), ((65537, 1, N, 2), EUNSUPPORTED), ((32768, 16384, N, 2), EUNSUPPORTED)):
        assert lib.enslam_event_cmax_workspace(*args, ctypes.byref(n)) == code and n.value == -1, args
    # three float64 images and the widest first level of partials: ceil(H W / 256) pixel blocks against ceil(N / 256) P
    assert lib.enslam_event_cmax_workspace(45, 61, 700, 3, ctypes.byref(n)) == 0 and n.value == (3 * 2745 + 11) * 8
    assert lib.enslam_event_cmax_workspace(5, 7, 20000, 3, ctypes.byref(n)) == 0 and n.value == (3 * 35 + 79 * 3) * 8


def test_every_refusal_has_its_code_and_its_error_class():
    from evennicer_slam_amd import _lib as L
    from evennicer_slam_amd import event_cmax as M
    from evennicer_slam_amd import functional as EF
    host = (ctypes.c_double * 8192)()
    a = ctypes.addressof(host)
    assert a % 8 == 0
    check_refusals(a, a, a, a, 10, 5, 7, a, 8192 * 8, a, a, a, a)
    s = CC.stream(_CASES['hand_5x7'])
    ok = dict(H=5, W=7, calib=(2.0, 2.0, 3.0, 2.0), model='flow', theta=[4.0, -2.0], t_ref=0.0, taps=[1.0])
    for bad in (dict(model='affine'), dict(theta=[1.0]), dict(theta=[1.0, float('nan')]), dict(calib=(0.0, 2.0, 3.0, 2.0)),
                dict(taps=[0.5, 0.5]), dict(taps=[1.0 / 33] * 33), dict(H=0), dict(W=70000), dict(t_ref=float('inf'))):
        with pytest.raises(L.EnslamError):
            M.cmax_numpy(*s, **dict(ok, **bad))
    for sigma, k in ((1.5, 4), (1.5, 33), (1.5, -1)):
        with pytest.raises(L.EnslamError):
            M.blur_taps(sigma, k)
    assert M.blur_taps(1.5) == CC.taps_of(9) and len(M.blur_taps(1.5)) == 9 and M.blur_taps(0.0) == [1.0] and M.blur_taps(1.5, 1) == [1.0]
    with pytest.raises(L.EnslamError):                                  # the device entry point takes device tensors only
        EF.event_cmax_eval(*(torch.from_numpy(v) for v in s), 5, 7, ok['calib'], 'flow', ok['theta'], 0.0, [1.0])
