"""No GPU: the event-generation-model loss (event_model.py) -- hand-worked pixels and a hand-worked reflect adjoint, the float64
yardstick tests/event_model_numpy.py against float64 torch autograd of the torch statement, the bracket on the derived tolerance
(the float32 torch statement stays inside it on every case; three deliberately wrong variants leave it by a factor 10 and more
on the border cases), the conditions of tests/event_model_cases.py, fit_thresholds, the tracker's `predictor: 'model'` route on
CPU tensors, the tools' flags, the ABI export list and every refusal's error class."""
import ctypes
import inspect
import math
import os
import re
import types

import numpy as np
import pytest
import torch

from tests import event_model_cases as MC
from tests import event_model_numpy as Y
from tests.util import load

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPORTS = ("enslam_event_model_workspace", "enslam_event_model_loss")
_CASES = {c['name']: c for c in MC.CASES}
_NAMES = [c['name'] for c in MC.CASES]
_REF = {}


def _reference(name):
    if name not in _REF:
        _REF[name] = MC.reference(_CASES[name])
    return _REF[name]


def _torch_route(case, dtype):
    from evennicer_slam_amd import event_model as M
    cur, prev, gt = (torch.from_numpy(a).to(dtype) for a in MC.inputs(case))
    cur.requires_grad_(True)
    loss, pred, terms, gts, preds = M.event_model_loss_torch(cur, prev, gt, case['c_neg'], case['c_pos'], case['eps'], True,
                                                             case['ksizes'], case['weights'], unblurred_weight=1.0)
    loss.backward()
    n = lambda t: t.detach().double().numpy()
    return dict(loss=float(loss.detach()), pred=n(pred), terms=np.array([float(t.detach()) for t in terms]), grad=n(cur.grad),
                blur_gt=[n(g) for g in gts], blur_pred=[n(p) for p in preds])


# ------------------------------------------------------------------------------------------------
# by hand
# ------------------------------------------------------------------------------------------------
def test_hand_worked_pixels():
    """grey pixels (Y = the grey level up to rounding): one per polarity, one tie, one clamped; K = 0"""
    from evennicer_slam_amd import event_model as M
    eps, c_neg, c_pos = 1e-3, 0.25, 0.1
    grey = lambda v: (v, v, v)
    prev = np.array([[grey(0.2), grey(0.5), grey(0.4), grey(0.3)]])
    cur = np.array([[grey(0.5), grey(0.2), grey(0.4), grey(-0.1)]])
    gt = np.array([[(0.0, 9.0), (3.0, 0.0), (1.0, 2.0), (20.0, 0.0)]])
    d_up, d_down, d_clamp = math.log(0.501 / 0.201), math.log(0.201 / 0.501), math.log(0.001 / 0.301)
    want_pred = np.array([[(0.0, d_up / c_pos), (-d_down / c_neg, 0.0), (0.0, 0.0), (-d_clamp / c_neg, 0.0)]])
    want_r = want_pred - gt
    want_loss = float((want_r ** 2).sum())
    # dloss/dcur_ch = 2 r (+-) w_ch / (c (Y + eps)); the tie and the clamped pixel carry none
    want_g = np.zeros((1, 4, 3))
    want_g[0, 0] = 2 * want_r[0, 0, 1] / (c_pos * 0.501) * np.array(Y.LUMA)
    want_g[0, 1] = -2 * want_r[0, 1, 0] / (c_neg * 0.201) * np.array(Y.LUMA)
    ref = Y.event_model(cur, prev, gt, c_neg, c_pos, eps)
    assert np.allclose(ref['pred'], want_pred, rtol=1e-13, atol=0) and ref['loss'] == pytest.approx(want_loss, rel=1e-13)
    assert np.allclose(ref['grad'], want_g, rtol=1e-12, atol=0)
    assert np.all(ref['grad'][0, 2:] == 0) and np.all(ref['pred'][0, 2] == 0) and list(ref['branch'][0]) == [1, -1, 0, -1]
    ct = torch.tensor(cur, requires_grad=True)
    loss, pred, terms, gts, preds = M.event_model_loss(ct, torch.tensor(prev), torch.tensor(gt), c_neg, c_pos, eps, blur=False,
                                                       unblurred_weight=0.5)
    loss.backward()
    assert np.allclose(pred.numpy(), want_pred, rtol=1e-13, atol=0) and float(loss.detach()) == pytest.approx(want_loss, rel=1e-13)
    assert np.allclose(ct.grad.numpy(), want_g, rtol=1e-12, atol=0) and np.all(ct.grad.numpy()[0, 2:] == 0)
    assert len(terms) == 1 and float(terms[0]) == pytest.approx(0.5 * want_loss, rel=1e-13) and gts == [] and preds == []


def test_hand_worked_reflect_adjoint():
    """n = 4, taps (a, b, a): B reads pixel 1 twice for output 0 (directly and through the reflection of -1), so column 1 of B
    -- row 1 of B^T -- holds 2a where B's own row 1 holds a"""
    a, b = 0.25, 0.5
    taps = np.array([a, b, a])
    B = np.array([[b, 2 * a, 0, 0], [a, b, a, 0], [0, a, b, a], [0, 0, 2 * a, b]])
    eye = np.eye(4)
    got_B = np.stack([Y.blur_axis(eye[:, j], taps, 0) for j in range(4)], axis=1)
    got_BT = np.stack([Y.blur_axis_adjoint(eye[:, j], taps, 0) for j in range(4)], axis=1)
    assert np.array_equal(got_B, B) and np.array_equal(got_BT, B.T) and not np.array_equal(B, B.T)
    v = np.array([1.0, 2.0, 4.0, 8.0])
    assert np.array_equal(Y.blur_axis_adjoint(v, taps, 0), [b * 1 + a * 2, 2 * a * 1 + b * 2 + a * 4, a * 2 + b * 4 + 2 * a * 8, a * 4 + b * 8])
    # two dimensions: <B x, y> = <x, B^T y>
    rng = np.random.default_rng(0)
    x, y = rng.standard_normal((5, 7, 2)), rng.standard_normal((5, 7, 2))
    t9 = Y.gaussian_taps(9)
    assert float((Y.blur(x, t9) * y).sum()) == pytest.approx(float((x * Y.blur_adjoint(y, t9)).sum()), rel=1e-12)


def test_taps_are_the_projects():
    from evennicer_slam_amd import functional as EF
    from evennicer_slam_amd.event import gaussian_kernel1d
    for k in (3, 9, 31):
        assert np.allclose(Y.gaussian_taps(k), gaussian_kernel1d(k, dtype=torch.float64).numpy(), rtol=1e-14, atol=0)
    K, ksizes, weights, taps = EF.event_model_kernels((9, 5), (1.0, 0.5))
    assert K == 2 and list(ksizes) == [9, 5] and list(weights) == [1.0, 0.5]
    for i, k in enumerate((9, 5)):
        row = np.array(taps[i * EF.EVENT_MODEL_MAX_KSIZE:(i + 1) * EF.EVENT_MODEL_MAX_KSIZE])
        assert np.array_equal(row[:k], gaussian_kernel1d(k).numpy()) and np.all(row[k:] == 0)
    assert (EF.EVENT_MODEL_TILE, EF.EVENT_MODEL_MAX_KERNELS, EF.EVENT_MODEL_MAX_KSIZE) == (MC.TILE, MC.MAX_KERNELS, MC.MAX_KSIZE)
    header = open(os.path.join(ROOT, "include", "enslam_hip.h")).read()
    for name, val in (('TILE', MC.TILE), ('MAX_KERNELS', MC.MAX_KERNELS), ('MAX_KSIZE', MC.MAX_KSIZE)):
        assert re.search(r"#define ENSLAM_EVENT_MODEL_%s %d\b" % (name, val), header)


# ------------------------------------------------------------------------------------------------
# the yardstick, the cases and the tolerance
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", _NAMES)
def test_yardstick_equals_float64_autograd(name):
    case, ref = _CASES[name], _reference(name)
    got = _torch_route(case, torch.float64)
    assert got['loss'] == pytest.approx(ref['loss'], rel=1e-12)
    assert np.allclose(got['terms'], ref['terms'], rtol=1e-12, atol=0)
    assert np.allclose(got['pred'], ref['pred'], rtol=1e-12, atol=1e-300)
    assert np.abs(got['grad'] - ref['grad']).max() <= 1e-11 * np.abs(ref['grad']).max()
    for a, b in zip(got['blur_gt'] + got['blur_pred'], ref['blur_gt'] + ref['blur_pred']):
        assert np.abs(a - b).max() <= 1e-12 * np.abs(b).max()


@pytest.mark.parametrize("name", _NAMES)
def test_case_conditions(name):
    case, ref = _CASES[name], _reference(name)
    assert all(k % 2 == 1 and k // 2 < min(case['h'], case['w']) and k <= MC.MAX_KSIZE for k in case['ksizes'])
    assert len(case['ksizes']) == len(case['weights']) <= MC.MAX_KERNELS and max(case['h'], case['w']) <= 300
    assert case['h'] * case['w'] <= 39 * 51 or case['h'] == 5
    near = np.abs(ref['d']) <= MC.branch_margin(case['eps'])
    if case['kind'] == 'tie':
        assert np.all(ref['d'][MC.TIE_BLOCK] == 0) and np.all(ref['grad'][MC.TIE_BLOCK] == 0)
        near[MC.TIE_BLOCK] = False                               # (an exact 0 is a decision every route makes alike)
    assert near.mean() <= MC.MAX_BRANCH_SHARE
    if case['kind'] == 'negative':
        cur = MC.inputs(case)[0]
        assert Y.luma_raw(cur)[2, 3] < 0 and np.all(ref['grad'][2, 3] == 0) and ref['pred'][2, 3, 0] > 0
    if case['kind'] == 'dark':
        assert Y.luma_raw(MC.inputs(case)[0]).max() < 5 * case['eps']
    assert (ref['branch'] > 0).any() and (ref['branch'] < 0).any()
    # the derived tolerance has room under a tenth of the smallest displacement a wrong adjoint causes (4 % of max|dloss/dr|)
    b = MC.bounds(case, ref)
    assert MC.fraction(b['g_r'], ref['g_r']) < 4e-3 and MC.fraction(b['pred'], ref['pred']) < 1e-4


def test_case_list_covers_what_it_has_to():
    shapes = {(c['h'], c['w']) for c in MC.CASES}
    T = MC.TILE
    assert {(5, 5), (5, 7), (5, 300), (39, 51)} <= shapes
    for n in (T - 1, T, T + 1, 2 * T + 1):
        assert any(h == n for h, _ in shapes) and any(w == n for _, w in shapes)
    assert {len(c['ksizes']) for c in MC.CASES} >= {0, 1, 2}
    assert any(c['c_neg'] != c['c_pos'] for c in MC.CASES) and {c['kind'] for c in MC.CASES} == {'plain', 'dark', 'tie', 'negative'}
    assert any(c['ksizes'] == (9,) and c['weights'] == (1.0,) for c in MC.CASES)
    assert any(len(set(c['ksizes'])) == 2 and len(set(c['weights'])) == 2 for c in MC.CASES)


def _errors(case, got, ref):
    """max |got - ref| per quantity, each with its bound"""
    b = MC.bounds(case, ref)
    out = {'pred': (np.abs(got['pred'] - ref['pred']).max(), b['pred']), 'loss': (abs(got['loss'] - ref['loss']), b['loss']),
           'grad': (np.abs(got['grad'] - ref['grad']).max(), b['grad'])}
    for j, (t, e) in enumerate(zip(ref['terms'], b['terms'])):
        out[f'term{j}'] = (abs(got['terms'][j] - t), e)
    for i in range(len(case['ksizes'])):
        for key in ('blur_gt', 'blur_pred'):
            if key in got:
                out[f'{key}{i}'] = (np.abs(got[key][i] - ref[key][i]).max(), b[key][i])
    return out


@pytest.mark.parametrize("name", _NAMES)
def test_float32_torch_statement_is_inside_the_tolerance(name):
    case, ref64 = _CASES[name], _reference(name)
    got = _torch_route(case, torch.float32)
    branch = np.where(got['pred'][..., 1] > 0, 1, np.where(got['pred'][..., 0] > 0, -1, 0))
    differ = branch != ref64['branch']
    assert np.all(np.abs(ref64['d'][differ]) <= MC.branch_margin(case['eps'])) and differ.mean() <= MC.MAX_BRANCH_SHARE
    ref = MC.reference(case, branch=branch) if differ.any() else ref64
    errs = _errors(case, got, ref)
    print(name, {k: '%.2e / %.2e' % (MC.fraction(e, 1.0), MC.fraction(bd, 1.0)) for k, (e, bd) in errs.items()})
    for k, (e, bd) in errs.items():
        assert e <= bd, (k, e, bd)


@pytest.mark.parametrize("name", MC.BORDER_CASES + ('39x51_k9',))
@pytest.mark.parametrize("variant", ['B_for_BT', 'zero_pad', 'blur_pred_only'])
def test_wrong_variants_leave_the_tolerance(name, variant):
    case, ref = _CASES[name], _reference(name)
    wrong = MC.reference(case, variant=variant)
    wrong = dict(wrong, terms=np.asarray(wrong['terms']))
    errs = _errors(case, {k: wrong[k] for k in ('pred', 'loss', 'grad', 'terms')}, ref)
    factor = 10.0
    assert errs['grad'][0] >= factor * errs['grad'][1], errs['grad']
    moved = float(np.abs(wrong['g_r'] - ref['g_r']).max() / np.abs(ref['g_r']).max())
    print(name, variant, 'dloss/dr moved by %.1f %% of its maximum; grad error / bound = %.0f' % (100 * moved, errs['grad'][0] / errs['grad'][1]))
    if variant == 'B_for_BT':
        assert errs['loss'][0] == 0 and moved >= (0.10 if name in MC.BORDER_CASES else 0.03)        # only the gradient is wrong
    else:
        assert errs['loss'][0] >= factor * errs['loss'][1] and errs['term1'][0] >= factor * errs['term1'][1]


# ------------------------------------------------------------------------------------------------
# thresholds
# ------------------------------------------------------------------------------------------------
def test_fit_thresholds_recovers_unquantised_counts():
    from evennicer_slam_amd import event_model as M
    rng = np.random.default_rng(5)
    pairs = []
    for _ in range(3):
        prev, cur = (torch.from_numpy(rng.random((12, 17, 3))) for _ in range(2))
        pairs.append((prev, cur, M.predict_events(cur, prev, c_neg=0.31, c_pos=0.17, eps=1e-3)))
    fit = M.fit_thresholds(pairs, eps=1e-3)
    assert abs(fit['c_pos'] - 0.17) <= 1e-12 and abs(fit['c_neg'] - 0.31) <= 1e-12 and fit['n_pos'] + fit['n_neg'] == 3 * 12 * 17
    flat = torch.full((4, 4, 3), 0.5, dtype=torch.float64)
    assert M.fit_thresholds([(flat, flat, torch.zeros(4, 4, 2))]) == dict(c_pos=None, c_neg=None, n_pos=0, n_neg=0)


# ------------------------------------------------------------------------------------------------
# the tracker's route (the renderer has no CPU form: the rescaled render is a differentiable stand-in on the CPU)
# ------------------------------------------------------------------------------------------------
class model_tracker_setup:
    """TrackerIteration with `predictor: 'model'` and NO event_net on the images of tests/golden/tiny_event_iter.npz.  On a HIP
    device the tiny golden scene is rendered; on the CPU `_render_rescaled` is replaced by a smooth function of the camera
    tensor and only the event term runs."""

    def __init__(self, device, blur=True, activate=True):
        import evennicer_slam_amd as E
        fx = self.fx = load("tiny_event_iter")
        self.device, self.on_gpu = device, device != 'cpu'
        H, W, fxx, fy, cx, cy = [float(x) for x in fx['cam']]
        cfg = {'tracking': {'device': device, 'w_color_loss': float(fx['w_color_loss']), 'ignore_edge_W': int(fx['edge'][1]),
                            'ignore_edge_H': int(fx['edge'][0]), 'handle_dynamic': True, 'use_color_in_tracking': True},
               'event': {'activate_events': activate, 'blur': blur, 'kernel_sizes': [9], 'kernel_weights': [1.0], 'unblurred_weight': 0.0,
                         'balancer': float(fx['balancer']), 'predictor': 'model', 'c_pos': 0.15, 'c_neg': 0.25}}
        renderer, bound, grids, model = None, None, None, None
        if self.on_gpu:
            from tests.hip_util import cfg_like, tiny_on_gpu
            _s, bound, model, grids, _rays, renderer = tiny_on_gpu()
            for p in model.parameters():
                p.requires_grad_(False)
            cfg = dict(cfg_like(), **cfg)
        slam = types.SimpleNamespace(nice=True, bound=bound, renderer=renderer, event_net=None, H=int(H), W=int(W), fx=fxx, fy=fy,
                                     cx=cx, cy=cy, low_gpu_mem=False)
        self.trk = E.tracker.TrackerIteration(cfg, None, slam)
        self.trk.c, self.trk.decoders = grids, model
        self.img = {k: torch.from_numpy(fx[k]).to(device) for k in ('gt_depth', 'gt_color', 'pre_gt_color', 'gt_event', 'gt_mask')}
        self.sf = float(fx['scale_factor'])
        if not self.on_gpu:
            base = torch.from_numpy(fx['full_color_current'])
            self.trk._render_rescaled = lambda ct, gd, sf: base * (1.0 + 0.2 * ct[4]) + 0.05 * ct[5] * ct[0]

    def camera(self):
        return torch.from_numpy(self.fx['camera_tensor']).to(self.device).clone().requires_grad_(True)

    def frames(self, n):
        """n frames' (gt_color, gt_depth, gt_event, gt_mask, pre_gt_color): the fixture's, then variations of it"""
        i = self.img
        out = [(i['gt_color'], i['gt_depth'], i['gt_event'], i['gt_mask'], i['pre_gt_color'])]
        for k in range(1, n):
            out.append((i['gt_color'].flip(1).contiguous(), i['gt_depth'].flip(1).contiguous(), (i['gt_event'] + k).flip(0).contiguous(),
                        i['gt_mask'], (i['pre_gt_color'] * 0.8).contiguous()))
        return out

    def run(self, mode, frames=2, iters=2):
        """[dict(rgbd, event, camera)] per iteration: 'eager' = iteration_losses(static_shapes=True) + backward + FusedAdam,
        'graph' = GraphedCameraIteration replays; both restart camera and optimiser per frame and use the fixture's pixel draw"""
        import evennicer_slam_amd as E
        from evennicer_slam_amd import functional as EF
        from evennicer_slam_amd.mapper import FusedAdam
        trk, n = self.trk, int(self.fx['batch_size'])
        idx = torch.from_numpy(self.fx['idx']).to(self.device)
        ct = self.camera()
        init = ct.detach().clone()
        opt = FusedAdam([ct], lr=2e-3)
        fr = self.frames(frames)
        real_randint, out = torch.randint, []
        torch.randint = lambda *a, **k: idx
        try:
            git = None
            if mode == 'graph':
                git = E.tracker.GraphedCameraIteration(trk, ct, opt, fr[0][0], fr[0][1], fr[0][2], fr[0][3], fr[0][4], batch_size=n,
                                                       rgbd=True, event=True, scale_factor=self.sf, n_draws=iters)
            for f in fr:
                with torch.no_grad():
                    ct.copy_(init)
                opt.reset()
                if git is not None:
                    git.set_frame(*f)
                else:
                    frame = trk.prepare_event_frame(f[2], f[3], f[4], self.sf)
                for _ in range(iters):
                    if git is not None:
                        l_rgbd, l_event, l_mask = git.step()
                        assert float(l_mask) == 0.0
                    else:
                        opt.zero_grad()
                        o = trk.iteration_losses(ct, f[0], f[1], frame, n, True, True, self.sf, static_shapes=True)
                        assert o['mask'] is None and o['event_mask'] is None and o['gts_blurred'] == [] and o['full_event'] is not None
                        with EF.engine_on_calling_thread():
                            o['total'].backward()
                        opt.step()
                        l_rgbd, l_event = o['rgbd'].detach(), o['event'].detach()
                        del o
                    out.append(dict(rgbd=float(l_rgbd), event=float(l_event), camera=ct.detach().cpu().numpy().copy()))
        finally:
            torch.randint = real_randint
        return out


class _SgdOnce:
    def __init__(self, p):
        self.p, self.grad = p, None

    def zero_grad(self):
        self.p.grad = None

    def step(self):
        self.grad = None if self.p.grad is None else self.p.grad.detach().clone()


@pytest.mark.parametrize("blur", [True, False])
def test_tracker_model_route_on_cpu(blur):
    from evennicer_slam_amd import event_model as M
    s = model_tracker_setup('cpu', blur=blur)
    trk, img, fx = s.trk, s.img, s.fx
    assert trk.event_net is None and trk.event_predictor == 'model' and (trk.event_c_pos, trk.event_c_neg, trk.event_eps) == (0.15, 0.25, 1e-3)
    ct = s.camera()
    frame = trk.prepare_event_frame(img['gt_event'], img['gt_mask'], img['pre_gt_color'], s.sf)
    o = trk.iteration_losses(ct, img['gt_color'], img['gt_depth'], frame, 80, rgbd=False, event=True, scale_factor=s.sf)
    h, w = fx['gt_event_s'].shape[:2]
    assert o['mask'] is None and o['event_mask'] is None and o['rgbd'] is None and o['total'] is o['event']
    assert tuple(o['full_event'].shape) == (h, w, 2) and len(o['terms']) == (2 if blur else 1)
    assert len(o['gts_blurred']) == len(o['preds_blurred']) == (1 if blur else 0)
    want = M.event_model_loss_torch(trk._render_rescaled(ct, None, s.sf), frame[2], frame[0], 0.25, 0.15, 1e-3, blur, (9,), (1.0,))
    assert float(o["event"].detach()) == pytest.approx(float(want[0].detach()) * float(fx['balancer']), rel=1e-6)
    assert torch.allclose(o['full_event'], want[1].detach()) and (not blur or torch.allclose(o['preds_blurred'][0], want[4][0]))
    g_want, = torch.autograd.grad(want[0] * float(fx['balancer']), ct)
    opt = _SgdOnce(ct)
    ret = trk.optimize_cam_in_batch(ct, None, img['gt_color'], img['gt_depth'], img['gt_event'], img['gt_mask'], 80, opt, 0, 0,
                                    img['pre_gt_color'], rgbd=False, event=True, scale_factor=s.sf)
    assert len(ret) == (10 if blur else 7)
    assert ret[0] is None and ret[1] == pytest.approx(float(o["event"].detach()), rel=1e-6) and ret[2] is None and ret[-1] is None
    assert tuple(ret[3].shape) == tuple(ret[4].shape) == (h, w, 2) and tuple(ret[-2].shape) == (h, w, 1)
    if blur:
        assert len(ret[5]) == len(ret[6]) == 1 and tuple(ret[5][0].shape) == (h, w, 2) and len(ret[7]) == 2 and ret[7][0] == 0.0
    assert torch.allclose(opt.grad, g_want, rtol=1e-4, atol=1e-7) and float(opt.grad.abs().max()) > 0
    # activate_events off: reported, not back-propagated
    s2 = model_tracker_setup('cpu', blur=blur, activate=False)
    o2 = s2.trk.iteration_losses(s2.camera(), img['gt_color'], img['gt_depth'], frame, 80, rgbd=False, event=True, scale_factor=s.sf)
    assert o2['total'] is None and float(o2["event"].detach()) == pytest.approx(float(o["event"].detach()), rel=1e-6)


def test_predictor_key_and_harness_switch():
    import evennicer_slam_amd as E
    from evennicer_slam_amd.slam import SLAM
    s = model_tracker_setup('cpu')
    cfg = {'tracking': s.trk.cfg['tracking'], 'event': dict(s.trk.cfg['event'], predictor='oracle')}
    slam = types.SimpleNamespace(bound=None, renderer=None, H=48, W=64, fx=1.0, fy=1.0, cx=0.0, cy=0.0)
    with pytest.raises(ValueError):
        E.tracker.TrackerIteration(cfg, None, slam)
    cfg['event'].pop('predictor')
    trk = E.tracker.TrackerIteration(cfg, None, slam)                # the default: the network route, which needs a network
    assert trk.event_predictor == 'net'
    with pytest.raises(RuntimeError):
        trk.iteration_losses(s.camera(), None, None, (None, None, None), 80, rgbd=False, event=True)
    src = inspect.getsource(SLAM.track)
    assert "predictor" in src and "'model'" in src


# ------------------------------------------------------------------------------------------------
# tools, ABI
# ------------------------------------------------------------------------------------------------
def test_tools_take_the_new_flags(capsys):
    import importlib.util

    def module(name):
        spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        return mod

    run_slam = module("run_slam")
    with pytest.raises(SystemExit) as e:
        run_slam.main(['--help'])
    assert e.value.code == 0 and '--event-predictor {net,model}' in capsys.readouterr().out
    with pytest.raises(SystemExit) as e:
        run_slam.main(['cfg.yaml', '--event-predictor', 'oracle'])
    assert e.value.code == 2
    synth = module("run_synthetic_slam")
    params = inspect.signature(synth.run).parameters
    assert all(k in params and params[k].default is None for k in ('event_predictor', 'c_pos', 'c_neg'))
    text = open(os.path.join(ROOT, "tools", "run_synthetic_slam.py")).read()
    assert all(flag in text for flag in ("'--event-predictor'", "'--c-pos'", "'--c-neg'"))
    bench_text = open(os.path.join(ROOT, "tools", "bench_event_iter.py")).read()
    assert re.search(r"add_argument\('--predictor', choices=\('net', 'model'\), default='net'", bench_text)
    fit = module("fit_event_thresholds")
    with pytest.raises(SystemExit) as e:
        fit.main(['--help'])
    assert e.value.code == 0


def test_abi_exports():
    import evennicer_slam_amd as E
    header = open(os.path.join(ROOT, "include", "enslam_hip.h")).read()
    handle = E._lib.lib()
    for name in EXPORTS:
        assert name in E._lib.EXPORTS and re.search(r"\b%s\s*\(" % name, header) and hasattr(handle, name), name


def check_refusals(cur, prev, gt, h, w, ws, ws_bytes, pred, sums, grad):
    """Every refusal of enslam_event_model_loss returns its code; nothing is launched (the GPU test looks at the buffers).  The
    pointers only have to be non-NULL: a refusal comes before any of them is used."""
    from evennicer_slam_amd import _lib as L
    from evennicer_slam_amd import functional as EF
    lib = L.lib()
    EINVAL, EUNSUPPORTED = -1, -3
    taps = (ctypes.c_float * (8 * EF.EVENT_MODEL_MAX_KSIZE))()
    wts = (ctypes.c_float * 8)(*([1.0] * 8))

    def call(ks=(3,), c_neg=0.2, c_pos=0.2, eps=1e-3, hh=h, ww=w, ptrs=None, nbytes=ws_bytes, blur=(None, None), kptr=True):
        p = dict(cur=cur, prev=prev, gt=gt, ws=ws, pred=pred, sums=sums, grad=grad)
        p.update(ptrs or {})
        ksz = (ctypes.c_int32 * 8)(*(list(ks) + [3] * (8 - len(ks))))
        return lib.enslam_event_model_loss(p['cur'], p['prev'], p['gt'], hh, ww, c_neg, c_pos, eps, len(ks), ksz if kptr else None,
                                           wts if kptr else None, taps if kptr else None, p['ws'], nbytes, p['pred'], p['sums'],
                                           p['grad'], blur[0], blur[1], None)

    assert call(ks=(4,)) == EINVAL and call(ks=(3, 0)) == EINVAL and call(ks=(-3,)) == EINVAL                 # even / non-positive k
    assert call(ks=(EF.EVENT_MODEL_MAX_KSIZE + 2,), hh=64, ww=64) == EUNSUPPORTED                             # k above the maximum
    assert call(ks=(2 * min(h, w) + 1,)) == EINVAL and call(ks=(2 * min(h, w) - 1,), nbytes=0) == EINVAL      # reflect range (then ws)
    assert call(ks=(3,) * (EF.EVENT_MODEL_MAX_KERNELS + 1)) == EUNSUPPORTED                                   # K above the maximum
    for bad in (0.0, -0.2, float('nan')):
        assert call(c_neg=bad) == EINVAL and call(c_pos=bad) == EINVAL and call(eps=bad) == EINVAL
    for name in ('cur', 'prev', 'gt', 'ws', 'pred', 'sums', 'grad'):
        assert call(ptrs={name: None}) == EINVAL, name
    assert call(kptr=False) == EINVAL and call(blur=(pred, None)) == EINVAL and call(blur=(None, pred)) == EINVAL
    assert call(hh=0) == EINVAL and call(ww=-1) == EINVAL and call(nbytes=8) == EINVAL
    n = ctypes.c_int64(-1)
    assert lib.enslam_event_model_workspace(h, w, 1, None) == EINVAL and lib.enslam_event_model_workspace(0, w, 1, ctypes.byref(n)) == EINVAL
    assert lib.enslam_event_model_workspace(h, w, EF.EVENT_MODEL_MAX_KERNELS + 1, ctypes.byref(n)) == EUNSUPPORTED and n.value == -1
    assert lib.enslam_event_model_workspace(33, 17, 2, ctypes.byref(n)) == 0 and n.value == 3 * 2 * 2 * 3 * 8


def test_every_refusal_has_its_error_class():
    from evennicer_slam_amd import _lib as L
    from evennicer_slam_amd import event_model as M
    from evennicer_slam_amd import functional as EF
    host = (ctypes.c_double * 4096)()
    p = ctypes.addressof(host)
    check_refusals(p, p, p, 5, 7, p, 4096 * 8, p, p, p)
    for ks, ws in (((4,), (1.0,)), ((33,), (1.0,)), ((3,) * 5, (1.0,) * 5), ((3, 5), (1.0,)), ((0,), (1.0,))):
        with pytest.raises(L.EnslamError):
            EF.event_model_kernels(ks, ws)
    cur, prev, gt = torch.rand(5, 7, 3), torch.rand(5, 7, 3), torch.rand(5, 7, 2)
    with pytest.raises(L.EnslamError):
        EF.event_model_loss(cur, prev, gt)                                    # the kernel has no CPU form: EventModelLoss routes CPU tensors
    with pytest.raises(ValueError):
        M.event_model_loss_torch(cur, prev, gt, kernel_sizes=(11,))          # k // 2 >= min(h, w)
    with pytest.raises(ValueError):
        M.event_model_loss_torch(cur, prev, gt, kernel_sizes=(4,))
    with pytest.raises(ValueError):
        M.predict_events(cur, prev, c_pos=0.0)
    with pytest.raises(ValueError):
        M.event_model_loss(cur, prev, gt, kernel_sizes=(9, 5), kernel_weights=(1.0,))
