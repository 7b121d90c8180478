"""-m gpu: csrc/event_model.hip -- enslam_event_model_loss behind event_model.EventModelLoss on a HIP device -- against the
float64 yardstick tests/event_model_numpy.py on the cases of tests/event_model_cases.py, within the tolerance derived there.

Per case: pred, every term and the loss, the unit gradient under the device's own hinge decisions, the blurred images; the
device's decisions differ from float64 only inside the margin; the planted tie block is exactly zero; two calls give the same
bits and leave the inputs alone; guard regions around every output stay intact.  Then the ABI refusals (no launch), the
backward's scaling, and the graphed camera iteration with `predictor: 'model'` against the eager one."""
import ctypes

import numpy as np
import pytest
import torch

from tests import event_model_cases as MC

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
GUARD = 256
_CASES = {c['name']: c for c in MC.CASES}
_REF = {}


def _reference(name):
    if name not in _REF:
        _REF[name] = MC.reference(_CASES[name])
    return _REF[name]


def _device_inputs(case):
    return tuple(torch.from_numpy(a).to(DEV) for a in MC.inputs(case))


def _run(case, want_blurred=True):
    from evennicer_slam_amd import functional as EF
    cur, prev, gt = _device_inputs(case)
    out = EF.event_model_loss(cur, prev, gt, case['c_neg'], case['c_pos'], case['eps'], case['ksizes'], case['weights'], want_blurred)
    torch.cuda.synchronize()
    return (cur, prev, gt), out


@pytest.mark.parametrize("name", [c['name'] for c in MC.CASES])
def test_case_against_the_yardstick(name):
    case, ref64 = _CASES[name], _reference(name)
    K = len(case['ksizes'])
    (cur, prev, gt), (pred, sums, grad, bg, bp) = _run(case)
    pred_n, sums_n, grad_n = pred.cpu().numpy().astype(np.float64), sums.cpu().numpy(), grad.cpu().numpy().astype(np.float64)
    assert pred.dtype == torch.float32 and grad.dtype == torch.float32 and sums.dtype == torch.float64 and sums_n.shape == (K + 2,)
    # the hinge decisions of the device: different from float64 only inside the margin, on at most 1 % of the pixels
    branch = np.where(pred_n[..., 1] > 0, 1, np.where(pred_n[..., 0] > 0, -1, 0))
    differ = branch != ref64['branch']
    assert bool(np.all(np.abs(ref64['d'][differ]) <= MC.branch_margin(case['eps']))), np.abs(ref64['d'][differ]).max()
    assert differ.mean() <= MC.MAX_BRANCH_SHARE
    assert not np.any((pred_n[..., 0] > 0) & (pred_n[..., 1] > 0))
    ref = MC.reference(case, branch=branch) if differ.any() else ref64
    b = MC.bounds(case, ref)
    report = {}

    def close(what, got, want, bound):
        err = float(np.abs(got - want).max()) if np.size(want) else 0.0
        report[what] = (MC.fraction(err, want), MC.fraction(bound, want))
        assert err <= bound, (what, err, bound, report)

    close('pred', pred_n, ref['pred'], b['pred'])
    for j in range(K + 1):
        close(f'term{j}', sums_n[j], ref['terms'][j], b['terms'][j])
    close('loss', sums_n[K + 1], ref['loss'], b['loss'])
    close('grad', grad_n, ref['grad'], b['grad'])
    if K:
        assert tuple(bg.shape) == tuple(bp.shape) == (K, case['h'], case['w'], 2)
        for i in range(K):
            close(f'blur_gt{i}', bg[i].cpu().numpy().astype(np.float64), ref['blur_gt'][i], b['blur_gt'][i])
            close(f'blur_pred{i}', bp[i].cpu().numpy().astype(np.float64), ref['blur_pred'][i], b['blur_pred'][i])
    else:
        assert bg is None and bp is None
    print(name, {k: '%.2e / %.2e' % v for k, v in report.items()})
    if case['kind'] == 'tie':
        blk = MC.TIE_BLOCK
        assert np.all(pred_n[blk] == 0) and np.all(grad_n[blk] == 0)
    if case['kind'] == 'negative':
        assert np.all(grad_n[2, 3] == 0) and pred_n[2, 3, 0] > 0
    # the same bits again, with and without the blurred images, and untouched inputs
    (cur2, prev2, gt2), (pred2, sums2, grad2, bg2, bp2) = _run(case, want_blurred=False)
    assert bg2 is None and bp2 is None
    for a, a2 in ((pred, pred2), (grad, grad2)):
        assert torch.equal(a.view(torch.int32), a2.view(torch.int32))
    assert torch.equal(sums.view(torch.int64), sums2.view(torch.int64))
    for a, src in zip((cur, prev, gt), MC.inputs(case)):
        assert np.array_equal(a.cpu().numpy().view(np.uint32), src.view(np.uint32))


@pytest.mark.parametrize("name", ['5x7_k9', '2Tp1x2Tp1_K2', '5x300_k9'])
def test_guard_regions_stay_intact(name):
    """every output sits between GUARD sentinel elements inside one allocation; the raw entry is called on the views"""
    from evennicer_slam_amd import _lib as L
    from evennicer_slam_amd import functional as EF
    case = _CASES[name]
    h, w, K = case['h'], case['w'], len(case['ksizes'])
    cur, prev, gt = _device_inputs(case)
    nbytes = ctypes.c_int64(0)
    L.check(L.lib().enslam_event_model_workspace(h, w, K, ctypes.byref(nbytes)), "workspace")
    tiles = ((h + MC.TILE - 1) // MC.TILE) * ((w + MC.TILE - 1) // MC.TILE)
    assert nbytes.value == tiles * 2 * (K + 1) * 8

    def guarded(n, dtype, fill):
        buf = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=DEV)
        return buf, buf[GUARD:GUARD + n]

    bufs = {k: guarded(n, dt, fill) for k, (n, dt, fill) in dict(
        pred=(h * w * 2, torch.float32, -7.5), grad=(h * w * 3, torch.float32, -7.5), sums=(K + 2, torch.float64, -7.5),
        ws=(nbytes.value // 8, torch.float64, -7.5), bg=(K * h * w * 2, torch.float32, -7.5),
        bp=(K * h * w * 2, torch.float32, -7.5)).items()}
    Kc, ksizes, weights, taps = EF.event_model_kernels(case['ksizes'], case['weights'])
    v = {k: b[1] for k, b in bufs.items()}
    rc = L.lib().enslam_event_model_loss(cur.data_ptr(), prev.data_ptr(), gt.data_ptr(), h, w, case['c_neg'], case['c_pos'], case['eps'],
                                         Kc, ksizes, weights, taps, v['ws'].data_ptr(), nbytes.value, v['pred'].data_ptr(),
                                         v['sums'].data_ptr(), v['grad'].data_ptr(), v['bg'].data_ptr(), v['bp'].data_ptr(), EF._stream())
    torch.cuda.synchronize()
    assert rc == 0
    for k, (buf, view) in bufs.items():
        assert bool((buf[:GUARD] == -7.5).all()) and bool((buf[GUARD + view.numel():] == -7.5).all()), k
        assert not bool((view == -7.5).any()), k                                # ... and every element inside was written
    pred, sums, grad, bg, bp = EF.event_model_loss(cur, prev, gt, case['c_neg'], case['c_pos'], case['eps'], case['ksizes'],
                                                   case['weights'], True)
    assert torch.equal(pred.reshape(-1), v['pred']) and torch.equal(grad.reshape(-1), v['grad']) and torch.equal(sums, v['sums'])
    assert torch.equal(bg.reshape(-1), v['bg']) and torch.equal(bp.reshape(-1), v['bp'])


def test_abi_refusals_return_their_codes_without_a_launch():
    from tests.test_event_model_cpu import check_refusals
    cur, prev, gt = _device_inputs(_CASES['5x7_k9'])
    out = torch.full((5 * 7 * 3 + 16,), -7.5, dtype=torch.float32, device=DEV)
    sums = torch.full((8,), -7.5, dtype=torch.float64, device=DEV)
    ws = torch.full((64,), -7.5, dtype=torch.float64, device=DEV)
    check_refusals(cur.data_ptr(), prev.data_ptr(), gt.data_ptr(), 5, 7, ws.data_ptr(), 64 * 8, out.data_ptr(), sums.data_ptr(),
                   out.data_ptr())
    torch.cuda.synchronize()
    assert bool((out == -7.5).all()) and bool((sums == -7.5).all()) and bool((ws == -7.5).all())       # nothing was launched


def test_backward_scales_the_unit_gradient():
    from evennicer_slam_amd import event_model as M
    from evennicer_slam_amd import functional as EF
    case = _CASES['Tp1xTm1_k9']
    cur, prev, gt = _device_inputs(case)
    unit = EF.event_model_loss(cur, prev, gt, case['c_neg'], case['c_pos'], case['eps'], case['ksizes'], case['weights'])[2]
    leaf = cur.clone().requires_grad_(True)
    loss, pred, terms, gts, preds = M.event_model_loss(leaf, prev, gt, case['c_neg'], case['c_pos'], case['eps'], True, case['ksizes'],
                                                       case['weights'], unblurred_weight=0.5)
    assert loss.dtype == torch.float64 and loss.requires_grad and not pred.requires_grad and len(terms) == 2 and len(gts) == len(preds) == 1
    (loss * 0.375).backward()
    assert torch.equal(leaf.grad, unit * 0.375)                               # (0.375 is exact in float32: one rounding each side)
    ref = _reference(case['name'])
    assert abs(float(terms[0]) - 0.5 * ref['terms'][0]) <= 0.5 * MC.bounds(case, ref)['terms'][0]
    # the CPU route of the same function: the torch statement, inside the same tolerance
    cl = cur.cpu().requires_grad_(True)
    l_cpu = M.event_model_loss(cl, prev.cpu(), gt.cpu(), case['c_neg'], case['c_pos'], case['eps'], True, case['ksizes'], case['weights'])[0]
    l_cpu.backward()
    b = MC.bounds(case, ref)
    assert abs(float(l_cpu.detach()) - ref['loss']) <= b['loss'] and float((cl.grad.double().numpy() - ref['grad']).__abs__().max()) <= b['grad']


def test_graphed_camera_iteration_equals_the_eager_one():
    """GraphedCameraIteration with predictor 'model' on the tiny golden scene, two frames: the replayed losses equal the eager
    iteration's on the same pixel draws, and the camera moves the same way."""
    from tests.test_event_model_cpu import model_tracker_setup
    runs = {}
    for mode in ('eager', 'graph'):
        runs[mode] = model_tracker_setup(DEV).run(mode, frames=2, iters=2)
    for a, b in zip(runs['eager'], runs['graph']):
        assert a['rgbd'] == pytest.approx(b['rgbd'], rel=1e-5, abs=1e-7), (a, b)
        assert a['event'] == pytest.approx(b['event'], rel=1e-5, abs=1e-7), (a, b)
        assert a['event'] > 0 and np.allclose(a['camera'], b['camera'], rtol=1e-5, atol=1e-7)
