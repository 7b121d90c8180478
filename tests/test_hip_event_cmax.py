"""-m gpu: csrc/event_cmax.hip -- enslam_event_cmax_eval behind functional.event_cmax_eval and event_cmax.py on a HIP device.

Per case of tests/event_cmax_cases.py: the image, the counters, mu, f, the gradient and the blurred image BIT-EQUAL to the numpy
route (the header fixes every operation and every sum order), and within the bound derived in the cases file of the yardstick
tests/event_cmax_numpy.py; two calls give the same bits and leave the inputs alone.  Guard regions around every output and the
workspace stay intact.  estimate_motion follows the same theta trace to the bit on the device as on the CPU route.  The refusals
leave the buffers alone.  The demo tool runs on three frames."""
import ctypes
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

from tests import event_cmax_cases as CC

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
GUARD = 256
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_CASES = {c['name']: c for c in CC.CASES}


def _device_stream(case):
    return tuple(torch.from_numpy(a).to(DEV) for a in CC.stream(case))


def _run(case, arrays, **over):
    from evennicer_slam_amd import functional as EF
    kw = CC.arguments(case)
    kw.update(over)
    out = EF.event_cmax_eval(*arrays, kw['H'], kw['W'], kw['calib'], kw['model'], kw['theta'], kw['t_ref'], kw['taps'], signed=kw['signed'],
                             want_grad=kw.get('want_grad', True), want_blurred=kw.get('want_blurred', True))
    torch.cuda.synchronize()
    return out


def _bits(a):
    return a.view(torch.int64) if a.dtype == torch.float64 else a


@pytest.mark.parametrize("name", [c['name'] for c in CC.CASES])
def test_case_on_the_device(name):
    from evennicer_slam_amd import event_cmax as M
    case = _CASES[name]
    ref = CC.reference(case)
    CC.check_conditions(case, ref)
    arrays = _device_stream(case)
    iwe, J, stats, dropped = _run(case, arrays)
    P = M.MODELS[case['model']]
    assert iwe.dtype == torch.int64 and tuple(iwe.shape) == tuple(J.shape) == (case['H'], case['W']) and tuple(stats.shape) == (2 + P,)
    # bit-equal to the numpy route
    n_iwe, n_J, n_stats, n_dropped = M.cmax_numpy(*CC.stream(case), **CC.arguments(case))
    assert np.array_equal(iwe.cpu().numpy(), n_iwe) and dropped.cpu().tolist() == n_dropped.tolist()
    assert np.array_equal(J.cpu().numpy().view(np.int64), n_J.view(np.int64))
    got = stats.cpu().numpy()
    assert np.array_equal(got.view(np.int64), n_stats.view(np.int64)), (got, n_stats)
    # within the derived bound of the yardstick
    assert np.array_equal(iwe.cpu().numpy(), ref['iwe']) and dropped.cpu().tolist() == ref['dropped'].tolist()
    b = CC.bounds(case, ref)
    errs = dict(mu=abs(got[0] - ref['mu']), f=abs(got[1] - ref['f']), grad=np.abs(got[2:] - ref['grad']))
    print(name, {k: (np.asarray(errs[k]).tolist(), np.asarray(b[k]).tolist()) for k in errs})
    assert errs['mu'] <= b['mu'] and errs['f'] <= b['f'] and np.all(errs['grad'] <= b['grad']), (errs, b)
    # the same bits again, with and without the blurred image and the gradient; untouched inputs
    iwe2, J2, stats2, dropped2 = _run(case, arrays, want_blurred=False)
    assert J2 is None and torch.equal(iwe, iwe2) and torch.equal(_bits(stats), _bits(stats2)) and torch.equal(dropped, dropped2)
    iwe3, J3, stats3, dropped3 = _run(case, arrays, want_grad=False)
    assert torch.equal(iwe, iwe3) and torch.equal(_bits(J), _bits(J3)) and torch.equal(_bits(stats[:2]), _bits(stats3[:2]))
    assert not bool(stats3[2:].any()) and torch.equal(dropped, dropped3)
    for a, src in zip(arrays, CC.stream(case)):
        assert np.array_equal(a.cpu().numpy().view(np.uint8), src.view(np.uint8))


@pytest.mark.parametrize("name", ['hand_5x7', '45x61_N257', '8x9_N65537', '1x300_k9_wider'])
def test_guard_regions_stay_intact(name):
    """every output and the workspace sit between GUARD sentinel elements inside one allocation; the raw entry is called"""
    from evennicer_slam_amd import _lib as L
    from evennicer_slam_amd import event_cmax as M
    from evennicer_slam_amd import functional as EF
    case = _CASES[name]
    kw = CC.arguments(case)
    H, W, N, P = case['H'], case['W'], case['N'], M.MODELS[case['model']]
    arrays = _device_stream(case)
    nbytes = ctypes.c_int64(0)
    L.check(L.lib().enslam_event_cmax_workspace(H, W, N, P, ctypes.byref(nbytes)), "workspace")
    assert nbytes.value == (3 * H * W + max(-(-H * W // 256), -(-N // 256) * P)) * 8

    def guarded(n, dtype, fill):
        buf = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=DEV)
        return buf, buf[GUARD:GUARD + n]

    SENT_I, SENT_F = -(1 << 62) + 12345, -7.5
    bufs = dict(iwe=guarded(H * W, torch.int64, SENT_I), blurred=guarded(H * W, torch.float64, SENT_F),
                stats=guarded(2 + P, torch.float64, SENT_F), dropped=guarded(3, torch.int64, SENT_I),
                ws=guarded(nbytes.value // 8, torch.float64, SENT_F))
    v = {k: b[1] for k, b in bufs.items()}
    code = EF.EVENT_CMAX_MODELS[case['model']][0]
    cal, taps = kw['calib'], kw['taps']
    rc = L.lib().enslam_event_cmax_eval(*(a.data_ptr() for a in arrays), N, H, W, cal[0], cal[1], cal[2], cal[3], code,
                                        (ctypes.c_double * P)(*kw['theta']), kw['t_ref'], 1 if kw['signed'] else 0, len(taps),
                                        (ctypes.c_double * len(taps))(*taps), v['ws'].data_ptr(), nbytes.value, v['iwe'].data_ptr(),
                                        v['blurred'].data_ptr(), v['stats'].data_ptr(), v['dropped'].data_ptr(), 1, EF._stream())
    torch.cuda.synchronize()
    assert rc == 0
    for k, (buf, view) in bufs.items():
        sent = SENT_I if buf.dtype == torch.int64 else SENT_F
        assert bool((buf[:GUARD] == sent).all()) and bool((buf[GUARD + view.numel():] == sent).all()), k
        if k != 'ws':
            assert not bool((view == sent).any()), k                            # ... and every element inside was written
    iwe, J, stats, dropped = _run(case, arrays)
    assert torch.equal(iwe.reshape(-1), v['iwe']) and torch.equal(_bits(J.reshape(-1)), _bits(v['blurred']))
    assert torch.equal(_bits(stats), _bits(v['stats'])) and torch.equal(dropped, v['dropped'])


@pytest.mark.parametrize("model", ['flow', 'rotation'])
def test_estimate_motion_follows_the_cpu_trace_to_the_bit(model):
    from evennicer_slam_amd import event_cmax as M
    from evennicer_slam_amd.event_stream import EventStream
    for seed in CC.REC_SEEDS[:2]:
        host = EventStream(*CC.planted_stream(model, seed))
        kw = dict(H=CC.REC_H, W=CC.REC_W, sigma=CC.SIGMA, ksize=CC.REC_K, t_ref=CC.REC_WINDOW / 2)
        cpu = M.estimate_motion(host, CC.REC_CALIB, model, **kw)
        dev = M.estimate_motion(host.to(DEV), CC.REC_CALIB, model, **kw)
        assert dev['thetas'] == cpu['thetas'] and dev['trace'] == cpu['trace'] and dev['evals'] == cpu['evals'] and len(cpu['trace']) > 3
        f, grad = M.contrast(host.to(DEV), CC.REC_CALIB, model, cpu['theta'], CC.REC_H, CC.REC_W, t_ref=kw['t_ref'], ksize=CC.REC_K)
        assert f == cpu['trace'][-1]
        img, blurred = M.warp_image(host.to(DEV), CC.REC_CALIB, model, cpu['theta'], CC.REC_H, CC.REC_W, t_ref=kw['t_ref'], ksize=CC.REC_K)
        img_c, blurred_c = M.warp_image(host, CC.REC_CALIB, model, cpu['theta'], CC.REC_H, CC.REC_W, t_ref=kw['t_ref'], ksize=CC.REC_K)
        assert img.device.type == 'cuda' and torch.equal(img.cpu(), img_c) and torch.equal(_bits(blurred.cpu()), _bits(blurred_c))


def test_abi_refusals_leave_the_buffers_alone():
    from tests.test_event_cmax_cpu import check_refusals
    case = _CASES['hand_5x7']
    t, x, y, p = _device_stream(case)
    n = 4096
    out_i = torch.full((n,), -12345, dtype=torch.int64, device=DEV)
    out_f = {k: torch.full((n,), -7.5, dtype=torch.float64, device=DEV) for k in ('ws', 'blurred', 'stats')}
    drop = torch.full((16,), -12345, dtype=torch.int64, device=DEV)
    check_refusals(t.data_ptr(), x.data_ptr(), y.data_ptr(), p.data_ptr(), case['N'], 5, 7, out_f['ws'].data_ptr(), n * 8, out_i.data_ptr(),
                   out_f['blurred'].data_ptr(), out_f['stats'].data_ptr(), drop.data_ptr())
    torch.cuda.synchronize()
    assert bool((out_i == -12345).all()) and bool((drop == -12345).all()) and all(bool((b == -7.5).all()) for b in out_f.values())
    for a, src in zip((t, x, y, p), CC.stream(case)):
        assert np.array_equal(a.cpu().numpy().view(np.uint8), src.view(np.uint8))


def test_demo_tool_on_three_frames(capsys):
    spec = importlib.util.spec_from_file_location("event_motion", os.path.join(ROOT, "tools", "event_motion.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    out = tool.main(['--demo', '3', '--device', DEV])
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert line['intervals'] == 2 and line['model'] == 'rotation' and len(out['rows']) == 2
    for row in out['rows']:
        assert row['events'] > 1000 and len(row['theta']) == len(row['omega_from_poses']) == 3
        assert row['contrast_after'] > row['contrast_before'] and row['steps'] >= 1 and all(np.isfinite(row['theta']))
