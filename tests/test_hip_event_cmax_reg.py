"""-m gpu: the event-collapse regularisers of csrc/event_cmax.hip -- enslam_event_cmax_reg_eval through ctypes and behind
functional.event_cmax_eval(reg=...) and event_cmax.py on a HIP device.

Per case of tests/event_cmax_reg_cases.py and per kind, the raw entry between guard regions: iwe, blurred, stats, dropped and
reg_stats BIT-EQUAL to the numpy route and reg_stats within the derived bound of the yardstick; the shared outputs bit-equal to
the existing entries for all three reg_kinds, and reg_stats all zero for ENSLAM_CMAX_REG_NONE.  The same bits for time-ordered,
pixel-major and shuffled streams (R inside the bound: the header sums in stream order).  One regularised evaluation captured in
a graph and replayed three times over refilled outputs.  estimate_motion's trace with a regulariser bit-equal on both routes.
Refusals return without a launch.  The prior through SLAM.track with tracking.cmax_reg: divergence."""
import ctypes

import numpy as np
import pytest
import torch

from tests import event_cmax_cases as CC
from tests import event_cmax_reg_cases as GC
from tests import event_cmax_reg_numpy as YG
from tests import event_cmax_rigid_cases as RC

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
GUARD = 256
MODEL_CODE = dict(flow=0, rotation=1, rigid=2)
KIND_CODE = dict(none=0, divergence=1, deformation=2)
SENT_I, SENT_F = -(1 << 62) + 12345, -7.5


def _bits(a):
    return a.view(torch.int64) if a.dtype == torch.float64 else a


def _guarded(n, dtype, fill):
    buf = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=DEV)
    return buf, buf[GUARD:GUARD + n]


def _raw(arrays, kw, kind, want_grad=True):
    """enslam_event_cmax_reg_eval itself, every output, the workspace and the depth between GUARD sentinel elements; returns
    dict(name -> (whole buffer, view))"""
    from evennicer_slam_amd import _lib as L
    from evennicer_slam_amd import functional as EF
    H, W, N, model = kw['H'], kw['W'], int(arrays[0].shape[0]), kw['model']
    P, rigid = YG.PARAMS[model], model == 'rigid'
    nbytes = ctypes.c_int64(0)
    L.check(L.lib().enslam_event_cmax_reg_workspace(H, W, N, MODEL_CODE[model], ctypes.byref(nbytes)), "workspace")
    assert nbytes.value == (3 * H * W + max(-(-H * W // 256), -(-N // 256) * (1 + P))) * 8
    bufs = dict(iwe=_guarded(H * W, torch.int64, SENT_I), blurred=_guarded(H * W, torch.float64, SENT_F),
                stats=_guarded(2 + P, torch.float64, SENT_F), dropped=_guarded(4 if rigid else 3, torch.int64, SENT_I),
                reg_stats=_guarded(2 + P, torch.float64, SENT_F), ws=_guarded(nbytes.value // 8, torch.float64, SENT_F))
    if rigid:
        bufs['depth'] = _guarded(H * W, torch.float32, float('nan'))
        bufs['depth'][1].copy_(torch.from_numpy(kw['depth']).reshape(-1))
    v = {k: b[1] for k, b in bufs.items()}
    cal, taps = kw['calib'], kw['taps']
    rc = L.lib().enslam_event_cmax_reg_eval(*(a.data_ptr() for a in arrays), N, H, W, cal[0], cal[1], cal[2], cal[3], MODEL_CODE[model],
                                            v['depth'].data_ptr() if rigid else None, (ctypes.c_double * P)(*kw['theta']), kw['t_ref'],
                                            1 if kw['signed'] else 0, len(taps), (ctypes.c_double * len(taps))(*taps), v['ws'].data_ptr(),
                                            nbytes.value, v['iwe'].data_ptr(), v['blurred'].data_ptr(), v['stats'].data_ptr(),
                                            v['dropped'].data_ptr(), KIND_CODE[kind], v['reg_stats'].data_ptr(), 1 if want_grad else 0,
                                            EF._stream())
    torch.cuda.synchronize()
    assert rc == 0
    for k, (buf, view) in bufs.items():
        if k == 'depth':
            assert bool(torch.isnan(buf[:GUARD]).all()) and bool(torch.isnan(buf[GUARD + view.numel():]).all())
            assert np.array_equal(view.cpu().numpy().view(np.uint8), kw['depth'].reshape(-1).view(np.uint8))
            continue
        sent = SENT_I if buf.dtype == torch.int64 else SENT_F
        assert bool((buf[:GUARD] == sent).all()) and bool((buf[GUARD + view.numel():] == sent).all()), k
        if k != 'ws':
            assert not bool((view == sent).any()), k                        # ... and every element inside was written
    return bufs


def _existing(arrays, kw, want_grad=True):
    from evennicer_slam_amd import functional as EF
    depth = torch.from_numpy(kw['depth']).to(DEV) if kw['model'] == 'rigid' else None
    out = EF.event_cmax_eval(*arrays, kw['H'], kw['W'], kw['calib'], kw['model'], kw['theta'], kw['t_ref'], kw['taps'], signed=kw['signed'],
                             want_grad=want_grad, want_blurred=True, depth=depth)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("cid", GC.IDS)
def test_case_on_the_device(cid):
    from evennicer_slam_amd import event_cmax as M
    src, case = GC.BY_ID[cid]
    base = GC.base_reference(src, case)
    refs = {kind: GC.reference(src, case, kind) for kind in GC.KINDS}
    GC.check_conditions(src, case, base, refs)
    kw = GC.arguments(src, case)
    host = GC.stream(src, case)
    arrays = tuple(torch.from_numpy(a).to(DEV) for a in host)
    old = _existing(arrays, kw)
    P = YG.PARAMS[case['model']]
    for kind in ('none',) + GC.KINDS:
        v = {k: b[1] for k, b in _raw(arrays, kw, kind).items()}
        # the shared outputs: the existing entries' bits, whatever the kind
        assert torch.equal(v['iwe'], old[0].reshape(-1)) and torch.equal(_bits(v['blurred']), _bits(old[1].reshape(-1)))
        assert torch.equal(_bits(v['stats']), _bits(old[2])) and torch.equal(v['dropped'], old[3])
        if kind == 'none':
            assert not bool(v['reg_stats'].any()) and not bool(torch.signbit(v['reg_stats']).any())
            continue
        n_iwe, n_J, n_stats, n_dropped, n_rs = M.cmax_numpy(*host, reg=kind, **kw)
        assert np.array_equal(v['iwe'].cpu().numpy(), n_iwe.reshape(-1)) and v['dropped'].cpu().tolist() == n_dropped.tolist()
        assert np.array_equal(v['blurred'].cpu().numpy().view(np.int64), n_J.reshape(-1).view(np.int64))
        assert np.array_equal(v['stats'].cpu().numpy().view(np.int64), n_stats.view(np.int64))
        got = v['reg_stats'].cpu().numpy()
        assert np.array_equal(got.view(np.int64), n_rs.view(np.int64)), (kind, got, n_rs)
        ref, b = refs[kind], GC.bounds(case, refs[kind])
        errs = dict(R=abs(got[0] - ref['R']), dR=np.abs(got[2:] - ref['dR']))
        print(cid, kind, {k: (np.asarray(errs[k]).tolist(), np.asarray(b[k]).tolist()) for k in errs})
        assert got[1] == ref['M'] and errs['R'] <= b['R'] and np.all(errs['dR'] <= b['dR']), (errs, b)
        # without the gradient: the same R and M, dR stays zero
        ng = {k: b_[1] for k, b_ in _raw(arrays, kw, kind, want_grad=False).items()}
        assert torch.equal(_bits(ng['reg_stats'][:2]), _bits(v['reg_stats'][:2])) and not bool(ng['reg_stats'][2:].any())
        assert torch.equal(ng['iwe'], v['iwe']) and torch.equal(_bits(ng['stats'][:2]), _bits(v['stats'][:2])) and not bool(ng['stats'][2:].any())
    for a, s in zip(arrays, host):
        assert np.array_equal(a.cpu().numpy().view(np.uint8), s.view(np.uint8))
    # behind the Python entry: the fifth tensor, the same bits
    out = M._evaluate(_stream_of(arrays), kw['H'], kw['W'], kw['calib'], kw['model'], kw['theta'], kw['t_ref'], kw['taps'], kw['signed'], True,
                      depth=torch.from_numpy(kw['depth']).to(DEV) if case['model'] == 'rigid' else None, reg='deformation')
    assert len(out) == 5 and np.array_equal(out[4].view(np.int64), M.cmax_numpy(*host, reg='deformation', **kw)[4].view(np.int64))
    assert out[4].shape == (2 + P,)


def _stream_of(arrays):
    from evennicer_slam_amd.event_stream import EventStream
    return EventStream(*arrays)


def test_the_bits_do_not_depend_on_the_run_or_on_the_order_of_the_stream():
    src, case = GC.BY_ID['rigid-45x61_N700']
    kw = GC.arguments(src, case)
    t, x, y, p = GC.stream(src, case)
    by_time = np.argsort(t, kind='stable')
    by_pixel = by_time[np.argsort((y.astype(np.int64) * case['W'] + x)[by_time], kind='stable')]
    assert not np.array_equal(by_time, by_pixel) and not np.array_equal(by_time, np.arange(len(t)))
    for kind in GC.KINDS:
        b = GC.bounds(case, GC.reference(src, case, kind))
        outs = []
        for order in (np.arange(len(t)), by_time, by_pixel):
            arrays = tuple(torch.from_numpy(np.ascontiguousarray(a[order])).to(DEV) for a in (t, x, y, p))
            first, again = _raw(arrays, kw, kind), _raw(arrays, kw, kind)
            for k in ('iwe', 'blurred', 'stats', 'dropped', 'reg_stats'):
                assert torch.equal(_bits(first[k][1]), _bits(again[k][1])), k          # two runs: every bit
            outs.append({k: v[1] for k, v in first.items()})
        for o in outs[1:]:
            assert torch.equal(o['iwe'], outs[0]['iwe']) and torch.equal(_bits(o['blurred']), _bits(outs[0]['blurred']))
            assert torch.equal(o['dropped'], outs[0]['dropped']) and torch.equal(_bits(o['stats'][:2]), _bits(outs[0]['stats'][:2]))
            assert o['reg_stats'][1] == outs[0]['reg_stats'][1]
            # (the header sums over the events in stream order: another order is another rounding of the same sum)
            diff = (o['reg_stats'] - outs[0]['reg_stats']).abs().cpu().numpy()
            assert diff[0] <= 2 * b['R'] and np.all(diff[2:] <= 2 * b['dR'])


def test_one_regularised_evaluation_inside_a_stream_capture():
    """the chain of launches with the regulariser's pass is captured once and replayed over refilled outputs: every time the
    bits of the eager call"""
    from evennicer_slam_amd import functional as EF
    src, case = GC.BY_ID['rigid-45x61_N700']
    kw = GC.arguments(src, case)
    arrays = tuple(torch.from_numpy(a).to(DEV) for a in GC.stream(src, case))
    depth = torch.from_numpy(kw['depth']).to(DEV)
    args = (*arrays, kw['H'], kw['W'], kw['calib'], 'rigid', kw['theta'], kw['t_ref'], kw['taps'])
    call = lambda: EF.event_cmax_eval(*args, signed=kw['signed'], want_blurred=True, depth=depth, reg='deformation')     # noqa: E731
    eager = call()
    torch.cuda.synchronize()
    assert len(eager) == 5 and float(eager[4][0]) > 0
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                        # warm-up on a side stream, as torch's capture recipe asks
        call()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = call()
    for _ in range(3):
        for o in out:
            o.fill_(-3)
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(out, eager):
            assert torch.equal(_bits(a), _bits(b))


def test_estimate_motion_follows_the_cpu_trace_to_the_bit():
    from evennicer_slam_amd import event_cmax as M
    from evennicer_slam_amd.event_stream import EventStream
    depth = torch.from_numpy(RC.rec_depth())
    host = EventStream(*RC.planted_stream(1))
    kw = dict(H=CC.REC_H, W=CC.REC_W, sigma=CC.SIGMA, ksize=CC.REC_K, t_ref=0.0, reg='divergence', reg_weight=GC.REC_WEIGHT)
    cpu = M.estimate_motion(host, CC.REC_CALIB, 'rigid', depth=depth, **kw)
    dev = M.estimate_motion(host.to(DEV), CC.REC_CALIB, 'rigid', depth=depth.to(DEV), **kw)
    for key in ('thetas', 'trace', 'f_trace', 'reg_trace', 'evals', 'reg_weight_abs'):
        assert dev[key] == cpu[key], key
    assert len(cpu['trace']) > 3 and abs(cpu['theta'][5]) < 2
    R, dR, Mv = M.regulariser(host.to(DEV), CC.REC_CALIB, 'rigid', cpu['theta'], CC.REC_H, CC.REC_W, t_ref=0.0, depth=depth.to(DEV))
    Rc, dRc, Mc = M.regulariser(host, CC.REC_CALIB, 'rigid', cpu['theta'], CC.REC_H, CC.REC_W, t_ref=0.0, depth=depth)
    assert R == Rc == cpu['reg_trace'][-1] and np.array_equal(dR.view(np.int64), dRc.view(np.int64)) and Mv == Mc
    F, G = M.contrast(host.to(DEV), CC.REC_CALIB, 'rigid', cpu['theta'], CC.REC_H, CC.REC_W, t_ref=0.0, ksize=CC.REC_K, depth=depth.to(DEV),
                      reg='divergence', reg_weight=cpu['reg_weight_abs'])
    assert F == cpu['trace'][-1] and G.shape == (6,)


def test_abi_refusals_leave_the_buffers_alone():
    from tests.test_event_cmax_reg_cpu import check_refusals
    src, case = GC.BY_ID['rigid-hand_5x7']
    host = GC.stream(src, case)
    t, x, y, p = (torch.from_numpy(a).to(DEV) for a in host)
    depth_host = RC.depth_image(case)
    depth = torch.from_numpy(depth_host).to(DEV)
    n = 4096
    out_i = torch.full((n,), -12345, dtype=torch.int64, device=DEV)
    out_f = {k: torch.full((n,), -7.5, dtype=torch.float64, device=DEV) for k in ('ws', 'blurred', 'stats', 'reg_stats')}
    drop = torch.full((16,), -12345, dtype=torch.int64, device=DEV)
    check_refusals(t.data_ptr(), x.data_ptr(), y.data_ptr(), p.data_ptr(), depth.data_ptr(), case['N'], 5, 7, out_f['ws'].data_ptr(), n * 8,
                   out_i.data_ptr(), out_f['blurred'].data_ptr(), out_f['stats'].data_ptr(), drop.data_ptr(), out_f['reg_stats'].data_ptr())
    torch.cuda.synchronize()
    assert bool((out_i == -12345).all()) and bool((drop == -12345).all()) and all(bool((b == -7.5).all()) for b in out_f.values())
    for a, s in zip((t, x, y, p, depth), host + (depth_host,)):
        assert np.array_equal(a.cpu().numpy().view(np.uint8), s.view(np.uint8))
    from evennicer_slam_amd import _lib as L
    from evennicer_slam_amd import functional as EF
    kw = GC.arguments(src, case)
    for model, theta, d, reg in (('rigid', kw['theta'], depth, 'curl'), ('rigid', kw['theta'], None, 'divergence'),
                                 ('rotation', [0.1, 0.2, 0.3], depth, 'divergence'), ('flow', [1.0, 2.0], depth, 'deformation')):
        with pytest.raises(L.EnslamError):
            EF.event_cmax_eval(t, x, y, p, 5, 7, kw['calib'], model, theta, 0.0, [1.0], depth=d, reg=reg)


def test_the_prior_through_slam_track(tmp_path_factory):
    """Five frames of the simulated demo sequence, tracking.iters = 0, tracking.cmax_reg: divergence: the tracker starts from
    the pose composed from the regularised estimate -- on the device, and bit for bit the CPU route's trace"""
    from evennicer_slam_amd import event_cmax as M
    from evennicer_slam_amd.slam import SLAM
    from tests.test_event_cmax_rigid_cpu import N_FRAMES, const_speed, demo_sequence, with_prior
    from tests.test_hip_event_cmax_rigid import slam_depth
    root = tmp_path_factory.mktemp('prior_reg')
    cfg, ds, poses, streams, stamps = demo_sequence(tmp_path_factory.mktemp('seq'), device=DEV)
    slam = SLAM(with_prior(cfg, 'cmax', cmax_reg='divergence', cmax_reg_weight=4.0), ds, str(root / 'reg'), device=DEV, static_shapes=True)
    for i in range(N_FRAMES):
        slam.estimate_c2w_list[i] = ds[i][-1].cpu()
    slam._last_rgbd = (0, ds[0][2])
    used = 0
    for idx in (2, 3, 4):
        got = slam.track(idx, None, None, None, None, None, rgbd=False).cpu()
        res = slam.motion_prior_last
        stream, t0, t1 = ds.event_slice(idx)
        assert stream.device.type == 'cuda'
        host = M.estimate_motion(stream.to('cpu'), (slam.fx, slam.fy, slam.cx, slam.cy), 'rigid', slam.H, slam.W, theta0=res['thetas'][0],
                                 t_ref=t0, iters=slam.cmax_iters, depth=slam_depth(slam, idx).cpu(), reg='divergence', reg_weight=4.0)
        assert host['thetas'] == res['thetas'] and host['trace'] == res['trace'] and host['f_trace'] == res['f_trace']
        pre = slam.estimate_c2w_list[idx - 1].double()
        if res['f_trace'][-1] > res['f_trace'][0]:
            assert torch.equal(got[:3], (pre @ M.relative_motion(res['theta'], t1 - t0)).float()[:3])
            used += 1
        else:
            assert torch.equal(got[:3], const_speed(slam, idx, DEV)[:3].cpu())
    st = slam.motion_prior_stats
    assert used >= 1 and st['cmax'] == used and st['no_rise'] == 3 - used and 'collapsed' not in st
