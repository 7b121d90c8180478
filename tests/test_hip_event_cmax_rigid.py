"""-m gpu: the rigid-motion model of csrc/event_cmax.hip -- enslam_event_cmax_rigid_eval behind functional.event_cmax_eval and
event_cmax.py on a HIP device -- and the tracker's opt-in pose prior on the device.

Per case of tests/event_cmax_rigid_cases.py: the image, the four counters, mu, f, the six gradient components and the blurred
image BIT-EQUAL to the numpy route, and within the bound of tests/event_cmax_cases.py of the yardstick
tests/event_cmax_rigid_numpy.py; two calls give the same bits and leave the inputs, the depth image among them, alone.  Guard
regions around every buffer stay intact, also where an event's x lies past the sensor.  The image does not depend on the order
of the stream.  Refusals leave the buffers alone.  One evaluation inside a stream capture replays to the same bits.
estimate_motion('rigid') follows the CPU route's trace to the bit.  SLAM.track starts from the recomposed pose under 'cmax' and
from the parent's under 'const_speed'."""
import ctypes

import numpy as np
import pytest
import torch

from tests import event_cmax_cases as CC
from tests import event_cmax_rigid_cases as RC

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
GUARD = 256
_CASES = {c['name']: c for c in RC.CASES}


def _device_stream(case):
    return tuple(torch.from_numpy(a).to(DEV) for a in RC.stream(case))


def _run(case, arrays, depth, **over):
    from evennicer_slam_amd import functional as EF
    kw = RC.arguments(case)
    kw.update(over)
    out = EF.event_cmax_eval(*arrays, kw['H'], kw['W'], kw['calib'], 'rigid', kw['theta'], kw['t_ref'], kw['taps'], signed=kw['signed'],
                             want_grad=kw.get('want_grad', True), want_blurred=kw.get('want_blurred', True), depth=depth)
    torch.cuda.synchronize()
    return out


def _bits(a):
    return a.view(torch.int64) if a.dtype == torch.float64 else a


@pytest.mark.parametrize("name", [c['name'] for c in RC.CASES])
def test_case_on_the_device(name):
    from evennicer_slam_amd import event_cmax as M
    case = _CASES[name]
    ref = RC.reference(case)
    RC.check_conditions(case, ref)
    arrays = _device_stream(case)
    depth_host = RC.depth_image(case)
    depth = torch.from_numpy(depth_host).to(DEV)
    iwe, J, stats, dropped = _run(case, arrays, depth)
    assert iwe.dtype == torch.int64 and tuple(iwe.shape) == tuple(J.shape) == (case['H'], case['W'])
    assert tuple(stats.shape) == (8,) and tuple(dropped.shape) == (4,)
    # bit-equal to the numpy route
    n_iwe, n_J, n_stats, n_dropped = M.cmax_numpy(*RC.stream(case), model='rigid', **RC.arguments(case))
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
    iwe2, J2, stats2, dropped2 = _run(case, arrays, depth, want_blurred=False)
    assert J2 is None and torch.equal(iwe, iwe2) and torch.equal(_bits(stats), _bits(stats2)) and torch.equal(dropped, dropped2)
    iwe3, J3, stats3, dropped3 = _run(case, arrays, depth, want_grad=False)
    assert torch.equal(iwe, iwe3) and torch.equal(_bits(J), _bits(J3)) and torch.equal(_bits(stats[:2]), _bits(stats3[:2]))
    assert not bool(stats3[2:].any()) and torch.equal(dropped, dropped3)
    for a, src in zip(arrays + (depth,), RC.stream(case) + (depth_host,)):
        assert np.array_equal(a.cpu().numpy().view(np.uint8), src.view(np.uint8))


@pytest.mark.parametrize("name", ['hand_5x7', '45x61_N257', '8x9_N65537', 'planted_9x12'])
def test_guard_regions_stay_intact(name):
    """every output, the workspace and the depth image sit between GUARD sentinel elements inside one allocation; the raw entry
    is called.  'planted_9x12' holds the event whose x lies past the sensor: its depth is never looked up."""
    from evennicer_slam_amd import _lib as L
    from evennicer_slam_amd import functional as EF
    case = _CASES[name]
    kw = RC.arguments(case)
    H, W, N, P = case['H'], case['W'], case['N'], RC.P
    arrays = _device_stream(case)
    nbytes = ctypes.c_int64(0)
    L.check(L.lib().enslam_event_cmax_rigid_workspace(H, W, N, ctypes.byref(nbytes)), "workspace")
    assert nbytes.value == (3 * H * W + max(-(-H * W // 256), -(-N // 256) * P)) * 8

    def guarded(n, dtype, fill):
        buf = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=DEV)
        return buf, buf[GUARD:GUARD + n]

    SENT_I, SENT_F = -(1 << 62) + 12345, -7.5
    bufs = dict(iwe=guarded(H * W, torch.int64, SENT_I), blurred=guarded(H * W, torch.float64, SENT_F),
                stats=guarded(2 + P, torch.float64, SENT_F), dropped=guarded(4, torch.int64, SENT_I),
                ws=guarded(nbytes.value // 8, torch.float64, SENT_F), depth=guarded(H * W, torch.float32, float('nan')))
    v = {k: b[1] for k, b in bufs.items()}
    v['depth'].copy_(torch.from_numpy(kw['depth']).reshape(-1))          # NaN all around: a depth read outside would be dropped, not voted
    cal, taps = kw['calib'], kw['taps']
    rc = L.lib().enslam_event_cmax_rigid_eval(*(a.data_ptr() for a in arrays), N, H, W, cal[0], cal[1], cal[2], cal[3],
                                              v['depth'].data_ptr(), (ctypes.c_double * P)(*kw['theta']), kw['t_ref'],
                                              1 if kw['signed'] else 0, len(taps), (ctypes.c_double * len(taps))(*taps), v['ws'].data_ptr(),
                                              nbytes.value, v['iwe'].data_ptr(), v['blurred'].data_ptr(), v['stats'].data_ptr(),
                                              v['dropped'].data_ptr(), 1, EF._stream())
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
            assert not bool((view == sent).any()), k                            # ... and every element inside was written
    iwe, J, stats, dropped = _run(case, arrays, torch.from_numpy(kw['depth']).to(DEV))
    assert torch.equal(iwe.reshape(-1), v['iwe']) and torch.equal(_bits(J.reshape(-1)), _bits(v['blurred']))
    assert torch.equal(_bits(stats), _bits(v['stats'])) and torch.equal(dropped, v['dropped'])
    assert dropped.cpu().tolist() == RC.reference(case)['dropped'].tolist()


def test_the_bits_do_not_depend_on_the_run_or_on_the_order_of_the_stream():
    case = _CASES['45x61_N700']
    ref = RC.reference(case)
    t, x, y, p = RC.stream(case)
    depth = torch.from_numpy(RC.depth_image(case)).to(DEV)
    by_time = np.argsort(t, kind='stable')
    by_pixel = by_time[np.argsort((y.astype(np.int64) * case['W'] + x)[by_time], kind='stable')]
    outs = []
    for order in (np.arange(len(t)), by_time, by_pixel):
        arrays = tuple(torch.from_numpy(np.ascontiguousarray(a[order])).to(DEV) for a in (t, x, y, p))
        first, again = _run(case, arrays, depth), _run(case, arrays, depth)
        for a, b in zip(first, again):
            assert torch.equal(_bits(a), _bits(b))                      # two runs: every bit, the gradient too
        outs.append(first)
    assert not np.array_equal(by_time, by_pixel) and not np.array_equal(by_time, np.arange(len(t)))
    slack = 2 * CC.bounds(case, ref)['grad']
    for iwe, J, stats, dropped in outs[1:]:
        assert torch.equal(iwe, outs[0][0]) and torch.equal(_bits(J), _bits(outs[0][1])) and torch.equal(dropped, outs[0][3])
        assert torch.equal(_bits(stats[:2]), _bits(outs[0][2][:2]))     # integer votes: image, blur, mu and f have no order
        # (the header sums the gradient over the events in stream order: another order is another rounding of the same sum)
        assert np.all(np.abs((stats[2:] - outs[0][2][2:]).cpu().numpy()) <= slack)


def test_abi_refusals_leave_the_buffers_alone():
    from tests.test_event_cmax_rigid_cpu import check_refusals
    case = _CASES['hand_5x7']
    t, x, y, p = _device_stream(case)
    depth_host = RC.depth_image(case)
    depth = torch.from_numpy(depth_host).to(DEV)
    n = 4096
    out_i = torch.full((n,), -12345, dtype=torch.int64, device=DEV)
    out_f = {k: torch.full((n,), -7.5, dtype=torch.float64, device=DEV) for k in ('ws', 'blurred', 'stats')}
    drop = torch.full((16,), -12345, dtype=torch.int64, device=DEV)
    check_refusals(t.data_ptr(), x.data_ptr(), y.data_ptr(), p.data_ptr(), depth.data_ptr(), case['N'], 5, 7, out_f['ws'].data_ptr(), n * 8,
                   out_i.data_ptr(), out_f['blurred'].data_ptr(), out_f['stats'].data_ptr(), drop.data_ptr())
    torch.cuda.synchronize()
    assert bool((out_i == -12345).all()) and bool((drop == -12345).all()) and all(bool((b == -7.5).all()) for b in out_f.values())
    for a, src in zip((t, x, y, p, depth), RC.stream(case) + (depth_host,)):
        assert np.array_equal(a.cpu().numpy().view(np.uint8), src.view(np.uint8))
    # the Python layer: a depth on another device, of another type or shape, or with a model that takes none
    from evennicer_slam_amd import _lib as L
    from evennicer_slam_amd import functional as EF
    kw = RC.arguments(case)
    call = lambda model, theta, d: EF.event_cmax_eval(t, x, y, p, 5, 7, kw['calib'], model, theta, 0.0, [1.0], depth=d)     # noqa: E731
    for model, theta, d in (('rigid', kw['theta'], None), ('rigid', kw['theta'], torch.from_numpy(depth_host)), ('rigid', kw['theta'], depth.double()),
                            ('rigid', kw['theta'], depth[:4]), ('rigid', kw['theta'], depth.t()), ('rigid', kw['theta'][:3], depth),
                            ('rotation', [0.1, 0.2, 0.3], depth), ('flow', [1.0, 2.0], depth)):
        with pytest.raises(L.EnslamError):
            call(model, theta, d)


def test_one_evaluation_inside_a_stream_capture():
    """the fixed chain of launches is captured once and replayed over refilled outputs: every time the bits of the eager call"""
    from evennicer_slam_amd import functional as EF
    case = _CASES['45x61_N700']
    kw = RC.arguments(case)
    arrays = _device_stream(case)
    depth = torch.from_numpy(kw['depth']).to(DEV)
    eager = _run(case, arrays, depth)
    args = (*arrays, kw['H'], kw['W'], kw['calib'], 'rigid', kw['theta'], kw['t_ref'], kw['taps'])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                        # warm-up on a side stream, as torch's capture recipe asks
        EF.event_cmax_eval(*args, signed=kw['signed'], want_blurred=True, depth=depth)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = EF.event_cmax_eval(*args, signed=kw['signed'], want_blurred=True, depth=depth)
    for _ in range(3):                                                    # (the third replay is not the second: see the zero kernel)
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
    for seed in RC.REC_SEEDS[:2]:
        host = EventStream(*RC.planted_stream(seed))
        kw = dict(H=CC.REC_H, W=CC.REC_W, sigma=CC.SIGMA, ksize=CC.REC_K, t_ref=CC.REC_WINDOW / 2, theta0=RC.rec_theta0(seed))
        cpu = M.estimate_motion(host, CC.REC_CALIB, 'rigid', depth=depth, **kw)
        dev = M.estimate_motion(host.to(DEV), CC.REC_CALIB, 'rigid', depth=depth.to(DEV), **kw)
        assert dev['thetas'] == cpu['thetas'] and dev['trace'] == cpu['trace'] and dev['evals'] == cpu['evals'] and len(cpu['trace']) > 3
        f, grad = M.contrast(host.to(DEV), CC.REC_CALIB, 'rigid', cpu['theta'], CC.REC_H, CC.REC_W, t_ref=kw['t_ref'], ksize=CC.REC_K,
                             depth=depth.to(DEV))
        assert f == cpu['trace'][-1] and grad.shape == (6,)
        img, blurred, dropped = M.warp_image(host.to(DEV), CC.REC_CALIB, 'rigid', cpu['theta'], CC.REC_H, CC.REC_W, t_ref=kw['t_ref'],
                                             ksize=CC.REC_K, depth=depth.to(DEV), with_dropped=True)
        img_c, blurred_c, dropped_c = M.warp_image(host, CC.REC_CALIB, 'rigid', cpu['theta'], CC.REC_H, CC.REC_W, t_ref=kw['t_ref'],
                                                   ksize=CC.REC_K, depth=depth, with_dropped=True)
        assert img.device.type == 'cuda' and torch.equal(img.cpu(), img_c) and torch.equal(_bits(blurred.cpu()), _bits(blurred_c))
        assert dropped == dropped_c and set(dropped) == set(M.DROPPED_RIGID)


def test_the_prior_through_slam_track(tmp_path_factory):
    """Five frames of the simulated demo sequence, tracking.iters = 0: under 'cmax' the tracker starts from the pose recomposed
    here from estimate_motion and relative_motion -- on the device, and bit for bit what the CPU route composes -- and under
    'const_speed' from the parent's."""
    from evennicer_slam_amd import event_cmax as M
    from evennicer_slam_amd.slam import SLAM
    from tests.test_event_cmax_rigid_cpu import N_FRAMES, const_speed, demo_sequence, recomposed, with_prior
    root = tmp_path_factory.mktemp('prior')
    cfg, ds, poses, streams, stamps = demo_sequence(tmp_path_factory.mktemp('seq'), device=DEV)
    assert ds.event_slice(2)[0].device.type == 'cuda'

    def harness(c, tag):
        slam = SLAM(c, ds, str(root / tag), device=DEV, static_shapes=True)
        for i in range(N_FRAMES):
            slam.estimate_c2w_list[i] = ds[i][-1].cpu()
        slam._last_rgbd = (0, ds[0][2])
        return slam

    track = lambda slam, idx: slam.track(idx, None, None, None, None, None, rgbd=False).cpu()     # noqa: E731  (no loss: est itself)
    plain, slam = harness(with_prior(cfg, 'const_speed'), 'plain'), harness(with_prior(cfg, 'cmax'), 'cmax')
    used = 0
    for idx in (2, 3, 4):
        want = torch.eye(4)
        want[:3] = const_speed(plain, idx, DEV)[:3].cpu()
        assert torch.equal(track(plain, idx), want)
        got = track(slam, idx)
        est, res = recomposed(slam, ds, idx)
        # the CPU route on the same interval and the same depth follows the same trace
        stream, t0, t1 = ds.event_slice(idx)
        host = M.estimate_motion(stream.to('cpu'), (slam.fx, slam.fy, slam.cx, slam.cy), 'rigid', slam.H, slam.W, theta0=res['thetas'][0],
                                 t_ref=t0, iters=slam.cmax_iters, depth=slam_depth(slam, idx).cpu())
        assert host['thetas'] == res['thetas'] and host['trace'] == res['trace']
        if res['trace'][-1] > res['trace'][0]:
            assert torch.equal(got[:3], est[:3].cpu()) and not torch.equal(got[:3], want[:3])
            used += 1
        else:
            assert torch.equal(got[:3], want[:3])
    st = slam.motion_prior_stats
    assert used >= 2 and st['cmax'] == used and st['no_rise'] == 3 - used and st['few_events'] == st['not_finite'] == st['no_depth'] == 0
    assert plain.motion_prior_stats['cmax'] == 0 and plain.motion_prior_stats['seconds'] == 0.0


def slam_depth(slam, idx):
    """the depth image the prior of frame idx warps the events under"""
    from evennicer_slam_amd import functional as EF
    src, depth = slam._last_rgbd
    m = EF.relative_camera_matrix(slam.estimate_c2w_list[src], slam.estimate_c2w_list[idx - 1].double())
    return EF.depth_forecast(depth.float().contiguous(), slam.cam, m, (slam.H, slam.W), radius=slam.forecast_radius, z_near=0.0,
                             fill=slam.forecast_fill)


def test_a_short_run_keeps_the_last_depth_and_reports_the_prior(tmp_path_factory):
    """slam.run under the dense schedule with the prior on: the last RGB-D frame's depth is kept for it, every tracked frame is
    counted once, and the result carries the counters"""
    from evennicer_slam_amd.slam import SLAM
    from tests.test_event_cmax_rigid_cpu import demo_sequence, with_prior
    cfg, ds, poses, streams, stamps = demo_sequence(tmp_path_factory.mktemp('seq'), device=DEV)
    cfg = with_prior(cfg, 'cmax')
    cfg['mapping'] = dict(cfg['mapping'], iters_first=5, iters=2)
    slam = SLAM(cfg, ds, str(tmp_path_factory.mktemp('run')), device=DEV, static_shapes=True)
    res = slam.run(max_frames=4, tracking_iters=0)
    st = res['motion_prior']
    assert slam._last_rgbd[0] == 3 and st == slam.motion_prior_stats
    assert st['cmax'] + st['few_events'] + st['no_depth'] + st['not_finite'] + st['no_rise'] == 3 and st['no_depth'] == 0
    assert bool(torch.isfinite(slam.estimate_c2w_list[:4]).all())
