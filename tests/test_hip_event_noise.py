"""-m gpu: csrc/event_noise.hip -- the count / image / emit kernels behind event_sim.EventSimulator(..., noise=EventNoise(...)) on a
HIP device -- against the scalar yardstick tests/event_noise_numpy.py on the cases and settings of tests/event_noise_cases.py.

Grey images (host table) and host-computed levels: image, L_ref, t_last, counts and every stream field bit-equal on all
settings.  RGB through the kernel's log and the analytic room: the pixels the rules of tests/event_noise_cases.py leave out
(at most 0.1 %) aside, RGB pixels may differ in count as the existing rule allows (at most LOG_PATH_MAX_DIFF_SHARE of them),
analytic ones not at all, and all others are compared event by event with `compare_streams`.  The count pass equals the
histogram of the emit pass, the one-launch form the two-launch form, two runs are bit-identical, the device accumulator
returns the image from the stream, `off` equals enslam_event_stream_*_emit to the bit, and the ABI refusals return their
codes without a launch."""
import ctypes

import numpy as np
import pytest
import torch

from tests import event_noise_cases as NC
from tests import event_sim_cases as C
from tests import event_sim_numpy as Y
from tests import event_stream_cases as SC
from tests.viz_cases import CAM

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SETTINGS = sorted(NC.SETTINGS)


def _sim(c, H, W, setting):
    from evennicer_slam_amd.event_sim import EventNoise, EventSimulator
    noise = None if setting is None else EventNoise(**NC.SETTINGS[setting])
    return EventSimulator(H, W, c_pos=c['c_pos'], c_neg=c['c_neg'], sigma_c=c.get('sigma_c', 0.0), substeps=c['K'], eps=C.EPS,
                          seed=c.get('seed', 0), device=DEV, noise=noise)


def _image_ref(name, setting, sim):
    if C.image_cases()[name]['sigma_c'] > 0:
        return NC.image_noise_reference(name, setting, sim.c_pos_map.cpu().numpy(), sim.c_neg_map.cpu().numpy())
    return NC.image_noise_reference(name, setting)


def _bit_equal(r, events, sim, stream):
    t, x, y, p = stream.numpy()
    assert t.dtype == np.float64 and x.dtype == np.uint16 and y.dtype == np.uint16 and p.dtype == np.uint8
    return (np.array_equal(events.cpu().numpy(), r['events']) and np.array_equal(sim.state.cpu().numpy(), r['ref'])
            and np.array_equal(sim.last_event_time.cpu().numpy(), r['t_last']) and np.array_equal(t, r['t'])
            and np.array_equal(x, r['x']) and np.array_equal(y, r['y']) and np.array_equal(p, r['p']))


@pytest.mark.parametrize("setting", SETTINGS)
@pytest.mark.parametrize("name", NC.IMAGE_NAMES)
def test_images_are_bit_equal(name, setting):
    """grey through the host table, RGB through host-computed levels: no device log decides, so everything is bit-equal.  Also
    the one-launch form, the count pass against the emit pass, and the round trip through the device accumulator."""
    from evennicer_slam_amd import event_stream as ES
    c = C.image_cases()[name]
    sim, image_only = _sim(c, *c['shape'], setting), _sim(c, *c['shape'], setting)
    ref = _image_ref(name, setting, sim)
    host_log = c['channels'] == 3
    sim.reset(c['images'][0], host_log=host_log)
    image_only.reset(c['images'][0], host_log=host_log)
    H, W = c['shape']
    for i, (prev, cur) in enumerate(zip(c['images'][:-1], c['images'][1:])):
        r = ref[i]
        events, stream = sim.step_images(prev, cur, host_log=host_log, stamps=r['stamps'])
        assert stream.device.type == 'cuda' and events.device.type == 'cuda'
        t = stream.numpy()[0]
        print(f"{name} {setting} interval {i}: {t.size} events ({r['t'].size} in the yardstick), "
              f"{int((t != r['t']).sum()) if t.size == r['t'].size else 'other count of'} stamps differ")
        assert _bit_equal(r, events, sim, stream)
        # the count pass: the per-pixel histogram of the emitted stream, and the yardstick's totals
        x, y = stream.numpy()[1:3]
        assert np.array_equal(np.bincount(y.astype(np.int64) * W + x, minlength=H * W).reshape(H, W), r['total'])
        # one launch: the same image and the same two states
        assert torch.equal(image_only.step_images(prev, cur, host_log=host_log, stamps=r['stamps'], stream=False), events)
        assert torch.equal(image_only.state, sim.state) and torch.equal(image_only.last_event_time.view(torch.int64),
                                                                        sim.last_event_time.view(torch.int64))
        counts, dropped = ES.accumulate(stream, [r['stamps'][0] - 1.0, r['stamps'][1]], H, W, with_dropped=True)
        assert counts.device.type == 'cuda' and torch.equal(counts[0], events) and dropped == (0, 0)


@pytest.mark.parametrize("name", NC.IMAGE_NAMES)
def test_off_equals_the_stream_entries(name):
    """all parameters zero: image, L_ref and stream of enslam_event_noisy_* equal enslam_event_stream_*_emit's to the bit, on
    the in-kernel log as well (both run the same device function)"""
    c = C.image_cases()[name]
    sim, plain = _sim(c, *c['shape'], 'off'), _sim(c, *c['shape'], None)
    imgs = [torch.from_numpy(im).to(DEV) for im in c['images']]
    sim.reset(imgs[0])
    plain.reset(imgs[0])
    for i, (prev, cur) in enumerate(zip(imgs[:-1], imgs[1:])):
        events, stream = sim.step_images(prev, cur, stamps=SC.stamps(i))
        want, want_stream = plain.step_images(prev, cur, stamps=SC.stamps(i))
        assert torch.equal(events, want) and torch.equal(sim.state.view(torch.int64), plain.state.view(torch.int64))
        assert len(stream) == len(want_stream)
        assert all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(stream.arrays(), want_stream.arrays()))


def _count_pass_images(sim, prev, cur, stamps, interval):
    """enslam_event_noisy_images_count alone, on the simulator's current states (which it only reads)"""
    from evennicer_slam_amd import _lib as L
    from evennicer_slam_amd import functional as EF
    H, W = sim.H, sim.W
    channels = 3 if cur.dim() == 3 else 1
    plan = EF.event_sim_plan(H, W, sim.substeps, sim.eps, sim.c_pos, sim.c_neg, channels=channels)
    params = EF.event_noise_params("test", sim.noise.params(interval), sim.substeps, stamps)
    counts = torch.full((H, W), -1, dtype=torch.int64, device=DEV)
    ptr = lambda a: None if a is None else a.data_ptr()     # noqa: E731
    rc = L.lib().enslam_event_noisy_images_count(ctypes.byref(plan), ptr(prev), ptr(cur), ptr(sim._lut), None, None, ptr(sim.c_pos_map),
                                                 ptr(sim.c_neg_map), ptr(sim.state), ptr(counts), ctypes.byref(params), stamps[0],
                                                 stamps[1], ptr(sim.last_event_time), None)
    assert rc == 0
    return counts


@pytest.mark.parametrize("setting", SETTINGS)
@pytest.mark.parametrize("name", sorted(n for n in NC.IMAGE_NAMES if C.image_cases()[n]['channels'] == 3))
def test_images_in_kernel_log(name, setting):
    """RGB with luminance and log in the kernel: left-out pixels aside, counts as the existing rule allows (within 1 per
    interval's signal, at most 0.1 % of the pixels), every stamp of the other pixels within the derived bound."""
    c = C.image_cases()[name]
    sim = _sim(c, *c['shape'], setting)
    ref = _image_ref(name, setting, sim)
    imgs = [torch.from_numpy(im).to(DEV) for im in c['images']]
    sim.reset(imgs[0])
    H, W = c['shape']
    for i, (prev, cur) in enumerate(zip(imgs[:-1], imgs[1:])):
        r = ref[i]
        before = (sim.state.clone(), sim.last_event_time.clone())
        counts = _count_pass_images(sim, prev, cur, r['stamps'], i)
        assert torch.equal(sim.state, before[0]) and torch.equal(sim.last_event_time, before[1])       # both only read
        events, stream = sim.step_images(prev, cur, stamps=r['stamps'])
        t, x, y, p = stream.numpy()
        assert np.array_equal(np.bincount(y.astype(np.int64) * W + x, minlength=H * W).reshape(H, W), counts.cpu().numpy())
        keep = ~r['left_out']
        out = SC.compare_streams(r, (t, x, y, p), (H, W), keep=keep)
        print(f"{name} {setting} interval {i}: {len(stream)} events, {int((~keep).sum())} pixels left out, {out}")
        assert int((~keep).sum()) <= C.MAX_LEFT_OUT * keep.size
        assert out['differ'] <= C.LOG_PATH_MAX_DIFF_SHARE * H * W
        assert out['polarity_ok'] and out['worst'] <= 1.0


def _count_pass_boxroom(sim, room, poses, stamps, interval):
    """enslam_event_noisy_boxroom_count alone (poses float64 [K+1,4,4], the previous frame's first), on the simulator's current
    states (which it only reads)"""
    from evennicer_slam_amd import _lib as L
    from evennicer_slam_amd import functional as EF
    H, W = sim.H, sim.W
    plan = EF.event_sim_plan(H, W, sim.substeps, sim.eps, sim.c_pos, sim.c_neg, cam=CAM, room=room)
    params = EF.event_noise_params("test", sim.noise.params(interval), sim.substeps, stamps)
    rows = torch.from_numpy(np.ascontiguousarray(np.asarray(poses, dtype=np.float64)[:, :3, :])).to(DEV)
    assert tuple(rows.shape) == (sim.substeps + 1, 3, 4)
    counts = torch.full((H, W), -1, dtype=torch.int64, device=DEV)
    rc = L.lib().enslam_event_noisy_boxroom_count(ctypes.byref(plan), rows.data_ptr(), None, None, sim.state.data_ptr(), counts.data_ptr(),
                                                  ctypes.byref(params), stamps[0], stamps[1], sim.last_event_time.data_ptr(), None)
    assert rc == 0
    return counts


@pytest.mark.parametrize("setting", SETTINGS)
@pytest.mark.parametrize("name", NC.ANALYTIC_NAMES)
def test_analytic_route(name, setting):
    from evennicer_slam_amd import event_stream as ES
    c, ref, frames, room = C.ANALYTIC[name], NC.analytic_noise_reference(name, setting), C.analytic_poses(name), C.demo_room()
    kw = dict(c_pos=c['c'], c_neg=c['c'], K=c['K'])
    sim, image_only = _sim(kw, CAM['H'], CAM['W'], setting), _sim(kw, CAM['H'], CAM['W'], setting)
    sim.reset((room, frames[0], CAM))
    image_only.reset((room, frames[0], CAM))
    H, W = CAM['H'], CAM['W']
    for i, r in enumerate(ref):
        before = (sim.state.clone(), sim.last_event_time.clone())
        counts = _count_pass_boxroom(sim, room, r['poses'], r['stamps'], i)
        assert torch.equal(sim.state, before[0]) and torch.equal(sim.last_event_time, before[1])       # both only read
        events, stream = sim.step_scene(room, frames[i], frames[i + 1], CAM, stamps=r['stamps'])
        x, y = stream.numpy()[1:3]
        assert np.array_equal(np.bincount(y.astype(np.int64) * W + x, minlength=H * W).reshape(H, W), counts.cpu().numpy())
        assert np.array_equal(counts.cpu().numpy()[~r['left_out']], r['total'][~r['left_out']])
        assert torch.equal(image_only.step_scene(room, frames[i], frames[i + 1], CAM, stamps=r['stamps'], stream=False), events)
        assert torch.equal(image_only.state, sim.state) and torch.equal(image_only.last_event_time.view(torch.int64),
                                                                        sim.last_event_time.view(torch.int64))
        keep = ~r['left_out']
        out = SC.compare_streams(r, stream.numpy(), (H, W), keep=keep)
        print(f"{name} {setting} interval {i}: {len(stream)} events, {int((~keep).sum())} pixels left out, {out}")
        assert int((~keep).sum()) <= C.MAX_LEFT_OUT * keep.size
        assert out['differ'] == 0 and out['polarity_ok'] and out['worst'] <= 1.0 and out['compared'] > 0
        assert np.array_equal(events.cpu().numpy()[keep], r['events'][keep])
        t = stream.numpy()[0]
        assert bool(np.all((t >= r['stamps'][0]) & (t <= r['stamps'][1])))
        assert torch.equal(ES.accumulate(stream, [r['stamps'][0] - 1.0, r['stamps'][1]], H, W)[0], events)
    if setting == 'off':
        plain = _sim(kw, H, W, None).reset((room, frames[0], CAM))
        again = _sim(kw, H, W, 'off').reset((room, frames[0], CAM))
        for i in range(len(ref)):
            a = again.step_scene(room, frames[i], frames[i + 1], CAM, stamps=SC.stamps(i))
            b = plain.step_scene(room, frames[i], frames[i + 1], CAM, stamps=SC.stamps(i))
            assert torch.equal(a[0], b[0]) and torch.equal(again.state.view(torch.int64), plain.state.view(torch.int64))
            assert len(a[1]) == len(b[1]) and all(torch.equal(u.view(torch.uint8), v.view(torch.uint8))
                                                  for u, v in zip(a[1].arrays(), b[1].arrays()))


def test_two_runs_are_bit_identical():
    runs = []
    for _ in range(2):
        out = []
        ic = C.image_cases()["37x53_rgb_K5_maps"]
        sim = _sim(ic, *ic['shape'], 'all').reset(ic['images'][0])
        for i, (a, b) in enumerate(zip(ic['images'][:-1], ic['images'][1:])):
            ev, st = sim.step_images(a, b, stamps=SC.stamps(i))
            out += [ev, *st.arrays(), sim.state.clone(), sim.last_event_time.clone()]
        name = "silhouette_K4"
        c, frames, room = C.ANALYTIC[name], C.analytic_poses(name), C.demo_room()
        sim = _sim(dict(c_pos=c['c'], c_neg=c['c'], K=c['K']), CAM['H'], CAM['W'], 'all').reset((room, frames[0], CAM))
        for i in range(len(frames) - 1):
            ev, st = sim.step_scene(room, frames[i], frames[i + 1], CAM, stamps=SC.stamps(i))
            out += [ev, *st.arrays(), sim.state.clone(), sim.last_event_time.clone()]
        runs.append(out)
    assert len(runs[0]) == len(runs[1]) and all(a.shape == b.shape and torch.equal(a.view(torch.uint8), b.view(torch.uint8))
                                                for a, b in zip(*runs))
    assert sum(a.numel() for a in runs[0]) > 10000


def test_walk_cap():
    """A threshold that is tiny against the level change: a sub-step walks at most 65536 candidates of a pixel, the count pass
    reports the cap for that pixel and the stream call refuses the interval; L_ref is the closed form's in the one-launch
    form, and a pixel just below the cap is walked in full."""
    from evennicer_slam_amd import functional as EF
    from evennicer_slam_amd._lib import EnslamError
    H, W = 1, 2
    state = torch.zeros((H, W), dtype=torch.float64, device=DEV)
    t_last = torch.full((H, W), float('-inf'), dtype=torch.float64, device=DEV)
    noise = dict(refractory=0.0, leak_rate=0.0, shot_rate=0.0, seed=0, interval=0)
    kw = dict(substeps=1, c_pos=2.0 ** -10, c_neg=2.0 ** -10)
    levels = (torch.zeros((H, W), dtype=torch.float64, device=DEV), torch.tensor([[64.0, 100.0]], dtype=torch.float64, device=DEV))
    with pytest.raises(EnslamError, match="events in one interval"):        # pixel 1: 102 400 candidates
        EF.event_noisy_images(None, None, state, t_last, (0.0, 1.0), noise, levels=levels, **kw)
    assert bool((state == 0.0).all()) and bool(torch.isneginf(t_last).all())                # the count pass wrote no state
    events = EF.event_noisy_images(None, None, state, t_last, (0.0, 1.0), noise, levels=levels, stream=False, **kw)
    assert events.tolist() == [[[0, 255], [0, 255]]] and state.tolist() == [[64.0, 100.0]]
    state.zero_()
    t_last.fill_(float('-inf'))
    levels[1][0, 1] = 63.0
    events, (t, x, y, p) = EF.event_noisy_images(None, None, state, t_last, (0.0, 1.0), noise, levels=levels, **kw)
    assert t.numel() == 65536 + 64512 and state.tolist() == [[64.0, 63.0]] and t_last.tolist() == [[1.0, 1.0]]


def test_wrapper_checks():
    from evennicer_slam_amd import functional as EF
    from evennicer_slam_amd._lib import EnslamError
    H, W = 4, 5
    img = torch.zeros((H, W), dtype=torch.uint8, device=DEV)
    state = torch.full((H, W), float(Y.table(C.EPS)[0]), dtype=torch.float64, device=DEV)
    t_last = torch.full((H, W), float('-inf'), dtype=torch.float64, device=DEV)
    lut = torch.from_numpy(Y.table(C.EPS)).to(DEV)
    noise = dict(refractory=1e-3, leak_rate=0.0, shot_rate=0.0, seed=0, interval=0)
    events, (t, x, y, p) = EF.event_noisy_images(img, img, state, t_last, (0.0, 1.0), noise, lut=lut)
    assert not bool(events.any()) and t.numel() == 0 and bool(torch.isneginf(t_last).all())
    assert not bool(EF.event_noisy_images(img, img, state, t_last, (0.0, 1.0), noise, lut=lut, stream=False).any())
    for kw in (dict(stamps=(1.0, 0.0)), dict(stamps=1.0), dict(t_last=t_last.cpu()), dict(t_last=t_last.float()), dict(t_last=t_last[:2]),
               dict(noise=dict(noise, refractory=-1.0)), dict(noise=dict(noise, shot_rate=100.0)), dict(noise=dict(noise, seed=-1)),
               dict(noise=dict(noise, interval=1 << 32)), dict(lut=None), dict(substeps=65)):
        args = dict(prev=img, cur=img, state=state, t_last=t_last, stamps=(0.0, 1.0), noise=noise, lut=lut)
        args.update(kw)
        with pytest.raises(EnslamError):
            EF.event_noisy_images(**args)
    cam, room = dict(CAM, H=H, W=W), C.demo_room()
    for kw in (dict(poses=np.eye(4)[None]), dict(stamps=(2.0, 1.0)), dict(t_last=t_last.cpu()), dict(noise=dict(noise, leak_rate=float('nan')))):
        args = dict(room=room, poses=np.tile(np.eye(4), (3, 1, 1)), cam=cam, state=state, t_last=t_last, stamps=(0.0, 1.0), noise=noise)
        args.update(kw)
        with pytest.raises(EnslamError):
            EF.event_noisy_boxroom(**args)


def test_abi_errors_return_without_launching():
    from evennicer_slam_amd import _lib as L
    from evennicer_slam_amd import functional as EF
    lib = L.lib()
    H, W, K = 4, 5, 2
    cam, room = dict(CAM, H=H, W=W), C.demo_room()
    img = torch.zeros((H, W, 3), dtype=torch.uint8, device=DEV)
    lut = torch.from_numpy(Y.table(C.EPS)).to(DEV)
    state = torch.full((H, W), -7.0, dtype=torch.float64, device=DEV)
    last = torch.full((H, W), -3.0, dtype=torch.float64, device=DEV)
    ev = torch.full((H * W * 2,), 9, dtype=torch.uint8, device=DEV)
    cnt = torch.full((H * W,), -5, dtype=torch.int64, device=DEV)
    ends = torch.zeros(H * W, dtype=torch.int64, device=DEV)
    poses = torch.eye(4, dtype=torch.float64, device=DEV)[None, :3].repeat(K + 1, 1, 1).contiguous()
    st = dict(t=torch.full((8,), -1.0, dtype=torch.float64, device=DEV), x=torch.full((8,), 9, dtype=torch.uint16, device=DEV),
              y=torch.full((8,), 9, dtype=torch.uint16, device=DEV), p=torch.full((8,), 9, dtype=torch.uint8, device=DEV))

    def plan(**over):
        q = EF.event_sim_plan(H, W, K, C.EPS, 0.2, 0.2, channels=3, cam=cam, room=room)
        for k, v in over.items():
            setattr(q, k, v)
        return q

    def noise(**over):
        n = L.EventNoiseParams()
        n.refractory, n.leak, n.shot, n.seed, n.interval = 1e-3, 0.1, 0.2, 5, 1
        for k, v in over.items():
            setattr(n, k, v)
        return n

    def ptr(a):
        return a.data_ptr() if a is not None else None

    def ref(a):
        return ctypes.byref(a) if a is not None else None

    def icount(q, n, prev=img, s=state, c=cnt, t_a=0.0, t_b=1.0, tl=last):
        return lib.enslam_event_noisy_images_count(ref(q), ptr(prev), ptr(img), ptr(lut), None, None, None, None, ptr(s), ptr(c), ref(n),
                                                   t_a, t_b, ptr(tl), None)

    def iemit(q, n, prev=img, s=state, e=ev, en=ends, total=0, t_a=0.0, t_b=1.0, t=st['t'], x=st['x'], y=st['y'], p=st['p'], tl=last):
        return lib.enslam_event_noisy_images_emit(ref(q), ptr(prev), ptr(img), ptr(lut), None, None, None, None, ptr(s), ptr(e), ptr(en),
                                                  total, t_a, t_b, ptr(t), ptr(x), ptr(y), ptr(p), ref(n), ptr(tl), None)

    def bcount(q, n, ps=poses, s=state, c=cnt, t_a=0.0, t_b=1.0, tl=last):
        return lib.enslam_event_noisy_boxroom_count(ref(q), ptr(ps), None, None, ptr(s), ptr(c), ref(n), t_a, t_b, ptr(tl), None)

    def bemit(q, n, ps=poses, s=state, e=ev, en=ends, total=0, t_a=0.0, t_b=1.0, t=st['t'], x=st['x'], tl=last):
        return lib.enslam_event_noisy_boxroom_emit(ref(q), ptr(ps), None, None, ptr(s), ptr(e), ptr(en), total, t_a, t_b, ptr(t), ptr(x),
                                                   ptr(st['y']), ptr(st['p']), ref(n), ptr(tl), None)

    inf, nan = float('inf'), float('nan')
    bad_noise = [noise(refractory=-1e-3), noise(refractory=inf), noise(refractory=nan), noise(leak=-0.1), noise(leak=inf), noise(leak=nan),
                 noise(shot=-0.1), noise(shot=nan), noise(shot=inf), noise(shot=1.0 + 2.0 ** -52)]
    inval = []
    for fn in (icount, iemit, bcount, bemit):
        inval += [fn(plan(), None), fn(plan(), noise(), tl=None), fn(None, noise()), fn(plan(), noise(), s=None), fn(plan(init=1), noise()),
                  fn(plan(K=0), noise()), fn(plan(), noise(), t_a=1.0, t_b=0.5), fn(plan(), noise(), t_b=inf), fn(plan(), noise(), t_a=nan)]
        inval += [fn(plan(), n) for n in bad_noise]
    # what the stream entries refuse
    inval += [icount(plan(), noise(), prev=None), icount(plan(), noise(), c=None), icount(plan(channels=2), noise()),
              icount(plan(c_pos=0.0), noise()), bcount(plan(), noise(), ps=None), bcount(plan(), noise(), c=None), bcount(plan(fx=0.0), noise()),
              iemit(plan(), noise(), prev=None), iemit(plan(), noise(), e=None), iemit(plan(), noise(), total=-1),
              iemit(plan(), noise(), total=4, t=None, x=None, y=None, p=None), iemit(plan(H=0), noise()),
              bemit(plan(), noise(), ps=None), bemit(plan(), noise(), e=None), bemit(plan(), noise(), total=-2), bemit(plan(eps=0.0), noise())]
    # only some of the five stream pointers
    inval += [iemit(plan(), noise(), en=None), iemit(plan(), noise(), en=None, t=None, x=None, y=None, p=None, total=3),
              iemit(plan(), noise(), en=None, t=None), iemit(plan(), noise(), t=None), iemit(plan(), noise(), x=None, total=4),
              iemit(plan(), noise(), p=None), bemit(plan(), noise(), en=None), bemit(plan(), noise(), t=None),
              bemit(plan(), noise(), en=None, t=None, x=None)]
    assert inval == [-1] * len(inval)
    kmax = lib.enslam_event_sim_max_substeps()
    unsupported = [iemit(plan(), noise(), total=2 ** 31), bemit(plan(), noise(), total=2 ** 31), icount(plan(K=kmax + 1), noise()),
                   bcount(plan(K=kmax + 1), noise()), icount(plan(W=65537), noise()), iemit(plan(H=65537), noise()),
                   iemit(plan(H=1 << 15, W=1 << 14), noise())]
    assert unsupported == [-3] * len(unsupported)
    torch.cuda.synchronize()
    # nothing ran
    assert bool((state == -7.0).all()) and bool((last == -3.0).all()) and bool((ev == 9).all()) and bool((cnt == -5).all())
    assert bool((st['t'] == -1.0).all())
    # the valid neighbours on a quiet pixel grid without leak or shot noise: q = 1 is accepted; the count pass writes zeros and
    # leaves both states; the one-launch form writes the image and the states only; total = 0 beside `ends` needs no arrays
    state.copy_(torch.from_numpy(Y.level_of_image(np.zeros((H, W, 3), dtype=np.uint8), C.EPS)))
    kept = state.clone()
    quiet = noise(leak=0.0, shot=0.0)
    assert icount(plan(), quiet) == 0
    torch.cuda.synchronize()
    assert bool((cnt == 0).all()) and torch.equal(state, kept) and bool((last == -3.0).all())
    assert iemit(plan(), quiet, en=None, t=None, x=None, y=None, p=None) == 0
    assert iemit(plan(), quiet, t=None, x=None, y=None, p=None) == 0
    torch.cuda.synchronize()
    assert bool((ev == 0).all()) and torch.equal(state, kept) and bool((last == -3.0).all()) and bool((st['t'] == -1.0).all())
    # q = 1: every pixel and sub-step fires both noise events; capacity 8 of the arrays is respected by the guarded stores
    full = noise(refractory=0.0, leak=0.0, shot=1.0)
    assert icount(plan(), full) == 0
    torch.cuda.synchronize()
    assert bool((cnt == 2 * K).all())
    ends.copy_(torch.cumsum(cnt, 0))
    assert iemit(plan(), full, total=8) == 0
    torch.cuda.synchronize()
    assert bool((ev == 2).all()) and torch.equal(state, kept) and bool((st['t'] >= 0.0).all()) and bool((st['t'] <= 1.0).all())
    assert st['x'].tolist() == [0, 0, 0, 0, 1, 1, 1, 1] and st['y'].tolist() == [0] * 8 and sorted(st['p'][:4].tolist()) == [0, 0, 1, 1]
