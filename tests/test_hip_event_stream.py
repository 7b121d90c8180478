"""-m gpu: csrc/event_stream.hip -- the count / emit kernels behind event_sim.EventSimulator(..., stamps=...) on a HIP device
and the accumulator behind event_stream.accumulate -- against the scalar yardstick tests/event_stream_numpy.py on the cases of
tests/event_stream_cases.py.

Emit: grey images (host table) and host-computed levels are bit-equal in t, x, y, p, the 345-event pixel and an all-quiet
interval included; RGB through the kernel's log and the analytic room follow the existing count rules (at most 0.1 % of the
pixels, by one event / the margin rule) and keep every compared time stamp within the derived bound of
tests/event_stream_cases.py.  The uint8 image and L_ref are bit-equal to the existing enslam_event_sim_* entry on the same
inputs; two runs are bit-identical.  Accumulator: every case bit-equal to the yardstick with its counters, shuffled equal to
sorted, the round trip on the device.  The ABI refusals return their codes without a launch."""
import ctypes

import numpy as np
import pytest
import torch

from tests import event_sim_cases as C
from tests import event_sim_numpy as Y
from tests import event_stream_cases as SC
from tests.viz_cases import CAM

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def _sim(c, H, W):
    from evennicer_slam_amd.event_sim import EventSimulator
    return EventSimulator(H, W, c_pos=c['c_pos'], c_neg=c['c_neg'], sigma_c=c.get('sigma_c', 0.0), substeps=c['K'], eps=C.EPS,
                          seed=c.get('seed', 0), device=DEV)


def _image_ref(name, sim):
    if C.image_cases()[name]['sigma_c'] > 0:
        return SC.image_stream_reference(name, sim.c_pos_map.cpu().numpy(), sim.c_neg_map.cpu().numpy())
    return SC.image_stream_reference(name)


@pytest.mark.parametrize("name", sorted(C.image_cases()))
def test_emit_images_is_bit_equal(name):
    """grey through the host table, RGB through host-computed levels: no device log decides, so everything is bit-equal"""
    from evennicer_slam_amd import event_stream as ES
    c = C.image_cases()[name]
    sim, plain = _sim(c, *c['shape']), _sim(c, *c['shape'])
    ref = _image_ref(name, sim)
    host_log = c['channels'] == 3
    sim.reset(c['images'][0], host_log=host_log)
    plain.reset(c['images'][0], host_log=host_log)
    H, W = c['shape']
    for i, (prev, cur) in enumerate(zip(c['images'][:-1], c['images'][1:])):
        r = ref[i]
        events, stream = sim.step_images(prev, cur, host_log=host_log, stamps=r['stamps'])
        assert stream.device.type == 'cuda' and events.device.type == 'cuda'
        t, x, y, p = stream.numpy()
        print(f"{name} interval {i}: {t.size} events, {int((t != r['t']).sum()) if t.size == r['t'].size else 'other count of'} stamps differ")
        assert t.dtype == np.float64 and x.dtype == np.uint16 and y.dtype == np.uint16 and p.dtype == np.uint8
        assert np.array_equal(t, r['t']) and np.array_equal(x, r['x']) and np.array_equal(y, r['y']) and np.array_equal(p, r['p'])
        # the image and L_ref: the existing entry's on the same inputs, and the yardstick's
        assert torch.equal(events, plain.step_images(prev, cur, host_log=host_log)) and torch.equal(sim.state, plain.state)
        assert np.array_equal(events.cpu().numpy(), r['events']) and np.array_equal(sim.state.cpu().numpy(), r['ref'])
        # the round trip on the device
        counts, dropped = ES.accumulate(stream, [r['stamps'][0] - 1.0, r['stamps'][1]], H, W, with_dropped=True)
        assert counts.device.type == 'cuda' and torch.equal(counts[0], events) and dropped == (0, 0)
        assert torch.equal(ES.accumulate(stream.time_sorted(), [r['stamps'][0] - 1.0, r['stamps'][1]], H, W)[0], events)
    if name == "37x53_grey_K5":
        assert int(ref[0]['total'][0, 0]) == 345                # the saturating pixel's run is in the stream in full
    # an all-quiet interval: the same image twice.  N = 0, nothing to emit, the state stays
    before = sim.state.clone()
    events, stream = sim.step_images(c['images'][-1], c['images'][-1], host_log=host_log, stamps=SC.stamps(3))
    if not bool(events.any()):
        assert len(stream) == 0 and torch.equal(sim.state, before)
    assert len(stream) == int(events.sum()) or bool((events == 255).any())


def test_all_quiet_interval_emits_nothing():
    c = C.image_cases()["37x53_grey_K5"]
    sim = _sim(dict(c, c_pos=0.2, c_neg=0.2), *c['shape']).reset(c['images'][0])
    before = sim.state.clone()
    events, stream = sim.step_images(c['images'][0], c['images'][0], stamps=(1.0, 2.0))
    assert len(stream) == 0 and not bool(events.any()) and torch.equal(sim.state, before)
    assert all(a.device.type == 'cuda' and a.numel() == 0 for a in stream.arrays())


@pytest.mark.parametrize("name", sorted(n for n, c in C.image_cases().items() if c['channels'] == 3))
def test_emit_images_in_kernel_log(name):
    """RGB with luminance and log in the kernel: counts as the existing rule allows (within 1, at most 0.1 % of the pixels),
    every stamp of the other pixels within the derived bound; image and L_ref bit-equal to the existing entry."""
    c = C.image_cases()[name]
    sim, plain = _sim(c, *c['shape']), _sim(c, *c['shape'])
    ref = _image_ref(name, sim)
    imgs = [torch.from_numpy(im).to(DEV) for im in c['images']]
    sim.reset(imgs[0])
    plain.reset(imgs[0])
    H, W = c['shape']
    for i, (prev, cur) in enumerate(zip(imgs[:-1], imgs[1:])):
        r = ref[i]
        events, stream = sim.step_images(prev, cur, stamps=r['stamps'])
        assert torch.equal(events, plain.step_images(prev, cur)) and torch.equal(sim.state, plain.state)
        out = SC.compare_streams(r, stream.numpy(), (H, W))
        print(f"{name} interval {i}: {len(stream)} events, {out}")
        assert out['max_count_diff'] <= 1 and out['differ'] <= C.LOG_PATH_MAX_DIFF_SHARE * H * W
        assert out['polarity_ok'] and out['worst'] <= 1.0


@pytest.mark.parametrize("name", sorted(C.ANALYTIC))
def test_emit_analytic_route(name):
    from evennicer_slam_amd import event_stream as ES
    c, ref, frames, room = C.ANALYTIC[name], SC.analytic_stream_reference(name), C.analytic_poses(name), C.demo_room()
    kw = dict(c_pos=c['c'], c_neg=c['c'], K=c['K'])
    sim, plain = _sim(kw, CAM['H'], CAM['W']), _sim(kw, CAM['H'], CAM['W'])
    sim.reset((room, frames[0], CAM))
    plain.reset((room, frames[0], CAM))
    for i, r in enumerate(ref):
        events, stream = sim.step_scene(room, frames[i], frames[i + 1], CAM, stamps=r['stamps'])
        assert torch.equal(events, plain.step_scene(room, frames[i], frames[i + 1], CAM)) and torch.equal(sim.state, plain.state)
        keep = ~r['left_out']
        out = SC.compare_streams(r, stream.numpy(), (CAM['H'], CAM['W']), keep=keep)
        print(f"{name} interval {i}: {len(stream)} events, {int((~keep).sum())} pixels left out, {out}")
        assert int((~keep).sum()) <= C.MAX_LEFT_OUT * keep.size
        assert out['differ'] == 0 and out['polarity_ok'] and out['worst'] <= 1.0 and out['compared'] > 0
        t = stream.numpy()[0]
        assert bool(np.all((t >= r['stamps'][0]) & (t <= r['stamps'][1])))
        assert torch.equal(ES.accumulate(stream, [r['stamps'][0] - 1.0, r['stamps'][1]], CAM['H'], CAM['W'])[0], events)


def test_two_runs_are_bit_identical():
    runs = []
    for _ in range(2):
        out = []
        ic = C.image_cases()["37x53_rgb_K5_maps"]
        sim = _sim(ic, *ic['shape']).reset(ic['images'][0])
        for i, (a, b) in enumerate(zip(ic['images'][:-1], ic['images'][1:])):
            ev, st = sim.step_images(a, b, stamps=SC.stamps(i))
            out += [ev, *st.arrays()]
        name = "silhouette_K4"
        c, frames, room = C.ANALYTIC[name], C.analytic_poses(name), C.demo_room()
        sim = _sim(dict(c_pos=c['c'], c_neg=c['c'], K=c['K']), CAM['H'], CAM['W']).reset((room, frames[0], CAM))
        for i in range(len(frames) - 1):
            ev, st = sim.step_scene(room, frames[i], frames[i + 1], CAM, stamps=SC.stamps(i))
            out += [ev, *st.arrays(), sim.state.clone()]
        runs.append(out)
    assert len(runs[0]) == len(runs[1]) and all(a.shape == b.shape and torch.equal(a.view(torch.uint8), b.view(torch.uint8))
                                                for a, b in zip(*runs))
    assert sum(a.numel() for a in runs[0]) > 10000


@pytest.mark.parametrize("name", sorted(SC.accumulate_cases()))
def test_accumulate_is_bit_equal(name):
    from evennicer_slam_amd import event_stream as ES
    c = SC.accumulate_cases()[name]
    counts, full, d_time, d_sensor = SC.accumulate_reference(name)
    stream = ES.EventStream(c['t'], c['x'], c['y'], c['p']).to(DEV)
    got, got_full, dropped = ES.accumulate(stream, c['edges'], c['H'], c['W'], want_unsaturated=True, with_dropped=True)
    assert got.device.type == 'cuda' and got.dtype == torch.uint8 and got_full.dtype == torch.uint32
    assert tuple(got.shape) == tuple(got_full.shape) == (c['B'], c['H'], c['W'], 2)
    print(f"{name}: binned {int(full.sum())}, dropped {dropped}, yardstick ({d_time}, {d_sensor})")
    assert np.array_equal(got.cpu().numpy(), counts) and np.array_equal(got_full.cpu().numpy().astype(np.int64), full)
    assert dropped == (d_time, d_sensor)
    shuffled = ES.accumulate(stream.take(torch.from_numpy(c['shuffled'])), c['edges'], c['H'], c['W'], want_unsaturated=True,
                             with_dropped=True)
    assert torch.equal(shuffled[0], got) and torch.equal(shuffled[1].view(torch.uint8), got_full.view(torch.uint8))
    assert shuffled[2] == dropped
    again = ES.accumulate(stream, c['edges'], c['H'], c['W'])
    assert torch.equal(again, got)


def test_accumulate_in_chunks_and_long_edges(monkeypatch):
    """the wrapper's split over the bins (forced small here) and edges too many for LDS give the same result"""
    from evennicer_slam_amd import event_stream as ES
    from evennicer_slam_amd import functional as EF
    name = "N70001_B65"
    c = SC.accumulate_cases()[name]
    counts, full, d_time, d_sensor = SC.accumulate_reference(name)
    stream = ES.EventStream(c['t'], c['x'], c['y'], c['p']).to(DEV)
    monkeypatch.setattr(EF, 'EVENT_ACCUMULATE_MAX_CELLS', 7 * c['H'] * c['W'])                   # ten calls, the last one short
    got, got_full, dropped = ES.accumulate(stream, c['edges'], c['H'], c['W'], want_unsaturated=True, with_dropped=True)
    assert np.array_equal(got.cpu().numpy(), counts) and np.array_equal(got_full.cpu().numpy().astype(np.int64), full)
    assert dropped == (d_time, d_sensor)
    monkeypatch.undo()
    # 2100 bins on a 2 x 3 sensor: the edges are searched in global memory
    rng = np.random.default_rng(9)
    B, n = 2100, 5000
    edges = np.arange(B + 1, dtype=np.float64) * 0.001
    t = rng.uniform(-0.01, edges[-1] + 0.01, n)
    t[:3] = edges[0], edges[1000], edges[-1]
    s = ES.EventStream(t, rng.integers(0, 3, n), rng.integers(0, 2, n), rng.integers(0, 2, n))
    want = ES.accumulate(s, edges, 2, 3, want_unsaturated=True, with_dropped=True)              # the numpy route, checked on the CPU
    have = ES.accumulate(s.to(DEV), edges, 2, 3, want_unsaturated=True, with_dropped=True)
    assert torch.equal(have[0].cpu(), want[0]) and np.array_equal(have[1].cpu().numpy().astype(np.int64), want[1].numpy())
    assert have[2] == want[2]


@pytest.mark.parametrize("prepare", ["host", "device"])
def test_reader_option_on_the_device(tmp_path, prepare):
    """`data.event_stream` + `data.frame_stamps` with the dataset on the HIP device: the stream is sorted, sliced and accumulated
    there, and the items equal those of the png folder written from the simulator's count images, on both preparation routes."""
    import os
    import types
    from evennicer_slam_amd import datasets as D
    from tests.test_event_stream_cpu import _demo_recording
    r = _demo_recording(tmp_path)
    args = types.SimpleNamespace(input_folder=None, event_folder=None)
    data = {'input_folder': r['inp'], 'prepare': prepare}
    from_png = D.get_dataset({'dataset': 'rpg_event', 'cam': r['cam'], 'data': dict(data, event_folder=r['evf'])}, args, 1.0, device=DEV)
    keys = dict(event_stream=os.path.join(r['root'], 'events.txt'), frame_stamps=os.path.join(r['root'], 'images.txt'))
    from_stream = D.get_dataset({'dataset': 'rpg_event', 'cam': r['cam'], 'data': dict(data, **keys)}, args, 1.0, device=DEV)
    assert from_stream._stream.device.type == 'cuda' and len(from_stream) == len(from_png) == r['n']
    for i in range(r['n']):
        a, b = from_png[i], from_stream[i]
        assert all(u.device.type == 'cuda' and torch.equal(u, v) for u, v in zip(a[1:], b[1:]))
        assert bool(b[3].any()) == (i > 0)
        if i:
            assert np.array_equal(b[3].cpu().numpy().astype(np.uint8), r['images'][i - 1])


def test_argument_checks():
    from evennicer_slam_amd import functional as EF
    from evennicer_slam_amd._lib import EnslamError
    H, W = 4, 5
    img = torch.zeros((H, W), dtype=torch.uint8, device=DEV)
    state = torch.full((H, W), float(Y.table(C.EPS)[0]), dtype=torch.float64, device=DEV)
    lut = torch.from_numpy(Y.table(C.EPS)).to(DEV)
    events, (t, x, y, p) = EF.event_stream_images(img, img, state, (0.0, 1.0), lut=lut)
    assert not bool(events.any()) and t.numel() == 0
    for kw in (dict(stamps=(1.0, 0.0)), dict(stamps=(0.0, float('inf'))), dict(stamps=1.0), dict(prev=img.cpu()), dict(lut=None),
               dict(state=state.cpu()), dict(substeps=65), dict(c_pos=0.0)):
        args = dict(prev=img, cur=img, state=state, stamps=(0.0, 1.0), lut=lut)
        args.update(kw)
        with pytest.raises(EnslamError):
            EF.event_stream_images(**args)
    cam, room = dict(CAM, H=H, W=W), C.demo_room()
    for kw in (dict(poses=np.eye(4)[None]), dict(poses=np.tile(np.eye(4, dtype=np.float32), (3, 1, 1))), dict(stamps=(2.0, 1.0)),
               dict(state=state.cpu())):
        args = dict(room=room, poses=np.tile(np.eye(4), (3, 1, 1)), cam=cam, state=state, stamps=(0.0, 1.0))
        args.update(kw)
        with pytest.raises(EnslamError):
            EF.event_stream_boxroom(**args)
    z = dict(t=torch.zeros(3, dtype=torch.float64, device=DEV), x=torch.zeros(3, dtype=torch.uint16, device=DEV),
             y=torch.zeros(3, dtype=torch.uint16, device=DEV), p=torch.zeros(3, dtype=torch.uint8, device=DEV))
    for kw in (dict(t=z['t'].cpu()), dict(x=z['x'][:2]), dict(p=z['p'].float()), dict(edges=[1.0, 0.0]), dict(edges=[0.0]), dict(H=0)):
        args = dict(z, edges=[0.0, 1.0], H=H, W=W)
        args.update(kw)
        with pytest.raises(EnslamError):
            EF.event_accumulate(**args)


def test_abi_errors_return_without_launching():
    from evennicer_slam_amd import _lib as L
    from evennicer_slam_amd import functional as EF
    lib = L.lib()
    H, W, K = 4, 5, 2
    cam, room = dict(CAM, H=H, W=W), C.demo_room()
    img = torch.zeros((H, W, 3), dtype=torch.uint8, device=DEV)
    lut = torch.from_numpy(Y.table(C.EPS)).to(DEV)
    state = torch.full((H, W), -7.0, dtype=torch.float64, device=DEV)
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

    def ptr(a):
        return a.data_ptr() if a is not None else None

    def icount(q, prev=img, cur=img, s=state, c=cnt):
        return lib.enslam_event_stream_images_count(ctypes.byref(q) if q is not None else None, ptr(prev), ptr(cur), ptr(lut), None, None,
                                                    None, None, ptr(s), ptr(c), None)

    def iemit(q, prev=img, s=state, e=ev, en=ends, total=0, t_a=0.0, t_b=1.0, t=st['t'], x=st['x']):
        return lib.enslam_event_stream_images_emit(ctypes.byref(q) if q is not None else None, ptr(prev), ptr(img), ptr(lut), None, None,
                                                   None, None, ptr(s), ptr(e), ptr(en), total, t_a, t_b, ptr(t), ptr(x), ptr(st['y']),
                                                   ptr(st['p']), None)

    def bcount(q, ps=poses, s=state, c=cnt):
        return lib.enslam_event_stream_boxroom_count(ctypes.byref(q) if q is not None else None, ptr(ps), None, None, ptr(s), ptr(c), None)

    def bemit(q, ps=poses, s=state, e=ev, en=ends, total=0, t_a=0.0, t_b=1.0, t=st['t']):
        return lib.enslam_event_stream_boxroom_emit(ctypes.byref(q) if q is not None else None, ptr(ps), None, None, ptr(s), ptr(e),
                                                    ptr(en), total, t_a, t_b, ptr(t), ptr(st['x']), ptr(st['y']), ptr(st['p']), None)

    inval = [icount(None), icount(plan(), prev=None), icount(plan(), s=None), icount(plan(), c=None), icount(plan(init=1)),
             icount(plan(K=0)), icount(plan(channels=2)), icount(plan(c_pos=0.0)),
             iemit(None), iemit(plan(), prev=None), iemit(plan(), s=None), iemit(plan(), e=None), iemit(plan(), en=None),
             iemit(plan(), total=-1), iemit(plan(), total=4, t=None), iemit(plan(), total=4, x=None), iemit(plan(init=1)),
             iemit(plan(), t_a=1.0, t_b=0.5), iemit(plan(), t_b=float('inf')), iemit(plan(), t_a=float('nan')), iemit(plan(H=0)),
             bcount(None), bcount(plan(), ps=None), bcount(plan(), s=None), bcount(plan(), c=None), bcount(plan(init=1)),
             bcount(plan(fx=0.0)),
             bemit(None), bemit(plan(), ps=None), bemit(plan(), e=None), bemit(plan(), en=None), bemit(plan(), total=-2),
             bemit(plan(), total=3, t=None), bemit(plan(), t_a=2.0, t_b=1.0), bemit(plan(init=1)), bemit(plan(eps=0.0))]
    assert inval == [-1] * len(inval)
    kmax = lib.enslam_event_sim_max_substeps()
    unsupported = [iemit(plan(), total=2 ** 31), bemit(plan(), total=2 ** 31), icount(plan(K=kmax + 1)), bcount(plan(K=kmax + 1)),
                   icount(plan(W=65537)), iemit(plan(H=65537)), iemit(plan(H=1 << 15, W=1 << 14))]
    assert unsupported == [-3] * len(unsupported)

    # the accumulator
    acc = torch.full((2 * H * W * 2,), 7, dtype=torch.int32, device=DEV)
    out = torch.full((2 * H * W * 2 + 2,), 9, dtype=torch.uint8, device=DEV)
    drop = torch.full((2,), -3, dtype=torch.int64, device=DEV)
    edges = np.array([0.0, 1.0, 2.0])
    edges_dev = torch.from_numpy(edges).to(DEV)

    def accumulate(t=st['t'], x=st['x'], N=8, host=edges, dev=edges_dev, B=2, h=H, w=W, a=acc, o=out, d=drop, odd=0):
        hp = host.ctypes.data_as(ctypes.POINTER(ctypes.c_double)) if host is not None else None
        return lib.enslam_event_accumulate(ptr(t), ptr(x), ptr(st['y']), ptr(st['p']), N, hp, ptr(dev), B, h, w, ptr(a),
                                           (ptr(o) + odd) if o is not None else None, ptr(d), None)

    inval = [accumulate(t=None), accumulate(x=None), accumulate(N=-1), accumulate(host=None), accumulate(dev=None), accumulate(a=None),
             accumulate(o=None), accumulate(d=None), accumulate(B=0), accumulate(h=0), accumulate(w=-1), accumulate(odd=1),
             accumulate(host=np.array([0.0, 2.0, 1.0])), accumulate(host=np.array([1.0, 0.0, 2.0])),
             accumulate(host=np.array([0.0, np.nan, 2.0]))]
    assert inval == [-1] * len(inval)
    unsupported = [accumulate(N=2 ** 31), accumulate(h=1 << 16, w=1 << 15)]
    assert unsupported == [-3] * len(unsupported)
    torch.cuda.synchronize()
    # nothing ran
    assert bool((state == -7.0).all()) and bool((ev == 9).all()) and bool((cnt == -5).all()) and bool((st['t'] == -1.0).all())
    assert bool((acc == 7).all()) and bool((out == 9).all()) and bool((drop == -3).all())
    # the valid neighbours: N = 0 clears the outputs without an event launch; equal edges and -inf are accepted
    assert accumulate(N=0, t=None, x=None) == 0
    torch.cuda.synchronize()
    assert bool((acc == 0).all()) and bool((out[:-2] == 0).all()) and bool((out[-2:] == 9).all()) and bool((drop == 0).all())
    assert accumulate(host=np.array([-np.inf, 1.0, 1.0]), dev=torch.tensor([-np.inf, 1.0, 1.0], dtype=torch.float64, device=DEV)) == 0
    torch.cuda.synchronize()
    assert drop.tolist() == [0, 8] and bool((acc == 0).all())   # the eight events sit at x = y = 9, outside the 4 x 5 sensor
    # count, then emit with total = 0 and NULL arrays on a quiet pixel grid: valid, and only the image and L_ref are written
    state.copy_(torch.from_numpy(Y.level_of_image(np.zeros((H, W, 3), dtype=np.uint8), C.EPS)))
    kept = state.clone()
    assert icount(plan()) == 0 and bcount(plan(c_pos=50.0, c_neg=50.0)) == 0
    torch.cuda.synchronize()
    assert bool((cnt == 0).all())
    assert iemit(plan(), total=0, t=None, x=None) == 0
    torch.cuda.synchronize()
    assert bool((ev == 0).all()) and torch.equal(state, kept) and bool((st['t'] == -1.0).all())
