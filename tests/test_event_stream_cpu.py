"""No GPU: the time-stamped event streams on the CPU -- the numpy route of event_sim.EventSimulator(..., stamps=...), the
numpy route of event_stream.accumulate, the text and .npz forms, frame_edges, tools/events_to_frames.py and the
`data.event_stream` option of the readers -- against the scalar yardstick tests/event_stream_numpy.py on the cases of
tests/event_stream_cases.py."""
import importlib.util
import json
import os
import types

import numpy as np
import pytest
import torch

from tests import event_sim_cases as C
from tests import event_sim_numpy as Y
from tests import event_stream_cases as SC
from tests import event_stream_numpy as YS
from tests.viz_cases import CAM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = types.SimpleNamespace(input_folder=None, event_folder=None)
EXPORTS = ("enslam_event_stream_images_count", "enslam_event_stream_images_emit", "enslam_event_stream_boxroom_count",
           "enslam_event_stream_boxroom_emit", "enslam_event_accumulate")


def _tool(name):
    spec = importlib.util.spec_from_file_location(name + "_tool", os.path.join(ROOT, "tools", name + ".py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    return tool


def _sim(c, H, W):
    from evennicer_slam_amd.event_sim import EventSimulator
    return EventSimulator(H, W, c_pos=c['c_pos'], c_neg=c['c_neg'], sigma_c=c.get('sigma_c', 0.0), substeps=c['K'], eps=C.EPS,
                          seed=c.get('seed', 0), device='cpu')


def _image_ref(name, sim):
    if C.image_cases()[name]['sigma_c'] > 0:
        return SC.image_stream_reference(name, sim.c_pos_map.numpy(), sim.c_neg_map.numpy())
    return SC.image_stream_reference(name)


def test_hand_worked_pixel():
    """Levels 0 -> 1 over one interval, C = 0.3, K = 2: sub-step 1 sees 0.5 and fires at level 0.3, sub-step 2 sees 1 and fires
    at 0.6 and 0.9.  With linear levels the crossings fall at t_a + 0.3, 0.6 and 0.9 of the interval."""
    from evennicer_slam_amd import event_sim as S
    t_a, dt = 2.0, 1.0
    levels = [np.array([[0.0]]), np.array([[0.5]]), np.array([[1.0]])]
    ref = YS.step_levels(Y.Sensor(levels[0], 0.3, 0.3), levels, t_a, t_a + dt)
    want = np.array([t_a + 0.3 * dt, t_a + 0.6 * dt, t_a + 0.9 * dt])
    assert ref['t'].shape == (3,) and np.all(np.abs(ref['t'] - want) <= 1e-15 * want)
    assert ref['p'].tolist() == [1, 1, 1] and ref['events'].tolist() == [[[0, 3]]]
    # the library's numpy route, step by step
    state, pos, neg = levels[0].copy(), np.zeros((1, 1)), np.zeros((1, 1))
    parts = []
    for s in (1, 2):
        R, pos0, neg0 = state.copy(), pos.copy(), neg.copy()
        S.sensor_update(levels[s], state, pos, neg, 0.3, 0.3)
        parts.append(S.stream_substep(s, 2, t_a, t_a + dt, R, pos - pos0, neg - neg0, 0.3, 0.3, levels[s - 1], levels[s]))
    t, x, y, p = S._stream_of(parts, 1).numpy()
    assert np.array_equal(t, ref['t']) and p.tolist() == [1, 1, 1] and x.tolist() == [0, 0, 0] and y.tolist() == [0, 0, 0]
    assert np.array_equal(state, ref['ref'])
    # a falling pixel mirrors it
    down = [np.array([[1.0]]), np.array([[0.5]]), np.array([[0.0]])]
    r2 = YS.step_levels(Y.Sensor(down[0], 0.3, 0.3), down, t_a, t_a + dt)
    assert r2['p'].tolist() == [0, 0, 0] and np.all(np.abs(r2['t'] - want) <= 1e-15 * want)


@pytest.mark.parametrize("name", sorted(C.image_cases()))
def test_numpy_route_is_bit_equal_and_round_trips(name):
    from evennicer_slam_amd import event_stream as ES
    c = C.image_cases()[name]
    sim, plain = _sim(c, *c['shape']), _sim(c, *c['shape'])
    ref = _image_ref(name, sim)
    sim.reset(c['images'][0])
    plain.reset(c['images'][0])
    H, W = c['shape']
    for i, (prev, cur) in enumerate(zip(c['images'][:-1], c['images'][1:])):
        t_a, t_b = SC.stamps(i)
        events, stream = sim.step_images(prev, cur, stamps=(t_a, t_b))
        assert isinstance(stream, ES.EventStream) and stream.device.type == 'cpu'
        t, x, y, p = stream.numpy()
        r = ref[i]
        assert t.dtype == np.float64 and x.dtype == np.uint16 and y.dtype == np.uint16 and p.dtype == np.uint8
        assert np.array_equal(t, r['t']) and np.array_equal(x, r['x']) and np.array_equal(y, r['y']) and np.array_equal(p, r['p'])
        # counts and L_ref: those of the call without stamps, and the yardstick's
        assert torch.equal(events, plain.step_images(prev, cur)) and torch.equal(sim.state, plain.state)
        assert np.array_equal(events.numpy(), r['events']) and np.array_equal(sim.state.numpy(), r['ref'])
        # every t inside the interval, non-decreasing per pixel, per-pixel totals = the unsaturated counts
        flat = y.astype(np.int64) * W + x
        assert bool(np.all((t >= t_a) & (t <= t_b))) and bool(np.all(np.diff(flat) >= 0))
        same = np.diff(flat) == 0
        assert bool(np.all(np.diff(t)[same] >= 0))
        assert np.array_equal(np.bincount(flat, minlength=H * W).reshape(H, W), r['total'])
        # round trip.  The lower edge sits below t_a: an event whose f is a few 1e-16 gets t_a itself, which the bin rule
        # (edges[b] < t) hands to the interval before
        counts, full, dropped = ES.accumulate(stream, [t_a - 1.0, t_b], H, W, want_unsaturated=True, with_dropped=True)
        assert torch.equal(counts[0], events) and dropped == (0, 0)
        assert np.array_equal(full[0].numpy().sum(-1), r['total'])
        at_start = int((t == t_a).sum())
        tight = ES.accumulate(stream, [t_a, t_b], H, W)[0]
        assert (at_start == 0) == torch.equal(tight, events)
        sorted_stream = stream.time_sorted()
        assert bool(np.all(np.diff(sorted_stream.numpy()[0]) >= 0))
        assert torch.equal(ES.accumulate(sorted_stream, [t_a - 1.0, t_b], H, W)[0], events)
    if name == "37x53_grey_K1":                                  # the case condition behind the lower edge, and the limit
        raw = np.concatenate([r['raw_f'] for r in ref])
        starts = sum(int((r['t'] == r['stamps'][0]).sum()) for r in ref)
        print(f"{name}: f before the limit in [{raw.min():.3e}, 1 + {raw.max() - 1:.3e}], {starts} events at t_a itself")
        assert raw.max() > 1.0 and starts >= 1


def test_case_totals_and_the_345_event_pixel():
    totals = {name: [int(r['total'].sum()) for r in SC.image_stream_reference(name)] for name in sorted(C.image_cases())
              if C.image_cases()[name]['sigma_c'] == 0}
    per_pixel = max(int(r['total'].max()) for name in totals for r in SC.image_stream_reference(name))
    print("events per interval:", totals, "most events of one pixel in one interval:", per_pixel)
    r = SC.image_stream_reference("37x53_grey_K5")[0]
    assert int(r['total'][0, 0]) == 345 and int(r['total'][0, 1]) == 0 and r['events'][0, 0].tolist() == [0, 255]
    assert all(v > 0 for row in totals.values() for v in row)


def test_derived_tolerance_and_left_out_share():
    """Prints the derived time tolerance over the device-log cases (the figure quoted in tests/event_stream_cases.py) and
    asserts that the yardstick alone leaves at most 0.1 % of an analytic case's pixels out."""
    worst, typical = 0.0, []
    for name in sorted(C.ANALYTIC):
        steps = SC.analytic_stream_reference(name)
        left = steps[-1]['left_out']
        assert left.sum() <= C.MAX_LEFT_OUT * left.size
        for r in steps:
            tol = SC.time_tolerance(r['den'], r['c'], r['K'], *r['stamps'])
            worst = max(worst, float(tol.max()))
            typical.append(float(np.median(tol)))
            assert float(tol.max()) <= (r['stamps'][1] - r['stamps'][0]) / r['K'] + 4 * np.spacing(r['stamps'][1])
    for name, c in sorted(C.image_cases().items()):
        if c['channels'] == 3 and c['sigma_c'] == 0:
            for r in SC.image_stream_reference(name):
                if r['t'].size:
                    tol = SC.time_tolerance(r['den'], r['c'], r['K'], *r['stamps'])
                    worst = max(worst, float(tol.max()))
                    typical.append(float(np.median(tol)))
    print(f"derived time tolerance over the device-log cases: largest {worst:.3e} s, median of the medians {np.median(typical):.3e} s")
    assert 0 < worst < SC.DT


@pytest.mark.parametrize("name", sorted(C.ANALYTIC))
def test_numpy_route_of_the_analytic_room(name):
    from evennicer_slam_amd import event_stream as ES
    c, ref, frames, room = C.ANALYTIC[name], SC.analytic_stream_reference(name), C.analytic_poses(name), C.demo_room()
    sim = _sim(dict(c_pos=c['c'], c_neg=c['c'], K=c['K']), CAM['H'], CAM['W'])
    plain = _sim(dict(c_pos=c['c'], c_neg=c['c'], K=c['K']), CAM['H'], CAM['W'])
    sim.reset((room, frames[0], CAM))
    plain.reset((room, frames[0], CAM))
    for i, r in enumerate(ref):
        events, stream = sim.step_scene(room, frames[i], frames[i + 1], CAM, stamps=r['stamps'])
        assert torch.equal(events, plain.step_scene(room, frames[i], frames[i + 1], CAM)) and torch.equal(sim.state, plain.state)
        out = SC.compare_streams(r, stream.numpy(), (CAM['H'], CAM['W']), keep=~r['left_out'])
        print(f"{name} interval {i}: {len(stream)} events, {out}")
        assert out['differ'] == 0 and out['polarity_ok'] and out['worst'] <= 1.0 and out['compared'] > 0
        t = stream.numpy()[0]
        assert bool(np.all((t >= r['stamps'][0]) & (t <= r['stamps'][1])))
        assert torch.equal(ES.accumulate(stream, [r['stamps'][0] - 1.0, r['stamps'][1]], CAM['H'], CAM['W'])[0], events)


@pytest.mark.parametrize("name", sorted(SC.accumulate_cases()))
def test_accumulate_numpy_route(name):
    from evennicer_slam_amd import event_stream as ES
    c = SC.accumulate_cases()[name]
    counts, full, d_time, d_sensor = SC.accumulate_reference(name)
    stream = ES.EventStream(c['t'], c['x'], c['y'], c['p'])
    got, got_full, dropped = ES.accumulate(stream, c['edges'], c['H'], c['W'], want_unsaturated=True, with_dropped=True)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (c['B'], c['H'], c['W'], 2)
    assert np.array_equal(got.numpy(), counts) and np.array_equal(got_full.numpy(), full) and dropped == (d_time, d_sensor)
    shuffled = ES.accumulate(stream.take(c['shuffled']), c['edges'], c['H'], c['W'], want_unsaturated=True, with_dropped=True)
    assert torch.equal(shuffled[0], got) and torch.equal(shuffled[1], got_full) and shuffled[2] == dropped
    assert int(full.sum()) + d_time + d_sensor == c['N']
    if c['N'] >= 6:                                             # the planted events, by the bin rule
        e, B = c['edges'], c['B']
        assert full[B - 1, 2, 7, 1] >= 1                        # t = edges[B]: the last bin
        inside = sum(int(full[b, 2, 7, 0]) for b in range(B))
        expect = int(((c['x'] == 7) & (c['y'] == 2) & (c['p'] == 0) & (c['t'] > e[0]) & (c['t'] <= e[-1])).sum())
        assert inside == expect                                 # the one at edges[0] is not among them
        if B >= 2:
            assert full[0, 2, 8, 1] >= 1 and int(((c['x'] == 8) & (c['y'] == 2) & (c['t'] == e[1])).sum()) == 1
        assert d_time >= 3 and d_sensor >= 1
    if c['N'] >= 1000:                                          # saturated against unsaturated
        y, x = SC.SATURATING_PIXEL
        assert full[0, y, x, 1] >= 300 and counts[0, y, x, 1] == 255
        assert np.array_equal(counts, np.minimum(full, 255))


def test_accumulate_far_out_coordinates_and_checks():
    from evennicer_slam_amd import event_stream as ES
    from evennicer_slam_amd._lib import EnslamError
    c = SC.far_out_case()
    stream = ES.EventStream(c['t'], c['x'], c['y'], c['p'])
    counts, dropped = ES.accumulate(stream, c['edges'], c['H'], c['W'], with_dropped=True)
    ref = YS.accumulate(c['t'], c['x'], c['y'], c['p'], c['edges'], c['H'], c['W'])
    assert np.array_equal(counts.numpy(), ref[0]) and dropped == (ref[2], ref[3]) == (0, 2) and int(counts.sum()) == 2
    # -inf as the first edge, a NaN time, an empty bin between equal edges
    s2 = ES.EventStream(np.array([-1e300, np.nan, 10.0]), [1, 1, 1], [1, 1, 1], [1, 1, 1])
    counts, dropped = ES.accumulate(s2, [-np.inf, 10.0, 10.0, 11.0], 4, 4, with_dropped=True)
    assert counts[:, 1, 1, 1].tolist() == [2, 0, 0] and dropped == (1, 0)
    for bad in ([10.0], [11.0, 10.0], [10.0, np.nan]):
        with pytest.raises(EnslamError):
            ES.accumulate(stream, bad, 4, 4)
    with pytest.raises(EnslamError):
        ES.accumulate(stream, [0.0, 1.0], 0, 4)
    with pytest.raises(EnslamError):
        ES.EventStream([0.0], [70000], [0], [1])
    with pytest.raises(EnslamError):
        ES.EventStream([0.0, 1.0], [1], [0], [1])


def test_text_and_npz_round_trips(tmp_path):
    from evennicer_slam_amd import event_stream as ES
    rng = np.random.default_rng(3)
    n = 5000
    t = np.sort(1.5e9 + rng.integers(0, 10 ** 9, n) * 1e-6)              # microsecond stamps near 1.5e9 s
    t = np.array([float(f"{v:.6f}") for v in t])                        # as a recording's text holds them
    stream = ES.EventStream(t, rng.integers(0, 346, n), rng.integers(0, 260, n), rng.integers(0, 2, n))
    path = str(tmp_path / 'events.txt')
    ES.write_events_txt(path, stream)
    with open(path) as f:
        first = f.readline().split()
    assert len(first) == 4 and float(first[0]) == t[0] and len(first[0]) <= 17 and first[3] in ("0", "1")
    for chunk in (1 << 20, 777):                                         # one chunk, and many with a short last one
        back = ES.read_events_txt(path, chunk=chunk)
        assert len(back) == n and all(np.array_equal(a, b) for a, b in zip(back.numpy(), stream.numpy()))
    with open(path, 'a') as f:
        f.write("# a comment\n\n")
    assert len(ES.read_events_txt(path)) == n
    stream.save(str(tmp_path / 's.npz'))
    again = ES.load_stream(str(tmp_path / 's.npz'))
    assert all(np.array_equal(a, b) and a.dtype == b.dtype for a, b in zip(again.numpy(), stream.numpy()))
    assert len(ES.EventStream.empty()) == 0 and len(ES.EventStream.empty().time_sorted()) == 0
    # a stable sort: ties keep their order
    tied = ES.EventStream([2.0, 1.0, 1.0, 1.0], [0, 1, 2, 3], [0, 0, 0, 0], [1, 0, 1, 0]).time_sorted()
    assert tied.x.tolist() == [1, 2, 3, 0]


def test_frame_edges():
    from evennicer_slam_amd import event_stream as ES
    from evennicer_slam_amd._lib import EnslamError
    stamps = [1.0 + 0.1 * i for i in range(10)]
    assert np.array_equal(ES.frame_edges(stamps), np.array(stamps))
    assert np.array_equal(ES.frame_edges(stamps, gap=3), np.array(stamps[::3]))                  # frames 0, 3, 6, 9
    dense = ES.frame_edges(stamps, density=4)
    assert dense.size == 9 * 4 + 1 and np.array_equal(dense[::4], np.array(stamps))
    a, b = stamps[2], stamps[3]
    assert dense[9] == a + (1 / 4) * (b - a) and dense[10] == a + (2 / 4) * (b - a) and bool(np.all(np.diff(dense) > 0))
    both = ES.frame_edges(stamps, gap=3, density=4)
    assert both.size == 3 * 4 + 1 and np.array_equal(both[::4], np.array(stamps[::3]))
    for kw in (dict(gap=0), dict(density=0), dict(gap=10)):
        with pytest.raises(EnslamError):
            ES.frame_edges(stamps, **kw)
    with pytest.raises(EnslamError):
        ES.frame_edges([1.0, 0.5, 2.0])


def _demo_recording(tmp_path, n=6, H=8, W=10):
    """n grey frames with depth and poses in the RPG layout, their simulated count images and stream, and the files a
    recording comes with: events.txt (time-sorted) and images.txt (frame times)."""
    from evennicer_slam_amd import datasets as D
    from evennicer_slam_amd import event_stream as ES
    from evennicer_slam_amd.event_sim import EventSimulator
    from tests.test_datasets_cpu import _poses
    rng = np.random.default_rng(21)
    greys = [rng.integers(0, 256, (H, W), dtype=np.uint8)]
    for _ in range(n - 1):
        greys.append(np.clip(greys[-1].astype(np.int64) + rng.integers(-40, 41, (H, W)), 0, 255).astype(np.uint8))
    depth = np.full((H, W), 1.5, dtype=np.float32)
    poses = _poses(n, seed=22)
    times = [1.5e9 + 0.04 * i for i in range(n)]
    sim = EventSimulator(H, W, c_pos=0.05, c_neg=0.05, substeps=4, device='cpu').reset(greys[0])
    images, streams = [], []
    for i in range(1, n):
        ev, st = sim.step_images(greys[i - 1], greys[i], stamps=(times[i - 1], times[i]))
        assert bool((st.t > times[i - 1]).all())                 # case condition: no event of this sequence rounds to t_a
        images.append(ev.numpy())
        streams.append(st)
    root = str(tmp_path / 'rec')
    inp, evf = D.write_rpg_event_sequence(root, [(g, depth) for g in greys], poses, 1000.0, images)
    whole = ES.EventStream.concatenate(streams).time_sorted()
    ES.write_events_txt(os.path.join(root, 'events.txt'), whole)
    with open(os.path.join(root, 'images.txt'), 'w') as f:
        f.write("# time file\n")
        for i, tt in enumerate(times):
            f.write(f"{tt!r} frame{i:06d}.png\n")
    cam = dict(H=H, W=W, fx=9.0, fy=9.0, cx=4.5, cy=3.5, png_depth_scale=1000.0, crop_edge=0)
    return dict(root=root, inp=inp, evf=evf, images=images, whole=whole, times=times, cam=cam, n=n, H=H, W=W, poses=poses)


def test_events_to_frames_tool(tmp_path, capsys):
    from evennicer_slam_amd import datasets as D
    from evennicer_slam_amd import event_stream as ES
    r = _demo_recording(tmp_path)
    tool = _tool("events_to_frames")
    events, stamps = os.path.join(r['root'], 'events.txt'), os.path.join(r['root'], 'images.txt')
    size = ['--height', str(r['H']), '--width', str(r['W']), '--device', 'cpu']
    # gap 1, density 1: byte-equal to the pngs written from the simulator's own count images
    out1 = str(tmp_path / 'gap1')
    info = tool.main([events, stamps, '--out', out1] + size)
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert line['events_read'] == len(r['whole']) == line['events_binned'] and line['dropped_by_time'] == 0 == line['dropped_by_sensor']
    assert line['files_written'] == r['n'] - 1 and info['saturated_pixels'] == sum(int((im == 255).sum()) for im in r['images']) == 0
    names = sorted(os.listdir(out1))
    assert names == sorted(os.listdir(r['evf'])) and len(names) == r['n'] - 1
    for name in names:
        with open(os.path.join(out1, name), 'rb') as a, open(os.path.join(r['evf'], name), 'rb') as b:
            assert a.read() == b.read(), name
    cfg = {'dataset': 'rpg_event', 'cam': r['cam'], 'data': {'input_folder': r['inp'], 'event_folder': out1}}
    ds = D.get_dataset(cfg, ARGS, 1.0, device='cpu')
    assert isinstance(ds, D.RPG_event) and len(ds) == r['n']
    for i in range(1, r['n']):
        assert np.array_equal(ds[i][3].numpy(), r['images'][i - 1])
    # density 2 with poses: RPG_event_dense reads it; two half-interval images sum to the interval's
    out2 = str(tmp_path / 'dense')
    info = tool.main([events, stamps, '--out', out2, '--density', '2', '--poses', os.path.join(r['inp'], 'traj.txt')] + size)
    assert info['files_written'] == (r['n'] - 1) * 2 and info['dense_pose_lines'] == (r['n'] - 1) * 2 + 1
    cfg = {'dataset': 'rpg_event_dense', 'cam': r['cam'], 'data': {'input_folder': r['inp'], 'event_folder': out2, 'density': 2}}
    dense = D.get_dataset(cfg, ARGS, 1.0, device='cpu')
    assert isinstance(dense, D.RPG_event_dense) and len(dense) == (r['n'] - 1) * 2 + 1
    for i in range(1, r['n']):
        two = dense[2 * i - 1][3].numpy().astype(np.int64) + dense[2 * i][3].numpy().astype(np.int64)
        assert np.array_equal(two, r['images'][i - 1].astype(np.int64))
        assert np.allclose(dense[2 * i][5].numpy(), r['poses'][i], atol=1e-6)                   # every second pose is a frame's
    # gap 5 keeps frames 0 and 5: one image with all the events; the replica layout's names
    out3 = str(tmp_path / 'gap5')
    info = tool.main([events, stamps, '--out', out3, '--gap', '5', '--layout', 'replica_event'] + size)
    assert sorted(os.listdir(out3)) == ['event_frame000001.png'] and info['events_binned'] == len(r['whole'])
    total = np.minimum(sum(im.astype(np.int64) for im in r['images']), 255)
    assert np.array_equal(D._imread_rgb(os.path.join(out3, 'event_frame000001.png'))[:, :, 1:], total)
    # a sensor smaller than the recording's: the events outside are counted, not written
    info = tool.main([events, stamps, '--out', str(tmp_path / 'small'), '--height', '4', '--width', '5', '--device', 'cpu'])
    x, y = r['whole'].numpy()[1:3]
    assert info['dropped_by_sensor'] == int(((x >= 5) | (y >= 4)).sum()) > 0
    assert info['events_binned'] + info['dropped_by_sensor'] == len(r['whole'])
    # .npz input
    r['whole'].save(str(tmp_path / 'e.npz'))
    assert tool.main([str(tmp_path / 'e.npz'), stamps, '--out', str(tmp_path / 'npz')] + size)['events_binned'] == len(r['whole'])
    assert isinstance(ES.load_stream(str(tmp_path / 'e.npz')), ES.EventStream)


@pytest.mark.parametrize("dataset", ["rpg_event", "rpg_event_dense"])
def test_reader_option_equals_the_png_folder(tmp_path, dataset):
    from evennicer_slam_amd import datasets as D
    r = _demo_recording(tmp_path)
    tool = _tool("events_to_frames")
    events, stamps = os.path.join(r['root'], 'events.txt'), os.path.join(r['root'], 'images.txt')
    density = 2 if dataset == 'rpg_event_dense' else 1
    folder = str(tmp_path / 'png')
    tool.main([events, stamps, '--out', folder, '--density', str(density), '--poses', os.path.join(r['inp'], 'traj.txt'),
               '--height', str(r['H']), '--width', str(r['W']), '--device', 'cpu'])
    data = {'input_folder': r['inp'], 'density': density}
    from_png = D.get_dataset({'dataset': dataset, 'cam': r['cam'], 'data': dict(data, event_folder=folder)}, ARGS, 1.0, device='cpu')
    from_stream = D.get_dataset({'dataset': dataset, 'cam': r['cam'], 'data': dict(data, event_stream=events, frame_stamps=stamps)},
                                ARGS, 1.0, device='cpu')
    assert len(from_png) == len(from_stream) == (r['n'] - 1) * density + 1 and from_stream.n_event == from_png.n_event
    for i in range(len(from_png)):
        a, b = from_png[i], from_stream[i]
        assert all(torch.equal(u, v) for u, v in zip(a[1:], b[1:])) and bool(b[3].any()) == (i > 0)
    with pytest.raises(ValueError):
        D.get_dataset({'dataset': dataset, 'cam': r['cam'], 'data': dict(data, event_stream=events)}, ARGS, 1.0, device='cpu')


def test_reader_option_replica_layout_and_simulate_tool(tmp_path, capsys):
    """tools/simulate_events.py --demo --stream on the CPU, then Replica_event from the stream = from the pngs it wrote."""
    from evennicer_slam_amd import datasets as D
    from evennicer_slam_amd import event_stream as ES
    from evennicer_slam_amd.synthetic import demo_config
    tool = _tool("simulate_events")
    n, fps = 4, 25.0
    stream_path = str(tmp_path / 'events.npz')
    out = tool.main(['--demo', str(n), '--out', str(tmp_path / 'demo'), '--device', 'cpu', '--c-pos', '0.04', '--c-neg', '0.04',
                     '--substeps', '3', '--stream', stream_path, '--fps', str(fps)])
    capsys.readouterr()
    stream = ES.load_stream(stream_path)
    assert out['stream_events'] == len(stream) > 0 and bool(np.all(np.diff(stream.numpy()[0]) >= 0))
    stamps = str(tmp_path / 'stamps.txt')
    with open(stamps, 'w') as f:
        f.write(''.join(f"{i / fps!r}\n" for i in range(n)))
    cfg = demo_config(out['input_folder'], out['event_folder'], tool.DEMO_CAM, device='cpu')
    from_png = D.get_dataset(cfg, ARGS, 1, device='cpu')
    cfg2 = demo_config(out['input_folder'], None, tool.DEMO_CAM, device='cpu')
    del cfg2['data']['event_folder']
    cfg2['data'].update(event_stream=stream_path, frame_stamps=stamps)
    from_stream = D.get_dataset(cfg2, ARGS, 1, device='cpu')
    assert isinstance(from_stream, D.Replica_event) and len(from_stream) == n
    starts = sum(int((stream.t == i / fps).sum()) for i in range(n))
    for i in range(n):
        a, b = from_png[i], from_stream[i]
        assert torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]) and torch.equal(a[5], b[5])
        if starts == 0:                                          # no event rounded to a frame's own time (the usual case)
            assert torch.equal(a[3], b[3]) and torch.equal(a[4], b[4])
    assert starts == 0


def test_simulate_tool_writes_the_stream_of_a_recorded_sequence(tmp_path, capsys):
    """tools/simulate_events.py CONFIG --stream events.txt --stamps images.txt: the text stream equals the one simulated
    directly, and the event folder it wrote is the one tools/events_to_frames.py makes from that stream."""
    import yaml
    from evennicer_slam_amd import event_stream as ES
    r = _demo_recording(tmp_path)
    cfg = {'dataset': 'rpg_event', 'scale': 1, 'data': {'input_folder': r['inp'], 'event_folder': r['evf']}, 'cam': r['cam']}
    path = str(tmp_path / 'seq.yaml')
    with open(path, 'w') as f:
        yaml.safe_dump(cfg, f)
    out, stream_path = str(tmp_path / 'sim_events'), str(tmp_path / 'sim_events.txt')
    stamps = os.path.join(r['root'], 'images.txt')
    info = _tool("simulate_events").main([path, '--out', out, '--device', 'cpu', '--c-pos', '0.05', '--c-neg', '0.05', '--substeps', '4',
                                          '--stream', stream_path, '--stamps', stamps])
    capsys.readouterr()
    assert info['stream_events'] == len(r['whole']) and info['event_images'] == r['n'] - 1
    got = ES.read_events_txt(stream_path)
    assert all(np.array_equal(a, b) for a, b in zip(got.numpy(), r['whole'].numpy()))
    again = str(tmp_path / 'again')
    _tool("events_to_frames").main([stream_path, stamps, '--out', again, '--height', str(r['H']), '--width', str(r['W']), '--device', 'cpu'])
    capsys.readouterr()
    for name in sorted(os.listdir(out)):
        with open(os.path.join(out, name), 'rb') as a, open(os.path.join(again, name), 'rb') as b:
            assert a.read() == b.read(), name
    assert len(os.listdir(again)) == len(os.listdir(out)) == r['n'] - 1


def test_exports_and_cpu_tensors_are_refused():
    import ctypes
    import re
    import evennicer_slam_amd as E
    from evennicer_slam_amd import functional as EF
    from evennicer_slam_amd._lib import EnslamError
    header = open(os.path.join(ROOT, "include", "enslam_hip.h")).read()
    handle = ctypes.CDLL(E.LIB_PATH)
    for name in EXPORTS:
        assert name in E._lib.EXPORTS and re.search(r"\b%s\s*\(" % name, header) and hasattr(handle, name), name
    state = torch.zeros((4, 5), dtype=torch.float64)
    img = torch.zeros((4, 5), dtype=torch.uint8)
    lut = torch.zeros(256, dtype=torch.float64)
    with pytest.raises(EnslamError):
        EF.event_stream_images(img, img, state, (0.0, 1.0), lut=lut)
    with pytest.raises(EnslamError):
        EF.event_stream_boxroom(C.demo_room(), np.tile(np.eye(4), (3, 1, 1)), dict(CAM, H=4, W=5), state, (0.0, 1.0))
    with pytest.raises(EnslamError):
        EF.event_accumulate(torch.zeros(3, dtype=torch.float64), torch.zeros(3, dtype=torch.uint16), torch.zeros(3, dtype=torch.uint16),
                            torch.zeros(3, dtype=torch.uint8), [0.0, 1.0], 4, 5)
