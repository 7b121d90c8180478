"""CPU tests of the event-stream filter (event_filter.py): the yardstick tests/event_filter_numpy.py against the hand-worked
classes of planted_5x7, then event_filter.filter_numpy against the yardstick on every case of tests/event_filter_cases.py
(bit-equal: classes, output stream, both states, counters), the case conditions, chunked against one-shot, the boundary tie,
the chunk-order refusal, the consistency with the simulator's refractory rule, hot_pixels, the composition with accumulate,
tools/events_to_frames.py with the new flags and a `*_event` reader with `data.event_filter`."""
import ctypes
import json
import math
import os
import re

import numpy as np
import pytest
import torch

from tests import event_filter_cases as FC
from tests import event_filter_numpy as YF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPORTS = ("enslam_event_pixel_counts", "enslam_event_filter_walk", "enslam_event_filter_support", "enslam_event_filter_compact")


def _stream(c, device='cpu'):
    from evennicer_slam_amd.event_stream import EventStream
    return EventStream(c['t'].copy(), c['x'].copy(), c['y'].copy(), c['p'].copy()).to(device)


def _filter(c, device='cpu'):
    from evennicer_slam_amd.event_filter import EventFilter
    return EventFilter(c['H'], c['W'], refractory=c['rho'], support_dt=c['dt'], hot_mask=c['hot_mask'], device=device)


def _bits(a):
    a = a.cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else a


def check_against(ref, kept, stats, classes, filt):
    """one filter result (or the concatenation of a chunked one) bit-equal to a run of the yardstick"""
    assert np.array_equal(_bits(classes), np.concatenate(ref['classes']))
    for k, a in zip('txyp', kept.arrays()):
        assert a.dtype == dict(t=torch.float64, x=torch.uint16, y=torch.uint16, p=torch.uint8)[k]
        assert np.array_equal(_bits(a), _bits(ref[k])), k
    assert stats == ref['counters']
    assert np.array_equal(_bits(filt.t_last), _bits(ref['t_last'])) and np.array_equal(_bits(filt.t_seen), _bits(ref['t_seen']))


def run_chunked(chunks, device='cpu'):
    """an EventFilter over the chunks with carried state: (kept EventStream, summed stats, classes, filter)"""
    from evennicer_slam_amd.event_stream import EventStream
    filt = _filter(chunks[0], device)
    parts, classes, total = [], [], None
    for c in chunks:
        kept, stats, cls = filt(_stream(c, device), return_classes=True)
        parts.append(kept)
        classes.append(cls.cpu())
        total = stats if total is None else {k: total[k] + stats[k] for k in stats}
    return EventStream.concatenate(parts), total, torch.cat(classes), filt


@pytest.mark.parametrize("setting", sorted(FC.PLANTED_EXPECTED))
def test_planted_events_one_by_one(setting):
    """the yardstick against the hand-worked classes of tests/event_filter_cases.py, event by event"""
    got = FC.reference(f'planted_5x7_{setting}')['classes'][0].tolist()
    want = FC.PLANTED_EXPECTED[setting]
    assert len(got) == len(want) == len(FC.PLANTED_EVENTS)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, (setting, i, FC.PLANTED_EVENTS[i], YF.NAMES[g], YF.NAMES[w])
    if setting == 'rho_support':
        assert set(got) == set(range(6))                        # condition: every class occurs
    c = FC.planted(setting)
    t_u = c['t'] / FC.U                                         # condition: times, rho and dt are multiples of 2^-10
    fin = np.isfinite(t_u)
    assert np.array_equal(t_u[fin], np.rint(t_u[fin])) and (c['rho'] / FC.U).is_integer() and (c['dt'] is None or (c['dt'] / FC.U).is_integer())


@pytest.mark.parametrize("name", sorted(FC.cases()))
def test_numpy_route_is_bit_equal(name):
    c, ref = FC.cases()[name], FC.reference(name)
    filt = _filter(c)
    stream = _stream(c)
    kept, stats, classes = filt(stream, return_classes=True)
    check_against(ref, kept, stats, classes, filt)
    assert all(np.array_equal(_bits(a), _bits(c[k])) for k, a in zip('txyp', stream.arrays()))          # the input is untouched
    assert len(filt(_stream(c).take(torch.zeros(0, dtype=torch.int64)))[0]) == 0                        # an empty chunk is valid


def test_case_conditions():
    ref = FC.reference('37x53_noisy_emitted')
    refr = ref['removed_refractory'] / ref['reached_refractory']
    supp = ref['removed_support'] / ref['reached_support']
    print(f"37x53_noisy: refractory removes {ref['removed_refractory']} of {ref['reached_refractory']} ({100 * refr:.1f} %), "
          f"support {ref['removed_support']} of {ref['reached_support']} ({100 * supp:.1f} %)")
    assert 0.05 <= refr <= 0.95 and 0.05 <= supp <= 0.95
    base = FC.noisy_base()
    key = np.stack([base['y'].astype(np.float64) * base['W'] + base['x'], base['t']], axis=1)
    assert np.unique(key, axis=0).shape[0] == key.shape[0]      # no two live events share pixel and time
    assert 10_000 <= base['t'].shape[0] <= 100_000
    # the orders are what their names say
    t = FC.noisy('time')[0]['t']
    assert bool(np.all(t[1:] >= t[:-1]))
    pm = FC.noisy('pixel_major')[0]
    o = pm['y'].astype(np.int64) * pm['W'] + pm['x']
    assert bool(np.all((o[1:] > o[:-1]) | ((o[1:] == o[:-1]) & (pm['t'][1:] >= pm['t'][:-1])))) and not bool(np.all(pm['t'][1:] >= pm['t'][:-1]))
    for order in ('emitted', 'shuffled'):
        e = FC.noisy(order)[0]
        o = e['y'].astype(np.int64) * e['W'] + e['x']
        assert bool(np.any(e['t'][1:] < e['t'][:-1])) and bool(np.any(o[1:] < o[:-1]))
    # the same events in every order get the same classes: compared through the permutation
    want = ref['classes'][0]
    for order in FC.NOISY_ORDERS:
        perm = FC.noisy(order)[1]
        assert np.array_equal(FC.reference(f'37x53_noisy_{order}')['classes'][0], want[perm])
    # 1 x 1: with support nothing survives, without it only the refractory stage acts
    a, b = FC.reference('1x1_support'), FC.reference('1x1_refractory')
    assert a['counters']['n_out'] == 0 and a['counters']['unsupported'] == b['counters']['n_out'] > 0
    assert a['counters']['refractory'] == b['counters']['refractory'] > 0 and b['counters']['unsupported'] == 0
    lr = FC.cases()['long_run']
    assert int(((lr['x'] == 4) & (lr['y'] == 4)).sum()) == 20000 and lr['t'].shape[0] == 25000
    assert np.unique(lr['t']).shape[0] == lr['t'].shape[0]
    assert [FC.cases()[f'edge_{n}']['t'].shape[0] for n in FC.EDGE_NS] == list(FC.EDGE_NS)


@pytest.mark.parametrize("count", FC.SPLIT_COUNTS)
def test_chunked_equals_one_shot(count):
    case = FC.noisy('time')[0]
    points = FC.split_points(count)
    assert len(points) == count and all(case['t'][q - 1] < case['t'][q] for q in points)
    chunks = FC.cut(case, points)
    one = FC.reference('37x53_noisy_time')
    chunked = FC.run_yardstick(chunks)                          # the yardstick itself: chunked = one call
    assert np.array_equal(np.concatenate(chunked['classes']), one['classes'][0]) and chunked['counters'] == one['counters']
    assert np.array_equal(_bits(chunked['t_last']), _bits(one['t_last'])) and np.array_equal(_bits(chunked['t_seen']), _bits(one['t_seen']))
    check_against(one, *run_chunked(chunks))


def test_boundary_tie():
    chunks, one_call, chunked = FC.boundary_tie()
    both = dict(chunks[0], **{k: np.concatenate([c[k] for c in chunks]) for k in 'txyp'})
    assert FC.run_yardstick([both])['classes'][0].tolist() == one_call
    ref = FC.run_yardstick(chunks)
    assert np.concatenate(ref['classes']).tolist() == chunked
    check_against(ref, *run_chunked(chunks))
    check_against(FC.run_yardstick([both]), *run_chunked([both]))


def test_chunk_order_refusal():
    from evennicer_slam_amd._lib import EnslamError
    from evennicer_slam_amd.event_filter import EventFilter
    from evennicer_slam_amd.event_stream import EventStream
    filt = EventFilter(2, 2, refractory=0.0)
    filt(EventStream([1.0, 2.0], [0, 1], [0, 0], [1, 1]))
    filt(EventStream([2.0, math.nan, 0.5], [0, 0, 9], [1, 0, 0], [1, 1, 1]))            # an equal time is fine; dead events do not count
    before = (filt.t_last.clone(), filt.t_seen.clone())
    with pytest.raises(EnslamError):
        filt(EventStream([3.0, 1.5], [0, 1], [0, 1], [1, 1]))
    assert torch.equal(filt.t_last, before[0]) and torch.equal(filt.t_seen, before[1])  # a refused chunk leaves the state
    filt.reset()
    assert filt(EventStream([0.5], [0], [0], [1]))[1]['n_out'] == 1
    for bad in (dict(refractory=-1.0), dict(refractory=math.inf), dict(support_dt=-1e-3), dict(support_dt=math.nan)):
        with pytest.raises(EnslamError):
            EventFilter(2, 2, **bad)
    with pytest.raises(EnslamError):
        EventFilter(0, 2)
    with pytest.raises(EnslamError):
        EventFilter(2, 2, hot_mask=np.zeros((3, 2)))


def simulator_stream(device, rho=5e-3):
    """the noisy simulator's stream of 37x53_grey_K5 with EventNoise(refractory=rho), all intervals, as emitted"""
    from evennicer_slam_amd.event_sim import EventNoise, EventSimulator
    from evennicer_slam_amd.event_stream import EventStream
    from tests import event_noise_cases as NC
    from tests import event_sim_cases as C
    c = C.image_cases()[FC.NOISY_SOURCE]
    H, W = c['shape']
    sim = EventSimulator(H, W, c_pos=c['c_pos'], c_neg=c['c_neg'], sigma_c=c.get('sigma_c', 0.0), substeps=c['K'], eps=C.EPS,
                         seed=c.get('seed', 0), device=device, noise=EventNoise(refractory=rho))
    sim.reset(c['images'][0])
    parts = [sim.step_images(prev, cur, stamps=NC.stamps(i))[1] for i, (prev, cur) in enumerate(zip(c['images'][:-1], c['images'][1:]))]
    return EventStream.concatenate(parts), H, W, sim


def check_simulator_consistency(device):
    """a stream emitted under ESIM's refractory rule passes the filter's refractory stage whole: the same rule, the same
    expression, and the filter's t_last ends where the simulator's does"""
    from evennicer_slam_amd.event_filter import filter_stream, EventFilter
    rho = 5e-3
    stream, H, W, sim = simulator_stream(device, rho)
    t, x, y, _ = stream.numpy()
    o = y.astype(np.int64) * W + x
    by = np.lexsort((np.arange(t.size), o))                     # stable by pixel, stream order inside
    same = o[by][1:] == o[by][:-1]
    assert len(stream) > 10_000 and bool(np.all(t[by][1:][same] >= t[by][:-1][same]))    # condition: times do not descend within a pixel
    filt = EventFilter(H, W, refractory=rho, device=device)
    kept, stats = filt(stream)
    assert stats['n_out'] == stats['n_in'] == len(stream) and stats['refractory'] == 0
    assert all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(kept.arrays(), stream.arrays()))
    fired = torch.isfinite(filt.t_last)
    assert torch.equal(filt.t_last[fired], sim.last_event_time[fired]) and bool(fired.any())
    assert filter_stream(stream, H, W, refractory=2 * rho)[1]['refractory'] > 0          # and a longer period does remove


def test_simulator_consistency():
    check_simulator_consistency('cpu')


def test_hot_pixels():
    from evennicer_slam_amd._lib import EnslamError
    from evennicer_slam_amd.event_filter import filter_stream, hot_pixels
    c = FC.planted()
    stream = _stream(c)
    t, x, y = c['t'], c['x'].astype(np.int64), c['y'].astype(np.int64)
    ok = (x < 7) & (y < 5) & np.isfinite(t)
    want = np.bincount(y[ok] * 7 + x[ok], minlength=35).reshape(5, 7)
    mask, counts = hot_pixels(stream, 5, 7, max_events=1)
    assert counts.dtype == torch.int64 and np.array_equal(counts.numpy(), want) and np.array_equal(mask.numpy(), want > 1)
    assert mask.dtype == torch.bool and int(mask.sum()) == 4                # (1,1), (1,3), (6,4) and (3,3); the TIME events of (2,2) and (5,1) do not count
    span = float(t[np.isfinite(t)].max() - t[np.isfinite(t)].min())
    rate = 2.5 / span
    mask_r, _ = hot_pixels(stream, 5, 7, rate=rate)
    assert np.array_equal(mask_r.numpy(), want > int(math.floor(rate * span)))
    base = FC.noisy_base()
    b = np.bincount(base['y'].astype(np.int64) * 53 + base['x'], minlength=37 * 53).reshape(37, 53)
    mask, counts = hot_pixels(_stream(base), 37, 53, max_events=40)
    assert np.array_equal(counts.numpy(), b) and np.array_equal(mask.numpy(), b > 40) and 0 < int(mask.sum()) < b.size
    # the learned mask drives the filter: every event of a hot pixel leaves as HOT
    stats = filter_stream(_stream(base), 37, 53, hot_mask=mask)[1]
    assert stats['hot'] == int(b[b > 40].sum()) and stats['n_out'] == int(b[b <= 40].sum())
    for bad in (dict(), dict(max_events=1, rate=1.0), dict(max_events=-1), dict(rate=-1.0)):
        with pytest.raises(EnslamError):
            hot_pixels(stream, 5, 7, **bad)


def test_composition_with_accumulate():
    from evennicer_slam_amd.event_filter import filter_stream
    from evennicer_slam_amd.event_stream import EventStream, accumulate
    c, ref = FC.cases()['37x53_noisy_shuffled'], FC.reference('37x53_noisy_shuffled')
    edges = np.linspace(c['t'].min() - 1e-3, c['t'].max(), 7)
    kept = filter_stream(_stream(c), c['H'], c['W'], c['rho'], c['dt'])[0]
    want = accumulate(EventStream(ref['t'], ref['x'], ref['y'], ref['p']), edges, c['H'], c['W'], with_dropped=True)
    got = accumulate(kept, edges, c['H'], c['W'], with_dropped=True)
    assert torch.equal(got[0], want[0]) and got[1] == want[1] == (0, 0) and int(got[0].sum()) == ref['counters']['n_out']


def _tool(name):
    import importlib.util
    spec = importlib.util.spec_from_file_location(name + "_tool", os.path.join(ROOT, "tools", name + ".py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    return tool


OPTIONS = dict(refractory=0.01, support_dt=0.004, hot_max=22)


def check_tool_route(tmp_path, capsys, device):
    """tools/events_to_frames.py with the filter flags writes what filter-then-bin gives (the yardstick's kept events binned by
    the plain tool) and reports the counters; returns the folder it wrote"""
    from evennicer_slam_amd import event_stream as ES
    from tests.test_event_stream_cpu import _demo_recording
    r = _demo_recording(tmp_path)
    tool = _tool("events_to_frames")
    events, stamps = os.path.join(r['root'], 'events.txt'), os.path.join(r['root'], 'images.txt')
    size = ['--height', str(r['H']), '--width', str(r['W']), '--device', device]
    t, x, y, p = r['whole'].numpy()
    counts = np.bincount(y.astype(np.int64) * r['W'] + x, minlength=r['H'] * r['W']).reshape(r['H'], r['W'])
    mask = (counts > OPTIONS['hot_max']).astype(np.uint8)
    ref = FC.run_yardstick([dict(H=r['H'], W=r['W'], t=t, x=x, y=y, p=p, rho=OPTIONS['refractory'], dt=OPTIONS['support_dt'], hot_mask=mask)])
    n = ref['counters']
    assert n['hot'] > 0 and n['refractory'] > 0 and n['unsupported'] > 0 and n['n_out'] > 0             # condition: every filter acts
    manual = str(tmp_path / 'manual.npz')
    ES.EventStream(ref['t'], ref['x'], ref['y'], ref['p']).save(manual)
    want_dir, got_dir = str(tmp_path / 'want'), str(tmp_path / f'got_{device.split(":")[0]}')
    tool.main([manual, stamps, '--out', want_dir, '--height', str(r['H']), '--width', str(r['W']), '--device', 'cpu'])
    capsys.readouterr()
    info = tool.main([events, stamps, '--out', got_dir, '--refractory', str(OPTIONS['refractory']), '--support-dt',
                      str(OPTIONS['support_dt']), '--hot-max', str(OPTIONS['hot_max'])] + size)
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert line['filter'] == info['filter'] == n and line['events_read'] == n['n_out'] == line['events_binned']
    names = sorted(os.listdir(want_dir))
    assert names == sorted(os.listdir(got_dir)) and len(names) == r['n'] - 1
    for name in names:
        with open(os.path.join(want_dir, name), 'rb') as a, open(os.path.join(got_dir, name), 'rb') as b:
            assert a.read() == b.read(), name
    # --hot-rate: the same mask through the rate form
    span = float(t.max() - t.min())
    rate = (OPTIONS['hot_max'] + 0.5) / span
    info = tool.main([events, stamps, '--out', str(tmp_path / 'rate'), '--hot-rate', repr(rate)] + size)
    capsys.readouterr()
    assert info['filter']['hot'] == int(counts[counts > OPTIONS['hot_max']].sum()) and info['filter']['refractory'] == 0
    # no flag: no filter, no `filter` key
    assert 'filter' not in tool.main([events, stamps, '--out', str(tmp_path / 'plain')] + size)
    capsys.readouterr()
    return r, got_dir, want_dir


def test_events_to_frames_with_filter_flags(tmp_path, capsys):
    check_tool_route(tmp_path, capsys, 'cpu')


def test_reader_with_event_filter(tmp_path, capsys):
    """RPG_event with data.event_stream + data.event_filter returns the event images of the manual route"""
    import types
    from evennicer_slam_amd import datasets as D
    r, got_dir, _ = check_tool_route(tmp_path, capsys, 'cpu')
    args = types.SimpleNamespace(input_folder=None, event_folder=None)
    events, stamps = os.path.join(r['root'], 'events.txt'), os.path.join(r['root'], 'images.txt')
    data = {'input_folder': r['inp']}
    from_png = D.get_dataset({'dataset': 'rpg_event', 'cam': r['cam'], 'data': dict(data, event_folder=got_dir)}, args, 1.0, device='cpu')
    from_stream = D.get_dataset({'dataset': 'rpg_event', 'cam': r['cam'],
                                 'data': dict(data, event_stream=events, frame_stamps=stamps, event_filter=dict(OPTIONS))}, args, 1.0, device='cpu')
    plain = D.get_dataset({'dataset': 'rpg_event', 'cam': r['cam'], 'data': dict(data, event_stream=events, frame_stamps=stamps)},
                          args, 1.0, device='cpu')
    assert from_stream.event_filter_stats['n_out'] < from_stream.event_filter_stats['n_in'] and plain.event_filter_stats is None
    differs = False
    for i in range(len(from_png)):
        a, b = from_png[i], from_stream[i]
        assert all(torch.equal(u, v) for u, v in zip(a[1:], b[1:]))
        differs = differs or not torch.equal(plain[i][3], b[3])
    assert differs
    with pytest.raises(ValueError):
        D.get_dataset({'dataset': 'rpg_event', 'cam': r['cam'],
                       'data': dict(data, event_stream=events, frame_stamps=stamps, event_filter=dict(rho=1.0))}, args, 1.0, device='cpu')
    # without data.event_stream the mapping is not honoured
    ignored = D.get_dataset({'dataset': 'rpg_event', 'cam': r['cam'], 'data': dict(data, event_folder=got_dir, event_filter=dict(OPTIONS))},
                            args, 1.0, device='cpu')
    assert torch.equal(ignored[1][3], from_png[1][3])


def test_filter_stream_leaves_its_input_unchanged():
    from evennicer_slam_amd.event_filter import filter_stream
    c = FC.cases()['long_run']
    stream = _stream(c)
    kept, stats, classes = filter_stream(stream, c['H'], c['W'], c['rho'], c['dt'], return_classes=True)
    assert all(np.array_equal(_bits(a), _bits(c[k])) for k, a in zip('txyp', stream.arrays()))
    assert len(kept) == stats['n_out'] == int((classes == 0).sum()) and stats == FC.reference('long_run')['counters']


def test_exports_header_and_cpu_tensors_are_refused():
    import evennicer_slam_amd as E
    from evennicer_slam_amd import functional as EF
    from evennicer_slam_amd._lib import EnslamError
    header = open(os.path.join(ROOT, "include", "enslam_hip.h")).read()
    handle = ctypes.CDLL(E.LIB_PATH)
    for name in EXPORTS:
        assert name in E._lib.EXPORTS and re.search(r"\b%s\s*\(" % name, header) and hasattr(handle, name), name
    for k, name in enumerate(YF.NAMES):
        assert re.search(r"#define ENSLAM_EVENT_%s %d\b" % (name.upper(), k), header) and EF.EVENT_CLASSES[k] == name
    z = torch.zeros(3, dtype=torch.float64)
    with pytest.raises(EnslamError):
        EF.event_pixel_counts(z, torch.zeros(3, dtype=torch.uint16), torch.zeros(3, dtype=torch.uint16), torch.zeros(3, dtype=torch.uint8), 4, 5)
