"""CPU tests of the noisy event sensor (event_sim.EventNoise): the yardstick tests/event_noise_numpy.py against hand-worked
pixels and the Philox known answers, the library's numpy route against the yardstick on the cases of
tests/event_noise_cases.py (bit-equal: image, L_ref, t_last and stream), the case conditions, the refractory property, the
shot-noise count, the tools and the declarations."""
import ctypes
import importlib.util
import math
import os
import re

import numpy as np
import pytest
import torch

from tests import event_noise_cases as NC
from tests import event_noise_numpy as YN
from tests import event_sim_cases as C
from tests import event_sim_numpy as Y
from tests import event_stream_cases as SC
from tests import event_stream_numpy as YS
from tests.viz_cases import CAM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPORTS = ("enslam_event_noise_bytes", "enslam_event_noisy_images_count", "enslam_event_noisy_images_emit",
           "enslam_event_noisy_boxroom_count", "enslam_event_noisy_boxroom_emit")
PHILOX_KAT = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
              ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
              ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]


def _tool(name):
    spec = importlib.util.spec_from_file_location(name + "_tool", os.path.join(ROOT, "tools", name + ".py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    return tool


def _noise(setting):
    from evennicer_slam_amd.event_sim import EventNoise
    return EventNoise(**NC.SETTINGS[setting])


def _sim(c, H, W, noise, device='cpu'):
    from evennicer_slam_amd.event_sim import EventSimulator
    return EventSimulator(H, W, c_pos=c['c_pos'], c_neg=c['c_neg'], sigma_c=c.get('sigma_c', 0.0), substeps=c['K'], eps=C.EPS,
                          seed=c.get('seed', 0), device=device, noise=noise)


def _image_ref(name, setting, sim):
    if C.image_cases()[name]['sigma_c'] > 0:
        return NC.image_noise_reference(name, setting, sim.c_pos_map.cpu().numpy(), sim.c_neg_map.cpu().numpy())
    return NC.image_noise_reference(name, setting)


def _same_step(r, events, sim, stream):
    t, x, y, p = stream.numpy()
    return (np.array_equal(events.cpu().numpy(), r['events']) and np.array_equal(sim.state.cpu().numpy(), r['ref'])
            and np.array_equal(sim.last_event_time.cpu().numpy(), r['t_last']) and np.array_equal(t, r['t'])
            and np.array_equal(x, r['x']) and np.array_equal(y, r['y']) and np.array_equal(p, r['p']))


def test_philox_known_answers():
    from evennicer_slam_amd.event_sim import philox4x32
    for counter, key, want in PHILOX_KAT:
        assert YN.philox4x32(counter, key) == want
        assert tuple(int(v) for v in philox4x32(counter, key)) == want
    # on arrays: every row its own block
    ctr = [np.array([c[0][i] for c in PHILOX_KAT], dtype=np.uint64) for i in range(4)]
    key = [np.array([c[1][i] for c in PHILOX_KAT], dtype=np.uint64) for i in range(2)]
    got = philox4x32(ctr, key)
    assert [tuple(int(w[j]) for w in got) for j in range(3)] == [c[2] for c in PHILOX_KAT]
    assert YN.uniform(0) == 2.0 ** -33 and YN.uniform(0xffffffff) == 1.0 - 2.0 ** -33


def _run_levels(levels_per_interval, stamps, K, c, **noise):
    """the yardstick and the library's numpy route over hand-made level images of one pixel row; returns both"""
    from evennicer_slam_amd import event_sim as S
    first = np.asarray(levels_per_interval[0][0], dtype=np.float64)
    sensor = YN.NoisySensor(first, c, c, **noise)
    en = S.EventNoise(**noise)
    ref, t_last = first.copy(), np.full(first.shape, -np.inf)
    out = []
    for i, (levels, (t_a, t_b)) in enumerate(zip(levels_per_interval, stamps)):
        levels = [np.asarray(v, dtype=np.float64) for v in levels]
        r = YN.step_levels(sensor, levels, t_a, t_b)
        pos, neg = np.zeros_like(ref), np.zeros_like(ref)
        parts = [S.noisy_substep(s, K, t_a, t_b, ref, t_last, neg, pos, c, c, levels[s - 1], levels[s], en, i) for s in range(1, K + 1)]
        t, x, y, p = S._stream_of(parts, first.shape[1]).numpy()
        assert np.array_equal(t, r['t']) and np.array_equal(x, r['x']) and np.array_equal(p, r['p'])
        assert np.array_equal(ref, r['ref']) and np.array_equal(t_last, r['t_last']) and np.array_equal(S.saturate(neg, pos), r['events'])
        out.append(r)
    return out


def test_hand_worked_leak():
    """Constant level 0, C = 0.1, K = 2 over [0, 1]: delta = 0.5, lambda = 1 Hz gives g = 0.5.  Sub-step 1: L_ref = -0.05, d =
    0.05, nothing.  Sub-step 2: L_ref = -0.1, d = 0.1 >= C: one positive event, L_ref back to 0; the level does not move, so
    the quotient is 0 / 0, f = 0, and the event leaves at the start of sub-step 2: t = 0.5.  One event per second = lambda."""
    zero = np.zeros((1, 1))
    r = _run_levels([[zero, zero, zero]] * 3, [(0.0, 1.0), (1.0, 2.0), (2.0, 3.0)], 2, 0.1, leak_rate=1.0)
    for i, step in enumerate(r):
        assert step['t'].tolist() == [i + 0.5] and step['p'].tolist() == [1] and step['events'].tolist() == [[[0, 1]]]
        assert step['ref'].tolist() == [[0.0]] and step['t_last'].tolist() == [[i + 0.5]]
    # the product, then the difference: g * C = 0.05 is subtracted, twice
    c = r[0]['candidates']
    assert c.shape[0] == 1 and c[0, 1] == 2 and c[0, 4] == 0


def test_hand_worked_refractory_across_the_boundary():
    """Level 0 -> 1 over [0, 1] and 1 -> 2 over [1, 2], C = 0.3, K = 1: candidates at 0.3, 0.6, 0.9, then 1.2, 1.5, 1.8.
    rho = 0.35: 0.3 leaves; 0.6 is 0.3 after it, suppressed; 0.9 leaves.  Next interval: 1.2 is 0.3 after the 0.9 carried in
    t_last, suppressed; 1.5 leaves; 1.8 suppressed.  L_ref moves by all three candidates each time."""
    lv = [np.array([[float(v)]]) for v in (0, 1, 2)]
    r = _run_levels([[lv[0], lv[1]], [lv[1], lv[2]]], [(0.0, 1.0), (1.0, 2.0)], 1, 0.3, refractory=0.35)
    assert np.allclose(r[0]['t'], [0.3, 0.9], rtol=0, atol=1e-12) and np.allclose(r[1]['t'], [1.5], rtol=0, atol=1e-12)
    assert r[0]['events'].tolist() == [[[0, 2]]] and r[1]['events'].tolist() == [[[0, 1]]]
    assert abs(r[0]['ref'][0, 0] - 0.9) < 1e-12 and abs(r[1]['ref'][0, 0] - 1.8) < 1e-12
    assert r[0]['candidates'][:, 5].tolist() == [1, 0, 1] and r[1]['candidates'][:, 5].tolist() == [0, 1, 0]
    assert abs(r[1]['candidates'][0, 6] - 0.9) < 1e-12              # suppressed through the t_last of the interval before
    assert abs(r[1]['t_last'][0, 0] - 1.5) < 1e-12
    # rho = 0.3 exactly at the boundary of ">=" is not worked by hand (0.6 - 0.3 rounds); rho = 0: everything leaves
    r0 = _run_levels([[lv[0], lv[1]], [lv[1], lv[2]]], [(0.0, 1.0), (1.0, 2.0)], 1, 0.3)
    assert [len(s['t']) for s in r0] == [3, 3]


def test_hand_worked_uniform_to_time_mapping():
    """A quiet pixel row (no signal), K = 2, q = 0.5: every block's words written out.  Negative noise iff (w0 + 0.5) 2^-32 <
    q at f = (w1 + 0.5) 2^-32, positive iff (w2 + 0.5) 2^-32 < q at f = (w3 + 0.5) 2^-32, t = t_a + (((s - 1) + f) / K)(t_b -
    t_a); within a sub-step in ascending t."""
    W, K, t_a, t_b, seed, interval = 7, 2, 3.0, 3.5, (5 << 32) | 9, 0
    quiet = np.full((1, W), -1.0)
    r = _run_levels([[quiet] * (K + 1)], [(t_a, t_b)], K, 0.2, shot_rate=0.5 / ((t_b - t_a) / K), seed=seed)[0]
    want = []
    for o in range(W):
        for s in range(1, K + 1):
            w = YN.philox4x32((o, interval, s, 0), (9, 5))
            here = []
            if (w[0] + 0.5) / 2.0 ** 32 < 0.5:
                here.append((t_a + (((s - 1) + (w[1] + 0.5) / 2.0 ** 32) / K) * (t_b - t_a), o, 0))
            if (w[2] + 0.5) / 2.0 ** 32 < 0.5:
                here.append((t_a + (((s - 1) + (w[3] + 0.5) / 2.0 ** 32) / K) * (t_b - t_a), o, 1))
            want += sorted(here, key=lambda e: e[0])
    assert len(want) >= W and [(float(t), int(x), int(p)) for t, x, p in zip(r['t'], r['x'], r['p'])] == want
    assert bool(np.all(r['ref'] == -1.0))                           # noise does not move L_ref
    assert (4.0 + 0.5) / 2.0 ** 32 == YN.uniform(4)


def test_hand_worked_merge_order_and_ties():
    """An interval of one float64 spacing: t_a = 2^60, t_b = t_a + 256, so every time rounds to t_a (offset below 128) or to
    t_b: ties everywhere.  K = 1, q = 1: both noise candidates exist.  Level 0 -> 1 at C = 0.3: signal at offsets 76.8 (t_a),
    153.6 and 230.4 (t_b).  The order must be: signal at t_a, noise at t_a (negative first), signal at t_b, noise at t_b
    (negative first) -- on equal t signal before noise, negative noise before positive noise."""
    t_a = 2.0 ** 60
    t_b = t_a + 256.0
    lv = [np.array([[0.0]]), np.array([[1.0]])]
    seen = set()
    for seed in range(24):
        r = _run_levels([lv], [(t_a, t_b)], 1, 0.3, shot_rate=1.0 / 256.0, seed=seed)[0]
        w = YN.philox4x32((0, 0, 1, 0), (seed, 0))
        neg_late, pos_late = YN.uniform(w[1]) * 256.0 > 128.0, YN.uniform(w[3]) * 256.0 > 128.0
        want = [(t_a, 1)] + [(t_a, q) for q, late in ((0, neg_late), (1, pos_late)) if not late]
        want += [(t_b, 1), (t_b, 1)] + [(t_b, q) for q, late in ((0, neg_late), (1, pos_late)) if late]
        assert list(zip(r['t'].tolist(), r['p'].tolist())) == want, seed
        seen.add((neg_late, pos_late))
    assert seen == {(False, False), (False, True), (True, False), (True, True)}     # a positive one before a negative one included


@pytest.mark.parametrize("name", NC.IMAGE_NAMES)
def test_off_equals_the_stream_yardstick(name):
    from evennicer_slam_amd.event_sim import EventNoise
    sim = _sim(C.image_cases()[name], *C.image_cases()[name]['shape'], EventNoise())
    maps = (sim.c_pos_map.numpy(), sim.c_neg_map.numpy()) if sim.c_pos_map is not None else (None, None)
    for a, b in zip(_image_ref(name, 'off', sim), SC.image_stream_reference(name, *maps)):
        assert all(np.array_equal(a[k], b[k]) for k in ('t', 'x', 'y', 'p', 'events', 'ref', 'total'))


@pytest.mark.parametrize("setting", sorted(NC.SETTINGS))
@pytest.mark.parametrize("name", NC.IMAGE_NAMES)
def test_numpy_route_is_bit_equal_on_images(name, setting):
    from evennicer_slam_amd import event_stream as ES
    c = C.image_cases()[name]
    sim = _sim(c, *c['shape'], _noise(setting))
    ref = _image_ref(name, setting, sim)
    sim.reset(c['images'][0])
    assert bool(torch.isneginf(sim.last_event_time).all())
    image_only = _sim(c, *c['shape'], _noise(setting)).reset(c['images'][0])
    H, W = c['shape']
    for i, (prev, cur) in enumerate(zip(c['images'][:-1], c['images'][1:])):
        r = ref[i]
        events, stream = sim.step_images(prev, cur, stamps=r['stamps'])
        assert _same_step(r, events, sim, stream), (name, setting, i)
        assert torch.equal(image_only.step_images(prev, cur, stamps=r['stamps'], stream=False), events)
        assert torch.equal(image_only.state, sim.state) and torch.equal(image_only.last_event_time, sim.last_event_time)
        # the round trip: the stream's bins are the image
        assert torch.equal(ES.accumulate(stream, [r['stamps'][0] - 1.0, r['stamps'][1]], H, W)[0], events)
    if name == "37x53_grey_K5" and setting == "off":
        assert int(ref[0]['total'][0, 0]) == 345


@pytest.mark.parametrize("setting", sorted(NC.SETTINGS))
@pytest.mark.parametrize("name", NC.ANALYTIC_NAMES)
def test_numpy_route_is_bit_equal_on_the_analytic_room(name, setting):
    c, ref, frames, room = C.ANALYTIC[name], NC.analytic_noise_reference(name, setting), C.analytic_poses(name), C.demo_room()
    sim = _sim(dict(c_pos=c['c'], c_neg=c['c'], K=c['K']), CAM['H'], CAM['W'], _noise(setting)).reset((room, frames[0], CAM))
    for i, r in enumerate(ref):
        events, stream = sim.step_scene(room, frames[i], frames[i + 1], CAM, stamps=r['stamps'])
        assert _same_step(r, events, sim, stream), (name, setting, i)
    if setting == 'off':
        for a, b in zip(ref, SC.analytic_stream_reference(name)):
            assert all(np.array_equal(a[k], b[k]) for k in ('t', 'x', 'y', 'p', 'events', 'ref'))


def test_case_conditions():
    """the conditions of tests/event_noise_cases.py on every image case, the figures of all cases printed, and the yardstick
    alone within the cap of left-out pixels wherever the device's own log / sin decides"""
    for name in NC.IMAGE_NAMES + NC.ANALYTIC_NAMES:
        image = name in NC.IMAGE_NAMES
        for setting in NC.SETTINGS:
            ref = NC.image_noise_reference(name, setting) if image else NC.analytic_noise_reference(name, setting)
            f = NC.conditions(ref)
            print(name, setting, f)
            assert f['left_out'] <= C.MAX_LEFT_OUT * ref[0]['margin'].size, (name, setting, f)
            if not image:
                continue
            if setting.startswith('refr_'):
                assert f['suppressed_share'] >= 0.10, (name, setting, f)
            if setting == 'refr_long':
                assert f['carried'] >= 1, (name, f)
            if setting == 'shot':
                assert f['noise_between_signal'] >= 1, (name, f)
            if setting == 'leak' and ref[0]['margin'].size > 1:
                assert f['quiet_pixel_positive'] >= 1, (name, f)
            if setting == 'off':
                assert f['suppressed'] == 0


@pytest.mark.parametrize("setting", ["refr_short", "refr_long", "all"])
def test_consecutive_events_of_a_pixel_are_a_refractory_period_apart(setting):
    name = "37x53_grey_K5"
    c = C.image_cases()[name]
    sim = _sim(c, *c['shape'], _noise(setting)).reset(c['images'][0])
    rho, W = NC.SETTINGS[setting]['refractory'], c['shape'][1]
    ts, px = [], []
    for i, (prev, cur) in enumerate(zip(c['images'][:-1], c['images'][1:])):
        t, x, y, _ = sim.step_images(prev, cur, stamps=NC.stamps(i))[1].numpy()
        ts.append(t), px.append(y.astype(np.int64) * W + x)
    t, px = np.concatenate(ts), np.concatenate(px)
    order = np.argsort(px, kind='stable')                           # keeps the intervals, and the order within them
    t, px = t[order], px[order]
    gaps = np.diff(t)[px[1:] == px[:-1]]
    print(setting, "events", t.size, "smallest gap", float(gaps.min()), "rho", rho)
    assert gaps.size > 1000 and bool(np.all(gaps >= rho))


def test_shot_noise_count():
    """A constant 64 x 64 image, 20 intervals of 0.05 s, K = 2, r = 8 Hz: no signal, no filter, so the stream is the noise.
    N = 64 * 64 * 2 * 20 * 2 Bernoulli draws of q = r * 0.025 = 0.2; the count must lie within 5 sqrt(N q (1 - q)) of N q (five
    standard deviations of the binomial: a bound from the model; the outcome itself is deterministic)."""
    from evennicer_slam_amd.event_sim import EventNoise, EventSimulator
    H = W = 64
    img = np.full((H, W), 120, dtype=np.uint8)
    sim = EventSimulator(H, W, c_pos=0.02, c_neg=0.02, substeps=2, device='cpu', noise=EventNoise(shot_rate=8.0, seed=3)).reset(img)
    n, by_polarity = 0, np.zeros(2, dtype=np.int64)
    for i in range(20):
        events, stream = sim.step_images(img, img, stamps=NC.stamps(i))
        n += len(stream)
        by_polarity += np.bincount(stream.numpy()[3], minlength=2)
        assert int(events.sum()) == len(stream)
    q = 8.0 * ((NC.stamps(0)[1] - NC.stamps(0)[0]) / 2)
    N = H * W * 2 * 20 * 2
    bound = 5.0 * math.sqrt(N * q * (1.0 - q))
    print("shot noise:", n, "events, expected", N * q, "+-", bound, "by polarity", by_polarity.tolist())
    assert abs(n - N * q) <= bound
    assert all(abs(v - N * q / 2) <= 5.0 * math.sqrt(N / 2 * q * (1.0 - q)) for v in by_polarity)
    assert np.array_equal(sim.state.numpy(), Y.table(1e-3)[img])   # L_ref untouched


def test_interval_index_and_seed_decide_the_noise():
    from evennicer_slam_amd.event_sim import EventNoise, EventSimulator
    img = np.full((9, 11), 120, dtype=np.uint8)

    def run(seed, steps):
        sim = EventSimulator(9, 11, substeps=3, device='cpu', noise=EventNoise(shot_rate=20.0, seed=seed)).reset(img)
        return [sim.step_images(img, img, stamps=(1.0, 1.05)) for _ in range(steps)]

    a, b = run(5, 2), run(5, 2)
    assert all(torch.equal(u[0], v[0]) and all(np.array_equal(p, q) for p, q in zip(u[1].numpy(), v[1].numpy())) for u, v in zip(a, b))
    assert not torch.equal(a[0][0], a[1][0])                       # the same stamps, the next interval index: other noise
    assert not torch.equal(a[0][0], run(6, 1)[0][0])               # another seed
    assert not torch.equal(a[0][0], run(5 + (1 << 32), 1)[0][0])   # the high key word counts
    sim = EventSimulator(9, 11, substeps=3, device='cpu', noise=EventNoise(shot_rate=20.0, seed=5)).reset(img)
    sim.step_images(img, img, stamps=(1.0, 1.05))
    sim.reset(img)                                                  # the counter starts again, and t_last
    again = sim.step_images(img, img, stamps=(1.0, 1.05))
    assert torch.equal(again[0], a[0][0]) and bool(torch.isneginf(sim.last_event_time).sum() == (again[0].sum(-1) == 0).sum())


def test_checks():
    from evennicer_slam_amd._lib import EnslamError
    from evennicer_slam_amd.event_sim import EventNoise, EventSimulator
    from evennicer_slam_amd.synthetic import write_demo_sequence
    img = np.zeros((4, 5), dtype=np.uint8)
    sim = EventSimulator(4, 5, device='cpu', noise=EventNoise(refractory=1e-3)).reset(img)
    with pytest.raises(EnslamError, match="stamps"):
        sim.step_images(img, img)
    with pytest.raises(EnslamError, match="stamps"):
        sim.step_scene(C.demo_room(), np.eye(4), np.eye(4), dict(CAM, H=4, W=5))
    for kw in (dict(refractory=-1.0), dict(leak_rate=float('inf')), dict(shot_rate=float('nan')), dict(seed=-1), dict(seed=1 << 64)):
        with pytest.raises(EnslamError):
            EventNoise(**kw)
    with pytest.raises(EnslamError):
        EventSimulator(4, 5, device='cpu', noise=dict(refractory=1.0))
    loud = EventSimulator(4, 5, substeps=2, device='cpu', noise=EventNoise(shot_rate=100.0)).reset(img)
    with pytest.raises(EnslamError, match="sub-steps"):
        loud.step_images(img, img, stamps=(0.0, 0.05))               # q = 2.5
    assert EventSimulator(4, 5, device='cpu').last_event_time is None
    with pytest.raises(ValueError, match="stamps"):
        write_demo_sequence("unused", 3, dict(CAM, H=4, W=5), events='simulate', noise=EventNoise(refractory=1e-3))


def test_simulate_tool_with_noise_then_events_to_frames(tmp_path, capsys):
    """tools/simulate_events.py CONFIG with the noise options and --stream: the tool's stream and event folder are those of
    the simulator driven directly, and tools/events_to_frames.py makes the same folder from the stream, byte for byte.
    (Refractory period and shot noise: a leak event of an unchanged pixel sits exactly on the start of a sub-step, at the
    first one on the frame time itself, which the accumulator's rule gives to the frame before.)"""
    import yaml
    from evennicer_slam_amd import event_stream as ES
    from evennicer_slam_amd.event_sim import EventNoise, EventSimulator
    from tests.test_event_stream_cpu import _demo_recording
    r = _demo_recording(tmp_path)
    cfg = {'dataset': 'rpg_event', 'scale': 1, 'data': {'input_folder': r['inp'], 'event_folder': r['evf']}, 'cam': r['cam']}
    path = str(tmp_path / 'seq.yaml')
    with open(path, 'w') as f:
        yaml.safe_dump(cfg, f)
    out, stream_path = str(tmp_path / 'sim_events'), str(tmp_path / 'sim_events.txt')
    stamps = os.path.join(r['root'], 'images.txt')
    tool = _tool("simulate_events")
    info = tool.main([path, '--out', out, '--device', 'cpu', '--c-pos', '0.05', '--c-neg', '0.05', '--substeps', '4', '--stream', stream_path,
                      '--stamps', stamps, '--refractory', '0.004', '--shot-rate', '6', '--noise-seed', '11'])
    capsys.readouterr()
    assert info['noise'] == dict(refractory=0.004, leak_rate=0.0, shot_rate=6.0, seed=11)
    # the simulator driven directly
    rng = np.random.default_rng(21)                                 # the frames of _demo_recording, drawn again
    greys = [rng.integers(0, 256, (r['H'], r['W']), dtype=np.uint8)]
    for _ in range(r['n'] - 1):
        greys.append(np.clip(greys[-1].astype(np.int64) + rng.integers(-40, 41, (r['H'], r['W'])), 0, 255).astype(np.uint8))
    sim = EventSimulator(r['H'], r['W'], c_pos=0.05, c_neg=0.05, substeps=4, device='cpu',
                         noise=EventNoise(refractory=0.004, shot_rate=6.0, seed=11)).reset(greys[0])
    streams, images = [], []
    for i in range(1, r['n']):
        ev, st = sim.step_images(greys[i - 1], greys[i], stamps=(r['times'][i - 1], r['times'][i]))
        assert bool((st.t > r['times'][i - 1]).all())               # case condition: no event rounds to the frame's own time
        streams.append(st), images.append(ev.numpy())
    whole = ES.EventStream.concatenate(streams).time_sorted()
    plain = sum(int(im.sum()) for im in r['images'])
    assert info['stream_events'] == len(whole) and len(whole) != plain and bool(whole.p.numel())
    got = ES.read_events_txt(stream_path)
    assert all(np.array_equal(a, b) for a, b in zip(got.numpy(), whole.numpy()))
    again = str(tmp_path / 'again')
    _tool("events_to_frames").main([stream_path, stamps, '--out', again, '--height', str(r['H']), '--width', str(r['W']), '--device', 'cpu'])
    capsys.readouterr()
    assert len(os.listdir(again)) == len(os.listdir(out)) == r['n'] - 1
    for name in sorted(os.listdir(out)):
        with open(os.path.join(out, name), 'rb') as a, open(os.path.join(again, name), 'rb') as b:
            assert a.read() == b.read(), name
    # --leak-rate through the tool: its folder and stream are the simulator's own (what binning by frame times makes of leak
    # events that sit on a frame time is pinned by test_leak_events_on_a_frame_time_bin_into_the_frame_before)
    out3, stream3 = str(tmp_path / 'sim_events_3'), str(tmp_path / 'sim_events_3.npz')
    info = tool.main([path, '--out', out3, '--device', 'cpu', '--c-pos', '0.05', '--c-neg', '0.05', '--substeps', '4', '--stream', stream3,
                      '--stamps', stamps, '--leak-rate', '40'])
    capsys.readouterr()
    leaky = EventSimulator(r['H'], r['W'], c_pos=0.05, c_neg=0.05, substeps=4, device='cpu',
                           noise=EventNoise(leak_rate=40.0)).reset(greys[0])
    steps = [leaky.step_images(greys[i - 1], greys[i], stamps=(r['times'][i - 1], r['times'][i])) for i in range(1, r['n'])]
    want = ES.EventStream.concatenate([st for _, st in steps]).time_sorted()
    assert info['stream_events'] == len(want) > len(r['whole'])
    assert all(np.array_equal(a, b) for a, b in zip(ES.load_stream(stream3).numpy(), want.numpy()))
    from evennicer_slam_amd import datasets as D
    for i, (ev, _) in enumerate(steps, start=1):
        shown = D._imread_rgb(os.path.join(out3, 'event%06d.png' % i))
        assert np.array_equal(shown[:, :, 1], ev.numpy()[:, :, 0]) and np.array_equal(shown[:, :, 0], ev.numpy()[:, :, 1])
    # without --stream the noisy tool still takes the frame times, and writes the same folder
    out2 = str(tmp_path / 'sim_events_2')
    tool.main([path, '--out', out2, '--device', 'cpu', '--c-pos', '0.05', '--c-neg', '0.05', '--substeps', '4', '--stamps', stamps,
               '--refractory', '0.004', '--shot-rate', '6', '--noise-seed', '11'])
    capsys.readouterr()
    for name in sorted(os.listdir(out)):
        with open(os.path.join(out, name), 'rb') as a, open(os.path.join(out2, name), 'rb') as b:
            assert a.read() == b.read(), name


def test_demo_sequence_with_noise(tmp_path):
    from evennicer_slam_amd import event_stream as ES
    from evennicer_slam_amd.event_sim import EventNoise
    from evennicer_slam_amd.synthetic import write_demo_sequence
    cam = dict(H=12, W=16, fx=14.0, fy=14.0, cx=7.5, cy=5.5)
    streams, times = [], [0.0, 0.04, 0.08]
    (inp, evf), _ = write_demo_sequence(str(tmp_path / 'demo'), 3, cam, events='simulate', stamps=times, streams=streams,
                                        noise=EventNoise(shot_rate=50.0, seed=2))
    assert len(streams) == 2 and all(len(s) > 0 for s in streams) and len(os.listdir(evf)) >= 2
    plain = []
    write_demo_sequence(str(tmp_path / 'plain'), 3, cam, events='simulate', stamps=times, streams=plain)
    assert sum(len(s) for s in streams) > sum(len(s) for s in plain)
    assert isinstance(streams[0], ES.EventStream)


def test_declarations():
    import evennicer_slam_amd as E
    from evennicer_slam_amd import _lib as L
    from evennicer_slam_amd import functional as EF
    header = open(os.path.join(ROOT, "include", "enslam_hip.h")).read()
    handle = ctypes.CDLL(E.LIB_PATH)
    for name in EXPORTS:
        assert name in L.EXPORTS and re.search(r"\b%s\s*\(" % name, header) and hasattr(handle, name), name
    assert "typedef struct enslam_event_noise" in header
    assert L.lib().enslam_event_noise_bytes() == ctypes.sizeof(L.EventNoiseParams) == 40
    p = EF.event_noise_params("test", dict(refractory=1e-3, leak_rate=30.0, shot_rate=8.0, seed=NC.ALL_SEED, interval=7), 5, (10.0, 10.05))
    delta = (10.05 - 10.0) / 5
    assert (p.refractory, p.leak, p.shot, p.seed, p.interval) == (1e-3, 30.0 * delta, 8.0 * delta, NC.ALL_SEED, 7)
    with pytest.raises(L.EnslamError):
        EF.event_noise_params("test", dict(shot_rate=1000.0), 1, (0.0, 1.0))
    state = torch.zeros((4, 5), dtype=torch.float64)
    img = torch.zeros((4, 5), dtype=torch.uint8)
    with pytest.raises(L.EnslamError):                             # CPU tensors are refused: there is no fallback
        EF.event_noisy_images(img, img, state, state.clone(), (0.0, 1.0), dict(refractory=1e-3), lut=torch.zeros(256, dtype=torch.float64))
    with pytest.raises(L.EnslamError):
        EF.event_noisy_boxroom(C.demo_room(), np.tile(np.eye(4), (3, 1, 1)), dict(CAM, H=4, W=5), state, state.clone(), (0.0, 1.0),
                               dict(refractory=1e-3))


def test_leak_events_on_a_frame_time_bin_into_the_frame_before():
    """What the tool round trip above leaves out, pinned: with leak, an event of a pixel whose level does not move has f = 0; at
    the first sub-step it carries the frame time t_a itself, and the accumulator's rule (edges[b] < t <= edges[b+1]) gives it to
    the frame before.  Binning the whole stream by the frame times returns the simulator's images except for exactly those
    events."""
    from evennicer_slam_amd import event_stream as ES
    from evennicer_slam_amd.event_sim import EventNoise, EventSimulator
    H, W, n = 8, 10, 6
    rng = np.random.default_rng(33)
    greys = [rng.integers(40, 200, (H, W), dtype=np.uint8)]
    for _ in range(n - 1):
        step = rng.integers(-20, 21, (H, W))
        step[rng.random((H, W)) < 0.5] = 0
        greys.append(np.clip(greys[-1].astype(np.int64) + step, 0, 255).astype(np.uint8))
    times = [2.0 + 0.04 * i for i in range(n)]
    sim = EventSimulator(H, W, c_pos=0.05, c_neg=0.05, substeps=4, device='cpu', noise=EventNoise(leak_rate=40.0)).reset(greys[0])
    images, streams, on_edge = [], [], []
    for i in range(1, n):
        ev, st = sim.step_images(greys[i - 1], greys[i], stamps=(times[i - 1], times[i]))
        t, x, y, p = st.numpy()
        hit = t == times[i - 1]
        moved = np.zeros((H, W, 2), dtype=np.int64)
        np.add.at(moved, (y[hit].astype(np.int64), x[hit].astype(np.int64), p[hit].astype(np.int64)), 1)
        images.append(ev.numpy().astype(np.int64)), streams.append(st), on_edge.append(moved)
        assert int(ev.max()) < 255
    assert sum(int(m.sum()) for m in on_edge) > 0 and all(int(m[..., 0].sum()) == 0 for m in on_edge)     # leak events are positive
    binned = ES.accumulate(ES.EventStream.concatenate(streams).time_sorted(), times, H, W).numpy().astype(np.int64)
    for i in range(n - 1):
        later = on_edge[i + 1] if i + 1 < n - 1 else 0
        assert np.array_equal(binned[i], images[i] - on_edge[i] + later), i
