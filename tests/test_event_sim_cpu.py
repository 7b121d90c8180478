"""No GPU: the event-camera simulator's yardstick (tests/event_sim_numpy.py) against hand-worked pixels and the model's
invariant, the library's numpy route (event_sim.EventSimulator on the CPU) bit-equal to the yardstick on every case of
tests/event_sim_cases.py, the conditions those cases promise, pose interpolation, the simulated demo sequence through the
writer and the Replica_event reader, and tools/simulate_events.py."""
import ctypes
import glob
import importlib.util
import json
import math
import os
import types

import numpy as np
import pytest
import torch

from tests import event_sim_cases as C
from tests import event_sim_numpy as Y
from tests.viz_cases import CAM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPORTS = ("enslam_event_sim_plan_bytes", "enslam_event_sim_max_substeps", "enslam_event_sim_images", "enslam_event_sim_boxroom")


def _tool(name):
    spec = importlib.util.spec_from_file_location(name + "_tool", os.path.join(ROOT, "tools", name + ".py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    return tool


def _level(v, eps=1e-3):
    return math.log(v / 255.0 + eps)


# ---- the yardstick itself ---------------------------------------------------------------------------------------------------
def test_yardstick_hand_worked_pixels():
    """One row of pixels worked by hand: unchanged / black -> white at C = 0.02 (345 thresholds, saturated) / 40 -> 90 at
    C_pos = 0.25 (d = 0.8074: three crossings in one sub-step) / 90 -> 40 at C_neg = 0.1 (eight) / 100 -> 105 at a threshold that
    is this step's d exactly (one event) and at the next float above it (none)."""
    prev = np.array([[77, 0, 40, 90, 100, 100]], dtype=np.uint8)
    cur = np.array([[77, 255, 90, 40, 105, 105]], dtype=np.uint8)
    cp = np.array([[0.02, 0.02, 0.25, 0.25, C.C_POS_EXACT, np.nextafter(C.C_POS_EXACT, 1.0)]])
    cn = np.array([[0.02, 0.02, 0.1, 0.1, 0.02, 0.02]])
    table = Y.table(1e-3)
    assert all(abs(table[v] - _level(v)) <= 1e-15 for v in (0, 40, 77, 90, 100, 105, 255))
    s = Y.Sensor(Y.level_of_image(prev, 1e-3), cp, cn)
    ev = Y.step_images(s, prev, cur, 1, 1e-3)
    assert ev.dtype == np.uint8 and ev.shape == (1, 6, 2)
    assert ev[0, :, 1].tolist() == [0, 255, 3, 0, 1, 0]               # +
    assert ev[0, :, 0].tolist() == [0, 0, 0, 8, 0, 0]                 # -
    d_bw = _level(255) - _level(0)
    assert math.floor(d_bw / 0.02) == 345 and abs(d_bw - 6.90875) < 1e-5
    assert s.ref[0, 0] == table[77]
    assert s.ref[0, 1] == table[0] + 345 * 0.02                        # moved by the unsaturated count
    assert s.ref[0, 2] == table[40] + 3 * 0.25 and s.ref[0, 3] == table[90] - 8 * 0.1
    assert s.ref[0, 4] == table[105] and s.ref[0, 5] == table[100]
    # five sub-steps of the 40 -> 90 pixel at C = 0.25: d_s = s / 5 * 0.8074 fires at s = 2, 4, 5, one event each
    s = Y.Sensor(Y.level_of_image(prev, 1e-3), 0.25, 0.1)
    ev = Y.step_images(s, prev, cur, 5, 1e-3)
    assert ev[0, 2].tolist() == [0, 3] and ev[0, 3].tolist() == [8, 0]
    assert abs(s.ref[0, 2] - (_level(40) + 0.75)) < 1e-15
    # the state is carried: the black -> white pixel, back to black, gives 345 or 344 negative events from a residual of
    # 0.00875, and the counts of a second interval do not include the first's
    s = Y.Sensor(Y.level_of_image(prev, 1e-3), 0.02, 0.02)
    Y.step_images(s, prev, cur, 1, 1e-3)
    back = Y.step_images(s, cur, prev, 1, 1e-3)
    assert back[0, 1].tolist() == [255, 0] and back[0, 0].tolist() == [0, 0]
    assert -0.02 < table[0] - s.ref[0, 1] < 0.02


def test_yardstick_rgb_luminance_and_margins():
    img = np.array([[[255, 0, 0], [0, 255, 0], [0, 0, 255], [10, 20, 30]]], dtype=np.uint8)
    L = Y.level_of_image(img, 1e-3)
    want = [math.log(0.299 + 1e-3), math.log(0.587 + 1e-3), math.log(0.114 + 1e-3),
            math.log((0.299 * (10 / 255.0) + 0.587 * (20 / 255.0)) + 0.114 * (30 / 255.0) + 1e-3)]
    assert np.abs(L[0] - np.array(want)).max() <= 1e-15
    # margins of d / C: below 1 the distance to 1, above it to the nearest integer
    m = Y.count_margin(np.array([0.0, 0.05, 0.19, 0.2, 0.25, 0.5, -0.31]), np.full(7, 0.2), np.full(7, 0.1))
    assert np.abs(m - np.array([1.0, 0.75, 0.05, 0.0, 0.25, 0.5, 0.1])).max() < 1e-12


@pytest.mark.parametrize("name", ["37x53_grey_K5", "37x53_rgb_K5_maps", "37x53_grey_K1_exact", "1x300_rgb_K1"])
def test_residual_stays_inside_the_thresholds(name):
    """-C_neg < L - L_ref < C_pos after every update, at every sub-step"""
    c = C.image_cases()[name]
    rng = np.random.default_rng(5)
    cp = c['c_pos'] if c['sigma_c'] == 0 else np.maximum(c['c_pos'] * (1 + c['sigma_c'] * rng.standard_normal(c['shape'])), 0.01)
    cn = c['c_neg'] if c['sigma_c'] == 0 else np.maximum(c['c_neg'] * (1 + c['sigma_c'] * rng.standard_normal(c['shape'])), 0.01)
    s = Y.Sensor(Y.level_of_image(c['images'][0], C.EPS), cp, cn)
    fired = 0
    for prev, cur in zip(c['images'][:-1], c['images'][1:]):
        la, lb = Y.level_of_image(prev, C.EPS), Y.level_of_image(cur, C.EPS)
        s.begin()
        for k in range(1, c['K'] + 1):
            lv = la + (k / c['K']) * (lb - la)
            s.visit(lv)
            r = lv - s.ref
            assert (r < s.c_pos).all() and (r > -s.c_neg).all()
        fired += int(s.pos.sum() + s.neg.sum())
    assert fired > 0


# ---- the cases ---------------------------------------------------------------------------------------------------------------
def test_image_case_set_contents():
    """what the docstring of the cases file promises: zero-change pixels, both polarities, the exact-threshold pixel,
    saturation"""
    cases = C.image_cases()
    assert {c['shape'] for c in cases.values()} == {(1, 1), (1, 300), (37, 53)}
    assert {c['K'] for c in cases.values()} == {1, 5} and {c['channels'] for c in cases.values()} == {1, 3}
    assert any(c['sigma_c'] > 0 for c in cases.values())
    for name, c in cases.items():
        assert len(c['images']) == 4 and all(im.dtype == np.uint8 for im in c['images'])
        if c['sigma_c'] > 0:
            continue
        steps = C.image_reference(name)
        first = steps[0][0].reshape(-1, 2)
        if c['c_pos'] == 0.02:
            assert first[0].tolist() == [0, 255] and steps[1][0].reshape(-1, 2)[0].tolist() == [255, 0]  # 345 > 255, both ways
        if first.shape[0] >= 4:
            assert all(not ev.reshape(-1, 2)[1].any() for ev, _ in steps)                           # the unchanged pixel
            assert (first[:, 0] > 0).any() and (first[:, 1] > 0).any()
            same = (c['images'][0] == c['images'][1]).reshape(first.shape[0], -1).all(axis=1)
            assert same.mean() > 0.2 and not first[same].any()
    for K in (1, 5):
        steps = C.image_reference(f"37x53_grey_K{K}_exact")
        assert steps[0][0].reshape(-1, 2)[2].tolist() == [0, 1]                                      # d == C_pos exactly
        assert steps[0][1].reshape(-1)[2] == Y.table(C.EPS)[105]
        assert C.image_reference(f"37x53_grey_K{K}")[0][0].reshape(-1, 2)[2].tolist() == [0, 2]      # the same pixel at 0.02


def test_analytic_case_conditions():
    """Margin condition: at most 0.1 % of a case's pixels left out by the margin rule (MARGIN = 1e-9, an estimate -- see the
    cases file).  Event-share condition: in every interval between 1 % and 50 % of the pixels carry an event.  The
    'silhouette' cases move the box's outline across pixels in every interval.  Also measured here for the record: the
    yardstick's frames against synthetic.BoxRoom.render."""
    room, worst_color, worst_depth = C.demo_room(), 0.0, 0.0
    for name in C.ANALYTIC:
        ref, poses = C.analytic_reference(name), C.analytic_poses(name)
        assert len(ref['steps']) >= 3
        box = [Y.render(Y.Room(room), poses[0], CAM)['on_box']] + [s['on_box'] for s in ref['steps']]
        for k, s in enumerate(ref['steps']):
            share = float((s['events'] != 0).any(axis=-1).mean())
            left = float(s['left_out'].mean())
            moved = int((box[k] != box[k + 1]).sum())
            print(f"{name} interval {k}: event share {share:.4f}, left out {left:.5f}, smallest margins count "
                  f"{s['count_margin'].min():.2e} geo {s['geo_margin'].min():.2e}, outline moved over {moved} pixels")
            assert 0.01 <= share <= 0.5
            assert left <= C.MAX_LEFT_OUT
            assert (s['events'][..., 0] > 0).any() and (s['events'][..., 1] > 0).any()
            if name.startswith("silhouette"):
                assert moved >= 5
            col, dep = room.render(torch.from_numpy(poses[k + 1]), CAM)
            worst_color = max(worst_color, float(np.abs(col.numpy() - s['color']).max()))
            worst_depth = max(worst_depth, float(np.abs(dep.numpy().astype(np.float64) - s['depth'].astype(np.float64)).max()))
        assert 0 < box[-1].mean() < 1
    print(f"yardstick frames against BoxRoom.render: colour {worst_color:.2e}, depth {worst_depth:.2e}")
    assert worst_color <= C.COLOR_TOL and worst_depth <= 1e-6


# ---- the library's numpy route ----------------------------------------------------------------------------------------------
def _cpu_sim(c, H, W):
    from evennicer_slam_amd.event_sim import EventSimulator
    return EventSimulator(H, W, c_pos=c['c_pos'], c_neg=c['c_neg'], sigma_c=c.get('sigma_c', 0.0), substeps=c['K'], eps=C.EPS,
                          seed=c.get('seed', 0), device='cpu')


@pytest.mark.parametrize("name", sorted(C.image_cases()))
def test_host_route_equals_yardstick_on_image_cases(name):
    c = C.image_cases()[name]
    sim = _cpu_sim(c, *c['shape'])
    if c['sigma_c'] > 0:
        steps = C.image_reference(name, sim.c_pos_map.numpy(), sim.c_neg_map.numpy())
    else:
        assert sim.c_pos_map is None
        steps = C.image_reference(name)
    assert sim.state is None
    sim.reset(c['images'][0])
    assert np.array_equal(sim.state.numpy(), Y.level_of_image(c['images'][0], C.EPS))
    for (ev, ref), prev, cur in zip(steps, c['images'][:-1], c['images'][1:]):
        got = sim.step_images(prev, cur)
        assert got.dtype == torch.uint8 and tuple(got.shape) == c['shape'] + (2,)
        assert np.array_equal(got.numpy(), ev)
        assert np.array_equal(sim.state.numpy(), ref)


@pytest.mark.parametrize("name", sorted(C.ANALYTIC))
def test_host_route_equals_yardstick_on_analytic_cases(name):
    c, ref, poses, room = C.ANALYTIC[name], C.analytic_reference(name), C.analytic_poses(name), C.demo_room()
    sim = _cpu_sim(dict(c_pos=c['c'], c_neg=c['c'], K=c['K']), CAM['H'], CAM['W'])
    sim.reset((room, poses[0], CAM))
    assert np.array_equal(sim.state.numpy(), ref['first'])
    for k, s in enumerate(ref['steps']):
        ev, col, dep = sim.step_scene(room, poses[k], torch.from_numpy(poses[k + 1]), CAM, want_frame=True)
        assert np.array_equal(ev.numpy(), s['events']) and np.array_equal(sim.state.numpy(), s['ref'])
        assert np.array_equal(col.numpy(), s['color']) and dep.dtype == torch.float32 and np.array_equal(dep.numpy(), s['depth'])
    again = _cpu_sim(dict(c_pos=c['c'], c_neg=c['c'], K=c['K']), CAM['H'], CAM['W']).reset((room, poses[0], CAM))
    assert np.array_equal(again.step_scene(room, poses[0], poses[1], CAM).numpy(), ref['steps'][0]['events'])


def test_threshold_maps_and_argument_checks():
    from evennicer_slam_amd._lib import EnslamError
    from evennicer_slam_amd.event_sim import EventSimulator
    a = EventSimulator(37, 53, c_pos=0.02, c_neg=0.03, sigma_c=0.6, seed=7, device='cpu')
    b = EventSimulator(37, 53, c_pos=0.02, c_neg=0.03, sigma_c=0.6, seed=7, device='cpu')
    other = EventSimulator(37, 53, c_pos=0.02, c_neg=0.03, sigma_c=0.6, seed=8, device='cpu')
    rng = np.random.default_rng(7)
    want_pos = np.maximum(0.02 * (1 + 0.6 * rng.standard_normal((37, 53))), 0.01)
    want_neg = np.maximum(0.03 * (1 + 0.6 * rng.standard_normal((37, 53))), 0.01)
    assert a.c_pos_map.dtype == torch.float64 and np.array_equal(a.c_pos_map.numpy(), want_pos)
    assert np.array_equal(a.c_neg_map.numpy(), want_neg) and torch.equal(a.c_pos_map, b.c_pos_map)
    assert not torch.equal(a.c_pos_map, other.c_pos_map)
    assert float(a.c_pos_map.min()) == 0.01 and (a.c_pos_map == 0.01).float().mean() > 0.05        # the floor is reached
    img = np.zeros((37, 53), dtype=np.uint8)
    with pytest.raises(EnslamError):
        a.step_images(img, img)                                                                 # before reset
    a.reset(img)
    with pytest.raises(EnslamError):
        a.step_images(img[:5], img[:5])
    with pytest.raises(EnslamError):
        a.step_images(img.astype(np.float32), img.astype(np.float32))
    with pytest.raises(EnslamError):
        a.step_scene(C.demo_room(), np.eye(4), np.eye(4), CAM)                                  # another camera size
    for bad in (dict(c_pos=0.0), dict(c_neg=-1.0), dict(eps=0.0), dict(substeps=0), dict(sigma_c=-0.1)):
        with pytest.raises(EnslamError):
            EventSimulator(4, 4, device='cpu', **bad)


def test_interpolate_poses():
    from evennicer_slam_amd.event_sim import interpolate_poses
    from evennicer_slam_amd.synthetic import look_at
    a = look_at([0.1, -0.2, 0.0], [1.0, 0.3, 0.1]).numpy()
    b = look_at([0.3, -0.1, 0.05], [0.8, 0.9, -0.1]).numpy()
    for K in (1, 4, 8):
        P = interpolate_poses(a, torch.from_numpy(b), K)
        assert P.shape == (K, 4, 4) and P.dtype == np.float64
        assert np.array_equal(P[-1], b)                                                          # the end point, exactly
        assert np.array_equal(P[:, 3], np.tile([0.0, 0.0, 0.0, 1.0], (K, 1)))
        R = P[:, :3, :3]
        assert np.abs(R @ R.transpose(0, 2, 1) - np.eye(3)).max() <= 1e-14
        assert np.abs(np.linalg.det(R) - 1).max() <= 1e-14
        for s in range(1, K):
            assert np.array_equal(P[s - 1, :3, 3], a[:3, 3] + (s / K) * (b[:3, 3] - a[:3, 3]))
    # the rotation turns at a constant rate about one axis: equal angles between neighbours
    P = interpolate_poses(a, b, 4)
    rots = [a[:3, :3]] + [P[s, :3, :3] for s in range(4)]
    ang = [math.acos(min((np.trace(r0.T @ r1) - 1) / 2, 1.0)) for r0, r1 in zip(rots[:-1], rots[1:])]
    assert max(ang) - min(ang) < 1e-9 and ang[0] > 1e-2
    # identical poses: every sub-pose is that pose; the identity pair gives the identity
    assert np.array_equal(interpolate_poses(np.eye(4), np.eye(4), 5), np.tile(np.eye(4), (5, 1, 1)))
    same = interpolate_poses(a, a, 3)
    assert np.array_equal(same[-1], a) and np.abs(same - a).max() <= 1e-15


# ---- sequences and the tool -------------------------------------------------------------------------------------------------
def test_write_demo_sequence_with_simulated_events(tmp_path):
    from evennicer_slam_amd import datasets as D
    from evennicer_slam_amd.event_sim import EventSimulator
    from evennicer_slam_amd.synthetic import demo_config, write_demo_sequence
    n = 4
    sim = EventSimulator(CAM['H'], CAM['W'], c_pos=0.04, c_neg=0.04, device='cpu')
    (inp, evf), poses = write_demo_sequence(str(tmp_path / 'sim'), n, CAM, step=0.02, yaw_deg=0.4, events='simulate', sim=sim)
    # the same intervals simulated directly
    twin = EventSimulator(CAM['H'], CAM['W'], c_pos=0.04, c_neg=0.04, device='cpu')
    room = C.demo_room()
    twin.reset((room, poses[0].double(), CAM))
    want = [twin.step_scene(room, poses[i - 1].double(), poses[i].double(), CAM) for i in range(1, n)]
    assert all(bool(w.any()) for w in want)
    assert torch.equal(twin.state, sim.state)
    cfg = demo_config(inp, evf, CAM, device='cpu')
    assert cfg['event']['activate_events'] is False                                              # the default is untouched
    ds = D.get_dataset(cfg, types.SimpleNamespace(input_folder=None, event_folder=None), 1, device='cpu')
    assert len(ds) == n and not bool(ds[0][3].any())
    for i in range(1, n):
        item = ds[i]
        assert item[3].dtype == torch.uint8 and torch.equal(item[3], want[i - 1])
        assert torch.equal(item[4], (want[i - 1] != 0).any(dim=-1) * 1)
    # the default call: all-zero event images, byte for byte what it wrote before, and the same frames
    (inp0, evf0), _ = write_demo_sequence(str(tmp_path / 'zero'), n, CAM, step=0.02, yaw_deg=0.4)
    from PIL import Image
    blank = tmp_path / 'blank.png'
    Image.fromarray(np.zeros((CAM['H'], CAM['W'], 3), dtype=np.uint8), 'RGB').save(str(blank))
    zeros = sorted(glob.glob(os.path.join(evf0, '*.png')))
    assert len(zeros) == n - 1
    assert all(open(p, 'rb').read() == open(str(blank), 'rb').read() for p in zeros)
    for a, b in zip(sorted(glob.glob(os.path.join(inp, 'results', '*'))), sorted(glob.glob(os.path.join(inp0, 'results', '*')))):
        assert os.path.basename(a) == os.path.basename(b) and open(a, 'rb').read() == open(b, 'rb').read()
    assert open(os.path.join(inp, 'traj.txt')).read() == open(os.path.join(inp0, 'traj.txt')).read()
    with pytest.raises(ValueError):
        write_demo_sequence(str(tmp_path / 'bad'), 2, CAM, events='zeros')


def test_simulate_events_tool_demo_on_the_cpu(tmp_path, capsys):
    tool = _tool("simulate_events")
    capsys.readouterr()
    out = tool.main(['--demo', '4', '--out', str(tmp_path / 'demo'), '--device', 'cpu', '--c-pos', '0.05', '--c-neg', '0.05'])
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert line == json.loads(json.dumps(out))
    assert line['frames'] == 4 and line['event_images'] == 3 and line['layout'] == 'replica_event' and line['device'] == 'cpu'
    assert 0 < line['event_pixel_share'] < 0.5 and line['mean_neg'] > 0 and line['mean_pos'] > 0
    assert line['saturated_share'] == 0 and line['seconds_per_frame'] > 0
    assert len(glob.glob(os.path.join(line['event_folder'], 'event_frame*.png'))) == 3
    assert len(glob.glob(os.path.join(line['input_folder'], 'results', 'frame*.jpg'))) == 4


@pytest.mark.parametrize("layout", ["rpg_event", "replica_event"])
def test_simulate_events_tool_on_a_recorded_sequence(tmp_path, capsys, layout):
    """A YAML chain naming a sequence without events: the tool reads the raw decoded colour images (grey for rpg) and writes
    the folder the *_event reader then accepts; read back, the events equal a direct simulation of those images."""
    import yaml
    from evennicer_slam_amd import datasets as D
    from evennicer_slam_amd.event_sim import EventSimulator
    H, W, n = 20, 31, 4
    rng = np.random.default_rng(3)
    base = rng.integers(30, 226, (H, W, 3))
    greys = [np.clip(base[..., 0] + 25 * k * ((np.arange(W) % 3) - 1), 0, 255).astype(np.uint8) for k in range(n)]
    depth = np.full((H, W), 1.5, dtype=np.float32)
    poses = [np.eye(4) for _ in range(n)]
    if layout == 'rpg_event':
        inp, _ = D.write_rpg_event_sequence(str(tmp_path / 'data'), [(g, depth) for g in greys], poses, 1000.0, [])
        name = 'rpg_event'
    else:
        colors = [np.stack([g, g[::-1], g[:, ::-1]], axis=-1) / 255.0 for g in greys]
        inp, _ = D.write_replica_event_sequence(str(tmp_path / 'data'), [(c, depth) for c in colors], poses, 1000.0, None)
        name = 'replica'
    evf = str(tmp_path / 'events')
    cfg = {'dataset': name, 'scale': 1, 'data': {'input_folder': inp, 'event_folder': evf},
           'cam': dict(H=H, W=W, fx=20.0, fy=20.0, cx=15.0, cy=9.5, png_depth_scale=1000.0, crop_edge=0)}
    root, child = str(tmp_path / 'root.yaml'), str(tmp_path / 'seq.yaml')
    with open(root, 'w') as f:
        yaml.safe_dump(cfg, f)
    with open(child, 'w') as f:
        yaml.safe_dump({'inherit_from': root}, f)
    tool = _tool("simulate_events")
    capsys.readouterr()
    tool.main([child, '--out', evf, '--device', 'cpu', '--c-pos', '0.05', '--c-neg', '0.07', '--substeps', '3', '--layout', layout])
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert line['frames'] == n and line['event_images'] == n - 1 and line['layout'] == layout and line['event_pixel_share'] > 0.1
    ds = D.get_dataset(dict(cfg, dataset=layout), types.SimpleNamespace(input_folder=None, event_folder=None), 1, device='cpu')
    raw = [tool.raw_color(p, layout == 'rpg_event') for p in ds.color_paths]
    if layout == 'rpg_event':
        assert all(np.array_equal(r, g) for r, g in zip(raw, greys))                             # png: lossless
    sim = EventSimulator(H, W, c_pos=0.05, c_neg=0.07, substeps=3, device='cpu').reset(raw[0])
    for i in range(1, n):
        want = sim.step_images(raw[i - 1], raw[i])
        assert bool((want[..., 0] > 0).any()) and bool((want[..., 1] > 0).any())
        assert torch.equal(ds[i][3], want)


def test_abi_declares_the_simulator():
    import evennicer_slam_amd as E
    header = open(os.path.join(ROOT, "include", "enslam_hip.h")).read()
    handle = ctypes.CDLL(E.LIB_PATH)
    for name in EXPORTS:
        assert name in E._lib.EXPORTS and name + "(" in header and hasattr(handle, name)
    assert "enslam_event_sim_plan" in header and "event_sim.o" in open(os.path.join(os.path.dirname(E.LIB_PATH), "csrc", "Makefile")).read()
    lib = E._lib.lib()
    assert lib.enslam_event_sim_plan_bytes() == ctypes.sizeof(E._lib.EventSimPlan)
    assert lib.enslam_event_sim_max_substeps() == 64
    assert len(E._lib._SIGS["enslam_event_sim_images"][1]) == 11 and len(E._lib._SIGS["enslam_event_sim_boxroom"][1]) == 9
    from evennicer_slam_amd import functional as EF
    from evennicer_slam_amd._lib import EnslamError
    with pytest.raises(EnslamError):                                                            # a CPU tensor: no quiet fall-back
        EF.event_sim_images(torch.zeros(4, 4, dtype=torch.uint8), torch.zeros(4, 4, dtype=torch.uint8),
                            torch.zeros(4, 4, dtype=torch.float64), lut=torch.zeros(256, dtype=torch.float64))
    with pytest.raises(EnslamError):
        EF.event_sim_boxroom(C.demo_room(), np.eye(4)[None], dict(CAM, H=4, W=4), torch.zeros(4, 4, dtype=torch.float64))
