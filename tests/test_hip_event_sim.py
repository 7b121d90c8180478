"""-m gpu: csrc/event_sim.hip (event_sim.EventSimulator on a HIP device, functional.event_sim_images / event_sim_boxroom)
against the float64 yardstick tests/event_sim_numpy.py on the cases of tests/event_sim_cases.py.

Image route: counts and L_ref bit-equal on every case with the state carried over three intervals -- grey through the
256-entry host table, RGB through the host-computed level images (host_log) so that no device log decides a count.  The
in-kernel log of the RGB path is compared separately: counts within 1, at most 0.1 % of the pixels differing.
Analytic route: counts equal on every pixel the margin rule does not leave out (tests/event_sim_cases.py: margin 1e-9, an
estimate; a pixel once left out stays out), L_ref within 1e-9, the frame outputs within 1e-12 (colour) and one float32 ulp
(depth) of the yardstick."""
import ctypes
import importlib.util
import os
import types

import numpy as np
import pytest
import torch

from tests import event_sim_cases as C
from tests import event_sim_numpy as Y
from tests.viz_cases import CAM

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _sim(c, H, W):
    from evennicer_slam_amd.event_sim import EventSimulator
    return EventSimulator(H, W, c_pos=c['c_pos'], c_neg=c['c_neg'], sigma_c=c.get('sigma_c', 0.0), substeps=c['K'], eps=C.EPS,
                          seed=c.get('seed', 0), device=DEV)


def _image_steps(name, sim):
    c = C.image_cases()[name]
    if c['sigma_c'] > 0:
        return C.image_reference(name, sim.c_pos_map.cpu().numpy(), sim.c_neg_map.cpu().numpy())
    return C.image_reference(name)


@pytest.mark.parametrize("name", sorted(C.image_cases()))
def test_image_route_is_bit_equal(name):
    c = C.image_cases()[name]
    sim = _sim(c, *c['shape'])
    steps = _image_steps(name, sim)
    host_log = c['channels'] == 3
    sim.reset(c['images'][0], host_log=host_log)
    assert sim.state.device.type == 'cuda' and sim.state.dtype == torch.float64
    assert np.array_equal(sim.state.cpu().numpy(), Y.level_of_image(c['images'][0], C.EPS))
    for k, ((ev, ref), prev, cur) in enumerate(zip(steps, c['images'][:-1], c['images'][1:])):
        got = sim.step_images(prev, cur, host_log=host_log)
        assert got.device.type == 'cuda' and got.dtype == torch.uint8 and tuple(got.shape) == c['shape'] + (2,)
        g = got.cpu().numpy()
        print(f"{name} interval {k}: {int((g != ev).sum())} counts differ, events - {int(ev[..., 0].sum())} + {int(ev[..., 1].sum())}")
        assert np.array_equal(g, ev)
        assert np.array_equal(sim.state.cpu().numpy(), ref)


@pytest.mark.parametrize("name", sorted(n for n, c in C.image_cases().items() if c['channels'] == 3))
def test_image_route_in_kernel_log(name):
    """RGB without the host's levels: luminance and log in the kernel.  Counts within 1 of the yardstick's, on at most 0.1 %
    of the pixels; the device tensors may be passed in directly."""
    c = C.image_cases()[name]
    sim = _sim(c, *c['shape'])
    steps = _image_steps(name, sim)
    imgs = [torch.from_numpy(im).to(DEV) for im in c['images']]
    sim.reset(imgs[0])
    first = np.abs(sim.state.cpu().numpy() - Y.level_of_image(c['images'][0], C.EPS)).max()
    print(f"{name}: first level against numpy's log {first:.2e}")
    assert first <= 1e-14
    for k, ((ev, ref), prev, cur) in enumerate(zip(steps, imgs[:-1], imgs[1:])):
        g = sim.step_images(prev, cur).cpu().numpy().astype(np.int64)
        diff = np.abs(g - ev.astype(np.int64))
        pixels = int((diff != 0).any(axis=-1).sum())
        print(f"{name} interval {k}: {pixels} of {diff.shape[0] * diff.shape[1]} pixels differ, by {int(diff.max())} at most")
        assert diff.max() <= 1
        assert pixels <= C.LOG_PATH_MAX_DIFF_SHARE * diff.shape[0] * diff.shape[1]


@pytest.mark.parametrize("name", sorted(C.ANALYTIC))
def test_analytic_route(name):
    c, ref, poses, room = C.ANALYTIC[name], C.analytic_reference(name), C.analytic_poses(name), C.demo_room()
    sim = _sim(dict(c_pos=c['c'], c_neg=c['c'], K=c['K']), CAM['H'], CAM['W'])
    sim.reset((room, poses[0], CAM))
    err = np.abs(sim.state.cpu().numpy() - ref['first']).max()
    print(f"{name}: first level against the yardstick {err:.2e}")
    assert err <= C.LREF_TOL
    for k, s in enumerate(ref['steps']):
        ev, col, dep = sim.step_scene(room, poses[k], poses[k + 1], CAM, want_frame=True)
        assert ev.dtype == torch.uint8 and col.dtype == torch.float64 and dep.dtype == torch.float32
        assert tuple(ev.shape) == (CAM['H'], CAM['W'], 2) and tuple(col.shape) == (CAM['H'], CAM['W'], 3)
        ev, col, dep = ev.cpu().numpy(), col.cpu().numpy(), dep.cpu().numpy()
        keep = ~s['left_out']
        wrong = int((ev != s['events']).any(axis=-1)[keep].sum())
        e_ref = float(np.abs(sim.state.cpu().numpy() - s['ref'])[keep].max())
        e_col = float(np.abs(col - s['color']).max())
        ulp = np.spacing(np.abs(s['depth']))
        e_dep = float((np.abs(dep.astype(np.float64) - s['depth'].astype(np.float64)) / ulp).max())
        print(f"{name} interval {k}: {wrong} pixels with other counts ({int((~keep).sum())} left out), L_ref {e_ref:.2e}, "
              f"colour {e_col:.2e}, depth {e_dep:.2f} ulp")
        assert wrong == 0
        assert e_ref <= C.LREF_TOL and e_col <= C.COLOR_TOL and e_dep <= 1.0


def test_two_runs_are_bit_identical_and_frames_do_not_change_events():
    name = "silhouette_K4"
    c, poses, room = C.ANALYTIC[name], C.analytic_poses(name), C.demo_room()
    runs = []
    for want_frame in (False, True, False):
        sim = _sim(dict(c_pos=c['c'], c_neg=c['c'], K=c['K']), CAM['H'], CAM['W'])
        sim.reset((room, poses[0], CAM))
        evs = []
        for a, b in zip(poses[:-1], poses[1:]):
            out = sim.step_scene(room, a, b, CAM, want_frame=want_frame)
            evs.append(out[0] if want_frame else out)
        runs.append((evs, sim.state.clone()))
    for evs, state in runs[1:]:
        assert all(torch.equal(a, b) for a, b in zip(evs, runs[0][0])) and torch.equal(state, runs[0][1])
    assert all(bool(e.any()) for e in runs[0][0])
    # the image route as well
    ic = C.image_cases()["37x53_rgb_K5_maps"]
    outs = []
    for _ in range(2):
        sim = _sim(ic, *ic['shape']).reset(ic['images'][0])
        outs.append(([sim.step_images(a, b) for a, b in zip(ic['images'][:-1], ic['images'][1:])], sim.state.clone()))
    assert all(torch.equal(a, b) for a, b in zip(outs[0][0], outs[1][0])) and torch.equal(outs[0][1], outs[1][1])


def test_argument_checks():
    from evennicer_slam_amd import functional as EF
    from evennicer_slam_amd._lib import EnslamError
    from evennicer_slam_amd.event_sim import EventSimulator
    H, W = 4, 5
    img = torch.zeros((H, W), dtype=torch.uint8, device=DEV)
    state = torch.full((H, W), float(Y.table(C.EPS)[0]), dtype=torch.float64, device=DEV)      # the level of a black image
    lut = torch.from_numpy(Y.table(C.EPS)).to(DEV)
    assert not bool(EF.event_sim_images(img, img, state, lut=lut).any())
    bad = [dict(prev=img.cpu()), dict(prev=img.float()), dict(state=state.float()), dict(state=state.cpu()), dict(lut=None),
           dict(lut=lut[:255]), dict(lut=lut.float()), dict(substeps=0), dict(substeps=65), dict(eps=0.0), dict(c_pos=0.0),
           dict(c_neg=float('nan')), dict(c_pos_map=state.float()), dict(c_neg_map=state[:3]), dict(state=state.t()),
           dict(prev=torch.zeros((H, W, 2), dtype=torch.uint8, device=DEV), cur=torch.zeros((H, W, 2), dtype=torch.uint8, device=DEV)),
           dict(levels=(state,)), dict(levels=(state, state.float()))]
    for kw in bad:
        args = dict(prev=img, cur=img, state=state, lut=lut)
        args.update(kw)
        with pytest.raises(EnslamError):
            EF.event_sim_images(**args)
    cam = dict(CAM, H=H, W=W)
    room, pose = C.demo_room(), np.eye(4)[None]
    assert EF.event_sim_boxroom(room, pose, cam, state, init=True) is None
    for kw in (dict(poses=pose.astype(np.float32)), dict(poses=pose[0]), dict(poses=np.tile(pose, (65, 1, 1))), dict(state=state.cpu()),
               dict(cam=dict(cam, fx=0.0)), dict(c_pos=-1.0), dict(cam=dict(cam, H=5))):
        args = dict(room=room, poses=pose, cam=cam, state=state)
        args.update(kw)
        with pytest.raises(EnslamError):
            EF.event_sim_boxroom(**args)
    with pytest.raises(EnslamError):
        EventSimulator(H, W, substeps=65, device=DEV)


def test_abi_errors_return_without_launching():
    from evennicer_slam_amd import _lib as L
    from evennicer_slam_amd import functional as EF
    lib = L.lib()
    assert lib.enslam_event_sim_plan_bytes() == ctypes.sizeof(L.EventSimPlan)
    kmax = lib.enslam_event_sim_max_substeps()
    H, W = 4, 5
    cam, room = dict(CAM, H=H, W=W), C.demo_room()
    img = torch.zeros((H, W, 3), dtype=torch.uint8, device=DEV)
    lut = torch.from_numpy(Y.table(C.EPS)).to(DEV)
    lv = torch.zeros((H, W), dtype=torch.float64, device=DEV)
    cmap = torch.full((H, W), 0.2, dtype=torch.float64, device=DEV)
    state = torch.full((H, W), -7.0, dtype=torch.float64, device=DEV)
    ev = torch.full((H * W * 2 + 2,), 9, dtype=torch.uint8, device=DEV)
    col = torch.full((H, W, 3), -1.0, dtype=torch.float64, device=DEV)
    dep = torch.full((H, W), -1.0, dtype=torch.float32, device=DEV)
    poses = torch.eye(4, dtype=torch.float64, device=DEV)[None, :3].contiguous()

    def plan(**over):
        p = EF.event_sim_plan(H, W, 2, C.EPS, 0.2, 0.2, channels=3, cam=cam, room=room)
        for k, v in over.items():
            setattr(p, k, v)
        return p

    def ptr(t):
        return t.data_ptr() if t is not None else None

    def images(p, prev=img, cur=img, table=lut, la=None, lb=None, cp=None, cn=None, st=state, e=ev, odd=False):
        return lib.enslam_event_sim_images(ctypes.byref(p) if p is not None else None, ptr(prev), ptr(cur), ptr(table), ptr(la), ptr(lb),
                                           ptr(cp), ptr(cn), ptr(st), (ptr(e) + 1 if odd else ptr(e)), None)

    def boxroom(p, ps=poses, cp=None, cn=None, st=state, e=ev, c=None, d=None):
        return lib.enslam_event_sim_boxroom(ctypes.byref(p) if p is not None else None, ptr(ps), ptr(cp), ptr(cn), ptr(st), ptr(e),
                                            ptr(c), ptr(d), None)

    inval = [images(None), images(plan(), st=None), images(plan(), e=None), images(plan(), prev=None), images(plan(), cur=None),
             images(plan(channels=1), table=None), images(plan(channels=2)), images(plan(channels=4)), images(plan(), la=lv),
             images(plan(), lb=lv), images(plan(H=0)), images(plan(W=-1)), images(plan(K=0)), images(plan(eps=0.0)),
             images(plan(eps=float('nan'))), images(plan(c_pos=0.0)), images(plan(c_neg=-0.2)), images(plan(c_pos=float('inf'))),
             images(plan(c_pos=0.0), cn=cmap), images(plan(), odd=True),
             boxroom(None), boxroom(plan(), ps=None), boxroom(plan(), st=None), boxroom(plan(), e=None), boxroom(plan(), c=col),
             boxroom(plan(), d=dep), boxroom(plan(K=0)), boxroom(plan(H=-3)), boxroom(plan(fx=0.0)), boxroom(plan(fy=float('nan'))),
             boxroom(plan(c_neg=0.0)), boxroom(plan(eps=-1.0))]
    assert inval == [-1] * len(inval)
    unsupported = [images(plan(K=kmax + 1)), boxroom(plan(K=kmax + 1)), images(plan(H=1 << 15, W=1 << 14))]
    assert unsupported == [-3] * len(unsupported)
    torch.cuda.synchronize()
    assert bool((state == -7.0).all()) and bool((ev == 9).all()) and bool((col == -1.0).all()) and bool((dep == -1.0).all())   # nothing ran
    # the valid neighbours of those calls: a threshold replaced by a map, levels in place of the images, init without events
    assert images(plan(c_pos=0.0), cp=cmap) == 0 and images(plan(), prev=None, cur=None, table=None, la=lv, lb=lv) == 0
    assert images(plan(init=1, c_pos=0.0), e=None) == 0 and boxroom(plan(K=1, init=1), e=None) == 0
    assert boxroom(plan(K=1), c=col, d=dep) == 0
    torch.cuda.synchronize()
    assert bool((ev[-2:] == 9).all()) and bool((ev[:-2] != 9).all()) and bool((col != -1.0).all()) and bool((dep > 0).all())


def test_simulated_demo_sequence_feeds_the_event_net_trainer(tmp_path):
    """Six 45 x 61 demo frames simulated on the device (the kernel renders the frames too), written, read back through
    Replica_event, and turned into the trainer's pairs: the ground-truth event images are no longer all zero."""
    from evennicer_slam_amd import datasets as D
    from evennicer_slam_amd.event_sim import EventSimulator
    from evennicer_slam_amd.synthetic import demo_config, write_demo_sequence
    n = 6
    sim = EventSimulator(CAM['H'], CAM['W'], c_pos=0.04, c_neg=0.04, device=DEV)
    (inp, evf), poses = write_demo_sequence(str(tmp_path / 'seq'), n, CAM, step=0.02, yaw_deg=0.4, events='simulate', sim=sim)
    host = EventSimulator(CAM['H'], CAM['W'], c_pos=0.04, c_neg=0.04, device='cpu')
    (inp_h, evf_h), _ = write_demo_sequence(str(tmp_path / 'host'), n, CAM, step=0.02, yaw_deg=0.4, events='simulate', sim=host)
    cfg = demo_config(inp, evf, CAM, device=DEV)
    ds = D.get_dataset(cfg, types.SimpleNamespace(input_folder=None, event_folder=None), 1, device=DEV)
    ds_h = D.get_dataset(demo_config(inp_h, evf_h, CAM, device='cpu'), types.SimpleNamespace(input_folder=None, event_folder=None), 1,
                         device='cpu')
    assert len(ds) == n
    differ = 0
    for i in range(1, n):
        ev = ds[i][3].cpu()
        assert bool(ev.any())
        differ += int((ev != ds_h[i][3]).any(dim=-1).sum())
        assert float((ds[i][1].cpu() - ds_h[i][1]).abs().max()) <= 1.5 / 255                   # the same frames, from the kernel
        assert float((ds[i][2].cpu() - ds_h[i][2]).abs().max()) <= 1.01 / 6553.5                # one level of the 16-bit depth png
    print(f"device against host sequence: {differ} of {(n - 1) * CAM['H'] * CAM['W']} event pixels differ")
    assert differ <= 1e-3 * (n - 1) * CAM['H'] * CAM['W']
    spec = importlib.util.spec_from_file_location("train_event_net_tool", os.path.join(ROOT, "tools", "train_event_net.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    pairs = tool.make_pairs(ds, cfg, 0.5)
    assert len(pairs) == n - 1
    for x, gt_event, gt_mask in pairs:
        assert tuple(x.shape) == (1, 6, 22, 30) and tuple(gt_event.shape) == (22, 30, 2)
    assert sum(float(p[1].abs().sum()) for p in pairs) > 0 and sum(int(p[2].sum()) for p in pairs) > 0
