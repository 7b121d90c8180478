"""-m gpu: csrc/frame_prep.hip (functional.frame_prepare, datasets `prepare='device'`) against the host route of datasets.py on
the same raw arrays (seeded random uint8 / uint16).  Outputs are 37x53 -- no multiple of a wave or of the kernel's 64x4 tile
in either axis, more than one workgroup -- or smaller.

Bounds: the undistortion, the depth and the masks are bit-equal; a uint8 resize is equal except, at most, where the host's
float64 value before rounding lies within 1e-9 of a half-integer (none at these shapes on the CPU this was written on);
float64 colour through every stage within 1e-14 (values <= 1, at most three chained resamplings of about 8 rounded
operations each: a few tens of 2^-53; measured 2.2e-16 at these shapes); float32 events through crop_size within 2.4e-4 (16
float32 ulp at 255)."""
import ctypes
import importlib.util
import json
import os
import types

import numpy as np
import pytest
import torch

from tests import frame_prep_cases as C
from tests.frame_prep_cases import HO, WO

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _device(*args, **kw):
    from evennicer_slam_amd import functional as EF
    return tuple(t.cpu().numpy() for t in EF.frame_prepare(*args, device=DEV, **kw))


def _both(*args, **kw):
    return C.host_route(*args, **kw), _device(*args, **kw)


@pytest.mark.parametrize("lens", ["tum", "rpg"])
@pytest.mark.parametrize("channels", [1, 3])
def test_undistort_is_bit_equal(lens, channels):
    from evennicer_slam_amd import datasets as D
    K, dist = (C.scaled_K(C.TUM_K, WO / 640), C.TUM_DIST) if lens == "tum" else (C.scaled_K(C.RPG_K, WO / 346), C.RPG_DIST)
    color = C.raw_color((HO, WO) if channels == 1 else (HO, WO, 3), 1)
    event, depth = C.raw_event((HO, WO, 3), 2), C.raw_depth((HO, WO), 3)
    host, dev = _both(color, depth, event, K=K, distortion=dist, png_depth_scale=1000.0, event_order='rpg')
    assert dev[0].dtype == np.float64 and dev[0].shape == (HO, WO, 3) and dev[2].dtype == np.uint8 and dev[3].dtype == np.int64
    want = D.undistort(color if channels == 3 else np.repeat(color[:, :, None], 3, axis=2), K, dist)
    assert np.array_equal(host[0], want / 255.)
    assert np.array_equal(dev[0], want / 255.)
    assert np.array_equal(dev[2], D.undistort(event, K, dist)[:, :, [1, 0]])
    assert np.array_equal(dev[3], host[3]) and np.array_equal(dev[1], host[1])
    assert (want != (color if channels == 3 else color[:, :, None])).mean() > 0.5            # the lens model did something
    # destination pixels all four of whose taps lie outside the image: the zero border
    u, v = np.meshgrid(np.arange(WO, dtype=np.float64), np.arange(HO, dtype=np.float64))
    xd, yd = D.distort_points((u - K[2]) / K[0], (v - K[3]) / K[1], dist)
    x0, y0 = np.floor(K[0] * xd + K[2]), np.floor(K[1] * yd + K[3])
    outside = (x0 < -1) | (x0 > WO - 1) | (y0 < -1) | (y0 > HO - 1)
    print(f"{lens} C={channels}: {int(outside.sum())} of {outside.size} pixels read only border taps")
    if lens == "tum":
        assert outside.sum() >= 1
    assert not want[outside].any() and not dev[0][outside].any()


@pytest.mark.parametrize("h0,w0", [(45, 61), (29, 41), (74, 106)])
def test_uint8_resize(h0, w0):
    """Events of another size than the depth: the cv2-style resize on uint8, rounded half-to-even."""
    event, color, depth = C.raw_event((h0, w0, 3), 4), C.raw_color((h0, w0, 3), 5), C.raw_depth((HO, WO), 6)
    if (h0, w0) == (74, 106):
        event[::2] = np.minimum(event[::2], 254) | 1               # even rows odd: more 2x2 block sums of the form 4 k + 2
    host, dev = _both(color, depth, event, png_depth_scale=1000.0)
    assert dev[2].dtype == np.uint8 and dev[2].shape == (HO, WO, 2)
    exact = C.resize_before_rounding(event, (HO, WO))[:, :, [1, 2]]
    frac = np.abs(exact - np.floor(exact) - 0.5)
    if (h0, w0) == (74, 106):
        # every weight is 1/4: the values are exact dyadics, and a good part of them exact halves -- strict equality, which
        # round-half-away-from-zero would miss
        halves = frac == 0
        print(f"{h0}x{w0}: {int(halves.sum())} of {halves.size} values are exact halves")
        assert halves.sum() > 500
        assert np.array_equal(exact * 4, np.round(exact * 4))
        assert np.array_equal(dev[2], host[2])
        away = np.floor(exact + 0.5).astype(np.uint8)
        assert (away != host[2]).sum() > 100
    else:
        near = frac < 1e-9
        diff = dev[2].astype(np.int64) - host[2].astype(np.int64)
        print(f"{h0}x{w0}: {int(near.sum())} of {near.size} values within 1e-9 of a half, {int((diff != 0).sum())} differ")
        assert near.sum() <= 1e-3 * near.size
        assert np.abs(diff).max() <= 1 and not (diff != 0)[~near].any()
    assert np.array_equal(dev[3], host[3])
    assert np.abs(dev[0] - host[0]).max() <= 1e-14                 # the colour took the float64 resize


def test_colour_float64_through_every_stage():
    """undistort -> / 255 -> resize from another size -> crop_size 37x53 -> 24x40 -> crop_edge 3"""
    color, depth = C.raw_color((45, 61, 3), 7), C.raw_depth((HO, WO), 8)
    kw = dict(K=C.scaled_K(C.TUM_K, 61 / 640), distortion=C.TUM_DIST, png_depth_scale=5000.0, crop_size=[24, 40], crop_edge=3)
    host, dev = _both(color, depth, **kw)
    assert len(dev) == 2 and dev[0].shape == (18, 34, 3) and dev[1].shape == (18, 34)
    err = np.abs(dev[0] - host[0]).max()
    print(f"colour through every stage: max |device - host| = {err:.3e}")
    assert err <= 1e-14
    assert np.array_equal(dev[1], host[1])
    # the same chain without the lens model, and from a smaller colour image (upscaling)
    for shape in ((45, 61, 3), (29, 41, 3)):
        color = C.raw_color(shape, 9)
        host, dev = _both(color, depth, png_depth_scale=5000.0, crop_size=[24, 40], crop_edge=3)
        err = np.abs(dev[0] - host[0]).max()
        print(f"colour {shape[0]}x{shape[1]} -> resize -> crop_size -> crop_edge: max |device - host| = {err:.3e}")
        assert err <= 1e-14


@pytest.mark.parametrize("order", ["replica", "rpg"])
def test_events_float32_through_crop_size_and_masks(order):
    color, depth, event = C.raw_color((HO, WO, 3), 10), C.raw_depth((HO, WO), 11), C.raw_event((45, 61, 3), 12)
    kw = dict(K=C.scaled_K(C.TUM_K, WO / 640), distortion=C.TUM_DIST, png_depth_scale=5000.0, crop_size=[24, 40], crop_edge=3,
              event_order=order, undistort_events=(order == 'rpg'))
    host, dev = _both(color, depth, event, **kw)
    assert dev[2].dtype == np.float32 and host[2].dtype == np.float32 and dev[2].shape == (18, 34, 2)
    err = np.abs(dev[2].astype(np.float64) - host[2].astype(np.float64)).max()
    print(f"float32 events through crop_size ({order}): max |device - host| = {err:.3e}")
    assert err <= 2.4e-4
    assert np.array_equal(dev[3], host[3]) and 0 < host[3].mean() < 1
    assert np.abs(dev[0] - host[0]).max() <= 1e-14 and np.array_equal(dev[1], host[1])
    # the two orders hand out different channels of the same png
    other = _device(color, depth, event, **dict(kw, event_order='rpg' if order == 'replica' else 'replica'))
    assert np.array_equal(other[2][..., 0], dev[2][..., 0]) and not np.array_equal(other[2][..., 1], dev[2][..., 1])


@pytest.mark.parametrize("order", ["replica", "rpg"])
def test_event_channel_orders_and_frame_zero(order):
    color, depth, event = C.raw_color((HO, WO, 3), 13), C.raw_depth((HO, WO), 14), C.raw_event((HO, WO, 3), 15)
    host, dev = _both(color, depth, event, png_depth_scale=6553.5, event_order=order)
    assert np.array_equal(dev[2], event[:, :, C.EVENT_CHANNELS[order]]) and np.array_equal(dev[2], host[2])
    assert np.array_equal(dev[3], host[3]) and np.array_equal(dev[0], color / 255.) and np.array_equal(dev[1], host[1])
    # frame 0: no event image, zero events and mask of the right types -- uint8, or float32 behind crop_size
    for crop in (None, [24, 40]):
        host, dev = _both(color, depth, None, events=True, png_depth_scale=6553.5, event_order=order, crop_size=crop, crop_edge=2)
        assert len(dev) == 4 and dev[2].dtype == host[2].dtype == (np.uint8 if crop is None else np.float32)
        assert dev[2].shape == host[2].shape and not dev[2].any() and dev[3].dtype == np.int64 and not dev[3].any()
        assert np.array_equal(dev[1], host[1])


@pytest.mark.parametrize("dtype", [np.uint16, np.int32])
def test_depth_is_bit_equal(dtype):
    color = C.raw_color((HO, WO, 3), 16)
    depth = C.raw_depth((HO, WO), 17, dtype)
    if dtype is np.int32:
        depth[1, :8] = [16777217, 33554435, 2147483647, 70000, 16777219, 100000, 65536, 1]      # rounded by float32(raw)
    for pds, scale in ((6553.5, 1.0), (5000.0, 0.3), (1000.0, 1.0)):
        host, dev = _both(color, depth, png_depth_scale=pds, scale=scale)
        assert dev[1].dtype == np.float32 and np.array_equal(dev[1], host[1])
        assert dev[1][0, 0] == 0 and dev[1][0, 1] == np.float32(np.float32(65535) / np.float32(pds)) * np.float32(scale)
        # torch's `nearest` at a non-integer ratio, at twice the size (its shift shortcut) and the crop_edge cut
        for crop, edge in (([24, 40], 0), ([24, 40], 3), ([74, 106], 1), ([50, 53], 0)):
            host, dev = _both(color, depth, png_depth_scale=pds, scale=scale, crop_size=crop, crop_edge=edge)
            assert dev[1].shape == (crop[0] - 2 * edge, crop[1] - 2 * edge) and np.array_equal(dev[1], host[1])
            assert np.abs(dev[0] - host[0]).max() <= 1e-14


def test_raw_tensors_on_the_device_and_argument_checks():
    from evennicer_slam_amd import functional as EF
    from evennicer_slam_amd._lib import EnslamError
    color, depth = C.raw_color((HO, WO, 3), 18), C.raw_depth((HO, WO), 19)
    want = C.host_route(color, depth, png_depth_scale=1000.0)
    got = EF.frame_prepare(torch.from_numpy(color).to(DEV), torch.from_numpy(depth.view(np.int16)).to(DEV), png_depth_scale=1000.0)
    assert got[0].device.type == 'cuda' and np.array_equal(got[0].cpu().numpy(), want[0]) and np.array_equal(got[1].cpu().numpy(), want[1])
    with pytest.raises(EnslamError):
        EF.frame_prepare(torch.from_numpy(color), depth)                                   # a CPU tensor
    with pytest.raises(EnslamError):
        EF.frame_prepare(color, depth, device='cpu')
    with pytest.raises(EnslamError):
        EF.frame_prepare(color.astype(np.float32), depth)
    with pytest.raises(EnslamError):
        EF.frame_prepare(color, depth.astype(np.float32))
    with pytest.raises(EnslamError):
        EF.frame_prepare(color[:, :, :2], depth)                                           # C = 2
    with pytest.raises(EnslamError):
        EF.frame_prepare(color, depth, distortion=C.TUM_DIST)                              # a lens model without intrinsics
    with pytest.raises(EnslamError):
        EF.frame_prepare(color, depth, crop_edge=19)                                       # nothing left of 37 rows


def test_abi_errors_return_without_launching():
    from evennicer_slam_amd import _lib as L
    from evennicer_slam_amd import functional as EF
    lib = L.lib()
    assert lib.enslam_frame_plan_bytes() == ctypes.sizeof(L.FramePlan)
    c = torch.zeros((HO, WO, 3), dtype=torch.uint8, device=DEV)
    d = torch.zeros((HO, WO), dtype=torch.int16, device=DEV)
    e = torch.zeros((HO, WO, 3), dtype=torch.uint8, device=DEV)
    co = torch.full((HO, WO, 3), -1.0, dtype=torch.float64, device=DEV)
    do = torch.full((HO, WO), -1.0, dtype=torch.float32, device=DEV)
    eo = torch.full((HO, WO, 2), 7, dtype=torch.uint8, device=DEV)
    mo = torch.full((HO, WO), -1, dtype=torch.int64, device=DEV)

    def call(plan, *ptrs):
        return lib.enslam_frame_prepare(ctypes.byref(plan) if plan is not None else None,
                                        *[t.data_ptr() if t is not None else None for t in ptrs], None)

    def plan(**over):
        p = EF.frame_plan((HO, WO, 3), (HO, WO), False, (HO, WO, 3))
        for k, v in over.items():
            setattr(p, k, v)
        return p

    bad = [call(None, c, d, e, co, do, eo, mo), call(plan(), None, d, e, co, do, eo, mo), call(plan(), c, None, e, co, do, eo, mo),
           call(plan(), c, d, e, None, do, eo, mo), call(plan(), c, d, e, co, None, eo, mo), call(plan(), c, d, e, co, do, eo, None),
           call(plan(), c, d, e, co, do, None, mo), call(plan(channels=2), c, d, e, co, do, eo, mo),
           call(plan(channels=4), c, d, e, co, do, eo, mo), call(plan(crop_edge=19), c, d, e, co, do, eo, mo),
           call(plan(crop_edge=-1), c, d, e, co, do, eo, mo), call(plan(crop_h=24, crop_w=40, crop_edge=12), c, d, e, co, do, eo, mo),
           call(plan(crop_h=24), c, d, e, co, do, eo, mo), call(plan(ev_pos=3), c, d, e, co, do, eo, mo),
           call(plan(H=0), c, d, e, co, do, eo, mo), call(plan(png_depth_scale=0.0), c, d, e, co, do, eo, mo),
           call(plan(has_dist=1), c, d, e, co, do, eo, mo)]                                # fx = fy = 0
    assert bad == [-1] * len(bad)
    torch.cuda.synchronize()
    assert bool((co == -1).all()) and bool((do == -1).all()) and bool((eo == 7).all()) and bool((mo == -1).all())      # nothing ran
    assert call(plan(crop_edge=18), c, d, e, co, do, eo, mo) == 0                          # one row left: valid
    torch.cuda.synchronize()
    assert bool((co[0, :17] == 0).all()) and bool((mo[0, :17] == 0).all())


def _items_close(host, dev):
    assert len(host) == len(dev) and host[0] == dev[0]
    h, d = [t.cpu() for t in host[1:]], [t.cpu() for t in dev[1:]]
    assert all(a.dtype == b.dtype and a.shape == b.shape for a, b in zip(h, d))
    assert all(t.device.type == 'cuda' for t in dev[1:])
    assert float((h[0] - d[0]).abs().max()) <= 1e-14 and torch.equal(h[1], d[1]) and torch.equal(h[-1], d[-1])
    if len(h) == 5:
        assert float((h[2].double() - d[2].double()).abs().max()) <= (2.4e-4 if h[2].dtype == torch.float32 else 0)
        assert torch.equal(h[3], d[3])


def _room_frames(n, cam):
    from evennicer_slam_amd.scene import scene_bound
    from evennicer_slam_amd.synthetic import BoxRoom, trajectory
    bound = scene_bound([[-1.0, 1.1], [-0.9, 0.8], [-0.7, 0.6]], 1.0, 0.32)
    room = BoxRoom.for_bound(bound, margin=0.12, seed=1)
    poses = trajectory(room, n, step=0.012, yaw_deg=0.5)
    return [tuple(t.numpy() for t in room.render(p.double(), cam)) for p in poses], [p.numpy() for p in poses]


def test_rpg_event_reader_device_equals_host(tmp_path):
    from evennicer_slam_amd import datasets as D
    cam = dict(H=HO, W=WO, fx=C.RPG_K[0] * WO / 346, fy=C.RPG_K[1] * WO / 346, cx=C.RPG_K[2] * WO / 346, cy=C.RPG_K[3] * WO / 346)
    rng = np.random.default_rng(20)
    frames = [(C.raw_color((HO, WO), 21 + i), rng.integers(300, 3000, (HO, WO)) / 1000.0) for i in range(3)]
    events = [C.raw_event((HO, WO, 3), 30 + i)[:, :, :2] for i in range(2)]
    poses = [np.eye(4) for _ in range(3)]
    inp, evf = D.write_rpg_event_sequence(str(tmp_path), frames, poses, 1000.0, events)
    cfg = {'dataset': 'rpg_event', 'data': {'input_folder': inp, 'event_folder': evf, 'prepare': 'device'},
           'cam': dict(cam, png_depth_scale=1000.0, crop_edge=2, distortion=C.RPG_DIST)}
    ds = D.get_dataset(cfg, types.SimpleNamespace(input_folder=None, event_folder=None), 0.5, device=DEV)
    assert ds.prepare == 'device'
    dev = [ds[i] for i in range(3)]
    ds.prepare = 'host'
    for i in range(3):
        _items_close(ds[i], dev[i])
    assert not bool(dev[0][3].any()) and bool(dev[1][3].any()) and dev[1][3].dtype == torch.uint8
    assert tuple(dev[1][1].shape) == (HO - 4, WO - 4, 3)


def test_tum_reader_device_equals_host_and_run_slam(tmp_path, capsys):
    """A TUM-layout sequence of the analytic room (lens model, crop_size, crop_edge): items of prepare='device' equal those
    of 'host'; tools/run_slam.py runs 3 frames of it from a YAML chain and leaves finite poses and a checkpoint."""
    import yaml
    from evennicer_slam_amd import datasets as D
    from evennicer_slam_amd.synthetic import demo_config
    cam = dict(H=48, W=64, fx=51.73, fy=51.65, cx=31.86, cy=25.53)
    frames, poses = _room_frames(3, cam)
    inp = D.write_tum_sequence(str(tmp_path / 'data'), frames, poses, 5000.0)
    cfg = demo_config(inp, None, cam, device=DEV, env={'ITERS_FIRST': 20, 'MAP_ITERS': 5, 'TRACK_ITERS': 3, 'EVERY': 1,
                                                       'MAP_PIXELS': 200, 'TRACK_PIXELS': 200})
    cfg['dataset'] = 'tumrgbd'
    cfg['data'] = {'dim': 3, 'input_folder': inp, 'output': str(tmp_path / 'out')}
    cfg['cam'] = dict(cam, png_depth_scale=5000.0, crop_size=[36, 48], crop_edge=2, distortion=C.TUM_DIST)
    cfg['mapping']['bound'] = [[-3.0, 3.0], [-3.0, 3.0], [-3.0, 3.0]]          # poses are relative to the first frame
    ds = D.get_dataset(cfg, types.SimpleNamespace(input_folder=None), 1, device=DEV)
    assert len(ds) == 3 and ds.prepare == 'host'
    host = [ds[i] for i in range(3)]
    ds.prepare = 'device'
    for i in range(3):
        _items_close(host[i], ds[i])
    assert tuple(host[0][1].shape) == (32, 44, 3)

    base, child = str(tmp_path / 'base.yaml'), str(tmp_path / 'seq.yaml')
    with open(base, 'w') as f:
        yaml.safe_dump(cfg, f)
    with open(child, 'w') as f:
        yaml.safe_dump({'inherit_from': base, 'tracking': {'iters': 2}}, f)
    spec = importlib.util.spec_from_file_location("run_slam_tool", os.path.join(ROOT, "tools", "run_slam.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    assert tool.slam_camera(cfg)['cam']['H'] == 36 and abs(tool.slam_camera(cfg)['cam']['fx'] - 51.73 * 0.75) < 1e-12
    capsys.readouterr()
    res = tool.main([child, '--max-frames', '3', '--prepare', 'device'])
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert line['frames'] == 3 and line['prepare'] == 'device' and os.path.isfile(line['ckpt']) and np.isfinite(line['ate_rmse'])
    ckpt = torch.load(res['ckpt'], map_location='cpu', weights_only=False)
    assert ckpt['idx'] == 2 and bool(torch.isfinite(ckpt['estimate_c2w_list'][:3]).all())
    assert torch.equal(ckpt['estimate_c2w_list'][0], ckpt['gt_c2w_list'][0])
