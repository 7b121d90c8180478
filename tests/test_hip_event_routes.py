"""-m gpu: the event simulator's entries against each other, on both routes (images through the host table, the analytic room).
Device against device, relations that hold by construction -- every entry runs the same device functions on the same levels --
so all of them are bit-exact, through the kernel's own sin and log as well, and need no yardstick:

  1 the frame entry's count image and L_ref equal the stream emit entry's
  2 a count pass equals the per-pixel histogram of the (x, y) its emit pass writes: plain stream, and the noisy sensor with all
    three effects on
  3 the noisy sensor with all parameters zero equals the plain stream: image, L_ref and t, x, y, p as bytes
  4 the noisy sensor's one-launch form (stream=False) equals its two-launch form in image, L_ref and t_last

A 5 x 67 sensor: one full 64 x 4 tile, a partial tile to the right and a partial tile below.  K = 3, thresholds 0.02, two
consecutive intervals so that the carried state matters."""
import ctypes

import numpy as np
import pytest
import torch

from tests import event_noise_cases as NC
from tests import event_sim_cases as C
from tests import event_stream_cases as SC

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
H, W, K, THRESHOLD = 5, 67, 3, 0.02
CAM = dict(H=H, W=W, fx=47.0, fy=47.0, cx=33.2, cy=2.3)
SENSORS = dict(frame=None, plain=None, off=NC.SETTINGS['off'], noisy=NC.SETTINGS['all'], noisy_image=NC.SETTINGS['all'])


def _sims():
    from evennicer_slam_amd.event_sim import EventNoise, EventSimulator
    return {k: EventSimulator(H, W, c_pos=THRESHOLD, c_neg=THRESHOLD, substeps=K, eps=C.EPS, device=DEV,
                              noise=None if n is None else EventNoise(**n)) for k, n in SENSORS.items()}


def _ptr(a):
    return None if a is None else a.data_ptr()


def _counts(entry, plan, source, sim, tail=()):
    """one count entry alone, on the simulator's current states (which it only reads)"""
    from evennicer_slam_amd import _lib as L
    counts = torch.full((H, W), -1, dtype=torch.int64, device=DEV)
    before = sim.state.clone()
    rc = getattr(L.lib(), entry)(ctypes.byref(plan), *source, None, None, _ptr(sim.state), _ptr(counts), *tail, None)
    assert rc == 0 and torch.equal(sim.state, before)
    return counts.cpu().numpy()


def _noise_tail(sim, stamps, interval):
    from evennicer_slam_amd import functional as EF
    params = EF.event_noise_params("test", sim.noise.params(interval), K, stamps)
    return ctypes.byref(params), stamps[0], stamps[1], _ptr(sim.last_event_time)


def _histogram(stream):
    x, y = stream.numpy()[1:3]
    return np.bincount(y.astype(np.int64) * W + x, minlength=H * W).reshape(H, W)


def _same_bytes(a, b):
    return len(a) == len(b) and all(torch.equal(u.view(torch.uint8), v.view(torch.uint8)) for u, v in zip(a.arrays(), b.arrays()))


def _bits(t):
    return t.view(torch.int64)


def _check_interval(i, sims, step, counts_plain, counts_noisy):
    """step(sim, **kw) runs one interval; counts_*(sim) the route's count entry on the simulator's states before it"""
    stamps = SC.stamps(i)
    n_plain, n_noisy = counts_plain(sims['plain']), counts_noisy(sims['noisy'], stamps, i)
    frame = step(sims['frame'])
    events, stream = step(sims['plain'], stamps=stamps)
    off_events, off_stream = step(sims['off'], stamps=stamps)
    noisy_events, noisy_stream = step(sims['noisy'], stamps=stamps)
    image_events = step(sims['noisy_image'], stamps=stamps, stream=False)
    print(f"interval {i}: {len(stream)} events, {len(noisy_stream)} through the noisy sensor")
    assert len(stream) > 0 and len(noisy_stream) > 0
    # 1
    assert torch.equal(frame, events) and torch.equal(_bits(sims['frame'].state), _bits(sims['plain'].state))
    # 2
    assert np.array_equal(n_plain, _histogram(stream))
    assert np.array_equal(n_noisy, _histogram(noisy_stream))
    # 3
    assert torch.equal(off_events, events) and torch.equal(_bits(sims['off'].state), _bits(sims['plain'].state))
    assert _same_bytes(off_stream, stream)
    # 4
    assert torch.equal(image_events, noisy_events)
    assert torch.equal(_bits(sims['noisy_image'].state), _bits(sims['noisy'].state))
    assert torch.equal(_bits(sims['noisy_image'].last_event_time), _bits(sims['noisy'].last_event_time))


def test_images_route():
    from evennicer_slam_amd import functional as EF
    rng = np.random.default_rng(2024)
    imgs = [rng.integers(0, 256, (H, W)).astype(np.uint8)]
    for _ in range(2):
        imgs.append(np.clip(imgs[-1].astype(np.int64) + rng.integers(-60, 61, (H, W)), 0, 255).astype(np.uint8))
    imgs = [torch.from_numpy(im).to(DEV) for im in imgs]
    sims = _sims()
    for sim in sims.values():
        sim.reset(imgs[0])
    plan = EF.event_sim_plan(H, W, K, C.EPS, THRESHOLD, THRESHOLD, channels=1)
    for i, (prev, cur) in enumerate(zip(imgs[:-1], imgs[1:])):
        source = (_ptr(prev), _ptr(cur), _ptr(sims['plain']._lut), None, None)
        _check_interval(
            i, sims, lambda sim, **kw: sim.step_images(prev, cur, **kw),
            lambda sim: _counts('enslam_event_stream_images_count', plan, source, sim),
            lambda sim, stamps, interval: _counts('enslam_event_noisy_images_count', plan, source, sim,
                                                  _noise_tail(sim, stamps, interval)))


def test_boxroom_route():
    from evennicer_slam_amd import functional as EF
    from evennicer_slam_amd.event_sim import interpolate_poses
    from evennicer_slam_amd.synthetic import trajectory
    room = C.demo_room()
    poses = [p.double().numpy() for p in trajectory(room, 3, step=0.05, yaw_deg=2.0)]
    sims = _sims()
    for sim in sims.values():
        sim.reset((room, poses[0], CAM))
    plan = EF.event_sim_plan(H, W, K, C.EPS, THRESHOLD, THRESHOLD, cam=CAM, room=room)
    for i, (a, b) in enumerate(zip(poses[:-1], poses[1:])):
        rows = np.concatenate([a[None], interpolate_poses(a, b, K)], axis=0)[:, :3, :]
        rows = torch.from_numpy(np.ascontiguousarray(rows)).to(DEV)           # [K+1,3,4], the previous frame's first
        sub = rows[1:]                                                          # contiguous: the K sub-steps
        _check_interval(
            i, sims, lambda sim, **kw: sim.step_scene(room, a, b, CAM, **kw),
            lambda sim: _counts('enslam_event_stream_boxroom_count', plan, (_ptr(sub),), sim),
            lambda sim, stamps, interval: _counts('enslam_event_noisy_boxroom_count', plan, (_ptr(rows),), sim,
                                                  _noise_tail(sim, stamps, interval)))
