"""-m gpu: the sparse RGB-D schedule through the run harness (slam.SLAM with event.schedule 'reference') on a 10-frame 60 x 80
analytic sequence with simulated events, the contrast-threshold model as the event predictor, every_frame = rgbd_every_frame = 3:
what the harness hands the tracker, that 'forecast' never reads a frame without RGB-D, that event-only iterations run (two
captured graphs on the graphed route), that 'dense' is today's behaviour, and the two camera learning rates on the device.
Nothing here asserts that events improve the trajectory."""
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
N, EVERY = 10, 3
CAM = dict(H=60, W=80, fx=70.0, fy=70.0, cx=39.5, cy=29.5)


def make_sequence(root):
    from evennicer_slam_amd import datasets as D
    from evennicer_slam_amd.event_sim import EventSimulator
    from evennicer_slam_amd.synthetic import demo_config, write_demo_sequence
    sim = EventSimulator(CAM['H'], CAM['W'], c_pos=0.2, c_neg=0.2, device=DEV)
    (inp, evf), _poses = write_demo_sequence(str(root / 'data'), N, CAM, events='simulate', sim=sim)
    cfg = demo_config(inp, evf, CAM, device=DEV, env={'EVERY': EVERY, 'TRACK_ITERS': 4, 'TRACK_PIXELS': 200, 'MAP_ITERS': 5,
                                                      'MAP_PIXELS': 300, 'ITERS_FIRST': 40})
    ds = D.get_dataset(cfg, types.SimpleNamespace(input_folder=None, event_folder=None), 1, device=DEV)
    assert len(ds) == N and len(ds[1]) == 6 and bool(ds[1][3].any())
    return cfg, ds, root


@pytest.fixture(scope='module')
def sequence(tmp_path_factory):
    return make_sequence(tmp_path_factory.mktemp('schedule'))


def _config(cfg, schedule, depth='measured', graphed=False, events=True, **tracking):
    out = dict(cfg)
    out['event'] = dict(cfg['event'], activate_events=events, predictor='model', c_pos=0.2, c_neg=0.2, schedule=schedule,
                        rgbd_every_frame=EVERY, depth_on_event_frames=depth)
    out['tracking'] = dict(cfg['tracking'], graphed=graphed, **tracking)
    return out


def _slam(cfg, ds, out):
    from evennicer_slam_amd.slam import SLAM
    torch.manual_seed(0)
    np.random.seed(0)
    slam = SLAM(cfg, ds, str(out), device=DEV, static_shapes=True)
    assert np.isfinite(slam.prefit_decoders([0, 3, 6, 9], iters=60))
    return slam


def _record(slam):
    """wrap tracker.optimize_cam_in_batch: keep its arguments, call through"""
    calls, inner = [], slam.tracker.optimize_cam_in_batch

    def wrapper(camera_tensor, pre_c2w, gt_color, gt_depth, gt_event, gt_mask, batch_size, optimizer, idx, it, pre_gt_color, **kw):
        calls.append(dict(idx=int(idx), it=int(it), gt_color=gt_color, gt_depth=gt_depth, gt_event=gt_event.clone(),
                          pre_gt_color=pre_gt_color.clone(), init=pre_c2w.clone(), kw=dict(kw)))
        return inner(camera_tensor, pre_c2w, gt_color, gt_depth, gt_event, gt_mask, batch_size, optimizer, idx, it, pre_gt_color, **kw)

    slam.tracker.optimize_cam_in_batch = wrapper
    return calls


def _const_speed_init(est, idx):
    pre = est[idx - 1].float()
    return (pre @ est[idx - 2].float().inverse()) @ pre if idx >= 2 else pre


class Poisoned(object):
    """the dataset with NaN-filled depth and colour on every frame the plan gives no RGB-D"""

    def __init__(self, ds, plan):
        self.ds, self.plan = ds, plan

    def __len__(self):
        return len(self.ds)

    def __getitem__(self, i):
        idx, color, depth, event, mask, pose = self.ds[i]
        if not self.plan[i].rgbd:
            color, depth = torch.full_like(color, float('nan')), torch.full_like(depth, float('nan'))
        return idx, color, depth, event, mask, pose


@pytest.mark.parametrize('depth', ['measured', 'forecast'])
def test_what_the_harness_hands_the_tracker(sequence, depth):
    from evennicer_slam_amd.slam import frame_plan
    cfg, ds, root = sequence
    slam = _slam(_config(cfg, 'reference', depth), ds, root / ('hands_' + depth))
    calls = _record(slam)
    res = slam.run()
    plan = frame_plan(N, EVERY, EVERY, 'reference')
    assert sorted({c['idx'] for c in calls}) == list(range(1, N)) and len(calls) == 4 * (N - 1)
    for c in calls:
        step = plan[c['idx']]
        assert c['kw']['rgbd'] is step.rgbd and c['kw']['event'] is True
        want = sum(ds[k][3].to(torch.int64) for k in step.integrate)
        assert torch.equal(c['gt_event'].to(torch.int64), want), c['idx']
        assert torch.equal(c['pre_gt_color'], ds[step.anchor][1].float()), c['idx']
        if depth == 'forecast' and not step.rgbd:
            # no image of the frame, the forecast as the guidance: at the event resolution, holes are zeros
            assert c['gt_color'] is None and c['gt_depth'] is None
            g = c['kw']['guide_depth']
            assert tuple(g.shape) == (30, 40) and g.dtype == torch.float32 and bool(torch.isfinite(g).all())
            assert float((g > 0).float().mean()) > 0.5
        else:
            assert 'guide_depth' not in c['kw'] and torch.equal(c['gt_depth'], ds[c['idx']][2])
    assert bool(plan[4].integrate == (4,)) and bool(plan[6].integrate == (4, 5, 6))       # the sum does restart after a mapped frame
    est = slam.estimate_c2w_list[:N]
    assert bool(torch.isfinite(est).all()) and res['frames'] == N
    # mapping and keyframes on frames with RGB-D only
    assert all(plan[k].rgbd for k in slam.keyframe_list)


def test_dense_is_untouched(sequence):
    cfg, ds, root = sequence
    dense = _config(cfg, 'dense')
    absent = dict(dense, event={k: v for k, v in dense['event'].items() if k not in ('schedule', 'depth_on_event_frames')})
    for tag, c in (('dense', dense), ('absent', absent)):           # rgbd_every_frame = 3 stays ignored in both
        slam = _slam(c, ds, root / ('dense_' + tag))
        calls = _record(slam)
        slam.run(max_frames=5)
        assert sorted({c['idx'] for c in calls}) == [1, 2, 3, 4] and len(calls) == 16
        for c in calls:
            assert c['kw'] == dict(rgbd=True, event=True, scale_factor=0.5)
            assert torch.equal(c['gt_event'], ds[c['idx']][3])
            assert torch.equal(c['pre_gt_color'], ds[c['idx'] - 1][1].float())
            assert torch.equal(c['gt_color'], ds[c['idx']][1].float()) and torch.equal(c['gt_depth'], ds[c['idx']][2])


@pytest.mark.parametrize('graphed', [False, True])
@pytest.mark.parametrize('depth', ['forecast', 'none', 'measured'])
def test_forecast_does_not_read_missing_frames(sequence, depth, graphed):
    """NaN-filled colour and depth on every frame without RGB-D: 'forecast' and 'none' never look, 'measured' reads the frame's
    depth as the reference does -- the poison is seen when it is read."""
    from evennicer_slam_amd.slam import frame_plan
    cfg, ds, root = sequence
    plan = frame_plan(N, EVERY, EVERY, 'reference')
    c = _config(cfg, 'reference', depth, graphed=graphed)
    if depth == 'measured':
        # two frames are enough to see it, and no mapping iteration has to run on a poisoned frame and pose: frame 1 is tracked
        # with the frame's own (NaN) depth as the guidance of its event render
        c['mapping'] = dict(c['mapping'], iters=0)
    slam = _slam(c, Poisoned(ds, plan), root / f'poison_{depth}_{int(graphed)}')
    slam.run(max_frames=2 if depth == 'measured' else None)
    est = slam.estimate_c2w_list[:N]
    if depth == 'measured':
        assert bool(torch.isfinite(est[0]).all()) and not bool(torch.isfinite(est[1]).all())
    else:
        assert bool(torch.isfinite(est).all())
        assert bool(torch.isfinite(slam.shared_c['grid_middle']).all()) and bool(torch.isfinite(slam.shared_c['grid_color']).all())


@pytest.mark.parametrize('graphed', [False, True])
def test_event_only_iterations_run(sequence, graphed, monkeypatch):
    from evennicer_slam_amd import graph as G
    from evennicer_slam_amd.slam import frame_plan
    captured = []

    class Counting(G.GraphedStep):
        def __init__(self, *a, **kw):
            captured.append(1)
            super().__init__(*a, **kw)

    monkeypatch.setattr(G, 'GraphedStep', Counting)
    cfg, ds, root = sequence
    plan = frame_plan(N, EVERY, EVERY, 'reference')
    slam = _slam(_config(cfg, 'reference', 'forecast', graphed=graphed, seperate_LR=graphed), ds, root / f'event_only_{int(graphed)}')
    slam.run()
    est = slam.estimate_c2w_list[:N]
    assert bool(torch.isfinite(est).all())
    moved = {i: float((est[i] - _const_speed_init(est, i)).abs().max()) for i in range(1, N) if not plan[i].rgbd}
    print('event-only frames, largest change of a pose entry against the constant-speed initialisation:', moved)
    assert len(moved) == 6 and all(v > 1e-5 for v in moved.values()), moved
    if graphed:
        assert len(captured) == 2 and sorted(k[3] for k in slam._gtracks) == [False, True]
    else:
        assert not captured


def test_events_off_arm_leaves_event_only_frames_at_their_initialisation(sequence):
    from evennicer_slam_amd.slam import frame_plan
    cfg, ds, root = sequence
    plan = frame_plan(N, EVERY, EVERY, 'reference')
    slam = _slam(_config(cfg, 'reference', 'none', events=False), ds, root / 'events_off')
    calls = _record(slam)
    slam.run()
    assert sorted({c['idx'] for c in calls}) == [3, 6, 9]                                  # no iteration without a loss term
    assert all(c['kw']['rgbd'] is True and c['kw']['event'] is False for c in calls)
    est = slam.estimate_c2w_list[:N]
    for i in range(1, N):
        if not plan[i].rgbd:
            assert torch.allclose(est[i], _const_speed_init(est, i).cpu(), atol=1e-6), i


def test_separate_rates_on_the_device():
    """Adam's first step moves a parameter by its rate against the sign of its gradient: the quaternion by 0.2 lr, the
    translation by lr (Tracker.py:335-336); one rate moves all seven by lr."""
    from evennicer_slam_amd.tracker import CameraParameter, camera_learning_rates
    init = torch.tensor([1.0, 0.0, 0.0, 0.0, 0.1, 0.2, 0.3], device=DEV)
    for separate in (True, False):
        cam = CameraParameter(init, camera_learning_rates({'lr': 0.01, 'seperate_LR': separate}))
        assert cam.separate is separate
        loss = cam.tensor().sum()
        cam.opt.zero_grad()
        loss.backward()
        cam.opt.step()
        torch.cuda.synchronize()
        moved = (init - cam.value()).cpu()
        want = torch.tensor([0.002] * 4 + [0.01] * 3) if separate else torch.full((7,), 0.01)
        assert torch.allclose(moved, want, rtol=1e-4, atol=0), (moved, want)
        cam.restart(init, camera_learning_rates({'lr': 0.01, 'seperate_LR': separate}))
        assert torch.equal(cam.value(), init)
