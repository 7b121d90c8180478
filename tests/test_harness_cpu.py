"""Run-harness pieces that need no GPU: the cv2-free Replica_event reader, the frustum mask, and the
checkpoint the harness's Logger writes -- read back the way the reference's src/tools/eval_ate.py reads it
(:281-303) and scored against the statistics the REFERENCE's own evaluate_ate gives for the same trajectories
(tests/golden/ate_checkpoint.npz, written by tests/golden/make_golden_ate.py)."""
import os
import types

import numpy as np
import torch

import evennicer_slam_amd as E
from evennicer_slam_amd import datasets as D
from tests.util import load


def _sequence(tmp_path, n=4, H=24, W=32, seed=0):
    rng = np.random.default_rng(seed)
    frames = [(rng.random((H, W, 3)), (rng.random((H, W)) * 3).astype(np.float32)) for _ in range(n)]
    poses = []
    for i in range(n):
        p = np.eye(4)
        p[:3, 3] = [0.1 * i, 0.02 * i, -0.05 * i]
        poses.append(p)
    events = [rng.integers(0, 3, (H, W, 2)).astype(np.uint8) for _ in range(n - 1)]
    inp, evf = D.write_replica_event_sequence(str(tmp_path), frames, poses, 6553.5, events)
    cfg = {'dataset': 'replica_event', 'cam': dict(H=H, W=W, fx=20., fy=20., cx=15.5, cy=11.5, png_depth_scale=6553.5, crop_edge=0),
           'data': {'input_folder': inp, 'event_folder': evf}}
    return cfg, frames, poses, events


def test_replica_event_reader_roundtrip(tmp_path):
    cfg, frames, poses, events = _sequence(tmp_path)
    ds = D.get_dataset(cfg, types.SimpleNamespace(input_folder=None, event_folder=None), 1, device='cpu')
    assert len(ds) == 4
    idx, color, depth, event, mask, pose = ds[2]
    assert idx == 2 and color.dtype == torch.float64 and depth.dtype == torch.float32 and event.dtype == torch.uint8
    assert tuple(color.shape) == (24, 32, 3) and tuple(event.shape) == (24, 32, 2) and mask.dtype == torch.int64
    assert float((color - torch.from_numpy(frames[2][0])).abs().max()) < 0.03          # JPEG, quality 100
    assert float((depth - torch.from_numpy(frames[2][1])).abs().max()) < 1.0 / 6553.5
    assert np.array_equal(event.numpy(), events[1])                                     # (-, +) of the png's (0, -, +)
    assert np.array_equal(mask.numpy(), (events[1] != 0).any(-1).astype(np.int64))
    assert np.allclose(pose.numpy(), poses[2], atol=1e-6)
    assert int(ds[0][3].abs().max()) == 0                                               # frame 0: all-black event image
    # crop_edge and scale follow the reference (:104-113)
    cfg['cam']['crop_edge'] = 2
    ds2 = D.get_dataset(cfg, types.SimpleNamespace(input_folder=None, event_folder=None), 2.0, device='cpu')
    _, c2, d2, e2, m2, p2 = ds2[1]
    assert tuple(d2.shape) == (20, 28) and tuple(e2.shape) == (20, 28, 2)
    assert np.allclose(d2.numpy(), 2.0 * frames[1][1][2:-2, 2:-2], atol=2.0 / 6553.5)
    assert np.allclose(p2[:3, 3].numpy(), 2.0 * poses[1][:3, 3], atol=1e-6)
    # a lens model on a Replica-layout sequence: the colour image is undistorted, the depth is not (datasets.py:84-88)
    ds3 = D.get_dataset(dict(cfg, cam=dict(cfg['cam'], crop_edge=0, distortion=[0.1, 0, 0, 0])), types.SimpleNamespace(), 1, device='cpu')
    _, c3, d3, _e, _m, _p = ds3[1]
    assert torch.equal(d3, ds[1][2]) and not torch.equal(c3, ds[1][1])


def test_frustum_mask_selects_what_the_camera_sees():
    from evennicer_slam_amd.slam import frustum_mask
    bound = torch.tensor([[-2.0, 2.0], [-2.0, 2.0], [-2.0, 2.0]], dtype=torch.float64)
    cam = dict(H=48, W=64, fx=50.0, fy=50.0, cx=31.5, cy=23.5)
    c2w = torch.eye(4)                                       # camera at the origin looking down -z (the path's convention)
    depth = torch.full((48, 64), 1.0)
    m = frustum_mask(c2w, depth, (21, 21, 21), bound, cam)
    assert m.dtype == torch.bool and tuple(m.shape) == (21, 21, 21)
    ax = torch.linspace(-2, 2, 21)
    zi = lambda z: int(torch.argmin((ax - z).abs()))
    c = 10                                                   # x = y = 0
    assert bool(m[zi(-1.0), c, c]) and bool(m[zi(-1.4), c, c])           # on the axis, in front, within depth + 0.5
    assert not bool(m[zi(-1.8), c, c])                                   # beyond depth + 0.5
    assert not bool(m[zi(1.0), c, c])                                    # behind the camera
    assert bool(m[zi(0.2), c, c])                                        # within 0.5 m of the camera centre
    assert not bool(m[zi(-1.0), c, 20])                                  # far off-axis: outside the image
    depth0 = torch.zeros((48, 64))
    depth0[:, :32] = 1.0
    m0 = frustum_mask(c2w, depth0, (21, 21, 21), bound, cam)             # zero depth -> filled with the maximum
    assert bool(m0[zi(-1.0), c, zi(0.2)]) and bool(m0[zi(-1.0), c, zi(-0.2)])     # one lands on a zero-depth pixel, one on a valid one


def _write_checkpoint(tmp_path, n=30, seed=3):
    rng = np.random.default_rng(seed)
    gt = torch.eye(4).repeat(n, 1, 1)
    est = torch.eye(4).repeat(n, 1, 1)
    t = np.linspace(0, 4, n)
    gt[:, :3, 3] = torch.from_numpy(np.stack([np.cos(t), np.sin(0.7 * t), 0.3 * t], 1)).float()
    est[:, :3, 3] = gt[:, :3, 3] + torch.from_numpy(0.02 * rng.standard_normal((n, 3))).float() + torch.tensor([0.3, -0.1, 0.2])
    model = E.get_model({'model': {'c_dim': 32, 'coarse_bound_enlarge': 2, 'pos_embedding_method': 'fourier'}, 'data': {'dim': 3},
                         'coarse': True, 'grid_len': {'coarse': 2, 'middle': 0.32, 'fine': 0.16, 'color': 0.16}})
    slam = types.SimpleNamespace(verbose=False, ckptsdir=str(tmp_path), shared_c={'grid_coarse': torch.zeros(1, 32, 2, 2, 2)},
                                 gt_c2w_list=gt, shared_decoders=model, estimate_c2w_list=est)
    path = E.eval_ate.Logger({}, None, slam).log(n - 1, [], [0, 5, 10])
    return path, gt, est


def test_checkpoint_format_and_ate_against_the_reference_tool(tmp_path):
    import evennicer_slam_amd.eval_ate as EA
    path, gt, est = _write_checkpoint(tmp_path)
    assert os.path.basename(path) == '00029.tar' and EA.latest_checkpoint(str(tmp_path)) == path
    ckpt = torch.load(path, map_location='cpu', weights_only=False)
    assert set(ckpt) == {'c', 'decoder_state_dict', 'gt_c2w_list', 'estimate_c2w_list', 'keyframe_list', 'selected_keyframes', 'idx'}
    mine = EA.evaluate_checkpoint(path, scale=1.0)
    assert mine['compared_pose_pairs'] == 30 and 0.0 < mine['absolute_translational_error.rmse'] < 0.1
    # the reference's own tool on the same trajectories (eval_ate.py:281-303 load the lists; convert_poses needs mathutils,
    # but evaluate_ate only reads the translations): its statistics are stored in the fixture, next to the translations
    # they were computed from, which must be the ones in this checkpoint
    fx = load("ate_checkpoint")
    N = ckpt['idx']
    assert np.array_equal(torch.stack([ckpt['gt_c2w_list'][i][:3, 3] for i in range(N + 1)]).numpy(), fx['gt_trans'])
    assert np.array_equal(torch.stack([ckpt['estimate_c2w_list'][i][:3, 3] for i in range(N + 1)]).numpy(), fx['est_trans'])
    keys = str(fx['stat_keys']).split('\n')
    assert sorted(mine) == keys
    for k, v in zip(keys, fx['stats']):
        assert abs(mine[k] - v) <= 1e-9 * max(1.0, abs(v)), k


def _smooth_image(u, v):
    """A smooth analytic grey image as a function of (undistorted) pixel coordinates."""
    return 127.5 + 60.0 * np.sin(0.05 * u + 0.3) * np.cos(0.04 * v - 0.2) + 40.0 * np.sin(0.021 * (u + v))


def test_undistort_round_trip_and_identity():
    """`undistort` = cv2.undistort(img, K, dist) restated (cv2 is not in the image): zero coefficients are the identity, and an
    image DISTORTED analytically with OpenCV's lens model (rational radial + tangential, the RPG configuration's coefficients
    times 5 to make the effect large) comes back as the undistorted original up to bilinear interpolation error."""
    H, W = 130, 173
    K = (98.36, 98.34, 86.25, 64.75)                                   # configs/rpg/rpg.yaml:62-68 at half resolution
    dist = np.array([-0.08409333, 0.05335822, -0.00065521, -0.0001679, 0, 0, 0, 0]) * 5
    u, v = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    ideal = _smooth_image(u, v)
    assert np.array_equal(D.undistort(ideal.astype(np.uint8), K, np.zeros(8)), ideal.astype(np.uint8))
    # what the lens shows at distorted pixel (u', v'): the scene ray (x, y) with distort(x, y) = ((u'-cx)/fx, (v'-cy)/fy);
    # invert the model by fixed-point iteration (the way cv2.undistortPoints does)
    xd, yd = (u - K[2]) / K[0], (v - K[3]) / K[1]
    x, y = xd.copy(), yd.copy()
    for _ in range(600):
        fx_, fy_ = D.distort_points(x, y, dist)
        x, y = x - (fx_ - xd), y - (fy_ - yd)
    fx_, fy_ = D.distort_points(x, y, dist)
    assert np.abs(fx_ - xd).max() < 1e-9 and np.abs(fy_ - yd).max() < 1e-9
    lens = _smooth_image(K[0] * x + K[2], K[1] * y + K[3])              # float image as the distorting lens records it
    back = D.undistort(lens, K, dist)
    # compare where the source position of the pixel lies inside the recorded image (elsewhere: zero border)
    sx, sy = D.distort_points((u - K[2]) / K[0], (v - K[3]) / K[1], dist)
    mx, my = K[0] * sx + K[2], K[1] * sy + K[3]
    inside = (mx >= 1) & (mx <= W - 2) & (my >= 1) & (my <= H - 2)
    assert inside.mean() > 0.8
    assert np.abs(back - ideal)[inside].max() < 0.25                    # grey levels of 255: bilinear error of a smooth image
    moved = np.hypot(mx - u, my - v)
    assert moved.max() > 3.0                                            # the lens model really moved pixels (by > 3 px at the rim)
    out8 = D.undistort(np.clip(np.rint(lens), 0, 255).astype(np.uint8), K, dist)
    assert out8.dtype == np.uint8 and np.abs(out8.astype(np.float64) - ideal)[inside].max() <= 1.5


def test_rpg_event_reader_roundtrip(tmp_path):
    """RPG_event (src/utils/datasets.py:242-319; BASELINE config 5's format): grey frames replicated to 3 channels, 16-bit depth
    / png_depth_scale, event pngs (+, -, 0) handed out as (-, +), mask, pose flip; with cam.distortion colour and events are
    undistorted and the depth is not."""
    rng = np.random.default_rng(3)
    n, H, W = 4, 26, 34
    frames = [((rng.random((H, W)) * 255).astype(np.uint8), (rng.random((H, W)) * 3).astype(np.float32)) for _ in range(n)]
    poses = []
    for i in range(n):
        p = np.eye(4)
        p[:3, 3] = [0.1 * i, 0.02 * i, -0.05 * i]
        poses.append(p)
    events = [rng.integers(0, 3, (H, W, 2)).astype(np.uint8) for _ in range(n - 1)]
    inp, evf = D.write_rpg_event_sequence(str(tmp_path), frames, poses, 1000.0, events)
    cam = dict(H=H, W=W, fx=19.6, fy=19.6, cx=16.5, cy=12.5, png_depth_scale=1000.0, crop_edge=0)
    cfg = {'dataset': 'rpg_event', 'cam': cam, 'data': {'input_folder': inp, 'event_folder': evf}}
    ds = D.get_dataset(cfg, types.SimpleNamespace(input_folder=None, event_folder=None), 1, device='cpu')
    assert len(ds) == n
    idx, color, depth, event, mask, pose = ds[2]
    assert color.dtype == torch.float64 and tuple(color.shape) == (H, W, 3)
    assert np.array_equal(np.rint(color.numpy() * 255).astype(np.uint8), np.repeat(frames[2][0][:, :, None], 3, 2))
    assert float((depth - torch.from_numpy(frames[2][1])).abs().max()) <= 0.5 / 1000.0 + 1e-6
    assert np.array_equal(event.numpy(), events[1]) and event.dtype == torch.uint8      # (-, +)
    assert np.array_equal(mask.numpy(), (events[1] != 0).any(-1).astype(np.int64))
    assert np.allclose(pose.numpy(), poses[2], atol=1e-6)
    assert int(ds[0][3].abs().max()) == 0
    cfg_d = dict(cfg, cam=dict(cam, distortion=[-0.4, 0.25, -0.003, -0.001, 0, 0, 0, 0]))
    dsd = D.get_dataset(cfg_d, types.SimpleNamespace(input_folder=None, event_folder=None), 1, device='cpu')
    _, cd, dd, ed, md, _pd = dsd[2]
    assert torch.equal(dd, depth)                                       # the depth is never undistorted
    assert not torch.equal(cd, color) and not torch.equal(ed, event)
    K = (cam['fx'], cam['fy'], cam['cx'], cam['cy'])
    want = D.undistort(np.repeat(frames[2][0][:, :, None], 3, 2), K, np.array(cfg_d['cam']['distortion']))
    assert np.array_equal(np.rint(cd.numpy() * 255).astype(np.uint8), want)
    assert 'rpg' in D.dataset_dict and issubclass(D.RPG_event, D.RPG)
