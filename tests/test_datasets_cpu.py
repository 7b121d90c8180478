"""No GPU: the readers of the reference's further sequence layouts (datasets.ScanNet / TUM_RGBD / Azure / RPG_event_dense),
their writers, config.load_config and the `prepare` switch, on 8x10 sequences written into tmp_path."""
import os
import types

import numpy as np
import pytest
import torch

H, W = 8, 10
ARGS = types.SimpleNamespace(input_folder=None, event_folder=None)
FLIP = np.diag([1.0, -1.0, -1.0, 1.0])


def _cfg(name, inp, evf=None, **cam):
    data = {'input_folder': inp}
    if evf is not None:
        data['event_folder'] = evf
    return {'dataset': name, 'data': data,
            'cam': dict(dict(H=H, W=W, fx=9.0, fy=9.0, cx=4.5, cy=3.5, png_depth_scale=1000.0, crop_edge=0), **cam)}


def _frames(n, seed=0, color_hw=(H, W), grey=False):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        color = rng.integers(0, 256, color_hw if grey else color_hw + (3,), dtype=np.uint8)
        out.append((color, rng.integers(200, 4000, (H, W)).astype(np.float64) / 1000.0))
    return out


def _poses(n, seed=1):
    """n rigid camera-to-world matrices (float64) with well-spread rotations"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        q *= np.sign(np.linalg.det(q))
        p = np.eye(4)
        p[:3, :3], p[:3, 3] = q, rng.normal(size=3)
        out.append(p)
    return out


def _get(cfg, scale=1.0):
    from evennicer_slam_amd import datasets as D
    return D.get_dataset(cfg, ARGS, scale, device='cpu')


def test_dataset_dict_has_the_reference_keys_but_cofusion():
    from evennicer_slam_amd import datasets as D
    assert set(D.dataset_dict) == {'replica', 'replica_event', 'rpg', 'rpg_event', 'rpg_event_dense', 'tumrgbd', 'scannet', 'azure'}


def test_quaternion_round_trip():
    from evennicer_slam_amd import datasets as D
    for p in _poses(20, seed=3):
        q = D.matrix_quaternion(p[:3, :3])
        assert abs(np.linalg.norm(q) - 1) < 1e-12 and q[3] >= 0
        assert np.abs(D.quaternion_matrix(q) - p[:3, :3]).max() < 1e-12
        assert np.abs(D.quaternion_matrix(3.0 * q) - p[:3, :3]).max() < 1e-12      # normalised on the way in
    # a half turn (w = 0) and the identity
    assert np.allclose(D.quaternion_matrix(D.matrix_quaternion(np.diag([1.0, -1.0, -1.0]))), np.diag([1.0, -1.0, -1.0]))
    assert np.allclose(D.matrix_quaternion(np.eye(3)), [0, 0, 0, 1])


def test_scannet_numeric_order_and_colour_resized_to_depth(tmp_path):
    from evennicer_slam_amd import datasets as D
    frames = _frames(3, color_hw=(12, 16))                      # colour larger than the 8x10 depth
    poses = _poses(3)
    inp = D.write_scannet_sequence(str(tmp_path), frames, poses, 1000.0, numbers=[2, 10, 0])
    assert sorted(os.listdir(os.path.join(inp, 'frames', 'color'))) == ['0.jpg', '10.jpg', '2.jpg']
    ds = _get(_cfg('scannet', inp))
    assert isinstance(ds, D.ScanNet) and len(ds) == 3
    assert [os.path.basename(p) for p in ds.color_paths] == ['0.jpg', '2.jpg', '10.jpg']
    assert [os.path.basename(p) for p in ds.depth_paths] == ['0.png', '2.png', '10.png']
    for item, src in zip((0, 1, 2), (2, 0, 1)):                 # file 0 was written third, 2 first, 10 second
        idx, color, depth, pose = ds[item]
        assert idx == item and tuple(color.shape) == (H, W, 3) and color.dtype == torch.float64
        assert tuple(depth.shape) == (H, W) and depth.dtype == torch.float32
        assert np.abs(depth.numpy() - frames[src][1]).max() <= 0.5 / 1000.0 + 1e-6
        assert np.allclose(pose.numpy(), poses[src], atol=1e-6) and pose.dtype == torch.float32
        want = D._resize_bilinear(D._imread_rgb(ds.color_paths[item]) / 255., (H, W))
        assert np.array_equal(color.numpy(), want)
    # the colour really went through the resize: it is no crop of the 12x16 image
    assert not np.array_equal(ds[0][1].numpy(), D._imread_rgb(ds.color_paths[0])[:H, :W] / 255.)


def _tum_expected(stamps, depth_stamps, pose_stamps, poses, max_dt=0.08, rate=32):
    """brute-force restatement of the association: kept colour indices, their depth stamps and their poses"""
    kept = []
    for i, t in enumerate(stamps):
        dd = [abs(td - t) for td in depth_stamps]
        dp = [abs(tp - t) for tp in pose_stamps]
        j, k = dd.index(min(dd)), dp.index(min(dp))
        if dd[j] < max_dt and dp[k] < max_dt:
            if not kept or t - stamps[kept[-1][0]] > 1.0 / rate:
                kept.append((i, j, k))
    first = poses[kept[0][2]] @ FLIP                             # the file's (OpenCV) convention: y / z columns flipped
    out = []
    for i, j, k in kept:
        rel = np.linalg.inv(first) @ (poses[k] @ FLIP)
        rel[:3, 1] *= -1
        rel[:3, 2] *= -1
        out.append(rel)
    return kept, out


def test_tum_association_thinning_and_relative_poses(tmp_path):
    from evennicer_slam_amd import datasets as D
    #          0     1      2     3     4      5
    stamps = [1.00, 1.02, 1.10, 1.20, 1.30, 1.335]              # 1 is 0.02 s after 0: thinned (1/32 s rule); 5 is 0.035 after 4: kept
    depth_stamps = [1.01, 1.03, 1.11, None, 1.29, 1.34]          # 3 has no depth image: the nearest (1.29) is 0.09 s away
    frames = _frames(6, seed=4)
    pose_stamps = [0.99, 1.095, 1.21, 1.31, 1.33]                # a different clock: the nearest pose is looked up per frame
    poses = _poses(5, seed=5)
    inp = D.write_tum_sequence(str(tmp_path), frames, poses, 5000.0, stamps=stamps, depth_stamps=depth_stamps,
                               pose_stamps=pose_stamps)
    ds = _get(_cfg('tumrgbd', inp, png_depth_scale=5000.0))
    d_list = [t for t in depth_stamps if t is not None]
    kept, want_poses = _tum_expected(stamps, d_list, pose_stamps, poses)
    assert [i for i, _, _ in kept] == [0, 2, 4, 5]                # 1 thinned, 3 dropped
    assert isinstance(ds, D.TUM_RGBD) and len(ds) == len(kept)
    assert [os.path.basename(p) for p in ds.color_paths] == [f'{stamps[i]:.6f}.png' for i, _, _ in kept]
    assert [os.path.basename(p) for p in ds.depth_paths] == [f'{d_list[j]:.6f}.png' for _, j, _ in kept]
    assert np.array_equal(ds.poses[0].numpy(), FLIP.astype(np.float32))
    for got, want in zip(ds.poses, want_poses):
        assert got.dtype == torch.float32 and np.abs(got.numpy() - want).max() < 1e-6
    assert np.abs(ds.poses[1].numpy() - FLIP).max() > 1e-2        # later poses are not the identity
    idx, color, depth, pose = ds[1]
    assert np.array_equal(color.numpy(), frames[2][0] / 255.)     # png colour: exact
    assert np.abs(depth.numpy() - frames[2][1]).max() <= 0.5 / 5000.0 + 1e-6
    # translation scaled in place on every access, as in the reference
    t0 = ds.poses[2][:3, 3].clone()
    ds2 = _get(_cfg('tumrgbd', inp, png_depth_scale=5000.0), scale=2.0)
    assert torch.equal(ds2[2][3][:3, 3], 2.0 * t0) and torch.equal(ds2[2][3][:3, 3], 4.0 * t0)


def test_tum_pose_txt_and_crop(tmp_path):
    from evennicer_slam_amd import datasets as D
    frames, poses = _frames(3, seed=6), _poses(3, seed=7)
    inp = D.write_tum_sequence(str(tmp_path), frames, poses, 5000.0, pose_file='pose.txt')
    ds = _get(_cfg('tumrgbd', inp, png_depth_scale=5000.0, crop_size=[6, 8], crop_edge=1))
    assert len(ds) == 3
    _, color, depth, _ = ds[0]
    assert tuple(color.shape) == (4, 6, 3) and tuple(depth.shape) == (4, 6)


def test_azure_log_records_and_identity_without_log(tmp_path):
    from evennicer_slam_amd import datasets as D
    frames, poses = _frames(3, seed=8), _poses(3, seed=9)
    inp = D.write_azure_sequence(str(tmp_path / 'a'), frames, poses, 1000.0)
    with open(os.path.join(inp, 'scene', 'trajectory.log')) as f:
        lines = f.readlines()
    assert len(lines) == 15 and lines[5].split() == ['1', '1', '2'] and len(lines[6].split()) == 4
    ds = _get(_cfg('azure', inp))
    assert isinstance(ds, D.Azure) and len(ds) == 3 and len(ds.poses) == 3
    for got, want in zip(ds.poses, poses):
        assert np.allclose(got.numpy(), want, atol=1e-6)
    assert tuple(ds[2][1].shape) == (H, W, 3)
    inp2 = D.write_azure_sequence(str(tmp_path / 'b'), frames, None, 1000.0)
    ds2 = _get(_cfg('azure', inp2))
    assert len(ds2.poses) == 3 and all(torch.equal(p, torch.eye(4)) for p in ds2.poses)
    assert ds2[1][3].dtype == torch.float32


def test_rpg_event_dense(tmp_path):
    from evennicer_slam_amd import datasets as D
    density, n_img = 3, 3
    n_event = (n_img - 1) * density
    frames = _frames(n_img, seed=10, grey=True)
    rng = np.random.default_rng(11)
    events = [rng.integers(0, 4, (H, W, 2)).astype(np.uint8) for _ in range(n_event)]
    for k, ev in enumerate(events):
        ev[0, 0] = (k + 1, 0)                                    # (-, +): distinguishes the channels and the frames
    poses = _poses(n_event + 1, seed=12)
    inp, evf = D.write_rpg_event_dense_sequence(str(tmp_path), frames, poses, 1000.0, events, density)
    cfg = _cfg('rpg_event_dense', inp, evf)
    cfg['data']['density'] = density
    ds = _get(cfg)
    assert isinstance(ds, D.RPG_event_dense) and len(ds) == n_event + 1 == 7 and ds.n_img == n_img and ds.n_event == n_event
    for i in range(len(ds)):
        idx, color, depth, event, mask, pose = ds[i]
        assert idx == i and np.allclose(pose.numpy(), poses[i], atol=1e-6)
        assert np.array_equal(color.numpy(), np.repeat(frames[i // density][0][:, :, None], 3, axis=2) / 255.)
        assert np.abs(depth.numpy() - frames[i // density][1]).max() <= 0.5 / 1000.0 + 1e-6
        assert event.dtype == torch.uint8 and tuple(event.shape) == (H, W, 2) and mask.dtype == torch.int64
        if i == 0:
            assert not bool(event.any()) and not bool(mask.any())
        else:
            assert np.array_equal(event.numpy(), events[i - 1])             # (-, +)
            assert tuple(event[0, 0].tolist()) == (i, 0)
            assert np.array_equal(mask.numpy(), (events[i - 1] != 0).any(-1).astype(np.int64))
    # the count assertions: an event frame too few, a pose line too few
    os.remove(sorted(os.path.join(evf, f) for f in os.listdir(evf))[-1])
    with pytest.raises(AssertionError, match="events does not match that of GT images"):
        _get(cfg)
    inp2, evf2 = D.write_rpg_event_dense_sequence(str(tmp_path / 'b'), frames, poses, 1000.0, events, density)
    traj = os.path.join(inp2, f'traj_density{density}.txt')
    with open(traj) as f:
        lines = f.readlines()
    with open(traj, 'w') as f:
        f.writelines(lines[:-1])
    cfg2 = _cfg('rpg_event_dense', inp2, evf2)
    cfg2['data']['density'] = density
    with pytest.raises(AssertionError, match="events does not match that of GT poses"):
        _get(cfg2)


def test_load_config_inherit_chain(tmp_path):
    import yaml
    from evennicer_slam_amd.config import load_config
    root, mid, leaf, default = (str(tmp_path / n) for n in ('root.yaml', 'mid.yaml', 'leaf.yaml', 'default.yaml'))
    with open(default, 'w') as f:
        yaml.safe_dump({'scale': 1, 'verbose': True, 'mapping': {'iters': 60, 'BA': False}}, f)
    with open(root, 'w') as f:
        yaml.safe_dump({'dataset': 'replica', 'mapping': {'iters': 10, 'pixels': 100, 'stage': {'color': {'lr': 0.1, 'decoders_lr': 0.2}}},
                        'cam': {'H': 680, 'W': 1200}}, f)
    with open(mid, 'w') as f:
        yaml.safe_dump({'inherit_from': root, 'dataset': 'tumrgbd', 'mapping': {'stage': {'color': {'lr': 0.5}}}, 'cam': {'H': 480}}, f)
    with open(leaf, 'w') as f:
        yaml.safe_dump({'inherit_from': mid, 'mapping': {'pixels': 7, 'brand_new': {'a': 1}}, 'data': {'input_folder': 'x', 'prepare': 'device'},
                        'cam': {'crop_size': [384, 512]}}, f)
    cfg = load_config(leaf, default)
    assert cfg['dataset'] == 'tumrgbd' and cfg['scale'] == 1 and cfg['verbose'] is True
    assert cfg['mapping'] == {'iters': 10, 'BA': False, 'pixels': 7, 'brand_new': {'a': 1},
                              'stage': {'color': {'lr': 0.5, 'decoders_lr': 0.2}}}
    assert cfg['cam'] == {'H': 480, 'W': 1200, 'crop_size': [384, 512]}
    assert cfg['data'] == {'input_folder': 'x', 'prepare': 'device'} and cfg['inherit_from'] == mid
    # without a default: the chain alone; a parent named relative to the child's folder is found too
    with open(mid, 'w') as f:
        yaml.safe_dump({'inherit_from': 'root.yaml', 'dataset': 'scannet'}, f)
    cfg = load_config(leaf)
    assert cfg['dataset'] == 'scannet' and 'scale' not in cfg and cfg['mapping']['iters'] == 10


def test_prepare_switch(tmp_path):
    from evennicer_slam_amd import datasets as D
    from evennicer_slam_amd._lib import EnslamError
    inp = D.write_azure_sequence(str(tmp_path), _frames(2, seed=13), None, 1000.0)
    cfg = _cfg('azure', inp)
    ds = _get(cfg)
    assert ds.prepare == 'host'
    host = ds[1]
    cfg['data']['prepare'] = 'device'
    ds_dev = _get(cfg)
    assert ds_dev.prepare == 'device'
    with pytest.raises(EnslamError, match="needs a HIP device"):
        ds_dev[1]
    ds_dev.prepare = 'host'                                      # can be set after construction
    assert all(torch.equal(a, b) for a, b in zip(host[1:], ds_dev[1][1:]))
    ds_dev.prepare = 'gpu'
    with pytest.raises(ValueError, match="'host' or 'device'"):
        ds_dev[1]
