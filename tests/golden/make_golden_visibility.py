#!/usr/bin/env python3
"""Golden fixture for the visibility kernel (csrc/visibility.hip): tests/golden/tiny_visibility.npz.

Runs only in the build container (needs /root/reference, CPU torch).  The reference's Mesher and Mapper modules import
open3d, skimage, trimesh, cv2, colorama, wandb, matplotlib and others that are absent here, but Mesher.point_masks and
Mapper.keyframe_selection_overlap themselves use only torch and numpy.  This script registers EMPTY stand-in modules for the
missing imports, loads the reference's modules from the reference tree, creates the two objects without running their
constructors (only the attributes the two methods read are set) and CALLS the reference's own methods on the CPU.  It
contains no reference statements.

Every array written is an input chosen here (camera, poses, depth images, point sets) or an output of those two reference
methods; `ov_points` is the project's own mapper.ray_sample_points applied on the CPU to the rays the reference's
get_samples returned (recorded by wrapping get_samples in the reference module's namespace).

Inputs: the tiny camera (H 48, W 64, f 50), 8 seeded keyframe poses in and around a 4 m box -- some look across the box,
some outwards, so that the seen, forecast and unseen classes each hold a fair share of the lattice -- and 8 seeded smooth
depth images with some zero pixels.  Masks are bit-packed; lattice points are stored as axis specifications (lo, hi, n).

Usage:  python tests/golden/make_golden_visibility.py"""
import os
import sys
import types

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG  # noqa: E402,F401  (sets up sys.path, the torchvision stub, cwd = the reference tree)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def _stand_in(name, **attrs):
    m = types.ModuleType(name)
    for k, v in attrs.items():
        setattr(m, k, v)
    sys.modules[name] = m
    return m


for _name in ('open3d', 'skimage', 'trimesh', 'cv2', 'wandb', 'matplotlib', 'matplotlib.pyplot', 'PIL', 'PIL.Image'):
    if _name not in sys.modules:
        try:
            __import__(_name)
        except Exception:
            _stand_in(_name)
_stand_in('colorama', Fore=None, Style=None)
# modules of the reference that exist but drag in more missing imports: the two methods use none of their names
_stand_in('src.utils.datasets', get_dataset=None)
_stand_in('src.utils.Visualizer', Visualizer=None)
_stand_in('src.event_net', inference_event=None)

import src.Mapper as ref_mapper_mod  # noqa: E402
from src.Mapper import Mapper as RefMapper  # noqa: E402
from src.utils.Mesher import Mesher as RefMesher  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from tests import visibility_numpy as V  # noqa: E402

CAM = V.CAM
LATTICE_SPEC = np.array([[-2.0, 2.0, 64], [-2.0, 2.0, 64], [-2.0, 2.0, 64]], np.float64)
LATTICE_CHUNK = 100000          # points_batch_size for the lattice: 262144 points span three chunks
N_SCATTER = 5000


def look_at(pos, target):
    """float32 camera-to-world [4,4] of a camera at pos looking at target (camera axes: x right, y up, -z forward)"""
    pos, target = np.asarray(pos, np.float64), np.asarray(target, np.float64)
    f = (target - pos) / np.linalg.norm(target - pos)
    right = np.cross(f, [0.0, 0.0, 1.0])
    right /= np.linalg.norm(right)
    up = np.cross(right, f)
    m = np.eye(4)
    m[:3, 0], m[:3, 1], m[:3, 2], m[:3, 3] = right, up, -f, pos
    return m.astype(np.float32)


def make_inputs(seed=7):
    rng = np.random.default_rng(seed)
    # cameras gathered in a slab of the +x half of the box; five look across it (-x, little tilt, so the region behind them
    # stays unseen), three stand near a wall and look outwards along +y / -y / +z
    c2w = []
    outward = [np.array([-0.2, 1.0, 0.1]), np.array([-0.2, -1.0, -0.1]), np.array([-0.3, 0.2, 1.0])]
    for k in range(8):
        pos = np.array([rng.uniform(0.2, 0.9), rng.uniform(-1.2, 1.2), rng.uniform(-0.8, 0.8)])
        if k < 5:
            target = pos + np.array([-1.0, rng.uniform(-0.35, 0.35), rng.uniform(-0.25, 0.25)])
        else:
            pos = np.where(np.abs(outward[k - 5]) == 1.0, outward[k - 5] * rng.uniform(0.8, 1.2), pos)
            target = pos + outward[k - 5] + 0.1 * rng.standard_normal(3)
        c2w.append(look_at(pos, target))
    c2w = np.stack(c2w)
    H, W = CAM['H'], CAM['W']
    jj, ii = np.meshgrid(np.arange(H), np.arange(W), indexing='ij')
    depth = []
    for k in range(8):
        a, b, ph = rng.uniform(0.05, 0.15), rng.uniform(0.05, 0.12), rng.uniform(0, 6.28, 2)
        d = 0.6 + a * np.sin(b * ii + ph[0]) + a * np.cos(b * jj + ph[1]) + 0.01 * rng.standard_normal((H, W))
        if k < 5:       # one half of the view is far (an open door): the depth limit 1.1 x max is wide, and the depth test
            d[:, :W // 2] += 4.0        # drops the near points in front of the far half
        else:           # the outward views measure far walls only: the depth test drops what is near them
            d += 2.8
        d[rng.random((H, W)) < 0.03] = 0.0
        depth.append(d.astype(np.float32))
    depth = np.stack(depth)
    scatter = rng.uniform(-2.5, 2.5, (N_SCATTER, 3)).astype(np.float32)
    return c2w, depth, scatter


def ref_mesher(depth_test, points_batch_size):
    m = object.__new__(RefMesher)
    m.points_batch_size = points_batch_size
    m.depth_test = depth_test
    m.H, m.W, m.fx, m.fy, m.cx, m.cy = (CAM[k] for k in ('H', 'W', 'fx', 'fy', 'cx', 'cy'))
    return m


def pack3(seen, forecast, unseen):
    assert not (seen & forecast).any() and ((seen | forecast) ^ unseen).all()
    return np.packbits(seen), np.packbits(forecast)


def main():
    c2w, depth, scatter = make_inputs()
    keyframes = [dict(est_c2w=torch.from_numpy(c2w[k]), depth=torch.from_numpy(depth[k])) for k in range(8)]
    c2w_list = torch.from_numpy(c2w)
    lattice = torch.from_numpy(V.lattice_points(V.axes_from_spec(LATTICE_SPEC)).astype(np.float32))
    out = dict(cam=np.array([CAM[k] for k in ('H', 'W', 'fx', 'fy', 'cx', 'cy')], np.float64), c2w=c2w, depth=depth,
               lattice_spec=LATTICE_SPEC, lattice_chunk=np.int64(LATTICE_CHUNK), scatter=scatter,
               scatter_chunk=np.int64(2000), all_frames_idx=np.int64(7))
    share = {}
    for name, pts, chunk in (('lattice', lattice, LATTICE_CHUNK), ('scatter', torch.from_numpy(scatter), 2000)):
        for variant, depth_test, all_frames in (('plain', False, False), ('depth', True, False), ('all', False, True)):
            m = ref_mesher(depth_test, chunk)
            with torch.no_grad():
                s, f, u = m.point_masks(pts.clone(), keyframes, c2w_list, 7, 'cpu', get_mask_use_all_frames=all_frames)
            out[f'{name}_{variant}_seen'], out[f'{name}_{variant}_forecast'] = pack3(s, f, u)
            share[name, variant] = (s.mean(), f.mean(), u.mean())
            print(f'{name:8s} {variant:6s} seen {s.mean():.3f} forecast {f.mean():.3f} unseen {u.mean():.3f}')
    assert min(share['lattice', 'plain']) >= 0.05, "each class must hold at least 5 % of the lattice"
    assert share['lattice', 'plain'][0] - share['lattice', 'depth'][0] >= 0.05, "the depth test must cost seen 5 % of the lattice"

    # ---- keyframe_selection_overlap: current frame = a ninth seeded view, the 8 keyframes above
    rng = np.random.default_rng(11)
    cur_c2w = torch.from_numpy(look_at([1.0, 0.3, 0.2], [-2.0, -0.4, 0.0]))
    cur_depth = torch.from_numpy((1.5 + 0.5 * rng.random((CAM['H'], CAM['W']))).astype(np.float32))
    cur_color = torch.from_numpy(rng.random((CAM['H'], CAM['W'], 3)).astype(np.float32))
    mp = object.__new__(RefMapper)
    mp.device = 'cpu'
    mp.H, mp.W, mp.fx, mp.fy, mp.cx, mp.cy = (CAM[k] for k in ('H', 'W', 'fx', 'fy', 'cx', 'cy'))
    recorded = []
    ref_get_samples = ref_mapper_mod.get_samples

    def recording_get_samples(*a, **k):
        r = ref_get_samples(*a, **k)
        recorded.append([t.detach().clone() for t in r])
        return r

    ref_mapper_mod.get_samples = recording_get_samples
    try:
        torch.manual_seed(5)
        np.random.seed(3)
        sel_all = mp.keyframe_selection_overlap(cur_color, cur_depth, cur_c2w, keyframes, 8)
        torch.manual_seed(5)                      # the same pixels again
        np.random.seed(3)
        sel_3 = mp.keyframe_selection_overlap(cur_color, cur_depth, cur_c2w, keyframes, 3)
    finally:
        ref_mapper_mod.get_samples = ref_get_samples
    assert all(torch.equal(a, b) for a, b in zip(recorded[0], recorded[1]))
    rays_o, rays_d, d, _ = recorded[0]
    sys.path.insert(0, ROOT)
    import evennicer_slam_amd.mapper as our_mapper
    pts = our_mapper.ray_sample_points(rays_o, rays_d, d, 16).numpy()
    print('overlap: selected', sorted(int(i) for i in sel_all), 'of 8; k = 3 under np.random.seed(3):', [int(i) for i in sel_3])
    assert 0 < len(sel_all) < 8, "the selection should keep some keyframes and drop some"
    out.update(ov_c2w=cur_c2w.numpy(), ov_rays_o=rays_o.numpy(), ov_rays_d=rays_d.numpy(), ov_depth=d.numpy(), ov_points=pts,
               ov_selected_all=np.array(sorted(int(i) for i in sel_all), np.int64), ov_selected_3=np.array(sel_3, np.int64),
               ov_numpy_seed=np.int64(3))
    path = os.path.join(HERE, 'tiny_visibility.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
