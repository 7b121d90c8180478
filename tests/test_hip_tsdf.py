"""TSDF fusion on the GPU (csrc/tsdf.hip, tsdf.TSDFVolume) against the numpy restatement (tests/tsdf_numpy.py) on the case of
tests/tsdf_cases.py, bit for bit; Mesher.bound_method = 'tsdf'; tools/tsdf_fuse.py."""
import ctypes
import importlib.util
import json
import os
import types

import numpy as np
import pytest
import torch

from tests import tsdf_cases as C
from tests import tsdf_numpy as T

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _gpu_volume(stride, color, lo=None, hi=None):
    from evennicer_slam_amd.tsdf import TSDFVolume
    if lo is None:
        lo, hi = C.box()
    return TSDFVolume(C.VOXEL, C.TRUNC, lo, hi, C.CAM, color=color, depth_sampling_stride=stride, device=DEV)


def _integrate(vol, k):
    dep, col, c2w = C.frames()[k]
    vol.integrate(torch.from_numpy(dep).to(DEV), torch.from_numpy(col).to(DEV) if vol.has_color else None, torch.from_numpy(c2w))


def _dense(vol):
    """(units set, tsdf, weight, color) of a GPU volume laid out as the restatement's dense arrays."""
    units = vol.block_units().cpu().numpy()
    D = tuple(n * 16 for n in vol.nu)
    tsdf, weight = np.zeros(D, np.float32), np.zeros(D, np.float32)
    color = np.zeros(D + (3,), np.float32) if vol.has_color else None
    t, w = vol.tsdf.cpu().numpy(), vol.weight.cpu().numpy()
    c = vol.color.cpu().numpy() if vol.has_color else None
    for b, u in enumerate(units):
        s = tuple(slice(int(a) * 16, int(a) * 16 + 16) for a in (u - np.array(vol.unit_lo)))
        tsdf[s], weight[s] = t[b], w[b]
        if color is not None:
            color[s] = c[b]
    return {tuple(int(x) for x in u) for u in units}, tsdf, weight, color


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint64)


@pytest.mark.parametrize("stride", C.STRIDES)
@pytest.mark.parametrize("color", [True, False])
def test_volume_state_after_every_frame_is_the_restatements(stride, color):
    C.check_case()
    vol = _gpu_volume(stride, color)
    assert vol.nu == [4, 4, 3] and min(vol.unit_lo) < 0
    for k in range(3):
        _integrate(vol, k)
        ref = C.volume(stride, color, upto=k + 1)
        units, tsdf, weight, col = _dense(vol)
        assert units == ref.units()
        assert np.array_equal(_bits(weight), _bits(ref.weight))
        assert np.array_equal(_bits(tsdf), _bits(ref.tsdf))
        if color:
            assert np.array_equal(_bits(col), _bits(ref.color))
        else:
            assert vol.color is None
    st, rst = vol.stats, C.volume(stride, color).stats
    assert st['blocks'] == rst[-1]['blocks'] and len(st['frames']) == 3
    for got, want in zip(st['frames'], rst):
        assert {k: got[k] for k in got} == {k: want[k] for k in got}


@pytest.mark.parametrize("stride", C.STRIDES)
def test_mesh_is_the_restatements_bit_for_bit_and_deterministic(stride):
    C.check_case()
    rv, rf, rc = C.mesh(stride)

    def built(order):
        vol = _gpu_volume(stride, True)
        for k in order:
            _integrate(vol, k)
        return vol

    vol = built((0, 1, 2))
    v, f, c = vol.extract_mesh()
    assert v.dtype == torch.float64 and f.dtype == torch.int32 and c.dtype == torch.uint8 and v.is_cuda
    assert tuple(v.shape) == rv.shape and np.array_equal(_bits(v.cpu().numpy()), _bits(rv))
    assert np.array_equal(f.cpu().numpy(), rf)
    assert np.array_equal(c.cpu().numpy(), rc)
    v2, f2, c2 = vol.extract_mesh()                                  # a second extraction
    assert torch.equal(v.view(torch.int64), v2.view(torch.int64)) and torch.equal(f, f2) and torch.equal(c, c2)
    v3, f3, c3 = built((0, 1, 2)).extract_mesh()                     # the same volume rebuilt from scratch
    assert torch.equal(v.view(torch.int64), v3.view(torch.int64)) and torch.equal(f, f3) and torch.equal(c, c3)
    # frames in the order 3, 1, 2: other block ids, the same units and weights (the float32 running average itself depends
    # on the order, in Open3D as well: no assertion on tsdf across orders)
    other = built((2, 0, 1))
    ua, _, wa, _ = _dense(vol)
    ub, _, wb, _ = _dense(other)
    assert ua == ub and np.array_equal(wa, wb)
    assert not torch.equal(vol.block_units(), other.block_units())
    # without colour: the same geometry, no colours
    plain = _gpu_volume(stride, False)
    for k in range(3):
        _integrate(plain, k)
    pv, pf, pc = plain.extract_mesh()
    assert pc is None and torch.equal(pv.view(torch.int64), v.view(torch.int64)) and torch.equal(pf, f)


def test_edges_empty_frames_no_surface_and_points_outside_the_box():
    vol = _gpu_volume(4, True)
    H, W = C.CAM['H'], C.CAM['W']
    zero = torch.zeros((H, W), device=DEV)
    vol.integrate(zero, torch.zeros((H, W, 3), device=DEV), torch.eye(4))          # an all-zero depth frame: a no-op
    assert vol.n_blocks == 0 and vol.stats['frames'][0] == dict(blocks=0, touched=0, touched_outside=0, integrated_voxels=0)
    v, f, c = vol.extract_mesh()                                                   # nothing allocated
    assert tuple(v.shape) == (0, 3) and tuple(f.shape) == (0, 3) and tuple(c.shape) == (0, 3)
    assert v.dtype == torch.float64 and f.dtype == torch.int32 and c.dtype == torch.uint8
    _integrate(vol, 0)
    ref = C.volume(4, True, upto=1)
    assert _dense(vol)[0] == ref.units() and np.array_equal(_bits(_dense(vol)[1]), _bits(ref.tsdf))   # ... and it left no trace
    # a volume with blocks but no sign change: a wall 0.7 m away, the table ends in front of it
    far = _gpu_volume(1, False, [-0.1, -0.1, -0.30], [0.1, 0.1, -0.25])
    far.integrate(torch.full((H, W), 0.7, device=DEV), None, torch.eye(4))
    st = far.stats['frames'][0]
    assert far.n_blocks > 0 and st['integrated_voxels'] > 0 and st['touched_outside'] > 0
    assert float(far.tsdf[far.weight > 0].min()) > 0
    v, f, c = far.extract_mesh()
    assert tuple(v.shape) == (0, 3) and tuple(f.shape) == (0, 3) and c is None
    # every point outside an explicit small box: counted, nothing allocated
    away = _gpu_volume(1, False, [5.0, 5.0, 5.0], [5.5, 5.5, 5.5])
    dep = torch.from_numpy(C.frames()[0][0]).to(DEV)
    away.integrate(dep, None, torch.from_numpy(C.frames()[0][2]))
    assert away.n_blocks == 0 and away.stats['frames'][0]['touched_outside'] == int((dep > 0).sum())
    assert away.stats['frames'][0]['integrated_voxels'] == 0


def test_bad_arguments_raise_or_return_the_error_codes():
    import evennicer_slam_amd as E
    from evennicer_slam_amd import functional as EF
    from evennicer_slam_amd.tsdf import TSDFVolume
    with pytest.raises(ValueError, match="sdf_trunc"):
        TSDFVolume(0.01, 0.17, [0, 0, 0], [1, 1, 1], C.CAM, device=DEV)                # sdf_trunc > 16 voxels
    with pytest.raises(ValueError, match="block table"):
        TSDFVolume(0.004, 0.01, [-20, -20, -20], [20, 20, 1000.0], C.CAM, device=DEV)     # a stray far pixel: 625^2 * 15938 units
    vol = _gpu_volume(4, True)
    H, W = C.CAM['H'], C.CAM['W']
    with pytest.raises(ValueError):
        vol.integrate(torch.zeros((H, W + 1), device=DEV), torch.zeros((H, W, 3), device=DEV), torch.eye(4))
    with pytest.raises(ValueError):
        vol.integrate(torch.zeros((H, W), device=DEV), None, torch.eye(4))                 # a colour volume wants colour
    with pytest.raises(E.EnslamError):                                                     # the raw call: float32 depth only
        EF.tsdf_touch(torch.zeros((H, W), dtype=torch.float64, device=DEV), np.eye(4), C.CAM, 4, C.TRUNC, C.VOXEL, vol.unit_lo, vol.nu,
                      1, vol.stamps)
    assert vol.n_blocks == 0 and int(vol.stamps.abs().sum()) == 0
    # the C ABI: error codes before any launch
    lib = E._lib.lib()
    cam = (ctypes.c_double * 4)(35, 35, 19.5, 14.5)
    pose = (ctypes.c_double * 12)(1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0)
    lo, nu = (ctypes.c_int32 * 3)(-2, -2, -1), (ctypes.c_int32 * 3)(4, 4, 3)
    big = (ctypes.c_int32 * 3)(1024, 1024, 1024)
    depth = torch.zeros((H, W), device=DEV)
    part = torch.full((8,), -7, dtype=torch.int32, device=DEV)
    d, s, p = depth.data_ptr(), vol.stamps.data_ptr(), part.data_ptr()
    assert lib.enslam_tsdf_touch(None, H, W, 4, cam, pose, C.TRUNC, C.VOXEL, lo, nu, 1, s, p, None) == -1
    assert lib.enslam_tsdf_touch(d, H, W, 0, cam, pose, C.TRUNC, C.VOXEL, lo, nu, 1, s, p, None) == -1
    assert lib.enslam_tsdf_touch(d, H, W, 4, cam, pose, 17 * C.VOXEL, C.VOXEL, lo, nu, 1, s, p, None) == -1
    assert lib.enslam_tsdf_touch(d, H, W, 4, cam, pose, C.TRUNC, C.VOXEL, lo, big, 1, s, p, None) == -3
    assert lib.enslam_tsdf_touch(d, H, W, 4, cam, None, C.TRUNC, C.VOXEL, lo, nu, 1, s, p, None) == -1
    assert lib.enslam_tsdf_integrate(d, d, None, H, W, cam, pose, C.VOXEL, C.TRUNC, lo, nu, 0, None, None, 0, None, None, None, None,
                                     None) == -1                                           # no multiplier table
    assert lib.enslam_tsdf_integrate(d, d, d, H, W, cam, pose, C.VOXEL, C.TRUNC, lo, nu, 0, None, None, 0, None, None, None, None,
                                     None) == -1                                           # colour image without voxel colours
    assert lib.enslam_tsdf_mesh_count(None, nu, 0, None, None, None, None, None, None, None) == -1
    assert lib.enslam_tsdf_mesh_emit(vol.table.data_ptr(), lo, nu, 0, None, None, None, None, None, C.VOXEL, None, 0, 0, None, None, None,
                                     None) == -1                                           # no workspace
    torch.cuda.synchronize()
    assert int(vol.stamps.abs().sum()) == 0 and bool((part == -7).all())                   # no kernel ran


# ---- Mesher.bound_method ----------------------------------------------------------------------------------------------------------
MESHER_SCALE = 4.0            # voxel_length 4 * scale / 512 = 0.03125, sdf_trunc 0.04 * scale = 0.16: small enough to restate


def _tiny_mesher(bound, renderer, **meshing):
    from evennicer_slam_amd.mesher import MESHING_DEFAULTS, Mesher
    from tests.hip_util import cfg_like
    cfg = dict(cfg_like(), scale=MESHER_SCALE, meshing=dict(MESHING_DEFAULTS, resolution=48, **meshing),
               mapping=dict(marching_cubes_bound=(bound.double() / MESHER_SCALE).tolist()))
    slam = types.SimpleNamespace(renderer=renderer, bound=bound, nice=True, verbose=False, **C.CAM)
    return Mesher(cfg, None, slam)


def _keyframes():
    return [dict(est_c2w=torch.from_numpy(c2w).float().to(DEV), depth=torch.from_numpy(dep).to(DEV), color=torch.from_numpy(col).to(DEV))
            for dep, col, c2w in C.frames()]


def _rows_match(a, b, tol):
    """Every row of a has a row of b within tol (largest absolute difference), and the other way round."""
    d = np.abs(a[:, None, :] - b[None, :, :]).max(axis=2)
    return d.min(axis=1).max() <= tol and d.min(axis=0).max() <= tol


def test_mesher_tsdf_bound_is_the_hull_of_the_restated_mesh(tmp_path, monkeypatch):
    from evennicer_slam_amd import mesher as MS
    from tests.hip_util import tiny_on_gpu
    s, bound, model, grids, rays, renderer = tiny_on_gpu()
    kfs = _keyframes()
    # the restatement of what the reference fuses: its voxel size and truncation, stride 4, the keyframes' float32 poses
    voxel, trunc = 4.0 * MESHER_SCALE / 512.0, 0.04 * MESHER_SCALE
    pts = []
    poses = [kf['est_c2w'].cpu().double().numpy() for kf in kfs]
    for (dep, _, _), c2w in zip(C.frames(), poses):
        j, i = np.nonzero(dep > 0)
        d = dep[j, i].astype(np.float64)
        cam = np.stack([(i - C.CAM['cx']) / C.CAM['fx'] * d, -(j - C.CAM['cy']) / C.CAM['fy'] * d, -d], 1)
        pts.append(cam @ c2w[:3, :3].T + c2w[:3, 3])
    pts = np.concatenate(pts)
    ref = T.Volume(voxel, trunc, pts.min(0) - trunc, pts.max(0) + trunc, C.CAM, color=False, stride=4)
    for (dep, _, _), c2w in zip(C.frames(), poses):
        ref.integrate(dep, None, c2w)
    rv, _, _ = ref.extract_mesh()
    want = MS.hull_halfspaces(np.concatenate([rv, np.stack([p[:3, 3] for p in poses])]), 1.02)

    m = _tiny_mesher(bound, renderer, bound_method='tsdf')
    got = m.get_bound_from_frames(kfs, MESHER_SCALE)
    assert m.tsdf_stats['blocks'] == int(ref.allocated.sum()) and len(m.tsdf_stats['frames']) == 3
    assert got.dtype == np.float64 and got.shape[1] == 4 and _rows_match(got, want, 1e-12)
    # ... and that is the bound get_mesh uses
    seen = []
    real = MS.hull_halfspaces
    monkeypatch.setattr(MS, 'hull_halfspaces', lambda p, sc: seen.append(real(p, sc)) or seen[-1])
    with torch.no_grad():
        m.get_mesh(str(tmp_path / "tsdf.ply"), grids, model, kfs, None, 0, device=DEV, clean_mesh=False)
    assert len(seen) == 1 and _rows_match(seen[0], want, 1e-12) and 'hull' in m.timing


def test_mesher_default_bound_is_unchanged(tmp_path, monkeypatch):
    """bound_method 'depth_points' (the default): the half-spaces are hull_halfspaces(backprojected_points(...)) exactly, and
    the arrays and the file of get_mesh are those of a Mesher whose bound is that expression, written out as it stood before
    bound_method existed."""
    from evennicer_slam_amd import mesher as MS
    from tests.hip_util import tiny_on_gpu
    s, bound, model, grids, rays, renderer = tiny_on_gpu()
    kfs = _keyframes()
    cam6 = tuple(C.CAM[k] for k in ('H', 'W', 'fx', 'fy', 'cx', 'cy'))
    m = _tiny_mesher(bound, renderer)
    assert m.bound_method == 'depth_points'
    before = MS.hull_halfspaces(MS.backprojected_points(kfs, *cam6), m.clean_mesh_bound_scale)
    assert np.array_equal(m.get_bound_from_frames(kfs, MESHER_SCALE), before)
    out = []
    for tag in ('now', 'before'):
        m = _tiny_mesher(bound, renderer)
        if tag == 'before':
            monkeypatch.setattr(m, 'get_bound_from_frames', lambda keyframe_dict, scale=1, device=None:
                                MS.hull_halfspaces(MS.backprojected_points(keyframe_dict, *cam6), m.clean_mesh_bound_scale))
        path = str(tmp_path / f"{tag}.ply")
        with torch.no_grad():
            res = m.get_mesh(path, grids, model, kfs, None, 0, device=DEV, clean_mesh=False)
        out.append((res, open(path, 'rb').read() if res is not None else None))
    (a, pa), (b, pb) = out
    assert (a is None) == (b is None)
    if a is not None:
        assert np.array_equal(_bits(a[0]), _bits(b[0])) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and pa == pb


# ---- the tool -----------------------------------------------------------------------------------------------------------------
def test_tsdf_fuse_tool_writes_a_mesh_of_the_demo_room(tmp_path, capsys):
    import yaml
    from evennicer_slam_amd import eval_recon as R
    from evennicer_slam_amd import mesher as MS
    from evennicer_slam_amd.scene import scene_bound
    from evennicer_slam_amd.synthetic import BoxRoom, demo_config, write_demo_sequence
    cam = dict(H=60, W=80, fx=70.0, fy=70.0, cx=39.5, cy=29.5)
    (inp, evf), poses = write_demo_sequence(str(tmp_path / 'data'), 5, cam)
    cfg = demo_config(inp, evf, cam, device=DEV)
    base, child = str(tmp_path / 'base.yaml'), str(tmp_path / 'seq.yaml')
    with open(base, 'w') as f:
        yaml.safe_dump(cfg, f)
    with open(child, 'w') as f:
        yaml.safe_dump({'inherit_from': base}, f)
    spec = importlib.util.spec_from_file_location("tsdf_fuse_tool", os.path.join(ROOT, "tools", "tsdf_fuse.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    voxel, trunc = 0.02, 0.06
    out = str(tmp_path / 'fused.ply')
    capsys.readouterr()
    tool.main([child, out, '--voxel', str(voxel), '--trunc', str(trunc), '--color', '--every', '1'])
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    verts, faces, colors = MS.read_ply(out)
    assert line['frames'] == 5 and line['vertices'] == len(verts) > 1000 and line['faces'] == len(faces) > 1000
    assert colors is not None and colors.shape == verts.shape and faces.max() < len(verts)
    room = BoxRoom.for_bound(scene_bound([[-1.0, 1.1], [-0.9, 0.8], [-0.7, 0.6]], 1.0, 0.32), margin=0.12, seed=1)
    acc = R.accuracy(room.sample_surface(200000).numpy(), verts)
    print(f"tsdf_fuse on 5 demo frames: {line}; accuracy {acc:.4f} m (bound {voxel + trunc:.2f} m)")
    assert np.isfinite(acc) and acc < voxel + trunc
