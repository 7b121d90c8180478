"""TSDF fusion without a GPU: the exports of csrc/tsdf.hip, the numpy restatement (tests/tsdf_numpy.py) on closed forms and on
the case of tests/tsdf_cases.py, mesher.hull_candidates against scipy alone, and Mesher.bound_method's host side."""
import ctypes
import os
import types

import numpy as np
import pytest
import torch

from tests import tsdf_cases as C
from tests import tsdf_numpy as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TSDF_EXPORTS = ("enslam_tsdf_touch", "enslam_tsdf_integrate", "enslam_tsdf_mesh_workspace", "enslam_tsdf_mesh_count",
                "enslam_tsdf_mesh_emit")


def test_tsdf_exports_in_header_binding_and_library():
    import __graft_entry__ as G
    G.build()
    import evennicer_slam_amd as E
    header = open(os.path.join(ROOT, "include", "enslam_hip.h")).read()
    handle = ctypes.CDLL(E.LIB_PATH)
    for name in TSDF_EXPORTS:
        assert name + "(" in header, name
        assert name in E._lib.EXPORTS and E._lib._SIGS[name][1], name
        assert hasattr(handle, name), name
    nb = ctypes.c_int64()
    lib = E._lib.lib()
    assert lib.enslam_tsdf_mesh_workspace(3, ctypes.byref(nb)) == 0 and nb.value >= 3 * 4096 * 6       # host arithmetic only
    assert lib.enslam_tsdf_mesh_workspace(3, None) == -1 and lib.enslam_tsdf_mesh_workspace(-1, ctypes.byref(nb)) == -1
    assert lib.enslam_tsdf_mesh_workspace(100001, ctypes.byref(nb)) == -3
    from evennicer_slam_amd import tsdf                                # noqa: F401  (the module imports without a device)
    with pytest.raises(NotImplementedError):
        tsdf.TSDFVolume(0.04, 0.12, [0, 0, 0], [1, 1, 1], C.CAM, device='cpu')


# ---- the restatement on closed forms ----------------------------------------------------------------------------------------
WALL_D = 1.0


def _wall_volume(views):
    """A wall at z = -WALL_D seen head-on by a camera at the origin with the identity pose, fused `views` times."""
    cam = C.CAM
    hx, hy = cam['W'] / 2 / cam['fx'] * WALL_D, cam['H'] / 2 / cam['fy'] * WALL_D
    vol = T.Volume(C.VOXEL, C.TRUNC, [-hx, -hy, -WALL_D - C.TRUNC], [hx, hy, -WALL_D + C.TRUNC], cam, color=False, stride=1)
    depth = np.full((cam['H'], cam['W']), WALL_D, np.float32)
    for _ in range(views):
        vol.integrate(depth, None, np.eye(4))
    return vol


def test_restatement_wall_head_on_matches_the_closed_form():
    cam = C.CAM
    for views in (1, 2):
        vol = _wall_volume(views)
        ix, iy, iz = np.nonzero(np.ones_like(vol.weight, bool))
        ctr = (np.stack([ix, iy, iz], 1) + vol.unit_lo * 16 + 0.5) * vol.vl
        zc = -ctr[:, 2]
        u = np.floor(ctr[:, 0] * cam['fx'] / zc + cam['cx'] + 0.5)
        v = np.floor(-ctr[:, 1] * cam['fy'] / zc + cam['cy'] + 0.5)
        in_image = (u >= 0) & (u < cam['W']) & (v >= 0) & (v < cam['H'])
        on_edge = (np.abs(ctr[:, 0] * cam['fx'] / zc + cam['cx'] + 0.5 - np.round(ctr[:, 0] * cam['fx'] / zc + cam['cx'] + 0.5)) < 1e-6) | \
                  (np.abs(-ctr[:, 1] * cam['fy'] / zc + cam['cy'] + 0.5 - np.round(-ctr[:, 1] * cam['fy'] / zc + cam['cy'] + 0.5)) < 1e-6)
        mult = np.sqrt(1 + ((u - cam['cx']) / cam['fx']) ** 2 + ((v - cam['cy']) / cam['fy']) ** 2)
        s = WALL_D - zc                                             # signed distance along the optical axis, + in front
        expect_seen = in_image & (s * mult > -C.TRUNC) & np.repeat(np.repeat(np.repeat(vol.allocated, 16, 0), 16, 1), 16, 2).reshape(-1)
        w, t = vol.weight.reshape(-1), vol.tsdf.reshape(-1)
        sure = ~on_edge & (np.abs(s * mult + C.TRUNC) > 1e-9)
        assert np.array_equal(w[sure] > 0, expect_seen[sure])
        assert set(np.unique(w[sure])) == {0.0, float(views)}
        sel = sure & expect_seen
        assert sel.sum() > 4000
        assert np.abs(t[sel] - np.minimum(1.0, s[sel] * mult[sel] / C.TRUNC)).max() <= 2e-7      # float32 rounding of values <= 1
        assert (t[sel] == 1.0).any() and (t[sel] < 0).any()


def test_restatement_one_view_mesh_faces_the_camera_and_references_every_vertex():
    vol = _wall_volume(1)
    v, f, c = vol.extract_mesh()
    assert c is None and f.shape[0] > 1000
    # (D - zc) * mult changes sign on z edges only, at the wall's plane; the two ends of an edge may project to different
    # pixels, and with r = mult_b / mult_a in [1 / rho, rho] the interpolated zero moves by at most (rho - 1) of a voxel
    rho = vol.mult.max() / vol.mult.min()
    assert np.abs(v[:, 2] + WALL_D).max() <= (rho - 1) * C.VOXEL
    tri = v[f]
    n = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    assert (np.einsum('ij,ij->i', n, -tri.mean(axis=1)) > 0).all()    # camera at the origin
    assert np.array_equal(np.unique(f), np.arange(v.shape[0]))


def test_case_reaches_every_branch_and_lies_on_the_analytic_surface():
    counts = C.check_case()
    print("case:", counts)
    for stride in C.STRIDES:
        v, f, c = C.mesh(stride)
        assert np.array_equal(np.unique(f), np.arange(v.shape[0]))
        assert c.shape == v.shape and c.dtype == np.uint8
        d = C.surface_distance(v)
        print(f"stride {stride}: {v.shape[0]} vertices, {f.shape[0]} faces, largest distance to the surface {d.max():.4f} m")
        # a vertex sits on an edge ending at a voxel with averaged tsdf in (-1, 0): within sdf_trunc behind an observed
        # surface point, and the vertex within one voxel of it
        assert d.max() <= C.VOXEL + C.TRUNC


def test_case_mesh_is_independent_of_the_block_opening_order_in_its_layout():
    """Frames in the order 3, 1, 2 open the blocks in another order: the same units, the same weights."""
    a, b = C.volume(4), C.new_volume(4, True, order=(2, 0, 1))
    assert a.units() == b.units()
    assert np.array_equal(a.weight, b.weight)


# ---- hull_candidates against scipy alone ---------------------------------------------------------------------------------------
def _hull_vertex_set(p):
    from scipy.spatial import ConvexHull
    return set(map(tuple, p[ConvexHull(p).vertices]))


def _check_candidates(points):
    from evennicer_slam_amd.mesher import hull_candidates
    cand = hull_candidates(torch.from_numpy(points)).numpy()
    assert _hull_vertex_set(cand) == _hull_vertex_set(points)
    assert set(map(tuple, cand)) <= set(map(tuple, points))
    return cand


def test_hull_candidates_keep_the_hull_of_the_case():
    v, _, _ = C.mesh(1)
    points = np.concatenate([v, np.stack([c2w[:3, 3] for _, _, c2w in C.frames()])])
    cand = _check_candidates(points)
    print(f"{len(_hull_vertex_set(points))} hull vertices, {len(cand)} survivors of {len(points)} points")
    assert len(cand) < len(points) // 3


def test_hull_candidates_on_a_gaussian_cloud_and_a_cube():
    from evennicer_slam_amd.mesher import hull_candidates
    cloud = np.random.default_rng(3).standard_normal((20000, 3))
    assert len(_check_candidates(cloud)) < 2000
    corners = np.array([[x, y, z] for x in (0., 1.) for y in (0., 1.) for z in (0., 1.)])
    inner = np.random.default_rng(4).uniform(0.05, 0.95, (500, 3))
    cand = _check_candidates(np.concatenate([inner[:250], corners, inner[250:]]))
    assert set(map(tuple, cand)) == set(map(tuple, corners))
    flat = np.random.default_rng(5).uniform(0, 1, (50, 3))
    flat[:, 2] = 0.25                                                # coplanar: scipy raises on the extremes, all points return
    assert np.array_equal(hull_candidates(torch.from_numpy(flat)).numpy(), flat)
    assert np.array_equal(hull_candidates(flat).numpy(), flat)       # numpy in, tensor out


# ---- Mesher.bound_method -------------------------------------------------------------------------------------------------------
def _mesher(**meshing):
    from evennicer_slam_amd.mesher import MESHING_DEFAULTS, Mesher
    slam = types.SimpleNamespace(renderer=None, bound=torch.zeros(3, 2), nice=True, verbose=False, **C.CAM)
    cfg = dict(coarse=True, scale=1.0, occupancy=True, meshing=dict(MESHING_DEFAULTS, **meshing),
               mapping=dict(marching_cubes_bound=[[-1, 1], [-1, 1], [-1, 1]]))
    return Mesher(cfg, None, slam)


def test_mesher_bound_method_default_unknown_and_cpu():
    from evennicer_slam_amd import mesher as MS
    assert MS.MESHING_DEFAULTS['bound_method'] == 'depth_points'
    assert _mesher().bound_method == 'depth_points'
    cfg_without = {k: v for k, v in MS.MESHING_DEFAULTS.items() if k != 'bound_method'}
    slam = types.SimpleNamespace(renderer=None, bound=torch.zeros(3, 2), nice=True, verbose=False, **C.CAM)
    m = MS.Mesher(dict(coarse=True, scale=1.0, occupancy=True, meshing=cfg_without, mapping=dict(marching_cubes_bound=[[-1, 1]] * 3)),
                  None, slam)
    assert m.bound_method == 'depth_points'                          # a config without the key keeps today's bound
    with pytest.raises(ValueError):
        _mesher(bound_method='open3d')
    dep, _, c2w = C.frames()[0]
    kfs = [dict(est_c2w=torch.from_numpy(c2w), depth=torch.from_numpy(dep))]
    base = m.get_bound_from_frames(kfs)
    assert np.array_equal(base, MS.hull_halfspaces(MS.backprojected_points(kfs, *(C.CAM[k] for k in ('H', 'W', 'fx', 'fy', 'cx', 'cy'))),
                                                   m.clean_mesh_bound_scale))
    m.bound_method = 'nonsense'                                      # settable after construction, checked when used
    with pytest.raises(ValueError):
        m.get_bound_from_frames(kfs)
    m.bound_method = 'tsdf'
    with pytest.raises(NotImplementedError):
        m.get_bound_from_frames(kfs)
    with pytest.raises(NotImplementedError):
        m.get_bound_from_frames(kfs, device='cpu')
