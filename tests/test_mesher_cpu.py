"""Mesh extraction without a GPU: the generated case table (tools/gen_mc_tables.py -> csrc/mc_tables.hpp), the numpy
restatement of the marching cubes (tests/mc_numpy.py) on analytic fields, and the host helpers of mesher.py / eval_recon.py
on hand-built cases."""
import itertools
import os
import types

import numpy as np
import pytest
import torch

from tests import mc_numpy as M
from tools import gen_mc_tables as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_generator_reproduces_the_committed_table():
    with open(os.path.join(ROOT, "evennicer-slam_amd", "csrc", "mc_tables.hpp")) as f:
        assert f.read() == G.render()
    assert G.MAX_TRIS == 5


def _face_segments_drawn(case, face):
    """Undirected segments {edge, edge} the case's triangles draw on one cube face: triangle sides whose two edges both lie
    on that face and are not a fan diagonal inside the cell (a side on the face shared by exactly one triangle)."""
    on_face = {e for e in range(12) if face in G.EDGE_FACES[e]}
    sides = {}
    for t in G.TRIS[case]:
        for a, b in ((t[0], t[1]), (t[1], t[2]), (t[2], t[0])):
            if a in on_face and b in on_face:
                k = frozenset((a, b))
                sides[k] = sides.get(k, 0) + 1
    return {k for k, n in sides.items() if n == 1}


def test_face_segments_depend_only_on_the_face_bits():
    """Crack-freedom, exhaustively: what the table draws on a cube face is a function of that face's four corner bits, so
    the two cells sharing a face draw the same segments on it."""
    for f, (_axis, _side, cyc) in enumerate(G.FACES):
        by_bits = {}
        for case in range(256):
            bits = tuple((case >> c) & 1 for c in cyc)
            segs = _face_segments_drawn(case, f)
            assert by_bits.setdefault(bits, segs) == segs, (f, case)
        for bits, segs in by_bits.items():              # 0 / 2 crossings -> 0 / 1 segment; ambiguous -> 2
            crossings = sum(bits[k] != bits[(k + 1) % 4] for k in range(4))
            assert len(segs) == crossings // 2


def _oriented_sides(tris):
    return {(a, b) for t in tris for a, b in ((t[0], t[1]), (t[1], t[2]), (t[2], t[0]))}


def test_complementary_cases_reverse_the_winding_except_on_ambiguous_faces():
    """The rule for a face with four crossings (occupied corners diagonal): each OCCUPIED corner is cut off, so the free
    corners stay connected across the face.  Complementing the case swaps which pair is cut off, so cases with an ambiguous
    face differ from their complement by more than the winding; every other case gives the same surface reversed."""
    n_unamb = 0
    for case in range(256):
        comp = 255 - case
        amb = any(sum(((case >> cyc[k]) & 1) != ((case >> cyc[(k + 1) % 4]) & 1) for k in range(4)) == 4
                  for _a, _s, cyc in G.FACES)
        sides = _oriented_sides(G.TRIS[case])
        rev = {(b, a) for a, b in _oriented_sides(G.TRIS[comp])}
        loops = sorted(sorted(l) for l in G.case_loops(case))
        loops_c = sorted(sorted(l) for l in G.case_loops(comp))
        if not amb:
            n_unamb += 1
            assert loops == loops_c                     # same vertex loops ...
            boundary = {s for s in sides if (s[1], s[0]) not in sides}
            boundary_c = {s for s in rev if (s[1], s[0]) not in rev}
            assert boundary == boundary_c               # ... traversed the other way round
        else:
            assert loops != loops_c or sides != rev
    assert 0 < n_unamb < 256


def test_single_corner_winding_points_from_occupied_to_free():
    """Case 1 (corner 0 occupied): one triangle on the x, y, z edges of corner 0 whose normal points away from it."""
    assert G.TRIS[1] == [(0, 4, 8)]
    v, f = M.marching_cubes(np.array([[[1, -1], [-1, -1]], [[-1, -1], [-1, -1]]], np.float32), 0.0)
    n = np.cross(v[f[0, 1]] - v[f[0, 0]], v[f[0, 2]] - v[f[0, 0]])
    assert (n > 0).all()


@pytest.mark.parametrize("field,chi", [(M.sphere_field, 2), (M.torus_field, 0)])
def test_numpy_marching_cubes_closed_manifold_euler_and_volume(field, chi):
    vol, h, exact = field(48)
    v, f = M.marching_cubes(vol, 0.0, (-1., -1., -1.), (h, h, h))
    assert M.is_closed_oriented_manifold(f)
    assert M.euler_characteristic(v, f) == chi
    got = M.signed_volume(v, f)
    assert got > 0                                      # outward normals: positive signed volume
    assert abs(got / exact - 1) < 0.02


def test_numpy_marching_cubes_vertex_order_and_positions():
    vol = M.smooth_random_field(20, 3)
    origin, spacing = (0.5, -1.0, 2.0), (0.1, 0.2, 0.3)
    v, f = M.marching_cubes(vol, 0.0, origin, spacing)
    # every vertex lies on a lattice edge: two of its coordinates are lattice values
    idx = (v - np.array(origin)) / np.array(spacing)
    on_lattice = np.abs(idx - np.round(idx)) < 1e-9
    assert (on_lattice.sum(axis=1) >= 2).all()
    # owner order: the owner point (floor of the index) is non-decreasing in linear order
    own = np.floor(idx + 1e-9).astype(np.int64)
    lin = (own[:, 0] * 20 + own[:, 1]) * 20 + own[:, 2]
    assert (np.diff(lin) >= 0).all()
    assert f.min() == 0 and f.max() == len(v) - 1


# ---- mesher helpers ----------------------------------------------------------------------------------------------------
def test_ply_round_trip(tmp_path):
    from evennicer_slam_amd import mesher
    rng = np.random.default_rng(0)
    v = rng.normal(size=(50, 3))
    f = rng.integers(0, 50, size=(70, 3)).astype(np.int32)
    c = rng.integers(0, 256, size=(50, 3)).astype(np.uint8)
    p = str(tmp_path / "m.ply")
    mesher.write_ply(p, v, f, c)
    rv, rf, rc = mesher.read_ply(p)
    assert np.array_equal(rv, v.astype(np.float32)) and np.array_equal(rf, f) and np.array_equal(rc, c)
    head = open(p, "rb").read(400)
    assert head.startswith(b"ply\nformat binary_little_endian 1.0\n") and b"property list uchar int vertex_indices" in head
    mesher.write_ply(p, v, f)
    rv, rf, rc = mesher.read_ply(p)
    assert rc is None and np.array_equal(rf, f)


def test_hull_halfspaces_and_inside_test():
    from evennicer_slam_amd import mesher
    cube = np.array(list(itertools.product([0., 1.], repeat=3)))
    pts = np.concatenate([cube, [[0.5, 0.5, 0.5], [0.2, 0.7, 0.1]]])        # interior points do not change the hull
    hs = mesher.hull_halfspaces(pts, 1.02)
    probe = torch.tensor([[0.5, 0.5, 0.5], [1.005, 0.5, 0.5], [-0.005, 0.2, 0.9], [1.02, 0.5, 0.5], [0.5, -0.02, 0.5],
                          [0.5, 0.5, 2.0]])
    got = mesher.inside_halfspaces(probe, torch.from_numpy(hs), block=2).tolist()
    assert got == [True, True, True, False, False, False]                  # scaled by 1.02 about (0.5, 0.5, 0.5)


def test_backprojected_points_reach_the_depth():
    from evennicer_slam_amd import mesher
    H, W, fx, fy, cx, cy = 6, 8, 5.0, 5.0, 3.5, 2.5
    depth = torch.full((H, W), 2.0)
    depth[0, 0] = 0.0
    c2w = torch.eye(4)
    c2w[:3, 3] = torch.tensor([1.0, 2.0, 3.0])
    p = mesher.backprojected_points([dict(est_c2w=c2w, depth=depth)], H, W, fx, fy, cx, cy)
    assert np.allclose(p[-1], [1, 2, 3])                                  # the camera centre
    assert np.allclose(p[:-1, 2], 3.0 - 2.0)                              # camera looks along -z: z_world = 3 - depth


def _two_squares():
    """Two separate unit squares (2 triangles each) at z = 0 and z = 5, the second 3x larger, plus one stray vertex."""
    sq = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]], float)
    v = np.concatenate([sq, sq * 3 + [0, 0, 5], [[9, 9, 9]]])
    f = np.array([[0, 1, 2], [0, 2, 3], [4, 5, 6], [4, 6, 7]], np.int32)
    return v, f


def test_component_area_filter_and_unreferenced_vertices():
    from evennicer_slam_amd import mesher
    v, f = _two_squares()
    lab, n = mesher.face_components(f)
    assert n == 2 and lab[0] == lab[1] and lab[2] == lab[3] and lab[0] != lab[2]
    assert np.allclose(mesher.face_areas(v, f), [0.5, 0.5, 4.5, 4.5])
    assert np.array_equal(mesher.filter_components(v, f, 2.0), f[2:])      # area 1 removed, area 9 kept
    assert np.array_equal(mesher.filter_components(v, f, 0.5), f)
    assert np.array_equal(mesher.filter_components(v, f, 100.0, largest_only=True), f[2:])
    vv, ff = mesher.drop_unreferenced(v, f[2:])
    assert np.array_equal(vv, v[4:8]) and np.array_equal(ff, f[2:] - 4)
    # vertex-only contact does not join components (trimesh.split joins faces that share an edge)
    lab, n = mesher.face_components(np.array([[0, 1, 2], [2, 3, 4]]))
    assert n == 2


def _mesher(H=10, W=10, f=10.0):
    from evennicer_slam_amd.mesher import MESHING_DEFAULTS, Mesher
    slam = types.SimpleNamespace(renderer=None, bound=torch.zeros(3, 2), nice=True, verbose=False, H=H, W=W, fx=f, fy=f,
                                 cx=W / 2, cy=H / 2)
    cfg = dict(coarse=True, scale=1.0, occupancy=True, meshing=dict(MESHING_DEFAULTS),
               mapping=dict(marching_cubes_bound=[[-1, 1], [-1, 1], [-1, 1]]))
    return Mesher(cfg, None, slam)


def test_point_masks_frustum_and_depth():
    """Camera at the origin looking along -z (identity pose); image 10 x 10, f = 10: the frustum's half-angle tangent is 0.5.
    The probes lie on the optical axis or symmetrically off it, so the reference's cam_cord[:, 0] *= -1 does not decide them."""
    m = _mesher()
    kf = dict(est_c2w=torch.eye(4), depth=torch.full((10, 10), 2.0))
    pts = np.array([[0, 0, -1.0],      # in front, in view
                    [0, 0, 1.0],       # behind the camera
                    [0, 0, -2.15],     # closer than 1.1 x max depth (2.2): seen
                    [0, 0, -2.3],      # beyond 2.2: not seen (forecast needs the depth test too)
                    [0.6, 0, -1.0],    # outside the image (|x/z| > 0.5), inside the 1000-pixel forecast band
                    [0, 0.6, -1.0]])
    seen, forecast, unseen = m.point_masks(pts, [kf], None, 0, 'cpu')
    assert seen.tolist() == [True, False, True, False, False, False]
    assert forecast.tolist() == [False, False, False, False, True, True]
    assert unseen.tolist() == [False, True, False, True, False, False]
    # all frames up to idx instead of the keyframes: no depth limit
    seen, _, _ = m.point_masks(pts, [], [torch.eye(4), torch.eye(4)], 1, 'cpu', get_mask_use_all_frames=True)
    assert seen.tolist() == [True, False, True, True, False, False]


def test_mesher_refuses_what_it_does_not_implement(tmp_path):
    m = _mesher()
    with pytest.raises(NotImplementedError):
        m.get_mesh(str(tmp_path / "x.ply"), None, None, [], None, 0, device='cpu', show_forecast=True)
    m.color_mesh_extraction_method = 'render_ray_along_normal'
    with pytest.raises(NotImplementedError, match="iMAP"):
        m.get_mesh(str(tmp_path / "x.ply"), None, None, [], None, 0, device='cpu')
    m.depth_test = True
    with pytest.raises(NotImplementedError):
        m.point_masks(np.zeros((1, 3)), [], None, 0, 'cpu')


def test_eval_recon_metrics():
    from evennicer_slam_amd import eval_recon as R
    gt = np.array([[0, 0, 0], [1, 0, 0], [2, 0, 0], [3, 0, 0]], float)
    rec = np.array([[0, 0.01, 0], [1, 0.1, 0]], float)
    assert R.accuracy(gt, rec) == pytest.approx((0.01 + 0.1) / 2)
    assert R.completion(gt, rec) == pytest.approx((0.01 + 0.1 + np.hypot(1, 0.1) + np.hypot(2, 0.1)) / 4)
    assert R.completion_ratio(gt, rec) == 0.25
    assert R.completion_ratio(gt, rec, dist_th=0.2) == 0.5


def test_box_room_sample_surface():
    from evennicer_slam_amd.synthetic import BoxRoom
    room = BoxRoom([-1, -1, -1], [1, 1, 1], [0.2, -1, 0.2], [0.6, -0.4, 0.6])
    p = room.sample_surface(20000, seed=3)
    assert p.shape == (20000, 3) and p.dtype == torch.float64
    lo, hi, blo, bhi = room.room_lo, room.room_hi, room.box_lo, room.box_hi
    on_room = ((p == lo) | (p == hi)).any(1) & ((p >= lo) & (p <= hi)).all(1)
    on_box = ((p == blo) | (p == bhi)).any(1) & ((p >= blo) & (p <= bhi)).all(1)
    assert bool((on_room | on_box).all())
    assert not bool((on_room & on_box).any())           # nothing hidden: no wall patch under the box, no box face on a wall
    # area weighting: the box's 5 visible faces (1.12 m^2) against 24 - 0.16 m^2 of visible wall: 4.5 %
    frac = float(on_box.double().mean())
    assert abs(frac - 1.12 / 24.96) < 0.005
    assert torch.equal(room.sample_surface(100, seed=3), room.sample_surface(100, seed=3))
