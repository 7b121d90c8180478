"""The headless visualiser without a GPU: the conditions the seeded cases of tests/viz_cases.py must meet, the numpy yardstick
of the rasteriser (tests/viz_numpy.py) against independent statements worked by hand, and the host side of
evennicer_slam_amd/viz.py and tools/visualizer.py (actors, viewer pose, intrinsics, bookkeeping, the frame walk)."""
import math
import os

import numpy as np
import pytest
import torch

from tests import viz_cases as C
from tests import viz_numpy as Y


# ---- the cases ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", C.NAMES)
def test_case_margins(name):
    C.check_margins(name)


def test_case_image_is_odd_and_small():
    assert C.CAM['H'] == 45 and C.CAM['W'] == 61 and C.K == 3 and len(C.soup_views()) == 3 and len(C.room_views()) == 3


def test_room_case_shows_with_culling_1_and_is_empty_with_culling_2():
    for r in C.case('room_cull1')[1]:
        assert (r['id'] >= 0).all()                                         # inside a closed room: every pixel sees a face
    for r in C.case('room_cull2')[1]:
        assert (r['id'] == -1).all() and (r['rgb'] == 255).all() and not r['depth'].any()
    for r1, r0 in zip(C.case('room_cull1')[1], C.case('room_cull0_plain')[1]):
        assert np.array_equal(r1['id'], r0['id']) and np.array_equal(r1['depth'], r0['depth'])
        assert not np.array_equal(r1['rgb'], r0['rgb'])                     # vertex colours against grey
    for rb, r1 in zip(C.case('roombox_cull1')[1], C.case('room_cull1')[1]):
        assert (rb['id'] >= 12).any() and (rb['id'][rb['id'] < 12] == r1['id'][rb['id'] < 12]).all()       # the box hides walls


def test_soup_case_reaches_every_route():
    v, f, _ = C.soup_mesh()
    assert 195 <= len(f) <= 210
    z = v[f[:C.SOUP_FACES]][:, :, 2]                                        # view 0 is the identity: camera space
    assert ((z.max(1) > 0) & (z.min(1) < 0)).sum() >= 8 and (z.min(1) > 0).sum() >= 8      # crossing the camera plane, behind it
    for k, m in enumerate(C.soup_views()):
        assert (C.box_pixels(v, f, m, C.CAM) > 256).sum() >= 4, k          # the large route, beside the whole-image boxes
    assert f[C.OUT_OF_RANGE].max() >= len(v)
    a, b, c = f[C.DEGENERATE]
    assert not Y.cross(v[b] - v[a], v[c] - v[a]).any()
    ids = C.case('soup_points4')[1][0]['id']
    for face, copy in C.DUPLICATES:
        assert np.array_equal(f[face], f[copy])
        assert (ids == face).sum() > 0 and (ids == copy).sum() == 0         # the tie goes to the smaller id
    assert not (ids == C.DEGENERATE).any() and not (ids == C.OUT_OF_RANGE).any()
    # culling splits the faces
    id1, id2 = C.case('soup_points1')[1][0]['id'], C.case('soup_cull2')[1][0]['id']
    assert (id1 >= 0).any() and (id2 >= 0).any() and not np.intersect1d(id1[id1 >= 0], id2[id2 >= 0]).size
    assert (C.case('soup_cull2')[1][0]['rgb'][id2 == -1] == (10, 20, 30)).all()


@pytest.mark.parametrize("point_size", [1, 4])
def test_point_case_reaches_every_route(point_size):
    p, _ = C.soup_points()
    assert 290 <= len(p) <= 310
    m = C.soup_views()[0]
    ok, z, a, b, _ = Y.point_squares(p, m, C.CAM, point_size, 0.0, 1000.0)
    assert (z <= 0).sum() >= 3 and (z > 1000).sum() == 3 and not ok[z <= 0].any() and not ok[z > 1000].any()
    if point_size == 4:                                                     # squares cut by the left, right, top, bottom border
        on = ok & (a < C.CAM['W']) & (a + 4 > 0) & (b < C.CAM['H']) & (b + 4 > 0)
        assert (on & (a < 0)).any() and (on & (a + 4 > C.CAM['W'])).any()
        assert (on & (b < 0)).any() and (on & (b + 4 > C.CAM['H'])).any()
    name = 'soup_points4' if point_size == 4 else 'soup_points1'
    r = C.case(name)[1][0]
    shown = np.unique(-2 - r['id'][r['id'] < -1])
    assert len(shown) >= 10                                                 # points in front of faces ...
    v, f, _ = C.soup_mesh()
    args = C.case(name)[0]
    alone = Y.raster(v[:0], f[:0], m, C.CAM, points=p, point_colors=args['point_colors'], point_size=point_size)
    hidden = (alone['id'] < -1) & (r['id'] >= 0)
    assert hidden.sum() >= 10                                               # ... and behind them
    if point_size == 4:
        assert np.array_equal(alone['id'], C.case('points_only')[1][0]['id'])


# ---- the yardstick against independent statements -------------------------------------------------------------------------------
def test_yardstick_fronto_parallel_triangle():
    cam = dict(H=9, W=11, fx=10.0, fy=10.0, cx=5.0, cy=4.0)
    # at depth 2 a pixel (j, i) sees the world point (x, y) = ((i - 5) / 5, -(j - 4) / 5)
    tri = np.array([[-0.73, -0.61, -2.0], [0.81, -0.52, -2.0], [0.07, 0.67, -2.0]])
    jj, ii = np.meshgrid(np.arange(9.0), np.arange(11.0), indexing='ij')
    x, y = (ii - 5) / 5, -(jj - 4) / 5
    inside = np.ones((9, 11), bool)
    for (ax, ay), (bx, by) in ((tri[0, :2], tri[1, :2]), (tri[1, :2], tri[2, :2]), (tri[2, :2], tri[0, :2])):
        inside &= (bx - ax) * (y - ay) - (by - ay) * (x - ax) >= 0         # to the left of each edge: counter-clockwise
    assert 5 <= inside.sum() <= 40
    eye = np.eye(4)[:3]
    ccw, cw = np.array([[0, 1, 2]]), np.array([[0, 2, 1]])
    # counter-clockwise seen from the eye: the stored normal points at the eye, det < 0: culling 2 keeps it, culling 1 drops it
    for faces, keep, drop in ((ccw, 2, 1), (cw, 1, 2)):
        for cull in (0, keep):
            r = Y.raster(tri, faces, eye, cam, cull=cull)
            assert np.array_equal(r['id'] == 0, inside) and np.array_equal(r['id'] == -1, ~inside)
            assert (r['depth'][inside] == np.float32(2.0)).all() and not r['depth'][~inside].any()
            # grey 0.7 and the face normal (0, 0, +-1): shade = 0.35 + 0.65 / |d|
            d = np.sqrt(((ii - 5) / 10) ** 2 + ((jj - 4) / 10) ** 2 + 1.0)[inside]                  # |((i - cx) / fx, ., -1)|
            want = np.floor(255 * 0.7 * (0.35 + 0.65 / d) + 0.5).astype(np.uint8)
            assert np.array_equal(r['rgb'][inside], np.repeat(want[:, None], 3, 1)) and (r['rgb'][~inside] == 255).all()
        assert (Y.raster(tri, faces, eye, cam, cull=drop)['id'] == -1).all()
    a, b, c = tri
    assert np.dot(a, np.cross(b, c)) < 0 and np.dot(np.cross(b - a, c - a), a) < 0      # det of the counter-clockwise winding


def test_yardstick_vertex_normals_by_hand():
    # two triangles that share the edge (0, 1): one in the plane z = 0, one in the plane y = 0; vertex 4 is unused
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [5, 5, 5.0]])
    f = np.array([[0, 1, 2], [0, 3, 1], [0, 1, 9]])                         # the last face is out of range
    n = Y.vertex_normals(v, f)
    n1 = np.cross(v[1] - v[0], v[2] - v[0])
    n2 = np.cross(v[3] - v[0], v[1] - v[0])
    assert np.array_equal(n1, [0, 0, 1]) and np.array_equal(n2, [0, 1, 0])
    s = 1 / math.sqrt(2)
    assert np.allclose(n[0], [0, s, s], atol=1e-15) and np.allclose(n[1], [0, s, s], atol=1e-15)
    assert np.array_equal(n[2], [0, 0, 1]) and np.array_equal(n[3], [0, 1, 0]) and not n[4].any()
    # opposite faces cancel to an exact zero, which stays zero
    f2 = np.array([[0, 1, 2], [0, 2, 1]])
    assert not Y.vertex_normals(v, f2).any()


def test_yardstick_point_square_by_hand():
    cam = dict(H=9, W=11, fx=10.0, fy=10.0, cx=5.0, cy=4.0)
    # depth 4, u = 5 + 10 * 1.3 / 4 = 8.25, w = 4 - 10 * (-0.5) / 4 = 5.25
    p, col = np.array([[1.3, -0.5, -4.0]]), np.array([[9, 8, 7]], np.uint8)
    eye = np.eye(4)[:3]
    r = Y.raster(np.zeros((0, 3)), np.zeros((0, 3), int), eye, cam, points=p, point_colors=col, point_size=4)
    want = np.zeros((9, 11), bool)
    want[4:8, 7:11] = True                                                  # first column ceil(6.25) = 7, first row ceil(3.25) = 4
    assert np.array_equal(r['id'] == -2, want) and (r['rgb'][want] == (9, 8, 7)).all() and (r['depth'][want] == 4).all()
    assert abs(r['point'] - 0.25) < 1e-12
    r = Y.raster(np.zeros((0, 3)), np.zeros((0, 3), int), eye, cam, points=p, point_colors=col, point_size=1)
    want[:] = False
    want[5, 8] = True                                                       # ceil(7.75) = 8, ceil(4.75) = 5
    assert np.array_equal(r['id'] == -2, want)
    # a face in front of the point hides it, the same face behind does not; at the very same depth the face wins
    for z, hidden in ((-3.0, True), (-5.0, False), (-4.0, True)):
        tri = np.array([[-9, -9, z], [9, -9, z], [0, 9, z]])
        r = Y.raster(tri, np.array([[0, 1, 2]]), eye, cam, cull=0, points=p, point_colors=col, point_size=1)
        assert (r['id'][5, 8] == 0) == hidden


# ---- viz.py ------------------------------------------------------------------------------------------------------------------
def test_camera_actor():
    from evennicer_slam_amd import viz
    pts, colour = viz.camera_actor(False, 0.3)
    assert pts.shape == (1200, 3) and colour == (255, 0, 0) and viz.camera_actor(True, 0.3)[1] == (0, 0, 0)
    corners = 0.3 * np.array([[0, 0, 0], [-1, -1, 1.5], [1, -1, 1.5], [1, 1, 1.5], [-1, 1, 1.5], [-0.5, 1, 1.5], [0.5, 1, 1.5],
                              [0, 1.2, 1.5]])
    lines = [[1, 2], [2, 3], [3, 4], [4, 1], [1, 3], [2, 4], [1, 0], [0, 2], [3, 0], [0, 4], [5, 7], [7, 6]]
    for s, (a, b) in enumerate(lines):
        seg = pts[100 * s:100 * s + 100]
        assert np.allclose(seg[0], corners[a], atol=1e-15) and np.allclose(seg[-1], corners[b], atol=1e-15)
        assert np.allclose(seg[50], corners[a] + (corners[b] - corners[a]) * 50 / 99, atol=1e-15)
    assert np.array_equal(viz.camera_actor()[0], viz.camera_actor(False, 0.005)[0])


def test_viewer_pose_is_the_reference_sequence():
    from evennicer_slam_amd import viz
    init = C.RC.rigid(37.0, (0.3, -1, 0.5), (0.4, -1.2, 2.5))
    keep = init.copy()
    got = viz.viewer_pose(init)
    assert np.array_equal(init, keep)                                       # the caller's array is left alone
    # draw_trajectory's operations, one by one
    pose = init.copy()
    pose[:3, 3] += 2 * (pose[:3, 2] / np.linalg.norm(pose[:3, 2]))
    pose[:3, 2] *= -1
    pose[:3, 1] *= -1
    extrinsic = np.linalg.inv(pose)
    # Open3D's extrinsic is world -> camera with x right, y down, z forward; ours looks down -z with y up
    ours = np.linalg.inv(got)
    assert np.allclose(np.diag([1.0, -1.0, -1.0, 1.0]) @ extrinsic, ours, atol=1e-14)
    assert np.allclose(got[:3, :3], init[:3, :3]) and np.allclose(got[:3, 3] - init[:3, 3], 2 * init[:3, 2], atol=1e-14)


def test_default_intrinsics():
    from evennicer_slam_amd import viz
    cam = viz.default_intrinsics()
    assert cam['H'] == 1080 and cam['W'] == 1920 and cam['cx'] == 959.5 and cam['cy'] == 539.5
    assert cam['fx'] == cam['fy'] and abs(cam['fx'] - 540 / math.tan(math.pi / 6)) < 1e-9
    assert abs(2 * math.degrees(math.atan(540 / cam['fy'])) - 60.0) < 1e-9
    small = viz.default_intrinsics(90, 160)
    assert small['cx'] == 79.5 and small['cy'] == 44.5 and abs(small['fy'] - 45 / math.tan(math.pi / 6)) < 1e-9
    assert viz.POINT_SIZE == 4 and viz.Z_FAR == 1000.0


def _poses(n, seed=0):
    rng = np.random.default_rng(seed)
    return np.stack([C.RC.rigid(rng.uniform(-30, 30), rng.normal(size=3), rng.normal(size=3)) for _ in range(n)])


def test_frontend_bookkeeping(tmp_path):
    from evennicer_slam_amd import viz
    est, gt = _poses(30, 1), _poses(30, 2)
    front = viz.SLAMFrontend(str(tmp_path), est[0], cam_scale=0.3, estimate_c2w_list=est, gt_c2w_list=gt, H=90, W=160)
    assert front.start() is front and front.join() is None
    assert front.cam == viz.default_intrinsics(90, 160) and front.z_near == 0.0 and front.z_far == 1000.0
    assert np.allclose(front.view_c2w, viz.viewer_pose(est[0]))
    before = est[3].copy()
    front.update_pose(1, est[3], gt=False)
    assert np.array_equal(est[3][:3, 2], -before[:3, 2]) and np.array_equal(est[3][:, [0, 1, 3]], before[:, [0, 1, 3]])
    front.update_pose(1, torch.from_numpy(gt[3]), gt=True)
    assert sorted(front.cameras) == [1, 100001]
    front.update_pose(1, est[4], gt=False)                                  # the same actor moves
    assert sorted(front.cameras) == [1, 100001] and np.array_equal(front.cameras[1][2], est[4])
    front.update_cam_trajectory(20, gt=False)
    front.update_cam_trajectory(10, gt=True)
    assert np.array_equal(front.traj_actor[0], est[1:20, :3, 3]) and front.traj_actor[1] == (255, 0, 0)
    assert np.array_equal(front.traj_actor_gt[0], gt[1:10, :3, 3]) and front.traj_actor_gt[1] == (0, 0, 0)
    pts, col = front.scene_points()
    assert pts.shape == (1200 + 1200 + 19 + 9, 3) and col.shape == pts.shape and col.dtype == np.uint8
    base = viz.camera_actor(False, 0.3)[0]
    assert np.allclose(pts[:1200], base @ est[4][:3, :3].T + est[4][:3, 3], atol=1e-14)
    assert (col[:1200] == (255, 0, 0)).all() and (col[1200:2400] == 0).all() and (col[2400:2419] == (255, 0, 0)).all()
    front.reset()
    assert front.cameras == {} and front.scene_points()[0].shape == (28, 3)
    assert not os.path.exists(tmp_path / 'tmp_rendering') and front.frame_idx == 0


def test_command_line_frame_walk(tmp_path, capsys):
    calls = []

    class Stub:
        def __init__(self, output, **kw):
            calls.append(('init', output, kw))

        def start(self):
            return self

        def join(self):
            calls.append(('join',))

        def update_mesh(self, path):
            calls.append(('mesh', os.path.basename(path)))

        def update_pose(self, index, pose, gt=False):
            calls.append(('pose', index, pose.copy(), gt))

        def update_cam_trajectory(self, i, gt):
            calls.append(('traj', i, gt))

        def render(self):
            calls.append(('render',))

    est, gt = _poses(15, 3), _poses(15, 4)
    cfg = C.write_run(tmp_path, est, gt, 11, 2.0, meshes=[('00000_mesh.ply', b''), ('00005_mesh.ply', b''), ('00012_mesh.ply', b'')])
    n = C.load_visualizer().main([cfg, '--save_rendering', '--vis_input_frame', '--height', '90', '--width', '160'], frontend=Stub)
    assert n == 12
    scaled = est.copy()
    scaled[:, :3, 3] /= 2.0
    kind, output, kw = calls[0]
    assert kind == 'init' and output == str(tmp_path) and kw['cam_scale'] == 0.3 and kw['save_rendering'] is True and kw['near'] == 0
    assert kw['H'] == 90 and kw['W'] == 160 and np.allclose(kw['init_pose'], scaled[0]) and np.allclose(kw['estimate_c2w_list'], scaled)
    want = []
    for i in range(12):
        want += [('mesh',)] if i in (0, 5) else []
        want += [('pose', False), ('pose', True)]
        want += [('traj', i, False), ('traj', i, True)] if i % 10 == 0 else []
        want += [('render',)]
    want += [('join',)]
    got = [(c[0], c[3]) if c[0] == 'pose' else ((c[0],) if c[0] == 'mesh' else c) for c in calls[1:]]
    assert got == want
    poses = [c for c in calls if c[0] == 'pose']
    assert all(c[1] == 1 for c in poses) and np.allclose(poses[6][2], scaled[3]) and np.allclose(poses[7][2][:3, 3], gt[3][:3, 3] / 2.0)
    out = capsys.readouterr().out
    assert 'ffmpeg' in out and 'vis_input_frame' in out and '00011.tar' in out
    calls.clear()
    C.load_visualizer().main([cfg, '--no_gt_traj'], frontend=Stub)
    assert not any(c[0] == 'pose' and c[3] for c in calls) and not any(c[0] == 'traj' and c[2] for c in calls)
    assert 'ffmpeg' not in capsys.readouterr().out
