"""The scene rasteriser on the GPU (csrc/scene_raster.hip, functional.scene_raster / vertex_normals) and the headless visualiser
built on it (evennicer_slam_amd/viz.py, tools/visualizer.py) against the float64 numpy yardstick of tests/viz_numpy.py at the
seeded cases of tests/viz_cases.py, whose margins tests/test_viz_cpu.py pins: every pixel is compared, none is excused."""
import numpy as np
import pytest
import torch

from tests import recon_edge_cases as E
from tests import viz_cases as C
from tests import viz_numpy as Y

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def dev(a, dtype=torch.float64):
    return None if a is None else torch.from_numpy(np.array(a)).to(DEV, dtype)         # a copy: the shared arrays are read-only


def _raster(args, views=None, cam=C.CAM, **over):
    """(rgb, depth, id) as numpy arrays of functional.scene_raster at a case's arguments"""
    from evennicer_slam_amd import functional as EF
    a = dict(args, **over)
    w2c = np.array(a.pop('views') if views is None else views)           # a copy: the shared arrays are read-only
    a.pop('views', None)
    v, f = dev(a.pop('vertices')), dev(a.pop('faces'), torch.int32)
    kw = dict(colors=dev(a.pop('colors', None), torch.uint8), normals=dev(a.pop('normals', None)),
              points=dev(a.pop('points', None)), point_colors=dev(a.pop('point_colors', None), torch.uint8))
    rgb, depth, ids = EF.scene_raster(v, f, w2c, cam, want_depth=True, want_id=True, **kw, **a)
    torch.cuda.synchronize()
    n = len(w2c)
    assert rgb.dtype == torch.uint8 and tuple(rgb.shape) == (n, cam['H'], cam['W'], 3)
    assert depth.dtype == torch.float32 and ids.dtype == torch.int32 and tuple(depth.shape) == tuple(ids.shape) == (n, cam['H'], cam['W'])
    return rgb.cpu().numpy(), depth.cpu().numpy(), ids.cpu().numpy()


def _check(got, want, what):
    rgb, depth, ids = got
    for k, r in enumerate(want):
        w64 = r['depth'].astype(np.float64)
        err = np.abs(depth[k].astype(np.float64) - w64)
        print(f"{what} view {k}: hit {np.mean(r['id'] != -1):.3f}, points {np.mean(r['id'] < -1):.3f}, id mismatches "
              f"{int((ids[k] != r['id']).sum())}, max err / depth {(err / np.maximum(w64, 1e-300)).max():.3e}, rgb mismatches "
              f"{int((rgb[k] != r['rgb']).any(-1).sum())}, margins edge {r['edge']:.2e} gap {r['gap']:.2e} round {r['round']:.2e} "
              f"point {r['point']:.2e}")
    for k, r in enumerate(want):
        assert np.array_equal(ids[k], r['id'])                              # the primitive at every pixel
        assert np.array_equal(depth[k] > 0, r['depth'] > 0)                 # hit / no hit at every pixel
        assert (np.abs(depth[k].astype(np.float64) - r['depth'].astype(np.float64)) <= 1.2e-7 * r['depth']).all()
        assert np.array_equal(rgb[k], r['rgb'])                             # the colour at every pixel


@pytest.fixture(scope="module")
def rendered():
    """name -> the (rgb, depth, id) of one K = 3 call; rendered once"""
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = _raster(C.case(name)[0])
        return cache[name]
    return get


@pytest.mark.parametrize("name", C.NAMES)
def test_scene_raster_matches_the_yardstick(rendered, name):
    C.check_margins(name)
    _check(rendered(name), C.case(name)[1], name)


@pytest.mark.parametrize("name", ['roombox_cull1', 'soup_points4'])
def test_vertex_normals_equal_the_yardstick_to_the_bit(name):
    from evennicer_slam_amd import functional as EF
    args = C.case(name)[0]
    got = EF.vertex_normals(dev(args['vertices']), dev(args['faces'], torch.int32))
    torch.cuda.synchronize()
    assert got.dtype == torch.float64 and tuple(got.shape) == args['vertices'].shape
    assert np.array_equal(got.cpu().numpy().view(np.uint64), np.ascontiguousarray(args['normals']).view(np.uint64))
    again = EF.vertex_normals(dev(args['vertices']), dev(args['faces'], torch.int32))
    assert torch.equal(got.view(torch.int64), again.view(torch.int64))


@pytest.mark.parametrize("name", ['roombox_cull1', 'soup_points4', 'soup_points1'])
def test_batching_and_reruns_do_not_change_a_bit(rendered, name):
    args = C.case(name)[0]
    whole = rendered(name)
    singles = [_raster(args, views=args['views'][k:k + 1]) for k in range(C.K)]
    again = _raster(args)
    for part in range(3):
        assert np.concatenate([s[part] for s in singles]).tobytes() == whole[part].tobytes()       # one K = 3 call == three K = 1 calls
        assert again[part].tobytes() == whole[part].tobytes()               # run to run


@pytest.mark.parametrize("name", ['roombox_cull1', 'soup_points4'])
def test_list_full_workspace_gives_the_same_images(rendered, name):
    from evennicer_slam_amd import functional as EF
    small = _raster(C.case(name)[0], workspace_bytes=C.tiny_workspace())
    for part in range(3):
        assert small[part].tobytes() == rendered(name)[part].tobytes()
    with pytest.raises(EF.L.EnslamError):                                   # no room for a single entry
        _raster(C.case(name)[0], workspace_bytes=C.tiny_workspace() - 8)


def test_empty_scenes_give_the_background():
    soup, pts = C.case('soup_points4')[0], C.case('points_only')[0]
    none = dict(vertices=soup['vertices'][:0], faces=soup['faces'][:0], views=soup['views'])
    for args, bg in ((none, (255, 255, 255)), (dict(none, background=(1, 2, 3)), (1, 2, 3)),
                     (dict(soup, faces=soup['faces'][:0], points=None, point_colors=None), (255, 255, 255)),
                     (dict(pts, points=pts['points'][:0], point_colors=pts['point_colors'][:0]), (255, 255, 255))):
        rgb, depth, ids = _raster(args)
        assert (rgb == np.array(bg, np.uint8)).all() and not depth.any() and (ids == -1).all()
    rgb, _, ids = _raster(soup, points=None, point_colors=None)             # a mesh and no points
    assert (ids >= -1).all() and (ids >= 0).any()


def test_bad_arguments_raise():
    from evennicer_slam_amd import functional as EF
    a = C.case('soup_points4')[0]
    v, f, w = dev(a['vertices']), dev(a['faces'], torch.int32), a['views']
    p, pc = dev(a['points']), dev(a['point_colors'], torch.uint8)
    bad_cam = dict(C.CAM, fx=float('nan'))
    for kw in (dict(z_near=2.0, z_far=1.0), dict(z_near=-1.0), dict(cull=3), dict(point_size=0), dict(ambient=1.5),
               dict(background=(0, 0, 256)), dict(points=p), dict(points=p, point_colors=pc[:5]),
               dict(colors=pc), dict(normals=v.float())):
        with pytest.raises(EF.L.EnslamError):
            EF.scene_raster(v, f, w, C.CAM, **kw)
    with pytest.raises(EF.L.EnslamError):
        EF.scene_raster(v, f, w, bad_cam)
    with pytest.raises(EF.L.EnslamError):
        EF.scene_raster(v, f, w, dict(C.CAM, fy=0.0))
    with pytest.raises(EF.L.EnslamError):
        EF.scene_raster(v.float(), f, w, C.CAM)
    with pytest.raises(EF.L.EnslamError):
        EF.scene_raster(v, f.long(), w, C.CAM)
    with pytest.raises(EF.L.EnslamError):
        EF.scene_raster(v, f, w[:, :2], C.CAM)
    with pytest.raises(EF.L.EnslamError):
        EF.vertex_normals(v.float(), f)


def test_depth_equals_mesh_depth_to_the_bit(rendered):
    from evennicer_slam_amd import functional as EF
    args = C.case('room_cull0_plain')[0]
    want = EF.mesh_depth(dev(args['vertices']), dev(args['faces'], torch.int32), args['views'], C.CAM, z_near=0.0, z_far=1000.0)
    torch.cuda.synchronize()
    assert (want > 0).all()
    assert np.array_equal(rendered('room_cull0_plain')[1].view(np.uint32), want.cpu().numpy().view(np.uint32))


@pytest.mark.parametrize("name", E.DEPTH_NAMES)
def test_exact_cases_equal_mesh_depth_and_the_exact_contract(name):
    """the exact cases of tests/recon_edge_cases.py (rays through vertices and along edges, t == z_far, degenerate triangles,
    the camera plane, both sides of the box split) through the renderer: its depth is mesh depth's and exact_depth's bit for
    bit, a pixel has no primitive exactly where its depth is 0, and a list of large triangles with room for one entry
    changes no byte"""
    from evennicer_slam_amd import functional as EF
    c = E.depth_cases()[name]
    args = dict(vertices=c['vertices'], faces=c['faces'], views=c['w2c'], cull=0, z_near=c['z_near'], z_far=c['z_far'])
    whole = _raster(args, cam=c['cam'])
    md = EF.mesh_depth(dev(c['vertices']), dev(c['faces'], torch.int32), np.array(c['w2c']), c['cam'], z_near=c['z_near'],
                       z_far=c['z_far'])
    torch.cuda.synchronize()
    got, md = whole[1].view(np.uint32), md.cpu().numpy().view(np.uint32)
    print(f"{name}: hit {int((c['want'] > 0).sum())} of {got.size}, differing from mesh depth {int((got != md).sum())}, from the "
          f"exact contract {int((got != c['want'].view(np.uint32)).sum())}")
    assert np.array_equal(got, md)
    assert np.array_equal(got, c['want'].view(np.uint32)) and np.array_equal(md, c['want'].view(np.uint32))
    assert np.array_equal(whole[2] == -1, got == 0) and (whole[2] >= -1).all()
    small = _raster(args, cam=c['cam'], workspace_bytes=C.tiny_workspace(len(c['w2c']), c['cam']))
    for part in range(3):
        assert small[part].tobytes() == whole[part].tobytes()


# ---- the tool, end to end ---------------------------------------------------------------------------------------------------------
REPLAY_EYES = (((0.6, 0.4, 0.1), (-1.0, -0.6, -0.3)), ((0.5, 0.3, 0.15), (-1.0, -0.7, -0.2)), ((0.4, 0.25, 0.2), (-1.0, -0.8, -0.1)))
REPLAY_SCALE = 2.0


def replay_run(folder):
    """a three-frame run in `folder`: estimated poses inside the box room that look away from the viewer's seat two units behind
    the first of them, ground truth beside them, the walls as frame 0's mesh and walls and box as frame 1's"""
    from evennicer_slam_amd.mesher import write_ply
    from evennicer_slam_amd.synthetic import look_at
    est = np.stack([look_at(e, t).numpy() for e, t in REPLAY_EYES]).astype(np.float64)
    gt = est.copy()
    gt[:, :3, 3] += np.array([0.05, -0.04, 0.03])
    est[:, :3, 3] *= REPLAY_SCALE                                           # the checkpoint holds scaled translations
    gt[:, :3, 3] *= REPLAY_SCALE
    cfg = C.write_run(folder, est, gt, 2, REPLAY_SCALE)
    for i, box in ((0, False), (1, True)):
        v, f, c = C.room_mesh(box=box)
        write_ply(str(folder / 'mesh' / f'{i:05d}_mesh.ply'), v, f, c)
    return cfg, est


def replay_middle_frame(folder, est, points, colours, cam):
    """the yardstick's image of the replay's middle frame: frame 1's mesh as the file holds it, the recorded actor points, the
    viewer two units behind the first pose"""
    from evennicer_slam_amd import viz
    from evennicer_slam_amd.eval_recon import load_mesh
    v, f, c = load_mesh(str(folder / 'mesh' / '00001_mesh.ply'))
    first = est[0].copy()
    first[:3, 3] /= REPLAY_SCALE
    w2c = np.linalg.inv(viz.viewer_pose(first))[:3]
    return Y.raster(v, f, w2c, cam, colors=c, normals=Y.vertex_normals(v, f), points=points, point_colors=colours, point_size=4,
                    cull=1, z_near=0.0, z_far=1000.0)


def test_visualizer_end_to_end(tmp_path):
    from PIL import Image
    from evennicer_slam_amd import viz
    cfg, est = replay_run(tmp_path)
    frames = []

    class Recording(viz.SLAMFrontend):
        def render(self):
            frame = super().render()
            frames.append((frame.clone(), self.scene_points()))
            return frame

    n = C.load_visualizer().main([cfg, '--save_rendering', '--height', '90', '--width', '160', '--device', DEV], frontend=Recording)
    torch.cuda.synchronize()
    assert n == 3 and len(frames) == 3
    for k in range(3):
        img = Image.open(tmp_path / 'tmp_rendering' / f'{k + 1:06d}.jpg')
        assert img.size == (160, 90) and np.asarray(img).shape == (90, 160, 3)
    assert len(list((tmp_path / 'tmp_rendering').iterdir())) == 3
    frame, (pts, col) = frames[1]
    assert frame.dtype == torch.uint8 and tuple(frame.shape) == (90, 160, 3) and frame.is_cuda and len(pts) == 2400
    want = replay_middle_frame(tmp_path, est, pts, col, viz.default_intrinsics(90, 160))
    for what, bound in C.MARGINS.items():
        assert want[what] > bound, f"the yardstick's own {what} margin is {want[what]:.3e}"
    assert (want['id'] >= 12).any() and (want['id'] < -1).any() and (want['id'] >= 0).mean() > 0.5     # box, actors, mostly mesh
    got = frame.cpu().numpy()
    print(f"middle frame: rgb mismatches {int((got != want['rgb']).any(-1).sum())} of {90 * 160}")
    assert np.array_equal(got, want['rgb'])
