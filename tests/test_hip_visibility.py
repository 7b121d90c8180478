"""The visibility kernel (csrc/visibility.hip) on the GPU: Mesher.point_masks against the reference's masks
(tests/golden/tiny_visibility.npz) and the float64 yardstick (tests/visibility_numpy.py), the overlap keyframe selection
against the reference's lists, determinism, chunking, edge sizes, the ABI's error paths, and get_mesh(show_forecast=True).

Exclusion rule for boolean comparisons (float32 comparisons may flip on a threshold): a point is left out when, in the
float64 yardstick, any tested quantity of any camera lies within 1e-5 (relative to W, H, 1000, the depth limit, 2.4, or 1 for
z) of its threshold; every other point must agree exactly, and at most 1e-3 of the points may be left out."""
import ctypes
import types

import numpy as np
import pytest
import torch

from tests import visibility_numpy as V

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


@pytest.fixture(scope="module")
def fx():
    return V.load_fixture()


def _mesher(depth_test=False, points_batch_size=500000):
    from evennicer_slam_amd.mesher import MESHING_DEFAULTS, Mesher
    slam = types.SimpleNamespace(renderer=None, bound=torch.zeros(3, 2), nice=True, verbose=False, **V.CAM)
    cfg = dict(coarse=True, scale=1.0, occupancy=True, meshing=dict(MESHING_DEFAULTS, depth_test=depth_test),
               mapping=dict(marching_cubes_bound=[[-1, 1], [-1, 1], [-1, 1]]))
    return Mesher(cfg, None, slam, points_batch_size=points_batch_size)


def _keyframes(fx):
    return [dict(est_c2w=torch.from_numpy(fx['c2w'][k]).to(DEV), depth=torch.from_numpy(fx['depth'][k]).to(DEV))
            for k in range(len(fx['c2w']))]


def _classes_of(masks):
    seen, forecast, unseen = masks
    assert not (seen & forecast).any() and np.array_equal(unseen, ~(seen | forecast))
    return np.where(seen, 1, np.where(forecast, 2, 0)).astype(np.uint8)


def _gpu_classes(fx, name, variant, mode):
    """classes of a point set of the fixture through the Mesher: explicit points (point_masks) or the lattice form"""
    v = V.VARIANTS[variant]
    pts, chunk = V.fixture_points(fx, name)
    m = _mesher(v['depth_test'], chunk)
    kfs, poses = _keyframes(fx), [torch.from_numpy(c) for c in fx['c2w']]
    if mode == 'points':
        return _classes_of(m.point_masks(pts.astype(np.float32), kfs, poses, int(fx['all_frames_idx']), DEV,
                                         get_mask_use_all_frames=v['all_frames']))
    axes = [torch.from_numpy(a).to(DEV) for a in V.axes_from_spec(fx['lattice_spec'])]
    views = m._views(kfs, poses, int(fx['all_frames_idx']), DEV, v['all_frames'])
    return m.point_classes(views, DEV, lattice=axes).cpu().numpy()


@pytest.mark.parametrize("name,mode", [('lattice', 'points'), ('lattice', 'lattice'), ('scatter', 'points')])
@pytest.mark.parametrize("variant", ['plain', 'depth', 'all'])
def test_masks_match_the_reference(fx, name, mode, variant):
    pts, chunk = V.fixture_points(fx, name)
    w2c, limit, depth = V.fixture_views(fx, variant)
    yard, _, near, _ = V.classify(pts, w2c, V.CAM, limit=limit, depth=depth, chunk=chunk)
    ref = V.fixture_classes(fx, name, variant, len(pts))
    got = _gpu_classes(fx, name, variant, mode)
    print(f"{name} {mode} {variant}: excluded share {near.mean():.3e}; kernel differs from the reference on "
          f"{int((got != ref).sum())} points ({int(((got != ref) & ~near).sum())} not excluded), from the float64 yardstick on "
          f"{int((got != yard).sum())} ({int(((got != yard) & ~near).sum())} not excluded)")
    assert near.mean() <= 1e-3
    assert np.array_equal(got[~near], ref[~near])
    assert np.array_equal(got[~near], yard[~near])


def test_limit_and_largest_sample_per_chunk_against_the_yardstick(fx):
    """One near-range camera, so that the depth limit (plain) and the largest depth sample of each chunk (depth test) decide
    classes inside the box -- in the eight-camera fixture other cameras cover most of what one camera's limit drops."""
    pts, _ = V.fixture_points(fx, 'lattice')
    chunk = 50000
    c2w = fx['c2w'][:1]
    img = (fx['depth'][5:6] - np.float32(1.6)).clip(0)            # an outward view's image (3.4 m walls) brought to ~1.8 m
    w2c = V.world_to_camera(c2w)
    kfs = [dict(est_c2w=torch.from_numpy(c2w[0]).to(DEV), depth=torch.from_numpy(img[0]).to(DEV))]
    for depth_test in (False, True):
        limit = None if depth_test else (img.reshape(1, -1).max(1) * np.float32(1.1)).astype(np.float32)
        yard, _, near, _ = V.classify(pts, w2c, V.CAM, limit=limit, depth=img if depth_test else None, chunk=chunk)
        got = _classes_of(_mesher(depth_test, chunk).point_masks(pts.astype(np.float32), kfs, None, 0, DEV))
        shares = [float((yard == c).mean()) for c in (0, 1, 2)]
        print(f"depth_test {depth_test}: shares {shares}, excluded {near.mean():.3e}, differing {int((got != yard).sum())}")
        assert near.mean() <= 1e-3 and min(shares) > 0.02
        assert np.array_equal(got[~near], yard[~near])
    # the largest sample really depends on the chunk: one chunk over everything gives other classes somewhere
    whole, _, near_w, _ = V.classify(pts, w2c, V.CAM, depth=img, chunk=None)
    got_w = _classes_of(_mesher(True, len(pts)).point_masks(pts.astype(np.float32), kfs, None, 0, DEV))
    assert np.array_equal(got_w[~near_w], whole[~near_w])
    print("points whose class depends on the chunking:", int((whole != yard).sum()))


def test_overlap_counts_and_selection(fx, monkeypatch):
    from evennicer_slam_amd import common, mapper
    kfs = _keyframes(fx)
    pts = torch.from_numpy(fx['ov_points']).to(DEV)
    counts = mapper.overlap_counts(pts, kfs, V.CAM)
    _, yard, _, near_k = V.classify(fx['ov_points'], V.world_to_camera(fx['c2w']), V.CAM, edge_seen=20, edge_forecast=20,
                                    z_eps=1e-5)
    print("overlap counts", counts.tolist(), "yardstick", yard.tolist(), "excluded per camera", near_k.sum(1).tolist())
    assert counts.dtype == np.int32 and counts.shape == (len(kfs),)
    assert (np.abs(counts.astype(np.int64) - yard) <= near_k.sum(1)).all()

    # the project's own point formation on the recorded rays gives the recorded points
    mine = mapper.ray_sample_points(*(torch.from_numpy(fx[k]).to(DEV) for k in ('ov_rays_o', 'ov_rays_d', 'ov_depth')), 16)
    assert np.abs(mine.cpu().numpy() - fx['ov_points']).max() <= 1e-6

    # the selection with the reference's pixel draw replayed: get_samples returns the rays the reference drew
    def replay(*a, **k):
        return tuple(torch.from_numpy(fx[n]).to(DEV) for n in ('ov_rays_o', 'ov_rays_d', 'ov_depth')) + (None,)

    monkeypatch.setattr(common, 'get_samples', replay)
    cur = torch.from_numpy(fx['ov_c2w']).to(DEV)
    img = torch.zeros(V.CAM['H'], V.CAM['W'], device=DEV)
    np.random.seed(int(fx['ov_numpy_seed']))
    sel_all = mapper.keyframe_selection_overlap(img[..., None].expand(-1, -1, 3), img, cur, kfs, len(kfs), V.CAM, device=DEV)
    np.random.seed(int(fx['ov_numpy_seed']))
    sel_3 = mapper.keyframe_selection_overlap(img[..., None].expand(-1, -1, 3), img, cur, kfs, 3, V.CAM, device=DEV)
    assert sorted(int(i) for i in sel_all) == fx['ov_selected_all'].tolist()
    assert [int(i) for i in sel_3] == fx['ov_selected_3'].tolist()
    assert mapper.keyframe_selection_overlap(img[..., None].expand(-1, -1, 3), img, cur, [], 3, V.CAM, device=DEV) == []


def test_overlap_selection_draws_its_own_pixels(fx):
    """Without the replay: the function draws pixels itself (torch's generator) and returns keyframe ids."""
    from evennicer_slam_amd import mapper
    kfs = _keyframes(fx)
    depth = torch.full((V.CAM['H'], V.CAM['W']), 1.7, device=DEV)
    color = torch.zeros(V.CAM['H'], V.CAM['W'], 3, device=DEV)
    sel = mapper.keyframe_selection_overlap(color, depth, torch.from_numpy(fx['ov_c2w']).to(DEV), kfs, 3, V.CAM, device=DEV)
    assert len(sel) == 3 and set(int(i) for i in sel) <= set(range(5))      # the outward views see none of it


def test_deterministic_chunk_free_and_lattice_equals_points(fx):
    from evennicer_slam_amd import functional as EF
    pts64, _ = V.fixture_points(fx, 'lattice')
    pts = torch.from_numpy(pts64.astype(np.float32)).to(DEV)
    axes = [torch.from_numpy(a).to(DEV) for a in V.axes_from_spec(fx['lattice_spec'])]
    for variant in ('plain', 'depth'):
        w2c, limit, depth = V.fixture_views(fx, variant)
        kw = dict(limit=None if limit is None else torch.from_numpy(limit).to(DEV),
                  depth=None if depth is None else torch.from_numpy(depth).to(DEV), want_counts=True)
        a, ca = EF.visibility(pts, w2c, V.CAM, **kw)
        b, cb = EF.visibility(pts, w2c, V.CAM, **kw)
        assert torch.equal(a, b) and torch.equal(ca, cb)                    # two calls: bitwise equal
        c, cc = EF.visibility(None, w2c, V.CAM, lattice=axes, **kw)
        assert torch.equal(a, c) and torch.equal(ca, cc)                    # lattice mode = explicit points
        # the counts do not stop the camera loop early; the classes are the same without them
        d, _ = EF.visibility(pts, w2c, V.CAM, **dict(kw, want_counts=False))
        assert torch.equal(a, d)
        assert int(ca.sum()) >= int((a == 1).sum()) > 0
    # depth_test False: the classes do not depend on the chunk size
    w2c, limit, _ = V.fixture_views(fx, 'plain')
    lim = torch.from_numpy(limit).to(DEV)
    whole, _ = EF.visibility(pts, w2c, V.CAM, limit=lim)
    for chunk in (1000, 65537):
        parts = [EF.visibility(pts[lo:lo + chunk], w2c, V.CAM, limit=lim)[0] for lo in range(0, len(pts), chunk)]
        assert torch.equal(torch.cat(parts), whole)
        lat = [EF.visibility(None, w2c, V.CAM, limit=lim, lattice=axes, first=lo, count=min(chunk, len(pts) - lo))[0]
               for lo in range(0, len(pts), chunk)]
        assert torch.equal(torch.cat(lat), whole)


@pytest.mark.parametrize("P", [0, 1, 63, 64, 65, 257, 1025])
def test_edge_sizes(fx, P):
    from evennicer_slam_amd import functional as EF
    pts64 = V.fixture_points(fx, 'scatter')[0][:P]
    pts = torch.from_numpy(pts64.astype(np.float32)).to(DEV).reshape(-1, 3)
    for variant in ('plain', 'depth'):
        w2c, limit, depth = V.fixture_views(fx, variant)
        cls, cnt = EF.visibility(pts, w2c, V.CAM, limit=None if limit is None else torch.from_numpy(limit).to(DEV),
                                 depth=None if depth is None else torch.from_numpy(depth).to(DEV), want_counts=True)
        yard, ycnt, near, near_k = V.classify(pts64, w2c, V.CAM, limit=limit, depth=depth)
        assert cls.shape == (P,) and cnt.shape == (len(w2c),)
        got = cls.cpu().numpy()
        assert np.array_equal(got[~near], yard[~near])
        assert (np.abs(cnt.cpu().numpy() - ycnt) <= near_k.sum(1)).all()


def test_no_cameras_and_a_point_at_a_camera_centre(fx):
    from evennicer_slam_amd import functional as EF
    pts = torch.from_numpy(fx['scatter'][:100]).to(DEV)
    cls, cnt = EF.visibility(pts, np.zeros((0, 3, 4)), V.CAM, want_counts=True)
    assert cls.shape == (100,) and not cls.any() and cnt.shape == (0,)
    seen, forecast, unseen = _mesher().point_masks(fx['scatter'][:100], [], None, 0, DEV)
    assert unseen.all() and not seen.any() and not forecast.any()
    # a point exactly at a camera centre (identity pose, the origin): cam = 0, z = z_eps > 0, so it is in front of nothing
    # -- unseen in both precisions, with and without the depth test, and no fault
    eye = np.eye(4)[None]
    origin = torch.zeros(1, 3, device=DEV)
    for dtype, eps in ((torch.float32, 1e-8), (torch.float64, 1e-5)):
        for depth in (None, torch.from_numpy(fx['depth'][:1]).to(DEV)):
            cls, cnt = EF.visibility(origin, eye, V.CAM, z_eps=eps, want_counts=True, dtype=dtype, depth=depth)
            assert cls.tolist() == [0] and cnt.tolist() == [0]
    # at the centre of a posed camera the float32 camera coordinates are rounding residue: any class, no fault
    centre = torch.from_numpy(fx['c2w'][0][:3, 3].copy()).reshape(1, 3).to(DEV)
    cls, _ = EF.visibility(centre, V.world_to_camera(fx['c2w'][:1]), V.CAM, depth=torch.from_numpy(fx['depth'][:1]).to(DEV))
    assert cls.tolist()[0] in (0, 1, 2)


def test_functional_argument_checks(fx):
    import evennicer_slam_amd as E
    from evennicer_slam_amd import functional as EF
    pts = torch.zeros(4, 3, device=DEV)
    w2c = V.world_to_camera(fx['c2w'])
    with pytest.raises(E.EnslamError, match="limit has 3 entries for 8 cameras"):
        EF.visibility(pts, w2c, V.CAM, limit=torch.ones(3, device=DEV))                     # mismatched K
    with pytest.raises(E.EnslamError, match="depth must be"):
        EF.visibility(pts, w2c, V.CAM, depth=torch.ones(3, 48, 64, device=DEV))             # mismatched K
    with pytest.raises(E.EnslamError, match="depth must be"):
        EF.visibility(pts, w2c, V.CAM, depth=torch.ones(8, 64, 48, device=DEV))
    with pytest.raises(E.EnslamError, match=r"\[P,3\]"):
        EF.visibility(torch.zeros(4, 2, device=DEV), w2c, V.CAM)
    with pytest.raises(E.EnslamError, match="w2c must be"):
        EF.visibility(pts, np.zeros((8, 4, 3)), V.CAM)
    with pytest.raises(E.EnslamError, match="either explicit points or a lattice"):
        EF.visibility(None, w2c, V.CAM)
    ax = [torch.linspace(0, 1, 4, device=DEV)] * 3
    with pytest.raises(E.EnslamError, match="leaves the 64 lattice points"):
        EF.visibility(None, w2c, V.CAM, lattice=ax, first=60, count=5)
    with pytest.raises(E.EnslamError, match="HIP device"):
        EF.visibility(pts.cpu(), w2c, V.CAM)
    with pytest.raises(E.EnslamError, match="float32 or float64"):
        EF.visibility(pts, w2c, V.CAM, dtype=torch.float16)


def test_abi_error_codes():
    """Every refusal of enslam_visibility returns its code before anything is launched."""
    import evennicer_slam_amd as E
    lib = E._lib.lib()
    nb = ctypes.c_int64()
    assert lib.enslam_visibility_workspace(4, None) == -1
    assert lib.enslam_visibility_workspace(-1, ctypes.byref(nb)) == -1
    assert lib.enslam_visibility_workspace(0, ctypes.byref(nb)) == 0 and nb.value >= 4
    assert lib.enslam_visibility_workspace(240, ctypes.byref(nb)) == 0 and nb.value >= 960
    pts = torch.zeros(8, 3, device=DEV)
    w2c = torch.zeros(2, 12, device=DEV)
    ax = torch.zeros(2, device=DEV)
    img = torch.ones(2, 48, 64, device=DEV)
    ws = torch.zeros(256, dtype=torch.uint8, device=DEV)
    cls = torch.zeros(8, dtype=torch.uint8, device=DEV)
    p, w, a, d, s, c = (t.data_ptr() for t in (pts, w2c, ax, img, ws, cls))

    def call(real64=0, n=8, points=p, ax=(None, None, None), dims=(0, 0, 0), first=0, K=2, w2c=w, fx=50.0, H=48, W=64,
             z_eps=1e-8, depth=None, wsp=None, classes=c):
        return lib.enslam_visibility(real64, n, points, ax[0], ax[1], ax[2], dims[0], dims[1], dims[2], first, K, w2c, fx, 50.0,
                                     31.5, 23.5, H, W, 0, -1000, z_eps, None, depth, wsp, classes, None, None)

    assert call() == 0
    assert call(real64=2) == -1
    assert call(n=-1) == -1
    assert call(K=-1) == -1
    assert call(w2c=None) == -1                                              # cameras announced, none given
    assert call(H=0) == -1 and call(W=-5) == -1
    assert call(fx=float('nan')) == -1 and call(z_eps=float('inf')) == -1
    assert call(depth=d, wsp=None) == -1                                     # the depth test needs the workspace
    assert call(depth=d, wsp=s, H=1) == -1
    assert call(points=None) == -1                                           # neither points nor a lattice
    assert call(points=None, ax=(a, a, None), dims=(2, 2, 2)) == -1
    assert call(points=None, ax=(a, a, a), dims=(2, 0, 2)) == -1
    assert call(points=None, ax=(a, a, a), dims=(2, 2, 2), first=-1) == -1
    assert call(points=None, ax=(a, a, a), dims=(2, 2, 2), first=1) == -1    # 1 + 8 points leave the 8-point lattice
    assert call(points=None, ax=(a, a, a), dims=(2, 2, 2)) == 0
    assert call(n=0, points=None) == 0 and call(K=0, w2c=None) == 0
    assert call(classes=None) == 0                                           # nothing asked for: nothing done
    torch.cuda.synchronize()


# ---- get_mesh(show_forecast=True) on the room0 scene of tests/test_hip_mesher.py -------------------------------------------
from tests.test_hip_mesher import _keyframe, _mesher_for, room0  # noqa: E402,F401


def test_get_mesh_show_forecast_on_room0(room0, tmp_path):
    from evennicer_slam_amd import functional as EF
    from evennicer_slam_amd import mesher as MS
    sc, model, grids, renderer = room0
    res = 96
    m = _mesher_for(sc, renderer, res)
    m.points_batch_size = 200000                                             # several chunks
    kfs = [_keyframe(sc)]
    xyz = m.get_grid_uniform(res)['xyz']
    with torch.no_grad():
        views = m._views(kfs, None, 0, DEV, False)
        vol, classes = m.forecast_volume(grids, model, xyz, views, DEV)
        ax = [torch.from_numpy(a.astype(np.float32)) for a in xyz]
        gx, gy, gz = torch.meshgrid(*ax, indexing='ij')
        p = torch.stack([gx, gy, gz], -1).reshape(-1, 3).to(DEV)
        cb = renderer._coarse_bound(model)
        fine = EF.eval_points(p, model, grids, 'fine', m.bound, apply_mask=True, coarse_bound=cb)[:, 3]
        coarse = EF.eval_points(p, model, grids, 'coarse', m.bound, apply_mask=True, coarse_bound=cb)[:, 3] + 0.2
    # the classes are point_masks' on the same points, and all three occur
    seen, forecast, unseen = m.point_masks(p, kfs, None, 0, DEV)
    cl = classes.cpu().numpy()
    assert np.array_equal(cl == 1, seen) and np.array_equal(cl == 2, forecast) and np.array_equal(cl == 0, unseen)
    print("room0 lattice shares seen / forecast / unseen:", seen.mean(), forecast.mean(), unseen.mean())
    assert seen.any() and forecast.any() and unseen.any()
    want = torch.where(classes == 1, fine, torch.where(classes == 2, coarse, torch.full_like(fine, -100.0)))
    assert torch.equal(vol.reshape(-1).view(torch.int32), want.view(torch.int32))           # bitwise

    for clean in (False, True):
        out = str(tmp_path / f"forecast_{int(clean)}.ply")
        res_mesh = m.get_mesh(out, grids, model, kfs, None, 0, device=DEV, show_forecast=True, clean_mesh=clean)
        assert res_mesh is not None
        verts, faces, colors = res_mesh
        assert len(faces) > 0 and faces.max() < len(verts) and colors.shape == (len(verts), 3)
        _, fc, _ = m.point_masks(verts * m.scale, kfs, None, 0, DEV)
        cyan = (colors == np.array([0, 255, 255], np.uint8)).all(axis=1)
        with torch.no_grad():
            col = EF.eval_points(torch.from_numpy(verts * m.scale).to(DEV).float(), model, grids, 'color', m.bound,
                                 apply_mask=True)[:, :3].cpu().numpy()
        natural = (np.clip(col, 0, 1) * 255).astype(np.uint8)
        assert fc.any() and np.array_equal(colors[fc], np.tile(np.array([0, 255, 255], np.uint8), (int(fc.sum()), 1)))
        assert np.array_equal(colors[~fc], natural[~fc])                    # every other vertex keeps the decoder's colour
        assert np.array_equal(cyan & ~fc, cyan & ~fc & (natural == [0, 255, 255]).all(axis=1))
        rv, rf, rc = MS.read_ply(out)
        assert np.array_equal(rv, verts.astype(np.float32)) and np.array_equal(rf, faces) and np.array_equal(rc, colors)
        if clean:                                                           # a face stays only with a vertex inside the hull
            hs = torch.from_numpy(m.get_bound_from_frames(kfs)).to(DEV)
            inside = MS.inside_halfspaces(torch.from_numpy(verts * m.scale).to(DEV), hs).cpu().numpy()
            assert inside[faces].any(axis=1).all()


def test_harness_completes_with_overlap_selection(monkeypatch):
    """tools/run_synthetic_slam.py with its overlap switch: the 30-frame analytic sequence runs to its checkpoint and ATE with
    mapping.keyframe_selection_method 'overlap', and the selection really goes through mapper.keyframe_selection_overlap.
    ATE-RMSE measured in five such runs on one MI355X: 0.6 / 0.8 / 2.2 / 3.1 / 4.5 cm; the `global` schedule's band is
    0.6-2.6 cm over 30 runs (tests/test_hip_harness.py).  A record, not a bar: the selection changes the mapping window and both
    random streams, and the runs are not bit-reproducible.  Asserted: completion with a finite ATE, and the selections made."""
    import importlib.util
    import os
    from evennicer_slam_amd import slam as S
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("run_synthetic_slam", os.path.join(root, "tools", "run_synthetic_slam.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    calls = []
    inner = S.keyframe_selection_overlap

    def counting(gt_color, gt_depth, c2w, keyframe_dict, k, cam, **kw):
        sel = inner(gt_color, gt_depth, c2w, keyframe_dict, k, cam, **kw)
        calls.append((len(keyframe_dict), [int(i) for i in sel]))
        return sel

    monkeypatch.setattr(S, 'keyframe_selection_overlap', counting)
    monkeypatch.setenv('SKIP_BASE', '1')
    out = tool.run(30, verbose=False, overlap=True)
    ate = float(out['tracked']['ate'])
    print("overlap harness: ATE-RMSE", ate, "selections", calls)
    assert calls and all(len(sel) <= 3 and all(0 <= i < n for i in sel) for n, sel in calls)
    assert any(sel for _, sel in calls)                                     # some keyframe did overlap the current frame
    assert np.isfinite(ate)
