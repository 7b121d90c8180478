"""Reconstruction evaluation on the GPU: the exact nearest-neighbour kernels (csrc/nearest.hip, functional.nearest), the mesh
depth renderer (csrc/mesh_depth.hip, functional.mesh_depth) and the tools of evennicer_slam_amd/eval_recon.py built on them,
against the float64 numpy yardsticks of tests/recon_numpy.py -- never against a second GPU path."""
import numpy as np
import pytest
import torch

from tests import recon_cases as C
from tests import recon_numpy as Y

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ROUTES = (None, 0)          # max_rings: the default (cell grid, then the brute-force tail) and the brute-force kernel alone


def dev(a, dtype=torch.float64):
    return torch.from_numpy(np.array(a)).to(DEV, dtype)             # a copy: the shared yardstick arrays are read-only


# ---- nearest neighbour ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def nn_cases():
    """name -> (ref, query, yardstick dist, yardstick idx); computed once, never modified"""
    room = C.room()
    ref = room.sample_surface(5000, seed=11).numpy()
    qry = room.sample_surface(5003, seed=12).numpy()
    rng = np.random.default_rng(5)
    cases = {
        'one': (ref[:1], qry[:300]),
        'coincident': (np.repeat(ref[7:8], 1000, axis=0), qry[:300]),
        'odd': (ref[:257], qry[:1]),
        'room': (ref, qry),
        'shift1.5': (ref, qry + np.array([1.5, 0.0, 0.0])),
        'shift30': (ref, qry[:1000] + np.array([0.0, 30.0, 0.0])),
        'duplicated': (np.concatenate([ref, ref]), qry),
        'volume': (rng.normal(size=(3001, 3)), rng.normal(size=(1001, 3)) * 1.5),
    }
    out = {}
    for name, (r, q) in cases.items():
        d, i = Y.nearest(q, r)
        for a in (r, q, d, i):
            a.setflags(write=False)
        out[name] = (r, q, d, i)
    return out


NN_NAMES = ('one', 'coincident', 'odd', 'room', 'shift1.5', 'shift30', 'duplicated', 'volume')


def _nearest(q, r, **kw):
    from evennicer_slam_amd import functional as EF
    d, i = EF.nearest(dev(q), dev(r), **kw)
    torch.cuda.synchronize()
    assert d.dtype == torch.float64 and i.dtype == torch.int32 and tuple(d.shape) == tuple(i.shape) == (len(q),)
    return d.cpu().numpy(), i.cpu().numpy()


@pytest.mark.parametrize("max_rings", ROUTES)
@pytest.mark.parametrize("name", NN_NAMES)
def test_nearest_matches_brute_force(nn_cases, name, max_rings):
    r, q, want_d, want_i = nn_cases[name]
    stats = {}
    d, i = _nearest(q, r, max_rings=max_rings, stats=stats)
    err = np.abs(d - want_d) / np.maximum(want_d, 1e-300)
    print(f"{name} max_rings={max_rings}: max rel err {err.max():.3e}, tail {stats['tail']} of {len(q)}, "
          f"idx equal {np.array_equal(i, want_i)}, bit-equal {np.array_equal(d, want_d)}")
    assert (np.abs(d - want_d) <= 1e-12 * want_d).all()                     # no query excluded
    assert i.min() >= 0 and i.max() < len(r)
    again = np.sqrt(((q - r[i]) ** 2).sum(-1))
    assert (np.abs(again - d) <= 1e-12 * d).all()
    assert np.array_equal(i, want_i)                                        # ties to the smallest index, as argmin
    if max_rings == 0:
        assert stats['tail'] == len(q)
    elif name == 'shift30':
        assert stats['tail'] > 0                                            # the default route reaches the brute-force tail
    elif name == 'room':
        assert stats['tail'] < len(q) // 10                                 # ... and the shells finish the ordinary case


def test_nearest_duplicates_give_the_smaller_index_on_both_routes(nn_cases):
    r, q, _, _ = nn_cases['duplicated']
    _, i_grid = _nearest(q, r)
    _, i_brute = _nearest(q, r, max_rings=0)
    assert (i_grid < len(r) // 2).all() and np.array_equal(i_grid, i_brute)


@pytest.mark.parametrize("max_rings", ROUTES)
def test_nearest_max_dist(nn_cases, max_rings):
    r, q, want_d, want_i = nn_cases['shift1.5']
    d, i = _nearest(q, r, max_dist=0.05, max_rings=max_rings)
    far = want_d >= 0.05
    assert 0 < far.sum() < len(q)
    assert np.array_equal(i == -1, far) and np.isinf(d[far]).all()
    assert np.array_equal(i[~far], want_i[~far]) and (np.abs(d[~far] - want_d[~far]) <= 1e-12 * want_d[~far]).all()


def test_nearest_empty_and_invalid_inputs():
    from evennicer_slam_amd import functional as EF
    ref = dev(np.random.default_rng(0).normal(size=(10, 3)))
    for rings in ROUTES:
        d, i = EF.nearest(ref[:0], ref, max_rings=rings)
        assert tuple(d.shape) == (0,) and tuple(i.shape) == (0,) and d.dtype == torch.float64 and i.dtype == torch.int32
    with pytest.raises(EF.L.EnslamError):
        EF.nearest(ref, ref[:0])
    bad = ref.clone()
    bad[3, 1] = float('nan')
    with pytest.raises(EF.L.EnslamError, match="non-finite"):
        EF.nearest(ref, bad)
    with pytest.raises(EF.L.EnslamError, match="non-finite"):
        EF.nearest(bad, ref)
    with pytest.raises(EF.L.EnslamError):
        EF.nearest(ref.cpu(), ref)
    with pytest.raises(EF.L.EnslamError):
        EF.nearest(ref.float(), ref)


# ---- mesh depth -------------------------------------------------------------------------------------------------------------
def _w2c(c2w):
    return np.stack([np.linalg.inv(m)[:3] for m in np.asarray(c2w, np.float64).reshape(-1, 4, 4)])


def _depth(v, f, w2c, **kw):
    from evennicer_slam_amd import functional as EF
    d = EF.mesh_depth(dev(v), dev(f, torch.int32), w2c, C.CAM, **kw)
    torch.cuda.synchronize()
    assert d.dtype == torch.float32 and tuple(d.shape) == (len(w2c), C.CAM['H'], C.CAM['W'])
    return d.cpu().numpy()


def _check_depth(got, want, margin, what):
    assert margin.min() > 1e-9, f"{what}: the yardstick's own edge margin is {margin.min():.3e}"
    w32 = want.astype(np.float32)
    err = np.abs(got.astype(np.float64) - w32.astype(np.float64))
    print(f"{what}: hit {np.mean(want > 0):.3f}, margin {margin.min():.3e}, max err / depth "
          f"{(err / np.maximum(want, 1e-300)).max():.3e}, hit mismatches {int(((got > 0) != (want > 0)).sum())}")
    assert np.array_equal(got > 0, want > 0)                                # hit / no hit at every pixel
    assert (err <= 1.2e-7 * want).all()


@pytest.fixture(scope="module")
def room_views():
    room = C.room()
    v, f = C.box_room_mesh(room)
    poses = C.view_poses()
    cast = [Y.ray_cast(v, f, m, C.CAM) for m in poses]
    analytic = [room.render(torch.from_numpy(m), C.CAM)[1].numpy() for m in poses]
    return v, f, poses, cast, analytic


def test_mesh_depth_box_room_views(room_views):
    v, f, poses, cast, analytic = room_views
    w2c = _w2c(poses)
    got = _depth(v, f, w2c)
    for k in range(3):
        want, margin = cast[k]
        assert (want > 0).all()
        _check_depth(got[k], want, margin, f"room view {k}")
        assert np.abs(got[k].astype(np.float64) - analytic[k]).max() <= 5e-7
    singles = np.concatenate([_depth(v, f, w2c[k:k + 1]) for k in range(3)])
    assert np.array_equal(got.view(np.uint32), singles.view(np.uint32))     # one K = 3 call == three K = 1 calls, to the bit


@pytest.mark.parametrize("seed", [0, 1])
def test_mesh_depth_triangle_soup(seed):
    v, f = C.triangle_soup(seed)
    eye = np.eye(4)
    want, margin = Y.ray_cast(v, f, eye, C.CAM)
    z = v[f][:, :, 2]
    assert ((z.max(1) > 0) & (z.min(1) < 0)).sum() >= 8 and (z.min(1) > 0).sum() >= 24     # crossing the camera plane, behind it
    assert 0.5 < np.mean(want > 0) < 0.9                                    # background zeros and hits
    got = _depth(v, f, _w2c(eye))[0]
    _check_depth(got, want, margin, f"soup {seed}")
    assert np.array_equal(got.view(np.uint32), _depth(v, f, _w2c(eye))[0].view(np.uint32))         # run to run
    want1, margin1 = Y.ray_cast(v, f, eye, C.CAM, z_near=1.0)
    assert (want1 != want).any()
    _check_depth(_depth(v, f, _w2c(eye), z_near=1.0)[0], want1, margin1, f"soup {seed}, z_near = 1")


def test_mesh_depth_empty_mesh_and_bad_arguments():
    from evennicer_slam_amd import functional as EF
    v, f = C.box_room_mesh()
    w2c = _w2c(C.view_poses()[:2])
    got = _depth(v, f[:0], w2c)
    assert got.shape == (2, 48, 64) and not got.any()
    with pytest.raises(EF.L.EnslamError):
        EF.mesh_depth(dev(v), dev(f, torch.int32), w2c, C.CAM, z_near=2.0, z_far=1.0)
    with pytest.raises(EF.L.EnslamError):
        EF.mesh_depth(dev(v, torch.float32), dev(f, torch.int32), w2c, C.CAM)
    with pytest.raises(EF.L.EnslamError):
        EF.mesh_depth(dev(v), dev(f, torch.int64), w2c, C.CAM)
    # a face with an index outside the vertices is dropped, not read
    f_bad = np.concatenate([f, [[0, 1, 99]]]).astype(np.int32)
    assert np.array_equal(_depth(v, f_bad, w2c), _depth(v, f, w2c))


# ---- surface sampling -------------------------------------------------------------------------------------------------------
def test_sample_surface_on_the_device():
    from evennicer_slam_amd import eval_recon as R
    v, f = C.box_room_mesh()
    n = 200000
    pts, pick = R.sample_surface(dev(v), dev(f, torch.int64), n, seed=3)
    assert pts.is_cuda and pts.dtype == torch.float64 and tuple(pts.shape) == (n, 3)
    C.check_samples(v, f, pts.cpu().numpy(), pick.cpu().numpy(), n)
    again, _ = R.sample_surface(dev(v), dev(f, torch.int64), n, seed=3)
    other, _ = R.sample_surface(dev(v), dev(f, torch.int64), n, seed=4)
    assert torch.equal(pts, again) and not torch.equal(pts, other)


# ---- ICP --------------------------------------------------------------------------------------------------------------------
def test_icp_on_the_device_recovers_a_known_motion():
    from evennicer_slam_amd import eval_recon as R
    src, dst = C.icp_case()
    T, it, fit, rmse = R.align_icp(dev(src), dev(dst))
    Ty, ity, _, _ = Y.icp(src, dst)
    print(f"device ICP: {it} iterations, max |T - truth| {np.abs(T - C.ICP_TRUTH).max():.3e}; yardstick {ity}, "
          f"{np.abs(Ty - C.ICP_TRUTH).max():.3e}")
    assert np.abs(T - C.ICP_TRUTH).max() <= 1e-9
    assert it == ity
    assert np.abs(np.eye(4) - C.ICP_TRUTH).max() > 1e-3                     # a no-op would fail


def test_icp_on_the_device_matches_the_host_on_other_samples():
    from evennicer_slam_amd import eval_recon as R
    src, dst = C.icp_case(other_seed=2)
    T, it, _, _ = R.align_icp(dev(src), dev(dst))
    Ty, ity, _, _ = Y.icp(src, dst)
    print(f"device ICP: {it} iterations, max |T - yardstick| {np.abs(T - Ty).max():.3e}; yardstick {ity} iterations, "
          f"{np.abs(Ty - C.ICP_TRUTH).max():.3e} from the truth")
    assert np.abs(T - Ty).max() <= 1e-9


# ---- metrics end to end -----------------------------------------------------------------------------------------------------
def test_calc_3d_metric_device_and_host_routes_agree():
    from evennicer_slam_amd import eval_recon as R
    v, f = C.box_room_mesh()
    moved = v + np.array([0.02, 0.0, 0.0])
    m = R.calc_3d_metric((moved, f), (v, f), align=False, n=20000, device=DEV, return_points=True)
    rec, gt = m['rec_points'], m['gt_points']
    assert rec.is_cuda and gt.is_cuda
    rec_h, gt_h = rec.cpu().numpy(), gt.cpu().numpy()
    host = {'accuracy': R.accuracy(gt_h, rec_h) * 100, 'completion': R.completion(gt_h, rec_h) * 100,
            'completion_ratio': R.completion_ratio(gt_h, rec_h) * 100}
    for key, want in host.items():
        print(f"{key}: device {m[key]!r} host {want!r}")
        assert abs(m[key] - want) <= 1e-12 * abs(want)
    aligned = R.calc_3d_metric((moved, f), (v, f), align=True, device=DEV)
    assert aligned['completion_ratio'] == 100.0
    assert np.abs(aligned['transform'][:3, 3] - [-0.02, 0, 0]).max() <= 1e-9


def test_calc_2d_metric_of_a_scaled_mesh():
    from evennicer_slam_amd import eval_recon as R
    from evennicer_slam_amd import functional as EF
    v, f = C.box_room_mesh()
    c = C.VIEW_CENTRE
    transform = np.eye(4)
    transform[:3, 3] = c
    unseen = C.box_top_points()
    m = R.calc_2d_metric((c + 1.01 * (v - c), f), (v, f), unseen, np.zeros(3), transform, align=False, n_imgs=8,
                         seed=C.VIEW_SEED, cam=C.CAM, device=DEV)
    assert m['c2w'].shape == (8, 4, 4) and m['rejected'] >= 1
    for pose in m['c2w']:
        assert np.allclose(pose[:3, 3], c) and not Y.check_proj(unseen, C.CAM, pose).any()
    gt = EF.mesh_depth(dev(v), dev(f, torch.int32), EF.world_to_camera(list(m['c2w'])), C.CAM)
    assert bool((gt > 0).all())
    want = 0.01 * float(gt.double().mean()) * 100
    print(f"depth L1 {m['depth_l1']!r} cm, 0.01 * mean depth {want!r} cm")
    assert abs(m['depth_l1'] - want) <= 1e-6 * want


def test_cull_mesh_on_the_device_matches_the_reference_loop():
    from evennicer_slam_amd import eval_recon as R
    v, f = C.box_room_mesh()
    want = Y.cull_faces(v, f, C.CULL_POSES, C.CAM)
    got = R.cull_mesh(dev(v), f, C.CULL_POSES, C.CAM)
    assert 0 < len(want) < len(f) and np.array_equal(got, want)
