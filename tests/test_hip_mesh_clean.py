"""Mesh cleaning on the GPU (csrc/mesh_clean.hip, functional.mesh_components / mesh_clean, Mesher.get_mesh's device route)
against the host helpers of mesher.py (face_components, face_areas, filter_components, drop_unreferenced) -- the yardstick is
always the host, never a second GPU path."""
import ctypes

import numpy as np
import pytest
import torch

from tests import mc_numpy as M
from tests import mesh_cases as C
from tests.test_hip_mesher import _keyframe, _mesher_for, room0  # noqa: F401

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
REL = 1e-9          # the keep decisions are pinned only where no area is this close (relative) to what it is compared with


def _labels(faces, n_verts):
    from evennicer_slam_amd import functional as EF
    lab = EF.mesh_components(torch.from_numpy(np.ascontiguousarray(faces)).to(DEV), n_verts)
    torch.cuda.synchronize()
    assert lab.dtype == torch.int32 and tuple(lab.shape) == (len(faces),)
    return lab.cpu().numpy()


def _check_labels(faces, n_verts, want_components=None):
    got = _labels(faces, n_verts)
    want, n = C.host_labels(faces)
    assert got.shape == want.shape and np.array_equal(got, want)            # every face, face by face
    if want_components is not None:
        assert n == want_components
    return n


@pytest.fixture(scope="module")
def noise():
    return {key: C.noise_mesh(*key) for key in sorted(C.NOISE_COUNTS)}


# ---- 1. labels = host partition ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(C.hand_built()))
def test_labels_hand_built(name):
    faces, n_verts, want = C.hand_built()[name]
    assert _labels(faces, n_verts).tolist() == want
    _check_labels(faces, n_verts)


@pytest.mark.parametrize("key", sorted(C.NOISE_COUNTS))
def test_labels_noise_meshes_closed_and_after_the_mask_drop(noise, key):
    v, f, mask = noise[key]
    F, comps, F_masked, comps_masked = C.NOISE_COUNTS[key]
    assert len(f) == F
    _check_labels(f, len(v), comps)
    fm = C.mask_drop(f, mask)
    assert len(fm) == F_masked
    _check_labels(fm, len(v), comps_masked)


def test_labels_one_large_component_and_a_long_tube():
    v, f = M.marching_cubes(M.smooth_random_field(96, 7), 0.0, (0., 0., 0.), (0.1, 0.1, 0.1))
    assert len(f) > 50_000
    assert _check_labels(f, len(v)) == 1
    v, f = C.tube_mesh()
    assert len(f) > 20_000
    assert _check_labels(f, len(v)) == 1
    rev = np.ascontiguousarray(f[::-1])                 # the faces in reverse order: the root is the far end of every chain
    assert _check_labels(rev, len(v)) == 1


def _room0_mc(room0, resolution):
    """The marching-cubes output get_mesh cleans (device tensors), with the mesher and its keyframe."""
    from evennicer_slam_amd import functional as EF
    sc, model, grids, renderer = room0
    m = _mesher_for(sc, renderer, resolution)
    kf = _keyframe(sc)
    xyz = m.get_grid_uniform(resolution)['xyz']
    with torch.no_grad():
        vol = m.lattice_volume(grids, model, xyz, m.get_bound_from_frames([kf]), DEV)
        v, f = EF.marching_cubes(vol, m.level_set, [a[0] for a in xyz], [a[2] - a[1] for a in xyz])
    return m, kf, v, f


def test_labels_room0_256(room0):
    m, kf, v, f = _room0_mc(room0, 256)
    assert f.shape[0] > 1_000_000
    n = _check_labels(f.cpu().numpy(), int(v.shape[0]))
    print(f"room0 256^3: {f.shape[0]} faces, {v.shape[0]} vertices, {n} components")


# ---- 2. filter + compaction = host result, bit for bit ----------------------------------------------------------------------
def _host_clean(v, f, mask, min_area, largest_only):
    """(vertices, faces, vertex_index) through the host helpers, after asserting that no keep decision is a near-tie."""
    from evennicer_slam_amd import mesher as MS
    fm = C.mask_drop(f, mask) if mask is not None else f
    lab, n = MS.face_components(fm)
    if n:
        area = np.bincount(lab, weights=MS.face_areas(v, fm), minlength=n)
        if largest_only:
            top = np.sort(area)[::-1]
            assert n == 1 or (top[0] - top[1]) > REL * top[0], "the two largest areas are a near-tie"
        else:
            assert (np.abs(area - min_area) > REL * np.maximum(area, abs(min_area))).all(), "an area is a near-tie of the threshold"
    kept = MS.filter_components(v, fm, min_area, largest_only)
    used = np.zeros(len(v), bool)
    used[kept.reshape(-1)] = True
    hv, hf = MS.drop_unreferenced(v, kept)
    return hv, hf, np.nonzero(used)[0].astype(np.int32), n


def _gpu_clean(v, f, mask, min_area, largest_only):
    from evennicer_slam_amd import functional as EF
    stats = {}
    gv, gf, gi = EF.mesh_clean(torch.from_numpy(v).to(DEV), torch.from_numpy(f).to(DEV),
                               None if mask is None else torch.from_numpy(mask).to(DEV), min_area, largest_only, stats=stats)
    torch.cuda.synchronize()
    assert gv.dtype == torch.float64 and gf.dtype == torch.int32 and gi.dtype == torch.int32
    return gv.cpu().numpy(), gf.cpu().numpy(), gi.cpu().numpy(), stats['components']


def _same_clean(v, f, mask, min_area, largest_only):
    hv, hf, hi, hn = _host_clean(v, f, mask, min_area, largest_only)
    gv, gf, gi, gn = _gpu_clean(v, f, mask, min_area, largest_only)
    assert gn == hn
    assert gf.shape == hf.shape and np.array_equal(gf, hf)
    assert gv.shape == hv.shape and np.array_equal(gv.view(np.int64), hv.view(np.int64))
    assert np.array_equal(gi, hi)
    return len(hf)


@pytest.mark.parametrize("key", sorted(C.NOISE_COUNTS))
@pytest.mark.parametrize("masked", [False, True])
def test_clean_equals_the_host_on_noise_meshes(noise, key, masked):
    v, f, mask = noise[key]
    mask = mask if masked else None
    total = len(C.mask_drop(f, mask)) if masked else len(f)
    kept = {thr: _same_clean(v, f, mask, thr, False) for thr in (0.01, 0.05, 0.2)}
    print(f"noise {key} masked={masked}: {total} faces, kept by threshold {kept}")
    assert total > kept[0.01] > kept[0.05] >= kept[0.2]
    assert _same_clean(v, f, mask, 1e9, False) == 0                          # keeps nothing
    assert _same_clean(v, f, mask, 0.0, False) == total                      # keeps everything (every component has area)
    assert _same_clean(v, f, mask, -1.0, False) == total
    n_largest = _same_clean(v, f, mask, 0.2, True)                           # the threshold is ignored
    assert 0 < n_largest < total


def test_clean_hand_built_and_degenerate_inputs():
    from evennicer_slam_amd import functional as EF
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0], [5, 5, 5], [6, 5, 5], [5, 7, 5], [9, 9, 9]], np.float64)
    f = np.array([[0, 1, 2], [2, 1, 3], [4, 5, 6]], np.int32)              # a unit square (area 1) and a triangle (area 1)
    f2 = np.array([[0, 1, 2], [4, 5, 6], [2, 1, 3]], np.int32)
    assert _same_clean(v, f, None, 0.5, False) == 3
    assert _same_clean(v, f, None, 1.0 + 1e-6, False) == 0
    assert _same_clean(v, f, None, 1.0 - 1e-6, False) == 3
    v[6, 1] = 7.5                                                           # the triangle's area becomes 1.25
    assert _same_clean(v, f, None, 1.1, False) == 1
    assert _same_clean(v, f2, None, 0.0, True) == 1
    keep = np.zeros(8, bool)
    keep[3] = True                                                          # only the second face of the square has a kept vertex
    assert _same_clean(v, f, keep, 0.0, False) == 1
    assert _same_clean(v, f, np.zeros(8, bool), 0.0, False) == 0            # no face survives the mask drop
    # equal largest areas: the first component wins, as np.argmax's first maximum
    v[6, 1] = 7.0
    gv, gf, gi, _ = _gpu_clean(v, f2, None, 0.0, True)
    assert np.array_equal(gi, [0, 1, 2, 3]) and np.array_equal(gf, [[0, 1, 2], [2, 1, 3]])
    # no faces: empty arrays without a launch
    ev, ef, ei = EF.mesh_clean(torch.from_numpy(v).to(DEV), torch.zeros((0, 3), dtype=torch.int32, device=DEV))
    assert tuple(ev.shape) == (0, 3) and tuple(ef.shape) == (0, 3) and tuple(ei.shape) == (0,)
    # degenerate faces (area exactly zero): dropped by `area > 0`, as on the host
    vz = np.array([[0, 0, 0], [1, 0, 0], [2, 0, 0], [0, 1, 0]], np.float64)
    fz = np.array([[0, 1, 2], [0, 1, 3]], np.int32)                         # collinear face and a proper one, sharing an edge
    assert _same_clean(vz, fz, None, 0.0, False) == 2
    from evennicer_slam_amd import mesher as MS
    hv, hf = MS.drop_unreferenced(vz, MS.filter_components(vz, fz[:1], 0.0))     # area == threshold exactly: strict, nothing stays
    gv, gf, gi, _ = _gpu_clean(vz, fz[:1], None, 0.0, False)
    assert hf.shape == gf.shape == (0, 3) and hv.shape == gv.shape == (0, 3) and gi.shape == (0,)


# ---- 3. reproducible --------------------------------------------------------------------------------------------------------
def test_clean_and_labels_are_deterministic(noise):
    from evennicer_slam_amd import functional as EF
    v, f, mask = noise[(96, 1)]
    tv, tf, tm = torch.from_numpy(v).to(DEV), torch.from_numpy(f).to(DEV), torch.from_numpy(mask).to(DEV)
    la, lb = EF.mesh_components(tf, len(v)), EF.mesh_components(tf, len(v))
    assert torch.equal(la, lb)
    a = EF.mesh_clean(tv, tf, tm, 0.05, False)
    b = EF.mesh_clean(tv, tf, tm, 0.05, False)
    assert a[1].shape[0] > 1000
    assert torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
    assert a[0].view(torch.int64).equal(b[0].view(torch.int64))


# ---- 4. refusals ------------------------------------------------------------------------------------------------------------
def test_mesh_clean_abi_rejects_bad_arguments():
    import evennicer_slam_amd as E
    lib = E._lib.lib()
    nb = ctypes.c_int64()
    assert lib.enslam_mesh_clean_workspace(4, 2, ctypes.byref(nb)) == 0 and nb.value > 0
    ws = torch.empty(nb.value, dtype=torch.uint8, device=DEV)
    v = torch.zeros((4, 3), dtype=torch.float64, device=DEV)
    f = torch.tensor([[0, 1, 2], [2, 1, 3]], dtype=torch.int32, device=DEV)
    lab = torch.empty(2, dtype=torch.int32, device=DEV)
    cnt = torch.empty(3, dtype=torch.int32, device=DEV)
    p = lambda t: t.data_ptr()                                              # noqa: E731
    assert lib.enslam_mesh_components(None, 2, 4, p(ws), p(lab), None) == -1
    assert lib.enslam_mesh_components(p(f), 2, 4, None, p(lab), None) == -1
    assert lib.enslam_mesh_components(p(f), 2, 4, p(ws), None, None) == -1
    assert lib.enslam_mesh_components(p(f), -1, 4, p(ws), p(lab), None) == -1
    assert lib.enslam_mesh_components(p(f), 2, -4, p(ws), p(lab), None) == -1
    assert lib.enslam_mesh_components(p(f), (1 << 24) + 1, 4, p(ws), p(lab), None) == -3
    assert lib.enslam_mesh_clean_count(None, 4, p(f), 2, None, 0.0, 0, p(ws), p(cnt), None) == -1
    assert lib.enslam_mesh_clean_count(p(v), 4, None, 2, None, 0.0, 0, p(ws), p(cnt), None) == -1
    assert lib.enslam_mesh_clean_count(p(v), 4, p(f), 2, None, 0.0, 0, None, p(cnt), None) == -1
    assert lib.enslam_mesh_clean_count(p(v), 4, p(f), 2, None, 0.0, 0, p(ws), None, None) == -1
    assert lib.enslam_mesh_clean_count(p(v), 4, p(f), 2, None, float('nan'), 0, p(ws), p(cnt), None) == -1
    assert lib.enslam_mesh_clean_count(p(v), -4, p(f), 2, None, 0.0, 0, p(ws), p(cnt), None) == -1
    assert lib.enslam_mesh_clean_count(p(v), 4, p(f), (1 << 24) + 1, None, 0.0, 0, p(ws), p(cnt), None) == -3
    assert lib.enslam_mesh_clean_count(p(v), (1 << 26) + 1, p(f), 2, None, 0.0, 0, p(ws), p(cnt), None) == -3
    assert lib.enslam_mesh_clean_emit(p(v), 4, p(f), 2, None, 4, 2, p(v), p(f), None, None) == -1
    assert lib.enslam_mesh_clean_emit(p(v), 4, p(f), 2, p(ws), 4, 2, None, p(f), None, None) == -1
    assert lib.enslam_mesh_clean_emit(p(v), 4, p(f), 2, p(ws), 4, 2, p(v), None, None, None) == -1
    assert lib.enslam_mesh_clean_emit(p(v), 4, p(f), 2, p(ws), 5, 2, p(v), p(f), None, None) == -1      # more than there are
    assert lib.enslam_mesh_clean_emit(p(v), 4, p(f), 2, p(ws), -1, 2, p(v), p(f), None, None) == -1
    torch.cuda.synchronize()


def test_functional_argument_checks():
    from evennicer_slam_amd import EnslamError
    from evennicer_slam_amd import functional as EF
    v = torch.zeros((4, 3), dtype=torch.float64, device=DEV)
    f = torch.tensor([[0, 1, 2], [2, 1, 3]], dtype=torch.int32, device=DEV)
    for bad in (lambda: EF.mesh_components(f.cpu(), 4), lambda: EF.mesh_components(f.long(), 4),
                lambda: EF.mesh_components(f.reshape(-1), 4), lambda: EF.mesh_components(f, -1),
                lambda: EF.mesh_clean(v.cpu(), f), lambda: EF.mesh_clean(v, f.cpu()), lambda: EF.mesh_clean(v.float(), f),
                lambda: EF.mesh_clean(v[:, :2], f), lambda: EF.mesh_clean(v, f, torch.ones(3, dtype=torch.bool, device=DEV)),
                lambda: EF.mesh_clean(v, f, torch.ones(4, dtype=torch.bool)), lambda: EF.mesh_clean(v, f, torch.ones(4, device=DEV)),
                lambda: EF.mesh_clean(v, f, None, float('nan'))):
        with pytest.raises(EnslamError):
            bad()


# ---- 5. get_mesh unchanged --------------------------------------------------------------------------------------------------
def _both_routes(room0, tmp_path, monkeypatch, resolution, tag, show_forecast=False, **meshing):
    """get_mesh through the device route and through the host route: arrays and files bit-identical.  The inputs of the device
    cleaning are captured, and the near-tie condition is asserted on their host areas."""
    from evennicer_slam_amd import functional as EF
    from evennicer_slam_amd import mesher as MS
    sc, model, grids, renderer = room0
    kfs = [_keyframe(sc)]
    seen = {}
    real = EF.mesh_clean

    def spy(vertices, faces, vertex_keep=None, min_area=0.0, largest_only=False, stats=None):
        seen.update(v=vertices.cpu().numpy(), f=faces.cpu().numpy(), keep=vertex_keep.cpu().numpy().astype(bool),
                    min_area=min_area, largest_only=largest_only)
        return real(vertices, faces, vertex_keep, min_area, largest_only, stats=stats)

    monkeypatch.setattr(EF, 'mesh_clean', spy)
    out = {}
    for route in ('device', 'host'):
        m = _mesher_for(sc, renderer, resolution, **meshing)
        m.clean_on_host = route == 'host'
        path = str(tmp_path / f"{tag}_{route}.ply")
        res = m.get_mesh(path, grids, model, kfs, None, 0, device=DEV, show_forecast=show_forecast, clean_mesh=True)
        assert res is not None
        out[route] = res + (open(path, 'rb').read(), dict(m.timing))
        assert {'clean', 'clean_masks', 'clean_components'} <= set(m.timing)
    assert 'v' in seen                                                       # the device route did run the kernel
    hv, hf, _, n = _host_clean(seen['v'], seen['f'], seen['keep'], seen['min_area'], seen['largest_only'])   # asserts no near-tie
    (dv, df, dc, dply, dt), (gv, gf, gc, gply, gt) = out['device'], out['host']
    assert dv.dtype == gv.dtype == np.float64 and df.dtype == gf.dtype == np.int32 and dc.dtype == gc.dtype == np.uint8
    assert dv.shape == gv.shape and np.array_equal(dv.view(np.int64), gv.view(np.int64))
    assert df.shape == gf.shape and np.array_equal(df, gf)
    assert dc.shape == gc.shape and np.array_equal(dc, gc)
    assert dply == gply
    assert np.array_equal(df, hf) and len(dv) == len(hv)                     # and both equal the helpers on the captured input
    print(f"{tag}: {len(seen['f'])} faces in, {n} components after the mask drop, {len(df)} faces / {len(dv)} vertices out; "
          f"clean device {dt['clean']:.4f} s (components {dt['clean_components']:.4f}), host {gt['clean']:.4f} s "
          f"(components {gt['clean_components']:.4f})")
    return dv, df, dc


def test_get_mesh_routes_agree_room0_128(room0, tmp_path, monkeypatch):
    v, f, c = _both_routes(room0, tmp_path, monkeypatch, 128, 'r128')
    assert len(f) > 1000 and f.max() < len(v)
    v1, f1, _ = _both_routes(room0, tmp_path, monkeypatch, 128, 'r128_largest', get_largest_components=True)
    assert 0 < len(f1) <= len(f)
    v2, f2, c2 = _both_routes(room0, tmp_path, monkeypatch, 128, 'r128_forecast', show_forecast=True)
    assert len(f2) > 0 and (c2 == np.array([0, 255, 255], np.uint8)).all(axis=1).any()
    v3, f3, c3 = _both_routes(room0, tmp_path, monkeypatch, 128, 'r128_empty', remove_small_geometry_threshold=1e6)
    assert v3.shape == (0, 3) and f3.shape == (0, 3) and c3.shape == (0, 3)     # an empty mesh file, not an exception


def test_get_mesh_routes_agree_room0_256(room0, tmp_path, monkeypatch):
    torch.cuda.synchronize()
    v, f, c = _both_routes(room0, tmp_path, monkeypatch, 256, 'r256')
    assert len(f) > 100_000 and f.max() < len(v)
