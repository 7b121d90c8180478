"""CPU side of the visibility kernel: the float64 numpy yardstick (tests/visibility_numpy.py) against the reference fixture
(tests/golden/tiny_visibility.npz, written by the reference's own Mesher.point_masks and Mapper.keyframe_selection_overlap),
the ABI declarations, and SLAM.map's keyframe selection when no selection method is configured."""
import os
import re
import types

import numpy as np
import pytest
import torch

from tests import visibility_numpy as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def fx():
    return V.load_fixture()


def test_fixture_shares(fx):
    """What the fixture was built to contain: each class holds >= 5 % of the lattice, and the depth test costs `seen` >= 5 %."""
    n = int(np.prod(fx['lattice_spec'][:, 2]))
    plain = V.fixture_classes(fx, 'lattice', 'plain', n)
    depth = V.fixture_classes(fx, 'lattice', 'depth', n)
    shares = [float((plain == c).mean()) for c in (0, 1, 2)]
    print("lattice shares unseen / seen / forecast:", shares, "seen with the depth test:", float((depth == 1).mean()))
    assert min(shares) >= 0.05
    assert (plain == 1).mean() - (depth == 1).mean() >= 0.05
    assert n > 2 * int(fx['lattice_chunk'])                                  # the lattice spans several chunks
    assert (fx['depth'] == 0).any()


@pytest.mark.parametrize("name", ['lattice', 'scatter'])
@pytest.mark.parametrize("variant", ['plain', 'depth', 'all'])
def test_yardstick_reproduces_the_reference_masks(fx, name, variant):
    pts, chunk = V.fixture_points(fx, name)
    w2c, limit, depth = V.fixture_views(fx, variant)
    classes, _, near, _ = V.classify(pts, w2c, V.CAM, limit=limit, depth=depth, chunk=chunk)
    ref = V.fixture_classes(fx, name, variant, len(pts))
    differ = classes != ref
    print(f"{name} {variant}: excluded share {near.mean():.2e}, differing {int(differ.sum())}, of them excluded "
          f"{int((differ & near).sum())}")
    assert near.mean() <= 1e-3
    assert not (differ & ~near).any()


def test_yardstick_overlap_agrees_with_the_reference_selection(fx):
    w2c = V.world_to_camera(fx['c2w'])
    pts = fx['ov_points']
    assert pts.dtype == np.float32 and pts.shape == (fx['ov_rays_o'].shape[0] * 16, 3)
    _, counts, _, near_k = V.classify(pts, w2c, V.CAM, edge_seen=20, edge_forecast=20, z_eps=1e-5)
    print("overlap counts", counts.tolist(), "excluded per camera", near_k.sum(1).tolist())
    sure = [k for k in range(len(w2c)) if counts[k] - near_k[k].sum() > 0]
    maybe = [k for k in range(len(w2c)) if counts[k] + near_k[k].sum() > 0]
    assert set(sure) <= set(fx['ov_selected_all'].tolist()) <= set(maybe)
    assert set(fx['ov_selected_3'].tolist()) <= set(fx['ov_selected_all'].tolist()) and len(fx['ov_selected_3']) == 3


def test_bilinear_matches_grid_sample():
    import torch.nn.functional as F
    rng = np.random.default_rng(0)
    img = rng.random((48, 64)).astype(np.float32)
    u, v = rng.uniform(-3, 67, 500), rng.uniform(-3, 51, 500)
    g = torch.tensor(np.stack([u / 63 * 2 - 1, v / 47 * 2 - 1], 1)).reshape(1, 1, -1, 2)
    ref = F.grid_sample(torch.from_numpy(img).double().reshape(1, 1, 48, 64), g, padding_mode='zeros', align_corners=True)
    assert np.abs(V.bilinear_zero_padded(img, u, v) - ref.reshape(-1).numpy()).max() < 1e-12


def test_visibility_entries_are_declared():
    import evennicer_slam_amd as E
    header = open(os.path.join(ROOT, "include", "enslam_hip.h")).read()
    declared = set(re.findall(r"\b(enslam_[a-z_0-9]+)\s*\(", header))
    for name in ("enslam_visibility", "enslam_visibility_workspace"):
        assert name in declared and name in E._lib.EXPORTS


def test_visibility_refuses_cpu_tensors():
    import evennicer_slam_amd as E
    from evennicer_slam_amd import functional as EF
    with pytest.raises(E.EnslamError, match="HIP device"):
        EF.visibility(torch.zeros(4, 3), np.eye(4)[None], V.CAM)


def test_overlap_selection_needs_the_device():
    import evennicer_slam_amd as E
    from evennicer_slam_amd import mapper
    kf = [dict(est_c2w=torch.eye(4), depth=torch.ones(48, 64))]
    with pytest.raises(E.EnslamError, match="HIP device"):
        mapper.keyframe_selection_overlap(torch.zeros(48, 64, 3), torch.ones(48, 64), torch.eye(4), kf, 3, V.CAM, device='cpu')


@pytest.mark.parametrize("cfg_mapping", [{}, {'keyframe_selection_method': 'global'}])
def test_map_selection_is_unchanged_without_the_key(monkeypatch, cfg_mapping):
    """SLAM.map with no keyframe_selection_method (or 'global') picks what it picked before the overlap method existed: the
    three statements of the random selection, restated here, under the same numpy seed."""
    from evennicer_slam_amd import slam as S
    picked = {}

    class Stop(Exception):
        pass

    def fake_iteration(cfg, renderer, c, decoders, frames, cam, **kw):
        picked['keys'] = [f['key'] for f in frames]
        picked['fixed'] = [f['fixed'] for f in frames]
        raise Stop

    def no_overlap(*a, **k):
        raise AssertionError("overlap selection must not run")

    monkeypatch.setattr(S, 'MapperIteration', fake_iteration)
    monkeypatch.setattr(S, 'keyframe_selection_overlap', no_overlap)
    n_kf, window = 9, 5
    kfs = [dict(depth=torch.ones(2, 2), color=torch.ones(2, 2, 3), est_c2w=torch.eye(4)) for _ in range(n_kf)]
    me = types.SimpleNamespace(cfg=dict(mapping=dict(cfg_mapping, mapping_window_size=window, frustum_feature_selection=False,
                                                     lr_factor=1.0)),
                               keyframe_dict=kfs, renderer=None, shared_c=None, shared_decoders=None, cam=V.CAM,
                               static_shapes=None, device='cpu')
    for seed in (0, 1, 2):
        np.random.seed(seed)
        with pytest.raises(Stop):
            S.SLAM.map(me, 3, torch.ones(2, 2, 3), torch.ones(2, 2), torch.eye(4), 1)
        np.random.seed(seed)
        n_old = n_kf - 1
        pick = list(np.random.permutation(n_old)[:max(window - 2, 0)]) if n_old > 0 else []
        pick = sorted(set(int(p) for p in pick) | {n_kf - 1})
        assert picked['keys'] == pick + [-1]
        assert picked['fixed'] == [k == min(pick) for k in pick] + [False]


def test_map_rejects_an_unknown_selection_method():
    from evennicer_slam_amd import slam as S
    kfs = [dict(depth=torch.ones(2, 2), color=torch.ones(2, 2, 3), est_c2w=torch.eye(4)) for _ in range(3)]
    me = types.SimpleNamespace(cfg=dict(mapping=dict(keyframe_selection_method='nearest')), keyframe_dict=kfs)
    with pytest.raises(ValueError, match="keyframe_selection_method"):
        S.SLAM.map(me, 3, torch.ones(2, 2, 3), torch.ones(2, 2), torch.eye(4), 1)


def test_slam_get_mesh_passes_mesh_coarse_level(monkeypatch):
    from evennicer_slam_amd import mesher as MS
    from evennicer_slam_amd import slam as S
    seen = {}

    def fake_get_mesh(self, path, c, decoders, kfs, poses, idx, **kw):
        seen.update(kw)
        return None

    monkeypatch.setattr(MS.Mesher, 'get_mesh', fake_get_mesh)
    me = types.SimpleNamespace(cfg=dict(coarse=True, scale=1.0, occupancy=True, meshing=dict(mesh_coarse_level=True),
                                        mapping=dict(marching_cubes_bound=[[-1, 1]] * 3)),
                               renderer=None, bound=torch.zeros(3, 2), nice=True, verbose=False, shared_c=None, shared_decoders=None,
                               keyframe_dict=[], estimate_c2w_list=None, device='cpu', scale=1.0, **V.CAM)
    S.SLAM.get_mesh(me, 'x.ply')
    assert seen['show_forecast'] is True
    me.cfg['meshing'] = {}
    S.SLAM.get_mesh(me, 'x.ply')
    assert seen['show_forecast'] is False
