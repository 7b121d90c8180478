"""iMAP mode, host side: the decoder's module tree, keys, size and seeded initialisation against the reference fixture
(tests/golden/tiny_imap.npz, tests/golden/make_golden_imap.py), the C entries and the configurations the renderer takes."""
import os
import re
import types

import numpy as np
import pytest
import torch

from tests.util import load

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IMAP_CFG = {'data': {'dim': 3}, 'model': {'c_dim': 32, 'pos_embedding_method': 'fourier'},
            'grid_len': {'coarse': 2, 'middle': 0.32, 'fine': 0.16, 'color': 0.16}, 'coarse': False}


def _model():
    import evennicer_slam_amd as E
    torch.manual_seed(int(load("tiny_imap")['seed']))
    return E.get_model(IMAP_CFG, nice=False)


def test_get_model_imap_tree_and_keys():
    fx = load("tiny_imap")
    m = _model()
    sd = m.state_dict()
    assert list(sd) == list(fx['sd_names'])
    for k, v in sd.items():
        assert tuple(v.shape) == tuple(fx['sd_shape_' + k]), k
    assert sum(p.numel() for p in m.parameters()) == 222747
    assert not hasattr(m, 'fc_c')
    names = [n for n, _ in m.named_modules() if n]
    assert names == ['embedder', 'pts_linears', 'pts_linears.0', 'pts_linears.1', 'pts_linears.2', 'pts_linears.3',
                     'output_linear']


def test_seeded_initialisation_is_bit_equal():
    """same seed, same draws in the same order: weights and B equal the reference's bit for bit (SHA-256 of the float32
    bytes), biases zero; the fixture's biases are those zeros plus its seeded perturbation."""
    from tests.imap_torch import fixture_decoder, sha256_of
    fx = load("tiny_imap")
    sd = _model().state_dict()
    digests = dict(zip(fx['sd_names'], fx['sd_sha256']))
    for k, v in sd.items():
        if k.endswith('bias'):
            assert not v.any(), k
        else:
            assert sha256_of(v) == str(digests[k]), k
    fixture_decoder(fx)           # rebuilds the perturbed decoder and checks every digest


def test_other_shapes_still_raise():
    from evennicer_slam_amd.decoder import MLP
    with pytest.raises(NotImplementedError):
        MLP(c_dim=0, hidden_size=128, n_blocks=4, skips=[], color=True)
    with pytest.raises(NotImplementedError):
        MLP(c_dim=0, hidden_size=256, n_blocks=4, skips=[2], color=True)
    with pytest.raises(NotImplementedError):
        MLP(c_dim=0, hidden_size=256, n_blocks=4, skips=[], color=True, pos_embedding_method='nerf')
    nice_color = MLP(name='color', c_dim=32, hidden_size=32, color=True)
    with pytest.raises(NotImplementedError):
        nice_color(torch.zeros(1, 3))


def test_imap_exports_in_header_and_binding():
    import evennicer_slam_amd as E
    header = open(os.path.join(ROOT, "include", "enslam_hip.h")).read()
    new = ('enslam_imap_packed_floats', 'enslam_imap_workspace_floats', 'enslam_imap_pack', 'enslam_imap_fwd',
           'enslam_imap_bwd', 'enslam_composite_density_fwd', 'enslam_composite_density_bwd')
    for n in new:
        assert re.search(r"\b" + n + r"\s*\(", header), n
        assert n in E._lib.EXPORTS, n
    assert E._lib.IMAP_PARAM_NAMES == tuple(k for k in _model().state_dict())


def test_imap_renderer_configuration_and_cpu_refusal():
    import evennicer_slam_amd as E
    fx = load("tiny_imap")
    cfg = {'rendering': {'lindisp': False, 'perturb': 0.0, 'N_samples': 32, 'N_surface': 0, 'N_importance': 12},
           'scale': 1, 'occupancy': False}
    bound = torch.from_numpy(fx['bound'])
    slam = types.SimpleNamespace(nice=False, bound=bound, H=48, W=64, fx=50., fy=50., cx=31.5, cy=23.5)
    r = E.Renderer(cfg, None, slam)
    m = _model()
    with pytest.raises(E.EnslamError):
        r.eval_points(torch.zeros(4, 3, dtype=torch.float64), m)
    with pytest.raises(E.EnslamError):
        r.render_batch_ray(None, m, torch.ones(2, 3), torch.zeros(2, 3), 'cpu', 'color', gt_depth=torch.ones(2))
    with pytest.raises(E.EnslamError):
        r.regulation(None, m, torch.ones(2, 3), torch.zeros(2, 3), torch.ones(2), 'cpu')
    with pytest.raises(NotImplementedError):
        r.render_batch_ray_rgbd_loss(None, m, torch.ones(2, 3), torch.zeros(2, 3), 'cpu', 'color', torch.ones(2),
                                     torch.ones(2, 3))
    assert not r.tracker_loss_ok(2, torch.ones(2))
    # iMAP decoder with occupancy compositing is not a configuration of the reference
    with pytest.raises(NotImplementedError):
        E.Renderer(dict(cfg, occupancy=True), None, slam)


def _fixture_params():
    from tests.imap_torch import NAMES, fixture_decoder
    named = dict(fixture_decoder(load("tiny_imap")).named_parameters())
    return [named[n].detach() for n in NAMES]


def test_float64_yardstick_reproduces_the_fixture():
    """mlp64 (the argument p . B in float32 in the kernel's order, the rest in float64) against the reference's float32
    eval_points: 7.5e-7 of the largest |raw|, so the fixture's own float32 rounding is all that separates them."""
    from tests.imap_torch import mlp64
    fx = load("tiny_imap")
    raw, margin = mlp64(torch.from_numpy(fx['ep_pts']), _fixture_params())
    ref = fx['ep_raw'].astype(np.float64)
    out = ref[:, 3] == 100
    assert out.sum() > 20 and (~out).sum() > 20
    got = raw.numpy()
    scale = np.abs(ref).max()
    assert np.abs(got[:, :3] - ref[:, :3]).max() <= 2e-6 * scale
    assert np.abs(got[~out, 3] - ref[~out, 3]).max() <= 2e-6 * scale
    assert margin.shape == (700,) and (margin >= 0).all() and np.median(margin.numpy()) > 1e-5


def test_float64_backward_equals_autograd():
    """grads64's explicit backward against float64 autograd of the restatement (mlp, with eval_points' bound mask) at the
    same float32 argument: the argument enters autograd as im_arg's value plus (p B - (p B).detach()), and mlp runs on it
    with an identity B, so the values are im_arg's and the gradient to p and B is float64's.  The points are float32
    values, so p32 = p there.  Scales are non-negative and bound every gradient."""
    from tests.imap_torch import NAMES, _outside, grads64, im_arg, mlp
    fx = load("tiny_imap")
    ps = _fixture_params()
    bound = torch.from_numpy(fx['bound'])
    g = torch.Generator().manual_seed(5)
    p = torch.cat([torch.from_numpy(fx['ep_pts']), (torch.rand(300, 3, generator=g, dtype=torch.float64) * 2 - 1) * 3])
    p = p.float().double()
    cot = torch.randn(p.shape[0], 4, generator=g, dtype=torch.float64)
    raw, d_pts, grads, scales, d_scale, raw_scale = grads64(p, ps, cot, bound)

    pa = p.clone().requires_grad_(True)
    pa64 = [q.double().clone().requires_grad_(True) for q in ps]
    lin = pa @ pa64[0]
    arg = im_arg(p, ps[0]).double() + (lin - lin.detach())
    r = mlp(arg, [torch.eye(93, dtype=torch.float64)] + pa64[1:])
    out = _outside(p, bound)
    assert out.any() and (~out).any()
    r = torch.cat([r[:, :3], torch.where(out, torch.full_like(r[:, 3], 100.), r[:, 3])[:, None]], 1)
    (r * cot).sum().backward()
    assert (r.detach() - raw).abs().max() <= 1e-12 * raw.abs().max()
    assert (d_pts - pa.grad).abs().max() <= 1e-12 * pa.grad.abs().max()
    for name, got, ref, s in zip(NAMES, grads, pa64, scales):
        assert got.shape == ref.shape and s.shape == ref.shape, name
        assert (got - ref.grad).abs().max() <= 1e-12 * ref.grad.abs().max(), name
        assert (s >= 0).all() and (got.abs() <= s * (1 + 1e-12)).all(), name
    assert (d_pts.abs() <= d_scale * (1 + 1e-12)).all() and (raw.abs() <= raw_scale * (1 + 1e-12)).all()
