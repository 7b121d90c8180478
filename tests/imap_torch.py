"""Torch restatement of the iMAP decoder and of density compositing, for the GPU tests and tools/bench_imap.py.

Written from the formulas (sin(p B), four ReLU linears 93->256->256->256->256, a linear 256->4; raw2outputs with volume
density): plain torch ops on whatever device the tensors live on, so on the GPU the linears run as hipBLASLt GEMMs."""
import torch
import torch.nn.functional as F

NAMES = ('embedder._B',) + tuple(f'pts_linears.{i}.{w}' for i in range(4) for w in ('weight', 'bias')) + \
    ('output_linear.weight', 'output_linear.bias')


def mlp(p, params):
    """raw [P,4] of points p [P,3]; params: the 11 tensors in NAMES order, float32 (the reference's precision) or
    float64 (an accuracy yardstick)."""
    B = params[0]
    h = torch.sin(p.to(B.dtype) @ B)
    for i in range(4):
        h = F.relu(F.linear(h, params[1 + 2 * i], params[2 + 2 * i]))
    return F.linear(h, params[9], params[10])


def eval_points(p, params, bound):
    raw = mlp(p, params)
    b = bound.to(p.device)
    inside = torch.ones(p.shape[0], dtype=torch.bool, device=p.device)
    for a in range(3):
        inside &= (p[:, a] < b[a, 1]) & (p[:, a] > b[a, 0])
    sigma = torch.where(inside, raw[:, 3], torch.full_like(raw[:, 3], 100.))
    return torch.cat([raw[:, :3], sigma[:, None]], 1)


def composite_density(raw, z, rays_d):
    """(depth, var, rgb, weights) with volume density (raw[..., 3] = sigma)."""
    dists = (z[..., 1:] - z[..., :-1]).float()
    dists = torch.cat([dists, torch.full_like(dists[..., :1], 1e10)], -1)
    dists = dists * torch.norm(rays_d[..., None, :], dim=-1)
    alpha = 1. - torch.exp(-F.relu(raw[..., 3]) * dists)
    T = torch.cumprod(torch.cat([torch.ones_like(alpha[:, :1]), 1. - alpha + 1e-10], -1), -1)[:, :-1]
    w = alpha * T
    rgb = (w[..., None] * raw[..., :3]).sum(-2)
    depth = (w * z).sum(-1)
    var = (w * (z - depth[:, None]) ** 2).sum(-1)
    return depth, var, rgb, w


def sha256_of(t):
    import hashlib
    return hashlib.sha256(t.detach().cpu().numpy().astype('<f4').tobytes()).hexdigest()


def fixture_decoder(fx):
    """The iMAP decoder of tests/golden/tiny_imap.npz, rebuilt on the CPU from the fixture's seeds (torch.manual_seed +
    get_model(nice=False), then the seeded bias perturbation of make_golden_imap.py); every tensor is checked against
    the fixture's SHA-256 digests, so the weights are the reference's bit for bit."""
    import evennicer_slam_amd as E
    cfg = {'data': {'dim': 3}, 'model': {'c_dim': 32, 'pos_embedding_method': 'fourier'}}
    torch.manual_seed(int(fx['seed']))
    model = E.get_model(cfg, nice=False)
    g = torch.Generator().manual_seed(int(fx['bias_seed']))
    with torch.no_grad():
        for name, p in model.named_parameters():
            if name.endswith('bias'):
                p.add_(torch.randn(p.shape, generator=g) * 0.05)
    sd = model.state_dict()
    assert list(sd) == list(fx['sd_names'])
    for (k, v), digest in zip(sd.items(), fx['sd_sha256']):
        assert sha256_of(v) == str(digest), k
    return model


def fixture_grad(fx, name, grad):
    """grad in the fixture's form: the [256, K] weights keep only the rows fx['grad_rows']"""
    if name.startswith('pts_linears.') and name.endswith('weight'):
        return grad[torch.as_tensor(fx['grad_rows']).to(grad.device)]
    return grad
