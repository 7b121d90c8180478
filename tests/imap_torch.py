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
    # the last interval is 1e10 (the reference expands 1e10 to dists[..., :1].shape, which is empty for one sample)
    dists = torch.cat([dists, dists.new_full(dists.shape[:-1] + (1,), 1e10)], -1)
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


# ------------------------------------------------------------------------------------------------ float64 yardstick
def im_arg(p, B):
    """the Fourier argument p . B as the kernel forms it (csrc/imap_mlp.hip im_arg): float32, the three products summed
    left to right, no fused multiply-add.  p [P,3], B [3,93]; returns float32 [P,93]."""
    p, B = p.float(), B.float()
    return (p[:, 0:1] * B[0] + p[:, 1:2] * B[1]) + p[:, 2:3] * B[2]


def _outside(p, bound):
    """points that Renderer.eval_points / eval_points above give sigma = 100 (compared in the points' precision)"""
    b = bound.to(p.device)
    inside = torch.ones(p.shape[0], dtype=torch.bool, device=p.device)
    for a in range(3):
        inside &= (p[:, a] < b[a, 1]) & (p[:, a] > b[a, 0])
    return ~inside


def _forward64(p, params):
    arg = im_arg(p, params[0]).double()
    h = torch.sin(arg)
    ins, dens, zs = [], [h.abs()], []
    margin = torch.full((p.shape[0],), float('inf'), dtype=torch.float64, device=p.device)
    for i in range(4):
        W, b = params[1 + 2 * i].double(), params[2 + 2 * i].double()
        z = h @ W.T + b
        den = h.abs() @ W.abs().T + b.abs()
        rel = torch.where(den > 0, z.abs() / den.clamp_min(1e-300), torch.full_like(z, float('inf')))
        margin = torch.minimum(margin, rel.min(1).values)
        ins.append(h)
        zs.append(z)
        h = torch.relu(z)
        dens.append(den * (z > 0))
    raw = h @ params[9].double().T + params[10].double()
    raw_scale = h.abs() @ params[9].double().abs().T + params[10].double().abs()
    return raw, margin, arg, ins, dens, zs, h, raw_scale


def mlp64(p, params):
    """(raw float64 [P,4], margin float64 [P]) of the iMAP decoder.  The argument p . B is formed in float32 exactly as
    the kernel forms it (im_arg); sin, the four ReLU linears and the output linear run in float64.  margin is the
    relative ReLU margin per point: the minimum over all 1024 pre-activations z = W h + b of |z| / (|W||h| + |b|).
    Where it is well above float32 rounding (~1e-6), a float32 evaluation of the point takes relu's branches as this
    one does."""
    raw, margin = _forward64(p, params)[:2]
    return raw, margin


def grads64(p, params, cot, bound=None):
    """An explicit float64 backward of eval_points (bound given) or mlp (bound None) at cotangent cot [P,4]; the argument
    is im_arg's float32 value, its gradient flows to p and B as in float64 (dB = p32^T dz, dp = dz B^T).

    Returns (raw, d_pts, grads, scales, d_pts_scale, raw_scale): raw [P,4] (sigma = 100 outside the bound), d_pts [P,3],
    the 11 parameter gradients in NAMES order, and for each one the scale of a float32 evaluation's rounding error: the
    same sum taken over the absolute values of its terms, where each factor is itself replaced by the abs-sum of the sum
    that formed it (|h_l| by [z_l > 0] (|W_l||h_{l-1}| + |b_l|), dPre_l by [z_l > 0] |dPre_{l+1}||W_{l+1}|, dz by
    |dPre_0||W_0||cos|).  So: Gd_l^T Hd_l for W_l, sum Gd_l for b_l, |p|^T Gz for B, Gz |B|^T for d_pts, |Wo||h_4| +
    |bo| for raw.  A plain |dPre_l|^T |in_l| does not bound the error: a ReLU output a little above its margin is the
    small difference of large terms and carries a few percent of error of its own."""
    raw, _, arg, ins, dens, zs, h4, raw_scale = _forward64(p, params)
    g = cot.double().clone()
    if bound is not None:
        out = _outside(p, bound)
        raw, raw_scale = raw.clone(), raw_scale.clone()
        raw[out, 3] = 100.
        raw_scale[out, 3] = 100.
        g[out, 3] = 0.
    W = [params[1 + 2 * i].double() for i in range(4)]
    Wo, B = params[9].double(), params[0].double()
    grads, scales = [None] * 11, [None] * 11
    grads[9], scales[9] = g.T @ h4, g.abs().T @ dens[4]
    grads[10], scales[10] = g.sum(0), g.abs().sum(0)
    dpre, gd = (g @ Wo) * (zs[3] > 0), (g.abs() @ Wo.abs()) * (zs[3] > 0)
    for i in range(3, -1, -1):
        grads[1 + 2 * i], scales[1 + 2 * i] = dpre.T @ ins[i], gd.T @ dens[i]
        grads[2 + 2 * i], scales[2 + 2 * i] = dpre.sum(0), gd.sum(0)
        d_in, a_in = dpre @ W[i], dpre.abs() @ W[i].abs()
        dpre, gd = (d_in * (zs[i - 1] > 0), a_in * (zs[i - 1] > 0)) if i > 0 else (d_in, a_in)
    c = torch.cos(arg)
    dz, gz = dpre * c, gd * c.abs()
    p32 = p.float().double()
    grads[0], scales[0] = p32.T @ dz, p32.abs().T @ gz
    return raw, dz @ B.T, grads, scales, gz @ B.abs().T, raw_scale
