"""Cases, references and tolerance rules shared by tests/test_eventnet_bn_cpu.py and tests/test_hip_eventnet_bn.py: the
training-mode BatchNorm route of the event network (event.compile_event_net_batchnorm, enslam_eventnet_bn_* and
enslam_eventnet_train_*).

Kernel cases are seeded [M, C] matrices with the channels that break a careless kernel: mean 100 with standard deviation
1e-2 (E[x^2] - E[x]^2 loses it), a constant channel (var = 0, xh = 0) and a channel whose output is <= 0 everywhere
(dgamma = dbeta = 0 and g_z = 0 exactly).  Their tolerances are the derived bounds of tests/eventnet_bn_numpy.py.

Whole-net outputs and running statistics are compared with the float64 torch module in .train(); the tolerance is 8x the
recorded error of the float32 torch module on the CPU against that module (the rule of eventnet_cases.F32_ERR).

Whole-net gradients are NOT compared with the plain float64 module: training-mode BatchNorm centres every pre-activation,
units within rounding of 0 take the other ReLU branch in float32, and at the deep levels (4 to 12 values per channel) one
such unit moves a whole gradient tensor (float32 torch on the CPU is already 1e-2 to 1e-1 off on most cases).  The
reference is `statement`: the module's forward in float64 with each ReLU replaced by a supplied 0/1 mask and each max-pool
by a gather at a supplied index.  With the decisions given the function is smooth, and a float32 evaluation under the SAME
decisions must match to float32 rounding; the GPU test takes the decisions from the device's own saved activations."""
import copy
import functools

import numpy as np
import torch
import torch.nn.functional as F

from tests.eventnet_cases import make_net
from tests.eventnet_train_cases import kind_of, rel_max  # noqa: F401  (re-exported)

# ---------------------------------------------------------------------------------------------------------------------
# kernel cases
# ---------------------------------------------------------------------------------------------------------------------
ROWS = 256                                                   # the kernels' split size
KERNEL_M = (2, 3, 63, 64, 65, 255, 256, 257, 700)            # 255 / 256 / 257: the split size +- 1; 700: three splits
KERNEL_C = (8, 64, 1024, 24)                                 # 24: a multiple of 8 and not of 64
KERNEL_CASES = [(M, 64) for M in KERNEL_M] + [(M, C) for C in (8, 1024, 24) for M in (3, 257, 700)]
EPS = 1e-5
CH_OFFSET, CH_CONST, CH_DEAD = 0, 1, 2                       # the three special channels


@functools.lru_cache(maxsize=None)
def kernel_case(M, C, seed=0):
    """dict of float32 numpy arrays z [M, C], gamma, beta [C], g_y [M, C] (read-only)."""
    rng = np.random.default_rng(1234 + 7919 * seed + 31 * M + C)
    z = (rng.standard_normal((M, C)) * rng.uniform(0.5, 2.0, C) + rng.standard_normal(C)).astype(np.float32)
    z[:, CH_OFFSET] = (100.0 + 1e-2 * rng.standard_normal(M)).astype(np.float32)
    z[:, CH_CONST] = np.float32(3.25)
    gamma = rng.uniform(1.5, 2.5, C).astype(np.float32)
    beta = (0.1 * rng.standard_normal(C)).astype(np.float32)
    gamma[CH_DEAD], beta[CH_DEAD] = np.float32(0.1), np.float32(-10.0)       # 0.1 xh - 10 < 0: |xh| <= sqrt(M) < 100
    g_y = rng.standard_normal((M, C)).astype(np.float32)
    out = {'z': z, 'gamma': gamma, 'beta': beta, 'g_y': g_y}
    for a in out.values():
        a.setflags(write=False)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# whole-net cases
# ---------------------------------------------------------------------------------------------------------------------
NET_CASES = {
    '1x32x32': (1, 32, 32),             # no padding anywhere; 2 x 2 bottom, M = 4 there
    '2x16x70': (2, 16, 70),             # batch; centred padding at two levels on one axis; 1 x 4 bottom
    '1x35x37': (1, 35, 37),             # padding on both axes
    '3x16x32': (3, 16, 32),             # odd batch; M = 6 at the bottom
    '2x39x51': (2, 39, 51),             # the trainer's own small shape
}
NET_SEED = {'1x32x32': 0, '2x16x70': 0, '1x35x37': 1, '3x16x32': 0, '2x39x51': 0}
KINDS = ('conv', 'bn_gamma', 'bn_beta', 'heads', 'gx')
TOL_MARGIN = 8.0
ADMISSIBLE = 1.25e-4                    # a gradient record above this would put the tolerance above 1e-3

# Error of the float32 torch module in .train() on the CPU against the float64 module (max |difference| / max |float64|):
# events and probs after the first and the second step (the worse), and the worst of the 52 running buffers after each.
# Re-measured by test_eventnet_bn_cpu.py::test_recorded_float32_errors, which fails when a record is off by more than 4x.
F32_ERR_OUT = {
    '1x32x32': {'events': 3.89e-06, 'probs': 3.47e-06, 'buffers': 8.43e-07},
    '2x16x70': {'events': 3.82e-06, 'probs': 3.18e-06, 'buffers': 5.23e-07},
    '1x35x37': {'events': 4.41e-06, 'probs': 2.71e-06, 'buffers': 1.01e-06},
    '3x16x32': {'events': 5.33e-06, 'probs': 4.70e-06, 'buffers': 5.86e-07},
    '2x39x51': {'events': 3.33e-06, 'probs': 3.25e-06, 'buffers': 4.04e-07},
}
# Error of `statement` in float32 against float64, both under the float64 run's decisions, per parameter kind (the worst
# tensor of the kind, max |difference| / max |float64|).  Re-measured by the same test.
F32_ERR_GRAD = {
    '1x32x32': {'conv': 4.11e-05, 'bn_gamma': 2.55e-05, 'bn_beta': 1.95e-05, 'heads': 4.08e-06, 'gx': 1.34e-05},
    '2x16x70': {'conv': 1.19e-05, 'bn_gamma': 8.76e-06, 'bn_beta': 5.12e-06, 'heads': 5.08e-06, 'gx': 3.42e-06},
    '1x35x37': {'conv': 2.85e-05, 'bn_gamma': 1.77e-05, 'bn_beta': 1.64e-05, 'heads': 4.34e-06, 'gx': 1.39e-05},
    '3x16x32': {'conv': 3.38e-05, 'bn_gamma': 1.39e-05, 'bn_beta': 1.06e-05, 'heads': 3.15e-06, 'gx': 1.16e-05},
    '2x39x51': {'conv': 8.22e-06, 'bn_gamma': 6.48e-06, 'bn_beta': 3.49e-06, 'heads': 3.32e-06, 'gx': 3.00e-06},
}


def tolerance_out(case, quantity):
    return TOL_MARGIN * F32_ERR_OUT[case][quantity]


def tolerance_grad(case, kind):
    return TOL_MARGIN * F32_ERR_GRAD[case][kind]


def make_bn_net(case):
    """eventnet_cases.make_net (randomised BatchNorm) with every parameter requiring a gradient, in training mode."""
    net = copy.deepcopy(make_net(NET_SEED[case]))
    net.requires_grad_(True)
    return net.train()


def make_bn_inputs(case, step=0):
    """x in [0, 1] [B,6,H,W] and upstream gradients for both outputs (float32, CPU); `step` picks another batch."""
    B, H, W = NET_CASES[case]
    gen = torch.Generator().manual_seed(77 + NET_SEED[case] + 1000 * step)
    x = torch.rand(B, 6, H, W, generator=gen)
    return x, torch.randn(B, 2, H, W, generator=gen), torch.randn(B, 2, H, W, generator=gen)


def conv_bn_pairs(net):
    """[(conv, bn)] x 26 in packing order."""
    import evennicer_slam_amd as E
    return [(p.double_conv[i], p.double_conv[i + 1]) for p in E.event._conv_pairs(net) for i in (0, 3)]


def buffers_of(net):
    """The 52 running buffers in packing order as float64 numpy arrays."""
    return [t.detach().cpu().double().numpy().copy() for _, bn in conv_bn_pairs(net) for t in (bn.running_mean, bn.running_var)]


def run_module_train(net, case, dtype, steps=2):
    """The torch module in .train() on the CPU in `dtype`: per step (events, probs, buffers) as float64 numpy; the state of
    `net` is not touched."""
    m = copy.deepcopy(net).to(dtype).train()
    out = []
    with torch.no_grad():
        for s in range(steps):
            e, p = m(make_bn_inputs(case, s)[0].to(dtype))
            out.append((e.double().numpy(), p.double().numpy(), buffers_of(m)))
    return out


@functools.lru_cache(maxsize=None)
def reference_train(case):
    return run_module_train(make_bn_net(case), case, torch.float64)


def first_max_route(f):
    """[B,C,H//2,W//2] int64: the index (0..3, row-major) of the first maximum of each 2 x 2 window of f [B,C,H,W]."""
    Ho, Wo = f.shape[2] // 2, f.shape[3] // 2
    w = [f[:, :, ky:2 * Ho:2, kx:2 * Wo:2] for ky in (0, 1) for kx in (0, 1)]
    best, idx = w[0], torch.zeros_like(w[0], dtype=torch.int64)
    for k in (1, 2, 3):
        upd = w[k] > best
        idx = torch.where(upd, torch.full_like(idx, k), idx)
        best = torch.where(upd, w[k], best)
    return idx


def statement(net, x, dtype, decisions=None):
    """(events, probs, decisions) of the training-mode net in `dtype` on the CPU, differentiable: each ReLU is a multiplication
    with a 0/1 mask, each max-pool a gather.  decisions = (masks: 26 bool [B,C,H,W] in packing order, routes: 4 int64
    [B,C,H//2,W//2] for the pools of f0..f3); None: the run's own (mask = pre-activation > 0, route = first maximum), which
    are returned either way.  `net`'s parameters are used as they are (cast to `dtype` with a graph), its buffers not at all."""
    pairs = conv_bn_pairs(net)
    masks_in, routes_in = decisions if decisions is not None else (None, None)
    masks, routes = [], []

    def layer(i, t):
        conv, bn = pairs[i]
        z = F.conv2d(t, conv.weight.to(dtype), padding=1)
        mean = z.mean(dim=(0, 2, 3), keepdim=True)
        var = ((z - mean) ** 2).mean(dim=(0, 2, 3), keepdim=True)
        y = bn.weight.to(dtype)[None, :, None, None] * ((z - mean) / torch.sqrt(var + bn.eps)) + bn.bias.to(dtype)[None, :, None, None]
        mask = masks_in[i] if masks_in is not None else (y.detach() > 0)
        masks.append(mask)
        return y * mask.to(dtype)

    def pool(l, f):
        route = routes_in[l] if routes_in is not None else first_max_route(f.detach())
        routes.append(route)
        Ho, Wo = f.shape[2] // 2, f.shape[3] // 2
        w = torch.stack([f[:, :, ky:2 * Ho:2, kx:2 * Wo:2] for ky in (0, 1) for kx in (0, 1)], dim=-1)
        return torch.gather(w, -1, route[..., None])[..., 0]

    feats = [layer(1, layer(0, x.to(dtype)))]
    for l in range(1, 5):
        feats.append(layer(2 * l + 1, layer(2 * l, pool(l - 1, feats[-1]))))
    outs = []
    for h in range(2):
        t = feats[4]
        for j in range(4):
            skip = feats[3 - j]
            t = F.interpolate(t, scale_factor=2, mode='bilinear', align_corners=True)
            dy, dx = skip.shape[2] - t.shape[2], skip.shape[3] - t.shape[3]
            t = F.pad(t, [dx // 2, dx - dx // 2, dy // 2, dy - dy // 2])
            i0 = 10 + 8 * h + 2 * j
            t = layer(i0 + 1, layer(i0, torch.cat([skip, t], dim=1)))
        c = getattr(net, f'outc_{h + 1}').conv
        outs.append(F.conv2d(t, c.weight.to(dtype), c.bias.to(dtype)))
    # masks were appended in call order: encoder 0..9, then head 1's 10..17, head 2's 18..25 -- the packing order
    return outs[0], torch.sigmoid(outs[1]), (masks, routes)


def statement_grads(net, case, dtype, decisions=None):
    """({parameter name: gradient}, gx, decisions) of `statement` for the case's step-0 inputs, float64 numpy arrays."""
    m = copy.deepcopy(net).to(dtype)
    m.requires_grad_(True)
    x, g_events, g_probs = make_bn_inputs(case)
    xx = x.detach().to(dtype).clone().requires_grad_(True)
    e, p, dec = statement(m, xx, dtype, decisions)
    (e * g_events.to(dtype)).sum().add((p * g_probs.to(dtype)).sum()).backward()
    return {n: q.grad.detach().double().numpy() for n, q in m.named_parameters()}, xx.grad.detach().double().numpy(), dec


def errors_by_kind(grads, gx, ref, ref_gx):
    """{kind: (worst rel_max over the kind's tensors, the name of the tensor that set it)} with 'gx' for the input gradient"""
    out = {'gx': (rel_max(gx, ref_gx), 'x')}
    for name, r in ref.items():
        e = rel_max(grads[name], r)
        k = kind_of(name)
        if k not in out or e > out[k][0]:
            out[k] = (e, name)
    return out
