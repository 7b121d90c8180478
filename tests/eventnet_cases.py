"""Cases, references and tolerances shared by tests/test_eventnet_cpu.py and tests/test_hip_eventnet.py.

Nets are built on the CPU under a seed.  BatchNorm's running statistics, gamma and beta are randomised: the defaults make
BN the identity and folding would go untested.  gamma is drawn around 2 so that the activations keep their scale through
the 18 convolutions of a path (Kaiming-uniform weights alone shrink them by ~0.4 per layer).  Every parameter is frozen.
"""
import functools

import numpy as np
import torch
import torch.nn.functional as F

U = 2.0 ** -24                      # float32 unit roundoff

# whole-net shapes, each for what it exercises
NET_SHAPES = {
    '16x16': (16, 16),              # no padding anywhere, 1 x 1 bottom level
    '17x19': (17, 19),              # padding at two levels, on both axes
    '16x70': (16, 70),              # pixel tiles crossed in x
    '39x51': (39, 51),              # the RPG event shape
}

# Error of the float32 torch module on the CPU against the float64 module on the CPU (max |difference| / max |float64|),
# nets and inputs as below.  Measured by test_eventnet_cpu.py::test_recorded_float32_errors, which re-measures them and
# fails when a recorded value is off by more than 4x; the GPU tolerances are 8x these values, capped at 1e-5.  The margin
# covers the blocked summation order of the MFMA tiles over reductions of up to 9 216 terms and the one extra rounding per
# folded weight; the cap keeps a wrong tap or a transposed weight (1e-2 or more) from passing.
F32_ERR = {
    '16x16': {'events': 1.01e-6, 'probs': 2.15e-7, 'gx': 3.01e-7},
    '17x19': {'events': 9.32e-7, 'probs': 1.42e-7, 'gx': 3.75e-7},
    '16x70': {'events': 9.83e-7, 'probs': 1.62e-7, 'gx': 3.49e-7},
    '39x51': {'events': 1.19e-6, 'probs': 1.90e-7, 'gx': 4.12e-7},
}
TOL_MARGIN, TOL_CAP = 8.0, 1e-5


def tolerance(shape, quantity):
    return min(TOL_MARGIN * F32_ERR[shape][quantity], TOL_CAP)


def make_net(seed=0):
    """Seeded frozen eval-mode UNet_2heads(6, 2, 2) with randomised BatchNorm, on the CPU (float32)."""
    import evennicer_slam_amd as E
    gen = torch.Generator().manual_seed(1000 + seed)
    torch.manual_seed(seed)
    net = E.event.UNet_2heads(6, 2, 2)
    for m in net.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            n = m.num_features
            m.running_mean.copy_(0.1 * torch.randn(n, generator=gen))
            m.running_var.copy_(0.5 + torch.rand(n, generator=gen))
            m.weight.data.copy_(1.5 + torch.rand(n, generator=gen))
            m.bias.data.copy_(0.1 * torch.randn(n, generator=gen))
    net.requires_grad_(False)
    return net.eval()


def make_inputs(shape, seed=0):
    """x in [0, 1] and upstream gradients for both outputs, float32 on the CPU."""
    H, W = NET_SHAPES[shape] if isinstance(shape, str) else shape
    gen = torch.Generator().manual_seed(77 + seed)
    x = torch.rand(1, 6, H, W, generator=gen)
    g_events = torch.randn(1, 2, H, W, generator=gen)
    g_probs = torch.randn(1, 2, H, W, generator=gen)
    return x, g_events, g_probs


def run_module(net, x, g_events, g_probs, dtype):
    """(events, probs, d/dx) of the torch module on the CPU in `dtype`, as float64 numpy arrays."""
    import copy
    m = copy.deepcopy(net).to(dtype)
    xx = x.to(dtype).requires_grad_(True)
    e, p = m(xx)
    (e * g_events.to(dtype)).sum().add((p * g_probs.to(dtype)).sum()).backward()
    return tuple(t.detach().double().numpy() for t in (e, p, xx.grad))


@functools.lru_cache(maxsize=None)
def reference(shape, seed=0):
    """float64 (events, probs, gx) of case `shape`: computed once, shared, never modified (arrays are read-only)."""
    out = run_module(make_net(seed), *make_inputs(shape, seed), torch.float64)
    for a in out:
        a.setflags(write=False)
    return out


def rel_max(a, ref):
    return float(np.abs(np.asarray(a, dtype=np.float64) - ref).max() / np.abs(ref).max())


# ---------------------------------------------------------------------------------------------------------------------
# numpy restatement of the packed layouts (include/enslam_hip.h): channels-last images, weight rows tap * C + c
# ---------------------------------------------------------------------------------------------------------------------
def np_conv3x3(rows, bias, src, relu=False):
    """out[y, x, n] = act(sum_{tap, c} src[y + ky - 1, x + kx - 1, c] * rows[tap * C + c, n] + bias[n]) in float64, zero
    padding, tap = 3 ky + kx.  src [H, W, C], rows [9 C, N]."""
    src = np.asarray(src, dtype=np.float64)
    rows = np.asarray(rows, dtype=np.float64)
    H, W, C = src.shape
    pad = np.zeros((H + 2, W + 2, C))
    pad[1:-1, 1:-1] = src
    out = np.zeros((H, W, rows.shape[1]))
    for tap in range(9):
        ky, kx = divmod(tap, 3)
        out += pad[ky:ky + H, kx:kx + W].reshape(H * W, C) .dot(rows[tap * C:(tap + 1) * C]).reshape(H, W, -1)
    if bias is not None:
        out += np.asarray(bias, dtype=np.float64)
    return np.maximum(out, 0.0) if relu else out


def gamma(n):
    return n * U / (1.0 - n * U)


def place(src1, H, W, oy, ox):
    """src1 [H1, W1, C] at offset (oy, ox) inside a zero [H, W, C] image (F.pad of the up-sampled feature)."""
    out = np.zeros((H, W, src1.shape[2]), dtype=src1.dtype)
    out[oy:oy + src1.shape[0], ox:ox + src1.shape[1]] = src1
    return out


def folded_forward(folded, heads, x):
    """The module's forward restated on folded convolutions (fold_event_net), float64 torch on the CPU."""
    def pair(i, t):
        for k in (i, i + 1):
            t = F.relu(F.conv2d(t, folded[k][0], folded[k][1], padding=1))
        return t
    feats = [pair(0, x)]
    for l in range(1, 5):
        feats.append(pair(2 * l, F.max_pool2d(feats[-1], 2)))
    outs = []
    for h in range(2):
        t = feats[4]
        for j in range(4):
            skip = feats[3 - j]
            t = F.interpolate(t, scale_factor=2, mode='bilinear', align_corners=True)
            dy, dx = skip.shape[2] - t.shape[2], skip.shape[3] - t.shape[3]
            t = F.pad(t, [dx // 2, dx - dx // 2, dy // 2, dy - dy // 2])
            t = pair(10 + 8 * h + 2 * j, torch.cat([skip, t], dim=1))
        outs.append(F.conv2d(t, heads[h][0], heads[h][1]))
    return outs[0], torch.sigmoid(outs[1])
