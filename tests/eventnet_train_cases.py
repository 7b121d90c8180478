"""Cases, references and tolerances shared by tests/test_eventnet_train_cpu.py and tests/test_hip_eventnet_train.py: the
parameter gradients of the event network (event.compile_event_net_trainable, enslam_eventnet_backward_weights).

Nets and inputs are those of tests/eventnet_cases.py with every parameter requiring a gradient; BatchNorm stays in eval
mode, so the gradients are those of the eval-mode module."""
import copy
import functools

import numpy as np
import torch

from tests.eventnet_cases import NET_SHAPES, U, gamma, make_inputs, make_net, place  # noqa: F401  (re-exported)

KINDS = ('conv', 'bn_gamma', 'bn_beta', 'heads')

# Error of the float32 torch module's parameter gradients on the CPU against the float64 module's, per shape and parameter
# kind: max |difference| / max |float64| per tensor, the worst over the tensors of the kind (seed 0).  Measured by
# test_eventnet_train_cpu.py::test_recorded_float32_errors, which re-measures them and fails when a recorded value is off
# by more than 4x.  The GPU tolerance is 8x the recorded value (the rule of eventnet_cases.F32_ERR), capped at 1e-4: the
# cap of 1e-5 used for the outputs would cut into the 8x margin here (8 x 1.92e-6 = 1.5e-5), and a wrong tap, a transposed
# block or a missing relu mask costs 1e-2 or more.
F32_ERR_PARAMS = {
    '16x16': {'conv': 9.14e-7, 'bn_gamma': 1.32e-6, 'bn_beta': 7.00e-7, 'heads': 3.55e-7},
    '17x19': {'conv': 7.24e-7, 'bn_gamma': 8.42e-7, 'bn_beta': 5.55e-7, 'heads': 8.44e-7},
    '16x70': {'conv': 1.28e-6, 'bn_gamma': 9.59e-7, 'bn_beta': 8.36e-7, 'heads': 6.34e-7},
    '39x51': {'conv': 1.92e-6, 'bn_gamma': 8.76e-7, 'bn_beta': 9.97e-7, 'heads': 1.59e-6},
}
TOL_MARGIN, TOL_CAP = 8.0, 1e-4


def tolerance(shape, kind):
    return min(TOL_MARGIN * F32_ERR_PARAMS[shape][kind], TOL_CAP)


def kind_of(name):
    """Parameter kind of a UNet_2heads parameter name."""
    if name.startswith('outc_'):
        return 'heads'
    mod, leaf = name.split('.')[-2:]
    if mod in ('0', '3'):
        return 'conv'
    assert mod in ('1', '4'), name
    return 'bn_gamma' if leaf == 'weight' else 'bn_beta'


def make_trainable_net(seed=0):
    """eventnet_cases.make_net with every parameter requiring a gradient (eval mode, float32, on the CPU)."""
    net = copy.deepcopy(make_net(seed))
    net.requires_grad_(True)
    return net.eval()


def run_module_params(net, x, g_events, g_probs, dtype):
    """({parameter name: gradient}, d/dx) of the eval-mode torch module on the CPU in `dtype`, as float64 numpy arrays."""
    m = copy.deepcopy(net).to(dtype).eval()
    m.requires_grad_(True)
    xx = x.detach().to(dtype).requires_grad_(True)
    e, p = m(xx)
    (e * g_events.to(dtype)).sum().add((p * g_probs.to(dtype)).sum()).backward()
    return {n: q.grad.detach().double().numpy() for n, q in m.named_parameters()}, xx.grad.detach().double().numpy()


@functools.lru_cache(maxsize=None)
def reference_params(shape, seed=0):
    """float64 ({name: gradient}, gx) of case `shape`: computed once, shared, never modified (arrays are read-only)."""
    grads, gx = run_module_params(make_net(seed), *make_inputs(shape, seed), torch.float64)
    for a in list(grads.values()) + [gx]:
        a.setflags(write=False)
    return grads, gx


def rel_max(a, ref):
    return float(np.abs(np.asarray(a, dtype=np.float64) - ref).max() / np.abs(ref).max())


def errors_by_kind(grads, ref):
    """{kind: (worst rel_max over the kind's tensors, the name of the tensor that set it)}"""
    out = {}
    for name, r in ref.items():
        e = rel_max(grads[name], r)
        k = kind_of(name)
        if k not in out or e > out[k][0]:
            out[k] = (e, name)
    return out


def np_conv3x3_wgrad(src, g, saved=None):
    """(dW [9 C, N], db [N]) of a 3x3 zero-padded convolution in float64: dW[tap * C + c, n] = sum_{y, x}
    src[y + ky - 1, x + kx - 1, c] * G[y, x, n], db[n] = sum G[y, x, n], tap = 3 ky + kx, G = g where saved > 0 (all of g
    without `saved`).  src [H, W, C], g / saved [H, W, N]."""
    src = np.asarray(src, dtype=np.float64)
    G = np.asarray(g, dtype=np.float64)
    if saved is not None:
        G = np.where(np.asarray(saved) > 0, G, 0.0)
    H, W, C = src.shape
    pad = np.zeros((H + 2, W + 2, C))
    pad[1:-1, 1:-1] = src
    G2 = G.reshape(H * W, -1)
    dW = np.concatenate([pad[ky:ky + H, kx:kx + W].reshape(H * W, C).T.dot(G2) for ky in range(3) for kx in range(3)], axis=0)
    return dW, G2.sum(axis=0)
