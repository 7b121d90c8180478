"""float64 numpy yardsticks of the three training-mode BatchNorm kernels of the event network (enslam_eventnet_bn_stats,
_bn_apply, _bn_backward, _bn_running; include/enslam_hip.h documents their arithmetic), with a bound for each quantity.

The bounds are derived from that arithmetic, not measured:
  * a float64 sum of n terms in any order is within (n - 1) u64 of its absolute sum; the kernels' sums add a division and a
    Chan merge per chunk of ROWS rows, a few more roundings each: K(M) = M + 4 ceil(M / ROWS) + 8 roundings cover them;
  * an elementwise result is float64 arithmetic on the terms that are added (a few u64 of their magnitudes) and ONE
    rounding to float32 (u32 of the result), plus what the bounds of the sums it uses let through.
tests/test_eventnet_bn_cpu.py checks the yardsticks against nn.BatchNorm2d in float64 and each bound against what float64
numpy itself differs by (from an extended-precision evaluation) and against 1e-4 of the tensor's maximum."""
import numpy as np

U32 = 2.0 ** -24
U64 = 2.0 ** -53
TINY32 = 2.0 ** -149                # half a float32 denormal step and more: results that round near zero
ROWS = 256                          # rows per chunk of the kernels (the split of M depends on M alone)


def K(M):
    return M + 4 * ((M + ROWS - 1) // ROWS) + 8


def stats(z, dtype=np.float64):
    """(mean [C], biased var [C]) of z [M, C], two-pass, in `dtype`."""
    z = np.asarray(z).astype(dtype)
    mean = z.sum(axis=0) / dtype(z.shape[0])
    var = ((z - mean) ** 2).sum(axis=0) / dtype(z.shape[0])
    return mean, var


def stats_bounds(z):
    """(bound on |mean error| [C], bound on |var error| [C]).  The variance: K u64 of the centred squares, plus what a
    chunk mean off by e = the mean's bound lets through Chan's delta^2 term (first order 4 e std, second order 4 e^2)."""
    z = np.asarray(z, dtype=np.float64)
    M = z.shape[0]
    mean, var = stats(z)
    b_mean = K(M) * U64 * np.abs(z).sum(axis=0) / M
    b_var = K(M) * U64 * var + 4.0 * b_mean * np.sqrt(var) + 4.0 * b_mean ** 2
    return b_mean, b_var


def apply(z, gamma, beta, mean, var, eps, relu=True, dtype=np.float64):
    z = np.asarray(z).astype(dtype)
    a = np.asarray(gamma).astype(dtype) / np.sqrt(np.asarray(var).astype(dtype) + dtype(eps))
    y = a * (z - np.asarray(mean).astype(dtype)) + np.asarray(beta).astype(dtype)
    return np.maximum(y, 0) if relu else y


def apply_bound(z, gamma, beta, mean, var, eps):
    """Elementwise: one float32 rounding of the result, 8 u64 of the two terms that are added (a carries a square root and a
    division, the product and the sum one rounding each)."""
    z = np.asarray(z, dtype=np.float64)
    a = np.asarray(gamma, dtype=np.float64) / np.sqrt(np.asarray(var, dtype=np.float64) + eps)
    t = np.abs(a * (z - mean))
    y = a * (z - mean) + np.asarray(beta, dtype=np.float64)
    return U32 * np.abs(y) + 8.0 * U64 * (t + np.abs(np.asarray(beta, dtype=np.float64))) + TINY32


def backward(z, y, g_y, gamma, mean, var, eps, dtype=np.float64):
    """(g_z [M, C], dgamma [C], dbeta [C]) with gh = g_y where y > 0 (y None: all of g_y) and xh recomputed from z."""
    z = np.asarray(z).astype(dtype)
    M = dtype(z.shape[0])
    inv = dtype(1) / np.sqrt(np.asarray(var).astype(dtype) + dtype(eps))
    xh = (z - np.asarray(mean).astype(dtype)) * inv
    gh = np.asarray(g_y).astype(dtype)
    if y is not None:
        gh = np.where(np.asarray(y) > 0, gh, dtype(0))
    dbeta = gh.sum(axis=0)
    dgamma = (gh * xh).sum(axis=0)
    g_z = (np.asarray(gamma).astype(dtype) * inv) * ((gh - dbeta / M) - xh * (dgamma / M))
    return g_z, dgamma, dbeta


def backward_bounds(z, y, g_y, gamma, mean, var, eps):
    """(bound g_z [M, C], bound dgamma [C], bound dbeta [C]).  The sums: K u64 of their absolute sums (xh adds 4 roundings
    to each product) and the float32 rounding on the way out.  g_z: one float32 rounding, 16 u64 of the terms that are added,
    and the float64 sums' bounds through dbeta / M and xh dgamma / M."""
    z = np.asarray(z, dtype=np.float64)
    M = z.shape[0]
    inv = 1.0 / np.sqrt(np.asarray(var, dtype=np.float64) + eps)
    xh = (z - mean) * inv
    gh = np.asarray(g_y, dtype=np.float64)
    if y is not None:
        gh = np.where(np.asarray(y) > 0, gh, 0.0)
    g_z, dgamma, dbeta = backward(z, y, g_y, gamma, mean, var, eps)
    s_beta = K(M) * U64 * np.abs(gh).sum(axis=0)
    s_gamma = (K(M) + 4) * U64 * np.abs(gh * xh).sum(axis=0)
    a = np.abs(np.asarray(gamma, dtype=np.float64) * inv)
    terms = np.abs(gh) + np.abs(dbeta) / M + np.abs(xh * dgamma) / M
    b_gz = U32 * np.abs(g_z) + 16.0 * U64 * a * terms + a * (s_beta + np.abs(xh) * s_gamma) / M
    b_gz = b_gz + np.where(terms > 0, TINY32, 0.0)
    return b_gz, s_gamma + U32 * np.abs(dgamma), s_beta + U32 * np.abs(dbeta)


def running(run_mean, run_var, mean, var, M, momentum):
    """torch's rule in float64: (1 - m) running + m batch, the variance unbiased."""
    rm = (1.0 - momentum) * np.asarray(run_mean, dtype=np.float64) + momentum * np.asarray(mean, dtype=np.float64)
    rv = (1.0 - momentum) * np.asarray(run_var, dtype=np.float64) + momentum * np.asarray(var, dtype=np.float64) * (M / (M - 1.0))
    return rm, rv


def running_bounds(run_mean, run_var, mean, var, M, momentum):
    """One float32 rounding of the result and 4 u64 of the two terms that are added."""
    rm, rv = running(run_mean, run_var, mean, var, M, momentum)
    tm, tv = running(np.abs(run_mean), np.abs(run_var), np.abs(mean), np.abs(var), M, momentum)
    return U32 * np.abs(rm) + 4.0 * U64 * tm + TINY32, U32 * np.abs(rv) + 4.0 * U64 * tv + TINY32
