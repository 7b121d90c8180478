"""numpy yardsticks of the small per-iteration kernels of csrc/util_kernels.hip: camera tensor -> rays and back, the tracker's
in-bound prefilter, the two L1 losses, Adam and the batch depth maximum.  Each one restates the per-element arithmetic in the
precision the kernel declares (np.float32 operations in the written order where the kernel computes in `float`: the library
is built with -ffp-contract=off, and float32 division and square root are correctly rounded) and reduces in float64.  A
reducing yardstick returns, next to each value, `A`: the same expression with every summed term replaced by its absolute
value -- the scale of the running error of a float64 sum taken in another order."""
import numpy as np

f32 = np.float32


def bits_equal(a, b):
    """same shape, same dtype, same bit patterns (so -0.0 != 0.0 and a NaN equals itself)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ---- camera tensor -> rays --------------------------------------------------------------------------------------------------
def rotation32(ct):
    """float32 [3,3] as pose_rotation forms it: s = 2 / (((qr^2 + qi^2) + qj^2) + qk^2), R = I + s P(q), one rounding per operation"""
    qr, qi, qj, qk = (f32(x) for x in np.asarray(ct, f32)[:4])
    one = f32(1.0)
    s = f32(2.0) / (((qr * qr + qi * qi) + qj * qj) + qk * qk)
    return np.array([[one - s * (qj * qj + qk * qk), s * (qi * qj - qk * qr), s * (qi * qk + qj * qr)],
                     [s * (qi * qj + qk * qr), one - s * (qi * qi + qk * qk), s * (qj * qk - qi * qr)],
                     [s * (qi * qk - qj * qr), s * (qj * qk + qi * qr), one - s * (qi * qi + qj * qj)]], f32)


def rotation64(ct):
    qr, qi, qj, qk = (float(x) for x in np.asarray(ct, f32)[:4])
    s = 2.0 / (qr * qr + qi * qi + qj * qj + qk * qk)
    return np.array([[1 - s * (qj * qj + qk * qk), s * (qi * qj - qk * qr), s * (qi * qk + qj * qr)],
                     [s * (qi * qj + qk * qr), 1 - s * (qi * qi + qk * qk), s * (qj * qk - qi * qr)],
                     [s * (qi * qk - qj * qr), s * (qj * qk + qi * qr), 1 - s * (qi * qi + qj * qj)]], np.float64)


def directions32(pi, pj, fx, fy, cx, cy):
    """float32 [n] x 2: (pi - cx) / fx and -(pj - cy) / fy, each operation rounded to float32"""
    pi, pj = np.asarray(pi, f32), np.asarray(pj, f32)
    return (pi - f32(cx)) / f32(fx), -(pj - f32(cy)) / f32(fy)


def pose_rays(ct, pi, pj, fx, fy, cx, cy):
    """(ro, rd) float32 [n,3]: the float32 mirror of pose_rays_fwd_kernel, rd_a = (d0 R_a0 + d1 R_a1) + d2 R_a2 with d2 = -1"""
    ct = np.asarray(ct, f32)
    R = rotation32(ct)
    d0, d1 = directions32(pi, pj, fx, fy, cx, cy)
    d2 = f32(-1.0)
    rd = np.stack([(d0 * R[a, 0] + d1 * R[a, 1]) + d2 * R[a, 2] for a in range(3)], -1).astype(f32)
    ro = np.broadcast_to(ct[4:7], rd.shape).copy()
    return ro, rd


def pose_rays64(ct, pi, pj, fx, fy, cx, cy):
    """(ro, rd, scale) float64 [n,3]: the same rays with every operation in float64 (inputs as the float32 numbers they are) and
    scale_a = |d0||R_a0| + |d1||R_a1| + |R_a2|, what the float32 roundings of the mirror are relative to"""
    ct = np.asarray(ct, f32).astype(np.float64)
    R = rotation64(ct)
    d0 = (np.asarray(pi, f32).astype(np.float64) - float(f32(cx))) / float(f32(fx))
    d1 = -(np.asarray(pj, f32).astype(np.float64) - float(f32(cy))) / float(f32(fy))
    rd = np.stack([d0 * R[a, 0] + d1 * R[a, 1] - R[a, 2] for a in range(3)], -1)
    scale = np.stack([np.abs(d0) * abs(R[a, 0]) + np.abs(d1) * abs(R[a, 1]) + abs(R[a, 2]) for a in range(3)], -1)
    return np.broadcast_to(ct[4:7], rd.shape).copy(), rd, scale


def pose_sums(pi, pj, fx, fy, cx, cy, g_ro, g_rd):
    """(G [3,3], gT [3], their A): G[a][b] = sum_n g_rd[n][a] dir[n][b], gT = sum_n g_ro[n] in float64 over the float32-rounded
    directions; a missing cotangent contributes zeros"""
    d0, d1 = directions32(pi, pj, fx, fy, cx, cy)
    d = np.stack([d0.astype(np.float64), d1.astype(np.float64), -np.ones(len(d0))], -1)
    G, GA, gT, gTA = np.zeros((3, 3)), np.zeros((3, 3)), np.zeros(3), np.zeros(3)
    if g_rd is not None:
        t = np.asarray(g_rd, f32).astype(np.float64)[:, :, None] * d[:, None, :]
        G, GA = t.sum(0), np.abs(t).sum(0)
    if g_ro is not None:
        t = np.asarray(g_ro, f32).astype(np.float64)
        gT, gTA = t.sum(0), np.abs(t).sum(0)
    return G, gT, GA, gTA


def _chain(G, q, absolute):
    """d loss / d quaternion from G through R = I + s P(q), s = 2/|q|^2 (ds/dq_x = -s^2 q_x); with `absolute` every summed
    term is replaced by its absolute value (G is then the matrix of absolute sums)"""
    a = abs if absolute else (lambda x: x)
    sm = lambda *terms: sum(a(t) for t in terms)
    qr, qi, qj, qk = q
    s = 2.0 / (qr * qr + qi * qi + qj * qj + qk * qk)
    P = [[sm(-qj * qj, -qk * qk), sm(qi * qj, -qk * qr), sm(qi * qk, qj * qr)],
         [sm(qi * qj, qk * qr), sm(-qi * qi, -qk * qk), sm(qj * qk, -qi * qr)],
         [sm(qi * qk, -qj * qr), sm(qj * qk, qi * qr), sm(-qi * qi, -qj * qj)]]
    dLds = sm(*(G[i][j] * P[i][j] for i in range(3) for j in range(3)))
    dr = sm(-qk * G[0][1], qj * G[0][2], qk * G[1][0], -qi * G[1][2], -qj * G[2][0], qi * G[2][1])
    di = sm(qj * G[0][1], qk * G[0][2], qj * G[1][0], -2 * qi * G[1][1], -qr * G[1][2], qk * G[2][0], qr * G[2][1], -2 * qi * G[2][2])
    dj = sm(-2 * qj * G[0][0], qi * G[0][1], qr * G[0][2], qi * G[1][0], qk * G[1][2], -qr * G[2][0], qk * G[2][1], -2 * qj * G[2][2])
    dk = sm(-2 * qk * G[0][0], -qr * G[0][1], qi * G[0][2], qr * G[1][0], -2 * qk * G[1][1], qj * G[1][2], qi * G[2][0], qj * G[2][1])
    ds = -s * s
    return np.array([sm(s * dx, dLds * ds * qx) for dx, qx in ((dr, qr), (di, qi), (dj, qj), (dk, qk))], np.float64)


def pose_rays_grad(ct, pi, pj, fx, fy, cx, cy, g_ro, g_rd):
    """(g float64 [7], A float64 [7]): d loss / d camera tensor of pose_rays from the ray cotangents (either may be None)"""
    q = [float(x) for x in np.asarray(ct, f32)[:4]]
    G, gT, GA, gTA = pose_sums(pi, pj, fx, fy, cx, cy, g_ro, g_rd)
    return np.concatenate([_chain(G, q, False), gT]), np.concatenate([_chain(GA, q, True), gTA])


# ---- the tracker's in-bound prefilter and batch maxima -----------------------------------------------------------------------
def depth_max(gd):
    """float32 [2]: max(gd) and fl32(max * 1.2f)"""
    m = np.asarray(gd, f32).max()
    return np.array([m, m * f32(1.2)], f32)


def tracker_prefilter(ro, rd, gd, bound):
    """(inside bool [n], dmax float32 [2]): t = min_axis max_side((bound - o) / d) in float64 with NaN propagating through max
    and min as in torch (such a ray is outside), inside = t >= gd, dmax = depth_max(where(inside, gd, 0))"""
    o, d = np.asarray(ro, f32).astype(np.float64), np.asarray(rd, f32).astype(np.float64)
    b = np.asarray(bound, np.float64).reshape(3, 2)
    gd = np.asarray(gd, f32)
    with np.errstate(divide='ignore', invalid='ignore'):
        t = (b[None, :, :] - o[:, :, None]) / d[:, :, None]
        t = np.min(np.max(t, axis=2), axis=1)               # np.max / np.min propagate NaN
        inside = t >= gd.astype(np.float64)
    return inside, depth_max(np.where(inside, gd, f32(0.0)))


# ---- losses -----------------------------------------------------------------------------------------------------------------
def _color_l1(color, gc):
    """float32 [n]: ((|gc0 - c0| + |gc1 - c1|) + |gc2 - c2|), every operation rounded to float32"""
    e = np.abs(np.asarray(gc, f32) - np.asarray(color, f32))
    return (e[:, 0] + e[:, 1]) + e[:, 2]


def _sign_grad(gd, depth, g):
    """float64 [n]: -g, +g, 0 where gd - depth is >, <, == 0"""
    diff = gd.astype(np.float64) - depth
    return np.where(diff > 0, -g, np.where(diff < 0, g, 0.0))


def _color_grad(color, gc, g, w):
    """float32 [n,3]: (-(fl32(g) * w)) * sign(gc - c)"""
    gw = f32(g) * f32(w)
    return ((-gw) * np.sign(np.asarray(gc, f32) - np.asarray(color, f32))).astype(f32)


def rgbd_loss(depth, color, gd, gc, w, g=1.0):
    """Mapper.py:553-562: sum_{gd>0} |gd - depth| + sum_rays (double)(w * c), c the float32 colour L1 of a ray (every ray).
    (value, A, g_depth float64 [n], g_color float32 [n,3] or None) for the upstream gradient g"""
    depth, gd = np.asarray(depth, np.float64), np.asarray(gd, f32)
    on = gd > 0
    terms = np.where(on, np.abs(gd.astype(np.float64) - depth), 0.0)
    g_depth = np.where(on, _sign_grad(gd, depth, float(g)), 0.0)
    g_color = None
    if color is not None:
        terms = np.concatenate([terms, (f32(w) * _color_l1(color, gc)).astype(np.float64)])
        g_color = _color_grad(color, gc, g, w)
    return float(terms.sum()), float(np.abs(terms).sum()), g_depth, g_color


def tracker_loss(depth, unc, color, gd, gc, w, g=1.0):
    """Tracker.py:187-195: sum_{gd>0} |gd - depth| / sqrt(unc + 1e-10) + sum_{gd>0} (double)w * (double)c.
    (value, A, g_depth, g_color) as rgbd_loss; both gradients are zero where gd <= 0"""
    depth, unc, gd = np.asarray(depth, np.float64), np.asarray(unc, np.float64), np.asarray(gd, f32)
    on = gd > 0
    root = np.sqrt(unc + 1e-10)
    terms = np.where(on, np.abs(gd.astype(np.float64) - depth) / root, 0.0)
    g_depth = np.where(on, _sign_grad(gd, depth, float(g)) / root, 0.0)
    g_color = None
    if color is not None:
        terms = np.concatenate([terms, np.where(on, float(f32(w)) * _color_l1(color, gc).astype(np.float64), 0.0)])
        g_color = np.where(on[:, None], _color_grad(color, gc, g, w), f32(0.0)).astype(f32)
    return float(terms.sum()), float(np.abs(terms).sum()), g_depth, g_color


# ---- Adam -------------------------------------------------------------------------------------------------------------------
def adam(p0, grads, lrs, mask=None, start_step=0, betas=(0.9, 0.999), eps=1e-8):
    """torch.optim.Adam (no weight decay, no amsgrad) in float64, as the kernel's header comment writes it:
        m = b1 m + (1 - b1) g ;  v = b2 v + (1 - b2) g g ;  p -= (lr / (1 - b1^t)) m / (sqrt(v) / sqrt(1 - b2^t) + eps)
    p0 [...], grads [T, ...], lrs [T]; step k (0-based) has t = start_step + k + 1; moments start at zero.  mask (bool over
    the leading axis of p0, or None): rows with mask == 0 keep p, m and v.  Returns (p, m, v), each float64 [T, ...]: the state
    after every step."""
    p = np.array(p0, np.float64)
    m, v = np.zeros_like(p), np.zeros_like(p)
    on = np.ones(p.shape[:1], bool) if mask is None else np.asarray(mask).astype(bool)
    b1, b2 = betas
    P, M, V = [], [], []
    for k, (g, lr) in enumerate(zip(grads, lrs)):
        t = start_step + k + 1
        g = np.asarray(g, np.float64)
        m[on] = b1 * m[on] + (1 - b1) * g[on]
        v[on] = b2 * v[on] + (1 - b2) * g[on] * g[on]
        p[on] = p[on] - (lr / (1 - b1 ** t)) * m[on] / (np.sqrt(v[on]) / np.sqrt(1 - b2 ** t) + eps)
        P.append(p.copy()), M.append(m.copy()), V.append(v.copy())
    return np.array(P), np.array(M), np.array(V)
