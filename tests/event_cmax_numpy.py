"""The yardstick of event motion compensation (enslam_event_cmax_eval), written from include/enslam_hip.h alone: one event at a
time in Python floats (IEEE float64, one rounding per operation, no contraction), Python ints for the fixed-point image, every
blur window spelled out with its zero padding, and math.fsum -- the correctly rounded sum -- wherever the header says SUM, so
that the stated tree order is checked against something that has no order.

`cmax` returns everything a test may want to look at: the integer image, the counters, J, mu, f, J - mu, D, the per-event
warped positions and gradient terms, and the gradient.  `cmax_torch` is the UNQUANTISED statement of the same objective in
torch float64 (votes are the float weights, sums are torch's), differentiable in theta by autograd."""
import math

import numpy as np
import torch

TWO32 = 4294967296
MODELS = {'flow': 2, 'rotation': 3}


def rint_even(v):
    """llrint: to the nearest integer, ties to even (Python's round on a float does exactly this)"""
    return int(round(v))


def warp(model, theta, calib, t_ref, t, x, y):
    """(x', y', mx, my, Bu, Bv) of one event in the header's operation order"""
    fx, fy, cx, cy = calib
    xd, yd = float(x), float(y)
    dt = t - t_ref
    if model == 'flow':
        Bu, Bv = (1.0 / fx, 0.0), (0.0, 1.0 / fy)
        du, dv = theta[0] / fx, theta[1] / fy
    else:
        u, v = (xd - cx) / fx, (yd - cy) / fy
        uv, pu, pv = u * v, 1.0 + u * u, 1.0 + v * v
        Bu, Bv = (uv, -pu, v), (pv, -uv, -u)
        du = (uv * theta[0] - pu * theta[1]) + v * theta[2]
        dv = (pv * theta[0] - uv * theta[1]) - u * theta[2]
    mx, my = -(dt * fx), -(dt * fy)
    return xd + mx * du, yd + my * dv, mx, my, Bu, Bv


def blur(img, taps, variant=None):
    """J = G img: rows then columns, each output its own window, 0.0 outside the image, taps ascending from 0.0"""
    H, W = len(img), len(img[0])
    k, R = len(taps), len(taps) // 2
    rows = [[0.0] * W for _ in range(H)]
    for yy in range(H):
        for xx in range(W):
            acc = 0.0
            for i in range(k):
                xs = xx - R + i
                acc = acc + taps[i] * (img[yy][xs] if 0 <= xs < W else 0.0)
            rows[yy][xx] = acc
    if variant == 'one_pass':
        return rows
    out = [[0.0] * W for _ in range(H)]
    for yy in range(H):
        for xx in range(W):
            acc = 0.0
            for i in range(k):
                ys = yy - R + i
                acc = acc + taps[i] * (rows[ys][xx] if 0 <= ys < H else 0.0)
            out[yy][xx] = acc
    return out


def cmax(t, x, y, p, H, W, calib, model, theta, t_ref, taps, signed=False, variant=None):
    """dict(iwe int64 [H,W], dropped [3] = (time, sensor, warp), J, mu, f, C, D, grad [P], and per event: xw, yw (nan where the
    event never reached the warp), voted (bool), g [N,P], Gx, Gy, lev_x, lev_y [N,P] = |mx Bu_k|, |my Bv_k|).
    variant: None, or a deliberately WRONG statement for bracketing the tolerance -- 'dw_sign' (d w / d x' of the first corner
    with the wrong sign), 'one_pass' (the blur of the gradient image without its column pass), 'no_scale' (2 / (H W) left out)."""
    P = MODELS[model]
    theta = [float(v) for v in theta]
    calib = tuple(float(v) for v in calib)
    taps = [float(v) for v in taps]
    t_ref = float(t_ref)
    N = len(t)
    iwe = [[0] * W for _ in range(H)]
    dropped = [0, 0, 0]
    votes = [None] * N
    xw_all, yw_all = np.full(N, np.nan), np.full(N, np.nan)
    for e in range(N):
        ex, ey, tv = int(x[e]), int(y[e]), float(t[e])
        if ex >= W or ey >= H:
            dropped[1] += 1
            continue
        if not math.isfinite(tv):
            dropped[0] += 1
            continue
        xw, yw, mx, my, Bu, Bv = warp(model, theta, calib, t_ref, tv, ex, ey)
        xw_all[e], yw_all[e] = xw, yw
        if not (xw > -1.0 and xw < float(W) and yw > -1.0 and yw < float(H)):
            dropped[2] += 1
            continue
        fx0, fy0 = math.floor(xw), math.floor(yw)
        a, b = xw - fx0, yw - fy0
        oa, ob = 1.0 - a, 1.0 - b
        s = -1 if (signed and not int(p[e])) else 1
        corners = []
        for c, w in enumerate((oa * ob, a * ob, oa * b, a * b)):
            px, py = fx0 + (c & 1), fy0 + (c >> 1)
            if 0 <= px < W and 0 <= py < H:
                iwe[py][px] += s * rint_even(w * float(TWO32))
                corners.append((c, py, px))
        votes[e] = (a, b, oa, ob, float(s), mx, my, Bu, Bv, corners)
    img = [[float(q) * (1.0 / TWO32) for q in row] for row in iwe]
    J = blur(img, taps)
    npix = float(H * W)
    mu = math.fsum(v for row in J for v in row) / npix
    C = [[v - mu for v in row] for row in J]
    f = math.fsum(v * v for row in C for v in row) / npix
    D = blur(C, taps, variant='one_pass' if variant == 'one_pass' else None)
    g, Gxs, Gys = np.zeros((N, P)), np.zeros(N), np.zeros(N)
    lev_x, lev_y = np.zeros((N, P)), np.zeros((N, P))
    for e in range(N):
        if votes[e] is None:
            continue
        a, b, oa, ob, s, mx, my, Bu, Bv, corners = votes[e]
        dwx, dwy = [-ob, ob, -b, b], [-oa, -a, oa, a]
        if variant == 'dw_sign':
            dwx[0] = ob
        Gx = Gy = 0.0
        for c, py, px in corners:
            Gx = Gx + D[py][px] * dwx[c]
            Gy = Gy + D[py][px] * dwy[c]
        Gxs[e], Gys[e] = Gx, Gy
        for k in range(P):
            g[e, k] = s * (Gx * (mx * Bu[k]) + Gy * (my * Bv[k]))
            lev_x[e, k], lev_y[e, k] = abs(mx * Bu[k]), abs(my * Bv[k])
    scale = 1.0 if variant == 'no_scale' else 2.0 / npix
    grad = np.array([scale * math.fsum(g[:, k].tolist()) for k in range(P)])
    return dict(iwe=np.array(iwe, dtype=np.int64).reshape(H, W), dropped=np.array(dropped, dtype=np.int64), J=np.array(J).reshape(H, W),
                mu=mu, f=f, C=np.array(C).reshape(H, W), D=np.array(D).reshape(H, W), grad=grad, xw=xw_all, yw=yw_all,
                voted=np.array([v is not None for v in votes], dtype=bool), g=g, Gx=Gxs, Gy=Gys, lev_x=lev_x, lev_y=lev_y)


def blur_matrix(n, taps):
    """the zero-padded blur along one dimension of length n as an n x n matrix (symmetric for symmetric taps)"""
    k, R = len(taps), len(taps) // 2
    M = torch.zeros((n, n), dtype=torch.float64)
    for o in range(n):
        for i in range(k):
            s = o - R + i
            if 0 <= s < n:
                M[o, s] = taps[i]
    return M


def cmax_torch(t, x, y, p, H, W, calib, model, theta, t_ref, taps, signed=False):
    """f(theta) of the unquantised statement as a torch float64 scalar; theta a float64 tensor [P] (requires_grad for autograd).
    The cell of every vote (floor) is piecewise constant, so autograd gives the derivative the header states."""
    fx, fy, cx, cy = (float(v) for v in calib)
    t = torch.as_tensor(np.asarray(t, dtype=np.float64))
    xi, yi = torch.as_tensor(np.asarray(x).astype(np.int64)), torch.as_tensor(np.asarray(y).astype(np.int64))
    keep = (xi < W) & (yi < H) & torch.isfinite(t)
    t, xi, yi = t[keep], xi[keep], yi[keep]
    pol = torch.as_tensor(np.asarray(p).astype(np.int64))[keep]
    xd, yd = xi.double(), yi.double()
    dt = t - t_ref
    if model == 'flow':
        du, dv = theta[0] / fx + 0 * xd, theta[1] / fy + 0 * xd
    else:
        u, v = (xd - cx) / fx, (yd - cy) / fy
        du = u * v * theta[0] - (1 + u * u) * theta[1] + v * theta[2]
        dv = (1 + v * v) * theta[0] - u * v * theta[1] - u * theta[2]
    xw, yw = xd - dt * fx * du, yd - dt * fy * dv
    ok = (xw > -1) & (xw < W) & (yw > -1) & (yw < H)
    xw, yw, pol = xw[ok], yw[ok], pol[ok]
    x0, y0 = torch.floor(xw).detach(), torch.floor(yw).detach()
    a, b = xw - x0, yw - y0
    s = torch.where((pol != 0) | (not signed), 1.0, -1.0).double()
    img = torch.zeros(H * W, dtype=torch.float64)
    for c, w in enumerate(((1 - a) * (1 - b), a * (1 - b), (1 - a) * b, a * b)):
        px, py = x0.long() + (c & 1), y0.long() + (c >> 1)
        ins = (px >= 0) & (px < W) & (py >= 0) & (py < H)
        img = img.index_add(0, (py * W + px)[ins], (s * w)[ins])
    J = blur_matrix(H, taps) @ img.reshape(H, W) @ blur_matrix(W, taps).T
    return ((J - J.mean()) ** 2).mean()
