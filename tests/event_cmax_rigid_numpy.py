"""The yardstick of the rigid-motion model of event motion compensation (enslam_event_cmax_rigid_eval), written from
include/enslam_hip.h alone, in the manner of tests/event_cmax_numpy.py: one event at a time in Python floats (IEEE float64, one
rounding per operation, no contraction), Python ints for the fixed-point image, math.fsum wherever the header says SUM.  The
blur and the rounding are that file's own (they are stated once in the header and shared by the three models).

`cmax` returns the keys of the existing yardstick; `dropped` has the fourth counter (time, sensor, warp, depth).  `cmax_torch`
is the UNQUANTISED statement in torch float64, differentiable in all six parameters by autograd.

variant: None, or a deliberately WRONG statement of the model for bracketing the tolerance -- 'v_sign' (the translation with
the wrong sign), 'rho_on_rotation' (the inverse depth applied to the rotation terms too), 'depth_at_warp' (the depth read at
the rounded rotation-warped position instead of the event's own pixel)."""
import math

import numpy as np
import torch

from tests.event_cmax_numpy import TWO32, blur, blur_matrix, rint_even

P = 6


def _depth_ok(z):
    return math.isfinite(z) and z > 0.0


def warp(theta, calib, t_ref, t, x, y, z, variant=None, depth=None):
    """(x', y', mx, my, Bu, Bv) of one event of depth z (a Python float holding the float32 value) in the header's order"""
    fx, fy, cx, cy = calib
    wx, wy, wz, vx, vy, vz = theta
    xd, yd = float(x), float(y)
    dt = t - t_ref
    u, v = (xd - cx) / fx, (yd - cy) / fy
    uv, pu, pv = u * v, 1.0 + u * u, 1.0 + v * v
    mx, my = -(dt * fx), -(dt * fy)
    ru = (uv * wx - pu * wy) + v * wz
    rv = (pv * wx - uv * wy) - u * wz
    if variant == 'depth_at_warp':
        H, W = depth.shape
        xr, yr = xd + mx * ru, yd + my * rv
        if math.isfinite(xr) and math.isfinite(yr):
            z = float(depth[min(max(int(round(yr)), 0), H - 1), min(max(int(round(xr)), 0), W - 1)])
            if not _depth_ok(z):
                z = 1.0
    rho = 1.0 / z if z != 0.0 else math.inf
    Bu = (uv, -pu, v, -rho, 0.0, u * rho)
    Bv = (pv, -uv, -u, 0.0, -rho, v * rho)
    if variant == 'v_sign':
        du, dv = ru - rho * (u * vz - vx), rv - rho * (v * vz - vy)
    elif variant == 'rho_on_rotation':
        du, dv = rho * ru + rho * (u * vz - vx), rho * rv + rho * (v * vz - vy)
    else:
        du = ru + rho * (u * vz - vx)
        dv = rv + rho * (v * vz - vy)
    return xd + mx * du, yd + my * dv, mx, my, Bu, Bv


def cmax(t, x, y, p, H, W, calib, theta, t_ref, taps, depth, signed=False, variant=None):
    """dict(iwe int64 [H,W], dropped [4] = (time, sensor, warp, depth), J, mu, f, C, D, grad [6], and per event: xw, yw (nan where
    the event never reached the warp), voted (bool), g [N,6], Gx, Gy, lev_x, lev_y [N,6] = |mx Bu_k|, |my Bv_k|)"""
    theta = [float(v) for v in theta]
    calib = tuple(float(v) for v in calib)
    taps = [float(v) for v in taps]
    t_ref = float(t_ref)
    depth = np.asarray(depth)
    assert depth.dtype == np.float32 and depth.shape == (H, W)
    N = len(t)
    iwe = [[0] * W for _ in range(H)]
    dropped = [0, 0, 0, 0]
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
        z = float(depth[ey, ex])                                        # only now: the pixel is inside
        if not _depth_ok(z):
            dropped[3] += 1
            continue
        with np.errstate(all='ignore'):
            xw, yw, mx, my, Bu, Bv = warp(theta, calib, t_ref, tv, ex, ey, z, variant=variant, depth=depth)
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
    D = blur(C, taps)
    g, Gxs, Gys = np.zeros((N, P)), np.zeros(N), np.zeros(N)
    lev_x, lev_y = np.zeros((N, P)), np.zeros((N, P))
    for e in range(N):
        if votes[e] is None:
            continue
        a, b, oa, ob, s, mx, my, Bu, Bv, corners = votes[e]
        dwx, dwy = [-ob, ob, -b, b], [-oa, -a, oa, a]
        Gx = Gy = 0.0
        for c, py, px in corners:
            Gx = Gx + D[py][px] * dwx[c]
            Gy = Gy + D[py][px] * dwy[c]
        Gxs[e], Gys[e] = Gx, Gy
        for k in range(P):
            g[e, k] = s * (Gx * (mx * Bu[k]) + Gy * (my * Bv[k]))
            lev_x[e, k], lev_y[e, k] = abs(mx * Bu[k]), abs(my * Bv[k])
    scale = 2.0 / npix
    grad = np.array([scale * math.fsum(g[:, k].tolist()) for k in range(P)])
    return dict(iwe=np.array(iwe, dtype=np.int64).reshape(H, W), dropped=np.array(dropped, dtype=np.int64), J=np.array(J).reshape(H, W),
                mu=mu, f=f, C=np.array(C).reshape(H, W), D=np.array(D).reshape(H, W), grad=grad, xw=xw_all, yw=yw_all,
                voted=np.array([v is not None for v in votes], dtype=bool), g=g, Gx=Gxs, Gy=Gys, lev_x=lev_x, lev_y=lev_y)


def cmax_torch(t, x, y, p, H, W, calib, theta, t_ref, taps, depth, signed=False):
    """f(theta) of the unquantised statement as a torch float64 scalar; theta a float64 tensor [6] (requires_grad for autograd)"""
    fx, fy, cx, cy = (float(v) for v in calib)
    t = torch.as_tensor(np.asarray(t, dtype=np.float64))
    xi, yi = torch.as_tensor(np.asarray(x).astype(np.int64)), torch.as_tensor(np.asarray(y).astype(np.int64))
    pol = torch.as_tensor(np.asarray(p).astype(np.int64))
    keep = (xi < W) & (yi < H) & torch.isfinite(t)
    t, xi, yi, pol = t[keep], xi[keep], yi[keep], pol[keep]
    z = torch.as_tensor(np.asarray(depth, dtype=np.float32)).double()[yi, xi]
    keep = torch.isfinite(z) & (z > 0)
    t, xi, yi, pol, z = t[keep], xi[keep], yi[keep], pol[keep], z[keep]
    xd, yd = xi.double(), yi.double()
    dt = t - t_ref
    rho = 1.0 / z
    u, v = (xd - cx) / fx, (yd - cy) / fy
    du = u * v * theta[0] - (1 + u * u) * theta[1] + v * theta[2] + rho * (u * theta[5] - theta[3])
    dv = (1 + v * v) * theta[0] - u * v * theta[1] - u * theta[2] + rho * (v * theta[5] - theta[4])
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
