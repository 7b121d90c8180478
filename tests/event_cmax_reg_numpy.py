"""The yardstick of the event-collapse regularisers of contrast maximisation (enslam_event_cmax_reg_eval), written from
include/enslam_hip.h alone, in the manner of tests/event_cmax_rigid_numpy.py: one event at a time in Python floats (IEEE float64,
one rounding per operation, no contraction), math.fsum wherever the header says SUM, M a Python int.  Which events vote is the
existing yardsticks' answer (`voted` of tests/event_cmax_numpy.py / tests/event_cmax_rigid_numpy.py): the regulariser adds no
check of its own.

`reg` returns dict(R, dR [P], M, r [N], dr [N,P]).  `reg_torch` is an independent statement in torch float64: the Jacobian of
the motion field by autograd in (u, v), d from the 2 x 2 determinant of 1 - dt c written out, R differentiable in theta.

variant: None, or a deliberately WRONG statement for bracketing the tolerance -- 'c11_u' (-u w_y in place of -2 u w_y in c11),
'det_plus' (+ c12 c21 in place of - c12 c21), 'over_N' (division by N instead of M)."""
import math

import numpy as np
import torch

KINDS = ('divergence', 'deformation')
PARAMS = {'flow': 2, 'rotation': 3, 'rigid': 6}


def event(theta6, dt, u, v, rho, kind, P, variant=None):
    """(d, dd [P]) of one event in the header's order; theta6 = (w, v) with zeros where the model has no parameter"""
    wx, wy, wz, _, _, vz = theta6
    two_u = u if variant == 'c11_u' else 2.0 * u
    c11 = (v * wx - two_u * wy) + rho * vz
    c22 = ((2.0 * v) * wx - u * wy) + rho * vz
    c12 = u * wx + wz
    c21 = -(v * wy) - wz
    e11 = (v, -two_u, 0.0, 0.0, 0.0, rho)
    e22 = (2.0 * v, -u, 0.0, 0.0, 0.0, rho)
    e12 = (u, 0.0, 1.0, 0.0, 0.0, 0.0)
    e21 = (0.0, -v, -1.0, 0.0, 0.0, 0.0)
    dt2 = dt * dt
    d = -(dt * (c11 + c22))
    if kind == 'deformation':
        d = d + dt2 * ((c11 * c22 + c12 * c21) if variant == 'det_plus' else (c11 * c22 - c12 * c21))
    dd = []
    for k in range(P):
        g = -(dt * (e11[k] + e22[k]))
        if kind == 'deformation':
            a, b = e11[k] * c22 + c11 * e22[k], e12[k] * c21 + c12 * e21[k]
            g = g + dt2 * ((a + b) if variant == 'det_plus' else (a - b))
        dd.append(g)
    return d, dd


def reg(t, x, y, voted, calib, model, theta, t_ref, kind, depth=None, variant=None):
    """the regulariser of a stream whose voting events are `voted` (bool [N], the base yardstick's)"""
    assert kind in KINDS
    P = PARAMS[model]
    fx, fy, cx, cy = (float(v) for v in calib)
    theta6 = [float(v) for v in theta] + [0.0] * (6 - P)
    t_ref = float(t_ref)
    N = len(t)
    M = int(np.count_nonzero(voted))
    r, dr = [0.0] * N, [[0.0] * P for _ in range(N)]
    if model != 'flow':
        for e in range(N):
            if not voted[e]:
                continue
            xd, yd = float(int(x[e])), float(int(y[e]))
            u, v = (xd - cx) / fx, (yd - cy) / fy
            dt = float(t[e]) - t_ref
            rho = 1.0 / float(depth[int(y[e]), int(x[e])]) if model == 'rigid' else 0.0
            d, dd = event(theta6, dt, u, v, rho, kind, P, variant=variant)
            sg = 1.0 if d > 0.0 else (-1.0 if d < 0.0 else 0.0)
            r[e] = abs(d)
            dr[e] = [sg * g for g in dd]
    div = N if variant == 'over_N' else M
    R = math.fsum(r) / div if div else 0.0
    dR = [math.fsum(row[k] for row in dr) / div if div else 0.0 for k in range(P)]
    return dict(R=R, dR=np.array(dR, dtype=np.float64), M=M, r=np.array(r, dtype=np.float64), dr=np.array(dr, dtype=np.float64).reshape(N, P))


def reg_torch(t, x, y, voted, calib, model, theta, t_ref, kind, depth=None):
    """R(theta) as a torch float64 scalar over the events of `voted`; theta a float64 tensor [P] (requires_grad for autograd)"""
    fx, fy, cx, cy = (float(v) for v in calib)
    keep = torch.as_tensor(np.asarray(voted, dtype=bool))
    if model == 'flow' or not bool(keep.any()):
        return (theta * 0.0).sum()
    tt = torch.as_tensor(np.asarray(t, dtype=np.float64))[keep]
    xi = torch.as_tensor(np.asarray(x).astype(np.int64))[keep]
    yi = torch.as_tensor(np.asarray(y).astype(np.int64))[keep]
    u = ((xi.double() - cx) / fx).requires_grad_(True)
    v = ((yi.double() - cy) / fy).requires_grad_(True)
    dt = tt - float(t_ref)
    if model == 'rigid':
        rho = 1.0 / torch.as_tensor(np.asarray(depth, dtype=np.float32)).double()[yi, xi]
        lin = theta[3:]
    else:
        rho, lin = torch.zeros_like(dt), torch.zeros(3, dtype=torch.float64)
    du = u * v * theta[0] - (1 + u * u) * theta[1] + v * theta[2] + rho * (u * lin[2] - lin[0])
    dv = (1 + v * v) * theta[0] - u * v * theta[1] - u * theta[2] + rho * (v * lin[2] - lin[1])
    # the events are independent: the gradient of the sum is the per-event derivative (the depth held constant)
    c11, c12 = torch.autograd.grad(du.sum(), (u, v), create_graph=True)
    c21, c22 = torch.autograd.grad(dv.sum(), (u, v), create_graph=True)
    if kind == 'divergence':
        d = -dt * (c11 + c22)
    else:
        d = (1 - dt * c11) * (1 - dt * c22) - (dt * c12) * (dt * c21) - 1
    return d.abs().mean()
