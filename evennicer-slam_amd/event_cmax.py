"""Event motion compensation by contrast maximisation (Gallego, Rebecq, Scaramuzza, CVPR 2018): what the time stamps of a
stream are for.  Every event is warped along a candidate motion to a reference time and voted into an image of warped events
(IWE); the motion that makes the blurred IWE sharpest (largest variance) compensates the stream's motion blur and is an
estimate of the image flow or of the camera's angular velocity from events alone -- or, with a depth image, of all six
velocity components of the camera at metric scale ('rigid').

    warp_image       the IWE (float64) of a stream under a motion, and its blur
    contrast         (f, grad): the variance of the blurred IWE and its gradient in the motion
    regulariser      (R, dR, M): the event-collapse regulariser of a motion, the mean absolute divergence or deformation of its warp
    estimate_motion  maximises f (or f - lambda R) from theta0: BFGS on the 2, 3 or 6 parameters on the host, float64, deterministic
    relative_rotation  the 4 x 4 camera-to-camera delta of an angular velocity over dt, in the project's camera convention
    relative_motion  the same for a six-vector (w, v) of 'rigid': the exact SE(3) exponential; camera_velocity is its inverse
    cmax_numpy       the CPU route: the operations and the sum order of include/enslam_hip.h in numpy

include/enslam_hip.h (enslam_event_cmax_eval, enslam_event_cmax_rigid_eval, enslam_event_cmax_reg_eval) fixes the model and the order of every float64 operation; a stream on a HIP
device runs csrc/event_cmax.hip, one on the CPU runs cmax_numpy, and the two return the same bits.

Motion models ('flow': theta = image flow in pixels / s; 'rotation': theta = angular velocity in rad / s; 'rigid': theta =
(angular velocity, linear velocity in depth units / s), with `depth` a float32 [H, W] image at the sensor's resolution) live in the PINHOLE
frame of the calibration (x right, y down, z forward), which is what the kernel sees.  The project's cameras look down -z with
y up (common.get_rays, synthetic.py): `to_pinhole` / `from_pinhole` flip y and z, and relative_rotation returns its delta in the
project's convention.  The warp is first order in |omega| dt (a few hundredths of a radian)."""
import math

import numpy as np
import torch

from ._lib import EnslamError

MODELS = {'flow': 2, 'rotation': 3, 'rigid': 6}
MAX_KSIZE = 31
DROPPED = ('time', 'sensor', 'warp')
DROPPED_RIGID = DROPPED + ('depth',)            # 'rigid' alone has the fourth counter
REGS = ('divergence', 'deformation')            # the collapse regularisers of enslam_event_cmax_reg_eval
_TWO32 = 4294967296.0


def blur_taps(sigma=1.5, ksize=None):
    """The float64 taps of the objective's blur: event.gaussian_kernel1d's own numbers.  ksize defaults to 2 int(3 sigma) + 1
    (9 at the default sigma); sigma <= 0 or ksize 1 means no blur."""
    from .event import gaussian_kernel1d
    if sigma is None or sigma <= 0:
        return [1.0]
    k = 2 * int(3.0 * sigma) + 1 if ksize is None else int(ksize)
    if k <= 0 or k % 2 == 0 or k > MAX_KSIZE:
        raise EnslamError(f"event_cmax: the blur size must be odd and in 1..{MAX_KSIZE} (got {k})")
    if k == 1:
        return [1.0]
    return gaussian_kernel1d(k, sigma=float(sigma), dtype=torch.float64).tolist()


def calib_tuple(calib):
    """(fx, fy, cx, cy) from a dict with those keys, a 3 x 3 matrix or four numbers"""
    if isinstance(calib, dict):
        return tuple(float(calib[k]) for k in ('fx', 'fy', 'cx', 'cy'))
    a = np.asarray(calib, dtype=np.float64)
    if a.shape == (3, 3):
        return float(a[0, 0]), float(a[1, 1]), float(a[0, 2]), float(a[1, 2])
    if a.shape == (4,):
        return tuple(float(v) for v in a)
    raise EnslamError("event_cmax: calib is a dict with fx, fy, cx, cy, a 3 x 3 matrix or (fx, fy, cx, cy)")


def to_pinhole(omega):
    """An axial vector of the project's camera frame (x right, y up, z back) in the pinhole frame (x right, y down, z forward):
    the two differ by the half turn about x, which flips y and z."""
    w = [float(v) for v in omega]
    return [w[0], -w[1], -w[2]]


from_pinhole = to_pinhole            # the flip is its own inverse


def tree_sum(v):
    """SUM of enslam_hip.h over a float64 vector: blocks of 256 padded with 0.0 through the halving tree, the block results
    256 at a time through the same tree, the rest added in ascending order from 0.0."""
    v = np.asarray(v, dtype=np.float64).reshape(-1)
    for _ in range(2):
        n = v.size
        blocks = -(-n // 256)
        w = np.zeros(blocks * 256, dtype=np.float64)
        w[:n] = v
        w = w.reshape(blocks, 256)
        s = 128
        while s >= 1:
            w[:, :s] += w[:, s:2 * s]
            s //= 2
        v = w[:, 0].copy()
    acc = np.float64(0.0)
    for x in v.tolist():
        acc = acc + np.float64(x)
    return float(acc)


def _blur(img, taps):
    """the zero-padded separable blur of the header: rows then columns, taps ascending from 0.0"""
    taps = [np.float64(v) for v in taps]
    k, R = len(taps), len(taps) // 2
    H, W = img.shape
    pad = np.zeros((H, W + 2 * R), dtype=np.float64)
    pad[:, R:R + W] = img
    rows = np.zeros((H, W), dtype=np.float64)
    for i in range(k):
        rows = rows + taps[i] * pad[:, i:i + W]
    pad = np.zeros((H + 2 * R, W), dtype=np.float64)
    pad[R:R + H, :] = rows
    out = np.zeros((H, W), dtype=np.float64)
    for i in range(k):
        out = out + taps[i] * pad[i:i + H, :]
    return out


def _host_depth(depth, model, H, W):
    """the float32 [H, W] numpy image of a 'rigid' call on the CPU route (a CPU tensor or an array); None for the other models"""
    if model != 'rigid':
        if depth is not None:
            raise EnslamError(f"event_cmax: model {model!r} takes no depth")
        return None
    if torch.is_tensor(depth) and depth.device.type == 'cpu':
        depth = depth.detach().numpy()
    if not isinstance(depth, np.ndarray) or depth.dtype != np.float32 or depth.shape != (H, W):
        raise EnslamError(f"event_cmax: model 'rigid' takes depth, a float32 [{H},{W}] image on the stream's device (got "
                          f"{(depth.dtype, tuple(depth.shape)) if hasattr(depth, 'shape') else type(depth).__name__})")
    return depth


def _check_reg(reg):
    if reg is not None and reg not in REGS:
        raise EnslamError(f"event_cmax: reg must be None or one of {list(REGS)} (got {reg!r})")


def cmax_numpy(t, x, y, p, H, W, calib, model, theta, t_ref, taps, signed=False, want_grad=True, depth=None, reg=None):
    """The CPU route of enslam_event_cmax_eval and enslam_event_cmax_rigid_eval on numpy arrays: (iwe int64 [H,W], blurred
    float64 [H,W], stats float64 [2 + P], dropped int64 [3], or [4] = (time, sensor, warp, depth) for 'rigid') with every
    operation and every sum in the header's order.  reg 'divergence' or 'deformation': the route of enslam_event_cmax_reg_eval,
    the same four and a fifth, reg_stats float64 [2 + P] = (R, M, dR...)."""
    if model not in MODELS:
        raise EnslamError(f"event_cmax: model must be one of {sorted(MODELS)} (got {model!r})")
    _check_reg(reg)
    P = MODELS[model]
    fx, fy, cx, cy = (np.float64(v) for v in calib_tuple(calib))
    th = [np.float64(v) for v in theta]
    taps = [float(v) for v in taps]
    H, W = int(H), int(W)
    if len(th) != P:
        raise EnslamError(f"event_cmax: model {model!r} takes {P} parameters (got {len(th)})")
    if H <= 0 or W <= 0 or H > 65536 or W > 65536 or H * W > (1 << 28):
        raise EnslamError(f"event_cmax: the sensor must have 1..65536 rows and columns and at most 2^28 pixels (got {H} x {W})")
    if len(taps) % 2 == 0 or len(taps) > MAX_KSIZE:
        raise EnslamError(f"event_cmax: the blur takes an odd number of taps up to {MAX_KSIZE} (got {len(taps)})")
    if not all(math.isfinite(float(v)) for v in list(th) + [fx, fy, cx, cy, t_ref] + taps) or fx == 0 or fy == 0:
        raise EnslamError("event_cmax: theta, t_ref, the intrinsics and the taps must be finite, fx and fy not 0")
    depth = _host_depth(depth, model, H, W)
    t = np.asarray(t, dtype=np.float64)
    N = t.size
    t_ref = np.float64(t_ref)
    xi, yi = np.asarray(x).astype(np.int64), np.asarray(y).astype(np.int64)
    pol = np.asarray(p) != 0
    with np.errstate(all='ignore'):
        sensor = (xi >= W) | (yi >= H)
        timed = ~sensor & ~np.isfinite(t)
        deep = np.zeros(N, dtype=bool)
        xd, yd = xi.astype(np.float64), yi.astype(np.float64)
        dt = t - t_ref
        zero = np.zeros(N, dtype=np.float64)
        if model == 'flow':
            Bu = [zero + np.float64(1.0) / fx, zero]
            Bv = [zero, zero + np.float64(1.0) / fy]
            du = zero + th[0] / fx
            dv = zero + th[1] / fy
        else:
            u, v = (xd - cx) / fx, (yd - cy) / fy
            uv, pu, pv = u * v, 1.0 + u * u, 1.0 + v * v
            Bu, Bv = [uv, -pu, v], [pv, -uv, -u]
            du = (uv * th[0] - pu * th[1]) + v * th[2]
            dv = (pv * th[0] - uv * th[1]) - u * th[2]
            if model == 'rigid':
                z = depth.reshape(-1)[np.where(sensor, 0, yi * W + xi)]            # the event's own pixel, once it is checked
                deep = ~sensor & ~timed & ~(np.isfinite(z) & (z > 0))
                rho = np.float64(1.0) / z.astype(np.float64)
                Bu, Bv = Bu + [-rho, zero, u * rho], Bv + [zero, -rho, v * rho]
                du = du + rho * (u * th[5] - th[3])
                dv = dv + rho * (v * th[5] - th[4])
        mx, my = -(dt * fx), -(dt * fy)
        xw, yw = xd + mx * du, yd + my * dv
        ok = ~sensor & ~timed & ~deep & (xw > -1.0) & (xw < np.float64(W)) & (yw > -1.0) & (yw < np.float64(H))
        warp = ~sensor & ~timed & ~deep & ~ok
        xw, yw = np.where(ok, xw, 0.0), np.where(ok, yw, 0.0)          # checked before any conversion
        fx0, fy0 = np.floor(xw), np.floor(yw)
        x0, y0 = fx0.astype(np.int64), fy0.astype(np.int64)
        a, b = xw - fx0, yw - fy0
        oa, ob = 1.0 - a, 1.0 - b
        s = np.where(pol | (not signed), 1.0, -1.0)
        ws = [oa * ob, a * ob, oa * b, a * b]
        iwe = np.zeros(H * W, dtype=np.int64)
        cells, inside = [], []
        for c in range(4):
            px, py = x0 + (c & 1), y0 + (c >> 1)
            ins = ok & (px >= 0) & (px < W) & (py >= 0) & (py < H)
            cell = np.where(ins, py * W + px, 0)
            q = np.rint(ws[c] * _TWO32).astype(np.int64)
            q = np.where(s < 0, -q, q)
            np.add.at(iwe, cell[ins], q[ins])
            cells.append(cell)
            inside.append(ins)
        iwe = iwe.reshape(H, W)
        J = _blur(iwe.astype(np.float64) * np.float64(1.0 / _TWO32), taps)
        npix = np.float64(H * W)
        mu = np.float64(tree_sum(J)) / npix
        C = J - mu
        f = np.float64(tree_sum(C * C)) / npix
        stats = np.zeros(2 + P, dtype=np.float64)
        stats[0], stats[1] = mu, f
        if want_grad:
            D = _blur(C, taps).reshape(-1)
            dwx, dwy = [-ob, ob, -b, b], [-oa, -a, oa, a]
            Gx, Gy = np.zeros(N, dtype=np.float64), np.zeros(N, dtype=np.float64)
            for c in range(4):
                d = D[cells[c]]
                Gx = Gx + np.where(inside[c], d * dwx[c], 0.0)
                Gy = Gy + np.where(inside[c], d * dwy[c], 0.0)
            scale = np.float64(2.0) / npix
            for k in range(P):
                g = np.where(ok, s * (Gx * (mx * Bu[k]) + Gy * (my * Bv[k])), 0.0)
                stats[2 + k] = scale * np.float64(tree_sum(g))
    dropped = np.array([int(timed.sum()), int(sensor.sum()), int(warp.sum())] + ([int(deep.sum())] if model == 'rigid' else []),
                       dtype=np.int64)
    if reg is None:
        return iwe, J, stats, dropped
    reg_stats = np.zeros(2 + P, dtype=np.float64)
    M = N - int(dropped.sum())
    reg_stats[1] = np.float64(M)
    if model != 'flow' and M > 0:
        with np.errstate(all='ignore'):
            rho_, vz = (rho, th[5]) if model == 'rigid' else (zero, np.float64(0.0))      # 'rotation': the rho = 0 case
            one = zero + 1.0
            c11 = (v * th[0] - (2.0 * u) * th[1]) + rho_ * vz
            c22 = ((2.0 * v) * th[0] - u * th[1]) + rho_ * vz
            c12 = u * th[0] + th[2]
            c21 = -(v * th[1]) - th[2]
            e11, e22 = [v, -(2.0 * u), zero, zero, zero, rho_], [2.0 * v, -u, zero, zero, zero, rho_]
            e12, e21 = [u, zero, one, zero, zero, zero], [zero, -v, -one, zero, zero, zero]
            dt2, deform = dt * dt, reg == 'deformation'
            d = -(dt * (c11 + c22))
            if deform:
                d = d + dt2 * (c11 * c22 - c12 * c21)
            Mf = np.float64(M)
            reg_stats[0] = np.float64(tree_sum(np.where(ok, np.abs(d), 0.0))) / Mf
            if want_grad:
                sg = np.where(d > 0.0, 1.0, np.where(d < 0.0, -1.0, 0.0))
                for k in range(P):
                    dd = -(dt * (e11[k] + e22[k]))
                    if deform:
                        dd = dd + dt2 * ((e11[k] * c22 + c11 * e22[k]) - (e12[k] * c21 + c12 * e21[k]))
                    reg_stats[2 + k] = np.float64(tree_sum(np.where(ok, sg * dd, 0.0))) / Mf
    return iwe, J, stats, dropped, reg_stats


def _evaluate(stream, H, W, calib, model, theta, t_ref, taps, signed, want_grad, want_blurred=False, depth=None, reg=None):
    """(iwe, blurred or None, stats, dropped) as CPU tensors / numpy, from the route of the stream's device; with reg also
    reg_stats (numpy)"""
    cal = calib_tuple(calib)
    more = {} if reg is None else dict(reg=reg)
    if stream.device.type == 'cuda':
        from . import functional as EF
        iwe, J, stats, dropped, *rs = EF.event_cmax_eval(*stream.arrays(), H, W, cal, model, theta, t_ref, taps, signed=signed,
                                                         want_grad=want_grad, want_blurred=want_blurred, depth=depth, **more)
        return (iwe, J, stats.cpu().numpy(), dropped.cpu().numpy()) + tuple(r.cpu().numpy() for r in rs)
    iwe, J, stats, dropped, *rs = cmax_numpy(*stream.numpy(), H, W, cal, model, theta, t_ref, taps, signed=signed, want_grad=want_grad,
                                             depth=depth, **more)
    return (torch.from_numpy(iwe), torch.from_numpy(J), stats, dropped) + tuple(rs)


def default_t_ref(stream):
    """The middle of the stream's time window: (min t + max t) / 2 over the finite stamps, 0 for an empty stream"""
    t = stream.t[torch.isfinite(stream.t)]
    if t.numel() == 0:
        return 0.0
    return 0.5 * (float(t.min()) + float(t.max()))


def warp_image(stream, calib, model, theta, H, W, t_ref=None, sigma=1.5, ksize=None, signed=False, with_dropped=False,
               depth=None):
    """(IWE float64 [H,W], blurred IWE float64 [H,W]) of the stream under the motion, on the stream's device; with_dropped also
    the dict of drop counters.  theta = zeros gives the uncompensated event image.  depth: the image of 'rigid'."""
    t_ref = default_t_ref(stream) if t_ref is None else float(t_ref)
    iwe, J, _, dropped = _evaluate(stream, int(H), int(W), calib, model, theta, t_ref, blur_taps(sigma, ksize), signed, False, True,
                                   depth=depth)
    img = iwe.to(torch.float64) * (1.0 / _TWO32)
    names = DROPPED_RIGID if model == 'rigid' else DROPPED
    return (img, J, dict(zip(names, (int(v) for v in dropped)))) if with_dropped else (img, J)


def contrast(stream, calib, model, theta, H, W, t_ref=None, sigma=1.5, ksize=None, signed=False, depth=None, reg=None, reg_weight=0.0):
    """(f, grad): the variance of the blurred IWE and its gradient in theta (numpy float64 [P]).  With reg ('divergence' or
    'deformation'): (F, grad F) of F = f - reg_weight R, reg_weight an ABSOLUTE weight (estimate_motion's is relative)."""
    _check_reg(reg)
    t_ref = default_t_ref(stream) if t_ref is None else float(t_ref)
    if reg is None:
        stats = _evaluate(stream, int(H), int(W), calib, model, theta, t_ref, blur_taps(sigma, ksize), signed, True, depth=depth)[2]
        return float(stats[1]), stats[2:].copy()
    lam = _finite_weight(reg_weight)
    out = _evaluate(stream, int(H), int(W), calib, model, theta, t_ref, blur_taps(sigma, ksize), signed, True, depth=depth, reg=reg)
    return float(out[2][1]) - lam * float(out[4][0]), out[2][2:] - lam * out[4][2:]


def _finite_weight(w):
    w = float(w)
    if not math.isfinite(w):
        raise EnslamError(f"event_cmax: reg_weight must be finite (got {w})")
    return w


def regulariser(stream, calib, model, theta, H, W, t_ref=None, kind='divergence', depth=None):
    """(R, dR, M): the collapse regulariser of enslam_event_cmax_reg_eval at theta -- the mean over the M events that vote of
    the absolute divergence of the warp's flow ('divergence') or of |det(dx'/dx) - 1| ('deformation') -- and its gradient in
    theta (numpy float64 [P]).  An event's depth is held locally constant.  'flow' has R = 0 exactly."""
    if kind not in REGS:
        raise EnslamError(f"event_cmax: kind must be one of {list(REGS)} (got {kind!r})")
    t_ref = default_t_ref(stream) if t_ref is None else float(t_ref)
    rs = _evaluate(stream, int(H), int(W), calib, model, theta, t_ref, [1.0], False, True, depth=depth, reg=kind)[4]
    return float(rs[0]), rs[2:].copy(), int(rs[1])


def _largest_rho(depth):
    """the largest finite inverse depth among the valid pixels (finite, > 0) of a depth image; 1.0 when there is none"""
    d = torch.as_tensor(depth).detach().reshape(-1)
    rho = 1.0 / d[torch.isfinite(d) & (d > 0)].double()
    rho = rho[torch.isfinite(rho)]
    return float(rho.max()) if rho.numel() else 1.0


def estimate_motion(stream, calib, model, H, W, theta0=None, t_ref=None, sigma=1.5, ksize=None, signed=False, iters=40,
                    tol_px=1e-3, max_halvings=20, depth=None, reg=None, reg_weight=8.0):
    """Maximises the contrast over theta from theta0 (zeros): BFGS on the host in float64 with a backtracking line search
    whose every accepted step raises f (sufficient increase 1e-4 of the predicted one).  The first step, and every step after
    a reset of the curvature estimate, moves the fastest event of the window by one pixel.  Stops after `iters` accepted steps,
    when a step moves no event by more than tol_px pixels, or when the line search finds no increase along the gradient.
    Deterministic: the same (f, grad) give the same steps, so the device and the CPU route follow the same trace to the bit.
    depth: the image of 'rigid' (float32 [H, W] on the stream's device).
    Returns dict(theta=[P], trace=[f after every accepted step, trace[0] = f(theta0)], thetas=[theta after every accepted step],
    evals=the number of evaluations, t_ref=...).
    reg ('divergence' or 'deformation'): maximises F = f - lambda R instead, R the collapse regulariser (`regulariser`), with
    lambda = reg_weight f(theta0) fixed at the first evaluation (reg_weight itself where f(theta0) == 0), so that the weight
    does not scale with the number of events.  `trace` then holds F, and the result also has f_trace, reg_trace (f and R beside
    every entry of trace) and reg_weight_abs = lambda; the step rules are the same.  R is an L1 term with a kink where an
    event's divergence changes sign -- at theta = 0 for every event at once: a weight so large that no step from theta0 raises
    F returns theta0 (the dead zone; about 16 on the 45 x 61 planted streams of the tests, where 4 - 8 recovers the motion)."""
    if model not in MODELS:
        raise EnslamError(f"event_cmax: model must be one of {sorted(MODELS)} (got {model!r})")
    _check_reg(reg)
    rel_weight = _finite_weight(reg_weight) if reg is not None else 0.0
    P = MODELS[model]
    fx, fy, cx, cy = calib_tuple(calib)
    H, W = int(H), int(W)
    t_ref = default_t_ref(stream) if t_ref is None else float(t_ref)
    taps = blur_taps(sigma, ksize)
    theta = np.zeros(P) if theta0 is None else np.array([float(v) for v in theta0], dtype=np.float64)
    if theta.shape != (P,):
        raise EnslamError(f"event_cmax: model {model!r} takes {P} parameters (got {theta.shape})")
    if (depth is None) != (model != 'rigid'):
        raise EnslamError(f"event_cmax: depth is required for 'rigid' and refused for the other models (model {model!r})")
    tf = stream.t[torch.isfinite(stream.t)]
    half = max(float((tf - t_ref).abs().max()), 1e-12) if tf.numel() else 1.0
    # pixels an event at the window's end moves per unit of each parameter (rotation: at the image corner, first order)
    if model == 'flow':
        px_per = np.array([half, half])
    else:
        um, vm = max(abs(cx), abs(W - 1 - cx)) / abs(fx), max(abs(cy), abs(H - 1 - cy)) / abs(fy)
        px_per = half * np.array([abs(fy) * (1 + vm * vm) + abs(fx) * um * vm, abs(fx) * (1 + um * um) + abs(fy) * um * vm,
                                  abs(fx) * vm + abs(fy) * um])
        if model == 'rigid':                                # translation: the nearest valid pixel, as if it sat at the corner
            rho = _largest_rho(depth)
            px_per = np.concatenate([px_per, half * rho * np.array([abs(fx), abs(fy), abs(fx) * um + abs(fy) * vm])])
    evals = [0]
    lam, parts = [None], {}                                 # lambda; (f, R) of the last evaluation

    def fg(th):
        evals[0] += 1
        if reg is None:
            st = _evaluate(stream, H, W, (fx, fy, cx, cy), model, th.tolist(), t_ref, taps, signed, True, depth=depth)[2]
            return float(st[1]), st[2:].astype(np.float64)
        out = _evaluate(stream, H, W, (fx, fy, cx, cy), model, th.tolist(), t_ref, taps, signed, True, depth=depth, reg=reg)
        st, rs = out[2], out[4]
        if lam[0] is None:
            lam[0] = rel_weight * float(st[1]) if float(st[1]) != 0.0 else rel_weight
        parts['last'] = (float(st[1]), float(rs[0]))
        return float(st[1]) - lam[0] * float(rs[0]), st[2:].astype(np.float64) - lam[0] * rs[2:].astype(np.float64)

    f, g = fg(theta)
    trace, thetas = [f], [theta.tolist()]
    f_trace, reg_trace = ([parts['last'][0]], [parts['last'][1]]) if reg is not None else (None, None)
    Hinv = None
    for _ in range(int(iters)):
        if not np.all(np.isfinite(g)) or not np.any(g != 0.0):
            break
        fresh = Hinv is None
        if fresh:
            d = g / (px_per * px_per)                       # steepest ascent in pixel units ...
            d = d / float(np.max(np.abs(d) * px_per))       # ... scaled to one pixel for the fastest event
        else:
            d = Hinv @ g
            if not (float(d @ g) > 0.0) or not np.all(np.isfinite(d)):
                Hinv = None
                continue
        slope = float(d @ g)
        alpha, accepted = 1.0, None
        for _h in range(int(max_halvings)):
            cand = theta + alpha * d
            fc, gc = fg(cand)
            if math.isfinite(fc) and fc > f and fc >= f + 1e-4 * alpha * slope:
                accepted = (cand, fc, gc)
                kept = parts.get('last')
                break
            alpha *= 0.5
        if accepted is None:
            if fresh:
                break
            Hinv = None
            continue
        cand, fc, gc = accepted
        sv, yv = cand - theta, g - gc                       # the curvature pair of -f
        sy = float(sv @ yv)
        if sy > 1e-12 * float(np.linalg.norm(sv)) * float(np.linalg.norm(yv)):
            if fresh:
                Hinv = np.eye(P) * (sy / float(yv @ yv))
            rho = 1.0 / sy
            V = np.eye(P) - rho * np.outer(sv, yv)
            Hinv = V @ Hinv @ V.T + rho * np.outer(sv, sv)
        else:
            Hinv = None
        moved = float(np.max(np.abs(sv) * px_per))
        theta, f, g = cand, fc, gc
        trace.append(f)
        thetas.append(theta.tolist())
        if reg is not None:
            f_trace.append(kept[0])
            reg_trace.append(kept[1])
        if moved < tol_px:
            break
    res = dict(theta=theta.tolist(), trace=trace, thetas=thetas, evals=evals[0], t_ref=t_ref)
    if reg is not None:
        res.update(f_trace=f_trace, reg_trace=reg_trace, reg_weight_abs=lam[0])
    return res


def relative_rotation(omega, dt):
    """The 4 x 4 delta D with c2w(t + dt) = c2w(t) @ D for a camera that turns with angular velocity omega (rad / s, in the
    PINHOLE frame, what estimate_motion('rotation') returns) for dt seconds, in the project's camera convention (y up, looking
    down -z).  Exact rotation (Rodrigues), float64."""
    w = np.array(from_pinhole(omega), dtype=np.float64) * float(dt)
    ang = float(np.linalg.norm(w))
    Kx = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    if ang < 1e-12:
        R = np.eye(3) + Kx
    else:
        R = np.eye(3) + (math.sin(ang) / ang) * Kx + ((1.0 - math.cos(ang)) / (ang * ang)) * (Kx @ Kx)
    out = np.eye(4)
    out[:3, :3] = R
    return torch.from_numpy(out)


def angular_velocity(c2w_a, c2w_b, dt):
    """The inverse of relative_rotation: the constant angular velocity (pinhole frame, rad / s) that turns pose a into pose b
    in dt seconds -- what a pair of ground-truth or tracked poses implies."""
    Ra = np.asarray(torch.as_tensor(c2w_a).double().cpu())[:3, :3]
    Rb = np.asarray(torch.as_tensor(c2w_b).double().cpu())[:3, :3]
    R = Ra.T @ Rb
    ang = math.acos(min(1.0, max(-1.0, (float(np.trace(R)) - 1.0) / 2.0)))
    axis = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    w = 0.5 * axis if ang < 1e-9 else axis * (ang / (2.0 * math.sin(ang)))
    return to_pinhole(w / float(dt))


def _skew(w):
    return np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])


def relative_motion(theta, dt):
    """The 4 x 4 delta D with c2w(t + dt) = c2w(t) @ D for a camera that moves with the constant body velocity theta = (w, v)
    (rad / s and depth units / s in the PINHOLE frame, what estimate_motion('rigid') returns) for dt seconds, in the project's
    camera convention: the flip of to_pinhole applies to w and to v alike.  The exact SE(3) exponential in float64; its
    rotation block is relative_rotation(w, dt)'s."""
    th = [float(x) for x in theta]
    if len(th) != 6:
        raise EnslamError(f"event_cmax: relative_motion takes (w_x, w_y, w_z, v_x, v_y, v_z) (got {len(th)} numbers)")
    w = np.array(from_pinhole(th[:3]), dtype=np.float64) * float(dt)
    v = np.array(from_pinhole(th[3:]), dtype=np.float64) * float(dt)
    ang = float(np.linalg.norm(w))
    Kx = _skew(w)
    if ang < 1e-12:
        V = np.eye(3) + 0.5 * Kx
    else:
        V = np.eye(3) + ((1.0 - math.cos(ang)) / (ang * ang)) * Kx + ((ang - math.sin(ang)) / (ang * ang * ang)) * (Kx @ Kx)
    out = relative_rotation(th[:3], dt).numpy().copy()
    out[:3, 3] = V @ v
    return torch.from_numpy(out)


def camera_velocity(c2w_a, c2w_b, dt):
    """The inverse of relative_motion: the constant body velocity (w, v) in the pinhole frame that carries pose a into pose b
    in dt seconds (the SE(3) logarithm of a^-1 b over dt) -- what a pair of ground-truth or tracked poses implies."""
    def full(c):
        m = np.eye(4)
        m[:3] = np.asarray(torch.as_tensor(c).detach().double().cpu())[:3]
        return m
    A, B = full(c2w_a), full(c2w_b)
    D = np.linalg.inv(A) @ B
    w = np.array(from_pinhole(angular_velocity(A, B, 1.0)), dtype=np.float64)       # the rotation vector, project frame
    ang = float(np.linalg.norm(w))
    Kx = _skew(w)
    if ang < 1e-6:
        Vinv = np.eye(3) - 0.5 * Kx + (1.0 / 12.0) * (Kx @ Kx)
    else:
        half = 0.5 * ang
        Vinv = np.eye(3) - 0.5 * Kx + ((1.0 - half * math.cos(half) / math.sin(half)) / (ang * ang)) * (Kx @ Kx)
    v = Vinv @ D[:3, 3]
    return [c / float(dt) for c in to_pinhole(w)] + [c / float(dt) for c in to_pinhole(v)]
