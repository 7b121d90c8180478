"""Float64 yardstick (numpy only) of the tracker's fused loss tail, ens_launch_tracker_tail of csrc/render_fwd.hip
(tracker_composite_kernel, tracker_loss_kernel, tracker_median_wg): Tracker.py:179-195 of the reference on top of the occupancy
compositing, with the `handle_dynamic` median mask, d(loss)/d(raw) for a unit loss gradient and the set of active tiles.
Built on tests/composite_numpy.py (the compositing, its backward and their bars) and tests/step_numpy.py (the loss's float32
colour statements).

THE STATEMENTS (gd, gc as the float32 numbers they are; everything else float64):
    depth, var, rgb = composite_numpy.forward(raw, z)
    tmp  = |gd - depth| / sqrt(var + 1e-10)
    med  = the LOWER middle element of tmp over the inside rays (sorted[(c - 1) // 2] of the c inside values, gd == 0 ones
           included: torch.median over the rays that passed the prefilter); +inf when there are none
    keep = inside & (tmp < 10 med)           (strict; handle_dynamic off: keep = inside)
    on   = keep & (gd > 0)
    loss = sum_on tmp + w sum_on |gc - rgb|
    d_raw = composite_numpy.backward(g_depth = sign(depth - gd) / sqrt(var + 1e-10) on the `on` rays, g_var = 0 -- the variance
            is detached, Tracker.py:179 --, g_rgb = -w sign(gc - rgb) on the `on` rays); rows of zeros elsewhere.

error_model (u = 2^-24 as in composite_numpy.error_model, v = 2^-53; nothing below is fitted to a run):

  depth', var', rgb': the kernels composite exactly as composite_fwd_kernel does, so composite_numpy.forward_bars applies:
          |depth' - depth| <= dbar, |var' - var| <= vbar, |rgb' - rgb| <= rbar; var' >= 0 (a sum of non-negative terms).
  tmp' = |gd - depth'| / sqrt(var' + 1e-10) in float64: with a = |gd - depth| and r^2 = var + 1e-10,
          tmp' lies in [ max(a - dbar, 0) / sqrt(r^2 + vbar),  (a + dbar) / sqrt(max(var - vbar, 0) + 1e-10) ] (1 +- 8v):
          the propagation of the two bars through the quotient.  Its first order is dbar / r + tmp vbar / (2 r^2); the interval
          is used as it stands because on closed rays vbar is not small against r^2 = 1e-10 + a variance of the same size, and a
          first-order bar would not be a bound there.  tbar = the larger distance of the interval's ends from tmp.
  isd' = 1 / sqrt(var' + 1e-10): relative error  ri = sqrt(r^2 / (max(var - vbar, 0) + 1e-10)) - 1 + 8v  (the lower end of var'
          is the larger deviation, 1/sqrt being convex).
  loss:   every term of an `on` ray is off by at most tbar + w (sum_channels rbar + 4u sum_channels |gc - rgb|)  (three float32
          subtractions, two float32 adds, then float64), and the float64 sum of <= 4096 + 16 terms in any order adds
          (n + 16) v sum |terms|.  This presumes the device's `on` is the yardstick's: the fragility rule below.
  d_raw:  with the signs decided, the device's cotangents are g_rgb exactly and g_depth (1 + rho), |rho| <= ri.  The backward is
          linear in g_depth, so d_raw' = float32 evaluation of backward(g_depth (1 + rho), g_rgb), off from backward(g_depth,
          g_rgb) by at most
              bar = backward_bars(g_depth, 0, g_rgb) (1 + ri)  +  ri * scale of backward_bars(g_depth alone)
          (the first term: the float32 evaluation error, which grows with the cotangent by at most (1 + ri); the second: the
          exact change, rho times the depth part, bounded by its abs-sum scale).  The colour columns g_rgb w do not depend on
          g_depth and keep their bar.

THE FRAGILITY RULE.  An order statistic is 1-Lipschitz in the sup norm: if every |tmp'_i - tmp_i| <= B over the inside rays, the
k-th smallest of tmp' is within B of the k-th smallest of tmp.  So |med' - med| <= B = max_inside tbar, and
    a ray is DECIDED when |tmp_i - 10 med| > tbar_i + 10 B            (its keep bit is the same on the device),
    a sign is DECIDED when |gd - depth| > dbar, per channel |gc - rgb| > rbar.
The rule is asked of EVERY ray of a batch (inside or not, whatever its gd) and the signs of every ray with gd > 0 (no sign is
taken of a ray with gd <= 0: it cannot be `on`).  `undecided` counts the rays and signs that miss it; the cases need 0."""
import numpy as np

from tests import composite_numpy as Y
from tests import step_numpy as SN

U = Y.U
V = 2.0 ** -53
EPS = 1e-10


def lower_median(v, *, upper=False):
    """the lower middle element of v (torch.median), +inf for an empty v; upper: the variant"""
    v = np.sort(np.asarray(v, np.float64))
    if v.size == 0:
        return np.inf
    return float(v[v.size // 2] if upper else v[(v.size - 1) // 2])


def decide(tmp, gd, inside, dynamic=True, *, upper=False, le=False, over='inside', factor=10.0):
    """(med, keep, on) from given tmp.  The keyword switches are the sensitivity variants: the upper median, <=, the median
    over 'all' rays / over the 'gdpos' rays (gd > 0, the mask ignored) / 'gdfirst' (inside & gd > 0: gd > 0 applied before the
    median), another factor."""
    tmp = np.asarray(tmp, np.float64)
    gd = np.asarray(gd, np.float32)
    ins = np.ones(tmp.shape, bool) if inside is None else np.asarray(inside).astype(bool)
    pool = {'inside': ins, 'all': np.ones_like(ins), 'gdpos': gd > 0, 'gdfirst': ins & (gd > 0)}[over]
    med = lower_median(tmp[pool], upper=upper)
    if dynamic:
        with np.errstate(invalid='ignore'):
            keep = ins & ((tmp <= factor * med) if le else (tmp < factor * med))
    else:
        keep = ins.copy()
    return med, keep, keep & (gd > 0)


def given_loss(tmp, rgb, gd, gc, w, on):
    """the loss of the loss_only route on arrays the caller chose: sum_on tmp + (double) w (double) c, c the float32 colour L1"""
    terms = np.where(on, np.asarray(tmp, np.float64), 0.0)
    if gc is not None:
        c = SN._color_l1(rgb, gc).astype(np.float64)
        terms = np.concatenate([terms, np.where(on, float(np.float32(w)) * c, 0.0)])
    return float(terms.sum()), float(np.abs(terms).sum())


def tail(raw, z, gd, gc, w, inside, dynamic, *, fwd=None, detach=True, colour_masked=True, **decision):
    """The yardstick.  raw f32 [N,S,4], z f64 [N,S], gd f32 [N], gc f32 [N,3] or None, w the colour weight, inside bool/uint8 [N]
    or None, dynamic: handle_dynamic.  Returns a dict: f (composite_numpy.forward), depth, var, rgb, tmp, med, keep, on, loss,
    loss_abs, terms [N] (each ray's share of the loss), g_depth, g_rgb, d_raw [N,S,4], tiles (S % 16 == 0, else None).
    fwd: a forward dict in place of the yardstick's; detach / colour_masked / **decision (see decide): sensitivity variants."""
    raw = np.asarray(raw, np.float32)
    z = np.asarray(z, np.float64)
    N, S = z.shape
    f = Y.forward(raw, z) if fwd is None else fwd
    g32 = np.asarray(gd, np.float32)
    g = g32.astype(np.float64)
    dep, var, rgb = f['depth'], f['var'], f['rgb']
    root = np.sqrt(var + EPS)
    tmp = np.abs(g - dep) / root
    med, keep, on = decide(tmp, g32, inside, dynamic, **decision)
    terms = np.where(on, tmp, 0.0)
    g_depth = np.where(on, SN._sign_grad(g32, dep, 1.0) / root, 0.0)
    g_var = None if detach else np.where(on, -0.5 * np.abs(g - dep) / (root * (var + EPS)), 0.0)
    g_rgb = None
    wc = float(np.float32(w))
    if gc is not None:
        dc = np.asarray(gc, np.float32).astype(np.float64) - rgb
        con = on if colour_masked else np.ones_like(on)
        terms = terms + np.where(con, wc * np.abs(dc).sum(-1), 0.0)
        g_rgb = np.where(con[:, None], -wc * np.sign(dc), 0.0)
    d_raw = Y.backward(raw, z, g_depth, g_var, g_rgb, f=f)
    return dict(f=f, depth=dep, var=var, rgb=rgb, tmp=tmp, med=med, keep=keep, on=on, loss=float(terms.sum()),
                loss_abs=float(np.abs(terms).sum()), terms=terms, g_depth=g_depth, g_rgb=g_rgb, d_raw=d_raw,
                tiles=Y.active_tiles(d_raw, S) if S % 16 == 0 else None, gd=g, gc=gc, w=wc,
                inside=np.ones(N, bool) if inside is None else np.asarray(inside).astype(bool), dynamic=bool(dynamic))


def bars(t):
    """dict over depth, var, rgb, tmp, loss (a float), d_raw and d_scale [N,S,4] (bar and scale of d_raw), B, decided [N],
    undecided (int): see error_model and THE FRAGILITY RULE"""
    f = t['f']
    scales, fb, _ = Y.forward_bars(f)
    dep, var, g = t['depth'], t['var'], t['gd']
    dbar, vbar, rbar = fb['depth'], fb['var'], fb['rgb']
    a = np.abs(g - dep)
    r2 = var + EPS
    lo2 = np.maximum(var - vbar, 0.0) + EPS
    t_hi = (a + dbar) / np.sqrt(lo2) * (1 + 8 * V)
    t_lo = np.maximum(a - dbar, 0.0) / np.sqrt(r2 + vbar) * (1 - 8 * V)
    tbar = np.maximum(t_hi - t['tmp'], t['tmp'] - t_lo)
    ri = np.sqrt(r2 / lo2) - 1.0 + 8 * V
    on, ins = t['on'], t['inside']
    N = dep.shape[0]
    per_ray = tbar.copy()
    sign_ok = a > dbar
    if t['gc'] is not None:
        dc = np.abs(np.asarray(t['gc'], np.float32).astype(np.float64) - t['rgb'])
        per_ray = per_ray + t['w'] * (rbar.sum(-1) + 4 * U * dc.sum(-1))
        sign_ok = sign_ok & (dc > rbar).all(-1)
    loss_bar = float(per_ray[on].sum() + (N + 16) * V * t['loss_abs']) * (1.0 + 1e-9) + 1e-300
    scale, bar = Y.backward_bars(f, t['g_depth'], None, t['g_rgb'])
    dscale, _ = Y.backward_bars(f, t['g_depth'], None, None)
    bar = bar * (1.0 + ri)[:, None, None]
    bar[..., 3] = bar[..., 3] + (ri[:, None] * dscale[..., 3]) * (1.0 + 1e-9)
    B = float(tbar[ins].max()) if ins.any() else 0.0
    if t['dynamic'] and np.isfinite(t['med']):
        with np.errstate(invalid='ignore'):
            decided = np.abs(t['tmp'] - 10.0 * t['med']) > tbar + 10.0 * B
    else:                                             # no median (or no inside ray: nothing can be on)
        decided = np.ones(N, bool)
    undecided = int((~decided).sum() + ((g > 0) & ~sign_ok).sum())
    return dict(depth=dbar, var=vbar, rgb=rbar, tmp=tbar, loss=loss_bar, d_raw=bar, d_scale=scale, B=B, decided=decided,
                sign_ok=sign_ok, undecided=undecided, ri=ri, scales=scales)
