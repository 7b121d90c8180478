"""Float64 yardstick (numpy only) of the occupancy compositing, raw2outputs_nerf_color as the kernels of csrc/render_fwd.hip
and csrc/render_bwd.hip define it (common.py:256-297, occupancy branch), of the mapper loss on top of it (Mapper.py:553-562),
and of the float32 rounding error such a kernel may make: scales, bars and the set of active tiles.

Forward.  x = 10 * occ is formed in float32 as the kernels (and the reference's float32 torch ops) form it; everything after
it is float64:  alpha = sigmoid(x),  1 - alpha = sigmoid(-x) (never a cancelling subtraction),  m = (1 - alpha) + c with c the
float32 value of 1e-10,  T = exclusive product of m,  w = alpha T,  depth = sum w z,  var = sum w (z - depth)^2,
rgb = sum w colour.

Backward with respect to raw, without a division (finite when m = c):
    d_colour_j = g_rgb w_j
    gw_j       = (g_depth - 2 g_var sum_k w_k tmp_k) z_j + g_var tmp_j^2 + g_rgb . colour_j        tmp = z - depth
    d_occ_j    = 10 alpha_j (1 - alpha_j) (gw_j T_j - sum_{k>j} gw_k alpha_k P_kj),     P_kj = prod_{i<k, i != j} m_i

Scales (as tests/imap_torch.py builds them): the abs-sum of the terms that form an output, each factor replaced by the
abs-sum that formed it.  Bars: a bound of what a float32 evaluation in the kernels' order can be off by, derived in
`error_model` below from per-operation errors; the constants are not fitted to any run."""
import numpy as np

U = 2.0 ** -24                       # float32 unit roundoff
C32 = float(np.float32(1e-10))       # the 1e-10 of the transmittance as float32 holds it
TINY = 2.0 ** -123                   # 8 * the smallest normal float32: what underflow can cost a product of <= 63 factors
F64 = 64 * 2.0 ** -53                # a float64 sum of <= 64 terms

error_model = """
Per-operation float32 errors (u = 2^-24; IEEE multiply, add and the correctly rounded divide each u relative; expf one ulp,
i.e. at most 2 u relative; the library is built without contraction, so there is no hidden fma):

  alpha' = 1 / (1 + expf(-x)):  relative error  ra = 2u (1 - alpha) + 2u   (expf's 2u enters through e / (1 + e) = 1 - alpha,
                                 then one add and one divide).
  (1 - alpha)' = 1.f - alpha':  ABSOLUTE error  doma = alpha ra + u (1 - alpha).  This is the granularity of float32 near 1.
  m' = (1 - alpha)' + 1e-10f:    absolute error  dm = alpha ra + 2u m,   relative  eps = dm / m + u  (the u: one multiply of
                                 the product chain per factor; a product of k factors takes k - 1 multiplies in any order).
  Closed ("exactly saturated") samples: where e = exp(-x) satisfies e (1 + 2u) < u (10 occ above 16.7), 1 + expf(-x) rounds to
                                 exactly 1, so alpha' = 1, (1 - alpha)' = 0 and m' = 1e-10f with NO rounding at all:
                                 ra = (1 - alpha) / alpha,  doma = dm = 1 - alpha  (0 for an out-of-bound sample's 100),  eps = dm / m + u.
                                 Without this branch the bar could not tell m = 1e-10 from m = 0 behind a closed sample.
  T'_j:   relative  E_j = prod_{i<j} (1 + eps_i) - 1  -- the full product, not its first order: where eps is near 1 (near-saturated
          samples) two such factors on one ray give a second-order term of the first order's size.
  w'_j:   wbar = w ((1 + E)(1 + ra)(1 + u) - 1) + TINY.   TINY = 2^-123 covers a product that leaves the normal range
          (flushed or denormal partial products: at most 2^-126 per level of the 6-level scan).
  depth:  float64 sum of float32 weights:  sum wbar |z| + 64 * 2^-53 sum w |z|.
  rgb:    float32 products and a 6-level float32 tree sum:  sum wbar |c| + 8u sum w |c|.
  var:    sum wbar tmp^2 + 2 dbar sum w |tmp| + dbar^2 sum w + float64 rounding   (dbar: the depth bar; tmp' = z - depth').

  Backward (depth as given to the kernel is exact here: the tests hand it the yardstick's):
  gw'_k:  the float64 part is rounded once to float32, the colour dot product takes 3 multiplies and 3 adds, and in the loss
          form the colour cotangent (float) g_loss * w_color is itself a rounded float32 product:
          dgw = 2 |g_var| (sum wbar |tmp|) |z| + 6u gwabs,   gwabs the abs-sum of gw's terms.
  d_occ'_j = 10 alpha' (1-alpha)' (gw' T' - suf' / m'),  suf' = (inclusive 6-level suffix scan of gw' w') - gw'_j w'_j.
          The division by m'_j removes the factor m'_j from every T'_k, k > j, up to u: term k is gw'_k alpha'_k P'_kj with
          relative error  e_kj = (1 + dgw/gwabs)(1 + ra_k)(prod_{i<k, i != j} (1 + eps_i))(1 + 8u) - 1,  and the leading term
          gw'_j T'_j has  e_jj = (1 + dgw/gwabs)(1 + E_j)(1 + 8u) - 1.   (8u: the products, the divide, the subtraction and the
          three final multiplies.)  The scan's own rounding, 7u sum_{k>=j} |gw'_k w'_k|, is divided by m'_j and multiplied by
          (1-alpha)'_j <= m'_j: it costs 7u (|gw_j| alpha_j T_j (1 + E_j) + ((1-alpha_j) + doma_j) sum_{k>j} |term k| (1 + e_kj)).
          A' = alpha' (1-alpha)' has absolute error dA = alpha doma + alpha (1-alpha) ra + 2u alpha (1-alpha).  Together:
          bar = 10 (dA G + (A + dA) dG + alpha (1 + ra) * scan) + 10 * 64 * TINY (1 + max gwabs),
          G = gwabs_j T_j + sum_{k>j} gwabs_k alpha_k P_kj  (the scale of d_occ is 10 G),  dG the same sum weighted by e.
  d_colour' = g_rgb w':  |g_rgb| wbar + u |g_rgb| w.
"""


def _sig(x):
    """sigmoid(x) in float64 without overflow"""
    e = np.exp(-np.abs(x))
    return np.where(x >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def _excl_cumprod(a, axis=-1):
    one = np.ones_like(np.take(a, [0], axis=axis))
    return np.cumprod(np.concatenate([one, a], axis=axis), axis=axis).take(range(a.shape[axis]), axis=axis)


def _pairs(m):
    """P[n, j, k] = prod_{i<k, i != j} m_i (any k; for k <= j this is T_k)"""
    N, S = m.shape
    mm = np.broadcast_to(m[:, None, :], (N, S, S)).copy()
    mm[:, np.arange(S), np.arange(S)] = 1.0
    return _excl_cumprod(mm, axis=2)


def alphas(raw, *, plus=C32):
    x = (np.float32(10.0) * np.asarray(raw, np.float32)[..., 3]).astype(np.float64)
    alpha, oma = _sig(x), _sig(-x)
    with np.errstate(over='ignore'):
        e = np.exp(-x)
    return alpha, oma, oma + plus, e


def forward(raw, z, *, inclusive=False, plus=C32):
    """dict(alpha, oma, m, T, w, depth, var, rgb) in float64.  raw [N,S,4] float32, z [N,S] float64.
    inclusive / plus exist for the sensitivity variants only."""
    raw = np.asarray(raw, np.float32)
    z = np.asarray(z, np.float64)
    alpha, oma, m, e = alphas(raw, plus=plus)
    T = np.cumprod(m, -1) if inclusive else _excl_cumprod(m)
    w = alpha * T
    col = raw[..., :3].astype(np.float64)
    depth = (w * z).sum(-1)
    tmp = z - depth[:, None]
    return dict(alpha=alpha, oma=oma, m=m, e=e, T=T, w=w, depth=depth, var=(w * tmp * tmp).sum(-1),
                rgb=(w[..., None] * col).sum(1), tmp=tmp, col=col, z=z)


def _cot(f, g_depth, g_var, g_rgb):
    N = f['z'].shape[0]
    gD = np.zeros(N) if g_depth is None else np.asarray(g_depth, np.float64)
    gV = np.zeros(N) if g_var is None else np.asarray(g_var, np.float64)
    gC = np.zeros((N, 3)) if g_rgb is None else np.asarray(g_rgb, np.float64)
    return gD, gV, gC


def backward(raw, z, g_depth=None, g_var=None, g_rgb=None, *, f=None, suffix_incl=False, no_depth_term=False,
             no_tmp2=False):
    """d_raw [N,S,4] float64 for any subset of the cotangents; never divides.  The keyword switches are the
    sensitivity variants (suffix sum including j, the -2 gV sum(w tmp) term dropped, g_var's tmp^2 term dropped)."""
    f = forward(raw, z) if f is None else f
    gD, gV, gC = _cot(f, g_depth, g_var, g_rgb)
    w, T, alpha, oma, tmp = f['w'], f['T'], f['alpha'], f['oma'], f['tmp']
    gDt = gD if no_depth_term else gD - 2.0 * gV * (w * tmp).sum(-1)
    gw = gDt[:, None] * f['z'] + (0.0 if no_tmp2 else gV[:, None] * tmp * tmp) + (gC[:, None, :] * f['col']).sum(-1)
    P = _pairs(f['m'])                                           # [n, j, k]
    S = w.shape[1]
    later = np.triu(np.ones((S, S), bool), 0 if suffix_incl else 1)[None]      # k > j  (k >= j in the variant)
    suf = (np.where(later, P, 0.0) * (gw * alpha)[:, None, :]).sum(-1)
    d = np.empty(w.shape + (4,))
    d[..., :3] = gC[:, None, :] * w[..., None]
    d[..., 3] = 10.0 * alpha * oma * (gw * T - suf)
    return d


def forward_bars(f):
    """(scales, bars): dicts over w, depth, var, rgb -- see error_model"""
    alpha, oma, m, T, w, z, tmp, col = (f[k] for k in ('alpha', 'oma', 'm', 'T', 'w', 'z', 'tmp', 'col'))
    closed = f['e'] * (1 + 2 * U) < U
    ra = np.where(closed, oma / np.maximum(alpha, 0.5), 2 * U * oma + 2 * U)
    doma = np.where(closed, oma, alpha * ra + U * oma)
    dm = np.where(closed, oma, alpha * ra + 2 * U * m)
    eps = dm / m + U
    # eps is at most ~1.2e3 (where m is the bare 1e-10), so 63 factors stay inside float64; where eps is ~1e-7 the
    # subtraction below keeps 9 digits
    E = _excl_cumprod(1.0 + eps) - 1.0
    wbar = w * ((1.0 + E) * (1.0 + ra) * (1.0 + U) - 1.0) + TINY
    s_depth = (w * np.abs(z)).sum(-1)
    dbar = (wbar * np.abs(z)).sum(-1) + F64 * s_depth
    s_rgb = (w[..., None] * np.abs(col)).sum(1)
    rbar = (wbar[..., None] * np.abs(col)).sum(1) + 8 * U * s_rgb
    s_var = (w * tmp * tmp).sum(-1)
    vbar = (wbar * tmp * tmp).sum(-1) + 2 * dbar * (w * np.abs(tmp)).sum(-1) + dbar * dbar * w.sum(-1) + 4 * F64 * s_var
    scales = dict(w=w, depth=s_depth, var=s_var, rgb=s_rgb)
    bars = dict(w=wbar, depth=dbar, var=vbar, rgb=rbar)
    return scales, bars, dict(ra=ra, dm=dm, doma=doma, eps=eps, E=E)


def backward_bars(f, g_depth=None, g_var=None, g_rgb=None):
    """(scale [N,S,4], bar [N,S,4]) of d_raw -- see error_model.  scale[..., 3] = 10 (gwabs_j T_j + sum_{k>j} gwabs_k alpha_k P_kj)."""
    gD, gV, gC = _cot(f, g_depth, g_var, g_rgb)
    alpha, oma, m, T, w, z, tmp, col = (f[k] for k in ('alpha', 'oma', 'm', 'T', 'w', 'z', 'tmp', 'col'))
    _, fb, aux = forward_bars(f)
    ra, eps, E, doma, wbar = aux['ra'], aux['eps'], aux['E'], aux['doma'], fb['w']
    S = w.shape[1]
    gDabs = np.abs(gD) + 2 * np.abs(gV) * (w * np.abs(tmp)).sum(-1)
    gwabs = gDabs[:, None] * np.abs(z) + np.abs(gV)[:, None] * tmp * tmp + (np.abs(gC)[:, None, :] * np.abs(col)).sum(-1)
    dgw = 2 * np.abs(gV)[:, None] * (wbar * np.abs(tmp)).sum(-1)[:, None] * np.abs(z) + 6 * U * gwabs
    rgw = np.where(gwabs > 0, dgw / np.where(gwabs > 0, gwabs, 1.0), 0.0)
    P = _pairs(m)
    Pe = _pairs(1.0 + eps)                                       # prod_{i<k, i != j} (1 + eps_i)
    later = np.triu(np.ones((S, S), bool), 1)[None]
    term = np.where(later, P, 0.0) * (gwabs * alpha)[:, None, :]                 # [n, j, k], k > j
    e_kj = (1.0 + rgw)[:, None, :] * (1.0 + ra)[:, None, :] * Pe * (1.0 + 8 * U) - 1.0
    e_jj = (1.0 + rgw) * (1.0 + E) * (1.0 + 8 * U) - 1.0
    G = gwabs * T + term.sum(-1)
    dG = gwabs * T * e_jj + (term * e_kj).sum(-1)
    A = alpha * oma
    dA = alpha * doma + A * ra + 2 * U * A
    scan = 7 * U * (gwabs * alpha * T * (1.0 + E) + (oma + doma) * (term * (1.0 + e_kj)).sum(-1))
    scale = np.empty(w.shape + (4,))
    bar = np.empty(w.shape + (4,))
    scale[..., 3] = 10.0 * G
    bar[..., 3] = 10.0 * (dA * G + (A + dA) * dG + alpha * (1.0 + ra) * scan) \
        + 10.0 * 64 * TINY * (1.0 + gwabs.max(-1))[:, None]
    scale[..., :3] = np.abs(gC)[:, None, :] * w[..., None]
    bar[..., :3] = np.abs(gC)[:, None, :] * wbar[..., None] + U * scale[..., :3]
    return scale, bar


def mapper_loss(f, gt_depth, gt_color=None, w_color=0.0):
    """The mapper's RGB-D loss on a forward result: sum_{gt_depth > 0} |gt_depth - depth| + w_color sum |gt_color - rgb|.
    Returns dict(loss, g_depth [N], g_rgb [N,3] or None: d loss / d depth, d rgb;  margin_depth [N] (inf on masked rays),
    margin_rgb [N,3]: the distance of every sign decision from its switch;  bar: what a float32 kernel's loss may be off by)."""
    gd = np.asarray(gt_depth, np.float32).astype(np.float64)
    keep = gd > 0
    diff = gd - f['depth']
    loss = np.abs(diff)[keep].sum()
    g_depth = np.where(keep, -np.sign(diff), 0.0)
    _, fb, _ = forward_bars(f)
    bar = fb['depth'][keep].sum() + F64 * np.abs(diff)[keep].sum()
    out = dict(g_depth=g_depth, g_rgb=None, margin_depth=np.where(keep, np.abs(diff), np.inf), margin_rgb=None)
    if gt_color is not None:
        wc = float(np.float32(w_color))
        dc = np.asarray(gt_color, np.float32).astype(np.float64) - f['rgb']
        loss = loss + wc * np.abs(dc).sum()
        out['g_rgb'] = -wc * np.sign(dc)
        out['margin_rgb'] = np.abs(dc)
        # three float32 subtractions, two adds and the multiply by w_color on top of the rgb bars
        bar = bar + wc * (fb['rgb'].sum() + 4 * U * np.abs(dc).sum())
    out['loss'], out['bar'] = float(loss), float(bar * (1.0 + 1e-9) + 1e-300)
    return out


def active_tiles(d_raw, S):
    """set of tile ids ray * S/16 + t whose 64 floats of d_raw [N,S,4] are not all zero (S a multiple of 16)"""
    d = np.asarray(d_raw).reshape(-1, S // 16, 64)
    ray, t = np.nonzero((d != 0).any(-1))
    return set((ray * (S // 16) + t).tolist())
