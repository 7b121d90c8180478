"""Seeded cases of the event-generation-model loss, the conditions they have to meet, and the tolerance rule.

Shapes are chosen by where the kernel can go wrong (csrc/event_model.hip: one workgroup per TILE x TILE tile and channel, a halo
of 2 (k // 2) in reflected coordinates): 5 x 5 and 5 x 7 with k = 9 put every pixel within reflect range of two borders; 5 x 300 is
one tile row by many tile columns; TILE - 1, TILE, TILE + 1 and 2 TILE + 1 appear in each dimension; 39 x 51 is the project's
small event resolution and the largest case.  k = 31 (the supported maximum) runs once.

THE TOLERANCE RULE is derived from the float32 operation counts, with u = 2^-24 (half an ulp of a rounded result), and is never
fitted to a device.  Inputs are float32 in every route, so they carry no error.
  Y      three products and two sums of non-negative terms, then the clamp: relative error <= 4 u
  log    the argument Y + eps adds one rounding (relative 5 u in all, which the logarithm turns into an ABSOLUTE 5 u); the
         function itself is taken as good to 2 ulp (LOG_ULP) of its value, at most |log eps|: 2 * 2 u |log eps|
  d      two logarithms and one difference: D_ERR = 2 (5 u + 4 u |log eps|) + u D_MAX, D_MAX = |log eps| + 1 bounding |d|
  pred   one division by float32(c) (c itself rounded: relative u): E_pred = D_ERR / c + 3 u max|pred|
  r      one difference with the exact gt: E_r = E_pred + u max|r|
  B x    two passes of k multiply-adds with taps rounded to float32; the taps are positive and sum to 1, so an input error
         passes through at most unchanged: E_B(x) = E_x + 2 (k + 2) u max|x|
  term   sum v^2 with |v - v'| <= E_v, squared and added in float64: |term - term'| <= 2 E_v sum|v| + N E_v^2
  g_r    2 r + sum_i 2 w_i B_i^T B_i r.  A column of B sums to at most 2 per dimension (a border pixel is read once directly and
         once through the reflection), so B^T amplifies by at most 4 in two dimensions:
         E_g = 2 E_r + sum_i 2 w_i (4 E_B(r) + 4 * 2 (k_i + 2) u max|B_i r| * 4) + 2 u max|g_r|
  grad   g_r w_ch / (c (Y + eps)): the factor carries Y's 5 u and three more roundings:
         E_grad = max_ch w_ch * max_p [ (E_g + 9 u |g_r|) / (c_min (Y + eps)) ]
Every bound is evaluated on the float64 reference of the case and quoted as a fraction of the tensor's maximum, the project's
convention.  The hinge: the device may decide the sign of d differently from float64 only where |d64| <= BRANCH_MARGIN = D_ERR,
and the gradient is compared under the device's decisions."""
import numpy as np

from tests import event_model_numpy as Y

TILE = 16                       # ENSLAM_EVENT_MODEL_TILE
MAX_KERNELS, MAX_KSIZE = 4, 31
U = 2.0 ** -24
LOG_ULP = 2.0
MAX_BRANCH_SHARE = 0.01


def d_err(eps):
    le = abs(np.log(eps))
    return 2.0 * (5.0 * U + 2.0 * LOG_ULP * U * le) + U * (le + 1.0)


def branch_margin(eps):
    return d_err(eps)


def _case(name, h, w, seed, ksizes=(9,), weights=(1.0,), c_neg=0.2, c_pos=0.2, eps=1e-3, kind='plain'):
    return dict(name=name, h=h, w=w, seed=seed, ksizes=tuple(ksizes), weights=tuple(weights), c_neg=c_neg, c_pos=c_pos, eps=eps,
                kind=kind)


T = TILE
CASES = [
    _case('5x5_k9', 5, 5, 1),
    _case('5x7_k9', 5, 7, 2),
    _case('5x300_k9', 5, 300, 3),
    _case('Tm1xT_k9', T - 1, T, 4),
    _case('TxTp1_k9', T, T + 1, 5),
    _case('Tp1xTm1_k9', T + 1, T - 1, 6),
    _case('2Tp1x2Tp1_K2', 2 * T + 1, 2 * T + 1, 7, ksizes=(5, 13), weights=(1.0, 0.5)),
    _case('Tm1x2Tp1_K0', T - 1, 2 * T + 1, 8, ksizes=(), weights=()),
    _case('2Tp1xTp1_k31', 2 * T + 1, T + 1, 9, ksizes=(31, 3), weights=(0.25, 2.0)),
    _case('39x51_k9', 39, 51, 10),
    _case('39x51_c', 39, 51, 11, c_neg=0.35, c_pos=0.15),
    _case('39x51_K2', 39, 51, 12, ksizes=(9, 5), weights=(1.0, 0.3), c_neg=0.25, c_pos=0.2),
    _case('Tp1xTp1_dark', T + 1, T + 1, 13, kind='dark'),
    _case('TxTm1_tie', T, T - 1, 14, kind='tie'),
    _case('5x7_tie', 5, 7, 15, kind='tie'),
    _case('Tp1xT_negative', T + 1, T, 16, kind='negative'),
]
BORDER_CASES = ('5x5_k9', '5x7_k9')
TIE_BLOCK = (slice(1, 4), slice(2, 5))         # rows, columns of the planted block of the 'tie' cases


def inputs(case):
    """cur, prev [h,w,3] and gt [h,w,2] as float32 arrays, from the case's seed alone."""
    rng = np.random.default_rng(case['seed'])
    h, w = case['h'], case['w']
    prev = rng.random((h, w, 3))
    cur = np.clip(prev + 0.25 * rng.standard_normal((h, w, 3)), 0.0, 1.0)
    gt = rng.integers(0, 4, (h, w, 2)).astype(np.float64)
    if case['kind'] == 'dark':                  # luminance of the order of eps: the steep end of the logarithm
        prev, cur = prev * 4e-3, cur * 4e-3
    prev, cur = prev.astype(np.float32), cur.astype(np.float32)
    if case['kind'] == 'tie':                   # d is exactly 0 there on every route: the same operations on the same numbers
        cur[TIE_BLOCK] = prev[TIE_BLOCK]
    if case['kind'] == 'negative':              # one colour below 0 with a negative luminance: the clamp
        cur[2, 3] = (-0.5, -0.25, 0.1)
    return cur, prev, gt.astype(np.float32)


def reference(case, branch=None, variant=None):
    cur, prev, gt = inputs(case)
    return Y.event_model(cur, prev, gt, case['c_neg'], case['c_pos'], case['eps'], case['ksizes'], case['weights'], branch, variant)


def bounds(case, ref):
    """The absolute error bounds of the rule above on the reference `ref` of `case`: dict with pred, blur_gt / blur_pred (per
    kernel), terms [1 + K], loss, g_r, grad."""
    amax = lambda a: float(np.abs(a).max()) if np.size(a) else 0.0
    c_min = min(case['c_neg'], case['c_pos'])
    e_pred = d_err(case['eps']) / c_min + 3.0 * U * amax(ref['pred'])
    e_r = e_pred + U * amax(ref['r'])
    e_blur = lambda e_x, x, k: e_x + 2.0 * (k + 2) * U * amax(x)
    n = ref['r'].size
    e_terms = [2.0 * e_r * float(np.abs(ref['r']).sum()) + n * e_r ** 2]
    e_g = 2.0 * e_r
    for k, wk, v in zip(case['ksizes'], case['weights'], ref['blur_r']):
        e_v = e_blur(e_r, ref['r'], k)
        e_terms.append(2.0 * e_v * float(np.abs(v).sum()) + n * e_v ** 2)
        e_g += 2.0 * wk * (4.0 * e_v + 4.0 * 4.0 * 2.0 * (k + 2) * U * amax(v))
    e_g += 2.0 * U * amax(ref['g_r'])
    e_loss = e_terms[0] + sum(wk * e for wk, e in zip(case['weights'], e_terms[1:]))
    g_mag = np.abs(ref['g_r']).max(axis=-1)
    e_grad = max(Y.LUMA) * float(((e_g + 9.0 * U * g_mag) * ref['scale']).max()) / c_min
    return dict(pred=e_pred, blur_gt=[e_blur(0.0, g, k) for k, g in zip(case['ksizes'], ref['blur_gt'])],
                blur_pred=[e_blur(e_pred, p, k) for k, p in zip(case['ksizes'], ref['blur_pred'])], terms=e_terms, loss=e_loss,
                g_r=e_g, grad=e_grad)


def fraction(err, ref):
    """`err` as a fraction of the maximum of |ref| (the form every bound is quoted in)."""
    m = float(np.abs(ref).max()) if np.size(ref) else 0.0
    return float(err) / m if m > 0 else (0.0 if err == 0 else float('inf'))
