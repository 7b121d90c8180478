"""Yardstick of the event-generation-model loss: written from the model's statement in include/enslam_hip.h (section "Event-
generation-model loss"), in float64 numpy, not from the library.  The blur is direct windows over explicitly reflected
indices, its adjoint an explicit scatter of every (pixel, tap) pair onto the pixel the reflection names.

`branch` (int [h,w]: +1, -1 or 0) fixes the hinge decision per pixel.  Without it the decision is the sign of the float64 d;
with the device's own decisions the prediction and the gradient are stated under them, so that a pixel whose d is a rounding
error away from 0 does not count as a disagreement (the training-mode BatchNorm tests treat ReLU the same way)."""
import numpy as np

LUMA = (0.299, 0.587, 0.114)


def gaussian_taps(k):
    """The normalised taps of event.gaussian_kernel1d, float64."""
    sigma = 0.3 * ((k - 1) * 0.5 - 1) + 0.8
    x = np.linspace(-(k - 1) * 0.5, (k - 1) * 0.5, k)
    pdf = np.exp(-0.5 * (x / sigma) ** 2)
    return pdf / pdf.sum()


def reflect(s, n):
    """Index of the reflect padding (no repeated border) for -(n - 1) <= s <= 2 (n - 1)."""
    if s < 0:
        return -s
    if s >= n:
        return 2 * (n - 1) - s
    return s


def blur_axis(a, taps, axis, padding='reflect'):
    """out[q] = sum_t taps[t] a[reflect(q + t - R)] along `axis` ('zero': positions outside the array contribute nothing)."""
    a = np.moveaxis(np.asarray(a, np.float64), axis, 0)
    n, R = a.shape[0], len(taps) // 2
    assert R < n, "reflect padding is undefined for k // 2 >= n"
    out = np.zeros_like(a)
    for q in range(n):
        for t, tap in enumerate(taps):
            s = q + t - R
            if padding == 'zero':
                if 0 <= s < n:
                    out[q] += tap * a[s]
            else:
                out[q] += tap * a[reflect(s, n)]
    return np.moveaxis(out, 0, axis)


def blur_axis_adjoint(v, taps, axis):
    """The adjoint of blur_axis: every product taps[t] v[q] is scattered onto the pixel reflect(q + t - R) it was read from."""
    v = np.moveaxis(np.asarray(v, np.float64), axis, 0)
    n, R = v.shape[0], len(taps) // 2
    assert R < n
    out = np.zeros_like(v)
    for q in range(n):
        for t, tap in enumerate(taps):
            out[reflect(q + t - R, n)] += tap * v[q]
    return np.moveaxis(out, 0, axis)


def blur(a, taps, padding='reflect'):
    """B a of an [h,w,c] image: rows (along w) first, then columns."""
    return blur_axis(blur_axis(a, taps, 1, padding), taps, 0, padding)


def blur_adjoint(v, taps):
    return blur_axis_adjoint(blur_axis_adjoint(v, taps, 0), taps, 1)


def luma_raw(a):
    a = np.asarray(a, np.float64)
    return (LUMA[0] * a[..., 0] + LUMA[1] * a[..., 1]) + LUMA[2] * a[..., 2]


def event_model(cur, prev, gt, c_neg, c_pos, eps, ksizes=(), weights=(), branch=None, variant=None):
    """dict of float64 arrays: d [h,w], branch, pred [h,w,2], r, terms [1 + K], loss, blur_r / blur_gt / blur_pred (lists),
    g_r = dloss/dr [h,w,2], scale [h,w] = 1 / (Y(cur) + eps) where Y was not clamped else 0, grad = dloss/dcur [h,w,3].
    `variant` builds one of three deliberately WRONG gradients / losses for the tests that show the tolerance can tell:
    'B_for_BT' (the blur in place of its adjoint), 'zero_pad' (zero padding in place of reflect), 'blur_pred_only' (the
    blurred term compares B pred with the raw gt)."""
    cur, prev, gt = (np.asarray(x, np.float64) for x in (cur, prev, gt))
    yc_raw = luma_raw(cur)
    yc, yp = np.maximum(yc_raw, 0.0), np.maximum(luma_raw(prev), 0.0)
    d = np.log(yc + eps) - np.log(yp + eps)
    if branch is None:
        branch = np.sign(d).astype(np.int64)
    branch = np.asarray(branch)
    pred = np.stack((np.where(branch < 0, -d / c_neg, 0.0), np.where(branch > 0, d / c_pos, 0.0)), axis=-1)
    r = pred - gt
    terms, g_r = [float((r ** 2).sum())], 2.0 * r
    blur_r, blur_gt, blur_pred = [], [], []
    pad = 'zero' if variant == 'zero_pad' else 'reflect'
    for k, wk in zip(ksizes, weights):
        taps = gaussian_taps(k)
        if variant == 'blur_pred_only':
            v = blur(pred, taps) - gt
        else:
            v = blur(r, taps, pad)
        blur_r.append(v)
        blur_gt.append(blur(gt, taps))
        blur_pred.append(blur(pred, taps))
        terms.append(float((v ** 2).sum()))
        if variant == 'B_for_BT':
            back = blur(v, taps)
        elif variant == 'zero_pad':
            back = blur(v, taps, 'zero')            # (the zero-padded blur with symmetric taps is its own adjoint)
        else:
            back = blur_adjoint(v, taps)
        g_r = g_r + 2.0 * wk * back
    loss = terms[0] + sum(wk * t for wk, t in zip(weights, terms[1:]))
    scale = np.where(yc_raw >= 0.0, 1.0 / (yc + eps), 0.0)
    g_d = np.where(branch > 0, g_r[..., 1] / c_pos, 0.0) - np.where(branch < 0, g_r[..., 0] / c_neg, 0.0)
    grad = (g_d * scale)[..., None] * np.asarray(LUMA)
    return dict(d=d, branch=branch, pred=pred, r=r, terms=np.asarray(terms), loss=float(loss), blur_r=blur_r, blur_gt=blur_gt,
                blur_pred=blur_pred, g_r=g_r, scale=scale, grad=grad)
