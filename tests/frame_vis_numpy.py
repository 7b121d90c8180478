"""Yardsticks of the frame report (csrc/frame_report.hip, evennicer_slam_amd/frame_vis.py), written from the rules the
header states and from nothing in the package:

  sheet(...)   the uint8 sheet, every pixel rule one numpy float32 operation at a time
  stats(...)   the four sums and the sums of their absolute terms, each term float64, added exactly (math.fsum)
  ssim(...)    the SSIM map in float64 by direct 11 x 11 windows (one 121-term weighted sum per moment and pixel)

The plasma table is an argument: the tests hand over the committed one (and compare that with matplotlib separately)."""
import math

import numpy as np

F = np.float32


def max_depth(gt_depth):
    """the maximum of gt_depth with NaNs skipped (fmaxf)"""
    return F(np.fmax.reduce(np.asarray(gt_depth, F).reshape(-1)))


def depth_rgb(v, maxd, lut):
    """uint8 [...,3] of float32 depths v against max_depth maxd"""
    v = np.asarray(v, F)
    out = np.empty(v.shape + (3,), np.uint8)
    if maxd == 0:
        out[...] = lut[0]
        return out
    with np.errstate(all='ignore'):
        u = v / F(maxd)
    nan = np.isnan(u)
    low, high = u < 0, u >= 1
    mid = ~(nan | low | high)
    idx = np.zeros(v.shape, np.int64)
    idx[mid] = (u[mid] * F(256.0)).astype(np.int64)              # truncation of a float32 product
    idx[high] = 255
    assert idx.min() >= 0 and idx.max() <= 255
    out[...] = lut[idx]
    out[nan] = 255
    return out


def clip01(c):
    c = np.asarray(c, F)
    c = np.where(c > 0, c, F(0))                                 # a NaN fails the comparison: 0
    return np.where(c < 1, c, F(1)).astype(F)


def color_level(c):
    return (clip01(c) * F(255.0) + F(0.5)).astype(np.uint8)


def event_level(e):
    v = np.asarray(e, F) * F(50.0)
    v = np.where(v > 0, v, F(0))
    v = np.where(v < 255, v, F(255))
    return v.astype(np.uint8)


def nearest_source(n_out, n_src):
    """source index of every panel index: ((2 i + 1) n_src) // (2 n_out)"""
    return np.array([((2 * i + 1) * n_src) // (2 * n_out) for i in range(n_out)], np.int64)


def event_rgb(e, H, W):
    lv = event_level(e)
    ys, xs = nearest_source(H, lv.shape[0]), nearest_source(W, lv.shape[1])
    out = np.zeros((H, W, 3), np.uint8)
    out[..., 0] = lv[..., 0][np.ix_(ys, xs)]
    out[..., 1] = lv[..., 1][np.ix_(ys, xs)]
    return out


def sheet(gt_depth, gt_color, depth, color, lut, gt_event=None, pred_event=None, gutter=8, title=16):
    gd, gc, d, c = (np.asarray(a, F) for a in (gt_depth, gt_color, depth, color))
    H, W = gd.shape
    R = 2 if gt_event is None else 3
    g, t = gutter, title
    out = np.full((R * H + (R + 1) * g + R * t, 3 * W + 4 * g, 3), 255, np.uint8)
    maxd = max_depth(gd)
    with np.errstate(invalid='ignore'):
        d_res = np.abs(gd - d).astype(F)
        c_res = np.abs(gc - c).astype(F)
    d_res[gd == 0] = 0
    c_res[gd == 0] = 0
    panels = {(0, 0): depth_rgb(gd, maxd, lut), (0, 1): depth_rgb(d, maxd, lut), (0, 2): depth_rgb(d_res, maxd, lut),
              (1, 0): color_level(gc), (1, 1): color_level(c), (1, 2): color_level(c_res)}
    if R == 3:
        a, b = event_rgb(gt_event, H, W), event_rgb(pred_event, H, W)
        panels[(2, 0)], panels[(2, 1)] = a, b
        panels[(2, 2)] = np.abs(a.astype(np.int32) - b.astype(np.int32)).astype(np.uint8)
    for (r, k), img in panels.items():
        y0, x0 = g + t + r * (H + g + t), g + k * (W + g)
        out[y0:y0 + H, x0:x0 + W] = img
    return out


def stats(gt_depth, gt_color, depth, color):
    """float64 [8]: n_valid, sum |depth residual| over gt_depth > 0, sum of squared clipped colour error over all pixels and
    channels and over gt_depth > 0, then the sums of the absolute values of the same terms"""
    gd, gc, d, c = (np.asarray(a, F) for a in (gt_depth, gt_color, depth, color))
    valid = gd > 0
    with np.errstate(invalid='ignore'):
        l1 = np.abs(gd - d).astype(F)[valid].astype(np.float64)
    sq = (clip01(gc) - clip01(c)).astype(F).astype(np.float64) ** 2
    terms = [np.ones(int(valid.sum())), l1, sq.reshape(-1), sq[valid].reshape(-1)]
    return np.array([math.fsum(t) for t in terms] + [math.fsum(np.abs(t)) for t in terms], np.float64)


def window():
    k = np.arange(-5, 6, dtype=np.float64)
    g = np.exp(-(k * k) / (2.0 * 1.5 * 1.5))
    g /= g.sum()
    return np.outer(g, g)


def ssim(x, y):
    """(mean, map float64 [H-10,W-10,C]) of x, y [H,W,C] with values in [0, 1]"""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    if x.ndim == 2:
        x, y = x[..., None], y[..., None]
    w = window()
    C1, C2 = 0.01 ** 2, 0.03 ** 2
    view = np.lib.stride_tricks.sliding_window_view

    def moment(a):                                               # [H-10,W-10,C]: the 121 products of each window
        return np.einsum('ijcab,ab->ijc', view(a, (11, 11), axis=(0, 1)), w)

    ux, uy, uxx, uyy, uxy = moment(x), moment(y), moment(x * x), moment(y * y), moment(x * y)
    vx, vy, vxy = uxx - ux * ux, uyy - uy * uy, uxy - ux * uy
    m = ((2 * ux * uy + C1) * (2 * vxy + C2)) / ((ux * ux + uy * uy + C1) * (vx + vy + C2))
    return math.fsum(m.reshape(-1)) / m.size, m
