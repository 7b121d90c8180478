"""Seeded cases of the frame report (tests/test_frame_vis_cpu.py, tests/test_hip_frame_vis.py) with the conditions each is
there for asserted, and the tolerances of the comparisons, derived here.

Panels: a thread of the kernel owns 4 consecutive pixels of the flattened sheet and a workgroup 1024, so the sizes are chosen
by the sheet they give: 45 x 61 leaves a 2-pixel (two rows) and a 1-pixel (three rows) tail behind the last whole thread and
50 x 70 none; neither sheet is a multiple of 1024 pixels, in either axis or as a whole."""
import numpy as np

U = 2.0 ** -53

# Statistics: every term is a float64, the yardstick adds them exactly; the kernel's chain of additions for the sizes here is
# 4 (thread) + 6 (wave) + 2 (workgroup) + at most 46 workgroups in index order < 64 roundings of at most U * A each.
STATS_RTOL = 64 * U

# SSIM map.  Each of the five moments is a sum of 121 weighted products of values in [0, 1] with weights that add up to 1:
# |moment| <= 1 and its rounding error is below D = 256 U in any order, with or without FMA.  With S = (A1 A2) / (B1 B2),
#   A1 = 2 ux uy + C1,  B1 = ux^2 + uy^2 + C1 >= C1 = 1e-4,   |A1| <= B1
#   A2 = 2 vxy + C2,    B2 = vx + vy + C2    >= C2 = 9e-4,   |A2| <= B2  (Cauchy-Schwarz)
# the errors are |dA1| <= 2 (|ux| + |uy|) D <= 4 D, |dB1| <= 4 D; a variance u_ab - u_a u_b moves by at most D + 2 D = 3 D, so
# |dA2| <= 6 D, |dB2| <= 6 D; to first order |d(A1/B1)| <= (|dA1| + |dB1|) / B1 <= 8 D / C1 and |d(A2/B2)| <= 12 D / C2, and
# since both quotients are at most 1 in magnitude |dS| <= 8 D / C1 + 12 D / C2 = 2.27e-9 + 3.8e-10 = 2.65e-9 for one
# implementation against exact arithmetic (the few roundings of the quotient itself, ~10 U, are far below that).  Two
# implementations (kernel and yardstick, or yardstick and skimage) differ by at most twice that.
SSIM_D = 256 * U
SSIM_ONE_SIDED = 8 * SSIM_D / 1e-4 + 12 * SSIM_D / 9e-4
SSIM_TOL = 2 * SSIM_ONE_SIDED + 64 * U
assert 5.2e-9 < SSIM_TOL < 5.4e-9

SSIM_TILE = (16, 32)            # output pixels of one workgroup (ENSLAM_SSIM_TILE_H, ENSLAM_SSIM_TILE_W)


def _frame(rng, H, W):
    gd = (rng.random((H, W), dtype=np.float32) * 3.0 + 0.25).astype(np.float32)
    d = (gd + rng.normal(size=(H, W)).astype(np.float32) * 0.2).astype(np.float32)
    gc = (rng.random((H, W, 3), dtype=np.float32) * 1.5 - 0.25).astype(np.float32)
    c = (rng.random((H, W, 3), dtype=np.float32) * 1.5 - 0.25).astype(np.float32)
    return gd, gc, d, c


def _events(rng, h, w):
    return (rng.random((h, w, 2), dtype=np.float32) * 8.0 - 1.5).astype(np.float32)


PANEL_CASES = ('holes_45x61', 'nan_valid_45x61', 'no_depth_45x61', 'events_39x51_on_45x61', 'events_equal_45x61', 'plain_50x70',
               'bare_50x70')


def panel_case(name):
    """dict(gt_depth, gt_color, depth, color, gt_event, pred_event, gutter, title) of float32 numpy arrays"""
    rng = np.random.default_rng(1000 + PANEL_CASES.index(name))
    H, W = (50, 70) if name.endswith('50x70') else (45, 61)
    gd, gc, d, c = _frame(rng, H, W)
    ge = pe = None
    gutter, title = (0, 0) if name == 'bare_50x70' else (8, 16)
    assert (gc < 0).any() and (gc > 1).any() and (c < 0).any() and (c > 1).any()          # colour outside [0, 1]
    if name != 'plain_50x70' and name != 'bare_50x70':
        gd[rng.random((H, W)) < 0.2] = 0                                                   # some zeros
        gd[3, 4] = 0
        d[3, 4] = np.nan                                                                   # a NaN where the residual is zeroed
        d[7, 9], d[8, 10], d[9, 11] = -0.5, 100.0, 1.0e4                                  # negative, above max_depth
        gd[7, 9], gd[8, 10], gd[9, 11] = 1.0, 1.0, 1.0
        assert (gd == 0).sum() > 100 and (gd > 0).sum() > 100
    if name == 'nan_valid_45x61':
        gd[20, 30] = 2.0
        d[20, 30] = np.nan                                                                 # a NaN residual: white, and a NaN sum
    if name == 'no_depth_45x61':
        gd[:] = 0                                                                          # max_depth 0
    if name.startswith('events'):
        h, w = (39, 51) if '39x51' in name else (H, W)
        ge, pe = _events(rng, h, w), _events(rng, h, w)
        ge[0, 0], pe[0, 0] = (5.2, 0.03), (0.0, 5.11)                                      # above 5.1 saturates, just above stays
        assert (ge < 0).any() and (ge > 5.1).any() and (pe < 0).any() and (pe > 5.1).any()
    if name != 'no_depth_45x61':
        m = np.fmax.reduce(gd.reshape(-1))
        assert (gd == m).sum() >= 1 and m > 0                                              # one pixel exactly max_depth: u = 1
        assert (d[np.isfinite(d)] > m).any() or name.endswith('50x70')
    R = 2 if ge is None else 3
    n_px = (R * H + (R + 1) * gutter + R * title) * (3 * W + 4 * gutter)
    assert n_px % 1024 != 0 and (3 * W + 4 * gutter) % 1024 != 0
    if H == 45:
        assert n_px % 4 != 0                                                               # the tail thread writes bytes
    else:
        assert n_px % 4 == 0
    return dict(gt_depth=gd, gt_color=gc, depth=d, color=c, gt_event=ge, pred_event=pe, gutter=gutter, title=title)


_TH, _TW = SSIM_TILE
SSIM_CASES = {                   # name -> (H, W, C, kind)
    'one_pixel_11x11': (11, 11, 1, 'noise'),
    'edge_one_axis_12x43': (12, 43, 3, 'noise'),
    'frame_45x61': (45, 61, 3, 'near'),
    'tiles_1x2_exact': (_TH + 10, 2 * _TW + 10, 3, 'near'),
    'tiles_1x2_plus_one': (_TH + 11, 2 * _TW + 11, 1, 'near'),
    'identical_45x61': (45, 61, 3, 'same'),
    'constant_vs_noise': (30, 47, 1, 'constant'),
}


def ssim_case(name):
    """(x, y) float32 [H,W,C] with values in [0, 1]"""
    H, W, C, kind = SSIM_CASES[name]
    rng = np.random.default_rng(2000 + list(SSIM_CASES).index(name))
    x = rng.random((H, W, C), dtype=np.float32)
    if kind == 'noise':
        y = rng.random((H, W, C), dtype=np.float32)
    elif kind == 'near':
        y = np.clip(x + rng.normal(size=(H, W, C)).astype(np.float32) * 0.1, 0, 1).astype(np.float32)
    elif kind == 'same':
        y = x.copy()
    else:
        x = np.full((H, W, C), 0.5, np.float32)
        y = rng.random((H, W, C), dtype=np.float32)
    assert x.min() >= 0 and x.max() <= 1 and y.min() >= 0 and y.max() <= 1
    if name == 'tiles_1x2_exact':
        assert (H - 10, W - 10) == (_TH, 2 * _TW)
    return x, y
