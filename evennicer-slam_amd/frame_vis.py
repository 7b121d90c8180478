"""Per-iteration figure writer and rendering metrics: the counterpart of the reference's src/utils/Visualizer.py.

`Visualizer.vis` / `vis_event` render the current frame from the current map and pose (`Renderer.render_img`, stage
'color', depth-guided) and write one sheet of panels to `{vis_dir}/{idx:05d}_{iter:04d}.jpg`:

    row 0   Input Depth | Generated Depth | Depth Residual         plasma colours against max(gt_depth)
    row 1   Input RGB   | Generated RGB   | RGB Residual
    row 2   Lo-Res GT Event | Generated Event | Event Residual     (vis_event only; events at their own resolution,
                                                                    shown at the frame's size by nearest source pixel)

On a HIP device the sheet and the frame's error sums come from one call of `functional.vis_panels`
(csrc/frame_report.hip; include/enslam_hip.h holds every pixel rule) and only the uint8 sheet and eight float64 numbers
are brought to the host, where PIL draws the titles into the white strips above the panels and encodes the JPEG.  CPU
tensors take the numpy route of this module, which applies the same rules in float32 and gives the same bytes.

Differences from the reference, all deliberate: no matplotlib (the layout is fixed: a white gutter around every panel, a
title strip above it, no resampling of the images); the event residual is the true |a - b| of the two uint8 images (the
reference subtracts the uint8 arrays, which wraps around); every call returns the frame's statistics (depth L1, PSNR)
and keeps them as `last_stats`; `experiment` is any object with a `.log(dict)` method and receives plain numbers and
uint8 arrays -- wandb is not imported.

`render_metrics` gives depth L1, PSNR and SSIM of a re-rendered frame (tools/eval_rendering.py)."""
import math
import os
import re

import numpy as np
import torch

from .common import get_camera_from_tensor

GUTTER = 8
TITLE = 16
TITLES = (('Input Depth', 'Generated Depth', 'Depth Residual'),
          ('Input RGB', 'Generated RGB', 'RGB Residual'),
          ('Lo-Res GT Event', 'Generated Event', 'Event Residual'))
_SSIM_SIGMA, _SSIM_RADIUS, _SSIM_C1, _SSIM_C2 = 1.5, 5, 0.01 ** 2, 0.03 ** 2

_plasma = None


def plasma_lut():
    """uint8 [256,3]: the table the kernel indexes, parsed from csrc/plasma_lut.hpp (one copy of the bytes)."""
    global _plasma
    if _plasma is None:
        path = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'csrc', 'plasma_lut.hpp')
        body = open(path).read().split('{', 1)[1].split('}', 1)[0]
        values = np.array([int(v) for v in re.findall(r'\d+', body)], dtype=np.uint8)
        if values.size != 768:
            raise RuntimeError(f"{path}: expected 768 table bytes, found {values.size}")
        _plasma = values.reshape(256, 3)
    return _plasma


def sheet_shape(H, W, rows, gutter=GUTTER, title=TITLE):
    return rows * H + (rows + 1) * gutter + rows * title, 3 * W + 4 * gutter, 3


def panel_origin(r, c, H, W, gutter=GUTTER, title=TITLE):
    """(row, column) of the first pixel of panel (r, c)."""
    return gutter + title + r * (H + gutter + title), gutter + c * (W + gutter)


# ------------------------------------------------------------------------------------------------
# the numpy route: the rules of enslam_vis_panels in float32
# ------------------------------------------------------------------------------------------------
def _depth_panel(v, max_depth, lut):
    if max_depth == 0:
        return np.broadcast_to(lut[0], v.shape + (3,)).copy()
    with np.errstate(all='ignore'):
        u = v / np.float32(max_depth)
        level = (np.where((u >= 0) & (u < 1), u, np.float32(0)) * np.float32(256.0)).astype(np.int32)
    level = np.where(u < 0, 0, np.where(u >= 1, 255, level))
    out = lut[np.where(np.isnan(u), 0, level)]
    out[np.isnan(u)] = 255
    return out


def _clip01(c):
    c = np.where(c > 0, c, np.float32(0))
    return np.where(c < 1, c, np.float32(1))


def _color_panel(c):
    return (_clip01(c) * np.float32(255.0) + np.float32(0.5)).astype(np.uint8)


def _event_panel(e, H, W):
    h, w = e.shape[:2]
    v = e * np.float32(50.0)
    v = np.where(v > 0, v, np.float32(0))
    v = np.where(v < 255, v, np.float32(255))
    ys = ((2 * np.arange(H) + 1) * h) // (2 * H)
    xs = ((2 * np.arange(W) + 1) * w) // (2 * W)
    img = np.zeros((H, W, 3), dtype=np.uint8)
    img[..., :2] = v.astype(np.uint8)[ys][:, xs]
    return img


def panels_numpy(gt_depth, gt_color, depth, color, gt_event=None, pred_event=None, gutter=GUTTER, title=TITLE):
    """(sheet uint8, stats float64 [8]) by the rules of `functional.vis_panels`, on the host."""
    f32 = lambda a: np.ascontiguousarray(np.asarray(a, dtype=np.float32))
    gd, gc, d, c = f32(gt_depth), f32(gt_color), f32(depth), f32(color)
    H, W = gd.shape
    rows = 2 if gt_event is None else 3
    lut = plasma_lut()
    max_depth = np.fmax.reduce(gd.reshape(-1))
    hole = gd == 0
    with np.errstate(invalid='ignore'):
        d_res = np.where(hole, np.float32(0), np.abs(gd - d))
        c_res = np.where(hole[..., None], np.float32(0), np.abs(gc - c))
    grid = [[_depth_panel(gd, max_depth, lut), _depth_panel(d, max_depth, lut), _depth_panel(d_res, max_depth, lut)],
            [_color_panel(gc), _color_panel(c), _color_panel(c_res)]]
    if rows == 3:
        a, b = _event_panel(f32(gt_event), H, W), _event_panel(f32(pred_event), H, W)
        grid.append([a, b, np.abs(a.astype(np.int16) - b.astype(np.int16)).astype(np.uint8)])
    sheet = np.full(sheet_shape(H, W, rows, gutter, title), 255, dtype=np.uint8)
    for r in range(rows):
        for k in range(3):
            y, x = panel_origin(r, k, H, W, gutter, title)
            sheet[y:y + H, x:x + W] = grid[r][k]
    valid = gd > 0
    err = (_clip01(gc) - _clip01(c)).astype(np.float64) ** 2
    with np.errstate(invalid='ignore'):
        l1 = np.abs(gd - d)[valid].astype(np.float64)
    s = [float(valid.sum()), float(l1.sum()), float(err.sum()), float(err[valid].sum())]
    return sheet, np.array(s + s, dtype=np.float64)


def ssim_numpy(x, y):
    """Mean SSIM in float64 on the host, the definition of `functional.ssim` (separable 11-tap Gaussian, sigma 1.5)."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    if x.ndim == 2:
        x, y = x[..., None], y[..., None]
    H, W, _ = x.shape
    if H < 11 or W < 11:
        raise ValueError(f"ssim: the window is 11 x 11, the images are {H} x {W}")
    k = np.arange(-_SSIM_RADIUS, _SSIM_RADIUS + 1, dtype=np.float64)
    g = np.exp(-(k * k) / (2.0 * _SSIM_SIGMA ** 2))
    g /= g.sum()

    def blur(a):
        a = sum(g[i] * a[:, i:i + W - 10] for i in range(11))
        return sum(g[i] * a[i:i + H - 10] for i in range(11))

    ux, uy, uxx, uyy, uxy = blur(x), blur(y), blur(x * x), blur(y * y), blur(x * y)
    vx, vy, vxy = uxx - ux * ux, uyy - uy * uy, uxy - ux * uy
    s = ((2 * ux * uy + _SSIM_C1) * (2 * vxy + _SSIM_C2)) / ((ux * ux + uy * uy + _SSIM_C1) * (vx + vy + _SSIM_C2))
    return float(s.mean())


# ------------------------------------------------------------------------------------------------
# numbers
# ------------------------------------------------------------------------------------------------
def _psnr(sq_sum, count):
    if count <= 0:
        return float('nan')
    mse = sq_sum / count
    if mse != mse:
        return float('nan')
    return float('inf') if mse == 0 else -10.0 * math.log10(mse)


def stats_dict(stats, n_pixels):
    """The frame's numbers from the eight sums of `vis_panels`: depth_l1 over the gt_depth > 0 pixels (nan when there are
    none), psnr over every pixel and channel, psnr_valid over the gt_depth > 0 pixels, n_valid."""
    n, l1, sq, sqv = (float(v) for v in stats[:4])
    return dict(depth_l1=l1 / n if n > 0 else float('nan'), psnr=_psnr(sq, 3 * n_pixels), psnr_valid=_psnr(sqv, 3 * n),
                n_valid=int(n))


def frame_report(gt_depth, gt_color, depth, color, gt_event=None, pred_event=None, gutter=GUTTER, title=TITLE):
    """(sheet uint8 numpy [.,.,3], stats dict): the device route for HIP tensors, the numpy route otherwise."""
    if torch.is_tensor(gt_depth) and gt_depth.is_cuda:
        from . import functional as EF
        dev = gt_depth.device
        on = lambda t: None if t is None else t.to(dev)
        sheet, stats = EF.vis_panels(gt_depth, on(gt_color), on(depth), on(color), on(gt_event), on(pred_event), gutter=gutter,
                                     title=title)
        sheet, stats = sheet.cpu().numpy(), stats.cpu().numpy()
    else:
        host = lambda t: None if t is None else (t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t))
        sheet, stats = panels_numpy(host(gt_depth), host(gt_color), host(depth), host(color), host(gt_event), host(pred_event),
                                    gutter=gutter, title=title)
    return sheet, stats_dict(stats, int(gt_depth.shape[0]) * int(gt_depth.shape[1]))


def render_metrics(depth, color, gt_depth, gt_color, ssim=True):
    """dict(depth_l1, psnr, ssim) of a rendered frame against its ground truth: depth_l1 the mean |gt - rendered| over the
    gt_depth > 0 pixels, psnr = -10 log10(mse) of the colours clipped to [0, 1] over every pixel and channel (inf for
    identical images), ssim of the clipped colours (None with ssim=False).  HIP tensors use the kernels
    (functional.vis_panels with no gutter, functional.ssim); CPU tensors the numpy route."""
    _, s = frame_report(gt_depth, gt_color, depth, color, gutter=0, title=0)
    out = dict(depth_l1=s['depth_l1'], psnr=s['psnr'], ssim=None)
    if ssim:
        if torch.is_tensor(color) and color.is_cuda:
            from . import functional as EF
            out['ssim'] = float(EF.ssim(color.detach().float().clamp(0, 1), gt_color.to(color.device).float().clamp(0, 1)).item())
        else:
            host = lambda t: t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
            out['ssim'] = ssim_numpy(_clip01(host(color).astype(np.float32)), _clip01(host(gt_color).astype(np.float32)))
    return out


def draw_titles(sheet, H, W, rows, gutter=GUTTER, title=TITLE):
    """The sheet as a PIL image with the reference's titles drawn into the strips (nothing is drawn into a strip lower than
    10 pixels)."""
    from PIL import Image, ImageDraw
    img = Image.fromarray(sheet)
    if title >= 10:
        for r in range(rows):
            for c in range(3):
                y, x = panel_origin(r, c, H, W, gutter, title)
                strip = Image.new('RGB', (W, title), (255, 255, 255))           # a title longer than its panel is cut off
                ImageDraw.Draw(strip).text((2, (title - 10) // 2), TITLES[r][c], fill=(0, 0, 0))
                img.paste(strip, (x, y - title))
    return img


class Visualizer(object):
    """The reference's Visualizer: `vis` / `vis_event` are called every iteration and write a figure when
    idx % freq == 0 and iter % inside_freq == 0.  Each returns the frame's statistics (None when gated off)."""

    def __init__(self, freq, inside_freq, vis_dir, renderer, verbose, experiment=None, device='cuda:0', stage='tracker',
                 gutter=GUTTER, title=TITLE, quality=90):
        self.freq, self.inside_freq = freq, inside_freq
        self.device, self.vis_dir, self.verbose, self.renderer = device, vis_dir, verbose, renderer
        self.experiment, self.stage = experiment, stage
        self.gutter, self.title, self.quality = gutter, title, quality
        self.last_stats = None
        self.last_sheet = None              # the uint8 sheet before the titles and the JPEG encoding
        os.makedirs(f'{vis_dir}', exist_ok=True)

    def due(self, idx, iter):
        return (int(idx) % self.freq == 0) and (int(iter) % self.inside_freq == 0)

    def _c2w(self, c2w_or_camera_tensor):
        if len(c2w_or_camera_tensor.shape) == 1:
            c2w = get_camera_from_tensor(c2w_or_camera_tensor.clone().detach())
            bottom = torch.tensor([[0., 0., 0., 1.]], dtype=c2w.dtype, device=c2w.device)
            return torch.cat([c2w, bottom], dim=0)
        return c2w_or_camera_tensor

    def _figure(self, idx, iter, gt_depth, gt_color, gt_event, pred_event, c2w_or_camera_tensor, c, decoders, blurred):
        with torch.no_grad():
            c2w = self._c2w(c2w_or_camera_tensor)
            depth, _uncertainty, color = self.renderer.render_img(c, decoders, c2w, self.device, stage='color', gt_depth=gt_depth)
            H, W = int(gt_depth.shape[0]), int(gt_depth.shape[1])
            rows = 2 if gt_event is None else 3
            sheet, stats = frame_report(gt_depth, gt_color, depth.detach(), color.detach(),
                                        None if gt_event is None else gt_event.detach(),
                                        None if pred_event is None else pred_event.detach(), self.gutter, self.title)
            path = f'{self.vis_dir}/{int(idx):05d}_{int(iter):04d}.jpg'
            draw_titles(sheet, H, W, rows, self.gutter, self.title).save(path, quality=self.quality)
            self.last_sheet, self.last_stats = sheet, stats
            if self.verbose:
                kind = 'color/depth' if rows == 2 else 'color/depth/event'
                print(f'Saved rendering visualization of {kind} image at {path}')
            if self.experiment is not None:
                def panel(r, k):
                    y, x = panel_origin(r, k, H, W, self.gutter, self.title)
                    return sheet[y:y + H, x:x + W]

                log = {'Depth': {'GT Depth': panel(0, 0), f'Rendered Depth ({self.stage})': panel(0, 1),
                                 f'Depth Residual ({self.stage})': panel(0, 2)},
                       'RGB': {'GT RGB': panel(1, 0), f'Rendered RGB ({self.stage})': panel(1, 1),
                               f'RGB Residual ({self.stage})': panel(1, 2)},
                       f'Rendering ({self.stage})': dict(stats), 'Frame': int(idx)}
                if rows == 3:
                    ev = {f'Lo-Res GT Event ({self.stage})': panel(2, 0), f'Rendered Event ({self.stage})': panel(2, 1)}
                    for level, (g, p) in enumerate(blurred):
                        hw = (int(g.shape[0]), int(g.shape[1]))
                        ev[f'GT Event Blurred {level + 1} ({self.stage})'] = _event_panel(_host32(g), *hw)
                        ev[f'Rendered Event {level + 1} ({self.stage})'] = _event_panel(_host32(p), *hw)
                    log['Event'] = ev
                self.experiment.log(log)
            return stats

    def vis(self, idx, iter, gt_depth, gt_color, c2w_or_camera_tensor, c, decoders):
        """Depth and colour panels of frame idx at iteration iter (a 7-vector camera tensor or a 4 x 4 matrix)."""
        if not self.due(idx, iter):
            return None
        return self._figure(idx, iter, gt_depth, gt_color, None, None, c2w_or_camera_tensor, c, decoders, ())

    def vis_event(self, idx, iter, gt_depth, gt_color, gt_event, gt_event_lores, pred_event, gts_event_list, preds_event_list,
                  c2w_or_camera_tensor, c, decoders):
        """`vis` with the event row: gt_event_lores and pred_event [h,w,2] at the event iteration's resolution.  gt_event
        (full resolution) is not shown, as in the reference; the blurred lists only go to `experiment.log`."""
        if not self.due(idx, iter):
            return None
        return self._figure(idx, iter, gt_depth, gt_color, gt_event_lores, pred_event, c2w_or_camera_tensor, c, decoders,
                            tuple(zip(gts_event_list or (), preds_event_list or ())))


def _host32(t):
    return (t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)).astype(np.float32)
