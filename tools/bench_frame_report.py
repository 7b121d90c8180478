"""Cost of the per-iteration frame report (csrc/frame_report.hip, frame_vis.py) at 680 x 1200 and 260 x 346, device route
against host route in ONE process, alternating after a warm-up, median [min - max] of REPS (10) timed with device events
(an event pair around host work measures the host work: the second event is recorded after it).

    python tools/bench_frame_report.py [--reps 10] [--no-vis]

  sheet    device: functional.vis_panels + download of the uint8 sheet and the eight sums + JPEG (PIL)
           host:   download of the four float images + the numpy rules (frame_vis.panels_numpy) + JPEG
  ssim     device: functional.ssim + download of the mean;  host: skimage where importable, else frame_vis.ssim_numpy,
           on images already on the host
  kernels  enslam_vis_panels (three launches) and enslam_ssim (two) alone on preallocated buffers, 20 calls back to back per
           timing: unique bytes moved / time against the 6.3 TB/s that element-wise kernels reach on this machine;
           panels_call / ssim_call are the Python wrappers (allocations, checks) without a download
  vis      one Visualizer.vis call on the tiny golden scene's map at the size, split into render_img, panels, download, JPEG

Prints one JSON line.  Records, not bars: nothing in the package depends on these numbers."""
import argparse
import io
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

DEV = 'cuda:0'
HBM_CEILING = 6.3e12
RAW_CALLS = 20


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def summary(ms):
    ms = sorted(ms)
    return dict(median_ms=round(float(np.median(ms)), 4), min_ms=round(ms[0], 4), max_ms=round(ms[-1], 4))


def jpeg(sheet):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(sheet).save(buf, format='JPEG', quality=90)
    return buf.tell()


def frame(H, W, seed=0):
    g = torch.Generator().manual_seed(seed)
    gd = torch.rand(H, W, generator=g) * 3 + 0.2
    gd[torch.rand(H, W, generator=g) < 0.1] = 0
    gc = torch.rand(H, W, 3, generator=g)
    d = gd + torch.randn(H, W, generator=g) * 0.1
    c = (gc + torch.randn(H, W, 3, generator=g) * 0.1).clamp(0, 1)
    return [t.to(DEV) for t in (gd, gc, d, c)]


def bench_size(H, W, reps, with_vis):
    from evennicer_slam_amd import frame_vis as FV
    from evennicer_slam_amd import functional as EF
    gd, gc, d, c = frame(H, W)
    try:
        from skimage.metrics import structural_similarity
        host_ssim_name = 'skimage'

        def host_ssim(x, y):
            return float(structural_similarity(x, y, gaussian_weights=True, sigma=1.5, use_sample_covariance=False, data_range=1,
                                               channel_axis=2))
    except ImportError:
        host_ssim_name, host_ssim = 'frame_vis.ssim_numpy', FV.ssim_numpy
    c_host, gc_host = c.cpu().numpy(), gc.cpu().numpy()

    def sheet_device():
        sheet, stats = EF.vis_panels(gd, gc, d, c)
        return jpeg(sheet.cpu().numpy()), stats.cpu()

    def sheet_host():
        sheet, stats = FV.panels_numpy(gd.cpu().numpy(), gc.cpu().numpy(), d.cpu().numpy(), c.cpu().numpy())
        return jpeg(sheet), stats

    # the C entries alone on preallocated buffers, 20 calls back to back per timing: device time without the wrapper
    import ctypes
    from evennicer_slam_amd import _lib as L
    lib, n = L.lib(), ctypes.c_int64()
    L.check(lib.enslam_vis_panels_workspace(H, W, 2, FV.GUTTER, FV.TITLE, ctypes.byref(n)), "enslam_vis_panels_workspace")
    ws = torch.empty(n.value // 8, dtype=torch.float64, device=DEV)
    sheet_buf = torch.empty(FV.sheet_shape(H, W, 2), dtype=torch.uint8, device=DEV)
    stats_buf, mean_buf = torch.empty(8, dtype=torch.float64, device=DEV), torch.empty(1, dtype=torch.float64, device=DEV)
    m = ctypes.c_int64()
    L.check(lib.enslam_ssim_workspace(H, W, 3, ctypes.byref(m)), "enslam_ssim_workspace")
    sws = torch.empty(m.value // 8, dtype=torch.float64, device=DEV)
    stream = EF._stream()

    def raw_panels():
        for _ in range(RAW_CALLS):
            L.check(lib.enslam_vis_panels(gd.data_ptr(), gc.data_ptr(), d.data_ptr(), c.data_ptr(), None, None, H, W, 0, 0, FV.GUTTER,
                                          FV.TITLE, ws.data_ptr(), n.value, sheet_buf.data_ptr(), stats_buf.data_ptr(), stream),
                    "enslam_vis_panels")

    def raw_ssim():
        for _ in range(RAW_CALLS):
            L.check(lib.enslam_ssim(c.data_ptr(), gc.data_ptr(), H, W, 3, sws.data_ptr(), m.value, mean_buf.data_ptr(), None, stream),
                    "enslam_ssim")

    routes = {'panels_kernel': raw_panels, 'ssim_kernel': raw_ssim, 'sheet_device': sheet_device, 'sheet_host': sheet_host,
              'ssim_device': lambda: float(EF.ssim(c, gc).item()), 'ssim_host': lambda: host_ssim(c_host, gc_host),
              'panels_call': lambda: EF.vis_panels(gd, gc, d, c), 'ssim_call': lambda: EF.ssim(c, gc)}
    for fn in routes.values():                                              # warm-up
        fn()
        fn()
    times = {k: [] for k in routes}
    for _ in range(reps):                                                   # alternating
        for k, fn in routes.items():
            times[k].append(timed(fn)[0])
    for k in ('panels_kernel', 'ssim_kernel'):
        times[k] = [t / RAW_CALLS for t in times[k]]
    out = {k: summary(v) for k, v in times.items()}
    out['host_ssim'] = host_ssim_name
    sh = FV.sheet_shape(H, W, 2)
    panel_bytes = H * W * 32 + sh[0] * sh[1] * 3
    ssim_bytes = 2 * H * W * 3 * 4
    for k, nbytes in (('panels_kernel', panel_bytes), ('ssim_kernel', ssim_bytes)):
        rate = nbytes / (out[k]['median_ms'] * 1e-3)
        out[k].update(bytes=nbytes, gb_per_s=round(rate / 1e9, 1), hbm_share=round(rate / HBM_CEILING, 4))
    if with_vis:
        out['vis'] = bench_vis(H, W, reps)
    return out


def bench_vis(H, W, reps):
    """One Visualizer.vis call at H x W on the tiny golden scene's map, split into its phases."""
    import tempfile
    from evennicer_slam_amd import frame_vis as FV
    from evennicer_slam_amd import functional as EF
    from tests.hip_util import renderer_for, tiny_on_gpu
    s, bound, model, grids, rays, _ = tiny_on_gpu()
    renderer = renderer_for(bound, cam=(H, W, 0.8 * W, 0.8 * W, (W - 1) / 2, (H - 1) / 2))
    gd = (torch.rand(H, W, generator=torch.Generator().manual_seed(1)) * 0.8 + 0.4).to(DEV)
    gc = torch.rand(H, W, 3, generator=torch.Generator().manual_seed(2)).to(DEV)
    c2w = torch.eye(4, device=DEV)
    phases = {k: [] for k in ('render_img', 'panels', 'download', 'jpeg', 'vis_call')}
    with tempfile.TemporaryDirectory() as tmp:
        v = FV.Visualizer(1, 1, tmp, renderer, verbose=False, device=DEV)
        for rep in range(reps + 1):
            t_r, (d, _u, c) = timed(lambda: renderer.render_img(grids, model, c2w, DEV, stage='color', gt_depth=gd))
            t_p, (sheet, stats) = timed(lambda: EF.vis_panels(gd, gc, d, c))
            t_d, host = timed(lambda: (sheet.cpu().numpy(), stats.cpu().numpy()))
            t_j, _ = timed(lambda: FV.draw_titles(host[0], H, W, 2).save(os.path.join(tmp, 'x.jpg'), quality=90))
            t_v, _ = timed(lambda: v.vis(0, 0, gd, gc, c2w, grids, model))
            if rep:                                                         # the first round warms up
                for k, t in zip(phases, (t_r, t_p, t_d, t_j, t_v)):
                    phases[k].append(t)
    out = {k: summary(t) for k, t in phases.items()}
    out['rays_per_s'] = round(H * W / (out['render_img']['median_ms'] * 1e-3))
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--no-vis', action='store_true')
    args = ap.parse_args(argv)
    out = {f'{H}x{W}': bench_size(H, W, args.reps, not args.no_vis) for H, W in ((680, 1200), (260, 346))}
    out.update(reps=args.reps, device=torch.cuda.get_device_name(0))
    print(json.dumps(out), flush=True)
    return out


if __name__ == '__main__':
    main()
