"""-m gpu: csrc/frame_report.hip (functional.vis_panels, functional.ssim) and what is built on it (frame_vis.Visualizer,
frame_vis.render_metrics, SLAM(vis=True), tools/eval_rendering.py) against the yardsticks of tests/frame_vis_numpy.py on the
cases of tests/frame_vis_cases.py, where the tolerances are derived: the sheet byte for byte with no pixel left out, the
sums within 64 * 2^-53 of the sum of their absolute terms, the SSIM map and mean within the propagated rounding bound."""
import ctypes
import importlib.util
import json
import os
import types

import numpy as np
import pytest
import torch

from tests import frame_vis_cases as C
from tests import frame_vis_numpy as Y

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def lut():
    from evennicer_slam_amd import frame_vis as FV
    return FV.plasma_lut()


def _panels(case, cast=None):
    from evennicer_slam_amd import functional as EF
    t = {k: dev(case[k]) for k in ('gt_depth', 'gt_color', 'depth', 'color', 'gt_event', 'pred_event')}
    if cast is not None:
        t = {k: (None if v is None else v.to(cast)) for k, v in t.items()}
    sheet, stats = EF.vis_panels(gutter=case['gutter'], title=case['title'], **t)
    torch.cuda.synchronize()
    return sheet.cpu().numpy(), stats.cpu().numpy()


@pytest.mark.parametrize("name", C.PANEL_CASES)
def test_sheet_and_sums_match_the_yardstick(name):
    case = C.panel_case(name)
    sheet, stats = _panels(case)
    want = Y.sheet(lut=lut(), **case)
    assert sheet.shape == want.shape and sheet.dtype == np.uint8
    print(f"{name}: sheet {sheet.shape}, mismatching pixels {int((sheet != want).any(-1).sum())}")
    assert np.array_equal(sheet, want)
    ys = Y.stats(case['gt_depth'], case['gt_color'], case['depth'], case['color'])
    print(f"{name}: sums {stats.tolist()} yardstick {ys.tolist()}")
    assert stats[0] == ys[0] and stats[4] == ys[4]                           # n_valid is exact
    for k in (1, 2, 3):
        if np.isnan(ys[k]):
            assert name == 'nan_valid_45x61' and k == 1 and np.isnan(stats[k]) and np.isnan(stats[4 + k])
            continue
        assert abs(stats[k] - ys[k]) <= C.STATS_RTOL * ys[4 + k], (name, k, stats[k], ys[k])
        assert abs(stats[4 + k] - ys[4 + k]) <= C.STATS_RTOL * ys[4 + k], (name, k)
    again = _panels(case)
    assert np.array_equal(again[0], sheet) and again[1].tobytes() == stats.tobytes()       # two calls, the same bits
    if name == 'events_39x51_on_45x61':                                     # float64 inputs are cast to float32 once
        as64 = _panels(case, torch.float64)
        assert np.array_equal(as64[0], sheet) and as64[1].tobytes() == stats.tobytes()


@pytest.mark.parametrize("name", list(C.SSIM_CASES))
def test_ssim_map_and_mean_match_the_yardstick(name):
    from evennicer_slam_amd import functional as EF
    x, y = C.ssim_case(name)
    mean, smap = EF.ssim(dev(x), dev(y), want_map=True)
    alone = EF.ssim(dev(x), dev(y))
    torch.cuda.synchronize()
    want_mean, want_map = Y.ssim(x, y)
    got = smap.cpu().numpy()
    assert got.shape == want_map.shape == (x.shape[0] - 10, x.shape[1] - 10, x.shape[2]) and got.dtype == np.float64
    err = np.abs(got - want_map).max()
    print(f"{name}: mean {float(mean)} yardstick {want_mean}, map error {err:.3e}, bound {C.SSIM_TOL:.3e}")
    assert err <= C.SSIM_TOL and abs(float(mean) - want_mean) <= C.SSIM_TOL
    assert float(alone) == float(mean)                                      # two calls, with and without the map
    if name == 'identical_45x61':
        assert float(mean) == 1.0 and np.all(got == 1.0)
    if name == 'constant_vs_noise':
        assert abs(float(mean)) < 0.05
    if x.shape[2] == 1:
        assert float(EF.ssim(dev(x[..., 0]), dev(y[..., 0]))) == float(mean)                 # [H,W] is [H,W,1]


def test_bad_arguments_return_codes_before_any_launch():
    """Host-side checks only: every call below is refused before a kernel is launched."""
    from evennicer_slam_amd import _lib as L
    from evennicer_slam_amd import functional as EF
    lib = L.lib()
    n = ctypes.c_int64(-7)
    assert lib.enslam_vis_panels_workspace(45, 61, 2, 8, 16, ctypes.byref(n)) == 0 and n.value > 1024
    for args in ((0, 61, 2, 8, 16), (45, -1, 2, 8, 16), (45, 61, 4, 8, 16), (45, 61, 2, -1, 16), (45, 61, 2, 8, -1)):
        assert lib.enslam_vis_panels_workspace(*args, ctypes.byref(n)) == -1
    assert lib.enslam_vis_panels_workspace(45, 61, 2, 8, 16, None) == -1
    assert lib.enslam_vis_panels_workspace(30000, 30000, 2, 8, 16, ctypes.byref(n)) == -3
    H, W = 12, 13
    gd, d = torch.rand(H, W, device=DEV), torch.rand(H, W, device=DEV)
    gc, c = torch.rand(H, W, 3, device=DEV), torch.rand(H, W, 3, device=DEV)
    ev = torch.rand(5, 6, 2, device=DEV)
    lib.enslam_vis_panels_workspace(H, W, 3, 8, 16, ctypes.byref(n))
    ws = torch.empty(n.value // 8, dtype=torch.float64, device=DEV)
    sheet = torch.full((3 * H + 32 + 48, 3 * W + 32, 3), 7, dtype=torch.uint8, device=DEV)
    stats = torch.full((8,), -1.0, dtype=torch.float64, device=DEV)
    p = lambda t: None if t is None else t.data_ptr()

    def call(gd_=gd, gc_=gc, d_=d, c_=c, ge=None, pe=None, H_=H, W_=W, h=0, w=0, g=8, t=16, ws_=ws, nb=None, sh=sheet, st=stats):
        return lib.enslam_vis_panels(p(gd_), p(gc_), p(d_), p(c_), p(ge), p(pe), H_, W_, h, w, g, t, p(ws_),
                                     n.value if nb is None else nb, p(sh), p(st), None)

    for kw in (dict(gd_=None), dict(gc_=None), dict(d_=None), dict(c_=None), dict(ws_=None), dict(sh=None), dict(st=None),
               dict(ge=ev), dict(pe=ev), dict(ge=ev, pe=ev, h=0, w=6), dict(ge=ev, pe=ev, h=5, w=-1), dict(H_=0), dict(W_=-3),
               dict(g=-1), dict(t=-2), dict(nb=8)):
        assert call(**kw) == -1, kw
    torch.cuda.synchronize()
    assert bool((sheet == 7).all()) and bool((stats == -1.0).all())          # nothing ran
    assert call(ge=ev, pe=ev, h=5, w=6) == 0                                 # the same call with good arguments
    torch.cuda.synchronize()
    assert bool((sheet != 7).any())

    assert lib.enslam_ssim_workspace(45, 61, 3, ctypes.byref(n)) == 0 and n.value == 8 * 3 * 2 * 3
    for args in ((10, 61, 3), (45, 10, 3), (0, 61, 3), (45, 61, 2), (45, 61, 0), (45, 61, 4)):
        assert lib.enslam_ssim_workspace(*args, ctypes.byref(n)) == -1, args
    assert lib.enslam_ssim_workspace(45, 61, 3, None) == -1 and lib.enslam_ssim_workspace(20000, 20000, 1, ctypes.byref(n)) == -3
    x = torch.rand(45, 61, 3, device=DEV)
    lib.enslam_ssim_workspace(45, 61, 3, ctypes.byref(n))
    sws = torch.empty(n.value // 8, dtype=torch.float64, device=DEV)
    mean = torch.full((1,), -1.0, dtype=torch.float64, device=DEV)
    for a in ((None, p(x), 45, 61, 3, p(sws), n.value, p(mean)), (p(x), None, 45, 61, 3, p(sws), n.value, p(mean)),
              (p(x), p(x), 45, 61, 3, None, n.value, p(mean)), (p(x), p(x), 45, 61, 3, p(sws), n.value, None),
              (p(x), p(x), 45, 61, 3, p(sws), 8, p(mean)), (p(x), p(x), 10, 61, 3, p(sws), n.value, p(mean)),
              (p(x), p(x), 45, 10, 3, p(sws), n.value, p(mean)), (p(x), p(x), 45, 61, 2, p(sws), n.value, p(mean)),
              (p(x), p(x), -45, 61, 3, p(sws), n.value, p(mean))):
        assert lib.enslam_ssim(*a, None, None) == -1, a
    torch.cuda.synchronize()
    assert float(mean) == -1.0
    with pytest.raises(L.EnslamError):
        EF.ssim(x[:10], x[:10])
    with pytest.raises(L.EnslamError):
        EF.ssim(x[..., :2], x[..., :2])
    with pytest.raises(L.EnslamError):
        EF.vis_panels(gd, gc, d, c, gt_event=ev)
    with pytest.raises(L.EnslamError):
        EF.vis_panels(gd, gc[:, :, :2], d, c)
    with pytest.raises(NotImplementedError):
        EF.vis_panels(gd.cpu(), gc.cpu(), d.cpu(), c.cpu())


class Recording:
    """the real renderer, keeping what render_img returned"""

    def __init__(self, inner):
        self.inner, self.out = inner, None

    def render_img(self, *a, **k):
        self.out = self.inner.render_img(*a, **k)
        return self.out


def test_visualizer_on_the_tiny_golden_scene(tmp_path):
    from PIL import Image
    from evennicer_slam_amd import frame_vis as FV
    from tests.hip_util import tiny_on_gpu
    from tests.util import load
    s, bound, model, grids, rays, renderer = tiny_on_gpu()
    g = load("tiny_render_img")
    renderer.ray_batch_size = int(g["ray_batch_size"])
    c2w = torch.from_numpy(g["c2w"]).to(DEV)
    gt_depth = torch.from_numpy(g["depth_img"]).to(DEV)
    H, W = gt_depth.shape
    gt_color = torch.rand(H, W, 3, generator=torch.Generator().manual_seed(3)).to(DEV)
    rec = Recording(renderer)
    v = FV.Visualizer(1, 1, str(tmp_path / 'vis'), rec, verbose=False, device=DEV)
    stats = v.vis(4, 2, gt_depth, gt_color, c2w, grids, model)
    depth, _unc, color = rec.out
    assert Image.open(tmp_path / 'vis' / '00004_0002.jpg').size == (3 * W + 32, 2 * H + 24 + 32)
    host = lambda t: t.detach().cpu().numpy().astype(np.float32)
    want = Y.sheet(host(gt_depth), host(gt_color), host(depth), host(color), lut())
    assert np.array_equal(v.last_sheet, want)
    ys = Y.stats(host(gt_depth), host(gt_color), host(depth), host(color))
    assert stats['n_valid'] == int(ys[0]) and abs(stats['depth_l1'] - ys[1] / ys[0]) <= 1e-12 * ys[1] / ys[0]
    assert np.isfinite(stats['psnr']) and abs(stats['psnr'] + 10 * np.log10(ys[2] / (3 * H * W))) < 1e-9
    m = FV.render_metrics(depth, color, gt_depth, gt_color)
    assert m['depth_l1'] == stats['depth_l1'] and m['psnr'] == stats['psnr']
    assert abs(m['ssim'] - Y.ssim(Y.clip01(host(color)), Y.clip01(host(gt_color)))[0]) <= C.SSIM_TOL


def _load_tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, 'tools', name + '.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_slam_vis_and_eval_rendering_on_a_three_frame_demo_run(tmp_path, capsys):
    import yaml
    from evennicer_slam_amd import datasets as D
    from evennicer_slam_amd.slam import SLAM
    from evennicer_slam_amd.synthetic import demo_config, write_demo_sequence
    n = 3
    cam = dict(H=36, W=48, fx=42.0, fy=42.0, cx=23.5, cy=17.5)
    (inp, evf), poses = write_demo_sequence(str(tmp_path / 'data'), n, cam)
    cfg = demo_config(inp, evf, cam, device=DEV, env={'ITERS_FIRST': 30, 'MAP_ITERS': 10, 'TRACK_ITERS': 6, 'EVERY': 1})
    cfg['tracking'].update(vis_freq=1, vis_inside_freq=3)
    cfg['mapping'].update(vis_freq=2, vis_inside_freq=5)
    out = str(tmp_path / 'out')
    cfg['data']['output'] = out
    ds = D.get_dataset(cfg, types.SimpleNamespace(input_folder=None, event_folder=None), 1, device=DEV)
    torch.manual_seed(0)
    np.random.seed(0)
    slam = SLAM(cfg, ds, out, device=DEV, static_shapes=True, vis=True)
    slam.run()
    trk, mp = sorted(os.listdir(os.path.join(out, 'tracking_vis'))), sorted(os.listdir(os.path.join(out, 'mapping_vis')))
    assert trk == ['00000_0000.jpg', '00001_0000.jpg', '00001_0003.jpg', '00002_0000.jpg', '00002_0003.jpg']
    assert mp == ['00000_%04d.jpg' % j for j in range(0, 30, 5)] + ['00002_0000.jpg', '00002_0005.jpg']
    assert np.isfinite(slam.vis_mapper.last_stats['psnr']) and slam.vis_tracker.last_stats['n_valid'] > 0
    path = tmp_path / 'config.yaml'
    path.write_text(yaml.safe_dump(cfg))
    capsys.readouterr()
    res = _load_tool('eval_rendering').main([str(path), '--every', '1', '--save', str(tmp_path / 'sheets'), '--device', DEV])
    line = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith('{')][-1]
    parsed = json.loads(line)
    assert parsed['n_frames'] == 3 and [f['idx'] for f in parsed['frames']] == [0, 1, 2] and res['ckpt'].endswith('00002.tar')
    for f in parsed['frames']:
        assert all(np.isfinite(f[k]) for k in ('depth_l1', 'psnr', 'ssim')), f
        assert f['depth_l1'] >= 0 and -1 <= f['ssim'] <= 1
    assert all(np.isfinite(parsed[k]) for k in ('depth_l1', 'psnr', 'ssim'))
    assert sorted(os.listdir(tmp_path / 'sheets')) == ['00000_0000.jpg', '00001_0000.jpg', '00002_0000.jpg']
