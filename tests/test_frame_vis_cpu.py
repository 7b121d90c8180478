"""The frame report without a GPU: hand-worked pixels of every rule of tests/frame_vis_numpy.py (the yardstick of
tests/test_hip_frame_vis.py) and of the package's numpy route, the committed plasma table, the SSIM yardstick against
skimage, the C ABI, and frame_vis.Visualizer on CPU tensors with a stub renderer."""
import os
import re
import types

import numpy as np
import pytest
import torch

from tests import frame_vis_cases as C
from tests import frame_vis_numpy as Y

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def lut():
    from evennicer_slam_amd import frame_vis as FV
    return FV.plasma_lut()


def test_depth_levels_by_hand():
    t = lut()
    below_one = np.nextafter(F(1), F(0))
    v = np.array([0.0, 2.0 * below_one, 2.0, np.nan, -0.1, 3.0, 1.0, 2.0 / 256, np.nextafter(F(2.0 / 256), F(0))], F)
    got = Y.depth_rgb(v, F(2.0), t)
    for k, want in enumerate((0, 255, 255, None, 0, 255, 128, 1, 0)):
        assert np.array_equal(got[k], (255, 255, 255) if want is None else t[want]), (k, want)
    assert float(below_one * F(256.0)) < 256.0                              # the largest u below 1 still truncates to 255
    assert np.array_equal(Y.depth_rgb(np.array([0.0, 5.0, np.nan], F), F(0.0), t), np.tile(t[0], (3, 1)))   # max_depth 0


def test_colour_and_event_levels_by_hand():
    half = F(0.5) / F(255.0)
    under = F(0.49) / F(255.0)
    c = np.array([-0.3, 0.0, half, under, 1.0, 1.7, np.nan, 0.5], F)
    below = int(under * F(255.0) + F(0.5))
    assert Y.color_level(c).tolist() == [0, 0, int(half * F(255.0) + F(0.5)), below, 255, 255, 0, 128]
    assert int(half * F(255.0) + F(0.5)) == 1 and below == 0                 # rounding at 0.5 / 255
    e = np.array([-1.0, 0.0, 0.0199, 0.02, 1.999 / 50, 5.09, 5.1, 5.2, 100.0, np.nan], F)
    assert Y.event_level(e).tolist() == [0, 0, 0, 1, 1, 254, 255, 255, 255, 0]                 # truncation, saturation


def test_nearest_source_index_at_both_edges():
    for n_out, n_src in ((45, 39), (61, 51), (45, 45), (10, 3), (680, 68)):                # enlarging: both edges are reached
        s = Y.nearest_source(n_out, n_src)
        assert s[0] == 0 and s[-1] == n_src - 1 and np.all(np.diff(s) >= 0)
        if n_out == n_src:
            assert np.array_equal(s, np.arange(n_out))
    assert Y.nearest_source(4, 2).tolist() == [0, 0, 1, 1] and Y.nearest_source(2, 4).tolist() == [1, 3]
    assert Y.nearest_source(3, 10).tolist() == [1, 5, 8]                                   # shrinking: the pixel centres


def test_sheet_layout_and_event_residual():
    case = C.panel_case('events_39x51_on_45x61')
    s = Y.sheet(lut=lut(), **case)
    H, W, g, t = 45, 61, 8, 16
    assert s.shape == (3 * H + 4 * g + 3 * t, 3 * W + 4 * g, 3)
    inside = np.zeros(s.shape[:2], bool)
    for r in range(3):
        for k in range(3):
            y0, x0 = g + t + r * (H + g + t), g + k * (W + g)
            inside[y0:y0 + H, x0:x0 + W] = True
    assert np.all(s[~inside] == 255) and inside.sum() == 9 * H * W
    y0, x0 = g + t + 2 * (H + g + t), g
    a, b, res = (s[y0:y0 + H, x0 + k * (W + g):x0 + k * (W + g) + W].astype(int) for k in range(3))
    assert np.array_equal(res, np.abs(a - b)) and np.all(res[..., 2] == 0)
    assert (a[..., :2] < b[..., :2]).any()                                  # where uint8 subtraction would wrap
    assert a[0, 0].tolist() == [255, 1, 0] and b[0, 0].tolist() == [0, 255, 0]


def test_package_numpy_route_equals_the_yardstick():
    from evennicer_slam_amd import frame_vis as FV
    for name in C.PANEL_CASES:
        case = C.panel_case(name)
        sheet, stats = FV.panels_numpy(**case)
        assert np.array_equal(sheet, Y.sheet(lut=lut(), **case)), name
        want = Y.stats(case['gt_depth'], case['gt_color'], case['depth'], case['color'])
        assert stats[0] == want[0]
        for k in range(1, 8):
            assert (np.isnan(want[k]) and np.isnan(stats[k])) or abs(stats[k] - want[k]) <= 4096 * C.U * want[4 + k % 4], (name, k)
    for name in C.SSIM_CASES:
        x, y = C.ssim_case(name)
        assert abs(FV.ssim_numpy(x, y) - Y.ssim(x, y)[0]) <= C.SSIM_TOL, name


def test_plasma_table_is_matplotlibs():
    cm = pytest.importorskip("matplotlib.cm")
    assert np.array_equal(lut(), cm.plasma(np.arange(256), bytes=True)[:, :3])


def test_ssim_yardstick_by_hand():
    x, _ = C.ssim_case('identical_45x61')
    mean, m = Y.ssim(x, x)
    assert mean == 1.0 and np.all(m == 1.0)
    x, y = C.ssim_case('one_pixel_11x11')
    mean, m = Y.ssim(x, y)
    w = Y.window()
    a, b = x[..., 0].astype(np.float64), y[..., 0].astype(np.float64)
    ux, uy = (w * a).sum(), (w * b).sum()
    vx, vy, vxy = (w * a * a).sum() - ux * ux, (w * b * b).sum() - uy * uy, (w * a * b).sum() - ux * uy
    want = (2 * ux * uy + 1e-4) * (2 * vxy + 9e-4) / ((ux * ux + uy * uy + 1e-4) * (vx + vy + 9e-4))
    assert m.shape == (1, 1, 1) and abs(mean - want) <= C.SSIM_TOL


def test_ssim_yardstick_against_skimage():
    metrics = pytest.importorskip("skimage.metrics")
    for name in C.SSIM_CASES:
        x, y = C.ssim_case(name)
        per = [metrics.structural_similarity(x[..., c].astype(np.float64), y[..., c].astype(np.float64), gaussian_weights=True,
                                             sigma=1.5, use_sample_covariance=False, data_range=1, full=True)[1][5:-5, 5:-5]
               for c in range(x.shape[2])]
        assert np.abs(np.stack(per, -1) - Y.ssim(x, y)[1]).max() <= C.SSIM_TOL, name


def test_exports_present_in_header_binding_and_library():
    import ctypes
    import __graft_entry__ as G
    G.build()
    import evennicer_slam_amd as E
    header = open(os.path.join(ROOT, "include", "enslam_hip.h")).read()
    handle = ctypes.CDLL(E.LIB_PATH)
    for name in ("enslam_vis_panels_workspace", "enslam_vis_panels", "enslam_ssim_workspace", "enslam_ssim"):
        assert re.search(r"\b%s\s*\(" % name, header) and name in E._lib.EXPORTS and hasattr(handle, name), name
    from evennicer_slam_amd import functional as EF
    th, tw = (int(re.search(r"#define ENSLAM_SSIM_TILE_%s (\d+)" % a, header).group(1)) for a in "HW")
    assert EF.SSIM_TILE == (th, tw) == C.SSIM_TILE
    with pytest.raises(NotImplementedError):
        EF.vis_panels(torch.zeros(4, 4), torch.zeros(4, 4, 3), torch.zeros(4, 4), torch.zeros(4, 4, 3))
    with pytest.raises(NotImplementedError):
        EF.ssim(torch.zeros(11, 11, 1), torch.zeros(11, 11, 1))


class StubRenderer:
    """render_img returns canned tensors and records the pose it was given"""

    def __init__(self, depth, color):
        self.depth, self.color, self.calls = depth, color, []

    def render_img(self, c, decoders, c2w, device, stage, gt_depth=None):
        self.calls.append(dict(c2w=c2w.clone(), stage=stage, gt_depth=gt_depth, grad=torch.is_grad_enabled()))
        return self.depth, torch.zeros_like(self.depth), self.color


def test_visualizer_on_the_cpu_route(tmp_path):
    from PIL import Image
    from evennicer_slam_amd import frame_vis as FV
    from evennicer_slam_amd.common import get_camera_from_tensor
    case = C.panel_case('events_39x51_on_45x61')
    t = {k: (None if v is None else torch.from_numpy(v) if isinstance(v, np.ndarray) else v) for k, v in case.items()}
    logged = []
    stub = StubRenderer(t['depth'].double(), t['color'].double())
    v = FV.Visualizer(5, 2, str(tmp_path / 'vis'), stub, verbose=False, experiment=types.SimpleNamespace(log=logged.append),
                      device='cpu', stage='tracker')
    assert os.path.isdir(tmp_path / 'vis') and v.last_stats is None
    cam = torch.tensor([0.9, 0.1, -0.2, 0.3, 0.5, -0.25, 1.5])
    for idx, it in ((3, 0), (5, 1), (0, 3)):                                # gated off by freq / inside_freq
        assert v.vis(idx, it, t['gt_depth'], t['gt_color'], cam, None, None) is None
    assert not stub.calls and not os.listdir(tmp_path / 'vis') and not logged
    s2 = v.vis(10, 4, t['gt_depth'], t['gt_color'], cam, None, None)         # a camera tensor
    want = torch.cat([get_camera_from_tensor(cam), torch.tensor([[0., 0., 0., 1.]])])
    assert torch.equal(stub.calls[0]['c2w'], want) and stub.calls[0]['stage'] == 'color' and not stub.calls[0]['grad']
    assert stub.calls[0]['gt_depth'] is t['gt_depth']
    two = dict(case, gt_event=None, pred_event=None)
    assert np.array_equal(v.last_sheet, Y.sheet(lut=lut(), **two)) and s2 is v.last_stats
    img = Image.open(tmp_path / 'vis' / '00010_0004.jpg')
    assert img.size == (3 * 61 + 32, 2 * 45 + 24 + 32)
    c2w = torch.eye(4)
    s3 = v.vis_event(5, 0, t['gt_depth'], t['gt_color'], None, t['gt_event'], t['pred_event'], [t['gt_event']], [t['pred_event']],
                     c2w, None, None)                                        # a matrix, three rows
    assert torch.equal(stub.calls[1]['c2w'], c2w) and tuple(stub.calls[1]['c2w'].shape) == (4, 4)
    assert np.array_equal(v.last_sheet, Y.sheet(lut=lut(), **case))
    assert Image.open(tmp_path / 'vis' / '00005_0000.jpg').size == (215, 3 * 45 + 32 + 48)
    assert sorted(os.listdir(tmp_path / 'vis')) == ['00005_0000.jpg', '00010_0004.jpg']
    ys = Y.stats(case['gt_depth'], case['gt_color'], case['depth'], case['color'])
    assert set(s3) == {'depth_l1', 'psnr', 'psnr_valid', 'n_valid'} and s3 == s2 and s3['n_valid'] == int(ys[0])
    assert abs(s3['depth_l1'] - ys[1] / ys[0]) <= 1e-12 * ys[1] / ys[0]
    assert abs(s3['psnr'] + 10 * np.log10(ys[2] / (3 * 45 * 61))) < 1e-9 and abs(s3['psnr_valid'] + 10 * np.log10(ys[3] / (3 * ys[0]))) < 1e-9
    assert len(logged) == 2 and logged[0]['Frame'] == 10 and logged[1]['Frame'] == 5
    assert logged[0]['Depth']['GT Depth'].dtype == np.uint8 and logged[0]['Depth']['GT Depth'].shape == (45, 61, 3)
    assert 'Event' not in logged[0] and 'GT Event Blurred 1 (tracker)' in logged[1]['Event']
    assert logged[1]['Rendering (tracker)'] == s3 and 'wandb' not in str(type(logged[1]))


def test_render_metrics_on_the_cpu_route():
    from evennicer_slam_amd import frame_vis as FV
    case = C.panel_case('plain_50x70')
    t = {k: torch.from_numpy(case[k]) for k in ('gt_depth', 'gt_color', 'depth', 'color')}
    m = FV.render_metrics(t['depth'], t['color'], t['gt_depth'], t['gt_color'])
    ys = Y.stats(case['gt_depth'], case['gt_color'], case['depth'], case['color'])
    assert abs(m['depth_l1'] - ys[1] / ys[0]) < 1e-12 and abs(m['psnr'] + 10 * np.log10(ys[2] / (3 * 50 * 70))) < 1e-9
    assert abs(m['ssim'] - Y.ssim(Y.clip01(case['color']), Y.clip01(case['gt_color']))[0]) <= C.SSIM_TOL
    same = FV.render_metrics(t['gt_depth'], t['gt_color'], t['gt_depth'], t['gt_color'], ssim=False)
    assert same == dict(depth_l1=0.0, psnr=float('inf'), ssim=None)


def test_slam_without_vis_constructs_no_visualizer(tmp_path, monkeypatch):
    import inspect
    from evennicer_slam_amd import frame_vis as FV
    from evennicer_slam_amd import slam as S
    from evennicer_slam_amd.synthetic import demo_config
    made = []
    monkeypatch.setattr(FV, 'Visualizer', lambda *a, **k: made.append((a, k)) or types.SimpleNamespace())
    assert inspect.signature(S.SLAM.__init__).parameters['vis'].default is False
    cam = dict(H=12, W=16, fx=14.0, fy=14.0, cx=7.5, cy=5.5)
    cfg = demo_config('unused', 'unused', cam, device='cpu')
    plain = S.SLAM(cfg, [None] * 3, str(tmp_path / 'plain'), device='cpu')
    assert not made and plain.vis_tracker is None and plain.vis_mapper is None
    assert sorted(os.listdir(tmp_path / 'plain')) == ['ckpts']               # no new folders
    cfg['tracking'].update(vis_freq=7, vis_inside_freq=3)
    shown = S.SLAM(cfg, [None] * 3, str(tmp_path / 'shown'), device='cpu', vis=True)
    assert len(made) == 2 and shown.vis_tracker is not None and shown.vis_mapper is not None
    (_, trk), (_, mp) = made
    assert (trk['freq'], trk['inside_freq'], trk['stage']) == (7, 3, 'tracker') and trk['vis_dir'].endswith('tracking_vis')
    assert (mp['freq'], mp['inside_freq'], mp['stage']) == (50, 30, 'mapper') and mp['vis_dir'].endswith('mapping_vis')
