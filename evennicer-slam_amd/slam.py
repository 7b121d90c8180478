"""Single-process run harness: the reference's `run.py` -> `EvenNICER_SLAM.run` starts a tracker, a
mapper and a coarse-mapper PROCESS that hand the map over through shared tensors (src/EvenNICER_SLAM.py:278-332).  Here
the same per-frame schedule runs in one process on one GPU, tracker and mapper alternating on the HIP path:

  frame 0         pose = ground truth (Tracker.py:283-285); `mapping.iters_first` joint iterations on the first frame
  frame i > 0     tracker: constant-speed or last-pose initialisation (Tracker.py:295-303), `tracking.iters` camera
                  iterations (`TrackerIteration.optimize_cam_in_batch`, RGB-D term; the event term when an event network
                  is given), the candidate with the smallest loss is kept (:321-330)
  every `mapping.every_frame`-th frame: `mapping.iters` joint iterations (`mapper.MapperIteration`: frustum-masked grids,
                  colour decoder, local BA over the window of keyframes -- the reference's `global` selection: random
                  keyframes + the latest one + the current frame, Mapper.py:280-303; with
                  `mapping.keyframe_selection_method: 'overlap'` the keyframes that see the current frame's points,
                  `mapper.keyframe_selection_overlap`) and `update_para_from_mapping`
                  then -- `cfg['coarse']` -- the COARSE mapper's round on the same frame (the reference's third process,
                  EvenNICER_SLAM.py:303-311: `Mapper(..., coarse_mapper=True)` runs the same schedule with stage `coarse`
                  only, every voxel of `grid_coarse` optimisable, no depth guidance, no BA; Mapper.py:133-136,326-328,
                  460-461,550,797-798)
  keyframes       every `mapping.keyframe_every` frames (Mapper.py:687-692)
  end             `Logger.log` checkpoint in the reference's format, ATE through `eval_ate.evaluate_checkpoint`

`SLAM.prefit_decoders` stands in for the pretrained ConvONet decoders the reference loads (EvenNICER_SLAM.load_pretrain;
the checkpoints are not in the image): decoders and grids are fitted jointly to a few ground-truth-posed frames of the
sequence, the decoders are kept, the grids are re-initialised -- the run itself then optimises grids (and the colour decoder)
only, as the reference does.

THE SPARSE RGB-D SCHEDULE.  `event.schedule` picks what the tracker is handed per frame; `frame_plan` is the one place that
decides it.  'dense' (the default): RGB-D term and the frame's own event image on every frame, the previous frame's colour as
the event term's first image, the candidate with the smallest summed loss.  'reference': src/Tracker.py:350-375,439-442,461-466
as written -- the RGB-D term only where idx % event.rgbd_every_frame == 0, the event term on every frame against the events
summed since the last frame with idx % mapping.every_frame == 0, that frame's colour as the first image, the candidate with
the smallest EVENT loss.  `event.depth_on_event_frames` says what guides the reduced-resolution render of a frame without
RGB-D: 'measured' (the reference: that frame's depth image, which a sensor that delivers RGB-D every k-th frame does not have),
'forecast' (the last measured depth image warped into the frame's initial pose, functional.depth_forecast) or 'none'.  With
'forecast' and 'none' the colour and depth images of a frame without RGB-D are dropped as soon as the dataset has handed them
over: tracker, mapper, keyframes and figures never see them.

THE POSE PRIOR.  `tracking.motion_prior` says where the camera iterations of a frame start: 'const_speed' (the default, the
reference's constant-speed pose) or 'cmax' (opt-in): the six-component camera velocity that maximises the contrast of the
frame interval's events (event_cmax.estimate_motion('rigid')) under the last measured depth image warped into the previous
pose, composed onto that pose (`SLAM._cmax_prior`).  It needs `data.event_stream` and `data.frame_stamps` on an uncropped
sensor; `tracking.cmax_min_events` (500) and `tracking.cmax_iters` (10 accepted steps at most) bound it.  A frame falls back to
the constant-speed pose, counted in `motion_prior_stats`, with too few events, without a depth image yet, with a result that
is not finite and with a contrast that did not rise above f(theta0).  Measured on the analytic room the prior does not
help -- the six-parameter contrast rises without bound along v_z and the estimate follows it -- so the default stays 'const_speed'.
`tracking.cmax_reg` ('none'; 'divergence' or 'deformation') with `tracking.cmax_reg_weight` (8) subtracts the collapse regulariser
of event_cmax.py from that contrast, and `tracking.cmax_max_reg` (unset) adds a fallback, 'collapsed', for an estimate whose
regulariser exceeds it.  Measured the same way, the regularised prior no longer loses the trajectory and still does not help.

Mesh extraction is opt-in: `SLAM.get_mesh` (or `run(mesh_file=...)`) runs `mesher.Mesher.get_mesh` on the run's keyframes and
poses.  The per-iteration figures of the reference's Visualizer are opt-in too: `SLAM(vis=True)` builds one
`frame_vis.Visualizer` for the tracker (`tracking.vis_freq` / `vis_inside_freq`, folder `tracking_vis`) and one for the mapper
(`mapping.vis_freq` / `vis_inside_freq`, folder `mapping_vis`) and calls them where Tracker.py:306-308,444-447 and
Mapper.py:705-713 do; `mapping.no_vis_on_first_frame` is honoured (absent: False).  Not here: wandb."""
import os
import time
import types
import typing

import numpy as np
import torch

from . import functional as EF
from .common import get_camera_from_tensor, get_tensor_from_camera
from .decoder import get_model
from .eval_ate import Logger, evaluate_checkpoint
from .mapper import FusedAdam, MapperIteration, keyframe_selection_overlap
from .renderer import Renderer
from .scene import GRID_KEYS, grid_init, scene_bound
from .tracker import CameraParameter, TrackerIteration, camera_learning_rates

MAP_KEYS = ('grid_middle', 'grid_fine', 'grid_color')
SCHEDULES = ('dense', 'reference')
DEPTH_ON_EVENT_FRAMES = ('measured', 'forecast', 'none')
MOTION_PRIORS = ('const_speed', 'cmax')
CMAX_REGS = ('none', 'divergence', 'deformation')


class FrameStep(typing.NamedTuple):
    rgbd: bool              # the tracker's RGB-D term runs on this frame
    anchor: typing.Optional[int]    # the frame whose colour is pre_gt_color (None: the frame is not tracked)
    integrate: tuple        # the frames whose event images are summed into the event image the tracker gets
    map: bool               # the frame is mapped (the harness drops the extra round on a last frame it may not read)
    reset: bool             # the integration restarts after this frame


def frame_plan(n, every_frame, rgbd_every_frame=1, schedule='dense'):
    """What the harness does on each of n frames: a list of FrameStep.  Pure host function.
    'dense': RGB-D on every frame, the frame's own events, the previous frame's colour; rgbd_every_frame is ignored.
    'reference' (src/Tracker.py): rgbd = (idx % rgbd_every_frame == 0) (:357); the events of every tracked frame join the sum
    before its iterations (:351); after a frame with idx % every_frame == 0 that frame's colour becomes pre_gt_color and the sum
    restarts (:462-466).  Frame 0 is not tracked.  Mapped in both: frame 0, every every_frame-th frame and the last one."""
    if schedule not in SCHEDULES:
        raise ValueError(f"event.schedule must be one of {SCHEDULES} (got {schedule!r})")
    n, every_frame, rgbd_every_frame = int(n), int(every_frame), int(rgbd_every_frame)
    if every_frame < 1 or rgbd_every_frame < 1:
        raise ValueError(f"mapping.every_frame and event.rgbd_every_frame must be at least 1 (got {every_frame}, {rgbd_every_frame})")
    plan, anchor, since = [], None, []
    for idx in range(n):
        mapped = idx == 0 or idx % every_frame == 0 or idx == n - 1
        if schedule == 'dense':
            plan.append(FrameStep(True, idx - 1 if idx > 0 else None, (idx,) if idx > 0 else (), mapped, True))
            continue
        if idx > 0:
            since.append(idx)
        restart = idx % every_frame == 0
        plan.append(FrameStep(idx % rgbd_every_frame == 0, anchor if idx > 0 else None, tuple(since), mapped, restart))
        if restart:
            anchor, since = idx, []
    return plan


def frustum_mask(c2w, depth, shape, bound, cam):
    """Frustum feature selection (Mapper.get_mask_from_c2w, src/Mapper.py:114-186) in torch: voxels of a [D,H,W] grid
    that project into the image in front of the measured depth (+0.5 m), plus those within 0.5 m of the camera.
    Returns bool [D,H,W].  (The reference samples the depth with cv2.remap INTER_LINEAR and a zero border; the same
    bilinear lookup is F.grid_sample(align_corners=True, padding zeros).)"""
    H, W, fx, fy, cx, cy = (cam[k] for k in ('H', 'W', 'fx', 'fy', 'cx', 'cy'))
    dev = depth.device
    D_, H_, W_ = shape
    X, Y, Z = torch.meshgrid(torch.linspace(float(bound[0][0]), float(bound[0][1]), W_),
                             torch.linspace(float(bound[1][0]), float(bound[1][1]), H_),
                             torch.linspace(float(bound[2][0]), float(bound[2][1]), D_), indexing='ij')
    pts = torch.stack([X, Y, Z], -1).reshape(-1, 3).to(dev)
    c2w4 = torch.eye(4, device=dev, dtype=torch.float64)
    c2w4[:3] = c2w[:3].double().to(dev)
    w2c = torch.linalg.inv(c2w4)
    cam_pts = (w2c[:3, :3] @ pts.double().T + w2c[:3, 3:4]).T
    cam_pts[:, 0] *= -1
    K = torch.tensor([[fx, 0., cx], [0., fy, cy], [0., 0., 1.]], dtype=torch.float64, device=dev)
    uv = (K @ cam_pts.T).T
    z = uv[:, 2:3] + 1e-5
    uv = (uv[:, :2] / z).float()
    gx = 2 * uv[:, 0] / (W - 1) - 1
    gy = 2 * uv[:, 1] / (H - 1) - 1
    depths = torch.nn.functional.grid_sample(depth[None, None].float(), torch.stack([gx, gy], -1)[None, :, None, :],
                                             mode='bilinear', padding_mode='zeros', align_corners=True).reshape(-1, 1)
    mask = (uv[:, 0] < W) & (uv[:, 0] > 0) & (uv[:, 1] < H) & (uv[:, 1] > 0)
    depths = torch.where(depths == 0, depths.max(), depths)
    mask = mask & (0 <= -z[:, 0]) & (-z[:, 0] <= depths[:, 0].double() + 0.5)
    near = ((pts - c2w[:3, 3].to(dev, pts.dtype)[None]) ** 2).sum(1) < 0.25
    return (mask | near).reshape(W_, H_, D_).permute(2, 1, 0).contiguous()


def schedule_settings(cfg):
    """(event.schedule, event.rgbd_every_frame, event.depth_on_event_frames) of a configuration, defaults ('dense', 1, 'measured');
    ValueError for an unknown value and for a sparse schedule whose mapper would need images that frames without RGB-D lack."""
    e = cfg.get('event') or {}
    schedule = e.get('schedule', 'dense')
    rgbd_every = int(e.get('rgbd_every_frame', 1))
    depth_mode = e.get('depth_on_event_frames', 'measured')
    if schedule not in SCHEDULES:
        raise ValueError(f"event.schedule must be one of {SCHEDULES} (got {schedule!r})")
    if depth_mode not in DEPTH_ON_EVENT_FRAMES:
        raise ValueError(f"event.depth_on_event_frames must be one of {DEPTH_ON_EVENT_FRAMES} (got {depth_mode!r})")
    if schedule == 'reference':
        every = int(cfg['mapping']['every_frame'])
        if rgbd_every < 1:
            raise ValueError(f"event.rgbd_every_frame must be at least 1 (got {rgbd_every})")
        if depth_mode != 'measured' and every % rgbd_every:
            # the mapper needs the frame's images: without the measured ones it can only map frames that have RGB-D
            raise ValueError(f"mapping.every_frame ({every}) must be a multiple of event.rgbd_every_frame ({rgbd_every}) with "
                             f"event.depth_on_event_frames {depth_mode!r}: frames without RGB-D are not mapped")
    return schedule, rgbd_every, depth_mode


class SLAM:
    def __init__(self, cfg, dataset, output, device='cuda:0', event_net=None, verbose=False, static_shapes=False, vis=False,
                 experiment=None):
        self.cfg, self.dataset, self.output, self.device, self.verbose = cfg, dataset, output, device, verbose
        self.schedule, self.rgbd_every, self.depth_mode = schedule_settings(cfg)      # (refuses before anything is built)
        self.static_shapes = static_shapes
        self.scale = cfg['scale']
        self.H, self.W = cfg['cam']['H'] - 2 * cfg['cam']['crop_edge'], cfg['cam']['W'] - 2 * cfg['cam']['crop_edge']
        self.fx, self.fy = cfg['cam']['fx'], cfg['cam']['fy']
        self.cx, self.cy = cfg['cam']['cx'] - cfg['cam']['crop_edge'], cfg['cam']['cy'] - cfg['cam']['crop_edge']
        self.cam = dict(H=self.H, W=self.W, fx=self.fx, fy=self.fy, cx=self.cx, cy=self.cy)
        self.bound = scene_bound(cfg['mapping']['bound'], self.scale, cfg['grid_len']['bound_divisible'])   # load_bound
        self.shared_decoders = get_model(cfg).to(device)
        self.shared_decoders.bound = self.bound
        for name in ('middle_decoder', 'fine_decoder', 'color_decoder'):
            getattr(self.shared_decoders, name).bound = self.bound
        self.shared_decoders.coarse_decoder.bound = self.bound * cfg['model']['coarse_bound_enlarge']
        # channels_last_3d: the reference's grid tensors stored voxel-major (read in place by the kernels; cfg['grid_memory_format']
        # = 'contiguous' keeps the reference's strides)
        mf = None if (cfg.get('grid_memory_format', 'channels_last_3d') == 'contiguous' or str(device) == 'cpu') else torch.channels_last_3d
        self.shared_c = grid_init(self.bound, cfg['grid_len'], cfg['model']['c_dim'], cfg['model']['coarse_bound_enlarge'], device,
                                  memory_format=mf)
        n = len(dataset)
        self.n_img = n
        self.estimate_c2w_list = torch.zeros((n, 4, 4))
        self.gt_c2w_list = torch.zeros((n, 4, 4))
        self.ckptsdir = os.path.join(output, 'ckpts')
        os.makedirs(self.ckptsdir, exist_ok=True)
        self.nice = True
        self.renderer = Renderer(cfg, None, self)
        if event_net is not None and (cfg.get('event') or {}).get('net_backend', 'torch') == 'hip':
            from .event import HipUNet2Heads, compile_event_net
            if not isinstance(event_net, HipUNet2Heads):
                event_net = compile_event_net(event_net)
        self.event_net = event_net
        self.low_gpu_mem = False
        self.logger = Logger(cfg, None, self)
        self.tracker = TrackerIteration(cfg, None, self)
        e = cfg.get('event') or {}
        # radius (full-resolution pixels) and hole filling of the depth forecast (functional.depth_forecast)
        self.forecast_radius = float(e.get('forecast_radius', 1.0))
        self.forecast_fill = bool(e.get('forecast_fill', True))
        self._last_rgbd = None                              # (frame index, its depth image) of the last frame with RGB-D
        tr = cfg['tracking']
        self.motion_prior = tr.get('motion_prior', 'const_speed')
        if self.motion_prior not in MOTION_PRIORS:
            raise ValueError(f"tracking.motion_prior must be one of {MOTION_PRIORS} (got {self.motion_prior!r})")
        self.cmax_min_events, self.cmax_iters = int(tr.get('cmax_min_events', 500)), int(tr.get('cmax_iters', 10))
        # frames whose initial pose came from the events, the fallbacks by cause, and the seconds the prior took
        self.motion_prior_stats = dict(cmax=0, few_events=0, no_depth=0, not_finite=0, no_rise=0, seconds=0.0)
        # the collapse regulariser of the prior's objective (event_cmax.estimate_motion's reg / reg_weight), and the optional
        # ceiling on the estimate's R above which the frame falls back (counted under 'collapsed', a key only then)
        self.cmax_reg = tr.get('cmax_reg', 'none')
        if self.cmax_reg not in CMAX_REGS:
            raise ValueError(f"tracking.cmax_reg must be one of {CMAX_REGS} (got {self.cmax_reg!r})")
        self.cmax_reg_weight = float(tr.get('cmax_reg_weight', 8.0))
        if not np.isfinite(self.cmax_reg_weight):
            raise ValueError(f"tracking.cmax_reg_weight must be finite (got {self.cmax_reg_weight})")
        self.cmax_max_reg = None if tr.get('cmax_max_reg') is None else float(tr['cmax_max_reg'])
        if self.cmax_max_reg is not None:
            self.motion_prior_stats['collapsed'] = 0
        if self.motion_prior == 'cmax':
            if getattr(dataset, '_stream', None) is None:
                raise ValueError("tracking.motion_prior = 'cmax' needs the time-stamped events of data.event_stream and "
                                 "data.frame_stamps")
            if cfg['cam']['crop_edge'] != 0 or cfg['cam'].get('crop_size') is not None:
                raise ValueError("tracking.motion_prior = 'cmax' needs an uncropped sensor (cam.crop_edge 0, no cam.crop_size): "
                                 "the stream's pixels are the raw frame's")
        self._gtracks = {}                                  # captured camera iterations (_track_graphed)
        self.keyframe_dict, self.keyframe_list = [], []
        self.timing = dict(track=0.0, map=0.0)
        self.vis_tracker = self.vis_mapper = None
        if vis:
            from .frame_vis import Visualizer
            tr, mp = cfg['tracking'], cfg['mapping']
            self.vis_tracker = Visualizer(freq=tr.get('vis_freq', 50), inside_freq=tr.get('vis_inside_freq', 25),
                                          vis_dir=os.path.join(output, 'tracking_vis'), renderer=self.renderer, verbose=verbose,
                                          experiment=experiment, device=device, stage='tracker')
            self.vis_mapper = Visualizer(freq=mp.get('vis_freq', 50), inside_freq=mp.get('vis_inside_freq', 30),
                                         vis_dir=os.path.join(output, 'mapping_vis'), renderer=self.renderer, verbose=verbose,
                                         experiment=experiment, device=device, stage='mapper')

    # ---------------------------------------------------------------- tracker side
    def update_para_from_mapping(self):
        """Tracker.update_para_from_mapping (Tracker.py:247-259): the tracker's own copies of the map."""
        import copy
        self.tracker.decoders = copy.deepcopy(self.shared_decoders)
        for p in self.tracker.decoders.parameters():
            p.requires_grad_(False)
        self.tracker.c = {k: v.detach().clone() for k, v in self.shared_c.items()}

    def track(self, idx, gt_color, gt_depth, gt_event, gt_mask, pre_gt_color, rgbd=True, forecast=False, by_event=False):
        """The camera iterations of frame idx.  As the dense schedule calls it (the defaults): RGB-D term on, the candidate with the
        smallest summed loss.  The reference schedule passes the plan's `rgbd`, the integrated events as gt_event and by_event=True
        (the candidate with the smallest event loss, Tracker.py:439-442); forecast=True guides the reduced-resolution render by
        the last measured depth warped into the frame's initial pose (gt_depth is then None)."""
        t = getattr(self, '_track_cfg', None) or self.cfg['tracking']
        pre = self.estimate_c2w_list[idx - 1].to(self.device)
        if t.get('const_speed_assumption', True) and idx - 2 >= 0:         # Tracker.py:295-301
            pre = pre.float()
            delta = pre @ self.estimate_c2w_list[idx - 2].to(self.device).float().inverse()
            est = delta @ pre
        else:
            est = pre
        prior = 'const_speed'
        if self.motion_prior == 'cmax':
            est, prior = self._cmax_prior(idx, est)
        # (predictor 'model': the contrast-threshold model predicts the events, no network is needed)
        has_predictor = self.event_net is not None or self.cfg['event'].get('predictor', 'net') == 'model'
        use_event = has_predictor and self.cfg['event'].get('activate_events', False)
        if not rgbd and not use_event:
            # no RGB-D image and no event term: the frame has no loss, its pose stays the initialisation and nothing is launched
            c2w = torch.eye(4, device=self.device)
            c2w[:3] = est[:3].float()
            return c2w
        by_event = by_event and use_event
        guide = self._forecast_depth(est) if (forecast and use_event) else None
        extra = {} if guide is None else dict(guide_depth=guide)
        rates = camera_learning_rates(t)
        if t.get('graphed', False) and int(t['iters']) > 0:
            return self._track_graphed(idx, est, gt_color, gt_depth, gt_event, gt_mask, pre_gt_color, t, use_event, rgbd, guide,
                                       by_event)
        cam = CameraParameter(get_tensor_from_camera(est.detach()).to(self.device), rates)
        opt = cam.opt
        best, best_loss, first_loss = cam.value().clone(), None, None
        for it in range(t['iters']):
            camera_tensor = cam.tensor()
            out = self.tracker.optimize_cam_in_batch(camera_tensor, est, gt_color, gt_depth, gt_event, gt_mask, t['pixels'], opt,
                                                     idx, it, pre_gt_color, rgbd=rgbd, event=use_event,
                                                     scale_factor=self.cfg['event'].get('scale_factor', 0.1), **extra)
            if by_event:
                loss = out[1]                                               # Tracker.py:439-442: "it is always available"
            else:
                loss = out[0] + (out[1] if (use_event and out[1] is not None) else 0.0)
            if it == 0:
                first_loss = loss
            # (by_event: a loss that is not a number is taken, as the graphed route's device argmin takes it -- a poisoned input
            # shows in the pose instead of leaving the initialisation in place)
            if best_loss is None or loss < best_loss or (by_event and loss != loss):   # Tracker.py:321-330 (candidate with the least loss)
                best_loss, best = loss, cam.value().clone()
            if self.vis_tracker is not None and gt_color is not None and gt_depth is not None:
                self._vis_camera_iteration(idx, it, gt_depth, gt_color, cam.value(), out if use_event else None)
        c2w = torch.eye(4, device=self.device)
        c2w[:3] = get_camera_from_tensor(best)
        if self.verbose:
            gt = self.gt_c2w_list[idx][:3, 3].to(self.device)
            print(f'frame {idx}: tracking loss {first_loss} -> {best_loss}; translation error init ({prior}) '
                  f'{float((est[:3, 3] - gt).norm()):.4f} -> {float((c2w[:3, 3] - gt).norm()):.4f} m', flush=True)
        return c2w

    def _cmax_prior(self, idx, fallback):
        """(est, what made it) of frame idx under tracking.motion_prior = 'cmax': the previous estimated pose composed with
        the camera motion that the events of (stamp[idx-1], stamp[idx]] imply.  The six velocity components maximise the
        contrast of those events (event_cmax.estimate_motion('rigid'), from the velocity of the last two estimated poses) under
        the depth image of the last frame with RGB-D warped into the previous pose at the sensor's full size.  `fallback`, the
        constant-speed pose, is returned -- and the cause counted in motion_prior_stats -- when the interval has fewer than
        tracking.cmax_min_events events, when no depth image has been kept yet, when the result is not finite and when the
        contrast did not rise above f(theta0).  tracking.cmax_reg ('divergence' or 'deformation') maximises the contrast less
        tracking.cmax_reg_weight (8) times the collapse regulariser instead; the rise is still asked of the pure contrast.
        tracking.cmax_max_reg, when set, also sends an estimate whose regulariser (the mean absolute divergence or
        deformation of its warp) exceeds it back to the constant-speed pose, counted under 'collapsed'."""
        from . import event_cmax as CM
        stats, t_start = self.motion_prior_stats, time.perf_counter()

        def back(cause):
            stats[cause] += 1
            stats['seconds'] += time.perf_counter() - t_start
            return fallback, f'const_speed, cmax fell back: {cause}'
        stream, t0, t1 = self.dataset.event_slice(idx)
        if len(stream) < self.cmax_min_events:
            return back('few_events')
        if self._last_rgbd is None:
            return back('no_depth')
        pre = self.estimate_c2w_list[idx - 1].double()
        theta0 = [0.0] * 6
        if idx >= 2:
            ta = self.dataset.event_slice(idx - 1)[1]
            if t0 > ta:
                theta0 = CM.camera_velocity(self.estimate_c2w_list[idx - 2], pre, t0 - ta)
        src, depth = self._last_rgbd
        M = EF.relative_camera_matrix(self.estimate_c2w_list[src], pre)
        depth = EF.depth_forecast(depth.float().contiguous(), self.cam, M, (self.H, self.W), radius=self.forecast_radius, z_near=0.0,
                                  fill=self.forecast_fill).to(stream.device)
        reg = {} if self.cmax_reg == 'none' else dict(reg=self.cmax_reg, reg_weight=self.cmax_reg_weight)
        res = CM.estimate_motion(stream, (self.fx, self.fy, self.cx, self.cy), 'rigid', self.H, self.W, theta0=theta0, t_ref=t0,
                                 iters=self.cmax_iters, depth=depth, **reg)
        self.motion_prior_last = res
        if not (np.all(np.isfinite(res['theta'])) and np.isfinite(res['trace'][-1])):
            return back('not_finite')
        rise = res['f_trace'] if reg else res['trace']                  # the pure contrast, whatever was maximised
        if not rise[-1] > rise[0]:
            return back('no_rise')
        if self.cmax_max_reg is not None:
            R = res['reg_trace'][-1] if reg else CM.regulariser(stream, (self.fx, self.fy, self.cx, self.cy), 'rigid', res['theta'],
                                                                 self.H, self.W, t_ref=t0, depth=depth)[0]
            if not R <= self.cmax_max_reg:
                return back('collapsed')
        est = (pre @ CM.relative_motion(res['theta'], t1 - t0)).float().to(self.device)
        stats['cmax'] += 1
        stats['seconds'] += time.perf_counter() - t_start
        return est, 'cmax'

    def _forecast_depth(self, est):
        """Guidance depth of a frame without RGB-D at the event resolution: the depth image of the last frame that had one, at that
        frame's final estimated pose (after its mapping round and BA), warped into the initial pose `est` of this frame
        (functional.depth_forecast).  Once per frame, constant over its camera iterations."""
        if self._last_rgbd is None:
            raise RuntimeError("depth forecast: no frame with RGB-D yet")
        src, depth = self._last_rgbd
        M = EF.relative_camera_matrix(self.estimate_c2w_list[src], est)
        size = self.tracker.event_size(self.cfg['event'].get('scale_factor', 0.1))
        return EF.depth_forecast(depth.float().contiguous(), self.cam, M, size, radius=self.forecast_radius, z_near=0.0,
                                 fill=self.forecast_fill)

    def _vis_camera_iteration(self, idx, it, gt_depth, gt_color, camera_tensor, out):
        """The tracker's figure of camera iteration `it` (Tracker.py:444-447): with the event term `out` is the tuple of
        `optimize_cam_in_batch` (low-resolution ground-truth events at [3], predicted events at [4], with blur the lists at
        [5], [6]); without it (None) the two-row figure."""
        v, trk = self.vis_tracker, self.tracker
        if not v.due(idx, it):
            return
        if out is not None and out[4] is not None:
            blurred = (out[5], out[6]) if len(out) == 10 else ([], [])
            v.vis_event(idx, it, gt_depth, gt_color, None, out[3], out[4], blurred[0], blurred[1], camera_tensor.detach(), trk.c,
                        trk.decoders)
        else:
            v.vis(idx, it, gt_depth, gt_color, camera_tensor.detach(), trk.c, trk.decoders)

    def _track_graphed(self, idx, est, gt_color, gt_depth, gt_event, gt_mask, pre_gt_color, t, use_event, rgbd=True, guide=None,
                       by_event=False):
        """`track` with the camera iterations as replays of a hipGraph (tracker.GraphedCameraIteration, captured at the first tracked
        frame of its shape and kept): per frame the initial pose goes into the captured camera tensor, the optimiser is reset, the
        images are copied in (set_frame draws the frame's pixels ahead) and the map the mapper has just published is copied into the
        captured tensors (refresh_map); the losses stay on the device and the least-loss candidate (Tracker.py:321-330; by_event:
        the least EVENT loss, :439-442) is picked by one argmin behind the last iteration -- no host round trip per iteration.
        The sparse schedule alternates between two shapes, RGB-D + event and event only: one captured graph each, in
        `self._gtracks` keyed by (iterations, pixels, event term, RGB-D term); nothing is captured again per frame."""
        from .tracker import GraphedCameraIteration
        iters, n = int(t['iters']), int(t['pixels'])
        sf = self.cfg['event'].get('scale_factor', 0.1)
        rates = camera_learning_rates(t)
        init = get_tensor_from_camera(est.detach()).to(self.device).float()
        images = (gt_color if rgbd else None, gt_depth)                  # (the event-only shape never looks at the colour image)
        events = (gt_event, gt_mask, pre_gt_color) if use_event else (None, None, None)
        key = (iters, n, use_event, bool(rgbd))
        g = self._gtracks.get(key)
        if g is None or g['rates'] != rates:
            cam = CameraParameter(init, rates)
            git = GraphedCameraIteration(self.tracker, cam.tensor, cam.opt, images[0], images[1], *events, batch_size=n, rgbd=rgbd,
                                         event=use_event, scale_factor=sf, n_draws=iters, guide=guide)
            g = self._gtracks[key] = dict(key=key, cam=cam, rates=rates, git=git,
                                          cams=torch.empty((iters, 7), dtype=torch.float32, device=self.device),
                                          losses=torch.empty(iters, dtype=torch.float64, device=self.device))
        cam, git = g['cam'], g['git']
        cam.restart(init, rates)
        git.refresh_map()                                   # (update_para_from_mapping replaced the tracker's map objects)
        git.set_frame(images[0], images[1], *events, guide=guide)
        for it in range(iters):
            l_rgbd, l_event, _l_mask = git.step()
            g['losses'][it].copy_(l_event if by_event else (l_rgbd + l_event if use_event else l_rgbd))
            g['cams'][it].copy_(cam.value().reshape(-1))         # the candidate of this loss: the pose AFTER the step (Tracker.py:321-330)
            if self.vis_tracker is not None and gt_color is not None and gt_depth is not None:
                # between two replays, never inside a capture: the captured camera tensor
                self._vis_camera_iteration(idx, it, gt_depth, gt_color, cam.value().reshape(-1), None)
        k = torch.argmin(g['losses'])
        best = g['cams'][k]
        c2w = torch.eye(4, device=self.device)
        c2w[:3] = get_camera_from_tensor(best)
        if self.verbose:
            gt = self.gt_c2w_list[idx][:3, 3].to(self.device)
            print(f'frame {idx}: tracking loss {float(g["losses"][0])} -> {float(g["losses"][k])} (graphed); translation error init '
                  f'{float((est[:3, 3] - gt).norm()):.4f} -> {float((c2w[:3, 3] - gt).norm()):.4f} m', flush=True)
        return c2w

    # ---------------------------------------------------------------- mapper side
    def map(self, idx, gt_color, gt_depth, cur_c2w, iters):
        m = self.cfg['mapping']
        window = m.get('mapping_window_size', 5)
        frames = []
        if self.keyframe_dict:                                               # keyframe selection, Mapper.py:280-303
            n_old = len(self.keyframe_dict) - 1
            method = m.get('keyframe_selection_method', 'global')
            if method == 'overlap':                                          # Mapper.py:290-293
                pick = keyframe_selection_overlap(gt_color, gt_depth, cur_c2w, self.keyframe_dict[:-1], max(window - 2, 0),
                                                  self.cam, device=self.device)
            elif method == 'global':
                pick = list(np.random.permutation(n_old)[:max(window - 2, 0)]) if n_old > 0 else []
            else:
                raise ValueError(f"mapping.keyframe_selection_method {method!r}: 'global' or 'overlap'")
            pick = sorted(set(int(p) for p in pick) | {len(self.keyframe_dict) - 1})
            oldest = min(pick)
            for k in pick:
                kf = self.keyframe_dict[k]
                frames.append(dict(depth=kf['depth'], color=kf['color'], c2w=kf['est_c2w'], fixed=(k == oldest), key=k))
        frames.append(dict(depth=gt_depth, color=gt_color.float(), c2w=cur_c2w, fixed=False, key=-1))
        masks = None
        if m.get('frustum_feature_selection', True):                         # Mapper.py:330-361
            masks = {k: frustum_mask(cur_c2w, gt_depth, tuple(self.shared_c[k].shape[2:]), self.bound, self.cam) for k in MAP_KEYS}
        ba = bool(m.get('BA', False)) and len(self.keyframe_dict) > 4 and idx > 0      # Mapper.py:700: BA once 4 keyframes exist
        cfg = dict(self.cfg)
        # the first frame is mapped with lr_first_factor (Mapper.py:794-796: lr_factor = lr_first_factor with iters_first)
        cfg['mapping'] = dict(m, BA=ba, lr_factor=m.get('lr_first_factor', m['lr_factor']) if idx == 0 else m['lr_factor'])
        it = MapperIteration(cfg, self.renderer, self.shared_c, self.shared_decoders, frames, self.cam, masks=masks, keys=MAP_KEYS,
                             static_shapes=self.static_shapes)
        loss = None
        show = self.vis_mapper is not None and not (idx == 0 and m.get('no_vis_on_first_frame', False))
        for j in range(iters):
            loss = it.step(j, iters)
            if show and self.vis_mapper.due(idx, j):                         # Mapper.py:705-713
                ct = it.camera_tensors[-1]
                self.vis_mapper.vis(idx, j, gt_depth, gt_color.float(), cur_c2w if ct is None else ct.detach(),
                                    it.grid_opt.render_grids(), self.shared_decoders)
        cams = it.finish()
        if self.cfg.get('coarse', False):
            # the coarse mapper's round on this frame (the reference's third process): stage `coarse`, every voxel of grid_coarse,
            # the same selected frames at their current (fixed) poses
            cfg_c = dict(self.cfg)
            cfg_c['mapping'] = dict(cfg['mapping'], BA=False)
            frames_c = [dict(f, fixed=True) for f in frames]
            itc = MapperIteration(cfg_c, self.renderer, self.shared_c, self.shared_decoders, frames_c, self.cam, masks=None,
                                  keys=('grid_coarse',), static_shapes=self.static_shapes)
            for j in range(iters):
                self.last_coarse_loss = itc.step(j, iters)
            itc.finish()
        if ba:                                                               # Mapper.py:644-660: poses back to the lists
            for f, ct in zip(frames, cams):
                if ct is None:
                    continue
                c2w = torch.eye(4, device=self.device)
                c2w[:3] = get_camera_from_tensor(ct)
                if f['key'] == -1:
                    cur_c2w = c2w
                else:
                    self.keyframe_dict[f['key']]['est_c2w'] = c2w
        return cur_c2w, (float(loss.item()) if loss is not None else None)

    # ---------------------------------------------------------------- the run
    def prefit_decoders(self, indices, iters=300, pixels=None, lr_grid=0.02, lr_dec=2e-3, seed=0):
        """Stand-in for `load_pretrain` (no checkpoint ships with the image): fit ALL decoders and the grids jointly to the
        frames `indices` of the dataset at their ground-truth poses (random pixels -> render -> the mapper's loss -> Adam,
        colour stage, through the HIP path), keep the decoders, re-initialise the grids.  Returns the final loss."""
        from .common import get_samples
        from .losses import rgbd_loss
        dev = self.device
        pixels = pixels or self.cfg['mapping']['pixels']
        items = [self.dataset[i] for i in indices]
        frames = [(it[1].float(), it[2], it[-1][:3].to(dev)) for it in items]
        grids = {k: v.detach().clone().requires_grad_(True) for k, v in self.shared_c.items()}
        dec = self.shared_decoders
        params = [q for q in dec.parameters()]
        for q in params:
            q.requires_grad_(True)
        opt = torch.optim.Adam([{'params': [grids[k] for k in MAP_KEYS], 'lr': lr_grid}, {'params': params, 'lr': lr_dec}])
        gen = torch.cuda.get_rng_state(dev)
        torch.manual_seed(seed)
        n = max(pixels // len(frames), 1)
        loss = None
        for _ in range(iters):
            ro, rd, gd, gc = [], [], [], []
            for color, depth, c2w in frames:
                o, d, dep, col = get_samples(0, self.H, 0, self.W, n, self.H, self.W, self.fx, self.fy, self.cx, self.cy, c2w,
                                             depth, color, dev)
                ro.append(o.float()); rd.append(d.float()); gd.append(dep.float()); gc.append(col.float())
            ro, rd, gd, gc = torch.cat(ro), torch.cat(rd), torch.cat(gd), torch.cat(gc)
            opt.zero_grad(set_to_none=True)
            depth, _u, color = self.renderer.render_batch_ray(grids, dec, rd, ro, dev, 'color', gt_depth=gd)
            loss = rgbd_loss(depth, color, gd, gc, self.cfg['mapping']['w_color_loss'])
            with EF.engine_on_calling_thread():
                loss.backward()
            opt.step()
        for q in params:
            q.grad = None
        torch.cuda.set_rng_state(gen, dev)
        return float(loss.item()) if loss is not None else None

    def run(self, max_frames=None, tracking_iters=None, mesh_file=None):
        """tracking_iters overrides cfg['tracking']['iters'] (0: poses stay at their constant-speed initialisation -- the
        baseline an ATE improvement is measured against).  mesh_file: write the final mesh there (`get_mesh`); no meshing
        otherwise."""
        m, t = self.cfg['mapping'], dict(self.cfg['tracking'])
        if tracking_iters is not None:
            t['iters'] = int(tracking_iters)
        self._track_cfg = t
        n = self.n_img if max_frames is None else min(max_frames, self.n_img)
        plan = frame_plan(n, m['every_frame'], self.rgbd_every, self.schedule)
        dense = self.schedule == 'dense'
        # with 'forecast' / 'none' a frame without RGB-D has no colour and no depth image: they are dropped right here
        strict = not dense and self.depth_mode != 'measured'
        pre_color, integrated = None, None
        self._last_rgbd = None
        for idx in range(n):
            step = plan[idx]
            item = self.dataset[idx]
            if len(item) == 6:
                _, gt_color, gt_depth, gt_event, gt_mask, gt_c2w = item
            else:
                (_, gt_color, gt_depth, gt_c2w), gt_event, gt_mask = item, None, None
            if strict and not step.rgbd:
                gt_color = gt_depth = None
            self.gt_c2w_list[idx] = gt_c2w.clone().cpu()
            t0 = time.perf_counter()
            if idx == 0 or t.get('gt_camera', False):
                c2w = gt_c2w.clone()
                integrated = None                                                                        # Tracker.py:304-311
                if self.vis_tracker is not None and not m.get('no_vis_on_first_frame', False) and gt_color is not None:   # Tracker.py:306-308
                    # (before the first mapping round the tracker holds no copy of the map yet: the shared one)
                    self.vis_tracker.vis(idx, 0, gt_depth, gt_color.float(), c2w.to(self.device), self.tracker.c or self.shared_c,
                                         self.tracker.decoders or self.shared_decoders)
            elif dense:
                c2w = self.track(idx, gt_color.float(), gt_depth, gt_event, gt_mask, pre_color)
            else:
                if gt_event is not None:                                                                 # Tracker.py:350-351
                    integrated = gt_event if integrated is None else integrated + gt_event
                c2w = self.track(idx, None if gt_color is None else gt_color.float(), gt_depth, integrated, gt_mask, pre_color,
                                 rgbd=step.rgbd, forecast=(self.depth_mode == 'forecast' and not step.rgbd), by_event=True)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            self.timing['track'] += t1 - t0
            if step.map and gt_color is not None:             # (the extra round on the last frame needs that frame's images)
                iters = m['iters_first'] if idx == 0 else m['iters']
                c2w, loss = self.map(idx, gt_color, gt_depth, c2w, iters)
                self.update_para_from_mapping()
                if self.verbose:
                    print(f'frame {idx}: mapping loss {loss}')
                if idx % m['keyframe_every'] == 0 or idx == n - 2:           # Mapper.py:687-692
                    self.keyframe_list.append(idx)
                    self.keyframe_dict.append(dict(gt_c2w=gt_c2w.cpu(), idx=idx, color=gt_color.float(), depth=gt_depth,
                                                   est_c2w=c2w.clone()))
            torch.cuda.synchronize()
            self.timing['map'] += time.perf_counter() - t1
            self.estimate_c2w_list[idx] = c2w.detach().cpu()
            if dense:
                pre_color = gt_color.float()
            elif step.reset:                                                 # Tracker.py:461-466
                pre_color, integrated = gt_color.float(), None
            if step.rgbd and ((not dense and self.depth_mode == 'forecast') or (self.motion_prior == 'cmax' and gt_depth is not None)):
                self._last_rgbd = (idx, gt_depth)
        self.last_idx = n - 1
        ckpt = self.logger.log(n - 1, self.keyframe_dict, self.keyframe_list, selected_keyframes=None)
        out = dict(ckpt=ckpt, frames=n, fps=n / max(self.timing['track'] + self.timing['map'], 1e-9), timing=dict(self.timing))
        if self.motion_prior == 'cmax':
            out['motion_prior'] = dict(self.motion_prior_stats)
        if mesh_file is not None:
            out['mesh'] = self.get_mesh(mesh_file)
        return out

    def get_mesh(self, path, idx=None, color=True, clean_mesh=True, get_mask_use_all_frames=False, **meshing):
        """Mesh of the current map through `mesher.Mesher` (the reference's Mapper.py:858-876 call), with this run's keyframes
        and estimated poses; idx defaults to the last processed frame.  cfg['meshing'] (else the reference's defaults,
        mesher.MESHING_DEFAULTS) and cfg['mapping']['marching_cubes_bound'] (else the scene bound) configure it; keyword
        arguments override cfg['meshing'] entries.  Returns what Mesher.get_mesh returns."""
        from .mesher import MESHING_DEFAULTS, Mesher
        cfg = dict(self.cfg)
        cfg['meshing'] = dict(MESHING_DEFAULTS, **self.cfg.get('meshing', {}), **meshing)
        if 'marching_cubes_bound' not in cfg['mapping']:
            cfg['mapping'] = dict(cfg['mapping'], marching_cubes_bound=(self.bound / self.scale).tolist())
        mesher = self.mesher = Mesher(cfg, None, self)
        idx = getattr(self, 'last_idx', 0) if idx is None else idx
        return mesher.get_mesh(path, self.shared_c, self.shared_decoders, self.keyframe_dict, self.estimate_c2w_list, idx,
                               device=self.device, show_forecast=bool(cfg['meshing']['mesh_coarse_level']), color=color,
                               clean_mesh=clean_mesh, get_mask_use_all_frames=get_mask_use_all_frames)

    def evaluate(self, ckpt):
        return evaluate_checkpoint(ckpt, scale=self.scale)
