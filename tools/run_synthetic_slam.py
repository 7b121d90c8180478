"""The run harness on an analytic, view-consistent sequence (synthetic.BoxRoom): ATE of the full schedule against the ATE of
poses left at their constant-speed initialisation (tracking_iters = 0).  usage: python tools/run_synthetic_slam.py [n_frames]
[--mesh DIR] [--tsdf] [--overlap]: --mesh also meshes the tracked run's map (SLAM.get_mesh) into DIR/mesh.ply and reports accuracy,
completion and completion ratio (eval_recon, metres) against the room's analytic surfaces seen by the keyframes, of the mesh
vertices and, under 'surface_samples', of area-weighted samples of the mesh (eval_recon.sample_surface); with --tsdf the
keyframes' depth fused under the estimated poses (tsdf.TSDFVolume, the reference's voxel size) is written to DIR/tsdf.ply and
evaluated beside the neural mesh, under 'tsdf'; --overlap selects
the mapping window with mapping.keyframe_selection_method 'overlap' (mapper.keyframe_selection_overlap) instead of 'global'.
[--events simulate] writes the sequence with events simulated on the device (event_sim.EventSimulator over the trajectory,
thresholds EVENT_C, default 0.2) instead of all-zero event images and sets event.activate_events; [--event-net PATH] loads a
state_dict (tools/train_event_net.py) into a frozen eval-mode UNet_2heads(6, 2, 2) and hands it to the harness, which the
event term needs; [--net-backend hip|torch] picks event.net_backend for it; [--event-predictor net|model]
sets event.predictor ('model': the event term from the contrast-threshold model of event_model.py, no network needed) and
[--c-pos C] [--c-neg C] its thresholds (default: what the simulator was given); [--vis DIR] keeps the tracked run's per-iteration
figures (frame_vis.Visualizer: DIR/tracking_vis, DIR/mapping_vis; VIS_FREQ and VIS_INSIDE_FREQ, default 5 and 10, set both
stages' vis_freq / vis_inside_freq); with --events simulate, [--refractory S] [--leak-rate HZ] [--shot-rate HZ] [--noise-seed N]
switch the simulator to the noisy sensor (event_sim.EventNoise; the frame times are i / 30 s, those of
tools/simulate_events.py's default --fps); [--schedule dense|reference] [--rgbd-every K] [--depth-on-event-frames
measured|forecast|none] set event.schedule, event.rgbd_every_frame and event.depth_on_event_frames (slam.py; the sparse RGB-D
schedule), [--motion-prior const_speed|cmax] sets tracking.motion_prior ('cmax' needs --events simulate: the sequence is then
simulated with time stamps, 30 frames per second, and the stream and the stamps are written beside it as data.event_stream and
data.frame_stamps; the result carries the prior's counters; CMAX_MIN_EVENTS in the environment sets tracking.cmax_min_events;
[--cmax-reg none|divergence|deformation] [--cmax-reg-weight W] set tracking.cmax_reg and tracking.cmax_reg_weight, the prior's
collapse regulariser) and [--no-events] keeps event.activate_events off with simulated events (the "events off" arm).  SEED (environment, default 0) seeds torch and numpy for each run."""
import os, sys, tempfile, types
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
import evennicer_slam_amd as E
from evennicer_slam_amd import datasets as D
from evennicer_slam_amd.slam import SLAM
from evennicer_slam_amd.synthetic import BoxRoom, trajectory
from evennicer_slam_amd.scene import scene_bound

DEV = 'cuda:0'


from evennicer_slam_amd.synthetic import demo_config, write_demo_sequence


def schedule_overrides(event_cfg, schedule=None, rgbd_every=None, depth_on_event_frames=None):
    """event_cfg with --schedule, --rgbd-every and --depth-on-event-frames applied (None: left as it is)."""
    out = dict(event_cfg)
    if schedule is not None:
        out['schedule'] = schedule
    if rgbd_every is not None:
        out['rgbd_every_frame'] = int(rgbd_every)
    if depth_on_event_frames is not None:
        out['depth_on_event_frames'] = depth_on_event_frames
    return out


def parse_args(args):
    """(n_frames, keyword arguments of run) from the command line."""
    args = list(args)
    mesh_dir = None
    if '--mesh' in args:
        k = args.index('--mesh')
        mesh_dir = args[k + 1]
        del args[k:k + 2]
    flags = {}
    for flag, key in (('--overlap', 'overlap'), ('--tsdf', 'tsdf'), ('--no-events', 'no_events')):
        flags[key] = flag in args
        if flags[key]:
            args.remove(flag)
    opts = {}
    for flag, key in (('--events', 'events'), ('--event-net', 'event_net'), ('--net-backend', 'net_backend'), ('--vis', 'vis'),
                      ('--event-predictor', 'event_predictor'), ('--c-pos', 'c_pos'), ('--c-neg', 'c_neg'),
                      ('--schedule', 'schedule'), ('--rgbd-every', 'rgbd_every'), ('--depth-on-event-frames', 'depth_on_event_frames'),
                      ('--motion-prior', 'motion_prior'), ('--cmax-reg', 'cmax_reg'), ('--cmax-reg-weight', 'cmax_reg_weight')):
        if flag in args:
            k = args.index(flag)
            opts[key] = args[k + 1]
            del args[k:k + 2]
    if opts.get('events') not in (None, 'simulate'):
        raise SystemExit("--events takes 'simulate'")
    if opts.get('event_predictor') not in (None, 'net', 'model'):
        raise SystemExit("--event-predictor takes 'net' or 'model'")
    if opts.get('schedule') not in (None, 'dense', 'reference'):
        raise SystemExit("--schedule takes 'dense' or 'reference'")
    if opts.get('depth_on_event_frames') not in (None, 'measured', 'forecast', 'none'):
        raise SystemExit("--depth-on-event-frames takes 'measured', 'forecast' or 'none'")
    if opts.get('motion_prior') not in (None, 'const_speed', 'cmax'):
        raise SystemExit("--motion-prior takes 'const_speed' or 'cmax'")
    if opts.get('motion_prior') == 'cmax' and opts.get('events') != 'simulate':
        raise SystemExit("--motion-prior cmax needs --events simulate")
    if opts.get('cmax_reg') not in (None, 'none', 'divergence', 'deformation'):
        raise SystemExit("--cmax-reg takes 'none', 'divergence' or 'deformation'")
    if ('cmax_reg' in opts or 'cmax_reg_weight' in opts) and opts.get('motion_prior') != 'cmax':
        raise SystemExit("--cmax-reg and --cmax-reg-weight need --motion-prior cmax")
    if 'cmax_reg_weight' in opts:
        opts['cmax_reg_weight'] = float(opts['cmax_reg_weight'])
    if 'rgbd_every' in opts:
        opts['rgbd_every'] = int(opts['rgbd_every'])
    noise = {}
    for flag, key, kind in (('--refractory', 'refractory', float), ('--leak-rate', 'leak_rate', float), ('--shot-rate', 'shot_rate', float),
                            ('--noise-seed', 'seed', int)):
        if flag in args:
            k = args.index(flag)
            noise[key] = kind(args[k + 1])
            del args[k:k + 2]
    if any(noise.get(k, 0) > 0 for k in ('refractory', 'leak_rate', 'shot_rate')):
        from evennicer_slam_amd.event_sim import EventNoise
        opts['noise'] = EventNoise(**noise)
    return (int(args[0]) if args else 30), dict(mesh_dir=mesh_dir, **flags, **opts)


def tsdf_metrics(slam, path, gt):
    """The same three numbers for the TSDF-fused mesh of the run's keyframes under their estimated poses (written to path)."""
    from evennicer_slam_amd import eval_recon as R
    from evennicer_slam_amd import mesher as MS
    from evennicer_slam_amd.tsdf import TSDFVolume
    cam = dict(H=slam.H, W=slam.W, fx=slam.fx, fy=slam.fy, cx=slam.cx, cy=slam.cy)
    vol = TSDFVolume.for_frames(slam.keyframe_dict, cam, 4.0 * slam.scale / 512.0, 0.04 * slam.scale, color=True, device=slam.device)
    verts, faces, colors = (t.cpu().numpy() for t in vol.extract_mesh())
    verts = verts / slam.scale
    MS.write_ply(path, verts, faces, colors)
    if not len(verts) or not len(gt):
        return dict(accuracy=None, completion=None, completion_ratio=0.0, vertices=0, faces=0)
    return dict(accuracy=R.accuracy(gt, verts), completion=R.completion(gt, verts), completion_ratio=R.completion_ratio(gt, verts),
                vertices=int(len(verts)), faces=int(len(faces)), blocks=vol.stats['blocks'], bytes=vol.stats['bytes'])


def mesh_metrics(slam, path, n_gt=200000, tsdf=False):
    """accuracy / completion / completion ratio (5 cm) of SLAM.get_mesh's mesh against BoxRoom.sample_surface points that
    the keyframes see (the room of synthetic.write_demo_sequence)."""
    from evennicer_slam_amd import eval_recon as R
    room = BoxRoom.for_bound(slam.bound, margin=0.12, seed=1)
    got = slam.get_mesh(path)
    if got is None:
        return dict(accuracy=None, completion=None, completion_ratio=0.0, vertices=0, faces=0)
    verts, faces, _ = got
    gt = room.sample_surface(n_gt).numpy()
    seen, _, _ = slam.mesher.point_masks(gt, slam.keyframe_dict, slam.estimate_c2w_list, slam.last_idx, slam.device)
    gt = gt[seen]
    out = dict(accuracy=R.accuracy(gt, verts), completion=R.completion(gt, verts), completion_ratio=R.completion_ratio(gt, verts),
               vertices=int(len(verts)), faces=int(len(faces)), gt_points_seen=int(len(gt)), timing=dict(slam.mesher.timing))
    # the same three numbers on surface samples of the mesh (what the reference's tool measures), on the device
    dev = torch.device(slam.device)
    if len(faces) and len(gt) and dev.type == 'cuda':
        pts = R.sample_surface(torch.as_tensor(np.asarray(verts, np.float64)), torch.as_tensor(np.asarray(faces)), n_gt, seed=0,
                               device=dev)[0]
        g = torch.from_numpy(gt).to(dev)
        out['surface_samples'] = dict(accuracy=R.accuracy(g, pts), completion=R.completion(g, pts),
                                      completion_ratio=R.completion_ratio(g, pts), samples=int(n_gt))
    if tsdf:
        out['tsdf'] = tsdf_metrics(slam, os.path.join(os.path.dirname(path), 'tsdf.ply'), gt)
    return out


def run(n=30, verbose=True, mesh_dir=None, overlap=False, tsdf=False, events=None, event_net=None, net_backend=None, vis=None,
        noise=None, event_predictor=None, c_pos=None, c_neg=None, schedule=None, rgbd_every=None, depth_on_event_frames=None,
        no_events=False, motion_prior=None, cmax_reg=None, cmax_reg_weight=None):
    cam = dict(H=60, W=80, fx=70.0, fy=70.0, cx=39.5, cy=29.5)
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        sim = None
        if events == 'simulate':
            from evennicer_slam_amd.event_sim import EventSimulator
            c = float(os.environ.get('EVENT_C', 0.2))
            sim = EventSimulator(cam['H'], cam['W'], c_pos=c, c_neg=c, device=DEV, noise=noise)
        elif noise is not None:
            raise SystemExit("the noise options need --events simulate")
        stamps = [i / 30.0 for i in range(n)]
        streams = [] if motion_prior == 'cmax' else None
        (inp, evf), poses = write_demo_sequence(os.path.join(tmp, 'data'), n, cam, step=float(os.environ.get('STEP', 0.012)), yaw_deg=float(os.environ.get('YAW', 0.5)),
                                                events=events, sim=sim, streams=streams,
                                                stamps=None if (noise is None and streams is None) else stamps)
        cfg = demo_config(inp, evf, cam, device=DEV, env=os.environ)
        if motion_prior is not None:
            cfg['tracking'] = dict(cfg['tracking'], motion_prior=motion_prior)
            if 'CMAX_MIN_EVENTS' in os.environ:
                cfg['tracking']['cmax_min_events'] = int(os.environ['CMAX_MIN_EVENTS'])
            if cmax_reg is not None:
                cfg['tracking']['cmax_reg'] = cmax_reg
            if cmax_reg_weight is not None:
                cfg['tracking']['cmax_reg_weight'] = float(cmax_reg_weight)
        if streams is not None:                             # the stream and the frame times the prior reads
            from evennicer_slam_amd.event_stream import EventStream
            EventStream.concatenate(streams).save(os.path.join(tmp, 'events.npz'))
            with open(os.path.join(tmp, 'stamps.txt'), 'w') as f:
                f.write(''.join(f'{v!r}\n' for v in stamps))
            cfg['data'] = dict(cfg['data'], event_stream=os.path.join(tmp, 'events.npz'), frame_stamps=os.path.join(tmp, 'stamps.txt'))
        extra = {}
        if events == 'simulate':
            cfg['event'] = dict(cfg['event'], activate_events=True)
        if event_predictor is not None:
            c_sim = float(os.environ.get('EVENT_C', 0.2))
            cfg['event'] = dict(cfg['event'], predictor=event_predictor, c_pos=c_sim if c_pos is None else float(c_pos),
                                c_neg=c_sim if c_neg is None else float(c_neg))
        if no_events:
            cfg['event'] = dict(cfg['event'], activate_events=False)
        cfg['event'] = schedule_overrides(cfg['event'], schedule, rgbd_every, depth_on_event_frames)
        if event_net is not None:
            from evennicer_slam_amd.event import UNet_2heads
            net = UNet_2heads(6, 2, 2)
            net.load_state_dict(torch.load(event_net, map_location='cpu'))
            extra['event_net'] = net.requires_grad_(False).to(DEV).eval()
            if net_backend is not None:
                cfg['event'] = dict(cfg['event'], net_backend=net_backend)
        if overlap:
            cfg['mapping'] = dict(cfg['mapping'], keyframe_selection_method='overlap')
        if vis is not None:
            freq = dict(vis_freq=int(os.environ.get('VIS_FREQ', 5)), vis_inside_freq=int(os.environ.get('VIS_INSIDE_FREQ', 10)))
            cfg['mapping'], cfg['tracking'] = dict(cfg['mapping'], **freq), dict(cfg['tracking'], **freq)
        ds = D.get_dataset(cfg, types.SimpleNamespace(input_folder=None, event_folder=None), 1, device=DEV)
        for tag, iters in ((('tracked', None),) if os.environ.get('SKIP_BASE') == '1' else (('tracked', None), ('const_speed_init', 0))):
            seed = int(os.environ.get('SEED', 0))
            torch.manual_seed(seed); np.random.seed(seed)
            shown = vis is not None and tag == 'tracked'
            slam = SLAM(cfg, ds, vis if shown else os.path.join(tmp, 'out_' + tag), device=DEV, static_shapes=True,
                        verbose=os.environ.get('VERBOSE') == '1', **(dict(extra, vis=True) if shown else extra))
            fit = slam.prefit_decoders(list(range(0, n, max(n // 6, 1))), iters=int(os.environ.get('PREFIT', 400)))
            res = slam.run(tracking_iters=iters)
            ate = slam.evaluate(res['ckpt'])
            ck = torch.load(res['ckpt'], map_location='cpu', weights_only=False)
            err = (ck['estimate_c2w_list'][:, :3, 3] - ck['gt_c2w_list'][:, :3, 3]).norm(dim=1)
            out[tag] = dict(ate=ate['absolute_translational_error.rmse'], raw_rmse=float((err ** 2).mean().sqrt()), raw_max=float(err.max()),
                            fps=res['fps'], prefit_loss=fit, **({'motion_prior': res['motion_prior']} if 'motion_prior' in res else {}))
            if mesh_dir is not None and tag == 'tracked':
                os.makedirs(mesh_dir, exist_ok=True)
                out[tag]['mesh'] = mesh_metrics(slam, os.path.join(mesh_dir, 'mesh.ply'), tsdf=tsdf)
            if verbose:
                print(tag, out[tag], flush=True)
    return out


if __name__ == '__main__':
    n_frames, kw = parse_args(sys.argv[1:])
    run(n_frames, **kw)
