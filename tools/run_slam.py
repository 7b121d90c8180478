"""Run the single-process harness (slam.SLAM) on a sequence described by a YAML configuration in the reference's format.

    python tools/run_slam.py CONFIG [--default-config PATH] [--input_folder DIR] [--event_folder DIR] [--output DIR]
                                    [--max-frames N] [--prepare host|device] [--prefit ITERS] [--device cuda:0]
                                    [--event-net PATH] [--net-backend hip|torch] [--event-predictor net|model] [--vis]
                                    [--schedule dense|reference] [--rgbd-every K]
                                    [--depth-on-event-frames measured|forecast|none] [--motion-prior const_speed|cmax]

CONFIG may name parents with `inherit_from` (config.load_config); --default-config is the root under a chain that names
none (the reference passes configs/nice_slam.yaml).  The reference's YAML files are not part of this repository: point at
your own copy.  --prepare overrides `data.prepare` (frame preparation on the host or in csrc/frame_prep.hip); --prefit fits
the decoders to a handful of ground-truth-posed frames first (SLAM.prefit_decoders, the stand-in for the reference's
pretrained decoders); --event-net loads a state_dict (tools/train_event_net.py, or a reference checkpoint) into a frozen
eval-mode UNet_2heads(6, 2, 2) and hands it to the harness as its event network, --net-backend picks `event.net_backend`
for it (hip: event.compile_event_net); without --event-net the harness runs without one, as before; --event-predictor
model sets `event.predictor`: the event term from the contrast-threshold model (event_model.py; thresholds `event.c_pos`,
`event.c_neg`, `event.eps` of the configuration), which needs no network.  --schedule, --rgbd-every and
--depth-on-event-frames override `event.schedule`, `event.rgbd_every_frame` and `event.depth_on_event_frames` (slam.py: 'dense' --
the default, also for a configuration that sets rgbd_every_frame -- runs RGB-D on every frame; 'reference' is the reference
tracker's sparse schedule).  --motion-prior overrides `tracking.motion_prior`: 'cmax' starts every frame from the camera motion
its events imply (slam.py, THE POSE PRIOR; needs data.event_stream and data.frame_stamps) and adds the prior's counters to the
line.  Prints one JSON line: checkpoint path, frames, frames per second and the ATE."""
import argparse
import copy
import json
import os
import sys
import types

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def slam_camera(cfg):
    """A copy of cfg whose `cam` is the camera of the frames the reader hands out BEFORE the crop_edge cut (which SLAM
    applies itself): with cam.crop_size the image is resized, so the intrinsics scale with it (EvenNICER_SLAM.update_cam)."""
    out = copy.deepcopy(cfg)
    cam = out['cam']
    if cam.get('crop_size') is not None:
        ch, cw = cam['crop_size']
        sy, sx = ch / cam['H'], cw / cam['W']
        cam['fx'], cam['cx'], cam['fy'], cam['cy'] = sx * cam['fx'], sx * cam['cx'], sy * cam['fy'], sy * cam['cy']
        cam['H'], cam['W'] = ch, cw
    return out


def add_schedule_arguments(ap):
    ap.add_argument('--schedule', choices=('dense', 'reference'), default=None)
    ap.add_argument('--rgbd-every', type=int, default=None)
    ap.add_argument('--depth-on-event-frames', choices=('measured', 'forecast', 'none'), default=None)
    ap.add_argument('--motion-prior', choices=('const_speed', 'cmax'), default=None)


def apply_schedule_arguments(cfg, args):
    """--schedule, --rgbd-every and --depth-on-event-frames over cfg['event'], --motion-prior over cfg['tracking']."""
    ev = cfg.setdefault('event', {})
    for key, value in (('schedule', args.schedule), ('rgbd_every_frame', args.rgbd_every),
                       ('depth_on_event_frames', args.depth_on_event_frames)):
        if value is not None:
            ev[key] = value
    if getattr(args, 'motion_prior', None) is not None:
        cfg.setdefault('tracking', {})['motion_prior'] = args.motion_prior
    return cfg


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('config')
    ap.add_argument('--default-config', default=None)
    ap.add_argument('--input_folder', default=None)
    ap.add_argument('--event_folder', default=None)
    ap.add_argument('--output', default=None)
    ap.add_argument('--max-frames', type=int, default=None)
    ap.add_argument('--prepare', choices=('host', 'device'), default=None)
    ap.add_argument('--prefit', type=int, default=0)
    ap.add_argument('--device', default='cuda:0')
    ap.add_argument('--event-net', default=None)
    ap.add_argument('--net-backend', choices=('hip', 'torch'), default=None)
    ap.add_argument('--event-predictor', choices=('net', 'model'), default=None)
    ap.add_argument('--vis', action='store_true')
    add_schedule_arguments(ap)
    args = ap.parse_args(argv)

    import numpy as np
    import torch
    from evennicer_slam_amd import datasets as D
    from evennicer_slam_amd.config import load_config
    from evennicer_slam_amd.slam import SLAM

    cfg = load_config(args.config, args.default_config)
    if args.prepare is not None:
        cfg.setdefault('data', {})['prepare'] = args.prepare
    if args.event_predictor is not None:
        cfg.setdefault('event', {})['predictor'] = args.event_predictor
    apply_schedule_arguments(cfg, args)
    output = args.output or cfg.get('data', {}).get('output') or 'output'
    ds = D.get_dataset(cfg, types.SimpleNamespace(input_folder=args.input_folder, event_folder=args.event_folder), cfg['scale'],
                       device=args.device)
    torch.manual_seed(0)
    np.random.seed(0)
    extra = {}
    if args.event_net is not None:
        from evennicer_slam_amd.event import UNet_2heads
        net = UNet_2heads(6, 2, 2)
        net.load_state_dict(torch.load(args.event_net, map_location='cpu'))
        extra['event_net'] = net.requires_grad_(False).to(args.device).eval()
        if args.net_backend is not None:
            cfg.setdefault('event', {})['net_backend'] = args.net_backend
    slam = SLAM(slam_camera(cfg), ds, output, device=args.device, static_shapes=True, vis=args.vis, **extra)
    n = len(ds) if args.max_frames is None else min(args.max_frames, len(ds))
    if args.prefit > 0:
        slam.prefit_decoders(list(range(0, n, max(n // 6, 1))), iters=args.prefit)
    res = slam.run(max_frames=args.max_frames)
    ate = slam.evaluate(res['ckpt'])
    print(json.dumps(dict(ckpt=res['ckpt'], frames=res['frames'], fps=res['fps'], prepare=ds.prepare,
                          ate_rmse=float(ate['absolute_translational_error.rmse']),
                          compared_pose_pairs=int(ate['compared_pose_pairs']),
                          **({'motion_prior': res['motion_prior']} if 'motion_prior' in res else {}))), flush=True)
    return res


if __name__ == '__main__':
    main()
