"""Rendering quality of a finished SLAM run: every N-th frame of the sequence re-rendered from the newest checkpoint's map at
the frame's ESTIMATED pose (Renderer.render_img, stage 'color', depth-guided) and compared with the frame itself.

    python tools/eval_rendering.py CONFIG [--output DIR] [--every N] [--save DIR] [--default-config YAML]
                                          [--input_folder DIR] [--event_folder DIR] [--max-frames N] [--device cuda:0]

The checkpoint is found the way tools/visualizer.py finds it (the newest under OUTPUT/ckpts; OUTPUT is data.output of the
configuration unless --output names it).  Prints one JSON line: per frame and as means depth L1 (in the units of the
sequence's depth after `scale`, over the pixels with a measurement), PSNR (dB, colours clipped to [0, 1]) and SSIM
(frame_vis.render_metrics: csrc/frame_report.hip on the device).  --save writes the sheet of input / generated / residual
panels of every evaluated frame to DIR/{idx:05d}_0000.jpg (frame_vis.Visualizer)."""
import argparse
import importlib.util
import json
import math
import os
import sys
import types

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _run_slam():
    spec = importlib.util.spec_from_file_location('run_slam', os.path.join(os.path.dirname(os.path.abspath(__file__)), 'run_slam.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('config')
    ap.add_argument('--default-config', default=None)
    ap.add_argument('--input_folder', default=None)
    ap.add_argument('--event_folder', default=None)
    ap.add_argument('--output', default=None)
    ap.add_argument('--every', type=int, default=5)
    ap.add_argument('--save', default=None)
    ap.add_argument('--max-frames', type=int, default=None)
    ap.add_argument('--device', default='cuda:0')
    args = ap.parse_args(argv)
    if args.every < 1:
        raise SystemExit('--every must be at least 1')

    import torch
    from evennicer_slam_amd import datasets as D
    from evennicer_slam_amd.config import load_config
    from evennicer_slam_amd.eval_ate import latest_checkpoint
    from evennicer_slam_amd.frame_vis import Visualizer, render_metrics
    from evennicer_slam_amd.slam import SLAM

    cfg = load_config(args.config, args.default_config)
    output = args.output or cfg.get('data', {}).get('output') or 'output'
    ckpt_path = latest_checkpoint(f'{output}/ckpts')
    if ckpt_path is None:
        raise SystemExit(f'no checkpoint under {output}/ckpts')
    ckpt = torch.load(ckpt_path, map_location=torch.device('cpu'), weights_only=False)
    ds = D.get_dataset(cfg, types.SimpleNamespace(input_folder=args.input_folder, event_folder=args.event_folder), cfg['scale'],
                       device=args.device)
    slam = SLAM(_run_slam().slam_camera(cfg), ds, output, device=args.device)
    slam.shared_decoders.load_state_dict(ckpt['decoder_state_dict'])
    grids = {k: v.detach().to(args.device) for k, v in ckpt['c'].items()}
    est = ckpt['estimate_c2w_list']
    n = min(int(ckpt['idx']) + 1, len(ds)) if args.max_frames is None else min(args.max_frames, int(ckpt['idx']) + 1, len(ds))
    vis = None
    if args.save is not None:
        vis = Visualizer(1, 1, args.save, slam.renderer, verbose=False, device=args.device, stage='eval')
    frames = []
    for idx in range(0, n, args.every):
        item = ds[idx]
        gt_color, gt_depth = item[1].float().to(args.device), item[2].to(args.device)
        c2w = est[idx].to(args.device).float()
        depth, _unc, color = slam.renderer.render_img(grids, slam.shared_decoders, c2w, args.device, stage='color', gt_depth=gt_depth)
        m = render_metrics(depth, color, gt_depth, gt_color)
        frames.append(dict(idx=idx, **m))
        if vis is not None:
            vis.vis(idx, 0, gt_depth, gt_color, c2w, grids, slam.shared_decoders)

    def mean(key):
        vals = [f[key] for f in frames if f[key] is not None and math.isfinite(f[key])]
        return sum(vals) / len(vals) if vals else None

    out = dict(ckpt=ckpt_path, frames=frames, n_frames=len(frames), every=args.every, depth_l1=mean('depth_l1'), psnr=mean('psnr'),
               ssim=mean('ssim'), saved=args.save)
    print(json.dumps(out), flush=True)
    return out


if __name__ == '__main__':
    main()
