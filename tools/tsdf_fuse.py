"""Fuse the depth images of a sequence into a TSDF volume under given poses and write the mesh (tsdf.TSDFVolume, csrc/tsdf.hip):
the classical baseline to compare a neural map with, and a ground-truth-like mesh for sequences that ship none.

    python tools/tsdf_fuse.py CONFIG out.ply [--default-config PATH] [--input_folder DIR] [--event_folder DIR] [--ckpt FILE]
                                             [--every N] [--max-frames N] [--voxel M] [--trunc M] [--color] [--stride S]
                                             [--device cuda:0]

CONFIG is a YAML configuration in the reference's format (config.load_config; `inherit_from` chains, --default-config as in
tools/run_slam.py); the frames come from datasets.get_dataset.  Poses are the dataset's ground truth, or with --ckpt the
estimated poses of a run's checkpoint (`estimate_c2w_list`).  --voxel / --trunc default to the reference's 4 * scale / 512 and
0.04 * scale (Mesher.py:229-233).  The file is written by mesher.write_ply in the units of the data (vertices / scale), so
tools/eval_recon.py and tools/cull_mesh.py read it.  Prints one JSON line: frames, blocks, bytes, vertices, faces."""
import argparse
import json
import os
import sys
import types

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def frame_camera(cfg):
    """H, W, fx, fy, cx, cy of the frames the reader hands out: cam.crop_size resizes (the intrinsics scale with it), cam.crop_edge
    cuts that many pixels off every side (the principal point moves with the cut)."""
    cam = dict(cfg['cam'])
    H, W, fx, fy, cx, cy = (cam[k] for k in ('H', 'W', 'fx', 'fy', 'cx', 'cy'))
    if cam.get('crop_size') is not None:
        ch, cw = cam['crop_size']
        sy, sx = ch / H, cw / W
        fx, cx, fy, cy, H, W = sx * fx, sx * cx, sy * fy, sy * cy, ch, cw
    e = cam.get('crop_edge', 0)
    return dict(H=H - 2 * e, W=W - 2 * e, fx=fx, fy=fy, cx=cx - e, cy=cy - e)


def fuse(ds, cam, indices, poses=None, voxel=None, trunc=None, scale=1.0, color=False, stride=4, device='cuda:0'):
    """The TSDFVolume of the frames `indices` of dataset `ds` (items: index, colour, depth, ..., pose) under the dataset's own
    poses or `poses` (indexable by frame index)."""
    from evennicer_slam_amd.tsdf import TSDFVolume
    voxel = 4.0 * scale / 512.0 if voxel is None else voxel
    trunc = 0.04 * scale if trunc is None else trunc
    frames = []
    for i in indices:
        item = ds[i]
        frames.append(dict(depth=item[2], color=item[1], c2w=item[-1] if poses is None else poses[i]))
    return TSDFVolume.for_frames(frames, cam, voxel, trunc, color=color, depth_sampling_stride=stride, device=device)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('config')
    ap.add_argument('out')
    ap.add_argument('--default-config', default=None)
    ap.add_argument('--input_folder', default=None)
    ap.add_argument('--event_folder', default=None)
    ap.add_argument('--ckpt', default=None)
    ap.add_argument('--every', type=int, default=1)
    ap.add_argument('--max-frames', type=int, default=None)
    ap.add_argument('--voxel', type=float, default=None)
    ap.add_argument('--trunc', type=float, default=None)
    ap.add_argument('--color', action='store_true')
    ap.add_argument('--stride', type=int, default=4)
    ap.add_argument('--device', default='cuda:0')
    args = ap.parse_args(argv)

    import torch
    from evennicer_slam_amd import datasets as D
    from evennicer_slam_amd import mesher as MS
    from evennicer_slam_amd.config import load_config

    cfg = load_config(args.config, args.default_config)
    scale = cfg['scale']
    ds = D.get_dataset(cfg, types.SimpleNamespace(input_folder=args.input_folder, event_folder=args.event_folder), scale,
                       device=args.device)
    n = len(ds) if args.max_frames is None else min(args.max_frames, len(ds))
    poses = None
    if args.ckpt is not None:
        ck = torch.load(args.ckpt, map_location='cpu', weights_only=False)
        poses = ck['estimate_c2w_list']
        n = min(n, int(ck['idx']) + 1)
    vol = fuse(ds, frame_camera(cfg), range(0, n, max(args.every, 1)), poses, args.voxel, args.trunc, scale, args.color, args.stride,
               args.device)
    verts, faces, colors = vol.extract_mesh()
    MS.write_ply(args.out, verts.cpu().numpy() / scale, faces.cpu().numpy(), colors.cpu().numpy() if colors is not None else None)
    st = vol.stats
    out = dict(out=args.out, frames=len(st['frames']), blocks=st['blocks'], bytes=st['bytes'], vertices=int(verts.shape[0]),
               faces=int(faces.shape[0]), touched_outside=sum(f['touched_outside'] for f in st['frames']))
    print(json.dumps(out), flush=True)
    return out


if __name__ == '__main__':
    main()
