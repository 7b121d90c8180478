"""The depth forecast (csrc/depth_forecast.hip, functional.depth_forecast) on one GPU against the numpy route of the same model on
the host, at the workload's two sizes: 680 x 1200 -> 102 x 180 (Replica at event.scale_factor 0.15) and 260 x 346 -> 39 x 51 (RPG).

The source image is the analytic room (synthetic.BoxRoom.render) seen from a pose of the demo trajectory, the target the pose five
frames later -- the longest gap of the sparse schedule with event.rgbd_every_frame 5.  The device call (allocation of output
and workspace, one memset, two launches) is timed by device events, the numpy route by a wall clock; the two alternate in one
process, --repeat (10) pairs after one warm-up pair; median [min-max].  Per size and fill setting: whether every device output is
bit-equal to the numpy route's, and the share of target pixels left at 0 without and with the fill, at the harness's radius (1
full-resolution pixel) and at half a target spacing (every point votes).  Prints one JSON line.

    python tools/bench_depth_forecast.py [--repeat 10] [--no-numpy]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

SIZES = (('replica_680x1200_to_102x180', 680, 1200, 102, 180), ('rpg_260x346_to_39x51', 260, 346, 39, 51))
GAP = 5


def scene(H, W):
    """(depth float32 [H,W] on the host, cam, M) of the analytic room: frame 10 of the demo trajectory into frame 10 + GAP"""
    from evennicer_slam_amd import functional as EF
    from evennicer_slam_amd.scene import scene_bound
    from evennicer_slam_amd.synthetic import BoxRoom, trajectory
    cam = dict(H=H, W=W, fx=0.875 * W, fy=0.875 * W, cx=(W - 1) / 2.0, cy=(H - 1) / 2.0)
    room = BoxRoom.for_bound(scene_bound([[-1.0, 1.1], [-0.9, 0.8], [-0.7, 0.6]], 1.0, 0.32), margin=0.12, seed=1)
    poses = trajectory(room, 10 + GAP + 1, step=0.012, yaw_deg=0.5)
    _col, dep = room.render(poses[10].double(), cam)
    return dep.float().contiguous(), cam, EF.relative_camera_matrix(poses[10], poses[10 + GAP])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeat', type=int, default=10)
    ap.add_argument('--no-numpy', action='store_true')
    args = ap.parse_args()
    from evennicer_slam_amd import functional as EF

    if not torch.cuda.is_available():
        raise SystemExit("bench_depth_forecast needs a HIP device: it times the kernel")
    dev = 'cuda:0'
    span = lambda xs: [float(np.median(xs)), float(np.min(xs)), float(np.max(xs))]     # noqa: E731
    rows = {}
    for name, H, W, Ho, Wo in SIZES:
        host, cam, M = scene(H, W)
        depth = host.to(dev)
        half = 0.5 * max((W - 1) / (Wo - 1), (H - 1) / (Ho - 1))
        for radius_name, radius in (('radius_1', 1.0), ('radius_half_spacing', half)):
            for fill in (False, True):
                kw = dict(radius=radius, z_near=0.0, fill=fill)
                dev_ms, host_ms, same, out = [], [], True, None
                for r in range(args.repeat + 1):                # the first pair warms up
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    torch.cuda.synchronize()
                    a.record()
                    out = EF.depth_forecast(depth, cam, M, (Ho, Wo), **kw)
                    b.record()
                    torch.cuda.synchronize()
                    if r:
                        dev_ms.append(a.elapsed_time(b))
                    if not args.no_numpy:
                        t0 = time.perf_counter()
                        ref = EF.depth_forecast(host, cam, M, (Ho, Wo), **kw)
                        if r:
                            host_ms.append((time.perf_counter() - t0) * 1e3)
                        same = same and np.array_equal(out.cpu().numpy().view(np.uint32), ref.numpy().view(np.uint32))
                row = dict(radius=radius, fill=fill, device_ms_med_min_max=span(dev_ms),
                           empty_share=float((out == 0).float().mean()), source_bytes=4 * H * W)
                if not args.no_numpy:
                    row.update(numpy_ms_med_min_max=span(host_ms), device_below_numpy='yes' if max(dev_ms) < min(host_ms) else 'no',
                               equal_to_numpy=bool(same))
                rows[f'{name}_{radius_name}_fill{int(fill)}'] = row
        print(f'{name}: done', file=sys.stderr, flush=True)
    print(json.dumps(dict(repeat=args.repeat, gap_frames=GAP, rows=rows, device=torch.cuda.get_device_name(0))))


if __name__ == '__main__':
    main()
