"""Motion compensation of a time-stamped event stream by contrast maximisation (evennicer_slam_amd/event_cmax.py): per frame
interval the image flow, the camera's angular velocity or, with a depth image, its six velocity components that make the image
of warped events sharpest.

    python tools/event_motion.py --stream EVENTS --size H W --calib FX FY CX CY (--stamps FILE | --fps F)
                                 [--model rotation|flow|rigid] [--depth PATH [--depth-scale S]] [--gap 1] [--sigma 1.5] [--ksize K] [--iters 40] [--signed]
                                 [--max-intervals N] [--out DIR [--images]] [--device cuda:0]
                                 [--reg divergence|deformation [--reg-weight 8] [--t-ref start|middle]]
    python tools/event_motion.py --demo N [--model rigid] [--yaw-deg 8.0] [--step 0.002] [--device cuda:0] [--out DIR [--images]]

EVENTS is a `.npz` of event_stream.EventStream.save or the text layout `t x y p`.  The frame times come from --stamps (first
field per non-comment line) or are i / --fps from the first event's time to the last; every --gap-th frame bounds an interval,
and an event at a frame's own time belongs to the interval that ends there (the bin rule of event_stream.py).  The reference
time of an interval is its middle.  'rotation' is in rad / s in the pinhole frame of the calibration (x right, y down, z
forward); 'flow' in pixels / s; 'rigid' is (angular velocity, linear velocity in depth units / s) in the same frame and needs
--depth PATH: one `.npy` image or one 16-bit PNG divided by --depth-scale (1), at the sensor's size, used for every interval.

--out DIR writes theta.json (per interval: the times, the number of events, theta, the contrast before and after, the number
of evaluations) and with --images the uncompensated and the compensated event image of every interval as PNGs (each scaled by
its own maximum).

--demo N runs the analytic room of synthetic.py under EventSimulator.step_scene(..., stamps=...) for N frames at 30 Hz and
prints the estimated angular velocities beside the ones implied by the ground-truth poses (event_cmax.angular_velocity).  The
camera also translates there, which a pure rotation cannot explain: the comparison is a record, not a bar.  --demo N --model
rigid estimates all six components under the room's own depth frame at the start of each interval and prints them beside
event_cmax.camera_velocity of the ground-truth poses.

--reg maximises the contrast less --reg-weight times f(theta0) times the collapse regulariser of that kind
(event_cmax.estimate_motion's reg / reg_weight: what keeps the six-parameter model from contracting every event onto the
principal point); each row then also has `contrast_only_before` / `contrast_only_after` and `regulariser_after`, and
`contrast_*` are the regularised objective.  --t-ref start puts the reference time at the start of each interval (the middle by
default), where the pose prior of slam.py has it.

--device cpu runs the numpy route of the same model.  Prints one JSON line."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

DEMO_CAM = dict(H=120, W=160, fx=140.0, fy=140.0, cx=79.5, cy=59.5)


def write_png(path, img):
    import numpy as np
    from PIL import Image
    a = np.abs(np.asarray(img.cpu(), dtype=np.float64))
    m = float(a.max()) if a.size else 0.0
    Image.fromarray((255.0 * a / m if m > 0 else a).astype(np.uint8)).save(path)


def intervals_of(stream, edges):
    """the sub-streams a < t <= b of consecutive edges"""
    for a, b in zip(edges[:-1], edges[1:]):
        keep = (stream.t > a) & (stream.t <= b)
        yield float(a), float(b), stream.take(keep.nonzero().reshape(-1))


def read_depth(path, scale, H, W):
    """float32 [H, W] from a `.npy` file or a 16-bit PNG divided by scale"""
    import numpy as np
    if str(path).endswith('.npy'):
        d = np.load(path)
    else:
        from PIL import Image
        with Image.open(path) as im:
            d = np.asarray(im)
    d = np.ascontiguousarray(d, dtype=np.float32) / np.float32(scale)
    if d.shape != (H, W):
        raise SystemExit(f"{path}: the depth image is {d.shape}, the sensor {H} x {W}")
    return d


def estimate(stream, a, b, cal, H, W, args, out_dir=None, index=0, depth=None):
    from evennicer_slam_amd import event_cmax as M
    kw = dict(H=H, W=W, t_ref=a if args.t_ref == 'start' else 0.5 * (a + b), sigma=args.sigma, ksize=args.ksize, signed=args.signed)
    if depth is not None:
        kw['depth'] = depth
    reg = {} if args.reg is None else dict(reg=args.reg, reg_weight=args.reg_weight)
    res = M.estimate_motion(stream, cal, args.model, iters=args.iters, **kw, **reg)
    row = dict(t_a=a, t_b=b, events=len(stream), theta=res['theta'], contrast_before=res['trace'][0], contrast_after=res['trace'][-1],
               evaluations=res['evals'], steps=len(res['trace']) - 1)
    if reg:
        row.update(contrast_only_before=res['f_trace'][0], contrast_only_after=res['f_trace'][-1], regulariser_after=res['reg_trace'][-1],
                   reg_weight_abs=res['reg_weight_abs'])
    if out_dir is not None and args.images:
        zero = [0.0] * len(res['theta'])
        write_png(os.path.join(out_dir, f'interval{index:05d}_raw.png'), M.warp_image(stream, cal, args.model, zero, **kw)[0])
        write_png(os.path.join(out_dir, f'interval{index:05d}_compensated.png'), M.warp_image(stream, cal, args.model, res['theta'], **kw)[0])
    return row


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--stream', default=None)
    ap.add_argument('--size', type=int, nargs=2, metavar=('H', 'W'), default=None)
    ap.add_argument('--calib', type=float, nargs=4, metavar=('FX', 'FY', 'CX', 'CY'), default=None)
    ap.add_argument('--stamps', default=None)
    ap.add_argument('--fps', type=float, default=None)
    ap.add_argument('--gap', type=int, default=1)
    ap.add_argument('--model', choices=('rotation', 'flow', 'rigid'), default='rotation', metavar='{rotation,flow}|rigid')
    ap.add_argument('--depth', default=None)
    ap.add_argument('--depth-scale', type=float, default=1.0)
    ap.add_argument('--sigma', type=float, default=1.5)
    ap.add_argument('--ksize', type=int, default=None)
    ap.add_argument('--iters', type=int, default=40)
    ap.add_argument('--signed', action='store_true')
    ap.add_argument('--max-intervals', type=int, default=None)
    ap.add_argument('--out', default=None)
    ap.add_argument('--images', action='store_true')
    ap.add_argument('--demo', type=int, default=None)
    ap.add_argument('--yaw-deg', type=float, default=8.0)
    ap.add_argument('--step', type=float, default=0.002)
    ap.add_argument('--device', default='cuda:0')
    ap.add_argument('--reg', choices=('divergence', 'deformation'), default=None)
    ap.add_argument('--reg-weight', type=float, default=8.0)
    ap.add_argument('--t-ref', choices=('start', 'middle'), default='middle')
    args = ap.parse_args(argv)
    if (args.demo is None) == (args.stream is None):
        ap.error("give either --stream EVENTS or --demo N")
    if args.images and args.out is None:
        ap.error("--images needs --out DIR")
    if args.demo is None and (args.model == 'rigid') != (args.depth is not None):
        ap.error("--model rigid and --depth PATH come together")
    if args.demo is not None and args.depth is not None:
        ap.error("--demo takes its depth from the room")

    import numpy as np
    from evennicer_slam_amd import event_cmax as M
    from evennicer_slam_amd.event_stream import frame_edges, load_stream, read_stamps

    if args.out is not None:
        os.makedirs(args.out, exist_ok=True)
    out = dict(model=args.model, device=args.device, sigma=args.sigma)
    if args.reg is not None:
        out.update(reg=args.reg, reg_weight=args.reg_weight)
    rows = []
    if args.demo is not None:
        if args.demo < 2:
            ap.error("--demo needs at least 2 frames")
        from evennicer_slam_amd.event_sim import EventSimulator
        from evennicer_slam_amd.scene import scene_bound
        from evennicer_slam_amd.synthetic import BoxRoom, trajectory
        if args.model != 'rigid':
            args.model = out['model'] = 'rotation'
        cam = DEMO_CAM
        H, W = cam['H'], cam['W']
        room = BoxRoom.for_bound(scene_bound([[-1.0, 1.1], [-0.9, 0.8], [-0.7, 0.6]], 1.0, 0.32), margin=0.12, seed=1)
        poses = [p.double() for p in trajectory(room, args.demo, step=args.step, yaw_deg=args.yaw_deg)]
        times = [i / 30.0 for i in range(args.demo)]
        sim = EventSimulator(H, W, device=args.device).reset((room, poses[0], cam))
        cal = M.calib_tuple(cam)
        for i in range(args.demo - 1):
            stream = sim.step_scene(room, poses[i], poses[i + 1], cam, stamps=(times[i], times[i + 1]))[1]
            if args.model == 'rigid':
                depth = room.render(poses[i], cam)[1].float().contiguous().to(stream.device)
                row = estimate(stream, times[i], times[i + 1], cal, H, W, args, args.out, i, depth=depth)
                row['velocity_from_poses'] = M.camera_velocity(poses[i], poses[i + 1], times[i + 1] - times[i])
            else:
                row = estimate(stream, times[i], times[i + 1], cal, H, W, args, args.out, i)
                row['omega_from_poses'] = M.angular_velocity(poses[i], poses[i + 1], times[i + 1] - times[i])
            rows.append(row)
        out.update(demo=args.demo, yaw_deg=args.yaw_deg, step=args.step, sensor=f'{H}x{W}')
    else:
        if args.size is None or args.calib is None:
            ap.error("--stream needs --size H W and --calib FX FY CX CY")
        if (args.stamps is None) == (args.fps is None):
            ap.error("give the frame times with either --stamps FILE or --fps F")
        H, W = args.size
        stream = load_stream(args.stream, device=args.device)
        depth = None
        if args.model == 'rigid':
            import torch
            depth = torch.from_numpy(read_depth(args.depth, args.depth_scale, H, W)).to(stream.device)
        if args.stamps is not None:
            times = read_stamps(args.stamps)
        else:
            import torch
            tf = stream.t[torch.isfinite(stream.t)]
            if tf.numel() == 0:
                raise SystemExit(f"{args.stream}: no event with a finite time")
            t0, t1 = float(tf.min()), float(tf.max())
            n = max(int(np.ceil((t1 - t0) * args.fps)), 1)
            times = np.nextafter(t0, -np.inf) + np.arange(n + 1) / args.fps
        edges = frame_edges(times, gap=args.gap)
        for i, (a, b, part) in enumerate(intervals_of(stream, edges)):
            if args.max_intervals is not None and i >= args.max_intervals:
                break
            rows.append(estimate(part, a, b, tuple(args.calib), H, W, args, args.out, i, depth=depth))
        out.update(stream=args.stream, events=len(stream), sensor=f'{H}x{W}', gap=args.gap)
    out.update(intervals=len(rows), rows=rows)
    if args.out is not None:
        with open(os.path.join(args.out, 'theta.json'), 'w') as f:
            json.dump(rows, f, indent=1)
        out['out'] = args.out
    print(json.dumps(out))
    return out


if __name__ == '__main__':
    main()
