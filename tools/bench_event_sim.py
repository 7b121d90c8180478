"""One interval of the event-camera simulator (event_sim.EventSimulator, csrc/event_sim.hip) on one GPU against the numpy
route of the same model on the host, at 680 x 1200 (Replica's frame) and 260 x 346 (a DAVIS346 sensor), K = 8 sub-steps,
default thresholds:

    images_grey   two uint8 grey images already on the device (seeded: a random image and one whose pixels moved by up to 60
                  levels, a third of them not at all)
    images_rgb    the same in RGB, luminance and log in the kernel
    scene         the analytic demo room between two neighbouring poses of the demo trajectory, rendered in the kernel at the 8
                  interpolated poses (pose interpolation on the host is part of the call)
    scene_frame   the same call also returning the colour and depth frame of the last pose

Per row the device call and the host call ALTERNATE in one process; `--repeat` (10) timed rounds after one warm-up round, the
median [min - max] each: the device by device events with a synchronise behind the call, the host by a wall clock.  The sensor
state is restored before every call, outside the timed window, so every call does the same work.  `device_below_host` states the
comparison: slowest device run below fastest host run, yes or no.  Prints one JSON line.

    python tools/bench_event_sim.py [--repeat 10] [--sizes 680x1200,260x346]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def images(H, W, channels, seed):
    rng = np.random.default_rng(seed)
    shape = (H, W) if channels == 1 else (H, W, 3)
    a = rng.integers(0, 256, shape)
    step = rng.integers(-60, 61, shape)
    step[rng.random((H, W)) < 1.0 / 3.0] = 0
    return a.astype(np.uint8), np.clip(a + step, 0, 255).astype(np.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeat', type=int, default=10)
    ap.add_argument('--sizes', default='680x1200,260x346')
    args = ap.parse_args()
    from evennicer_slam_amd.event_sim import EventSimulator
    from evennicer_slam_amd.scene import scene_bound
    from evennicer_slam_amd.synthetic import BoxRoom, trajectory

    if not torch.cuda.is_available():
        raise SystemExit("bench_event_sim needs a HIP device: it times the kernels")
    dev = 'cuda:0'
    room = BoxRoom.for_bound(scene_bound([[-1.0, 1.1], [-0.9, 0.8], [-0.7, 0.6]], 1.0, 0.32), margin=0.12, seed=1)
    pa, pb = (p.double() for p in trajectory(room, 5, step=0.012, yaw_deg=0.5)[3:5])

    def device_ms(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), out

    def host_ms(fn):
        t0 = time.perf_counter()
        out = fn()
        return (time.perf_counter() - t0) * 1e3, out

    span = lambda xs: [float(np.median(xs)), float(np.min(xs)), float(np.max(xs))]     # noqa: E731
    rows = {}
    for size in args.sizes.split(','):
        H, W = (int(v) for v in size.split('x'))
        cam = dict(H=H, W=W, fx=0.875 * W, fy=0.875 * W, cx=(W - 1) / 2, cy=(H - 1) / 2)
        sims = {d: EventSimulator(H, W, device=d) for d in (dev, 'cpu')}
        work = {}
        for name, channels in (('images_grey', 1), ('images_rgb', 3)):
            a, b = images(H, W, channels, 1)
            da, db = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
            work[name] = (a, (lambda s, da=da, db=db: s.step_images(da, db)), (lambda s, a=a, b=b: s.step_images(a, b)))
        for name, frame in (('scene', False), ('scene_frame', True)):
            call = (lambda s, frame=frame: s.step_scene(room, pa, pb, cam, want_frame=frame))
            work[name] = ((room, pa, cam), call, call)
        for name, (first, on_device, on_host) in work.items():
            t_dev, t_host, share, same = [], [], None, None
            for s in sims.values():
                s.reset(first)
            start = {d: s.state.clone() for d, s in sims.items()}
            for r in range(args.repeat + 1):                 # the first round warms up
                for d, s in sims.items():
                    s.state.copy_(start[d])
                td, out_d = device_ms(lambda: on_device(sims[dev]))
                th, out_h = host_ms(lambda: on_host(sims['cpu']))
                if r:
                    t_dev.append(td)
                    t_host.append(th)
                ev_d, ev_h = (o[0] if isinstance(o, tuple) else o for o in (out_d, out_h))
                share = float((ev_h != 0).any(dim=-1).double().mean())
                same = float((ev_d.cpu() == ev_h).all(dim=-1).double().mean())
            rows[f'{size}_{name}'] = dict(device_ms_med_min_max=span(t_dev), host_ms_med_min_max=span(t_host),
                                          device_below_host='yes' if max(t_dev) < min(t_host) else 'no',
                                          event_pixel_share=share, pixels_equal_to_host=same)
    print(json.dumps(dict(substeps=8, repeat=args.repeat, rows=rows, device=torch.cuda.get_device_name(0))))


if __name__ == '__main__':
    main()
