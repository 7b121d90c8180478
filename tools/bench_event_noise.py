"""The noisy event sensor (csrc/event_noise.hip) on one GPU against the noise-free stream call of the same build and against the
numpy route of the same model on the host.

One interval, K = 8, default thresholds (0.2), stamps (0, 0.04), at 260 x 346 (a DAVIS346 sensor) and 680 x 1200 (Replica's
frame), on both routes:
    images    two seeded uint8 grey images already on the device (a random image and one whose pixels moved by up to 60 levels,
              a third of them not at all)
    analytic  the demo room of synthetic.write_demo_sequence between two poses of synthetic.trajectory, rendered in the kernel
Per route and size, these calls ALTERNATE in one process, `--repeat` (10) timed rounds after one warm-up round, the median
[min - max] each -- device calls by device events with a synchronise behind the call, the host by a wall clock:
    plain_stream   EventSimulator.step_*(stamps=...) without noise: count launch, prefix sum, read-back, emit launch
    noisy_stream   the same call with EventNoise(all three effects): two launches of the noisy kernels
    noisy_image    the noisy call with stream=False: one launch, no prefix sum, no read-back
    numpy          the noisy call on a CPU simulator
and the sweep: noisy_stream with each effect alone (refractory 1e-3 s, leak 30 Hz, shot 30 Hz; `all` is the three together,
seed 1).  The order of the calls within a round is a seeded permutation, drawn anew for every round, so that no call always
runs right after the host route: the device is idle for its 0.1 to 1 s, and the first device call after it takes several
times as long (it shows in the maxima).  Both states are restored before every call, outside the timed window.  `noisy_over_plain` is the ratio of the two
medians; `device_below_numpy` says whether the slowest device run of noisy_stream is below the fastest numpy run;
`equal_to_numpy` whether image, states and stream of the device equal the host's bit for bit (grey images through the host
table: expected; the analytic route runs the device's own sin / log: recorded, not expected).  Records, not bars.  Prints one
JSON line.

    python tools/bench_event_noise.py [--repeat 10] [--sizes 260x346,680x1200] [--no-numpy]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

STAMPS = (0.0, 0.04)
EFFECTS = dict(refractory=dict(refractory=1e-3), leak=dict(leak_rate=30.0), shot=dict(shot_rate=30.0))


def images(H, W, seed):
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 256, (H, W))
    step = rng.integers(-60, 61, (H, W))
    step[rng.random((H, W)) < 1.0 / 3.0] = 0
    return a.astype(np.uint8), np.clip(a + step, 0, 255).astype(np.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeat', type=int, default=10)
    ap.add_argument('--sizes', default='260x346,680x1200')
    ap.add_argument('--no-numpy', action='store_true')
    args = ap.parse_args()
    from evennicer_slam_amd.event_sim import EventNoise, EventSimulator
    from evennicer_slam_amd.scene import scene_bound
    from evennicer_slam_amd.synthetic import BoxRoom, trajectory

    if not torch.cuda.is_available():
        raise SystemExit("bench_event_noise needs a HIP device: it times the kernels")
    dev = 'cuda:0'

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
    room = BoxRoom.for_bound(scene_bound([[-1.0, 1.1], [-0.9, 0.8], [-0.7, 0.6]], 1.0, 0.32), margin=0.12, seed=1)
    pose_a, pose_b = (p.double() for p in trajectory(room, 2, step=0.012, yaw_deg=0.5))
    both = dict(EFFECTS['refractory'], **EFFECTS['leak'], **EFFECTS['shot'], seed=1)

    rows = {}
    for size in args.sizes.split(','):
        H, W = (int(v) for v in size.split('x'))
        cam = dict(H=H, W=W, fx=0.875 * W, fy=0.875 * W, cx=(W - 1) / 2.0, cy=(H - 1) / 2.0)
        a, b = images(H, W, 1)
        da, db = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
        for route in ('images', 'analytic'):
            first = a if route == 'images' else (room, pose_a, cam)

            def step(sim, on_dev, **kw):
                if route == 'images':
                    return sim.step_images(da if on_dev else a, db if on_dev else b, stamps=STAMPS, **kw)
                return sim.step_scene(room, pose_a, pose_b, cam, stamps=STAMPS, **kw)

            calls = {'plain_stream': (EventSimulator(H, W, device=dev), {}),
                     'noisy_stream': (EventSimulator(H, W, device=dev, noise=EventNoise(**both)), {}),
                     'noisy_image': (EventSimulator(H, W, device=dev, noise=EventNoise(**both)), dict(stream=False))}
            for name, kw in EFFECTS.items():
                calls['noisy_stream_' + name + '_only'] = (EventSimulator(H, W, device=dev, noise=EventNoise(seed=1, **kw)), {})
            if not args.no_numpy:
                calls['numpy'] = (EventSimulator(H, W, device='cpu', noise=EventNoise(**both)), {})
            for sim, _ in calls.values():
                sim.reset(first)
            start = {k: sim.state.clone() for k, (sim, _) in calls.items()}
            times, outs = {k: [] for k in calls}, {}
            order = np.random.default_rng(5)
            for r in range(args.repeat + 1):                 # the first round warms up
                for k in order.permutation(list(calls)).tolist():
                    sim, kw = calls[k]
                    if sim.noise is not None:
                        sim.reset(first)                     # t_last := -inf, interval := 0
                    sim.state.copy_(start[k])
                    ms, out = (host_ms if k == 'numpy' else device_ms)(lambda: step(sim, k != 'numpy', **kw))
                    outs[k] = out
                    if r:
                        times[k].append(ms)
            row = {k + '_ms_med_min_max': span(v) for k, v in times.items()}
            row['events_plain'], row['events_noisy'] = len(outs['plain_stream'][1]), len(outs['noisy_stream'][1])
            row['noisy_over_plain'] = row['noisy_stream_ms_med_min_max'][0] / row['plain_stream_ms_med_min_max'][0]
            row['noisy_image_over_plain'] = row['noisy_image_ms_med_min_max'][0] / row['plain_stream_ms_med_min_max'][0]
            row['image_equals_stream_call'] = bool(torch.equal(outs['noisy_image'], outs['noisy_stream'][0]))
            if not args.no_numpy:
                row['device_below_numpy'] = 'yes' if max(times['noisy_stream']) < min(times['numpy']) else 'no'
                (ev_d, st_d), (ev_h, st_h) = outs['noisy_stream'], outs['numpy']
                row['equal_to_numpy'] = bool(
                    torch.equal(ev_d.cpu(), ev_h) and len(st_d) == len(st_h)
                    and all(torch.equal(p.cpu().view(torch.uint8), q.view(torch.uint8)) for p, q in zip(st_d.arrays(), st_h.arrays()))
                    and torch.equal(calls['noisy_stream'][0].last_event_time.cpu(), calls['numpy'][0].last_event_time))
            rows[f'{route}_{size}'] = row
    print(json.dumps(dict(repeat=args.repeat, substeps=8, stamps=STAMPS, noise=both, rows=rows, device=torch.cuda.get_device_name(0))))


if __name__ == '__main__':
    main()
