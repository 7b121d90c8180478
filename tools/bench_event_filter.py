"""The event-stream filter (csrc/event_filter.hip, event_filter.EventFilter) on one GPU against the numpy route of the same model
on the host, and one quality record.  Records, not bars.  Prints one JSON line.

Shapes, each with refractory + support on (rho = 5e-3 s, dt = 2e-3 s), each in three orders -- `time` (time_sorted()),
`pixel_major` (what the simulator emits) and `shuffled` (seeded):
    sim_680x1200   the noisy simulator's stream of one 680 x 1200 interval (two seeded grey images, K = 8, stamps (0, 0.04),
                   EventNoise(refractory 1e-3 s, leak 30 Hz, shot 30 Hz, seed 1): the shape of tools/bench_event_noise.py)
    rand_260x346   --events (10 M) seeded uniform events over one second on 260 x 346
The device route and the numpy route ALTERNATE in one process: `--repeat` (10) timed pairs after one warm-up pair, the median
[min - max] each -- the device call by device events with a synchronise behind it, the host by a wall clock.  The numpy route
gets at most --numpy-events (1 M) events, a seeded subset in the same order, where the shape has more (`numpy_events` says how
many; the device timings are of the whole stream).  The device call is split by device events recorded between its stages into
classify (one launch and the read-back of the flags), order (torch's sorts and cumsum, and the chunk-order check's two
read-backs), walk, support (with the state update) and compact (with torch's prefix sum of the keep flags and the read-back of
the total); host waits inside a stage count for it.  `device_below_numpy` says whether the slowest device run is below the
fastest numpy run; `equal_to_numpy` whether the two routes give the same classes on the numpy route's events.

Quality record (`quality`): the simulator with only shot noise (refractory = leak = 0) emits exactly the noise-free stream plus
the noise events, so on the analytic demo room (260 x 346, --quality-intervals (5) intervals of 0.04 s, K = 8, shot 5 Hz) every
event of the noisy stream that the noise-free stream of the same inputs also holds (same t, x, y, p, bit for bit) is
signal, every other one noise.  Per support_dt: the share of signal kept and of noise removed by the support filter alone.

    python tools/bench_event_filter.py [--repeat 10] [--events 10000000] [--numpy-events 1000000] [--no-numpy]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

RHO, DT = 5e-3, 2e-3
STAGES = ('classify', 'order', 'walk', 'support', 'compact')
QUALITY_DTS = (1e-3, 3e-3, 1e-2)
NOISE = dict(refractory=1e-3, leak_rate=30.0, shot_rate=30.0, seed=1)


def simulator_stream(H, W, device):
    """one noisy 680 x 1200-style interval: the images of tools/bench_event_noise.py"""
    from evennicer_slam_amd.event_sim import EventNoise, EventSimulator
    rng = np.random.default_rng(1)
    a = rng.integers(0, 256, (H, W))
    step = rng.integers(-60, 61, (H, W))
    step[rng.random((H, W)) < 1.0 / 3.0] = 0
    a, b = a.astype(np.uint8), np.clip(a + step, 0, 255).astype(np.uint8)
    sim = EventSimulator(H, W, device=device, noise=EventNoise(**NOISE)).reset(a)
    return sim.step_images(a, b, stamps=(0.0, 0.04))[1]


def random_stream(H, W, n, device):
    from evennicer_slam_amd.event_stream import EventStream
    rng = np.random.default_rng(2)
    return EventStream(rng.uniform(0.0, 1.0, n), rng.integers(0, W, n).astype(np.uint16), rng.integers(0, H, n).astype(np.uint16),
                       rng.integers(0, 2, n).astype(np.uint8)).to(device)


def orders(stream, W):
    """name -> the stream in that order"""
    by_t = stream.time_sorted()
    pix = (by_t.y.view(torch.int16).to(torch.int32) & 0xFFFF) * W + (by_t.x.view(torch.int16).to(torch.int32) & 0xFFFF)
    gen = torch.Generator().manual_seed(3)
    return dict(time=by_t, pixel_major=by_t.take(torch.sort(pix, stable=True).indices),
                shuffled=by_t.take(torch.randperm(len(by_t), generator=gen).to(stream.device)))


def quality(H, W, intervals, device):
    """the share of signal kept / noise removed by the support filter on the analytic room with shot noise only"""
    from evennicer_slam_amd.event_filter import filter_stream
    from evennicer_slam_amd.event_sim import EventNoise, EventSimulator
    from evennicer_slam_amd.event_stream import EventStream
    from evennicer_slam_amd.scene import scene_bound
    from evennicer_slam_amd.synthetic import BoxRoom, trajectory
    room = BoxRoom.for_bound(scene_bound([[-1.0, 1.1], [-0.9, 0.8], [-0.7, 0.6]], 1.0, 0.32), margin=0.12, seed=1)
    poses = [p.double() for p in trajectory(room, intervals + 1, step=0.012, yaw_deg=0.5)]
    cam = dict(H=H, W=W, fx=0.875 * W, fy=0.875 * W, cx=(W - 1) / 2.0, cy=(H - 1) / 2.0)
    shot = 5.0
    streams = {}
    for name, noise in (('clean', None), ('noisy', EventNoise(shot_rate=shot, seed=1))):
        sim = EventSimulator(H, W, device=device, noise=noise).reset((room, poses[0], cam))
        streams[name] = EventStream.concatenate([sim.step_scene(room, poses[i], poses[i + 1], cam, stamps=(0.04 * i, 0.04 * (i + 1)))[1]
                                                 for i in range(intervals)])

    def keys(s):
        t, x, y, p = s.numpy()
        return np.rec.fromarrays([t.view(np.int64), (y.astype(np.int64) * W + x) * 2 + p])

    noisy = streams['noisy']
    signal = np.isin(keys(noisy), keys(streams['clean']))
    out = dict(sensor=f'{H}x{W}', intervals=intervals, shot_rate_hz=shot, events_noise_free=len(streams['clean']), events_noisy=len(noisy),
               signal=int(signal.sum()), noise=int((~signal).sum()), every_noise_free_event_found=bool(int(signal.sum()) == len(streams['clean'])),
               by_support_dt={})
    for dt in QUALITY_DTS:
        classes = filter_stream(noisy, H, W, support_dt=dt, return_classes=True)[2].cpu().numpy()
        kept = classes == 0
        out['by_support_dt'][repr(dt)] = dict(signal_kept=float(kept[signal].mean()) if signal.any() else None,
                                              noise_removed=float((~kept[~signal]).mean()) if (~signal).any() else None)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeat', type=int, default=10)
    ap.add_argument('--events', type=int, default=10_000_000)
    ap.add_argument('--numpy-events', type=int, default=1_000_000)
    ap.add_argument('--quality-intervals', type=int, default=5)
    ap.add_argument('--no-numpy', action='store_true')
    args = ap.parse_args()
    from evennicer_slam_amd.event_filter import EventFilter

    if not torch.cuda.is_available():
        raise SystemExit("bench_event_filter needs a HIP device: it times the kernels")
    dev = 'cuda:0'
    span = lambda xs: [float(np.median(xs)), float(np.min(xs)), float(np.max(xs))]     # noqa: E731

    def device_call(filt, stream):
        marks = [torch.cuda.Event(enable_timing=True)]
        filt.reset()
        torch.cuda.synchronize()
        marks[0].record()

        def mark(_name):
            marks.append(torch.cuda.Event(enable_timing=True))
            marks[-1].record()

        out = filt(stream, return_classes=True, mark=mark)
        torch.cuda.synchronize()
        return marks[0].elapsed_time(marks[-1]), [a.elapsed_time(b) for a, b in zip(marks[:-1], marks[1:])], out

    rows = {}
    shapes = (('sim_680x1200', 680, 1200, lambda: simulator_stream(680, 1200, dev)),
              ('rand_260x346', 260, 346, lambda: random_stream(260, 346, args.events, dev)))
    for shape, H, W, make in shapes:
        for order, stream in orders(make(), W).items():
            n = len(stream)
            host = stream.to('cpu')
            if n > args.numpy_events:
                keep = np.sort(np.random.default_rng(4).choice(n, args.numpy_events, replace=False))
                host = host.take(torch.from_numpy(keep))
            f_dev, f_cpu = EventFilter(H, W, RHO, DT, device=dev), EventFilter(H, W, RHO, DT, device='cpu')
            total, stages, host_ms = [], [], []
            for r in range(args.repeat + 1):                 # the first pair warms up
                ms, parts, out = device_call(f_dev, stream)
                if r:
                    total.append(ms)
                    stages.append(parts)
                if not args.no_numpy:
                    f_cpu.reset()
                    t0 = time.perf_counter()
                    out_cpu = f_cpu(host, return_classes=True)
                    if r:
                        host_ms.append((time.perf_counter() - t0) * 1e3)
            row = dict(events=n, path=f_dev.last_path, stats=out[1], device_ms_med_min_max=span(total))
            for k, name in enumerate(STAGES):
                row[name + '_ms_med_min_max'] = span([s[k] for s in stages])
            if not args.no_numpy:
                row.update(numpy_events=len(host), numpy_ms_med_min_max=span(host_ms),
                           device_below_numpy='yes' if max(total) < min(host_ms) else 'no')
                f_dev.reset()
                same = f_dev(host.to(dev), return_classes=True)
                row['equal_to_numpy'] = bool(torch.equal(same[2].cpu(), out_cpu[2]) and same[1] == out_cpu[1])
            rows[f'{shape}_{order}'] = row
            print(f'{shape}_{order}: done', file=sys.stderr, flush=True)
    print(json.dumps(dict(repeat=args.repeat, refractory=RHO, support_dt=DT, rows=rows,
                          quality=quality(260, 346, args.quality_intervals, dev), device=torch.cuda.get_device_name(0))))


if __name__ == '__main__':
    main()
