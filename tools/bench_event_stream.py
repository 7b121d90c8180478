"""Time-stamped event streams (csrc/event_stream.hip) on one GPU against the numpy routes of the same model on the host:

    emit         one interval of EventSimulator.step_images(..., stamps=...) on two uint8 grey images already on the device
                 (seeded: a random image and one whose pixels moved by up to 60 levels, a third of them not at all), K = 8,
                 default thresholds, at 260 x 346 (a DAVIS346 sensor) and 680 x 1200 (Replica's frame): count launch, prefix
                 sum, the read-back of the total, emit launch
    accumulate   event_stream.accumulate of 10 M seeded events on 260 x 346 into B = 1 and B = 64 bins, in BOTH stream orders:
                 `time` (sorted by t, neighbouring events hit unrelated pixels) and `pixel` (the simulator's pixel-major
                 order: a wave's 64 events hit one or two pixels -- the worst case for same-address atomics)

Per row the device call and the host call ALTERNATE in one process; `--repeat` (10) timed rounds after one warm-up round, the
median [min - max] each: the device by device events with a synchronise behind the call, the host by a wall clock.  The
sensor state is restored before every emit call, outside the timed window.  `bytes` is what the algorithm must move, computed
from the shapes (emit: both images read twice, L_ref read twice and written once, counts and prefix sums, the image and 12
bytes per event written; accumulate: 12 bytes per event read, the uint32 counts cleared, read and the uint8 image written,
plus 4 bytes of atomic traffic per binned event) and `hbm_floor_ms` that over 6.29 TB/s, the measured copy rate of the
part; `floor_share` = floor / median.  Records, not bars.  Prints one JSON line.

    python tools/bench_event_stream.py [--repeat 10] [--events 10000000]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

HBM_BYTES_PER_S = 6.29e12


def images(H, W, seed):
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 256, (H, W))
    step = rng.integers(-60, 61, (H, W))
    step[rng.random((H, W)) < 1.0 / 3.0] = 0
    return a.astype(np.uint8), np.clip(a + step, 0, 255).astype(np.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeat', type=int, default=10)
    ap.add_argument('--events', type=int, default=10_000_000)
    ap.add_argument('--sizes', default='260x346,680x1200')
    args = ap.parse_args()
    from evennicer_slam_amd import event_stream as ES
    from evennicer_slam_amd.event_sim import EventSimulator

    if not torch.cuda.is_available():
        raise SystemExit("bench_event_stream needs a HIP device: it times the kernels")
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

    def row(t_dev, t_host, nbytes, **more):
        floor = nbytes / HBM_BYTES_PER_S * 1e3
        return dict(device_ms_med_min_max=span(t_dev), host_ms_med_min_max=span(t_host),
                    device_below_host='yes' if max(t_dev) < min(t_host) else 'no', bytes=int(nbytes), hbm_floor_ms=floor,
                    floor_share=floor / float(np.median(t_dev)), **more)

    rows = {}
    for size in args.sizes.split(','):
        H, W = (int(v) for v in size.split('x'))
        a, b = images(H, W, 1)
        da, db = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
        sims = {d: EventSimulator(H, W, device=d).reset(a) for d in (dev, 'cpu')}
        start = {d: s.state.clone() for d, s in sims.items()}
        t_dev, t_host, n, same = [], [], 0, None
        for r in range(args.repeat + 1):                     # the first round warms up
            for d, s in sims.items():
                s.state.copy_(start[d])
            td, (ev_d, st_d) = device_ms(lambda: sims[dev].step_images(da, db, stamps=(0.0, 0.04)))
            th, (ev_h, st_h) = host_ms(lambda: sims['cpu'].step_images(a, b, stamps=(0.0, 0.04)))
            if r:
                t_dev.append(td)
                t_host.append(th)
            n = len(st_d)
            same = bool(torch.equal(ev_d.cpu(), ev_h) and all(torch.equal(p.cpu().view(torch.uint8), q.view(torch.uint8))
                                                             for p, q in zip(st_d.arrays(), st_h.arrays())))
        px = H * W
        nbytes = 2 * 2 * px + 2 * 8 * px + 8 * px + 3 * 8 * px + 2 * px + 12 * n
        rows[f'emit_{size}'] = row(t_dev, t_host, nbytes, events=n, stream_equal_to_host=same)

    H, W, N = 260, 346, args.events
    rng = np.random.default_rng(7)
    t = np.sort(rng.uniform(0.0, 1.0, N))
    x, y, p = rng.integers(0, W, N), rng.integers(0, H, N), rng.integers(0, 2, N)
    by_time = ES.EventStream(t, x, y, p)
    order = np.argsort(y.astype(np.int64) * W + x, kind='stable')
    by_pixel = by_time.take(torch.from_numpy(order))
    for B in (1, 64):
        edges = np.linspace(0.0, 1.0, B + 1)
        results = {}
        for name, s in (('time', by_time), ('pixel', by_pixel)):
            sd = s.to(dev)
            t_dev, t_host, out_d = [], [], None
            for r in range(args.repeat + 1):
                td, out_d = device_ms(lambda: ES.accumulate(sd, edges, H, W, with_dropped=True))
                th, out_h = host_ms(lambda: ES.accumulate(s, edges, H, W, with_dropped=True))
                if r:
                    t_dev.append(td)
                    t_host.append(th)
            results[name] = out_d[0]
            binned = N - sum(out_d[1])
            cells = B * H * W * 2
            nbytes = 12 * N + 4 * cells + 4 * cells + cells + 4 * binned
            rows[f'accumulate_B{B}_{name}_order'] = row(t_dev, t_host, nbytes, events=N, binned=binned,
                                                        equal_to_host=bool(torch.equal(out_d[0].cpu(), out_h[0])))
        rows[f'accumulate_B{B}_orders_equal'] = bool(torch.equal(results['time'], results['pixel']))
        rows[f'accumulate_B{B}_pixel_over_time'] = rows[f'accumulate_B{B}_pixel_order']['device_ms_med_min_max'][0] / \
            rows[f'accumulate_B{B}_time_order']['device_ms_med_min_max'][0]
    print(json.dumps(dict(repeat=args.repeat, rows=rows, wave_pre_merge='no', device=torch.cuda.get_device_name(0))))


if __name__ == '__main__':
    main()
