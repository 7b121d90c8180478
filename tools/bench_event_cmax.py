"""Contrast maximisation (csrc/event_cmax.hip, event_cmax.py) on one GPU against the numpy route of the same model on the host.
Records, not bars.  Prints one JSON line.

Shapes, each one evaluation WITH gradient of the rotation model at omega = (0.2, -0.3, 0.5) rad / s, sigma 1.5 (k = 9), the
reference time in the middle of the window:
    sim_260x346    the noisy simulator's stream of one 260 x 346 interval (two seeded grey images, K = 8, stamps (0, 0.04),
                   EventNoise(refractory 1e-3 s, leak 30 Hz, shot 30 Hz, seed 1): the shape of tools/bench_event_filter.py)
    sim_680x1200   the same at 680 x 1200 (about 3.45 M events), in `time` order (time_sorted()) and `pixel_major` (what the
                   simulator emits)
The device route and the numpy route ALTERNATE in one process: `--repeat` (10) timed pairs after one warm-up pair, the median
[min - max] each -- the device call by device events with a synchronise behind it, the host by a wall clock.
`device_below_numpy` says whether the slowest device run is below the fastest numpy run; `equal_to_numpy` whether the two
routes return the same bits (image, counters, mu, f, gradient).
Every shape and order also has a `<shape>_<order>_rigid` row: one evaluation with gradient of the rigid-motion model at
(omega, v) = (OMEGA, (0.1, -0.05, 0.2) units / s) under a seeded depth image in [0.5, 4] with 5 % invalid pixels, timed in the
same alternation, with the same two fields.

The vote atomics: `vote_ms` is the median of an evaluation without gradient minus the median of the same evaluation of an
EMPTY stream on the same sensor (the same memsets, blur and sums; only the vote launch differs), `vote_atomics` the number of
64-bit atomic adds the vote kernel sends (corners inside the image with a non-zero weight, counted by a torch restatement of
the warp), `vote_atomic_gbytes_per_s` = 8 bytes x vote_atomics / vote_ms.

`estimate` times a whole event_cmax.estimate_motion from zero on each shape on the device (--estimate-repeat, 3) and once on
the numpy route for sim_260x346, with the number of evaluations it took.

--reg divergence|deformation adds a `<shape>_<order>_rigid_reg` row per shape (the last order of each): the rigid evaluation
with gradient through enslam_event_cmax_reg_eval with that regulariser against the plain rigid evaluation of the same build,
the two ALTERNATING in one process, --repeat timed pairs after a warm-up pair; `reg_over_plain` is the ratio of the medians,
`plain_below_reg` whether the slowest plain run is below the fastest regularised one, `shared_outputs_equal` whether image,
counters and stats of the two are the same bits.

    python tools/bench_event_cmax.py [--repeat 10] [--estimate-repeat 3] [--no-numpy] [--reg divergence|deformation]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

NOISE = dict(refractory=1e-3, leak_rate=30.0, shot_rate=30.0, seed=1)
OMEGA = [0.2, -0.3, 0.5]
VELOCITY = [0.1, -0.05, 0.2]
STAMPS = (0.0, 0.04)
SIGMA = 1.5


def simulator_stream(H, W, device):
    """one noisy interval: the images of tools/bench_event_noise.py"""
    from evennicer_slam_amd.event_sim import EventNoise, EventSimulator
    rng = np.random.default_rng(1)
    a = rng.integers(0, 256, (H, W))
    step = rng.integers(-60, 61, (H, W))
    step[rng.random((H, W)) < 1.0 / 3.0] = 0
    a, b = a.astype(np.uint8), np.clip(a + step, 0, 255).astype(np.uint8)
    sim = EventSimulator(H, W, device=device, noise=EventNoise(**NOISE)).reset(a)
    return sim.step_images(a, b, stamps=STAMPS)[1]


def depth_image(H, W):
    """float32 [H, W] in [0.5, 4], every twentieth pixel or so invalid (0)"""
    rng = np.random.default_rng(2)
    d = rng.uniform(0.5, 4.0, (H, W)).astype(np.float32)
    d[rng.random((H, W)) < 0.05] = 0.0
    return d


def calib_of(H, W):
    return (0.875 * W, 0.875 * W, (W - 1) / 2.0, (H - 1) / 2.0)


def vote_atomics(stream, H, W, cal, theta, t_ref):
    """corners inside the image with a weight that rounds to a non-zero fixed-point vote"""
    fx, fy, cx, cy = cal
    t, x, y = stream.t, stream.x.view(torch.int16).to(torch.int64) & 0xFFFF, stream.y.view(torch.int16).to(torch.int64) & 0xFFFF
    xd, yd = x.double(), y.double()
    u, v = (xd - cx) / fx, (yd - cy) / fy
    du = (u * v * theta[0] - (1 + u * u) * theta[1]) + v * theta[2]
    dv = ((1 + v * v) * theta[0] - u * v * theta[1]) - u * theta[2]
    dt = t - t_ref
    xw, yw = xd - dt * fx * du, yd - dt * fy * dv
    ok = (x < W) & (y < H) & torch.isfinite(t) & (xw > -1) & (xw < W) & (yw > -1) & (yw < H)
    xw, yw = xw[ok], yw[ok]
    x0, y0 = torch.floor(xw), torch.floor(yw)
    a, b = xw - x0, yw - y0
    n = 0
    for c, w in enumerate(((1 - a) * (1 - b), a * (1 - b), (1 - a) * b, a * b)):
        px, py = x0 + (c & 1), y0 + (c >> 1)
        n += int(((px >= 0) & (px < W) & (py >= 0) & (py < H) & (torch.round(w * 4294967296.0) != 0)).sum())
    return n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeat', type=int, default=10)
    ap.add_argument('--estimate-repeat', type=int, default=3)
    ap.add_argument('--no-numpy', action='store_true')
    ap.add_argument('--reg', choices=('divergence', 'deformation'), default=None)
    args = ap.parse_args()
    from evennicer_slam_amd import event_cmax as M
    from evennicer_slam_amd import functional as EF
    from evennicer_slam_amd.event_stream import EventStream

    if not torch.cuda.is_available():
        raise SystemExit("bench_event_cmax needs a HIP device: it times the kernels")
    dev = 'cuda:0'
    span = lambda xs: [float(np.median(xs)), float(np.min(xs)), float(np.max(xs))]     # noqa: E731
    taps = M.blur_taps(SIGMA)
    t_ref = 0.5 * (STAMPS[0] + STAMPS[1])

    def device_ms(stream, H, W, cal, want_grad=True, depth=None, reg=None):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        model, theta = ('rotation', OMEGA) if depth is None else ('rigid', OMEGA + VELOCITY)
        torch.cuda.synchronize()
        a.record()
        out = EF.event_cmax_eval(*stream.arrays(), H, W, cal, model, theta, t_ref, taps, want_grad=want_grad, depth=depth, reg=reg)
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b), out

    rows, estimates = {}, {}
    for shape, H, W, names in (('sim_260x346', 260, 346, ('pixel_major',)), ('sim_680x1200', 680, 1200, ('time', 'pixel_major'))):
        cal = calib_of(H, W)
        emitted = simulator_stream(H, W, dev)
        streams = dict(pixel_major=emitted, time=emitted.time_sorted())
        empty = EventStream.empty(dev)
        depth_host = depth_image(H, W)
        depth = torch.from_numpy(depth_host).to(dev)
        for order in names:
            stream = streams[order]
            host = stream.numpy()
            total, nograd, idle, host_ms, rigid, rigid_host_ms = [], [], [], [], [], []
            for r in range(args.repeat + 1):                 # the first pair warms up
                ms, out = device_ms(stream, H, W, cal)
                ms_ng = device_ms(stream, H, W, cal, want_grad=False)[0]
                ms_0 = device_ms(empty, H, W, cal, want_grad=False)[0]
                if r:
                    total.append(ms)
                    nograd.append(ms_ng)
                    idle.append(ms_0)
                if not args.no_numpy:
                    t0 = time.perf_counter()
                    ref = M.cmax_numpy(*host, H, W, cal, 'rotation', OMEGA, t_ref, taps)
                    if r:
                        host_ms.append((time.perf_counter() - t0) * 1e3)
                ms_r, out_r = device_ms(stream, H, W, cal, depth=depth)
                if r:
                    rigid.append(ms_r)
                if not args.no_numpy:
                    t0 = time.perf_counter()
                    ref_r = M.cmax_numpy(*host, H, W, cal, 'rigid', OMEGA + VELOCITY, t_ref, taps, depth=depth_host)
                    if r:
                        rigid_host_ms.append((time.perf_counter() - t0) * 1e3)
            n_atomics = vote_atomics(stream, H, W, cal, OMEGA, t_ref)
            vote_ms = float(np.median(nograd) - np.median(idle))
            row = dict(events=len(stream), device_ms_med_min_max=span(total), device_no_grad_ms_med_min_max=span(nograd),
                       device_empty_stream_ms_med_min_max=span(idle), vote_ms=vote_ms, vote_atomics=n_atomics,
                       vote_atomic_gbytes_per_s=(8.0 * n_atomics / (vote_ms * 1e-3) / 1e9) if vote_ms > 0 else None,
                       dropped=dict(zip(M.DROPPED, out[3].cpu().tolist())), f=float(out[2][1]))
            if not args.no_numpy:
                same = (np.array_equal(out[0].cpu().numpy(), ref[0]) and np.array_equal(out[3].cpu().numpy(), ref[3])
                        and np.array_equal(out[2].cpu().numpy().view(np.int64), ref[2].view(np.int64)))
                row.update(numpy_ms_med_min_max=span(host_ms), device_below_numpy='yes' if max(total) < min(host_ms) else 'no',
                           equal_to_numpy=bool(same))
            rows[f'{shape}_{order}'] = row
            row = dict(events=len(stream), device_ms_med_min_max=span(rigid), dropped=dict(zip(M.DROPPED_RIGID, out_r[3].cpu().tolist())),
                       f=float(out_r[2][1]))
            if not args.no_numpy:
                same = (np.array_equal(out_r[0].cpu().numpy(), ref_r[0]) and np.array_equal(out_r[3].cpu().numpy(), ref_r[3])
                        and np.array_equal(out_r[2].cpu().numpy().view(np.int64), ref_r[2].view(np.int64)))
                row.update(numpy_ms_med_min_max=span(rigid_host_ms), device_below_numpy='yes' if max(rigid) < min(rigid_host_ms) else 'no',
                           equal_to_numpy=bool(same))
            rows[f'{shape}_{order}_rigid'] = row
            print(f'{shape}_{order}: done', file=sys.stderr, flush=True)
        stream = streams[names[-1]]
        if args.reg is not None:
            plain, regd = [], []
            for r in range(args.repeat + 1):
                ms_p, out_p = device_ms(stream, H, W, cal, depth=depth)
                ms_g, out_g = device_ms(stream, H, W, cal, depth=depth, reg=args.reg)
                if r:
                    plain.append(ms_p)
                    regd.append(ms_g)
            same = all(torch.equal(a.view(torch.int64), b.view(torch.int64)) for a, b in zip((out_p[0], out_p[2], out_p[3]), (out_g[0], out_g[2], out_g[3])))
            rows[f'{shape}_{names[-1]}_rigid_reg'] = dict(
                events=len(stream), reg=args.reg, plain_ms_med_min_max=span(plain), reg_ms_med_min_max=span(regd),
                reg_over_plain=float(np.median(regd) / np.median(plain)), plain_below_reg='yes' if max(plain) < min(regd) else 'no',
                shared_outputs_equal=bool(same), reg_stats=out_g[4].cpu().tolist())
            print(f'{shape}_{names[-1]}_rigid_reg: done', file=sys.stderr, flush=True)
        # a whole estimate from zero
        kw = dict(H=H, W=W, t_ref=t_ref, sigma=SIGMA)
        ms, res = [], None
        for r in range(args.estimate_repeat + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = M.estimate_motion(stream, cal, 'rotation', **kw)
            torch.cuda.synchronize()
            if r:
                ms.append((time.perf_counter() - t0) * 1e3)
        est = dict(order=names[-1], events=len(stream), device_ms_med_min_max=span(ms), evaluations=res['evals'],
                   steps=len(res['trace']) - 1, theta=res['theta'], contrast_before=res['trace'][0], contrast_after=res['trace'][-1])
        if not args.no_numpy and shape == 'sim_260x346':
            t0 = time.perf_counter()
            ref = M.estimate_motion(stream.to('cpu'), cal, 'rotation', **kw)
            est.update(numpy_ms_once=(time.perf_counter() - t0) * 1e3, same_trace_as_numpy=bool(ref['thetas'] == res['thetas']))
        estimates[shape] = est
        print(f'{shape}_estimate: done', file=sys.stderr, flush=True)
    print(json.dumps(dict(repeat=args.repeat, estimate_repeat=args.estimate_repeat, model='rotation', omega=OMEGA, rigid_velocity=VELOCITY, sigma=SIGMA,
                          ksize=len(taps), stamps=STAMPS, noise=NOISE, rows=rows, estimate=estimates,
                          device=torch.cuda.get_device_name(0))))


if __name__ == '__main__':
    main()
