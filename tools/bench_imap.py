#!/usr/bin/env python3
"""iMAP mode timings on one GPU: the HIP path (csrc/imap_mlp.hip + density compositing) against the torch restatement of
tests/imap_torch.py (hipBLASLt GEMMs) on the same device.  Three steps:
  fwd      the decoder's forward over a 1 M-point lattice (points mode);
  mapper   5000 rays: first pass 32 samples forward only, second pass 44 samples forward + backward, regulation
           5000 x 32 points forward + backward;
  tracker  the tracker's shape: 5000 rays x 44 samples forward + backward (gradient to the rays).
Prints one line per step and path (ms, TFLOP, fraction of the 157.3 TF fp32-MFMA peak) and a JSON summary.  Each
configuration runs in a child process under `timeout` (ENSLAM_BENCH_CHILD set in the child).
    python tools/bench_imap.py [--iters 20] [--warmup 5]"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PEAK = 157.3e12
FLOP_PT = 2 * (93 * 256 + 3 * 256 * 256 + 256 * 4)        # forward, per point


def child(step, path, iters, warmup):
    sys.path.insert(0, ROOT)
    import types
    import torch
    import evennicer_slam_amd as E
    from evennicer_slam_amd import functional as EF
    from tests import imap_torch as T
    dev = 'cuda:0'
    torch.manual_seed(0)
    cfg = {'data': {'dim': 3}, 'model': {'c_dim': 32, 'pos_embedding_method': 'fourier'},
           'rendering': {'lindisp': False, 'perturb': 0.0, 'N_samples': 32, 'N_surface': 0, 'N_importance': 12},
           'scale': 1, 'occupancy': False}
    model = E.get_model(cfg, nice=False).to(dev)
    bound = torch.tensor([[-1.0, 1.1], [-0.9, 0.8], [-0.7, 0.6]], dtype=torch.float64)
    r = E.Renderer(cfg, None, types.SimpleNamespace(nice=False, bound=bound, H=680, W=1200, fx=600., fy=600., cx=599.5,
                                                    cy=339.5))
    params = EF.imap_params(model)
    N = 5000
    g = torch.Generator(device=dev).manual_seed(1)
    ro = (torch.rand(N, 3, device=dev, generator=g) - .5) * 0.2
    rd = torch.randn(N, 3, device=dev, generator=g)
    gd = torch.rand(N, device=dev, generator=g) * 1.5 + 0.3
    z1 = torch.sort(torch.rand(N, 32, device=dev, generator=g, dtype=torch.float64) * 2 + 0.01, -1)[0]
    z2 = torch.sort(torch.rand(N, 44, device=dev, generator=g, dtype=torch.float64) * 2 + 0.01, -1)[0]
    zr = torch.sort(torch.rand(N, 32, device=dev, generator=g) * 1.2, -1)[0]

    def mlp(p):
        return r.eval_points(p, model) if path == 'hip' else T.eval_points(p, params, bound)

    def comp(raw, z, d):
        return (EF.composite_density if path == 'hip' else T.composite_density)(raw, z, d)

    def pts(o, d, z):
        return (o[:, None] + d[:, None] * z[..., None]).reshape(-1, 3)

    if step == 'fwd':
        n = 100
        ax = torch.linspace(-1., 1., n, device=dev, dtype=torch.float64)
        lat = torch.stack(torch.meshgrid(ax, ax, ax, indexing='ij'), -1).reshape(-1, 3)
        flop = FLOP_PT * lat.shape[0]

        def run():
            with torch.no_grad():
                mlp(lat)
    elif step == 'mapper':
        flop = FLOP_PT * N * (32 + 3 * 44 + 3 * 32)

        def run():
            with torch.no_grad():
                comp(mlp(pts(ro, rd, z1)).reshape(N, 32, 4), z1, rd)
            o, d = ro.clone().requires_grad_(True), rd.clone().requires_grad_(True)
            depth, _, color, _ = comp(mlp(pts(o, d, z2)).reshape(N, 44, 4), z2, d)
            sig = mlp(pts(o, d, zr))[:, 3]
            (depth.sum() + color.sum() + 0.0005 * sig.abs().sum()).backward()
    else:
        flop = FLOP_PT * N * 3 * 44

        def run():
            o, d = ro.clone().requires_grad_(True), rd.clone().requires_grad_(True)
            depth, _, color, _ = comp(mlp(pts(o, d, z2)).reshape(N, 44, 4), z2, d)
            (depth.sum() + color.sum()).backward()
    for _ in range(warmup):
        run()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for a, b in ev:
        a.record()
        run()
        b.record()
    torch.cuda.synchronize()
    ts = sorted(a.elapsed_time(b) for a, b in ev)
    ms = ts[len(ts) // 2]
    print(json.dumps({'step': step, 'path': path, 'ms': ms, 'ms_min': ts[0], 'tflop': flop / 1e12,
                      'peak_fraction': flop / (ms * 1e-3) / PEAK}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--timeout', type=int, default=300)
    a = ap.parse_args()
    if os.environ.get('ENSLAM_BENCH_CHILD'):
        child(os.environ['ENSLAM_BENCH_STEP'], os.environ['ENSLAM_BENCH_PATH'], a.iters, a.warmup)
        return
    res = []
    for step in ('fwd', 'mapper', 'tracker'):
        for path in ('hip', 'torch'):
            env = dict(os.environ, ENSLAM_BENCH_CHILD='1', ENSLAM_BENCH_STEP=step, ENSLAM_BENCH_PATH=path)
            p = subprocess.run(['timeout', '-k', '10', str(a.timeout), sys.executable, os.path.abspath(__file__),
                                '--iters', str(a.iters), '--warmup', str(a.warmup)], env=env, capture_output=True, text=True)
            if p.returncode != 0:
                print(f"{step}/{path} failed with status {p.returncode}:\n{p.stderr[-2000:]}")
                sys.exit(1)
            r = json.loads(p.stdout.strip().splitlines()[-1])
            res.append(r)
            print(f"{step:8s} {path:6s} {r['ms']:9.3f} ms  {r['tflop']:.3f} TFLOP  {r['peak_fraction']:.3f} of fp32 MFMA peak")
    print(json.dumps(res))


if __name__ == '__main__':
    main()
