"""Visibility timings on one GPU at the sizes a user runs: the 256^3 lattice of the room0 marching-cubes bound against K = 32
and K = 240 keyframes of the room0 camera (680 x 1200).  The HIP kernel (csrc/visibility.hip, through Mesher.point_masks and
alone) against the torch loop over cameras that point_masks ran before it (Mesher.point_masks_torch) on the same device-resident
points with depth_test False, the two ALTERNATING in one process; then the kernel with depth_test True and in lattice mode,
and the float64 overlap count.  Device events, median and spread of --repeat runs after a warm-up.  Prints one JSON line.

    python tools/bench_visibility.py [--resolution 256] [--repeat 10] [--cams 32 240]

Bounds reported beside the kernel: bytes = 13 B per point (12 read, 1 written; lattice mode 1 B) at 8 TB/s; flops = 45 per
point and camera VISITED at full K (no early exit) at the 157 TFLOP/s fp32 vector peak.  The early exit makes the real visit
count smaller, so the kernel can run below the full-K flop bound."""
import argparse
import json
import os
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

PEAK_BYTES, PEAK_FLOPS, FLOPS_PER_VISIT = 8.0e12, 157.3e12, 45


def look_at(pos, target):
    f = (target - pos) / np.linalg.norm(target - pos)
    right = np.cross(f, [0.0, 0.0, 1.0])
    right /= np.linalg.norm(right)
    m = np.eye(4, dtype=np.float32)
    m[:3, 0], m[:3, 1], m[:3, 2], m[:3, 3] = right, np.cross(right, f), -f, pos
    return m


def keyframes(K, bound, cam, dev, seed=0):
    """K seeded views from inside the room towards seeded points of it, each with a seeded smooth depth image (1.5-4.5 m, 2 %
    zero pixels)"""
    rng = np.random.default_rng(seed)
    lo, hi = np.array(bound)[:, 0], np.array(bound)[:, 1]
    H, W = cam['H'], cam['W']
    jj, ii = np.meshgrid(np.arange(H, dtype=np.float32), np.arange(W, dtype=np.float32), indexing='ij')
    out = []
    for _ in range(K):
        pos = lo + (hi - lo) * rng.uniform(0.25, 0.75, 3)
        target = lo + (hi - lo) * rng.uniform(0.0, 1.0, 3)
        d = 3.0 + 1.5 * np.sin(0.004 * ii + rng.uniform(0, 6.28)) * np.cos(0.006 * jj + rng.uniform(0, 6.28))
        d[rng.random((H, W)) < 0.02] = 0.0
        out.append(dict(est_c2w=torch.from_numpy(look_at(pos, target)).to(dev), depth=torch.from_numpy(d.astype(np.float32)).to(dev)))
    return out


def timed(fn, repeat, warmup=2):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(repeat):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return ms


def stats(ms):
    ms = sorted(ms)
    return dict(median_ms=round(float(np.median(ms)), 4), min_ms=round(ms[0], 4), max_ms=round(ms[-1], 4), n=len(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--resolution', type=int, default=256)
    ap.add_argument('--repeat', type=int, default=10)
    ap.add_argument('--cams', type=int, nargs='+', default=[32, 240])
    args = ap.parse_args()
    import bench
    from evennicer_slam_amd import functional as EF
    from evennicer_slam_amd import mapper
    from evennicer_slam_amd.mesher import MESHING_DEFAULTS, Mesher
    from tests import visibility_numpy as V

    dev = 'cuda:0'
    cam = dict(bench.CAM)
    bound = bench.SCENES['room0']
    slam = types.SimpleNamespace(renderer=None, bound=torch.tensor(bound), nice=True, verbose=False, **cam)

    def mesher(depth_test):
        cfg = dict(coarse=True, scale=1.0, occupancy=True, meshing=dict(MESHING_DEFAULTS, resolution=args.resolution, depth_test=depth_test),
                   mapping=dict(marching_cubes_bound=bound))
        return Mesher(cfg, None, slam)

    m0, m1 = mesher(False), mesher(True)
    xyz = m0.get_grid_uniform(args.resolution)['xyz']
    axes = [torch.from_numpy(a.astype(np.float32)).to(dev) for a in xyz]
    pts = torch.stack([g.reshape(-1) for g in torch.meshgrid(*axes, indexing='ij')], 1).contiguous()
    P = pts.shape[0]
    out = dict(points=P, camera=[cam['H'], cam['W']], chunk=m0.points_batch_size, repeat=args.repeat, cases={})
    for K in args.cams:
        kfs = keyframes(K, bound, cam, dev)
        views0, views1 = m0._views(kfs, None, 0, dev, False), m1._views(kfs, None, 0, dev, False)
        hip = lambda: m0.point_masks(pts, kfs, None, 0, dev)                       # noqa: E731
        old = lambda: m0.point_masks_torch(pts, kfs, None, 0, dev)                 # noqa: E731
        a, b = hip(), old()
        same = all(np.array_equal(x, y) for x, y in zip(a, b))
        shares = [float(x.mean()) for x in a]
        t_hip, t_old = [], []
        for _ in range(args.repeat):                                              # alternate the two
            t_hip += timed(hip, 1, warmup=0)
            t_old += timed(old, 1, warmup=0)
        # points on which the two float32 evaluations disagree, and how many of them the float64 yardstick does NOT place within
        # 1e-5 of a threshold (tests/visibility_numpy.py: the exclusion rule of tests/test_hip_visibility.py)
        differ = np.nonzero((a[0] != b[0]) | (a[1] != b[1]))[0]
        _, _, near, _ = V.classify(pts[torch.from_numpy(differ).to(dev)].cpu().numpy(), views0[0], cam, limit=views0[1].cpu().numpy())
        case = dict(point_masks_hip=stats(t_hip), point_masks_torch=stats(t_old), masks_equal=bool(same),
                    differing_points=int(len(differ)), differing_points_not_on_a_threshold=int((~near).sum()),
                    shares_seen_forecast_unseen=shares)
        case['speedup_median'] = round(case['point_masks_torch']['median_ms'] / case['point_masks_hip']['median_ms'], 1)
        case['speedup_worst_over_best'] = round(case['point_masks_torch']['min_ms'] / case['point_masks_hip']['max_ms'], 1)
        # the kernel alone (classes stay on the device), explicit points / lattice / depth test
        case['kernel_points'] = stats(timed(lambda: m0.point_classes(views0, dev, points=pts), args.repeat))
        case['kernel_lattice'] = stats(timed(lambda: m0.point_classes(views0, dev, lattice=axes), args.repeat))
        case['kernel_lattice_depth_test'] = stats(timed(lambda: m1.point_classes(views1, dev, lattice=axes), args.repeat))
        w2c = views0[0]
        one = lambda: EF.visibility(None, w2c, cam, limit=views0[1], lattice=axes)  # noqa: E731
        case['kernel_lattice_one_launch'] = stats(timed(one, args.repeat))
        cnt = lambda: EF.visibility(None, w2c, cam, limit=views0[1], lattice=axes, want_counts=True)  # noqa: E731
        case['kernel_lattice_one_launch_all_cameras'] = stats(timed(cnt, args.repeat))
        case['bound_bytes_ms'] = round(13.0 * P / PEAK_BYTES * 1e3, 4)
        case['bound_flops_full_K_ms'] = round(FLOPS_PER_VISIT * P * K / PEAK_FLOPS * 1e3, 4)
        sel = pts[torch.randint(0, P, (1600,), device=dev)]
        case['overlap_counts_1600_points_f64'] = stats(timed(lambda: mapper.overlap_counts(sel, kfs, cam), args.repeat))
        out['cases'][f'K{K}'] = case
        del kfs, views0, views1
    print(json.dumps(out))


if __name__ == '__main__':
    main()
