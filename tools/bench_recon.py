"""Timings of the reconstruction evaluation on one GPU.  Prints one JSON line; every list is [min, median, max] in ms.

Nearest neighbour (csrc/nearest.hip): 200 000 x 200 000 area-weighted surface samples of an analytic room inside the room0
bound, both directions (the metric's own workload), the device route (functional.NearestIndex: grid build and query by
device events, the whole call by a host clock around a synchronise) alternating with scipy.spatial.cKDTree (build + query,
host clock) in this process; the share of queries the brute-force tail finished; the worst case (queries offset by 1 m);
max_rings = 0 alone on a subset of the queries (the pure brute-force rate).  Upload and download are timed separately.

Mesh depth (csrc/mesh_depth.hip): the room mesh subdivided to about 1.5 M faces (and its 24-triangle original, which has
the same images: all triangles large), `--views` random 500 x 500 views from inside the room in batches of `--batch`, by
device events; reported per view, with the image pixels finished per second.

ICP (eval_recon.align_icp): two different sample sets of the room, the source moved by 2 degrees; at `--points` the device
and the host (cKDTree) route alternate, `--repeat` timed runs each after a warm-up pair; at `--icp-points` the device route
alone (a host run takes minutes there), `--repeat` timed runs.  Host clock around a synchronise.

    python tools/bench_recon.py [--points 200000] [--repeat 5] [--views 16] [--batch 8]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def span(xs):
    return [float(np.min(xs)), float(np.median(xs)), float(np.max(xs))]


def subdivide(v, f, times):
    """each triangle into four (edge midpoints; shared midpoints are not merged: the renderer does not need them to be)"""
    for _ in range(times):
        a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
        ab, bc, ca = 0.5 * (a + b), 0.5 * (b + c), 0.5 * (c + a)
        n = len(f)
        v = np.concatenate([a, b, c, ab, bc, ca])
        i = np.arange(n)
        A, B, C, AB, BC, CA = i, i + n, i + 2 * n, i + 3 * n, i + 4 * n, i + 5 * n
        f = np.concatenate([np.stack(t, 1) for t in ((A, AB, CA), (AB, B, BC), (CA, BC, C), (AB, BC, CA))]).astype(np.int32)
    return v, f


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--points', type=int, default=200000)
    ap.add_argument('--repeat', type=int, default=5)
    ap.add_argument('--views', type=int, default=16)
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--subdivide', type=int, default=8)
    ap.add_argument('--brute-queries', type=int, default=20000)
    ap.add_argument('--icp-points', type=int, default=1000000)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_recon.py measures on a GPU; none is visible")
    import bench
    from scipy.spatial import cKDTree
    from evennicer_slam_amd import eval_recon as R
    from evennicer_slam_amd import functional as EF
    from evennicer_slam_amd.synthetic import BoxRoom
    from tests import recon_cases as C

    dev = torch.device('cuda:0')
    room = BoxRoom.for_bound(bench.SCENES['room0'], margin=0.7, seed=1)
    v, f = C.box_room_mesh(room)
    n, rep = args.points, args.repeat
    rec = R.sample_surface(v, f, n, seed=0, device=dev)[0]
    gt = R.sample_surface(v, f, n, seed=1, device=dev)[0]
    rec_h, gt_h = rec.cpu().numpy(), gt.cpu().numpy()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    res = dict(device=torch.cuda.get_device_name(0), points=n, repeat=rep,
               room=[room.room_lo.tolist(), room.room_hi.tolist()])

    def device_pair(q, r, **kw):
        """(build ms, query ms, call ms, tail) of one functional.NearestIndex build + query"""
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ev[0].record()
        index = EF.NearestIndex(r)
        index._grid()
        ev[1].record()
        stats = {}
        d, _ = index.query(q, stats=stats, **kw)
        ev[2].record()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        return ev[0].elapsed_time(ev[1]), ev[1].elapsed_time(ev[2]), (t1 - t0) * 1e3, stats['tail'], d

    def host_pair(q, r):
        t0 = time.perf_counter()
        d, _ = cKDTree(r).query(q)
        return (time.perf_counter() - t0) * 1e3, d

    # both directions of the metric, the two routes alternating; the first round warms up
    t = {k: [] for k in ('build', 'query', 'call', 'host')}
    tails, same = [], True
    for r_ in range(rep + 1):
        b = q = c = h = 0.0
        for (qq, rr, qh, rh) in ((rec, gt, rec_h, gt_h), (gt, rec, gt_h, rec_h)):
            tb, tq, tc, tail, d = device_pair(qq, rr)
            th, dh = host_pair(qh, rh)
            b, q, c, h = b + tb, q + tq, c + tc, h + th
            if r_ == 0:
                tails.append(tail)
                same = same and bool(np.abs(d.cpu().numpy() - dh).max() <= 1e-12)
        if r_:
            for k, x in zip(('build', 'query', 'call', 'host'), (b, q, c, h)):
                t[k].append(x)
    res.update(nn_both_directions_grid_build_ms=span(t['build']), nn_both_directions_query_ms=span(t['query']),
               nn_both_directions_device_call_ms=span(t['call']), nn_both_directions_ckdtree_ms=span(t['host']),
               nn_device_slowest_below_ckdtree_fastest=bool(max(t['call']) < min(t['host'])),
               nn_ckdtree_over_device=float(np.median(t['host']) / np.median(t['call'])),
               nn_tail_share=float(sum(tails) / (2 * n)), nn_distances_equal_ckdtree_to_1e12=same)

    # transfers: the two point sets up, distances and indices down
    up, down = [], []
    d, i = EF.nearest(rec, gt)
    for _ in range(rep):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        a, b = torch.from_numpy(rec_h).to(dev), torch.from_numpy(gt_h).to(dev)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        d.cpu(), i.cpu()
        t2 = time.perf_counter()
        up.append((t1 - t0) * 1e3)
        down.append((t2 - t1) * 1e3)
    res.update(nn_upload_two_sets_ms=span(up), nn_download_dist_idx_ms=span(down))

    # the worst case: every query 1 m off the surfaces' box axis, and the brute-force kernel alone
    off = rec + torch.tensor([1.0, 1.0, 1.0], dtype=torch.float64, device=dev)
    off_h = off.cpu().numpy()
    tw, twh, tail_w = [], [], 0
    for r_ in range(rep + 1):
        _, tq, _, tail_w, _ = device_pair(off, gt)
        th, _ = host_pair(off_h, gt_h)
        if r_:
            tw.append(tq)
            twh.append(th)
    res.update(nn_offset_1m_query_ms=span(tw), nn_offset_1m_ckdtree_ms=span(twh), nn_offset_1m_tail_share=tail_w / n)
    nb = min(args.brute_queries, n)
    tb = []
    for r_ in range(rep + 1):
        _, tq, _, _, _ = device_pair(rec[:nb], gt, max_rings=0)
        if r_:
            tb.append(tq)
    res.update(nn_brute_force_queries=nb, nn_brute_force_ms=span(tb),
               nn_brute_force_pairs_per_s=float(nb * n / (np.median(tb) * 1e-3)))

    # ---- ICP: the device route at the size of a mesh's vertices, both routes at the metric's size -----------------------------
    inv = np.linalg.inv(C.ICP_TRUTH)
    for tag, m, with_host in (('200k', n, True), ('1m', args.icp_points, False)):
        dst = R.sample_surface(v, f, m, seed=2, device=dev)[0]
        src = R._transform(R.sample_surface(v, f, m, seed=3, device=dev)[0], inv)
        src_h, dst_h = (src.cpu().numpy(), dst.cpu().numpy()) if with_host else (None, None)
        ti, th, its, ith = [], [], 0, 0
        for r_ in range(rep + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            T, its, _, _ = R.align_icp(src, dst)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            if with_host:
                Th, ith, _, _ = R.align_icp(src_h, dst_h)
            t2 = time.perf_counter()
            if r_:
                ti.append((t1 - t0) * 1e3)
                th.append((t2 - t1) * 1e3)
        res[f'icp_{tag}_points'] = m
        res[f'icp_{tag}_device_ms'] = span(ti)
        res[f'icp_{tag}_iterations'] = its
        res[f'icp_{tag}_max_abs_from_truth'] = float(np.abs(T - C.ICP_TRUTH).max())
        if with_host:
            res[f'icp_{tag}_host_ms'] = span(th)
            res[f'icp_{tag}_host_iterations'] = ith
            res[f'icp_{tag}_device_host_max_abs'] = float(np.abs(T - Th).max())
            res[f'icp_{tag}_device_slowest_below_host_fastest'] = bool(max(ti) < min(th))

    # ---- mesh depth -----------------------------------------------------------------------------------------------------
    cam = R.EVAL_CAM
    extents, transform = R.view_box(v)
    c2w, _ = R.sample_views(extents, transform, args.views, np.zeros((0, 3)), cam=cam, seed=0, device=dev)
    w2c = EF.world_to_camera(list(c2w))
    fine_v, fine_f = subdivide(v, f, args.subdivide)
    meshes = {'coarse': (torch.from_numpy(v).to(dev), torch.from_numpy(f).to(dev)),
              'fine': (torch.from_numpy(fine_v).to(dev), torch.from_numpy(fine_f).to(dev))}
    images = {}
    for name, (mv, mf) in meshes.items():
        ts = []
        for r_ in range(rep + 1):
            torch.cuda.synchronize()
            ev[0].record()
            out = [EF.mesh_depth(mv, mf, w2c[lo:lo + args.batch], cam) for lo in range(0, args.views, args.batch)]
            ev[1].record()
            torch.cuda.synchronize()
            if r_:
                ts.append(ev[0].elapsed_time(ev[1]) / args.views)
        images[name] = torch.cat(out)
        res[f'depth_{name}_faces'] = int(mf.shape[0])
        res[f'depth_{name}_ms_per_view'] = span(ts)
    px = args.views * cam['H'] * cam['W']
    res.update(depth_views=args.views, depth_batch=args.batch, depth_image=[cam['H'], cam['W']],
               depth_hit_share=float((images['fine'] > 0).double().mean()),
               depth_fine_equals_coarse_max_abs=float((images['fine'] - images['coarse']).abs().max()),
               depth_fine_image_pixels_per_s=float(px / args.views / (res['depth_fine_ms_per_view'][1] * 1e-3)),
               depth_fine_1000_views_two_meshes_s=float(2 * 1000 * res['depth_fine_ms_per_view'][1] * 1e-3))
    print(json.dumps(res))


if __name__ == '__main__':
    main()
