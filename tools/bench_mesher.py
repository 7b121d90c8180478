"""Mesh extraction timings on one GPU: mesher.Mesher.get_mesh at 256^3 on the room0 scene (bench.py's seeded random-init map,
one keyframe at the bench camera), by phase, and the HIP marching cubes split into its count and emit calls against the
numpy restatement (tests/mc_numpy.py) on the same volume; then the `clean` phase of get_mesh through the device route
(csrc/mesh_clean.hip) and the host route (scipy / numpy), alternating in this process, and the device cleaning split into its
calls by device events.  Prints one JSON line.

    python tools/bench_mesher.py [--resolution 256] [--repeat 5]"""
import argparse
import ctypes
import json
import os
import sys
import tempfile
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--resolution', type=int, default=256)
    ap.add_argument('--repeat', type=int, default=5)
    args = ap.parse_args()
    import bench
    import evennicer_slam_amd as E
    from evennicer_slam_amd import functional as EF
    from evennicer_slam_amd.mesher import MESHING_DEFAULTS, Mesher
    from tests import mc_numpy as M

    dev = 'cuda:0'
    sc = bench.build_scene_cpu('room0', seed=0)
    model = sc['model'].cuda()
    bench.attach_bounds(model, sc['bound'])
    grids = {k: v.cuda() for k, v in sc['grids'].items()}
    renderer = E.Renderer(sc['cfg'], None, types.SimpleNamespace(nice=True, bound=sc['bound'], **sc['cam']))
    cfg = dict(sc['cfg'], meshing=dict(MESHING_DEFAULTS, resolution=args.resolution),
               mapping=dict(marching_cubes_bound=bench.SCENES['room0']))
    mesher = Mesher(cfg, None, types.SimpleNamespace(renderer=renderer, bound=sc['bound'], nice=True, verbose=False, **sc['cam']))
    c2w = torch.eye(4)
    c2w[:3] = sc['c2w']
    kf = dict(est_c2w=c2w.cuda(), depth=sc['depth_img'].cuda(), color=sc['color_img'].cuda())

    phases, counts = [], None
    with tempfile.TemporaryDirectory() as tmp, torch.no_grad():
        for r in range(args.repeat + 1):                 # the first call warms up (module loads, caches)
            verts, faces, colors = mesher.get_mesh(os.path.join(tmp, 'm.ply'), grids, model, [kf], None, 0, device=dev)
            if r:
                phases.append(dict(mesher.timing))
            counts = (len(verts), len(faces))

        # marching cubes alone on the lattice volume: count (with the read-back of the sizes) and emit
        xyz = mesher.get_grid_uniform(args.resolution)['xyz']
        vol = mesher.lattice_volume(grids, model, xyz, mesher.get_bound_from_frames([kf]), dev)
        lib = E._lib.lib()
        nx, ny, nz = vol.shape
        nb = ctypes.c_int64()
        E._lib.check(lib.enslam_marching_cubes_workspace(nx, ny, nz, ctypes.byref(nb)), "workspace")
        ws = torch.empty(nb.value, dtype=torch.uint8, device=dev)
        cnt = torch.empty(2, dtype=torch.int32, device=dev)
        org = (ctypes.c_double * 3)(*[a[0] for a in xyz])
        spc = (ctypes.c_double * 3)(*[a[2] - a[1] for a in xyz])
        s = EF._stream()
        t_count, t_emit, t_call = [], [], []
        for r in range(args.repeat + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            E._lib.check(lib.enslam_marching_cubes_count(vol.data_ptr(), nx, ny, nz, 0.0, ws.data_ptr(), cnt.data_ptr(), s), "count")
            V, F = cnt.tolist()
            t1 = time.perf_counter()
            v = torch.empty((V, 3), dtype=torch.float64, device=dev)
            f = torch.empty((F, 3), dtype=torch.int32, device=dev)
            E._lib.check(lib.enslam_marching_cubes_emit(vol.data_ptr(), nx, ny, nz, 0.0, org, spc, ws.data_ptr(), V, F,
                                                        v.data_ptr(), f.data_ptr(), s), "emit")
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            EF.marching_cubes(vol, 0.0, list(org), list(spc))
            torch.cuda.synchronize()
            t3 = time.perf_counter()
            if r:
                t_count.append(t1 - t0)
                t_emit.append(t2 - t1)
                t_call.append(t3 - t2)
        vol_h = vol.cpu().numpy()
        t0 = time.perf_counter()
        nv, nf = M.marching_cubes(vol_h, 0.0, list(org), list(spc))
        t_np = time.perf_counter() - t0
        same = bool(np.array_equal(nf, f.cpu().numpy()) and np.abs(nv - v.cpu().numpy()).max(initial=0) <= 1e-12)

        # the cleaning of get_mesh through both routes, alternating (the first pair warms up)
        clean = {'device': [], 'host': []}
        comps = {'device': [], 'host': []}
        for r in range(args.repeat + 1):
            for route in ('device', 'host'):
                mesher.clean_on_host = route == 'host'
                mesher.get_mesh(os.path.join(tmp, 'm.ply'), grids, model, [kf], None, 0, device=dev)
                if r:
                    clean[route].append(mesher.timing['clean'])
                    comps[route].append(mesher.timing['clean_components'])
        mesher.clean_on_host = False
        clean_stats = dict(mesher.clean_stats)

        # the device cleaning alone on the marching-cubes output, by call (device events): labelling only, count, emit
        keep = (mesher.point_classes(mesher._views([kf], None, 0, dev, False), dev, points=v) == 1).view(torch.uint8)
        Vn, Fn = int(v.shape[0]), int(f.shape[0])
        E._lib.check(lib.enslam_mesh_clean_workspace(Vn, Fn, ctypes.byref(nb)), "workspace")
        cws = torch.empty(nb.value, dtype=torch.uint8, device=dev)
        clean_ws_bytes = nb.value
        lab = torch.empty(Fn, dtype=torch.int32, device=dev)
        cnt3 = torch.empty(3, dtype=torch.int32, device=dev)
        min_area = mesher.remove_small_geometry_threshold * mesher.scale * mesher.scale
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        t_lab, t_cnt, t_emt = [], [], []
        for r in range(args.repeat + 1):
            torch.cuda.synchronize()
            ev[0].record()
            E._lib.check(lib.enslam_mesh_components(f.data_ptr(), Fn, Vn, cws.data_ptr(), lab.data_ptr(), s), "components")
            ev[1].record()
            E._lib.check(lib.enslam_mesh_clean_count(v.data_ptr(), Vn, f.data_ptr(), Fn, keep.data_ptr(), min_area, 0, cws.data_ptr(),
                                                     cnt3.data_ptr(), s), "clean_count")
            Vo, Fo, Nc = cnt3.tolist()
            vo = torch.empty((Vo, 3), dtype=torch.float64, device=dev)
            fo = torch.empty((Fo, 3), dtype=torch.int32, device=dev)
            torch.cuda.synchronize()
            ev[2].record()
            E._lib.check(lib.enslam_mesh_clean_emit(v.data_ptr(), Vn, f.data_ptr(), Fn, cws.data_ptr(), Vo, Fo, vo.data_ptr(),
                                                    fo.data_ptr(), None, s), "clean_emit")
            ev[3].record()
            torch.cuda.synchronize()
            if r:
                t_lab.append(ev[0].elapsed_time(ev[1]))
                t_emt.append(ev[2].elapsed_time(ev[3]))
            if r == 0:
                first_cnt = (Vo, Fo, Nc)
        for r in range(args.repeat):                     # the count call on its own (above, the read-back of the counts follows it)
            torch.cuda.synchronize()
            ev[0].record()
            E._lib.check(lib.enslam_mesh_clean_count(v.data_ptr(), Vn, f.data_ptr(), Fn, keep.data_ptr(), min_area, 0, cws.data_ptr(),
                                                     cnt3.data_ptr(), s), "clean_count")
            ev[1].record()
            torch.cuda.synchronize()
            t_cnt.append(ev[0].elapsed_time(ev[1]))
        assert tuple(cnt3.tolist()) == first_cnt

    med = lambda xs: float(np.median(xs)) * 1e3        # noqa: E731
    span = lambda xs: [float(np.min(xs)) * 1e3, float(np.median(xs)) * 1e3, float(np.max(xs)) * 1e3]     # noqa: E731
    res = dict(resolution=args.resolution, scene='room0 (seeded random-init map, one keyframe)',
               vertices=counts[0], faces=counts[1], mc_vertices_unclean=int(V), mc_faces_unclean=int(F),
               get_mesh_ms={k: med([p[k] for p in phases]) for k in phases[0]},
               mc_count_ms=med(t_count), mc_emit_ms=med(t_emit), mc_binding_call_ms=med(t_call),
               mc_numpy_ms=t_np * 1e3, mc_equal_to_numpy=same,
               clean_device_ms_min_med_max=span(clean['device']), clean_host_ms_min_med_max=span(clean['host']),
               clean_components_device_ms_min_med_max=span(comps['device']),
               clean_components_host_ms_min_med_max=span(comps['host']),
               clean_device_faster_in_every_repeat=bool(max(clean['device']) < min(clean['host'])),
               clean_host_over_device=float(np.median(clean['host']) / np.median(clean['device'])),
               clean_components_after_mask=clean_stats.get('components'), clean_vertices=clean_stats.get('vertices'),
               clean_faces=clean_stats.get('faces'),
               mesh_components_call_ms=float(np.median(t_lab)), mesh_clean_count_call_ms=float(np.median(t_cnt)),
               mesh_clean_emit_call_ms=float(np.median(t_emt)), mesh_clean_workspace_mib=clean_ws_bytes / 2**20,
               device=torch.cuda.get_device_name(0))
    print(json.dumps(res))


if __name__ == '__main__':
    main()
