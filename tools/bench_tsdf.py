"""TSDF fusion timings on one GPU (tsdf.TSDFVolume, csrc/tsdf.hip): the analytic room of synthetic.BoxRoom.for_bound(room0
bound) seen by the 680 x 1200 bench camera along a trajectory of 1, 32 and 240 keyframes, the reference's voxel size
(4 / 512 m, sdf_trunc 0.04 m, stride 4, no colour).  From device events, median [min - max] over the frames of the repeats:
integrate ms per frame split into touch, allocation (the torch plumbing between the kernels) and the integrate kernel;
extraction ms; blocks and bytes.  Then get_mesh's `hull` phase with bound_method 'depth_points' and 'tsdf', alternating in this
process after a warm-up pair, at 1 and 32 keyframes.  Prints one JSON line.

    python tools/bench_tsdf.py [--repeat 3] [--resolution 128] [--frames 1,32,240] [--hull-frames 1,32]"""
import argparse
import json
import os
import sys
import tempfile
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def span(xs):
    return [float(np.min(xs)), float(np.median(xs)), float(np.max(xs))] if len(xs) else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeat', type=int, default=3)
    ap.add_argument('--resolution', type=int, default=128)
    ap.add_argument('--frames', default='1,32,240')
    ap.add_argument('--hull-frames', default='1,32')
    args = ap.parse_args()
    import bench
    import evennicer_slam_amd as E
    from evennicer_slam_amd.mesher import MESHING_DEFAULTS, Mesher
    from evennicer_slam_amd.synthetic import BoxRoom, trajectory
    from evennicer_slam_amd.tsdf import TSDFVolume

    dev = 'cuda:0'
    sc = bench.build_scene_cpu('room0', seed=0)
    cam = sc['cam']
    room = BoxRoom.for_bound(sc['bound'], margin=0.7, seed=0)
    voxel, trunc = 4.0 / 512.0, 0.04

    def keyframes(n):
        out = []
        for c2w in trajectory(room, n, step=2.0 / n, yaw_deg=180.0 / n):
            col, dep = room.render(c2w.double(), cam, device=dev)
            out.append(dict(est_c2w=c2w.to(dev), depth=dep, color=col.float()))
        return out

    res = dict(voxel_length=voxel, sdf_trunc=trunc, stride=4, camera=[cam['H'], cam['W']], device=torch.cuda.get_device_name(0),
               scene='BoxRoom.for_bound(room0 bound, margin 0.7)', fuse={}, hull={})
    sets = {}
    for n in sorted({int(x) for x in (args.frames + ',' + args.hull_frames).split(',')}):
        sets[n] = keyframes(n)
    for n in (int(x) for x in args.frames.split(',')):
        kfs = sets[n]
        touch, alloc, kern, total, extract = [], [], [], [], []
        for r in range(args.repeat + 1):                 # the first build warms up
            lo, hi = TSDFVolume.frames_box(kfs, cam, dev)
            vol = TSDFVolume(voxel, trunc, lo - trunc, hi + trunc, cam, color=False, depth_sampling_stride=4, device=dev)
            vol.profile = []
            for kf in kfs:
                vol.integrate(kf['depth'], None, kf['est_c2w'])
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            torch.cuda.synchronize()
            ev[0].record()
            verts, faces, _ = vol.extract_mesh()
            ev[1].record()
            torch.cuda.synchronize()
            if r:
                for m in vol.profile:
                    touch.append(m[0].elapsed_time(m[1]))
                    alloc.append(m[1].elapsed_time(m[2]))
                    kern.append(m[2].elapsed_time(m[3]))
                    total.append(m[0].elapsed_time(m[3]))
                extract.append(ev[0].elapsed_time(ev[1]))
        st = vol.stats
        res['fuse'][str(n)] = dict(integrate_ms_per_frame_min_med_max=span(total), touch_ms=span(touch), allocation_ms=span(alloc),
                                   integrate_kernel_ms=span(kern), extract_ms_min_med_max=span(extract), blocks=st['blocks'],
                                   bytes=st['bytes'], table=vol.nu, vertices=int(verts.shape[0]), faces=int(faces.shape[0]),
                                   integrated_voxels_per_frame=float(np.mean([f['integrated_voxels'] for f in st['frames']])),
                                   touched_outside=sum(f['touched_outside'] for f in st['frames']))
        del vol, verts, faces

    # get_mesh's hull phase, both methods alternating (seeded random-init room0 map; only the keyframes matter to this phase)
    model = sc['model'].cuda()
    bench.attach_bounds(model, sc['bound'])
    grids = {k: v.cuda() for k, v in sc['grids'].items()}
    renderer = E.Renderer(sc['cfg'], None, types.SimpleNamespace(nice=True, bound=sc['bound'], **cam))
    cfg = dict(sc['cfg'], meshing=dict(MESHING_DEFAULTS, resolution=args.resolution), mapping=dict(marching_cubes_bound=bench.SCENES['room0']))
    mesher = Mesher(cfg, None, types.SimpleNamespace(renderer=renderer, bound=sc['bound'], nice=True, verbose=False, **cam))
    with tempfile.TemporaryDirectory() as tmp, torch.no_grad():
        for n in (int(x) for x in args.hull_frames.split(',')):
            kfs = sets[n]
            hull = {'depth_points': [], 'tsdf': []}
            steps = {k: [] for k in ('hull_fuse', 'hull_extract', 'hull_candidates', 'hull_scipy')}
            planes = {}
            for r in range(args.repeat + 1):             # the first pair warms up
                for method in ('depth_points', 'tsdf'):
                    mesher.bound_method = method
                    mesher.get_mesh(os.path.join(tmp, 'm.ply'), grids, model, kfs, None, 0, device=dev, clean_mesh=False, color=False)
                    if r:
                        hull[method].append(mesher.timing['hull'] * 1e3)
                        if method == 'tsdf':
                            for k in steps:
                                steps[k].append(mesher.timing[k] * 1e3)
            for method in hull:
                mesher.bound_method = method
                planes[method] = int(mesher.get_bound_from_frames(kfs, 1, dev).shape[0])
            res['hull'][str(n)] = dict(depth_points_ms_min_med_max=span(hull['depth_points']), tsdf_ms_min_med_max=span(hull['tsdf']),
                                       slowest_tsdf_below_fastest_depth_points=bool(max(hull['tsdf']) < min(hull['depth_points'])),
                                       tsdf_steps_ms_median={k: float(np.median(v)) for k, v in steps.items()},
                                       half_spaces=planes, tsdf_blocks=mesher.tsdf_stats.get('blocks'),
                                       tsdf_points=mesher.tsdf_stats.get('points'), tsdf_candidates=mesher.tsdf_stats.get('candidates'))
    print(json.dumps(res))


if __name__ == '__main__':
    main()
