"""One frame of the headless visualiser on one GPU (csrc/scene_raster.hip): the 1080 x 1920 image of mesher.Mesher.get_mesh's
256^3 mesh of the room0 scene (bench.py's seeded random-init map, about 1.5 M faces) with both camera actors and a 2 000-pose
trajectory, from the viewer's seat two units behind the first pose.  Device events, the median [min - max] of `--repeat` calls
after a warm-up: the whole frame, then its fill + triangle pass, point pass and resolve pass one by one on one workspace, and
in the same run enslam_mesh_depth at the same mesh, camera and image size.  Prints one JSON line.

    python tools/bench_viz.py [--resolution 256] [--repeat 10] [--height 1080] [--width 1920]"""
import argparse
import ctypes
import json
import os
import sys
import tempfile
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--resolution', type=int, default=256)
    ap.add_argument('--repeat', type=int, default=10)
    ap.add_argument('--height', type=int, default=1080)
    ap.add_argument('--width', type=int, default=1920)
    args = ap.parse_args()
    import bench
    import evennicer_slam_amd as E
    from evennicer_slam_amd import functional as EF
    from evennicer_slam_amd import viz
    from evennicer_slam_amd.mesher import MESHING_DEFAULTS, Mesher

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

    # a 2 000-pose trajectory: the bench camera drifting along a helix; the ground truth a little beside it
    n_traj = 2000
    first = c2w.double().numpy()
    est = np.repeat(first[None], n_traj + 1, axis=0)
    a = np.linspace(0.0, 6 * np.pi, n_traj + 1)
    est[:, :3, 3] += np.stack([0.4 * np.sin(a), 0.4 * (1 - np.cos(a)), 0.1 * a / a[-1]], -1)
    gt = est.copy()
    gt[:, :3, 3] += 0.02
    with tempfile.TemporaryDirectory() as tmp, torch.no_grad():
        path = os.path.join(tmp, '00000_mesh.ply')
        mesher.get_mesh(path, grids, model, [kf], None, 0, device=dev)
        front = viz.SLAMFrontend(tmp, est[0], cam_scale=0.3, estimate_c2w_list=est, gt_c2w_list=gt, H=args.height, W=args.width,
                                 device=dev)
        front.update_mesh(path)
    front.update_pose(1, est[n_traj].copy(), gt=False)
    front.update_pose(1, gt[n_traj].copy(), gt=True)
    front.update_cam_trajectory(n_traj + 1, gt=False)
    front.update_cam_trajectory(n_traj + 1, gt=True)
    v, f, col, nrm = front.mesh
    pts, pcol = front.scene_points()
    pts, pcol = torch.from_numpy(pts).to(dev), torch.from_numpy(pcol).to(dev)
    w2c = torch.from_numpy(np.ascontiguousarray(np.linalg.inv(front.view_c2w)[:3])).to(dev)
    cam, H, W = front.cam, args.height, args.width
    V, F, P = int(v.shape[0]), int(f.shape[0]), int(pts.shape[0])

    lib = E._lib.lib()
    nb = ctypes.c_int64()
    E._lib.check(lib.enslam_scene_raster_workspace(F, 1, H, W, ctypes.byref(nb)), "workspace")
    nb_raster = nb.value
    ws = torch.empty(nb_raster, dtype=torch.uint8, device=dev)
    rgb = torch.empty((H, W, 3), dtype=torch.uint8, device=dev)
    ids = torch.empty((H, W), dtype=torch.int32, device=dev)
    s = EF._stream()

    def raster(passes):
        E._lib.check(lib.enslam_scene_raster(v.data_ptr(), V, f.data_ptr(), F, None if col is None else col.data_ptr(), nrm.data_ptr(),
                                             pts.data_ptr(), P, pcol.data_ptr(), viz.POINT_SIZE, w2c.data_ptr(), 1, H, W, cam['fx'],
                                             cam['fy'], cam['cx'], cam['cy'], 0.0, viz.Z_FAR, 1, 0.35, 0xFFFFFF, passes, ws.data_ptr(),
                                             nb_raster, rgb.data_ptr(), None, ids.data_ptr(), s), "enslam_scene_raster")

    E._lib.check(lib.enslam_mesh_depth_workspace(F, 1, ctypes.byref(nb)), "workspace")
    dws = torch.empty(nb.value, dtype=torch.uint8, device=dev)
    depth = torch.empty((H, W), dtype=torch.float32, device=dev)

    def mesh_depth():
        E._lib.check(lib.enslam_mesh_depth(v.data_ptr(), V, f.data_ptr(), F, w2c.data_ptr(), 1, H, W, cam['fx'], cam['fy'], cam['cx'],
                                           cam['cy'], 0.0, viz.Z_FAR, dws.data_ptr(), depth.data_ptr(), s), "enslam_mesh_depth")

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    t = {k: [] for k in ('frame', 'visibility', 'points', 'resolve', 'mesh_depth', 'normals')}
    for r in range(args.repeat + 1):                     # the first round warms up
        row = dict(frame=timed(lambda: raster(7)))
        whole = rgb.clone()
        row.update(visibility=timed(lambda: raster(1)), points=timed(lambda: raster(2)), resolve=timed(lambda: raster(4)))
        assert torch.equal(whole, rgb)                   # the three passes one by one give the frame
        row.update(mesh_depth=timed(mesh_depth), normals=timed(lambda: EF.vertex_normals(v, f)))
        if r:
            for k, x in row.items():
                t[k].append(x)
    span = lambda xs: [float(np.median(xs)), float(np.min(xs)), float(np.max(xs))]     # noqa: E731
    idh = ids.cpu().numpy()
    res = dict(scene=f'room0 (seeded random-init map, one keyframe), get_mesh at {args.resolution}^3', H=H, W=W, vertices=V,
               faces=F, points=P, trajectory_poses=n_traj, repeat=args.repeat,
               frame_ms_med_min_max=span(t['frame']), visibility_ms_med_min_max=span(t['visibility']),
               points_ms_med_min_max=span(t['points']), resolve_ms_med_min_max=span(t['resolve']),
               mesh_depth_ms_med_min_max=span(t['mesh_depth']), vertex_normals_ms_med_min_max=span(t['normals']),
               pixels_mesh=float(np.mean(idh >= 0)), pixels_points=float(np.mean(idh < -1)), pixels_background=float(np.mean(idh == -1)),
               workspace_mib=nb_raster / 2**20, device=torch.cuda.get_device_name(0))
    print(json.dumps(res))


if __name__ == '__main__':
    main()
