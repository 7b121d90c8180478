"""`Mesher` with the reference's constructor and `get_mesh` signature (src/utils/Mesher.py:13-51,349-574), on the HIP path:
the lattice is formed on the device chunk by chunk and evaluated through enslam_eval_points, the iso-surface is the HIP
marching cubes (functional.marching_cubes), and the file is written by a small PLY writer of our own.  skimage, trimesh and
open3d are not needed.

Numerical differences from the reference:
  * inside mask: the reference fuses the keyframes into a TSDF (open3d) and keeps the lattice points inside the convex hull
    of that mesh and the camera centres, scaled by `clean_mesh_bound_scale`.  `bound_method` selects how the hull's points
    are made.  'depth_points' (the default): the keyframes' back-projected valid depth pixels and the camera centres.
    'tsdf' (HIP device only): the reference's way -- the keyframes fused into a block-sparse TSDF volume with its
    voxel_length 4 * scale / 512 and sdf_trunc 0.04 * scale (tsdf.TSDFVolume, csrc/tsdf.hip), the vertices of that volume's
    mesh and the camera centres, thinned by `hull_candidates` before scipy sees them.  What still differs from Open3D
    there: float64 per-voxel geometry, a deterministic output order, a table-bounded volume sized from the frames.  Either
    way the hull (scipy.spatial.ConvexHull) is scaled about the mean of its vertices and tested against the lattice by
    its half-spaces on the GPU;
  * faces: the case table resolves ambiguous cube faces by one fixed rule (csrc/mc_tables.hpp), skimage by the Lewiner
    table, so face sets may differ in ambiguous cells; the vertex set does not;
  * order: after cleaning, the kept faces keep their marching-cubes order and the vertices their order, where trimesh
    regroups both per connected component.  The geometry is the same.
With clean_mesh on a HIP device the mesh stays on the device from the lattice to the download before the file is written: the
vertex mask, the connected-component filter and the compaction are functional.mesh_clean (csrc/mesh_clean.hip), the colour
query and the forecast classes read the device vertices.  The host helpers at the end of this file (face_components,
filter_components, drop_unreferenced) are what device='cpu' runs, what `mesher.clean_on_host = True` (an attribute, set after
construction) selects on a HIP device, and what the tests compare the kernels with; both routes give bit-identical arrays and
files.
On a HIP device the seen / forecast / unseen classification (point_masks, with and without depth_test, and the lattice of
show_forecast) is one enslam_visibility launch per chunk of points (csrc/visibility.hip).  On device='cpu' point_masks keeps
its torch form for depth_test False; depth_test True and show_forecast need the HIP device there (NotImplementedError).
Not implemented anywhere: the iMAP colour method render_ray_along_normal."""
import numpy as np
import torch

from . import functional as EF

# configs/nice_slam.yaml `meshing` (the reference's defaults), for callers whose config has no such section
MESHING_DEFAULTS = dict(level_set=0, resolution=256, eval_rec=False, clean_mesh=True, depth_test=False, mesh_coarse_level=False,
                        clean_mesh_bound_scale=1.02, get_largest_components=False,
                        color_mesh_extraction_method='direct_point_query', remove_small_geometry_threshold=0.2,
                        bound_method='depth_points')
BOUND_METHODS = ('depth_points', 'tsdf')


class Mesher(object):

    def __init__(self, cfg, args, slam, points_batch_size=500000, ray_batch_size=100000):
        self.points_batch_size = points_batch_size
        self.ray_batch_size = ray_batch_size
        self.renderer = slam.renderer
        self.coarse = cfg['coarse']
        self.scale = cfg['scale']
        self.occupancy = cfg['occupancy']

        self.resolution = cfg['meshing']['resolution']
        self.level_set = cfg['meshing']['level_set']
        self.clean_mesh_bound_scale = cfg['meshing']['clean_mesh_bound_scale']
        self.remove_small_geometry_threshold = cfg['meshing']['remove_small_geometry_threshold']
        self.color_mesh_extraction_method = cfg['meshing']['color_mesh_extraction_method']
        self.get_largest_components = cfg['meshing']['get_largest_components']
        self.depth_test = cfg['meshing']['depth_test']
        # how get_bound_from_frames makes the points of the hull (the header comment); settable after construction
        self.bound_method = cfg['meshing'].get('bound_method', 'depth_points')
        if self.bound_method not in BOUND_METHODS:
            raise ValueError(f"meshing.bound_method must be one of {BOUND_METHODS} (got {self.bound_method!r})")
        self.tsdf_stats = {}        # blocks / bytes / per-frame counts of the last 'tsdf' bound

        self.bound = slam.bound
        self.nice = slam.nice
        self.verbose = slam.verbose

        self.marching_cubes_bound = torch.from_numpy(np.array(cfg['mapping']['marching_cubes_bound']) * self.scale)
        # the reference opens a dataset reader only for its length; nothing here reads frames
        self.n_img = getattr(slam, 'n_img', None)

        self.H, self.W, self.fx, self.fy, self.cx, self.cy = slam.H, slam.W, slam.fx, slam.fy, slam.cx, slam.cy
        self.timing = {}            # seconds of the last get_mesh, per phase (tools/bench_mesher.py)
        # set after construction (the constructor keeps the reference's signature): True runs the cleaning of get_mesh through
        # the host helpers below on a HIP device as well -- what device='cpu' always does, and what the device route is tested against
        self.clean_on_host = False
        self.clean_stats = {}       # components / vertices / faces of the last device-route cleaning

    # ------------------------------------------------------------------ masks
    def _views(self, keyframe_dict, estimate_c2w_list, idx, device, get_mask_use_all_frames):
        """(w2c float64 numpy [K,3,4], limit float32 [K] or None, depth float32 [K,H,W] or None) of the cameras point_masks
        tests: every frame up to idx (no depth limit, no depth test: Mesher.py:88-122) or the keyframes, each with
        1.1 x its largest depth as limit, or with its depth image when depth_test is set (Mesher.py:124-186)."""
        if get_mask_use_all_frames:
            return EF.world_to_camera([estimate_c2w_list[i] for i in range(0, idx + 1)]), None, None
        w2c = EF.world_to_camera([kf['est_c2w'] for kf in keyframe_dict])
        if len(keyframe_dict) == 0:
            return w2c, None, None
        if self.depth_test:
            return w2c, None, torch.stack([kf['depth'].to(device).float().reshape(self.H, self.W) for kf in keyframe_dict])
        return w2c, torch.stack([torch.max(kf['depth']).to(device).float() * 1.1 for kf in keyframe_dict]), None

    def point_classes(self, views, device, points=None, lattice=None):
        """uint8 device tensor [P] (0 unseen, 1 seen, 2 forecast) of explicit points [P,3] or of a lattice (three float32
        device axes, Mesher.lattice_volume's order), one enslam_visibility call per points_batch_size chunk: with depth_test
        the forecast test uses the largest depth sample of the chunk, as the reference's per-chunk torch.max does."""
        w2c, limit, depth = views
        w2c = torch.from_numpy(w2c).float().to(device)          # rounded and uploaded once for all chunks
        cam = dict(H=self.H, W=self.W, fx=self.fx, fy=self.fy, cx=self.cx, cy=self.cy)
        P = points.shape[0] if points is not None else lattice[0].shape[0] * lattice[1].shape[0] * lattice[2].shape[0]
        out = torch.empty(P, dtype=torch.uint8, device=device)
        for lo in range(0, P, self.points_batch_size):
            n = min(self.points_batch_size, P - lo)
            if points is not None:
                cls, _ = EF.visibility(points[lo:lo + n].to(device).float(), w2c, cam, limit=limit, depth=depth)
            else:
                cls, _ = EF.visibility(None, w2c, cam, limit=limit, depth=depth, lattice=lattice, first=lo, count=n)
            out[lo:lo + n] = cls
        return out

    def point_masks(self, input_points, keyframe_dict, estimate_c2w_list, idx, device, get_mask_use_all_frames=False):
        """(seen, forecast, unseen) bool numpy masks of the points (Mesher.py:53-211): a point is seen when it projects
        strictly inside the image of a keyframe (or of every frame up to idx), in front of the camera and closer than
        1.1 x that frame's largest depth -- with depth_test, within 2.4 of the keyframe's depth sampled at its pixel instead;
        forecast: the same with the image enlarged by 1000 pixels (with depth_test: closer than the largest depth sample of
        the chunk), and not seen.  HIP device: csrc/visibility.hip; cpu: the torch form below, depth_test False only."""
        if torch.device(device).type == 'cuda':
            if not isinstance(input_points, torch.Tensor):
                input_points = torch.from_numpy(np.asarray(input_points))
            views = self._views(keyframe_dict, estimate_c2w_list, idx, device, get_mask_use_all_frames)
            cls = self.point_classes(views, device, points=input_points.reshape(-1, 3)).cpu().numpy()
            return cls == 1, cls == 2, cls == 0
        return self.point_masks_torch(input_points, keyframe_dict, estimate_c2w_list, idx, device, get_mask_use_all_frames)

    def point_masks_torch(self, input_points, keyframe_dict, estimate_c2w_list, idx, device, get_mask_use_all_frames=False):
        """point_masks as a loop of torch operations over the cameras (depth_test False only): what device='cpu' runs, and the
        baseline tools/bench_visibility.py times the kernel against on the GPU."""
        if self.depth_test:
            raise NotImplementedError("point_masks with depth_test=True needs a HIP device (csrc/visibility.hip)")
        H, W, fx, fy, cx, cy = self.H, self.W, self.fx, self.fy, self.cx, self.cy
        if not isinstance(input_points, torch.Tensor):
            input_points = torch.from_numpy(np.asarray(input_points))
        if get_mask_use_all_frames:
            views = [(estimate_c2w_list[i], None) for i in range(0, idx + 1)]
        else:
            views = [(kf['est_c2w'], kf['depth']) for kf in keyframe_dict]
        K = torch.tensor([[fx, .0, cx], [.0, fy, cy], [.0, .0, 1.0]], dtype=torch.float32, device=device)
        cams = []
        for c2w, depth in views:
            w2c = torch.from_numpy(np.linalg.inv(c2w.detach().cpu().numpy().astype(np.float64))).to(device).float()
            max_depth = torch.max(depth).to(device) * 1.1 if depth is not None else None
            cams.append((w2c, max_depth))
        seen_l, forecast_l = [], []
        for pnts in torch.split(input_points, self.points_batch_size, dim=0):
            points = pnts.to(device).float()
            seen = torch.zeros(points.shape[0], dtype=torch.bool, device=device)
            forecast = torch.zeros_like(seen)
            for w2c, max_depth in cams:
                cam = points @ w2c[:3, :3].T + w2c[:3, 3]
                cam[:, 0] *= -1
                uv = cam @ K.T
                z = uv[:, 2] + 1e-8
                u, v = uv[:, 0] / z, uv[:, 1] / z
                s = (u < W) & (u > 0) & (v < H) & (v > 0) & (z < 0)
                f = (u < W + 1000) & (u > -1000) & (v < H + 1000) & (v > -1000) & (z < 0)
                if max_depth is not None:
                    s &= -cam[:, 2] < max_depth
                    f &= -cam[:, 2] < max_depth
                seen |= s
                forecast |= f
            forecast &= ~seen
            seen_l.append(seen.cpu().numpy())
            forecast_l.append(forecast.cpu().numpy())
        seen = np.concatenate(seen_l) if seen_l else np.zeros(0, bool)
        forecast = np.concatenate(forecast_l) if forecast_l else np.zeros(0, bool)
        return seen, forecast, ~(seen | forecast)

    def get_bound_from_frames(self, keyframe_dict, scale=1, device=None):
        """Half-spaces [K,4] float64 (n . x + d <= 0 inside) of the convex hull of the keyframes' back-projected valid depth
        pixels and camera centres, scaled by clean_mesh_bound_scale about the mean of its vertices (Mesher.py:213-262
        with the TSDF replaced by the depth points themselves).  With bound_method 'tsdf' the points are the vertices of the
        keyframes' fused TSDF mesh and the camera centres, as in the reference; `device` defaults to the keyframes'."""
        if self.bound_method not in BOUND_METHODS:
            raise ValueError(f"bound_method must be one of {BOUND_METHODS} (got {self.bound_method!r})")
        if self.bound_method == 'tsdf':
            import time
            points = self.tsdf_bound_points(keyframe_dict, scale, device)
            t0 = time.perf_counter()
            halfspaces = hull_halfspaces(points, self.clean_mesh_bound_scale)
            self.timing['hull_scipy'] = time.perf_counter() - t0
            return halfspaces
        return hull_halfspaces(backprojected_points(keyframe_dict, self.H, self.W, self.fx, self.fy, self.cx, self.cy),
                               self.clean_mesh_bound_scale)

    def tsdf_bound_points(self, keyframe_dict, scale=1, device=None):
        """float64 numpy [P,3]: the candidates for the hull of Mesher.py:214-279 -- the keyframes' depth fused with est_c2w into a
        TSDF volume of voxel_length 4 * scale / 512 and sdf_trunc 0.04 * scale (stride 4, no colour: the reference integrates
        colour and never reads it), the vertices of its mesh and the camera centres, passed through hull_candidates."""
        from .tsdf import TSDFVolume
        if device is None:
            device = keyframe_dict[0]['depth'].device if len(keyframe_dict) else 'cpu'
        if torch.device(device).type != 'cuda':
            raise NotImplementedError("bound_method 'tsdf' needs a HIP device (csrc/tsdf.hip)")
        import time
        cam = dict(H=self.H, W=self.W, fx=self.fx, fy=self.fy, cx=self.cx, cy=self.cy)
        frames = [dict(depth=kf['depth'].reshape(self.H, self.W), est_c2w=kf['est_c2w']) for kf in keyframe_dict]
        t0 = time.perf_counter()

        def lap(name):                  # seconds per step of the bound, beside timing['hull'] (tools/bench_tsdf.py)
            nonlocal t0
            torch.cuda.synchronize(device)
            self.timing[name] = time.perf_counter() - t0
            t0 = time.perf_counter()
        vol = TSDFVolume.for_frames(frames, cam, 4.0 * scale / 512.0, 0.04 * scale, color=False, depth_sampling_stride=4, device=device)
        lap('hull_fuse')
        verts, _, _ = vol.extract_mesh()
        lap('hull_extract')
        centres = torch.stack([kf['est_c2w'].detach().double()[:3, 3] for kf in keyframe_dict]).to(verts.device)
        points = hull_candidates(torch.cat([verts, centres])).cpu().numpy()
        lap('hull_candidates')
        self.tsdf_stats = dict(vol.stats, points=int(verts.shape[0]) + len(keyframe_dict), candidates=int(points.shape[0]))
        return points

    # ------------------------------------------------------------------ lattice
    def get_grid_uniform(self, resolution):
        """Axes of the lattice (Mesher.py:318-347): np.linspace over marching_cubes_bound padded by 0.05 per side."""
        bound = self.marching_cubes_bound
        padding = 0.05
        xyz = [np.linspace(float(bound[a][0]) - padding, float(bound[a][1]) + padding, resolution) for a in range(3)]
        return {"xyz": xyz}

    def lattice_volume(self, c, decoders, xyz, halfspaces, device):
        """float32 [nx, ny, nz] volume: stage-`fine` occupancy of the lattice points (float32 coordinates, as the reference's
        dtype=torch.float grid), 100 outside the scene bound (enslam_eval_points' mask) and outside the hull."""
        ax = [torch.from_numpy(a.astype(np.float32)).to(device) for a in xyz]
        nx, ny, nz = (len(a) for a in xyz)
        vol = torch.empty((nx, ny, nz), dtype=torch.float32, device=device)
        flat = vol.view(-1)
        hs = torch.from_numpy(halfspaces).to(device) if halfspaces is not None else None
        coarse_bound = self.renderer._coarse_bound(decoders)
        for lo in range(0, nx * ny * nz, self.points_batch_size):
            lin = torch.arange(lo, min(lo + self.points_batch_size, nx * ny * nz), device=device)
            pts = torch.stack([ax[0][lin // (ny * nz)], ax[1][(lin // nz) % ny], ax[2][lin % nz]], 1)
            raw = EF.eval_points(pts, decoders, c, 'fine', self.bound, apply_mask=True, coarse_bound=coarse_bound)
            z = flat[lo:lo + lin.shape[0]]
            z.copy_(raw[:, 3])
            if hs is not None:
                z.masked_fill_(~inside_halfspaces(pts, hs), 100.0)
        return vol

    def forecast_volume(self, c, decoders, xyz, views, device):
        """(float32 [nx, ny, nz] volume, uint8 [nx*ny*nz] classes) of show_forecast (Mesher.py:389-425): stage-`fine` occupancy
        where the lattice point is seen, stage-`coarse` occupancy + 0.2 where it is forecast, -100 where unseen.  Only the
        points of a class are evaluated (compact, evaluate, scatter back)."""
        ax = [torch.from_numpy(a.astype(np.float32)).to(device) for a in xyz]
        nx, ny, nz = (len(a) for a in xyz)
        classes = self.point_classes(views, device, lattice=ax)
        flat = torch.full((nx * ny * nz,), -100.0, dtype=torch.float32, device=device)
        coarse_bound = self.renderer._coarse_bound(decoders)
        for cls, stage, offset in ((1, 'fine', None), (2, 'coarse', 0.2)):
            for lin in torch.split(torch.nonzero(classes == cls).reshape(-1), self.points_batch_size):
                if lin.numel() == 0:
                    continue
                pts = torch.stack([ax[0][lin // (ny * nz)], ax[1][(lin // nz) % ny], ax[2][lin % nz]], 1)
                occ = EF.eval_points(pts, decoders, c, stage, self.bound, apply_mask=True, coarse_bound=coarse_bound)[:, 3]
                flat[lin] = occ if offset is None else occ + offset
        return flat.view(nx, ny, nz), classes

    # ------------------------------------------------------------------ the mesh
    def get_mesh(self, mesh_out_file, c, decoders, keyframe_dict, estimate_c2w_list, idx, device='cuda:0', show_forecast=False,
                 color=True, clean_mesh=True, get_mask_use_all_frames=False):
        """Extract the mesh of the map, write it to mesh_out_file (binary PLY: float xyz, uchar rgb, int faces) and return
        (vertices float64 [V,3], faces int32 [F,3], colours uint8 [V,3] or None); None when no surface is found (the
        reference prints a message and returns there as well)."""
        import time
        if show_forecast and torch.device(device).type != 'cuda':
            raise NotImplementedError("show_forecast (mesh_coarse_level) needs a HIP device (csrc/visibility.hip)")
        if color and self.color_mesh_extraction_method != 'direct_point_query':
            raise NotImplementedError(f"color_mesh_extraction_method {self.color_mesh_extraction_method!r} belongs to iMAP; "
                                      "the HIP path implements direct_point_query")
        timing = self.timing
        timing.clear()

        def lap(name, t0):
            torch.cuda.synchronize(device)
            timing[name] = time.perf_counter() - t0
            return time.perf_counter()

        with torch.no_grad():
            t0 = time.perf_counter()
            xyz = self.get_grid_uniform(self.resolution)['xyz']
            views = self._views(keyframe_dict, estimate_c2w_list, idx, device, get_mask_use_all_frames) if show_forecast else None
            halfspaces = self.get_bound_from_frames(keyframe_dict, self.scale, device) if clean_mesh or not show_forecast else None
            t0 = lap('hull', t0)
            if show_forecast:
                vol, _ = self.forecast_volume(c, decoders, xyz, views, device)
            else:
                vol = self.lattice_volume(c, decoders, xyz, halfspaces, device)
            t0 = lap('lattice', t0)
            verts, faces = EF.marching_cubes(vol, self.level_set, [a[0] for a in xyz],
                                             [a[2] - a[1] for a in xyz])
            del vol
            t0 = lap('marching_cubes', t0)
            if faces.shape[0] == 0:
                print('marching_cubes error. Possibly no surface extracted from the level set.')
                return None
            on_device = clean_mesh and torch.device(device).type == 'cuda' and not self.clean_on_host
            if on_device:
                return self._finish_on_device(mesh_out_file, verts, faces, halfspaces, c, decoders, keyframe_dict, estimate_c2w_list,
                                              idx, device, show_forecast, color, get_mask_use_all_frames, lap, t0)
            vertices, faces = verts.cpu().numpy(), faces.cpu().numpy()

            if clean_mesh:
                t1 = time.perf_counter()
                if show_forecast:                       # Mesher.py:472-486: faces with a vertex inside the keyframes' hull stay
                    hs = torch.from_numpy(halfspaces).to(device)
                    keep = torch.cat([inside_halfspaces(p, hs) for p in torch.split(verts, self.points_batch_size)]).cpu().numpy()
                else:
                    keep, _, _ = self.point_masks(vertices, keyframe_dict, estimate_c2w_list, idx, device=device,
                                                  get_mask_use_all_frames=get_mask_use_all_frames)
                faces = faces[~(~keep)[faces].all(axis=1)]
                if torch.device(device).type == 'cuda':
                    torch.cuda.synchronize(device)
                timing['clean_masks'] = time.perf_counter() - t1
                t1 = time.perf_counter()
                faces = filter_components(vertices, faces, self.remove_small_geometry_threshold * self.scale * self.scale,
                                          self.get_largest_components)
                vertices, faces = drop_unreferenced(vertices, faces)
                timing['clean_components'] = time.perf_counter() - t1
            t0 = lap('clean', t0)

            vertex_colors = None
            if color:
                pts = torch.from_numpy(vertices).to(device).float()
                z = np.zeros((0, 3), np.float32)
                if pts.shape[0]:
                    z = torch.cat([EF.eval_points(p, decoders, c, 'color', self.bound, apply_mask=True)[:, :3]
                                   for p in torch.split(pts, self.points_batch_size)]).cpu().numpy()
                vertex_colors = (np.clip(z, 0, 1) * 255).astype(np.uint8)
                if show_forecast:                       # Mesher.py:556-563: cyan for the forecast region
                    _, forecast, _ = self.point_masks(vertices, keyframe_dict, estimate_c2w_list, idx, device=device,
                                                      get_mask_use_all_frames=get_mask_use_all_frames)
                    vertex_colors[forecast] = (0, 255, 255)
            t0 = lap('color', t0)

            vertices = vertices / self.scale
            write_ply(mesh_out_file, vertices, faces, vertex_colors)
            lap('write', t0)
            if self.verbose:
                print('Saved mesh at', mesh_out_file)
            return vertices, faces, vertex_colors

    def _finish_on_device(self, mesh_out_file, verts, faces, halfspaces, c, decoders, keyframe_dict, estimate_c2w_list, idx, device,
                          show_forecast, color, get_mask_use_all_frames, lap, t0):
        """get_mesh from the marching-cubes output on, with clean_mesh, on a HIP device: the vertex mask, the component filter
        and the compaction (functional.mesh_clean), the colour query and the forecast classes stay on the device; vertices,
        faces, colours and the forecast mask are downloaded once, before the file is written.  Every array and the file are
        bit-identical to the host route's (clean_on_host = True): the same float32 roundings of the same float64 vertices,
        the same chunks, the same kept faces and vertices in the same order."""
        import time
        timing = self.timing
        t1 = time.perf_counter()
        if show_forecast:                               # Mesher.py:472-486: faces with a vertex inside the keyframes' hull stay
            hs = torch.from_numpy(halfspaces).to(device)
            keep = torch.cat([inside_halfspaces(p, hs) for p in torch.split(verts, self.points_batch_size)])
        else:
            views = self._views(keyframe_dict, estimate_c2w_list, idx, device, get_mask_use_all_frames)
            keep = self.point_classes(views, device, points=verts) == 1
        torch.cuda.synchronize(device)
        timing['clean_masks'] = time.perf_counter() - t1
        t1 = time.perf_counter()
        stats = {}
        verts, faces, _ = EF.mesh_clean(verts, faces, keep, self.remove_small_geometry_threshold * self.scale * self.scale,
                                        self.get_largest_components, stats=stats)
        torch.cuda.synchronize(device)
        timing['clean_components'] = time.perf_counter() - t1
        self.clean_stats = dict(components=stats['components'], vertices=int(verts.shape[0]), faces=int(faces.shape[0]))
        t0 = lap('clean', t0)

        z = forecast = None
        if color:
            pts = verts.float()
            z = torch.zeros((0, 3), dtype=torch.float32, device=device)
            if pts.shape[0]:
                z = torch.cat([EF.eval_points(p, decoders, c, 'color', self.bound, apply_mask=True)[:, :3]
                               for p in torch.split(pts, self.points_batch_size)])
            if show_forecast:                           # Mesher.py:556-563: cyan for the forecast region
                views = self._views(keyframe_dict, estimate_c2w_list, idx, device, get_mask_use_all_frames)
                forecast = self.point_classes(views, device, points=verts) == 2
        vertices, faces = verts.cpu().numpy(), faces.cpu().numpy()
        vertex_colors = None
        if color:
            vertex_colors = (np.clip(z.cpu().numpy(), 0, 1) * 255).astype(np.uint8)
            if forecast is not None:
                vertex_colors[forecast.cpu().numpy()] = (0, 255, 255)
        t0 = lap('color', t0)

        vertices = vertices / self.scale
        write_ply(mesh_out_file, vertices, faces, vertex_colors)
        lap('write', t0)
        if self.verbose:
            print('Saved mesh at', mesh_out_file)
        return vertices, faces, vertex_colors


# ---------------------------------------------------------------------------------------------------------------------
# helpers (host side, numpy / scipy; tests/test_mesher_cpu.py checks each on a hand-built case)
# ---------------------------------------------------------------------------------------------------------------------
def backprojected_points(keyframe_dict, H, W, fx, fy, cx, cy):
    """float64 [P,3]: per keyframe the convex-hull vertices of its valid depth pixels back-projected with est_c2w (pixel
    (i, j) -> depth * [(i - cx) / fx, -(j - cy) / fy, -1], the reference's camera axes), and its camera centre."""
    from scipy.spatial import ConvexHull
    out = []
    for kf in keyframe_dict:
        c2w = kf['est_c2w'].detach().cpu().numpy().astype(np.float64)
        depth = kf['depth'].detach().cpu().numpy().astype(np.float64).reshape(H, W)
        j, i = np.nonzero(depth > 0)
        d = depth[j, i]
        cam = np.stack([(i - cx) / fx * d, -(j - cy) / fy * d, -d], 1)
        world = cam @ c2w[:3, :3].T + c2w[:3, 3]
        if world.shape[0] >= 4:
            try:
                world = world[ConvexHull(world).vertices]
            except Exception:       # degenerate (planar) view: keep its points
                pass
        out.append(world)
        out.append(c2w[None, :3, 3])
    return np.concatenate(out, 0)


def hull_halfspaces(points, scale):
    """[K,4] half-spaces of the convex hull of points, scaled by `scale` about the mean of the hull's vertices."""
    from scipy.spatial import ConvexHull
    v = points[ConvexHull(points).vertices]
    center = v.mean(axis=0)
    return ConvexHull((v - center) * scale + center).equations.astype(np.float64)


_HULL_DIRECTIONS = []


def hull_directions():
    """float64 numpy [70,3]: the fixed unit directions of hull_candidates -- 64 seeded Gaussian directions and +- the axes."""
    if not _HULL_DIRECTIONS:
        d = np.random.default_rng(0).standard_normal((64, 3))
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        _HULL_DIRECTIONS.append(np.concatenate([d, np.eye(3), -np.eye(3)]))
    return _HULL_DIRECTIONS[0]


def hull_candidates(points):
    """The points (float64 [P,3], tensor on either device, or numpy) that can be vertices of their convex hull, as a tensor on the
    points' device: the extreme points along 70 fixed directions span an inner hull (scipy, on <= 70 points); every point
    deeper than a relative 1e-9 inside all of its half-spaces (inside_halfspaces' arithmetic) is dropped.  A vertex of the hull
    of all points is never strictly inside the hull of some of them, so ConvexHull(survivors) has the vertex set of
    ConvexHull(points) at a fraction of its cost.  A degenerate extreme set (scipy raises) returns all points."""
    from scipy.spatial import ConvexHull
    p = (torch.from_numpy(np.asarray(points)) if not torch.is_tensor(points) else points).double()
    if p.shape[0] < 5:
        return p
    dirs = torch.from_numpy(hull_directions()).to(p.device)
    extreme = torch.unique(torch.argmax(p @ dirs.T, dim=0))
    try:
        hs = ConvexHull(p[extreme].cpu().numpy()).equations.astype(np.float64)
    except Exception:               # degenerate (planar) set: keep the points
        return p
    eps = 1e-9 * float((p.max(0).values - p.min(0).values).max())
    hs[:, 3] += eps                 # n . x + d + eps <= 0: deeper than eps inside this half-space
    return p[~inside_halfspaces(p, torch.from_numpy(hs).to(p.device))]


def inside_halfspaces(points, halfspaces, block=32):
    """bool [P]: points (device, [P,3]) on the inner side of every half-space (n . x + d <= 0), in float64."""
    p = points.double()
    inside = torch.ones(p.shape[0], dtype=torch.bool, device=p.device)
    for k in range(0, halfspaces.shape[0], block):
        h = halfspaces[k:k + block]
        inside &= ((p @ h[:, :3].T + h[:, 3]) <= 0).all(dim=1)
    return inside


def face_components(faces):
    """Label per face of its edge-connected component (faces sharing an edge are connected) and the component count."""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    f = np.asarray(faces, dtype=np.int64)
    F = f.shape[0]
    if F == 0:
        return np.zeros(0, np.int64), 0
    e = np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), axis=1)
    _, edge_id = np.unique(e, axis=0, return_inverse=True)
    edge_id = edge_id.reshape(-1)
    E = int(edge_id.max()) + 1
    rows = np.tile(np.arange(F), 3)
    g = coo_matrix((np.ones(3 * F, np.int8), (rows, F + edge_id)), shape=(F + E, F + E))
    n, labels = connected_components(g, directed=False)
    lab = labels[:F]
    _, lab = np.unique(lab, return_inverse=True)
    return lab.reshape(-1), int(lab.max()) + 1


def face_areas(vertices, faces):
    v = np.asarray(vertices, dtype=np.float64)[np.asarray(faces, dtype=np.int64)]
    return 0.5 * np.linalg.norm(np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]), axis=1)


def filter_components(vertices, faces, min_area, largest_only=False):
    """Faces of the components whose area exceeds min_area, or of the largest one (Mesher.py:530-541)."""
    lab, n = face_components(faces)
    if n == 0:
        return faces
    area = np.bincount(lab, weights=face_areas(vertices, faces), minlength=n)
    keep = np.zeros(n, bool)
    if largest_only:
        keep[int(np.argmax(area))] = True
    else:
        keep = area > min_area
    return faces[keep[lab]]


def drop_unreferenced(vertices, faces):
    """(vertices, faces) without the vertices no face uses; the rest keep their order."""
    used = np.zeros(len(vertices), bool)
    used[np.asarray(faces, dtype=np.int64).reshape(-1)] = True
    remap = np.cumsum(used) - 1
    return vertices[used], remap[faces].astype(np.int32)


def write_ply(path, vertices, faces, colors=None):
    """Binary little-endian PLY: float32 x y z (+ uchar red green blue), faces as uchar-counted int32 index lists."""
    V, F = len(vertices), len(faces)
    vt = [('x', '<f4'), ('y', '<f4'), ('z', '<f4')]
    if colors is not None:
        vt += [('red', 'u1'), ('green', 'u1'), ('blue', 'u1')]
    vrec = np.empty(V, dtype=vt)
    v = np.asarray(vertices)
    vrec['x'], vrec['y'], vrec['z'] = v[:, 0], v[:, 1], v[:, 2]
    if colors is not None:
        c = np.asarray(colors, dtype=np.uint8)
        vrec['red'], vrec['green'], vrec['blue'] = c[:, 0], c[:, 1], c[:, 2]
    frec = np.empty(F, dtype=[('n', 'u1'), ('i', '<i4', (3,))])
    frec['n'] = 3
    frec['i'] = np.asarray(faces)
    head = ["ply", "format binary_little_endian 1.0", f"element vertex {V}", "property float x", "property float y",
            "property float z"]
    if colors is not None:
        head += ["property uchar red", "property uchar green", "property uchar blue"]
    head += [f"element face {F}", "property list uchar int vertex_indices", "end_header"]
    with open(path, "wb") as fh:
        fh.write(("\n".join(head) + "\n").encode("ascii"))
        fh.write(vrec.tobytes())
        fh.write(frec.tobytes())


def read_ply(path):
    """(vertices float32 [V,3], faces int32 [F,3], colours uint8 [V,3] or None) of a file written by write_ply."""
    with open(path, "rb") as fh:
        data = fh.read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    head = data[:end].decode("ascii").split("\n")
    V = int(next(h for h in head if h.startswith("element vertex")).split()[-1])
    F = int(next(h for h in head if h.startswith("element face")).split()[-1])
    has_color = "property uchar red" in head
    vt = [('x', '<f4'), ('y', '<f4'), ('z', '<f4')] + ([('red', 'u1'), ('green', 'u1'), ('blue', 'u1')] if has_color else [])
    vrec = np.frombuffer(data, dtype=vt, count=V, offset=end)
    frec = np.frombuffer(data, dtype=[('n', 'u1'), ('i', '<i4', (3,))], count=F, offset=end + vrec.nbytes)
    if F and not (frec['n'] == 3).all():
        raise ValueError("read_ply reads triangle meshes only")
    verts = np.stack([vrec['x'], vrec['y'], vrec['z']], 1)
    colors = np.stack([vrec['red'], vrec['green'], vrec['blue']], 1) if has_color else None
    return verts, frec['i'].astype(np.int32), colors
