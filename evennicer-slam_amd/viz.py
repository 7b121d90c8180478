"""The reference's SLAM visualiser (src/tools/viz.py) without a window: the same SLAMFrontend surface, but instead of an
Open3D process that draws into a 1080 x 1920 window, `render()` rasterises the current scene on the device
(functional.scene_raster, csrc/scene_raster.hip) and returns the frame -- and writes it as a JPEG with save_rendering.

What is kept of the reference: the camera frustum actor (12 segments x 100 samples, red for the estimate, black for the
ground truth), the viewer's pose (two units behind the first estimated pose), Open3D's default pinhole camera of that window
(60 degree vertical field of view), point size 4, z_near = `near`, z_far = 1000, hidden back faces after the reversal of
every triangle (culling 1 of the rasteriser: derived from the reference's code, not checked against Open3D itself), the
in-place negation of a pose's third column in update_pose, the key i + 100000 of ground-truth actors and the trajectory
actor [1:i].  What differs: an actor's points are its frustum under the latest pose, not the product of every pose change
since it was made; the shading is ambient + (1 - ambient) |n . d|, not Open3D's Phong lights; there is no process."""
import math
import os
import shutil

import numpy as np

GT_KEY_OFFSET = 100000
POINT_SIZE = 4
Z_FAR = 1000.0
_CAM_POINTS = np.array([[0, 0, 0], [-1, -1, 1.5], [1, -1, 1.5], [1, 1, 1.5], [-1, 1, 1.5], [-0.5, 1, 1.5], [0.5, 1, 1.5],
                        [0, 1.2, 1.5]], np.float64)
_CAM_LINES = ((1, 2), (2, 3), (3, 4), (4, 1), (1, 3), (2, 4), (1, 0), (0, 2), (3, 0), (0, 4), (5, 7), (7, 6))
RED, BLACK = (255, 0, 0), (0, 0, 0)


def camera_actor(is_gt=False, scale=0.005):
    """(points float64 [1200,3], colour (r, g, b) in 0..255) of create_camera_actor: 100 samples, linspace(0, 1, 100), on each
    of the 12 segments of the 8-point frustum; black for the ground truth, red for the estimate"""
    pts = scale * _CAM_POINTS
    t = np.linspace(0., 1., 100)
    seg = [pts[a][None, :] * (1. - t)[:, None] + pts[b][None, :] * t[:, None] for a, b in _CAM_LINES]
    return np.concatenate(seg), (BLACK if is_gt else RED)


def viewer_pose(init_c2w):
    """float64 [4,4]: the viewer's camera-to-world matrix, the first estimated pose moved 2 units along its own +z (backwards:
    the camera looks down -z) -- what draw_trajectory sets up before it flips the y and z columns for Open3D and inverts"""
    pose = np.array(init_c2w, np.float64)
    z = pose[:3, 2]
    pose[:3, 3] += 2 * (z / np.linalg.norm(z))
    return pose


def default_intrinsics(H=1080, W=1920):
    """Open3D's default pinhole camera of an H x W window: 60 degree vertical field of view, the principal point at the centre
    of the pixel grid"""
    f = (H / 2.0) / math.tan(math.radians(30.0))
    return dict(H=int(H), W=int(W), fx=f, fy=f, cx=W / 2.0 - 0.5, cy=H / 2.0 - 0.5)


class SLAMFrontend:
    def __init__(self, output, init_pose, cam_scale=1, save_rendering=False, near=0, estimate_c2w_list=None, gt_c2w_list=None,
                 H=1080, W=1920, device='cuda:0'):
        self.output, self.cam_scale, self.save_rendering, self.device = output, cam_scale, save_rendering, device
        self.estimate_c2w_list, self.gt_c2w_list = estimate_c2w_list, gt_c2w_list
        self.cam = default_intrinsics(H, W)
        self.z_near, self.z_far = float(near), Z_FAR
        self.view_c2w = viewer_pose(init_pose)
        self.cameras = {}               # key -> (frustum points [1200,3], colour, pose)
        self.traj_actor = self.traj_actor_gt = None         # (points [n,3], colour)
        self.mesh = None                # (vertices, faces, colours or None, normals) on the device
        self.frame_idx = 0
        if save_rendering:
            shutil.rmtree(os.path.join(output, 'tmp_rendering'), ignore_errors=True)

    def update_pose(self, index, pose, gt=False):
        if hasattr(pose, 'cpu'):
            pose = pose.cpu().numpy()
        pose[:3, 2] *= -1               # in the caller's array, as the reference does
        key = index + GT_KEY_OFFSET if gt else index
        if key in self.cameras:
            base, colour, _ = self.cameras[key]
        else:
            base, colour = camera_actor(gt, self.cam_scale)
        self.cameras[key] = (base, colour, np.array(pose, np.float64))

    def update_mesh(self, path):
        import torch
        from . import eval_recon
        from . import functional as EF
        v, f, c = eval_recon.load_mesh(path)
        v = torch.from_numpy(np.ascontiguousarray(v, np.float64)).to(self.device)
        f = torch.from_numpy(np.ascontiguousarray(f, np.int32)).to(self.device)
        c = None if c is None else torch.from_numpy(np.ascontiguousarray(c, np.uint8)).to(self.device)
        self.mesh = (v, f, c, EF.vertex_normals(v, f))

    def update_cam_trajectory(self, c2w_list, gt):
        i = c2w_list                    # the reference's name for the frame index
        poses = self.gt_c2w_list if gt else self.estimate_c2w_list
        actor = (np.array(poses[1:i, :3, 3], np.float64), BLACK if gt else RED)
        if gt:
            self.traj_actor_gt = actor
        else:
            self.traj_actor = actor

    def reset(self):
        self.cameras = {}

    def start(self):
        return self

    def join(self):
        return None

    def scene_points(self):
        """(points float64 [P,3], colours uint8 [P,3]): the camera actors in the order they were made, then the estimated and
        the ground-truth trajectory"""
        pts, col = [], []
        for base, colour, pose in self.cameras.values():
            pts.append(base @ pose[:3, :3].T + pose[:3, 3])
            col.append(np.tile(np.array(colour, np.uint8), (len(base), 1)))
        for actor in (self.traj_actor, self.traj_actor_gt):
            if actor is not None:
                pts.append(actor[0])
                col.append(np.tile(np.array(actor[1], np.uint8), (len(actor[0]), 1)))
        if not pts:
            return np.zeros((0, 3)), np.zeros((0, 3), np.uint8)
        return np.concatenate(pts), np.concatenate(col)

    def render(self):
        """the current frame, uint8 [H,W,3] on the device; with save_rendering also output/tmp_rendering/{n:06d}.jpg"""
        import torch
        from . import functional as EF
        if self.mesh is None:
            v = torch.zeros((0, 3), dtype=torch.float64, device=self.device)
            f, c, n = torch.zeros((0, 3), dtype=torch.int32, device=self.device), None, None
        else:
            v, f, c, n = self.mesh
        pts, col = self.scene_points()
        pts, col = (torch.from_numpy(pts).to(self.device), torch.from_numpy(col).to(self.device)) if len(pts) else (None, None)
        w2c = np.linalg.inv(self.view_c2w)[None, :3]
        frame = EF.scene_raster(v, f, w2c, self.cam, colors=c, normals=n, points=pts, point_colors=col, point_size=POINT_SIZE,
                                cull=1, z_near=self.z_near, z_far=self.z_far)[0]
        if self.save_rendering:
            from PIL import Image
            self.frame_idx += 1
            folder = os.path.join(self.output, 'tmp_rendering')
            os.makedirs(folder, exist_ok=True)
            Image.fromarray(frame.cpu().numpy()).save(os.path.join(folder, f'{self.frame_idx:06d}.jpg'))
        return frame
