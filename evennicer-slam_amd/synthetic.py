"""Analytic, view-consistent RGB-D scenes (no dataset ships with the image): an axis-aligned room seen from inside with one
box standing in it.  Depth and colour of every pixel follow from ray / box intersections, so the frames of a camera
trajectory are renderings of ONE fixed geometry -- what the run harness needs to show that tracking converges
and what `bench.py` uses for its second scene variant (a map with real surfaces instead of random-init occupancy).

Conventions are the reference's: pixel (i, j) -> direction [(i - cx) / fx, -(j - cy) / fy, -1] rotated by c2w[:3, :3]
(src/common.py:74-89); `depth` is the ray parameter of that un-normalised direction, i.e. the z-buffer depth the datasets
store (src/utils/datasets.py:107-113)."""
import math

import numpy as np
import torch


class BoxRoom:
    """Room = inside of the box [room_lo, room_hi]; one solid box [box_lo, box_hi] in it.  Colour is a smooth function of the
    3-D hit point (three sinusoids per channel), so it is consistent across views and learnable by the colour grid."""

    def __init__(self, room_lo, room_hi, box_lo=None, box_hi=None, seed=0):
        self.room_lo = torch.tensor(room_lo, dtype=torch.float64)
        self.room_hi = torch.tensor(room_hi, dtype=torch.float64)
        self.box_lo = torch.tensor(box_lo, dtype=torch.float64) if box_lo is not None else None
        self.box_hi = torch.tensor(box_hi, dtype=torch.float64) if box_hi is not None else None
        g = torch.Generator().manual_seed(seed)
        self.freq = (torch.rand(3, 3, generator=g, dtype=torch.float64) * 1.6 + 0.8)       # rad / m, per channel and axis
        self.phase = torch.rand(3, generator=g, dtype=torch.float64) * 2 * math.pi

    @staticmethod
    def for_bound(bound, margin=0.7, seed=0):
        """A room `margin` metres inside a scene bound [3,2] with a box on its floor (z is up in none of the reference's
        scenes in particular; the box simply sits against the low-y wall)."""
        b = torch.as_tensor(bound, dtype=torch.float64)
        lo, hi = b[:, 0] + margin, b[:, 1] - margin
        ext = hi - lo
        box_lo = lo + ext * torch.tensor([0.55, 0.0, 0.25], dtype=torch.float64)
        box_hi = lo + ext * torch.tensor([0.75, 0.35, 0.55], dtype=torch.float64)
        return BoxRoom(lo.tolist(), hi.tolist(), box_lo.tolist(), box_hi.tolist(), seed=seed)

    def intersect(self, rays_o, rays_d):
        """Ray parameter t >= 0 of the first surface hit (float64 [N]) for origins inside the room."""
        o, d = rays_o.double(), rays_d.double()
        dev = o.device
        d = torch.where(d.abs() < 1e-12, torch.full_like(d, 1e-12), d)
        lo, hi = self.room_lo.to(dev), self.room_hi.to(dev)
        t_wall = torch.maximum((lo - o) / d, (hi - o) / d).min(dim=-1).values
        if self.box_lo is None:
            return t_wall
        blo, bhi = self.box_lo.to(dev), self.box_hi.to(dev)
        ta, tb = (blo - o) / d, (bhi - o) / d
        t1 = torch.minimum(ta, tb).max(dim=-1).values
        t2 = torch.maximum(ta, tb).min(dim=-1).values
        hit = (t1 < t2) & (t1 > 0)
        return torch.where(hit & (t1 < t_wall), t1, t_wall)

    def sample_surface(self, n, seed=0):
        """n points (float64 [n,3]) spread uniformly by area over the surfaces a camera inside the room can see: the room's
        six walls without the patches the box covers, and the box's faces without those lying on a wall (the ground truth
        of eval_recon's metrics)."""
        g = torch.Generator().manual_seed(seed)
        boxes = [(self.room_lo, self.room_hi)] + ([(self.box_lo, self.box_hi)] if self.box_lo is not None else [])
        faces = []                                          # (box, axis, side, area)
        for b, (lo, hi) in enumerate(boxes):
            ext = hi - lo
            for a in range(3):
                for side in (0, 1):
                    faces.append((b, a, side, float(ext[(a + 1) % 3] * ext[(a + 2) % 3])))
        area = torch.tensor([f[3] for f in faces], dtype=torch.float64)
        out, have = [], 0
        while have < n:
            m = 2 * (n - have) + 64
            pick = torch.multinomial(area, m, replacement=True, generator=g)
            u = torch.rand(m, 3, generator=g, dtype=torch.float64)
            p = torch.empty(m, 3, dtype=torch.float64)
            for k, (b, a, side, _) in enumerate(faces):
                sel = pick == k
                lo, hi = boxes[b]
                q = lo + u[sel] * (hi - lo)
                q[:, a] = hi[a] if side else lo[a]
                p[sel] = q
            keep = torch.ones(m, dtype=torch.bool)
            if self.box_lo is not None:
                on_box = pick >= 6
                covered = ((p >= self.box_lo) & (p <= self.box_hi)).all(dim=1)
                on_wall = ((p == self.room_lo) | (p == self.room_hi)).any(dim=1)
                keep = torch.where(on_box, ~on_wall, ~covered)
            out.append(p[keep])
            have += int(keep.sum())
        return torch.cat(out)[:n]

    def color_at(self, pts):
        p = pts.double()
        dev = p.device
        return 0.5 + 0.45 * torch.sin(p @ self.freq.to(dev).T + self.phase.to(dev))

    def render(self, c2w, cam, device='cpu'):
        """(color float64 [H,W,3] in [0.05, 0.95], depth float32 [H,W]) of the view c2w ([3|4,4])."""
        H, W, fx, fy, cx, cy = (cam[k] for k in ('H', 'W', 'fx', 'fy', 'cx', 'cy'))
        c2w = torch.as_tensor(c2w, dtype=torch.float64, device=device)
        j, i = torch.meshgrid(torch.arange(H, dtype=torch.float64, device=device),
                              torch.arange(W, dtype=torch.float64, device=device), indexing='ij')
        dirs = torch.stack([(i - cx) / fx, -(j - cy) / fy, -torch.ones_like(i)], -1).reshape(-1, 3)
        rays_d = dirs @ c2w[:3, :3].T
        rays_o = c2w[:3, 3].expand_as(rays_d)
        t = self.intersect(rays_o, rays_d)
        pts = rays_o + rays_d * t[:, None]
        return self.color_at(pts).reshape(H, W, 3), t.float().reshape(H, W)


def look_at(eye, target, up=(0., 0., 1.)):
    """c2w float64 [4,4] of a camera at `eye` looking at `target` in the reference's axes (camera looks along -z, y up)."""
    eye, target, up = (np.asarray(v, dtype=np.float64) for v in (eye, target, up))
    f = target - eye
    f /= np.linalg.norm(f)
    r = np.cross(f, up)
    r /= np.linalg.norm(r)
    u = np.cross(r, f)
    c2w = np.eye(4)
    c2w[:3, 0], c2w[:3, 1], c2w[:3, 2], c2w[:3, 3] = r, u, -f, eye
    return torch.from_numpy(c2w)


def trajectory(room, n_frames, step=0.02, yaw_deg=0.4):
    """n_frames camera-to-world poses (float32 [4,4]) on a gentle arc inside the room: `step` metres and `yaw_deg` degrees of
    change in the viewing direction per frame, looking towards the box side of the room."""
    lo, hi = room.room_lo.numpy(), room.room_hi.numpy()
    c = 0.5 * (lo + hi)
    ext = hi - lo
    start = c - ext * np.array([0.25, 0.10, 0.05])
    poses = []
    for k in range(n_frames):
        a = math.radians(yaw_deg) * k
        eye = start + step * k * np.array([math.cos(0.3), math.sin(0.3), 0.15])
        tgt = c + ext * np.array([0.20 * math.cos(a) + 0.10, -0.25 + 0.20 * math.sin(a), 0.02 * math.sin(2 * a)])
        poses.append(look_at(eye, tgt).float())
    return poses


def demo_config(inp, evf, cam, device='cuda:0', env=None):
    """Configuration of the run harness for the tiny analytic room of `write_demo_sequence` (the reference's schedule and
    learning rates, configs/nice_slam.yaml, at a size that runs in seconds; environment-style overrides through `env`).
    One deliberate difference: lr_first_factor is 1, not 5 -- the decoders here are fitted to a handful of frames
    (SLAM.prefit_decoders), not ConvONet-pretrained, and a middle-grid learning rate of 0.5 on frame 0 left the map at its
    initial loss in about half of the runs (measured: tools/run_synthetic_slam.py, LR_FIRST=5)."""
    env = env or {}
    stage = {'coarse': dict(decoders_lr=0.0, coarse_lr=0.001, middle_lr=0.0, fine_lr=0.0, color_lr=0.0),
             'middle': dict(decoders_lr=0.0, coarse_lr=0.0, middle_lr=0.1, fine_lr=0.0, color_lr=0.0),
             'fine': dict(decoders_lr=0.0, coarse_lr=0.0, middle_lr=0.005, fine_lr=0.005, color_lr=0.0),
             'color': dict(decoders_lr=0.005, coarse_lr=0.0, middle_lr=0.005, fine_lr=0.005, color_lr=0.005)}
    return {
        'dataset': 'replica_event', 'scale': 1, 'occupancy': True, 'coarse': True, 'data': {'dim': 3, 'input_folder': inp, 'event_folder': evf},
        'rendering': {'lindisp': False, 'perturb': 0.0, 'N_samples': 32, 'N_surface': 16, 'N_importance': 0},
        'model': {'c_dim': 32, 'coarse_bound_enlarge': 2, 'pos_embedding_method': 'fourier'},
        'grid_len': {'coarse': 0.8, 'middle': 0.32, 'fine': 0.16, 'color': 0.16, 'bound_divisible': 0.32},
        'cam': dict(cam, png_depth_scale=6553.5, crop_edge=0),
        'mapping': {'bound': [[-1.0, 1.1], [-0.9, 0.8], [-0.7, 0.6]], 'w_color_loss': 0.2, 'lr_factor': 1, 'lr_first_factor': float(env.get('LR_FIRST', 1)),
                    'BA': False, 'BA_cam_lr': 0.001, 'middle_iter_ratio': 0.4, 'fine_iter_ratio': 0.6, 'fix_fine': True,
                    'fix_color': False, 'pixels': int(env.get('MAP_PIXELS', 600)), 'iters_first': int(env.get('ITERS_FIRST', 400)),
                    'iters': int(env.get('MAP_ITERS', 30)), 'every_frame': int(env.get('EVERY', 2)), 'keyframe_every': 6,
                    'mapping_window_size': 5, 'frustum_feature_selection': True, 'stage': stage},
        'tracking': {'device': device, 'w_color_loss': 0.5, 'ignore_edge_W': 4, 'ignore_edge_H': 4, 'handle_dynamic': True,
                     'use_color_in_tracking': True, 'lr': float(env.get('TRACK_LR', 0.002)), 'pixels': int(env.get('TRACK_PIXELS', 1000)),
                     'iters': int(env.get('TRACK_ITERS', 40)), 'const_speed_assumption': True, 'gt_camera': False,
                     'graphed': bool(int(env.get('TRACK_GRAPHED', 0)))},
        'event': {'activate_events': False, 'blur': True, 'kernel_sizes': [9], 'kernel_weights': [1], 'unblurred_weight': 0,
                  'balancer': 0.025, 'scale_factor': 0.5},
    }


def write_demo_sequence(root, n, cam, step=0.012, yaw_deg=0.5, events=None, sim=None, stamps=None, streams=None, noise=None):
    """n frames of a BoxRoom inside the demo bound along `trajectory`, written in the Replica_event layout.
    events: None writes all-zero event images; 'simulate' fills them from `event_sim.EventSimulator.step_scene` along the
    trajectory with `sim` (default: a simulator with default parameters on the CPU, its numpy route; pass one on a HIP device
    to run the kernel, which then renders the frames as well -- one launch per frame).
    stamps (n frame times) with events = 'simulate': the intervals are simulated with time stamps and the list `streams`
    receives one event_stream.EventStream per interval (pixel-major); the frames then come from BoxRoom.render.
    noise (an event_sim.EventNoise) with events = 'simulate': the default simulator is built with it (a `sim` passed in
    carries its own); the noisy sensor needs `stamps`.
    Returns ((input_folder, event_folder), poses)."""
    from . import datasets as D
    from .scene import scene_bound
    if events not in (None, 'simulate'):
        raise ValueError(f"write_demo_sequence: events must be None or 'simulate' (got {events!r})")
    bound = scene_bound([[-1.0, 1.1], [-0.9, 0.8], [-0.7, 0.6]], 1.0, 0.32)
    room = BoxRoom.for_bound(bound, margin=0.12, seed=1)
    poses = trajectory(room, n, step=step, yaw_deg=yaw_deg)
    if events == 'simulate' and sim is None:
        from .event_sim import EventSimulator
        sim = EventSimulator(cam['H'], cam['W'], device='cpu', noise=noise)
    if events == 'simulate' and sim.noise is not None and stamps is None:
        raise ValueError("write_demo_sequence: a simulator with noise needs the frame times `stamps`")
    frames, evs = [], []
    for i, c2w in enumerate(poses):
        if events is None:
            col, dep = room.render(c2w.double(), cam)
            if i > 0:
                evs.append(np.zeros((cam['H'], cam['W'], 2), dtype=np.uint8))
        elif i == 0:
            col, dep = room.render(c2w.double(), cam)
            sim.reset((room, c2w.double(), cam))
        elif stamps is not None:
            col, dep = room.render(c2w.double(), cam)
            if streams is None and sim.noise is not None:           # the noisy sensor, images only: its one-launch form
                ev = sim.step_scene(room, poses[i - 1].double(), c2w.double(), cam, stamps=(stamps[i - 1], stamps[i]), stream=False)
            else:
                ev, stream = sim.step_scene(room, poses[i - 1].double(), c2w.double(), cam, stamps=(stamps[i - 1], stamps[i]))
                if streams is not None:
                    streams.append(stream)
            evs.append(ev.cpu().numpy())
        elif sim.on_device:
            ev, col, dep = sim.step_scene(room, poses[i - 1].double(), c2w.double(), cam, want_frame=True)
            evs.append(ev.cpu().numpy())
        else:
            col, dep = room.render(c2w.double(), cam)
            evs.append(sim.step_scene(room, poses[i - 1].double(), c2w.double(), cam).numpy())
        frames.append((col.cpu().numpy(), dep.cpu().numpy()))
    return D.write_replica_event_sequence(root, frames, [p.numpy() for p in poses], 6553.5, evs), poses
