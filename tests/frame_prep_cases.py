"""Shared by the frame-preparation tests: the HOST route of datasets.py restated on raw arrays (the very functions the readers
call: datasets.undistort, datasets._resize_bilinear, BaseDataset._crop), camera constants and seeded raw images."""
import types

import numpy as np
import torch

# freiburg1 (TUM RGB-D) and the RPG camera of BASELINE config 5: intrinsics for 640x480 / 346x260, OpenCV distortion
TUM_K, TUM_DIST = (517.3, 516.5, 318.6, 255.3), [0.2624, -0.9531, -0.0054, 0.0026, 1.1633]
RPG_K, RPG_DIST = (196.71854278974607, 196.68898128242577, 172.5, 129.5), [-0.08409333, 0.05335822, -0.00065521, -0.0001679, 0, 0, 0, 0]
EVENT_CHANNELS = {'replica': [1, 2], 'rpg': [1, 0]}        # (-, +) of pngs (0, -, +) / (+, -, 0)
HO, WO = 37, 53                                            # no multiple of a wave or of the 64 x 4 tile in either axis


def scaled_K(K, factor):
    return tuple(v * factor for v in K)


def raw_color(shape, seed):
    return np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)


def raw_event(shape, seed):
    """uint8 [h,w,3], about half of the 6x6 blocks all zero (so that the mask keeps both values through the resamplings)"""
    rng = np.random.default_rng(seed)
    ev = rng.integers(0, 256, shape, dtype=np.uint8)
    blocks = rng.random(((shape[0] + 5) // 6, (shape[1] + 5) // 6)) < 0.5
    ev[np.kron(blocks, np.ones((6, 6), dtype=bool))[:shape[0], :shape[1]]] = 0
    return ev


def raw_depth(shape, seed, dtype=np.uint16):
    d = np.random.default_rng(seed).integers(0, 65536, shape).astype(dtype)
    d[0, 0], d[0, 1], d[-1, -1] = 0, 65535, 65535
    return d


def host_route(color, depth, event=None, events=False, K=None, distortion=None, png_depth_scale=1.0, scale=1.0, crop_size=None,
               crop_edge=0, event_order='replica', undistort_events=True):
    """(color float64, depth float32[, event, mask]) as numpy arrays, by the host route's own functions in its order."""
    from evennicer_slam_amd import datasets as D
    if color.ndim == 2:
        color = np.repeat(color[:, :, None], 3, axis=2)
    if distortion is not None:
        color = D.undistort(color, K, distortion)
        if event is not None and undistort_events:
            event = D.undistort(event, K, distortion)
    depth = depth.astype(np.float32) / png_depth_scale
    H, W = depth.shape
    color = torch.from_numpy(D._resize_bilinear(color / 255., (H, W)))
    depth = torch.from_numpy(depth) * scale
    want_events = events or event is not None
    ev = None
    if want_events:
        ev = torch.from_numpy(D._resize_bilinear(event, (H, W))) if event is not None else torch.zeros((H, W, 3), dtype=torch.uint8)
    color, depth, ev = D.BaseDataset._crop(types.SimpleNamespace(crop_size=crop_size, crop_edge=crop_edge), color, depth, ev)
    if not want_events:
        return color.numpy(), depth.numpy()
    ev = ev[:, :, EVENT_CHANNELS[event_order]]
    mask = torch.any(ev != 0, dim=-1) * 1
    return color.numpy(), depth.numpy(), ev.numpy(), mask.numpy()


def resize_before_rounding(img, size_hw):
    """the float64 values datasets._resize_bilinear rounds for a uint8 image"""
    import torch.nn.functional as F
    t = torch.from_numpy(np.ascontiguousarray(img)).double().permute(2, 0, 1)[None]
    return F.interpolate(t, size=size_hw, mode='bilinear', align_corners=False)[0].permute(1, 2, 0).numpy()
