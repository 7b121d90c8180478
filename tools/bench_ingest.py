"""Frame preparation, host route against device route (datasets `prepare`), per frame, on synthetic sequences of three layouts:

    rpg      260x346 grey frames + events, the RPG lens model                       (datasets.RPG_event)
    tum      480x640 colour, the TUM lens model, crop_size [384,512], crop_edge 8   (datasets.TUM_RGBD)
    replica  680x1200 colour + events                                               (datasets.Replica_event)

    python tools/bench_ingest.py [--frames 12] [--shapes rpg,tum,replica] [--verbose]

For every frame after a warm-up pair the two routes alternate in one process, each timed from the call of `dataset[i]` to
a device synchronisation: image decoding (PIL), preparation and upload.  The decoders alone are timed on the same frame
right before (the files are in the page cache by then), so `*_prep_ms` = item - decode is what the route itself costs:
numpy / torch on the host and the upload of the prepared tensors, or the upload of the raw arrays and one kernel.
`kernel_ms` is that kernel alone between two device events on raw arrays that are already uploaded.  `launches` and
`uploads` are what the device route enqueues per frame (one enslam_frame_prepare launch; colour, depth and, after frame
0, events).  Every figure is the median [min, max] over the timed frames.  One JSON line on stdout; `device_below_host`
says whether the device route's SLOWEST frame is below the host route's FASTEST, on whole items."""
import argparse
import json
import os
import sys
import tempfile
import time
import types

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

RPG_DIST = [-0.08409333, 0.05335822, -0.00065521, -0.0001679, 0, 0, 0, 0]
TUM_DIST = [0.2624, -0.9531, -0.0054, 0.0026, 1.1633]
SHAPES = {
    'rpg': dict(dataset='rpg_event', cam=dict(H=260, W=346, fx=196.71854278974607, fy=196.68898128242577, cx=172.5, cy=129.5,
                                              png_depth_scale=1000.0, crop_edge=0, distortion=RPG_DIST)),
    'tum': dict(dataset='tumrgbd', cam=dict(H=480, W=640, fx=517.3, fy=516.5, cx=318.6, cy=255.3, png_depth_scale=5000.0,
                                            crop_edge=8, crop_size=[384, 512], distortion=TUM_DIST)),
    'replica': dict(dataset='replica_event', cam=dict(H=680, W=1200, fx=600.0, fy=600.0, cx=599.5, cy=339.5,
                                                      png_depth_scale=6553.5, crop_edge=0)),
}


def synthetic_frames(n, H, W, seed):
    """smooth textured colour (float [H,W,3]), depth (metres) and sparse events (uint8 [H,W,2]) that change from frame to frame"""
    rng = np.random.default_rng(seed)
    y, x = np.meshgrid(np.arange(H) / H, np.arange(W) / W, indexing='ij')
    frames, events = [], []
    for i in range(n):
        ph = rng.random(3) * 6.28
        color = np.stack([0.5 + 0.4 * np.sin(9 * x + 5 * y + ph[0] + 0.1 * i), 0.5 + 0.4 * np.sin(7 * y - 3 * x + ph[1]),
                          0.5 + 0.4 * np.sin(11 * x * y + ph[2])], -1) + 0.02 * rng.standard_normal((H, W, 3))
        depth = 1.5 + 0.8 * np.sin(3 * x + 0.05 * i) * np.cos(2 * y) + 0.002 * rng.standard_normal((H, W))
        frames.append((np.clip(color, 0, 1), depth))
        if i > 0:
            events.append((rng.random((H, W, 2)) < 0.08).astype(np.uint8) * rng.integers(1, 4, (H, W, 2)).astype(np.uint8))
    return frames, events


def write_sequence(name, root, n):
    from evennicer_slam_amd import datasets as D
    spec = SHAPES[name]
    cam = spec['cam']
    frames, events = synthetic_frames(n, cam['H'], cam['W'], seed=len(name))
    poses = [np.eye(4) for _ in range(n)]
    data = {}
    if name == 'rpg':
        grey = [(np.clip(np.rint(c.mean(-1) * 255), 0, 255).astype(np.uint8), d) for c, d in frames]
        data['input_folder'], data['event_folder'] = D.write_rpg_event_sequence(root, grey, poses, cam['png_depth_scale'], events)
    elif name == 'tum':
        # stamps 0.1 s apart: nothing is thinned or dropped
        data['input_folder'] = D.write_tum_sequence(root, frames, poses, cam['png_depth_scale'])
    else:
        data['input_folder'], data['event_folder'] = D.write_replica_event_sequence(root, frames, poses, cam['png_depth_scale'], events)
    return {'dataset': spec['dataset'], 'cam': cam, 'data': data}


def decode(ds, i):
    """the image decoding of item i alone, as the reader does it"""
    from PIL import Image
    from evennicer_slam_amd import datasets as D
    if isinstance(ds, D.RPG_event):
        with Image.open(ds.color_paths[i]) as im:
            np.array(im.convert('L'))
    else:
        D._imread_rgb(ds.color_paths[i])
    D._imread_depth(ds.depth_paths[i])
    if hasattr(ds, 'event_paths') and i >= 1:
        D._imread_rgb(ds.event_paths[i - 1])


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def kernel_ms(ds, i):
    """enslam_frame_prepare alone on uploaded raw arrays, by device events"""
    from evennicer_slam_amd import datasets as D
    from evennicer_slam_amd import functional as EF
    from PIL import Image
    dev = torch.device(ds.device)
    rpg = isinstance(ds, D.RPG_event)
    if rpg:
        with Image.open(ds.color_paths[i]) as im:
            color = np.array(im.convert('L'))
    else:
        color = D._imread_rgb(ds.color_paths[i])
    depth = D._imread_depth(ds.depth_paths[i])
    has_events = hasattr(ds, 'event_paths')
    event = D._imread_rgb(ds.event_paths[i - 1]) if has_events and i >= 1 else None
    raw = [EF._raw_image(color, dev, "colour", (torch.uint8,)), EF._raw_image(depth, dev, "depth", (torch.int16, torch.int32)),
           EF._raw_image(event, dev, "events", (torch.uint8,)) if event is not None else None]
    kw = dict(events=has_events, K=(ds.fx, ds.fy, ds.cx, ds.cy), distortion=ds.distortion, png_depth_scale=ds.png_depth_scale,
              scale=ds.scale, crop_size=ds.crop_size, crop_edge=ds.crop_edge, event_order='rpg' if rpg else 'replica',
              undistort_events=rpg)
    EF.frame_prepare(*raw, **kw)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    EF.frame_prepare(*raw, **kw)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def stats(v):
    return [round(float(np.median(v)), 3), round(float(np.min(v)), 3), round(float(np.max(v)), 3)]


def bench_shape(name, n, device, verbose=False):
    from evennicer_slam_amd import datasets as D
    with tempfile.TemporaryDirectory() as tmp:
        cfg = write_sequence(name, tmp, n)
        ds = D.get_dataset(cfg, types.SimpleNamespace(input_folder=None, event_folder=None), 1, device=device)
        assert len(ds) == n
        t = dict(decode=[], host=[], device=[], kernel=[])
        for i in range(n):
            dec, _ = timed(lambda: decode(ds, i))
            ds.prepare = 'host'
            host, item_h = timed(lambda: ds[i])
            ds.prepare = 'device'
            devt, item_d = timed(lambda: ds[i])
            if i < 2:                                               # the warm-up pair: frame 0 (no events) and frame 1
                assert float((item_h[1] - item_d[1]).abs().max()) <= 1e-14 and torch.equal(item_h[2], item_d[2])
                continue
            t['decode'].append(dec)
            t['host'].append(host)
            t['device'].append(devt)
            t['kernel'].append(kernel_ms(ds, i))
            if verbose:
                print(f"{name} frame {i}: decode {dec:.3f} host {host:.3f} device {devt:.3f} kernel {t['kernel'][-1]:.3f} ms",
                      file=sys.stderr, flush=True)
        out = {'frames_timed': len(t['host']), 'raw_hw': [cfg['cam']['H'], cfg['cam']['W']], 'out_hw': list(item_d[2].shape),
               'decode_ms': stats(t['decode']), 'host_item_ms': stats(t['host']), 'device_item_ms': stats(t['device']),
               'host_prep_ms': stats(np.array(t['host']) - np.array(t['decode'])),
               'device_prep_ms': stats(np.array(t['device']) - np.array(t['decode'])), 'kernel_ms': stats(t['kernel']),
               'launches': 1, 'uploads': 3 if hasattr(ds, 'event_paths') else 2,
               'device_below_host': bool(max(t['device']) < min(t['host']))}
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--frames', type=int, default=12)
    ap.add_argument('--shapes', default='rpg,tum,replica')
    ap.add_argument('--device', default='cuda:0')
    ap.add_argument('--verbose', action='store_true', help="every frame's times on stderr")
    args = ap.parse_args(argv)
    assert args.frames >= 12, "a warm-up pair and at least 10 timed frames"
    res = {'bench': 'ingest', 'device': torch.cuda.get_device_name(torch.device(args.device)), 'torch_threads': torch.get_num_threads(),
           'shapes': {name: bench_shape(name, args.frames, args.device, args.verbose) for name in args.shapes.split(',')}}
    print(json.dumps(res), flush=True)
    return res


if __name__ == '__main__':
    main()
