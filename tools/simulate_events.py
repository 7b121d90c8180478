"""Simulate the event images of a sequence with the contrast-threshold sensor of evennicer_slam_amd.event_sim.

    python tools/simulate_events.py CONFIG [--default-config PATH] [--input_folder DIR] --out DIR
                                    [--layout replica_event|rpg_event] [--max-frames N] [--host-log]
    python tools/simulate_events.py --demo N --out DIR
    common: [--device cuda:0|cpu] [--c-pos C] [--c-neg C] [--sigma-c S] [--substeps K] [--eps E] [--seed N]
            [--stream OUT [--stamps FILE | --fps F]]
            [--refractory S] [--leak-rate HZ] [--shot-rate HZ] [--noise-seed N]

With a reference-format YAML chain (config.load_config; --input_folder overrides data.input_folder) the colour images of
any sequence the readers support are read RAW -- decoded, nothing else: grey for the rpg* layouts, RGB otherwise -- and the
events between consecutive images are written into --out as n - 1 pngs in the layout the `replica_event` reader
(event_frame%06d.png, channels (0, -, +)) or the `rpg_event` reader (event%06d.png, (+, -, 0)) expects; the default layout
follows the configuration's dataset.  Point `data.event_folder` (or --event_folder of the other tools) at --out afterwards.
--host-log takes the log intensities from the host, so that a device run equals a CPU run bit for bit on RGB images too.

--demo N writes the analytic room of synthetic.write_demo_sequence with simulated events (frames, depth, poses and events)
under --out; on a HIP device the kernel renders the frames as well.

--stream OUT also writes the simulated events with their time stamps (linear level-crossing interpolation inside each
sub-step, event_sim.py), sorted by time: OUT ending in .npz as event_stream.EventStream.save writes it, any other name as text,
one event per line `t x y p`.  The frame times come from --stamps (first field per non-comment line) or are i / --fps (30).
tools/events_to_frames.py bins such a stream back into event images, at any gap or density.

--refractory S, --leak-rate HZ, --shot-rate HZ (any of them above zero; --noise-seed N seeds the shot noise) switch to the
noisy sensor (event_sim.EventNoise): refractory period in seconds, leak events at HZ under constant light, shot-noise events at
HZ per pixel and polarity.  Its rates are in seconds, so the frame times are needed: the ones --stream uses (--stamps, or
i / --fps), with or without --stream (without it the one-launch image-only form runs).  The event images then count the
emitted events, and a stream written alongside bins back into exactly them (tools/events_to_frames.py) -- with one exception
under --leak-rate: a leak event of a pixel that does not change between two frames sits exactly on the start of a sub-step, at
the first sub-step on the frame time itself, and binning by frame times gives an event on an edge to the frame before.

--device cpu runs the numpy route of the same model.  Prints one JSON line: frames, the share of pixels with an event, the
mean counts per polarity and pixel, the share of saturated pixels, and seconds per frame (wall time of the whole loop,
decoding and writing included, per event image)."""
import argparse
import json
import os
import sys
import time
import types

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

DEMO_CAM = dict(H=60, W=80, fx=70.0, fy=70.0, cx=39.5, cy=29.5)       # the camera of tools/run_synthetic_slam.py
BASE_READER = {'replica_event': 'replica', 'rpg_event': 'rpg', 'rpg_event_dense': 'rpg'}


def add_noise_options(ap):
    ap.add_argument('--refractory', type=float, default=0.0)
    ap.add_argument('--leak-rate', type=float, default=0.0)
    ap.add_argument('--shot-rate', type=float, default=0.0)
    ap.add_argument('--noise-seed', type=int, default=0)


def noise_of(args):
    """the EventNoise the options ask for, None when all three effects are off"""
    if not (args.refractory > 0 or args.leak_rate > 0 or args.shot_rate > 0):
        return None
    from evennicer_slam_amd.event_sim import EventNoise
    return EventNoise(refractory=args.refractory, leak_rate=args.leak_rate, shot_rate=args.shot_rate, seed=args.noise_seed)


def simulator(args, H, W):
    from evennicer_slam_amd.event_sim import EventSimulator
    return EventSimulator(H, W, c_pos=args.c_pos, c_neg=args.c_neg, sigma_c=args.sigma_c, substeps=args.substeps, eps=args.eps,
                          seed=args.seed, device=args.device, noise=noise_of(args))


def event_stats(events):
    """Summary of a list of event images (uint8 [H,W,2] arrays): share of pixels with an event, mean counts per polarity,
    share of saturated pixels."""
    import numpy as np
    ev = np.stack([np.asarray(e) for e in events]) if len(events) else np.zeros((0, 1, 1, 2), dtype=np.uint8)
    n = max(ev.shape[0] * ev.shape[1] * ev.shape[2], 1)
    return dict(event_pixel_share=float((ev != 0).any(axis=-1).sum() / n), mean_neg=float(ev[..., 0].sum() / n),
                mean_pos=float(ev[..., 1].sum() / n), saturated_share=float((ev == 255).any(axis=-1).sum() / n))


def raw_color(path, grey):
    import numpy as np
    from PIL import Image
    with Image.open(path) as im:
        return np.array(im.convert('L' if grey else 'RGB'))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('config', nargs='?', default=None)
    ap.add_argument('--default-config', default=None)
    ap.add_argument('--input_folder', default=None)
    ap.add_argument('--out', required=True)
    ap.add_argument('--layout', choices=('replica_event', 'rpg_event'), default=None)
    ap.add_argument('--demo', type=int, default=None)
    ap.add_argument('--max-frames', type=int, default=None)
    ap.add_argument('--host-log', action='store_true')
    ap.add_argument('--device', default='cuda:0')
    ap.add_argument('--c-pos', type=float, default=0.2)
    ap.add_argument('--c-neg', type=float, default=0.2)
    ap.add_argument('--sigma-c', type=float, default=0.0)
    ap.add_argument('--substeps', type=int, default=8)
    ap.add_argument('--eps', type=float, default=1e-3)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--stream', default=None)
    ap.add_argument('--stamps', default=None)
    ap.add_argument('--fps', type=float, default=30.0)
    add_noise_options(ap)
    args = ap.parse_args(argv)
    if (args.demo is None) == (args.config is None):
        ap.error("give either a CONFIG or --demo N")

    import numpy as np
    import torch
    from evennicer_slam_amd import datasets as D

    sync = torch.cuda.synchronize if torch.device(args.device).type == 'cuda' else (lambda: None)
    out = dict(out=args.out, device=args.device)
    streams = []
    noise = noise_of(args)
    if noise is not None:
        out.update(noise=dict(refractory=noise.refractory, leak_rate=noise.leak_rate, shot_rate=noise.shot_rate, seed=noise.seed))

    def frame_times(n):
        if args.stream is None and noise is None:
            return None
        if args.stamps is not None:
            from evennicer_slam_amd.event_stream import read_stamps
            times = read_stamps(args.stamps)
            if len(times) < n:
                raise SystemExit(f"{args.stamps}: {len(times)} frame times for {n} frames")
            return times[:n].tolist()
        return [i / args.fps for i in range(n)]

    if args.demo is not None:
        from evennicer_slam_amd.synthetic import write_demo_sequence
        if args.demo < 2:
            ap.error("--demo needs at least 2 frames")
        sim = simulator(args, DEMO_CAM['H'], DEMO_CAM['W'])
        t0 = time.perf_counter()
        (inp, evf), _ = write_demo_sequence(args.out, args.demo, DEMO_CAM, events='simulate', sim=sim,
                                            stamps=frame_times(args.demo), streams=streams if args.stream is not None else None)
        sync()
        seconds = time.perf_counter() - t0
        events = [D._imread_rgb(os.path.join(evf, p))[:, :, 1:] for p in sorted(os.listdir(evf))]
        out.update(input_folder=inp, event_folder=evf, frames=args.demo, layout='replica_event')
    else:
        from evennicer_slam_amd.config import load_config
        cfg = load_config(args.config, args.default_config)
        name = cfg['dataset']
        layout = args.layout or ('rpg_event' if name.startswith('rpg') else 'replica_event')
        grey = name.startswith('rpg')
        # the plain reader of the layout: the *_event readers insist on the event images this tool is about to write
        reader = D.dataset_dict[BASE_READER.get(name, name)]
        ds = reader(cfg, types.SimpleNamespace(input_folder=args.input_folder), cfg.get('scale', 1), device='cpu')
        paths = ds.color_paths if args.max_frames is None else ds.color_paths[:args.max_frames]
        if len(paths) < 2:
            raise SystemExit("the sequence needs at least two colour images")
        os.makedirs(args.out, exist_ok=True)
        t0 = time.perf_counter()
        prev = raw_color(paths[0], grey)
        sim = simulator(args, prev.shape[0], prev.shape[1]).reset(prev, host_log=args.host_log)
        events = []
        times = frame_times(len(paths))
        for i in range(1, len(paths)):
            cur = raw_color(paths[i], grey)
            if times is None:
                ev = sim.step_images(prev, cur, host_log=args.host_log).cpu().numpy()
            elif args.stream is None:                               # the noisy sensor, images only: one launch
                ev = sim.step_images(prev, cur, host_log=args.host_log, stamps=(times[i - 1], times[i]), stream=False).cpu().numpy()
            else:
                ev, stream = sim.step_images(prev, cur, host_log=args.host_log, stamps=(times[i - 1], times[i]))
                ev = ev.cpu().numpy()
                streams.append(stream.to('cpu'))
            D.save_event_image(args.out, i, ev, layout)
            events.append(ev)
            prev = cur
        sync()
        seconds = time.perf_counter() - t0
        out.update(input_folder=ds.input_folder, event_folder=args.out, frames=len(paths), layout=layout)
    out.update(event_images=len(events), **event_stats(events), seconds_per_frame=seconds / max(len(events), 1))
    if args.stream is not None:
        from evennicer_slam_amd.event_stream import EventStream, write_events_txt
        whole = EventStream.concatenate([s.to('cpu') for s in streams]).time_sorted()
        if args.stream.endswith('.npz'):
            whole.save(args.stream)
        else:
            write_events_txt(args.stream, whole)
        out.update(stream=args.stream, stream_events=len(whole))
    print(json.dumps(out), flush=True)
    return out


if __name__ == '__main__':
    main()
