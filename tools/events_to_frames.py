"""Bin a recorded event stream into the event folder the `*_event` readers take.

    python tools/events_to_frames.py EVENTS STAMPS --out DIR --height H --width W
                                     [--gap G] [--density D] [--layout rpg_event|replica_event]
                                     [--poses traj.txt] [--device cuda:0|cpu]
                                     [--refractory S] [--support-dt S] [--hot-rate HZ | --hot-max N]

EVENTS: a stream, `.npz` (event_stream.EventStream.save) or the RPG / DAVIS text layout, one event per line `t x y p` with t in
seconds and p in {0, 1}.  STAMPS: a text file whose first field per non-comment line is a frame time (the recordings'
images.txt).  Every --gap-th frame is kept and each kept interval is split into --density equal parts
(event_stream.frame_edges); one png per part is written into --out, numbered from 1 like the sequence writers do:
event%06d.png with channels (+, -, 0) for `rpg_event` (RPG_event at density 1, RPG_event_dense above), event_frame%06d.png
with (0, -, +) for `replica_event`.  For n kept frames that is (n - 1) * density files, what the readers assert.  An event
whose time is exactly a frame time belongs to the part that ENDS there; a simulated stream with leak (tools/simulate_events.py
--leak-rate) holds such events at the start of an interval, which therefore count for the frame before, not for their own.

--poses traj.txt (one row-major 4x4 camera-to-world per line, one line per frame of STAMPS) with --density above 1 also
writes traj_density{D}.txt next to it, in the format of datasets.write_rpg_event_dense_sequence: the kept frames' poses with
density - 1 poses interpolated in between (event_sim.interpolate_poses), (n - 1) * density + 1 lines.

--refractory S, --support-dt S, --hot-rate HZ / --hot-max N (all opt-in) denoise the stream before it is binned
(event_filter.py: refractory filter, neighbour-support filter, hot-pixel mask).  With a hot flag the mask is learned from the
whole stream first (a pixel is hot above N events, or above HZ times the stream's duration); then the stream is filtered in
one call, and the counters join the JSON line as `filter`; `events_read` and the drop counts then refer to the filtered stream.

--device cpu bins (and filters) with numpy under the same rules.  Prints one JSON line: events read, binned, dropped by time, dropped by
sensor, saturated pixels (pixel-polarity counts above 255), files written."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

BINS_PER_CALL = 64


def dense_poses(poses, density):
    """[(n - 1) * density + 1, 4, 4] float64: the poses with density - 1 interpolated ones in every interval"""
    import numpy as np
    from evennicer_slam_amd.event_sim import interpolate_poses
    out = [np.asarray(poses[0], dtype=np.float64)]
    for a, b in zip(poses[:-1], poses[1:]):
        out.extend(interpolate_poses(a, b, density))
    return np.stack(out)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('events')
    ap.add_argument('stamps')
    ap.add_argument('--out', required=True)
    ap.add_argument('--height', type=int, required=True)
    ap.add_argument('--width', type=int, required=True)
    ap.add_argument('--gap', type=int, default=1)
    ap.add_argument('--density', type=int, default=1)
    ap.add_argument('--layout', choices=('rpg_event', 'replica_event'), default='rpg_event')
    ap.add_argument('--poses', default=None)
    ap.add_argument('--device', default='cuda:0')
    ap.add_argument('--refractory', type=float, default=None, metavar='S')
    ap.add_argument('--support-dt', type=float, default=None, metavar='S')
    hot = ap.add_mutually_exclusive_group()
    hot.add_argument('--hot-rate', type=float, default=None, metavar='HZ')
    hot.add_argument('--hot-max', type=int, default=None, metavar='N')
    args = ap.parse_args(argv)

    import numpy as np
    from evennicer_slam_amd import datasets as D
    from evennicer_slam_amd import event_stream as ES

    H, W = args.height, args.width
    stamps = ES.read_stamps(args.stamps)
    edges = ES.frame_edges(stamps, args.gap, args.density)
    stream = ES.load_stream(args.events, device=args.device)
    filter_stats = None
    if any(v is not None for v in (args.refractory, args.support_dt, args.hot_rate, args.hot_max)):
        from evennicer_slam_amd import event_filter as EFI
        stream, filter_stats = EFI.filter_from_options(stream, H, W, args.refractory, args.support_dt, args.hot_rate, args.hot_max)
    os.makedirs(args.out, exist_ok=True)
    B = len(edges) - 1
    binned = saturated = 0
    sensor = None
    missed = 0                                                   # summed over the calls: events outside THAT call's bins
    calls = 0
    for b0 in range(0, B, BINS_PER_CALL):
        b1 = min(b0 + BINS_PER_CALL, B)
        counts, full, dropped = ES.accumulate(stream, edges[b0:b1 + 1], H, W, want_unsaturated=True, with_dropped=True)
        counts, full = counts.cpu().numpy(), full.cpu().numpy().astype(np.int64)
        binned += int(full.sum())
        saturated += int((full > 255).sum())
        missed += dropped[0]
        sensor = dropped[1]
        calls += 1
        for b in range(b0, b1):
            D.save_event_image(args.out, b + 1, counts[b - b0], args.layout)
    out = dict(out=args.out, layout=args.layout, gap=args.gap, density=args.density, frames_kept=(B // args.density) + 1,
               events_read=len(stream), events_binned=binned, dropped_by_time=len(stream) - (sensor or 0) - binned,
               dropped_by_sensor=sensor or 0, saturated_pixels=saturated, files_written=B, device=args.device)
    if filter_stats is not None:
        out['filter'] = filter_stats
    assert calls == 0 or missed - (calls - 1) * (len(stream) - (sensor or 0)) == out['dropped_by_time']
    if args.poses is not None and args.density > 1:
        with open(args.poses, 'r') as f:
            poses = [np.array(line.split(), dtype=np.float64).reshape(4, 4) for line in f if line.strip()]
        if len(poses) < len(stamps):
            raise SystemExit(f"{args.poses}: {len(poses)} poses for {len(stamps)} frame times")
        dense = dense_poses(poses[:len(stamps)][::args.gap], args.density)
        path = os.path.join(os.path.dirname(os.path.abspath(args.poses)), f'traj_density{args.density}.txt')
        with open(path, 'w') as f:
            for pose in dense:
                f.write(' '.join(repr(float(v)) for v in pose.reshape(-1)) + '\n')
        out.update(dense_poses=path, dense_pose_lines=len(dense))
    print(json.dumps(out), flush=True)
    return out


if __name__ == '__main__':
    main()
