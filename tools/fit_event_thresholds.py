"""Least-squares contrast thresholds of a recorded `*_event` sequence (event_model.fit_thresholds), for `event.c_pos` /
`event.c_neg` of the model predictor (`event.predictor: model`).

    python tools/fit_event_thresholds.py CONFIG [--default-config PATH] [--input_folder DIR] [--event_folder DIR]
                                                [--max-frames N] [--eps EPS] [--device cpu]

CONFIG is a YAML chain in the reference's format (config.load_config) that names an event dataset; frame i's event image is
paired with the colour frames i - 1 and i.  Prints one JSON line: c_pos, c_neg, the pixel counts behind them, frames used.
Event counts are floored by the sensor (and by event_sim.py), so the estimate leans towards larger thresholds."""
import argparse
import json
import os
import sys
import types

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def sequence_pairs(ds, n):
    """(prev colour, cur colour, event image) of frames 1 .. n - 1 of an event dataset"""
    prev = None
    for i in range(n):
        item = ds[i]
        if len(item) != 6:
            raise SystemExit(f"{type(ds).__name__} yields no event images: fit_event_thresholds needs a *_event dataset")
        color, event = item[1], item[3]
        if prev is not None:
            yield prev, color, event
        prev = color


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('config')
    ap.add_argument('--default-config', default=None)
    ap.add_argument('--input_folder', default=None)
    ap.add_argument('--event_folder', default=None)
    ap.add_argument('--max-frames', type=int, default=None)
    ap.add_argument('--eps', type=float, default=1e-3)
    ap.add_argument('--device', default='cpu')
    args = ap.parse_args(argv)

    from evennicer_slam_amd import datasets as D
    from evennicer_slam_amd.config import load_config
    from evennicer_slam_amd.event_model import fit_thresholds

    cfg = load_config(args.config, args.default_config)
    ds = D.get_dataset(cfg, types.SimpleNamespace(input_folder=args.input_folder, event_folder=args.event_folder), cfg['scale'],
                       device=args.device)
    n = len(ds) if args.max_frames is None else min(args.max_frames, len(ds))
    fit = fit_thresholds(sequence_pairs(ds, n), eps=args.eps)
    out = dict(fit, frames=max(n - 1, 0), eps=args.eps)
    print(json.dumps(out), flush=True)
    return out


if __name__ == '__main__':
    main()
