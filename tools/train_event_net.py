"""Train the event network UNet_2heads(6, 2, 2) on a sequence in one of the `*_event` layouts, from the supervision the
sequence carries: (previous colour, current colour) -> ground-truth event image and event mask.

    python tools/train_event_net.py CONFIG [--default-config PATH] [--input_folder DIR] [--event_folder DIR] --out PATH
                                           [--backend hip|torch] [--device cuda:0] [--epochs N] [--lr LR] [--scale-factor S]
                                           [--calibrate N] [--max-frames N] [--seed K] [--bn frozen|batch] [--batch-size N]

For every frame with a predecessor the pair is the one the tracker forms (tracker.TrackerIteration.prepare_event_frame):
both ground-truth colour images and the event image / mask resized with `resize_nearest` to the event resolution
(`event.scale_factor`, --scale-factor overrides it).  The loss is the tracker's two event terms: `event.event_loss` on
events x P(event) with the configuration's blur settings, times `event.balancer`, plus the cross entropy of the
probabilities against the mask.  Adam, one pair per step.  BatchNorm's statistics are frozen throughout (the network the
tracker uses is an eval-mode one); --calibrate N sets them first from N pairs with the torch module in training mode
under no_grad (a cumulative average), which a freshly initialised network needs: its activations otherwise shrink by
about 0.4 per layer.  --backend hip trains through event.compile_event_net_trainable (csrc/event_net.hip), torch through
the PyTorch module.  Saves the net's state_dict (what `UNet_2heads.load_state_dict` and tools/run_slam.py --event-net
take) and prints one JSON line: pairs, steps, the mean loss of the first and of the last epoch, seconds per step.

--bn batch trains with live BatchNorm instead: batch statistics in the forward, their terms in the backward, running
statistics updated with momentum and saved with the state_dict (--calibrate keeps working and is simply unnecessary).
--backend hip then trains through event.compile_event_net_batchnorm in training mode, torch through the plain module in
.train().  --batch-size N (above 1 only with --bn batch, at most 8 on the hip backend) puts N pairs into a step: the loss is
the mean of the pairs' event terms plus the cross entropy over the batch; an epoch's incomplete last batch is dropped
(BatchNorm refuses a batch whose deepest level holds one value per channel)."""
import argparse
import json
import os
import sys
import time
import types

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def make_pairs(ds, cfg, scale_factor, max_frames=None):
    """[(x [1,6,h,w] float32, gt_event [h,w,2] float32, gt_mask [1,h,w] int64)] of every frame with a predecessor."""
    import torch
    from evennicer_slam_amd.event import resize_nearest
    n = len(ds) if max_frames is None else min(max_frames, len(ds))
    pairs, prev = [], None
    for idx in range(n):
        item = ds[idx]
        if len(item) != 6:
            raise SystemExit(f"dataset {cfg['dataset']!r} carries no events: train on one of the *_event layouts")
        _, color, _, gt_event, gt_mask, _ = item
        if prev is not None:
            g = gt_event.permute(2, 0, 1)
            size = (int(scale_factor * g.shape[1]), int(scale_factor * g.shape[2]))
            if size[0] <= 0 or size[1] <= 0:
                raise SystemExit('Scale is too small, resized images would have no pixels')
            a, b = (resize_nearest(c.permute(2, 0, 1), size) for c in (prev, color))
            x = torch.cat((a, b), dim=0)[None].to(torch.float32)
            pairs.append((x, resize_nearest(g, size).permute(1, 2, 0).to(torch.float32),
                          resize_nearest(gt_mask[None, :, :], size).long()))
        prev = color
    return pairs


def pair_loss(model, pair, ecfg):
    import torch.nn.functional as F
    from evennicer_slam_amd.event import event_loss
    x, gt_event, gt_mask = pair
    events, probs = model(x)
    full_event = (events * probs[:, 1][:, None])[0].permute(1, 2, 0)
    le = event_loss(gt_event, full_event, ecfg.get('blur', True), ecfg.get('kernel_sizes', (9,)), ecfg.get('unblurred_weight', 0.0),
                    ecfg.get('kernel_weights', (1.0,)))[0]
    return le * ecfg.get('balancer', 1.0) + F.cross_entropy(probs, gt_mask)


def batch_loss(model, batch, ecfg):
    """pair_loss of a list of pairs run as one batch: the mean of the pairs' event terms plus the cross entropy over the
    batch (one pair: pair_loss itself)."""
    import torch
    import torch.nn.functional as F
    from evennicer_slam_amd.event import event_loss
    if len(batch) == 1:
        return pair_loss(model, batch[0], ecfg)
    events, probs = model(torch.cat([x for x, _, _ in batch], dim=0))
    full = (events * probs[:, 1][:, None]).permute(0, 2, 3, 1)
    terms = [event_loss(gt, full[b], ecfg.get('blur', True), ecfg.get('kernel_sizes', (9,)), ecfg.get('unblurred_weight', 0.0),
                        ecfg.get('kernel_weights', (1.0,)))[0] for b, (_, gt, _) in enumerate(batch)]
    return torch.stack(terms).mean() * ecfg.get('balancer', 1.0) + F.cross_entropy(probs, torch.cat([m for _, _, m in batch], dim=0))


def calibrate(net, pairs, n):
    """BatchNorm running statistics := the cumulative average over the first n pairs, run in batches (training mode, no
    gradients)."""
    import torch
    bns = [m for m in net.modules() if isinstance(m, torch.nn.BatchNorm2d)]
    momenta = [m.momentum for m in bns]
    for m in bns:
        m.reset_running_stats()
        m.momentum = None
    xs = torch.cat([x for x, _, _ in pairs[:n]], dim=0)
    if xs.shape[0] < 2:
        raise SystemExit("--calibrate needs at least 2 pairs: the deepest level may be a single pixel per pair")
    net.train()
    with torch.no_grad():
        for chunk in xs.chunk((xs.shape[0] + 7) // 8):             # batches of 2 to 8 pairs
            net(chunk)
    net.eval()
    for m, mom in zip(bns, momenta):
        m.momentum = mom


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('config')
    ap.add_argument('--default-config', default=None)
    ap.add_argument('--input_folder', default=None)
    ap.add_argument('--event_folder', default=None)
    ap.add_argument('--out', required=True)
    ap.add_argument('--backend', choices=('hip', 'torch'), default='hip')
    ap.add_argument('--device', default='cuda:0')
    ap.add_argument('--epochs', type=int, default=10)
    ap.add_argument('--lr', type=float, default=1e-4)
    ap.add_argument('--scale-factor', type=float, default=None)
    ap.add_argument('--calibrate', type=int, default=0)
    ap.add_argument('--max-frames', type=int, default=None)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--bn', choices=('frozen', 'batch'), default='frozen')
    ap.add_argument('--batch-size', type=int, default=1)
    args = ap.parse_args(argv)
    if args.batch_size < 1 or (args.batch_size > 1 and args.bn != 'batch'):
        ap.error("--batch-size above 1 needs --bn batch (the frozen route runs one pair per step)")

    import torch
    from evennicer_slam_amd import datasets as D
    from evennicer_slam_amd import event as EV
    from evennicer_slam_amd.config import load_config

    cfg = load_config(args.config, args.default_config)
    ecfg = cfg.get('event') or {}
    sf = args.scale_factor if args.scale_factor is not None else ecfg.get('scale_factor', 0.1)
    ds = D.get_dataset(cfg, types.SimpleNamespace(input_folder=args.input_folder, event_folder=args.event_folder), cfg['scale'],
                       device=args.device)
    pairs = make_pairs(ds, cfg, sf, args.max_frames)
    if not pairs:
        raise SystemExit("the sequence has no frame with a predecessor")
    torch.manual_seed(args.seed)
    net = EV.UNet_2heads(6, 2, 2).to(args.device).eval()
    if args.calibrate > 0:
        calibrate(net, pairs, args.calibrate)
    if args.bn == 'batch':
        if len(pairs) < args.batch_size:
            raise SystemExit(f"--batch-size {args.batch_size} needs at least that many pairs (the sequence has {len(pairs)})")
        model = EV.compile_event_net_batchnorm(net) if args.backend == 'hip' else net
        model.train()
    else:
        model = EV.compile_event_net_trainable(net) if args.backend == 'hip' else net
    opt = torch.optim.Adam(net.parameters(), lr=args.lr)
    order = torch.Generator().manual_seed(args.seed)
    epoch_means, steps = [], 0
    sync = torch.cuda.synchronize if torch.device(args.device).type == 'cuda' else (lambda: None)
    sync()
    t0 = time.perf_counter()
    for _ in range(args.epochs):
        losses = []
        perm = torch.randperm(len(pairs), generator=order).tolist()
        for at in range(0, len(perm) - args.batch_size + 1, args.batch_size):
            opt.zero_grad(set_to_none=True)
            loss = batch_loss(model, [pairs[k] for k in perm[at:at + args.batch_size]], ecfg)
            loss.backward()
            opt.step()
            losses.append(loss.detach())
            steps += 1
        epoch_means.append(float(torch.stack(losses).mean()))
    sync()
    seconds = time.perf_counter() - t0
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    torch.save({k: v.detach().cpu() for k, v in net.state_dict().items()}, args.out)
    out = dict(out=args.out, backend=args.backend, bn=args.bn, batch_size=args.batch_size, pairs=len(pairs), steps=steps, event_size=list(pairs[0][0].shape[2:]),
               first_loss=epoch_means[0], last_loss=epoch_means[-1], seconds_per_step=seconds / max(steps, 1))
    print(json.dumps(out), flush=True)
    return out


if __name__ == '__main__':
    main()
