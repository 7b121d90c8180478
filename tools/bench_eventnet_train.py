"""One training step of the event network, both routes in one process: the device route (event.compile_event_net_trainable,
csrc/event_net.hip) and the PyTorch-ROCm UNet_2heads(6, 2, 2) in eval mode with every parameter requiring a gradient (seeded
weights, BatchNorm statistics and scales randomised as in tests/eventnet_cases.py), at
the Replica event resolution (102 x 180) and RPG's (39 x 51).  A step is pack + forward + loss + backward with all
parameter gradients (the loss is tools/train_event_net.py's without the blur: squared error of events x P(event) plus the
mask's cross entropy); the optimiser is timed on its own.  After a warm-up the two routes alternate; every repeat is
timed with device events around INNER back-to-back iterations.  Reports median [min - max] per route, whether the slowest
HIP repeat is below the fastest torch repeat, and the HIP step's parts: the pack, the forward, the input-gradient
launches, the weight-gradient launches (backward_weights minus the input-gradient launches) and autograd through the pack; and, beside them, the pack
built from torch operations (event.pack_event_net_differentiable) with autograd through it, which the fused fold replaces.
Prints one JSON line per shape.

    python tools/bench_eventnet_train.py [--repeats 12] [--inner 3] [--shapes 102x180,39x51] [--bn frozen|batch] [--batch B]

--bn batch --batch B measures the training-mode route instead (event.compile_event_net_batchnorm against the torch module in
.train(), a batch of B pairs): the two routes alternate in the same way; the HIP step is split into convolutions (with
pooling, up-sampling, heads and the weight pre-pack), BatchNorm statistics, BatchNorm apply, BatchNorm backward and weight
gradients.  The three BatchNorm figures are the single-operation entries run over the 26 layers' shapes; convolutions and
weight gradients are what remains of the whole-net forward / backward calls (the backward with and without the convolution
weights' gradients).  Each BatchNorm kernel's algorithmic bytes (statistics: one read; apply: a read and a write;
backward: three reads for the sums, three reads and a write for g_z) are set against the HBM ceiling.
"""
import argparse, copy, json, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F
import evennicer_slam_amd as E
from evennicer_slam_amd import functional as EF

HBM_CEILING = 6.3e12                                        # bytes per second, as tools/bench_frame_report.py


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=12)
    ap.add_argument('--inner', type=int, default=3)
    ap.add_argument('--shapes', '--size', default='102x180,39x51')
    ap.add_argument('--bn', choices=('frozen', 'batch'), default='frozen')
    ap.add_argument('--batch', type=int, default=1)
    args = ap.parse_args(argv)
    if args.repeats < 10:
        ap.error("at least 10 repeats")
    if args.batch < 1 or args.batch > 8 or (args.batch > 1 and args.bn != 'batch'):
        ap.error("--batch is 1 to 8, above 1 only with --bn batch")
    return args


def timed(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner


def stats(ts):
    return {'median_ms': statistics.median(ts), 'min_ms': min(ts), 'max_ms': max(ts)}


def fmt(s):
    return f"{s['median_ms']:.3f} [{s['min_ms']:.3f} - {s['max_ms']:.3f}] ms"


def seeded_net(dev):
    torch.manual_seed(0)
    net = E.event.UNet_2heads(6, 2, 2)
    gen = torch.Generator().manual_seed(1)
    for m in net.modules():                                     # BatchNorm away from the identity, activations keeping their scale
        if isinstance(m, torch.nn.BatchNorm2d):
            n = m.num_features
            m.running_mean.copy_(0.1 * torch.randn(n, generator=gen))
            m.running_var.copy_(0.5 + torch.rand(n, generator=gen))
            m.weight.data.copy_(1.5 + torch.rand(n, generator=gen))
            m.bias.data.copy_(0.1 * torch.randn(n, generator=gen))
    return net.to(dev)


def bench_batch(args, dev):
    """--bn batch: one training-mode step of a batch of args.batch pairs, both routes, and the HIP step's split."""
    net = seeded_net(dev).train()
    hip = E.event.compile_event_net_batchnorm(net)
    B = args.batch
    for shape in args.shapes.split(','):
        H, W = (int(v) for v in shape.split('x'))
        x = torch.rand(B, 6, H, W, device=dev)
        target = torch.randn(B, 2, H, W, device=dev)
        mask = (torch.rand(B, H, W, device=dev) < 0.3).long()
        ge, gp = torch.randn(B, 2, H, W, device=dev), torch.randn(B, 2, H, W, device=dev)

        def step(module):
            net.zero_grad(set_to_none=True)
            e, p = module(x)
            loss = ((e * p[:, 1][:, None] - target) ** 2).sum() + F.cross_entropy(p, mask)
            loss.backward()
            return loss

        for _ in range(3):
            step(net), step(hip)
        ws = hip.workspace(B, H, W, dev)
        params, bns = hip._params()
        params = [p.detach() for p in params]
        eps = float(bns[0].eps)
        all_needs, no_conv = [True] * 82, [k >= 78 or k % 3 != 0 for k in range(82)]
        layers = []
        for i, c in enumerate(EF.EVENTNET_BN_COUT):
            lvl = EF.eventnet_conv_level(i)
            M = B * (H >> lvl) * (W >> lvl)
            z = torch.randn(M, c, device=dev)
            mean, var = EF.eventnet_bn_stats(z)
            gamma, beta = torch.rand(c, device=dev) + 1.5, torch.randn(c, device=dev)
            layers.append((z, EF.eventnet_bn_apply(z, gamma, beta, mean, var, eps), torch.randn(M, c, device=dev), gamma, beta, mean, var))
        elems = sum(z.numel() for z, *_ in layers)
        parts = {'train_forward': lambda: EF.eventnet_train_forward(params, x, ws, eps),
                 'train_backward': lambda: EF.eventnet_train_backward(params, ws, ge, gp, eps, all_needs),
                 'train_backward_no_conv_weights': lambda: EF.eventnet_train_backward(params, ws, ge, gp, eps, no_conv),
                 'bn_stats': lambda: [EF.eventnet_bn_stats(z) for z, *_ in layers],
                 'bn_apply': lambda: [EF.eventnet_bn_apply(z, g, b, m, v, eps) for z, _, _, g, b, m, v in layers],
                 'bn_backward': lambda: [EF.eventnet_bn_backward(z, y, gy, g, m, v, eps) for z, y, gy, g, _, m, v in layers]}
        t = {k: [] for k in ('torch', 'hip') + tuple(parts)}
        for f in parts.values():
            f()
        for _ in range(args.repeats):
            t['torch'].append(timed(lambda: step(net), args.inner))
            t['hip'].append(timed(lambda: step(hip), args.inner))
        for _ in range(args.repeats):
            for k, f in parts.items():
                t[k].append(timed(f, args.inner))
        res = {k: stats(v) for k, v in t.items()}
        med = lambda k: res[k]['median_ms']
        split = {'convolutions_ms': med('train_forward') - med('bn_stats') - med('bn_apply')
                 + med('train_backward_no_conv_weights') - med('bn_backward'),
                 'bn_stats_ms': med('bn_stats'), 'bn_apply_ms': med('bn_apply'), 'bn_backward_ms': med('bn_backward'),
                 'weight_gradients_ms': med('train_backward') - med('train_backward_no_conv_weights')}
        bytes_moved = {'bn_stats': 4 * elems, 'bn_apply': 8 * elems, 'bn_backward': 28 * elems}
        hbm = {k: {'bytes': v, 'bound_ms': v / HBM_CEILING * 1e3, 'fraction_of_bound': v / HBM_CEILING * 1e3 / med(k)}
               for k, v in bytes_moved.items()}
        out = {'bench': 'eventnet_train', 'bn': 'batch', 'batch': B, 'shape': shape, 'repeats': args.repeats, 'inner': args.inner,
               'routes': res, 'hip_slowest_below_torch_fastest': res['hip']['max_ms'] < res['torch']['min_ms'],
               'hip_step_split': split, 'bn_kernels_against_hbm': hbm}
        print(f"event network training-mode step B={B} {shape}: torch {fmt(res['torch'])}   hip {fmt(res['hip'])};  slowest hip "
              f"below fastest torch: {out['hip_slowest_below_torch_fastest']};  hip split "
              + ", ".join(f"{k} {v:.3f}" for k, v in split.items()) + ";  BatchNorm kernels, 26 layers, share of the HBM bound: "
              + ", ".join(f"{k} {v['fraction_of_bound']:.3f} ({v['bytes'] / 1e6:.1f} MB)" for k, v in hbm.items()))
        print(json.dumps(out))


def bench_frozen(args, dev):
    net = seeded_net(dev).eval()
    hip = E.event.compile_event_net_trainable(net)
    opt = torch.optim.Adam(net.parameters(), lr=0.0)           # lr 0: the step's work without moving the weights

    for shape in args.shapes.split(','):
        H, W = (int(v) for v in shape.split('x'))
        x = torch.rand(1, 6, H, W, device=dev)
        target = torch.randn(1, 2, H, W, device=dev)
        mask = (torch.rand(1, H, W, device=dev) < 0.3).long()
        ge, gp = torch.randn(1, 2, H, W, device=dev), torch.randn(1, 2, H, W, device=dev)

        def step(module):
            net.zero_grad(set_to_none=True)
            e, p = module(x)
            loss = ((e * p[:, 1][:, None] - target) ** 2).sum() + F.cross_entropy(p, mask)
            loss.backward()
            return loss

        # same numbers first, which is also the warm-up pair
        step(net)
        gt = {n: q.grad.clone() for n, q in net.named_parameters()}
        step(hip)
        gh = {n: q.grad.clone() for n, q in net.named_parameters()}
        net64 = copy.deepcopy(net).double().eval()              # the float64 module on the device: both routes' yardstick
        e, p = net64(x.double())
        (((e * p[:, 1][:, None] - target.double()) ** 2).sum() + F.cross_entropy(p, mask)).backward()
        g64 = {n: q.grad for n, q in net64.named_parameters()}
        worst = lambda got: max(float((got[n].double() - g64[n]).abs().max() / g64[n].abs().max()) for n in g64)
        agree = {'hip_vs_float64': worst(gh), 'torch_vs_float64': worst(gt)}
        del net64, g64
        for _ in range(2):
            step(net), step(hip)
        opt.step()
        ws, scratch = hip._workspaces[(H, W, x.device)]
        packed = hip.packed(dev).detach()
        g_packed = torch.randn_like(packed)

        def pack_and_back():
            hip.packed(dev).backward(g_packed)

        def torch_pack():                                       # the same image from torch operations (what the fused fold replaces)
            return E.event.pack_event_net_differentiable(net, dev, hip._bn_constants(dev))

        parts = {'pack': lambda: hip.packed(dev),
                 'forward': lambda: EF.eventnet_forward(packed, x, ws),
                 'input_grad_launches': lambda: EF.eventnet_backward(packed, ws, ge, gp),
                 'backward_weights': lambda: EF.eventnet_backward_weights(packed, ws, scratch, ge, gp),
                 'pack_and_autograd': pack_and_back,
                 'torch_pack': torch_pack,
                 'torch_pack_and_autograd': lambda: torch_pack().backward(g_packed),
                 'adam_step': opt.step}
        t = {k: [] for k in ('torch', 'hip') + tuple(parts)}
        for f in parts.values():
            f()
        for _ in range(args.repeats):
            t['torch'].append(timed(lambda: step(net), args.inner))
            t['hip'].append(timed(lambda: step(hip), args.inner))
        step(hip)                                               # gradients for the optimiser
        for _ in range(args.repeats):
            for k, f in parts.items():
                t[k].append(timed(f, args.inner))
        res = {k: stats(v) for k, v in t.items()}
        med = lambda k: res[k]['median_ms']
        split = {'pack_ms': med('pack'), 'forward_ms': med('forward'), 'input_grad_launches_ms': med('input_grad_launches'),
                 'weight_grad_launches_ms': med('backward_weights') - med('input_grad_launches'),
                 'autograd_through_pack_ms': med('pack_and_autograd') - med('pack')}
        torch_ops = {'pack_ms': med('torch_pack'), 'autograd_through_pack_ms': med('torch_pack_and_autograd') - med('torch_pack')}
        out = {'bench': 'eventnet_train', 'shape': shape, 'repeats': args.repeats, 'inner': args.inner, 'routes': res,
               'hip_slowest_below_torch_fastest': res['hip']['max_ms'] < res['torch']['min_ms'], 'hip_step_split': split,
               'pack_with_torch_operations': torch_ops, 'adam_step_ms': med('adam_step'), 'param_grad_max_rel_err': agree}
        print(f"event network training step {shape}: torch {fmt(res['torch'])}   hip {fmt(res['hip'])};  slowest hip below fastest "
              f"torch: {out['hip_slowest_below_torch_fastest']};  hip split " + ", ".join(f"{k} {v:.3f}" for k, v in split.items())
              + f";  the pack from torch operations instead: pack {torch_ops['pack_ms']:.3f}, autograd through it {torch_ops['autograd_through_pack_ms']:.3f}"
              + f";  Adam step alone {fmt(res['adam_step'])};  parameter gradients against the float64 module on the device, worst "
              f"tensor: hip {agree['hip_vs_float64']:.2e}, torch {agree['torch_vs_float64']:.2e}")
        print(json.dumps(out))


def main(argv=None):
    args = parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_eventnet_train.py measures on the GPU; none is visible")
    dev = torch.device('cuda', 0)
    (bench_batch if args.bn == 'batch' else bench_frozen)(args, dev)


if __name__ == '__main__':
    main()
