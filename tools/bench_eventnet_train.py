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

    python tools/bench_eventnet_train.py [--repeats 12] [--inner 3] [--shapes 102x180,39x51]
"""
import argparse, copy, json, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F
import evennicer_slam_amd as E
from evennicer_slam_amd import functional as EF

ap = argparse.ArgumentParser()
ap.add_argument('--repeats', type=int, default=12)
ap.add_argument('--inner', type=int, default=3)
ap.add_argument('--shapes', default='102x180,39x51')
args = ap.parse_args()
assert args.repeats >= 10, "at least 10 repeats"
if not torch.cuda.is_available():
    raise SystemExit("bench_eventnet_train.py measures on the GPU; none is visible")
dev = torch.device('cuda', 0)


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
net = net.to(dev).eval()
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
