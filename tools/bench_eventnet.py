"""The event network alone, both routes in one process: the PyTorch-ROCm UNet_2heads(6, 2, 2) with frozen parameters and
its device route (event.compile_event_net, csrc/event_net.hip), forward + input gradient, at the Replica event resolution
(102 x 180) and RPG's (39 x 51).  After one warm-up pair the two routes alternate; every repeat is timed with device events
around INNER back-to-back iterations.  Reports median [min - max] per route, whether the slowest HIP repeat is below the
fastest torch repeat, and for the HIP route the time of every convolution (forward / input gradient, through the
single-operation ABI entry on the layer's real shapes and packed weights) with its share of the 157.3 TFLOP/s fp32-MFMA
yardstick.  FLOPs are counted here: 2 x MAC of the 3 x 3 convolutions only.  Prints one JSON line per shape.

    python tools/bench_eventnet.py [--repeats 12] [--inner 5] [--shapes 102x180,39x51]
"""
import argparse, ctypes, json, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import evennicer_slam_amd as E

PEAK = 157.3e12
ap = argparse.ArgumentParser()
ap.add_argument('--repeats', type=int, default=12)
ap.add_argument('--inner', type=int, default=5)
ap.add_argument('--shapes', default='102x180,39x51')
args = ap.parse_args()
assert args.repeats >= 10, "at least 10 repeats"
if not torch.cuda.is_available():
    raise SystemExit("bench_eventnet.py measures on the GPU; none is visible")
dev = torch.device('cuda', 0)
lib = E._lib.lib()
CONVS = E.event.EVENTNET_CONVS
NAMES = [f'{b}.{k}' for b in ('inc', 'down1', 'down2', 'down3', 'down4') for k in (0, 1)] + \
        [f'up{l}_{h}.{k}' for h in (1, 2) for l in (1, 2, 3, 4) for k in (0, 1)]


def levels(H, W):
    out = [(H, W)]
    for _ in range(4):
        out.append((out[-1][0] // 2, out[-1][1] // 2))
    return out


def conv_level(i):
    return i // 2 if i < 10 else 3 - ((i - 10) % 8) // 2


def conv_flops(H, W):
    """2 x MAC per convolution (the first layer with its 6 real input channels), one direction"""
    lv = levels(H, W)
    return [2 * 9 * (6 if i == 0 else cin) * cout * lv[conv_level(i)][0] * lv[conv_level(i)][1] for i, (cin, cout) in enumerate(CONVS)]


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
net.requires_grad_(False)
net = net.to(dev).eval()
hip = E.event.compile_event_net(net)
stream = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

for shape in args.shapes.split(','):
    H, W = (int(v) for v in shape.split('x'))
    x = torch.rand(1, 6, H, W, device=dev, requires_grad=True)
    ge, gp = torch.randn(1, 2, H, W, device=dev), torch.randn(1, 2, H, W, device=dev)

    def run(module):
        e, p = module(x)
        g, = torch.autograd.grad([e, p], [x], [ge, gp])
        return e, p, g

    def fwd(module):
        with torch.no_grad():
            return module(x)

    # same numbers first (measuring-on-mi355x section 6), which is also the warm-up pair
    rt, rh = run(net), run(hip)
    agree = {k: float((a.detach() - b.detach()).abs().max() / a.detach().abs().max()) for k, a, b in zip(('events', 'probs', 'gx'), rt, rh)}
    for _ in range(2):
        run(net), run(hip), fwd(net), fwd(hip)
    t = {'torch': [], 'hip': [], 'torch_fwd': [], 'hip_fwd': []}
    for _ in range(args.repeats):
        t['torch'].append(timed(lambda: run(net), args.inner))
        t['hip'].append(timed(lambda: run(hip), args.inner))
        t['torch_fwd'].append(timed(lambda: fwd(net), args.inner))
        t['hip_fwd'].append(timed(lambda: fwd(hip), args.inner))
    res = {k: stats(v) for k, v in t.items()}
    fl = conv_flops(H, W)
    total = 2 * sum(fl)                                   # forward + input gradient

    # per convolution and direction, HIP route: the layer's shapes, its packed weights, random activations
    packed = hip.packed(dev)
    lv = levels(H, W)
    scratch = torch.empty((1 << 22) + H * W * 64, device=dev)
    layers, off = [], 0
    for i, (cin, cout) in enumerate(CONVS):
        n = 9 * cin * cout
        wf, b, wt = packed[off:off + n], packed[off + n:off + n + cout], packed[off + n + cout:off + 2 * n + cout]
        off += 2 * n + cout
        h, w = lv[conv_level(i)]
        two = i >= 10 and (i - 10) % 2 == 0
        C0, C1 = (cin // 2, cin // 2) if two else (cin, 0)
        H1, W1 = (2 * (h // 2), 2 * (w // 2)) if two else (0, 0)
        a0, a1 = torch.rand(h * w * C0, device=dev), (torch.rand(H1 * W1 * C1, device=dev) if two else None)
        out, g, saved = torch.empty(h * w * cout, device=dev), torch.randn(h * w * cout, device=dev), torch.randn(h * w * cout, device=dev)
        d0, d1 = torch.empty(h * w * C0, device=dev), (torch.empty(H1 * W1 * C1, device=dev) if two else None)
        p = lambda q: None if q is None else q.data_ptr()

        def f_fwd():
            assert lib.enslam_eventnet_conv3x3(p(wf), p(b), h, w, C0, C1, H1, W1, 0, 0, cout, p(a0), p(a1), p(out), None, 1, 0,
                                               p(scratch), scratch.numel(), stream()) == 0

        def f_bwd():
            assert lib.enslam_eventnet_conv3x3(p(wt), None, h, w, C0, C1, H1, W1, 0, 0, cout, p(g), p(saved), p(d0), p(d1), 0, 1,
                                               p(scratch), scratch.numel(), stream()) == 0
        row = {'layer': NAMES[i], 'pixels': h * w, 'cin': cin, 'cout': cout, 'gflop': fl[i] / 1e9}
        for name, f in (('fwd', f_fwd), ('bwd', f_bwd)):
            f(), f()
            ts = [timed(f, args.inner) for _ in range(args.repeats)]
            row[name + '_ms'] = statistics.median(ts)
            row[name + '_of_peak'] = fl[i] / (row[name + '_ms'] * 1e-3) / PEAK
        layers.append(row)
    conv_ms = sum(r['fwd_ms'] + r['bwd_ms'] for r in layers)
    out = {'bench': 'eventnet', 'shape': shape, 'repeats': args.repeats, 'inner': args.inner,
           'gflop_fwd_plus_input_grad': total / 1e9, 'routes': res,
           'hip_slowest_below_torch_fastest': res['hip']['max_ms'] < res['torch']['min_ms'],
           'hip_of_peak': total / (res['hip']['median_ms'] * 1e-3) / PEAK,
           'torch_of_peak': total / (res['torch']['median_ms'] * 1e-3) / PEAK,
           'hip_vs_torch_max_rel_diff': agree, 'hip_conv_layers_sum_ms': conv_ms, 'hip_layers': layers}
    print(f"event network {shape}: forward + input gradient  torch {fmt(res['torch'])}   hip {fmt(res['hip'])}   "
          f"(forward alone: torch {fmt(res['torch_fwd'])}, hip {fmt(res['hip_fwd'])});  slowest hip below fastest torch: "
          f"{out['hip_slowest_below_torch_fastest']};  {total / 1e9:.2f} GFLOP -> hip {out['hip_of_peak']:.3f}, torch "
          f"{out['torch_of_peak']:.3f} of 157.3 TFLOP/s;  hip vs torch {agree}")
    print(f"  {'layer':10s} {'pixels':>6s} {'cin':>5s} {'cout':>5s} {'GFLOP':>7s} {'fwd ms':>8s} {'of peak':>8s} {'bwd ms':>8s} {'of peak':>8s}")
    for r in layers:
        print(f"  {r['layer']:10s} {r['pixels']:6d} {r['cin']:5d} {r['cout']:5d} {r['gflop']:7.3f} {r['fwd_ms']:8.4f} {r['fwd_of_peak']:8.3f} "
              f"{r['bwd_ms']:8.4f} {r['bwd_of_peak']:8.3f}")
    print(f"  convolutions alone, summed: {conv_ms:.3f} ms")
    print(json.dumps(out))
