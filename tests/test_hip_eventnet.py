"""-m gpu: the device event network (csrc/event_net.hip, event.compile_event_net) -- single operations through the C ABI
against float64 numpy / torch on the CPU, the whole net against the float64 module on the CPU, determinism, graph replay,
repacking, the tracker integration and the ABI's error codes.  Cases and tolerances: tests/eventnet_cases.py."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import eventnet_cases as C

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def _E():
    import evennicer_slam_amd as E
    return E


def _lib():
    return _E()._lib.lib()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _conv(w, bias, H, W, C0, C1, H1, W1, oy, ox, Cn, a0, a1, d0, d1, relu, transposed):
    scratch = torch.empty((1 << 22) + H * W * max(C0 + C1, Cn), dtype=torch.float32, device=DEV)
    p = lambda t: None if t is None else t.data_ptr()
    code = _lib().enslam_eventnet_conv3x3(p(w), p(bias), H, W, C0, C1, H1, W1, oy, ox, Cn, p(a0), p(a1), p(d0), p(d1), relu,
                                          transposed, p(scratch), scratch.numel(), _stream())
    torch.cuda.synchronize()
    return code


# ---------------------------------------------------------------------------------------------------------------------
# convolution, forward and transposed, against float64 numpy with the derived bound
#   |computed - exact| <= gamma_{K+2} (sum |w x| + |b|),  gamma_n = n u / (1 - n u),  K the reduction length:
# it holds for any summation order of K products and one bias addition (Higham, Accuracy and Stability, 3.1/3.4).
# ---------------------------------------------------------------------------------------------------------------------
PIXELS = [(1, 1), (2, 3), (6, 11), (9, 13), (17, 19)]
CHANNELS = [(8, 0, 64), (64, 0, 64), (128, 64, 64), (512, 0, 512), (1024, 0, 512)]
# 46 x 45 pixels, 64 -> 512: 33 x 8 output tiles, where the reduction is no longer split (the direct epilogue)
EXTRA = [((46, 45), (64, 0, 512))]


def _conv_case(H, W, C0, C1, Cn, off):
    rng = np.random.default_rng(1000 * H + 10 * W + C0 + C1 + Cn + off)
    H1, W1 = (max(1, H - 1), max(1, W - 1)) if C1 else (0, 0)
    Cin = C0 + C1
    f32 = lambda *s: rng.standard_normal(s).astype(np.float32)
    wf, b = f32(9 * Cin, Cn) / np.float32(np.sqrt(9 * Cin)), f32(Cn)
    x0 = f32(H, W, C0)
    x1 = f32(H1, W1, C1) if C1 else None
    # forward
    full = x0 if not C1 else np.concatenate([x0, C.place(x1, H, W, off, off)], axis=2)
    ref = C.np_conv3x3(wf, b, full, relu=True)
    bound = C.gamma(9 * Cin + 2) * (C.np_conv3x3(np.abs(wf), np.abs(b), np.abs(full)))
    out = torch.full((H, W, Cn), float('nan'), device=DEV)
    code = _conv(_dev(wf), _dev(b), H, W, C0, C1, H1, W1, off, off, Cn, _dev(x0), _dev(x1) if C1 else None, out, None, 1, 0)
    assert code == 0
    got = out.cpu().numpy().astype(np.float64)
    assert np.isfinite(got).all()
    worst = float((np.abs(got - ref) / np.maximum(bound, 1e-300)).max())
    print(f"conv {H}x{W} {C0}+{C1}->{Cn} off {off}: forward error / bound {worst:.3f}")
    assert (np.abs(got - ref) <= bound).all()
    # transposed: g [H, W, Cn] masked by saved > 0 -> d0 [H, W, C0], d1 [H1, W1, C1]
    wt, g, saved = f32(9 * Cn, Cin) / np.float32(np.sqrt(9 * Cn)), f32(H, W, Cn), f32(H, W, Cn)
    saved[rng.random(saved.shape) < 0.1] = 0.0                      # relu'(0) = 0
    gm = np.where(saved > 0, g, np.float32(0))
    ref = C.np_conv3x3(wt, None, gm)
    bound = C.gamma(9 * Cn + 2) * C.np_conv3x3(np.abs(wt), None, np.abs(gm))
    d0 = torch.full((H, W, C0), float('nan'), device=DEV)
    d1 = torch.full((H1, W1, C1), float('nan'), device=DEV) if C1 else None
    code = _conv(_dev(wt), None, H, W, C0, C1, H1, W1, off, off, Cn, _dev(g), _dev(saved), d0, d1, 0, 1)
    assert code == 0
    parts = [(d0.cpu().numpy().astype(np.float64), ref[..., :C0], bound[..., :C0])]
    if C1:
        sl = (slice(off, off + H1), slice(off, off + W1), slice(C0, None))
        parts.append((d1.cpu().numpy().astype(np.float64), ref[sl], bound[sl]))
    for got, r, bd in parts:
        assert np.isfinite(got).all()
        assert (np.abs(got - r) <= bd).all()


@pytest.mark.parametrize("chan", CHANNELS, ids=lambda c: f"{c[0]}+{c[1]}to{c[2]}")
@pytest.mark.parametrize("pix", PIXELS, ids=lambda p: f"{p[0]}x{p[1]}")
def test_conv3x3_forward_and_transposed(pix, chan):
    (H, W), (C0, C1, Cn) = pix, chan
    offsets = (0, 1) if C1 and min(H, W) > 1 else (0,)
    for off in offsets:
        _conv_case(H, W, C0, C1, Cn, off)


@pytest.mark.parametrize("pix,chan", EXTRA, ids=["46x45-64to512-unsplit"])
def test_conv3x3_unsplit_reduction(pix, chan):
    _conv_case(pix[0], pix[1], chan[0], chan[1], chan[2], 0)


def test_conv3x3_is_deterministic():
    rng = np.random.default_rng(3)
    H, W, C0, Cn = 9, 13, 512, 512
    w, b, x = (_dev(rng.standard_normal(s)) for s in ((9 * C0, Cn), (Cn,), (H, W, C0)))
    outs = []
    for _ in range(2):
        out = torch.empty((H, W, Cn), device=DEV)
        assert _conv(w, b, H, W, C0, 0, 0, 0, 0, 0, Cn, x, None, out, None, 1, 0) == 0
        outs.append(out.cpu())
    assert torch.equal(outs[0], outs[1])


# ---------------------------------------------------------------------------------------------------------------------
# pooling and up-sampling
# ---------------------------------------------------------------------------------------------------------------------
def _cl(t):
    """[1,C,H,W] CPU tensor -> channels-last [H,W,C] device tensor"""
    return t[0].permute(1, 2, 0).contiguous().to(DEV)


def _nchw(t):
    return t.cpu().permute(2, 0, 1)[None].contiguous()


@pytest.mark.parametrize("H,W,Ch", [(2, 2, 8), (5, 7, 16), (6, 11, 64), (17, 19, 24)])
def test_pool2_forward_and_backward_bit_equal_to_torch(H, W, Ch):
    gen = torch.Generator().manual_seed(H * 100 + W)
    x = torch.randn(1, Ch, H, W, generator=gen)
    # constructed ties: whole windows equal (channel 0), equal row pairs (1), few distinct values (2, 3)
    x[:, 0] = 1.0
    x[:, 1, 1::2, :] = x[:, 1, 0:2 * (H // 2):2, :]
    x[:, 2] = torch.round(x[:, 2])
    x[:, 3] = torch.round(2 * x[:, 3]) / 2
    xr = x.clone().requires_grad_(True)
    y = F.max_pool2d(xr, 2)
    g = torch.randn(y.shape, generator=gen)
    y.backward(g)
    lib = _lib()
    xd, gd = _cl(x), _cl(g)                            # held: the calls below take raw addresses
    out = torch.full((H // 2, W // 2, Ch), float('nan'), device=DEV)
    assert lib.enslam_eventnet_pool2(xd.data_ptr(), H, W, Ch, None, out.data_ptr(), 0, _stream()) == 0
    torch.cuda.synchronize()
    assert torch.equal(_nchw(out), y.detach())
    dx = torch.full((H, W, Ch), float('nan'), device=DEV)
    assert lib.enslam_eventnet_pool2(xd.data_ptr(), H, W, Ch, gd.data_ptr(), dx.data_ptr(), 1, _stream()) == 0
    torch.cuda.synchronize()
    assert torch.equal(_nchw(dx), xr.grad)


@pytest.mark.parametrize("h,w", [(1, 1), (2, 3), (6, 11)])
def test_up2_matches_interpolate(h, w):
    Ch = 16
    lib = _lib()
    gen = torch.Generator().manual_seed(h * 10 + w)

    def up(x):
        xd = _cl(x)                                    # held: the call takes raw addresses
        out = torch.full((2 * h, 2 * w, Ch), float('nan'), device=DEV)
        assert lib.enslam_eventnet_up2(xd.data_ptr(), h, w, Ch, out.data_ptr(), 0, _stream()) == 0
        torch.cuda.synchronize()
        return _nchw(out)

    # one-hot images: every output is one product of two interpolation weights, rounded once -- bit-equal to F.interpolate
    # exactly when the weights are
    hot = torch.zeros(1, Ch, h, w)
    for c in range(Ch):
        hot[0, c].view(-1)[(c * 7) % (h * w)] = 1.0
    ref = F.interpolate(hot, scale_factor=2, mode='bilinear', align_corners=True)
    assert torch.equal(up(hot), ref)
    x = torch.randn(1, Ch, h, w, generator=gen)
    ref = F.interpolate(x, scale_factor=2, mode='bilinear', align_corners=True)
    assert float((up(x) - ref).abs().max()) <= 4 * C.U * float(x.abs().max())
    # backward: the gather against float64 autograd (a sum of at most 16 weighted terms per pixel, weights <= 1)
    xr = x.double().requires_grad_(True)
    g = torch.randn(1, Ch, 2 * h, 2 * w, generator=gen)
    F.interpolate(xr, scale_factor=2, mode='bilinear', align_corners=True).backward(g.double())
    gd = _cl(g)
    dx = torch.full((h, w, Ch), float('nan'), device=DEV)
    assert lib.enslam_eventnet_up2(gd.data_ptr(), h, w, Ch, dx.data_ptr(), 1, _stream()) == 0
    torch.cuda.synchronize()
    # At most 16 output pixels touch one input pixel and their weights sum to at most 6.  Per term the float32 weight is
    # off float64's by at most 2u(h + w) + 3u (the source coordinate scale * dst carries ~2u * dst, two subtractions and a
    # product round once each); the running fmaf sum adds gamma_16 of sum |w g|.
    tol = C.U * (16 * (2 * (h + w) + 3) + 16 * 6) * float(g.abs().max())
    assert float((_nchw(dx).double() - xr.grad).abs().max()) <= tol


# ---------------------------------------------------------------------------------------------------------------------
# whole net
# ---------------------------------------------------------------------------------------------------------------------
_compiled = {}


def _net(seed=0):
    if seed not in _compiled:
        _compiled[seed] = _E().event.compile_event_net(C.make_net(seed))
    return _compiled[seed]


def _run(net, shape, seed=0):
    x, ge, gp = (t.to(DEV) for t in C.make_inputs(shape, seed))
    x.requires_grad_(True)
    e, p = net(x)
    torch.autograd.backward([e, p], [ge, gp])
    torch.cuda.synchronize()
    return e.detach().cpu(), p.detach().cpu(), x.grad.cpu()


@pytest.mark.parametrize("shape", list(C.NET_SHAPES))
def test_whole_net_against_float64_module(shape):
    ref = C.reference(shape)
    got = _run(_net(), shape)
    H, W = C.NET_SHAPES[shape]
    assert got[0].shape == got[1].shape == (1, 2, H, W) and got[2].shape == (1, 6, H, W)
    errs = {q: C.rel_max(g.numpy(), r) for q, g, r in zip(('events', 'probs', 'gx'), got, ref)}
    print(f"{shape}: HIP vs float64 module {errs}; tolerances { {q: C.tolerance(shape, q) for q in errs} }")
    for q, e in errs.items():
        assert e <= C.tolerance(shape, q), (q, e)


def test_two_calls_are_bit_equal_and_a_graph_replays_the_eager_call():
    net = _net()
    a = _run(net, '17x19')
    b = _run(net, '17x19')
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    x, ge, gp = (t.to(DEV) for t in C.make_inputs('17x19'))
    xs = x.clone().requires_grad_(True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                     # warm-up on the side stream, as torch's capture recipe asks
        e, p = net(xs)
        torch.autograd.backward([e, p], [ge, gp])
    torch.cuda.current_stream().wait_stream(side)
    xs.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        e, p = net(xs)
        gx, = torch.autograd.grad([e, p], [xs], [ge, gp])
    for _ in range(2):
        e.zero_(), p.zero_(), gx.zero_()
        graph.replay()
        torch.cuda.synchronize()
        for u, v in zip(a, (e, p, gx)):
            assert torch.equal(u, v.detach().cpu())


def test_no_backward_launch_without_an_input_gradient():
    from evennicer_slam_amd import functional as EF
    net = _net()
    ref = _run(net, '16x16')
    x, ge, gp = (t.to(DEV) for t in C.make_inputs('16x16'))
    before = dict(EF.eventnet_launches)
    e, p = net(x)                                      # x does not require a gradient
    assert not e.requires_grad and not p.requires_grad
    scale = torch.ones((), device=DEV, requires_grad=True)
    ((e * ge).sum() * scale + (p * gp).sum() * scale).backward()
    torch.cuda.synchronize()
    assert EF.eventnet_launches['forward'] == before['forward'] + 1
    assert EF.eventnet_launches['backward'] == before['backward']
    assert scale.grad is not None
    assert torch.equal(e.cpu(), ref[0]) and torch.equal(p.cpu(), ref[1])
    with torch.no_grad():
        e2, p2 = net(x)
    assert torch.equal(e2.cpu(), ref[0]) and torch.equal(p2.cpu(), ref[1])


def test_backward_after_another_forward_of_the_same_size():
    """The workspace is shared per image size: a backward whose forward is no longer the last one restores it first."""
    net = _net()
    ref = _run(net, '16x16')
    x, ge, gp = (t.to(DEV) for t in C.make_inputs('16x16'))
    x.requires_grad_(True)
    e, p = net(x)
    with torch.no_grad():
        net(torch.rand_like(x))
    torch.autograd.backward([e, p], [ge, gp])
    assert torch.equal(x.grad.cpu(), ref[2])


def test_repack_after_a_buffer_changes_in_place():
    E = _E()
    base = C.make_net(2)
    net = E.event.compile_event_net(base)
    x = C.make_inputs('16x16', 2)[0].to(DEV)
    with torch.no_grad():
        e0, p0 = net(x)
        base.down2.maxpool_conv[1].double_conv[1].running_mean.mul_(-3.0)
        e1, p1 = net(x)
        fresh = E.event.compile_event_net(base)
        e2, p2 = fresh(x)
        assert not torch.equal(e0, e1) and not torch.equal(p0, p1)
        assert torch.equal(e1, e2) and torch.equal(p1, p2)
        sd = C.make_net(2).state_dict()              # load_state_dict goes through copy_: seen as well
        base.load_state_dict(sd)
        e3, _ = net(x)
        assert torch.equal(e3, e0)


def test_tracker_iteration_with_the_compiled_net(monkeypatch):
    """TrackerIteration.iteration_losses on tests/golden/tiny_event_iter.npz with the torch net and with its compiled form:
    event loss, mask loss and pose gradient agree.  Tolerance: the 24 x 32 event image is between the 17x19 and 39x51
    cases, so the per-tensor tolerances of 39x51 (the larger ones) apply to events / probs / d/dx; the losses are smooth
    functions of those tensors and the pose gradient is linear in d/dx, so the same relative-to-maximum bound carries
    over with the two tensors' errors added (events and probs enter the event image as a product)."""
    from tests.test_hip_event import _setup
    from tests.util import load
    E = _E()
    fx = load("tiny_event_iter")
    tol = C.tolerance('39x51', 'events') + C.tolerance('39x51', 'probs') + C.tolerance('39x51', 'gx')
    out = {}
    for kind in ('torch', 'hip'):
        trk, img, dev = _setup(fx)
        if kind == 'hip':
            trk.event_net = E.event.compile_event_net(trk.event_net)
        idx = torch.from_numpy(fx['idx']).to(dev)
        monkeypatch.setattr(torch, 'randint', lambda *a, **k: idx)
        sf = float(fx['scale_factor'])
        ct = torch.from_numpy(fx['camera_tensor']).to(dev).requires_grad_(True)
        frame = trk.prepare_event_frame(img['gt_event'], img['gt_mask'], img['pre_gt_color'], sf)
        o = trk.iteration_losses(ct, img['gt_color'], img['gt_depth'], frame, int(fx['batch_size']), False, True, sf)
        o['total'].backward()
        out[kind] = (o['event'].item(), o['mask'].item(), ct.grad.cpu().double().numpy())
    (le0, lm0, g0), (le1, lm1, g1) = out['torch'], out['hip']
    print(f"event loss {le0} / {le1}, mask loss {lm0} / {lm1}, pose gradient error {np.abs(g1 - g0).max() / np.abs(g0).max():.3e}, tol {tol:.3e}")
    assert abs(le1 - le0) <= tol * abs(le0)
    assert abs(lm1 - lm0) <= tol * abs(lm0)
    assert np.abs(g1 - g0).max() <= tol * np.abs(g0).max()


def test_abi_error_codes():
    lib = _lib()
    E = _E()
    buf = torch.zeros(1 << 16, device=DEV)
    p, st = buf.data_ptr(), _stream()
    EINVAL, EUNSUPPORTED = -1, -3
    assert lib.enslam_eventnet_forward(None, p, 16, 16, p, p, p, st) == EINVAL
    assert lib.enslam_eventnet_forward(p, p, 16, 16, None, p, p, st) == EINVAL
    assert lib.enslam_eventnet_forward(p, p, 15, 16, p, p, p, st) == EINVAL
    assert lib.enslam_eventnet_forward(p, p, 16, 15, p, p, p, st) == EINVAL
    assert lib.enslam_eventnet_backward(p, p, None, p, p, 16, 16, st) == EINVAL
    assert lib.enslam_eventnet_backward(p, p, p, p, p, 15, 16, st) == EINVAL
    assert lib.enslam_eventnet_workspace_floats(15, 16) == 0
    conv = lambda C0, C1, Cn, w=p, a1=None: lib.enslam_eventnet_conv3x3(w, None, 4, 4, C0, C1, 3, 3, 0, 0, Cn, p, a1, p, None, 0, 0, p,
                                                                      buf.numel(), st)
    assert conv(8, 0, 8, w=None) == EINVAL
    assert conv(6, 0, 64) == EUNSUPPORTED and conv(64, 0, 60) == EUNSUPPORTED and conv(1024, 64, 64) == EUNSUPPORTED
    assert conv(8, 8, 8) == EINVAL                      # a second source is announced but missing
    assert lib.enslam_eventnet_pool2(None, 4, 4, 8, None, p, 0, st) == EINVAL
    assert lib.enslam_eventnet_pool2(p, 4, 4, 8, None, p, 1, st) == EINVAL
    assert lib.enslam_eventnet_up2(p, 0, 4, 8, p, 0, st) == EINVAL
    torch.cuda.synchronize()
    assert not buf.any()                                # nothing was launched
    assert lib.enslam_abi_version() == 1
