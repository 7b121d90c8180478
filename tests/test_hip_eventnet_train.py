"""-m gpu: event-network training on the device (csrc/event_net.hip: conv3x3_wgrad_kernel, heads_wgrad_kernel,
enslam_eventnet_backward_weights; event.compile_event_net_trainable) -- the single weight gradient through the C ABI
against float64 numpy with a derived bound, determinism, the whole net's parameter gradients against the float64 module
on the CPU, bit-equality with the frozen route, repacking after a step, subsets of trainable parameters, an overfit
control against the torch module, the two tools end to end and the ABI's error codes.  Cases and tolerances: tests/eventnet_train_cases.py."""
import copy
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import eventnet_train_cases as T

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


_scratch = {}


def _wgrad(H, W, C0, C1, H1, W1, oy, ox, Cn, a0, a1, g, saved, dw, db):
    if 'buf' not in _scratch:
        _scratch['buf'] = torch.empty(1 << 22, dtype=torch.float32, device=DEV)       # the header: always suffices
    scratch = _scratch['buf']
    p = lambda t: None if t is None else t.data_ptr()
    code = _lib().enslam_eventnet_conv3x3_wgrad(H, W, C0, C1, H1, W1, oy, ox, Cn, p(a0), p(a1), p(g), p(saved), p(dw), p(db),
                                                p(scratch), scratch.numel(), _stream())
    torch.cuda.synchronize()
    return code


# ---------------------------------------------------------------------------------------------------------------------
# one weight gradient against float64 numpy with the derived bound
#   |dW - exact| <= gamma_{P+2} sum_p |in G|,   |db - exact| <= gamma_P sum_p |G|,   gamma_n = n u / (1 - n u),
# P = H W the reduction length: it holds for any summation order of P products (Higham, Accuracy and Stability, 3.1).
# ---------------------------------------------------------------------------------------------------------------------
PIXELS = [(1, 1), (2, 3), (6, 11), (9, 13), (17, 19)]
CHANNELS = [(8, 0, 64), (64, 0, 64), (128, 64, 64), (512, 0, 512), (1024, 0, 512)]
# The pixel axis is split when the weight block has fewer than 256 tiles of 64 x 64 (and more than one chunk of 32 pixels):
#   216 -> 512 has 31 x 8 = 248 tiles (split), 224 -> 512 has 32 x 8 = 256 (not split);
#   46 x 45 pixels, 64 -> 64: 65 chunks over 33 splits of 2, the last split has one chunk, and that chunk 22 pixels;
#   8 -> 128: two N tiles and a partial last M tile (72 rows).
EXTRA = [((9, 13), (216, 0, 512)), ((9, 13), (224, 0, 512)), ((46, 45), (64, 0, 64)), ((9, 13), (8, 0, 128))]


def _wgrad_case(H, W, C0, C1, Cn, off, with_saved=True, with_db=True):
    rng = np.random.default_rng(1000 * H + 10 * W + C0 + C1 + Cn + off)
    H1, W1 = (max(1, H - 1), max(1, W - 1)) if C1 else (0, 0)
    f32 = lambda *s: rng.standard_normal(s).astype(np.float32)
    x0 = f32(H, W, C0)
    x1 = f32(H1, W1, C1) if C1 else None
    g, saved = f32(H, W, Cn), f32(H, W, Cn)
    saved[rng.random(saved.shape) < 0.1] = 0.0                      # relu'(0) = 0
    full = x0 if not C1 else np.concatenate([x0, T.place(x1, H, W, off, off)], axis=2)
    ref_w, ref_b = T.np_conv3x3_wgrad(full, g, saved if with_saved else None)
    gm = np.abs(g) if not with_saved else np.where(saved > 0, np.abs(g), 0.0)
    bound_w, bound_b = T.np_conv3x3_wgrad(np.abs(full), gm)
    P = H * W
    bound_w, bound_b = T.gamma(P + 2) * bound_w, T.gamma(P) * bound_b
    dw = torch.full((9 * (C0 + C1), Cn), float('nan'), device=DEV)
    db = torch.full((Cn,), float('nan'), device=DEV) if with_db else None
    code = _wgrad(H, W, C0, C1, H1, W1, off, off, Cn, _dev(x0), _dev(x1) if C1 else None, _dev(g),
                  _dev(saved) if with_saved else None, dw, db)
    assert code == 0
    got_w = dw.cpu().numpy().astype(np.float64)
    assert np.isfinite(got_w).all()
    worst = float((np.abs(got_w - ref_w) / np.maximum(bound_w, 1e-300)).max())
    worst_b = 0.0
    assert (np.abs(got_w - ref_w) <= bound_w).all()
    if with_db:
        got_b = db.cpu().numpy().astype(np.float64)
        assert np.isfinite(got_b).all()
        worst_b = float((np.abs(got_b - ref_b) / np.maximum(bound_b, 1e-300)).max())
        assert (np.abs(got_b - ref_b) <= bound_b).all()
    print(f"wgrad {H}x{W} {C0}+{C1}->{Cn} off {off}: error / bound dW {worst:.3f}, db {worst_b:.3f}")


@pytest.mark.parametrize("chan", CHANNELS, ids=lambda c: f"{c[0]}+{c[1]}to{c[2]}")
@pytest.mark.parametrize("pix", PIXELS, ids=lambda p: f"{p[0]}x{p[1]}")
def test_conv3x3_wgrad(pix, chan):
    (H, W), (C0, C1, Cn) = pix, chan
    offsets = (0, 1) if C1 and min(H, W) > 1 else (0,)
    for off in offsets:
        _wgrad_case(H, W, C0, C1, Cn, off)


@pytest.mark.parametrize("pix,chan", EXTRA, ids=["248tiles-split", "256tiles-unsplit", "short-last-split", "two-n-tiles-partial-m"])
def test_conv3x3_wgrad_split_edges(pix, chan):
    _wgrad_case(pix[0], pix[1], chan[0], chan[1], chan[2], 0)


def test_conv3x3_wgrad_without_mask_and_bias():
    _wgrad_case(6, 11, 64, 0, 64, 0, with_saved=False, with_db=False)


@pytest.mark.parametrize("chan", [(64, 64), (512, 512)], ids=["split", "unsplit"])
def test_conv3x3_wgrad_is_deterministic(chan):
    rng = np.random.default_rng(3)
    H, W, (C0, Cn) = 9, 13, chan
    x, g, saved = (_dev(rng.standard_normal(s)) for s in ((H, W, C0), (H, W, Cn), (H, W, Cn)))
    outs = []
    for _ in range(2):
        dw, db = torch.empty((9 * C0, Cn), device=DEV), torch.empty((Cn,), device=DEV)
        assert _wgrad(H, W, C0, 0, 0, 0, 0, 0, Cn, x, None, g, saved, dw, db) == 0
        outs.append((dw.cpu(), db.cpu()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


# ---------------------------------------------------------------------------------------------------------------------
# whole net
# ---------------------------------------------------------------------------------------------------------------------
def _trainable(seed=0):
    E = _E()
    base = T.make_trainable_net(seed).to(DEV)
    return E.event.compile_event_net_trainable(base), base


def _run(tnet, shape, seed=0):
    """(events, probs, gx, {name: gradient}) of one forward + backward, on the CPU"""
    x, ge, gp = (t.to(DEV) for t in T.make_inputs(shape, seed))
    x.requires_grad_(True)
    tnet.zero_grad(set_to_none=True)
    e, p = tnet(x)
    torch.autograd.backward([e, p], [ge, gp])
    torch.cuda.synchronize()
    grads = {n: q.grad.detach().cpu() for n, q in tnet.net.named_parameters() if q.grad is not None}
    return e.detach().cpu(), p.detach().cpu(), x.grad.cpu(), grads


def _check_grads(shape, grads, gx, ref, ref_gx, what):
    from tests import eventnet_cases as C
    errs = T.errors_by_kind({n: g.numpy() for n, g in grads.items()}, ref)
    e_gx = T.rel_max(gx.numpy(), ref_gx)
    print(f"{shape} {what}: HIP vs float64 module " + ", ".join(f"{k} {e:.3e} ({n}; tol {T.tolerance(shape, k):.3e})"
                                                                for k, (e, n) in errs.items())
          + f", gx {e_gx:.3e} (tol {C.tolerance(shape, 'gx'):.3e})")
    for k, (e, n) in errs.items():
        assert e <= T.tolerance(shape, k), (k, n, e)
    assert e_gx <= C.tolerance(shape, 'gx')


@pytest.mark.parametrize("shape", list(T.NET_SHAPES))
def test_whole_net_parameter_gradients(shape):
    from evennicer_slam_amd import functional as EF
    E = _E()
    ref, ref_gx = T.reference_params(shape)
    tnet, base = _trainable()
    before = dict(EF.eventnet_launches)
    e, p, gx, grads = _run(tnet, shape)
    assert EF.eventnet_launches['wgrad'] == before['wgrad'] + 1
    assert set(grads) == set(ref) and all(grads[n].shape == ref[n].shape for n in ref)
    assert all(bool(torch.isfinite(g).all()) for g in grads.values())
    _check_grads(shape, grads, gx, ref, ref_gx, "all parameters")
    # the frozen route on the same weights: one forward and one input gradient to the bit
    frozen = E.event.compile_event_net(T.make_net(0))
    x, ge, gp = (t.to(DEV) for t in T.make_inputs(shape))
    x.requires_grad_(True)
    e0, p0 = frozen(x)
    torch.autograd.backward([e0, p0], [ge, gp])
    assert torch.equal(e0.detach().cpu(), e) and torch.equal(p0.detach().cpu(), p) and torch.equal(x.grad.cpu(), gx)
    with torch.no_grad():
        assert torch.equal(tnet.packed(torch.device(DEV)).cpu(), E.event.pack_event_net(T.make_net(0)))
    # two backward passes are bit-equal
    e2, p2, gx2, grads2 = _run(tnet, shape)
    assert torch.equal(e2, e) and torch.equal(p2, p) and torch.equal(gx2, gx)
    assert all(torch.equal(grads2[n], grads[n]) for n in grads)


def test_packs_on_the_device_equal_the_host_pack_and_each_other():
    """Both device packs -- the torch operations of pack_event_net_differentiable and the fused fold_pack the trainable
    route uses -- are bit-equal to pack_event_net; for a random g_packed their chain rules agree: dw and dbeta to the bit
    (the same float64 product rounded once; a copy), dgamma within 2 u of its maximum (a float64 sum of up to 9 216
    products in another order, rounded once to float32)."""
    from evennicer_slam_amd import functional as EF
    E = _E()
    dev = torch.device(DEV)
    want = E.event.pack_event_net(T.make_net(3))
    out = {}
    for kind in ('torch', 'fused'):
        tnet, base = _trainable(3)
        before = EF.eventnet_launches['fold_pack']
        packed = E.event.pack_event_net_differentiable(base, dev) if kind == 'torch' else tnet.packed(dev)
        assert EF.eventnet_launches['fold_pack'] == before + (kind == 'fused')
        assert packed.requires_grad and torch.equal(packed.detach().cpu(), want)
        g = torch.randn(packed.numel(), generator=torch.Generator().manual_seed(4)).to(DEV)
        packed.backward(g)
        torch.cuda.synchronize()
        out[kind] = {n: q.grad.cpu() for n, q in base.named_parameters()}
    assert set(out['torch']) == set(out['fused'])
    for n, a in out['torch'].items():
        b = out['fused'][n]
        if T.kind_of(n) == 'bn_gamma':
            assert float((a - b).abs().max()) <= 2 * T.U * float(a.abs().max()), n
        else:
            assert torch.equal(a, b), n


def test_fold_pack_backward_sees_an_in_place_update_and_serves_the_heads_alone():
    """The fold saves its inputs through autograd: a parameter changed in place between forward and backward is an error,
    not a gradient from other weights.  With only the heads requiring gradients their gradients are the block's slices."""
    dev = torch.device(DEV)
    tnet, base = _trainable(3)
    packed = tnet.packed(dev)
    with torch.no_grad():
        base.inc.double_conv[1].weight.mul_(2.0)
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        packed.sum().backward()
    tnet, base = _trainable(3)
    base.requires_grad_(False)
    for h in (base.outc_1, base.outc_2):
        h.requires_grad_(True)
    g = torch.randn(tnet.packed(dev).numel(), generator=torch.Generator().manual_seed(4)).to(DEV)
    tnet.packed(dev).backward(g)
    assert torch.equal(base.outc_1.conv.weight.grad.reshape(-1), g[-264:-136])
    assert torch.equal(base.outc_2.conv.weight.grad.reshape(-1), g[-136:-8])
    assert torch.equal(base.outc_1.conv.bias.grad, g[-8:-6]) and torch.equal(base.outc_2.conv.bias.grad, g[-6:-4])
    assert all(q.grad is None for n, q in base.named_parameters() if not n.startswith('outc_'))


def test_gradients_follow_the_weights_after_a_step():
    shape = '17x19'
    tnet, base = _trainable()
    _, _, _, g1 = _run(tnet, shape)
    x, ge, gp = (t.to(DEV) for t in T.make_inputs(shape))
    opt = torch.optim.SGD(tnet.parameters(), lr=1e-5)
    opt.step()                                                      # on the gradients _run has left
    _, _, gx2, g2 = _run(tnet, shape)
    cpu = copy.deepcopy(base).cpu()
    ref, ref_gx = T.run_module_params(cpu, *T.make_inputs(shape), torch.float64)
    _check_grads(shape, g2, gx2, ref, ref_gx, "after one SGD step")
    # the step was large enough to tell: against the first step's gradients the same check fails by far
    stale = T.errors_by_kind({n: g.numpy() for n, g in g1.items()}, ref)
    assert all(e > 10 * T.tolerance(shape, k) for k, (e, _) in stale.items()), stale


def test_only_the_heads_require_gradients():
    from evennicer_slam_amd import functional as EF
    shape = '17x19'
    ref, ref_gx = T.reference_params(shape)
    tnet, base = _trainable()
    base.requires_grad_(False)
    for h in (base.outc_1, base.outc_2):
        h.requires_grad_(True)
    before = dict(EF.eventnet_launches)
    e, p, gx, grads = _run(tnet, shape)
    assert EF.eventnet_launches['wgrad'] == before['wgrad']          # no convolution weight gradient was launched
    assert EF.eventnet_launches['heads_wgrad'] == before['heads_wgrad'] + 1
    assert set(grads) == {n for n in ref if n.startswith('outc_')}
    heads_ref = {n: r for n, r in ref.items() if n in grads}
    errs = T.errors_by_kind({n: g.numpy() for n, g in grads.items()}, heads_ref)
    print(f"heads only: {errs}")
    assert errs['heads'][0] <= T.tolerance(shape, 'heads')
    from tests import eventnet_cases as C
    assert T.rel_max(gx.numpy(), ref_gx) <= C.tolerance(shape, 'gx')


def test_nothing_requires_gradients_is_the_frozen_route():
    from evennicer_slam_amd import functional as EF
    E = _E()
    tnet, base = _trainable()
    base.requires_grad_(False)
    frozen = E.event.compile_event_net(T.make_net(0))
    x, ge, gp = (t.to(DEV) for t in T.make_inputs('16x16'))
    before = dict(EF.eventnet_launches)
    xa, xb = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
    ea, pa = tnet(xa)
    torch.autograd.backward([ea, pa], [ge, gp])
    assert EF.eventnet_launches['wgrad'] == before['wgrad'] and EF.eventnet_launches['heads_wgrad'] == before['heads_wgrad']
    eb, pb = frozen(xb)
    torch.autograd.backward([eb, pb], [ge, gp])
    assert torch.equal(ea, eb) and torch.equal(pa, pb) and torch.equal(xa.grad, xb.grad)
    assert all(q.grad is None for q in base.parameters())
    # trainable parameters under no_grad: no graph, the same outputs
    base.requires_grad_(True)
    with torch.no_grad():
        ec, pc = tnet(x)
    assert not ec.requires_grad and torch.equal(ec, eb) and torch.equal(pc, pb)


def test_backward_after_another_forward_of_the_same_size():
    tnet, base = _trainable()
    _, _, gx0, g0 = _run(tnet, '16x16')
    x, ge, gp = (t.to(DEV) for t in T.make_inputs('16x16'))
    x.requires_grad_(True)
    tnet.zero_grad(set_to_none=True)
    e, p = tnet(x)
    with torch.no_grad():
        tnet(torch.rand_like(x))
    torch.autograd.backward([e, p], [ge, gp])
    assert torch.equal(x.grad.cpu(), gx0)
    assert all(torch.equal(q.grad.cpu(), g0[n]) for n, q in base.named_parameters())


def test_overfit_one_pair_with_the_torch_module_as_control():
    """20 Adam steps on one 17 x 19 pair with synthetic targets: the loss falls on the HIP route, and on the torch module
    on the same device from the same weights (the control: if it did not, the case would say nothing)."""
    E = _E()
    x = T.make_inputs('17x19', 5)[0].to(DEV)
    gen = torch.Generator().manual_seed(11)
    target = torch.randn(1, 2, 17, 19, generator=gen).to(DEV)
    mask = (torch.rand(1, 17, 19, generator=gen) < 0.3).long().to(DEV)
    out = {}
    for kind in ('hip', 'torch'):
        net = T.make_trainable_net(5).to(DEV)
        model = E.event.compile_event_net_trainable(net) if kind == 'hip' else net
        opt = torch.optim.Adam(net.parameters(), lr=1e-4)
        losses = []
        for _ in range(20):
            opt.zero_grad(set_to_none=True)
            ev, pr = model(x)
            loss = ((ev * pr[:, 1][:, None] - target) ** 2).sum() + F.cross_entropy(pr, mask)
            loss.backward()
            opt.step()
            losses.append(float(loss.detach()))
        out[kind] = losses
    print(f"overfit: hip {out['hip'][0]:.4f} -> {out['hip'][-1]:.4f}, torch {out['torch'][0]:.4f} -> {out['torch'][-1]:.4f}")
    for kind, losses in out.items():
        assert np.isfinite(losses).all() and losses[-1] < losses[0], kind


def test_no_graph_capture_of_a_training_step(monkeypatch):
    """Inside a capture the trainable route raises before anything is launched (the capture itself is stood in for: the
    route asks functional._capturing())."""
    from evennicer_slam_amd import functional as EF
    tnet, base = _trainable()
    x = T.make_inputs('16x16')[0].to(DEV)
    before = dict(EF.eventnet_launches)
    monkeypatch.setattr(EF, '_capturing', lambda: True)
    with pytest.raises(RuntimeError, match="graph capture"):
        tnet(x)
    assert EF.eventnet_launches == before


def test_abi_error_codes():
    lib = _lib()
    buf = torch.zeros(1 << 16, device=DEV)
    p, st = buf.data_ptr(), _stream()
    n = buf.numel()
    EINVAL, EUNSUPPORTED = -1, -3
    bw = lib.enslam_eventnet_backward_weights
    assert bw(None, p, p, p, p, p, p, 1 << 40, 16, 16, st) == EINVAL
    assert bw(p, None, p, p, p, p, p, 1 << 40, 16, 16, st) == EINVAL
    assert bw(p, p, None, p, p, p, p, 1 << 40, 16, 16, st) == EINVAL
    assert bw(p, p, p, None, p, p, p, 1 << 40, 16, 16, st) == EINVAL
    assert bw(p, p, p, p, None, None, p, 1 << 40, 16, 16, st) == EINVAL      # g_x may be NULL, g_packed may not
    assert bw(p, p, p, p, p, p, None, 1 << 40, 16, 16, st) == EINVAL
    assert bw(p, p, p, p, p, p, p, 1 << 40, 15, 16, st) == EINVAL
    assert bw(p, p, p, p, p, p, p, 1 << 40, 16, 15, st) == EINVAL
    assert bw(p, p, p, p, p, p, p, lib.enslam_eventnet_wgrad_scratch_floats(16, 16) - 1, 16, 16, st) == EINVAL
    assert lib.enslam_eventnet_wgrad_scratch_floats(15, 16) == 0 and lib.enslam_eventnet_wgrad_scratch_floats(16, 16) > 0
    hw = lib.enslam_eventnet_heads_wgrad
    assert hw(None, p, p, p, p, n, 16, 16, st) == EINVAL and hw(p, p, p, None, p, n, 16, 16, st) == EINVAL
    assert hw(p, p, p, p, p, n, 15, 16, st) == EINVAL and hw(p, p, p, p, p, 259, 16, 16, st) == EINVAL
    wg = lambda C0, C1, Cn, a0=p, a1=None, g=p, dw=p, H=4, W=4, fl=n: lib.enslam_eventnet_conv3x3_wgrad(
        H, W, C0, C1, 3, 3, 0, 0, Cn, a0, a1, g, None, dw, None, p, fl, st)
    assert wg(8, 0, 8, a0=None) == EINVAL and wg(8, 0, 8, g=None) == EINVAL and wg(8, 0, 8, dw=None) == EINVAL
    assert wg(8, 0, 8, H=0) == EINVAL
    assert wg(6, 0, 64) == EUNSUPPORTED and wg(64, 0, 60) == EUNSUPPORTED and wg(1024, 64, 64) == EUNSUPPORTED
    assert wg(8, 8, 8) == EINVAL                        # a second source is announced but missing
    assert wg(64, 0, 64, H=9, W=13, fl=16) == EINVAL    # a split shape with too little scratch
    torch.cuda.synchronize()
    assert not buf.any()                                # nothing was launched
    assert lib.enslam_abi_version() == 1


# ---------------------------------------------------------------------------------------------------------------------
# the tools end to end: train on a written sequence with the HIP route, run the harness with the checkpoint
# ---------------------------------------------------------------------------------------------------------------------
def _load_tool(name):
    import importlib.util
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location(name + "_tool", os.path.join(root, "tools", name + ".py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    return tool


def test_train_tool_on_the_hip_backend_and_run_slam_with_its_checkpoint(tmp_path, capsys, monkeypatch):
    """tools/train_event_net.py --backend hip on 5 frames of the analytic room (48 x 64, events = the thresholded
    log-intensity difference, event size 24 x 32) writes a state_dict; tools/run_slam.py --event-net --net-backend hip runs
    3 frames with it as the harness's event network, wrapped by the frozen device route, and leaves finite poses."""
    import json
    import os
    import yaml
    from evennicer_slam_amd import datasets as D
    from evennicer_slam_amd import slam as S
    from evennicer_slam_amd.scene import scene_bound
    from evennicer_slam_amd.synthetic import BoxRoom, demo_config, trajectory
    E = _E()
    cam = dict(H=48, W=64, fx=51.73, fy=51.65, cx=31.86, cy=25.53)
    room = BoxRoom.for_bound(scene_bound([[-1.0, 1.1], [-0.9, 0.8], [-0.7, 0.6]], 1.0, 0.32), margin=0.12, seed=1)
    poses = trajectory(room, 5, step=0.03, yaw_deg=1.5)
    frames, events = [], []
    for i, c2w in enumerate(poses):
        col, dep = room.render(c2w.double(), cam)
        frames.append((col.numpy(), dep.numpy()))
        if i:
            d = np.log(frames[i][0].mean(-1) + 1e-3) - np.log(frames[i - 1][0].mean(-1) + 1e-3)
            events.append(np.stack([d < -0.1, d > 0.1], axis=-1).astype(np.uint8))
    assert all(e.any() for e in events)
    inp, evf = D.write_replica_event_sequence(str(tmp_path), frames, [p.numpy() for p in poses], 6553.5, events)
    cfg = demo_config(inp, evf, cam, device=DEV, env={'ITERS_FIRST': 20, 'MAP_ITERS': 5, 'TRACK_ITERS': 2, 'EVERY': 1,
                                                      'MAP_PIXELS': 200, 'TRACK_PIXELS': 200})
    cfg['event']['activate_events'] = True
    cfg['data']['output'] = str(tmp_path / 'out')
    path = str(tmp_path / 'seq.yaml')
    with open(path, 'w') as f:
        yaml.safe_dump(cfg, f)
    ck = str(tmp_path / 'eventnet.pth')
    _load_tool('train_event_net').main([path, '--out', ck, '--backend', 'hip', '--device', DEV, '--epochs', '3', '--calibrate', '4',
                                        '--scale-factor', '0.5'])
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    print(f"train_event_net.py (hip): loss {line['first_loss']:.4f} -> {line['last_loss']:.4f}, {line['seconds_per_step'] * 1e3:.1f} ms per step")
    assert line['backend'] == 'hip' and line['pairs'] == 4 and line['steps'] == 12 and line['event_size'] == [24, 32]
    assert np.isfinite(line['last_loss']) and line['last_loss'] < line['first_loss']
    state = torch.load(ck)
    E.event.UNet_2heads(6, 2, 2).load_state_dict(state)

    seen = {}
    init = S.SLAM.__init__

    def spy(self, *a, **k):
        init(self, *a, **k)
        seen['event_net'] = self.event_net
    monkeypatch.setattr(S.SLAM, '__init__', spy)
    res = _load_tool('run_slam').main([path, '--max-frames', '3', '--event-net', ck, '--net-backend', 'hip', '--device', DEV])
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert line['frames'] == 3 and os.path.isfile(line['ckpt']) and np.isfinite(line['ate_rmse'])
    net = seen['event_net']
    assert isinstance(net, E.event.HipUNet2Heads) and not net.net.training
    assert not any(q.requires_grad for q in net.net.parameters())
    assert all(torch.equal(v.cpu(), state[k]) for k, v in net.net.state_dict().items())
    ckpt = torch.load(res['ckpt'], map_location='cpu', weights_only=False)
    assert bool(torch.isfinite(ckpt['estimate_c2w_list'][:3]).all())
