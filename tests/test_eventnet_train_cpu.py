"""No GPU: the host side of event-network training (event.compile_event_net_trainable, csrc/event_net.hip:
enslam_eventnet_backward_weights) -- the recorded tolerances, the differentiable pack and its closed-form gradients, the
numpy restatement of the weight gradient, the ABI's declarations, the wrapper's refusals and tools/train_event_net.py on
the torch backend."""
import ctypes
import importlib.util
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import eventnet_train_cases as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _E():
    import evennicer_slam_amd as E
    return E


@pytest.mark.parametrize("shape", list(T.NET_SHAPES))
def test_recorded_float32_errors(shape):
    """Re-measure the float32 module's parameter-gradient errors against float64 on this CPU: the recorded values (and so
    the GPU tolerances, 8x them) must sit within a factor 4 of them, and 8x every recorded value below the cap."""
    ref, ref_gx = T.reference_params(shape)
    assert all(np.abs(r).max() > 0 for r in ref.values())          # no parameter tensor has an all-zero gradient
    got, _ = T.run_module_params(T.make_net(0), *T.make_inputs(shape, 0), torch.float32)
    errs = T.errors_by_kind(got, ref)
    assert set(errs) == set(T.KINDS)
    for kind, (measured, name) in errs.items():
        recorded = T.F32_ERR_PARAMS[shape][kind]
        print(f"{shape} {kind}: float32 module vs float64 {measured:.3e} ({name}), recorded {recorded:.3e}, "
              f"tolerance {T.tolerance(shape, kind):.3e}")
        assert recorded / 4 <= measured <= recorded * 4
        assert T.U / 2 <= recorded and T.tolerance(shape, kind) == 8 * recorded < T.TOL_CAP == 1e-4
        assert measured <= T.TOL_CAP                                # the reference alone stays inside the cap


def test_parameter_kinds():
    names = [n for n, _ in T.make_net().named_parameters()]
    kinds = [T.kind_of(n) for n in names]
    assert kinds.count('conv') == kinds.count('bn_gamma') == kinds.count('bn_beta') == 26 and kinds.count('heads') == 4
    assert T.kind_of('up3_1.conv.double_conv.0.weight') == 'conv' and T.kind_of('down3.maxpool_conv.1.double_conv.4.bias') == 'bn_beta'


def test_differentiable_pack_is_bit_equal_to_the_host_pack():
    ev = _E().event
    for seed in (0, 1):
        net = T.make_trainable_net(seed)
        got = ev.pack_event_net_differentiable(net, 'cpu')
        assert got.requires_grad and got.dtype == torch.float32
        assert torch.equal(got.detach(), ev.pack_event_net(net))
    frozen = T.make_net(2)
    got = ev.pack_event_net_differentiable(frozen, 'cpu')
    assert not got.requires_grad and torch.equal(got, ev.pack_event_net(frozen))


def test_autograd_through_the_pack_equals_the_closed_forms():
    """For a random g_packed: dw = dWf s, dgamma = (sum dWf w - mean db) / sqrt(var + eps), dbeta = db, with
    s = gamma / sqrt(var + eps); the Wt blocks and the pad carry no gradient; the heads block is the heads' own."""
    ev = _E().event
    net = T.make_trainable_net(4)
    packed = ev.pack_event_net_differentiable(net, 'cpu')
    gen = torch.Generator().manual_seed(9)
    g = torch.randn(packed.numel(), generator=gen)
    packed.backward(g)
    g64 = g.double()
    convs = [(p.double_conv[i], p.double_conv[i + 1]) for p in ev._conv_pairs(net) for i in (0, 3)]
    off = 0
    for (conv, bn), (cin, cout) in zip(convs, ev.EVENTNET_CONVS):
        n = 9 * cin * cout
        dwf = g64[off:off + n].reshape(3, 3, cin, cout).permute(3, 2, 0, 1)[:, :conv.in_channels]   # as conv.weight
        db = g64[off + n:off + n + cout]
        off += 2 * n + cout
        sq = torch.sqrt(bn.running_var.double() + bn.eps)
        s = bn.weight.detach().double() / sq
        w = conv.weight.detach().double()
        want = {'w': dwf * s[:, None, None, None],
                'gamma': ((dwf * w).sum(dim=(1, 2, 3)) - bn.running_mean.double() * db) / sq,
                'beta': db}
        for what, got in (('w', conv.weight.grad), ('gamma', bn.weight.grad), ('beta', bn.bias.grad)):
            ref = want[what]
            # float32 results of a float64 chain: one rounding to float32, plus the float64 sum of up to 9 216 products
            assert float((got.double() - ref).abs().max()) <= 2 * T.U * float(ref.abs().max()), what
    heads = g[off:]
    assert off + 264 == packed.numel()
    assert torch.equal(net.outc_1.conv.weight.grad.reshape(-1), heads[:128])
    assert torch.equal(net.outc_2.conv.weight.grad.reshape(-1), heads[128:256])
    assert torch.equal(net.outc_1.conv.bias.grad, heads[256:258]) and torch.equal(net.outc_2.conv.bias.grad, heads[258:260])


def test_np_conv3x3_wgrad_against_float64_autograd():
    ev = _E().event
    gen = torch.Generator().manual_seed(6)
    cin, cout, H, W = 8, 16, 5, 7
    w = torch.randn(cout, cin, 3, 3, generator=gen).double().requires_grad_(True)
    b = torch.randn(cout, generator=gen).double().requires_grad_(True)
    x = torch.randn(1, cin, H, W, generator=gen).double()
    g = torch.randn(1, cout, H, W, generator=gen).double()
    y = F.relu(F.conv2d(x, w, b, padding=1))
    y.backward(g)
    cl = lambda t: t[0].permute(1, 2, 0).numpy()
    dW, db = T.np_conv3x3_wgrad(cl(x), cl(g), cl(y.detach()))
    assert (cl(y.detach()) == 0).any()                              # the mask matters in this case
    n = 9 * cin * cout
    want = ev.pack_conv(w.grad, b.grad).numpy()                     # the forward layout of the gradient
    assert np.abs(dW.reshape(-1) - want[:n]).max() <= 1e-12 * np.abs(want[:n]).max()
    assert np.abs(db - want[n:n + cout]).max() <= 1e-12 * np.abs(db).max()
    dW_all, _ = T.np_conv3x3_wgrad(cl(x), cl(g))
    assert np.abs(dW_all - dW).max() > 1e-3


def test_abi_declares_the_training_entries():
    import __graft_entry__ as G
    G.build()
    E = _E()
    names = ("enslam_eventnet_wgrad_scratch_floats", "enslam_eventnet_backward_weights", "enslam_eventnet_heads_wgrad",
             "enslam_eventnet_conv3x3_wgrad")
    header = open(os.path.join(ROOT, "include", "enslam_hip.h")).read()
    handle = ctypes.CDLL(E.LIB_PATH)
    for name in names:
        assert name in E._lib.EXPORTS and name + "(" in header and hasattr(handle, name)
    assert E._lib._SIGS["enslam_eventnet_backward_weights"][0] is ctypes.c_int
    assert len(E._lib._SIGS["enslam_eventnet_backward_weights"][1]) == 11
    assert len(E._lib._SIGS["enslam_eventnet_conv3x3_wgrad"][1]) == 18
    lib = E._lib.lib()
    assert lib.enslam_eventnet_wgrad_scratch_floats(15, 16) == 0 and lib.enslam_eventnet_wgrad_scratch_floats(16, 15) == 0
    assert lib.enslam_eventnet_wgrad_scratch_floats(102, 180) > 0
    pinned = {(16, 16): 590336, (17, 19): 885120, (16, 70): 1770240, (39, 51): 2360320, (180, 240): 2361344, (480, 640): 2361344}
    assert {hw: lib.enslam_eventnet_wgrad_scratch_floats(*hw) for hw in pinned} == pinned
    from evennicer_slam_amd import functional as EF
    assert {'forward', 'backward', 'wgrad'} <= set(EF.eventnet_launches)


def test_trainable_wrapper_refusals():
    ev = _E().event
    with pytest.raises(NotImplementedError, match="eval"):
        ev.compile_event_net_trainable(T.make_trainable_net().train())
    with pytest.raises(NotImplementedError, match="bilinear"):
        ev.compile_event_net_trainable(ev.UNet_2heads(6, 2, 2, bilinear=False).eval())
    with pytest.raises(NotImplementedError, match=r"UNet_2heads\(6, 2, 2\)"):
        ev.compile_event_net_trainable(ev.UNet_2heads(6, 3, 2).eval())

    class Narrow(ev.UNet_2heads):
        WIDTHS = (32, 64, 128, 256, 512)
    with pytest.raises(NotImplementedError, match="widths"):
        ev.compile_event_net_trainable(Narrow(6, 2, 2).eval())
    base = T.make_trainable_net()
    tnet = ev.compile_event_net_trainable(base)
    assert isinstance(tnet, ev.HipUNet2HeadsTrainable) and isinstance(tnet, torch.nn.Module) and tnet.net is base
    assert [id(p) for p in tnet.parameters()] == [id(p) for p in base.parameters()]
    assert set(tnet.state_dict()) == {'net.' + k for k in base.state_dict()}
    torch.optim.Adam(tnet.parameters())
    with pytest.raises(NotImplementedError, match="eval"):
        tnet.train()
    with pytest.raises(NotImplementedError, match="HIP device"):
        tnet(torch.rand(1, 6, 16, 16))
    base.train()
    with pytest.raises(NotImplementedError, match="eval"):
        tnet(torch.rand(1, 6, 16, 16))
    # the frozen route still refuses what it refused
    with pytest.raises(NotImplementedError, match="[Ff]reeze"):
        ev.compile_event_net(T.make_trainable_net())


def _tiny_event_sequence(root):
    """4 frames of 40 x 56 with events = the thresholded log-intensity difference of consecutive frames, and its YAML."""
    import yaml
    from evennicer_slam_amd import datasets as D
    from evennicer_slam_amd.synthetic import demo_config
    rng = np.random.default_rng(0)
    H, W = 40, 56
    yy, xx = np.mgrid[0:H, 0:W]
    frames, events = [], []
    for k in range(4):
        col = np.stack([0.5 + 0.4 * np.sin(0.3 * xx + 0.9 * k + c) * np.cos(0.25 * yy - 0.5 * k) for c in range(3)], axis=-1)
        frames.append((np.clip(col + 0.01 * rng.standard_normal(col.shape), 0, 1), np.full((H, W), 2.0, dtype=np.float32)))
        if k:
            d = np.log(frames[k][0].mean(-1) + 1e-3) - np.log(frames[k - 1][0].mean(-1) + 1e-3)
            events.append(np.stack([(d < -0.2), (d > 0.2)], axis=-1).astype(np.uint8))
    poses = [np.eye(4) for _ in frames]
    inp, evf = D.write_replica_event_sequence(root, frames, poses, 6553.5, events)
    cam = dict(H=H, W=W, fx=50.0, fy=50.0, cx=W / 2, cy=H / 2)
    cfg = demo_config(inp, evf, cam, device='cpu')
    path = os.path.join(root, 'tiny.yaml')
    with open(path, 'w') as f:
        yaml.safe_dump(cfg, f)
    return path, events


def test_train_tool_on_the_torch_backend(tmp_path, capsys):
    path, events = _tiny_event_sequence(str(tmp_path))
    assert all(e.any() for e in events) and not all(e.all() for e in events)
    spec = importlib.util.spec_from_file_location("train_event_net_tool", os.path.join(ROOT, "tools", "train_event_net.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    out = str(tmp_path / 'net.pth')
    res = tool.main([path, '--out', out, '--backend', 'torch', '--device', 'cpu', '--epochs', '4', '--lr', '1e-4',
                     '--calibrate', '3', '--scale-factor', '0.5'])
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert line['pairs'] == 3 and line['steps'] == 12 and line['event_size'] == [20, 28]
    assert line['first_loss'] == res['first_loss'] and line['seconds_per_step'] > 0
    print(f"train_event_net.py (torch, cpu): loss {line['first_loss']:.4f} -> {line['last_loss']:.4f}")
    assert np.isfinite(line['last_loss']) and line['last_loss'] < line['first_loss']
    net = _E().event.UNet_2heads(6, 2, 2)
    net.load_state_dict(torch.load(out))
    bn = net.inc.double_conv[1]
    assert float((bn.running_var - 1).abs().max()) > 0              # the calibration has set the statistics
