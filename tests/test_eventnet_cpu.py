"""No GPU: the host side of the device event network (event.compile_event_net, csrc/event_net.hip) -- BatchNorm folding,
the packed weight layouts of both directions restated in numpy, the wrapper's refusals, and the recorded tolerances."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import eventnet_cases as C


def _E():
    import evennicer_slam_amd as E
    return E


def test_folded_weights_reproduce_the_module_in_float64():
    E = _E()
    net = C.make_net(3)
    folded = E.event.fold_event_net(net)
    assert len(folded) == 26
    assert tuple((w.shape[1], w.shape[0]) for w, _ in folded) == ((6, 64),) + E.event.EVENTNET_CONVS[1:]
    heads = [(getattr(net, f'outc_{h}').conv.weight.double(), getattr(net, f'outc_{h}').conv.bias.double()) for h in (1, 2)]
    x, _, _ = C.make_inputs((17, 19), 3)
    with torch.no_grad():
        e0, p0 = net.double()(x.double())
        e1, p1 = C.folded_forward(folded, heads, x.double())
    for a, b in ((e0, e1), (p0, p1)):
        assert float((a - b).abs().max() / a.abs().max()) <= 1e-12
    # BN is not the identity in these nets: unfolded convolutions alone miss by far
    raw = [(m.weight.double(), None) for m in net.modules() if isinstance(m, torch.nn.Conv2d) and m.kernel_size == (3, 3)]
    with torch.no_grad():
        e2, _ = C.folded_forward(raw, heads, x.double())
    assert float((e0 - e2).abs().max() / e0.abs().max()) > 1e-2


@pytest.mark.parametrize("cin,cout", [(6, 64), (64, 128)])
def test_packed_layouts_reproduce_a_convolution_and_its_input_gradient(cin, cout):
    """pack_conv's forward rows give conv2d, its transposed rows give conv2d's input gradient -- through the SAME
    channels-last restatement (np_conv3x3) the kernel implements."""
    E = _E()
    gen = torch.Generator().manual_seed(5)
    w = torch.randn(cout, cin, 3, 3, generator=gen)
    b = torch.randn(cout, generator=gen)
    H, W = 5, 7
    x = torch.randn(1, cin, H, W, generator=gen).double().requires_grad_(True)
    g = torch.randn(1, cout, H, W, generator=gen).double()
    y = F.conv2d(x, w.double(), b.double(), padding=1)
    y.backward(g)
    cp = cin + (-cin) % 8
    packed = E.event.pack_conv(w, b).numpy()
    n = 9 * cp * cout
    assert packed.shape == (2 * n + cout,)
    wf, bias, wt = packed[:n].reshape(9 * cp, cout), packed[n:n + cout], packed[n + cout:].reshape(9 * cout, cp)
    x_cl = np.zeros((H, W, cp))
    x_cl[..., :cin] = x.detach().numpy()[0].transpose(1, 2, 0)
    got = C.np_conv3x3(wf, bias, x_cl)
    assert np.abs(got - y.detach().numpy()[0].transpose(1, 2, 0)).max() <= 1e-12 * np.abs(got).max()
    gx = C.np_conv3x3(wt, None, g.numpy()[0].transpose(1, 2, 0))
    assert np.abs(gx[..., :cin] - x.grad.numpy()[0].transpose(1, 2, 0)).max() <= 1e-12 * np.abs(gx).max()
    assert not gx[..., cin:].any()


def test_pack_matches_the_library_size_and_order():
    E = _E()
    import __graft_entry__ as G
    G.build()
    net = C.make_net(1)
    packed = E.event.pack_event_net(net)
    assert packed.dtype == torch.float32 and packed.dim() == 1
    assert packed.numel() == E._lib.lib().enslam_eventnet_pack_floats()
    assert packed.numel() == sum(2 * 9 * a * b + b for a, b in E.event.EVENTNET_CONVS) + E.event.EVENTNET_HEADS_FLOATS
    # the heads block closes the image
    assert torch.equal(packed[-264:-264 + 128], net.outc_1.conv.weight.reshape(-1))
    assert torch.equal(packed[-264 + 256:-264 + 258], net.outc_1.conv.bias)
    assert torch.equal(packed[-264 + 258:-264 + 260], net.outc_2.conv.bias)
    lib = E._lib.lib()
    assert lib.enslam_eventnet_workspace_floats(15, 64) == 0 and lib.enslam_eventnet_workspace_floats(64, 15) == 0
    assert lib.enslam_eventnet_workspace_floats(16, 16) > 0
    # the sizes are part of the contract with allocated workspaces: pinned, region by region rounded to 64 floats
    assert lib.enslam_eventnet_pack_floats() == 50224136
    pinned = {(16, 16): 912896, (17, 19): 1121664, (16, 70): 2687936, (39, 51): 3915072, (180, 240): 57179520,
              (480, 640): 390144000}
    assert {hw: lib.enslam_eventnet_workspace_floats(*hw) for hw in pinned} == pinned
    assert lib.enslam_abi_version() == 1


def test_wrapper_refusals():
    E = _E()
    ev = E.event
    with pytest.raises(NotImplementedError, match="eval"):
        ev.compile_event_net(C.make_net().train())
    with pytest.raises(NotImplementedError, match="bilinear"):
        ev.compile_event_net(ev.UNet_2heads(6, 2, 2, bilinear=False).requires_grad_(False).eval())
    with pytest.raises(NotImplementedError, match=r"UNet_2heads\(6, 2, 2\)"):
        ev.compile_event_net(ev.UNet_2heads(6, 3, 2).requires_grad_(False).eval())
    with pytest.raises(NotImplementedError, match=r"UNet_2heads\(6, 2, 2\)"):
        ev.compile_event_net(ev.UNet_2heads(3, 2, 2).requires_grad_(False).eval())

    class Narrow(ev.UNet_2heads):
        WIDTHS = (32, 64, 128, 256, 512)
    with pytest.raises(NotImplementedError, match="widths"):
        ev.compile_event_net(Narrow(6, 2, 2).requires_grad_(False).eval())
    with pytest.raises(NotImplementedError, match="UNet_2heads only"):
        ev.compile_event_net(torch.nn.Conv2d(6, 2, 3))
    hot = C.make_net()
    hot.up3_2.conv.double_conv[0].weight.requires_grad_(True)
    with pytest.raises(NotImplementedError, match=r"(?s)up3_2.*[Ff]reeze"):
        ev.compile_event_net(hot)
    net = ev.compile_event_net(C.make_net())
    assert isinstance(net, ev.HipUNet2Heads) and isinstance(net, torch.nn.Module)
    with pytest.raises(NotImplementedError, match="HIP device"):
        net(torch.rand(1, 6, 16, 16))


def test_wrapper_refuses_batches_and_small_images():
    """The shape checks come before anything touches the device, so they can be told apart from 'not on a HIP device' only
    with a device tensor; a meta tensor stands in for one here."""
    E = _E()
    net = E.event.compile_event_net(C.make_net())

    class OnDevice(torch.Tensor):
        is_cuda = True
    for shape, what in (((2, 6, 16, 16), "batch 1"), ((1, 6, 15, 16), "H, W >= 16"), ((1, 5, 16, 16), "H, W >= 16")):
        x = torch.empty(shape, device='meta').as_subclass(OnDevice)
        with pytest.raises(NotImplementedError, match=what):
            net(x)


def test_case_conditions():
    """Each whole-net shape exercises what eventnet_cases says it does."""
    def levels(n):
        out = [n]
        for _ in range(4):
            out.append(out[-1] // 2)
        return out
    pads = {k: [sum(1 for a, b in zip(levels(d), levels(d)[1:]) if a != 2 * b) for d in hw] for k, hw in C.NET_SHAPES.items()}
    assert pads['16x16'] == [0, 0] and levels(16)[-1] == 1
    assert pads['17x19'][0] >= 1 and pads['17x19'][1] >= 2 and sum(pads['17x19']) >= 2
    assert C.NET_SHAPES['16x70'][1] > 64 and 16 * 70 > 64             # a 64-pixel tile spans rows, a row spans tiles
    assert C.NET_SHAPES['39x51'] == (39, 51)
    for k, (h, w) in C.NET_SHAPES.items():
        assert h >= 16 and w >= 16
    x, ge, gp = C.make_inputs('17x19')
    assert float(x.min()) >= 0 and float(x.max()) <= 1 and ge.shape == gp.shape == (1, 2, 17, 19)
    bn = [m for m in C.make_net().modules() if isinstance(m, torch.nn.BatchNorm2d)]
    assert len(bn) == 26 and all(float((m.running_mean.abs()).max()) > 0 and float((m.running_var - 1).abs().max()) > 0.1
                                 and float((m.weight - 1).abs().min()) > 0.4 for m in bn)
    assert not any(p.requires_grad for p in C.make_net().parameters())


@pytest.mark.parametrize("shape", list(C.NET_SHAPES))
def test_recorded_float32_errors(shape):
    """Re-measure the float32 module's error against float64 on this CPU; the recorded values (and so the GPU tolerances,
    8x them) must sit within a factor 4 of it, above rounding noise and below the cap."""
    ref = C.reference(shape)
    got = C.run_module(C.make_net(0), *C.make_inputs(shape, 0), torch.float32)
    for q, g, r in zip(('events', 'probs', 'gx'), got, ref):
        measured, recorded = C.rel_max(g, r), C.F32_ERR[shape][q]
        print(f"{shape} {q}: float32 module vs float64 {measured:.3e}, recorded {recorded:.3e}, tolerance {C.tolerance(shape, q):.3e}")
        assert recorded / 4 <= measured <= recorded * 4
        assert C.U / 2 <= recorded and C.tolerance(shape, q) == min(8 * recorded, 1e-5) <= 1e-5


def test_abi_declares_the_event_network():
    E = _E()
    for name in ("enslam_eventnet_pack_floats", "enslam_eventnet_workspace_floats", "enslam_eventnet_forward",
                 "enslam_eventnet_backward", "enslam_eventnet_conv3x3", "enslam_eventnet_pool2", "enslam_eventnet_up2"):
        assert name in E._lib.EXPORTS
    assert E._lib._SIGS["enslam_eventnet_forward"][0] is ctypes.c_int


def test_slam_wiring_is_opt_in():
    """cfg['event']['net_backend'] is absent from the defaults; only 'hip' wraps the caller's net."""
    import inspect
    E = _E()
    from evennicer_slam_amd import slam
    src = inspect.getsource(slam.SLAM.__init__)
    assert "get('net_backend', 'torch') == 'hip'" in src and "compile_event_net" in src
