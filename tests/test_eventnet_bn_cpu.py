"""No GPU: the yardsticks of tests/eventnet_bn_numpy.py against nn.BatchNorm2d in float64 and their bounds against what
float64 numpy itself differs by; the recorded float32 errors and the float64 statement of tests/eventnet_bn_cases.py; the
refusals of event.compile_event_net_batchnorm that need no device; the library's new symbols; both tools' arguments and the
trainer's --bn batch on the torch backend."""
import copy
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

from tests import eventnet_bn_cases as C
from tests import eventnet_bn_numpy as Y

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL_CASES = [(3, 8), (65, 64), (257, 24), (700, 64)]


def _E():
    import evennicer_slam_amd as E
    return E


def _tool(name):
    spec = importlib.util.spec_from_file_location(name + "_tool", os.path.join(ROOT, "tools", name + ".py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    return tool


# ---------------------------------------------------------------------------------------------------------------------
# the yardsticks
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,Cn", SMALL_CASES)
def test_yardstick_is_batchnorm2d_in_float64(M, Cn):
    """Forward, autograd backward and the buffers after two steps (the rows as a [M, C, 1, 1] batch)."""
    k = C.kernel_case(M, Cn)
    bn = torch.nn.BatchNorm2d(Cn, eps=C.EPS, momentum=0.1).double().train()
    with torch.no_grad():
        bn.weight.copy_(torch.from_numpy(k['gamma'].astype(np.float64)))
        bn.bias.copy_(torch.from_numpy(k['beta'].astype(np.float64)))
    z = torch.from_numpy(k['z'].astype(np.float64))[:, :, None, None].requires_grad_(True)
    y = torch.relu(bn(z))
    y.backward(torch.from_numpy(k['g_y'].astype(np.float64))[:, :, None, None])
    mean, var = Y.stats(k['z'])
    y_ref = Y.apply(k['z'], k['gamma'], k['beta'], mean, var, C.EPS)
    g_z, dgamma, dbeta = Y.backward(k['z'], y_ref, k['g_y'], k['gamma'], mean, var, C.EPS)
    close = lambda a, b: np.abs(a - b).max() <= 1e-11 * max(np.abs(b).max(), 1e-30)
    assert close(y_ref, y.detach().numpy()[:, :, 0, 0])
    # the offset channel divides rounding noise of the input by sigma = 1e-2: torch's own formulation differs there by more
    keep = np.arange(Cn) != C.CH_OFFSET
    assert close(g_z[:, keep], z.grad.numpy()[:, keep, 0, 0])
    assert close(dgamma[keep], bn.weight.grad.numpy()[keep]) and close(dbeta, bn.bias.grad.numpy())
    rm, rv = Y.running(np.zeros(Cn), np.ones(Cn), mean, var, M, 0.1)
    assert close(rm, bn.running_mean.numpy()) and close(rv, bn.running_var.numpy())
    z2 = np.ascontiguousarray(k['z'][::-1] * 0.5)
    with torch.no_grad():
        bn(torch.from_numpy(z2.astype(np.float64))[:, :, None, None])
    rm, rv = Y.running(rm, rv, *Y.stats(z2), M, 0.1)
    assert close(rm, bn.running_mean.numpy()) and close(rv, bn.running_var.numpy())
    assert int(bn.num_batches_tracked) == 2


@pytest.mark.parametrize("M,Cn", SMALL_CASES)
def test_bounds_are_above_float64_noise_and_far_below_a_wrong_formula(M, Cn):
    """Each bound is at least what float64 numpy differs from an extended-precision evaluation by, and at most 1e-4 of the
    tensor's maximum, so that a dropped -dbeta / M term, a biased-for-unbiased swap or a missing mask cannot pass."""
    k = C.kernel_case(M, Cn)
    ld = np.longdouble
    mean, var = Y.stats(k['z'])
    y = Y.apply(k['z'], k['gamma'], k['beta'], mean, var, C.EPS).astype(np.float32)

    def check(name, value64, value_ld, bound):
        noise = np.abs(value64.astype(ld) - value_ld).astype(np.float64)
        assert (noise <= bound).all(), name
        assert bound.max() <= 1e-4 * np.abs(value64).max(), name

    mean_ld, var_ld = Y.stats(k['z'], ld)
    b_mean, b_var = Y.stats_bounds(k['z'])
    check('mean', mean, mean_ld, b_mean)
    check('var', var, var_ld, b_var)
    check('y', Y.apply(k['z'], k['gamma'], k['beta'], mean, var, C.EPS), Y.apply(k['z'], k['gamma'], k['beta'], mean, var, C.EPS, dtype=ld),
          Y.apply_bound(k['z'], k['gamma'], k['beta'], mean, var, C.EPS))
    ref = Y.backward(k['z'], y, k['g_y'], k['gamma'], mean, var, C.EPS)
    ref_ld = Y.backward(k['z'], y, k['g_y'], k['gamma'], mean, var, C.EPS, dtype=ld)
    bounds = Y.backward_bounds(k['z'], y, k['g_y'], k['gamma'], mean, var, C.EPS)
    for name, a, b, c in zip(('g_z', 'dgamma', 'dbeta'), ref, ref_ld, bounds):
        check(name, a, b, c)
    # wrong formulas miss the bounds
    gamma64, inv = k['gamma'].astype(np.float64), 1.0 / np.sqrt(var + C.EPS)
    xh = (k['z'] - mean) * inv
    gh = np.where(y > 0, k['g_y'].astype(np.float64), 0.0)
    no_beta_term = (gamma64 * inv) * (gh - xh * (ref[1] / M))
    assert (np.abs(no_beta_term - ref[0]) > bounds[0]).any()
    no_mask = Y.backward(k['z'], None, k['g_y'], k['gamma'], mean, var, C.EPS)
    assert all((np.abs(a - b) > c).any() for a, b, c in zip(no_mask, ref, bounds))
    e2 = (k['z'] ** 2).mean(axis=0, dtype=np.float32) - k['z'].mean(axis=0, dtype=np.float32) ** 2     # E[x^2] - E[x]^2
    assert abs(float(e2[C.CH_OFFSET]) - var[C.CH_OFFSET]) > b_var[C.CH_OFFSET]
    rm, rv = Y.running(np.zeros(Cn), np.ones(Cn), mean, var, M, 0.1)
    b_rm, b_rv = Y.running_bounds(np.zeros(Cn), np.ones(Cn), mean, var, M, 0.1)
    biased = 0.9 * np.ones(Cn) + 0.1 * var
    assert (np.abs(biased - rv) > b_rv).any()


# ---------------------------------------------------------------------------------------------------------------------
# the whole-net references
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(C.NET_CASES))
def test_recorded_float32_errors(case):
    """Re-measures F32_ERR_OUT and F32_ERR_GRAD (a record off by more than 4x fails); the statement with the float64 run's
    own decisions is the plain float64 module to 1e-12; every gradient record is admissible (<= 1.25e-4)."""
    net = C.make_bn_net(case)
    ref = C.reference_train(case)
    f32 = C.run_module_train(net, case, torch.float32)
    got = {'events': max(C.rel_max(f32[s][0], ref[s][0]) for s in range(2)),
           'probs': max(C.rel_max(f32[s][1], ref[s][1]) for s in range(2)),
           'buffers': max(C.rel_max(a, b) for s in range(2) for a, b in zip(f32[s][2], ref[s][2]))}
    print(case, {k: f"{v:.3g}" for k, v in got.items()})
    for k, v in got.items():
        assert C.F32_ERR_OUT[case][k] / 4 <= v <= C.F32_ERR_OUT[case][k] * 4, (k, v)
    g64, gx64, dec = C.statement_grads(net, case, torch.float64)
    m = copy.deepcopy(net).double().train()
    x, ge, gp = C.make_bn_inputs(case)
    xx = x.double().requires_grad_(True)
    e, p = m(xx)
    (e * ge.double()).sum().add((p * gp.double()).sum()).backward()
    plain = {n: q.grad.numpy() for n, q in m.named_parameters()}
    assert max(C.rel_max(g64[n], plain[n]) for n in plain) <= 1e-12 and C.rel_max(gx64, xx.grad.numpy()) <= 1e-12
    g32, gx32, _ = C.statement_grads(net, case, torch.float32, dec)
    errs = C.errors_by_kind(g32, gx32, g64, gx64)
    print(case, {k: f"{errs[k][0]:.3g} ({errs[k][1]})" for k in C.KINDS})
    for k in C.KINDS:
        rec = C.F32_ERR_GRAD[case][k]
        assert rec / 4 <= errs[k][0] <= rec * 4, (k, errs[k])
        assert rec <= C.ADMISSIBLE and C.tolerance_grad(case, k) <= 1e-3


def test_first_max_route_is_max_pool2d():
    gen = torch.Generator().manual_seed(3)
    f = torch.relu(torch.randn(2, 5, 7, 9, generator=gen, dtype=torch.float64))
    f[0, 0, 0:2, 0:2] = 1.5                                              # a tie: the first maximum wins
    route = C.first_max_route(f)
    assert int(route[0, 0, 0, 0]) == 0
    w = torch.stack([f[:, :, ky:6:2, kx:8:2] for ky in (0, 1) for kx in (0, 1)], dim=-1)
    assert torch.equal(torch.gather(w, -1, route[..., None])[..., 0], torch.nn.functional.max_pool2d(f, 2))


# ---------------------------------------------------------------------------------------------------------------------
# the public face without a device
# ---------------------------------------------------------------------------------------------------------------------
def test_refusals_without_a_device():
    E = _E()
    EV = E.event
    net = EV.UNet_2heads(6, 2, 2)
    model = EV.compile_event_net_batchnorm(net)
    assert isinstance(model, EV.HipUNet2HeadsBatchNorm) and model.training and net.training
    assert set(model.state_dict()) == {'net.' + k for k in net.state_dict()}
    assert [id(p) for p in model.parameters()] == [id(p) for p in net.parameters()]
    assert [id(b) for b in model.buffers()] == [id(b) for b in net.buffers()]
    model.eval()
    assert not net.training and not model.training
    model.train()
    assert net.training
    with pytest.raises(NotImplementedError, match="HIP device"):
        model(torch.rand(2, 6, 32, 32))
    with pytest.raises(NotImplementedError, match="bilinear"):
        EV.compile_event_net_batchnorm(EV.UNet_2heads(6, 2, 2, bilinear=False))
    with pytest.raises(NotImplementedError, match=r"UNet_2heads\(6, 2, 2\)"):
        EV.compile_event_net_batchnorm(EV.UNet_2heads(3, 2, 2))

    def with_bn(**kw):
        n = EV.UNet_2heads(6, 2, 2)
        for key, value in kw.items():
            setattr(n.inc.double_conv[1], key, value)
        return n
    with pytest.raises(NotImplementedError, match="momentum"):
        EV.compile_event_net_batchnorm(with_bn(momentum=None))
    with pytest.raises(NotImplementedError, match="track_running_stats"):
        EV.compile_event_net_batchnorm(with_bn(track_running_stats=False))
    with pytest.raises(NotImplementedError, match="affine"):
        EV.compile_event_net_batchnorm(with_bn(affine=False))
    wide = EV.UNet_2heads(6, 2, 2)
    wide.inc = EV._ConvPair(6, 64, 32)
    with pytest.raises(NotImplementedError, match="widths"):
        EV.compile_event_net_batchnorm(wide)
    # the existing routes keep refusing a net in training mode
    with pytest.raises(NotImplementedError, match="eval mode"):
        EV.compile_event_net_trainable(EV.UNet_2heads(6, 2, 2))


def test_library_exports_and_launch_names():
    E = _E()
    from evennicer_slam_amd import functional as EF
    lib = E._lib.lib()
    for name in ('bn_stats', 'bn_apply', 'bn_backward', 'bn_running', 'bn_workspace_floats', 'bn_saved_offset', 'train_forward',
                 'train_backward'):
        assert hasattr(lib, 'enslam_eventnet_' + name), name
    assert {'train_forward', 'train_backward', 'bn_running', 'bn_stats', 'bn_apply', 'bn_backward'} <= set(EF.eventnet_launches)
    assert {'forward', 'backward', 'wgrad', 'heads_wgrad', 'fold_pack'} <= set(EF.eventnet_launches)
    # host arithmetic only: sizes and refusals
    assert lib.enslam_eventnet_bn_workspace_floats(1, 16, 16) == 0 and lib.enslam_eventnet_bn_workspace_floats(9, 32, 32) == 0
    assert lib.enslam_eventnet_bn_workspace_floats(2, 16, 16) > 0
    pinned = {(1, 32, 32): 65201792, (2, 16, 70): 67024128, (3, 16, 32): 65010304, (2, 39, 51): 70895808, (8, 180, 240): 730994048}
    assert {bhw: lib.enslam_eventnet_bn_workspace_floats(*bhw) for bhw in pinned} == pinned
    assert lib.enslam_eventnet_bn_saved_offset(2, 39, 51, 26) == -1
    offs = [lib.enslam_eventnet_bn_saved_offset(2, 39, 51, i) for i in range(26)]
    assert len(set(offs)) == 26 and min(offs) > 0 and max(offs) < lib.enslam_eventnet_bn_workspace_floats(2, 39, 51)
    assert sum(EF.EVENTNET_BN_COUT) == EF.EVENTNET_BN_CHANNELS == 5888
    assert EF.EVENTNET_BN_COUT == tuple(c for _, c in E.event.EVENTNET_CONVS)
    assert [EF.eventnet_conv_level(i) for i in (0, 1, 2, 9, 10, 11, 16, 17, 18, 25)] == [0, 0, 1, 4, 3, 3, 0, 0, 3, 0]


# ---------------------------------------------------------------------------------------------------------------------
# the tools
# ---------------------------------------------------------------------------------------------------------------------
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
    return path


def test_tool_arguments(capsys):
    train, bench = _tool('train_event_net'), _tool('bench_eventnet_train')
    with pytest.raises(SystemExit):
        train.main(['cfg.yaml', '--out', 'x.pth', '--batch-size', '2'])          # above 1 only with --bn batch
    assert "--bn batch" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        train.main(['cfg.yaml', '--out', 'x.pth', '--bn', 'live'])
    capsys.readouterr()
    args = bench.parse_args(['--bn', 'batch', '--batch', '4', '--size', '39x51'])
    assert args.bn == 'batch' and args.batch == 4
    args = bench.parse_args([])
    assert args.bn == 'frozen' and args.batch == 1
    with pytest.raises(SystemExit):
        bench.parse_args(['--batch', '4'])                                       # above 1 only with --bn batch
    with pytest.raises(SystemExit):
        bench.parse_args(['--bn', 'batch', '--batch', '9'])
    capsys.readouterr()


def test_train_tool_with_batch_statistics_on_the_torch_backend(tmp_path, capsys):
    path = _tiny_event_sequence(str(tmp_path))
    out = str(tmp_path / 'net.pth')
    res = _tool('train_event_net').main([path, '--out', out, '--backend', 'torch', '--device', 'cpu', '--epochs', '3', '--lr', '1e-4',
                                         '--scale-factor', '0.5', '--bn', 'batch', '--batch-size', '2'])
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert line['bn'] == 'batch' and line['batch_size'] == 2 and line['pairs'] == 3 and line['steps'] == 3
    assert line['event_size'] == [20, 28] and line['first_loss'] == res['first_loss'] and np.isfinite(line['last_loss'])
    fresh = _E().event.UNet_2heads(6, 2, 2).state_dict()
    state = torch.load(out)
    moved = [k for k in state if k.endswith('running_mean') or k.endswith('running_var')]
    assert len(moved) == 52 and all(not torch.equal(state[k], fresh[k]) for k in moved)
    assert all(int(v) == 3 for k, v in state.items() if k.endswith('num_batches_tracked'))
    net = _E().event.UNet_2heads(6, 2, 2)
    net.load_state_dict(state)
