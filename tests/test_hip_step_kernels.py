"""The small launches of every tracker and mapper iteration (csrc/util_kernels.hip: camera tensor -> rays and back, the head of
the tracker's iteration, the two L1 losses, the two Adam kernels, the batch depth maximum) against the numpy yardsticks of
tests/step_numpy.py on the cases of tests/step_cases.py -- never against a second GPU path.  Tolerances are the output
rounding plus the float64 reordering bound on the yardstick's own A; Adam's is the measured one (step_cases.ADAM_TOL)."""
import ctypes

import numpy as np
import pytest
import torch

from tests import step_cases as C
from tests import step_numpy as Y

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
f32 = np.float32
CT_NAMES = tuple(C.CAMERA_TENSORS)


def dev(a, dtype=None):
    t = torch.from_numpy(np.array(a)).to(DEV)                       # a copy: the shared case arrays are read-only
    return t if dtype is None else t.to(dtype)


def host(t):
    torch.cuda.synchronize()
    return t.detach().cpu().numpy()


# ---- camera tensor -> rays and back -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CT_NAMES)
def test_pose_rays_forward(name):
    from evennicer_slam_amd import tracker
    for n in C.N_EDGES:
        c = C.pose_case(name, n)
        ro, rd = tracker.rays_from_camera_tensor(dev(c.ct), dev(c.px.pi), dev(c.px.pj), *C.CAM)
        ro, rd = host(ro), host(rd)
        err = np.abs(rd.astype(np.float64) - c.rd64) / (2.0 ** -24 * c.scale)
        print(f"{name} n={n}: rd bit-equal to the float32 mirror {Y.bits_equal(rd, c.rd)}, within {err.max():.2f} x 2^-24 x scale of float64")
        assert ro.dtype == np.float32 and rd.dtype == np.float32 and ro.shape == rd.shape == (n, 3)
        assert (err <= 8).all()
        assert Y.bits_equal(ro, np.broadcast_to(c.ct[4:7], (n, 3)))
        assert Y.bits_equal(rd, c.rd)


def _check_pose_grad(got, ref, A, n, what):
    got = got.astype(np.float64)
    tol = 2.0 ** -23 * np.abs(ref) + n * 2.0 ** -52 * A
    with np.errstate(divide='ignore', invalid='ignore'):
        print(f"{what}: |got - ref| / tol = {np.where(tol > 0, np.abs(got - ref) / tol, np.abs(got - ref))}")
    assert (np.abs(got - ref) <= tol).all(), what


@pytest.mark.parametrize("name", CT_NAMES)
def test_pose_rays_backward(name):
    """all three thread counts of pose_rays_bwd_kernel (n <= 64, <= 256, more), with both cotangents and each alone"""
    from evennicer_slam_amd import tracker
    for n in C.N_EDGES:
        c = C.pose_case(name, n)
        for which in C.COTANGENTS:
            ct = dev(c.ct).requires_grad_(True)
            ro, rd = tracker.rays_from_camera_tensor(ct, dev(c.px.pi), dev(c.px.pj), *C.CAM)
            g_ro, g_rd = C.cotangents(c.px, which)
            outs = [(o, dev(g)) for o, g in ((ro, g_ro), (rd, g_rd)) if g is not None]
            got = host(torch.autograd.grad([o for o, _ in outs], ct, [g for _, g in outs])[0])
            ref, A = c.grad[which]
            assert got.dtype == np.float32 and got.shape == (7,)
            _check_pose_grad(got, ref, A, n, f"{name} n={n} {which}")
            if g_rd is None:                                    # the translation part alone: fl32(sum g_ro), the quaternion's exactly 0
                assert not got[:4].any()
                assert (np.abs(got[4:].astype(np.float64) - g_ro.astype(np.float64).sum(0)) <= 2.0 ** -23 * np.abs(ref[4:]) + n * 2.0 ** -52 * A[4:]).all()
            if g_ro is None:
                assert not got[4:].any()


# ---- the head of the tracker's iteration ------------------------------------------------------------------------------------
def _tracker_rays(c, color_dtype=torch.float32, prefilter=True, idx=None, counter=None, ct=None):
    import evennicer_slam_amd.functional as EF
    from evennicer_slam_amd.tracker import _TrackerRays
    bound = torch.tensor(C.TR_BOUND, dtype=torch.float64)
    return _TrackerRays.apply(dev(c.ct) if ct is None else ct, dev(c.idx) if idx is None else idx, C.EDGE_H, C.EDGE_W, C.WIN_W,
                              dev(c.depth), dev(c.color, color_dtype), *c.cam, EF.bound6(bound), prefilter, counter)


def _check_tracker_outputs(out, m, what):
    ro, rd, gd, gc, inside, dmax = (host(t) if t is not None else None for t in out)
    print(f"{what}: inside {int(m.inside.sum())} of {len(m.gd)}, dmax {dmax} (yardstick {m.dmax})")
    assert Y.bits_equal(gd, m.gd) and Y.bits_equal(gc, m.gc), what
    assert Y.bits_equal(ro, m.ro) and Y.bits_equal(rd, m.rd), what
    assert inside.dtype == np.uint8 and np.array_equal(inside.astype(bool), m.inside), what
    assert Y.bits_equal(dmax, m.dmax), what


@pytest.mark.parametrize("kind", C.TR_KINDS)
def test_tracker_rays(kind):
    for n in C.TR_N:
        c = C.tracker_case(kind, n)
        for dtype in (torch.float32, torch.float64):
            _check_tracker_outputs(_tracker_rays(c, dtype), c, f"{kind} n={n} {dtype}")
    out = _tracker_rays(c, prefilter=False)                      # no mask: the maxima run over every ray
    assert out[4] is None and Y.bits_equal(host(out[5]), c.dmax_all) and Y.bits_equal(host(out[1]), c.rd)


@pytest.mark.parametrize("color_f64", [0, 1])
def test_tracker_rays_pixels(color_f64):
    """the pixel coordinates the launch keeps for its backward (no Python caller reads them): the C entry by hand"""
    import evennicer_slam_amd as E
    import evennicer_slam_amd.functional as EF
    L, P = E._lib, EF._ptr
    c = C.tracker_case('last_max', 1025)
    n = c.n
    idx, depth, ct = dev(c.idx), dev(c.depth), dev(c.ct)
    color = dev(c.color, torch.float64 if color_f64 else torch.float32)
    new = lambda *shape, dtype=torch.float32: torch.empty(shape, dtype=dtype, device=DEV)
    pi, pj, ro, rd, gd, gc, dmax, inside = new(n), new(n), new(n, 3), new(n, 3), new(n), new(n, 3), new(2), new(n, dtype=torch.uint8)
    bound = EF.bound6(torch.tensor(C.TR_BOUND, dtype=torch.float64))
    fx, fy, cx, cy = (ctypes.c_float(x) for x in c.cam)
    L.check(L.lib().enslam_tracker_rays(n, P(ct), P(idx), C.EDGE_H, C.EDGE_W, C.WIN_W, C.IMG_W, C.IMG_H, P(depth), P(color), color_f64, fx, fy,
                                        cx, cy, bound, 1, P(pi), P(pj), P(ro), P(rd), P(gd), P(gc), P(inside), P(dmax), None, 0,
                                        EF._stream()), "enslam_tracker_rays")
    assert Y.bits_equal(host(pi), c.pi) and Y.bits_equal(host(pj), c.pj)
    _check_tracker_outputs((ro, rd, gd, gc, inside, dmax), c, f"by hand, color_f64={color_f64}")
    gi, gj, gdd, gcc = EF.gather_pixels(idx, C.EDGE_H, C.EDGE_W, C.WIN_W, depth, color)         # the stand-alone gather
    assert Y.bits_equal(host(gi), c.pi) and Y.bits_equal(host(gj), c.pj) and Y.bits_equal(host(gdd), c.gd)
    assert Y.bits_equal(host(gcc).astype(f32), c.gc) and gcc.dtype == color.dtype


def test_tracker_rays_draw_counter_walks_the_table():
    d = C.draw_table()
    idx, counter = dev(d.idx), torch.zeros(1, dtype=torch.int32, device=DEV)
    for call in range(C.DRAW_CALLS):
        out = _tracker_rays(d, idx=idx, counter=counter)
        _check_tracker_outputs(out, d.rows[call % C.N_DRAWS], f"call {call}")
        assert int(counter.item()) == call + 1


def test_tracker_rays_backward():
    t = C.tracker_grad_case()
    c = t.case
    for which in C.COTANGENTS:
        ct = dev(c.ct).requires_grad_(True)
        out = _tracker_rays(c, ct=ct)
        g_ro, g_rd = C.cotangents(t.px, which)
        outs = [(o, dev(g)) for o, g in ((out[0], g_ro), (out[1], g_rd)) if g is not None]
        got = host(torch.autograd.grad([o for o, _ in outs], ct, [g for _, g in outs])[0])
        _check_pose_grad(got, *t.grad[which], c.n, f"tracker rays n={c.n} {which}")


# ---- losses -----------------------------------------------------------------------------------------------------------------
def _ulps64(got, ref):
    return np.abs(got - ref) / np.spacing(np.maximum(np.abs(ref), np.finfo(np.float64).tiny))


@pytest.mark.parametrize("which", ['map', 'trk'])
@pytest.mark.parametrize("kind", C.LOSS_KINDS)
def test_losses(kind, which):
    from evennicer_slam_amd import losses
    for n in C.LOSS_N:
        if n == 0 and kind not in ('random', 'no_color'):
            continue
        c = C.loss_case(kind, n)
        ref, A, ref_gd, ref_gc = getattr(c, which)
        depth = dev(c.depth).requires_grad_(True)
        color = dev(c.color).requires_grad_(True) if c.color is not None else None
        if which == 'map':
            loss = losses.rgbd_loss(depth, color, dev(c.gd), dev(c.gc), C.W_MAPPER)
        else:
            loss = losses.tracker_loss(depth, dev(c.unc), color, dev(c.gd), dev(c.gc), C.W_TRACKER)
        assert loss.dtype == torch.float64
        got = float(loss.item())
        print(f"{which} {kind} n={n}: loss {got!r} yardstick {ref!r}, |diff| {abs(got - ref):.3e}, allowed {max(n, 1) * 2.0 ** -52 * A:.3e}")
        if kind == 'tail':
            assert ref > 0
        assert abs(got - ref) <= max(n, 1) * 2.0 ** -52 * A
        if n == 0 or kind == 'all_zero_no_color':
            assert got == 0.0
        (loss * C.G_UP).backward()
        g_depth = host(depth.grad)
        ulps = _ulps64(g_depth, ref_gd)
        print(f"    g_depth bit-equal {Y.bits_equal(g_depth, ref_gd)}, worst {ulps.max() if n else 0.0:.2f} ulp")
        assert g_depth.dtype == np.float64 and (ulps <= 2).all()
        assert not g_depth[ref_gd == 0].any()                   # masked rays and depth == gt_depth: exactly zero
        if color is None:
            continue
        g_color = host(color.grad)
        assert Y.bits_equal(g_color, ref_gc)
        on = c.gd > 0
        if which == 'trk':
            assert not g_color[~on].any()
        elif n and kind != 'tail':
            assert g_color[~on].any() or on.all()               # the mapper's colour term does not look at the depth


# ---- Adam over tensor lists -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", tuple(C.ADAM_LISTS))
def test_adam_tensors(name):
    from evennicer_slam_amd.mapper import FusedAdam
    c = C.adam_list(name)
    params = [dev(p).requires_grad_(True) for p in c.p0]
    opt = FusedAdam(params, lr=0.0)
    z = C.zero_tensor(c.numels)
    before = [p.copy() for p in c.p0]
    worst = 0.0
    for k, lr in enumerate(C.ADAM_LRS):
        for p, g in zip(params, c.grads):
            p.grad = dev(g[k])
        opt.step(lr)
        assert int(opt.step_t.item()) == k + 1                  # counted by the launch (one workgroup) or by the host
        now = [host(p) for p in params]
        for i, (p, old) in enumerate(zip(now, before)):
            ref = c.ref[i][0][k]
            e = np.abs(p.astype(np.float64) - ref).max() / C.adam_scale(ref, C.ADAM_LRS[:k + 1])
            worst = max(worst, float(e))
            assert e <= C.ADAM_TOL, (name, i, k, e)             # every element (the first and the last of every tensor too)
            if lr == 0.0:
                assert Y.bits_equal(p, old), (name, i, k)
            else:                                               # ... and nothing left behind: whatever the yardstick moves by
                prev = c.ref[i][0][k - 1] if k else c.p0[i].astype(np.float64)          # more than a few ulp has moved
                moved = np.abs(ref - prev) > 4 * np.spacing(np.abs(old))
                assert moved.any() and (p != old)[moved].all(), (name, i, k)
        if k == 1:                                              # zero gradients in both steps so far: no update at lr = 0.005
            assert Y.bits_equal(now[z][C.ZERO_SLICE], c.p0[z][C.ZERO_SLICE])
        before = now
    print(f"{name}: worst distance {worst:.3e} of the allowed {C.ADAM_TOL:.3e} (units of 2^-24 max|p| + sum lr)")
    for i in range(len(params)):
        _, m, v = c.ref[i]
        assert (np.abs(host(opt.exp_avg[i]) - m[-1]) <= C.moment_bound(c.grads[i], 1)).all()
        assert (np.abs(host(opt.exp_avg_sq[i]) - v[-1]) <= C.moment_bound(c.grads[i], 2)).all()


# ---- masked Adam on voxel-major grids ---------------------------------------------------------------------------------------
class _PaddedGrids:
    """mapper.MaskedGridOptimizer over grids of V voxels whose four arrays (values, gradient accumulator, both moments) each
    sit in front of C.PAD voxels of sentinel values"""

    def __init__(self, cases):
        from evennicer_slam_amd.functional import VoxelMajorGrid
        from evennicer_slam_amd.mapper import MaskedGridOptimizer
        self.keys = tuple(f"grid_{k}" for k in range(len(cases)))
        grids = {key: dev(np.ascontiguousarray(c.p0.T).reshape(1, 32, 1, 1, c.V)) for key, c in zip(self.keys, cases)}
        masks = {key: (dev(c.mask).bool().reshape(1, 1, c.V) if c.mask is not None else None) for key, c in zip(self.keys, cases)}
        self.opt = MaskedGridOptimizer(grids, masks, keys=self.keys)
        self.opt.native.clear()
        self.buf = {}
        for key, c in zip(self.keys, cases):
            b = [torch.full((c.V + C.PAD, 32), C.SENTINEL, dtype=torch.float32, device=DEV) for _ in range(4)]
            p, g, m, v = (x[:c.V] for x in b)
            p.copy_(dev(c.p0)), g.zero_(), m.zero_(), v.zero_()
            assert torch.equal(self.opt.grids[key].vm, p)               # (the constructor's own layout conversion agrees)
            self.opt.grids[key] = VoxelMajorGrid((1, 1, c.V), p, g)
            self.opt.m[key], self.opt.v[key] = m, v
            self.buf[key] = b

    def step(self, grads, stepping, lrs):
        for key, g, s in zip(self.keys, grads, stepping):
            self.opt.grids[key].grad_vm.copy_(dev(g))
            self.opt.grids[key].has_grad = self.opt.grids[key].has_grad or s
        self.opt.step(dict(zip(self.keys, lrs)))

    def state(self, key):
        """(p, m, v) float32 [V,32]; checks on the way that the accumulator is cleared and no sentinel was touched"""
        V = self.opt.grids[key].vm.shape[0]
        p, g, m, v = (host(b) for b in self.buf[key])
        assert not g[:V].any(), key
        for a in (p, g, m, v):
            assert (a[V:] == f32(C.SENTINEL)).all(), key
        return p[:V], m[:V], v[:V]


def _check_grid(state, c, ref_step, lrs_so_far, grads_so_far, start, what):
    """state after `ref_step + 1` steps of case c against its yardstick; `start` = the state before the first step"""
    p, m, v = state
    on = np.ones(c.V, bool) if c.mask is None else c.mask.astype(bool)
    for a, b in zip(state, start):
        assert Y.bits_equal(a[~on], b[~on]), what                # masked-out voxels: p, m and v bit-identical
    rp, rm, rv = (r[ref_step] for r in c.ref)
    if on.any():
        e = np.abs(p[on].astype(np.float64) - rp[on]).max() / C.adam_scale(rp, lrs_so_far)
        print(f"{what}: distance {e:.3e} of the allowed {C.ADAM_TOL:.3e}")
        assert e <= C.ADAM_TOL, what
        assert (np.abs(m - rm)[on] <= C.moment_bound(grads_so_far, 1)[on]).all(), what
        assert (np.abs(v - rv)[on] <= C.moment_bound(grads_so_far, 2)[on]).all(), what
        assert m[on].any() and v[on].any()
    if not np.any(lrs_so_far):
        assert Y.bits_equal(p, start[0]), what                   # lr = 0: the moments advance, the values do not move


@pytest.mark.parametrize("mask_kind", C.GRID_MASKS)
@pytest.mark.parametrize("V", C.GRID_V)
def test_adam_masked_alone(V, mask_kind):
    c = C.grid_case(V, mask_kind)
    G = _PaddedGrids([c])
    start = G.state(G.keys[0])
    for k, lr in enumerate(c.lrs):
        G.step([c.grads[k]], [True], [lr])
        assert G.opt.steps == [k + 1] and int(G.opt.step_t.item()) == k + 1
        _check_grid(G.state(G.keys[0]), c, k, c.lrs[:k + 1], c.grads[:k + 1], start, f"V={V} {mask_kind} step {k + 1}")


def test_adam_masked_four_grids_in_one_launch():
    cases = C.four_grids()
    G = _PaddedGrids(cases)
    start = [G.state(key) for key in G.keys]
    for call in range(C.FOUR_CALLS):
        G.step([c.grads[call] for c in cases], [call >= c.first for c in cases], [c.lr for c in cases])
        for key, c, s0 in zip(G.keys, cases, start):
            state = G.state(key)                                 # (accumulator cleared, sentinels whole: stepping or not)
            done = call - c.first + 1
            if done <= 0:                                        # a grid at step 0: untouched
                assert all(Y.bits_equal(a, b) for a, b in zip(state, s0)), (key, call)
            else:
                _check_grid(state, c, done - 1, [c.lr] * done, c.grads[c.first:call + 1], s0, f"{key} V={c.V} launch {call + 1} step {done}")
    assert G.opt.steps == list(C.FOUR_STEPS) and host(G.opt.step_t).tolist() == list(C.FOUR_STEPS)


# ---- batch depth maximum and the sampler ------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", C.DMAX_KINDS)
def test_batch_depth_max(kind):
    import evennicer_slam_amd.functional as EF
    for n in C.DMAX_N:
        c = C.depth_case(kind, n)
        assert Y.bits_equal(host(EF.batch_depth_max(dev(c.gd))), c.dmax), n


@pytest.fixture(scope="module")
def scene():
    from tests.util import load
    return load('tiny_scene')


@pytest.mark.parametrize("n", C.SAMPLER_N)
def test_sample_rays_reduces_the_batch_maximum_itself(scene, n):
    """4096 rays: every wave reduces the depths itself; 4097: depth_max_kernel (the last depth, the largest, sits in its
    fifth, partial stride).  Bit-equal to the oracle, whose far clamp and no-depth surface samples use that maximum."""
    import evennicer_slam_amd.functional as EF
    from oracle import render_oracle as R
    ro, rd, gd = C.sampler_case(scene, n)
    bound = torch.from_numpy(scene['bound'].copy())
    assert 0.1 < (gd == 0).mean() < 0.35 and gd[n - 1] == gd.max() > gd[:-1].max()
    want = R.sample_depths(torch.from_numpy(ro), torch.from_numpy(rd), torch.from_numpy(gd), bound, 32, 16, 'color').numpy()
    z = host(EF.sample_rays(dev(ro), dev(rd), dev(gd), bound, 32, 16))
    assert z.dtype == np.float64 and Y.bits_equal(z, want)
    given = host(EF.sample_rays(dev(ro), dev(rd), dev(gd), bound, 32, 16, depth_max=dev(Y.depth_max(gd))))
    assert Y.bits_equal(given, want)


def test_depth_max_kernel_at_the_largest_batch(scene):
    """100000 rays (ray_batch_size): the samples with the kernel's own maximum equal those with the yardstick's handed in"""
    import evennicer_slam_amd.functional as EF
    ro, rd, gd = C.sampler_case(scene, 100000)
    bound = torch.from_numpy(scene['bound'].copy())
    ro, rd, gd_d = dev(ro), dev(rd), dev(gd)
    own = EF.sample_rays(ro, rd, gd_d, bound, 32, 16)
    given = EF.sample_rays(ro, rd, gd_d, bound, 32, 16, depth_max=dev(Y.depth_max(gd)))
    assert torch.equal(own, given)
    short = EF.sample_rays(ro, rd, gd_d, bound, 32, 16, depth_max=dev(Y.depth_max(gd[:-1])))
    assert not torch.equal(own, short)                           # (the last depth does decide the samples)
