"""iMAP kernels (csrc/imap_mlp.hip) at the edges where a tiling, slicing or chunking fault hides: values against the
float64 yardstick of tests/imap_torch.py (mlp64 / grads64) at tile and slice boundaries, and exact checks that need no
tolerance at all.  The forward and the dX chain compute every point on its own row with one fmaf order (f32 MFMA), so a
point's results do not depend on where it sits in the batch; with a cotangent on one point, every other point adds exact
zeros to dW and to the slice reduce.  Any dropped, doubled or misrouted point therefore breaks a bitwise equality."""
import ctypes

import numpy as np
import pytest
import torch

import evennicer_slam_amd as E
from evennicer_slam_amd import functional as EF
from tests import imap_torch as T
from tests.util import load, rel_err

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
EINVAL = -1


@pytest.fixture(scope="module")
def dec():
    fx = load("tiny_imap")
    model = T.fixture_decoder(fx).to(DEV)
    cpu = [q.detach().cpu() for q in EF.imap_params(model)]
    return model, cpu, torch.from_numpy(fx['bound'])


def _run(model, p, cot, bound=None):
    """(raw, d_pts, 11 parameter gradients) of one HIP forward + backward at cotangent cot"""
    model.zero_grad(set_to_none=True)
    x = p.detach().to(DEV).requires_grad_(True)
    raw = EF.imap_mlp(x, model, bound=bound)
    (raw * cot.to(DEV)).sum().backward()
    return raw.detach(), x.grad, [q.grad.clone() for q in EF.imap_params(model)]


def _set_chunk(monkeypatch, chunk):
    """make imap_chunk_points() return `chunk` (a multiple of 64)"""
    per = E._lib.lib().enslam_imap_workspace_floats(1 << 16) / float(1 << 16) * 4
    monkeypatch.setattr(EF, 'IMAP_WS_LIMIT_BYTES', int(per * (chunk + 0.5)))
    assert EF.imap_chunk_points() == chunk


def _mixed_points(P, bound, g, dtype=torch.float64):
    """points over the bound's box and a margin of a fifth of its size on every side: about a third lie outside"""
    lo, hi = bound[:, 0], bound[:, 1]
    u = torch.rand(P, 3, generator=g, dtype=torch.float64) * 1.4 - 0.2
    return (lo + (hi - lo) * u).to(dtype)


# ------------------------------------------------------------------------------------------------ a. values vs float64
TOL = 3e-5


@pytest.fixture(scope="module")
def margin_points(dec):
    """points in [-4, 4]^3 (Fourier arguments up to ~480) whose relative ReLU margin is above 3e-5 (about 82 % of them):
    float32 takes every relu branch as float64 does there"""
    g = torch.Generator().manual_seed(11)
    p = (torch.rand(6000, 3, generator=g, dtype=torch.float64) * 2 - 1) * 4
    p = p[T.mlp64(p, dec[1])[1] > 3e-5]
    assert p.shape[0] > 4097
    return p


@pytest.mark.parametrize("P", [1, 2, 63, 64, 65, 127, 1023, 1024, 1025, 2049, 4097])
def test_values_against_float64(dec, margin_points, P):
    """raw, d_pts and every parameter gradient, elementwise: |got - ref| <= TOL * scale, scale the error scale of
    grads64 (the abs-sum of the terms, each factor replaced by the abs-sum that formed it).

    Error model: every layer is an f32 fmaf chain of at most 256 terms, whose rounding error is below 256 u = 1.5e-5 of
    its abs-sum and in practice a few ulp; sinf / cosf add about an ulp of the embedding; the argument is formed as the
    yardstick forms it.  TOL = 3e-5 is twice that chain bound; measured on an MI355X the worst ratio over all P and all
    13 outputs is 2.8e-7 (raw at P = 4097; printed with -s), about 100x headroom.  The bar still sees one point: at every P, the float64 gradients with the last
    point left out exceed it for each of the 11 parameters (the last point's share of an entry's scale is 1.2e-4 or
    more at P = 4097), which is what a tile, slice or tail fault does."""
    model, ps, _ = dec
    p = margin_points[:P]
    g = torch.Generator().manual_seed(100 + P)
    cot = torch.randn(P, 4, generator=g)
    raw, dp, grads = _run(model, p, cot)
    ref_raw, ref_dp, ref_g, scales, dp_scale, raw_scale = T.grads64(p, ps, cot)
    worst = {}

    def check(name, got, ref, scale):
        err = (got.detach().cpu().double() - ref).abs()
        assert (err <= TOL * scale).all(), (name, float((err / scale.clamp_min(1e-300)).max()))
        worst[name] = float((err / scale.clamp_min(1e-300)).max())

    check('raw', raw, ref_raw, raw_scale)
    check('d_pts', dp, ref_dp, dp_scale)
    for name, got, ref, s in zip(T.NAMES, grads, ref_g, scales):
        check(name, got, ref, s)
    print(f"P={P} worst |got - ref| / scale:", max(worst.values()), worst)
    # sensitivity: the bar sees one missing point in every parameter gradient
    drop = T.grads64(p[:-1], ps, cot[:-1])[2] if P > 1 else [torch.zeros_like(r) for r in ref_g]
    for name, d, ref, s in zip(T.NAMES, drop, ref_g, scales):
        assert ((d - ref).abs() > TOL * s).any(), name


# ------------------------------------------------------------------------------------------------ b. position invariance
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("chunk", [None, 64, 128, 2368])
def test_permutation_is_bitwise(dec, monkeypatch, dtype, chunk):
    """raw and d_pts of a permuted batch (cotangent permuted alike) are the permuted results bit for bit, unchunked and
    in backward chunks of 64, 128 and 2368 (37 tiles) points; chunking does not change a bit either."""
    model, _, bound = dec
    P = 245760 + 37
    g = torch.Generator().manual_seed(21)
    p = _mixed_points(P, bound, g, dtype)
    cot = torch.randn(P, 4, generator=g)
    perm = torch.randperm(P, generator=g)
    raw, dp, _ = _run(model, p, cot, bound)
    assert dp.dtype == dtype
    out = raw[:, 3] == 100
    assert 0.2 < out.float().mean().item() < 0.8
    if chunk is not None:
        _set_chunk(monkeypatch, chunk)
        raw_c, dp_c, _ = _run(model, p, cot, bound)
        assert torch.equal(raw_c, raw) and torch.equal(dp_c, dp)
    raw2, dp2, _ = _run(model, p[perm], cot[perm], bound)
    pd = perm.to(DEV)
    assert torch.equal(raw2, raw[pd])
    assert torch.equal(dp2, dp[pd])


# ------------------------------------------------------------------------------------------------ c. one-hot, bitwise
def _slice_edges(P):
    """(per, first point of the last non-empty slice) of imap_dw_kernel's split of P points"""
    slices = max(1, min(64, P // 1024))
    per = -(-P // slices)
    per += per & 1
    return per, (P - 1) // per * per


@pytest.mark.parametrize("chunk", [None, 64, 2368])
def test_one_hot_gradients_are_a_single_point_call(dec, monkeypatch, chunk):
    """With the cotangent on point i alone, all 11 parameter gradients and d_pts[i] equal those of a P = 1 call on point
    i bit for bit, and every other row of d_pts is exactly 0.  P = 65536 + 37: 64 slices of 1026 points, the last one
    with 935.  The points i sit at tile edges (63 | 64), slice edges (1025 | 1026), in the middle, at both ends of the
    last slice, outside the bound and, with chunks, on both sides of chunk seams."""
    model, _, bound = dec
    P = 65536 + 37
    per, last0 = _slice_edges(P)
    assert per == 1026 and last0 == 63 * 1026
    g = torch.Generator().manual_seed(31)
    p = _mixed_points(P, bound, g)
    out = T._outside(p, bound)
    idx = [0, 63, 64, 1025, 1026, 1027, P // 2, last0 - 1, last0, P - 1, int(torch.nonzero(out)[7])]
    if chunk is not None:
        _set_chunk(monkeypatch, chunk)
        idx += [chunk - 1, chunk, 5 * chunk - 1, 5 * chunk, (P - 1) // chunk * chunk - 1, (P - 1) // chunk * chunk]
    assert out[idx[10]]
    vals = torch.randn(len(idx), 4, generator=g) + 0.5
    for i, v in zip(idx, vals):
        cot = torch.zeros(P, 4)
        cot[i] = v
        _, dp, grads = _run(model, p, cot, bound)
        _, dp1, grads1 = _run(model, p[i:i + 1], v[None], bound)
        for name, a, b in zip(T.NAMES, grads, grads1):
            assert torch.equal(a, b), (i, name)
        assert torch.equal(dp[i], dp1[0]), i
        others = torch.ones(P, dtype=torch.bool, device=DEV)
        others[i] = False
        assert not dp[others].any(), i
        assert grads[1].any() and dp1.any(), i     # the point does reach the parameters


# ------------------------------------------------------------------------------------------------ d. bound faces
def _face_points(bound, dtype):
    """points exactly on each of the six faces (the face value in the points' precision), one ulp inside and one ulp
    outside; the other two coordinates at the box's centre.  float64 batches also hold the float32-rounded faces."""
    b = bound.to(dtype)
    c = b.mean(1)
    rows = []
    for a in range(3):
        for side, inward in ((0, 1.), (1, -1.)):
            f = b[a, side]
            faces = [f] if dtype == torch.float32 else [f, bound[a, side].float().double()]
            for f in faces:
                for v in (f, torch.nextafter(f, f + inward), torch.nextafter(f, f - inward)):
                    q = c.clone()
                    q[a] = v
                    rows.append(q)
    return torch.stack(rows)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_bound_faces(dec, dtype):
    """the sigma = 100 mask equals eval_points' strict comparison point for point on and next to every face; a batch of
    points that are all outside, with a cotangent on sigma only, gets exactly zero d_pts and parameter gradients"""
    model, ps, bound = dec
    p = _face_points(bound, dtype)
    g = torch.Generator().manual_seed(41)
    cot = torch.randn(p.shape[0], 4, generator=g)
    raw, dp, _ = _run(model, p, cot, bound)
    ref = T.eval_points(p, ps, bound)
    mask = (raw[:, 3] == 100).cpu()
    assert torch.equal(mask, ref[:, 3] == 100)
    assert torch.equal(mask, T._outside(p, bound))
    assert mask.any() and (~mask).any()
    outside = p[mask]
    cot = torch.zeros(outside.shape[0], 4)
    cot[:, 3] = torch.randn(outside.shape[0], generator=g)
    _, dp, grads = _run(model, outside, cot, bound)
    assert not dp.any()
    for name, q in zip(T.NAMES, grads):
        assert not q.any(), name


# ------------------------------------------------------------------------------------------------ e. empty batch
def test_empty_batch(dec):
    model, _, bound = dec
    x = torch.zeros(0, 3, device=DEV, requires_grad=True)
    model.zero_grad(set_to_none=True)
    raw = EF.imap_mlp(x, model, bound=bound)
    assert raw.shape == (0, 4)
    raw.sum().backward()
    assert x.grad.shape == (0, 3)
    params = EF.imap_params(model)
    for name, q in zip(T.NAMES, params):
        assert q.grad is not None and q.grad.shape == q.shape and not q.grad.any(), name
    # a second backward adds nothing to existing gradients
    g = torch.Generator().manual_seed(51)
    for q in params:
        q.grad = torch.randn(q.shape, generator=g).to(DEV)
    before = [q.grad.clone() for q in params]
    EF.imap_mlp(x, model).sum().backward()
    for name, q, b in zip(T.NAMES, params, before):
        assert torch.equal(q.grad, b), name


# ------------------------------------------------------------------------------------------------ f. C-ABI errors
def test_imap_abi_error_paths(dec):
    """EINVAL for a negative count and for each pointer the entries check; an empty batch is OK"""
    model, _, _ = dec
    lib = E._lib.lib()
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    P = 4
    pts = torch.zeros(P, 3, dtype=torch.float64, device=DEV)
    params = [q.detach() for q in EF.imap_params(model)]
    grads = [torch.zeros_like(q) for q in params]
    packed = torch.zeros(lib.enslam_imap_packed_floats(), device=DEV)
    raw = torch.zeros(P, 4, device=DEV)
    ws = torch.zeros(lib.enslam_imap_workspace_floats(P), device=DEV)
    dpts = torch.zeros(P, 3, device=DEV)
    ptr = lambda t: t.data_ptr()

    def arr(ts, null=None):
        return (ctypes.c_void_p * 11)(*[None if i == null else t.data_ptr() for i, t in enumerate(ts)])

    assert lib.enslam_imap_workspace_floats(-1) == 0
    # pack
    assert lib.enslam_imap_pack(None, ptr(packed), st) == EINVAL
    assert lib.enslam_imap_pack(arr(params), None, st) == EINVAL
    for i in range(11):
        assert lib.enslam_imap_pack(arr(params, i), ptr(packed), st) == EINVAL, i
    # forward
    assert lib.enslam_imap_fwd(-1, ptr(pts), ptr(packed), None, ptr(raw), st) == EINVAL
    assert lib.enslam_imap_fwd(P, None, ptr(packed), None, ptr(raw), st) == EINVAL
    assert lib.enslam_imap_fwd(P, ptr(pts), None, None, ptr(raw), st) == EINVAL
    assert lib.enslam_imap_fwd(P, ptr(pts), ptr(packed), None, None, st) == EINVAL
    assert lib.enslam_imap_fwd(0, None, None, None, None, st) == 0
    # backward
    full = dict(points=ptr(pts), packed=ptr(packed), d_raw=ptr(raw), ws=ptr(ws), d_points=ptr(dpts))

    def bwd(n, params_=None, grads_=None, **null):
        a = {k: (None if k in null else v) for k, v in full.items()}
        return lib.enslam_imap_bwd(n, a['points'], params_, a['packed'], None, a['d_raw'], a['ws'], 1, grads_,
                                   a['d_points'], st)

    assert bwd(-1, arr(params), arr(grads)) == EINVAL
    assert bwd(P, None, arr(grads)) == EINVAL
    assert bwd(P, arr(params), None) == EINVAL
    for i in range(11):
        assert bwd(P, arr(params, i), arr(grads)) == EINVAL, i
        assert bwd(P, arr(params), arr(grads, i)) == EINVAL, i
    for k in full:
        assert bwd(P, arr(params), arr(grads), **{k: True}) == EINVAL, k
    assert lib.enslam_imap_bwd(0, None, arr(params), None, None, None, None, 1, arr(grads), None, st) == 0
    assert lib.enslam_imap_bwd(0, None, arr(params), None, None, None, None, 0, arr(grads), None, st) == 0
    torch.cuda.synchronize()
    assert not any(q.any() for q in grads)
    # density compositing
    N, S = 4, 8
    r = torch.zeros(N, S, 4, device=DEV)
    z = torch.zeros(N, S, dtype=torch.float64, device=DEV)
    d = torch.zeros(N, 3, device=DEV)
    dd = torch.zeros(N, dtype=torch.float64, device=DEV)
    c = torch.zeros(N, 3, device=DEV)
    fwd = [ptr(r), ptr(z), ptr(d), ptr(dd), ptr(dd), ptr(c)]
    for s in (0, 65):
        assert lib.enslam_composite_density_fwd(N, s, *fwd, None, st) == EINVAL, s
        assert lib.enslam_composite_density_bwd(N, s, ptr(r), ptr(z), ptr(d), ptr(dd), None, None, None, ptr(r), None,
                                                st) == EINVAL, s
    assert lib.enslam_composite_density_fwd(-1, S, *fwd, None, st) == EINVAL
    assert lib.enslam_composite_density_bwd(-1, S, ptr(r), ptr(z), ptr(d), ptr(dd), None, None, None, ptr(r), None,
                                            st) == EINVAL
    for i in range(6):
        a = list(fwd)
        a[i] = None
        assert lib.enslam_composite_density_fwd(N, S, *a, None, st) == EINVAL, i
    bw = [ptr(r), ptr(z), ptr(d), ptr(dd)]
    for i in range(5):
        a = bw + [ptr(r)]
        a[i] = None
        assert lib.enslam_composite_density_bwd(N, S, *a[:4], None, None, None, a[4], None, st) == EINVAL, i
    assert lib.enslam_composite_density_fwd(0, S, *([None] * 7), st) == 0
    assert lib.enslam_composite_density_bwd(0, S, *([None] * 9), st) == 0
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ g. density compositing
def _density_case(N, S, g):
    z = torch.sort(torch.rand(N, S, generator=g, dtype=torch.float64) * 3 + 0.1, -1)[0]
    if S > 3:
        z[:4, 1:3] = z[:4, 1:2]                               # zero-length intervals
    raw = torch.randn(N, S, 4, generator=g)
    raw[:, :, 3] = raw[:, :, 3] * 20
    raw[8:12, :, 3] = 0.                                      # sigma exactly 0
    raw[12:16, ::2, 3] = 0.
    rd = torch.randn(N, 3, generator=g) * 1.7
    rd[16] = torch.tensor([0., 0., -1.])
    return raw, z, rd


def _density_run(fn, raw, z, rd, cot):
    a, b = raw.to(DEV).requires_grad_(True), rd.to(DEV).requires_grad_(True)
    d, v, c, w = fn(a, z.to(DEV), b)
    ((d * cot[0].to(DEV)).sum() + (v * cot[1].to(DEV)).sum() + (c * cot[2].to(DEV)).sum()).backward()
    return [t.detach().cpu() for t in (d, v, c, w, a.grad, b.grad)]


@pytest.mark.parametrize("S", [1, 2, 63])
def test_composite_density_against_float64(S):
    """outputs and gradients against the restatement in float64 on the same float32 inputs (its dists are rounded to
    float32 as the reference rounds them)"""
    g = torch.Generator().manual_seed(60 + S)
    N = 96
    raw, z, rd = _density_case(N, S, g)
    cot = (torch.randn(N, generator=g, dtype=torch.float64), torch.randn(N, generator=g, dtype=torch.float64),
           torch.randn(N, 3, generator=g))
    got = _density_run(EF.composite_density, raw, z, rd, cot)
    ref = _density_run(T.composite_density, raw.double(), z, rd.double(), (cot[0], cot[1], cot[2].double()))
    for name, a, b, bar in zip(('depth', 'var', 'rgb', 'weights', 'd_raw', 'd_rays_d'), got, ref,
                               (1e-5,) * 6):
        assert a.shape == b.shape, name
        assert torch.isfinite(a).all(), name
        assert rel_err(a.double().numpy(), b.double().numpy()) < bar, name


def test_composite_density_ray_permutation_is_bitwise():
    g = torch.Generator().manual_seed(70)
    N, S = 1000, 48
    raw, z, rd = _density_case(N, S, g)
    cot = (torch.randn(N, generator=g, dtype=torch.float64), torch.randn(N, generator=g, dtype=torch.float64),
           torch.randn(N, 3, generator=g))
    perm = torch.randperm(N, generator=g)
    a = _density_run(EF.composite_density, raw, z, rd, cot)
    b = _density_run(EF.composite_density, raw[perm], z[perm], rd[perm], tuple(c[perm] for c in cot))
    for name, x, y in zip(('depth', 'var', 'rgb', 'weights', 'd_raw', 'd_rays_d'), a, b):
        assert torch.equal(x[perm], y), name


def test_composite_density_null_cotangents():
    """NULL g_depth / g_var / g_rgb (and d_rays_d) through the ABI give what zero cotangents give, bit for bit"""
    lib = E._lib.lib()
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    g = torch.Generator().manual_seed(80)
    N, S = 200, 33
    raw, z, rd = (t.to(DEV) for t in _density_case(N, S, g))
    cot = [torch.randn(N, generator=g, dtype=torch.float64).to(DEV),
           torch.randn(N, generator=g, dtype=torch.float64).to(DEV), torch.randn(N, 3, generator=g).to(DEV)]
    depth = torch.empty(N, dtype=torch.float64, device=DEV)
    var, rgb = torch.empty_like(depth), torch.empty(N, 3, device=DEV)
    assert lib.enslam_composite_density_fwd(N, S, raw.data_ptr(), z.data_ptr(), rd.data_ptr(), depth.data_ptr(),
                                            var.data_ptr(), rgb.data_ptr(), None, st) == 0

    def bwd(cs, with_rd=True):
        d_raw = torch.full((N, S, 4), float('nan'), device=DEV)
        d_rd = torch.full((N, 3), float('nan'), device=DEV)
        assert lib.enslam_composite_density_bwd(N, S, raw.data_ptr(), z.data_ptr(), rd.data_ptr(), depth.data_ptr(),
                                                *[c.data_ptr() if c is not None else None for c in cs],
                                                d_raw.data_ptr(), d_rd.data_ptr() if with_rd else None, st) == 0
        torch.cuda.synchronize()
        return d_raw, d_rd

    for k in range(3):
        nulled = [None if j == k else c for j, c in enumerate(cot)]
        zeroed = [torch.zeros_like(c) if j == k else c for j, c in enumerate(cot)]
        a, b = bwd(nulled), bwd(zeroed)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), k
    a, b = bwd([None] * 3), bwd([torch.zeros_like(c) for c in cot])
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    full = bwd(cot)
    d_raw, d_rd = bwd(cot, with_rd=False)
    assert torch.equal(d_raw, full[0]) and torch.isnan(d_rd).all()     # d_rays_d NULL: not written


def test_composite_density_65_samples_raise():
    import types
    raw = torch.zeros(2, 65, 4, device=DEV)
    z = torch.linspace(0.1, 2., 65, dtype=torch.float64, device=DEV).expand(2, 65).contiguous()
    with pytest.raises(E.EnslamError):
        EF.composite_density(raw, z, torch.ones(2, 3, device=DEV))
    fx = load("tiny_imap")
    cfg = {'rendering': {'lindisp': False, 'perturb': 0.0, 'N_samples': 53, 'N_surface': 0, 'N_importance': 12},
           'scale': 1, 'occupancy': False}
    slam = types.SimpleNamespace(nice=False, bound=torch.from_numpy(fx['bound']), H=48, W=64, fx=50., fy=50., cx=31.5,
                                 cy=23.5)
    r = E.Renderer(cfg, None, slam)
    model = T.fixture_decoder(fx).to(DEV)
    with pytest.raises(NotImplementedError):
        r.render_batch_ray(None, model, torch.ones(2, 3, device=DEV), torch.zeros(2, 3, device=DEV), DEV, 'color',
                           gt_depth=torch.ones(2, device=DEV))
