"""-m gpu: the occupancy compositing kernels on their own terms -- composite_fwd_kernel (csrc/render_fwd.hip: plain form,
fused mapper loss, fused loss + unit backward + work list), composite_bwd_kernel (csrc/render_bwd.hip: incoming cotangents,
loss-derived cotangents, 16-rays-per-workgroup list form) and append_active_tiles_wg (csrc/common.hpp) -- elementwise against
the float64 yardstick of tests/composite_numpy.py on the seeded cases of tests/composite_cases.py, with exact statements and
bitwise equalities wherever the code guarantees them.

THE BAR (derived, not fitted; the derivation is composite_numpy.error_model, u = 2^-24).  Per operation: expf one ulp (2 u),
IEEE add / multiply / correctly rounded divide u each, no contraction (the library is built with -ffp-contract=off).
1 - alpha is a float32 subtraction, so it carries an ABSOLUTE error of about 4 u alpha -- a relative error 4 u alpha / m of
that factor of the transmittance, 30 u at 10 occ = 2, of order 1 for 10 occ in [12, 16.7] -- while above 16.7 the kernels'
alpha is exactly 1 and m exactly 1e-10f.  The bar is the full (not first-order) propagation of these per-factor errors
through the product chain (<= 63 factors, one u per multiply), the 6-level float32 tree sums (rgb; the suffix scan, whose
`inclusive - own` costs 7 u of the sum including the own term), float64 sums of float32 weights (depth, var), plus an
absolute 2^-123 (8 x the smallest normal float32) times the ray's largest cotangent term for products that leave float32's
normal range.  For d_occ the propagation of an absolute error of a few u in each 1 - alpha_i is therefore what applies on
near-saturated rays, the relative chain bound elsewhere; one formula yields both.  tests/test_composite_cpu.py shows from
the reference alone that this bar rejects a dropped last sample, an inclusive scan, a suffix sum including j, either lost
g_var term, a lost 1e-10 and two swapped rays.

MEASURED on an MI355X (this module with -s; worst |got - ref| / bar over all 330 cases and all cotangent choices, and the
worst error in units of u of the element's scale):
                 patterns a, b, c, d (unsaturated / closed / empty)      patterns e, f (near-saturated samples)
    weights      0.49 of the bar     43 u of scale                        1.000000 of the bar (below it by rounding terms)
    depth        0.30                5.8 u                                0.73
    var          0.25                13 u                                 0.999999
    rgb          0.21                5.2 u                                0.57
    d_colour     0.50                43 u                                 1.000000 (g_rgb times the weights' error)
    d_occ        0.18                9.9 u (of 10 G, composite_numpy)     0.999997
    fused loss   |got - ref| <= 3.1e-7 against bars of 8e-7 ... 9e-5 (N = 1 ... 33)
Headroom, stated and not tuned: a factor 2 to 5 where nothing is near-saturated -- the bar is a worst case of 4 u alpha per
1 - alpha, the kernels' errors are the usual half of that -- and none at all behind a sample with 10 occ in (16.7, 20]: there
the kernels' m is exactly 1e-10f while the true m is up to 6e-8, the error IS the modelled dm = 1 - alpha (deterministic, the
same on every run), and the bar exceeds it only by its rounding terms.  In u of the scale those elements are off by ~4e7:
a bar relative to an element's own scale cannot be met there by any float32 evaluation.

BITWISE CLAIMS and why the code guarantees them:
  * position / batch-size invariance: a ray is composited by one wave; every cross-lane step is a shuffle within that wave
    (prefix product, suffix sum, wave_sum butterflies) in a fixed lane order; nothing a ray computes reads another ray, and
    the ray's index only selects addresses.  So a ray's bits do not depend on N, on its place, or on blockDim.
  * plain form == fused-loss form == plain form on that call's raw_out (depth, var, rgb): ONE compiled kernel; the forms
    differ in blockDim (64 vs 1024) and in uniform branches taken after depth / var / rgb are final.
  * list form == no-list form (d_raw): ONE compiled kernel again; the work list changes blockDim and appends after d_raw is
    stored.
  * enslam_composite_loss_bwd(g) == enslam_composite_bwd fed g_depth = -/+ g (float64) and g_rgb = -((float) g * w_color) sign
    (float32): same kernel; the loss branch only fills gD and gc[] with exactly these values before the shared arithmetic.
  * d_raw_unit (forward kernel) == enslam_composite_loss_bwd with g_loss = 1: two kernels, but the same source expressions
    on the same inputs (depth and rgb are the forward's own bits), IEEE operations without contraction, the same expf.  The
    backward kernel's extra terms vanish exactly: g_var = 0 gives gD - 2*0*sum = gD and (float)(gD z + 0*tmp*tmp) =
    (float)(gD z); (float) 1.0 * w_color = w_color.
  * the loss value is NOT bitwise: one float64 atomic per 16 rays, their order moves the last bits; it is compared with the
    float64 sum under the sum of the per-ray bars."""
import ctypes

import numpy as np
import pytest
import torch

from tests import composite_cases as C
from tests import composite_numpy as Y

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
EINVAL = -1
SENTINEL = -7
U = Y.U


# ------------------------------------------------------------------------------------------------ plumbing
def _api():
    import evennicer_slam_amd as E
    import evennicer_slam_amd.functional as EF
    return E._lib, E._lib.lib(), EF


def _dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).to(DEV).contiguous()


def _np(t):
    return t.detach().cpu().numpy()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64 if a.dtype == np.float64 else np.int32)


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and bool((_bits(a) == _bits(b)).all())


def _fwd(raw, z):
    """EF.composite: (depth f64 [N], var f64 [N], rgb f32 [N,3], w f32 [N,S]) as numpy"""
    _, _, EF = _api()
    return tuple(_np(t) for t in EF.composite(_dev(raw, torch.float32), _dev(z, torch.float64)))


def _list_buffers(N, S):
    n = N * (S // 16)
    return torch.full((n + 8,), SENTINEL, dtype=torch.int32, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)


def _bwd(raw, z, depth, gD=None, gV=None, gC=None, work=None):
    """enslam_composite_bwd (work None) or enslam_composite_bwd_list (work = (list, count)); d_raw [N,S,4] numpy.
    d_raw is prefilled with NaN: an element the kernel does not write fails every comparison."""
    L, lib, EF = _api()
    P, st = EF._ptr, EF._stream()
    N, S = z.shape
    r, zz, dep = _dev(raw, torch.float32), _dev(z, torch.float64), _dev(depth, torch.float64)
    g = [None if x is None else _dev(x, dt) for x, dt in ((gD, torch.float64), (gV, torch.float64), (gC, torch.float32))]
    d = torch.full((N, S, 4), float('nan'), dtype=torch.float32, device=DEV)
    if work is None:
        L.check(lib.enslam_composite_bwd(N, S, P(r), P(zz), P(dep), P(g[0]), P(g[1]), P(g[2]), P(d), st), "composite_bwd")
    else:
        L.check(lib.enslam_composite_bwd_list(N, S, P(r), P(zz), P(dep), P(g[0]), P(g[1]), P(g[2]), P(d), P(work[0]), P(work[1]),
                                              st), "composite_bwd_list")
    torch.cuda.synchronize()
    return _np(d)


def _loss_bwd(raw, z, depth, rgb, gt_depth, gt_color, g_loss, work=None):
    L, lib, EF = _api()
    P, st = EF._ptr, EF._stream()
    N, S = z.shape
    r, zz, dep = _dev(raw, torch.float32), _dev(z, torch.float64), _dev(depth, torch.float64)
    c = _dev(rgb, torch.float32)
    gd = _dev(gt_depth, torch.float32)
    gc = None if gt_color is None else _dev(gt_color, torch.float32)
    gl = torch.tensor([g_loss], dtype=torch.float64, device=DEV)
    d = torch.full((N, S, 4), float('nan'), dtype=torch.float32, device=DEV)
    wl, wc = (None, None) if work is None else work
    L.check(lib.enslam_composite_loss_bwd(N, S, P(r), P(zz), P(dep), P(c), P(gd), P(gc), C.W_COLOR, P(gl), P(d), P(wl), P(wc), st),
            "composite_loss_bwd")
    torch.cuda.synchronize()
    return _np(d)


def _loss_cotangents(depth, rgb, gt_depth, gt_color, g):
    """the cotangents the loss branch of composite_bwd_kernel forms, value for value"""
    gd = gt_depth.astype(np.float32)
    diff = gd.astype(np.float64) - depth
    gD = np.where(gd > 0, np.where(diff > 0, -g, np.where(diff < 0, g, 0.0)), 0.0)
    if gt_color is None:
        return gD, None
    gw = np.float32(g) * np.float32(C.W_COLOR)
    d = gt_color.astype(np.float32) - rgb.astype(np.float32)
    return gD, (-gw * np.sign(d).astype(np.float32)).astype(np.float32)


@pytest.fixture(scope="module")
def cases():
    return {(c['S'], c['N'], c['pattern']): c for c in C.all_cases()}


def _ratio(err, bar):
    """max err / bar over the elements whose bar is not 0 (a bar of 0 asks for, and got, an exact 0)"""
    pos = bar > 0
    return float((err[pos] / bar[pos]).max()) if pos.any() else 0.0


class _Worst:
    def __init__(self):
        self.bar, self.u = {}, {}

    def add(self, name, err, bar, scale):
        self.bar[name] = max(self.bar.get(name, 0.0), _ratio(err, bar))
        ok = scale > 1e-30
        if ok.any():
            self.u[name] = max(self.u.get(name, 0.0), float((err[ok] / scale[ok]).max() / U))


def _check(worst, name, got, ref, bar, scale, where):
    err = np.abs(got.astype(np.float64) - ref)
    assert np.isfinite(got).all(), (name, where)
    bar = np.broadcast_to(bar, err.shape)
    assert (err <= bar).all(), (name, where, _ratio(err, bar))
    worst.add(name, err, bar, np.broadcast_to(scale, err.shape))


# ------------------------------------------------------------------------------------------------ values
@pytest.mark.parametrize("pattern", list(C.PATTERNS))
def test_values_against_float64(cases, pattern):
    """EF.composite forward (weights, depth, var, rgb) and enslam_composite_bwd with each cotangent alone (the others NULL)
    and all together, and enslam_composite_loss_bwd (g_loss = 0.37, with and without colour) against the yardstick's loss
    cotangents: every element within the derived bar, at all 55 shapes.  The backward is handed the yardstick's float64
    depth (the kernel's own forward depth is pinned separately, above); the loss form is handed the kernel's own depth
    and rgb, whose signs against gt are the yardstick's by the margin condition of composite_cases.check_conditions.

    Measured on an MI355X: the table in the module docstring (printed per pattern with -s)."""
    worst = _Worst()
    for S in C.S_LIST:
        for N in C.N_LIST:
            c = cases[S, N, pattern]
            raw, z, f, where = c['raw'], c['z'], c['f'], (S, N, pattern)
            depth, var, rgb, w = _fwd(raw, z)
            scales, bars, _ = Y.forward_bars(f)
            for k, got in (('w', w), ('depth', depth), ('var', var), ('rgb', rgb)):
                _check(worst, k, got, f[k], bars[k], scales[k], where)
            gD, gV, gC = c['g_depth'], c['g_var'], c['g_rgb']
            for tag, cots in (('gD', (gD, None, None)), ('gV', (None, gV, None)), ('gC', (None, None, gC)), ('all', (gD, gV, gC))):
                d = _bwd(raw, z, f['depth'], *cots)
                ref = Y.backward(raw, z, *cots, f=f)
                scale, bar = Y.backward_bars(f, *cots)
                _check(worst, 'd_col/' + tag, d[..., :3], ref[..., :3], bar[..., :3], scale[..., :3], where)
                _check(worst, 'd_occ/' + tag, d[..., 3], ref[..., 3], bar[..., 3], scale[..., 3], where)
            g = 0.37
            for tag, gtc, Lk in (('loss', c['gt_color'], 'loss'), ('loss_depth', None, 'loss_depth_only')):
                d = _loss_bwd(raw, z, depth, rgb, c['gt_depth'], gtc, g)
                yl = c[Lk]
                cots = (g * yl['g_depth'], None, None if gtc is None else g * yl['g_rgb'])
                ref = Y.backward(raw, z, *cots, f=f)
                scale, bar = Y.backward_bars(f, *cots)
                _check(worst, 'd_col/' + tag, d[..., :3], ref[..., :3], bar[..., :3], scale[..., :3], where)
                _check(worst, 'd_occ/' + tag, d[..., 3], ref[..., 3], bar[..., 3], scale[..., 3], where)
    print(f"pattern {pattern}: worst err/bar", {k: f"{v:.6g}" for k, v in worst.bar.items()})
    print(f"pattern {pattern}: worst err in u of scale", {k: f"{v:.3g}" for k, v in worst.u.items()})


# ------------------------------------------------------------------------------------------------ exact statements
def test_exact_zeros(cases):
    """No tolerance: pattern d (alpha exactly 0) gives all-zero weights, depth, var, rgb and d_raw; behind pattern c's run of
    six every weight and every d_raw component is 0; every sample at occupancy 100 has d_occ == 0 (the kernels' 1 - alpha
    is exactly 0 there); masked rays (gt_depth <= 0) have all-zero d_raw in the loss forms without a colour term."""
    seen = dict(d=0, behind=0, occ100=0, masked=0)
    for (S, N, pattern), c in cases.items():
        if pattern not in 'bcdf':
            continue
        raw, z, f = c['raw'], c['z'], c['f']
        depth, var, rgb, w = _fwd(raw, z)
        work = _list_buffers(N, S) if S % 16 == 0 else None
        d_all = _bwd(raw, z, depth, c['g_depth'], c['g_var'], c['g_rgb'], work=work)
        d_loss = _loss_bwd(raw, z, depth, rgb, c['gt_depth'], c['gt_color'], 1.0)
        d_ld = _loss_bwd(raw, z, depth, rgb, c['gt_depth'], None, 0.37, work=_list_buffers(N, S) if S % 16 == 0 else None)
        assert np.isfinite(d_all).all() and np.isfinite(d_loss).all() and np.isfinite(d_ld).all()
        for r in range(N):
            p = C.ray_pattern(pattern, r)
            if p == 'd':
                assert (w[r] == 0).all() and depth[r] == 0 and var[r] == 0 and (rgb[r] == 0).all()
                assert (d_all[r] == 0).all() and (d_loss[r] == 0).all() and (d_ld[r] == 0).all()
                seen['d'] += 1
            if p == 'c' and S > C.run_start(S) + 6:
                b = C.run_start(S) + 6
                assert (w[r, b:] == 0).all()
                assert (d_all[r, b:] == 0).all() and (d_loss[r, b:] == 0).all() and (d_ld[r, b:] == 0).all()
                seen['behind'] += 1
            o = raw[r, :, 3] == 100.0
            assert (d_all[r, o, 3] == 0).all() and (d_loss[r, o, 3] == 0).all() and (d_ld[r, o, 3] == 0).all()
            seen['occ100'] += int(o.sum())
            if C.masked(r):
                assert (d_ld[r] == 0).all()
                seen['masked'] += 1
    assert all(v > 0 for v in seen.values()), seen


# ------------------------------------------------------------------------------------------------ position and form invariance
def _all_forms(c, sel):
    """forward and the three backward forms on the rays `sel` of case c: dict of numpy arrays"""
    raw, z = c['raw'][sel], c['z'][sel]
    N, S = z.shape
    depth, var, rgb, w = _fwd(raw, z)
    out = dict(depth=depth, var=var, rgb=rgb, w=w)
    out['d'] = _bwd(raw, z, depth, c['g_depth'][sel], c['g_var'][sel], c['g_rgb'][sel])
    out['d_loss'] = _loss_bwd(raw, z, depth, rgb, c['gt_depth'][sel], c['gt_color'][sel], 0.37)
    if S % 16 == 0:
        out['d_list'] = _bwd(raw, z, depth, c['g_depth'][sel], c['g_var'][sel], c['g_rgb'][sel], work=_list_buffers(N, S))
        out['d_loss_list'] = _loss_bwd(raw, z, depth, rgb, c['gt_depth'][sel], c['gt_color'][sel], 0.37, work=_list_buffers(N, S))
    return out


@pytest.mark.parametrize("S", C.S_LIST)
def test_position_and_batch_size_do_not_change_a_bit(cases, S):
    """the 33-ray mixed batch (pattern f): permuted, and split at 15, 16 and 17 into two calls, every output of every form
    equals the whole batch's bit for bit (module docstring: one wave per ray, shuffles only)"""
    c = cases[S, 33, 'f']
    whole = _all_forms(c, np.arange(33))
    perm = np.random.default_rng(S).permutation(33)
    got = _all_forms(c, perm)
    for k, v in whole.items():
        assert _same_bits(got[k], v[perm]), ('permuted', k)
    for cut in (15, 16, 17):
        a, b = _all_forms(c, np.arange(cut)), _all_forms(c, np.arange(cut, 33))
        for k, v in whole.items():
            assert _same_bits(np.concatenate([a[k], b[k]]), v), ('split', cut, k)
    if S % 16 == 0:                                              # the 16-rays-per-workgroup forms against the one-wave forms
        assert _same_bits(whole['d_list'], whole['d']) and _same_bits(whole['d_loss_list'], whole['d_loss'])


def test_list_form_and_loss_form_share_the_plain_backward_bits(cases):
    """every pattern, S in {16, 32, 48, 64}, every N: enslam_composite_bwd_list == enslam_composite_bwd in d_raw;
    enslam_composite_loss_bwd(g) (with and without a list, with and without colour) == enslam_composite_bwd fed the same
    cotangents as float64 / float32 values.  One compiled kernel each way: see the module docstring."""
    g = 0.37
    for S in C.LIST_S:
        for N in C.N_LIST:
            for pattern in C.PATTERNS:
                c = cases[S, N, pattern]
                raw, z = c['raw'], c['z']
                depth, var, rgb, w = _fwd(raw, z)
                plain = _bwd(raw, z, depth, c['g_depth'], c['g_var'], c['g_rgb'])
                assert _same_bits(_bwd(raw, z, depth, c['g_depth'], c['g_var'], c['g_rgb'], work=_list_buffers(N, S)), plain)
                for gtc in (c['gt_color'], None):
                    gD, gC = _loss_cotangents(depth, rgb, c['gt_depth'], gtc, g)
                    want = _bwd(raw, z, depth, gD, None, gC)
                    assert _same_bits(_loss_bwd(raw, z, depth, rgb, c['gt_depth'], gtc, g), want), (S, N, pattern)
                    assert _same_bits(_loss_bwd(raw, z, depth, rgb, c['gt_depth'], gtc, g, work=_list_buffers(N, S)), want)


# ------------------------------------------------------------------------------------------------ the fused forward (fixture scene)
class _Scene:
    """the tiny fixture scene driven through the ABI as tests/test_hip_abi_direct.py drives it"""

    def __init__(self):
        from tests.hip_util import tiny_on_gpu
        L, lib, EF = _api()
        s, bound, model, grids, rays, renderer = tiny_on_gpu()
        kinds = (1, 2, 3)
        self.keep = (s, bound, model, grids)
        self.ro, self.rd = rays['rays_o'].contiguous(), rays['rays_d'].contiguous()
        self.gd, self.gc = rays['gt_depth'].contiguous().float(), rays['gt_color'].contiguous().float()
        grids_vm = {k: EF._grid_cache.get(grids[L.GRID_NAMES[k]]) for k in kinds}
        dims = {k: tuple(grids[L.GRID_NAMES[k]].shape[2:]) for k in kinds}
        packed = {k: EF.packed_decoder(getattr(model, L.MLP_NAMES[k]), k) for k in kinds}
        self.keep += (grids_vm, packed)
        self.sc = EF._scene_struct('color', EF.bound6(bound), EF.bound6(bound * 2), grids_vm, dims, packed)
        assert self.ro.shape[0] >= 33

    def z(self, N, S):
        """S sorted samples per ray from 0.3 to 1.5 of the ray's gt depth (1 where that is not positive)"""
        base = torch.where(self.gd[:N] > 0, self.gd[:N], torch.ones_like(self.gd[:N])).double()
        return (base[:, None] * torch.linspace(0.3, 1.5, S, dtype=torch.float64, device=DEV)[None]).contiguous()

    def loss_fwd(self, N, S, gt_depth=None, colour=True, unit=True, work=True):
        L, lib, EF = _api()
        P, st = EF._ptr, EF._stream()
        z = self.z(N, S)
        o = dict(z=z, depth=torch.empty(N, dtype=torch.float64, device=DEV), var=torch.empty(N, dtype=torch.float64, device=DEV),
                 rgb=torch.empty((N, 3), dtype=torch.float32, device=DEV),
                 raw=torch.full((N, S, 4), float('nan'), dtype=torch.float32, device=DEV),
                 loss=torch.zeros(1, dtype=torch.float64, device=DEV),
                 gd=(self.gd[:N] if gt_depth is None else gt_depth).contiguous(), gc=self.gc[:N].contiguous() if colour else None)
        o['unit'] = torch.full((N, S, 4), float('nan'), dtype=torch.float32, device=DEV) if unit else None
        o['wl'], o['wc'] = _list_buffers(N, S) if work else (None, None)
        L.check(lib.enslam_render_loss_fwd(3, N, S, P(self.ro[:N].contiguous()), P(self.rd[:N].contiguous()), P(z),
                                           ctypes.byref(self.sc), P(o['depth']), P(o['var']), P(o['rgb']), P(o['raw']), None, 0,
                                           P(o['gd']), P(o['gc']), C.W_COLOR, P(o['loss']), P(o['unit']), P(o['wl']), P(o['wc']),
                                           st), "enslam_render_loss_fwd")
        torch.cuda.synchronize()
        return o

    def plain_fwd(self, N, S):
        L, lib, EF = _api()
        P, st = EF._ptr, EF._stream()
        z = self.z(N, S)
        depth, var = torch.empty(N, dtype=torch.float64, device=DEV), torch.empty(N, dtype=torch.float64, device=DEV)
        rgb = torch.empty((N, 3), dtype=torch.float32, device=DEV)
        raw = torch.empty((N, S, 4), dtype=torch.float32, device=DEV)
        L.check(lib.enslam_render_fwd(3, N, S, P(self.ro[:N].contiguous()), P(self.rd[:N].contiguous()), P(z), ctypes.byref(self.sc),
                                      P(depth), P(var), P(rgb), P(raw), None, 0, st), "enslam_render_fwd")
        torch.cuda.synchronize()
        return _np(depth), _np(var), _np(rgb), _np(raw)


@pytest.fixture(scope="module")
def scene():
    return _Scene()


@pytest.mark.parametrize("colour", [True, False])
@pytest.mark.parametrize("N", C.N_LIST)
def test_fused_forward_forms_and_loss_value(scene, N, colour):
    """enslam_render_loss_fwd on the fixture scene (S = 48):
    * depth, var, rgb have the bits of enslam_render_fwd (plain one-wave form) and of enslam_composite_fwd re-run on the
      call's raw_out;
    * d_raw_unit has the bits of enslam_composite_loss_bwd with g_loss = 1 on the same raw, depth and rgb;
    * loss[0] is the float64 mapper loss of the yardstick on raw_out within the sum of the per-ray bars (the atomics'
      order only moves the last float64 bits, which the bar's float64 term covers)."""
    S = 48
    o = scene.loss_fwd(N, S, colour=colour)
    raw, z = _np(o['raw']), _np(o['z'])
    depth, var, rgb = _np(o['depth']), _np(o['var']), _np(o['rgb'])
    assert np.isfinite(raw).all()
    pd, pv, pc, praw = scene.plain_fwd(N, S)
    assert _same_bits(praw, raw)
    assert _same_bits(pd, depth) and _same_bits(pv, var) and _same_bits(pc, rgb)
    d2, v2, c2, _ = _fwd(raw, z)
    assert _same_bits(d2, depth) and _same_bits(v2, var) and _same_bits(c2, rgb)
    gd, gc = _np(o['gd']), (_np(o['gc']) if colour else None)
    unit = _np(o['unit'])
    assert _same_bits(unit, _loss_bwd(raw, z, depth, rgb, gd, gc, 1.0))
    f = Y.forward(raw, z)
    yl = Y.mapper_loss(f, gd, gc, C.W_COLOR)
    err = abs(float(o['loss']) - yl['loss'])
    print(f"N={N} colour={colour}: loss {float(o['loss']):.12g}, |got - ref| = {err:.3g}, bar = {yl['bar']:.3g}")
    assert err <= yl['bar']
    # the forward's own values on this real raw, under the same bars
    scales, bars, _ = Y.forward_bars(f)
    for k, got in (('depth', depth), ('var', var), ('rgb', rgb)):
        assert (np.abs(got - f[k]) <= bars[k]).all(), k


# ------------------------------------------------------------------------------------------------ work list
def _check_list(d_raw, S, wl, wc, where):
    """count == number of active tiles of the returned d_raw; listed set == that set; no entry twice; sentinel past count"""
    want = Y.active_tiles(d_raw, S)
    n = int(wc)
    lst = _np(wl)
    assert n == len(want), (where, n, len(want))
    got = lst[:n].tolist()
    assert len(set(got)) == n, where
    assert set(got) == want, where
    assert (lst[n:] == SENTINEL).all(), where
    return n


def _only_last(c):
    """cotangents / gt of case c with every ray but the last inert"""
    z = np.zeros_like
    gD, gV, gC, gtd = z(c['g_depth']), z(c['g_var']), z(c['g_rgb']), z(c['gt_depth'])
    gD[-1], gV[-1], gC[-1], gtd[-1] = 1.0, 0.1, 1.0, 9.0
    return gD, gV, gC, gtd


@pytest.mark.parametrize("S", C.LIST_S)
def test_work_list_of_the_backward_forms(cases, S):
    """enslam_composite_bwd_list and enslam_composite_loss_bwd, list prefilled with a sentinel and count 0: every N,
    every pattern (c: the tiles behind the run are absent; d: the list is empty), and a 17-ray batch in which only the
    last ray is active (the one ray of the second workgroup)."""
    empties = behind = 0
    for N in C.N_LIST:
        for pattern in C.PATTERNS:
            c = cases[S, N, pattern]
            raw, z = c['raw'], c['z']
            depth, var, rgb, w = _fwd(raw, z)
            work = _list_buffers(N, S)
            d = _bwd(raw, z, depth, c['g_depth'], c['g_var'], c['g_rgb'], work=work)
            n = _check_list(d, S, *work, ('bwd_list', S, N, pattern))
            for gtc in (c['gt_color'], None):
                work = _list_buffers(N, S)
                d = _loss_bwd(raw, z, depth, rgb, c['gt_depth'], gtc, 0.37, work=work)
                n = _check_list(d, S, *work, ('loss_bwd', S, N, pattern, gtc is None))
            if pattern == 'd':
                assert n == 0
                empties += 1
            if pattern == 'c' and S >= 32:
                last_tile = {r * (S // 16) + S // 16 - 1 for r in range(N)}
                assert (C.run_start(S) + 6) <= S - 16 and not (last_tile & set(_np(work[0])[:n].tolist()))
                behind += 1
    assert empties == len(C.N_LIST) and (behind > 0 or S == 16)
    c = cases[S, 17, 'a']
    gD, gV, gC, gtd = _only_last(c)
    depth, var, rgb, w = _fwd(c['raw'], c['z'])
    work = _list_buffers(17, S)
    d = _bwd(c['raw'], c['z'], depth, gD, gV, gC, work=work)
    n = _check_list(d, S, *work, ('bwd_list last ray', S))
    assert n > 0 and (_np(work[0])[:n] >= 16 * (S // 16)).all() and (d[:16] == 0).all()
    work = _list_buffers(17, S)
    d = _loss_bwd(c['raw'], c['z'], depth, rgb, gtd, None, 1.0, work=work)
    n = _check_list(d, S, *work, ('loss_bwd last ray', S))
    assert n > 0 and (_np(work[0])[:n] >= 16 * (S // 16)).all() and (d[:16] == 0).all()


@pytest.mark.parametrize("S", C.LIST_S)
def test_work_list_of_the_fused_forward(scene, S):
    """enslam_render_loss_fwd with d_raw_unit and a work list on the fixture scene: every N with and without colour, a
    batch whose list is empty (every gt_depth 0, no colour) and a 17-ray batch in which only the last ray is active."""
    for N in C.N_LIST:
        for colour in (True, False):
            o = scene.loss_fwd(N, S, colour=colour)
            n = _check_list(_np(o['unit']), S, o['wl'], o['wc'], ('fused', S, N, colour))
            assert n > 0 or not colour
        o = scene.loss_fwd(N, S, gt_depth=torch.zeros(N, device=DEV), colour=False)
        assert _check_list(_np(o['unit']), S, o['wl'], o['wc'], ('fused empty', S, N)) == 0
        assert (_np(o['unit']) == 0).all() and float(o['loss']) == 0.0
    gd = torch.zeros(17, device=DEV)
    gd[16] = scene.gd[16] if float(scene.gd[16]) > 0 else 1.0
    o = scene.loss_fwd(17, S, gt_depth=gd, colour=False)
    n = _check_list(_np(o['unit']), S, o['wl'], o['wc'], ('fused last ray', S))
    assert n > 0 and (_np(o['wl'])[:n] >= 16 * (S // 16)).all() and (_np(o['unit'])[:16] == 0).all()


def test_a_work_list_needs_whole_tiles():
    """with a work list n_samples must be a multiple of 16 (ENSLAM_EINVAL, nothing launched: the list keeps its sentinel);
    without one every S from 1 to 64 is served (the values test runs S = 1 ... 63 that way)"""
    L, lib, EF = _api()
    P, st = EF._ptr, EF._stream()
    for S in (1, 15, 17, 28, 63):
        N = 3
        raw = torch.zeros((N, S, 4), device=DEV)
        z = torch.ones((N, S), dtype=torch.float64, device=DEV)
        dep = torch.zeros(N, dtype=torch.float64, device=DEV)
        gd = torch.ones(N, device=DEV)
        d = torch.empty((N, S, 4), device=DEV)
        wl, wc = _list_buffers(N, 64)
        assert lib.enslam_composite_bwd_list(N, S, P(raw), P(z), P(dep), P(dep), None, None, P(d), P(wl), P(wc), st) == EINVAL
        assert lib.enslam_composite_loss_bwd(N, S, P(raw), P(z), P(dep), None, P(gd), None, 0.2, P(dep), P(d), P(wl), P(wc), st) == EINVAL
        assert lib.enslam_composite_bwd_list(N, S, P(raw), P(z), P(dep), P(dep), None, None, P(d), None, None, st) == 0
        torch.cuda.synchronize()
        assert int(wc) == 0 and (_np(wl) == SENTINEL).all()
