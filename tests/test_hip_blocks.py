"""-m gpu: the block flags and the block-sparse grid movement, bit-exact against the numpy yardstick (tests/blocks_numpy.py) on the
seeded cases of tests/blocks_cases.py, driven through the C ABI by hand.

  a  the marks of every route (enslam_mark_blocks_g, the sampler's inline marking in enslam_sample_rays_g and
     enslam_sample_prepare, the product path, parallel.batch_block_flags) equal the yardstick's flags at 64 / 32 / 16 / 8 voxels
     per flag; marking only sets flags, and leaves grids outside the stage (or without a flag array) alone
  b  the forward's gather reads flagged blocks only: voxel-major buffers that hold NaN outside the yardstick's blocks render
     the same bits as fully converted ones
  c  the backward's scatter writes only taps of the yardstick's corner set, all inside flagged blocks
  d  the movement kernels (enslam_grids_convert, enslam_grids_convert_sparse, enslam_zero_blocks, enslam_step_finish,
     enslam_step_finish_rays_prev, the flag move of enslam_step_finish_native) equal the yardstick's pure functions

Every array a kernel writes is a slice of a larger buffer filled with a sentinel; the slices on both sides must come back
unchanged (`Guarded.intact`).  Every comparison is for equality."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests import blocks_cases as K
from tests import blocks_numpy as Y

pytestmark = pytest.mark.gpu

GUARD = 512                                  # sentinel elements on either side of a guarded array
SENTINEL = {torch.uint8: 0xA5, torch.float32: 7777.0, torch.float64: 7777.0}
RENDER_STAGES = ('middle', 'fine', 'color')


def _env():
    import evennicer_slam_amd as E
    import evennicer_slam_amd.functional as EF
    from tests.hip_util import DEV
    return E._lib, E._lib.lib(), EF, DEV


class Guarded:
    """`t`: n elements inside a sentinel-filled buffer, `offset` elements off the allocation's alignment"""

    def __init__(self, n, dtype, fill=None, offset=0):
        from tests.hip_util import DEV
        self.buf = torch.full((GUARD + offset + n + GUARD,), SENTINEL[dtype], dtype=dtype, device=DEV)
        self.lo, self.n = GUARD + offset, n
        self.t = self.buf[self.lo:self.lo + n]
        if fill is not None:
            self.t.copy_(fill if torch.is_tensor(fill) else torch.as_tensor(np.ascontiguousarray(fill).reshape(-1), dtype=dtype))

    def ptr(self):
        return self.t.data_ptr()

    def intact(self):
        s = SENTINEL[self.buf.dtype]
        return bool((self.buf[:self.lo] == s).all()) and bool((self.buf[self.lo + self.n:] == s).all())

    def numpy(self):
        return self.t.cpu().numpy()


def _arr(*ptrs):
    return (ctypes.c_void_p * max(len(ptrs), 1))(*ptrs)


def _i64(*vals):
    return (ctypes.c_int64 * max(len(vals), 1))(*vals)


def _dbl6(b):
    return (ctypes.c_double * 6)(*[float(v) for v in np.asarray(b, dtype=np.float64).reshape(-1)])


def _same(got, want, what):
    """equality of a flag array (or any flat array) with a message that names the first element that differs"""
    got = got.numpy() if isinstance(got, Guarded) else (got.cpu().numpy() if torch.is_tensor(got) else np.asarray(got))
    got, want = got.reshape(-1), np.asarray(want).reshape(-1)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.flatnonzero(~((got == want) | ((got != got) & (want != want))))
    assert bad.size == 0, f"{what}: element / block {bad[0]} is {got[bad[0]]}, want {want[bad[0]]} ({bad.size} differ)"


def _before(nb, seed):
    """flags set before a marking call: marking must keep them"""
    f = np.zeros(nb, dtype=np.uint8)
    f[seed % 5::5] = 1
    return f


def _rays(c, rays=None):
    _, _, _, DEV = _env()
    sel = slice(None) if rays is None else rays
    ro = torch.from_numpy(np.ascontiguousarray(c['ro'][sel])).to(DEV)
    rd = torch.from_numpy(np.ascontiguousarray(c['rd'][sel])).to(DEV)
    z = torch.from_numpy(np.ascontiguousarray(c['z'][sel])).to(DEV)
    return ro, rd, z


def _mark_scene(c):
    L, _, _, _ = _env()
    msc = L.Scene()
    msc.bound, msc.coarse_bound = _dbl6(c['bound']), _dbl6(c['coarse_bound'])
    for k, d in c['dims'].items():
        msc.grids[k].D, msc.grids[k].H, msc.grids[k].W = (int(v) for v in d)
    return msc


def _flag_arrays(c, bs, seed):
    before = {k: _before(Y.n_blocks(K.n_voxels(d), bs), seed + k) for k, d in c['dims'].items()}
    return before, {k: Guarded(len(b), torch.uint8, b) for k, b in before.items()}


def _check_flags(flags, want, what):
    for k in sorted(want):
        if flags.get(k) is not None:
            _same(flags[k], want[k], f"{what}, grid {k}")
            assert flags[k].intact(), f"{what}, grid {k}: guard overwritten"


# ================================================================================================ a  marks
@pytest.mark.parametrize('stage', Y.STAGES)
@pytest.mark.parametrize('case', K.CASE_NAMES)
def test_mark_blocks_equals_the_yardstick(case, stage):
    L, lib, EF, DEV = _env()
    c = K.CASES[case]
    ro, rd, z = _rays(c)
    msc = _mark_scene(c)
    N, S = c['z'].shape
    for bs in Y.BLOCK_SIZES:
        before, flags = _flag_arrays(c, bs, 1)
        L.check(lib.enslam_mark_blocks_g(L.STAGE[stage], N, S, EF._ptr(ro), EF._ptr(rd), EF._ptr(z), ctypes.byref(msc),
                                         _arr(*[flags[k].ptr() for k in range(4)]), bs, EF._stream()), "enslam_mark_blocks_g")
        torch.cuda.synchronize()
        _check_flags(flags, K.expected_flags(case, stage, bs, before=before), f"mark_blocks_g {case} {stage} {bs} voxels per flag")
    # a grid of the stage without a flag array is skipped, the others are marked all the same
    skipped = Y.stage_grids(stage)[0]
    before, flags = _flag_arrays(c, 64, 2)
    ptrs = [None if k == skipped else flags[k].ptr() for k in range(4)]
    L.check(lib.enslam_mark_blocks_g(L.STAGE[stage], N, S, EF._ptr(ro), EF._ptr(rd), EF._ptr(z), ctypes.byref(msc), _arr(*ptrs), 64,
                                     EF._stream()), "enslam_mark_blocks_g")
    torch.cuda.synchronize()
    want = K.expected_flags(case, stage, 64, before=before)
    want[skipped] = before[skipped]
    _check_flags(flags, want, f"mark_blocks_g {case} {stage} without grid {skipped}")


def _sampler_call(c, stage, bs, guided, prepare):
    """enslam_sample_rays_g / enslam_sample_prepare on the case's sampler rays.  Returns what the call left and what the
    yardstick expects from the z the call returned."""
    L, lib, EF, DEV = _env()
    rays = c['sampler_rays']
    ro, rd, _ = _rays(c, rays)
    N, S = len(rays), c['S']
    n_lin, n_surf = (S // 2, S // 2) if guided else (S, 0)
    gd = torch.from_numpy(c['gt_depth'][rays].copy()).to(DEV) if guided else None
    t_lin = torch.linspace(0., 1., steps=n_lin, device=DEV)
    t_surf = torch.linspace(0., 1., steps=max(n_surf, 1), device=DEV).double() if guided else None
    scratch = torch.empty(2, dtype=torch.float32, device=DEV)
    z = Guarded(N * S, torch.float64)
    msc = _mark_scene(c)
    before, flags = _flag_arrays(c, bs, 3)
    before64, flags64 = _flag_arrays(c, 64, 4)
    f64 = _arr(*[flags64[k].ptr() for k in range(4)]) if bs < 64 else None
    head = (N, n_lin, n_surf, EF._ptr(ro), EF._ptr(rd), EF._ptr(gd), msc.bound, EF._ptr(t_lin), EF._ptr(t_surf), 0, None,
            EF._ptr(scratch), 0, z.ptr(), L.STAGE[stage], ctypes.byref(msc), _arr(*[flags[k].ptr() for k in range(4)]), bs, f64)
    extra = None
    if prepare:                             # a non-empty zero job rides in the same launch
        dims = [c['dims'][2], c['dims'][0]]
        V = [K.n_voxels(d) for d in dims]
        rng = np.random.default_rng(8)
        acc = [rng.standard_normal((v, Y.C)).astype(np.float32) for v in V]
        zneed = K.flag_pattern('random', dims, seed=5)
        flat0 = rng.standard_normal(300).astype(np.float32)
        g_acc = [Guarded(v * Y.C, torch.float32, a) for v, a in zip(V, acc)]
        g_need = [Guarded(len(f), torch.uint8, f) for f in zneed]
        g_flat = Guarded(255, torch.float32, flat0[:255])
        L.check(lib.enslam_sample_prepare(*head, 0, None, None, None, 2, _arr(*[g.ptr() for g in g_acc]), _i64(*V),
                                          _arr(*[g.ptr() for g in g_need]), g_flat.ptr(), 255, EF._stream()), "enslam_sample_prepare")
        want_acc, want_flat = Y.zero_blocks(acc, zneed, flat0[:255], 255)
        extra = (g_acc, g_need, g_flat, want_acc, zneed, want_flat)
    else:
        L.check(lib.enslam_sample_rays_g(*head, EF._stream()), "enslam_sample_rays_g")
    torch.cuda.synchronize()
    zz = z.numpy().reshape(N, S)
    assert np.isfinite(zz).all() and z.intact()
    want = K.expected_flags(c, stage, bs, z=zz, rays=rays, before=before)
    want64 = K.expected_flags(c, stage, 64, z=zz, rays=rays, before=before64) if bs < 64 else before64
    return flags, want, flags64, want64, extra


@pytest.mark.parametrize('guided', [True, False], ids=['gt_depth', 'no_depth'])
@pytest.mark.parametrize('stage', Y.STAGES)
@pytest.mark.parametrize('case', K.RAY_CASES)
def test_sampler_marks_equal_the_yardstick(case, stage, guided):
    c = K.CASES[case]
    for bs in Y.BLOCK_SIZES:
        what = f"sample_rays_g {case} {stage} {bs} voxels per flag"
        flags, want, flags64, want64, _ = _sampler_call(c, stage, bs, guided, prepare=False)
        _check_flags(flags, want, what)
        _check_flags(flags64, want64, what + " (64-voxel form)")        # bs == 64: flags64 is not used and stays as it was


@pytest.mark.parametrize('guided', [True, False], ids=['gt_depth', 'no_depth'])
@pytest.mark.parametrize('stage', Y.STAGES)
@pytest.mark.parametrize('case', K.RAY_CASES)
def test_sample_prepare_marks_and_clears(case, stage, guided):
    c = K.CASES[case]
    for bs in Y.BLOCK_SIZES:
        what = f"sample_prepare {case} {stage} {bs} voxels per flag"
        flags, want, flags64, want64, (g_acc, g_need, g_flat, want_acc, zneed, want_flat) = _sampler_call(c, stage, bs, guided, True)
        _check_flags(flags, want, what)
        _check_flags(flags64, want64, what + " (64-voxel form)")
        for i, g in enumerate(g_acc):
            _same(g, want_acc[i], f"{what}: cleared accumulator {i}")
            _same(g_need[i], zneed[i], f"{what}: zero_need {i}")
            assert g.intact() and g_need[i].intact()
        _same(g_flat, want_flat, what + ": flat range")
        assert g_flat.intact()


def test_sample_calls_without_rays_leave_everything_alone():
    L, lib, EF, DEV = _env()
    c = K.CASES['no_rays']
    msc = _mark_scene(c)
    before, flags = _flag_arrays(c, 16, 6)
    fp = _arr(*[flags[k].ptr() for k in range(4)])
    t_lin = torch.linspace(0., 1., steps=16, device=DEV)
    L.check(lib.enslam_sample_rays_g(0, 16, 0, None, None, None, msc.bound, EF._ptr(t_lin), None, 0, None, None, 0, None, 3,
                                     ctypes.byref(msc), fp, 16, None, EF._stream()), "enslam_sample_rays_g")
    acc = Guarded(K.n_voxels(c['dims'][1]) * Y.C, torch.float32, np.ones(K.n_voxels(c['dims'][1]) * Y.C, np.float32))
    L.check(lib.enslam_sample_prepare(0, 16, 0, None, None, None, msc.bound, EF._ptr(t_lin), None, 0, None, None, 0, None, 3,
                                      ctypes.byref(msc), fp, 16, None, 0, None, None, None, 1, _arr(acc.ptr()),
                                      _i64(K.n_voxels(c['dims'][1])), None, None, 0, EF._stream()), "enslam_sample_prepare")
    torch.cuda.synchronize()
    _check_flags(flags, before, "no rays")
    assert not acc.numpy().any() and acc.intact()           # the prepare role still runs


@functools.lru_cache(maxsize=None)
def _product(scene):
    """(bound tensor, NICE with the fixture's weights, Renderer, dense grids) over a scene of the cases"""
    from tests.hip_util import DEV, model_from_state, renderer_for
    from tests.util import load
    L, _, _, _ = _env()
    sc = K.SCENES[scene]
    bound = torch.from_numpy(sc['bound'].copy())
    model = model_from_state(load('tiny_scene'), bound)
    gen = torch.Generator().manual_seed(11)
    grids = {L.GRID_NAMES[k]: (0.1 * torch.randn((1, Y.C) + tuple(d), generator=gen)).to(DEV) for k, d in sc['dims'].items()}
    return bound, model, renderer_for(bound), grids


def _product_z(c, stage, ro, rd, gd):
    _, _, EF, _ = _env()
    bound = _product(c['scene'])[0]
    return EF.sample_rays(ro, rd, None if stage == 'coarse' else gd, bound, 32, 0 if stage == 'coarse' else 16).cpu().numpy()


@pytest.mark.parametrize('stage', Y.STAGES)
@pytest.mark.parametrize('case', K.RAY_CASES)
def test_product_path_flags_equal_the_yardstick(case, stage):
    L, lib, EF, DEV = _env()
    from evennicer_slam_amd import parallel as PAR
    c = K.CASES[case]
    bound, model, renderer, grids = _product(c['scene'])
    rays = c['sampler_rays']
    ro, rd, _ = _rays(c, rays)
    gd = torch.from_numpy(c['gt_depth'][rays].copy()).to(DEV)
    zz = _product_z(c, stage, ro, rd, gd)
    assert np.isfinite(zz).all()
    cg = {k: v.clone().requires_grad_(True) for k, v in grids.items()}
    renderer.render_batch_ray(cg, model, rd, ro, DEV, stage, gt_depth=gd)
    got = EF.last_block_flags()
    torch.cuda.synchronize()
    want = K.expected_flags(c, stage, 64, z=zz, rays=rays)
    assert set(got) == {id(cg[L.GRID_NAMES[k]]) for k in Y.stage_grids(stage)}
    for k in Y.stage_grids(stage):
        _same(got[id(cg[L.GRID_NAMES[k]])], want[k], f"render_batch_ray {case} {stage}, grid {k}")
    for bs in (64, 16):
        fl = PAR.batch_block_flags(renderer, grids, model, ro, rd, gd, stage, block_voxels=bs)
        torch.cuda.synchronize()
        wb = K.expected_flags(c, stage, bs, z=zz, rays=rays)
        for k in Y.stage_grids(stage):
            g = grids[L.GRID_NAMES[k]]
            _same(fl[id(g)], wb[k], f"batch_block_flags {case} {stage} {bs} voxels per flag, grid {k}")
            if bs != 64:
                _same(fl[('c64', id(g))], want[k], f"batch_block_flags {case} {stage} 64-voxel form, grid {k}")


# ================================================================================================ b, c  gather and scatter
@functools.lru_cache(maxsize=None)
def _dense_grids(scene):
    rng = np.random.default_rng(21)
    return {k: rng.standard_normal((Y.C, K.n_voxels(d))).astype(np.float32) * np.float32(0.1) for k, d in K.SCENES[scene]['dims'].items()}


def _voxel_major(c, kinds, need):
    """{k: Guarded voxel-major buffer}: need None -> every block converted (enslam_grids_convert); else NaN everywhere but the
    needed blocks (enslam_grids_convert_sparse)"""
    L, lib, EF, DEV = _env()
    dense = {k: torch.from_numpy(_dense_grids(c['scene'])[k]).to(DEV) for k in kinds}
    V = [K.n_voxels(c['dims'][k]) for k in kinds]
    out = {k: Guarded(v * Y.C, torch.float32, None if need is None else np.full(v * Y.C, np.nan, np.float32)) for k, v in zip(kinds, V)}
    src, dst = _arr(*[dense[k].data_ptr() for k in kinds]), _arr(*[out[k].ptr() for k in kinds])
    if need is None:
        L.check(lib.enslam_grids_convert(len(kinds), src, dst, _i64(*V), 1, EF._stream()), "enslam_grids_convert")
    else:
        fl = [torch.from_numpy(need[k]).to(DEV) for k in kinds]
        L.check(lib.enslam_grids_convert_sparse(len(kinds), src, dst, _i64(*V), _arr(*[f.data_ptr() for f in fl]), None, 1,
                                                EF._stream()), "enslam_grids_convert_sparse")
    torch.cuda.synchronize()
    return out


def _scene(c, stage, vm):
    L, lib, EF, DEV = _env()
    _, model, _, _ = _product(c['scene'])
    kinds = Y.stage_grids(stage)
    packed = {k: EF.packed_decoder(getattr(model, L.MLP_NAMES[k]), k) for k in kinds}
    sc = L.Scene()
    sc.bound, sc.coarse_bound = _dbl6(c['bound']), _dbl6(c['coarse_bound'])
    for k in kinds:
        sc.grids[k].data = vm[k].ptr()
        sc.grids[k].D, sc.grids[k].H, sc.grids[k].W = (int(v) for v in c['dims'][k])
        sc.packed[k] = packed[k].data_ptr()
    return sc, packed


def _render_fwd(c, stage, sc, with_raw, act=None):
    L, lib, EF, DEV = _env()
    ro, rd, z = _rays(c)
    N, S = c['z'].shape
    depth = torch.empty(N, dtype=torch.float64, device=DEV)
    var = torch.empty(N, dtype=torch.float64, device=DEV)
    rgb = torch.empty((N, 3), dtype=torch.float32, device=DEV)
    raw = torch.empty((N * S, 4), dtype=torch.float32, device=DEV) if with_raw else None
    L.check(lib.enslam_render_fwd(L.STAGE[stage], N, S, EF._ptr(ro), EF._ptr(rd), EF._ptr(z), ctypes.byref(sc), EF._ptr(depth),
                                  EF._ptr(var), EF._ptr(rgb), EF._ptr(raw), EF._ptr(act), 0, EF._stream()), "enslam_render_fwd")
    torch.cuda.synchronize()
    return depth, var, rgb, raw


@pytest.mark.parametrize('stage', RENDER_STAGES)
@pytest.mark.parametrize('case', K.RAY_CASES)
def test_the_gather_reads_flagged_blocks_only(case, stage):
    L, lib, EF, DEV = _env()
    c = K.CASES[case]
    kinds = Y.stage_grids(stage)
    need = K.expected_flags(case, stage, 64)
    full, sparse = _voxel_major(c, kinds, None), _voxel_major(c, kinds, need)
    for k in kinds:                          # the sparse buffers hold the grid in the flagged blocks and NaN everywhere else
        V = K.n_voxels(c['dims'][k])
        m = np.repeat(need[k].astype(bool), Y.BLOCK)[:V]
        want = np.where(m[:, None], _dense_grids(c['scene'])[k].T, np.float32(np.nan))
        _same(sparse[k], want, f"convert_sparse {case} {stage}, grid {k}")
        _same(full[k], _dense_grids(c['scene'])[k].T, f"grids_convert {case} {stage}, grid {k}")
        assert sparse[k].intact() and full[k].intact()
    sc_full, keep_f = _scene(c, stage, full)
    sc_sparse, keep_s = _scene(c, stage, sparse)
    for with_raw in (True, False):
        if not with_raw and c['S'] == 64:    # 64 samples per ray exist in the tile-per-wave form alone: refused, not run
            N = c['z'].shape[0]
            ro, rd, z = _rays(c)
            out = torch.empty(N * 5, dtype=torch.float64, device=DEV)
            assert lib.enslam_render_fwd(L.STAGE[stage], N, 64, EF._ptr(ro), EF._ptr(rd), EF._ptr(z), ctypes.byref(sc_sparse), EF._ptr(out),
                                         EF._ptr(out[N:]), EF._ptr(out[2 * N:]), None, None, 0, EF._stream()) == -3
            continue
        a = _render_fwd(c, stage, sc_full, with_raw)
        b = _render_fwd(c, stage, sc_sparse, with_raw)
        for name, x, y in zip(('depth', 'var', 'rgb', 'raw'), a, b):
            if x is None:
                continue
            assert bool(torch.isfinite(y).all()), f"render_fwd {case} {stage} raw={with_raw}: {name} read an unflagged block"
            assert torch.equal(x, y), f"render_fwd {case} {stage} raw={with_raw}: {name}"
    pts = torch.from_numpy(K.points(case)[:-3].copy()).to(DEV)           # a point count that is no multiple of 16
    assert pts.shape[0] % 16 != 0
    outs = []
    for sc in (sc_full, sc_sparse):
        for mask in (1, 0):
            raw = torch.empty((pts.shape[0], 4), dtype=torch.float32, device=DEV)
            L.check(lib.enslam_eval_points(L.STAGE[stage], pts.shape[0], EF._ptr(pts), ctypes.byref(sc), mask, EF._ptr(raw), EF._stream()),
                    "enslam_eval_points")
            outs.append(raw)
    torch.cuda.synchronize()
    for x, y in ((outs[0], outs[2]), (outs[1], outs[3])):
        assert bool(torch.isfinite(y).all()), f"eval_points {case} {stage}: read an unflagged block"
        assert torch.equal(x, y), f"eval_points {case} {stage}"


def _scatter_is_inside(grad_rows, c, k, pts, need, what):
    """grad_rows bool [V]: voxels with a non-zero gradient"""
    V = K.n_voxels(c['dims'][k])
    taps = Y.corner_voxels(pts, Y.lookup_bound(k, c['bound'], c['coarse_bound']), c['dims'][k])
    stray = np.flatnonzero(grad_rows & ~taps)
    assert stray.size == 0, f"{what}, grid {k}: voxel {stray[0]} (block {stray[0] // 64}) is no tap of any sample ({stray.size} such)"
    blocks = np.unique(np.flatnonzero(grad_rows) // 64)
    assert need[k][blocks].all(), f"{what}, grid {k}: block {blocks[~need[k][blocks].astype(bool)][:1]} holds a gradient and is not flagged"
    assert grad_rows.any() and V == grad_rows.size, f"{what}, grid {k}: no gradient at all"


@pytest.mark.parametrize('with_workspace', [True, False], ids=['workspace', 'recompute'])
@pytest.mark.parametrize('stage', RENDER_STAGES)
@pytest.mark.parametrize('case', K.RAY_CASES)
def test_the_scatter_writes_flagged_blocks_only(case, stage, with_workspace):
    L, lib, EF, DEV = _env()
    c = K.CASES[case]
    kinds = Y.stage_grids(stage)
    kstage = L.STAGE[stage]
    N, S = c['z'].shape
    ro, rd, z = _rays(c)
    need = K.expected_flags(case, stage, 64)
    full = _voxel_major(c, kinds, None)
    sc, keep = _scene(c, stage, full)
    act = torch.empty(lib.enslam_activation_floats(kstage, N, S, 0), dtype=torch.float32, device=DEV) if with_workspace else None
    depth, var, rgb, raw = _render_fwd(c, stage, sc, True, act)
    gen = torch.Generator().manual_seed(7)
    gD = torch.randn(N, generator=gen).double().to(DEV)
    gV = (0.1 * torch.randn(N, generator=gen)).double().to(DEV)
    gC = torch.randn(N, 3, generator=gen).to(DEV)
    gg = (L.Grid * 4)()
    gpk = (ctypes.c_void_p * 4)()
    acc, acc_p = {}, {}
    for k in kinds:
        V = K.n_voxels(c['dims'][k])
        acc[k] = Guarded(V * Y.C, torch.float32, np.zeros(V * Y.C, np.float32))
        acc_p[k] = torch.zeros(lib.enslam_packed_grad_floats(k), dtype=torch.float32, device=DEV)
        gg[k].data, (gg[k].D, gg[k].H, gg[k].W) = acc[k].ptr(), tuple(int(v) for v in c['dims'][k])
        gpk[k] = acc_p[k].data_ptr()
    g_ro = torch.zeros((N, 3), dtype=torch.float32, device=DEV)
    g_rd = torch.zeros((N, 3), dtype=torch.float32, device=DEV)
    d_raw = torch.empty((N * S, 4), dtype=torch.float32, device=DEV)
    dgw = torch.empty(lib.enslam_grid_handoff_floats(kstage, N, S), dtype=torch.float32, device=DEV) if with_workspace else None
    P = EF._ptr
    L.check(lib.enslam_render_bwd(kstage, N, S, P(ro), P(rd), P(z), ctypes.byref(sc), P(raw), P(depth), P(gD), P(gV), P(gC), gg, gpk,
                                  P(g_ro), P(g_rd), P(d_raw), P(act), 0, P(dgw), EF._stream()), "enslam_render_bwd")
    torch.cuda.synchronize()
    pts = K.points(case)
    for k in kinds:
        rows = (acc[k].numpy().reshape(-1, Y.C) != 0).any(axis=1)
        _scatter_is_inside(rows, c, k, pts, need, f"render_bwd {case} {stage}")
        assert acc[k].intact(), f"render_bwd {case} {stage}, grid {k}: guard overwritten"


@pytest.mark.parametrize('layout', ['contiguous', 'channels_last_3d'])
@pytest.mark.parametrize('stage', RENDER_STAGES)
@pytest.mark.parametrize('case', K.RAY_CASES)
def test_product_path_gradients_stay_inside_the_flagged_blocks(case, stage, layout):
    L, lib, EF, DEV = _env()
    from tests.hip_util import as_layout
    c = K.CASES[case]
    bound, model, renderer, grids = _product(c['scene'])
    rays = c['sampler_rays']
    ro, rd, _ = _rays(c, rays)
    gd = torch.from_numpy(c['gt_depth'][rays].copy()).to(DEV)
    zz = _product_z(c, stage, ro, rd, gd)
    cg = {k: as_layout(v, layout).requires_grad_(True) for k, v in grids.items()}
    depth, var, color = renderer.render_batch_ray(cg, model, rd, ro, DEV, stage, gt_depth=gd)
    (depth.sum() + var.sum() + color.sum().double()).backward()
    torch.cuda.synchronize()
    for p in model.parameters():
        p.grad = None
    pts = Y.sample_points(c['ro'][rays], c['rd'][rays], zz)
    need = K.expected_flags(c, stage, 64, z=zz, rays=rays)
    for k in Y.stage_grids(stage):
        g = cg[L.GRID_NAMES[k]].grad
        assert g is not None and g.shape == cg[L.GRID_NAMES[k]].shape
        rows = (g.reshape(Y.C, -1) != 0).any(dim=0).cpu().numpy()
        _scatter_is_inside(rows, c, k, pts, need, f"render_batch_ray backward {case} {stage} {layout}")


# ================================================================================================ d  movement
def _movement(gset, seed=3):
    dims_list = K.GRID_SETS[gset]
    rng = np.random.default_rng(seed)
    V = [K.n_voxels(d) for d in dims_list]
    dense = [rng.standard_normal((Y.C, v)).astype(np.float32) for v in V]
    vm = [rng.standard_normal((v, Y.C)).astype(np.float32) for v in V]
    return dims_list, V, dense, vm


def _guarded(arrays, dtype, offset=0):
    return [Guarded(a.size, dtype, a, offset) for a in arrays]


def _ptrs(gs):
    return _arr(*[g.ptr() for g in gs])


def _check_all(gs, want, what):
    for i, (g, w) in enumerate(zip(gs, want)):
        _same(g, w, f"{what}, grid {i}")
        assert g.intact(), f"{what}, grid {i}: guard overwritten"


@pytest.mark.parametrize('gset', list(K.GRID_SETS))
def test_grids_convert_both_directions(gset):
    L, lib, EF, DEV = _env()
    dims_list, V, dense, vm = _movement(gset)
    n = len(V)
    src = _guarded(dense, torch.float32)
    dst = _guarded(vm, torch.float32)
    L.check(lib.enslam_grids_convert(n, _ptrs(src), _ptrs(dst), _i64(*V), 1, EF._stream()), "enslam_grids_convert")
    torch.cuda.synchronize()
    _check_all(dst, [Y.to_voxel_major(d) for d in dense], f"grids_convert to voxel-major {gset}")
    _check_all(src, dense, f"grids_convert source {gset}")
    src = _guarded(vm, torch.float32)
    dst = _guarded(dense, torch.float32)
    L.check(lib.enslam_grids_convert(n, _ptrs(src), _ptrs(dst), _i64(*V), 0, EF._stream()), "enslam_grids_convert")
    torch.cuda.synchronize()
    _check_all(dst, [Y.from_voxel_major(v) for v in vm], f"grids_convert from voxel-major {gset}")


@pytest.mark.parametrize('pattern', K.PATTERNS)
@pytest.mark.parametrize('gset', list(K.GRID_SETS))
def test_grids_convert_sparse_equals_the_yardstick(gset, pattern):
    L, lib, EF, DEV = _env()
    dims_list, V, dense, vm = _movement(gset)
    n = len(V)
    need = K.flag_pattern(pattern, dims_list, seed=1)
    for with_valid in (True, False):
        what = f"grids_convert_sparse {gset} {pattern} valid={with_valid}"
        valid = K.flag_pattern('random', dims_list, seed=2) if with_valid else None
        src, dst, g_need = _guarded(dense, torch.float32), _guarded(vm, torch.float32), _guarded(need, torch.uint8)
        g_valid = _guarded(valid, torch.uint8) if with_valid else None

        def call():
            L.check(lib.enslam_grids_convert_sparse(n, _ptrs(src), _ptrs(dst), _i64(*V), _ptrs(g_need),
                                                    _ptrs(g_valid) if with_valid else None, 1, EF._stream()), "enslam_grids_convert_sparse")
            torch.cuda.synchronize()

        call()
        want, want_valid = Y.convert_sparse_to_vm(dense, vm, need, valid)
        _check_all(dst, want, what)
        _check_all(g_need, need, what + ": need")
        if with_valid:
            _check_all(g_valid, want_valid, what + ": valid")
            for s in src:                    # a second call has nothing left to convert: a changed source must not show
                s.t.add_(1.0)
        call()
        _check_all(dst, want, what + ", second call")
        if with_valid:
            _check_all(g_valid, want_valid, what + ": valid after the second call")
            again, again_valid = Y.convert_sparse_to_vm([d + 1 for d in dense], want, need, want_valid)
            assert all(np.array_equal(a, b) for a, b in zip(again, want)) and all(np.array_equal(a, b) for a, b in zip(again_valid, want_valid))


@pytest.mark.parametrize('pattern', K.PATTERNS)
@pytest.mark.parametrize('gset', list(K.GRID_SETS))
def test_zero_blocks_equals_the_yardstick(gset, pattern):
    L, lib, EF, DEV = _env()
    dims_list, V, dense, vm = _movement(gset)
    n = len(V)
    need = K.flag_pattern(pattern, dims_list, seed=1)
    flat0 = np.random.default_rng(9).standard_normal(2049).astype(np.float32)
    for n_flat in (0, 1, 255, 2048, 2049):
        for with_need in (True, False):
            what = f"zero_blocks {gset} {pattern} need={with_need} n_flat={n_flat}"
            dst, g_need = _guarded(vm, torch.float32), _guarded(need, torch.uint8)
            flat = Guarded(n_flat, torch.float32, flat0[:n_flat])
            L.check(lib.enslam_zero_blocks(n, _ptrs(dst), _i64(*V), _ptrs(g_need) if with_need else None,
                                           flat.ptr() if n_flat else None, n_flat, EF._stream()), "enslam_zero_blocks")
            torch.cuda.synchronize()
            want, want_flat = Y.zero_blocks(vm, need if with_need else None, flat0[:n_flat], n_flat)
            _check_all(dst, want, what)
            _check_all(g_need, need, what + ": need")
            _same(flat, want_flat, what + ": flat range")
            assert flat.intact(), what + ": flat guard overwritten"
    # the flat range alone, and one grid of the launch without flags (all of its blocks are cleared)
    flat = Guarded(2049, torch.float32, flat0)
    L.check(lib.enslam_zero_blocks(0, None, None, None, flat.ptr(), 2049, EF._stream()), "enslam_zero_blocks")
    dst, g_need = _guarded(vm, torch.float32), _guarded(need, torch.uint8)
    mixed = [None if i == n - 1 else g_need[i].ptr() for i in range(n)]
    L.check(lib.enslam_zero_blocks(n, _ptrs(dst), _i64(*V), _arr(*mixed), None, 0, EF._stream()), "enslam_zero_blocks")
    torch.cuda.synchronize()
    assert not flat.numpy().any() and flat.intact()
    _check_all(dst, Y.zero_blocks(vm, need[:-1] + [None])[0], f"zero_blocks {gset} {pattern}, last grid without flags")


@pytest.mark.parametrize('pattern', K.PATTERNS)
@pytest.mark.parametrize('gset', list(K.GRID_SETS))
def test_step_finish_equals_the_yardstick(gset, pattern):
    L, lib, EF, DEV = _env()
    dims_list, V, dense, vm = _movement(gset)
    n = len(V)
    need = K.flag_pattern(pattern, dims_list, seed=1)
    for offset in (0, 1):                    # 1: a destination that is not 16-byte aligned
        what = f"step_finish {gset} {pattern} offset={offset}"
        src, dst, g_need = _guarded(vm, torch.float32), _guarded(dense, torch.float32, offset), _guarded(need, torch.uint8)
        L.check(lib.enslam_step_finish(n, _ptrs(src), _ptrs(dst), _i64(*V), _ptrs(g_need), 0, None, None, None, EF._stream()),
                "enslam_step_finish")
        torch.cuda.synchronize()
        _check_all(dst, Y.finish(vm, dense, need), what)
        _check_all(g_need, need, what + ": need")
        _check_all(src, vm, what + ": source")


@pytest.mark.parametrize('offset', [0, 1], ids=['aligned', 'off_by_one_float'])
@pytest.mark.parametrize('gset', ['partial', 'whole_blocks', 'exact_4', 'room0_4', 'small_4'])
def test_step_finish_rays_prev_sequence_equals_the_yardstick(gset, offset):
    L, lib, EF, DEV = _env()
    dims_list, V, dense0, vm = _movement(gset)
    n = len(V)
    seq = [K.flag_pattern('random', dims_list, seed=s) for s in (31, 32, 33)]
    if gset in ('partial', 'exact_4'):
        assert V[0] % 4 != 0                 # the zero-fill cannot take its 16-byte path
    for f in seq[1:]:
        f[0][:2] = 0                         # blocks 0 and 1 of grid 0: untouched in the second and third call
    seq[0][0][:1], seq[0][0][1:2] = 1, 0
    dense = [np.zeros_like(d) for d in dense0]
    prev = [np.zeros(Y.n_blocks(v), np.uint8) for v in V]
    src = _guarded(vm, torch.float32)
    g_dense, g_prev = _guarded(dense, torch.float32, offset), _guarded(prev, torch.uint8)
    planted = 0
    for it, need in enumerate(seq):
        what = f"step_finish_rays_prev {gset} offset={offset}, call {it}"
        if it == 2:                          # untouched now and in the call before: not written, a planted value survives
            for i in range(n):
                for blk in np.flatnonzero((seq[1][i] == 0) & (seq[2][i] == 0)):
                    v = Y.block_voxels_of(int(blk), V[i])
                    dense[i][:, v] = 123.0
                    planted += v.size
                g_dense[i].t.copy_(torch.from_numpy(dense[i].reshape(-1)))
            assert planted >= 64
        g_need = _guarded(need, torch.uint8)
        L.check(lib.enslam_step_finish_rays_prev(n, _ptrs(src), _ptrs(g_dense), _i64(*V), _ptrs(g_need), _ptrs(g_prev), 0, None, None,
                                                 None, 3, 0, 48, None, None, None, None, None, None, None, None, None, EF._stream()),
                "enslam_step_finish_rays_prev")
        torch.cuda.synchronize()
        dense, want_need, prev = Y.finish_prev(vm, dense, need, prev)
        _check_all(g_dense, dense, what)
        _check_all(g_need, want_need, what + ": need")
        _check_all(g_prev, prev, what + ": prev")
        if it == 2:
            assert sum(int((d == 123.0).sum()) for d in dense) == planted * Y.C
    _check_all(src, vm, f"step_finish_rays_prev {gset}: source")


@pytest.mark.parametrize('n_move', [1, 255, 256, 257])
def test_step_finish_native_moves_the_flags(n_move):
    L, lib, EF, DEV = _env()
    rng = np.random.default_rng(n_move)
    need = (rng.uniform(size=300) < 0.4).astype(np.uint8)
    prev = (rng.uniform(size=300) < 0.4).astype(np.uint8)
    g_need, g_prev = Guarded(n_move, torch.uint8, need[:n_move]), Guarded(n_move, torch.uint8, prev[:n_move])
    L.check(lib.enslam_step_finish_native(0, None, None, None, None, None, 0, None, None, None, None, 3, 0, 48, None, None, None, None,
                                          None, None, None, None, None, g_need.ptr(), g_prev.ptr(), n_move, EF._stream()),
            "enslam_step_finish_native")
    torch.cuda.synchronize()
    want_need, want_prev = Y.move_flags(need[:n_move], prev[:n_move], n_move)
    _same(g_need, want_need, f"flag move n_move={n_move}: need")
    _same(g_prev, want_prev, f"flag move n_move={n_move}: prev")
    assert g_need.intact() and g_prev.intact()
