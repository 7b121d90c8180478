"""-m gpu: the NICE decoder forward (render_fwd_ring_kernel, render_fwd_res_kernel, render_fwd_kernel) against the float64
yardstick of tests/decoder_numpy.py, elementwise, at tile, group and route edges.  Cases and the bar: tests/decoder_cases.py
(|device - yardstick| <= 8 * e_ref[col], e_ref the float32 CPU oracle's own worst error over the case's pool).
Run with -s to see the worst |error| / e_ref of every case."""
import ctypes

import numpy as np
import pytest
import torch

from tests import blocks_numpy as BN
from tests import decoder_cases as DC
from tests import decoder_numpy as DN

pytestmark = pytest.mark.gpu

XYZ_STAGES = ('middle', 'fine', 'color')
TILE_EDGES = (1, 15, 16, 17, 63, 64, 65, 127, 1025)     # 16: a tile; 64: a workgroup's four tiles; 65: three idle waves in the last group
COARSE_EDGES = (1, 47, 48, 49, 97)                       # the coarse kernel's units are 48 points
CHUNK = 65536                                            # 4096 tiles: a chunk of this size stays on the ring kernel
GUARD = 64                                               # rows behind raw_out that no lane may write
SENTINEL = -7.25


@pytest.fixture(scope='module')
def dev():
    """models of both families and the grids on the GPU"""
    import evennicer_slam_amd as E
    import evennicer_slam_amd.functional as EF
    from tests.hip_util import DEV, model_from_state
    bound = torch.from_numpy(DC.scene()[2].copy())
    models = {f: model_from_state(DC.state_arrays(f), bound) for f in ('generic', 'exact')}
    grids = {k: torch.from_numpy(v.copy()).to(DEV) for k, v in DC.scene()[1].items()}
    T = int(E._lib.lib().enslam_fwd_res_min_tiles())
    assert T > CHUNK // 16, "the chunks of the bitwise comparisons must stay below the weight-stationary kernel's threshold"
    return dict(E=E, EF=EF, L=E._lib, lib=E._lib.lib(), DEV=DEV, bound=bound, coarse_bound=bound * 2, models=models, grids=grids, T=T)


def scene_struct(dev, family, stage):
    EF, L = dev['EF'], dev['L']
    kinds = L.STAGE_KINDS[stage]
    grids_vm = {k: EF._grid_cache.get(dev['grids'][L.GRID_NAMES[k]]) for k in kinds}
    dims = {k: tuple(dev['grids'][L.GRID_NAMES[k]].shape[2:]) for k in kinds}
    packed = {k: EF.packed_decoder(getattr(dev['models'][family], L.MLP_NAMES[k]), k) for k in kinds}
    sc = EF._scene_struct(stage, EF.bound6(dev['bound']), EF.bound6(dev['coarse_bound']), grids_vm, dims, packed)
    return sc, (grids_vm, packed)                        # (the second value keeps the device buffers alive)


def eval_points(dev, family, points, stage, apply_mask=True):
    """EF.eval_points on float64 points (numpy or device tensor) -> device float32 [P, 4]"""
    p = points if torch.is_tensor(points) else torch.from_numpy(np.array(points, dtype=np.float64)).to(dev['DEV'])
    with torch.no_grad():
        return dev['EF'].eval_points(p, dev['models'][family], dev['grids'], stage, dev['bound'], apply_mask=apply_mask)


def eval_points_guarded(dev, family, points, stage, apply_mask):
    """enslam_eval_points by hand into a buffer with GUARD sentinel rows behind the P rows: (raw [P, 4], guard rows) on the host"""
    EF, L, lib = dev['EF'], dev['L'], dev['lib']
    p = torch.from_numpy(np.array(points, dtype=np.float64)).to(dev['DEV'])
    P = p.shape[0]
    sc, keep = scene_struct(dev, family, stage)
    buf = torch.full((P + GUARD, 4), SENTINEL, dtype=torch.float32, device=dev['DEV'])
    L.check(lib.enslam_eval_points(L.STAGE[stage], P, EF._ptr(p), ctypes.byref(sc), int(apply_mask), EF._ptr(buf), EF._stream()),
            "enslam_eval_points")
    torch.cuda.synchronize()
    out = buf.cpu().numpy()
    return out[:P], out[P:]


def chunked(dev, family, points, stage, apply_mask=True):
    """eval_points in chunks of CHUNK points (device tensor in, device tensor out): every chunk runs on the ring kernel"""
    return torch.cat([eval_points(dev, family, points[i:i + CHUNK], stage, apply_mask) for i in range(0, points.shape[0], CHUNK)])


# ------------------------------------------------------------------------------------------------ a. values
def _value_cases():
    for stage in DC.STAGES:
        for P in (COARSE_EDGES if stage == 'coarse' else TILE_EDGES):
            yield stage, P


@pytest.mark.parametrize("apply_mask", [True, False], ids=['mask', 'nomask'])
@pytest.mark.parametrize("name", DC.POOLS)
@pytest.mark.parametrize("stage,P", list(_value_cases()))
def test_eval_points_values(dev, stage, P, name, apply_mask):
    points = DC.pool(name, stage)[:P]
    want, eref = DC.yardstick(name, stage, apply_mask)[:P], DC.e_ref(name, stage)
    masked = DC.masked_rows(points, apply_mask)
    got, guard = eval_points_guarded(dev, DC.FAMILY[name], points, stage, apply_mask)
    label = f"stage {stage}, family {name}, mask {int(apply_mask)}, P {P}"
    print(f"{label}: worst |error| / e_ref = {DC.worst_ratio(got, want, eref, masked):.3f}")
    if not (guard == SENTINEL).all():
        r, c = (int(v[0]) for v in np.nonzero(guard != SENTINEL))
        raise AssertionError(f"{label}: row {P + r}, column {c} behind the last point was written ({float(guard[r, c])!r})")
    DC.assert_within_bar(got, want, eref, masked, label)


@pytest.mark.parametrize("name", DC.POOLS)
@pytest.mark.parametrize("stage", DC.STAGES)
def test_eval_points_values_whole_pool(dev, stage, name):
    """all 4 099 points of the pool (257 tiles, 65 groups): the figures of DESIGN.md's table"""
    points, eref = DC.pool(name, stage), DC.e_ref(name, stage)
    for apply_mask in (True, False):
        want, masked = DC.yardstick(name, stage, apply_mask), DC.masked_rows(points, apply_mask)
        got = eval_points(dev, DC.FAMILY[name], points, stage, apply_mask).cpu().numpy()
        label = f"stage {stage}, family {name}, mask {int(apply_mask)}, P {DC.POOL}"
        print(f"{label}: worst |error| / e_ref = {DC.worst_ratio(got, want, eref, masked):.3f}")
        DC.assert_within_bar(got, want, eref, masked, label)


# ------------------------------------------------------------------------------------------------ b. position invariance
@pytest.mark.parametrize("stage", DC.STAGES)
def test_position_in_the_batch_is_invisible(dev, stage):
    p = torch.from_numpy(DC.mixed_points(DC.POOL, 501)).to(dev['DEV'])
    perm = torch.from_numpy(np.random.default_rng(502).permutation(DC.POOL)).to(dev['DEV'])
    straight, moved = eval_points(dev, 'generic', p, stage), eval_points(dev, 'generic', p[perm].contiguous(), stage)
    n_masked = int((straight[:, 3] == 100.0).sum())
    assert 0.2 * DC.POOL < n_masked < 0.5 * DC.POOL
    bad = (moved.view(torch.int32) != straight[perm].view(torch.int32)).any(dim=1).nonzero().flatten()
    assert bad.numel() == 0, f"stage {stage}: {bad.numel()} rows differ by position; first: row {int(perm[bad[0]])} moved to {int(bad[0])}"


# ------------------------------------------------------------------------------------------------ c. the weight-stationary route
def _subsample(P):
    """sorted row indices: the first 64, the last 64 and seeded rows between, at most POOL in all"""
    if P <= DC.POOL:
        return np.arange(P)
    between = np.random.default_rng(503).choice(np.arange(64, P - 64), size=DC.POOL - 128, replace=False)
    return np.sort(np.concatenate([np.arange(64), between, np.arange(P - 64, P)]))


@pytest.mark.parametrize("where", ['last_ring', 'first_resident', 'threshold', 'ragged'])
def test_weight_stationary_route_at_its_threshold(dev, where):
    T = dev['T']
    P = {'last_ring': 16 * (T - 1), 'first_resident': 16 * (T - 1) + 1, 'threshold': 16 * T, 'ragged': 16 * T + 37863}[where]
    assert ((P + 15) // 16 >= T) == (where != 'last_ring')
    points = DC.mixed_points(P, 504)
    p = torch.from_numpy(points).to(dev['DEV'])
    whole, parts = eval_points(dev, 'generic', p, 'color'), chunked(dev, 'generic', p, 'color')
    bad = (whole.view(torch.int32) != parts.view(torch.int32)).any(dim=1).nonzero().flatten()
    assert bad.numel() == 0, f"P {P}: {bad.numel()} rows differ between one call and {CHUNK}-point chunks; first: row {int(bad[0])}, last: row {int(bad[-1])}"
    rows = _subsample(P)
    params, grids, bound = DC.scene()
    want = DN.eval_points(params, grids, points[rows], 'color', bound, apply_mask=True)
    masked = DC.masked_rows(points[rows], True)
    assert 0.2 < masked.mean() < 0.5
    got = whole[torch.from_numpy(rows).to(dev['DEV'])].cpu().numpy()
    eref = DC.e_ref('mixed', 'color')
    label = f"stage color, family mixed, mask 1, P {P} ({where})"
    print(f"{label}: worst |error| / e_ref = {DC.worst_ratio(got, want, eref, masked):.3f}")
    DC.assert_within_bar(got, want, eref, masked, label, row_ids=rows)


# ------------------------------------------------------------------------------------------------ d. ray mode through the C ABI
def render_fwd_raw(dev, stage, ro, rd, z, workspace):
    """raw [N * S, 4] of enslam_render_fwd; workspace: None (act_ws NULL), 'full' or 'light'"""
    EF, L, lib = dev['EF'], dev['L'], dev['lib']
    N, S = z.shape
    sc, keep = scene_struct(dev, 'generic', stage)
    depth = torch.empty(N, dtype=torch.float64, device=dev['DEV'])
    var = torch.empty(N, dtype=torch.float64, device=dev['DEV'])
    rgb = torch.empty((N, 3), dtype=torch.float32, device=dev['DEV'])
    raw = torch.full((N * S + GUARD, 4), SENTINEL, dtype=torch.float32, device=dev['DEV'])
    light = int(workspace == 'light')
    act = None if workspace is None else torch.empty(lib.enslam_activation_floats(L.STAGE[stage], N, S, light), dtype=torch.float32,
                                                     device=dev['DEV'])
    P = EF._ptr
    L.check(lib.enslam_render_fwd(L.STAGE[stage], N, S, P(ro), P(rd), P(z), ctypes.byref(sc), P(depth), P(var), P(rgb), P(raw), P(act),
                                  light, EF._stream()), "enslam_render_fwd")
    torch.cuda.synchronize()
    assert bool((raw[N * S:] == SENTINEL).all()), f"stage {stage}, N {N}, S {S}: a row behind the last sample was written"
    return raw[:N * S]


def _rays_on_device(dev, n, S, seed):
    ro, rd, z = DC.rays(n, S, seed)
    return (ro, rd, z), tuple(torch.from_numpy(a).to(dev['DEV']) for a in (ro, rd, z))


@pytest.mark.parametrize("S", [16, 32, 48, 64])
@pytest.mark.parametrize("N", [1, 3, 5, 64, 65])
@pytest.mark.parametrize("stage", XYZ_STAGES)
def test_ray_mode_forms_the_pinned_points(dev, stage, N, S):
    """the production kernels form point, bound mask and cell themselves from rays_o + rays_d * z: the same bits as the pinned
    helper's points through eval_points, with and without an activation workspace"""
    _, (ro, rd, z) = _rays_on_device(dev, N, S, 600 + 7 * N + S)
    pts, inside = dev['EF'].ray_points(ro, rd, z, dev['bound'])
    assert not bool(inside.all()) and bool(inside.any())
    want = eval_points(dev, 'generic', pts, stage)
    assert torch.equal(want[:, 3] == 100.0, ~inside)
    for workspace in (None, 'full', 'light'):
        raw = render_fwd_raw(dev, stage, ro, rd, z, workspace)
        bad = (raw.view(torch.int32) != want.view(torch.int32)).any(dim=1).nonzero().flatten()
        assert bad.numel() == 0, (f"stage {stage}, N {N}, S {S}, workspace {workspace}: {bad.numel()} samples differ from eval_points of "
                                  f"ray_points; first: ray {int(bad[0]) // S}, sample {int(bad[0]) % S}")


def test_ray_mode_on_the_weight_stationary_route(dev):
    N, S = (dev['T'] + 2) // 3 + 1, 48
    assert N * (S // 16) >= dev['T']
    _, (ro, rd, z) = _rays_on_device(dev, N, S, 601)
    pts, inside = dev['EF'].ray_points(ro, rd, z, dev['bound'])
    assert 0.02 < 1.0 - float(inside.float().mean()) < 0.9
    want = chunked(dev, 'generic', pts, 'color')
    raw = render_fwd_raw(dev, 'color', ro, rd, z, None)
    bad = (raw.view(torch.int32) != want.view(torch.int32)).any(dim=1).nonzero().flatten()
    assert bad.numel() == 0, f"{bad.numel()} samples differ; first: ray {int(bad[0]) // S}, sample {int(bad[0]) % S}"


@pytest.mark.parametrize("S", [16, 32, 48, 64])
@pytest.mark.parametrize("N", [1, 3, 5, 64, 65])
def test_ray_mode_coarse_values(dev, N, S):
    (ro_h, rd_h, z_h), (ro, rd, z) = _rays_on_device(dev, N, S, 700 + 7 * N + S)
    points = BN.sample_points(ro_h, rd_h, z_h)
    params, grids, bound = DC.scene()
    want = DN.eval_points(params, grids, points, 'coarse', bound, apply_mask=True)
    masked = DC.masked_rows(points, True)
    assert masked.any() and not masked.all()
    got = render_fwd_raw(dev, 'coarse', ro, rd, z, None).cpu().numpy()
    eref = DC.e_ref('mixed', 'coarse')
    label = f"stage coarse, ray mode, N {N}, S {S}"
    print(f"{label}: worst |error| / e_ref = {DC.worst_ratio(got, want, eref, masked):.3f}")
    DC.assert_within_bar(got, want, eref, masked, label)


# ------------------------------------------------------------------------------------------------ e. attribution
def test_device_sines_account_for_the_sine_share(dev):
    """exact-argument colour case: the yardstick fed the DEVICE's sines of the (exact) float32 arguments leaves the layers'
    accumulation alone, and that meets 4 * e_ref.  The first thing to look at if the values above are tight."""
    points = DC.pool('exact', 'color')
    params, (_, grids, bound) = DC.params_of('exact'), DC.scene()
    sines, worst_sine = {}, 0.0
    for name in DC.XYZ_DECODERS:
        arg = DN.fourier_argument(points, params[name + '.embedder._B'], np.float32)
        s, _ = dev['EF'].fourier_sincos(torch.from_numpy(arg).to(dev['DEV']))
        sines[name] = s.cpu().numpy().astype(np.float64)
        worst_sine = max(worst_sine, float(np.abs(sines[name] - np.sin(arg.astype(np.float64))).max()))
    want = DN.eval_points(params, grids, points, 'color', bound, apply_mask=True, sines=sines)
    got = eval_points(dev, 'exact', points, 'color').cpu().numpy()
    eref, masked = DC.e_ref('exact', 'color'), DC.masked_rows(points, True)
    print(f"device sines: worst |sin error| {worst_sine:.3e}; accumulation alone: worst |error| / e_ref = "
          f"{DC.worst_ratio(got, want, eref, masked):.3f}; with the sine: {DC.worst_ratio(got, DC.yardstick('exact', 'color', True), eref, masked):.3f}")
    assert worst_sine <= 2e-7
    DC.assert_within_bar(got, want, eref, masked, "stage color, family exact, device sines", margin=4.0)
