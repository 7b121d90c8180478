"""Seeded cases for the float64 yardstick of the NICE decoder forward (tests/decoder_numpy.py).

Decoders and grids come from tests/golden/tiny_scene.npz.  Two input families, a pool of POOL points per stage each:
  generic  points uniform in the bound ('generic'), and for the mask a separate set uniform in the bound enlarged by OUTSIDE_SCALE
           about its centre ('mixed': about a third of it lies outside)
  exact    points on the 2^-6 lattice strictly inside the bound, with a copy of the model whose Fourier matrices `_B` are
           clamped to [-128, 128] and rounded to the 2^-8 lattice: every product p * B is a multiple of 2^-14 below 2^10 and
           so is every partial sum of three of them -- 24 bits, the Fourier argument has NO float32 rounding in any
           summation order, and what is left of an error is the sine and the layers' accumulation
The module asserts these conditions itself (`check_conditions`, run on first use).

The bar of a case (pool, stage): e_ref[col] = the worst |float32 CPU oracle - yardstick| of the column over the whole pool; a
device value passes if |device - yardstick| <= MARGIN * e_ref[col].  MARGIN = 8: the device's sine is held to 2e-7 absolute,
about three times a float32 libm sine; the MFMA accumulation order differs from the BLAS one, taken as a factor of 2; 6.6
rounded up to a power of two.  CAP keeps the bar honest: MARGIN * e_ref[col] may be at most CAP[family] of max |yardstick[:, col]|.
Colour columns that a stage leaves at zero and masked occupancies of 100 are compared for equality."""
import functools

import numpy as np
import torch

from oracle import render_oracle as R
from tests import decoder_numpy as DN
from tests.util import GRID_KEYS, load

POOL = 4099
STAGES = DN.STAGES
XYZ_DECODERS = ('middle_decoder', 'fine_decoder', 'color_decoder')
POOLS = ('generic', 'mixed', 'exact')            # 'mixed' is the generic family's set for the mask
FAMILY = {'generic': 'generic', 'mixed': 'generic', 'exact': 'exact'}
MARGIN = 8.0
CAP = {'generic': 5e-5, 'exact': 1e-5}
OUTSIDE_SCALE = 1.145                            # (1 / 1.145)^3 = 0.67 of the enlarged box is the bound
POINT_STEP, B_STEP, B_MAX = 2.0 ** -6, 2.0 ** -8, 128.0


def _frozen(a):
    a = np.ascontiguousarray(a)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def scene():
    """(state arrays 'sd_*' as in the fixture, params {name: float32 array}, grids {name: float32 array}, bound float64 [3, 2])"""
    s = load('tiny_scene')
    params = {k[3:]: _frozen(v) for k, v in s.items() if k.startswith('sd_')}
    grids = {k: _frozen(s[k]) for k in GRID_KEYS}
    return params, grids, _frozen(s['bound'].astype(np.float64))


def exact_B(B):
    return (np.round(np.clip(np.asarray(B, dtype=np.float64), -B_MAX, B_MAX) / B_STEP) * B_STEP).astype(np.float32)


@functools.lru_cache(maxsize=None)
def params_of(family):
    """the fixture's parameters; family 'exact': with every embedder's _B on the 2^-8 lattice"""
    params = dict(scene()[0])
    if family == 'exact':
        for name in XYZ_DECODERS:
            params[name + '.embedder._B'] = _frozen(exact_B(params[name + '.embedder._B']))
    return params


def state_arrays(family):
    """'sd_*' arrays for tests.hip_util.model_from_state"""
    return {'sd_' + k: v for k, v in params_of(family).items()}


def _seed(pool, stage):
    return 9000 + 10 * POOLS.index(pool) + STAGES.index(stage)


def uniform_points(n, rng, scale=1.0):
    bound = scene()[2]
    mid, half = 0.5 * (bound[:, 0] + bound[:, 1]), 0.5 * (bound[:, 1] - bound[:, 0])
    return mid + (rng.random((n, 3)) * 2.0 - 1.0) * half * scale


def mixed_points(n, seed):
    """float64 [n, 3], about a third outside the bound"""
    return uniform_points(n, np.random.default_rng(seed), OUTSIDE_SCALE)


def lattice_points(n, rng):
    bound = scene()[2]
    lo = np.floor(bound[:, 0] / POINT_STEP).astype(np.int64) + 1
    hi = np.ceil(bound[:, 1] / POINT_STEP).astype(np.int64) - 1
    return rng.integers(lo, hi + 1, size=(n, 3)).astype(np.float64) * POINT_STEP


@functools.lru_cache(maxsize=None)
def pool(name, stage):
    """float64 [POOL, 3]"""
    rng = np.random.default_rng(_seed(name, stage))
    if name == 'generic':
        return _frozen(uniform_points(POOL, rng))
    if name == 'mixed':
        return _frozen(uniform_points(POOL, rng, OUTSIDE_SCALE))
    return _frozen(lattice_points(POOL, rng))


@functools.lru_cache(maxsize=None)
def check_conditions():
    bound = scene()[2]
    for stage in STAGES:
        assert DN.inside_bound(pool('generic', stage), bound).all()
        p = pool('exact', stage)
        assert DN.inside_bound(p, bound).all(), "lattice points must lie strictly inside the bound"
        assert np.array_equal(p.astype(np.float32).astype(np.float64), p)
        for name in XYZ_DECODERS:
            B = params_of('exact')[name + '.embedder._B']
            a32, a64 = DN.fourier_argument(p, B, np.float32), DN.fourier_argument(p, B, np.float64)
            assert a32.dtype == np.float32 and np.array_equal(a32.astype(np.float64), a64), (stage, name)
        share = 1.0 - DN.inside_bound(pool('mixed', stage), bound).mean()
        assert 0.2 <= share <= 0.5, (stage, share)
    return True


@functools.lru_cache(maxsize=None)
def yardstick(name, stage, apply_mask):
    """float64 [POOL, 4]"""
    check_conditions()
    params, (_, grids, bound) = params_of(FAMILY[name]), scene()
    return _frozen(DN.eval_points(params, grids, pool(name, stage), stage, bound, apply_mask=apply_mask))


def oracle_inputs(family):
    params = {k: torch.from_numpy(v.copy()) for k, v in params_of(family).items()}
    grids = {k: torch.from_numpy(v.copy()) for k, v in scene()[1].items()}
    return params, grids, torch.from_numpy(scene()[2].copy())


@functools.lru_cache(maxsize=None)
def oracle(name, stage, apply_mask):
    """the float32 CPU oracle on the same parameters, grids and points: float64 copy of its float32 [POOL, 4]"""
    params, grids, bound = oracle_inputs(FAMILY[name])
    p = torch.from_numpy(pool(name, stage).copy())
    with torch.no_grad():
        raw = (R.eval_points if apply_mask else R.decode_stage)(params, grids, p, stage, bound)
    return _frozen(raw.double().numpy())


@functools.lru_cache(maxsize=None)
def e_ref(name, stage):
    """float64 [4]: worst |oracle - yardstick| per column over the whole pool (unmasked, so every point counts)"""
    return _frozen(np.abs(oracle(name, stage, False) - yardstick(name, stage, False)).max(axis=0))


def masked_rows(points, apply_mask):
    bound = scene()[2]
    return ~DN.inside_bound(points, bound) if apply_mask else np.zeros(len(points), dtype=bool)


def beyond_bar(got, want, eref, masked, margin=MARGIN):
    """bool [P, 4]: entries of `got` that miss the bar against the yardstick rows `want` (masked: bool [P], rows whose
    occupancy is the mask's 100)"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    bad = ~(np.abs(got - want) <= margin * eref[None, :])            # (a NaN misses)
    for col in range(4):
        if eref[col] == 0.0:
            bad[:, col] = got[:, col] != want[:, col]
    bad[masked, 3] = got[masked, 3] != 100.0
    return bad


def worst_ratio(got, want, eref, masked):
    """worst |got - want| / e_ref over the entries that have a bar (not the equality ones)"""
    err = np.abs(np.asarray(got, dtype=np.float64) - want)
    err[masked, 3] = 0.0
    cols = eref > 0
    return float((err[:, cols] / eref[cols]).max()) if cols.any() and len(err) else 0.0


def assert_within_bar(got, want, eref, masked, label, margin=MARGIN, row_ids=None):
    bad = beyond_bar(got, want, eref, masked, margin)
    if bad.any():
        r, c = (int(v[0]) for v in np.nonzero(bad))
        rid = r if row_ids is None else int(row_ids[r])
        raise AssertionError(f"{label}: {int(bad.any(axis=1).sum())} of {len(bad)} rows beyond {margin:g} * e_ref; first at row {rid}, "
                             f"column {c}: device {float(np.asarray(got)[r, c])!r}, float64 {float(want[r, c])!r}, "
                             f"e_ref {float(eref[c]):.3e}" + (" (masked: 100 expected)" if c == 3 and masked[r] else ""))


# ------------------------------------------------------------------------------------------------ rays
def rays(n, S, seed):
    """(rays_o float32 [n, 3], rays_d float32 [n, 3], z_vals float64 [n, S] ascending): origins near the centre of the bound,
    directions over the sphere, distances up to beyond the bound's far side, so that every batch of a few rays has samples
    inside and outside"""
    rng = np.random.default_rng(seed)
    bound = scene()[2]
    mid, half = 0.5 * (bound[:, 0] + bound[:, 1]), 0.5 * (bound[:, 1] - bound[:, 0])
    ro = (mid + (rng.random((n, 3)) - 0.5) * 0.5 * half).astype(np.float32)
    rd = rng.standard_normal((n, 3))
    rd = (rd / np.linalg.norm(rd, axis=1, keepdims=True)).astype(np.float32)
    z = np.sort(0.01 + rng.random((n, S)) * 1.6 * float(half.min()), axis=1)
    z[0, -1] = 2.5 * float(np.linalg.norm(half))                    # the first ray's last sample is outside for certain
    return ro, rd, np.ascontiguousarray(z)
