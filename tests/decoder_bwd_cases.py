"""Seeded cases, fragility rule and bar for the float64 yardstick of the NICE decoder backward (tests/decoder_bwd_numpy.py).

Scene and parameters: decoder_cases.scene() (tests/golden/tiny_scene.npz, generic family); rays: decoder_cases.rays(n, S, seed),
which leave the bound on purpose.  The cotangent d_raw of a case is seeded float32 standard normal in all four columns, then
set to ZERO on every fragile sample.

Fragile samples.  A ReLU whose pre-activation lies within rounding of zero takes either branch depending on the arithmetic;
the forward cannot see it and the gradient of that sample jumps.  A sample is fragile if, for any decoder of the stage, any
hidden pre-activation of the float64 forward has |pre| < MARGIN * e_pre[decoder], where e_pre[decoder] is the worst
|float32 CPU oracle pre-activation - float64| over the stage's reference batch (N = 65, S = 64).  The backward is linear in
d_raw and samples are independent, so with a zero cotangent there the yardstick does not depend on the branch those samples
take, and the retained samples take the same branch in float64, in the float32 oracle and on any device whose pre-activations
are within MARGIN * e_pre.  Asserted: fragile samples are at most FRAGILE_CAP of any case.

Listed cases zero whole 16-sample tiles of d_raw as well -- every third tile, the first tile of ray 0 and the last tile of the
last ray -- and carry the work list (ascending ids ray * S / 16 + tile of the tiles that are not all zero).

The bar.  MARGIN = decoder_cases.MARGIN = 8 (the device's sine is held to three times a float32 libm sine, the MFMA / atomic
summation order differs from the BLAS one, taken as a factor of 2; 6.6 rounded up to a power of two -- the derivation of the
forward's bar; the backward multiplies by the cosine, which the device holds to 1e-6: see COS_NOTE).  For each stage and tensor
family, e_rel = the worst |float32 oracle autograd - yardstick| / A over the elements with A > 0 of the stage's reference batch
(no zeroed tiles); for the decoder parameters, whose gradients are sums over the whole batch, the larger of that and the
oracle's own error on the case's inputs (`case_e_rel` says why).  A device element passes if |device - yardstick| <= MARGIN * e_rel * A[element]; where A == 0 it must
be exactly 0.  Asserted: MARGIN * e_rel <= CAP_REL for every family.  Families: each grid; weights (with the Fourier matrix)
and biases of each decoder; rays_o; rays_d.

Deferred-scatter route (ENSLAM_DEFER_SCATTER): its documented flush (csrc/grid_scatter.hip: fixed-point sums scaled by the ray
group's largest |dC|, exact above 2^-40 of that value, flushed to zero below it) adds ONE absolute term to the bar of grid
gradients: DEFER_FLUSH * max |dC| of the launch.  Nothing else changes for that route."""
import collections
import functools

import numpy as np
import torch

from oracle import render_oracle as R
from tests import blocks_numpy as BN
from tests import decoder_bwd_numpy as DB
from tests import decoder_cases as DC
from tests import decoder_numpy as DN

STAGES = DN.STAGES
MARGIN = DC.MARGIN
CAP_REL = 1e-4                      # MARGIN * e_rel of every family stays below it
FRAGILE_CAP = 0.05
DEFER_FLUSH = 2.0 ** -40
REF_N, REF_S = 65, 64
TILE = 16
SHAPES_N, SHAPES_S = (1, 3, 5, 64, 65), (16, 32, 48, 64)
LISTED_SHAPES = tuple((n, s) for n in (3, 65) for s in (16, 48))
COS_NOTE = "ray gradients go through the device's cosine (1e-6 absolute); no family has needed a margin of its own"

Case = collections.namedtuple('Case', 'stage N S ro rd z d_raw fragile work g A dC_max erel')


def _frozen(a):
    return DC._frozen(a)


def _seed(stage, N, S):
    return 7100 + 1000 * STAGES.index(stage) + 7 * N + S


@functools.lru_cache(maxsize=None)
def rays(stage, N, S):
    return tuple(_frozen(a) for a in DC.rays(N, S, _seed(stage, N, S)))


# ------------------------------------------------------------------------------------------------ fragility
def _oracle_preacts_xyz(params, name, p, c):
    emb = R.fourier_embed(p.float(), params[f'{name}.embedder._B'])
    h, pres = emb, []
    for i in range(DN.N_BLOCKS):
        pres.append(R._lin(params, f'{name}.pts_linears.{i}', h))
        h = torch.relu(pres[i]) + R._lin(params, f'{name}.fc_c.{i}', c)
        if i == DN.SKIP:
            h = torch.cat([emb, h], -1)
    assert torch.equal(R._lin(params, f'{name}.output_linear', h), R.decode_xyz(params, name, p, c))
    return torch.stack(pres, dim=1)


def _oracle_preacts_feat(params, name, c):
    h, pres = c, []
    for i in range(DN.N_BLOCKS):
        pres.append(R._lin(params, f'{name}.pts_linears.{i}', h))
        h = torch.relu(pres[i])
        if i == DN.SKIP:
            h = torch.cat([c, h], -1)
    assert torch.equal(R._lin(params, f'{name}.output_linear', h), R.decode_feat(params, name, c))
    return torch.stack(pres, dim=1)


def oracle_preactivations(stage, points):
    """{decoder: float64 copy of the float32 oracle's hidden pre-activations [P, 5, 32]}: the oracle's own operations in its
    own order (checked against its decoder outputs bit for bit)"""
    params, grids, bound = DC.oracle_inputs('generic')
    p = torch.from_numpy(np.array(points, dtype=np.float64))
    out = {}
    with torch.no_grad():
        if stage == 'coarse':
            out['coarse_decoder'] = _oracle_preacts_feat(params, 'coarse_decoder', R.trilinear(grids['grid_coarse'], p, bound * 2))
        else:
            c_mid = R.trilinear(grids['grid_middle'], p, bound)
            out['middle_decoder'] = _oracle_preacts_xyz(params, 'middle_decoder', p, c_mid)
            if stage in ('fine', 'color'):
                c_fine = torch.cat([R.trilinear(grids['grid_fine'], p, bound), c_mid], -1)
                out['fine_decoder'] = _oracle_preacts_xyz(params, 'fine_decoder', p, c_fine)
            if stage == 'color':
                out['color_decoder'] = _oracle_preacts_xyz(params, 'color_decoder', p, R.trilinear(grids['grid_color'], p, bound))
    return {k: v.double().numpy() for k, v in out.items()}


@functools.lru_cache(maxsize=None)
def e_pre(stage):
    """{decoder: worst |float32 oracle pre-activation - float64| over the stage's reference batch}"""
    params, grids, bound = DC.scene()
    points = BN.sample_points(*rays(stage, REF_N, REF_S))
    want, got = DB.preactivations(params, grids, points, stage, bound), oracle_preactivations(stage, points)
    return {name: float(np.abs(got[name] - want[name]).max()) for name in DB.STAGE_DECODERS[stage]}


def fragile_samples(stage, points):
    """bool [P]: samples with a hidden pre-activation within MARGIN * e_pre of zero"""
    params, grids, bound = DC.scene()
    pres, epre = DB.preactivations(params, grids, points, stage, bound), e_pre(stage)
    out = np.zeros(len(points), dtype=bool)
    for name, p in pres.items():
        out |= (np.abs(p) < MARGIN * epre[name]).any(axis=(1, 2))
    return out


def branch_differences(stage, points):
    """number of retained (non-fragile) pre-activations whose float32 oracle sign differs from float64's"""
    params, grids, bound = DC.scene()
    want, got = DB.preactivations(params, grids, points, stage, bound), oracle_preactivations(stage, points)
    keep = ~fragile_samples(stage, points)
    return sum(int(((want[n][keep] > 0) != (got[n][keep] > 0)).sum()) for n in want)


# ------------------------------------------------------------------------------------------------ cases
def zeroed_tiles(N, S):
    """bool [N * S / 16]: the tiles a listed case zeroes"""
    n = N * (S // TILE)
    z = np.zeros(n, dtype=bool)
    z[::3] = True
    z[0] = True
    z[n - 1] = True
    return z


@functools.lru_cache(maxsize=None)
def case(stage, N, S, listed=False):
    ro, rd, z = rays(stage, N, S)
    params, grids, bound = DC.scene()
    points = BN.sample_points(ro, rd, z)
    fragile = fragile_samples(stage, points)
    d_raw = np.random.default_rng(_seed(stage, N, S) + 50000).standard_normal((N * S, 4)).astype(np.float32)
    d_raw[fragile] = 0.0
    work = None
    if listed:
        d_raw[np.repeat(zeroed_tiles(N, S), TILE)] = 0.0
        work = np.nonzero((d_raw.reshape(-1, TILE * 4) != 0).any(axis=1))[0].astype(np.int32)
    g, A = DB.backward(params, grids, ro, rd, z, d_raw, stage, bound)
    dC_max = A.pop('dC_max')
    c = Case(stage, N, S, ro, rd, z, _frozen(d_raw), _frozen(fragile), None if work is None else _frozen(work),
             {k: _frozen(v) for k, v in g.items()}, {k: _frozen(v) for k, v in A.items()}, dC_max, None)
    return c._replace(erel=case_e_rel(c))


def check_case(c):
    """the conditions every case must meet (asserted by the CPU test for the fixed shapes, by the GPU test for its own)"""
    bound = DC.scene()[2]
    points = BN.sample_points(c.ro, c.rd, c.z)
    keep = DN.inside_bound(points, bound)
    assert keep.any() and not keep.all(), "a case needs masked and unmasked samples"
    assert c.fragile.mean() <= FRAGILE_CAP, (c.stage, c.N, c.S, float(c.fragile.mean()))
    if c.N >= 3:
        name = 'grid_coarse' if c.stage == 'coarse' else 'grid_middle'
        co = DB.coordinates(points, bound * 2 if c.stage == 'coarse' else bound, DC.scene()[1][name].shape[2:])
        assert any((~DB.inner(x, size)).any() for x, size, _ in co), "no sample clipped on an axis"
    for fam, v in c.erel.items():
        assert 0 < MARGIN * v <= CAP_REL, (c.stage, c.N, c.S, fam, v)
    if c.work is not None:
        tiles = (c.d_raw.reshape(-1, TILE * 4) != 0).any(axis=1)
        assert tiles.any() and not tiles.all() and len(c.work) == int(tiles.sum()) and (np.diff(c.work) > 0).all()


# ------------------------------------------------------------------------------------------------ the bar
def family_of(name):
    if name.startswith('grid_') or name in ('rays_o', 'rays_d'):
        return name
    dec = name.split('.')[0]
    return dec + ('.biases' if name.endswith('.bias') else '.weights')


def scale_of(name, A):
    """A broadcast to the gradient's shape"""
    if name.startswith('grid_'):
        return A[None, :]
    if name in ('rays_o', 'rays_d'):
        return A[:, None]
    return A


def oracle_gradients(stage, ro, rd, z, d_raw):
    """float64 copies of the float32 CPU oracle's autograd gradients of (eval_points * d_raw).sum()"""
    params, grids, bound = DC.oracle_inputs('generic')
    leaves = {k: v.requires_grad_(True) for k, v in params.items() if k.split('.')[0] in DB.STAGE_DECODERS[stage]}
    leaves.update({k: grids[k].requires_grad_(True) for k in DB.STAGE_GRIDS[stage]})
    o, d = torch.from_numpy(ro.copy()).requires_grad_(True), torch.from_numpy(rd.copy()).requires_grad_(True)
    zz = torch.from_numpy(z.copy())
    pts = (o[:, None, :] + d[:, None, :] * zz[:, :, None]).reshape(-1, 3)
    raw = R.eval_points(params, grids, pts, stage, bound)
    (raw * torch.from_numpy(d_raw.copy())).sum().backward()
    out = {'rays_o': o.grad, 'rays_d': d.grad}
    out.update({k: v.grad for k, v in leaves.items()})
    return {k: (v.reshape(32, -1) if k.startswith('grid_') else v).double().numpy() for k, v in out.items()}


def oracle_error(c):
    """{family: worst |float32 oracle autograd - yardstick| / A over the elements with A > 0} on the case's own inputs"""
    got = oracle_gradients(c.stage, c.ro, c.rd, c.z, c.d_raw)
    out = {}
    for name, want in c.g.items():
        A = np.broadcast_to(scale_of(name, c.A[name]), want.shape)
        assert got[name].shape == want.shape, name
        if (A > 0).any():
            fam = family_of(name)
            out[fam] = max(out.get(fam, 0.0), float((np.abs(got[name] - want)[A > 0] / A[A > 0]).max()))
    return out


@functools.lru_cache(maxsize=None)
def e_rel(stage):
    """{family: the oracle's error on the stage's reference batch (N = 65, S = 64, no zeroed tiles)}"""
    params, grids, bound = DC.scene()
    ro, rd, z = rays(stage, REF_N, REF_S)
    points = BN.sample_points(ro, rd, z)
    d_raw = np.random.default_rng(_seed(stage, REF_N, REF_S) + 50000).standard_normal((REF_N * REF_S, 4)).astype(np.float32)
    d_raw[fragile_samples(stage, points)] = 0.0
    g, A = DB.backward(params, grids, ro, rd, z, d_raw, stage, bound)
    A.pop('dC_max')
    return oracle_error(Case(stage, REF_N, REF_S, ro, rd, z, d_raw, None, None, g, A, None, None))


def batch_sum(family):
    """decoder parameters: their gradients are sums over EVERY sample of the batch"""
    return family.endswith('.weights') or family.endswith('.biases')


def case_e_rel(c):
    """{family: e_rel of the case}.  Grids and rays: the reference batch's (their sums are local -- a voxel's taps, a ray's
    samples -- and the figure carries over to every shape: the oracle itself stays below 3 of it on all of them).  Decoder
    parameters: the larger of the reference batch's and the ORACLE's OWN ERROR ON THE CASE'S INPUTS.  A float32 sum of n terms
    errs by about 1 / sqrt(n) of the sum of their magnitudes, so the figure of the 4 160-sample reference batch is up to
    sqrt(4160 / 16) = 16 times too tight for a one-tile batch: measured, the oracle itself sits at 37 times it there, the
    device at the same place.  The cap CAP_REL holds for every case's figures (check_case)."""
    ref = e_rel(c.stage)
    own = oracle_error(c)
    return {fam: (max(v, own.get(fam, 0.0)) if batch_sum(fam) else v) for fam, v in ref.items()}


def beyond_bar(name, got, want, A, erel, margin=MARGIN, extra_abs=0.0):
    """bool array: elements of `got` that miss the bar; where A == 0 the element must be exactly 0"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    A = np.broadcast_to(scale_of(name, A), want.shape)
    bad = ~(np.abs(got - want) <= margin * erel * A + extra_abs)          # (a NaN misses)
    return np.where(A > 0, bad, got != 0.0)


def worst_ratio(name, got, want, A, erel):
    """worst |got - want| / (e_rel * A) over the elements with A > 0"""
    A = np.broadcast_to(scale_of(name, A), np.shape(want))
    if not (A > 0).any() or erel == 0.0:
        return 0.0
    return float((np.abs(np.asarray(got, dtype=np.float64) - want)[A > 0] / (erel * A[A > 0])).max())


def assert_within_bar(name, got, want, A, erel, label, margin=MARGIN, extra_abs=0.0):
    bad = beyond_bar(name, got, want, A, erel, margin, extra_abs)
    if bad.any():
        at = tuple(int(v[0]) for v in np.nonzero(bad))
        Ab = np.broadcast_to(scale_of(name, A), np.shape(want))
        raise AssertionError(f"{label}, {name}: {int(bad.sum())} of {bad.size} elements beyond {margin:g} * e_rel * A; first at {at}: "
                             f"got {float(np.asarray(got)[at])!r}, float64 {float(want[at])!r}, A {float(Ab[at]):.3e}, "
                             f"e_rel {erel:.3e}" + (" (A == 0: exactly 0 expected)" if Ab[at] == 0 else ""))
