"""Seeded inputs for the ray-sampler tests (tests/test_sampler_cpu.py, tests/test_hip_sampler.py) and the conditions they rely on,
asserted on the yardstick alone (tests/sampler_numpy.py) by check_case(), so that no kernel test can pass by missing one.

One bound with three different extents, none centred on 0, every face a float32 value (an origin can sit exactly on it).
N = 37 rays (N % 4 == 1: the four-rays-per-workgroup entry ends on a single ray).

Ray pool 'edges' (ROLE names the rays; the rest are generic: origin strictly inside, no zero component):
  axis-parallel   one component +0.0, one -0.0, two components (+0.0, -0.0) and (-0.0, +0.0): infinite face distances, no NaN
  on a face       origin exactly on the low x face and on the high y face, the component along that axis pointing in and out
  outside         origin beyond a face, pointing towards the box and away from it (far_bb < 0: with depth the clamp gives far == 0,
                  without depth z descends -- the reference does not sort there, so the kernel must not either)
Ray pool 'inside': the same with the on-face and outside rays replaced by generic ones.  lindisp divides by near and by far, so
lindisp cases take this pool and depths >= 0.05 (the reference gives inf / NaN otherwise; outside the contract).
Ray pool 'nan': 'edges' with two rays put on a face with a zero component along that axis (0/0): the out-of-contract group.

Depths 'mixed': uniform in [0.3, 3.3], about a fifth exactly 0, one negative, one 1e-37 (near = fl32(1e-37f * 0.01f) is a
float32 subnormal: the row that tells a flushing build from a correct one), two equal pairs, the largest on the last ray.
'positive': uniform in [0.05, 3.3], an equal pair, the largest last (lindisp).  'shallow': all 0.4 (the cap fl32(max d * 1.2f)
binds on most rays).  'zero': all 0 (max d == 0).  Batches of one ray: 'one' (ray 12 with its depth) and 'onezero'.

Counts: COUNTS, each with depth and without (n_surf is still passed as given without depth wherever n_lin + n_surf <= 64 -- the
entry then ignores it), lindisp 0 and 1, with and without t_rand (uniform float32 draws; row 0 exactly 0, row 1 1 - 2^-24)."""
import types

import numpy as np
import torch

from tests import sampler_numpy as Y

f32 = np.float32
N = 37
BOUND = np.array([[-1.25, 2.875], [0.5, 3.125], [-2.25, -0.375]], np.float64)
COUNTS = ((1, 0), (1, 1), (1, 63), (2, 1), (5, 3), (16, 0), (32, 16), (33, 31), (48, 16), (63, 1), (64, 0))
BATCH_N = (1, 2, 3, 4, 5, 8, 37)
ROLE = {'x+0': 0, 'x-0': 1, 'y+0z-0': 2, 'x-0y+0': 3, 'lowx_in': 4, 'lowx_out': 5, 'highy_in': 6, 'highy_out': 7,
        'outside_towards': 8, 'outside_away': 9, 'outside_away_z': 10}
NAN_RAYS = (11, 30)                      # pool 'nan': on the low x face with d_x = +0.0; on the high z face with d_z = -0.0
ZERO_DEPTH = (2, 9, 13, 17, 22, 28, 33)  # about a fifth of 37, an axis-parallel and an outside ray among them
NEGATIVE, SUBNORMAL, EQUAL = 15, 19, ((20, 21), (23, 31))
ONE_RAY = 12


def _rng(*key):
    return np.random.default_rng([20240917] + [int(k) for k in key])


def linspaces(n_lin, n_surf):
    """t_lin float32 [n_lin], t_surf float64 [n_surf] or None: the ABI defines them as torch.linspace's values"""
    t_lin = torch.linspace(0., 1., steps=n_lin).numpy()
    t_surf = torch.linspace(0., 1., steps=n_surf).double().numpy() if n_surf > 0 else None
    return t_lin, t_surf


def rays(pool):
    """(rays_o, rays_d) float32 [N, 3]"""
    r = _rng(1)
    lo, hi = BOUND[:, 0], BOUND[:, 1]
    ro = (lo + (hi - lo) * r.uniform(0.1, 0.9, (N, 3))).astype(f32)
    rd = r.standard_normal((N, 3))
    rd = np.where(np.abs(rd) < 0.05, 0.05, rd)
    rd = (rd / np.linalg.norm(rd, axis=1, keepdims=True)).astype(f32)
    R = ROLE
    rd[R['x+0'], 0] = f32(0.0)
    rd[R['x-0'], 0] = f32(-0.0)
    rd[R['y+0z-0'], 1:] = (f32(0.0), f32(-0.0))
    ro[R['y+0z-0'], 0], rd[R['y+0z-0'], 0] = f32(lo[0] + 0.0625), f32(1.0)     # the long way along x: past any cap here
    rd[R['x-0y+0'], :2] = (f32(-0.0), f32(0.0))
    if pool in ('edges', 'nan'):
        ro[R['lowx_in'], 0] = ro[R['lowx_out'], 0] = f32(lo[0])
        rd[R['lowx_in'], 0], rd[R['lowx_out'], 0] = f32(0.6), f32(-0.6)
        ro[R['highy_in'], 1] = ro[R['highy_out'], 1] = f32(hi[1])
        rd[R['highy_in'], 1], rd[R['highy_out'], 1] = f32(-0.5), f32(0.5)
        ro[R['outside_towards'], 0], rd[R['outside_towards'], 0] = f32(hi[0] + 0.75), f32(-0.8)
        ro[R['outside_away'], 0], rd[R['outside_away'], 0] = f32(hi[0] + 0.75), f32(0.8)
        ro[R['outside_away_z'], 2], rd[R['outside_away_z'], 2] = f32(lo[2] - 0.5), f32(-0.7)
    if pool == 'nan':
        ro[NAN_RAYS[0], 0], rd[NAN_RAYS[0], 0] = f32(lo[0]), f32(0.0)
        ro[NAN_RAYS[1], 2], rd[NAN_RAYS[1], 2] = f32(hi[2]), f32(-0.0)
    return ro, rd


def depths(kind):
    """float32 [N], or None for 'none'"""
    r = _rng(2)
    if kind == 'none':
        return None
    if kind == 'shallow':
        return np.full(N, 0.4, f32)
    if kind == 'zero':
        return np.zeros(N, f32)
    gd = r.uniform(0.3 if kind == 'mixed' else 0.05, 3.3, N).astype(f32)
    for a, b in EQUAL:
        gd[b] = gd[a]
    if kind == 'mixed':
        gd[list(ZERO_DEPTH)] = f32(0.0)
        gd[NEGATIVE] = f32(-0.7)
        gd[SUBNORMAL] = f32(1e-37)
    else:
        assert kind == 'positive'
    gd[N - 1] = f32(1.01) * gd.max()
    return gd


def make(n_lin, n_surf, depth='mixed', lindisp=False, perturb=False, pool=None, n=N, order=None):
    """One case: the first n rays of the pool (order: a permutation applied to rays, depths and t_rand rows instead).
    Without depth n_surf is what the caller still passes; the yardstick sees none."""
    pool = pool or ('inside' if lindisp else 'edges')
    ro, rd = rays(pool)
    gd = depths(depth if depth not in ('one', 'onezero') else 'mixed')
    t_rand = None
    if perturb:
        t_rand = _rng(3, n_lin).random((N, n_lin), dtype=f32)
        t_rand[0] = f32(0.0)
        t_rand[1] = f32(1.0) - f32(2.0 ** -24)
    pick = np.arange(n) if order is None else np.asarray(order)
    if depth in ('one', 'onezero'):
        pick = np.array([ONE_RAY])
        if depth == 'onezero':
            gd = np.zeros(N, f32)
    ro, rd = np.ascontiguousarray(ro[pick]), np.ascontiguousarray(rd[pick])
    gd = None if gd is None else np.ascontiguousarray(gd[pick])
    t_rand = None if t_rand is None else np.ascontiguousarray(t_rand[pick])
    t_lin, t_surf = linspaces(n_lin, n_surf)
    c = types.SimpleNamespace(n_lin=n_lin, n_surf=n_surf, depth=depth, lindisp=bool(lindisp), perturb=bool(perturb), pool=pool,
                              N=len(pick), ro=ro, rd=rd, gd=gd, t_rand=t_rand, t_lin=t_lin, t_surf=t_surf, bound=BOUND,
                              pick=pick, whole=order is None and len(pick) == N)
    c.S = n_lin + (n_surf if gd is not None else 0)
    c.dmax = None if gd is None else Y.depth_max(gd)
    c.z, c.ok = Y.sample(ro, rd, gd, BOUND, t_lin, t_surf if gd is not None else None, lindisp, t_rand)
    c.out = tuple(int(i) for i in np.nonzero(np.isin(pick, NAN_RAYS))[0]) if pool == 'nan' else ()
    c.name = f"{n_lin}+{n_surf}-{depth}-{pool}" + ('-lindisp' if lindisp else '') + ('-perturb' if perturb else '') + \
        (f'-N{len(pick)}' if len(pick) != N else '') + ('-permuted' if order is not None else '')
    return c


def grid_cases():
    """every count with depth and without, lindisp 0 and 1, with and without t_rand"""
    for n_lin, n_surf in COUNTS:
        for guided in (True, False):
            for lindisp in (False, True):
                for perturb in (False, True):
                    depth = ('positive' if lindisp else 'mixed') if guided else 'none'
                    yield make(n_lin, n_surf, depth, lindisp, perturb)


def batch_cases():
    """whole batches of their own, and the batch sizes around the four-rays-per-workgroup form, on (32, 16) (and one small count)"""
    for n_lin, n_surf in ((32, 16), (5, 3)):
        for depth in ('zero', 'one', 'onezero', 'shallow'):
            yield make(n_lin, n_surf, depth)
    for n in BATCH_N:
        if n != N:
            yield make(32, 16, 'mixed', n=n)


def in_contract_cases():
    yield from grid_cases()
    yield from batch_cases()


def nan_cases():
    """the out-of-contract group: rays NAN_RAYS divide 0 by 0"""
    yield make(32, 16, 'mixed', pool='nan')
    yield make(5, 3, 'none', pool='nan', perturb=True)


def permutation():
    return _rng(4).permutation(N)


def is_subnormal32(x):
    x = np.asarray(x, f32)
    return (x != 0) & (np.abs(x) < np.finfo(f32).tiny)


def check_case(c):
    """every condition the tests lean on, from the yardstick alone"""
    assert c.ro.dtype == c.rd.dtype == f32 and c.ro.shape == c.rd.shape == (c.N, 3)
    assert c.z.dtype == np.float64 and c.z.shape == (c.N, c.S) and c.S <= 64 and c.n_lin >= 1
    assert c.t_lin.dtype == f32 and c.t_lin.shape == (c.n_lin,) and c.t_lin[0] == 0 and (c.n_lin == 1 or c.t_lin[-1] == 1)
    # the cap on what a test may leave out: all rays in contract but the designated ones
    assert sorted(np.nonzero(~c.ok)[0].tolist()) == sorted(c.out), (c.name, np.nonzero(~c.ok)[0])
    assert np.isfinite(c.z[c.ok]).all()
    assert not (np.signbit(c.z) & (c.z == 0)).any()                  # no -0.0: a sort may order it either side of +0.0
    assert len(set((BOUND[:, 1] - BOUND[:, 0]).tolist())) == 3
    assert (np.abs(BOUND.mean(1)) > 0.1).all() and (BOUND.astype(f32) == BOUND).all()
    o, d = c.ro.astype(np.float64), c.rd.astype(np.float64)
    with np.errstate(all='ignore'):
        t = (BOUND[None] - o[:, :, None]) / d[:, :, None]
        far_bb = np.min(np.max(t, 2), 1) + 0.01
    inside = ((o > BOUND[:, 0]) & (o < BOUND[:, 1])).all(1)
    if c.perturb:
        assert c.t_rand.dtype == f32 and c.t_rand.shape == (c.N, c.n_lin)
        assert (c.t_rand >= 0).all() and (c.t_rand < 1).all()
    if c.gd is not None:
        assert c.gd.dtype == f32 and np.isfinite(c.gd).all()
        assert Y.depth_max(c.gd).tobytes() == c.dmax.tobytes()
    if c.lindisp:
        assert inside.all() and (c.gd is None or (c.gd >= f32(0.05)).all())
    if not c.whole:
        return
    # ---- whole pools: the named rays are what they claim
    R = ROLE
    if c.perturb:
        assert (c.t_rand[0] == 0).all() and (c.t_rand[1] == f32(1.0) - f32(2.0 ** -24)).all() and (c.t_rand[1] < 1).all()
        assert ((c.t_rand[2:] > 0) & (c.t_rand[2:] < 1)).any()
    zero = (c.rd == 0)
    neg0 = zero & np.signbit(c.rd)
    assert zero[R['x+0']].tolist() == [True, False, False] and not neg0[R['x+0'], 0]
    assert zero[R['x-0']].tolist() == [True, False, False] and neg0[R['x-0'], 0]
    assert zero[R['y+0z-0']].tolist() == [False, True, True] and neg0[R['y+0z-0']].tolist() == [False, False, True]
    assert zero[R['x-0y+0']].tolist() == [True, True, False] and neg0[R['x-0y+0']].tolist() == [True, False, False]
    for k in ('x+0', 'x-0', 'y+0z-0', 'x-0y+0'):
        assert inside[R[k]] and np.isinf(t[R[k]]).any() and not np.isnan(t[R[k]]).any() and np.isfinite(far_bb[R[k]])
    generic = np.ones(c.N, bool)
    generic[list(R.values())] = False
    if c.pool == 'nan':
        generic[list(NAN_RAYS)] = False
        assert np.isnan(t[list(NAN_RAYS)]).any(axis=(1, 2)).all() and not np.isnan(np.delete(t, NAN_RAYS, 0)).any()
        assert zero[NAN_RAYS[0], 0] and not neg0[NAN_RAYS[0], 0] and neg0[NAN_RAYS[1], 2]
    assert inside[generic].all() and not zero[generic].any() and generic.sum() >= 20
    if c.pool == 'inside':
        assert inside.all()
    else:
        lo, hi = BOUND[:, 0], BOUND[:, 1]
        assert o[R['lowx_in'], 0] == lo[0] == o[R['lowx_out'], 0] and d[R['lowx_in'], 0] > 0 > d[R['lowx_out'], 0]
        assert o[R['highy_in'], 1] == hi[1] == o[R['highy_out'], 1] and d[R['highy_in'], 1] < 0 < d[R['highy_out'], 1]
        assert o[R['outside_towards'], 0] > hi[0] and d[R['outside_towards'], 0] < 0 and far_bb[R['outside_towards']] > 0
        assert o[R['outside_away'], 0] > hi[0] and d[R['outside_away'], 0] > 0 and far_bb[R['outside_away']] < 0
        assert o[R['outside_away_z'], 2] < lo[2] and d[R['outside_away_z'], 2] < 0 and far_bb[R['outside_away_z']] < 0
        if c.gd is None and not c.lindisp and c.n_lin >= 2:
            # far = far_bb < 0: the row descends and stays unsorted
            row = c.z[R['outside_away']]
            assert c.perturb or (np.diff(row) < 0).all()
            assert not (np.diff(row) >= 0).all()
    if c.gd is None:
        return
    # ---- depths
    if c.depth == 'mixed':
        assert 0.15 < (c.gd == 0).mean() < 0.25 and (c.gd[list(ZERO_DEPTH)] == 0).all()
        assert c.gd[NEGATIVE] < 0 and (c.gd < 0).sum() == 1
        near = c.gd[SUBNORMAL] * f32(0.01)
        assert c.gd[SUBNORMAL] == f32(1e-37) and is_subnormal32(near) and c.ok[SUBNORMAL]
        assert is_subnormal32(c.gd * f32(0.01)).sum() == 1
        if not c.perturb:
            assert c.z[SUBNORMAL].min() == np.float64(near) > 0      # the subnormal itself is the row's first sample
        if c.pool != 'inside':
            cl = far_bb < 0                                           # with depth the clamp then gives far == 0
            assert cl[R['outside_away']] and cl[R['outside_away_z']] and c.gd[R['outside_away']] == 0 < c.gd[R['outside_away_z']]
            if not c.perturb and c.n_lin >= 2:
                assert c.z[R['outside_away_z'], :].min() == 0.0
    if c.depth in ('mixed', 'positive'):
        for a, b in EQUAL:
            assert c.gd[a] == c.gd[b] > 0
        assert c.gd[N - 1] == c.gd.max() > c.gd[:-1].max()
        cap = np.float64(c.dmax[1])
        binds = np.maximum(far_bb, 0) > cap
        assert binds.any() and (~binds & (far_bb > 0)).any(), c.name
    if c.depth == 'shallow':
        assert (np.maximum(far_bb, 0) > np.float64(c.dmax[1])).sum() > N // 2
    if c.depth == 'zero':
        assert c.dmax[0] == 0 and c.dmax[1] == 0
