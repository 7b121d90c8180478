"""Seeded inputs for the block-flag and grid-movement tests (tests/test_blocks_cpu.py, tests/test_hip_blocks.py) and the
conditions they rely on, counted through the numpy yardstick alone (tests/blocks_numpy.py).

Scenes (grids as (D, H, W); grid 0 lives over the coarse bound = 2 * bound, as the product path has it):
  exact   bound x [-1, 1], y [0, 4], z [-1, 1]: every extent a power of two, so cell coordinates of dyadic points are exact
          0 (5, 7, 9)      V = 315: V % 64 != 0 and V % 4 != 0 (partial last block, scalar zero-fill)
          1 (9, 9, 17)     W - 1 = 16: integer cell coordinates are exact in float32
          2 (12, 20, 28)   V = 6720 = 105 whole blocks; W = 28 does not divide 64 (an x-pair straddles block edges)
          3 (11, 13, 5)    W < 8: the z-neighbour of a tap lies 65 voxels on, several 8- and 16-voxel blocks away
  room0   the non-round bound of tests/golden/bounds.npz (room0)
          0 (6, 5, 3)   1 (5, 7, 9)   2 (10, 6, 16) (V = 960 = 15 whole blocks, W divides 64)   3 (7, 9, 11) (V % 4 == 1)
  small   exact's bound; 0 (2, 3, 4)   1 (5, 7, 9)   2 (4, 4, 4) (exactly one block)   3 (3, 3, 3) (less than one block)
Every scene's four grids differ in size.

Cases are (ro float32 [N, 3], rd float32 [N, 3], z float64 [N, S] ascending per ray, gt_depth float32 [N]), N <= 64:
  planes    exact, S = 48: axis-aligned and diagonal rays whose samples sit ON the cell planes of grid 1 and a few float32 ulps
            to either side of them
  faces     exact, S = 16: rays inside each of the six bound faces and outside each of them, rays through the whole bound, rays
            along the top edge (the partial last block of grid 0)
  random64  room0, S = 64: random rays from inside that leave the bound on every side
  random32  exact, S = 32: the same over the exact bound
  local     exact, S = 16: a handful of short rays around one spot: most blocks of every grid stay unflagged (the cases above
            flag most 64-voxel blocks of grids this small)
  below_planes  exact, S = 16: rays that only hold points a fraction of a float32 spacing below cell planes of grid 1 (on the
            plane in float32, one cell lower for a floor taken in float64), with nothing else near them
  lattice   small, S = 16: one ray along x through every (y, z) row of grid 1: every block of grid 1 is flagged at every size
  no_rays   small, S = 16, N = 0: nothing is flagged anywhere
Every case with rays ends with 8 `sampler rays` (origin strictly inside, no zero direction component, gt_depth > 0 for the even
ones): the subset the sampler routes use, whose far bound is finite by construction.

Flag patterns for the movement kernels: zeros, ones, random 30 %, first and last block of every grid only, everything but those."""
import os

import numpy as np

from tests import blocks_numpy as Y

F32, F64 = np.float32, np.float64
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')

_EXACT = np.array([[-1.0, 1.0], [0.0, 4.0], [-1.0, 1.0]])
_ROOM0 = np.load(os.path.join(GOLDEN, 'bounds.npz'))['room0_bound'].astype(F64)

SCENES = {
    'exact': dict(bound=_EXACT, coarse_bound=_EXACT * 2, dims={0: (5, 7, 9), 1: (9, 9, 17), 2: (12, 20, 28), 3: (11, 13, 5)}),
    'room0': dict(bound=_ROOM0, coarse_bound=_ROOM0 * 2, dims={0: (6, 5, 3), 1: (5, 7, 9), 2: (10, 6, 16), 3: (7, 9, 11)}),
    'small': dict(bound=_EXACT, coarse_bound=_EXACT * 2, dims={0: (2, 3, 4), 1: (5, 7, 9), 2: (4, 4, 4), 3: (3, 3, 3)}),
}
N_SAMPLER_RAYS = 8


def n_voxels(dims):
    return int(dims[0]) * int(dims[1]) * int(dims[2])


# grid sets of the movement tests: single grids, then the scenes' grids as launches over n = 1..4 grids
GRID_SETS = {'whole_blocks': [(12, 20, 28)], 'partial': [(5, 7, 9)], 'one_block': [(4, 4, 4)], 'below_one_block': [(3, 3, 3)]}
for _name, _sc in SCENES.items():
    for _n in (2, 3, 4):
        GRID_SETS[f'{_name}_{_n}'] = [_sc['dims'][k] for k in range(_n)]
PATTERNS = ('zeros', 'ones', 'random', 'ends', 'not_ends')


def flag_pattern(pattern, dims_list, seed=0):
    """[uint8 flags per 64-voxel block] for every grid of a grid set"""
    rng = np.random.default_rng(seed)
    out = []
    for d in dims_list:
        nb = Y.n_blocks(n_voxels(d))
        ends = np.zeros(nb, dtype=np.uint8)
        ends[[0, nb - 1]] = 1
        r = (rng.uniform(size=nb) < 0.3).astype(np.uint8)
        out.append({'zeros': np.zeros(nb, np.uint8), 'ones': np.ones(nb, np.uint8), 'random': r, 'ends': ends,
                    'not_ends': (1 - ends).astype(np.uint8)}[pattern])
    return out


# ------------------------------------------------------------------------------------------------ rays
def _sampler_rays(rng, bound):
    """origins strictly inside, directions with no zero component"""
    lo, hi = bound[:, 0], bound[:, 1]
    ro = (lo + (hi - lo) * rng.uniform(0.2, 0.8, (N_SAMPLER_RAYS, 3))).astype(F32)
    rd = (rng.uniform(0.3, 1.0, (N_SAMPLER_RAYS, 3)) * rng.choice([-1.0, 1.0], (N_SAMPLER_RAYS, 3))).astype(F32)
    return ro, rd


def _finish(rng, scene, S, ro, rd, z, reach=1.2):
    """append the sampler rays (their samples reach `reach` extents far), sort each ray's z, attach gt_depth"""
    bound = SCENES[scene]['bound']
    sro, srd = _sampler_rays(rng, bound)
    ext = float((bound[:, 1] - bound[:, 0]).max())
    sz = rng.uniform(0.0, reach * ext, (N_SAMPLER_RAYS, S))
    ro = np.concatenate([np.asarray(ro, F32).reshape(-1, 3), sro])
    rd = np.concatenate([np.asarray(rd, F32).reshape(-1, 3), srd])
    z = np.sort(np.concatenate([np.asarray(z, F64).reshape(-1, S), sz]), axis=1)
    N = ro.shape[0]
    gt = (0.3 * ext * rng.uniform(0.5, 1.5, N)).astype(F32)
    gt[1::2] = 0.0                                          # no depth reading: the sampler spreads the surface samples instead
    sampler = np.arange(N - N_SAMPLER_RAYS, N)
    assert N <= 64 and S in (16, 32, 48, 64)
    assert np.all(srd != 0) and np.all(sro > bound[:, 0]) and np.all(sro < bound[:, 1])
    return dict(scene=scene, S=S, ro=ro, rd=rd, z=z, gt_depth=gt, sampler_rays=sampler, **SCENES[scene])


def _planes(rng):
    """exact scene, grid 1 = (9, 9, 17): x = -1 + j / 8, y = j / 2, z = -1 + j / 4 are its cell planes"""
    S = 48
    ro, rd, z = [], [], []
    mids = [(0.3, -0.35), (1.7, 0.15), (3.1, 0.6), (2.2, -0.8)]

    def ladder(t_planes):
        """S distances: every plane distance and 1/2, 1 and 2 float32 spacings of it to either side (the cell coordinate is a
        power of two times the distance here, so these land on the float32 neighbours of the plane; count_conditions counts),
        and 1/1000 of a spacing to either side: on the plane once cast to float32, beside it in float64"""
        t = []
        for tp in t_planes:
            e = float(np.spacing(F32(tp)))
            t += [tp] + [tp + s * u * e for u in (0.001, 0.5, 1.0, 2.0) for s in (1.0, -1.0)]
        return np.resize(np.array(t, dtype=F64), S)

    def add(o, d, t_planes):
        for i in range(0, len(t_planes), 5):
            ro.append(o); rd.append(d); z.append(ladder(t_planes[i:i + 5]))

    for (a, b) in mids:
        add((-1.0, a, b), (1.0, 0.0, 0.0), [j / 8.0 for j in range(1, 16)])      # along +x: x = -1 + t, planes at t = j / 8
        add((b, 0.0, b * 0.5), (0.0, 1.0, 0.0), [j / 2.0 for j in range(1, 8)])     # along +y: y = t, planes at t = j / 2
        add((b, a, -1.0), (0.0, 0.0, 1.0), [j / 4.0 for j in range(1, 8)])          # along +z: z = -1 + t, planes at t = j / 4
    add((-1.0, 0.0, -1.0), (1.0, 2.0, 1.0), [j / 8.0 for j in range(1, 16)])        # diagonal (-1 + t, 2 t, -1 + t)
    return _finish(rng, 'exact', S, ro, rd, z)


def _below_planes(rng):
    """exact scene, grid 1: rays that ONLY hold points 1/1000 of a float32 spacing below every third cell plane of their axis.
    float32 puts such a point on the plane (taps j, j + 1); a floor taken in float64 puts it one cell lower (taps j - 1, j).  The
    sampler rays stay around one spot, away from these rows, so that nothing else flags the blocks in question."""
    S = 16
    ro, rd, z = [], [], []

    def below(step):
        return np.resize(np.array([j * step - 0.001 * float(np.spacing(F32(j * step))) for j in (2, 5)], dtype=F64), S)

    for (y, zz) in ((2.7, -0.1), (0.8, 0.7)):
        ro.append((-1.0, y, zz)); rd.append((1.0, 0.0, 0.0)); z.append(below(1 / 8.0) if y > 1 else below(1 / 8.0) + 1.0)
    ro.append((0.55, 0.0, -0.6)); rd.append((0.0, 1.0, 0.0)); z.append(below(1 / 2.0))
    ro.append((-0.55, 3.3, -1.0)); rd.append((0.0, 0.0, 1.0)); z.append(below(1 / 4.0))
    c = _finish(rng, 'exact', S, ro, rd, z, reach=0.05)
    spot = np.array([-0.8, 0.3, -0.8])
    c['ro'][c['sampler_rays']] = (spot + rng.uniform(-0.05, 0.05, (N_SAMPLER_RAYS, 3))).astype(F32)
    return c


def _faces(rng):
    S = 16
    b = _EXACT
    mid = b.mean(axis=1)
    ro, rd, z = [], [], []
    for a in range(3):
        other = (a + 1) % 3
        ext = b[other, 1] - b[other, 0]
        for side in (0, 1):
            sign = -1.0 if side == 0 else 1.0
            for off in (0.0, 0.3 * sign, 1.7 * sign):       # inside the face, just outside, far outside (beyond the coarse bound)
                o = mid.copy()
                o[a] = b[a, side] + off
                o[other] = b[other, 0] - 0.25 * ext
                d = np.zeros(3)
                d[other] = 1.0
                ro.append(o); rd.append(d); z.append(np.linspace(0.0, 1.5 * ext, S))
        o = mid.copy()                                      # through the whole bound along the axis, from outside to outside
        o[a] = b[a, 0] - 0.5 * (b[a, 1] - b[a, 0])
        d = np.zeros(3)
        d[a] = 1.0
        ro.append(o); rd.append(d); z.append(np.linspace(0.0, 2.0 * (b[a, 1] - b[a, 0]), S))
    for frac in (0.93, 0.97, 1.0, 1.04):                    # along x near the top y and z faces: the last voxels of every grid
        o = np.array([b[0, 0], b[1, 0] + frac * (b[1, 1] - b[1, 0]), b[2, 0] + frac * (b[2, 1] - b[2, 0])])
        ro.append(o); rd.append((1.0, 0.0, 0.0)); z.append(np.linspace(0.0, 2.0, S))
        o2 = b[:, 0] + frac * (b[:, 1] - b[:, 0]) * 2 - (b[:, 1] - b[:, 0]) * 0.5      # the same for the coarse bound
        ro.append(o2); rd.append((1.0, 0.0, 0.0)); z.append(np.linspace(-1.0, 1.0, S))
    return _finish(rng, 'exact', S, ro, rd, z)


def _random(rng, scene, S, N):
    b = SCENES[scene]['bound']
    lo, hi = b[:, 0], b[:, 1]
    ro = lo + (hi - lo) * rng.uniform(0.05, 0.95, (N, 3))
    rd = rng.normal(size=(N, 3))
    rd /= np.linalg.norm(rd, axis=1, keepdims=True)
    z = rng.uniform(0.0, 1.3 * float((hi - lo).max()), (N, S))
    return _finish(rng, scene, S, ro, rd, z)


def _local(rng):
    """a handful of short rays around one spot: most blocks of every grid stay unflagged"""
    S = 16
    b = _EXACT
    spot = b[:, 0] + (b[:, 1] - b[:, 0]) * np.array([0.3, 0.6, 0.7])
    ro = spot + rng.uniform(-0.05, 0.05, (8, 3))
    rd = rng.normal(size=(8, 3))
    rd /= np.linalg.norm(rd, axis=1, keepdims=True)
    c = _finish(rng, 'exact', S, ro, rd, rng.uniform(0.0, 0.3, (8, S)), reach=0.08)
    c['ro'][c['sampler_rays']] = (spot + rng.uniform(-0.05, 0.05, (N_SAMPLER_RAYS, 3))).astype(F32)
    return c


def _lattice(rng):
    S = 16
    b = _EXACT
    D, H, W = SCENES['small']['dims'][1]
    ro, rd, z = [], [], []
    for iz in range(D):
        for iy in range(H):
            y = b[1, 0] + (b[1, 1] - b[1, 0]) * (iy + 0.25) / (H - 1) if iy < H - 1 else b[1, 1]
            zz = b[2, 0] + (b[2, 1] - b[2, 0]) * (iz + 0.25) / (D - 1) if iz < D - 1 else b[2, 1]
            ro.append((b[0, 0], y, zz)); rd.append((1.0, 0.0, 0.0)); z.append(np.linspace(0.0, b[0, 1] - b[0, 0], S))
    return _finish(rng, 'small', S, ro, rd, z)


def _no_rays():
    e = np.zeros((0, 3), dtype=F32)
    return dict(scene='small', S=16, ro=e, rd=e.copy(), z=np.zeros((0, 16), F64), gt_depth=np.zeros(0, F32),
                sampler_rays=np.zeros(0, np.int64), **SCENES['small'])


def _build():
    rng = np.random.default_rng(20240611)
    return {'planes': _planes(rng), 'faces': _faces(rng), 'random64': _random(rng, 'room0', 64, 56),
            'random32': _random(rng, 'exact', 32, 40), 'local': _local(rng), 'below_planes': _below_planes(rng), 'lattice': _lattice(rng), 'no_rays': _no_rays()}


CASES = _build()
CASE_NAMES = tuple(CASES)
RAY_CASES = tuple(n for n in CASE_NAMES if CASES[n]['ro'].shape[0] > 0)     # cases a render call can run


def points(case):
    c = CASES[case] if isinstance(case, str) else case
    return Y.sample_points(c['ro'], c['rd'], c['z'])


def expected_flags(case, stage, block_voxels, z=None, rays=None, before=None):
    """{k: flags} of the yardstick for a case (z: other sample distances for the same rays; rays: a subset of the rays)"""
    c = CASES[case] if isinstance(case, str) else case
    ro, rd, zz = c['ro'], c['rd'], c['z'] if z is None else z
    if rays is not None:
        ro, rd = ro[rays], rd[rays]
        zz = zz[rays] if z is None else zz
    return Y.scene_flags(Y.sample_points(ro, rd, zz), stage, c['bound'], c['coarse_bound'], c['dims'], block_voxels, before)


# ------------------------------------------------------------------------------------------------ conditions, counted here
def _grids_of(c):
    for k, d in c['dims'].items():
        yield k, d, Y.lookup_bound(k, c['bound'], c['coarse_bound'])


def count_conditions():
    """the counts the tests assert (tests/test_blocks_cpu.py::test_case_conditions), summed over all cases; a sample counts once per
    condition however many grids or axes meet it"""
    n = dict(on_plane=0, ulp_below=0, ulp_above=0, partial_block=0, z_jump=0)
    n.update({f'straddle_{bs}': 0 for bs in Y.BLOCK_SIZES})
    n.update({f'{kind}_{ax}{side}': 0 for kind in ('face', 'outside') for ax in 'xyz' for side in ('lo', 'hi')})
    for c in CASES.values():
        pts = points(c)
        P = pts.shape[0]
        if P == 0:
            continue
        on, below, above, partial, zjump = (np.zeros(P, bool) for _ in range(5))
        straddle = {bs: np.zeros(P, bool) for bs in Y.BLOCK_SIZES}
        for k, d, bnd in _grids_of(c):
            D, H, W = d
            for a, size in ((0, W), (1, H), (2, D)):
                cu = Y.unnormalise(Y.normalise(pts[:, a], bnd[a, 0], bnd[a, 1]), size)      # float32, before the clip
                r = np.rint(cu)
                interior = (r > 0) & (r < size - 1)
                on |= interior & (cu == r)
                below |= interior & (cu == np.nextafter(r, F32(-np.inf)))
                above |= interior & (cu == np.nextafter(r, F32(np.inf)))
            idx, exists, _ = Y.corners(pts, bnd, d)
            V = n_voxels(d)
            if V % 64:
                partial |= (idx >= (V // 64) * 64).any(axis=1)
            for bs in Y.BLOCK_SIZES:
                pair = exists[:, 1::2] & (Y.block_of(idx[:, 0::2], bs) != Y.block_of(idx[:, 1::2], bs))
                straddle[bs] |= pair.any(axis=1)
            zjump |= exists[:, 4] & (Y.block_of(idx[:, 4], 8) - Y.block_of(idx[:, 0], 8) > 1) & (W < 8)
        for a, ax in enumerate('xyz'):
            lo, hi = c['bound'][a]
            n[f'face_{ax}lo'] += int((pts[:, a] == lo).sum())
            n[f'face_{ax}hi'] += int((pts[:, a] == hi).sum())
            n[f'outside_{ax}lo'] += int((pts[:, a] < lo).sum())
            n[f'outside_{ax}hi'] += int((pts[:, a] > hi).sum())
        n['on_plane'] += int(on.sum()); n['ulp_below'] += int(below.sum()); n['ulp_above'] += int(above.sum())
        n['partial_block'] += int(partial.sum()); n['z_jump'] += int(zjump.sum())
        for bs in Y.BLOCK_SIZES:
            n[f'straddle_{bs}'] += int(straddle[bs].sum())
    return n


MINIMUM = dict(on_plane=32, ulp_below=32, ulp_above=32, partial_block=16, z_jump=16)
MINIMUM.update({f'straddle_{bs}': 16 for bs in Y.BLOCK_SIZES})
MINIMUM.update({f'{kind}_{ax}{side}': 16 for kind in ('face', 'outside') for ax in 'xyz' for side in ('lo', 'hi')})
