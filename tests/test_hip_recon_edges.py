"""-m gpu: csrc/mesh_depth.hip (functional.mesh_depth) and csrc/nearest.hip (functional.nearest, functional.NearestIndex) on the
exact cases of tests/recon_edge_cases.py: rays through vertices, along edges and shared diagonals, t == z_far and t == z_near,
degenerate triangles, the camera plane, the split between the one-thread and the one-workgroup route, one-pixel images;
exact ties between distinct reference points, planar and collinear sets, an outlier, queries outside the box, every
max_rings, max_dist at an attained distance, both sides of the tile and block sizes.  Every pixel and every query is compared
with the exact yardstick bit for bit, none excused; the cases with generic coordinates keep the two bars of
tests/test_hip_recon.py.  Guard regions around the outputs and behind the workspaces stay intact."""
import ctypes

import numpy as np
import pytest
import torch

from tests import recon_edge_cases as E

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
GUARD = 256
RINGS = (0, 1, 2, None, 64)


def dev(a, dtype=torch.float64):
    return torch.from_numpy(np.array(a)).to(DEV, dtype)             # a copy: the shared case arrays are read-only


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint64)


# ---- mesh depth -------------------------------------------------------------------------------------------------------------
def _depth(c, faces=None, views=slice(None)):
    from evennicer_slam_amd import functional as EF
    w2c = np.array(c['w2c'][views])                                         # a copy: the case arrays are read-only
    d = EF.mesh_depth(dev(c['vertices']), dev(c['faces'] if faces is None else faces, torch.int32), w2c, c['cam'],
                      z_near=c['z_near'], z_far=c['z_far'])
    torch.cuda.synchronize()
    assert d.dtype == torch.float32 and tuple(d.shape) == (len(w2c), c['cam']['H'], c['cam']['W'])
    return d.cpu().numpy()


def _same_bits(got, want, what):
    differ = bits(got) != bits(want)
    print(f"{what}: hit {int((want > 0).sum())} of {want.size}, differing {int(differ.sum())}")
    assert not differ.any(), (what, [(tuple(p), got[tuple(p)], want[tuple(p)]) for p in np.argwhere(differ)[:8]])


@pytest.mark.parametrize("name", E.DEPTH_NAMES)
def test_mesh_depth_equals_the_exact_contract(name):
    c = E.depth_cases()[name]
    got = _depth(c)
    _same_bits(got, c['want'], name)
    assert np.array_equal(bits(_depth(c)), bits(got))                       # run to run


def test_mesh_depth_box_split_routes_agree():
    """16 x 16 = TRI_SMALL pixels of box: the thread rasterises it; 16 x 17: a workgroup does; together: both in one call"""
    c = E.depth_cases()
    small, large, both = (_depth(c[n]) for n in ('box_split/256', 'box_split/272', 'box_split/both'))
    for n, got in (('box_split/256', small), ('box_split/272', large), ('box_split/both', both)):
        _same_bits(got, c[n]['want'], n)
    assert not ((small > 0) & (large > 0)).any()
    assert np.array_equal(bits(both), np.where(small > 0, bits(small), bits(large)))
    # each triangle of the pair alone, picked out of the pair's mesh
    pair = c['box_split/both']
    assert np.array_equal(bits(_depth(pair, faces=pair['faces'][:1])), bits(small))
    assert np.array_equal(bits(_depth(pair, faces=pair['faces'][1:])), bits(large))


def test_mesh_depth_many_views_in_one_call_and_one_by_one():
    c = E.depth_cases()['many']
    got = _depth(c)
    _same_bits(got, c['want'], 'many, K = 3')
    singles = np.concatenate([_depth(c, views=slice(k, k + 1)) for k in range(3)])
    assert np.array_equal(bits(singles), bits(got))


def test_mesh_depth_degenerate_triangles_change_nothing():
    c = E.depth_cases()['degenerate']
    assert np.array_equal(bits(_depth(c, faces=c['faces'][:3])), bits(_depth(c)))


@pytest.mark.parametrize("name", ['seam', 'camera_plane', 'box_split/both', 'many', 'shape/1x1/hit', 'shape/24x1/edge'])
def test_mesh_depth_guard_regions(name):
    """the raw entry: the images sit between GUARD sentinel elements inside one allocation, the workspace has the bytes
    enslam_mesh_depth_workspace states and a sentinel tail; the sentinels stay and every pixel inside is written"""
    from evennicer_slam_amd import _lib as L
    from evennicer_slam_amd import functional as EF
    c = E.depth_cases()[name]
    v, f, w = dev(c['vertices']), dev(c['faces'], torch.int32), dev(c['w2c']).contiguous()
    V, F, K, H, W = len(c['vertices']), len(c['faces']), len(c['w2c']), c['cam']['H'], c['cam']['W']
    nbytes = ctypes.c_int64(0)
    L.check(L.lib().enslam_mesh_depth_workspace(F, K, ctypes.byref(nbytes)), "workspace")
    assert nbytes.value == 256 + 8 * F * K
    n = K * H * W
    out = torch.full((n + 2 * GUARD,), -7.5, dtype=torch.float32, device=DEV)
    ws = torch.full((nbytes.value + 8 * GUARD,), 0xA5, dtype=torch.uint8, device=DEV)
    cam = c['cam']
    rc = L.lib().enslam_mesh_depth(v.data_ptr(), V, f.data_ptr(), F, w.data_ptr(), K, H, W, cam['fx'], cam['fy'], cam['cx'], cam['cy'],
                                   c['z_near'], c['z_far'], ws.data_ptr(), out[GUARD:].data_ptr(), EF._stream())
    torch.cuda.synchronize()
    assert rc == 0
    assert bool((out[:GUARD] == -7.5).all()) and bool((out[GUARD + n:] == -7.5).all())
    assert bool((ws[nbytes.value:] == 0xA5).all())
    inside = out[GUARD:GUARD + n].cpu().numpy().reshape(K, H, W)
    assert not (inside == -7.5).any()                                       # every pixel was written
    _same_bits(inside, c['want'], name + ' (raw entry)')


# ---- nearest neighbour ------------------------------------------------------------------------------------------------------
def _nearest(q, r, **kw):
    from evennicer_slam_amd import functional as EF
    d, i = EF.nearest(dev(q), dev(r), **kw)
    torch.cuda.synchronize()
    assert d.dtype == torch.float64 and i.dtype == torch.int32 and tuple(d.shape) == tuple(i.shape) == (len(q),)
    return d.cpu().numpy(), i.cpu().numpy()


def _check_nearest(c, d, i, what):
    """exact cases: the indices and the distance bits; the others: the two bars of test_nearest_matches_brute_force"""
    if c['exact']:
        wrong = (i != c['idx']) | (bits(d) != bits(c['dist']))
        assert not wrong.any(), (what, [(int(m), i[m], c['idx'][m], d[m], c['dist'][m]) for m in np.nonzero(wrong)[0][:8]])
    else:
        assert np.array_equal(i, c['idx']), what
        assert (np.abs(d - c['dist']) <= 1e-12 * c['dist']).all(), what


# where the brute-force tail must have been reached after one shell: (case, group of queries)
TAIL_AT_ONE_RING = {'outside': 'boxes30', 'planar': 'far'}


@pytest.mark.parametrize("name", E.NEAREST_NAMES)
def test_nearest_equals_the_yardstick_at_every_max_rings(name):
    c = E.nearest_cases()[name]
    results, tails = {}, {}
    for rings in RINGS:
        stats = {}
        results[rings] = _nearest(c['query'], c['ref'], max_rings=rings, stats=stats)
        tails[rings] = stats['tail']
    print(f"{name}: N {len(c['ref'])}, M {len(c['query'])}, tail at max_rings " + ", ".join(f"{r}: {t}" for r, t in tails.items()))
    d0, i0 = results[0]
    for rings, (d, i) in results.items():
        assert np.array_equal(i, i0) and np.array_equal(bits(d), bits(d0)), f"{name}: max_rings {rings} differs from brute force"
        _check_nearest(c, d, i, f"{name}, max_rings {rings}")
    assert tails[0] == len(c['query'])
    if name in TAIL_AT_ONE_RING:
        sl = c['groups'][TAIL_AT_ONE_RING[name]]
        stats = {}
        d, i = _nearest(c['query'][sl], c['ref'], max_rings=1, stats=stats)
        print(f"{name}: tail at max_rings 1 on the {TAIL_AT_ONE_RING[name]} queries: {stats['tail']} of {sl.stop - sl.start}")
        assert stats['tail'] > 0
        assert np.array_equal(i, i0[sl]) and np.array_equal(bits(d), bits(d0[sl]))
    if name == 'lattice':
        assert tails[64] == 0                                               # every query left the shell loop on its own


@pytest.mark.parametrize("rings", RINGS)
def test_nearest_max_dist_at_an_attained_distance(rings):
    """d < max_dist, strict: the 150 queries one step off the lattice have their nearest point at exactly 1.0"""
    c = E.nearest_cases()['lattice']
    at_one = c['dist'] == 1.0
    assert at_one.sum() == 150
    for max_dist in (1.0, float(np.nextafter(1.0, 2.0)), float(np.nextafter(1.0, 0.0)), 0.5, 0.0):
        want_d, want_i = E.apply_max_dist(c['dist'], c['idx'], max_dist)
        d, i = _nearest(c['query'], c['ref'], max_dist=max_dist, max_rings=rings)
        assert np.array_equal(i, want_i) and np.array_equal(bits(d), bits(want_d)), (rings, max_dist)
    d, i = _nearest(c['query'], c['ref'], max_dist=1.0, max_rings=rings)
    assert (i[at_one] == -1).all() and np.isinf(d[at_one]).all() and (i[c['dist'] < 1.0] >= 0).all()
    d, i = _nearest(c['query'], c['ref'], max_dist=float(np.nextafter(1.0, 2.0)), max_rings=rings)
    assert np.array_equal(i, c['idx']) and (d[at_one] == 1.0).all()
    d, i = _nearest(c['query'], c['ref'], max_dist=0.0, max_rings=rings)
    assert (i == -1).all() and np.isinf(d).all() and (c['dist'] == 0).sum() >= 125


@pytest.mark.parametrize("rings", RINGS)
def test_nearest_small_max_dist_outside_the_box(rings):
    """every query is at least half a box away: lb >= max_dist stops the shells at once, and nothing is found"""
    c = E.nearest_cases()['outside']
    assert c['dist'].min() > 1e-3
    d, i = _nearest(c['query'], c['ref'], max_dist=1e-3, max_rings=rings)
    assert (i == -1).all() and np.isinf(d).all()


def test_nearest_index_is_reusable():
    """one NearestIndex queried three times with different M (M = 0 in between), as the ICP does: the results of fresh ones"""
    from evennicer_slam_amd import functional as EF
    c = E.nearest_cases()['planar']
    index = EF.NearestIndex(dev(c['ref']))
    q = c['query']
    for part in (slice(0, 300), slice(0, 0), slice(300, 317), slice(0, len(q))):
        d, i = index.query(dev(q[part]))
        torch.cuda.synchronize()
        d, i = d.cpu().numpy(), i.cpu().numpy()
        assert d.shape == i.shape == (part.stop - part.start,)
        if len(d):
            fd, fi = _nearest(q[part], c['ref'])
            assert np.array_equal(i, fi) and np.array_equal(bits(d), bits(fd))
            assert np.array_equal(i, c['idx'][part]) and np.array_equal(bits(d), bits(c['dist'][part]))


@pytest.mark.parametrize("rings", (1, 4, 64))
@pytest.mark.parametrize("name", ['lattice', 'collinear', 'outlier'])
def test_nearest_guard_regions(name, rings):
    """the raw entries: dist and idx sit between GUARD sentinel elements, the grid and the query workspace have the bytes
    enslam_nn_workspace states and a sentinel tail; the sentinels stay and every element inside is written"""
    from evennicer_slam_amd import _lib as L
    from evennicer_slam_amd import functional as EF
    lib = L.lib()
    c = E.nearest_cases()[name]
    ref, qry = dev(c['ref']), dev(c['query'])
    N, M = len(c['ref']), len(c['query'])
    gb, qb = ctypes.c_int64(0), ctypes.c_int64(0)
    L.check(lib.enslam_nn_workspace(N, M, ctypes.byref(gb), ctypes.byref(qb)), "workspace")
    grid = torch.full((gb.value + 8 * GUARD,), 0xA5, dtype=torch.uint8, device=DEV)
    qws = torch.full((qb.value + 8 * GUARD,), 0xA5, dtype=torch.uint8, device=DEV)
    dist = torch.full((M + 2 * GUARD,), -7.5, dtype=torch.float64, device=DEV)
    idx = torch.full((M + 2 * GUARD,), -77, dtype=torch.int32, device=DEV)
    tail = torch.zeros(1, dtype=torch.int32, device=DEV)
    assert lib.enslam_nn_build(ref.data_ptr(), N, grid.data_ptr(), EF._stream()) == 0
    rc = lib.enslam_nn_query(ref.data_ptr(), N, qry.data_ptr(), M, float('inf'), rings, grid.data_ptr(), qws.data_ptr(),
                             dist[GUARD:].data_ptr(), idx[GUARD:].data_ptr(), tail.data_ptr(), EF._stream())
    torch.cuda.synchronize()
    assert rc == 0
    assert bool((grid[gb.value:] == 0xA5).all()) and bool((qws[qb.value:] == 0xA5).all())
    for buf, fill in ((dist, -7.5), (idx, -77)):
        assert bool((buf[:GUARD] == fill).all()) and bool((buf[GUARD + M:] == fill).all())
        assert not bool((buf[GUARD:GUARD + M] == fill).any())               # every query was answered
    _check_nearest(c, dist[GUARD:GUARD + M].cpu().numpy(), idx[GUARD:GUARD + M].cpu().numpy(), f"{name} (raw entries), max_rings {rings}")
    assert 0 <= int(tail.item()) <= M
