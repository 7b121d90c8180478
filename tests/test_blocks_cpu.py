"""The numpy yardstick of the block flags and the block-sparse grid movement (tests/blocks_numpy.py) against the golden fixtures
and against torch on the CPU, the conditions of the seeded cases (tests/blocks_cases.py), and the sharpness of those cases: each
of a list of plausible faults, written as a one-line change of the yardstick, changes a flag array or a moved array of at least
one case.  No kernel runs here; tests/test_hip_blocks.py holds the kernels to the same yardstick on the GPU."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import blocks_cases as K
from tests import blocks_numpy as Y
from tests.util import load

F32, F64 = np.float32, np.float64
GRID_NAMES = {0: 'grid_coarse', 1: 'grid_middle', 2: 'grid_fine', 3: 'grid_color'}


# ------------------------------------------------------------------------------------------------ yardstick vs goldens
@pytest.mark.parametrize('stage', Y.STAGES)
def test_cells_reproduce_the_golden_voxel_indices(stage):
    """ix, iy, iz, fx, fy, fz of every grid the stage reads, from the golden sample points, bit for bit"""
    scene, g = load('tiny_scene'), load('tiny_' + stage)
    bound = scene['bound'].astype(F64)
    seen = 0
    for k in Y.stage_grids(stage):
        name = GRID_NAMES[k]
        v = Y.cells(g['pts'], Y.lookup_bound(k, bound, bound * 2), scene[name].shape[2:])
        for key in ('ix', 'iy', 'iz', 'fx', 'fy', 'fz'):
            want = g[f'vox_{name}_{key}']
            assert v[key].dtype == want.dtype and np.array_equal(v[key], want), (stage, name, key)
            seen += 1
    assert seen == 6 * len(Y.stage_grids(stage))


def test_sample_points_reproduce_the_golden_points():
    scene, g = load('tiny_scene'), load('tiny_color')
    assert np.array_equal(Y.sample_points(scene['rays_o'], scene['rays_d'], g['z_vals']), g['pts'])


# ------------------------------------------------------------------------------------------------ yardstick vs torch (CPU)
def _grid_sample_gradient(pts, bound, dims):
    """bool [V]: voxels of a one-channel grid with a non-zero gradient of sum(F.grid_sample(...)) at the points"""
    D, H, W = dims
    p = torch.from_numpy(np.array(pts))
    b = torch.from_numpy(np.array(bound))
    for a in range(3):                                      # common.normalize_3d_coordinate, float64
        p[:, a] = ((p[:, a] - b[a, 0]) / (b[a, 1] - b[a, 0])) * 2 - 1.0
    vgrid = p.float()[None, :, None, None, :]
    grid = torch.ones((1, 1, D, H, W), dtype=torch.float32, requires_grad=True)
    F.grid_sample(grid, vgrid, padding_mode='border', align_corners=True, mode='bilinear').sum().backward()
    return (grid.grad.reshape(-1) != 0).numpy()


@pytest.mark.parametrize('case', K.RAY_CASES)
def test_corner_set_against_grid_sample_on_the_cpu(case):
    c = K.CASES[case]
    pts = K.points(case)
    for k, d in c['dims'].items():
        bnd = Y.lookup_bound(k, c['bound'], c['coarse_bound'])
        touched = _grid_sample_gradient(pts, bnd, d)
        assert not (touched & ~Y.corner_voxels(pts, bnd, d)).any(), (case, k)
        assert np.array_equal(touched, Y.corner_voxels(pts, bnd, d, nonzero_only=True)), (case, k)


def test_flags_cover_the_corner_set_at_every_block_size():
    for case in K.RAY_CASES:
        c = K.CASES[case]
        pts = K.points(case)
        for bs in Y.BLOCK_SIZES:
            fl = Y.scene_flags(pts, 'color', c['bound'], c['coarse_bound'], c['dims'], bs)
            for k in (1, 2, 3):
                vox = np.flatnonzero(Y.corner_voxels(pts, c['bound'], c['dims'][k]))
                want = np.zeros_like(fl[k])
                want[np.unique(vox // bs)] = 1
                assert np.array_equal(fl[k], want), (case, k, bs)
                assert np.array_equal(Y.coarsen(fl[k], bs, K.n_voxels(c['dims'][k])),
                                      Y.scene_flags(pts, 'color', c['bound'], c['coarse_bound'], c['dims'], 64)[k])
            assert not fl[0].any()                          # the colour stage leaves the coarse grid alone


# ------------------------------------------------------------------------------------------------ movement vs torch
def _movement_inputs(dims_list, seed):
    rng = np.random.default_rng(seed)
    V = [K.n_voxels(d) for d in dims_list]
    dense = [rng.standard_normal((Y.C, v)).astype(F32) for v in V]
    vm = [rng.standard_normal((v, Y.C)).astype(F32) for v in V]
    return V, dense, vm


def _voxel_mask(flags, V):
    return torch.from_numpy(np.repeat(flags.astype(bool), Y.BLOCK)[:V])


@pytest.mark.parametrize('pattern', K.PATTERNS)
@pytest.mark.parametrize('gset', list(K.GRID_SETS))
def test_movement_against_torch_expressions(gset, pattern):
    dims_list = K.GRID_SETS[gset]
    V, dense, vm = _movement_inputs(dims_list, 3)
    need = K.flag_pattern(pattern, dims_list, seed=1)
    valid = K.flag_pattern('random', dims_list, seed=2)
    prev = K.flag_pattern('random', dims_list, seed=4)
    t = torch.from_numpy
    for i, d in enumerate(dims_list):
        D, H, W = d
        g5 = t(dense[i]).reshape(1, Y.C, D, H, W)
        assert torch.equal(t(Y.to_voxel_major(dense[i])), g5.permute(0, 2, 3, 4, 1).reshape(V[i], Y.C))
        assert torch.equal(t(Y.from_voxel_major(Y.to_voxel_major(dense[i]))), t(dense[i]))
    got, got_valid = Y.convert_sparse_to_vm(dense, vm, need, valid)
    got_nv, none_valid = Y.convert_sparse_to_vm(dense, vm, need, None)
    zeroed, flat = Y.zero_blocks(vm, need, np.ones(300, F32), 255)
    zeroed_all, _ = Y.zero_blocks(vm, [None] * len(vm))
    fin = Y.finish(vm, dense, need)
    pfin, pneed, pprev = Y.finish_prev(vm, dense, need, prev)
    for i in range(len(dims_list)):
        m, mv, mp = _voxel_mask(need[i], V[i]), _voxel_mask(valid[i], V[i]), _voxel_mask(prev[i], V[i])
        assert torch.equal(t(got[i]), torch.where((m & ~mv)[:, None], t(dense[i]).T, t(vm[i])))
        assert torch.equal(t(got_nv[i]), torch.where(m[:, None], t(dense[i]).T, t(vm[i])))
        assert np.array_equal(got_valid[i], valid[i] | need[i]) and none_valid[i] is None
        assert torch.equal(t(zeroed[i]), torch.where(m[:, None], torch.zeros(()), t(vm[i])))
        assert not zeroed_all[i].any()
        assert torch.equal(t(fin[i]), torch.where(m[None, :], t(vm[i]).T, torch.zeros(())))
        assert torch.equal(t(pfin[i]), torch.where(m[None, :], t(vm[i]).T, torch.where(mp[None, :], torch.zeros(()), t(dense[i]))))
        assert np.array_equal(pprev[i], need[i]) and not pneed[i].any()
    assert not flat[:255].any() and (flat[255:] == 1).all()
    cat = np.concatenate(need)
    n2, p2 = Y.move_flags(cat, np.concatenate(prev), len(cat) - 1)
    assert np.array_equal(p2[:-1], cat[:-1]) and p2[-1] == np.concatenate(prev)[-1] and not n2[:-1].any() and n2[-1] == cat[-1]


def test_launch_blocks_number_the_grids_back_to_back():
    for gset, dims_list in K.GRID_SETS.items():
        want = [(g, b) for g, d in enumerate(dims_list) for b in range(Y.n_blocks(K.n_voxels(d)))]
        assert Y.launch_blocks([K.n_voxels(d) for d in dims_list]) == want, gset


# ------------------------------------------------------------------------------------------------ case conditions
def test_grid_sets_and_bounds():
    all_dims = [d for sc in K.SCENES.values() for d in sc['dims'].values()]
    V = [K.n_voxels(d) for d in all_dims]
    assert any(v % 64 == 0 for v in V)
    assert any(v % 64 != 0 and v % 4 != 0 for v in V)
    assert any((d[2] - 1) & (d[2] - 2) == 0 and d[2] > 2 for d in all_dims)       # W - 1 a power of two
    assert any(64 % d[2] != 0 for d in all_dims) and any(d[2] < 8 for d in all_dims)
    for sc in K.SCENES.values():
        assert len({K.n_voxels(d) for d in sc['dims'].values()}) == 4
    assert np.array_equal(K.SCENES['exact']['bound'][:2], [[-1, 1], [0, 4]])
    assert np.array_equal(K.SCENES['room0']['bound'], np.load(K.GOLDEN + '/bounds.npz')['room0_bound'])
    assert any(len(s) == n for s in K.GRID_SETS.values() for n in (1,)) and {len(s) for s in K.GRID_SETS.values()} == {1, 2, 3, 4}


def test_case_conditions():
    n = K.count_conditions()
    print(n)
    for key, least in K.MINIMUM.items():
        assert n[key] >= least, (key, n[key], least)
    for name, c in K.CASES.items():
        assert c['ro'].dtype == F32 and c['rd'].dtype == F32 and c['z'].dtype == F64 and c['gt_depth'].dtype == F32
        assert c['ro'].shape[0] <= 64 and c['z'].shape == (c['ro'].shape[0], c['S']) and c['S'] in (16, 32, 48, 64)
        assert np.all(np.diff(c['z'], axis=1) >= 0) and np.isfinite(c['z']).all(), name
        if c['ro'].shape[0]:
            r = c['sampler_rays']
            assert len(r) == K.N_SAMPLER_RAYS and np.all(c['rd'][r] != 0)
            assert np.all(c['ro'][r] > c['bound'][:, 0]) and np.all(c['ro'][r] < c['bound'][:, 1])
            assert (c['gt_depth'][r] > 0).any() and (c['gt_depth'][r] == 0).any()
    assert {c['S'] for c in K.CASES.values()} == {16, 32, 48, 64}


def test_a_case_flags_nothing_and_a_case_flags_every_block():
    for bs in Y.BLOCK_SIZES:
        for stage in Y.STAGES:
            assert not any(f.any() for f in K.expected_flags('no_rays', stage, bs).values())
        assert K.expected_flags('lattice', 'color', bs)[1].all()
        for k, f in K.expected_flags('local', 'color', bs).items():      # the case that keeps the sparse tests from being vacuous
            assert k == 0 or 0 < int(f.sum()) < len(f) // 2, (k, bs)


# ------------------------------------------------------------------------------------------------ sharpness
def _all_flags():
    out = []
    for case in K.CASE_NAMES:
        for stage in Y.STAGES:
            for bs in Y.BLOCK_SIZES:
                f = K.expected_flags(case, stage, bs)
                out += [f[k] for k in sorted(f)]
    return out


def _all_weight_sets():
    """the voxels with a non-zero tap weight: what the scatter tests hold the gradients to"""
    out = []
    for case in K.RAY_CASES:
        c = K.CASES[case]
        out += [Y.corner_voxels(K.points(case), Y.lookup_bound(k, c['bound'], c['coarse_bound']), d, nonzero_only=True)
                for k, d in c['dims'].items()]
    return out


def _all_moved():
    out = []
    for gset, dims_list in K.GRID_SETS.items():
        V, dense, vm = _movement_inputs(dims_list, 3)
        for pattern in K.PATTERNS:
            need = K.flag_pattern(pattern, dims_list, seed=1)
            prev = K.flag_pattern('random', dims_list, seed=4)
            out += Y.convert_sparse_to_vm(dense, vm, need, None)[0]
            out += Y.zero_blocks(vm, need)[0]
            out += Y.finish(vm, dense, need)
            a, b, c = Y.finish_prev(vm, dense, need, prev)
            out += a + b + c
    return out


def _differs(fn, baseline):
    """a fault shows as a different array somewhere -- or as an index outside an array, numpy's word for an overrun"""
    try:
        got = fn()
    except IndexError:
        return True
    return any(not np.array_equal(a, b) for a, b in zip(got, baseline))


def _cell_clip_after_floor(pn, size):
    c = Y.unnormalise(pn, size)
    fl = Y.clip(np.floor(c), size)
    return fl.astype(np.int32), c - fl, c


def _finish_prev_keeps_prev(src, dst, need, prev):
    d, n, _ = _FINISH_PREV(src, dst, need, prev)
    return d, n, [np.array(p) for p in prev]


_FINISH_PREV = Y.finish_prev
# name -> (attribute of the yardstick, its wrong replacement, what must change)
FAULTS = {
    'floor taken in float64': ('cast32', lambda a: a, 'flags'),
    'no clip': ('clip', lambda c, size: c, 'flags'),
    # floor and a clip to integer bounds commute, so the cell INDEX (and with it every flag) is the same either way; what
    # changes is the fraction of a point below the bound (negative instead of 0), i.e. which taps carry weight
    'clip after floor': ('cell', _cell_clip_after_floor, 'weights'),
    'idx + dx block not flagged': ('FLAGGED_CORNERS', (0, 2, 4, 6), 'flags'),
    'y/z neighbours not clamped': ('clamp', lambda i, size, axis: i if axis else np.minimum(i, size - 1), 'flags'),
    'coarse grid looked up in the fine bound': ('lookup_bound', lambda k, bound, coarse_bound: bound, 'flags'),
    'shift off by one': ('block_of', lambda idx, bv: idx >> (Y.SHIFT[bv] + 1), 'flags'),
    'group lookup using > for >=': ('group_of', lambda b, begin: int(np.searchsorted(np.asarray(begin), b, side='left')) - 1, 'moved'),
    'partial block treated as whole': ('block_voxels_of', lambda blk, V: np.arange(blk * Y.BLOCK, blk * Y.BLOCK + Y.BLOCK), 'moved'),
    'prev not updated': ('finish_prev', _finish_prev_keeps_prev, 'moved'),
}
_COLLECT = {'flags': _all_flags, 'weights': _all_weight_sets, 'moved': _all_moved}


@pytest.fixture(scope='module')
def baselines():
    return {what: fn() for what, fn in _COLLECT.items()}


@pytest.mark.parametrize('fault', list(FAULTS))
def test_the_cases_see_the_fault(fault, baselines, monkeypatch):
    attr, wrong, what = FAULTS[fault]
    assert not _differs(_COLLECT[what], baselines[what])    # the collection itself is deterministic
    monkeypatch.setattr(Y, attr, wrong)
    assert _differs(_COLLECT[what], baselines[what]), fault


def test_clip_after_floor_cannot_change_a_flag(baselines, monkeypatch):
    """documents why that fault is held by the weights: its flags are identical by construction"""
    monkeypatch.setattr(Y, 'cell', _cell_clip_after_floor)
    assert not _differs(_all_flags, baselines['flags'])
