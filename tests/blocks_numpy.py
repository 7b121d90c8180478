"""Numpy yardstick for the block flags and the block-sparse grid movement (tests/test_blocks_cpu.py, tests/test_hip_blocks.py).

It restates the REFERENCE, operation for operation, not the kernels:
  points   Renderer.render_batch_ray: pts = rays_o + rays_d * z_vals in float64
  cells    common.normalize_3d_coordinate in float64, the .float() cast, then ATen's grid_sampler_unnormalize /
           clip_coordinates / floor (align_corners=True, padding_mode='border') in float32
  corners  ATen's eight taps tnw, tne, tsw, tse, bnw, bne, bsw, bse (k = 4 dz + 2 dy + dx) with weight (wx * wy) * wz; a tap
           beyond the last voxel does not exist for ATen (it is skipped) -- the kernels load it from the clamped index with
           weight 0, so its block must be flagged as well
Every float64 and float32 operation is one numpy operation of that dtype (the library is built with -ffp-contract=off).

The movement functions are pure: they copy their arguments and return EVERY array the kernel may write, so a caller can assert
what was left untouched.  Dense grids are [32, V] (the reference's [1, 32, D, H, W] flattened), voxel-major ones [V, 32]; a
launch over several grids numbers its 64-voxel blocks through all grids, grid after grid (`launch_blocks`).

The small helpers (`cast32`, `clip`, `clamp`, `lookup_bound`, `block_of`, `group_of`, `block_voxels_of`, `FLAGGED_CORNERS`) exist
so that tests/test_blocks_cpu.py can state a wrong variant as a one-line replacement of one of them."""
import numpy as np

F32, F64 = np.float32, np.float64
C = 32                                   # channels of a feature grid
BLOCK = 64                               # voxels per block of the movement kernels
BLOCK_SIZES = (64, 32, 16, 8)
SHIFT = {64: 6, 32: 5, 16: 4, 8: 3}
STAGES = ('coarse', 'middle', 'fine', 'color')
FLAGGED_CORNERS = tuple(range(8))        # all eight taps, zero-weight ones included: the gather loads them


def stage_grids(stage):
    """grids (0 coarse, 1 middle, 2 fine, 3 colour) that NICE.forward reads in a stage"""
    return {'coarse': (0,), 'middle': (1,), 'fine': (1, 2), 'color': (1, 2, 3)}[stage]


def lookup_bound(k, bound, coarse_bound):
    """the coarse grid lives over the enlarged bound, the others over the scene bound"""
    return coarse_bound if k == 0 else bound


# ------------------------------------------------------------------------------------------------ points, cells, corners
def sample_points(ro, rd, z):
    """float64 [N*S, 3]: rays_o[..., None, :] + rays_d[..., None, :] * z_vals[..., :, None]"""
    ro, rd, z = np.asarray(ro), np.asarray(rd), np.asarray(z)
    assert ro.dtype == F32 and rd.dtype == F32 and z.dtype == F64
    pw = ro.astype(F64)[:, None, :] + rd.astype(F64)[:, None, :] * z[:, :, None]
    return pw.reshape(-1, 3)


def cast32(a):
    return a.astype(F32)


def normalise(p, lo, hi):
    """float64 ((p - lo) / (hi - lo)) * 2 - 1, then .float()"""
    p = np.asarray(p, dtype=F64)
    lo, hi = F64(lo), F64(hi)
    return cast32(((p - lo) / (hi - lo)) * F64(2.0) - F64(1.0))


def unnormalise(pn, size):
    """float32 ((pn + 1) / 2) * (size - 1)"""
    return ((pn + F32(1.0)) / F32(2.0)) * F32(size - 1)


def clip(c, size):
    """clip_coordinates: min(size - 1, max(c, 0))"""
    return np.minimum(np.maximum(c, F32(0.0)), F32(size - 1))


def cell(pn, size):
    """(index int32, fraction, clipped coordinate) of one axis"""
    c = clip(unnormalise(pn, size), size)
    fl = np.floor(c)
    return fl.astype(np.int32), c - fl, c


def cells(points, bound, dims):
    """dict ix, iy, iz (int32), fx, fy, fz (float32), cx, cy, cz (the clipped float32 coordinates) of float64 points [P, 3] in
    a grid of dims (D, H, W) over bound [3, 2]: x runs along W, y along H, z along D"""
    points = np.asarray(points, dtype=F64)
    bound = np.asarray(bound, dtype=F64)
    D, H, W = (int(v) for v in dims)
    out = {}
    for a, size, name in ((0, W, 'x'), (1, H, 'y'), (2, D, 'z')):
        pn = normalise(points[:, a], bound[a, 0], bound[a, 1])
        out['i' + name], out['f' + name], out['c' + name] = cell(pn, size)
    return out


def clamp(i, size, axis):
    """index of a +1 neighbour, kept inside the grid (axis 0 x, 1 y, 2 z)"""
    return np.minimum(i, size - 1)


def corners(points, bound, dims):
    """(idx int64 [P, 8] clamped linear index, exists bool [P, 8], weight float32 [P, 8]) of the eight taps"""
    D, H, W = (int(v) for v in dims)
    v = cells(points, bound, dims)
    ix, iy, iz = (v[k].astype(np.int64) for k in ('ix', 'iy', 'iz'))
    one = F32(1.0)
    P = ix.shape[0]
    idx = np.empty((P, 8), dtype=np.int64)
    exists = np.empty((P, 8), dtype=bool)
    weight = np.empty((P, 8), dtype=F32)
    for k in range(8):
        dx, dy, dz = k & 1, (k >> 1) & 1, k >> 2
        x, y, z = ix + dx, iy + dy, iz + dz
        exists[:, k] = (x < W) & (y < H) & (z < D)
        x, y, z = clamp(x, W, 0), clamp(y, H, 1), clamp(z, D, 2)
        wx = v['fx'] if dx else one - v['fx']
        wy = v['fy'] if dy else one - v['fy']
        wz = v['fz'] if dz else one - v['fz']
        weight[:, k] = np.where(exists[:, k], (wx * wy) * wz, F32(0.0))
        idx[:, k] = (z * H + y) * W + x
    return idx, exists, weight


def n_blocks(n_voxels, block_voxels=BLOCK):
    return (int(n_voxels) + block_voxels - 1) // block_voxels


def block_of(idx, block_voxels):
    return idx >> SHIFT[block_voxels]


def block_flags(points, bound, dims, block_voxels, flags=None):
    """uint8 [ceil(V / block_voxels)]: 1 for every block that holds one of the eight clamped taps of a point.  Marking only
    ever sets: `flags` (optional) are the flags before the call."""
    D, H, W = (int(v) for v in dims)
    out = np.zeros(n_blocks(D * H * W, block_voxels), dtype=np.uint8) if flags is None else np.array(flags, dtype=np.uint8)
    if len(points):
        idx, _, _ = corners(points, bound, dims)
        out[np.unique(block_of(idx[:, list(FLAGGED_CORNERS)], block_voxels))] = 1
    return out


def corner_voxels(points, bound, dims, nonzero_only=False):
    """bool [V]: the voxels that are a tap of some point (nonzero_only: a tap that exists and has a non-zero weight)"""
    D, H, W = (int(v) for v in dims)
    out = np.zeros(D * H * W, dtype=bool)
    if len(points):
        idx, exists, weight = corners(points, bound, dims)
        out[np.unique(idx[exists & (weight != 0)] if nonzero_only else idx)] = True
    return out


def scene_flags(points, stage, bound, coarse_bound, dims, block_voxels, flags=None):
    """{k: flags} for all four grids of a scene (dims: {k: (D, H, W)}): the stage's grids are marked, the others keep what they
    held (`flags`: {k: flags before the call}; missing: zeros)"""
    out = {}
    for k, d in dims.items():
        before = None if flags is None else flags.get(k)
        if k in stage_grids(stage):
            out[k] = block_flags(points, lookup_bound(k, bound, coarse_bound), d, block_voxels, before)
        else:
            out[k] = np.zeros(n_blocks(int(np.prod(d)), block_voxels), np.uint8) if before is None else np.array(before, np.uint8)
    return out


def coarsen(flags, block_voxels, n_voxels):
    """flags per `block_voxels` voxels -> flags per 64 voxels (a 64-voxel block is touched iff one of its parts is)"""
    r = BLOCK // block_voxels
    pad = np.zeros(n_blocks(n_voxels) * r, dtype=np.uint8)
    pad[:len(flags)] = flags
    return pad.reshape(-1, r).max(axis=1)


# ------------------------------------------------------------------------------------------------ movement
def to_voxel_major(dense):
    """[32, V] -> [V, 32]"""
    return np.ascontiguousarray(np.asarray(dense).T)


def from_voxel_major(vm):
    """[V, 32] -> [32, V]"""
    return np.ascontiguousarray(np.asarray(vm).T)


def group_of(b, begin):
    """grid of launch block b: the last grid whose first block is <= b (begin: first block of each grid, ascending)"""
    return int(np.searchsorted(np.asarray(begin), b, side='right')) - 1


def launch_blocks(n_voxels):
    """[(grid, block in grid)] for every block of a launch over grids of n_voxels[i] voxels, in launch order"""
    counts = [n_blocks(v) for v in n_voxels]
    begin = np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(np.int64) if counts else np.zeros(0, np.int64)
    out = []
    for b in range(int(sum(counts))):
        g = group_of(b, begin)
        out.append((g, b - int(begin[g])))
    return out


def block_voxels_of(blk, n_voxels):
    """voxel indices of 64-voxel block blk of a grid: the last block of a grid may be partial"""
    return np.arange(blk * BLOCK, min(blk * BLOCK + BLOCK, n_voxels))


def _copies(arrays):
    return [None if a is None else np.array(a) for a in arrays]


def convert_sparse_to_vm(src, dst, need, valid=None):
    """dense src[i] [32, V_i] -> voxel-major dst[i] [V_i, 32] for the blocks with need and not valid; valid (optional, per grid
    optional) is set for them.  Returns (dst, valid)."""
    dst = _copies(dst)
    valid = [None] * len(src) if valid is None else _copies(valid)
    for g, blk in launch_blocks([s.shape[1] for s in src]):
        if not need[g][blk] or (valid[g] is not None and valid[g][blk]):
            continue
        v = block_voxels_of(blk, src[g].shape[1])
        dst[g][v, :] = src[g][:, v].T
        if valid[g] is not None:
            valid[g][blk] = 1
    return dst, valid


def zero_blocks(dst, need, flat=None, n_flat=0):
    """zero-fills the flagged blocks (need[i] None: all blocks) of voxel-major dst[i] and flat[:n_flat].  Returns (dst, flat)."""
    dst = _copies(dst)
    for g, blk in launch_blocks([d.shape[0] for d in dst]):
        if need is not None and need[g] is not None and not need[g][blk]:
            continue
        dst[g][block_voxels_of(blk, dst[g].shape[0]), :] = 0
    if flat is not None:
        flat = np.array(flat)
        flat[:n_flat] = 0
    return dst, flat


def finish(src, dst, need):
    """gradient direction: flagged blocks of voxel-major src[i] are transposed back into dense dst[i], unflagged blocks of dst[i]
    are zero-filled.  Returns dst."""
    dst = _copies(dst)
    for g, blk in launch_blocks([s.shape[0] for s in src]):
        v = block_voxels_of(blk, src[g].shape[0])
        dst[g][:, v] = src[g][v, :].T if need[g][blk] else 0
    return dst


def finish_prev(src, dst, need, prev):
    """`finish` into persistent destinations: a block untouched now (need 0) and untouched by the previous call (prev 0) is
    skipped; the others are written as in `finish`; prev takes need and the need flags that were served are cleared.
    Returns (dst, need, prev)."""
    dst, need, prev = _copies(dst), _copies(need), _copies(prev)
    for g, blk in launch_blocks([s.shape[0] for s in src]):
        needed, was = bool(need[g][blk]), bool(prev[g][blk])
        if not needed and not was:
            continue
        v = block_voxels_of(blk, src[g].shape[0])
        dst[g][:, v] = src[g][v, :].T if needed else 0
        prev[g][blk] = 1 if needed else 0
        need[g][blk] = 0
    return dst, need, prev


def move_flags(need, prev, n_move):
    """the flag hand-over of gradients in the kernels' own layout: prev[:n] = need[:n]; need[:n] = 0.  Returns (need, prev)."""
    need, prev = np.array(need), np.array(prev)
    prev[:n_move] = need[:n_move]
    need[:n_move] = 0
    return need, prev
