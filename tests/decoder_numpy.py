"""Float64 numpy yardstick for the NICE decoder forward (tests/test_decoder_cpu.py, tests/test_hip_decoder_fwd.py).

It restates the REFERENCE's rules, not the kernels:
  cells      common.normalize_3d_coordinate in float64, the .float() cast, then ATen's unnormalise / clip / floor in float32 and
             the eight clamped taps (tests/blocks_numpy.py: `cells`, `corners`)
  interp     the eight tap weights (wx * wy) * wz and the weighted sum in float64, from those float32 fractions
  embedding  sin(float64(float32(p)) @ float64(B))                                                (decoder.py: GaussianFourier)
  decoders   middle / fine / colour: five blocks h = relu(W h + b) + (Wc c + bc), the embedding concatenated in front after
             block 2, then the output layer; the fine decoder takes c = [c_fine, c_middle]; the coarse decoder runs on its
             features alone (no embedding, no fc_c), over the doubled bound
  stage      coarse: occ = coarse(c_coarse); middle: occ = middle; fine: occ = fine + middle; colour: rgb = colour[:, :3] and
             the fine occupancy; colour columns of the other stages are 0                          (decoder.py: NICE.forward)
  mask       Renderer.eval_points: occupancy 100 where not (p > lo and p < hi) on every axis
Parameters are the float32 values of the state dict, cast to float64; every sum is a float64 numpy sum.

`sines` (optional): {decoder name: [P, 93] array} taken in place of sin(p @ B) -- the device's own sines, to separate the
sine's share of an error from the accumulation's.

The small helpers (`TAPS`, `embedding_columns`, `fine_features`, `skip_concat`, `inside`, `rows`) exist so that
tests/test_decoder_cpu.py can state a wrong variant as a one-line replacement of one of them."""
import numpy as np

from tests import blocks_numpy as BN

F32, F64 = np.float32, np.float64
STAGES = ('coarse', 'middle', 'fine', 'color')
N_BLOCKS, SKIP = 5, 2
TAPS = tuple(range(8))


def as64(a):
    return np.asarray(a, dtype=F64)


def interp(grid, points, bound):
    """float64 [P, 32]: trilinear features of grid [1, 32, D, H, W] at float64 points [P, 3]"""
    grid = np.asarray(grid)
    dims = grid.shape[2:]
    v = BN.cells(points, bound, dims)
    idx, exists, _ = BN.corners(points, bound, dims)
    g = as64(grid).reshape(grid.shape[1], -1)
    fx, fy, fz = as64(v['fx']), as64(v['fy']), as64(v['fz'])
    out = np.zeros((idx.shape[0], grid.shape[1]), dtype=F64)
    for k in TAPS:
        dx, dy, dz = k & 1, (k >> 1) & 1, k >> 2
        w = ((fx if dx else 1.0 - fx) * (fy if dy else 1.0 - fy)) * (fz if dz else 1.0 - fz)
        out += g[:, idx[:, k]].T * np.where(exists[:, k], w, 0.0)[:, None]
    return out


def fourier_argument(points, B, dtype=F64):
    """float32(p) @ B, accumulated in `dtype`"""
    return np.asarray(points, dtype=F64).astype(F32).astype(dtype) @ np.asarray(B).astype(dtype)


def embedding_columns(emb):
    return emb


def embedding(points, B, sines=None):
    return embedding_columns(np.sin(fourier_argument(points, B)) if sines is None else as64(sines))


def linear(params, prefix, x):
    return x @ as64(params[prefix + '.weight']).T + as64(params[prefix + '.bias'])


def relu(x):
    return np.maximum(x, 0.0)


def skip_concat(emb, h):
    return np.concatenate([emb, h], axis=-1)


def fine_features(c_fine, c_middle):
    return np.concatenate([c_fine, c_middle], axis=-1)


def decode_xyz(params, name, points, c, sines=None):
    emb = embedding(points, params[name + '.embedder._B'], None if sines is None else sines.get(name))
    h = emb
    for i in range(N_BLOCKS):
        h = relu(linear(params, f'{name}.pts_linears.{i}', h)) + linear(params, f'{name}.fc_c.{i}', c)
        if i == SKIP:
            h = skip_concat(emb, h)
    return linear(params, name + '.output_linear', h)


def decode_feat(params, name, c):
    h = c
    for i in range(N_BLOCKS):
        h = relu(linear(params, f'{name}.pts_linears.{i}', h))
        if i == SKIP:
            h = skip_concat(c, h)
    return linear(params, name + '.output_linear', h)


def inside(p, lo, hi):
    return (p > lo) & (p < hi)


def inside_bound(points, bound):
    points, bound = as64(points), as64(bound)
    keep = np.ones(points.shape[0], dtype=bool)
    for a in range(3):
        keep &= inside(points[:, a], bound[a, 0], bound[a, 1])
    return keep


def rows(raw):
    return raw


def decode_stage(params, grids, points, stage, bound, coarse_enlarge=2, sines=None):
    """float64 [P, 4] = [r, g, b, occ] of the stage, unmasked"""
    points, bound = as64(points), as64(bound)
    raw = np.zeros((points.shape[0], 4), dtype=F64)
    if stage == 'coarse':
        c = interp(grids['grid_coarse'], points, bound * coarse_enlarge)
        raw[:, 3] = decode_feat(params, 'coarse_decoder', c)[:, 0]
        return rows(raw)
    c_mid = interp(grids['grid_middle'], points, bound)
    mid = decode_xyz(params, 'middle_decoder', points, c_mid, sines)[:, 0]
    if stage == 'middle':
        raw[:, 3] = mid
        return rows(raw)
    c_fine = fine_features(interp(grids['grid_fine'], points, bound), c_mid)
    raw[:, 3] = decode_xyz(params, 'fine_decoder', points, c_fine, sines)[:, 0] + mid
    if stage == 'fine':
        return rows(raw)
    c_col = interp(grids['grid_color'], points, bound)
    raw[:, :3] = decode_xyz(params, 'color_decoder', points, c_col, sines)[:, :3]
    return rows(raw)


def eval_points(params, grids, points, stage, bound, apply_mask=True, coarse_enlarge=2, sines=None):
    """float64 [P, 4]; apply_mask: occupancy 100 for the points that are not strictly inside the bound"""
    raw = decode_stage(params, grids, points, stage, bound, coarse_enlarge, sines)
    if apply_mask:
        raw[:, 3] = np.where(inside_bound(points, bound), raw[:, 3], 100.0)
    return raw
