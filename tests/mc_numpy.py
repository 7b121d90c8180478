"""numpy restatement of csrc/marching_cubes.hip (the oracle of its tests; a plain helper module, not a conftest).

Same conventions as the kernel (include/enslam_hip.h): a corner is occupied iff value > level (compared in float64), each
lattice point owns its +x / +y / +z edges, vertices in (owner point, axis) order at origin + (index + t) * spacing,
triangles in (cell, case-table) order with the table of tools/gen_mc_tables.py."""
import numpy as np

from tools import gen_mc_tables as G

_COUNT = np.array([len(t) for t in G.TRIS], dtype=np.int64)
_EDGES = np.full((256, 3 * G.MAX_TRIS), -1, dtype=np.int64)
for _c, _tris in enumerate(G.TRIS):
    _flat = [e for t in _tris for e in t]
    _EDGES[_c, :len(_flat)] = _flat
_C0 = np.array([G.EDGES[e][0] for e in range(12)], dtype=np.int64)


def marching_cubes(volume, level, origin=(0., 0., 0.), spacing=(1., 1., 1.)):
    """(verts float64 [V,3], faces int32 [F,3]) for a volume [nx, ny, nz] (evaluated as float32, z fastest)."""
    vol = np.ascontiguousarray(volume, dtype=np.float32)
    nx, ny, nz = vol.shape
    v64 = vol.astype(np.float64)
    level = float(level)
    occ = v64 > level
    origin = np.asarray(origin, dtype=np.float64)
    spacing = np.asarray(spacing, dtype=np.float64)

    # vertex masks: bit a set where the point's +a edge crosses
    crossing = []
    for a in range(3):
        m = np.zeros(vol.shape, dtype=bool)
        lo = [slice(None)] * 3
        hi = [slice(None)] * 3
        lo[a], hi[a] = slice(0, -1), slice(1, None)
        m[tuple(lo)] = occ[tuple(lo)] != occ[tuple(hi)]
        crossing.append(m.reshape(-1))
    vmask = crossing[0] * 1 + crossing[1] * 2 + crossing[2] * 4
    nv = crossing[0].astype(np.int64) + crossing[1] + crossing[2]
    vbase = np.concatenate([[0], np.cumsum(nv)[:-1]]).astype(np.int64)

    # vertices in (point, axis) order
    pts = np.nonzero(nv)[0]
    owner = np.repeat(pts, nv[pts])
    bits = np.stack(crossing, 1)[pts]                                   # [P, 3] in axis order per point
    axes = np.nonzero(bits)[1]                                          # row-major: point first, then axis
    idx = np.stack(np.unravel_index(owner, vol.shape), 1).astype(np.float64)
    strides = np.array([ny * nz, nz, 1], dtype=np.int64)
    a0 = v64.reshape(-1)[owner]
    a1 = v64.reshape(-1)[owner + strides[axes]]
    t = (level - a0) / (a1 - a0)
    frac = np.zeros_like(idx)
    frac[np.arange(len(axes)), axes] = t
    verts = origin + (idx + frac) * spacing

    # cases of the cells (lowest corner at a point with every coordinate below the last)
    cells = np.zeros(vol.shape, dtype=np.int64)
    core = occ[:-1, :-1, :-1] * 0
    for c in range(8):
        dx, dy, dz = c & 1, (c >> 1) & 1, (c >> 2) & 1
        core = core + (occ[dx:nx - 1 + dx, dy:ny - 1 + dy, dz:nz - 1 + dz].astype(np.int64) << c)
    cells[:-1, :-1, :-1] = core
    cases = cells.reshape(-1)
    nt = _COUNT[cases]
    cell_of = np.repeat(np.arange(cases.size), nt)
    k = np.arange(cell_of.size) - np.repeat(np.cumsum(nt) - nt, nt)
    cs = cases[cell_of]
    faces = np.empty((cell_of.size, 3), dtype=np.int64)
    for j in range(3):
        e = _EDGES[cs, 3 * k + j]
        c0 = _C0[e]
        q = cell_of + (c0 & 1) * strides[0] + ((c0 >> 1) & 1) * strides[1] + ((c0 >> 2) & 1)
        a = e >> 2
        below = (vmask[q] & ((1 << a) - 1))
        faces[:, j] = vbase[q] + (below & 1) + ((below >> 1) & 1)
    return verts, faces.astype(np.int32)


# ---- mesh checks shared by the CPU and GPU tests ------------------------------------------------------------------------
def edge_use(faces):
    """{(a, b): count} of directed edges."""
    f = np.asarray(faces, dtype=np.int64)
    d = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    keys, counts = np.unique(d, axis=0, return_counts=True)
    return {(int(a), int(b)): int(n) for (a, b), n in zip(keys, counts)}


def is_closed_oriented_manifold(faces):
    """Every undirected edge in exactly two faces, traversed once in each direction."""
    use = edge_use(faces)
    if any(n != 1 for n in use.values()):
        return False
    return all((b, a) in use for (a, b) in use)


def euler_characteristic(verts, faces):
    f = np.asarray(faces, dtype=np.int64)
    e = np.unique(np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), axis=1), axis=0)
    used = np.unique(f)
    return int(used.size - e.shape[0] + f.shape[0])


def signed_volume(verts, faces):
    """Divergence theorem: sum of v0 . (v1 x v2) / 6 over the triangles (positive when normals point outward)."""
    v = np.asarray(verts, dtype=np.float64)[np.asarray(faces, dtype=np.int64)]
    return float(np.einsum('ij,ij->i', v[:, 0], np.cross(v[:, 1], v[:, 2])).sum() / 6.0)


# ---- analytic test fields ----------------------------------------------------------------------------------------------
def lattice(n, lo=-1.0, hi=1.0):
    ax = np.linspace(lo, hi, n)
    X, Y, Z = np.meshgrid(ax, ax, ax, indexing='ij')
    return X, Y, Z, ax[1] - ax[0]


def sphere_field(n=48, r=0.7):
    """value = r - |p| on [-1, 1]^3: occupied inside, free space along the border."""
    X, Y, Z, h = lattice(n)
    return (r - np.sqrt(X ** 2 + Y ** 2 + Z ** 2)).astype(np.float32), h, 4.0 / 3.0 * np.pi * r ** 3


def torus_field(n=48, R=0.55, r=0.25):
    X, Y, Z, h = lattice(n)
    q = np.sqrt(X ** 2 + Y ** 2) - R
    return (r - np.sqrt(q ** 2 + Z ** 2)).astype(np.float32), h, 2.0 * np.pi ** 2 * R * r ** 2


def smooth_random_field(n, seed, pad=2):
    """Sum of random Gaussian bumps minus a constant, with `pad` planes of free space on every side."""
    rng = np.random.default_rng(seed)
    X, Y, Z, _ = lattice(n)
    v = np.full(X.shape, -0.3)
    for _ in range(12):
        c = rng.uniform(-0.7, 0.7, 3)
        s = rng.uniform(0.12, 0.35)
        v += rng.uniform(0.4, 1.0) * np.exp(-((X - c[0]) ** 2 + (Y - c[1]) ** 2 + (Z - c[2]) ** 2) / (2 * s * s))
    v = v.astype(np.float32)
    v[:pad], v[-pad:], v[:, :pad], v[:, -pad:], v[:, :, :pad], v[:, :, -pad:] = -1, -1, -1, -1, -1, -1
    return v
