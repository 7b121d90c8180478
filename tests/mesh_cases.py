"""Test meshes of the mesh-cleaning tests (tests/test_mesh_clean_cpu.py, tests/test_hip_mesh_clean.py): hand-built faces, the
many-component noise meshes, a long thin tube.  numpy only; the marching cubes is tests/mc_numpy.py."""
import numpy as np

from tests import mc_numpy as M

# (lattice size, seed) -> (faces, components, faces after the mask drop, components after the mask drop)
NOISE_COUNTS = {(64, 0): (131276, 5836, 95597, 6234), (96, 1): (445288, 20012, 322472, 21257)}
NOISE_SPACING = 0.05


def noise_field(n, seed, rng=None):
    """float32 [n,n,n]: white noise, lightly smoothed (two passes of the mean of each point and its six np.roll neighbours),
    the two outermost planes of every side free."""
    rng = np.random.default_rng(seed) if rng is None else rng
    v = rng.standard_normal((n, n, n)).astype(np.float32)
    for _ in range(2):
        s = v.copy()
        for axis in range(3):
            s = s + np.roll(v, 1, axis) + np.roll(v, -1, axis)
        v = s / 7
    v[:2], v[-2:], v[:, :2], v[:, -2:], v[:, :, :2], v[:, :, -2:] = -1, -1, -1, -1, -1, -1
    return v


def noise_mesh(n, seed):
    """(vertices float64 [V,3], faces int32 [F,3], vertex mask bool [V] with 35 % kept) of the level set of noise_field at its
    0.93 quantile: thousands of closed components (every edge in exactly two faces); after the mask drop 23 % of the
    edges have one face."""
    rng = np.random.default_rng(seed)
    vol = noise_field(n, seed, rng)
    level = float(np.quantile(vol, 0.93))
    v, f = M.marching_cubes(vol, level, (0., 0., 0.), (NOISE_SPACING,) * 3)
    mask = rng.random(v.shape[0]) < 0.35
    return v, f, mask


def mask_drop(faces, keep):
    """faces with at least one kept vertex (mesher.py's `faces[~(~keep)[faces].all(axis=1)]`)."""
    return faces[~(~keep)[faces].all(axis=1)]


def tube_field(n=128, turns=10, radius=0.055):
    """float32 [n,n,n]: positive inside a tube of the given radius around a helix of `turns` turns (radius 0.6, z from -0.8 to
    0.8) through the volume [-1, 1]^3 -- ONE component whose graph diameter is its whole length (the case that breaks label
    propagation).  The distance is taken to the helix point at the lattice point's own angle, turn by turn."""
    X, Y, Z, _ = M.lattice(n)
    theta = np.mod(np.arctan2(Y, X), 2 * np.pi)
    r = np.sqrt(X ** 2 + Y ** 2) - 0.6
    d2 = np.full(X.shape, np.inf)
    for k in range(turns):
        zk = -0.8 + 1.6 * (theta + 2 * np.pi * k) / (2 * np.pi * turns)
        d2 = np.minimum(d2, r ** 2 + (Z - zk) ** 2)
    return (radius - np.sqrt(d2)).astype(np.float32)


def tube_mesh(n=128, turns=10):
    return M.marching_cubes(tube_field(n, turns), 0.0, (-1., -1., -1.), (2.0 / (n - 1),) * 3)


def hand_built():
    """name -> (faces int32 [F,3], n_verts, expected labels): the adjacency rule case by case."""
    i = lambda *rows: np.asarray(rows, np.int32).reshape(-1, 3)           # noqa: E731
    return {
        'shared_edge': (i([0, 1, 2], [2, 1, 3]), 4, [0, 0]),
        'shared_vertex_only': (i([0, 1, 2], [2, 3, 4]), 5, [0, 1]),
        'three_on_one_edge': (i([0, 1, 2], [1, 0, 3], [0, 1, 4]), 5, [0, 0, 0]),
        'duplicated_face': (i([0, 1, 2], [3, 4, 5], [0, 1, 2]), 6, [0, 1, 0]),
        'single_face': (i([0, 1, 2]), 3, [0]),
        'indices_0_and_last': (i([0, 5, 9], [1, 2, 3], [9, 0, 7]), 10, [0, 1, 0]),
        'chain_joined_late': (i([0, 1, 2], [3, 4, 5], [6, 7, 8], [2, 1, 3], [3, 5, 6], [3, 1, 4]), 9, [0, 0, 2, 0, 0, 0]),
        'no_faces': (np.zeros((0, 3), np.int32), 4, []),
    }


def host_labels(faces):
    """Per face the smallest face index of its mesher.face_components class: what functional.mesh_components returns."""
    from evennicer_slam_amd.mesher import face_components
    lab, n = face_components(faces)
    first = np.full(n, len(faces), np.int64)
    np.minimum.at(first, lab, np.arange(len(faces)))
    return first[lab].astype(np.int32), n
