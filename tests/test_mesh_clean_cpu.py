"""Mesh cleaning, the part that needs no GPU: the new entry points are declared, exported and bound; the test meshes of
tests/test_hip_mesh_clean.py (tests/mesh_cases.py) are the multi-component ones they are meant to be."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import mesh_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ('enslam_mesh_clean_workspace', 'enslam_mesh_components', 'enslam_mesh_clean_count', 'enslam_mesh_clean_emit')


def test_mesh_clean_exports_in_header_library_and_binding():
    import evennicer_slam_amd as E
    from evennicer_slam_amd import functional as EF
    header = open(os.path.join(ROOT, "include", "enslam_hip.h")).read()
    handle = ctypes.CDLL(E.LIB_PATH)
    for n in ENTRIES:
        assert re.search(r"\b" + n + r"\s*\(", header), n
        assert n in E._lib.EXPORTS, n
        assert hasattr(handle, n), n
    assert callable(EF.mesh_components) and callable(EF.mesh_clean)


def test_mesh_clean_size_checks_run_on_the_host():
    """The workspace query is host arithmetic: sizes, the refusal beyond the stated limits, the NULL check."""
    import evennicer_slam_amd as E
    lib = E._lib.lib()
    nb = ctypes.c_int64()
    assert lib.enslam_mesh_clean_workspace(10, 10, None) == -1
    assert lib.enslam_mesh_clean_workspace(-1, 10, ctypes.byref(nb)) == -1
    assert lib.enslam_mesh_clean_workspace(10, -1, ctypes.byref(nb)) == -1
    assert lib.enslam_mesh_clean_workspace(10, (1 << 24) + 1, ctypes.byref(nb)) == -3
    assert lib.enslam_mesh_clean_workspace((1 << 26) + 1, 10, ctypes.byref(nb)) == -3
    assert lib.enslam_mesh_clean_workspace(0, 0, ctypes.byref(nb)) == 0 and nb.value > 0
    assert lib.enslam_mesh_clean_workspace(1 << 24, 1 << 24, ctypes.byref(nb)) == 0
    big = nb.value
    assert lib.enslam_mesh_clean_workspace(800_000, 1_500_000, ctypes.byref(nb)) == 0
    print(f"workspace: {nb.value / 2**20:.0f} MiB at 1.5 M faces, {big / 2**20:.0f} MiB at the limit")
    assert nb.value < 512 * 2**20            # room0 at 256^3 stays far below the 2 GiB the mesher test allows


def test_functional_refuses_host_tensors():
    import torch
    from evennicer_slam_amd import EnslamError
    from evennicer_slam_amd import functional as EF
    f = torch.zeros((2, 3), dtype=torch.int32)
    v = torch.zeros((4, 3), dtype=torch.float64)
    with pytest.raises(EnslamError):
        EF.mesh_components(f, 4)
    with pytest.raises(EnslamError):
        EF.mesh_clean(v, f)


def test_mesher_keeps_its_constructor_and_gains_the_host_switch():
    import inspect
    import types
    from evennicer_slam_amd.mesher import MESHING_DEFAULTS, Mesher
    assert list(inspect.signature(Mesher.__init__).parameters) == ['self', 'cfg', 'args', 'slam', 'points_batch_size', 'ray_batch_size']
    cfg = dict(coarse=False, scale=1, occupancy=True, meshing=dict(MESHING_DEFAULTS), mapping=dict(marching_cubes_bound=[[0, 1]] * 3))
    slam = types.SimpleNamespace(renderer=None, bound=None, nice=True, verbose=False, H=4, W=4, fx=1., fy=1., cx=2., cy=2.)
    m = Mesher(cfg, None, slam)
    assert m.clean_on_host is False                     # the device route is the default on a HIP device


@pytest.mark.parametrize("name", sorted(C.hand_built()))
def test_hand_built_labels_are_the_host_partition(name):
    faces, n_verts, want = C.hand_built()[name]
    assert faces.max(initial=-1) < n_verts
    lab, n = C.host_labels(faces)
    assert lab.tolist() == want and n == len(set(want))


@pytest.mark.parametrize("n,seed", sorted(C.NOISE_COUNTS))
def test_noise_meshes_have_the_quoted_components(n, seed):
    from evennicer_slam_amd.mesher import face_components
    F, comps, F_masked, comps_masked = C.NOISE_COUNTS[(n, seed)]
    v, f, mask = C.noise_mesh(n, seed)
    assert len(f) == F and face_components(f)[1] == comps
    e = np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), axis=1)
    assert (np.unique(e, axis=0, return_counts=True)[1] == 2).all()          # closed: every edge in exactly two faces
    fm = C.mask_drop(f, mask)
    assert len(fm) == F_masked and face_components(fm)[1] == comps_masked
    e = np.sort(np.concatenate([fm[:, [0, 1]], fm[:, [1, 2]], fm[:, [2, 0]]]), axis=1)
    one = (np.unique(e, axis=0, return_counts=True)[1] == 1).mean()
    assert 0.2 < one < 0.3                                                   # boundary edges after the drop


def test_tube_is_one_long_component():
    from evennicer_slam_amd.mesher import face_components
    v, f = C.tube_mesh()
    assert len(f) > 20_000 and face_components(f)[1] == 1
    # ten turns: the surface passes through every octant sector of the helix many times over
    ang = np.arctan2(v[:, 1], v[:, 0])
    z = v[:, 2]
    assert z.max() - z.min() > 1.5 and np.unique(np.floor((ang + np.pi) / (np.pi / 4)).astype(int)).size == 8
