"""Host side of the reconstruction evaluation (evennicer_slam_amd/eval_recon.py): the PLY reader, surface sampling, the ICP,
culling and the metrics on a CPU device, and the yardsticks of tests/recon_numpy.py against each other."""
import numpy as np
import pytest
import torch

from evennicer_slam_amd import eval_recon as R
from evennicer_slam_amd import functional as EF
from evennicer_slam_amd import mesher
from tests import recon_cases as C
from tests import recon_numpy as Y


# ---- load_mesh --------------------------------------------------------------------------------------------------------------
def test_load_mesh_round_trips_write_ply(tmp_path):
    v, f = C.box_room_mesh()
    col = (np.arange(len(v) * 3) % 251).astype(np.uint8).reshape(-1, 3)
    mesher.write_ply(str(tmp_path / "m.ply"), v, f, col)
    gv, gf, gc = R.load_mesh(str(tmp_path / "m.ply"))
    assert gv.dtype == np.float64 and gf.dtype == np.int32
    assert np.array_equal(gv, v.astype(np.float32).astype(np.float64)) and np.array_equal(gf, f) and np.array_equal(gc, col)
    mesher.write_ply(str(tmp_path / "n.ply"), v, f)
    assert R.load_mesh(str(tmp_path / "n.ply"))[2] is None
    rv, rf, _ = mesher.read_ply(str(tmp_path / "n.ply"))
    assert np.array_equal(rv, gv.astype(np.float32)) and np.array_equal(rf, gf)


ASCII_PLY = """ply
format ascii 1.0
comment hand-written: normals, one quad and one triangle
element vertex 5
property float x
property float y
property float z
property float nx
property float ny
property float nz
property uchar red
property uchar green
property uchar blue
element face 2
property list uchar int vertex_indices
end_header
0 0 0 0 0 1 255 0 0
1 0 0 0 0 1 0 255 0
1 1 0 0 0 1 0 0 255
0 1 0 0 0 1 9 8 7
0.5 0.5 1.25 0 0 1 1 2 3
4 0 1 2 3
3 0 1 4
"""
WANT_V = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0], [0.5, 0.5, 1.25]], np.float64)
WANT_F = np.array([[0, 1, 2], [0, 2, 3], [0, 1, 4]], np.int32)
WANT_C = np.array([[255, 0, 0], [0, 255, 0], [0, 0, 255], [9, 8, 7], [1, 2, 3]], np.uint8)


def test_load_mesh_ascii_with_normals_and_a_quad(tmp_path):
    p = tmp_path / "a.ply"
    p.write_text(ASCII_PLY)
    v, f, c = R.load_mesh(str(p))
    assert np.array_equal(v, WANT_V) and np.array_equal(f, WANT_F) and np.array_equal(c, WANT_C)


def test_load_mesh_binary_with_normals_and_a_quad(tmp_path):
    head = "\n".join(["ply", "format binary_little_endian 1.0", "element vertex 5", "property double x", "property double y",
                      "property double z", "property float nx", "property float ny", "property float nz",
                      "element face 2", "property list uchar uint vertex_indices", "end_header"]) + "\n"
    vt = np.dtype([('p', '<f8', (3,)), ('n', '<f4', (3,))])
    rec = np.zeros(5, vt)
    rec['p'], rec['n'] = WANT_V, (0, 0, 1)
    faces = b"\x04" + np.array([0, 1, 2, 3], '<u4').tobytes() + b"\x03" + np.array([0, 1, 4], '<u4').tobytes()
    p = tmp_path / "b.ply"
    p.write_bytes(head.encode() + rec.tobytes() + faces)
    v, f, c = R.load_mesh(str(p))
    assert np.array_equal(v, WANT_V) and np.array_equal(f, WANT_F) and c is None


def test_load_mesh_rejects_what_it_cannot_read(tmp_path):
    p = tmp_path / "c.ply"
    p.write_text(ASCII_PLY.replace("4 0 1 2 3", "5 0 1 2 3 4"))
    with pytest.raises(ValueError, match="5 vertices"):
        R.load_mesh(str(p))
    p.write_text(ASCII_PLY.replace("format ascii", "format binary_big_endian"))
    with pytest.raises(ValueError, match="binary_big_endian"):
        R.load_mesh(str(p))
    p.write_text("solid\n")
    with pytest.raises(ValueError, match="not a PLY"):
        R.load_mesh(str(p))
    head = "ply\nformat binary_little_endian 1.0\nelement vertex 1\nproperty float x\nproperty float y\nproperty float z\n" \
           "element face 1\nproperty list uchar int vertex_indices\nend_header\n"
    p.write_bytes(head.encode() + np.zeros(3, '<f4').tobytes())            # ends right after the vertex block
    with pytest.raises(ValueError, match="ends inside the face data"):
        R.load_mesh(str(p))
    p.write_bytes(head.encode() + np.zeros(2, '<f4').tobytes())
    with pytest.raises(ValueError, match="ends inside the vertex data"):
        R.load_mesh(str(p))


# ---- sampling ---------------------------------------------------------------------------------------------------------------
def test_sample_surface_cpu():
    v, f = C.box_room_mesh()
    n = 200000
    pts, pick = R.sample_surface(v, f, n, seed=3, device='cpu')
    assert pts.dtype == torch.float64 and tuple(pts.shape) == (n, 3) and pts.device.type == 'cpu'
    C.check_samples(v, f, pts.numpy(), pick.numpy(), n)
    again, _ = R.sample_surface(v, f, n, seed=3, device='cpu')
    other, _ = R.sample_surface(v, f, n, seed=4, device='cpu')
    assert torch.equal(pts, again) and not torch.equal(pts, other)


# ---- ICP --------------------------------------------------------------------------------------------------------------------
def test_host_icp_recovers_a_known_motion():
    src, dst = C.icp_case()
    T, it, fit, rmse = R.align_icp(src, dst)
    Ty, ity, _, _ = Y.icp(src, dst)
    assert np.abs(Ty - C.ICP_TRUTH).max() <= 1e-9            # the yardstick itself
    assert np.abs(T - C.ICP_TRUTH).max() <= 1e-9 and it == ity and it < 30
    assert fit == 1.0 and rmse <= 1e-9


# ---- culling and metrics ----------------------------------------------------------------------------------------------------
def test_cull_mesh_cpu_matches_the_reference_loop():
    v, f = C.box_room_mesh()
    want = Y.cull_faces(v, f, C.CULL_POSES, C.CAM)
    got = R.cull_mesh(v, f, C.CULL_POSES, C.CAM, device='cpu')
    assert 0 < len(want) < len(f)
    assert np.array_equal(got, want)


def test_cull_tool_reads_a_trajectory_file(tmp_path):
    import importlib.util
    import os
    spec = importlib.util.spec_from_file_location(
        "cull_mesh_tool", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "cull_mesh.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    rows = np.arange(32, dtype=np.float64).reshape(2, 16) / 7
    (tmp_path / "traj.txt").write_text("\n".join(" ".join(repr(float(x)) for x in r) for r in rows) + "\n\n")
    poses = tool.load_poses(str(tmp_path / "traj.txt"))
    want = rows.reshape(2, 4, 4).copy()
    want[:, :3, 1] *= -1
    want[:, :3, 2] *= -1
    assert poses.dtype == np.float32 and np.array_equal(poses, want.astype(np.float32))
    (tmp_path / "one.txt").write_text(" ".join(repr(float(x)) for x in rows[0]))
    assert tool.load_poses(str(tmp_path / "one.txt")).shape == (1, 4, 4)


def test_metrics_cpu():
    v, f = C.box_room_mesh()
    m = R.calc_3d_metric((v + np.array([0.02, 0.0, 0.0]), f), (v, f), align=False, n=20000, device='cpu', return_points=True)
    rec, gt = m['rec_points'], m['gt_points']
    assert isinstance(rec, np.ndarray)
    d_acc = Y.nearest(rec[:2000], gt)[0]
    assert np.allclose(R.accuracy(gt, rec[:2000]) * 100, d_acc.mean() * 100, rtol=1e-12)
    # 20 000 samples of 64 m^2 lie about 0.5 / sqrt(313 per m^2) = 2.8 cm from their nearest neighbour, the shift adds up to 2 cm
    assert 1.0 < m['accuracy'] < 5.0 and 1.0 < m['completion'] < 5.0 and 50 < m['completion_ratio'] <= 100
    assert np.array_equal(m['transform'], np.eye(4))
    m2 = R.calc_3d_metric((v + np.array([0.02, 0.0, 0.0]), f), (v, f), align=True, n=20000, device='cpu')
    assert np.abs(m2['transform'][:3, 3] - [-0.02, 0, 0]).max() <= 1e-9 and m2['accuracy'] < m['accuracy']


def test_sample_views_cpu_rejects_views_of_the_unseen_points():
    c = np.array([-0.5, 0.3, 0.1])
    transform = np.eye(4)
    transform[:3, 3] = c
    unseen = C.box_top_points()
    c2w, stats = R.sample_views(np.zeros(3), transform, 8, unseen, cam=C.CAM, seed=C.VIEW_SEED, device='cpu')
    assert c2w.shape == (8, 4, 4) and stats['rejected'] >= 1 and stats['candidates'] == 8 + stats['rejected']
    for m in c2w:
        assert np.allclose(m[:3, 3], c) and np.allclose(m[:3, :3].T @ m[:3, :3], np.eye(3), atol=1e-12)
        assert not Y.check_proj(unseen, C.CAM, m).any()


def test_depth_tools_need_a_hip_device():
    v, f = C.box_room_mesh()
    with pytest.raises(NotImplementedError, match="needs a HIP device"):
        EF.mesh_depth(torch.from_numpy(v), torch.from_numpy(f), np.zeros((1, 3, 4)), C.CAM)
    with pytest.raises(NotImplementedError, match="needs a HIP device"):
        R.calc_2d_metric((v, f), (v, f), np.zeros((1, 3)), np.zeros(3), np.eye(4), device='cpu')


# ---- the yardsticks against each other --------------------------------------------------------------------------------------
def test_ray_caster_matches_the_analytic_room():
    room = C.room()
    v, f = C.box_room_mesh(room)
    for c2w in C.view_poses():
        depth, margin = Y.ray_cast(v, f, c2w, C.CAM)
        assert margin.min() > 1e-9 and (depth > 0).all()
        want = room.render(torch.from_numpy(c2w), C.CAM)[1].numpy()
        assert np.abs(depth - want).max() <= 5e-7


def test_brute_force_nearest_matches_ckdtree():
    from scipy.spatial import cKDTree
    rng = np.random.default_rng(0)
    ref, q = rng.normal(size=(700, 3)), rng.normal(size=(300, 3))
    d, i = Y.nearest(q, ref)
    dk, ik = cKDTree(ref).query(q)
    assert np.array_equal(i, ik) and np.allclose(d, dk, rtol=1e-12, atol=0)
