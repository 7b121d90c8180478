"""Seeded inputs of the scene-rasteriser tests (tests/test_viz_cpu.py, tests/test_hip_viz.py) at the smallest shapes that
reach every route of csrc/scene_raster.hip: a 45 x 61 image (odd, below one workgroup row), three views, a box room seen
from inside, a triangle soup of about 200 faces and about 300 points.  The seeds were chosen on the CPU so that the
yardstick's own margins (tests/viz_numpy.py) clear MARGINS in every view: no pixel has to be excused."""
import functools
import importlib.util
import os

import numpy as np
import torch

from tests import recon_cases as RC
from tests import viz_numpy as Y

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAM = dict(H=45, W=61, fx=47.0, fy=47.0, cx=29.7, cy=22.3)
K = 3
# edges and point squares > 1e-9, relative depth gap > 1e-5, rounding > 1e-6 of a level
MARGINS = dict(edge=1e-9, point=1e-9, gap=1e-5, round=1e-6)
SOUP_SEED, POINT_SEED, ROOM_SEED = 0, 0, 1
SOUP_FACES = 200


def w2c_of(c2w):
    return np.stack([np.linalg.inv(m)[:3] for m in np.asarray(c2w, np.float64).reshape(-1, 4, 4)])


def tiny_workspace(n_views=K, cam=CAM):
    """bytes of a workspace whose list of large triangles has one entry"""
    return 256 + (8 * n_views * cam['H'] * cam['W'] + 255) // 256 * 256 + 8


def soup_views():
    """float64 [3,3,4] world-to-camera matrices: the identity (the soup is laid out in its camera space) and two cameras
    turned and moved a little"""
    return w2c_of([np.eye(4), RC.rigid(7.0, (0.2, 1, 0.1), (0.3, -0.1, 0.2)), RC.rigid(-11.0, (1, 0.3, -0.2), (-0.2, 0.15, -0.3))])


def soup_mesh(seed=SOUP_SEED, n=SOUP_FACES):
    """(vertices float64 [3n+3,3], faces int32 [n+4,3], colours uint8 [3n+3,3]): recon_cases.triangle_soup (centres in [-4,4]
    x [-3,3] x [-9,1.5], the first four triangles of scale 4, a degenerate one at the end), then copies of faces 0 and 1 (the
    id tie) and a face with an index outside the vertices"""
    v, f = RC.triangle_soup(seed, n)
    f = np.concatenate([f, f[0:1], f[1:2], [[0, 1, len(v) + 5]]]).astype(np.int32)
    col = np.random.default_rng(seed + 100).integers(0, 256, (len(v), 3)).astype(np.uint8)
    return v, f, col


DUPLICATES = ((0, SOUP_FACES + 1), (1, SOUP_FACES + 2))     # (face, its copy)
DEGENERATE, OUT_OF_RANGE = SOUP_FACES, SOUP_FACES + 3
BORDER_UW = ((-0.4, 20.2), (60.4, 11.3), (33.6, -0.3), (14.7, 44.6))        # (u, w) of the points on the four borders


def soup_points(seed=POINT_SEED, n=290):
    """(points float64 [n+10,3], colours uint8 [n+10,3]) in the camera space of view 0: uniform in [-4,4] x [-3,3] with depths
    in [-2, 10] (some behind the camera), then four points at depth 2 whose squares straddle the four image borders, three
    beyond z_far = 1000 and three behind the camera"""
    rng = np.random.default_rng(seed)
    p = rng.uniform([-4, -3, -10], [4, 3, 2], (n, 3))
    border = [((u - CAM['cx']) / CAM['fx'] * 2.0, -(w - CAM['cy']) / CAM['fy'] * 2.0, -2.0) for u, w in BORDER_UW]
    far = rng.uniform([-1, -1, -1500], [1, 1, -1100], (3, 3))
    behind = rng.uniform([-1, -1, 0.5], [1, 1, 3], (3, 3))
    p = np.concatenate([p, border, far, behind])
    return p, rng.integers(0, 256, (len(p), 3)).astype(np.uint8)


def room_mesh(seed=ROOM_SEED, box=False):
    """(vertices, faces int32, colours uint8): the six walls of recon_cases.box_room_mesh (8 vertices, 12 faces; with `box` also
    the box that stands in the room: 16 and 24) with every face reversed, so that the stored normals point away from a camera
    inside the room: culling 1 shows the walls, culling 2 nothing of them (of the box it shows the far sides)"""
    v, f = RC.box_room_mesh()
    if not box:
        v, f = v[:8], f[:12]
    col = np.random.default_rng(seed).integers(40, 256, (len(v), 3)).astype(np.uint8)
    return v, np.ascontiguousarray(f[:, ::-1]), col


def room_views():
    return w2c_of(RC.view_poses())


def box_pixels(v, f, m, cam):
    """per face: -1 when a vertex is at or behind the camera plane (the kernel takes the whole image), else the pixel count
    of the box of the projected vertices clipped to the image"""
    out = []
    for a, b, c in f:
        if max(a, b, c) >= len(v):
            out.append(0)
            continue
        p = Y.to_camera(m, v[[a, b, c]])
        if (-p[:, 2]).min() <= 0:
            out.append(-1)
            continue
        u, w = cam['cx'] + cam['fx'] * (p[:, 0] / -p[:, 2]), cam['cy'] - cam['fy'] * (p[:, 1] / -p[:, 2])
        i0, i1 = max(np.floor(u.min() - 1e-3), 0), min(np.ceil(u.max() + 1e-3), cam['W'] - 1)
        j0, j1 = max(np.floor(w.min() - 1e-3), 0), min(np.ceil(w.max() + 1e-3), cam['H'] - 1)
        out.append(int(max(i1 - i0 + 1, 0) * max(j1 - j0 + 1, 0)))
    return np.array(out)


def _freeze(r):
    for a in r.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return r


# name -> the arguments of viz_numpy.raster / functional.scene_raster beyond the mesh, the views and the camera
def _cases():
    sv, sf, sc = soup_mesh()
    sn = Y.vertex_normals(sv, sf)
    pp, pc = soup_points()
    rv, rf, rc = room_mesh()
    rn = Y.vertex_normals(rv, rf)
    soup = dict(vertices=sv, faces=sf, colors=sc, normals=sn, views=soup_views())
    room = dict(vertices=rv, faces=rf, colors=rc, normals=rn, views=room_views())
    bv, bf, bc = room_mesh(box=True)
    return {
        'room_cull1': dict(room, cull=1),
        'room_cull2': dict(room, cull=2),
        'room_cull0_plain': dict(room, cull=0, colors=None, normals=None),
        'roombox_cull1': dict(vertices=bv, faces=bf, colors=bc, normals=Y.vertex_normals(bv, bf), views=room_views(), cull=1),
        'soup_points4': dict(soup, cull=0, points=pp, point_colors=pc, point_size=4),
        'soup_points1': dict(soup, cull=1, points=pp, point_colors=pc, point_size=1),
        'soup_cull2': dict(soup, cull=2, normals=None, ambient=0.2, background=(10, 20, 30)),
        'points_only': dict(vertices=sv[:0], faces=sf[:0], views=soup_views(), points=pp, point_colors=pc, point_size=4),
    }


NAMES = ('room_cull1', 'room_cull2', 'room_cull0_plain', 'roombox_cull1', 'soup_points4', 'soup_points1', 'soup_cull2', 'points_only')


@functools.lru_cache(maxsize=None)
def case(name):
    """(arguments dict, [yardstick result per view]); computed once, read-only"""
    args = _cases()[name]
    kw = {k: v for k, v in args.items() if k not in ('vertices', 'faces', 'views')}
    want = [_freeze(Y.raster(args['vertices'], args['faces'], m, CAM, **kw)) for m in args['views']]
    for a in args.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return args, want


def check_margins(name):
    _, want = case(name)
    for k, r in enumerate(want):
        for what, bound in MARGINS.items():
            assert r[what] > bound, f"{name} view {k}: the yardstick's own {what} margin is {r[what]:.3e}"


def load_visualizer():
    """tools/visualizer.py as a module"""
    spec = importlib.util.spec_from_file_location("tools_visualizer", os.path.join(ROOT, "tools", "visualizer.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def write_run(folder, est, gt, idx, scale, meshes=()):
    """a run's output folder: config.yaml, ckpts/{idx:05d}.tar in the reference's format and (name, bytes) mesh files"""
    os.makedirs(folder / 'ckpts')
    os.makedirs(folder / 'mesh')
    (folder / 'config.yaml').write_text(f"scale: {scale}\ndata:\n  output: {folder}\n")
    for old in (0, idx):                                                    # the newest checkpoint is the one that counts
        torch.save({'estimate_c2w_list': torch.from_numpy(est * (1 if old else 0)), 'gt_c2w_list': torch.from_numpy(gt),
                    'idx': old}, folder / 'ckpts' / f'{old:05d}.tar', _use_new_zipfile_serialization=False)
    for name, data in meshes:
        (folder / 'mesh' / name).write_bytes(data)
    return str(folder / 'config.yaml')
