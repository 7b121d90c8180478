"""The case of the TSDF tests (tests/test_tsdf_cpu.py, tests/test_hip_tsdf.py): a small analytic room seen from three
poses, fused by the numpy restatement (tests/tsdf_numpy.py).  The restated volumes are computed once per (stride, colour)
and shared; nobody modifies them.  `check_case` asserts that the inputs reach every branch of the kernels -- conditions on
the case, so no kernel test can pass by missing one."""
import functools

import numpy as np

from tests import tsdf_numpy as T

ROOM = dict(room_lo=[-0.9, -0.7, -0.5], room_hi=[1.1, 0.9, 0.8], box_lo=[0.2, -0.7, -0.4], box_hi=[0.64, 0.0, 0.0])
CAM = dict(H=30, W=40, fx=35.0, fy=35.0, cx=19.5, cy=14.5)
VOXEL, TRUNC = 0.04, 0.12
VIEWS = [dict(eye=[-0.5, 0.5, 0.1], target=[0.6, -0.5, 0.0]),
         dict(eye=[0.7, 0.6, 0.4], target=[0.3, -0.6, -0.2], up=(0.2, 0.1, 1.0)),
         dict(eye=[-0.6, -0.3, -0.2], target=[1.0, 0.2, 0.5], up=(0, 0.3, 1))]
STRIDES = (1, 4)


def room():
    from evennicer_slam_amd.synthetic import BoxRoom
    return BoxRoom(ROOM['room_lo'], ROOM['room_hi'], ROOM['box_lo'], ROOM['box_hi'])


@functools.lru_cache(maxsize=None)
def frames():
    """[(depth float32 [H,W], color float32 [H,W,3], c2w float64 [4,4])] of the three views; rows 10-12 of the second depth
    image are holes."""
    from evennicer_slam_amd.synthetic import look_at
    r = room()
    out = []
    for k, v in enumerate(VIEWS):
        c2w = look_at(**v)
        col, dep = r.render(c2w, CAM)
        dep = dep.numpy().copy()
        if k == 1:
            dep[10:13] = 0
        out.append((dep, col.float().numpy(), c2w.numpy()))
    return out


def box():
    """World corners (lo, hi) of the volume: the frames' back-projected valid pixels +- TRUNC (what for_frames computes)."""
    pts = []
    for dep, _, c2w in frames():
        j, i = np.nonzero(dep > 0)
        d = dep[j, i].astype(np.float64)
        cam = np.stack([(i - CAM['cx']) / CAM['fx'] * d, -(j - CAM['cy']) / CAM['fy'] * d, -d], 1)
        pts.append(cam @ c2w[:3, :3].T + c2w[:3, 3])
    pts = np.concatenate(pts)
    return pts.min(0) - TRUNC, pts.max(0) + TRUNC


def new_volume(stride, color, order=(0, 1, 2), upto=None):
    lo, hi = box()
    vol = T.Volume(VOXEL, TRUNC, lo, hi, CAM, color=color, stride=stride)
    for k in order[:upto]:
        dep, col, c2w = frames()[k]
        vol.integrate(dep, col if color else None, c2w)
    return vol


@functools.lru_cache(maxsize=None)
def volume(stride, color=True, upto=3):
    """The restated volume after the first `upto` frames (shared: do not modify)."""
    return new_volume(stride, color, upto=upto)


@functools.lru_cache(maxsize=None)
def mesh(stride, color=True):
    return volume(stride, color).extract_mesh()


def surface_distance(points):
    """Distance of points [P,3] to the room's surfaces (walls and box faces), float64 [P]."""
    p = np.asarray(points, np.float64)

    def to_box_shell(lo, hi):
        lo, hi = np.asarray(lo), np.asarray(hi)
        out = np.maximum(np.maximum(lo - p, p - hi), 0.0)
        d_out = np.linalg.norm(out, axis=1)
        d_in = np.minimum(p - lo, hi - p).min(axis=1)
        return np.where(d_out > 0, d_out, d_in)

    return np.minimum(to_box_shell(ROOM['room_lo'], ROOM['room_hi']), to_box_shell(ROOM['box_lo'], ROOM['box_hi']))


@functools.lru_cache(maxsize=None)
def check_case():
    """Asserts the branch coverage of the case on the restatement and returns the counts."""
    v1, v4 = volume(1), volume(4)
    out = {}
    for stride, vol in ((1, v1), (4, v4)):
        st = vol.stats
        assert tuple(vol.nu) == (4, 4, 3) and (vol.unit_lo < 0).all()
        assert st[1]['blocks'] > st[0]['blocks'] and st[2]['blocks'] > st[1]['blocks']          # frames 2 and 3 open blocks
        assert all(s['touched'] < s['blocks'] for s in st[1:])         # ... and leave earlier blocks untouched
        assert {1.0, 2.0, 3.0} <= set(np.unique(vol.weight))
        assert all(s['clipped'] > 0 and s['skipped_behind'] > 0 for s in st)
        valid, neg, cv, case = vol.cells()
        surf = cv & (case > 0) & (case < 255)
        x, y, z = np.nonzero(surf)
        straddle = (x % 16 == 15).astype(int) + (y % 16 == 15) + (z % 16 == 15)
        crossing, vertex = vol.edge_masks()
        orphan = sum(int((c & ~v).sum()) for c, v in zip(crossing, vertex))
        out[stride] = dict(blocks=st[-1]['blocks'], straddle=[int((straddle == k).sum()) for k in (1, 2, 3)], orphan_edges=orphan,
                           vertices=sum(int(v.sum()) for v in vertex))
        assert all(n > 0 for n in out[stride]['straddle']), out[stride]
        assert orphan > 0
    assert out[4]['blocks'] < out[1]['blocks']
    return out
