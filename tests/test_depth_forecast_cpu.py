"""No GPU: the depth forecast (enslam_depth_forecast, functional.depth_forecast).

The yardstick (tests/depth_forecast_numpy.py, one source pixel at a time in Python floats) on hand-worked pixels, on the identity
and on a plane with a closed form; the numpy route of functional.depth_forecast (CPU tensors) against it on every case of
tests/depth_forecast_cases.py -- EQUAL bits; every refusal of the wrapper; the entry in header, binding and Makefile."""
import os

import numpy as np
import pytest
import torch

from tests import depth_forecast_cases as C
from tests import depth_forecast_numpy as Y

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def numpy_route(case, fill):
    from evennicer_slam_amd import functional as EF
    out = EF.depth_forecast(torch.from_numpy(case['depth'].copy()), case['cam'], case['M'], case['size'], radius=case['radius'],
                            z_near=case['z_near'], fill=bool(fill))
    assert out.dtype == torch.float32 and tuple(out.shape) == tuple(case['size'])
    return out.numpy()


def test_hand_worked_plane_5x7():
    """Plane at depth 2, camera 1 closer, principal point (3, 2), f = 4: source (j, i) lands on (2 j - 2, 2 i - 3) at depth 1.
    Rows 1, 2, 3 -> 0, 2, 4 and columns 2, 3, 4 -> 1, 3, 5 stay inside the 5 x 7 image."""
    c = C.BY_NAME['5x7_plane']
    want = np.zeros((5, 7), dtype=np.float32)
    for jo in (0, 2, 4):
        for io in (1, 3, 5):
            want[jo, io] = 1.0
    assert np.array_equal(bits(C.expected(c, 0)), bits(want))
    # fill: every empty pixel (columns 0, 2, 4, 6 and rows 1, 3) touches a voted one
    assert np.array_equal(bits(C.expected(c, 1)), bits(np.ones((5, 7), dtype=np.float32)))
    u, v, z = Y.project(2.0, 1, 4, c['cam'], c['M'], 0.0)
    assert (u, v, float(z)) == (5.0, 0.0, 1.0)


def test_hand_worked_plane_5x7_to_3x4():
    """The same points onto 3 x 4: spacings sx = 6 / 3 = 2, sy = 4 / 2 = 2, radius 1.  Landing columns u = -3 .. 9 step 2 are odd:
    u / 2 + 0.5 is an integer, io = (u + 1) / 2 and |u - 2 io| = 1 <= radius.  u = 1, 3, 5 -> io = 1, 2, 3 (u = -1 -> io = 0 too);
    rows v = 0, 2, 4 -> jo = 0, 1, 2 exactly."""
    c = C.BY_NAME['5x7_to_3x4']
    want = np.ones((3, 4), dtype=np.float32)
    assert np.array_equal(bits(C.expected(c, 0)), bits(want))
    votes = C.case_votes(c)
    assert sorted(votes) == [(jo, io) for jo in range(3) for io in range(4)]
    assert all(len(z) == 1 for z in votes.values())


def test_hand_worked_single_pixel_and_row():
    c = C.BY_NAME['1x1']
    assert float(C.expected(c, 0)[0, 0]) == 0.75                    # 1.25 deep, the camera moved 0.5 forward (down -z)
    c = C.BY_NAME['5x7_to_1x4']
    votes = C.case_votes(c)
    assert votes and all(jo == 0 for (jo, _io) in votes)            # Ho = 1 stands for full-resolution row 0


def test_occlusion_winner_and_filled_hole():
    """Near band (depth 1, columns 20..39) and far surface (depth 3), camera 0.1 to the right, f = 50: the band moves 5 columns
    left onto 15..34, far columns i land on i - 5/3.  Column 16 receives the band's column 21 and the far column 18 (16.33, within
    the radius 0.5): the band wins.  Columns 35, 36, 37 receive nothing (far column 40 lands on 38.33); with the fill, 35 takes
    the band's 1 (its only voted neighbours are in column 34), 37 the far surface's 3 (column 38), 36 stays empty."""
    c = C.BY_NAME['45x61_occlusion']
    votes = C.case_votes(c)
    assert sorted(float(z) for z in votes[(10, 16)]) == [1.0, 3.0]
    a, b = C.expected(c, 0), C.expected(c, 1)
    assert a[10, 16] == 1.0 and a[10, 34] == 1.0 and a[10, 38] == 3.0
    assert (a[10, 35], a[10, 36], a[10, 37]) == (0.0, 0.0, 0.0)
    assert (b[10, 35], b[10, 36], b[10, 37]) == (1.0, 0.0, 3.0)
    assert np.array_equal(bits(a)[a != 0], bits(b)[a != 0])          # the fill changes no voted pixel


def test_identity_returns_the_input_bit_for_bit():
    for name in ('45x61_identity', '1x300_identity'):
        c = C.BY_NAME[name]
        d = c['depth']
        valid = np.isfinite(d) & (d > 0)
        want = np.where(valid, d, np.float32(0.0)).astype(np.float32)
        assert np.array_equal(bits(C.expected(c, 0)), bits(want)), name
        assert np.array_equal(bits(numpy_route(c, 0)), bits(want)), name


def test_plane_towards_closed_form():
    """Plane at depth 3, camera 0.7 closer: every vote is float32(3 - 0.7), and source (j, i) lands on the principal point plus
    (i - cx, j - cy) * 3 / 2.3.  The voted set is the set of rounded landing positions that pass the radius test."""
    c = C.BY_NAME['45x61_plane_towards']
    img = C.expected(c, 0)
    z = np.float32(3.0 - 0.7)
    assert set(np.unique(img).tolist()) == {0.0, float(z)}
    s = 3.0 / (3.0 - 0.7)
    cols = {round(30 + (i - 30) * s) for i in range(61) if abs(30 + (i - 30) * s - round(30 + (i - 30) * s)) < 0.49}
    rows = {round(22 + (j - 22) * s) for j in range(45) if abs(22 + (j - 22) * s - round(22 + (j - 22) * s)) < 0.49}
    cols, rows = {x for x in cols if 0 <= x <= 60}, {y for y in rows if 0 <= y <= 44}
    got = {(int(j), int(i)) for j, i in zip(*np.nonzero(img))}
    assert got == {(j, i) for j in rows for i in cols}


@pytest.mark.parametrize('fill', C.FILLS)
@pytest.mark.parametrize('case', C.CASES, ids=[c['name'] for c in C.CASES])
def test_numpy_route_equals_the_yardstick(case, fill):
    assert np.array_equal(bits(numpy_route(case, fill)), bits(C.expected(case, fill)))


def test_refusals():
    from evennicer_slam_amd import functional as EF
    from evennicer_slam_amd._lib import EnslamError
    c = C.BY_NAME['5x7_plane']
    d = torch.from_numpy(c['depth'].copy())
    ok = dict(radius=1.0, z_near=0.0, fill=True)
    EF.depth_forecast(d, c['cam'], c['M'], (5, 7), **ok)
    with pytest.raises(EnslamError):
        EF.depth_forecast(d.double(), c['cam'], c['M'], (5, 7), **ok)                # wrong dtype
    with pytest.raises(EnslamError):
        EF.depth_forecast(d.t(), c['cam'], c['M'], (5, 7), **ok)                     # not contiguous
    with pytest.raises(EnslamError):
        EF.depth_forecast(d[None], c['cam'], c['M'], (5, 7), **ok)                   # not [H,W]
    for size in ((0, 7), (5, 0), (-1, 3)):
        with pytest.raises(EnslamError):
            EF.depth_forecast(d, c['cam'], c['M'], size, **ok)
    with pytest.raises(EnslamError):
        EF.depth_forecast(d, c['cam'], c['M'], (5, 7), radius=-0.5)
    with pytest.raises(EnslamError):
        EF.depth_forecast(d, c['cam'], c['M'], (5, 7), z_near=-1.0)
    with pytest.raises(EnslamError):
        EF.depth_forecast(d, c['cam'], c['M'], (5, 7), radius=float('nan'))
    with pytest.raises(EnslamError):
        EF.depth_forecast(d, c['cam'], np.zeros((3, 3)), (5, 7), **ok)
    bad = c['M'].copy()
    bad[1, 2] = np.inf
    with pytest.raises(EnslamError):
        EF.depth_forecast(d, c['cam'], bad, (5, 7), **ok)
    with pytest.raises(EnslamError):
        EF.depth_forecast(d, dict(c['cam'], fx=0.0), c['M'], (5, 7), **ok)
    with pytest.raises(EnslamError):
        EF.depth_forecast(d[:1].contiguous(), c['cam'], c['M'], (3, 7), **ok)        # one source row onto three


def check_refusals(depth, ws, out):
    """Every refusal of enslam_depth_forecast returns its code without a launch (the pointers are never followed; the GPU test
    passes real buffers and looks at them afterwards)."""
    import ctypes
    from evennicer_slam_amd import _lib as L
    fn = L.lib().enslam_depth_forecast
    m = [1.0, 0, 0, 0, 0, 1.0, 0, 0, 0, 0, 1.0, 0]
    M = (ctypes.c_double * 12)(*m)
    good = dict(depth=depth, H=5, W=7, fx=4.0, fy=4.0, cx=3.0, cy=2.0, M=M, Ho=5, Wo=7, radius=1.0, z_near=0.0, fill=1, ws=ws,
                out=out)

    def call(**over):
        a = dict(good, **over)
        return fn(a['depth'], a['H'], a['W'], a['fx'], a['fy'], a['cx'], a['cy'], a['M'], a['Ho'], a['Wo'], a['radius'], a['z_near'],
                  a['fill'], a['ws'], a['out'], None)

    nan, inf = float('nan'), float('inf')
    einval = [dict(depth=None), dict(ws=None), dict(out=None), dict(M=None), dict(H=0), dict(W=-1), dict(Ho=0), dict(Wo=0),
              dict(fx=0.0), dict(fy=0.0), dict(fx=nan), dict(cy=inf), dict(radius=-0.5), dict(radius=nan), dict(radius=inf),
              dict(z_near=-1.0), dict(z_near=nan), dict(fill=2), dict(fill=-1), dict(ws=ws + 2), dict(out=out + 1),
              dict(depth=depth + 2), dict(H=1, Ho=2), dict(W=1, Wo=3)]
    for k in range(12):
        bad = list(m)
        bad[k] = nan if k % 2 else inf
        einval.append(dict(M=(ctypes.c_double * 12)(*bad)))
    for over in einval:
        assert call(**over) == -1, over
    for over in (dict(H=1 << 15, W=(1 << 15) + 1), dict(Ho=(1 << 15) + 1, Wo=1 << 15)):
        assert call(**over) == -3, over


def test_abi_refusals():
    check_refusals(1 << 20, 2 << 20, 3 << 20)


def test_relative_camera_matrix_is_float64_on_the_host():
    from evennicer_slam_amd import functional as EF
    a, b = np.eye(4), np.eye(4)
    a[:3, 3] = (1.0, 2.0, 3.0)
    b[:3, 3] = (1.5, 2.0, 2.0)
    m = EF.relative_camera_matrix(torch.from_numpy(a).float(), torch.from_numpy(b)[:3])
    assert m.dtype == np.float64 and m.shape == (3, 4)
    assert np.array_equal(m, np.array([[1.0, 0, 0, -0.5], [0, 1.0, 0, 0], [0, 0, 1.0, 1.0]]))


def test_entry_is_declared_bound_and_built():
    from evennicer_slam_amd import _lib as L
    assert "enslam_depth_forecast" in L.EXPORTS
    header = open(os.path.join(ROOT, "include", "enslam_hip.h")).read()
    assert "int enslam_depth_forecast(" in header
    make = open(os.path.join(ROOT, "evennicer-slam_amd", "csrc", "Makefile")).read()
    assert "depth_forecast.o" in make
