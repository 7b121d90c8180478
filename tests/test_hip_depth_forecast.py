"""GPU: the depth forecast kernel (csrc/depth_forecast.hip, functional.depth_forecast) -- every case of
tests/depth_forecast_cases.py bit-equal to the yardstick with both fill settings, the same bits in a second call, the ABI
refusals with real buffers, and guard regions around output and workspace."""
import ctypes

import numpy as np
import pytest
import torch

from tests import depth_forecast_cases as C

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
GUARD = 256


def _bits(t):
    return t.detach().cpu().contiguous().numpy().view(np.uint32)


def _run(case, fill, depth=None):
    from evennicer_slam_amd import functional as EF
    d = torch.from_numpy(case['depth']).to(DEV) if depth is None else depth
    out = EF.depth_forecast(d, case['cam'], case['M'], case['size'], radius=case['radius'], z_near=case['z_near'], fill=bool(fill))
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize('fill', C.FILLS)
@pytest.mark.parametrize('case', C.CASES, ids=[c['name'] for c in C.CASES])
def test_case_on_the_device(case, fill):
    d = torch.from_numpy(case['depth']).to(DEV)
    out = _run(case, fill, d)
    assert out.is_cuda and out.dtype == torch.float32 and tuple(out.shape) == tuple(case['size'])
    want = C.expected(case, fill).view(np.uint32)
    got = _bits(out)
    print(case['name'], fill, 'pixels that differ:', int((got != want).sum()), 'of', want.size)
    assert np.array_equal(got, want)
    assert np.array_equal(_bits(_run(case, fill, d)), got)                          # the same bits again
    assert np.array_equal(_bits(d), case['depth'].view(np.uint32))                  # the input is only read


@pytest.mark.parametrize('name', ['1x1', '5x7_to_3x4', '45x61_occlusion', '45x61_rotation_7x9'])
def test_guard_regions_stay_intact(name):
    """output and workspace sit between GUARD sentinel elements inside one allocation; the raw entry is called"""
    from evennicer_slam_amd import _lib as L
    from evennicer_slam_amd import functional as EF
    case = C.BY_NAME[name]
    H, W = case['depth'].shape
    Ho, Wo = case['size']
    cam = case['cam']
    d = torch.from_numpy(case['depth']).to(DEV)
    SENT = -7.5

    def guarded(n):
        buf = torch.full((n + 2 * GUARD,), SENT, dtype=torch.float32, device=DEV)
        return buf, buf[GUARD:GUARD + n]

    bufs = dict(out=guarded(Ho * Wo), ws=guarded(Ho * Wo))
    for fill in C.FILLS:
        rc = L.lib().enslam_depth_forecast(d.data_ptr(), H, W, cam['fx'], cam['fy'], cam['cx'], cam['cy'],
                                           (ctypes.c_double * 12)(*case['M'].reshape(-1)), Ho, Wo, case['radius'], case['z_near'], fill,
                                           bufs['ws'][1].data_ptr(), bufs['out'][1].data_ptr(), EF._stream())
        torch.cuda.synchronize()
        assert rc == 0
        for k, (buf, view) in bufs.items():
            assert bool((buf[:GUARD] == SENT).all()) and bool((buf[GUARD + view.numel():] == SENT).all()), k
        assert not bool((bufs['out'][1] == SENT).any())                              # every pixel inside was written
        assert np.array_equal(_bits(bufs['out'][1]).reshape(Ho, Wo), C.expected(case, fill).view(np.uint32))


def test_abi_refusals_leave_the_buffers_alone():
    from tests.test_depth_forecast_cpu import check_refusals
    case = C.BY_NAME['5x7_plane']
    d = torch.from_numpy(case['depth']).to(DEV)
    out = torch.full((4096,), -7.5, dtype=torch.float32, device=DEV)
    ws = torch.full((4096,), -7.5, dtype=torch.float32, device=DEV)
    check_refusals(d.data_ptr(), ws.data_ptr(), out.data_ptr())
    torch.cuda.synchronize()
    assert bool((out == -7.5).all()) and bool((ws == -7.5).all())
    assert np.array_equal(_bits(d), case['depth'].view(np.uint32))


def test_wrapper_refusals_on_the_device():
    from evennicer_slam_amd import functional as EF
    from evennicer_slam_amd._lib import EnslamError
    case = C.BY_NAME['5x7_plane']
    d = torch.from_numpy(case['depth']).to(DEV)
    for bad in (d.double(), d.t(), d[None]):
        with pytest.raises(EnslamError):
            EF.depth_forecast(bad, case['cam'], case['M'], (5, 7))
    for kw in (dict(out_size=(0, 7)), dict(out_size=(5, 7), radius=-1.0)):
        with pytest.raises(EnslamError):
            EF.depth_forecast(d, case['cam'], case['M'], **kw)
