"""-m gpu: the tracker's fused loss tail on its own terms -- ens_launch_tracker_tail of csrc/render_fwd.hip
(tracker_composite_kernel, tracker_loss_kernel<COMPOSITE> with tracker_median_wg inside) through enslam_tracker_tail, by hand
through the C ABI, against the float64 yardstick of tests/tracker_tail_numpy.py on the seeded cases of
tests/tracker_tail_cases.py; never against another GPU route.  Every output buffer has sentinel rows behind it.

FULL TAIL (the device composites, handle_dynamic 0 and 1): depth, var, rgb, tmp and d_raw_unit elementwise within the derived
bars (tracker_tail_numpy.error_model: composite_numpy's bars propagated through |gd - depth| / sqrt(var + 1e-10) and through
the device's own 1 / sqrt(var' + 1e-10)); d_raw_unit exactly 0 on every ray that is not `on`; the loss within the sum of its
terms' bars; the work list equal, as a set and in its count, to the active tiles of the device's own d_raw.  The device's `on`
set is the yardstick's because every case has ZERO undecided rays and signs under the fragility rule (order statistics are
1-Lipschitz in the sup norm; tracker_tail_cases.check_conditions asserts it on the CPU).

LOSS_ONLY (the test writes tmp, depth, var, rgb; only tracker_loss_kernel<false> runs): at every batch-size edge of the launch
and of the median's two shapes (rank counting with 1024 / P lanes per entry up to 1024 rays, its 8-wide loop and its remainder;
the bitonic network above) the set of rays with a non-zero d_raw row equals the yardstick's `on` EXACTLY -- on distinct values,
all-equal values, two values split at and next to the middle, runs of ties at the median with masked entries interleaved, a
zero median, kept counts of 0, 1, 2, even and odd, a value of exactly ten medians next to one an ulp below, and +inf among
the values -- and the loss equals the float64 sum of the given terms to 1e-12.

MEASURED on an MI355X (this module with -s; worst |got - ref| / bar over all 92 full cases, forward-only reruns included):
                 mixes a, ad, abcd (unsaturated / closed / empty)      mix abcde (near-saturated samples)
    depth        0.45                                                  0.88
    var          0.39                                                  1.00 (below the bar by its rounding terms)
    rgb          0.31                                                  0.97
    tmp          0.41                                                  1.00
    d_raw_unit   0.48                                                  1.00
    loss         0.13                                                  1.00
As in tests/test_hip_composite.py there is no headroom behind a sample with 10 occ in (16.7, 20]: the kernels' m is exactly
1e-10f there, the error is the modelled 1 - alpha itself, the same on every run.  Every exact-decision case agreed at all 25
batch sizes; no kernel was changed."""

import numpy as np
import pytest
import torch

from tests import composite_numpy as Y
from tests import tracker_tail_cases as C
from tests import tracker_tail_numpy as T

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
OK, EINVAL, EUNSUPPORTED = 0, -1, -3
GUARD = 64                                       # sentinel rows behind every output buffer
SENTINEL = -7.25
N_GROUPS = 6


# ------------------------------------------------------------------------------------------------ plumbing
def _api():
    import evennicer_slam_amd as E
    import evennicer_slam_amd.functional as EF
    return E._lib.lib(), EF


def _dev(a, dtype):
    return None if a is None else torch.tensor(np.ascontiguousarray(a), dtype=dtype, device=DEV).contiguous()


def _sentinel(floating):
    return SENTINEL if floating else int(SENTINEL)


def _guarded(rows, cols, dtype, fill):
    """[rows + GUARD, cols] on the device: `fill` in the rows, SENTINEL behind them"""
    t = torch.full((rows + GUARD, cols), _sentinel(dtype.is_floating_point), dtype=dtype, device=DEV)
    t[:rows] = fill
    return t


class _Buffers:
    """the tail's output buffers, each with GUARD sentinel rows behind it; depth / var / rgb / tmp prefilled with NaN (an
    element the kernels do not write fails every comparison) or with what a loss_only test hands in"""

    def __init__(self, N, S, given=None, d_raw=True, work=True):
        nan = float('nan')
        self.N, self.S = N, S
        self.depth = _guarded(N, 1, torch.float64, nan)
        self.var = _guarded(N, 1, torch.float64, nan)
        self.rgb = _guarded(N, 3, torch.float32, nan)
        self.tmp = _guarded(N, 1, torch.float64, nan)
        if given is not None:
            for k in ('depth', 'var', 'tmp'):
                getattr(self, k)[:N, 0] = _dev(given[k], torch.float64)
            self.rgb[:N] = _dev(given['rgb'], torch.float32)
        self.loss = _guarded(1, 1, torch.float64, 0.0)
        self.d_raw = _guarded(N * S, 4, torch.float32, nan) if d_raw else None
        self.n_tiles = N * (S // 16)
        self.work = _guarded(self.n_tiles, 1, torch.int32, int(SENTINEL)) if work else None
        self.count = _guarded(1, 1, torch.int32, 0) if work else None

    def host(self):
        """dict of numpy arrays (guards cut off) after asserting that every guard row still holds the sentinel"""
        torch.cuda.synchronize()
        out = {}
        for k, rows in (('depth', self.N), ('var', self.N), ('rgb', self.N), ('tmp', self.N), ('loss', 1),
                        ('d_raw', self.N * self.S), ('work', self.n_tiles), ('count', 1)):
            t = getattr(self, k)
            if t is None:
                out[k] = None
                continue
            a = t.cpu().numpy()
            assert (a[rows:] == _sentinel(a.dtype.kind == 'f')).all(), f"{k}: a row behind the last of {rows} was written"
            out[k] = a[:rows]
        out['depth'], out['var'], out['tmp'] = out['depth'][:, 0], out['var'][:, 0], out['tmp'][:, 0]
        out['loss'] = float(out['loss'][0, 0])
        if out['d_raw'] is not None:
            out['d_raw'] = out['d_raw'].reshape(self.N, self.S, 4)
        if out['work'] is not None:
            out['work'], out['count'] = out['work'][:, 0], int(out['count'][0, 0])
        return out


def _call(N, S, raw, z, gd, gc, w, inside, dynamic, buf, loss_only=0):
    """enslam_tracker_tail by hand; returns the code"""
    lib, EF = _api()
    P = EF._ptr
    keep = [_dev(raw, torch.float32), _dev(z, torch.float64), _dev(gd, torch.float32), _dev(gc, torch.float32),
            _dev(inside, torch.uint8)]
    rc = lib.enslam_tracker_tail(N, S, P(keep[0]), P(keep[1]), P(buf.depth), P(buf.var), P(buf.rgb), P(keep[2]), P(keep[3]),
                                 float(w), P(keep[4]), int(dynamic), P(buf.tmp), P(buf.loss), P(buf.d_raw), P(buf.work),
                                 P(buf.count), int(loss_only), EF._stream())
    torch.cuda.synchronize()
    return rc


def _run_case(c, d_raw=True):
    buf = _Buffers(c['N'], c['S'], d_raw=d_raw, work=d_raw and c['S'] % 16 == 0)
    rc = _call(c['N'], c['S'], c['raw'], c['z'], c['gd'], c['gc'], c['w'], c['inside'], c['dynamic'], buf)
    assert rc == OK, (c['name'], rc)
    return buf.host()


def _ratio(err, bar):
    pos = bar > 0
    return float((err[pos] / bar[pos]).max()) if pos.any() else 0.0


def _within(worst, name, got, ref, bar, where):
    got = np.asarray(got, np.float64)
    assert np.isfinite(got).all(), (name, where)
    err = np.abs(got - ref)
    bar = np.broadcast_to(bar, err.shape)
    r = _ratio(err, bar)
    print(f"    {where}: {name} worst |error| / bar = {r:.3g}")
    assert (err <= bar).all(), (name, where, r)
    worst[name] = max(worst.get(name, 0.0), r)


def _check_work_list(got, S, where):
    """the list equals, as a set and in its count, the active tiles of the device's own d_raw; nothing behind the count"""
    tiles = Y.active_tiles(got['d_raw'], S)
    assert got['count'] == len(tiles), (where, got['count'], len(tiles))
    listed = got['work'][:got['count']].tolist()
    assert len(set(listed)) == len(listed) and set(listed) == tiles, where
    assert (got['work'][got['count']:] == int(SENTINEL)).all(), where


# ------------------------------------------------------------------------------------------------ the full tail
@pytest.mark.parametrize("group", range(N_GROUPS))
def test_full_tail_against_float64(group):
    """every full case (a sixth of them per parameter): depth, var, rgb, tmp, d_raw_unit within their bars, exact zeros off the
    `on` rays and where the scale is 0, the loss within its bar, the work list exact; the loss alone (d_raw_unit NULL) the same.
    Measured on an MI355X: see the module docstring (printed per case with -s)."""
    worst = {}
    for c in C.full_cases()[group::N_GROUPS]:
        y, b, where = c['y'], c['b'], c['name']
        got = _run_case(c)
        for k in ('depth', 'var', 'rgb', 'tmp'):
            _within(worst, k, got[k], y[k], b[k], where)
        d = got['d_raw']
        assert not d[~y['on']].any(), (where, "a gradient on a ray that is not on")
        assert not d[b['d_scale'] == 0].any(), where
        _within(worst, 'd_raw', d, y['d_raw'], b['d_raw'], where)
        assert ((d != 0).any((1, 2)) <= y['on']).all()
        _within(worst, 'loss', np.array([got['loss']]), y['loss'], b['loss'], where)
        if c['S'] % 16 == 0:
            _check_work_list(got, c['S'], where)
            if not y['on'].any():
                assert got['count'] == 0, where
        if c['dup']:                                             # copies of a ray: the same bits of tmp wherever they sit
            cp = np.nonzero(np.arange(c['N']) % 3 == 2)[0]
            assert (got['tmp'][cp].view(np.int64) == got['tmp'][0:1].view(np.int64)).all(), where
            assert (got['depth'][cp].view(np.int64) == got['depth'][0:1].view(np.int64)).all(), where
        lone = _run_case(c, d_raw=False)                         # forward only: the same outputs, the loss within its bar
        for k in ('depth', 'var', 'rgb', 'tmp'):
            assert got[k].tobytes() == lone[k].tobytes(), (where, k)
        assert abs(lone['loss'] - y['loss']) <= b['loss'], where
    print("  worst |error| / bar:", {k: round(v, 4) for k, v in worst.items()})


# ------------------------------------------------------------------------------------------------ exact decisions
def _given(e):
    """what a loss_only test hands in besides tmp: depth = gd + 1 (the depth sign is +), var = 1, rgb = 0.25 against
    gt_color = 0.75 (every colour sign is +): an `on` ray's colour columns are -w * weight != 0, so a zero row means not on"""
    N = e['N']
    return dict(tmp=e['tmp'], depth=e['gd'].astype(np.float64) + 1.0, var=np.ones(N), rgb=np.full((N, 3), 0.25, np.float32)), \
        np.full((N, 3), 0.75, np.float32)


def _run_exact(e, raw, z, w=0.5):
    N = e['N']
    given, gc = _given(e)
    buf = _Buffers(N, 16, given=given)
    rc = _call(N, 16, raw, z, e['gd'], gc, w, e['inside'], 1, buf, loss_only=1)
    assert rc == OK, (e['name'], N, rc)
    got = buf.host()
    for k in ('depth', 'var', 'tmp', 'rgb'):                     # the loss launch only reads them
        assert got[k].tobytes() == np.ascontiguousarray(given[k]).tobytes(), (e['name'], N, k)
    return got, given, gc


@pytest.mark.parametrize("N", C.N_EDGES)
def test_loss_only_keeps_exactly_the_yardsticks_rays(N):
    raw, z = C._rows(16, N, 'a')
    assert (Y.forward(raw, z)['w'][:, 0] > 1e-3).all()           # every ray's first weight is far from 0
    for e in C.exact_cases(N):
        got, given, gc = _run_exact(e, raw, z)
        rows = (got['d_raw'] != 0).any((1, 2))
        where = (e['name'], N)
        assert (rows == e['on']).all(), (where, np.nonzero(rows != e['on'])[0][:8].tolist(), e['med'])
        assert np.isfinite(got['d_raw']).all(), where
        ref, ref_abs = T.given_loss(given['tmp'], given['rgb'], e['gd'], gc, 0.5, e['on'])
        assert abs(got['loss'] - ref) <= 1e-12 * ref_abs, (where, got['loss'], ref)
        _check_work_list(got, 16, where)
        assert got['count'] == int(e['on'].sum()) and set(got['work'][:got['count']].tolist()) == set(np.nonzero(e['on'])[0].tolist())


def test_the_same_case_at_1024_and_1025_rays():
    """rank counting at 1024 rays, the bitonic network at 1025 with the extra ray masked out: the same rays kept -- on tmp the
    test wrote (the extra ray's 0 would move the median if it counted) and on device-composited rays"""
    raw, z = C._rows(16, 1025, 'a')
    for name in ('distinct, no mask', 'tie run at the median', 'ten times the median', 'a few inf'):
        e = next(x for x in C.exact_cases(1024) if x['name'] == name)
        ins = np.ones(1024, np.uint8) if e['inside'] is None else e['inside']
        e2 = dict(name=name + ' + 1', N=1025, tmp=np.append(e['tmp'], 0.0), gd=np.append(e['gd'], np.float32(2.0)),
                  inside=np.append(ins, np.uint8(0)))
        a, _, _ = _run_exact(e, raw[:1024], z[:1024])
        b2, _, _ = _run_exact(e2, raw, z)
        ra, rb = (a['d_raw'] != 0).any((1, 2)), (b2['d_raw'] != 0).any((1, 2))
        assert (ra == e['on']).all() and (rb[:1024] == e['on']).all() and not rb[1024], name
    c = next(x for x in C.full_cases() if x['N'] == 1024 and x['dynamic'] and x['inside_kind'] == 'null')
    ap = lambda v, i=5: np.concatenate([v, v[i:i + 1]])
    c2 = dict(c, N=1025, raw=ap(c['raw']), z=ap(c['z']), gd=ap(c['gd']), gc=None if c['gc'] is None else ap(c['gc']),
              inside=np.append(np.ones(1024, np.uint8), np.uint8(0)), name=c['name'] + ' + 1')
    a, b2 = _run_case(c), _run_case(c2)
    ra, rb = (a['d_raw'] != 0).any((1, 2)), (b2['d_raw'] != 0).any((1, 2))
    on, plain = c['y']['on'], np.arange(1024) % len(c['mix']) == 0       # (an empty or closed ray that is on may have a zero row)
    assert (ra == rb[:1024]).all() and not rb[1024] and (ra <= on).all() and (ra[plain] == on[plain]).all()
    assert on[plain].any() and not on[plain].all()
    assert a['tmp'].tobytes() == b2['tmp'][:1024].tobytes() and a['d_raw'].tobytes() == b2['d_raw'][:1024].tobytes()


# ------------------------------------------------------------------------------------------------ argument rules
def test_error_codes_of_the_entry():
    lib, EF = _api()
    P, st = EF._ptr, EF._stream()
    assert lib.enslam_tracker_tail_max_rays() == 4096
    N, S = 20, 16
    raw, z = C._rows(17, N, 'a')                                 # room for the calls with 17 samples; 16 read its first rows
    gd = np.full(N, 2.0, np.float32)
    r, zz, g = _dev(raw, torch.float32), _dev(z, torch.float64), _dev(gd, torch.float32)

    def call(n=N, s=S, loss_only=0, dynamic=1, buf=None, **null):
        buf = buf or _Buffers(N, 17)
        a = dict(raw=P(r), z=P(zz), depth=P(buf.depth), var=P(buf.var), rgb=P(buf.rgb), gd=P(g), tmp=P(buf.tmp), loss=P(buf.loss),
                 d_raw=P(buf.d_raw), work=P(buf.work), count=P(buf.count))
        a.update({k: None for k in null})
        rc = lib.enslam_tracker_tail(n, s, a['raw'], a['z'], a['depth'], a['var'], a['rgb'], a['gd'], None, 0.5, None, dynamic,
                                     a['tmp'], a['loss'], a['d_raw'], a['work'], a['count'], loss_only, st)
        got = buf.host()                                         # asserts the guards
        for k in ('depth', 'var', 'tmp', 'rgb', 'd_raw'):
            if rc != OK or n == 0:                               # a refused call, and an empty one, touch nothing
                assert np.isnan(got[k]).all(), (k, rc)
        if rc != OK or n == 0:
            assert got['loss'] == 0.0 and got['count'] == 0 and (got['work'] == int(SENTINEL)).all()
        return rc

    assert call() == OK
    assert call(n=4097) == EUNSUPPORTED
    assert call(n=-1) == EINVAL
    assert call(s=0) == EINVAL and call(s=65) == EINVAL
    assert call(s=17) == EINVAL                                  # a work list needs whole 16-sample tiles
    assert call(s=17, work=1, count=1) == OK
    for name in ('raw', 'z', 'depth', 'var', 'rgb', 'gd', 'tmp', 'loss'):
        assert call(**{name: 1}) == EINVAL, name
    assert call(work=1) == EINVAL and call(count=1) == EINVAL    # a list without its count, a count without its list
    assert call(d_raw=1) == EINVAL                               # a work list without d_raw_unit
    assert call(d_raw=1, work=1, count=1) == OK
    assert call(loss_only=1, dynamic=0) == EINVAL
    assert call(n=0) == OK
    assert call(n=0, raw=1, z=1, depth=1) == OK                  # an empty batch returns before it looks at anything
