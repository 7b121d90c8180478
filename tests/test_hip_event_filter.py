"""-m gpu: csrc/event_filter.hip -- the classify / walk / support / state / compact kernels behind event_filter.EventFilter on a
HIP device -- against the scalar yardstick tests/event_filter_numpy.py on the cases of tests/event_filter_cases.py.

Everything is bit-equal: classes, t / x / y / p of the output, t_last, t_seen and the counters, for every case; the four
orders of 37x53_noisy each take the ordering path their flags select; chunked with carried state equals one call; two runs
are bit-identical and the input is untouched.  The entries are memory-safe with a wrong `order`, `starts` and `ends` (guard
regions around every output), and the ABI refusals return their codes without a launch."""
import os

import numpy as np
import pytest
import torch

from tests import event_filter_cases as FC
from tests.test_event_filter_cpu import (_bits, _filter, _stream, check_against, check_simulator_consistency, check_tool_route,
                                         run_chunked)

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
GUARD = 64


@pytest.mark.parametrize("name", sorted(FC.cases()))
def test_device_is_bit_equal(name):
    c, ref = FC.cases()[name], FC.reference(name)
    filt = _filter(c, DEV)
    stream = _stream(c, DEV)
    kept, stats, classes = filt(stream, return_classes=True)
    assert all(a.device.type == 'cuda' for a in kept.arrays()) and classes.device.type == 'cuda' and classes.dtype == torch.uint8
    assert filt.t_last.device.type == 'cuda' and filt.t_seen.device.type == 'cuda'
    check_against(ref, kept, stats, classes, filt)
    assert all(np.array_equal(_bits(a), _bits(c[k])) for k, a in zip('txyp', stream.arrays()))          # the input is untouched
    # a second run on a fresh filter: the same bits
    again = _filter(c, DEV)
    kept2, stats2, classes2 = again(stream, return_classes=True)
    assert stats2 == stats and torch.equal(classes2, classes) and torch.equal(again.t_last.view(torch.int64), filt.t_last.view(torch.int64))
    assert torch.equal(again.t_seen.view(torch.int64), filt.t_seen.view(torch.int64))
    assert all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(kept.arrays(), kept2.arrays()))


def test_empty_stream_gives_four_empty_device_arrays():
    c = FC.cases()['edge_0']
    kept, stats = _filter(c, DEV)(_stream(c, DEV))
    assert len(kept) == 0 and stats['n_in'] == stats['n_out'] == 0
    assert [a.dtype for a in kept.arrays()] == [torch.float64, torch.uint16, torch.uint16, torch.uint8]
    assert all(a.device.type == 'cuda' and tuple(a.shape) == (0,) for a in kept.arrays())


@pytest.mark.parametrize("order", FC.NOISY_ORDERS)
def test_orders_take_their_own_path(order):
    """the flags the classify entry reports, the path they select, and the same classes through the permutation"""
    from evennicer_slam_amd import functional as EF
    c, perm = FC.noisy(order)
    stream = _stream(c, DEV)
    path, flags = FC.NOISY_PATHS[order]
    cls, pix, counts, got_flags = EF.event_pixel_counts(*stream.arrays(), c['H'], c['W'])
    assert got_flags == flags
    assert bool((cls == 0).all()) and np.array_equal(pix.cpu().numpy(), c['y'].astype(np.int32) * c['W'] + c['x'])
    assert np.array_equal(counts.cpu().numpy().reshape(-1), np.bincount(pix.cpu().numpy(), minlength=c['H'] * c['W']))
    order_t, starts, got_path = EF.event_filter_order(stream.t, cls, pix, counts, got_flags)
    assert got_path == path and order_t.dtype == torch.int32 and starts.dtype == torch.int64
    o, t = pix.cpu().numpy()[order_t.cpu().numpy()], c['t'][order_t.cpu().numpy()]
    assert bool(np.all((o[1:] > o[:-1]) | ((o[1:] == o[:-1]) & (t[1:] >= t[:-1]))))
    filt = _filter(c, DEV)
    classes = filt(stream, return_classes=True)[2]
    assert filt.last_path == path
    assert np.array_equal(classes.cpu().numpy(), FC.reference('37x53_noisy_emitted')['classes'][0][perm])
    # a single emitted interval is pixel-major: no sort
    one = FC.cut(FC.noisy('emitted')[0], [int(np.flatnonzero(np.diff(FC.noisy('emitted')[0]['y'].astype(np.int64)) < 0)[0]) + 1])[0]
    assert EF.event_pixel_counts(*_stream(one, DEV).arrays(), one['H'], one['W'])[3] & EF.EVENT_NOT_PIXEL_MAJOR == 0


def test_flags_with_dead_events_between_live_ones():
    """dead events between two live ones are looked through; more than 32 in a row report both bits (which only costs a sort)"""
    from evennicer_slam_amd import functional as EF
    from evennicer_slam_amd.event_stream import EventStream

    def flags(t, x):
        s = EventStream(np.array(t, dtype=np.float64), np.array(x, dtype=np.uint16), np.zeros(len(t), dtype=np.uint16),
                        np.zeros(len(t), dtype=np.uint8)).to(DEV)
        return EF.event_pixel_counts(*s.arrays(), 1, 4)[3]

    assert flags([1.0, 5.0, 2.0], [0, 9, 1]) == 0                           # the SENSOR event in between does not count
    assert flags([1.0, np.nan, 0.5], [0, 0, 1]) == EF.EVENT_NOT_TIME_ORDERED
    assert flags([1.0, np.nan, 2.0], [1, 0, 0]) == EF.EVENT_NOT_PIXEL_MAJOR
    assert flags([1.0] + [0.0] * 32 + [2.0], [0] + [9] * 32 + [1]) == 0
    assert flags([1.0] + [0.0] * 33 + [2.0], [0] + [9] * 33 + [1]) == 3
    assert flags([0.0] * 20 + [2.0], [9] * 20 + [1]) == 0                   # no live event before it at all


@pytest.mark.parametrize("count", FC.SPLIT_COUNTS)
def test_chunked_with_carried_state_equals_one_shot(count):
    chunks = FC.cut(FC.noisy('time')[0], FC.split_points(count))
    check_against(FC.reference('37x53_noisy_time'), *run_chunked(chunks, DEV))


def test_boundary_tie_and_chunk_order_refusal():
    from evennicer_slam_amd._lib import EnslamError
    chunks, _, chunked = FC.boundary_tie()
    ref = FC.run_yardstick(chunks)
    assert np.concatenate(ref['classes']).tolist() == chunked
    kept, stats, classes, filt = run_chunked(chunks, DEV)
    check_against(ref, kept, stats, classes, filt)
    before = (filt.t_last.clone(), filt.t_seen.clone())
    early = dict(chunks[0], t=chunks[0]['t'] - FC.U)
    with pytest.raises(EnslamError):
        filt(_stream(early, DEV))
    assert torch.equal(filt.t_last, before[0]) and torch.equal(filt.t_seen, before[1])
    with pytest.raises(EnslamError):
        filt(_stream(early, 'cpu'))                             # a stream on another device


def test_simulator_consistency_on_the_device():
    check_simulator_consistency(DEV)


def test_hot_pixels_on_the_device():
    from evennicer_slam_amd.event_filter import filter_stream, hot_pixels
    for c in (FC.planted(), FC.noisy('shuffled')[0]):
        H, W = c['H'], c['W']
        t, x, y = c['t'], c['x'].astype(np.int64), c['y'].astype(np.int64)
        ok = (x < W) & (y < H) & np.isfinite(t)
        want = np.bincount(y[ok] * W + x[ok], minlength=H * W).reshape(H, W)
        limit = int(np.median(want[want > 0]))
        mask, counts = hot_pixels(_stream(c, DEV), H, W, max_events=limit)
        assert mask.device.type == 'cuda' and mask.dtype == torch.bool and counts.dtype == torch.int64
        assert np.array_equal(counts.cpu().numpy(), want) and np.array_equal(mask.cpu().numpy(), want > limit) and bool(mask.any())
        span = float(t[np.isfinite(t)].max() - t[np.isfinite(t)].min())
        mask_r = hot_pixels(_stream(c, DEV), H, W, rate=(limit + 0.5) / span)[0]
        cpu_r = hot_pixels(_stream(c), H, W, rate=(limit + 0.5) / span)[0]
        assert torch.equal(mask_r.cpu(), cpu_r)
        stats = filter_stream(_stream(c, DEV), H, W, hot_mask=mask)[1]
        assert stats['hot'] == int(want[want > limit].sum())


def test_tool_on_the_device_writes_the_bytes_of_the_cpu_route(tmp_path, capsys):
    r, dev_dir, want_dir = check_tool_route(tmp_path, capsys, DEV)          # byte-equal to the yardstick's events binned on the CPU
    assert len(os.listdir(dev_dir)) == len(os.listdir(want_dir)) == r['n'] - 1
    from tests.test_event_filter_cpu import OPTIONS, _tool
    cpu_dir = str(tmp_path / 'flags_cpu')
    flags = ['--refractory', str(OPTIONS['refractory']), '--support-dt', str(OPTIONS['support_dt']), '--hot-max', str(OPTIONS['hot_max'])]
    info = _tool("events_to_frames").main([os.path.join(r['root'], 'events.txt'), os.path.join(r['root'], 'images.txt'), '--out', cpu_dir,
                                           '--height', str(r['H']), '--width', str(r['W']), '--device', 'cpu'] + flags)
    capsys.readouterr()
    assert info['filter']['n_out'] == info['events_binned'] > 0
    for name in sorted(os.listdir(cpu_dir)):
        with open(os.path.join(cpu_dir, name), 'rb') as a, open(os.path.join(dev_dir, name), 'rb') as b:
            assert a.read() == b.read(), name


def _guarded(n, dtype, fill):
    whole = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=DEV)
    return whole, whole[GUARD:GUARD + n]


def _guards_intact(whole, n, fill):
    return bool((whole[:GUARD] == fill).all()) and bool((whole[GUARD + n:] == fill).all())


def test_wrong_order_and_starts_stay_in_bounds():
    """a reversed permutation as `order`, `starts` all zero (and, second, the right starts with the wrong order), `ends` that
    point past the capacity: every entry returns without error and the guard regions around every output are unchanged"""
    from evennicer_slam_amd import _lib as L
    from evennicer_slam_amd import functional as EF
    lib = L.lib()
    c = FC.noisy('shuffled')[0]
    H, W, N, P = c['H'], c['W'], c['t'].shape[0], c['H'] * c['W']
    s = _stream(c, DEV)
    ptr = lambda a: a.data_ptr()
    cls_w, cls = _guarded(N, torch.uint8, 0x5A)
    pix_w, pix = _guarded(N, torch.int32, 0x5A5A)
    cnt_w, cnt = _guarded(P, torch.int32, 0x5A5A)
    flg_w, flg = _guarded(1, torch.int32, 0x5A5A)
    assert lib.enslam_event_pixel_counts(ptr(s.t), ptr(s.x), ptr(s.y), N, H, W, None, ptr(cls), ptr(pix), ptr(cnt), ptr(flg), None) == 0
    torch.cuda.synchronize()
    assert _guards_intact(cls_w, N, 0x5A) and _guards_intact(pix_w, N, 0x5A5A) and _guards_intact(cnt_w, P, 0x5A5A) and _guards_intact(flg_w, 1, 0x5A5A)
    assert int(cnt.sum()) == N and int(flg.item()) == 3
    right_starts = EF.event_filter_order(s.t, cls, pix, cnt.reshape(H, W), 3)[1]
    reversed_order = torch.arange(N - 1, -1, -1, dtype=torch.int32, device=DEV)
    for starts in (torch.zeros(P + 1, dtype=torch.int64, device=DEV), right_starts,
                   torch.full((P + 1,), 2 ** 40, dtype=torch.int64, device=DEV), -right_starts):
        cls.copy_(torch.zeros_like(cls))
        tl_w, tl = _guarded(P, torch.float64, -7.0)
        ts_w, ts = _guarded(P, torch.float64, -7.0)
        tl.fill_(-np.inf)
        ts.fill_(-np.inf)
        st_w, st = _guarded(N, torch.float64, -7.0)
        se_w, se = _guarded(N, torch.int32, 0x5A5A)
        sc_w, sc = _guarded(P, torch.int32, 0x5A5A)
        assert lib.enslam_event_filter_walk(ptr(s.t), N, H, W, c['rho'], ptr(pix), ptr(reversed_order), N, ptr(starts), ptr(cls), ptr(tl),
                                            ptr(st), ptr(se), ptr(sc), None) == 0
        assert lib.enslam_event_filter_support(N, H, W, 1, c['dt'], ptr(pix), N, ptr(starts), ptr(cls), ptr(tl), ptr(ts), ptr(st), ptr(se),
                                               ptr(sc), None) == 0
        torch.cuda.synchronize()
        assert _guards_intact(cls_w, N, 0x5A) and _guards_intact(tl_w, P, -7.0) and _guards_intact(ts_w, P, -7.0)
        assert _guards_intact(st_w, N, -7.0) and _guards_intact(se_w, N, 0x5A5A) and _guards_intact(sc_w, P, 0x5A5A)
        assert bool((cls <= 5).all()) and bool((sc >= 0).all()) and bool((se >= -1).all()) and bool((se < N).all())
    n_out = 100
    outs = [_guarded(n_out, d, f) for d, f in ((torch.float64, -7.0), (torch.uint16, 0x5A5A), (torch.uint16, 0x5A5A), (torch.uint8, 0x5A))]
    cls.copy_(torch.zeros_like(cls))
    for ends in (torch.full((N,), n_out + 5, dtype=torch.int64, device=DEV), torch.zeros(N, dtype=torch.int64, device=DEV),
                 torch.arange(N, dtype=torch.int64, device=DEV) - 50):
        assert lib.enslam_event_filter_compact(ptr(s.t), ptr(s.x), ptr(s.y), ptr(s.p), N, ptr(cls), ptr(ends), n_out,
                                               *(ptr(v) for _, v in outs), None) == 0
        torch.cuda.synchronize()
        for (whole, _), fill in zip(outs, (-7.0, 0x5A5A, 0x5A5A, 0x5A)):
            assert _guards_intact(whole, n_out, fill)


def test_abi_refusals_without_a_launch():
    from evennicer_slam_amd import _lib as L
    lib = L.lib()
    H, W, N, P = 4, 5, 8, 20
    ptr = lambda a: a.data_ptr() if a is not None else None
    t = torch.full((N,), -1.0, dtype=torch.float64, device=DEV)
    x = torch.full((N + 1,), 1, dtype=torch.uint16, device=DEV)
    y = torch.full((N,), 1, dtype=torch.uint16, device=DEV)
    p = torch.full((N,), 1, dtype=torch.uint8, device=DEV)
    cls = torch.full((N,), 9, dtype=torch.uint8, device=DEV)
    pix = torch.full((N + 1,), -5, dtype=torch.int32, device=DEV)
    cnt = torch.full((P + 1,), -5, dtype=torch.int32, device=DEV)
    flg = torch.full((2,), -5, dtype=torch.int32, device=DEV)
    order = torch.zeros(N + 1, dtype=torch.int32, device=DEV)
    starts = torch.zeros(P + 2, dtype=torch.int64, device=DEV)
    tl = torch.full((P + 1,), -7.0, dtype=torch.float64, device=DEV)
    ts = torch.full((P + 1,), -7.0, dtype=torch.float64, device=DEV)
    st = torch.full((N + 1,), -7.0, dtype=torch.float64, device=DEV)
    se = torch.full((N + 1,), -5, dtype=torch.int32, device=DEV)
    sc = torch.full((P + 1,), -5, dtype=torch.int32, device=DEV)
    ends = torch.zeros(N + 1, dtype=torch.int64, device=DEV)
    to = torch.full((N + 1,), -7.0, dtype=torch.float64, device=DEV)
    xo = torch.full((N + 1,), 7, dtype=torch.uint16, device=DEV)
    yo = torch.full((N + 1,), 7, dtype=torch.uint16, device=DEV)
    po = torch.full((N,), 7, dtype=torch.uint8, device=DEV)
    inf, nan = float('inf'), float('nan')

    def off(a, nbytes):
        return a.data_ptr() + nbytes

    def counts(t_=ptr(t), x_=ptr(x), y_=ptr(y), n=N, h=H, w=W, cls_=ptr(cls), pix_=ptr(pix), cnt_=ptr(cnt), flg_=ptr(flg)):
        return lib.enslam_event_pixel_counts(t_, x_, y_, n, h, w, None, cls_, pix_, cnt_, flg_, None)

    def walk(t_=ptr(t), n=N, h=H, w=W, rho=0.0, pix_=ptr(pix), order_=ptr(order), nl=N, starts_=ptr(starts), cls_=ptr(cls), tl_=ptr(tl),
             st_=ptr(st), se_=ptr(se), sc_=ptr(sc)):
        return lib.enslam_event_filter_walk(t_, n, h, w, rho, pix_, order_, nl, starts_, cls_, tl_, st_, se_, sc_, None)

    def support(n=N, h=H, w=W, dt=0.0, pix_=ptr(pix), nl=N, starts_=ptr(starts), cls_=ptr(cls), tl_=ptr(tl), ts_=ptr(ts), st_=ptr(st),
                se_=ptr(se), sc_=ptr(sc)):
        return lib.enslam_event_filter_support(n, h, w, 1, dt, pix_, nl, starts_, cls_, tl_, ts_, st_, se_, sc_, None)

    def compact(t_=ptr(t), x_=ptr(x), n=N, cls_=ptr(cls), ends_=ptr(ends), n_out=N, to_=ptr(to), xo_=ptr(xo), yo_=ptr(yo), po_=ptr(po)):
        return lib.enslam_event_filter_compact(t_, x_, ptr(y), ptr(p), n, cls_, ends_, n_out, to_, xo_, yo_, po_, None)

    inval = [counts(t_=None), counts(x_=None), counts(y_=None), counts(n=-1), counts(h=0), counts(w=-2), counts(cls_=None),
             counts(pix_=None), counts(cnt_=None), counts(flg_=None), counts(x_=off(x, 1)), counts(pix_=off(pix, 2)),
             counts(cnt_=off(cnt, 1)), counts(flg_=off(flg, 2)), counts(t_=off(t, 4)),
             walk(t_=None), walk(n=-1), walk(h=0), walk(w=0), walk(rho=-1e-3), walk(rho=inf), walk(rho=nan), walk(pix_=None),
             walk(order_=None), walk(nl=-1), walk(nl=N + 1), walk(starts_=None), walk(cls_=None), walk(tl_=None), walk(st_=None),
             walk(se_=None), walk(sc_=None), walk(order_=off(order, 2)), walk(starts_=off(starts, 4)), walk(tl_=off(tl, 4)),
             walk(st_=off(st, 4)), walk(se_=off(se, 2)), walk(sc_=off(sc, 2)),
             support(n=-1), support(h=0), support(dt=-1.0), support(dt=inf), support(dt=nan), support(pix_=None), support(nl=N + 1),
             support(starts_=None), support(cls_=None), support(tl_=None), support(ts_=None), support(st_=None), support(se_=None),
             support(sc_=None), support(ts_=off(ts, 4)), support(starts_=off(starts, 4)),
             compact(t_=None), compact(x_=None), compact(n=-1), compact(cls_=None), compact(ends_=None), compact(n_out=-1),
             compact(n_out=N + 1), compact(to_=None), compact(xo_=None), compact(yo_=None), compact(po_=None),
             compact(ends_=off(ends, 4)), compact(to_=off(to, 4)), compact(xo_=off(xo, 1)), compact(yo_=off(yo, 1))]
    assert inval == [-1] * len(inval), inval
    unsupported = [counts(n=2 ** 31), counts(h=65537), counts(w=65537), counts(h=1 << 15, w=1 << 14),
                   walk(h=65537), walk(h=1 << 15, w=1 << 14), support(w=65537), support(h=1 << 15, w=1 << 14), compact(n=2 ** 31, n_out=0)]
    assert unsupported == [-3] * len(unsupported), unsupported
    torch.cuda.synchronize()
    # nothing ran
    assert bool((cls == 9).all()) and bool((pix == -5).all()) and bool((cnt == -5).all()) and bool((flg == -5).all())
    assert bool((tl == -7.0).all()) and bool((ts == -7.0).all()) and bool((st == -7.0).all()) and bool((se == -5).all()) and bool((sc == -5).all())
    assert bool((to == -7.0).all()) and bool((xo == 7).all()) and bool((yo == 7).all()) and bool((po == 7).all())
    # the valid neighbours: N = 0 with NULL arrays clears counts and flags; n_live = 0 walks nothing and writes zero counts
    assert counts(t_=None, x_=None, y_=None, n=0, cls_=None, pix_=None) == 0
    torch.cuda.synchronize()
    assert bool((cnt[:P] == 0).all()) and int(cnt[P]) == -5 and flg.tolist() == [0, -5]
    assert walk(order_=None, nl=0, st_=None, se_=None) == 0 and compact(n_out=0, to_=None, xo_=None, yo_=None, po_=None) == 0
    torch.cuda.synchronize()
    assert bool((sc[:P] == 0).all()) and int(sc[P]) == -5 and bool((tl == -7.0).all())
