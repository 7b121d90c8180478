"""Cases of the event-stream filter (event_filter.EventFilter, csrc/event_filter.hip), shared by tests/test_event_filter_cpu.py
and tests/test_hip_event_filter.py; the yardstick is tests/event_filter_numpy.py.  Every expectation is bit-equal.

planted_5x7   H = 5, W = 7; every time is a multiple of U = 2^-10 s, rho = 2 U, dt = 4 U, pixel (5, 1) is hot.  One planted
              event per rule, by stream position (x, y; time in U):
                 0  (1,1) 100   first event of its pixel; kept through 1
                 1  (0,0) 100   corner; equal-time neighbour of 0: they support each other
                 2  (1,1) 102   gap exactly rho: passes; (0,0) lies 2 U back: kept
                 3  (1,1) 103   gap rho - U: REFRACTORY  (rho = 0: kept, (0,0) lies 3 U back)
                 4  (3,1) 200   nobody around: UNSUPPORTED, but it supports 5
                 5  (4,2) 204   t - t' exactly dt to 4, a supporter that is itself UNSUPPORTED: kept
                 6  (2,0) 205   t - t' = dt + U to 4: UNSUPPORTED
                 7  (1,3) 300   nobody around: UNSUPPORTED
                 8  (1,3) 301   REFRACTORY  (rho = 0: passes, UNSUPPORTED)
                 9  (0,4) 305   corner; 7 lies 5 U back, 8 lies 4 U back but is REFRACTORY and supports nobody: UNSUPPORTED
                                (rho = 0: 8 passed and supports: kept)
                10  (5,1) 400   HOT
                11  (6,0) 401   corner; its only neighbour with activity is hot: UNSUPPORTED
                12  (6,4) 500   corner; nobody around: UNSUPPORTED
                13  (6,4) 503   passes the refractory stage; its own event lies 3 U back but a pixel never supports itself:
                                UNSUPPORTED
                14  (6,2) 600   flat index 20
                15  (0,3) 600   flat index 21: adjacent in memory to 14, equal time, NOT a neighbour: both UNSUPPORTED
                16  (3,3) 700   kept through 18
                17  (3,3) 700   same pixel and time, later stream position: REFRACTORY  (rho = 0: kept)
                18  (2,4) 700   equal-time neighbour of 16: kept
                19  x = W, 20  y = H, 21  x = 65535 with t = NaN: SENSOR (before the time is looked at)
                22  t = NaN, 23  +inf, 24  -inf on (2,2), 25  +inf on the hot pixel: TIME (before the mask)
              Condition: every class occurs.
1x1           40 events on the only pixel: with support everything that passes stage 1 is UNSUPPORTED
1x300         600 events: only left and right neighbours exist
edge_N        N = 0, 1, 255, 256, 257 events on 5 x 7 (the workgroup size is 256)
37x53_noisy   the streams of 37x53_grey_K5 of tests/event_noise_cases.py under `all` (read-only), the three intervals
              concatenated: 49 679 events.  Orders: `emitted` (pixel-major per interval: neither flag holds), `time`
              (time_sorted(): the time_ordered path), `pixel_major` (a stable sort of `time` by pixel: the no-sort path; a single
              emitted interval has this order) and `shuffled` (seeded; compared through the permutation).  rho = 8e-3 s,
              dt = 5e-4 s, first values, kept.  Measured in the yardstick (test_case_conditions prints them): the refractory
              stage removes REFR_SHARE of what reaches it, the support stage SUPP_SHARE; asked for: each between 5 % and
              95 %.  Condition: no two live events share pixel and time (none do; `_dedupe` would drop them).
long_run      9 x 9, 20 000 events on pixel (4, 4) and 5 000 on its eight neighbours, shuffled: search depth and the linear walk
splits        the `time` order of 37x53_noisy cut at 1, 2 and 7 seeded points that lie between distinct times
boundary_tie  1 x 2, dt = U, rho = 0: pixel 0 at time T in the first chunk, pixel 1 at T in the second.  In one call both are
              kept; chunked, the first is UNSUPPORTED (nothing supports it yet) and the second is kept through t_seen

Measured shares of 37x53_noisy at rho = 8e-3, dt = 5e-4: REFR_SHARE = 58.4 % (28 998 of 49 679), SUPP_SHARE = 68.5 %
(14 167 of 20 681)."""
import math

import numpy as np

from tests import event_filter_numpy as YF

U = 2.0 ** -10
INF, NAN = math.inf, math.nan

PLANTED_RHO, PLANTED_DT = 2 * U, 4 * U
PLANTED_EVENTS = [                  # (time in U, x, y, p)
    (100, 1, 1, 1), (100, 0, 0, 0), (102, 1, 1, 0), (103, 1, 1, 1),
    (200, 3, 1, 1), (204, 4, 2, 0), (205, 2, 0, 1),
    (300, 1, 3, 0), (301, 1, 3, 1), (305, 0, 4, 1),
    (400, 5, 1, 1), (401, 6, 0, 0),
    (500, 6, 4, 1), (503, 6, 4, 0),
    (600, 6, 2, 1), (600, 0, 3, 1),
    (700, 3, 3, 1), (700, 3, 3, 0), (700, 2, 4, 1),
    (800, 7, 0, 1), (800, 0, 5, 0), (NAN, 65535, 0, 1),
    (NAN, 2, 2, 1), (INF, 2, 2, 0), (-INF, 2, 2, 1), (INF, 5, 1, 0),
]
K, S, T, H_, R, N_ = YF.KEPT, YF.SENSOR, YF.TIME, YF.HOT, YF.REFRACTORY, YF.UNSUPPORTED
PLANTED_EXPECTED = {                # hand-worked, see above
    'rho_support': [K, K, K, R, N_, K, N_, N_, R, N_, H_, N_, N_, N_, N_, N_, K, R, K, S, S, S, T, T, T, T],
    'rho0_support': [K, K, K, K, N_, K, N_, N_, N_, K, H_, N_, N_, N_, N_, N_, K, K, K, S, S, S, T, T, T, T],
    'rho_only': [K, K, K, R, K, K, K, K, R, K, H_, K, K, K, K, K, K, R, K, S, S, S, T, T, T, T],
}
PLANTED_SETTINGS = {'rho_support': (PLANTED_RHO, PLANTED_DT), 'rho0_support': (0.0, PLANTED_DT), 'rho_only': (PLANTED_RHO, None)}

NOISY_SOURCE = '37x53_grey_K5'
NOISY_RHO, NOISY_DT = 8e-3, 5e-4
NOISY_ORDERS = ('emitted', 'time', 'pixel_major', 'shuffled')
# which ordering path each order takes on the device, and the flag bits (1 = not time-ordered, 2 = not pixel-major)
NOISY_PATHS = {'emitted': ('unordered', 3), 'time': ('time_ordered', 2), 'pixel_major': ('pixel_major', 1), 'shuffled': ('unordered', 3)}
SPLIT_COUNTS = (1, 2, 7)
EDGE_NS = (0, 1, 255, 256, 257)

_cache = {}


def _case(H, W, t, x, y, p, rho, dt, hot_mask=None):
    return dict(H=H, W=W, t=np.ascontiguousarray(t, dtype=np.float64), x=np.ascontiguousarray(x, dtype=np.uint16),
                y=np.ascontiguousarray(y, dtype=np.uint16), p=np.ascontiguousarray(p, dtype=np.uint8), rho=rho, dt=dt,
                hot_mask=hot_mask)


def _take(c, order):
    return dict(c, t=c['t'][order], x=c['x'][order], y=c['y'][order], p=c['p'][order])


def _dedupe(c):
    """drops every live event that repeats the pixel and time of an earlier one"""
    key = np.stack([c['y'].astype(np.float64) * c['W'] + c['x'], c['t']], axis=1)
    _, first = np.unique(key, axis=0, return_index=True)
    return _take(c, np.sort(first))


def planted(setting='rho_support'):
    rho, dt = PLANTED_SETTINGS[setting]
    e = PLANTED_EVENTS
    mask = np.zeros((5, 7), dtype=np.uint8)
    mask[1, 5] = 1
    return _case(5, 7, [v[0] * U for v in e], [v[1] for v in e], [v[2] for v in e], [v[3] for v in e], rho, dt, mask)


def _random_case(seed, H, W, n, span, rho, dt, grid=None):
    rng = np.random.default_rng(seed)
    t = rng.integers(0, grid, n) * (span / grid) if grid else rng.uniform(0.0, span, n)
    return _case(H, W, t, rng.integers(0, W, n), rng.integers(0, H, n), rng.integers(0, 2, n), rho, dt)


def noisy_base():
    """37x53_noisy in the order `emitted`"""
    if 'noisy_base' not in _cache:
        from tests import event_noise_cases as NC
        steps = NC.image_noise_reference(NOISY_SOURCE, 'all')
        c = _case(37, 53, *(np.concatenate([s[k] for s in steps]) for k in 'txyp'), NOISY_RHO, NOISY_DT)
        _cache['noisy_base'] = _dedupe(c)
    return _cache['noisy_base']


def noisy(order):
    """(case, perm): case['t'] = noisy_base()['t'][perm]"""
    base = noisy_base()
    n = base['t'].shape[0]
    by_t = np.argsort(base['t'], kind='stable')
    if order == 'emitted':
        perm = np.arange(n)
    elif order == 'time':
        perm = by_t
    elif order == 'pixel_major':
        pix = base['y'].astype(np.int64) * base['W'] + base['x']
        perm = by_t[np.argsort(pix[by_t], kind='stable')]
    else:
        perm = np.random.default_rng(20261).permutation(n)
    return _take(base, perm), perm


def cases():
    """name -> case: every one-call case (read-only)"""
    if 'cases' not in _cache:
        out = {f'planted_5x7_{s}': planted(s) for s in PLANTED_SETTINGS}
        out['1x1_support'] = _random_case(11, 1, 1, 40, 1.0, 0.02, 0.5)
        out['1x1_refractory'] = dict(out['1x1_support'], dt=None)
        out['1x300'] = _random_case(12, 1, 300, 600, 1.0, 0.05, 0.01)
        out['1x300_grid'] = _random_case(13, 1, 300, 600, 1.0, 4.0 / 64, 1.0 / 64, grid=64)     # many equal times
        for n in EDGE_NS:
            out[f'edge_{n}'] = _random_case(100 + n, 5, 7, n, 1.0, 0.05, 0.02)
        for o in NOISY_ORDERS:
            out[f'37x53_noisy_{o}'] = noisy(o)[0]
        rng = np.random.default_rng(14)
        n_c, n_r = 20000, 5000
        ring = [(dx, dy) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dx, dy) != (0, 0)]
        pick = rng.integers(0, 8, n_r)
        x = np.concatenate([np.full(n_c, 4), 4 + np.array([ring[k][0] for k in pick])])
        y = np.concatenate([np.full(n_c, 4), 4 + np.array([ring[k][1] for k in pick])])
        long_run = _case(9, 9, rng.uniform(0.0, 1.0, n_c + n_r), x, y, rng.integers(0, 2, n_c + n_r), 2e-5, 1e-4)
        out['long_run'] = _take(long_run, rng.permutation(n_c + n_r))
        _cache['cases'] = out
    return _cache['cases']


def split_points(count):
    """`count` seeded cut positions of the `time` order of 37x53_noisy, each between two distinct times"""
    t = noisy('time')[0]['t']
    ok = np.flatnonzero(t[1:] > t[:-1]) + 1
    return np.sort(np.random.default_rng(300 + count).choice(ok, count, replace=False)).tolist()


def boundary_tie():
    """(chunks, one-call expectation, chunked expectation): see the docstring"""
    T0 = 5 * U
    first, second = _case(1, 2, [T0], [0], [0], [1], 0.0, U), _case(1, 2, [T0], [1], [0], [0], 0.0, U)
    return [first, second], [K, K], [N_, K]


def run_yardstick(chunks):
    """The yardstick over a list of chunks of one stream with carried state: dict with classes / kept (per chunk), the kept
    events of all chunks as arrays t, x, y, p, counters (summed), t_last, t_seen (float64 [H,W]) and the stage figures."""
    c0 = chunks[0]
    state = YF.FilterState(c0['H'], c0['W'])
    mask = None if c0['hot_mask'] is None else c0['hot_mask'].tolist()
    res = [YF.filter_chunk(state, c['t'].tolist(), c['x'].tolist(), c['y'].tolist(), c['p'].tolist(), c['rho'],
                           c['dt'] is not None, c['dt'] if c['dt'] is not None else 0.0, mask) for c in chunks]
    out = dict(classes=[np.array(r['classes'], dtype=np.uint8) for r in res], kept=[np.array(r['kept'], dtype=np.int64) for r in res])
    for k in 'txyp':
        out[k] = np.concatenate([c[k][kept] for c, kept in zip(chunks, out['kept'])])
    out['counters'] = {k: sum(r['counters'][k] for r in res) for k in res[0]['counters']}
    out['t_last'] = np.array(state.plane('t_last'), dtype=np.float64).reshape(c0['H'], c0['W'])
    out['t_seen'] = np.array(state.plane('t_seen'), dtype=np.float64).reshape(c0['H'], c0['W'])
    for k in ('reached_refractory', 'removed_refractory', 'reached_support', 'removed_support'):
        out[k] = sum(r[k] for r in res)
    return out


def reference(name):
    """the yardstick's one-call result of cases()[name], once per process (read-only)"""
    key = ('ref', name)
    if key not in _cache:
        _cache[key] = run_yardstick([cases()[name]])
    return _cache[key]


def cut(case, points):
    """the chunks of a case cut at the stream positions `points`"""
    edges = [0] + list(points) + [case['t'].shape[0]]
    return [_take(case, slice(a, b)) for a, b in zip(edges[:-1], edges[1:])]
