"""Seeded inputs for the tracker-tail tests (tests/test_tracker_tail_cpu.py, tests/test_hip_tracker_tail.py), built once per
process and read-only, and the conditions the tests lean on, asserted from the yardstick alone (tests/tracker_tail_numpy.py).

FULL cases (the device composites): raw and z are rows of tests/composite_cases.make -- ray r takes pattern mix[r mod len(mix)]
of  a unsaturated, b one out-of-bound 100, c a closed run of six 100s, d empty, e near-saturated samples.
  gt_depth = depth + s t sqrt(var + 1e-10) rounded to float32, so that tmp is t up to that rounding: t in [0.5, 2] on ordinary
      rays, t in [60, 200] on the OUTLIERS (r mod 7 == 3: the rays the median mask drops although gt_depth > 0), exactly 0 on
      r mod 9 == 1 (these rays enter the median with tmp = depth / sqrt(var + 1e-10) and are never `on`).  On closed rays the
      root is ~1e-5, so their gt_depth is a few float32 ulps off the depth and tmp is coarse but decided.
  gt_color = rgb + an offset of 0.2 ... 0.7 of either sign, or absent.
  inside: NULL, scattered (r mod 3 != 2), everything but one 16-ray block, only the last ray, none.
  Duplicated rays (the `dup` cases): the tail composites a ray with one wave from the ray's own data only -- every cross-lane
      step is a shuffle inside that wave, the ray's index only selects addresses -- so copies of a ray have the same bits of
      depth, var, rgb and tmp wherever they sit; a third of the batch is one ray copied, placed so that the run of equal tmp
      straddles the median.  This is the only way to a tie in device-computed tmp.
Near-saturated patterns (e, and f = abcde) have forward bars that are large behind the saturated sample; they run with
handle_dynamic off, and with it on where the fragility rule still decides every ray (check_conditions asserts it).

EXACT cases (loss_only: the test writes tmp, depth, var, rgb): see exact_cases."""
import functools

import numpy as np

from tests import composite_cases as CC
from tests import tracker_tail_numpy as T

N_EDGES = (1, 2, 15, 16, 17, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049,
           4095, 4096)
S_LIST = (1, 15, 16, 17, 48, 63, 64)
S_AT = (33, 257)
INSIDE_KINDS = ('null', 'scattered', 'block', 'last', 'none')


def inside_mask(kind, N):
    """uint8 [N] or None"""
    r = np.arange(N)
    if kind == 'null':
        return None
    if kind == 'scattered':
        m = r % 3 != 2
    elif kind == 'block':                       # everything but the second 16-ray block (a batch of one block: scattered)
        m = (r // 16) != 1 if N > 16 else r % 3 != 2
    elif kind == 'last':
        m = r == N - 1
    else:
        m = np.zeros(N, bool)
    return m.astype(np.uint8)


def outlier(r):
    return r % 7 == 3


def zero_depth(r):
    return r % 9 == 1


@functools.lru_cache(maxsize=None)
def _rows(S, N, mix):
    parts = {p: CC.make(S, N, p, seed=3) for p in set(mix)}
    raw = np.stack([parts[mix[r % len(mix)]]['raw'][r] for r in range(N)])
    z = np.stack([parts[mix[r % len(mix)]]['z'][r] for r in range(N)])
    return raw, z


def make(N, S, mix, dynamic, inside, colour, w, dup=False):
    """dict(name, N, S, raw, z, gd, gc, w, inside, dynamic, y: the yardstick's tail, b: its bars)"""
    raw, z = _rows(S, N, mix)
    raw, z = raw.copy(), z.copy()
    if dup:                                     # one ray copied into a third of the batch, spread over the workgroups
        src = 0
        for r in range(N):
            if r % 3 == 2:
                raw[r], z[r] = raw[src], z[src]
    rng = np.random.default_rng([11, N, S, len(mix), int(dynamic)])
    f = T.Y.forward(raw, z)
    root = np.sqrt(f['var'] + T.EPS)
    r = np.arange(N)
    t = rng.uniform(0.5, 2.0, N)
    t[outlier(r)] = rng.uniform(60.0, 200.0, int(outlier(r).sum()))
    s = np.where((f['depth'] - 1.05 * t * root < 0.05) | (rng.uniform(size=N) < 0.5), 1.0, -1.0)
    if dup:                                     # the copies share gt too; t = 1.25 puts their tmp in the middle of [0.5, 2]
        cp = r % 3 == 2
        t[cp], s[cp] = 1.25, 1.0
        t[src], s[src] = 1.25, 1.0
    gd = (f['depth'] + s * t * root).astype(np.float32)
    gd[zero_depth(r)] = 0.0
    gc = None
    if colour:
        off = rng.uniform(0.2, 0.7, (N, 3)) * np.where(rng.uniform(size=(N, 3)) < 0.5, 1.0, -1.0)
        if dup:
            off[cp] = off[src]
        gc = (f['rgb'] + off).astype(np.float32)
    ins = inside_mask(inside, N)
    y = T.tail(raw, z, gd, gc, w, ins, dynamic)
    name = f"N{N}-S{S}-{mix}-{'dyn' if dynamic else 'static'}-{inside}-{'w%g' % w if colour else 'nocolour'}{'-dup' if dup else ''}"
    for a in (raw, z, gd) + (() if gc is None else (gc,)) + (() if ins is None else (ins,)):
        a.setflags(write=False)
    return dict(name=name, N=N, S=S, mix=mix, raw=raw, z=z, gd=gd, gc=gc, w=w, inside=ins, inside_kind=inside,
                dynamic=dynamic, dup=dup, y=y, b=T.bars(y))


@functools.lru_cache(maxsize=None)
def full_cases():
    out = []
    for i, N in enumerate(N_EDGES):             # every batch-size edge at S = 16
        kind = ('null', 'scattered', 'block')[i % 3]
        out.append(make(N, 16, 'abcd', 1, kind, i % 4 != 3, (0.5, 0.2)[i % 2]))
        out.append(make(N, 16, 'abcde', 0, ('scattered', 'block', 'null')[i % 3], i % 4 != 1, (0.2, 0.5)[i % 2]))
    for N in (17, 1024, 1025, 4096):            # one inside ray; none
        out.append(make(N, 16, 'abcd', 1, 'last', True, 0.5))
        out.append(make(N, 16, 'abcd', 1, 'none', True, 0.2))
    out.append(make(17, 16, 'abcd', 0, 'none', True, 0.2))
    out.append(make(17, 16, 'abcd', 0, 'last', False, 0.2))
    for N in S_AT:                              # every sample-count edge
        for j, S in enumerate(S_LIST):
            # (S = 1 under the mask: unsaturated and empty rays only.  A closed one-sample ray has var = 0 exactly, and with
            # gt_depth = 0 its tmp = depth / 1e-5 carries a bar of ~1e2, which as B would leave every ray undecided.)
            out.append(make(N, S, 'abcd' if S > 1 else 'ad', 1, ('null', 'scattered')[j % 2], j % 3 != 2, (0.5, 0.2)[j % 2]))
            out.append(make(N, S, 'abcde', 0, ('scattered', 'null')[j % 2], j % 3 != 0, (0.2, 0.5)[j % 2]))
    for N in (200, 1500):                       # ties in device-computed tmp, in both median shapes
        out.append(make(N, 16, 'a', 1, 'null', True, 0.5, dup=True))
    for N in DYN_NEAR_SATURATED:                # near-saturated samples under the median mask, where the rule holds
        out.append(make(N, 16, 'abcde', 1, 'null', True, 0.5))
    return tuple(out)


DYN_NEAR_SATURATED = (17, 63, 65)


def check_conditions(c):
    """every condition the full-tail tests lean on, from the yardstick alone"""
    y, b, N, S = c['y'], c['b'], c['N'], c['S']
    assert c['raw'].dtype == np.float32 and c['raw'].shape == (N, S, 4) and c['z'].dtype == np.float64 and c['z'].shape == (N, S)
    assert c['gd'].dtype == np.float32 and (c['gc'] is None or c['gc'].dtype == np.float32)
    assert c['inside'] is None or (c['inside'].dtype == np.uint8 and c['inside'].shape == (N,))
    assert np.isfinite(y['tmp']).all() and np.isfinite(b['tmp']).all() and np.isfinite(b['d_raw']).all()
    assert b['undecided'] == 0, (c['name'], b['undecided'], b['B'], y['med'])          # THE condition: see T's fragility rule
    r = np.arange(N)
    assert ((c['gd'] == 0) == zero_depth(r)).all() and (c['gd'] >= 0).all()
    ins, can = y['inside'], y['inside'] & (c['gd'] > 0)
    if c['dynamic'] and c['inside_kind'] in ('null', 'scattered', 'block') and N >= 15:
        dropped, kept = int((can & ~y['keep']).sum()), int(y['on'].sum())
        assert 0 < dropped < kept, (c['name'], dropped, kept)                           # the mask drops rays with gd > 0
        assert (can & ~y['keep'] & outlier(r)).any()
        assert (ins & (c['gd'] == 0)).any()                                            # gd == 0 rays enter the median
    if not c['dynamic']:
        assert (y['keep'] == ins).all()
    if c['inside_kind'] == 'none':
        assert y['med'] == np.inf and not y['on'].any() and y['loss'] == 0.0 and not y['d_raw'].any()
    if c['inside_kind'] == 'last':
        assert ins.sum() == 1 and ins[-1] and (not c['dynamic'] or y['med'] == y['tmp'][-1])
        assert int(y['on'].sum()) == int(c['gd'][-1] > 0)
    if c['dup']:
        cp = np.nonzero(r % 3 == 2)[0]
        assert len(cp) >= N // 3 and (y['tmp'][cp] == y['tmp'][0]).all() and y['med'] == y['tmp'][0]
        assert (y['tmp'] < y['med']).sum() >= 8 and (y['tmp'] > y['med']).sum() >= 8
        assert len(set((cp // 16).tolist())) >= 4                                      # spread over workgroups
    assert not y['d_raw'][~y['on']].any()
    if 'e' in c['mix'] and N >= 5:
        x = np.float32(10.0) * c['raw'][..., 3]
        assert ((x >= 12.0) & (x <= 20.0)).any()


# ------------------------------------------------------------------------------------------------ exact decisions (loss_only)
def _place(rng, N, vals, decoys, pos=None):
    """tmp [N] with the multiset `vals` at `pos` (default: len(vals) positions drawn by rng) in shuffled order, inside = those
    positions (None when they are all N), the other entries cycling through `decoys`"""
    c = len(vals)
    pos = np.sort(rng.choice(N, c, replace=False)) if pos is None else np.asarray(pos)
    tmp = np.empty(N, np.float64)
    rest = np.setdiff1d(np.arange(N), pos)
    tmp[rest] = [decoys[i % len(decoys)] for i in range(len(rest))]
    tmp[pos] = rng.permutation(np.asarray(vals, np.float64))
    ins = np.zeros(N, np.uint8)
    ins[pos] = 1
    return tmp, (None if c == N else ins)


@functools.lru_cache(maxsize=None)
def exact_cases(N):
    """tuple of dict(name, tmp f64 [N], gd f32 [N], inside uint8 [N] or None, med, keep, on): tmp arrays a test hands to the
    loss_only route; med / keep / on are tracker_tail_numpy.decide's.  The decoys (entries outside the mask) are values that
    would change the outcome if the mask were ignored."""
    rng = np.random.default_rng([5, N])
    out = []

    def add(name, tmp, inside, gd=None, kept=None):
        gd = np.full(N, 2.0, np.float32) if gd is None else gd
        med, keep, on = T.decide(tmp, gd, inside)
        if kept is not None:
            assert int(on.sum()) == kept, (name, N, int(on.sum()))
        for a in (tmp, gd) + (() if inside is None else (inside,)):
            a.setflags(write=False)
        out.append(dict(name=name, N=N, tmp=tmp, gd=gd, inside=inside, med=med, keep=keep, on=on))

    sc = inside_mask('scattered', N) if N >= 3 else None
    c_sc = N if sc is None else int(sc.sum())
    pos_sc = np.arange(N) if sc is None else np.nonzero(sc)[0]

    # distinct random values, a fifth of them beyond ten medians, gd == 0 on some
    tmp = rng.uniform(0.1, 3.0, N) * np.where(rng.uniform(size=N) < 0.2, 30.0, 1.0)
    gd = np.where(rng.uniform(size=N) < 0.15, 0.0, 2.0).astype(np.float32)
    add('distinct', tmp, sc, gd)
    add('distinct, no mask', tmp.copy(), None)
    # all equal: every ray is the median, and 1 < 10
    add('all equal', np.ones(N), None, kept=N)
    add('all equal, masked', *_place(rng, N, np.ones(c_sc), (0.01, 500.0), pos_sc), kept=c_sc)
    # two values 1 and 20 (20 is not below 10 * 1; everything is below 10 * 20): k ones
    mid = (N - 1) // 2
    for k in sorted({min(max(k, 0), N) for k in (mid, mid + 1, mid + 2)}):
        tmp, ins = _place(rng, N, [1.0] * k + [20.0] * (N - k), (1.0,))
        add(f'two values, {k} low', tmp, ins, kept=k if k > mid else N)
    # runs of ties around the median, masked entries interleaved
    lo, hi = c_sc // 3, c_sc // 4
    vals = np.concatenate([rng.uniform(0.1, 0.9, lo), np.ones(c_sc - lo - hi), rng.uniform(2.0, 9.0, hi // 2),
                           rng.uniform(11.0, 100.0, hi - hi // 2)])
    tmp, ins = _place(rng, N, vals, (1.0, 0.001, 500.0), pos_sc)
    gd = np.where(np.arange(N) % 5 == 4, 0.0, 2.0).astype(np.float32)
    add('tie run at the median', tmp, ins, gd)
    assert out[-1]['med'] == 1.0
    # med == 0: tmp < 0 is false for every ray
    nz = c_sc // 2 + 1
    tmp, ins = _place(rng, N, np.concatenate([np.zeros(nz), rng.uniform(0.5, 5.0, c_sc - nz)]), (1.0,), pos_sc)
    add('median zero', tmp, ins, kept=0)
    assert out[-1]['med'] == 0.0
    # the gd == 0 rays hold the lower half: they set the median (0.1), and no gd > 0 ray (5.0) is below ten times it
    low = np.arange(N) % 2 == 0
    add('gd == 0 rays set the median', np.where(low, 0.1, 5.0), None, np.where(low, 0.0, 2.0).astype(np.float32), kept=0)
    # kept counts 0, 1, 2, even, odd: few inside rays among decoys of 1.5 (kept if they counted)
    add('kept 0: nothing inside', np.full(N, 1.5), np.zeros(N, np.uint8), kept=0)
    for kept, vals in ((1, [1.0]), (1, [1.0, 20.0]), (2, [1.0, 5.0]), (2, [1.0, 2.0, 50.0]), (4, [1.0, 2.0, 3.0, 4.0, 100.0]),
                       (5, [1.0, 2.0, 3.0, 4.0, 5.0, 100.0])):
        if len(vals) <= N:
            pos = np.sort(rng.choice(N - 1, len(vals) - 1, replace=False)) if len(vals) > 1 else np.zeros(0, int)
            tmp, ins = _place(rng, N, vals, (1.5,), np.concatenate([pos, [N - 1]]).astype(int))     # the last ray is inside
            add(f'kept {kept} of {len(vals)} inside', tmp, ins, kept=kept)
    # exactly 10 * med (not kept) and one ulp below (kept): med = 1.5, 15.0 = 10 * 1.5 exactly in float64
    if N >= 4:
        m = (N - 1) // 2
        rest = N - m - 3
        vals = np.concatenate([rng.uniform(0.5, 1.4, m), [1.5, 15.0, np.nextafter(15.0, 0.0)], rng.uniform(2.0, 14.0, rest // 2),
                               rng.uniform(16.0, 40.0, rest - rest // 2)])
        tmp, ins = _place(rng, N, vals, (1.0,))
        add('ten times the median', tmp, ins, kept=m + 2 + rest // 2)
        e = out[-1]
        assert e['med'] == 1.5 and 10.0 * e['med'] == 15.0
        assert not e['keep'][tmp == 15.0].any() and e['keep'][tmp == np.nextafter(15.0, 0.0)].all()
    # +inf among the values: a few (the median is finite, inf is not kept), most (the median is inf: the finite ones are kept)
    if c_sc >= 3:
        ni = max(1, c_sc // 5)
        tmp, ins = _place(rng, N, np.concatenate([rng.uniform(0.5, 4.0, c_sc - ni), np.full(ni, np.inf)]), (1.0, np.inf), pos_sc)
        add('a few inf', tmp, ins, kept=c_sc - ni)
    nf = (c_sc - 1) // 2
    tmp, ins = _place(rng, N, np.concatenate([rng.uniform(0.5, 4.0, nf), np.full(c_sc - nf, np.inf)]), (1.0,), pos_sc)
    add('mostly inf', tmp, ins, kept=nf)
    assert out[-1]['med'] == np.inf
    return tuple(out)
