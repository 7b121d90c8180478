"""Seeded inputs for the compositing tests (tests/test_composite_cpu.py, tests/test_hip_composite.py) and the conditions
they rely on, asserted from the float64 yardstick alone (tests/composite_numpy.py).

Shapes: S = 1 and 64 (the most one wave composites), both sides of every 16-sample tile, 28 (the padded-tile count the renderer
composites), crossed with N on both sides of the 16-rays-per-workgroup form.
Patterns (occupancy = raw[..., 3]; 10 * occupancy is the sigmoid's argument):
  a  unsaturated: even rays dense (|10 occ| <= 2, the ray closes within a few samples), odd rays thin (10 occ in [-6, -3]: the ray
     stays open, sum w < 1, which is where the -2 g_var sum(w tmp) term of the backward is not negligible)
  b  a, with one sample at 100 (an out-of-bound sample): first, middle or last position by ray index mod 3
  c  a, with a run of six at 100: six factors of 1e-10 are 0 in float32 in any product order
  d  all at -100: alpha is exactly 0
  e  a, with samples whose 10 occ lies in [12, 20]: 1 - alpha at the granularity of float32
  f  ray r takes pattern 'abcde'[r mod 5]"""
import numpy as np

from tests import composite_numpy as Y

S_LIST = (1, 2, 15, 16, 17, 28, 32, 33, 48, 63, 64)
N_LIST = (1, 15, 16, 17, 33)
LIST_S = (16, 32, 48, 64)
PATTERNS = 'abcdef'
W_COLOR = 0.2


def run_start(S):
    """first sample of pattern c's run of six (the whole ray where S <= 6)"""
    return max(0, min(S // 3, S - 6))


def _occ(rng, S, pattern, r):
    occ = rng.uniform(-0.6, -0.3, S) if r % 2 == 1 else rng.uniform(-0.2, 0.2, S)
    if pattern == 'b':
        occ[(0, S // 2, S - 1)[r % 3]] = 100.0
    elif pattern == 'c':
        occ[run_start(S):run_start(S) + 6] = 100.0
    elif pattern == 'd':
        occ[:] = -100.0
    elif pattern == 'e':
        near = rng.uniform(size=S) < 0.15
        near[rng.integers(S)] = True
        occ[near] = rng.uniform(1.2, 2.0, int(near.sum()))
    return occ


def ray_pattern(pattern, r):
    return 'abcde'[r % 5] if pattern == 'f' else pattern


def zero_colour(r):
    return r % 4 == 2


def masked(r):
    """gt_depth 0 (r mod 5 == 1) or negative (r mod 5 == 3): the depth term skips the ray"""
    return r % 5 in (1, 3)


def make(S, N, pattern, seed=0):
    """dict(raw f32 [N,S,4], z f64 [N,S], gt_depth f32 [N], gt_color f32 [N,3], g_depth f64 [N], g_var f64 [N], g_rgb f32 [N,3],
    f: the yardstick's forward, loss: its mapper loss with W_COLOR)"""
    rng = np.random.default_rng([seed, S, N, PATTERNS.index(pattern)])
    raw = np.empty((N, S, 4), np.float32)
    raw[..., :3] = rng.uniform(0.0, 1.0, (N, S, 3))
    for r in range(N):
        raw[r, :, 3] = _occ(rng, S, ray_pattern(pattern, r), r)
        if zero_colour(r):
            raw[r, :, :3] = 0.0
    z = np.sort(rng.uniform(0.1, 6.0, (N, S)), -1)
    f = Y.forward(raw, z)
    off = rng.uniform(0.3, 1.3, N) * np.where((f['depth'] < 1.5) | (rng.uniform(size=N) < 0.5), 1.0, -1.0)
    gt_depth = (f['depth'] + off).astype(np.float32)
    coff = rng.uniform(0.2, 0.7, (N, 3)) * np.where(rng.uniform(size=(N, 3)) < 0.5, 1.0, -1.0)
    gt_color = (f['rgb'] + coff).astype(np.float32)
    for r in range(N):
        if masked(r):
            gt_depth[r] = 0.0 if r % 5 == 1 else -1.0
        if zero_colour(r):
            gt_color[r] = 0.0
    c = dict(S=S, N=N, pattern=pattern, raw=raw, z=z, gt_depth=gt_depth, gt_color=gt_color, f=f,
             g_depth=rng.standard_normal(N), g_var=0.1 * rng.standard_normal(N),
             g_rgb=rng.standard_normal((N, 3)).astype(np.float32))
    c['loss'] = Y.mapper_loss(f, gt_depth, gt_color, W_COLOR)
    c['loss_depth_only'] = Y.mapper_loss(f, gt_depth)
    return c


def all_cases(s_list=S_LIST, n_list=N_LIST, patterns=PATTERNS):
    for S in s_list:
        for N in n_list:
            for p in patterns:
                yield make(S, N, p)


def saturated(c):
    """patterns whose rays hold a sample with m = 1e-10 exactly or 1 - alpha near float32's granularity"""
    return c['pattern'] in 'bcef'


def check_conditions(c):
    """every condition the tests lean on, from the reference alone"""
    S, N, raw, z, f = c['S'], c['N'], c['raw'], c['z'], c['f']
    assert raw.dtype == np.float32 and z.dtype == np.float64 and raw.shape == (N, S, 4) and z.shape == (N, S)
    assert (np.diff(z, axis=-1) >= 0).all() and z.min() >= 0.1 and z.max() <= 6.0
    x32 = np.float32(10.0) * raw[..., 3]
    with np.errstate(over='ignore'):
        a32 = np.float32(1.0) / (np.float32(1.0) + np.exp(-x32, dtype=np.float32))        # the kernels' alpha
    six = np.float32(1.0)
    for _ in range(6):
        six = six * np.float32(Y.C32)
    assert six == 0.0                                                 # a run of six closes the ray exactly
    for r in range(N):
        p, xr = ray_pattern(c['pattern'], r), x32[r]
        plain = ((xr >= -6.0) & (xr <= -3.0)) if r % 2 == 1 else (np.abs(xr) <= 2.0)
        if p == 'a':
            assert plain.all()
        elif p == 'b':
            pos = (0, S // 2, S - 1)[r % 3]
            assert raw[r, pos, 3] == 100.0 and a32[r, pos] == 1.0 and np.delete(plain, pos).all()
        elif p == 'c':
            s0 = run_start(S)
            assert (raw[r, s0:s0 + 6, 3] == 100.0).all() and (a32[r, s0:s0 + 6] == 1.0).all()
            assert np.delete(plain, np.arange(s0, min(S, s0 + 6))).all()
            if S >= s0 + 6:
                assert (f['T'][r, s0 + 6:] <= 1.1e-60).all()
        elif p == 'd':
            assert (raw[r, :, 3] == -100.0).all() and (a32[r] == 0.0).all() and (f['w'][r] <= 1e-300).all()
        elif p == 'e':
            near = (xr >= 12.0) & (xr <= 20.0)
            assert near.any() and (near | plain).all()
        if zero_colour(r):
            assert (raw[r, :, :3] == 0).all() and (c['gt_color'][r] == 0).all()
        assert (c['gt_depth'][r] <= 0) == masked(r)
    if N >= 4:
        assert (c['gt_depth'] == 0).any() and (c['gt_depth'] < 0).any()
    # sign margins: above 100 forward bars, or exactly 0 by construction (zero colour against gt_color = 0)
    _, bars, _ = Y.forward_bars(f)
    L = c['loss']
    assert (L['margin_depth'] > 100 * bars['depth']).all()
    for r in range(N):
        if zero_colour(r):
            assert (L['margin_rgb'][r] == 0).all() and (f['rgb'][r] == 0).all()
        else:
            assert (L['margin_rgb'][r] > 100 * bars['rgb'][r]).all()
