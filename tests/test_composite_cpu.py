"""The compositing yardstick (tests/composite_numpy.py) checked without a GPU: against float64 autograd of the reference
formula, against the float32 oracle, for finiteness on saturated rays, for the case conditions of tests/composite_cases.py,
and for sensitivity -- the derived bar must reject every structural variant of the yardstick that a faulty kernel could
compute (tests/test_hip_composite.py compares the kernels against the same bar)."""
import numpy as np
import pytest
import torch

from tests import composite_cases as C
from tests import composite_numpy as Y

CASES = {(c['S'], c['N'], c['pattern']): c for c in C.all_cases()}


def _cot(c):
    return c['g_depth'], c['g_var'], c['g_rgb']


def _torch64(c, cots):
    """float64 autograd of the reference formula; the leaf is x = 10 occ (the float32 product), so d_occ = 10 dx"""
    raw = torch.from_numpy(c['raw'])
    x = (np.float32(10.0) * raw[..., 3]).double().requires_grad_(True)
    col = raw[..., :3].double().requires_grad_(True)
    z = torch.from_numpy(c['z'])
    alpha = torch.sigmoid(x)
    trans = torch.cumprod(torch.cat([torch.ones_like(alpha[:, :1]), 1. - alpha + Y.C32], -1), -1)[:, :-1]
    w = alpha * trans
    rgb = (w.unsqueeze(-1) * col).sum(-2)
    depth = (w * z).sum(-1)
    dz = z - depth.unsqueeze(-1)
    var = (w * dz * dz).sum(1)
    gD, gV, gC = cots
    tot = 0
    if gD is not None:
        tot = tot + (depth * torch.from_numpy(gD)).sum()
    if gV is not None:
        tot = tot + (var * torch.from_numpy(gV)).sum()
    if gC is not None:
        tot = tot + (rgb * torch.from_numpy(gC).double()).sum()
    tot.backward()
    d = torch.cat([torch.zeros_like(col) if col.grad is None else col.grad, 10.0 * x.grad.unsqueeze(-1)], -1)
    return {k: v.detach().numpy() for k, v in dict(w=w, depth=depth, var=var, rgb=rgb).items()}, d.numpy()


@pytest.mark.parametrize("pattern", ['a', 'd'])
def test_agrees_with_float64_autograd(pattern):
    """forward and backward (each cotangent alone and all together) equal torch.autograd in float64 to 1e-12 of scale
    where nothing saturates (autograd's 1 - alpha cancels and its cumprod backward divides)"""
    for S in C.S_LIST:
        for N in (1, 17):
            c = CASES[S, N, pattern]
            gD, gV, gC = _cot(c)
            for cots in ((gD, None, None), (None, gV, None), (None, None, gC), (gD, gV, gC)):
                ft, dt = _torch64(c, cots)
                scales, _, _ = Y.forward_bars(c['f'])
                for k in ('w', 'depth', 'var', 'rgb'):
                    assert (np.abs(ft[k] - c['f'][k]) <= 1e-12 * scales[k] + 1e-300).all(), (S, N, k)
                d = Y.backward(c['raw'], c['z'], *cots, f=c['f'])
                scale, _ = Y.backward_bars(c['f'], *cots)
                assert (np.abs(d - dt) <= 1e-12 * scale + 1e-300).all(), (S, N)


def test_agrees_with_the_float32_oracle():
    """oracle.render_oracle.composite (float32 torch ops, sequential cumprod) lies within the float32 bar of the yardstick
    on every case; its autograd gradient on the unsaturated ones"""
    from oracle import render_oracle as R
    for c in CASES.values():
        raw = torch.from_numpy(c['raw']).requires_grad_(c['pattern'] == 'a')
        depth, var, rgb, w = R.composite(raw, torch.from_numpy(c['z']))
        _, bars, _ = Y.forward_bars(c['f'])
        got = dict(w=w, depth=depth, var=var, rgb=rgb)
        for k in got:
            err = np.abs(got[k].detach().double().numpy() - c['f'][k])
            assert (err <= bars[k]).all(), (c['S'], c['N'], c['pattern'], k, float((err / bars[k]).max()))
        if c['pattern'] == 'a':
            gD, gV, gC = _cot(c)
            ((depth * torch.from_numpy(gD)).sum() + (var * torch.from_numpy(gV)).sum()
             + (rgb * torch.from_numpy(gC)).sum().double()).backward()
            d = Y.backward(c['raw'], c['z'], gD, gV, gC, f=c['f'])
            _, bar = Y.backward_bars(c['f'], gD, gV, gC)
            # the oracle's depth inside var's tmp is its own float32-weight depth, not the yardstick's: its share is
            # within the depth bar's effect on gw, (2 |gV| (|tmp| + sum w |tmp|) dbar) |z| per sample, far below `bar` here
            err = np.abs(raw.grad.double().numpy() - d)
            assert (err <= 2 * bar).all(), (c['S'], c['N'], float((err / bar).max()))


def test_backward_is_finite_on_saturated_rays():
    for c in CASES.values():
        if C.saturated(c):
            d = Y.backward(c['raw'], c['z'], *_cot(c), f=c['f'])
            scale, bar = Y.backward_bars(c['f'], *_cot(c))
            assert np.isfinite(d).all() and np.isfinite(scale).all() and np.isfinite(bar).all()
            _, fb, _ = Y.forward_bars(c['f'])
            assert all(np.isfinite(v).all() for v in fb.values())
            occ100 = c['raw'][..., 3] == 100.0
            assert (d[..., 3][occ100] == 0).all()                       # sigmoid'(1000) is exactly 0 in float64 too


def test_case_conditions():
    n = 0
    for c in CASES.values():
        C.check_conditions(c)
        n += 1
    assert n == len(C.S_LIST) * len(C.N_LIST) * len(C.PATTERNS)
    for S in C.LIST_S:
        assert S in C.S_LIST


# ------------------------------------------------------------------------------------------------ sensitivity
def _pad_last(a, axis):
    pad = [(0, 0)] * a.ndim
    pad[axis] = (0, 1)
    return np.pad(a, pad)


def _variants(c):
    """name -> (forward dict or None, d_raw or None) of each faulty restatement, all cotangents together"""
    raw, z, f = c['raw'], c['z'], c['f']
    cots = _cot(c)
    out = {}
    if c['S'] > 1:
        fd = Y.forward(raw[:, :-1], z[:, :-1])
        dd = Y.backward(raw[:, :-1], z[:, :-1], *cots, f=fd)
        out['last sample dropped'] = (dict(w=_pad_last(fd['w'], 1), depth=fd['depth'], var=fd['var'], rgb=fd['rgb']),
                                      _pad_last(dd, 1))
    else:                                                             # nothing is left of a one-sample ray
        out['last sample dropped'] = ({k: np.zeros_like(f[k]) for k in ('w', 'depth', 'var', 'rgb')}, np.zeros(raw.shape))
    fi = Y.forward(raw, z, inclusive=True)
    out['inclusive transmittance'] = (fi, Y.backward(raw, z, *cots, f=fi))
    out['suffix sum including j'] = (None, Y.backward(raw, z, *cots, f=f, suffix_incl=True))
    out['-2 gV sum(w tmp) left out'] = (None, Y.backward(raw, z, *cots, f=f, no_depth_term=True))
    out["g_var's tmp^2 left out"] = (None, Y.backward(raw, z, *cots, f=f, no_tmp2=True))
    if (raw[..., 3] == 100.0).any():         # closed samples only: behind a near-saturated one float32 cannot see 1e-10
        f0 = Y.forward(raw, z, plus=0.0)
        out['1e-10 left out of m'] = (f0, Y.backward(raw, z, *cots, f=f0))
    if c['N'] >= 2:
        sw = np.arange(c['N'])
        sw[-2:] = sw[-2:][::-1]
        out['rays N-1 and N-2 swapped'] = ({k: f[k][sw] for k in ('w', 'depth', 'var', 'rgb')},
                                           Y.backward(raw, z, *cots, f=f)[sw])
    return out


def _floor(c, scale):
    """what a difference must exceed, besides 1e-3 of its element's scale, to count as one a float32 kernel could show:
    1e-30 (the normal range), and on rays with a near-saturated sample (10 occ in [12, 20]) 8 u of the ray's largest scale:
    an absolute error of 2 u in that one factor 1 - alpha moves every element behind it by about 2 u of the ray's terms"""
    x = np.float32(10.0) * c['raw'][..., 3]
    near = ((x >= 12.0) & (x <= 20.0)).any(-1)
    fl = np.full(scale.shape, 1e-30)
    if scale.ndim >= 2 and scale.shape[1] == c['S']:
        fl = fl + 8 * Y.U * scale.max(1, keepdims=True) * near.reshape((-1,) + (1,) * (scale.ndim - 1))
    return fl


def _exceeds(c, fwd, d, bars, dbar, ref_d, factor_of=None):
    """does the variant leave the bar (factor_of None), or 1e-3 of the scale + _floor (factor_of = scales), in any element"""
    hit = False
    if fwd is not None:
        for k in ('w', 'depth', 'var', 'rgb'):
            lim = bars[k] if factor_of is None else 1e-3 * factor_of[0][k] + _floor(c, factor_of[0][k])
            hit = hit or bool((np.abs(fwd[k] - c['f'][k]) > lim).any())
    lim = dbar if factor_of is None else 1e-3 * factor_of[1] + _floor(c, factor_of[1])
    return hit or bool((np.abs(d - ref_d) > lim).any())


def test_bar_rejects_every_variant():
    """A variant APPLIES to a case when its exact float64 result differs from the yardstick's by more than 1e-3 of an
    element's scale plus the floor of _floor somewhere; else it is the same function as far as float32 can tell: an
    inclusive scan of all-ones, a dropped sample of weight 0 or behind a sample that float32 cannot resolve.  On every case where it applies the bar must reject it in at least one element; the variants must apply
    where the mathematics says they do, so that the statement is not empty."""
    applied = {}
    for key, c in CASES.items():
        scales, bars, _ = Y.forward_bars(c['f'])
        ref_d = Y.backward(c['raw'], c['z'], *_cot(c), f=c['f'])
        dscale, dbar = Y.backward_bars(c['f'], *_cot(c))
        for name, (fwd, d) in _variants(c).items():
            if _exceeds(c, fwd, d, bars, dbar, ref_d, factor_of=(scales, dscale)):
                applied.setdefault(name, set()).add(key)
                assert _exceeds(c, fwd, d, bars, dbar, ref_d), (name, key)
    for S in C.S_LIST:
        for N in C.N_LIST:
            # nothing saturates in pattern a: these three differ at every shape
            for name in ('last sample dropped', 'inclusive transmittance', 'suffix sum including j'):
                assert (S, N, 'a') in applied[name], (name, S, N)
            if N >= 2:
                assert (S, N, 'a') in applied['rays N-1 and N-2 swapped']
            # the two g_var terms need a ray whose g_var is not small against its g_depth; sum(w tmp) = depth * (the
            # ray's final transmittance) needs an open ray besides: the thin odd rays
            if N >= 15:
                assert (S, N, 'a') in applied["g_var's tmp^2 left out"], (S, N)
                assert (S, N, 'a') in applied['-2 gV sum(w tmp) left out'], (S, N)
            # a closed sample with a sample behind it: ray 0 of pattern b (position 0) and pattern c
            if S >= 2:
                for p in 'bc':
                    assert (S, N, p) in applied['1e-10 left out of m'], (S, N, p)
    print({k: len(v) for k, v in applied.items()}, 'of', len(CASES))
