"""The tracker-tail yardstick (tests/tracker_tail_numpy.py) checked without a GPU: the case conditions of
tests/tracker_tail_cases.py (the fragility rule among them), agreement with float64 torch autograd of the reference's
statements (Tracker.py:179-195, torch.median), the float32 statements inside the derived bars, and sensitivity -- the bars, and
the exact `on` sets of the loss_only cases, must reject every structural variant a faulty kernel could compute
(tests/test_hip_tracker_tail.py compares the kernels against the same bars and sets)."""
import numpy as np
import pytest
import torch

from tests import composite_numpy as Y
from tests import tracker_tail_cases as C
from tests import tracker_tail_numpy as T


def test_case_conditions():
    cases = C.full_cases()
    for c in cases:
        C.check_conditions(c)
    have = {(c['N'], c['S'], c['dynamic']) for c in cases}
    for N in C.N_EDGES:
        assert (N, 16, 1) in have and (N, 16, 0) in have
        names = [e['name'] for e in C.exact_cases(N)]
        assert len(set(names)) == len(names) and len(names) >= (12 if N >= 6 else 8), (N, names)
    for N in C.S_AT:
        for S in C.S_LIST:
            assert (N, S, 1) in have and (N, S, 0) in have
    assert {c['inside_kind'] for c in cases} == set(C.INSIDE_KINDS)
    assert {c['w'] for c in cases if c['gc'] is not None} == {0.5, 0.2} and any(c['gc'] is None for c in cases)
    assert any('e' in c['mix'] and c['dynamic'] for c in cases) and sum(c['dup'] for c in cases) == 2
    assert {c['N'] > 1024 for c in cases if c['dup']} == {False, True}


def test_exact_cases_cover_what_they_claim():
    """per batch size: both outcomes of the two-value split, a kept count of 0, 1, 2, an even and an odd one, the +inf median"""
    for N in C.N_EDGES:
        ex = {e['name']: e for e in C.exact_cases(N)}
        kept = {int(e['on'].sum()) for e in ex.values()}
        assert 0 in kept and (N < 1 or 1 in kept) and (N < 2 or 2 in kept) and (N < 5 or 4 in kept) and (N < 6 or 5 in kept)
        two = [e for n, e in ex.items() if n.startswith('two values')]
        assert N < 3 or {e['med'] for e in two} == {1.0, 20.0}
        assert ex['mostly inf']['med'] == np.inf and ex['median zero']['med'] == 0.0
        tie = ex['tie run at the median']
        ins = np.ones(N, bool) if tie['inside'] is None else tie['inside'].astype(bool)
        assert N < 8 or ((tie['tmp'][ins] == 1.0).sum() >= 3 and (~ins & (tie['tmp'] == 1.0)).any())
        for e in ex.values():                                    # the expectation is the plain sort, restated here
            ins = np.ones(N, bool) if e['inside'] is None else e['inside'].astype(bool)
            v = np.sort(e['tmp'][ins])
            med = v[(len(v) - 1) // 2] if len(v) else np.inf
            assert med == e['med'] and (e['on'] == (ins & (e['tmp'] < 10.0 * med) & (e['gd'] > 0))).all()


# ------------------------------------------------------------------------------------------------ the reference's statements
def _statements(depth, var, rgb, gd, gc, w, inside, dynamic):
    """Tracker.py:170-195 on torch tensors: the prefilter's selection, then the lines as written.  (loss, on [N] bool, tmp)"""
    N = depth.shape[0]
    sel = torch.ones(N, dtype=torch.bool) if inside is None else torch.tensor(inside.astype(bool))
    idx = torch.nonzero(sel)[:, 0]
    depth, uncertainty, color = depth[sel], var[sel], rgb[sel]
    batch_gt_depth = torch.tensor(gd)[sel]
    uncertainty = uncertainty.detach()
    on = torch.zeros(N, dtype=torch.bool)
    if idx.numel() == 0:                                         # (torch.median of nothing raises; the tracker never gets here)
        return depth.sum() * 0.0, on.numpy(), None
    tmp = torch.abs(batch_gt_depth - depth) / torch.sqrt(uncertainty + 1e-10)
    if dynamic:
        mask = (tmp < 10 * tmp.median()) & (batch_gt_depth > 0)
    else:
        mask = batch_gt_depth > 0
    loss = (torch.abs(batch_gt_depth - depth) / torch.sqrt(uncertainty + 1e-10))[mask].sum()
    if gc is not None:
        color_loss = torch.abs(torch.tensor(gc)[sel] - color)[mask].sum()
        loss = loss + w * color_loss
    on[idx[mask]] = True
    full = torch.full((N,), float('nan'), dtype=tmp.dtype)
    full[idx] = tmp.detach()
    return loss, on.numpy(), full.numpy()


def _composite64(raw, z):
    raw = torch.tensor(raw)
    x = (np.float32(10.0) * raw[..., 3]).double().requires_grad_(True)
    col = raw[..., :3].double().requires_grad_(True)
    z = torch.tensor(z)
    alpha = torch.sigmoid(x)
    trans = torch.cumprod(torch.cat([torch.ones_like(alpha[:, :1]), 1. - alpha + Y.C32], -1), -1)[:, :-1]
    w = alpha * trans
    rgb = (w.unsqueeze(-1) * col).sum(-2)
    depth = (w * z).sum(-1)
    dz = z - depth.unsqueeze(-1)
    return x, col, depth, (w * dz * dz).sum(1), rgb


@pytest.mark.parametrize("dynamic", [0, 1])
def test_agrees_with_float64_autograd(dynamic):
    """the yardstick equals float64 torch autograd of the reference's statements to 1e-12 of scale on unsaturated and empty rays
    (autograd's 1 - alpha cancels and its cumprod backward divides, so saturated rays are left to the yardstick's own form,
    which tests/test_composite_cpu.py pins)"""
    for N in (1, 17, 257):
        for S in C.S_LIST:
            for kind, colour in (('null', True), ('scattered', False), ('block', True)):
                c = C.make(N, S, 'ad', dynamic, kind, colour, 0.2)
                y, b = c['y'], c['b']
                x, col, depth, var, rgb = _composite64(c['raw'], c['z'])
                loss, on, tmp = _statements(depth, var, rgb, c['gd'], None if c['gc'] is None else c['gc'].astype(np.float64),
                                            float(np.float32(c['w'])), c['inside'], dynamic)
                assert (on == y['on']).all(), c['name']
                for k, got in (('depth', depth), ('var', var), ('rgb', rgb)):
                    assert (np.abs(got.detach().numpy() - y[k]) <= 1e-12 * b['scales'][k] + 1e-300).all(), (c['name'], k)
                ins = y['inside']
                assert (np.abs(tmp[ins] - y['tmp'][ins]) <= 1e-12 * y['tmp'][ins] + 1e-300).all(), c['name']
                assert abs(float(loss.detach()) - y['loss']) <= 1e-12 * y['loss_abs'] + 1e-300, c['name']
                if y['on'].any():
                    loss.backward()
                    d = torch.cat([torch.zeros_like(col) if col.grad is None else col.grad, 10.0 * x.grad.unsqueeze(-1)], -1).numpy()
                else:
                    d = np.zeros(c['raw'].shape)
                assert (np.abs(d - y['d_raw']) <= 1e-12 * b['d_scale'] + 1e-300).all(), c['name']


def test_float32_statements_lie_within_the_bars():
    """oracle.render_oracle.composite (float32 torch ops), then the reference's lines in the types the reference gives them
    (gt float32, depth and uncertainty float64, colour float32): depth, var, rgb, tmp, the mask, the loss and, on the rays without
    a saturated sample (autograd's cumprod backward divides), the gradient lie within the yardstick's bars on every case"""
    from oracle import render_oracle as R
    for c in C.full_cases():
        y, b = c['y'], c['b']
        raw = torch.from_numpy(c['raw'].copy()).requires_grad_(True)
        depth, var, rgb, _ = R.composite(raw, torch.tensor(c['z']))
        loss, on, tmp = _statements(depth, var, rgb, c['gd'], c['gc'], c['w'], c['inside'], c['dynamic'])
        for k, got in (('depth', depth), ('var', var), ('rgb', rgb)):
            err = np.abs(got.detach().double().numpy() - y[k])
            assert (err <= b[k]).all(), (c['name'], k, float((err / b[k]).max()))
        ins = y['inside']
        if ins.any():
            assert (np.abs(tmp[ins] - y['tmp'][ins]) <= b['tmp'][ins]).all(), c['name']
        assert (on == y['on']).all(), c['name']
        assert abs(float(loss.detach()) - y['loss']) <= b['loss'], (c['name'], float(loss.detach()) - y['loss'], b['loss'])
        if y['on'].any():
            loss.backward()
            x = np.float32(10.0) * c['raw'][..., 3]
            plain = (np.abs(x) <= 6.0).all(-1) | (c['raw'][..., 3] == -100.0).all(-1)
            err = np.abs(raw.grad.double().numpy() - y['d_raw'])[plain]
            assert (err <= b['d_raw'][plain]).all(), (c['name'], float((err / b['d_raw'][plain]).max()))


# ------------------------------------------------------------------------------------------------ sensitivity
DECISION_VARIANTS = {
    'upper median': dict(upper=True),
    '<= in place of <': dict(le=True),
    'median over all rays': dict(over='all'),
    'median over the gd > 0 rays': dict(over='gdpos'),
    'gd > 0 applied before the median': dict(over='gdfirst'),
    'factor 9': dict(factor=9.0),
    'factor 11': dict(factor=11.0),
}


def _pad(a):
    return np.pad(a, [(0, 0), (0, 1)] + [(0, 0)] * (a.ndim - 2))


def _variants(c):
    """name -> the tail a faulty restatement computes on the case's inputs"""
    raw, z = c['raw'], c['z']
    args = (c['gd'], c['gc'], c['w'], c['inside'], c['dynamic'])
    out = {}
    if c['dynamic']:
        for name, kw in DECISION_VARIANTS.items():
            out[name] = T.tail(raw, z, *args, **kw)
    out['variance not detached'] = T.tail(raw, z, *args, detach=False)
    if c['gc'] is not None:
        out['colour term not masked'] = T.tail(raw, z, *args, colour_masked=False)
    if c['S'] > 1:
        v = dict(T.tail(raw[:, :-1], z[:, :-1], *args))
        v['d_raw'] = _pad(v['d_raw'])
        out['last sample dropped'] = v
    out['inclusive transmittance'] = T.tail(raw, z, *args, fwd=Y.forward(raw, z, inclusive=True))
    if (raw[..., 3] == 100.0).any():
        out['1e-10 left out of m'] = T.tail(raw, z, *args, fwd=Y.forward(raw, z, plus=0.0))
    if c['N'] >= 2:
        sw = np.arange(c['N'])
        sw[-2:] = sw[-2:][::-1]
        v = dict(c['y'])
        for k in ('depth', 'var', 'rgb', 'tmp', 'd_raw', 'on'):
            v[k] = c['y'][k][sw]
        out['rays N-1 and N-2 swapped'] = v
    return out


def _rejected(c, v):
    """would the GPU test's assertions fail on these outputs: an element outside its bar, the loss outside its bar, or a
    non-zero gradient on a ray that is not `on`"""
    y, b = c['y'], c['b']
    for k in ('depth', 'var', 'rgb', 'tmp'):
        if (np.abs(v[k] - y[k]) > b[k]).any():
            return True
    if abs(v['loss'] - y['loss']) > b['loss'] or (np.abs(v['d_raw'] - y['d_raw']) > b['d_raw']).any():
        return True
    return bool(v['d_raw'][~y['on']].any())


def test_bars_and_exact_sets_reject_every_variant():
    """Every listed variant is rejected: the structural ones (compositing, detached variance, colour mask, swapped rays) by the
    bars on the full cases wherever they apply; the decision variants (which median, which comparison, which factor) by the
    exact `on` set of at least one loss_only case at EVERY batch size that can tell them apart, and by the bars on the full cases
    where a ray happens to sit between the two thresholds (smooth data rarely does: that is what the exact cases are for)."""
    killed = {}
    cases = [c for c in C.full_cases() if c['N'] <= 513]
    for c in cases:
        for name, v in _variants(c).items():
            if _rejected(c, v):
                killed.setdefault(name, set()).add(c['name'])
    by_exact = {}
    for N in C.N_EDGES:
        for e in C.exact_cases(N):
            for name, kw in DECISION_VARIANTS.items():
                _, _, on = T.decide(e['tmp'], e['gd'], e['inside'], **kw)
                if (on != e['on']).any():
                    by_exact.setdefault(name, set()).add(N)
    print({k: len(v) for k, v in killed.items()}, 'of', len(cases), {k: len(v) for k, v in by_exact.items()})
    for c in cases:                                              # the structural variants, on every case where they apply
        on = c['y']['on']
        if not on.any():
            continue
        assert c['name'] in killed['variance not detached'], c['name']
        if c['gc'] is not None and (~on).any():
            assert c['name'] in killed['colour term not masked'], c['name']
        if c['S'] > 1 and 'a' in c['mix'] and c['inside_kind'] == 'null':
            assert c['name'] in killed['last sample dropped'] and c['name'] in killed['inclusive transmittance'], c['name']
        if c['N'] >= 2 and c['inside_kind'] == 'null' and not c['dup']:
            assert c['name'] in killed['rays N-1 and N-2 swapped'], c['name']
        if c['S'] >= 2 and c['N'] >= 8 and c['inside_kind'] == 'null' and ('b' in c['mix'] or 'c' in c['mix']):
            assert c['name'] in killed['1e-10 left out of m'], c['name']
    for name in DECISION_VARIANTS:                               # the decision variants, at every batch size that can show them
        need = {N for N in C.N_EDGES if N >= (4 if name.startswith('factor') or name.startswith('<=') else 3)}
        assert need <= by_exact.get(name, set()), (name, sorted(need - by_exact.get(name, set())))
