"""The float64 yardstick of the NICE decoder forward (tests/decoder_numpy.py) and its cases (tests/decoder_cases.py), without
a GPU: the yardstick agrees with the float32 CPU oracle and with the reference's goldens, the bar is tight (the caps), the
exact-argument construction is exact, and single faults written into the float64 statement land beyond the bar -- so the
same bar catches them on the device (tests/test_hip_decoder_fwd.py)."""
import numpy as np
import pytest

from tests import decoder_cases as DC
from tests import decoder_numpy as DN
from tests.util import load

CASES = [(name, stage) for name in DC.POOLS for stage in DC.STAGES]


@pytest.mark.parametrize("name,stage", CASES)
def test_yardstick_agrees_with_the_float32_oracle(name, stage):
    eref = DC.e_ref(name, stage)
    used = [3] if stage != 'color' else [0, 1, 2, 3]
    assert np.isfinite(eref).all() and all(eref[c] > 0 for c in used) and all(eref[c] == 0 for c in range(4) if c not in used)
    points = DC.pool(name, stage)
    for apply_mask in (False, True):
        masked = DC.masked_rows(points, apply_mask)
        assert masked.any() == (apply_mask and name == 'mixed')
        want, got = DC.yardstick(name, stage, apply_mask), DC.oracle(name, stage, apply_mask)
        assert (want[masked, 3] == 100.0).all() and (want[~masked, 3] != 100.0).all()
        DC.assert_within_bar(got, want, eref, masked, f"oracle {name} {stage} mask {apply_mask}", margin=1.0)


@pytest.mark.parametrize("stage", DC.STAGES)
def test_yardstick_agrees_with_the_reference_goldens(stage):
    """the reference's own eval_points on its 200 fixture points (some of them outside the bound), within 4 * e_ref"""
    g = load('tiny_eval_points')
    params, grids, bound = DC.scene()
    masked = DC.masked_rows(g['p'], True)
    assert 0 < masked.sum() < len(masked)
    want = DN.eval_points(params, grids, g['p'], stage, bound, apply_mask=True)
    DC.assert_within_bar(g['raw_' + stage], want, DC.e_ref('mixed', stage), masked, f"golden {stage}", margin=4.0)


@pytest.mark.parametrize("name,stage", CASES)
def test_bar_stays_below_its_cap(name, stage):
    eref, want = DC.e_ref(name, stage), DC.yardstick(name, stage, False)
    for col in range(4):
        if eref[col] > 0:
            share = DC.MARGIN * eref[col] / np.abs(want[:, col]).max()
            assert share <= DC.CAP[DC.FAMILY[name]], (name, stage, col, share)


def test_exact_argument_construction():
    assert DC.check_conditions()
    for dec in DC.XYZ_DECODERS:
        B, B0 = DC.params_of('exact')[dec + '.embedder._B'], DC.params_of('generic')[dec + '.embedder._B']
        assert np.abs(B).max() <= DC.B_MAX and np.array_equal(np.round(B.astype(np.float64) / DC.B_STEP) * DC.B_STEP, B)
        assert np.abs(B.astype(np.float64) - np.clip(B0, -DC.B_MAX, DC.B_MAX)).max() <= DC.B_STEP / 2
        # ... while the generic family's argument does round in float32
        p = DC.pool('generic', 'color')
        assert not np.array_equal(DN.fourier_argument(p, B0, np.float32).astype(np.float64), DN.fourier_argument(p, B0))


# ------------------------------------------------------------------------------------------------ fault table
def _params_fault(key, index, family='generic'):
    def params():
        out = dict(DC.params_of(family))
        w = out[key].copy()
        assert (w[index] != 0).all()
        w[index] = 0
        out[key] = w
        return out
    return params


def _roll_rows(raw):
    return np.roll(raw, 1, axis=0)


def _zero_last_embedding_column(emb):
    emb = emb.copy()
    emb[:, 92] = 0.0
    return emb


# (name, stage, replacement in decoder_numpy or None, parameters or None)
FAULTS = [
    ('one bias entry zeroed', 'color', None, _params_fault('middle_decoder.pts_linears.1.bias', (5,))),
    ('one weight zeroed', 'color', None, _params_fault('color_decoder.pts_linears.3.weight', (7, 100))),
    ('last embedding column zeroed', 'color', ('embedding_columns', _zero_last_embedding_column), None),
    ('last feature column of fc_c.4 of the fine decoder zeroed', 'fine', None,
     _params_fault('fine_decoder.fc_c.4.weight', (slice(None), 63))),
    ('last input column of the colour output layer zeroed', 'color', None,
     _params_fault('color_decoder.output_linear.weight', (slice(None), 31))),
    ('row shifted by one', 'color', ('rows', _roll_rows), None),
    ('row shifted by one, coarse', 'coarse', ('rows', _roll_rows), None),
    ('corner tap 7 dropped', 'middle', ('TAPS', tuple(range(7))), None),
    ('corner tap 7 dropped, coarse', 'coarse', ('TAPS', tuple(range(7))), None),
    ('c_fine and c_middle swapped', 'fine', ('fine_features', lambda cf, cm: np.concatenate([cm, cf], axis=-1)), None),
    ('skip concat in the wrong order', 'middle', ('skip_concat', lambda emb, h: np.concatenate([h, emb], axis=-1)), None),
    ('fc_c left out of block 0', 'middle', None, _params_fault('middle_decoder.fc_c.0.weight', (slice(None), slice(None)))),
]


def fault_share(pool_name, stage, replacement, params, monkeypatch):
    """share of the pool's points that the fault moves beyond the bar"""
    _, grids, bound = DC.scene()
    with monkeypatch.context() as m:
        if replacement is not None:
            m.setattr(DN, replacement[0], replacement[1])
        got = DN.eval_points(params() if params else DC.params_of(DC.FAMILY[pool_name]), grids, DC.pool(pool_name, stage), stage,
                             bound, apply_mask=False)
    bad = DC.beyond_bar(got, DC.yardstick(pool_name, stage, False), DC.e_ref(pool_name, stage), np.zeros(DC.POOL, dtype=bool))
    return float(bad.any(axis=1).mean())


@pytest.mark.parametrize("fault", FAULTS, ids=[f[0] for f in FAULTS])
def test_fault_lands_beyond_the_bar(fault, monkeypatch):
    name, stage, replacement, params = fault
    share = fault_share('generic', stage, replacement, params, monkeypatch)
    print(f"{name} ({stage}): {100 * share:.1f} % of the points beyond the bar")
    assert share >= 0.10, (name, share)
    # ... and without the fault nothing is (the replacement is undone, the parameters were a copy)
    assert fault_share('generic', stage, None, None, monkeypatch) == 0.0


def test_fault_mask_with_equality_changes_face_points(monkeypatch):
    """points ON a face of the bound are outside (strict comparison); a mask with >= / <= lets them in"""
    params, grids, bound = DC.scene()
    p = DC.pool('generic', 'color')[:12].copy()
    for i in range(12):
        p[i, i % 3] = bound[i % 3, (i // 3) % 2]
    assert not DN.inside_bound(p, bound).any()
    want = DN.eval_points(params, grids, p, 'color', bound, apply_mask=True)
    assert (want[:, 3] == 100.0).all()
    monkeypatch.setattr(DN, 'inside', lambda q, lo, hi: (q >= lo) & (q <= hi))
    got = DN.eval_points(params, grids, p, 'color', bound, apply_mask=True)
    assert (got[:, 3] != 100.0).all()
    assert DC.beyond_bar(got, want, DC.e_ref('mixed', 'color'), np.ones(12, dtype=bool)).any(axis=1).all()
