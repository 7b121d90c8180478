"""The float64 yardstick of the NICE decoder backward (tests/decoder_bwd_numpy.py) and its cases (tests/decoder_bwd_cases.py),
without a GPU: the numpy backward IS the gradient (torch float64 autograd of a float64 restatement of decoder_numpy's forward,
to 1e-12 * A), the scale arrays bound their gradients and vanish exactly where nothing contributes, the conditions of the
cases hold (fragile share, caps of the bar, masked / clipped samples, zeroed tiles), and single faults written into the float64
statement land beyond the bar -- so the same bar catches them on the device (tests/test_hip_decoder_bwd.py)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import blocks_numpy as BN
from tests import decoder_bwd_cases as BC
from tests import decoder_bwd_numpy as DB
from tests import decoder_cases as DC
from tests import decoder_numpy as DN


# ------------------------------------------------------------------------------------------------ 1. the gradient
def _t(a):
    return torch.from_numpy(np.array(a, dtype=np.float64))


def _interp_t(grid, pts, bound):
    """decoder_numpy.interp in torch float64: the float32 fractions of blocks_numpy.cells as constants plus a differentiable
    term (p - lo) / (hi - lo) * (size - 1) that is zero in value and carries ATen's slope where the axis is not clipped"""
    dims = tuple(grid.shape[2:])
    p = pts.detach().numpy()
    v = BN.cells(p, bound, dims)
    idx, exists, _ = BN.corners(p, bound, dims)
    fr = []
    for a, (co, size, slope) in enumerate(DB.coordinates(p, bound, dims)):
        live = pts[:, a] * float(slope)
        fr.append(_t(v['f' + 'xyz'[a]]) + (live - live.detach()) * _t(DB.inner(co, size)))
    g = grid.reshape(grid.shape[1], -1)
    out = 0
    for k in range(8):
        dx, dy, dz = k & 1, (k >> 1) & 1, k >> 2
        w = ((fr[0] if dx else 1.0 - fr[0]) * (fr[1] if dy else 1.0 - fr[1])) * (fr[2] if dz else 1.0 - fr[2])
        out = out + g[:, torch.from_numpy(idx[:, k])].t() * (w * _t(exists[:, k])).unsqueeze(-1)
    return out


def _decode_xyz_t(P, name, pts, c):
    p32 = _t(pts.detach().numpy().astype(np.float32))
    emb = torch.sin((p32 + (pts - pts.detach())) @ P[name + '.embedder._B'])
    h = emb
    for i in range(DN.N_BLOCKS):
        h = torch.relu(F.linear(h, P[f'{name}.pts_linears.{i}.weight'], P[f'{name}.pts_linears.{i}.bias'])) + \
            F.linear(c, P[f'{name}.fc_c.{i}.weight'], P[f'{name}.fc_c.{i}.bias'])
        if i == DN.SKIP:
            h = torch.cat([emb, h], -1)
    return F.linear(h, P[name + '.output_linear.weight'], P[name + '.output_linear.bias'])


def _decode_feat_t(P, name, c):
    h = c
    for i in range(DN.N_BLOCKS):
        h = torch.relu(F.linear(h, P[f'{name}.pts_linears.{i}.weight'], P[f'{name}.pts_linears.{i}.bias']))
        if i == DN.SKIP:
            h = torch.cat([c, h], -1)
    return F.linear(h, P[name + '.output_linear.weight'], P[name + '.output_linear.bias'])


def autograd_gradients(stage, ro, rd, z, d_raw):
    """torch float64 autograd of sum(eval_points * d_raw) through the restatement above"""
    params, grids, bound = DC.scene()
    P = {k: _t(v).requires_grad_(True) for k, v in params.items() if k.split('.')[0] in DB.STAGE_DECODERS[stage]}
    G = {k: _t(grids[k]).requires_grad_(True) for k in DB.STAGE_GRIDS[stage]}
    o, d = _t(ro).requires_grad_(True), _t(rd).requires_grad_(True)
    pts = (o[:, None, :] + d[:, None, :] * _t(z)[:, :, None]).reshape(-1, 3)
    keep = _t(DN.inside_bound(pts.detach().numpy(), bound))
    dr = _t(d_raw)
    if stage == 'coarse':
        occ = _decode_feat_t(P, 'coarse_decoder', _interp_t(G['grid_coarse'], pts, bound * 2))[:, 0]
    else:
        c_mid = _interp_t(G['grid_middle'], pts, bound)
        occ = _decode_xyz_t(P, 'middle_decoder', pts, c_mid)[:, 0]
        if stage in ('fine', 'color'):
            c_fine = torch.cat([_interp_t(G['grid_fine'], pts, bound), c_mid.detach()], -1)
            occ = occ + _decode_xyz_t(P, 'fine_decoder', pts, c_fine)[:, 0]
    loss = (occ * keep * dr[:, 3]).sum()
    if stage == 'color':
        rgb = _decode_xyz_t(P, 'color_decoder', pts, _interp_t(G['grid_color'], pts, bound))[:, :3]
        loss = loss + (rgb * dr[:, :3]).sum()
    loss.backward()
    out = {'rays_o': o.grad, 'rays_d': d.grad}
    out.update({k: v.grad for k, v in P.items()})
    out.update({k: v.grad.reshape(32, -1) for k, v in G.items()})
    return {k: v.numpy() for k, v in out.items()}


@pytest.mark.parametrize("stage", BC.STAGES)
def test_numpy_backward_is_the_gradient(stage):
    ro, rd, z = BC.rays(stage, 5, 32)
    params, grids, bound = DC.scene()
    points = BN.sample_points(ro, rd, z)
    keep = DN.inside_bound(points, bound)
    name = 'grid_coarse' if stage == 'coarse' else 'grid_middle'
    clipped = [(~DB.inner(co, size)) for co, size, _ in DB.coordinates(points, bound * 2 if stage == 'coarse' else bound,
                                                                        grids[name].shape[2:])]
    assert keep.any() and not keep.all() and any(c.any() for c in clipped)
    # the cotangent is NOT zeroed on fragile samples here: float64 against float64 takes the same branches
    d_raw = np.random.default_rng(31 + BC.STAGES.index(stage)).standard_normal((points.shape[0], 4)).astype(np.float32)
    assert (d_raw[BC.fragile_samples(stage, points)] != 0).all()
    g, A = DB.backward(params, grids, ro, rd, z, d_raw, stage, bound)
    A.pop('dC_max')
    want = autograd_gradients(stage, ro, rd, z, d_raw)
    assert set(g) == set(want)
    for k in g:
        Ab = np.broadcast_to(BC.scale_of(k, A[k]), g[k].shape)
        assert g[k].shape == want[k].shape, k
        assert (np.abs(g[k] - want[k]) <= 1e-12 * Ab).all(), (stage, k, float((np.abs(g[k] - want[k]) / np.maximum(Ab, 1e-300)).max()))


# ------------------------------------------------------------------------------------------------ 2. the scale arrays
@pytest.mark.parametrize("stage", BC.STAGES)
def test_scale_arrays(stage):
    c = BC.case(stage, 3, 48, True)
    bound = DC.scene()[2]
    for k, g in c.g.items():
        Ab = np.broadcast_to(BC.scale_of(k, c.A[k]), g.shape)
        assert (Ab >= 0).all() and (np.abs(g) <= Ab * (1 + 1e-12)).all(), k
        assert (g[Ab == 0] == 0).all(), k
    points = BN.sample_points(c.ro, c.rd, c.z)
    live = (c.d_raw != 0).any(axis=1)
    # rays whose tiles are all zeroed: nothing contributes
    dead_rays = ~live.reshape(c.N, c.S).any(axis=1)
    assert np.array_equal(c.A['rays_o'] == 0, dead_rays) and np.array_equal(c.A['rays_d'] == 0, dead_rays)
    # grid rows: exactly the existing, non-zero-weight taps of the samples that send a feature gradient to that grid
    name, lookup, sends = {'coarse': ('grid_coarse', bound * 2, live & DN.inside_bound(points, bound)),
                           'middle': ('grid_middle', bound, live & DN.inside_bound(points, bound)),
                           'fine': ('grid_fine', bound, live & DN.inside_bound(points, bound)),
                           'color': ('grid_color', bound, live)}[stage]
    touched = BN.corner_voxels(points[sends], lookup, DC.scene()[1][name].shape[2:], nonzero_only=True)
    assert np.array_equal(c.A[name] > 0, touched) and touched.any() and not touched.all(), name
    if stage == 'color':       # the colour decoder's fourth output row
        assert (c.A['color_decoder.output_linear.weight'][3] == 0).all() and c.A['color_decoder.output_linear.bias'][3] == 0
        assert (c.A['color_decoder.output_linear.weight'][:3] > 0).all()


# ------------------------------------------------------------------------------------------------ 3. the conditions
@pytest.mark.parametrize("stage", BC.STAGES)
def test_conditions_of_the_cases(stage):
    epre = BC.e_pre(stage)
    assert all(0 < v < 1e-4 for v in epre.values()), epre
    shares = []
    for N in BC.SHAPES_N:
        for S in BC.SHAPES_S:
            c = BC.case(stage, N, S)
            BC.check_case(c)
            shares.append(float(c.fragile.mean()))
    for N, S in BC.LISTED_SHAPES:
        BC.check_case(BC.case(stage, N, S, True))
    ref = BC.case(stage, BC.REF_N, BC.REF_S)
    assert BC.branch_differences(stage, BN.sample_points(ref.ro, ref.rd, ref.z)) == 0
    erel = BC.e_rel(stage)
    print(f"{stage}: e_pre {epre}; fragile share {min(shares):.4f} .. {max(shares):.4f} (reference batch {ref.fragile.mean():.4f}); e_rel "
          + ", ".join(f"{k} {v:.2e}" for k, v in erel.items()))
    assert set(erel) == {BC.family_of(k) for k in ref.g} and ref.erel == erel
    for fam, v in erel.items():
        assert 0 < BC.MARGIN * v <= BC.CAP_REL, (stage, fam, v)
    # how far the smaller batches' own figures (decoder parameters only) lie above the reference batch's
    worst = max(BC.case(stage, N, S).erel[fam] / erel[fam] for N in BC.SHAPES_N for S in BC.SHAPES_S for fam in erel)
    print(f"{stage}: largest e_rel of a case / e_rel of the reference batch: {worst:.1f}")


def test_reference_batch_figures_carry_over_to_grids_and_rays():
    """the float32 oracle on every other shape stays within MARGIN of the reference batch's e_rel for grids and rays (worst:
    6.5, rays_d of the colour stage at N 65, S 16); the decoder parameters' figures do NOT carry over to small batches
    (decoder_bwd_cases.case_e_rel)"""
    beyond = 0
    for stage in BC.STAGES:
        ref = BC.e_rel(stage)
        for N in BC.SHAPES_N:
            for S in BC.SHAPES_S:
                c = BC.case(stage, N, S)
                got = BC.oracle_gradients(stage, c.ro, c.rd, c.z, c.d_raw)
                for k in c.g:
                    fam = BC.family_of(k)
                    if BC.batch_sum(fam):
                        beyond += BC.worst_ratio(k, got[k], c.g[k], c.A[k], ref[fam]) > BC.MARGIN
                    else:
                        BC.assert_within_bar(k, got[k], c.g[k], c.A[k], ref[fam], f"oracle, stage {stage}, N {N}, S {S}")
    assert beyond > 0, "the oracle meets the reference batch's figures for decoder parameters everywhere: case_e_rel is not needed"


# ------------------------------------------------------------------------------------------------ 4. fault table
def _identity(x):
    return x


def _ones(keep):
    return np.ones_like(keep)


def _drop_rows(n):
    def contributing(d_raw):
        d_raw = d_raw.copy()
        d_raw[-n:] = 0.0
        return d_raw
    return contributing


def _z_forgotten_once(z):
    z = z.copy()
    z[:, z.shape[1] // 2] = 1.0
    return z


def _no_fc_c0(layer, delta, x):
    return np.zeros((delta.shape[1], x.shape[1])) if layer.endswith('fc_c.0') else delta.T @ x


def _neighbours_delta(layer, delta, x):
    return np.roll(delta, -1, axis=0).T @ x


LAST_RAY = 'last ray'
# (name, stage, helper of decoder_bwd_numpy, its replacement, {family or tensor: least share of its elements with A > 0 that must
#  move beyond the bar} -- LAST_RAY: the three elements of the last ray instead of the whole tensor.  The last samples of the last
#  ray lie outside the bound, so the two faults that drop them show in the colour decoder's families: only colour flows there.)
FAULTS = [
    ('detach on c_middle removed', 'fine', 'fine_middle_feature_grad', _identity, {'grid_middle': 0.1, 'rays_o': 0.1, 'rays_d': 0.1}),
    ('occupancy gradient through masked samples', 'middle', 'occupancy_mask', _ones,
     {'grid_middle': 0.1, 'middle_decoder.weights': 0.1, 'middle_decoder.biases': 0.1}),
    ('colour gradient of masked samples dropped', 'color', 'colour_mask', _identity,
     {'grid_color': 0.1, 'color_decoder.weights': 0.1, 'color_decoder.biases': 0.1}),
    ('tap 7 dropped in the scatter', 'middle', 'SCATTER_TAPS', tuple(range(7)), {'grid_middle': 0.1}),
    ('tap 7 dropped in the scatter, coarse', 'coarse', 'SCATTER_TAPS', tuple(range(7)), {'grid_coarse': 0.1}),
    ('last sample of the last tile dropped', 'color', 'contributing', _drop_rows(1),
     {'color_decoder.weights': 0.1, 'color_decoder.biases': 0.1, ('rays_o', LAST_RAY): 1.0, ('rays_d', LAST_RAY): 1.0}),
    ('last tile of the last ray dropped', 'color', 'contributing', _drop_rows(16),
     {'color_decoder.weights': 0.1, 'color_decoder.biases': 0.1, ('rays_o', LAST_RAY): 1.0, ('rays_d', LAST_RAY): 1.0}),
    ('z missing in g_rays_d for one sample per ray', 'color', 'ray_weights', _z_forgotten_once, {'rays_d': 0.9}),
    ('clipped axes given a position gradient', 'color', 'inner', lambda co, size: np.ones(co.shape, dtype=bool),
     {'rays_o': 0.1, 'rays_d': 0.1}),
    ('cosine with the wrong sign', 'middle', 'embedding_slope', lambda arg: -np.cos(arg), {'rays_o': 0.9, 'rays_d': 0.9}),
    ('fc_c of block 0 without weight gradient', 'middle', 'weight_grad', _no_fc_c0, {'middle_decoder.fc_c.0.weight': 0.9}),
    ("weight-gradient row taken from sample s+1's delta", 'color', 'weight_grad', _neighbours_delta,
     {'middle_decoder.weights': 0.1, 'fine_decoder.weights': 0.1, 'color_decoder.weights': 0.1}),
    ("d_raw's colour columns not ignored in the fine stage", 'fine', 'runs_colour', lambda stage: stage in ('fine', 'color'),
     {'rays_o': 0.1, 'rays_d': 0.1}),
]
FAULT_N, FAULT_S = 65, 48


def fault_shares(stage, helper, replacement, families, monkeypatch):
    c = BC.case(stage, FAULT_N, FAULT_S)
    erel = c.erel
    assert (c.d_raw[-1] != 0).all(), "the fault cases need a live last sample"
    params, grids, bound = DC.scene()
    with monkeypatch.context() as m:
        if helper is not None:
            m.setattr(DB, helper, replacement)
        g, _ = DB.backward(params, grids, c.ro, c.rd, c.z, c.d_raw, stage, bound)
    bad = {k: BC.beyond_bar(k, g[k], c.g[k], c.A[k], erel[BC.family_of(k)]) for k in c.g}
    live = {k: np.broadcast_to(BC.scale_of(k, c.A[k]), c.g[k].shape) > 0 for k in c.g}
    out = {}
    for fam in families:
        if isinstance(fam, tuple):
            out[fam] = float(bad[fam[0]][-1].mean())
            continue
        names = [k for k in c.g if k == fam or BC.family_of(k) == fam]
        assert names, fam
        out[fam] = sum(int(bad[k][live[k]].sum()) for k in names) / sum(int(live[k].sum()) for k in names)
    return out, sum(int(b.sum()) for b in bad.values())


@pytest.mark.parametrize("fault", FAULTS, ids=[f[0] for f in FAULTS])
def test_fault_lands_beyond_the_bar(fault, monkeypatch):
    name, stage, helper, replacement, families = fault
    shares, _ = fault_shares(stage, helper, replacement, families, monkeypatch)
    print(f"{name} ({stage}): " + ", ".join(f"{k if isinstance(k, str) else k[0] + ' of the ' + k[1]} {100 * v:.1f} %" for k, v in shares.items()))
    for fam, least in families.items():
        assert shares[fam] >= least, (name, fam, shares[fam])
    # ... and without the fault nothing is beyond the bar (the replacement is undone)
    assert fault_shares(stage, None, None, families, monkeypatch)[1] == 0
