"""The ray-sampler yardstick (tests/sampler_numpy.py) and its cases (tests/sampler_cases.py) checked without a GPU: bit for bit
against oracle.render_oracle.sample_depths (itself pinned to the reference by tests/test_oracle_golden.py) and against the golden
z_vals, for the case conditions, and for teeth -- every single-defect variant of the yardstick must differ from it in at least one
bit of at least one case, so a kernel with that defect cannot pass tests/test_hip_sampler.py.

Which case catches which defect (test_the_cases_have_teeth asserts these and prints the full count per defect):
  near product in float64                       32+16-mixed-edges        (near * (1 - t) is inexact in float32 on almost every ray)
  1.2 applied in float64                        32+16-mixed-edges        (the rays on which the cap binds)
  0.95f * d in float64                          5+3-mixed-edges          (every ray with d > 0)
  no-depth surface end from dmax1               2+1 does NOT (t_surf = [0]); 5+3-mixed-edges does (the zero-depth rays)
  last linear sample's upper from a neighbour   16+0-none-edges-perturb  (t_rand != 0 in the last column)
  clamp's lower bound dropped                   32+16-mixed-edges        (the two rays that point away from outside the box)
  merge skipped when n_surf == 1                63+1-mixed-edges, 2+1-mixed-edges (0.95 d lies below the last linear sample)
  subnormal near flushed                        1+0-mixed-edges ... every unperturbed mixed-depth case: ray 19's first sample is the subnormal"""
import numpy as np
import torch

from tests import sampler_cases as C
from tests import sampler_numpy as Y
from tests.util import load

CASES = {c.name: c for c in C.in_contract_cases()}


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _oracle(c, dmax=None):
    from oracle import render_oracle as R
    T = torch.from_numpy
    return R.sample_depths(T(c.ro), T(c.rd), None if c.gd is None else T(c.gd), T(c.bound), c.n_lin, c.n_surf, 'color',
                           lindisp=c.lindisp, t_rand=None if c.t_rand is None else T(c.t_rand),
                           depth_max=None if dmax is None else T(np.asarray(dmax[0]))).numpy()


def test_case_count_and_names():
    assert len(CASES) == len(C.COUNTS) * 8 + 8 + len(C.BATCH_N) - 1
    for n_lin, n_surf in C.COUNTS:
        assert 1 <= n_lin and n_lin + n_surf <= 64


def test_case_conditions():
    for c in CASES.values():
        C.check_case(c)
        assert c.ok.all() and c.out == ()
    for c in C.nan_cases():
        C.check_case(c)
        assert sorted(np.nonzero(~c.ok)[0].tolist()) == sorted(C.NAN_RAYS) and np.isnan(c.z[list(C.NAN_RAYS)]).any(1).all()
    p = C.permutation()
    assert sorted(p.tolist()) == list(range(C.N)) and (p != np.arange(C.N)).sum() > C.N // 2
    c, cp = CASES['32+16-mixed-edges-perturb'], C.make(32, 16, 'mixed', perturb=True, order=p)
    C.check_case(cp)
    assert np.array_equal(_bits(cp.z), _bits(c.z[p]))      # with the same maxima a ray's row does not depend on its place
    assert cp.dmax.tobytes() == c.dmax.tobytes()


def test_yardstick_equals_the_oracle_bit_for_bit():
    for c in CASES.values():
        want = _oracle(c)
        assert want.dtype == np.float64 and want.shape == c.z.shape, c.name
        assert np.array_equal(_bits(want), _bits(c.z)), (c.name, np.nonzero((_bits(want) != _bits(c.z)).any(1))[0])
    # the maxima handed in, as a ray-sharded caller does: the first 8 rays with the whole batch's maxima
    whole = CASES['32+16-mixed-edges']
    part = C.make(32, 16, 'mixed', n=8)
    z, ok = Y.sample(part.ro, part.rd, part.gd, part.bound, part.t_lin, part.t_surf, dmax=whole.dmax)
    assert ok.all() and np.array_equal(_bits(z), _bits(whole.z[:8])) and not np.array_equal(_bits(z), _bits(part.z))
    assert np.array_equal(_bits(_oracle(part, whole.dmax)), _bits(z))


def test_yardstick_equals_the_golden_z_vals():
    s, col, coarse = load('tiny_scene'), load('tiny_color'), load('tiny_coarse')
    t_lin, t_surf = C.linspaces(32, 16)
    z, ok = Y.sample(s['rays_o'], s['rays_d'], s['gt_depth'], s['bound'], t_lin, t_surf)
    assert ok.all() and np.array_equal(_bits(z), _bits(col['z_vals']))
    z, ok = Y.sample(s['rays_o'], s['rays_d'], None, s['bound'], t_lin, None)     # the coarse stage takes no depth
    assert ok.all() and np.array_equal(_bits(z), _bits(coarse['z_vals']))


MUST_CATCH = {
    'near product in float64': ('32+16-mixed-edges',),
    '1.2 applied in float64': ('32+16-mixed-edges',),
    '0.95f * d in float64': ('5+3-mixed-edges',),
    'no-depth surface end from dmax1': ('5+3-mixed-edges',),
    "last linear sample's upper from a neighbour": ('16+0-none-edges-perturb',),
    "clamp's lower bound dropped": ('32+16-mixed-edges',),
    'merge skipped when n_surf == 1': ('63+1-mixed-edges', '2+1-mixed-edges'),
    'subnormal near flushed': ('1+0-mixed-edges', '32+16-mixed-edges', '63+1-mixed-edges'),
}


def test_the_cases_have_teeth():
    """each defect changes at least one bit of at least one case, and of the cases named in MUST_CATCH"""
    assert set(MUST_CATCH) == set(Y.DEFECTS)
    caught = {d: [] for d in Y.DEFECTS}
    for c in CASES.values():
        for d in Y.DEFECTS:
            z, _ = Y.sample(c.ro, c.rd, c.gd, c.bound, c.t_lin, c.t_surf if c.gd is not None else None, c.lindisp, c.t_rand, defect=d)
            if not np.array_equal(_bits(z), _bits(c.z)):
                caught[d].append(c.name)
    for d, names in MUST_CATCH.items():
        for name in names:
            assert name in caught[d], (d, name)
    # t_surf = [0]: the zero-depth surface sample is 0.001 whatever the maximum
    assert '2+1-mixed-edges' not in caught['no-depth surface end from dmax1']
    print({d: len(v) for d, v in caught.items()}, 'of', len(CASES))
