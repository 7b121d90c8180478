"""-m gpu: the depth-guided ray sampler (sample_body in csrc/util_kernels.hip) against the numpy yardstick of
tests/sampler_numpy.py, bit for bit, through the C ABI by hand: enslam_sample_rays (one wave per ray) and enslam_sample_prepare
(four rays per workgroup; no decoder, no accumulator, no flat range, no marking).  Cases and the conditions they reach:
tests/sampler_cases.py.  No tolerance anywhere: z_vals equal the yardstick's uint64 view, GUARD_ROWS sentinel rows behind
N * S stay whole, the inputs keep their bytes.

Left where they are: block marks (test_hip_blocks), the 4096 / 4097 route choice and the 100000-ray batch
(test_hip_step_kernels), anything rendered."""
import numpy as np
import pytest
import torch

from tests import sampler_cases as C
from tests import sampler_numpy as Y

pytestmark = pytest.mark.gpu

GUARD_ROWS = 4
SENTINEL = -7.5e300                                       # no sample distance
SCRATCH_FILL = (-3.5, -4.5)                               # what scratch holds before a call that has to compute the maxima
ENTRIES = ('sample_rays', 'sample_prepare')
EINVAL = -1


@pytest.fixture(scope='module')
def dev():
    import evennicer_slam_amd as E
    import evennicer_slam_amd.functional as EF
    from tests.hip_util import DEV
    return dict(EF=EF, L=E._lib, lib=E._lib.lib(), DEV=DEV, bound=EF.bound6(torch.from_numpy(C.BOUND.copy())))


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _up(dev, a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev['DEV'])


def upload(dev, c):
    host = dict(ro=c.ro, rd=c.rd, gd=c.gd, t_lin=c.t_lin, t_surf=c.t_surf, t_rand=c.t_rand)
    return {k: _up(dev, v) for k, v in host.items()}, host


def run(dev, c, t, entry, given=None, n_surf=None, n_lin=None, S=None, bound=None):
    """One call.  given: float32 [2] maxima handed in (depth_max_given = 1), None: computed by the call.
    Returns (return code, z float64 [N, S], the guard rows behind it, scratch float32 [2])."""
    EF, lib = dev['EF'], dev['lib']
    P, st = EF._ptr, EF._stream()
    n_lin = c.n_lin if n_lin is None else n_lin
    n_surf = c.n_surf if n_surf is None else n_surf
    S = c.S if S is None else S
    zbuf = torch.full((c.N * S + GUARD_ROWS * 64,), SENTINEL, dtype=torch.float64, device=dev['DEV'])
    scratch = _up(dev, np.asarray(SCRATCH_FILL if given is None else given, np.float32))
    head = (c.N, n_lin, n_surf, P(t['ro']), P(t['rd']), P(t['gd']), bound or dev['bound'], P(t['t_lin']), P(t['t_surf']),
            int(c.lindisp), P(t['t_rand']), P(scratch), int(given is not None), P(zbuf), 0, None, None)
    if entry == 'sample_rays':
        rc = lib.enslam_sample_rays(*head, st)
    else:
        rc = lib.enslam_sample_prepare(*head, 64, None, 0, None, None, None, 0, None, None, None, None, 0, st)
    torch.cuda.synchronize()
    z = zbuf.cpu().numpy()
    return rc, z[:c.N * S].reshape(c.N, S), z[c.N * S:], scratch.cpu().numpy()


def inputs_unchanged(t, host, label):
    for k, v in host.items():
        if v is not None:
            assert t[k].cpu().numpy().tobytes() == np.ascontiguousarray(v).tobytes(), f"{label}: input {k} was written"


def guard_intact(guard, label):
    bad = np.nonzero(guard != SENTINEL)[0]
    assert bad.size == 0, f"{label}: double {int(bad[0])} behind z_vals' end was written ({guard[bad[0]]!r})"


def rows_equal(z, want, label, rows=None):
    rows = np.arange(want.shape[0]) if rows is None else np.asarray(rows)
    ne = (_bits(z)[rows] != _bits(want)[rows])
    if ne.any():
        r, s = np.argwhere(ne)[0]
        raise AssertionError(f"{label}: {int(ne.any(1).sum())} rows differ; ray {int(rows[r])} sample {int(s)}: "
                             f"{z[rows[r], s]!r} ({z[rows[r], s].hex()}), yardstick {want[rows[r], s]!r} ({want[rows[r], s].hex()})")


def check_all_routes(dev, c, rows=None):
    """both entries; with depth, the maxima computed by the call and the yardstick's handed in"""
    C.check_case(c)
    t, host = upload(dev, c)
    for entry in ENTRIES:
        for given in ((None,) if c.gd is None else (None, c.dmax)):
            label = f"{c.name} {entry} {'maxima given' if given is not None else 'maxima computed'}"
            rc, z, guard, _ = run(dev, c, t, entry, given)
            assert rc == 0, (label, rc)
            rows_equal(z, c.z, label, rows)
            guard_intact(guard, label)
    inputs_unchanged(t, host, c.name)


@pytest.mark.parametrize("counts", C.COUNTS, ids=lambda nm: f"{nm[0]}+{nm[1]}")
def test_counts_bit_equal(dev, counts):
    """every count with depth and without, lindisp 0 and 1, with and without t_rand.  The subnormal-near row (ray
    sampler_cases.SUBNORMAL of the 'mixed' depths) is among them: a build that flushes float32 subnormals fails here."""
    n = 0
    for c in C.grid_cases():
        if (c.n_lin, c.n_surf) == counts:
            assert c.ok.all()
            check_all_routes(dev, c)
            n += 1
    assert n == 8


def test_whole_batches_and_batch_sizes_bit_equal(dev):
    """all depths zero, one ray, one zero-depth ray, shallow depths; N in BATCH_N on (32, 16): the prepare entry's last workgroup
    holds 1, 2, 3 and 4 rays"""
    seen = set()
    for c in C.batch_cases():
        assert c.ok.all()
        check_all_routes(dev, c)
        seen.add(c.N)
    assert seen | {C.N} == set(C.BATCH_N) and {n % 4 for n in C.BATCH_N} == {0, 1, 2, 3}


def test_position_in_the_batch_is_invisible(dev):
    """with the maxima given, permuting the rays permutes the rows"""
    p = C.permutation()
    for perturb in (False, True):
        c = C.make(32, 16, 'mixed', perturb=perturb)
        cp = C.make(32, 16, 'mixed', perturb=perturb, order=p)
        C.check_case(cp)
        assert cp.dmax.tobytes() == c.dmax.tobytes()
        t, tp = upload(dev, c)[0], upload(dev, cp)[0]
        for entry in ENTRIES:
            _, z, _, _ = run(dev, c, t, entry, c.dmax)
            rc, zp, guard, _ = run(dev, cp, tp, entry, c.dmax)
            assert rc == 0
            rows_equal(zp, z[p], f"{cp.name} {entry} against the unpermuted call")
            rows_equal(zp, cp.z, f"{cp.name} {entry}")
            guard_intact(guard, cp.name)


def test_out_of_contract_rays_leave_the_others_alone(dev):
    """rays NAN_RAYS divide 0 by 0: nothing is asserted about their rows; every other row equals the yardstick, the guards are whole"""
    for c in C.nan_cases():
        assert sorted(c.out) == sorted(C.NAN_RAYS)
        check_all_routes(dev, c, rows=np.nonzero(c.ok)[0])


def _scene_batch(n):
    """n rays as step_cases.sampler_case draws them from the tiny scene, with the yardstick's samples"""
    from tests import step_cases
    from tests.util import load
    import types
    scene = load('tiny_scene')
    ro, rd, gd = step_cases.sampler_case(scene, n)
    t_lin, t_surf = C.linspaces(32, 16)
    c = types.SimpleNamespace(name=f'tiny-scene-N{n}', N=n, n_lin=32, n_surf=16, S=48, lindisp=False, ro=ro, rd=rd, gd=gd, t_rand=None,
                              t_lin=t_lin, t_surf=t_surf, dmax=Y.depth_max(gd))
    c.z, c.ok = Y.sample(ro, rd, gd, scene['bound'], t_lin, t_surf)
    assert c.ok.all() and gd[n - 1] == gd.max() > gd[:-1].max()
    return c, scene['bound']


@pytest.mark.parametrize("n", [5, 4097])
def test_scratch_holds_the_maxima_after_the_call(dev, n):
    """depth_max_given == 0: scratch holds {max d, fl32(max d * 1.2f)} on return, whether every wave reduced the depths itself
    (N = 5) or depth_max_kernel did (N = 4097); depth_max_given != 0: scratch keeps its bytes"""
    if n == 5:
        c, b, bound = C.make(32, 16, 'mixed', n=5), C.BOUND, None
    else:
        c, b = _scene_batch(n)
        bound = dev['EF'].bound6(torch.from_numpy(b.copy()))
    t, host = upload(dev, c)
    for entry in ENTRIES:
        label = f"{c.name} {entry}"
        rc, z, guard, scratch = run(dev, c, t, entry, None, bound=bound)
        assert rc == 0
        rows_equal(z, c.z, label)
        guard_intact(guard, label)
        assert scratch.tobytes() == c.dmax.tobytes(), (label, scratch, c.dmax)
        other = np.array([c.dmax[0] * np.float32(1.5), c.dmax[1] * np.float32(0.75)], np.float32)    # (not a pair depth_max gives)
        rc, z, guard, scratch = run(dev, c, t, entry, other, bound=bound)
        assert rc == 0 and scratch.tobytes() == other.tobytes(), label
        guard_intact(guard, label)
        rows_equal(z, Y.sample(c.ro, c.rd, c.gd, b, c.t_lin, c.t_surf, dmax=other)[0], label + ' given')
    inputs_unchanged(t, host, c.name)


def test_return_codes(dev):
    """the 64-sample limit is judged on the count that is written: (64, 16) without depth writes [N, 64]; (64, 1) with depth and
    (0, 0) are ENSLAM_EINVAL and write nothing"""
    c = C.make(64, 0, 'none', perturb=True)
    t, host = upload(dev, c)
    t16 = dict(t, t_surf=_up(dev, C.linspaces(64, 16)[1]))
    for entry in ENTRIES:
        rc, z, guard, _ = run(dev, c, t16, entry, None, n_surf=16)
        assert rc == 0, (entry, '(64, 16, gt_depth NULL)', rc)
        rows_equal(z, c.z, f"(64, 16, gt_depth NULL) {entry}")
        guard_intact(guard, entry)
    cd = C.make(64, 0, 'mixed')
    td, hostd = upload(dev, cd)
    td = dict(td, t_surf=_up(dev, C.linspaces(64, 1)[1]))
    for entry in ENTRIES:
        for what, kw in (('(64, 1, with depth)', dict(n_surf=1)), ('(0, 0)', dict(n_lin=0, n_surf=0))):
            rc, z, guard, scratch = run(dev, cd, td, entry, None, S=64, **kw)
            assert rc == EINVAL, (entry, what, rc)
            assert (z == SENTINEL).all() and scratch.tolist() == list(SCRATCH_FILL), (entry, what)
            guard_intact(guard, f"{entry} {what}")
    inputs_unchanged(t, host, c.name)
    inputs_unchanged(td, dict(hostd, t_surf=None), cd.name)


def test_functional_sample_rays(dev):
    """the wrapper: its own linspaces, scratch and n_surf handling"""
    EF = dev['EF']
    bound = torch.from_numpy(C.BOUND.copy())
    for c in (C.make(32, 16, 'mixed', perturb=True), C.make(33, 31, 'positive', lindisp=True), C.make(48, 16, 'none')):
        t, _ = upload(dev, c)
        z = EF.sample_rays(t['ro'], t['rd'], t['gd'], bound, c.n_lin, c.n_surf, lindisp=c.lindisp, t_rand=t['t_rand'])
        rows_equal(z.cpu().numpy(), c.z, c.name)
        if c.gd is not None:
            z = EF.sample_rays(t['ro'], t['rd'], t['gd'], bound, c.n_lin, c.n_surf, lindisp=c.lindisp, t_rand=t['t_rand'],
                               depth_max=_up(dev, c.dmax))
            rows_equal(z.cpu().numpy(), c.z, c.name + ' maxima given')
