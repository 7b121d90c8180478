"""No GPU: the event-collapse regularisers of contrast maximisation (event_cmax.py reg=..., enslam_event_cmax_reg_eval).

The hand-worked values; the numpy route against the yardstick (tests/event_cmax_reg_numpy.py) on every case of
tests/event_cmax_reg_cases.py under both kinds, inside the derived bound, with the four existing outputs bit-equal to a call
without a regulariser; dR against torch autograd on an independent statement; the bound bracketed by three deliberately wrong
statements; 'flow' exact zeros; 'rigid' without translation equal to 'rotation' bit for bit; reg=None returns today's tuples
and keys; every refusal; recovery of a planted motion from zero with the reference time at the window's start, where the
unregularised objective collapses; the tools' flags; the pose prior with tracking.cmax_reg and the `collapsed` fallback on CPU
tensors."""
import ctypes
import importlib.util
import math
import os
import re

import numpy as np
import pytest
import torch

from tests import event_cmax_cases as CC
from tests import event_cmax_reg_cases as GC
from tests import event_cmax_reg_numpy as YG
from tests import event_cmax_rigid_cases as RC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPORTS = ("enslam_event_cmax_reg_workspace", "enslam_event_cmax_reg_eval")


def _route(src, case, **over):
    from evennicer_slam_amd import event_cmax as M
    kw = dict(GC.arguments(src, case))
    kw.update(over)
    return M.cmax_numpy(*GC.stream(src, case), **kw)


def _bits(a):
    return np.asarray(a).view(np.int64)


# ---- by hand -------------------------------------------------------------------------------------------------------------------
def test_hand_worked_values():
    src, case = GC.BY_ID['own-reg_hand']
    base = GC.base_reference(src, case)
    refs = {kind: GC.reference(src, case, kind) for kind in GC.KINDS}
    GC.check_conditions(src, case, base, refs)
    for kind in GC.KINDS:
        want = GC.HAND[kind]
        assert refs[kind]['R'] == want['R'] and refs[kind]['dR'].tolist() == want['dR'] and refs[kind]['M'] == 1
        rs = _route(src, case, reg=kind)[4]
        assert rs.dtype == np.float64 and rs.tolist() == [want['R'], 1.0] + want['dR'], (kind, rs)
    # the deformation is det(dx'/dx) - 1 of the 2 x 2 Jacobian 1 - dt c, in exact arithmetic
    from fractions import Fraction as F
    dt, c11, c22, c12, c21 = F(1, 8), F(7, 4), F(9, 8), F(3, 4), F(-3, 4)
    assert (1 - dt * c11) * (1 - dt * c22) - dt * c12 * dt * c21 - 1 == -F(GC.HAND['deformation']['R'])
    assert -dt * (c11 + c22) == -F(GC.HAND['divergence']['R'])


# ---- the numpy route against the yardstick ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", GC.IDS)
def test_numpy_route_against_the_yardstick(cid):
    src, case = GC.BY_ID[cid]
    base = GC.base_reference(src, case)
    refs = {kind: GC.reference(src, case, kind) for kind in GC.KINDS}
    GC.check_conditions(src, case, base, refs)
    plain = _route(src, case)
    assert len(plain) == 4
    P = YG.PARAMS[case['model']]
    for kind in GC.KINDS:
        ref = refs[kind]
        out = _route(src, case, reg=kind)
        assert len(out) == 5
        for a, b in zip(out[:4], plain):                                    # the existing outputs: the same bits
            assert a.dtype == b.dtype and np.array_equal(a.view(np.int64), b.view(np.int64))
        rs = out[4]
        assert rs.shape == (2 + P,) and rs[1] == ref['M']
        b = GC.bounds(case, ref)
        errs = dict(R=abs(rs[0] - ref['R']), dR=np.abs(rs[2:] - ref['dR']))
        print(cid, kind, {k: (np.asarray(errs[k]).tolist(), np.asarray(b[k]).tolist()) for k in errs})
        assert errs['R'] <= b['R'] and np.all(errs['dR'] <= b['dR']), (errs, b)
        if ref['M'] <= 1:
            assert rs[0] == ref['R'] and rs[2:].tolist() == ref['dR'].tolist()          # one term: no sum to differ in
        ng = _route(src, case, reg=kind, want_grad=False)
        assert np.array_equal(_bits(ng[4][:2]), _bits(rs[:2])) and not ng[4][2:].any() and not ng[2][2:].any()
        if case['model'] == 'flow':
            assert rs[0] == 0.0 and not rs[2:].any() and rs[1] == ref['M']


GRAD_CASES = ['rigid-45x61_N257', 'rigid-45x61_N700_pixel', 'rigid-45x61_N700', 'base-45x61_rot_k9', 'base-45x61_N255', 'own-reg_both_signs',
              'own-reg_t_ref']


@pytest.mark.parametrize("cid", GRAD_CASES)
@pytest.mark.parametrize("kind", GC.KINDS)
def test_gradient_against_autograd(cid, kind):
    """dR of the yardstick against autograd on reg_torch, which takes the Jacobian of the motion field by autograd and the
    determinant written out.  Away from the kinks: no |d| is small without being zero (an exact zero has sgn 0 here and in
    torch.abs alike).  Tolerance: the two statements round differently in a handful of operations per event, each at most u
    times the magnitude of the terms of dd -- 64 u mean_e(|dt| (|e11| + |e22|) + dt^2 (|e11 c22| + |c11 e22| + |e12 c21| +
    |c12 e21|)), bounded here by 64 u mean_e(4 |dt| A + 8 dt^2 A^2) with A = max(1, |u|, |v|, rho) max(1, |theta|_inf) -- plus
    the SUM bound of the cases file."""
    src, case = GC.BY_ID[cid]
    ref = GC.reference(src, case, kind)
    kw = GC.arguments(src, case)
    t, x, y, _ = GC.stream(src, case)
    voted = GC.base_reference(src, case)['voted']
    nz = ref['r'][voted & (ref['r'] != 0)]
    assert nz.size > 0 and nz.min() > 1e-9
    theta = torch.tensor(kw['theta'], dtype=torch.float64, requires_grad=True)
    R = YG.reg_torch(t, x, y, voted, kw['calib'], kw['model'], theta, kw['t_ref'], kind, depth=kw.get('depth'))
    (g,) = torch.autograd.grad(R, theta)
    fx, fy, cx, cy = kw['calib']
    uu, vv = np.abs((x[voted].astype(np.float64) - cx) / fx), np.abs((y[voted].astype(np.float64) - cy) / fy)
    rho = 1.0 / kw['depth'][y[voted], x[voted]].astype(np.float64) if kw['model'] == 'rigid' else 0.0 * uu
    A = np.maximum(1.0, np.maximum(np.maximum(uu, vv), rho)) * max(1.0, max(abs(v) for v in kw['theta']))
    dt = np.abs(t[voted] - kw['t_ref'])
    tol = 64 * GC.U * float((4 * dt * A + 8 * dt * dt * A * A).mean())
    b = GC.bounds(case, ref)
    assert abs(float(R.detach()) - ref['R']) <= b['R'] + tol
    assert np.all(np.abs(g.numpy() - ref['dR']) <= b['dR'] + tol), (g.numpy(), ref['dR'], tol)
    assert tol + b['dR'].max() < 1e-9 * np.abs(ref['dR']).max()                         # the bound still tells right from wrong


@pytest.mark.parametrize("variant,kinds", [('c11_u', GC.KINDS), ('det_plus', ('deformation',)), ('over_N', GC.KINDS)])
def test_wrong_statements_leave_the_bound(variant, kinds):
    """on 'rigid-45x61_N700' (about a tenth of its events drop, theta within +-1) each wrong statement misses the route's R or
    dR by more than a thousand bounds, while the route stays inside the bound of the right one"""
    src, case = GC.BY_ID['rigid-45x61_N700']
    assert GC.base_reference(src, case)['dropped'].sum() > 20
    for kind in kinds:
        good, wrong = GC.reference(src, case, kind), GC.reference(src, case, kind, variant=variant)
        rs = _route(src, case, reg=kind)[4]
        b = GC.bounds(case, good)
        assert abs(rs[0] - good['R']) <= b['R'] and np.all(np.abs(rs[2:] - good['dR']) <= b['dR'])
        assert abs(rs[0] - wrong['R']) > 1000 * b['R'], (variant, kind)
        assert np.abs(rs[2:] - wrong['dR']).max() > 1000 * b['dR'].max(), (variant, kind)
    if variant == 'det_plus':                                              # the divergence has no such term
        assert GC.reference(src, case, 'divergence', variant=variant)['R'] == GC.reference(src, case, 'divergence')['R']


def test_without_translation_the_regulariser_is_the_rotation_models():
    """v = 0 and every depth valid: rho multiplies an exact zero, the same events vote, and (R, M, dR[:3]) are 'rotation's bits"""
    from evennicer_slam_amd import event_cmax as M
    for name in ('45x61_N700', '45x61_N257', '8x9_N65537'):
        case = {c['name']: c for c in RC.CASES}[name]
        kw = RC.arguments(case)
        depth = np.where(np.isfinite(kw['depth']) & (kw['depth'] > 0), kw['depth'], np.float32(1.25)).astype(np.float32)
        theta = kw['theta'][:3] + [0.0, 0.0, 0.0]
        common = dict(H=kw['H'], W=kw['W'], calib=kw['calib'], t_ref=kw['t_ref'], taps=kw['taps'], signed=kw['signed'])
        for kind in GC.KINDS:
            rig = M.cmax_numpy(*RC.stream(case), model='rigid', theta=theta, depth=depth, reg=kind, **common)[4]
            rot = M.cmax_numpy(*RC.stream(case), model='rotation', theta=theta[:3], reg=kind, **common)[4]
            assert rot[0] > 0 and np.array_equal(_bits(rig[:5]), _bits(rot)), (name, kind)


# ---- the Python layer --------------------------------------------------------------------------------------------------------------
def _planted(seed):
    from evennicer_slam_amd.event_stream import EventStream
    return EventStream(*RC.planted_stream(seed)), torch.from_numpy(RC.rec_depth())


def test_without_reg_everything_returns_what_it_did():
    from evennicer_slam_amd import event_cmax as M
    stream, depth = _planted(0)
    kw = dict(H=CC.REC_H, W=CC.REC_W, t_ref=0.0, ksize=CC.REC_K, depth=depth)
    res = M.estimate_motion(stream, CC.REC_CALIB, 'rigid', iters=2, **kw)
    assert set(res) == {'theta', 'trace', 'thetas', 'evals', 't_ref'}
    f, g = M.contrast(stream, CC.REC_CALIB, 'rigid', res['theta'], **kw)
    assert f == res['trace'][-1] and g.shape == (6,)
    assert len(M._evaluate(stream, CC.REC_H, CC.REC_W, CC.REC_CALIB, 'rigid', res['theta'], 0.0, [1.0], False, True, depth=depth)) == 4
    # with one: F = f - w R and its gradient, R and dR from `regulariser`; estimate_motion's extra keys
    for kind in GC.KINDS:
        R, dR, Mv = M.regulariser(stream, CC.REC_CALIB, 'rigid', res['theta'], CC.REC_H, CC.REC_W, t_ref=0.0, kind=kind, depth=depth)
        assert R > 0 and dR.shape == (6,) and 0 < Mv <= len(stream)
        F, G = M.contrast(stream, CC.REC_CALIB, 'rigid', res['theta'], reg=kind, reg_weight=0.25, **kw)
        assert F == f - 0.25 * R and np.array_equal(G, g - 0.25 * dR)
        reg = M.estimate_motion(stream, CC.REC_CALIB, 'rigid', iters=3, reg=kind, reg_weight=2.0, **kw)
        assert set(reg) == set(res) | {'f_trace', 'reg_trace', 'reg_weight_abs'}
        assert reg['reg_weight_abs'] == 2.0 * reg['f_trace'][0] and len(reg['f_trace']) == len(reg['reg_trace']) == len(reg['trace'])
        assert reg['reg_trace'][0] == 0.0 and reg['trace'][0] == reg['f_trace'][0]       # theta0 = 0 has no divergence
        assert all(F_ == f_ - reg['reg_weight_abs'] * r_ for F_, f_, r_ in zip(reg['trace'], reg['f_trace'], reg['reg_trace']))
    R, dR, Mv = M.regulariser(stream, CC.REC_CALIB, 'flow', [3.0, -2.0], CC.REC_H, CC.REC_W, t_ref=0.0)
    assert R == 0.0 and dR.tolist() == [0.0, 0.0] and Mv == len(stream)
    # the dead zone of the L1 term: a weight at which no step from theta0 = 0 raises F returns theta0
    dead = M.estimate_motion(stream, CC.REC_CALIB, 'rigid', reg='divergence', reg_weight=1e6, **kw)
    assert dead['theta'] == [0.0] * 6 and len(dead['trace']) == 1


def test_refusals():
    from evennicer_slam_amd import _lib as L
    from evennicer_slam_amd import event_cmax as M
    from evennicer_slam_amd import functional as EF
    stream, depth = _planted(0)
    src, case = GC.BY_ID['rigid-hand_5x7']
    s, ok = GC.stream(src, case), GC.arguments(src, case)
    rot = dict(ok, model='rotation', theta=[0.1, 0.2, 0.3], depth=None)
    for bad in (dict(reg='curl'), dict(reg='none'), dict(reg=1)):
        with pytest.raises(L.EnslamError):
            M.cmax_numpy(*s, **dict(ok, **bad))
    with pytest.raises(L.EnslamError):                                   # a depth with a model that takes none
        M.cmax_numpy(*s, **dict(rot, depth=ok['depth'], reg='divergence'))
    assert len(M.cmax_numpy(*s, **dict(rot, reg='divergence'))) == 5
    kw = dict(H=CC.REC_H, W=CC.REC_W, t_ref=0.0, ksize=CC.REC_K)
    zero = [0.0] * 6
    for call in (lambda: M.estimate_motion(stream, CC.REC_CALIB, 'rigid', depth=depth, reg='curl', **kw),
                 lambda: M.estimate_motion(stream, CC.REC_CALIB, 'rigid', depth=depth, reg='divergence', reg_weight=float('nan'), **kw),
                 lambda: M.estimate_motion(stream, CC.REC_CALIB, 'rigid', depth=depth, reg='deformation', reg_weight=float('inf'), **kw),
                 lambda: M.estimate_motion(stream, CC.REC_CALIB, 'rotation', depth=depth, reg='divergence', **kw),
                 lambda: M.contrast(stream, CC.REC_CALIB, 'rigid', zero, depth=depth, reg='curl', **kw),
                 lambda: M.contrast(stream, CC.REC_CALIB, 'rigid', zero, depth=depth, reg='divergence', reg_weight=float('-inf'), **kw),
                 lambda: M.contrast(stream, CC.REC_CALIB, 'rotation', zero[:3], depth=depth, reg='divergence', **kw),
                 lambda: M.regulariser(stream, CC.REC_CALIB, 'rigid', zero, CC.REC_H, CC.REC_W, kind='curl', depth=depth),
                 lambda: M.regulariser(stream, CC.REC_CALIB, 'rigid', zero, CC.REC_H, CC.REC_W, kind=None, depth=depth),
                 lambda: M.regulariser(stream, CC.REC_CALIB, 'rigid', zero, CC.REC_H, CC.REC_W),
                 lambda: M.regulariser(stream, CC.REC_CALIB, 'rotation', zero[:3], CC.REC_H, CC.REC_W, depth=depth),
                 lambda: EF.event_cmax_eval(*(torch.from_numpy(v) for v in s), 5, 7, ok['calib'], 'rotation', [0.1, 0.2, 0.3], 0.0, [1.0], reg='curl'),
                 lambda: EF.event_cmax_eval(*(torch.from_numpy(v) for v in s), 5, 7, ok['calib'], 'rotation', [0.1, 0.2, 0.3], 0.0, [1.0], reg='divergence')):
        with pytest.raises(L.EnslamError):
            call()


def test_abi_exports():
    import evennicer_slam_amd as E
    from evennicer_slam_amd import event_cmax as M
    from evennicer_slam_amd import functional as EF
    header = open(os.path.join(ROOT, "include", "enslam_hip.h")).read()
    handle = E._lib.lib()
    for name in EXPORTS:
        assert name in E._lib.EXPORTS and re.search(r"\b%s\s*\(" % name, header) and hasattr(handle, name), name
    for text in ("#define ENSLAM_CMAX_RIGID 2", "#define ENSLAM_CMAX_REG_NONE 0", "#define ENSLAM_CMAX_REG_DIVERGENCE 1", "#define ENSLAM_CMAX_REG_DEFORMATION 2"):
        assert re.search(re.escape(text) + r"\b", header), text
    assert EF.EVENT_CMAX_REGS == dict(divergence=1, deformation=2) and M.REGS == ('divergence', 'deformation')
    assert len(E._lib._SIGS["enslam_event_cmax_reg_eval"][1]) == len(E._lib._SIGS["enslam_event_cmax_rigid_eval"][1]) + 3


def check_refusals(t, x, y, p, depth, N, H, W, ws, ws_bytes, iwe, blurred, stats, dropped, reg_stats):
    """Every refusal of enslam_event_cmax_reg_eval returns its code; nothing is launched (the GPU test looks at the buffers).
    The pointers only have to be non-NULL and 8-byte aligned: a refusal comes before any of them is used."""
    from evennicer_slam_amd import _lib as L
    lib = L.lib()
    EINVAL, EUNSUPPORTED = -1, -3
    nan, inf = float('nan'), float('inf')
    RIGID, ROT, FLOW = 2, 1, 0

    def call(model=RIGID, kind=1, n=N, hh=H, ww=W, cal=(80.0, 80.0, 3.0, 2.0), theta=(0.1, 0.2, 0.3, 0.4, 0.5, 0.6), t_ref=0.0, k=3, taps=None,
             ptrs=None, nbytes=ws_bytes):
        q = dict(t=t, x=x, y=y, p=p, depth=depth if model == RIGID else None, ws=ws, iwe=iwe, blurred=blurred, stats=stats, dropped=dropped,
                 reg_stats=reg_stats, theta=(ctypes.c_double * 6)(*theta), taps=(ctypes.c_double * 64)(*(taps or [1.0 / max(k, 1)] * max(k, 1))))
        q.update(ptrs or {})
        return lib.enslam_event_cmax_reg_eval(q['t'], q['x'], q['y'], q['p'], n, hh, ww, cal[0], cal[1], cal[2], cal[3], model, q['depth'],
                                              q['theta'], t_ref, 0, k, q['taps'], q['ws'], nbytes, q['iwe'], q['blurred'], q['stats'],
                                              q['dropped'], kind, q['reg_stats'], 1, None)

    for name in ('t', 'x', 'y', 'p', 'depth', 'ws', 'iwe', 'stats', 'dropped', 'reg_stats', 'theta', 'taps'):
        assert call(ptrs={name: None}) == EINVAL, name
    for kind in (0, 1, 2):                                               # what is new: the model, the kind, the depth rule
        for model in (3, -1, 7):
            assert call(model=model, kind=kind) == EINVAL
        for model in (ROT, FLOW):
            assert call(model=model, kind=kind, ptrs=dict(depth=depth)) == EINVAL, (model, kind)
        assert call(kind=kind, ptrs=dict(reg_stats=reg_stats + 4)) == EINVAL
    for kind in (3, -1, 99):
        for model in (RIGID, ROT, FLOW):
            assert call(model=model, kind=kind) == EINVAL
    assert call(n=-1) == EINVAL and call(hh=0) == EINVAL and call(ww=-3) == EINVAL
    for bad in (nan, inf, -inf):
        for i in range(6):
            theta = [0.1, 0.2, 0.3, 0.4, 0.5, 0.6]
            theta[i] = bad
            assert call(theta=theta) == EINVAL, (i, bad)
            if i < 3:
                assert call(model=ROT, theta=theta) == EINVAL, (i, bad)
        assert call(t_ref=bad) == EINVAL and call(taps=[0.25, bad, 0.25]) == EINVAL
        for i in range(4):
            cal = [80.0, 80.0, 3.0, 2.0]
            cal[i] = bad
            assert call(cal=cal) == EINVAL
    assert call(cal=(0.0, 80.0, 3.0, 2.0)) == EINVAL and call(cal=(80.0, -0.0, 3.0, 2.0)) == EINVAL
    assert call(k=0) == EINVAL and call(k=4) == EINVAL and call(k=-3) == EINVAL and call(k=32) == EINVAL
    assert call(k=33) == EUNSUPPORTED
    need = ctypes.c_int64(-1)
    for model in (RIGID, ROT, FLOW):
        assert lib.enslam_event_cmax_reg_workspace(H, W, N, model, ctypes.byref(need)) == 0 and 0 < need.value <= ws_bytes
        assert call(model=model, nbytes=need.value - 8) == EINVAL and call(model=model, nbytes=0) == EINVAL
    for name, base in (('ws', ws), ('iwe', iwe), ('blurred', blurred), ('stats', stats), ('dropped', dropped)):
        assert call(ptrs={name: base + 4}) == EINVAL, name
    assert call(n=1 << 31) == EUNSUPPORTED and call(hh=65537) == EUNSUPPORTED and call(ww=65537) == EUNSUPPORTED
    assert call(hh=65536, ww=8192) == EUNSUPPORTED
    n = ctypes.c_int64(-1)
    assert lib.enslam_event_cmax_reg_workspace(H, W, N, RIGID, None) == EINVAL
    for args, code in (((0, W, N, RIGID), EINVAL), ((H, W, -1, ROT), EINVAL), ((H, W, N, 3), EINVAL), ((H, W, N, -1), EINVAL),
                       ((H, W, 1 << 31, FLOW), EUNSUPPORTED), ((65537, 1, N, RIGID), EUNSUPPORTED), ((32768, 16384, N, ROT), EUNSUPPORTED)):
        assert lib.enslam_event_cmax_reg_workspace(*args, ctypes.byref(n)) == code and n.value == -1, args
    # the existing formula with 1 + P partials per workgroup of events; the four existing entries keep theirs
    for model, P in ((RIGID, 6), (ROT, 3), (FLOW, 2)):
        assert lib.enslam_event_cmax_reg_workspace(45, 61, 700, model, ctypes.byref(n)) == 0 and n.value == (3 * 2745 + max(11, 3 * (1 + P))) * 8
        assert lib.enslam_event_cmax_reg_workspace(5, 7, 20000, model, ctypes.byref(n)) == 0 and n.value == (3 * 35 + 79 * (1 + P)) * 8
    assert lib.enslam_event_cmax_rigid_workspace(5, 7, 20000, ctypes.byref(n)) == 0 and n.value == (3 * 35 + 79 * 6) * 8
    assert lib.enslam_event_cmax_workspace(5, 7, 20000, 3, ctypes.byref(n)) == 0 and n.value == (3 * 35 + 79 * 3) * 8
    for P in (4, 5, 6, 7):
        assert lib.enslam_event_cmax_workspace(H, W, N, P, ctypes.byref(n)) == EINVAL
    # ... and the old pair still refuses the third model
    th, tp = (ctypes.c_double * 6)(0.1, 0.2, 0.3, 0.4, 0.5, 0.6), (ctypes.c_double * 3)(0.25, 0.5, 0.25)
    assert lib.enslam_event_cmax_eval(t, x, y, p, N, H, W, 80.0, 80.0, 3.0, 2.0, RIGID, th, 0.0, 0, 3, tp, ws, ws_bytes, iwe, blurred, stats,
                                      dropped, 1, None) == EINVAL


def test_every_refusal_has_its_code():
    host = (ctypes.c_double * 8192)()
    a = ctypes.addressof(host)
    assert a % 8 == 0
    check_refusals(a, a, a, a, a, 10, 5, 7, a, 8192 * 8, a, a, a, a, a)


# ---- recovery --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", RC.REC_SEEDS)
def test_recovery_from_zero_at_the_window_start(seed):
    """theta0 = 0, the reference time at the START of the window.  Conditions of the input: the unregularised estimate is worse
    than no motion at all and has v_z > 10 (truth 0.4) -- the collapse.  The bars: under either regulariser at weight 8 every
    accepted step raises F, the estimate's field is nearer the truth's than zero motion's, and |v_z| < 2."""
    from evennicer_slam_amd import event_cmax as M
    stream, depth = _planted(seed)
    kw = dict(H=CC.REC_H, W=CC.REC_W, sigma=CC.SIGMA, ksize=CC.REC_K, t_ref=0.0, depth=depth)
    truth = RC.field(RC.REC_TRUTH, CC.REC_WINDOW)
    off = lambda th: float(np.linalg.norm(RC.field(th, CC.REC_WINDOW) - truth, axis=-1).mean())     # noqa: E731
    zero = off([0.0] * 6)
    plain = M.estimate_motion(stream, CC.REC_CALIB, 'rigid', **kw)
    print(seed, 'none', off(plain['theta']), plain['theta'][5], 'zero motion', zero, 'recorded', GC.REC_REG_RECORD[seed])
    assert off(plain['theta']) > zero and plain['theta'][5] > 10 and 'f_trace' not in plain
    for kind in GC.KINDS:
        res = M.estimate_motion(stream, CC.REC_CALIB, 'rigid', reg=kind, reg_weight=GC.REC_WEIGHT, **kw)
        trace = res['trace']
        print(seed, kind, 'pixels off', off(res['theta']), 'v_z', res['theta'][5], 'steps', len(trace) - 1, 'evals', res['evals'], 'R', res['reg_trace'][-1])
        assert res['thetas'][0] == [0.0] * 6 and len(trace) == len(res['thetas']) > 3
        assert all(b > a for a, b in zip(trace, trace[1:]))
        assert res['reg_weight_abs'] == GC.REC_WEIGHT * plain['trace'][0]
        assert off(res['theta']) < zero and abs(res['theta'][5]) < 2


# ---- tools -------------------------------------------------------------------------------------------------------------------------
def _tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_tools_flags(capsys, tmp_path):
    import json
    from evennicer_slam_amd.event_stream import EventStream
    tool = _tool("event_motion")
    with pytest.raises(SystemExit) as e:
        tool.main(['--help'])
    text = capsys.readouterr().out
    assert e.value.code == 0 and all(flag in text for flag in ('--reg {divergence,deformation}', '--reg-weight', '--t-ref'))
    with pytest.raises(SystemExit) as e:
        tool.main(['--demo', '3', '--reg', 'curl'])
    assert e.value.code == 2
    capsys.readouterr()
    s = EventStream(*RC.planted_stream(1))
    s.save(str(tmp_path / 'events.npz'))
    np.save(str(tmp_path / 'depth.npy'), RC.rec_depth())
    (tmp_path / 'stamps.txt').write_text("0.0\n0.1\n")
    common = ['--stream', str(tmp_path / 'events.npz'), '--size', str(CC.REC_H), str(CC.REC_W), '--calib'] + [repr(v) for v in CC.REC_CALIB] + \
             ['--stamps', str(tmp_path / 'stamps.txt'), '--model', 'rigid', '--device', 'cpu', '--depth', str(tmp_path / 'depth.npy'), '--t-ref', 'start']
    plain = tool.main(common)['rows'][0]
    out = tool.main(common + ['--reg', 'divergence', '--reg-weight', '8'])
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    row = out['rows'][0]
    assert line['reg'] == 'divergence' and line['reg_weight'] == 8.0 and 'regulariser_after' not in plain
    assert plain['theta'][5] > 10 and abs(row['theta'][5]) < 2 and row['contrast_only_after'] > row['contrast_only_before']
    assert row['contrast_after'] == row['contrast_only_after'] - row['reg_weight_abs'] * row['regulariser_after']
    synth = _tool("run_synthetic_slam")
    opts = synth.parse_args(['7', '--events', 'simulate', '--motion-prior', 'cmax', '--cmax-reg', 'divergence', '--cmax-reg-weight', '4'])[1]
    assert opts['cmax_reg'] == 'divergence' and opts['cmax_reg_weight'] == 4.0
    assert 'cmax_reg' not in synth.parse_args(['7', '--events', 'simulate', '--motion-prior', 'cmax'])[1]
    for bad in (['--events', 'simulate', '--motion-prior', 'cmax', '--cmax-reg', 'curl'], ['--events', 'simulate', '--cmax-reg', 'divergence']):
        with pytest.raises(SystemExit):
            synth.parse_args(bad)
    bench = open(os.path.join(ROOT, "tools", "bench_event_cmax.py")).read()
    assert "add_argument('--reg'" in bench and "_rigid_reg'] = dict(" in bench and 'plain_below_reg=' in bench


# ---- the prior on CPU tensors ------------------------------------------------------------------------------------------------------
def test_the_prior_with_a_regulariser_on_cpu_tensors(tmp_path_factory):
    from evennicer_slam_amd import event_cmax as M
    from evennicer_slam_amd import functional as EF
    from evennicer_slam_amd.slam import SLAM
    from tests.test_event_cmax_rigid_cpu import N_FRAMES, const_speed, demo_sequence, with_prior
    root = tmp_path_factory.mktemp('prior_reg')
    cfg, ds, poses, streams, stamps = demo_sequence(tmp_path_factory.mktemp('seq'))

    def harness(c, tag):
        slam = SLAM(c, ds, str(root / tag), device='cpu')
        for i in range(N_FRAMES):
            slam.estimate_c2w_list[i] = ds[i][-1]
        slam._last_rgbd = (0, ds[0][2])
        return slam

    track = lambda slam, idx: slam.track(idx, None, None, None, None, None, rgbd=False)          # noqa: E731  (no loss: est itself)
    keys = dict(cmax=0, few_events=0, no_depth=0, not_finite=0, no_rise=0, seconds=0.0)
    plain = harness(with_prior(cfg, 'cmax'), 'plain')
    assert plain.cmax_reg == 'none' and plain.cmax_reg_weight == 8.0 and plain.cmax_max_reg is None and plain.motion_prior_stats == keys
    assert harness(with_prior(cfg, 'const_speed', cmax_reg='divergence'), 'unused').motion_prior_stats == keys
    slam = harness(with_prior(cfg, 'cmax', cmax_reg='divergence', cmax_reg_weight=4.0), 'reg')
    assert slam.motion_prior_stats == keys
    used = 0
    for idx in (2, 3, 4):
        got = track(slam, idx)
        res = slam.motion_prior_last
        # what the harness is specified to compose: the same estimate with the regulariser, the rise asked of the pure contrast
        stream, t0, t1 = ds.event_slice(idx)
        pre = slam.estimate_c2w_list[idx - 1].double()
        theta0 = M.camera_velocity(slam.estimate_c2w_list[idx - 2], slam.estimate_c2w_list[idx - 1], t0 - ds.event_slice(idx - 1)[1])
        src, depth = slam._last_rgbd
        d = EF.depth_forecast(depth.float().contiguous(), slam.cam, EF.relative_camera_matrix(slam.estimate_c2w_list[src], pre),
                              (slam.H, slam.W), radius=slam.forecast_radius, z_near=0.0, fill=slam.forecast_fill)
        want = M.estimate_motion(stream, (slam.fx, slam.fy, slam.cx, slam.cy), 'rigid', slam.H, slam.W, theta0=theta0, t_ref=t0, depth=d,
                                 iters=slam.cmax_iters, reg='divergence', reg_weight=4.0)
        assert want['thetas'] == res['thetas'] and want['trace'] == res['trace'] and 'f_trace' in res
        if res['f_trace'][-1] > res['f_trace'][0]:
            assert torch.equal(got[:3], (pre @ M.relative_motion(res['theta'], t1 - t0)).float()[:3])
            used += 1
        else:
            assert torch.equal(got[:3], const_speed(slam, idx)[:3])
    st = slam.motion_prior_stats
    assert set(st) == set(keys) and st['cmax'] == used and st['no_rise'] == 3 - used
    # the ceiling on R: set to nothing, every estimate that rose counts as collapsed and the pose is the constant-speed one
    capped = harness(with_prior(cfg, 'cmax', cmax_reg='divergence', cmax_reg_weight=4.0, cmax_max_reg=0.0), 'capped')
    assert capped.motion_prior_stats == dict(keys, collapsed=0)
    for idx in (2, 3, 4):
        assert torch.equal(track(capped, idx)[:3], const_speed(capped, idx)[:3])
    st = capped.motion_prior_stats
    assert st['cmax'] == 0 and st['collapsed'] == used > 0 and st['no_rise'] == 3 - used
    # ... without a regulariser in the objective too (R is then evaluated once, at the estimate), and a generous one lets it through
    bare = harness(with_prior(cfg, 'cmax', cmax_max_reg=0.0), 'bare')
    loose = harness(with_prior(cfg, 'cmax', cmax_max_reg=1e9), 'loose')
    for idx in (2, 3, 4):
        assert torch.equal(track(bare, idx)[:3], const_speed(bare, idx)[:3])
        assert torch.equal(track(loose, idx)[:3], track(plain, idx)[:3])
    assert bare.motion_prior_stats['collapsed'] + bare.motion_prior_stats['no_rise'] == 3 and bare.motion_prior_stats['collapsed'] > 0
    assert loose.motion_prior_stats['collapsed'] == 0 and loose.motion_prior_stats['cmax'] == plain.motion_prior_stats['cmax'] > 0
    for bad in (dict(cmax_reg='curl'), dict(cmax_reg_weight=float('nan'))):
        with pytest.raises(ValueError, match='cmax_reg'):
            SLAM(with_prior(cfg, 'cmax', **bad), ds, str(root / 'bad'), device='cpu')
