"""Cases of the event-collapse regularisers (enslam_event_cmax_reg_eval), the conditions each has to meet, and the tolerance rule.

The cases are the twelve rigid cases of tests/event_cmax_rigid_cases.py and the rotation and flow cases of
tests/event_cmax_cases.py, imported as they are (1 x 1 under a blur wider than the image, the planted 5 x 7 and 9 x 12 drops,
45 x 61 with N = 0, 1, 255, 256, 257, 700 in the three orders, the 65 537-event third tree level, one pixel under every vote),
each under both kinds, and five of this file's own:
    reg_hand        one rigid event whose every operand is a short binary fraction, worked by hand for both kinds (HAND below)
    reg_t_ref       three rigid events, one of them AT the reference time: its d is -0.0 or 0.0 exactly, sgn is 0
    reg_theta_zero  300 rotation events under theta = 0: every d is zero, R = 0, and every dr is a zero
    reg_all_dropped six rigid events none of which votes (depth 0, NaN time, x past the sensor): M = 0, R = dR = 0
    reg_both_signs  300 rotation events under theta = (1, 0, 0): d_div = -3 dt v changes sign with dt and with v inside the
                    first block of 256

THE TOLERANCE RULE, derived as tests/event_cmax_cases.py derives its SUM bound (u = 2^-53).  The yardstick
(tests/event_cmax_reg_numpy.py) performs the header's operations in the header's order, so the per-event r and dr have the
bound 0; the routes and the yardstick differ only in SUM (the stated tree against math.fsum) and agree on the integer M.  A value
of the tree passes DEPTH(N) = 16 + max(ceil(N / 65536), 1) rounding additions, the yardstick's fsum rounds once and the division
by M once more:
    E_R = (DEPTH(N) + 2) u sum|r| / M            E_dR[k] = (DEPTH(N) + 2) u sum|dr[k]| / M
evaluated on the yardstick of the case; nothing is fitted to a route.  M = 1 (one term, a tree of zeros, a division by one) has
the bound 0 in effect: the hand-worked values are asserted with ==.

The recovery record (REC_REG_RECORD) stands beside RC.REC_RECORD: see below."""
import numpy as np

from tests import event_cmax_cases as CC
from tests import event_cmax_numpy as Y
from tests import event_cmax_reg_numpy as YG
from tests import event_cmax_rigid_cases as RC
from tests import event_cmax_rigid_numpy as YR

KINDS = YG.KINDS
U = CC.U


def _own(name, H, W, N, model):
    return dict(name=name, H=H, W=W, N=N, model=model, seed=0, signed=False, k=1, order='shuffled', kind='reg')


OWN = [_own('reg_hand', 5, 7, 1, 'rigid'), _own('reg_t_ref', 5, 7, 3, 'rigid'), _own('reg_theta_zero', 45, 61, 300, 'rotation'),
       _own('reg_all_dropped', 5, 7, 6, 'rigid'), _own('reg_both_signs', 45, 61, 300, 'rotation')]
# (source, case): 'rigid' and 'base' cases keep their own names; the name of a case here is unique with its source
CASES = [('rigid', c) for c in RC.CASES] + [('base', c) for c in CC.CASES] + [('own', c) for c in OWN]
IDS = [f"{src}-{c['name']}" for src, c in CASES]
BY_ID = dict(zip(IDS, CASES))

# reg_hand: 5 x 7, fx = fy = 2, (cx, cy) = (3, 2), the pixel (4, 0) of depth 1 an eighth of a second after t_ref = 0 under
# theta = (1/2, -1/4, 1/2, 1, -1/2, 2): u = 1/2, v = -1, rho = 1, dt = 1/8.
#   c11 = (-1/2 + 1/4) + 2 = 7/4        c22 = (-1 + 1/8) + 2 = 9/8        c12 = 1/4 + 1/2 = 3/4        c21 = -1/4 - 1/2 = -3/4
#   d_div = -(1/8)(23/8) = -23/64       d_def = -23/64 + (1/64)(63/32 + 9/16) = -23/64 + 81/2048 = -655/2048
#   (det: (1 - 7/32)(1 - 9/64) + (1/64)(9/16) = 1375/2048 + 18/2048 = 1393/2048 = 1 - 655/2048)
#   e11 = (-1, -1, 0, 0, 0, 1), e22 = (-2, -1/2, 0, 0, 0, 1), e12 = (1/2, 0, 1, 0, 0, 0), e21 = (0, 1, -1, 0, 0, 0)
#   dd_div = (3/8, 3/16, -0, -0, -0, -1/4)
#   dd_def = dd_div + (1/64)(-17/4, -11/4, 3/2, 0, 0, 23/8) = (79/256, 37/256, 3/128, 0, 0, -105/512)
# sgn(d) = -1 for both kinds and M = 1: R = |d|, dR = -dd.
HAND = dict(divergence=dict(R=23 / 64, dR=[-3 / 8, -3 / 16, 0.0, 0.0, 0.0, 1 / 4]),
            deformation=dict(R=655 / 2048, dR=[-79 / 256, -37 / 256, -3 / 128, 0.0, 0.0, 105 / 512]))


def stream(src, case):
    """(t float64, x uint16, y uint16, p uint8)"""
    if src == 'rigid':
        return RC.stream(case)
    if src == 'base':
        return CC.stream(case)
    name = case['name']
    if name == 'reg_hand':
        t, x, y, p = [0.125], [4], [0], [1]
    elif name == 'reg_t_ref':
        t, x, y, p = [0.125, 0.0, -0.0625], [4, 2, 5], [0, 4, 3], [1, 0, 1]
    elif name == 'reg_all_dropped':
        t, x, y, p = [0.125, 0.0, float('nan'), 0.25, 0.125, 0.0], [4, 2, 5, 7, 0, 3], [0, 4, 3, 1, 5, 2], [1, 0, 1, 0, 1, 0]
    else:
        return CC.stream(dict(case, kind='random', seed=31 if name == 'reg_theta_zero' else 32))
    return (np.asarray(t, dtype=np.float64), np.asarray(x).astype(np.uint16), np.asarray(y).astype(np.uint16), np.asarray(p).astype(np.uint8))


def arguments(src, case):
    """the keyword arguments of the numpy route beside the stream and `reg` (model among them; depth for 'rigid')"""
    if src == 'rigid':
        return dict(RC.arguments(case), model='rigid')
    if src == 'base':
        return CC.arguments(case)
    name = case['name']
    kw = dict(H=case['H'], W=case['W'], model=case['model'], taps=[1.0], signed=False)
    if case['model'] == 'rigid':
        depth = RC.depth_image(dict(case, kind='hand'))
        if name == 'reg_all_dropped':
            depth = np.zeros_like(depth)
        return dict(kw, calib=(2.0, 2.0, 3.0, 2.0), theta=list(RC.HAND_THETA), t_ref=0.0, depth=depth)
    theta = [0.0, 0.0, 0.0] if name == 'reg_theta_zero' else [1.0, 0.0, 0.0]
    return dict(kw, calib=CC.calib(dict(case, kind='random')), theta=theta, t_ref=0.05)


_BASE, _REF = {}, {}


def base_reference(src, case):
    """the existing yardstick of the case (the image, the counters, which events vote), computed once and shared"""
    if src == 'rigid':
        return RC.reference(case)
    if src == 'base':
        return CC.reference(case)
    if case['name'] not in _BASE:
        kw = arguments(src, case)
        if kw['model'] == 'rigid':
            _BASE[case['name']] = YR.cmax(*stream(src, case), **{k: v for k, v in kw.items() if k != 'model'})
        else:
            _BASE[case['name']] = Y.cmax(*stream(src, case), **kw)
    return _BASE[case['name']]


def reference(src, case, kind, variant=None):
    """the regulariser's yardstick of the case, computed once and shared (never written to)"""
    key = (src, case['name'], kind, variant)
    if key not in _REF:
        kw = arguments(src, case)
        t, x, y, _ = stream(src, case)
        _REF[key] = YG.reg(t, x, y, base_reference(src, case)['voted'], kw['calib'], kw['model'], kw['theta'], kw['t_ref'], kind,
                           depth=kw.get('depth'), variant=variant)
    return _REF[key]


def bounds(case, ref):
    """dict(R, dR [P]) of the rule above on the yardstick `ref`"""
    M = ref['M']
    if M == 0:
        return dict(R=0.0, dR=np.zeros(ref['dr'].shape[1]))
    lev = CC.depth(max(case['N'], 1)) + 2
    return dict(R=lev * U * float(np.abs(ref['r']).sum()) / M, dR=lev * U * np.abs(ref['dr']).sum(axis=0) / M)


def check_conditions(src, case, base, refs):
    """what the case was built to exercise, asserted on the yardsticks; refs = {kind: reference}"""
    if src == 'rigid':
        RC.check_conditions(case, base)
    elif src == 'base':
        CC.check_conditions(case, base)
    N = case['N']
    voted = base['voted']
    for kind, ref in refs.items():
        assert ref['M'] == int(voted.sum()) == N - int(base['dropped'].sum())
        assert not ref['r'][~voted].any() and not ref['dr'][~voted].any()
        if case['model'] == 'flow':
            assert ref['R'] == 0.0 and not ref['dR'].any() and not ref['r'].any()
    name = case['name']
    if src == 'own':
        t = stream(src, case)[0]
        kw = arguments(src, case)
        if name == 'reg_hand':
            assert voted.all() and (base['xw'][0], base['yw'][0]) == (4.109375, 0.21875)
        if name == 'reg_t_ref':
            assert voted.all() and t[1] == kw['t_ref'] and any(kw['theta'])
            for ref in refs.values():
                assert ref['r'][1] == 0.0 and not ref['dr'][1].any() and ref['r'][0] > 0 and ref['r'][2] > 0
        if name == 'reg_theta_zero':
            assert not any(kw['theta']) and voted.sum() == N
            for ref in refs.values():
                assert ref['R'] == 0.0 and not ref['r'].any() and not ref['dr'].any()
        if name == 'reg_all_dropped':
            assert not voted.any() and base['dropped'].tolist() == [1, 2, 0, 3]
            for ref in refs.values():
                assert ref['M'] == 0 and ref['R'] == 0.0 and not ref['dR'].any()
        if name == 'reg_both_signs':
            fy, cy = kw['calib'][1], kw['calib'][3]
            y = stream(src, case)[2]
            d = -3.0 * (t - kw['t_ref']) * ((y.astype(np.float64) - cy) / fy)
            first = voted[:256]
            assert (d[:256][first] > 0).sum() > 20 and (d[:256][first] < 0).sum() > 20 and N > 256
            dr = refs['divergence']['dr'][:256]                              # sgn(d) dd: along w_x it is |d|, along w_y 3 sgn(d) dt u
            assert np.all(dr[:, 0] >= 0) and (dr[:, 1] > 0).sum() > 20 and (dr[:, 1] < 0).sum() > 20


# ---- the recovery test -------------------------------------------------------------------------------------------------------
# The planted streams of tests/event_cmax_rigid_cases.py (REC_SEEDS, 45 x 61, about a thousand events, window 0.1 s) from
# theta0 = 0 with the reference time at the window's START, where the pose prior has its depth image.  `off` is the mean
# end-of-window pixel distance of the estimate's field from the truth's (RC.field); zero motion scores 4.607.
# As the CPU route of estimate_motion gave it (a record beside RC.REC_RECORD; the bars are in the test):
#   seed: (off, v_z) without a regulariser, then (off, v_z) under 'divergence' and under 'deformation' at reg_weight 8
REC_REG_RECORD = {0: ((39.99, 36.6), (1.62, 0.030), (1.85, 0.11)), 1: ((35.81, 31.8), (1.70, 0.045), (1.81, 0.17)),
                  2: ((39.88, 34.9), (1.86, 0.040), (1.54, 0.13))}     # truth: v_z = 0.4
REC_WEIGHT = 8.0
