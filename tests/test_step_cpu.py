"""The yardsticks of tests/step_numpy.py against independent float64 formulations (the project's own torch statements under
float64 autograd, torch.optim.Adam on float64 tensors), the conditions the cases of tests/step_cases.py are built to meet,
and the measured Adam tolerance.  No GPU."""
import numpy as np
import pytest
import torch

from evennicer_slam_amd import common
from tests import step_cases as C
from tests import step_numpy as Y

f32 = np.float32
T64 = lambda a: torch.from_numpy(np.array(a, np.float64))
CT_NAMES = tuple(C.CAMERA_TENSORS)


def close(a, b, rel=1e-12):
    """max-norm agreement: |a - b| <= rel * max|b| element by element"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return bool((np.abs(a - b) <= rel * max(float(np.abs(b).max()) if b.size else 0.0, 1e-300)).all()) or (a.size == 0 and b.size == 0)


# ---- camera tensor -> rays --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CT_NAMES)
def test_pose_rays_float64_version_is_the_projects_statements(name):
    for n in C.N_EDGES:
        c = C.pose_case(name, n)
        c2w = common.get_camera_from_tensor(T64(c.ct))
        ro, rd = common.get_rays_from_uv(T64(c.px.pi), T64(c.px.pj), c2w, 680, 1200, *C.CAM, 'cpu')
        assert close(c.rd64, rd.numpy()) and np.array_equal(ro.numpy(), np.broadcast_to(c.ct[4:7].astype(np.float64), (n, 3)))


@pytest.mark.parametrize("name", CT_NAMES)
def test_pose_rays_mirror_is_float32_arithmetic_of_the_same_rays(name):
    """the float32 mirror keeps the distance from float64 that the GPU test asks of the kernel: 8 * 2^-24 * (|d0||R_a0| +
    |d1||R_a1| + |R_a2|); and it is float32 all the way (bit patterns of ro are the translation's)"""
    worst = 0.0
    for n in C.N_EDGES:
        c = C.pose_case(name, n)
        assert c.rd.dtype == np.float32 and c.ro.dtype == np.float32
        assert Y.bits_equal(c.ro, np.broadcast_to(c.ct[4:7], (n, 3)))
        err = np.abs(c.rd.astype(np.float64) - c.rd64) / (2.0 ** -24 * c.scale)
        worst = max(worst, float(err.max()))
        assert (err <= 8).all()
    print(f"{name}: mirror within {worst:.2f} x 2^-24 x scale of float64")
    if name in ('identity', 'half_turn'):
        assert worst <= 2.0                     # exact rotation entries: only the directions and the two sums round


@pytest.mark.parametrize("name", CT_NAMES)
def test_pose_gradient_yardstick_matches_float64_autograd(name):
    """the transcribed chain against autograd of get_camera_from_tensor + get_rays_from_uv in float64, fed the float32-rounded
    directions (as pixel coordinates of a camera with fx = fy = 1, cx = cy = 0)"""
    for n in C.N_EDGES:
        c = C.pose_case(name, n)
        d0, d1 = Y.directions32(c.px.pi, c.px.pj, *C.CAM)
        for which in C.COTANGENTS:
            g_ro, g_rd = C.cotangents(c.px, which)
            ct = T64(c.ct).requires_grad_(True)
            ro, rd = common.get_rays_from_uv(T64(d0), T64(-d1), common.get_camera_from_tensor(ct), 0, 0, 1.0, 1.0, 0.0, 0.0, 'cpu')
            loss = ct.sum() * 0
            if g_ro is not None:
                loss = loss + (ro * T64(g_ro)).sum()
            if g_rd is not None:
                loss = loss + (rd * T64(g_rd)).sum()
            loss.backward()
            want = ct.grad.numpy()
            g, A = c.grad[which]
            assert (A >= np.abs(g) * (1 - 1e-12)).all()
            # the quaternion part to 1e-12 of its largest component (one component of an axis-aligned quaternion is an exact
            # cancellation: scaling q does not change the rotation), the translation part likewise
            assert close(g[:4], want[:4]) and close(g[4:], want[4:]), (n, which)
            if g_rd is None:
                assert not g[:4].any() and not A[:4].any()
            if g_ro is None:
                assert not g[4:].any() and not A[4:].any()


def test_pose_cotangents_do_not_cancel():
    worst = 0.0
    for n in C.N_EDGES:
        px = C.pose_pixels(n)
        G, gT, GA, gTA = Y.pose_sums(px.pi, px.pj, *C.CAM, px.g_ro, px.g_rd)
        ratio = np.concatenate([(GA / np.abs(G)).ravel(), gTA / np.abs(gT)])
        worst = max(worst, float(ratio.max()))
        assert (ratio <= C.CANCEL_CAP).all(), n
        assert float(np.abs(px.pi - C.CAM[2]).min()) > 0 and float(np.abs(px.pj - C.CAM[3]).min()) > 0
    t = C.tracker_grad_case()
    G, gT, GA, gTA = Y.pose_sums(t.px.pi, t.px.pj, *t.case.cam, t.px.g_ro, t.px.g_rd)
    ratio = np.concatenate([(GA / np.abs(G)).ravel(), gTA / np.abs(gT)])
    assert (ratio <= C.CANCEL_CAP).all()
    print(f"largest A / |value| of a reduced sum: {max(worst, float(ratio.max())):.1f}")


def test_camera_tensors_cover_the_quaternion_norms():
    q = {k: np.linalg.norm(np.array(v[:4], f32).astype(np.float64)) for k, v in C.CAMERA_TENSORS.items()}
    assert abs(q['norm2_0.9'] ** 2 - 0.9) < 1e-6 and abs(q['norm_2.7'] - 2.7) < 0.05 and abs(q['norm_0.06'] - 0.06) < 0.002
    assert q['identity'] == 1.0 and q['half_turn'] == 1.0
    for v in C.CAMERA_TENSORS.values():
        assert all(float(t) != round(float(t), 1) for t in v[4:]) or v is C.CAMERA_TENSORS['norm2_0.9']


# ---- prefilter --------------------------------------------------------------------------------------------------------------
def _torch_prefilter(ro, rd, gd):
    ro, rd, gd = T64(ro), T64(rd), torch.from_numpy(np.array(gd))
    t = (T64(C.TR_BOUND).unsqueeze(0) - ro.unsqueeze(-1)) / rd.unsqueeze(-1)                # Tracker.py:164-170
    t, _ = torch.min(torch.max(t, dim=2)[0], dim=1)
    inside = t >= gd
    m = torch.where(inside, gd, gd.new_zeros(())).max().reshape(1)
    return t.numpy(), inside.numpy(), torch.cat([m, m * 1.2]).numpy()


@pytest.mark.parametrize("kind", C.TR_KINDS)
def test_prefilter_yardstick_and_tracker_cases(kind):
    for n in C.TR_N:
        c = C.tracker_case(kind, n)
        t, inside, dmax = _torch_prefilter(c.ro, c.rd, c.gd)
        assert np.array_equal(inside, c.inside) and Y.bits_equal(dmax, c.dmax)
        assert c.gd.dtype == np.float32 and c.gc.dtype == np.float32 and c.idx.min() >= 0 and c.idx.max() < C.WIN_H * C.WIN_W
        k = int(c.inside.sum())
        if kind == 'last_max':
            assert c.inside[n - 1] and c.gd[n - 1] == c.dmax[0] > 0
            assert n == 1 or (0 < k < n and np.where(c.inside[:-1], c.gd[:-1], 0).max() < c.gd[n - 1])   # the last ray decides
            assert n == 1 or c.dmax_all[0] > c.dmax[0]          # ... and the mask matters: a dropped ray has a larger depth
        if kind == 'none_inside':
            assert k == 0 and Y.bits_equal(c.dmax, np.zeros(2, f32))
        if kind in ('zero_component', 'on_face'):
            at = n // 2
            assert c.idx[at] == C.PRINCIPAL and c.rd[at, 0] == 0 and c.rd[at, 1] == 0 and c.rd[at, 2] == -1
        if kind == 'zero_component':
            assert np.isinf(t).sum() == 0 and not np.isnan(t).any() and c.inside[n // 2] == (t[n // 2] >= c.gd[n // 2])
            assert n == 1 or 0 < k < n
        if kind == 'on_face':
            assert np.isnan(t[n // 2]) and not c.inside[n // 2]                 # 0 / 0: outside, whatever its depth
            assert n == 1 or 0 < k < n


def test_draw_table_rows_differ():
    d = C.draw_table()
    assert d.idx.shape == (C.N_DRAWS, C.DRAW_N) and C.DRAW_CALLS > C.N_DRAWS
    for a in range(C.N_DRAWS):
        for b in range(a):
            assert not np.array_equal(d.rows[a].gd, d.rows[b].gd) and not np.array_equal(d.rows[a].inside, d.rows[b].inside)


# ---- losses -----------------------------------------------------------------------------------------------------------------
def _torch_losses(c):
    """the reference's statements in float64 with autograd: (mapper loss, tracker loss, their colour terms, gradients)"""
    out = {}
    for key, w in (('map', C.W_MAPPER), ('trk', C.W_TRACKER)):
        d = T64(c.depth).requires_grad_(True)
        col = T64(c.color).requires_grad_(True) if c.color is not None else None
        gd, gc, unc = T64(c.gd), T64(c.gc), T64(c.unc)
        mask = gd > 0
        w = float(f32(w))
        if key == 'map':                                                                     # Mapper.py:553-562
            loss = torch.abs(gd - d)[mask].sum()
            cterm = w * torch.abs(gc - col).sum() if col is not None else None
        else:                                                                                # Tracker.py:187-195
            loss = (torch.abs(gd - d) / torch.sqrt(unc + 1e-10))[mask].sum()
            cterm = w * torch.abs(gc - col)[mask].sum() if col is not None else None
        if cterm is not None:
            loss = loss + cterm
        (loss * C.G_UP).backward()
        out[key] = (loss.item(), cterm.item() if cterm is not None else 0.0, d.grad.numpy(),
                    col.grad.numpy() if col is not None else None)
    return out


@pytest.mark.parametrize("kind", C.LOSS_KINDS)
def test_loss_yardsticks_match_the_float64_statements(kind):
    for n in C.LOSS_N:
        if n == 0 and kind not in ('random', 'no_color'):
            continue
        c = C.loss_case(kind, n)
        ref = _torch_losses(c)
        for key in ('map', 'trk'):
            val, A, g_depth, g_color = getattr(c, key)
            want, cterm, wd, wc = ref[key]
            assert A == val >= 0.0                              # sums of absolute values
            # the depth term to 1e-12; the colour term is float32 arithmetic per ray in the kernels (difference, two sums
            # and, in the mapper loss, the product with w): 4 roundings of 2^-24 relative to the colour term
            assert abs(val - want) <= 1e-12 * abs(want) + 4 * 2.0 ** -24 * cterm, (key, n)
            assert g_depth.dtype == np.float64 and (np.abs(g_depth - wd) <= 1e-12 * np.abs(wd)).all()
            assert np.array_equal(g_depth == 0, wd == 0)
            assert (g_color is None) == (c.color is None)
            if g_color is not None:
                assert g_color.dtype == np.float32
                assert (np.abs(g_color - wc) <= 2 * 2.0 ** -24 * np.abs(wc)).all()        # fl32(g) and its product with w
                gw = f32(C.G_UP) * f32(C.W_MAPPER if key == 'map' else C.W_TRACKER)
                assert set(np.unique(np.abs(g_color))) <= {f32(0.0), gw}


def test_loss_cases_hold_what_they_are_for():
    for n in C.LOSS_N[1:]:
        k = np.arange(n)
        c = C.loss_case('holes', n)
        assert n < 7 or (0 < (c.gd == 0).sum() <= n // 7 + 1)
        assert n < 97 or (c.gd < 0).any()
        c = C.loss_case('all_zero_no_color', n)
        assert not c.gd.any() and c.color is None and c.map[0] == 0.0 and c.trk[0] == 0.0
        c = C.loss_case('all_zero', n)
        assert c.map[0] > 0.0 and c.trk[0] == 0.0               # the mapper's colour term does not look at the depth
        assert c.map[3].any() and not c.trk[3].any()
        c = C.loss_case('depth_equal', n)
        same = c.depth == c.gd.astype(np.float64)
        assert same.sum() == (k % 3 == 1).sum() and not c.map[2][same].any() and not c.trk[2][same].any()
        c = C.loss_case('color_equal', n)
        assert n < 8 or 0 < (c.color == c.gc).sum() < 3 * n
        c = C.loss_case('unc_zero', n)
        assert n < 4 or (c.unc == 0).any()
        c = C.loss_case('tail', n)                              # the last element decides: without it the loss is exactly 0
        for key, fn, w in (('map', Y.rgbd_loss, C.W_MAPPER), ('trk', Y.tracker_loss, C.W_TRACKER)):
            assert getattr(c, key)[0] >= 999.0
            args = [c.depth[:-1]] + ([c.unc[:-1]] if key == 'trk' else []) + [c.color[:-1], c.gd[:-1], c.gc[:-1], w]
            assert fn(*args)[0] == 0.0
    assert C.loss_case('random', 0).map[0] == 0.0 and C.loss_case('random', 0).trk[0] == 0.0


# ---- Adam -------------------------------------------------------------------------------------------------------------------
def _torch_adam(p0, grads, lrs, dtype, mask=None):
    """torch.optim.Adam on CPU tensors of `dtype`; with a mask the parameter is the masked rows (Mapper.py:343-361).  Returns
    the parameter after every step, float64 [T, ...] (unmasked rows keep p0)."""
    rows = slice(None) if mask is None else torch.from_numpy(np.asarray(mask).astype(bool))
    full = torch.from_numpy(np.array(p0)).to(dtype)
    out = []
    if mask is not None and not np.asarray(mask).any():
        return np.stack([full.double().numpy()] * len(lrs))
    p = full[rows].clone().requires_grad_(True)
    opt = torch.optim.Adam([p], lr=0.0)
    for g, lr in zip(grads, lrs):
        opt.param_groups[0]['lr'] = lr
        p.grad = torch.from_numpy(np.array(g)).to(dtype)[rows].clone()
        opt.step()
        now = full.clone()
        now[rows] = p.detach()
        out.append(now.double().numpy())
    return np.stack(out)


def _adam_runs():
    """(label, p0, grads, lrs, mask, yardstick p trajectory) of every Adam case"""
    for name in C.ADAM_LISTS:
        c = C.adam_list(name)
        for k in range(len(c.numels)):
            yield f"{name}[{k}]", c.p0[k], c.grads[k], C.ADAM_LRS, None, c.ref[k][0]
    for V in C.GRID_V:
        for kind in C.GRID_MASKS:
            c = C.grid_case(V, kind)
            yield f"grid{V}/{kind}", c.p0, c.grads, c.lrs, c.mask, c.ref[0]
    for k, c in enumerate(C.four_grids()):
        if c.steps:
            yield f"four[{k}]", c.p0, c.grads[c.first:], [c.lr] * c.steps, c.mask, c.ref[0]


def test_adam_yardstick_matches_torch_adam_in_float64():
    for label, p0, grads, lrs, mask, ref in _adam_runs():
        got = _torch_adam(p0, grads, lrs, torch.float64, mask)
        assert (np.abs(got - ref) <= 1e-12 * np.maximum(np.abs(ref), 1.0)).all(), label
        if mask is not None:
            off = ~np.asarray(mask).astype(bool)
            assert all(np.array_equal(ref[t][off], np.asarray(p0, np.float64)[off]) for t in range(len(lrs))), label


def test_adam_moments_of_the_yardstick():
    """m and v by their closed forms (the sums the recurrences unroll to), masked rows untouched, a later first step"""
    c = C.grid_case(65, 'pattern')
    _, m, v = c.ref
    g = c.grads.astype(np.float64)
    T = len(g)
    on = c.mask.astype(bool)
    m_want = sum(0.9 ** (T - 1 - s) * 0.1 * g[s] for s in range(T))
    v_want = sum(0.999 ** (T - 1 - s) * 0.001 * g[s] ** 2 for s in range(T))
    assert close(m[-1][on], m_want[on]) and close(v[-1][on], v_want[on])
    assert not m[-1][~on].any() and not v[-1][~on].any()
    a = Y.adam(c.p0, c.grads[:1], [0.1], start_step=4)[0][0]
    b = Y.adam(c.p0, c.grads[:1], [0.1])[0][0]
    gg = g[0]
    want = c.p0 - (0.1 / (1 - 0.9 ** 5)) * (0.1 * gg) / (np.sqrt(0.001 * gg * gg) / np.sqrt(1 - 0.999 ** 5) + 1e-8)
    assert close(a, want) and not np.array_equal(a, b)


def test_adam_tolerance_is_measured_not_guessed():
    """float32 torch.optim.Adam (CPU) against the float64 yardstick over every Adam case, in units of
    (2^-24 max|p| + sum of the learning rates so far): the committed constant is that figure times four, give or take"""
    measured, where = 0.0, None
    for label, p0, grads, lrs, mask, ref in _adam_runs():
        got = _torch_adam(p0, grads, lrs, torch.float32, mask)
        for t in range(len(lrs)):
            e = float(np.abs(got[t] - ref[t]).max()) / C.adam_scale(ref[t], lrs[:t + 1])
            if e > measured:
                measured, where = e, (label, t)
    print(f"float32 torch Adam vs float64: {measured:.3e} at {where}; ADAM_TOL = {C.ADAM_TOL:.3e}")
    assert measured <= C.ADAM_TOL <= 8 * measured


def test_adam_cases_hold_what_they_are_for():
    assert C.ADAM_LRS[:4] == (0.0, 0.005, 0.1, 0.001) and len(C.ADAM_LRS) == 12
    assert len(C.ADAM_LISTS['seventy_two']) == 72 and set(C.ADAM_LISTS['seventy_two']) == {1, 5, 1024, 1025, 3, 2048, 33}
    for name in C.ADAM_LISTS:
        c = C.adam_list(name)
        g = np.abs(np.concatenate([x.ravel() for x in c.grads]))
        assert g[g > 0].min() < 1e-5 and g.max() > 10.0
        z = C.zero_tensor(c.numels)
        assert not c.grads[z][:2, C.ZERO_SLICE].any() and c.grads[z][2, C.ZERO_SLICE].all()
        p, m, v = c.ref[z]
        assert np.array_equal(p[1][C.ZERO_SLICE], c.p0[z][C.ZERO_SLICE].astype(np.float64))      # ... at lr = 0.005: exactly no update
        assert not np.array_equal(p[1], p[0])
    for V in (65, 693):
        m = C.grid_mask('pattern', V).astype(bool)
        assert m[62:65].all() and not m[61] and 0 < m[:8].sum() < 8 and 0.15 < m.mean() < 0.5
    assert C.grid_mask('none', 5) is None and not C.grid_mask('zeros', 5).any() and C.grid_mask('ones', 5).all()
    four = C.four_grids()
    assert [c.steps for c in four] == [3, 0, 1, 7] and [c.lr for c in four] == [0.1, 0.1, 0.0, 0.005] and four[1].ref is None


# ---- depth maximum ----------------------------------------------------------------------------------------------------------
def test_depth_max_yardstick_and_cases():
    for n in C.DMAX_N:
        for kind in C.DMAX_KINDS:
            c = C.depth_case(kind, n)
            m = torch.from_numpy(np.array(c.gd)).max().reshape(1)
            assert Y.bits_equal(torch.cat([m, m * 1.2]).numpy(), c.dmax)                     # Renderer.py:110,145 in float32
            assert c.dmax[1] == f32(float(c.dmax[0]) * float(f32(1.2)))
        c = C.depth_case('last', n)
        assert c.gd[n - 1] == c.dmax[0] and (n == 1 or c.gd[:-1].max() < c.gd[n - 1])
