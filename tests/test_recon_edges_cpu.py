"""The exact cases of tests/recon_edge_cases.py on the host: the yardsticks are right (against the float64 yardsticks of
tests/recon_numpy.py where those are safe), every mesh-depth case is exact in float64 (a numpy restatement of tri_setup and
tri_cover equals the Fraction yardstick bit for bit), and each case decides the rule it is named for: with that one rule
broken the yardstick changes in at least 8 pixels or queries."""
import numpy as np
import pytest

from tests import recon_edge_cases as E
from tests import recon_numpy as Y

DECIDING = 8            # pixels or queries a case must decide for each rule it is named for


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint64)


# ---- the yardsticks against the float64 ones ----------------------------------------------------------------------------------
def test_exact_depth_equals_the_ray_caster_where_no_ray_is_near_an_edge():
    """the seam geometry with the principal point (11/16, -1/2) px aside: no ray within 1e-3 (barycentric) of an edge line, so
    Moeller-Trumbore in float64 decides every pixel as the exact contract does; on these dyadic inputs its numerator and
    determinant are exact too, so its t is the correctly rounded quotient and the float32 images are equal bit for bit"""
    c = E.depth_cases()['seam']
    cam = dict(c['cam'], cx=16.6875, cy=11.5)
    E.assert_budget(c['vertices'], c['faces'], c['w2c'], cam)
    want = E.exact_depth(c['vertices'], c['faces'], c['w2c'], cam)[0]
    cast, margin = Y.ray_cast(c['vertices'], c['faces'], np.eye(4), cam, z_far=E.Z_FAR)
    assert margin.min() > 1e-3 and 0 < (want > 0).sum() < want.size and len(np.unique(want)) > 20
    assert np.array_equal(bits(cast.astype(np.float32)), bits(want))


def test_exact_nearest_equals_brute_force_where_nothing_ties():
    rng = np.random.default_rng(3)
    ref, qry = rng.integers(0, 20000, (600, 3)) / 2.0, rng.integers(0, 20000, (300, 3)) / 2.0
    two = np.sort(((qry[:, None] - ref[None]) ** 2).sum(-1), 1)[:, :2]
    assert (two[:, 0] < two[:, 1]).all()                                    # no query has two nearest references
    d, i = E.exact_nearest(qry, ref)
    yd, yi = Y.nearest(qry, ref)
    assert np.array_equal(i, yi) and np.array_equal(bits(d), bits(yd))
    _, last = E.exact_nearest(qry, ref, last_index=True)
    assert np.array_equal(last, i)                                          # ... so the tie rule does not matter here


# ---- the budget check: tri_setup and tri_cover in float64 numpy -----------------------------------------------------------------
def md_float64(vertices, faces, w2c, cam, z_near, z_far):
    """float32 [K,H,W]: csrc/mesh_depth.hip restated in float64 numpy, expression by expression in the kernel's order:
    tri_setup (camera space, n0 n1 n2, det, the zero-normal and det tests, the depth cull, the pixel box) and tri_cover over
    the box; the unsigned minimum on the float32 bits; 0.0 where nothing was written"""
    V, H, W = len(vertices), cam['H'], cam['W']
    fx, fy, cx, cy = (np.float64(cam[k]) for k in ('fx', 'fy', 'cx', 'cy'))
    img = np.full((len(w2c), H, W), 0xFFFFFFFF, np.uint32)
    cross = lambda a, b: np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]])
    for k, m in enumerate(np.asarray(w2c, np.float64)):
        for face in faces:
            if any(int(v) < 0 or int(v) >= V for v in face):
                continue
            p = [np.array([((m[r, 0] * x + m[r, 1] * y) + m[r, 2] * z) + m[r, 3] for r in range(3)]) for x, y, z in vertices[face]]
            n0, n1, n2 = cross(p[1], p[2]), cross(p[2], p[0]), cross(p[0], p[1])
            det = (p[0][0] * n0[0] + p[0][1] * n0[1]) + p[0][2] * n0[2]
            nrm = n0 + n1 + n2
            if (nrm == 0.0).all() or not det != 0.0 or not det - det == 0.0:
                continue
            depths = [-q[2] for q in p]
            zmin, zmax = min(depths), max(depths)
            if not zmax > z_near or not zmin <= z_far:
                continue
            i0, i1, j0, j1 = 0, W - 1, 0, H - 1
            if zmin > 0.0:
                i0, i1, j0, j1 = E.pixel_box(*p, cam)
                if i0 > i1 or j0 > j1:
                    continue
            i, j = np.arange(i0, i1 + 1, dtype=np.float64)[None, :], np.arange(j0, j1 + 1, dtype=np.float64)[:, None]
            dx, dy = (i - cx) / fx, -(j - cy) / fy
            s0 = (dx * n0[0] + dy * n0[1]) - n0[2]
            s1 = (dx * n1[0] + dy * n1[1]) - n1[2]
            s2 = (dx * n2[0] + dy * n2[1]) - n2[2]
            inside = ((s0 >= 0.0) & (s1 >= 0.0) & (s2 >= 0.0)) | ((s0 <= 0.0) & (s1 <= 0.0) & (s2 <= 0.0))
            S = (s0 + s1) + s2
            with np.errstate(divide='ignore', invalid='ignore'):
                t = det / S
            hit = inside & (S != 0.0) & (t > z_near) & (t <= z_far)
            box = img[k, j0:j1 + 1, i0:i1 + 1]
            box[hit] = np.minimum(box[hit], bits(t.astype(np.float32))[hit])
    img[img == 0xFFFFFFFF] = 0
    return img.view(np.float32)


@pytest.mark.parametrize("name", E.DEPTH_NAMES)
def test_every_depth_case_is_exact_in_float64(name):
    """if this fails the case is not exact (or tri_setup's box cuts a pixel of the contract): the case has to change"""
    c = E.depth_cases()[name]
    got = md_float64(c['vertices'], c['faces'], c['w2c'], c['cam'], c['z_near'], c['z_far'])
    differ = bits(got) != bits(c['want'])
    print(f"{name}: F {len(c['faces'])}, K {len(c['w2c'])}, {c['cam']['H']} x {c['cam']['W']}, hit {int((c['want'] > 0).sum())}, "
          f"differing {int(differ.sum())}")
    assert not differ.any(), np.argwhere(differ)[:8]


# ---- what each case decides -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [n for n in E.DEPTH_NAMES if E.depth_cases()[n]['decides']])
def test_depth_case_decides_its_rules(name, capsys):
    c = E.depth_cases()[name]
    for rule in c['decides']:
        broken = E.exact_depth(c['vertices'], c['faces'], c['w2c'], c['cam'], c['z_near'], c['z_far'], **{rule: True})
        n = int((bits(broken) != bits(c['want'])).sum())
        with capsys.disabled():
            print(f"\n{name}: {rule} changes {n} of {int((c['want'] > 0).sum())} hit pixels", end='')
        assert n >= DECIDING


def test_every_depth_rule_has_a_case():
    assert {r for c in E.depth_cases().values() for r in c['decides']} == set(E.DEPTH_RULES)


def test_turned_views_see_the_same_image():
    c = E.depth_cases()
    for k in (1, 2):
        assert np.array_equal(bits(c[f'seam/view{k}']['want']), bits(c['seam']['want']))
        assert not np.array_equal(c[f'seam/view{k}']['vertices'], c['seam']['vertices'])


def test_limits_sit_on_an_attained_depth():
    """z_far = 4 keeps the 17 x 17 pixels of the front quad at exactly 4.0, one ulp below loses them, one above changes
    nothing; z_near = 4 loses them (the quad behind shows through), one ulp below keeps them"""
    c = E.depth_cases()
    at4 = c['seam']['want'][0] == np.float32(4.0)
    assert at4.sum() >= 200
    assert (c['limits/far_eq']['want'][0][at4] == 4.0).all() and (c['limits/far_above']['want'][0][at4] == 4.0).all()
    assert (c['limits/far_below']['want'][0][at4] == 0.0).all()
    assert (c['limits/near_eq']['want'][0][at4] == 8.0).all() and (c['limits/near_above']['want'][0][at4] == 8.0).all()
    assert (c['limits/near_below']['want'][0][at4] == 4.0).all()
    # the ramp: column 16 is at exactly 4.0 on more than 8 rows, the columns beside it are not
    ramp = c['limits/ramp']['want'][0]
    col = ramp[:, 16] == 4.0
    assert col.sum() >= 8 and (ramp[:, 15] != 4.0).all() and (ramp[:, 17] != 4.0).all()
    assert (c['limits/ramp_far_eq']['want'][0][col, 16] == 4.0).all() and (c['limits/ramp_far_below']['want'][0][col, 16] == 0.0).all()
    assert np.isin(c['limits/ramp_near_eq']['want'][0][col, 16], (0.0, 8.0)).all() and (c['limits/ramp_near_below']['want'][0][col, 16] == 4.0).all()


def test_degenerate_triangles_leave_their_neighbours_alone():
    c = E.depth_cases()['degenerate']
    ordinary = c['faces'][:3]                                                # the front quad and the slanted triangle
    alone = E.exact_depth(c['vertices'], ordinary, c['w2c'], c['cam'])
    assert len(c['faces']) == 10 and np.array_equal(bits(alone), bits(c['want']))


def test_camera_plane_and_off_image_triangles_are_seen():
    """every triangle of these two cases that can be hit decides pixels of the image (all behind / wholly outside: none)"""
    for name, silent in (('camera_plane', {6}), ('off_image', {4})):
        c = E.depth_cases()[name]
        for f in range(len(c['faces'])):
            without = E.exact_depth(c['vertices'], np.delete(c['faces'], f, axis=0), c['w2c'], c['cam'])
            n = int((bits(without) != bits(c['want'])).sum())
            print(f"{name}: face {f} decides {n} pixels")
            assert (n == 0) if f in silent else (n >= DECIDING)


def test_box_split_sizes():
    """tri_setup's box, restated, has 16 x 16 = TRI_SMALL pixels for one triangle (the one-thread route) and 16 x 17 for the
    other (the one-workgroup route)"""
    c = E.depth_cases()
    for name, (bw, bh) in E.BOX_SPLIT.items():
        i0, i1, j0, j1 = E.pixel_box(*c[name]['vertices'][c[name]['faces'][0]], c[name]['cam'])
        print(f"{name}: columns {i0}..{i1}, rows {j0}..{j1}: {(i1 - i0 + 1) * (j1 - j0 + 1)} pixels")
        assert (i1 - i0 + 1, j1 - j0 + 1) == (bw, bh)
    assert 16 * 16 == 256 and 16 * 17 > 256
    both = c['box_split/both']['want']
    assert np.array_equal(bits(both), np.where(c['box_split/256']['want'] > 0, bits(c['box_split/256']['want']), bits(c['box_split/272']['want'])))


def test_many_straddles_blocks_and_lists_large_boxes_in_every_view():
    c = E.depth_cases()['many']
    F, K = len(c['faces']), len(c['w2c'])
    assert F == 257 and K == 3 and F * K > 3 * 256
    for k in range(K):
        p = np.array([[float(x) for x in q] for q in E.camera_space(c['vertices'], c['w2c'][k])])
        assert (-p[:, 2]).min() > 0
        area = []
        for f in (0, F - 1, 1, 128):
            i0, i1, j0, j1 = E.pixel_box(*p[c['faces'][f]], c['cam'])
            area.append((i1 - i0 + 1) * (j1 - j0 + 1))
        assert area[0] > 256 and area[1] > 256 and area[2] <= 256 and area[3] <= 256, area
        assert (c['want'][k] > 0).sum() >= 50
    singles = np.concatenate([E.exact_depth(c['vertices'], c['faces'], c['w2c'][k:k + 1], c['cam']) for k in range(K)])
    assert np.array_equal(bits(singles), bits(c['want']))


# ---- nearest ----------------------------------------------------------------------------------------------------------------
def test_nearest_cases_have_the_named_sizes():
    c = E.nearest_cases()
    sizes = {n: (len(x['ref']), len(x['query'])) for n, x in c.items()}
    print(sizes)
    assert sizes['lattice'] == sizes['offset'] == (131, 879) and sizes['planar'][0] == 2000 and sizes['collinear'][0] == 500
    assert sizes['outlier'][0] == 2001 and sizes['two_points'][0] == 2
    assert np.ptp(c['planar']['ref'], 0)[2] == 0 and (np.ptp(c['collinear']['ref'], 0)[1:] == 0).all()
    for n in (1, 2, 3, 4, 5):
        assert sizes[f'generic_N{n}'][0] == n
    for n in (511, 512, 513, 1025):
        assert sizes[f'N{n}_M257'] == (n, 257)
    for m in (1, 255, 256, 257, 513):
        assert sizes[f'N1000_M{m}'] == (1000, m)


def test_lattice_ties_are_what_the_queries_are_named_for():
    c = E.nearest_cases()['lattice']
    q, r = c['query'], c['ref'][:125]                                        # without the duplicates
    d2 = ((q[:, None] - r[None]) ** 2).sum(-1)
    ways = (d2 == d2.min(1, keepdims=True)).sum(1)
    for group, n in (('cell_centres', 8), ('face_centres', 4), ('edge_midpoints', 2), ('lattice_points', 1), ('one_off', 1)):
        assert (ways[c['groups'][group]] == n).all(), group
    assert (c['dist'][c['groups']['lattice_points']] == 0).all() and (c['dist'][c['groups']['one_off']] == 1.0).all()
    dup = (c['query'][:, None] == c['ref'][None, 125:]).all(-1).any(1)
    assert dup.sum() >= 5 and (c['idx'][dup] < 125).all()                    # a duplicate at a high index never wins


@pytest.mark.parametrize("name", ['lattice', 'offset', 'planar', 'collinear', 'two_points'])
def test_nearest_case_decides_the_tie_rule(name, capsys):
    c = E.nearest_cases()[name]
    _, last = E.exact_nearest(c['query'], c['ref'], last_index=True)
    n = int((last != c['idx']).sum())
    with capsys.disabled():
        print(f"\n{name}: the last index winning changes {n} of {len(c['query'])} queries", end='')
    assert n >= DECIDING


def test_lattice_decides_the_max_dist_rule(capsys):
    c = E.nearest_cases()['lattice']
    d, i = E.apply_max_dist(c['dist'], c['idx'], 1.0)
    d_in, i_in = E.apply_max_dist(c['dist'], c['idx'], 1.0, inclusive=True)
    n = int((i != i_in).sum())
    with capsys.disabled():
        print(f"\nlattice: d <= max_dist at max_dist = 1 changes {n} of {len(i)} queries", end='')
    assert n >= DECIDING and n == (c['dist'] == 1.0).sum() and np.isinf(d[i == -1]).all()
    d_up, i_up = E.apply_max_dist(c['dist'], c['idx'], np.nextafter(1.0, 2.0))
    assert np.array_equal(i_up, c['idx']) and np.array_equal(d_up, c['dist'])
    assert (E.apply_max_dist(c['dist'], c['idx'], 0.0)[1] == -1).all()


def test_exact_nearest_cases_agree_with_brute_force_in_float64():
    """the integer yardstick against numpy's float64 one on every exact case: with (half-)integer coordinates float64 is
    exact too, so both the indices (first minimum) and the distance bits agree"""
    for name in E.NEAREST_EXACT:
        c = E.nearest_cases()[name]
        d, i = Y.nearest(c['query'], c['ref'])
        assert np.array_equal(i, c['idx']) and np.array_equal(bits(d), bits(c['dist'])), name
