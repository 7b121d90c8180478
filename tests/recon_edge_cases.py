"""Exact cases of the reconstruction-evaluation kernels (csrc/mesh_depth.hip, csrc/nearest.hip) at the places where their
contracts are decided, and yardsticks in exact arithmetic (tests/test_recon_edges_cpu.py, tests/test_hip_recon_edges.py).

Mesh depth.  Intrinsics, world-to-camera entries and vertex coordinates are small dyadic rationals, so every float64
intermediate of tri_cover (the edge normals n_i, det, the s_i and S) is exact; only t = det / S (correctly rounded) and
(float)t round.  exact_depth evaluates the contract -- both sides count, edges inclusive, degenerate triangles and triangles
whose plane holds the camera centre hit nothing, z_near < t <= z_far -- in fractions.Fraction and integers and returns
np.float32(float(t)): a ray through a vertex, along an edge or at t == z_far is decided, not excused by a margin.  Every case
asserts its own bit budget (assert_budget).

Nearest.  Coordinates are integers or half-integers: squared distances are exact, sqrt is correctly rounded on both sides,
a tie is a tie.  exact_nearest works in integers; the cases with generic coordinates use recon_numpy.nearest.

Pure numpy and stdlib; every array is read-only and built once (depth_cases(), nearest_cases())."""
import functools
import math
from fractions import Fraction

import numpy as np

from tests import recon_numpy as Y

EXACT_CAM = dict(H=24, W=32, fx=16.0, fy=16.0, cx=16.0, cy=12.0)
Z_FAR = 16.0
IDENTITY = np.array([[[1.0, 0, 0, 0], [0, 1.0, 0, 0], [0, 0, 1.0, 0]]])

# the rules exact_depth can be asked to break, one at a time (tests/test_recon_edges_cpu.py)
DEPTH_RULES = ('edges_strict', 'far_strict', 'near_inclusive', 'admit_degenerate')


def frozen(a, dtype=None):
    a = np.array(a, dtype=dtype)
    a.setflags(write=False)
    return a


# ---- exact mesh depth -------------------------------------------------------------------------------------------------------
def _fr(x):
    return Fraction(float(x))                   # a float is a dyadic rational: exact


def _cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def _sub(a, b):
    return (a[0] - b[0], a[1] - b[1], a[2] - b[2])


def camera_space(vertices, w2c_k):
    """[(x, y, z)] in Fraction: the upper three rows of one world-to-camera matrix applied to every vertex"""
    m = [[_fr(x) for x in row] for row in np.asarray(w2c_k)[:3]]
    return [tuple(m[r][0] * x + m[r][1] * y + m[r][2] * z + m[r][3] for r in range(3))
            for x, y, z in ([_fr(c) for c in v] for v in np.asarray(vertices))]


def _pixel_directions(cam):
    """(dx [W], dy [H]) in Fraction: the ray of pixel (row j, column i) is (dx[i], dy[j], -1)"""
    fx, fy, cx, cy = (_fr(cam[k]) for k in ('fx', 'fy', 'cx', 'cy'))
    return [(Fraction(i) - cx) / fx for i in range(cam['W'])], [-(Fraction(j) - cy) / fy for j in range(cam['H'])]


def _ray_segment(d, a, b):
    """the smallest t with t d on the closed segment a b (a point when a == b), None when the line of d misses it; when d
    runs along the segment, the parameter of its nearer end"""
    e = _sub(b, a)
    dd = _dot(d, d)
    if e == (0, 0, 0) or _cross(d, e) == (0, 0, 0):
        if _cross(d, a) != (0, 0, 0):
            return None
        return min(_dot(a, d) / dd, _dot(b, d) / dd)
    n = _cross(d, e)
    if _dot(a, n) != 0:
        return None
    nn = _dot(n, n)
    t, u = _dot(_cross(a, e), n) / nn, _dot(_cross(a, d), n) / nn
    return t if 0 <= u <= 1 else None


def exact_depth(vertices, faces, w2c, cam, z_near=0.0, z_far=Z_FAR, edges_strict=False, far_strict=False,
                near_inclusive=False, admit_degenerate=False):
    """float32 [K,H,W]: the contract of enslam_mesh_depth in exact arithmetic.  Per view and triangle, with a, b, c the
    camera-space vertices: n0 = b x c, n1 = c x a, n2 = a x b, det = a . n0 in Fraction; per pixel the signs of s_i = d . n_i
    in integers (the s_i over one positive common denominator); a hit has s0, s1, s2 of one sign (zeros count) and
    t = det / (s0 + s1 + s2) with z_near < t <= z_far; the smallest t, rounded to float64 and then to float32 as the kernel
    rounds it.  A triangle with a zero normal or with det == 0, or with an index outside [0, V), hits nothing.

    The keyword switches break one rule each, for the tests that show what a case decides: edges_strict (zeros do not
    count), far_strict (t < z_far), near_inclusive (t >= z_near), admit_degenerate (a triangle with a zero normal or
    det == 0 is hit where the ray meets the closed set its vertices span: a point, a segment, an edge-on triangle)."""
    V = len(vertices)
    H, W = cam['H'], cam['W']
    dxs, dys = _pixel_directions(cam)
    L = math.lcm(*(q.denominator for q in dxs + dys))
    DX = np.array([int(q * L) for q in dxs], dtype=object)[None, :]
    DY = np.array([int(q * L) for q in dys], dtype=object)[:, None]
    zn, zf = _fr(z_near), _fr(z_far)

    def in_range(t):
        return (t >= zn if near_inclusive else t > zn) and (t < zf if far_strict else t <= zf)

    out = np.zeros((len(w2c), H, W), np.float32)
    for k, m in enumerate(w2c):
        p = camera_space(vertices, m)
        best = {}
        for face in np.asarray(faces):
            if any(int(v) < 0 or int(v) >= V for v in face):
                continue
            a, b, c = (p[int(v)] for v in face)
            n = (_cross(b, c), _cross(c, a), _cross(a, b))
            det = _dot(a, n[0])
            if _cross(_sub(b, a), _sub(c, a)) == (0, 0, 0) or det == 0:
                if admit_degenerate:
                    for j in range(H):
                        for i in range(W):
                            d = (dxs[i], dys[j], Fraction(-1))
                            ts = [t for t in (_ray_segment(d, *e) for e in ((a, b), (b, c), (c, a))) if t is not None and in_range(t)]
                            if ts and ((j, i) not in best or min(ts) < best[j, i]):
                                best[j, i] = min(ts)
                continue
            D = math.lcm(*(x.denominator for ni in n for x in ni))
            s = [DX * int(ni[0] * D) + DY * int(ni[1] * D) - L * int(ni[2] * D) for ni in n]      # s_i * (L * D), Python ints
            if edges_strict:
                inside = ((s[0] > 0) & (s[1] > 0) & (s[2] > 0)) | ((s[0] < 0) & (s[1] < 0) & (s[2] < 0))
            else:
                inside = ((s[0] >= 0) & (s[1] >= 0) & (s[2] >= 0)) | ((s[0] <= 0) & (s[1] <= 0) & (s[2] <= 0))
            S = s[0] + s[1] + s[2]
            for j, i in zip(*np.nonzero(inside.astype(bool) & (S != 0).astype(bool))):
                t = det * (L * D) / int(S[j, i])
                if in_range(t) and ((j, i) not in best or t < best[j, i]):
                    best[j, i] = t
        for (j, i), t in best.items():
            out[k, j, i] = np.float32(float(t))
    return out


def assert_budget(vertices, faces, w2c, cam):
    """the bit budget of a case: per camera axis the coordinates are multiples of 2^-k_a and below 2^b_a in magnitude, the
    ray components multiples of 2^-g and below 2^1.  det, the n_i, the s_i and S are then sums of at most 18 products of one
    coordinate per axis (or a ray component in place of one), multiples of 2^-(kx+ky+kz+g) below 2^(bx+by+bz+1+5):
    exact in float64 while the exponents sum to at most 53.  Also: the camera-space coordinates themselves are exact."""
    dxs, dys = _pixel_directions(cam)
    g = max(q.denominator for q in dxs + dys).bit_length() - 1
    assert all(q.denominator & (q.denominator - 1) == 0 and abs(q) < 2 for q in dxs + dys)
    used = sorted({int(v) for f in np.asarray(faces) for v in f if all(0 <= int(u) < len(vertices) for u in f)})
    for m in w2c:
        p = camera_space(vertices, m)
        m = np.asarray(m, np.float64)
        for v in used:
            x, y, z = (float(c) for c in vertices[v])
            got = [((m[r, 0] * x + m[r, 1] * y) + m[r, 2] * z) + m[r, 3] for r in range(3)]          # tri_face's expression
            assert all(Fraction(got[r]) == p[v][r] for r in range(3)), "camera-space coordinates are not exact"
        bits = 0
        for axis in range(3):
            col = [p[v][axis] for v in used]
            assert all(q.denominator & (q.denominator - 1) == 0 for q in col), "a coordinate is no dyadic rational"
            k = max(q.denominator for q in col).bit_length() - 1
            b = max(1, max(abs(q.numerator) // q.denominator + 1 for q in col)).bit_length()
            bits += k + b
        assert bits + g + 1 + 5 <= 53, f"triple products need {bits + g + 6} bits"


def pixel_box(a, b, c, cam):
    """(i0, i1, j0, j1): tri_setup's inclusive pixel box of a camera-space triangle in front of the camera, restated: the
    projected vertices, 1e-3 px of slack, floor / ceil, the clamp into the image"""
    p = np.array([a, b, c], np.float64)
    assert (-p[:, 2]).min() > 0
    u = cam['cx'] + cam['fx'] * (p[:, 0] / -p[:, 2])
    w = cam['cy'] - cam['fy'] * (p[:, 1] / -p[:, 2])
    clamp = lambda x, n: int(min(max(x, -1.0), float(n)))
    i0, i1 = clamp(np.floor(u.min() - 1e-3), cam['W']), clamp(np.ceil(u.max() + 1e-3), cam['W'])
    j0, j1 = clamp(np.floor(w.min() - 1e-3), cam['H']), clamp(np.ceil(w.max() + 1e-3), cam['H'])
    return max(i0, 0), min(i1, cam['W'] - 1), max(j0, 0), min(j1, cam['H'] - 1)


# ---- mesh depth cases -------------------------------------------------------------------------------------------------------
def P(i, j, depth, cam=EXACT_CAM):
    """the camera-space point at `depth` on the ray through the centre of pixel (row j, column i)"""
    return ((i - cam['cx']) / cam['fx'] * depth, -(j - cam['cy']) / cam['fy'] * depth, -float(depth))


def _mesh(*parts):
    """(vertices, faces) of triangles / quads given as vertex tuples; a quad (a, b, c, d) is split along a-c"""
    v, f = [], []
    for part in parts:
        n = len(v)
        v += [tuple(float(x) for x in q) for q in part]
        f += [(n, n + 1, n + 2)] + ([(n, n + 2, n + 3)] if len(part) == 4 else [])
    return np.array(v, np.float64), np.array(f, np.int32)


# a 4 x 4 quad at depth 4 whose border and diagonal run through pixel centres, a quad behind it (depth 8, its border through
# pixel centres too) seen only past the first one's border, and a slanted triangle in front with depths that are no dyadic numbers
FRONT_QUAD = (P(8, 4, 4), P(24, 4, 4), P(24, 20, 4), P(8, 20, 4))
BACK_QUAD = (P(4, 2, 8), P(28, 2, 8), P(28, 22, 8), P(4, 22, 8))
SLANTED = ((-1.0, 0.5, -2.0), (0.25, 0.75, -3.0), (-0.5, -0.75, -2.5))

# signed axis permutations (proper rotations) with integer translations: the object sits around the world origin
VIEWS3 = np.array([[[1.0, 0, 0, 0], [0, 1.0, 0, 0], [0, 0, 1.0, -6.0]],
                   [[0, 1.0, 0, 0], [0, 0, 1.0, 1.0], [1.0, 0, 0, -5.0]],
                   [[0, 0, -1.0, 1.0], [1.0, 0, 0, 0], [0, -1.0, 0, -7.0]]])


def _many():
    """257 triangles (F * K = 771 straddles three 256-thread blocks): 255 small ones with vertices on the 1/16 lattice in
    [-2.5, 2.5]^3 and two large ones (the first and the last face) whose boxes exceed 256 pixels in every view"""
    rng = np.random.default_rng(257)
    centre = rng.integers(-32, 33, (255, 1, 3)) / 16.0
    small = centre + rng.integers(-8, 9, (255, 3, 3)) / 16.0
    big0 = np.array([[-4.0, -4.0, -1.0], [4.0, -3.0, 0.5], [-1.0, 4.0, 1.0]])
    big1 = np.array([[4.0, 4.0, -0.5], [-4.0, 2.0, 1.5], [2.0, -4.0, -1.5]])
    tris = np.concatenate([big0[None], small, big1[None]])
    return tris.reshape(-1, 3), np.arange(3 * 257, dtype=np.int32).reshape(-1, 3)


def _case(name, mesh, cam=EXACT_CAM, w2c=IDENTITY, z_near=0.0, z_far=Z_FAR, decides=()):
    v, f = mesh
    assert_budget(v, f, w2c, cam)
    return dict(name=name, vertices=frozen(v, np.float64), faces=frozen(f, np.int32), w2c=frozen(w2c, np.float64), cam=dict(cam),
                z_near=float(z_near), z_far=float(z_far), decides=tuple(decides))


def _depth_case_list():
    seam = _mesh(FRONT_QUAD, BACK_QUAD, SLANTED)
    cases = [_case('seam', seam, decides=('edges_strict',))]
    # the same camera-space geometry reached through a turned and shifted view: world = R^T (camera - t)
    for k in (1, 2):
        R, t = VIEWS3[k, :, :3], VIEWS3[k, :, 3]
        cases.append(_case(f'seam/view{k}', ((seam[0] - t) @ R, seam[1]), w2c=VIEWS3[k:k + 1], decides=('edges_strict',)))
    # one triangle: two vertices and the whole edge between them on the pixel centres of row 6, the third vertex on a centre too
    cases.append(_case('vertex_and_edge', _mesh((P(10, 6, 2), P(26, 6, 4), P(14, 20, 2))), decides=('edges_strict',)))
    # the front quad is at t = 4 exactly on 17 x 17 pixels
    up, down = float(np.nextafter(4.0, 5.0)), float(np.nextafter(4.0, 3.0))
    cases += [_case('limits/far_eq', seam, z_far=4.0, decides=('far_strict',)),
              _case('limits/far_below', seam, z_far=down),
              _case('limits/far_above', seam, z_far=up),
              _case('limits/near_eq', seam, z_near=4.0, decides=('near_inclusive',)),
              _case('limits/near_below', seam, z_near=down),
              _case('limits/near_above', seam, z_near=up)]
    # a triangle in the plane depth = 4 + x: t = 4 exactly down column 16 while its vertices are at depths 2, 6 and 4, so the
    # limits are decided per pixel (tri_cover), not by the cull on the triangle's depth range (tri_setup)
    ramp = _mesh(((-2.0, -2.0, -2.0), (2.0, -2.0, -6.0), (0.0, 3.0, -4.0)), BACK_QUAD)
    cases += [_case('limits/ramp', ramp),
              _case('limits/ramp_far_eq', ramp, z_far=4.0, decides=('far_strict',)),
              _case('limits/ramp_far_below', ramp, z_far=down),
              _case('limits/ramp_near_eq', ramp, z_near=4.0, decides=('near_inclusive',)),
              _case('limits/ramp_near_below', ramp, z_near=down)]
    # degenerate triangles at depth 2 - 3 in front of the ordinary ones, each through the centres of a row of pixels
    v, f = _mesh(FRONT_QUAD, SLANTED,
                 (P(10, 8, 2), P(10, 8, 2), P(20, 8, 2)),                   # a repeated vertex
                 (P(10, 10, 2), P(14, 10, 2), P(22, 10, 2)),                # three distinct collinear vertices
                 ((-1.0, 0.0, -2.0), (1.0, 0.0, -2.0), (0.0, 0.0, -3.0)),   # the plane y = 0 holds the camera centre: row 12
                 (P(12, 14, 2), P(12, 14, 2), P(12, 14, 2)))                # a point
    V = len(v)
    f = np.concatenate([f, [[0, 1, V], [-1, 2, 3], [0, 2 ** 31 - 1, 1]]]).astype(np.int32)
    cases.append(_case('degenerate', (v, f), decides=('admit_degenerate',)))
    # the homogeneous, whole-image-box path: vertices on and behind the camera plane
    cases.append(_case('camera_plane', _mesh(FRONT_QUAD,
                                             ((3.0, 2.0, 0.0), (-3.0, -1.0, -4.0), (1.0, -2.0, -6.0)),      # one vertex at z = 0
                                             ((-2.0, -3.0, 0.0), (2.0, -3.0, 0.0), (0.0, -1.0, -4.0)),      # two at z = 0
                                             ((0.0, 3.0, 2.0), (-2.0, -2.0, -3.0), (2.0, -1.0, -5.0)),      # one behind
                                             ((-3.0, -2.0, 1.0), (-3.0, 3.0, 1.0), (0.5, -0.5, -2.0)),     # two behind
                                             ((0.0, 0.0, 1.0), (1.0, 0.0, 2.0), (0.0, 1.0, 3.0)))))         # all behind
    t256 = (P(2, 3, 4), P(15, 3, 4), P(2, 16, 4))
    t272 = (P(17, 3, 4), P(30, 3, 4), P(17, 17, 4))
    cases += [_case('box_split/256', _mesh(t256)), _case('box_split/272', _mesh(t272)), _case('box_split/both', _mesh(t256, t272))]
    cases.append(_case('off_image', _mesh(((-12.0, -1.0, -4.0), (-3.0, -2.0, -4.0), (-3.0, 1.0, -4.0)),        # past the left border
                                          ((12.0, 1.0, -5.0), (3.0, 2.0, -5.0), (3.0, -1.0, -5.0)),            # right
                                          ((0.0, 9.0, -4.0), (-1.0, 2.0, -4.0), (1.0, 2.0, -4.0)),             # top
                                          ((0.0, -9.0, -6.0), (-1.0, -2.0, -6.0), (1.0, -2.0, -6.0)),          # bottom
                                          ((20.0, 0.0, -4.0), (24.0, 0.0, -4.0), (22.0, 2.0, -4.0)),           # wholly outside
                                          ((1.0, 1.0, -2.0 ** -20), (-1.0, -1.0, -4.0), (1.0, -1.5, -4.0)))))  # a huge projection
    cases.append(_case('many', _many(), w2c=VIEWS3))
    shape = _mesh(FRONT_QUAD, SLANTED)
    for h, w, variants in ((1, 1, dict(hit=(0.0, 0.0), miss=(16.0, 0.0), edge=(8.0, 0.0))),
                           (1, 32, dict(hit=(16.0, 0.0), miss=(16.0, 12.0), edge=(16.0, 8.0))),
                           (24, 1, dict(hit=(0.0, 12.0), miss=(16.0, 12.0), edge=(-8.0, 12.0)))):
        for what, (cx, cy) in variants.items():
            cases.append(_case(f'shape/{h}x{w}/{what}', shape, cam=dict(H=h, W=w, fx=16.0, fy=16.0, cx=cx, cy=cy)))
    return cases


BOX_SPLIT = {'box_split/256': (16, 16), 'box_split/272': (16, 17)}      # (width, height) of tri_setup's box


@functools.lru_cache(maxsize=None)
def depth_cases():
    """name -> case: vertices, faces, w2c [K,3,4], cam, z_near, z_far, decides (the rules the case is named for) and `want`,
    the float32 [K,H,W] image of exact_depth"""
    out = {}
    for c in _depth_case_list():
        c['want'] = frozen(exact_depth(c['vertices'], c['faces'], c['w2c'], c['cam'], c['z_near'], c['z_far']))
        out[c['name']] = c
    assert tuple(out) == DEPTH_NAMES
    for name, (bw, bh) in BOX_SPLIT.items():
        c = out[name]
        i0, i1, j0, j1 = pixel_box(*c['vertices'][c['faces'][0]], c['cam'])
        assert (i1 - i0 + 1, j1 - j0 + 1) == (bw, bh), (name, i0, i1, j0, j1)
    return out


DEPTH_NAMES = ('seam', 'seam/view1', 'seam/view2', 'vertex_and_edge', 'limits/far_eq', 'limits/far_below', 'limits/far_above', 'limits/near_eq',
               'limits/near_below', 'limits/near_above', 'limits/ramp', 'limits/ramp_far_eq', 'limits/ramp_far_below',
               'limits/ramp_near_eq', 'limits/ramp_near_below', 'degenerate', 'camera_plane', 'box_split/256', 'box_split/272',
               'box_split/both', 'off_image', 'many') + tuple(f'shape/{s}/{w}' for s in ('1x1', '1x32', '24x1')
                                                               for w in ('hit', 'miss', 'edge'))


# ---- exact nearest neighbour ------------------------------------------------------------------------------------------------
def _half_integers(a):
    a2 = np.asarray(a, np.float64) * 2.0
    i2 = np.rint(a2).astype(np.int64)
    assert np.array_equal(i2.astype(np.float64), a2) and np.abs(i2).max(initial=0) < 2 ** 30, "coordinates must be (half-)integers"
    return i2


def exact_nearest(query, ref, last_index=False, block=256):
    """(dist float64 [M], idx int64 [M]) of integer or half-integer points, in integers: the smallest index among the
    references at the exact smallest squared distance, dist = sqrt of that in float64 (the squared distance is a multiple
    of 1/4 below 2^48: exact in float64, and far from the 1e-15 relative window in which nn_consider compares square
    roots).  last_index breaks the tie rule: the largest index wins."""
    q, r = _half_integers(query), _half_integers(ref)
    dist, idx = np.empty(len(q)), np.empty(len(q), np.int64)
    for lo in range(0, len(q), block):
        d2 = ((q[lo:lo + block, None, :] - r[None, :, :]) ** 2).sum(-1)               # 4 * squared distance, int64
        assert d2.max() < 2 ** 50
        pick = d2.shape[1] - 1 - d2[:, ::-1].argmin(1) if last_index else d2.argmin(1)
        idx[lo:lo + block] = pick
        dist[lo:lo + block] = np.sqrt(d2[np.arange(d2.shape[0]), pick].astype(np.float64) / 4.0)
    return dist, idx


def apply_max_dist(dist, idx, max_dist, inclusive=False):
    """the max_dist rule on a yardstick result: idx -1 and dist inf unless d < max_dist (inclusive breaks it: d <= max_dist)"""
    ok = dist <= max_dist if inclusive else dist < max_dist
    return np.where(ok, dist, np.inf), np.where(ok, idx, -1)


def _lattice():
    rng = np.random.default_rng(125)
    g = np.arange(5.0)
    pts = np.stack(np.meshgrid(g, g, g, indexing='ij'), -1).reshape(-1, 3)
    ref = pts[rng.permutation(125)]
    ref = np.concatenate([ref, ref[[3, 50, 50, 124, 0, 77]]])                          # duplicates at high indices
    h = np.arange(4.0) + 0.5
    grid = lambda *ax: np.stack(np.meshgrid(*ax, indexing='ij'), -1).reshape(-1, 3)
    groups = {'cell_centres': grid(h, h, h),                                                                   # 8-way ties
              'face_centres': np.concatenate([grid(g, h, h), grid(h, g, h), grid(h, h, g)]),                   # 4-way
              'edge_midpoints': np.concatenate([grid(h, g, g), grid(g, h, g), grid(g, g, h)]),                 # 2-way
              'lattice_points': pts,                                                                           # d = 0
              # one step off each face of the lattice: the nearest point is at distance 1 exactly, and alone
              'one_off': np.concatenate([np.insert(pts[pts[:, 0] == 0][:, 1:], a, v, axis=1) for a in range(3) for v in (-1.0, 5.0)])}
    assert [len(x) for x in groups.values()] == [64, 240, 300, 125, 150]
    return ref, groups


def _planar():
    rng = np.random.default_rng(2000)
    ref = np.concatenate([rng.integers(0, 100, (2000, 2)) / 2.0, np.full((2000, 1), 3.0)], axis=1)            # the plane z = 3
    ends = np.array([[-30.0, 25.0, 3.0], [80.0, 25.0, 3.0], [25.0, -30.0, 3.0], [25.0, 80.0, 3.0], [-30.0, -30.0, 3.0], [80.0, 80.0, 3.0]])
    return ref, {'in_set': ref[:200], 'near': ref[200:400] + rng.integers(-2, 3, (200, 3)) / 2.0,
                 'far': ref[400:500] + np.array([0.0, 0.0, 1000.0]) * rng.choice([-1.0, 1.0], (100, 1)),
                 'beyond': np.concatenate([ends, ends + np.array([0.0, 0.0, 0.5])])}


def _collinear():
    rng = np.random.default_rng(500)
    ref = np.concatenate([rng.integers(0, 800, (500, 1)) / 2.0, np.full((500, 1), -2.0), np.full((500, 1), 7.5)], axis=1)
    ends = np.array([[-0.5, -2.0, 7.5], [-300.0, -2.0, 7.5], [400.0, -2.0, 7.5], [900.0, -2.0, 7.5], [-1.0, 3.0, 7.5], [401.0, -2.0, 2.5]])
    return ref, {'in_set': ref[:100], 'near': ref[100:250] + rng.integers(-2, 3, (150, 3)) / 2.0,
                 'far': ref[250:300] + np.array([0.0, 500.0, -500.0]), 'beyond': ends}


def _two_points():
    ref = np.array([[0.0, 0.0, 0.0], [8.0, 6.0, 4.0]])
    bisector = np.array([[4.0, 3.0, 2.0], [5.0, 3.0, 0.0], [2.0, 5.0, 3.0], [7.0, 1.0, -1.0], [1.0, 1.0, 11.0], [-2.0, 9.0, 5.0],
                         [10.0, -3.0, -1.0], [4.5, 2.0, 2.5]])
    assert np.array_equal(bisector @ ref[1], np.full(8, 58.0))
    return ref, {'bisector': bisector, 'sides': np.concatenate([bisector - 0.5, bisector + 0.5, ref, ref + 20.0, ref - 20.0])}


def _outlier():
    rng = np.random.default_rng(2001)
    ref = np.concatenate([rng.integers(0, 40, (2000, 3)) / 2.0, [[1e6, 1e6, 1e6]]])
    mid = np.array([[500000.0, 500000.0, 500000.0], [500010.0, 500010.0, 500010.0], [499990.0, 500000.0, 500010.0]])
    return ref, {'cluster': rng.integers(-4, 44, (200, 3)) / 2.0, 'at_outlier': 1e6 + rng.integers(-20, 21, (50, 3)) / 2.0,
                 'halfway': np.concatenate([mid, 500000.0 + rng.integers(-100, 101, (47, 3))])}


def _outside():
    rng = np.random.default_rng(1000)
    ref = rng.normal(size=(1000, 3))
    lo, hi = ref.min(0), ref.max(0)
    size = hi - lo
    groups = {}
    for what, boxes in (('half', 0.5), ('boxes30', 30.0)):
        q = []
        for a in range(3):
            for side in (-1.0, 1.0):
                p = rng.uniform(lo, hi, (20, 3))
                p[:, a] = (hi[a] if side > 0 else lo[a]) + side * boxes * size[a]
                q.append(p)
        q.append(hi + boxes * size * rng.uniform(0.9, 1.1, (20, 3)))                    # beyond a corner
        groups[what] = np.concatenate(q)
    return ref, groups


def _generic(n, m, seed):
    rng = np.random.default_rng(seed)
    return rng.normal(size=(n, 3)), {'all': rng.normal(size=(m, 3)) * 1.5}


NEAREST_EXACT = ('lattice', 'planar', 'collinear', 'two_points', 'outlier', 'offset')
NEAREST_NAMES = NEAREST_EXACT + ('outside',) + tuple(f'generic_N{n}' for n in (1, 2, 3, 4, 5)) \
    + tuple(f'N{n}_M257' for n in (511, 512, 513, 1025)) + tuple(f'N1000_M{m}' for m in (1, 255, 256, 257, 513))


@functools.lru_cache(maxsize=None)
def nearest_cases():
    """name -> case: ref [N,3], query [M,3], groups (name -> slice of the queries), exact (bool: the yardstick is
    exact_nearest and the bar bit equality; otherwise recon_numpy.nearest and the bars of test_nearest_matches_brute_force),
    dist float64 [M], idx int64 [M]"""
    made = {'lattice': _lattice(), 'planar': _planar(), 'collinear': _collinear(), 'two_points': _two_points(),
            'outlier': _outlier(), 'outside': _outside()}
    ref, groups = made['lattice']
    made['offset'] = (ref + 2.0 ** 20, {k: q + 2.0 ** 20 for k, q in groups.items()})
    for n in (1, 2, 3, 4, 5):
        made[f'generic_N{n}'] = _generic(n, 64, 10 + n)
    for n in (511, 512, 513, 1025):
        made[f'N{n}_M257'] = _generic(n, 257, n)
    for m in (1, 255, 256, 257, 513):
        made[f'N1000_M{m}'] = _generic(1000, m, 7000 + m)
    out = {}
    for name in NEAREST_NAMES:
        ref, groups = made[name]
        query, slices, at = np.concatenate(list(groups.values())), {}, 0
        for k, q in groups.items():
            slices[k] = slice(at, at + len(q))
            at += len(q)
        exact = name in NEAREST_EXACT
        assert len(ref) <= 2001 and len(query) <= 1025
        dist, idx = exact_nearest(query, ref) if exact else Y.nearest(query, ref)
        out[name] = dict(name=name, ref=frozen(ref, np.float64), query=frozen(query, np.float64), groups=slices, exact=exact,
                         dist=frozen(dist), idx=frozen(idx))
    return out
