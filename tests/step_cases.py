"""Inputs of the per-iteration kernel tests (tests/test_step_cpu.py, tests/test_hip_step_kernels.py): seeded, small, at the
sizes where a launch shape or a stride changes.  Every case is built once per process together with its yardstick outputs
(tests/step_numpy.py) and handed out read-only."""
import functools
import types

import numpy as np

from tests import step_numpy as Y

f32 = np.float32

# 64 / 256 / 1024 threads in pose_rays_bwd_kernel, the 256-thread blocks of the element-wise kernels and the 1024-thread
# strides of the one-workgroup reductions: one below, at and one above each, and a size with a partial third stride
N_EDGES = (1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2500)

CAM = (600.0, 600.0, 599.5, 339.5)                      # fx, fy, cx, cy of a 1200 x 680 image
CAMERA_TENSORS = {                                      # quaternion (real first), translation
    'norm2_0.9': (0.7, -0.2, 0.6, 0.1, 3.0, 1.0, -0.5),             # the camera tensor of tests/test_hip_tracker.py
    'norm_2.7': (1.9, -1.1, 1.3, 0.8, -0.731, 2.417, 0.0913),
    'norm_0.06': (0.031, 0.042, -0.025, 0.017, 1.2345, -0.6789, 2.7183),
    'identity': (1.0, 0.0, 0.0, 0.0, 0.3137, -1.6181, 0.5772),
    'half_turn': (0.0, 0.0, 1.0, 0.0, -2.0943, 0.4343, 1.4142),
}
COTANGENTS = ('both', 'ro', 'rd')
CANCEL_CAP = 1e3                                        # A / |value| of every reduced sum of a pose case


def _frozen(**kw):
    for v in kw.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return types.SimpleNamespace(**kw)


def _rng(tag, *ints):
    """a generator seeded by a fixed number per tag (no use of hash(): the same stream in every process)"""
    return np.random.default_rng([sum(ord(c) * (i + 1) for i, c in enumerate(tag))] + [int(i) for i in ints])


# ---- camera tensor -> rays and back -----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def pose_pixels(n):
    """pixels (column, row) of a 1200 x 680 image and ray cotangents that follow the directions (an affine function of them
    plus noise, as the gradient of a smooth loss does), so that no reduced sum is a near-cancellation"""
    r = _rng('pose', n)
    pi, pj = np.floor(r.random(n) * 1199).astype(f32), np.floor(r.random(n) * 679).astype(f32)
    d0, d1 = Y.directions32(pi, pj, *CAM)
    d = np.stack([d0, d1, -np.ones(n, f32)], -1).astype(np.float64)
    C = np.array([[1.3, -0.8, 0.6], [-0.7, 1.1, -0.9], [0.9, 0.5, 1.2]])
    g_rd = (d @ C.T + 0.4 * r.normal(size=(n, 3))).astype(f32)
    g_ro = (np.array([0.7, -0.4, 0.9]) + 0.5 * r.normal(size=(n, 3))).astype(f32)
    return _frozen(n=n, pi=pi, pj=pj, g_ro=g_ro, g_rd=g_rd)


def cotangents(px, which):
    return (px.g_ro if which in ('both', 'ro') else None), (px.g_rd if which in ('both', 'rd') else None)


@functools.lru_cache(maxsize=None)
def pose_case(name, n):
    """rays of CAMERA_TENSORS[name] through pose_pixels(n): float32 mirror, float64 version and, per cotangent choice, the
    gradient to the camera tensor with its A"""
    px = pose_pixels(n)
    ct = np.array(CAMERA_TENSORS[name], f32)
    ro, rd = Y.pose_rays(ct, px.pi, px.pj, *CAM)
    _, rd64, scale = Y.pose_rays64(ct, px.pi, px.pj, *CAM)
    grad = {}
    for which in COTANGENTS:
        g, A = Y.pose_rays_grad(ct, px.pi, px.pj, *CAM, *cotangents(px, which))
        g.setflags(write=False), A.setflags(write=False)
        grad[which] = (g, A)
    return _frozen(ct=ct, px=px, ro=ro, rd=rd, rd64=rd64, scale=scale, grad=grad)


# ---- losses -----------------------------------------------------------------------------------------------------------------
LOSS_N = (0,) + N_EDGES + (4097,)
LOSS_KINDS = ('random', 'holes', 'all_zero', 'all_zero_no_color', 'depth_equal', 'color_equal', 'unc_zero', 'tail', 'no_color')
W_MAPPER, W_TRACKER, G_UP = 0.2, 0.5, 1.7               # colour weights (Mapper / Tracker defaults) and the upstream gradient


@functools.lru_cache(maxsize=None)
def loss_case(kind, n):
    """one batch of n rays and the yardstick values of both losses on it (`map` = rgbd_loss, `trk` = tracker_loss)"""
    r = _rng('loss' + kind, n)
    gd = (0.1 + 2.9 * r.random(n)).astype(f32)
    depth = gd.astype(np.float64) + r.normal(size=n) * 0.3
    unc = r.random(n) * 0.1 + 1e-4
    gc = r.random((n, 3)).astype(f32)
    color = r.random((n, 3)).astype(f32)
    k = np.arange(n)
    if kind in ('holes', 'no_color'):
        gd[k % 7 == 3] = 0.0                                    # about 1/7 holes ...
        gd[k % 97 == 5] = -0.25                                 # ... and a few negatives (a loader's "invalid" mark)
    if kind in ('all_zero', 'all_zero_no_color'):
        gd[:] = 0.0
    if kind == 'depth_equal':
        depth[k % 3 == 1] = gd[k % 3 == 1].astype(np.float64)
    if kind == 'color_equal':
        same = r.random((n, 3)) < 0.3
        color[same] = gc[same]
    if kind == 'unc_zero':
        unc[k % 4 == 2] = 0.0
    if kind == 'tail':                                          # every term zero but the one of the last ray
        depth, color = gd.astype(np.float64), gc.copy()
        if n:
            depth[n - 1] = float(gd[n - 1]) + 1000.0
    if kind in ('no_color', 'all_zero_no_color'):
        color = None
    out = dict(kind=kind, n=n, depth=depth, unc=unc, color=color, gd=gd, gc=gc)
    for key, val in (('map', Y.rgbd_loss(depth, color, gd, gc, W_MAPPER, G_UP)),
                     ('trk', Y.tracker_loss(depth, unc, color, gd, gc, W_TRACKER, G_UP))):
        for a in val[2:]:
            if a is not None:
                a.setflags(write=False)
        out[key] = val
    return _frozen(**out)


def loss_cases():
    return [(kind, n) for n in LOSS_N for kind in (LOSS_KINDS if n else ('random', 'no_color'))]


# ---- Adam over tensor lists -------------------------------------------------------------------------------------------------
ADAM_STEPS = 12
ADAM_LRS = tuple((0.0, 0.005, 0.1, 0.001)[k % 4] for k in range(ADAM_STEPS))
ADAM_LISTS = {
    'six': (1, 7, 1023, 1024, 1025, 2049),
    'seventy_two': tuple((1, 5, 1024, 1025, 3, 2048, 33)[k % 7] for k in range(72)),      # every block -> tensor boundary
    'single_7': (7,), 'single_1024': (1024,),                   # one workgroup: the launch counts the step itself
    'single_1025': (1025,),                                     # two workgroups: the host counts it
}
ZERO_SLICE = slice(1, 4)        # exact-zero gradients of the second tensor (the first of a single one) in steps 1 and 2
# The measured distance of float32 torch.optim.Adam (CPU) from the float64 yardstick over ADAM_LISTS and the masked grids
# below, in units of (2^-24 max|p| + sum of the learning rates so far), is 3.301e-05: half an ulp of a parameter near 2 after
# the first step that moves it, when the learning rates so far add up to 0.005 (tests/test_step_cpu.py measures it again and
# brackets this constant: measured <= ADAM_TOL <= 8 measured).  The kernels' m*b1 + (1-b1)*g against torch's lerp differs by a
# few roundings per step: 4 x covers that; a bias correction one step off or a stale moment moves a parameter by several
# per cent of the learning rate, hundreds of times this.
ADAM_TOL = 1.32e-04


def adam_scale(p_ref, lrs_so_far):
    return 2.0 ** -24 * float(np.abs(p_ref).max()) + float(np.sum(lrs_so_far))


def zero_tensor(numels):
    return 1 if len(numels) > 1 else 0


@functools.lru_cache(maxsize=None)
def adam_list(name):
    """parameters, ADAM_STEPS gradients per tensor (|g| from 1e-6 to 1e2 element by element) and the float64 trajectory"""
    numels = ADAM_LISTS[name]
    r = _rng('adam' + name)
    p0 = [r.normal(size=k).astype(f32) for k in numels]
    grads = [(r.normal(size=(ADAM_STEPS, k)) * 10.0 ** r.uniform(-6, 2, size=(ADAM_STEPS, k))).astype(f32) for k in numels]
    z = zero_tensor(numels)
    if numels[z] >= ZERO_SLICE.stop:
        grads[z][:2, ZERO_SLICE] = 0.0
    ref = [Y.adam(p, g, ADAM_LRS) for p, g in zip(p0, grads)]
    for a in p0 + grads + [x for t in ref for x in t]:
        a.setflags(write=False)
    return _frozen(name=name, numels=numels, p0=p0, grads=grads, ref=ref)


# ---- masked Adam on voxel-major grids ---------------------------------------------------------------------------------------
GRID_V = (1, 63, 64, 65, 60, 693)
GRID_MASKS = ('none', 'zeros', 'ones', 'pattern')
GRID_STEPS = 4
GRID_LRS = ADAM_LRS[:GRID_STEPS]
FOUR_V = (65, 1, 693, 64)
FOUR_MASKS = ('pattern', 'none', 'pattern', 'ones')
FOUR_STEPS = (3, 0, 1, 7)                               # step count of each grid at the last of the 7 launches
FOUR_LRS = (0.1, 0.1, 0.0, 0.005)
FOUR_CALLS = max(FOUR_STEPS)
PAD = 64                                                # sentinel voxels behind every array
SENTINEL = 12345.0


def grid_mask(kind, V):
    """uint8 [V] or None; `pattern` turns on voxels 62..66 and every 5th: it cuts the 64-voxel block and the 8-voxel lane group"""
    if kind == 'none':
        return None
    v = np.arange(V)
    m = {'zeros': np.zeros(V, bool), 'ones': np.ones(V, bool), 'pattern': ((v >= 62) & (v <= 66)) | (v % 5 == 0)}[kind]
    return m.astype(np.uint8)


def _grid_data(tag, V, steps):
    r = _rng('grid' + tag, V)
    p0 = r.normal(size=(V, 32)).astype(f32)
    grads = (r.normal(size=(steps, V, 32)) * 10.0 ** r.uniform(-6, 2, size=(steps, V, 32))).astype(f32)
    return p0, grads


@functools.lru_cache(maxsize=None)
def grid_case(V, mask_kind):
    """one grid of V voxels launched alone for GRID_STEPS steps"""
    p0, grads = _grid_data('alone', V, GRID_STEPS)
    mask = grid_mask(mask_kind, V)
    ref = Y.adam(p0, grads, GRID_LRS, mask)
    for a in (p0, grads) + ref:
        a.setflags(write=False)
    return _frozen(V=V, p0=p0, grads=grads, mask=mask, ref=ref, lrs=GRID_LRS)


@functools.lru_cache(maxsize=None)
def four_grids():
    """four grids in one launch, FOUR_CALLS launches: grid k receives gradients (and counts steps) in the last FOUR_STEPS[k]
    launches only -- the way the mapper's stages add grids -- at the constant learning rate FOUR_LRS[k]"""
    out = []
    for k, (V, kind, steps, lr) in enumerate(zip(FOUR_V, FOUR_MASKS, FOUR_STEPS, FOUR_LRS)):
        p0, grads = _grid_data('four%d' % k, V, FOUR_CALLS)        # grads[c] is what launch c finds in the accumulator
        mask = grid_mask(kind, V)
        first = FOUR_CALLS - steps                                  # the first launch that steps this grid
        ref = Y.adam(p0, grads[first:], [lr] * steps, mask) if steps else None
        for a in (p0, grads) + (ref or ()):
            a.setflags(write=False)
        out.append(_frozen(V=V, p0=p0, grads=grads, mask=mask, first=first, steps=steps, lr=lr, ref=ref))
    return out


def moment_bound(grads_so_far, power):
    """how far a float32 moment may be from the float64 one after t steps, element by element: per step the two constants,
    the two products and the sum round (the square once more), each by at most 2^-25 of a quantity no larger than max|g|^power,
    and the old error comes back multiplied by beta < 1: t * 4 * 2^-24 * max_s |g_s|^power"""
    g = np.abs(np.asarray(grads_so_far, np.float64)) ** power
    return len(g) * 4 * 2.0 ** -24 * g.max(0)


# ---- tracker rays -----------------------------------------------------------------------------------------------------------
IMG_H, IMG_W, EDGE_H, EDGE_W = 120, 160, 10, 12         # the image and window of tests/test_hip_tracker.py
WIN_W = IMG_W - 2 * EDGE_W
WIN_H = IMG_H - 2 * EDGE_H
TR_CAM = (150.0, 152.0, 79.5, 59.5)
TR_CAM_INT = (150.0, 152.0, 80.0, 60.0)                 # integer principal point: the pixel (80, 60) looks down -z exactly
TR_BOUND = ((-2.0, 2.5), (-1.5, 2.0), (-1.0, 1.8))
TR_CT = (0.9, 0.1, -0.2, 0.05, 0.3, -0.2, 0.1)
TR_N = (1, 1023, 1024, 1025, 3000)
TR_KINDS = ('last_max', 'none_inside', 'zero_component', 'on_face')
PRINCIPAL = (60 - EDGE_H) * WIN_W + (80 - EDGE_W)       # window index of the pixel (80, 60)


def _mirror(ct, cam, idx, depth, color):
    """what tracker_rays_kernel gathers and computes for the window indices idx"""
    row, col = idx // WIN_W, idx % WIN_W
    pi, pj = (EDGE_W + col).astype(f32), (EDGE_H + row).astype(f32)
    gd = depth[EDGE_H + row, EDGE_W + col]
    gc = color[EDGE_H + row, EDGE_W + col].astype(f32)
    ro, rd = Y.pose_rays(ct, pi, pj, *cam)
    inside, dmax = Y.tracker_prefilter(ro, rd, gd, TR_BOUND)
    return dict(pi=pi, pj=pj, gd=gd, gc=gc, ro=ro, rd=rd, inside=inside, dmax=dmax, dmax_all=Y.depth_max(gd))


@functools.lru_cache(maxsize=None)
def tracker_case(kind, n):
    """a 120 x 160 depth image with holes, a colour image, n window indices and the mirror of the launch's outputs.
    last_max: the largest kept depth belongs to index n - 1; none_inside: every depth is beyond the bound;
    zero_component: identity rotation, integer principal point, the principal pixel sampled (direction components exactly 0);
    on_face: the same with the camera origin on the face x = lo, so that the rays with d_x = 0 divide 0 by 0"""
    r = _rng('trk' + kind, n)
    depth = (r.random((IMG_H, IMG_W)) * 6.0).astype(f32)
    depth[::7, ::5] = 0.0
    color = r.random((IMG_H, IMG_W, 3))                          # float64; the float32 image is its rounding
    idx = r.integers(0, WIN_H * WIN_W, size=n).astype(np.int64)
    ct, cam = np.array(TR_CT, f32), TR_CAM
    if kind in ('zero_component', 'on_face'):
        ct, cam = np.array((1.0, 0.0, 0.0, 0.0, 0.3, -0.2, 0.1), f32), TR_CAM_INT
        idx[n // 2] = PRINCIPAL
        if kind == 'on_face':
            ct[4] = TR_BOUND[0][0]
    if kind == 'none_inside':
        depth[:] = 50.0
    if kind == 'last_max':
        # the pixel whose ray runs longest inside the bound goes last, with a depth just short of that length
        cand = np.arange(WIN_H * WIN_W, dtype=np.int64)
        m = _mirror(ct, cam, cand, depth, color)
        with np.errstate(divide='ignore', invalid='ignore'):
            b = np.asarray(TR_BOUND)
            t = ((b[None] - m['ro'].astype(np.float64)[:, :, None]) / m['rd'].astype(np.float64)[:, :, None]).max(2).min(1)
        best = int(np.argmax(t))
        idx[idx == best] = (best + 1) % (WIN_H * WIN_W)
        idx[n - 1] = best
        depth[EDGE_H + best // WIN_W, EDGE_W + best % WIN_W] = f32(0.995 * t[best])
    out = _mirror(ct, cam, idx, depth, color)
    return _frozen(kind=kind, n=n, ct=ct, cam=cam, idx=idx, depth=depth, color=color, **out)


TR_GRAD_N = 3000


@functools.lru_cache(maxsize=None)
def tracker_grad_case():
    """cotangents for the rays of tracker_case('last_max', TR_GRAD_N), built like those of pose_pixels, and the gradient to the
    camera tensor with its A for each cotangent choice"""
    c = tracker_case('last_max', TR_GRAD_N)
    r = _rng('trkgrad')
    d0, d1 = Y.directions32(c.pi, c.pj, *c.cam)
    d = np.stack([d0, d1, -np.ones(c.n, f32)], -1).astype(np.float64)
    M = np.array([[1.3, -0.8, 0.6], [-0.7, 1.1, -0.9], [0.9, 0.5, 1.2]])
    px = _frozen(pi=c.pi, pj=c.pj, g_rd=(d @ M.T + 0.4 * r.normal(size=(c.n, 3))).astype(f32),
                 g_ro=(np.array([0.7, -0.4, 0.9]) + 0.5 * r.normal(size=(c.n, 3))).astype(f32))
    grad = {which: Y.pose_rays_grad(c.ct, c.pi, c.pj, *c.cam, *cotangents(px, which)) for which in COTANGENTS}
    return _frozen(case=c, px=px, grad=grad)


N_DRAWS, DRAW_CALLS, DRAW_N = 3, 4, 1025


@functools.lru_cache(maxsize=None)
def draw_table():
    """[N_DRAWS, DRAW_N] indices drawn ahead and the mirror of each row"""
    base = tracker_case('last_max', DRAW_N)
    idx = _rng('draws').integers(0, WIN_H * WIN_W, size=(N_DRAWS, DRAW_N)).astype(np.int64)
    rows = [_frozen(**_mirror(base.ct, base.cam, idx[k], base.depth, base.color)) for k in range(N_DRAWS)]
    return _frozen(idx=idx, depth=base.depth, color=base.color, ct=base.ct, cam=base.cam, rows=rows)


# ---- batch depth maximum and the sampler ------------------------------------------------------------------------------------
DMAX_N = (1, 1023, 1024, 1025, 4096, 4097, 100000)
DMAX_KINDS = ('last', 'equal', 'zero')


@functools.lru_cache(maxsize=None)
def depth_case(kind, n):
    gd = (0.2 + 4.0 * _rng('dmax', n).random(n)).astype(f32)
    if kind == 'last':
        gd[n - 1] = f32(4.7311)
    if kind == 'equal':
        gd[:] = f32(2.7183)
    if kind == 'zero':
        gd[:] = 0.0
    return _frozen(gd=gd, dmax=Y.depth_max(gd))


SAMPLER_N = (4096, 4097)                                # the in-wave reduction / depth_max_kernel


def sampler_case(scene, n):
    """the tiny scene's rays drawn n times with replacement, about a fifth of the depths zero, the largest depth last"""
    r = _rng('sampler', n)
    pick = r.integers(0, scene['rays_o'].shape[0], size=n)
    ro, rd = scene['rays_o'][pick].astype(f32), scene['rays_d'][pick].astype(f32)
    gd = scene['gt_depth'][pick].astype(f32)
    gd[r.random(n) < 0.2] = 0.0
    gd[n - 1] = f32(1.01) * gd.max()
    return ro, rd, gd
