"""The depth-guided ray sampler restated in plain numpy (Renderer.render_batch_ray lines 83-171; the kernel is sample_body in
csrc/util_kernels.hip): the yardstick of tests/test_sampler_cpu.py and tests/test_hip_sampler.py.  Whole arrays, np.max / np.min
as torch has them (a NaN goes through), np.sort on the values; no lanes and no network.

Every operation carries the dtype the reference's promotion gives it:
  t        float64  (bound - o) / d, o and d widened from float32; one distance per face
  far_bb   float64  min over axes of max over the two faces, + 0.01
  near     float32  gt_depth * 0.01f                      (the constant 0.01f without depth)
  cap      float32  max(gt_depth) * 1.2f, widened         (depth_max()[1])
  far      float64  min(max(far_bb, 0), cap)              (far_bb without depth)
  z_lin    float64  (double)(near * (1.f - t)) + far * (double)t
           lindisp: 1 / ((double)((1.f / near) * (1.f - t)) + (1 / far) * (double)t)        (1.f / near is 100.f without depth)
  perturb  float64  lower + (upper - lower) * (double)t_rand; mids 0.5 * (z[k + 1] + z[k]), the ends keep their own z
  surface  float64  (double)(0.95f * d) * (1 - ts) + (double)(1.05f * d) * ts    where d > 0
                    0.001 * (1 - ts) + (double)max(gt_depth) * ts                where d <= 0
  merge             ascending sort of the n_lin + n_surf values of a ray; without depth nothing is sorted

t_lin (float32 [n_lin]) and t_surf (float64 [n_surf]) are inputs, as they are inputs of the C ABI.

A ray is IN CONTRACT when no face distance is NaN and far_bb, far, near and every z of its row are finite (an infinite face distance
of an axis-parallel ray is in contract: it never becomes far_bb unless all three are).  What the kernel leaves in the row of a ray
outside the contract is unspecified (include/enslam_hip.h).

`defect` names ONE deliberate fault, for tests/test_sampler_cpu.py's proof that the cases can tell it from the yardstick."""
import numpy as np

from tests.step_numpy import depth_max  # noqa: F401  (the batch maxima {max d, fl32(max d * 1.2f)}: one restatement for both files)

f32, f64 = np.float32, np.float64

DEFECTS = ('near product in float64', '1.2 applied in float64', '0.95f * d in float64', 'no-depth surface end from dmax1',
           "last linear sample's upper from a neighbour", "clamp's lower bound dropped", 'merge skipped when n_surf == 1',
           'subnormal near flushed')


def sample(ro, rd, gd, bound, t_lin, t_surf, lindisp=False, t_rand=None, dmax=None, defect=None):
    """(z float64 [N, S], in_contract bool [N]).  gd None: no depth, S = n_lin.  dmax: float32 [2] replacing depth_max(gd)."""
    assert defect is None or defect in DEFECTS
    o, d = np.asarray(ro, f32).astype(f64), np.asarray(rd, f32).astype(f64)
    b = np.asarray(bound, f64).reshape(3, 2)
    t_lin = np.asarray(t_lin, f32)
    N, n_lin = o.shape[0], t_lin.shape[0]
    with np.errstate(all='ignore'):
        t = (b[None, :, :] - o[:, :, None]) / d[:, :, None]                          # [N, 3, 2]
        far_bb = np.min(np.max(t, axis=2), axis=1) + 0.01
        ok = ~np.isnan(t).any(axis=(1, 2)) & np.isfinite(far_bb)
        omt = f32(1.0) - t_lin
        if gd is None:
            near = np.full(N, 0.01, f32)
            inv_near = np.full(N, 100.0, f32)
            far = far_bb
        else:
            gd = np.asarray(gd, f32).reshape(N)
            dm = depth_max(gd) if dmax is None else np.asarray(dmax, f32)
            near = gd * f32(0.01)
            if defect == 'subnormal near flushed':
                near = np.where(np.abs(near) < np.finfo(f32).tiny, f32(0.0), near).astype(f32)
            inv_near = f32(1.0) / near
            cap = f64(dm[0]) * 1.2 if defect == '1.2 applied in float64' else f64(dm[1])
            far = far_bb if defect == "clamp's lower bound dropped" else np.maximum(far_bb, 0.0)
            far = np.minimum(far, cap)
        if not lindisp:
            if defect == 'near product in float64':
                lead = near.astype(f64)[:, None] * omt.astype(f64)[None, :]
            else:
                lead = (near[:, None] * omt[None, :]).astype(f64)                    # float32 product, then widened
            z = lead + far[:, None] * t_lin.astype(f64)[None, :]
        else:
            z = 1.0 / ((inv_near[:, None] * omt[None, :]).astype(f64) + (1.0 / far)[:, None] * t_lin.astype(f64)[None, :])
        ok &= np.isfinite(far) & np.isfinite(near)
        if t_rand is not None:
            mids = 0.5 * (z[:, 1:] + z[:, :-1])
            upper = np.concatenate([mids, z[:, -1:]], axis=1)
            lower = np.concatenate([z[:, :1], mids], axis=1)
            if defect == "last linear sample's upper from a neighbour" and n_lin >= 2:
                upper[:, -1] = mids[:, -1]
            z = lower + (upper - lower) * np.asarray(t_rand, f32).astype(f64)
        n_surf = 0 if gd is None or t_surf is None else len(t_surf)
        if n_surf > 0:
            ts = np.asarray(t_surf, f64)[None, :]
            if defect == '0.95f * d in float64':
                a = gd.astype(f64) * 0.95
            else:
                a = (f32(0.95) * gd).astype(f64)
            c = (f32(1.05) * gd).astype(f64)
            end = f64(dm[1] if defect == 'no-depth surface end from dmax1' else dm[0])
            zs = np.where((gd > 0)[:, None], a[:, None] * (1.0 - ts) + c[:, None] * ts, 0.001 * (1.0 - ts) + end * ts)
            z = np.concatenate([z, zs], axis=1)
            if not (defect == 'merge skipped when n_surf == 1' and n_surf == 1):
                z = np.sort(z, axis=1)
        ok &= np.isfinite(z).all(axis=1)
    return z, ok
