"""Float64 numpy yardstick for the NICE decoder BACKWARD (tests/test_decoder_bwd_cpu.py, tests/test_hip_decoder_bwd.py): the
gradients of  sum(raw * d_raw)  of Renderer.eval_points on the samples of a ray batch, for a cotangent d_raw the caller chooses.

It is built on tests/decoder_numpy.py (same forward helpers, same float32 fractions) and restates the REFERENCE's autograd
rules, not the kernels:
  mask        a sample that is not strictly inside the bound sends no OCCUPANCY gradient (its occupancy is overwritten by 100);
              its COLOUR gradient flows                                                             (Renderer.eval_points)
  fine concat c_middle inside the fine decoder's input is detached: no gradient to grid_middle and none to the position
  colour      the colour decoder's fourth output row gets no gradient (only [:, :3] is used); the colour columns of d_raw are
              ignored in the coarse / middle / fine stages                                          (decoder.py: NICE.forward)
  position    grid path: through the three fractions, factor (size - 1) / (hi - lo) per axis, zero on an axis whose
              unnormalised float32 coordinate is clipped (ATen's border rule: the `inner` flags), the fractions themselves
              the float32 values of blocks_numpy.cells;  embedding path: through cos(float32(p) @ B) * B
  z_vals      no gradient;  g_rays_o = sum_s dp,  g_rays_d = sum_s z * dp
  coarse      features only, over the doubled bound, ray gradient through the grid path alone
Every sum is a float64 numpy sum over the float32 parameter values cast to float64.

Next to every gradient g the module returns its SCALE array A, the same sum with every term replaced by its absolute value, so
that a bar can be stated per element (|error| <= bar * A) and A == 0 exactly where nothing touched the element:
  grid row v     sum over (sample s, tap k hitting v) of |w_k(s)| * max_ch |dC[s, ch]|   (one value per voxel, all 32 channels;
                 the per-channel sum |w * dC| is NOT used: dC cancels across the five fc_c layers)
  weight W[i,j]  sum_s D[s, i] * X[s, j], where D[s, i] = max_i' |delta[s, i']| if delta[s, i] != 0 else 0 and X likewise from
                 the layer's input (`sample_scale`, `weight_scale` say why);   bias: sum_s D[s, i]
  rays_o[r]      sum_s max_axis |dp[s]|;            rays_d[r]: the same weighted by z

The small helpers (`SCATTER_TAPS`, `occupancy_mask`, `colour_mask`, `fine_middle_feature_grad`, `colour_output_cotangent`,
`runs_colour`, `inner`, `embedding_slope`, `weight_grad`, `ray_weights`, `contributing`) exist so that
tests/test_decoder_bwd_cpu.py can state a wrong variant as a one-line replacement of one of them."""
import numpy as np

from tests import blocks_numpy as BN
from tests import decoder_numpy as DN

F32, F64 = np.float32, np.float64
as64 = DN.as64
N_BLOCKS, SKIP = DN.N_BLOCKS, DN.SKIP
SCATTER_TAPS = tuple(range(8))
STAGE_DECODERS = {'coarse': ('coarse_decoder',), 'middle': ('middle_decoder',), 'fine': ('middle_decoder', 'fine_decoder'),
                  'color': ('middle_decoder', 'fine_decoder', 'color_decoder')}
STAGE_GRIDS = {'coarse': ('grid_coarse',), 'middle': ('grid_middle',), 'fine': ('grid_middle', 'grid_fine'),
               'color': ('grid_middle', 'grid_fine', 'grid_color')}


# ------------------------------------------------------------------------------------------------ the rules, one helper each
def occupancy_mask(keep):
    """which samples send an occupancy gradient: the ones strictly inside the bound"""
    return keep


def colour_mask(keep):
    """which samples send a colour gradient: all of them (the mask overwrites the occupancy only)"""
    return np.ones_like(keep)


def fine_middle_feature_grad(dc_middle_part):
    """what the fine decoder's gradient w.r.t. its concatenated middle feature sends on: nothing (detached)"""
    return np.zeros_like(dc_middle_part)


def colour_output_cotangent(d_rgb):
    """cotangent of the colour decoder's four outputs: the fourth is unused"""
    return np.concatenate([d_rgb, np.zeros((d_rgb.shape[0], 1), dtype=F64)], axis=-1)


def runs_colour(stage):
    """the colour columns of d_raw count in the colour stage only"""
    return stage == 'color'


def inner(co, size):
    """ATen's clip_coordinates_set_grad on the unnormalised float32 coordinate: no gradient on a clipped axis"""
    return (co > F32(0.0)) & (co < F32(size - 1))


def embedding_slope(arg):
    return np.cos(arg)


def weight_grad(layer, delta, x):
    """[out, in] = sum_s delta[s, out] * x[s, in]"""
    return delta.T @ x


def ray_weights(z):
    """the factor of dp in g_rays_d: d(o + d z)/dd = z"""
    return z


def contributing(d_raw):
    """the cotangent rows that enter the sums: all of them"""
    return d_raw


# ------------------------------------------------------------------------------------------------ grids
def coordinates(points, bound, dims):
    """per axis (x, y, z): unnormalised float32 coordinate before the clip, its grid size, and d(coordinate)/d(p) in float64"""
    points, bound = as64(points), as64(bound)
    D, H, W = (int(v) for v in dims)
    out = []
    for a, size in ((0, W), (1, H), (2, D)):
        co = BN.unnormalise(BN.normalise(points[:, a], bound[a, 0], bound[a, 1]), size)
        out.append((co, size, F64(size - 1) / (bound[a, 1] - bound[a, 0])))
    return out


def tap_weights(fx, fy, fz, k):
    """float64 (weight, d/dfx, d/dfy, d/dfz) of tap k = 4 dz + 2 dy + dx"""
    dx, dy, dz = k & 1, (k >> 1) & 1, k >> 2
    wx, wy, wz = (fx if dx else 1.0 - fx), (fy if dy else 1.0 - fy), (fz if dz else 1.0 - fz)
    sx, sy, sz = (1.0 if dx else -1.0), (1.0 if dy else -1.0), (1.0 if dz else -1.0)
    return (wx * wy) * wz, sx * wy * wz, wx * sy * wz, wx * wy * sz


def grid_backward(grid, points, bound, dC):
    """gradient of a [1, 32, D, H, W] grid and of the points through the trilinear gather, for the feature cotangent dC [P, 32]:
    (g [32, V], A [V], dp [P, 3])"""
    grid = np.asarray(grid)
    dims = grid.shape[2:]
    C, V = grid.shape[1], int(np.prod(dims))
    v = BN.cells(points, bound, dims)
    idx, exists, _ = BN.corners(points, bound, dims)
    fx, fy, fz = as64(v['fx']), as64(v['fy']), as64(v['fz'])
    g64 = as64(grid).reshape(C, V)
    g, A = np.zeros((V, C), dtype=F64), np.zeros(V, dtype=F64)
    big = np.abs(dC).max(axis=1)
    dfrac = np.zeros((dC.shape[0], 3), dtype=F64)
    for k in range(8):
        w, *dw = tap_weights(fx, fy, fz, k)
        ok = exists[:, k]
        if k in SCATTER_TAPS:
            np.add.at(g, idx[:, k], np.where(ok, w, 0.0)[:, None] * dC)
            np.add.at(A, idx[:, k], np.where(ok, np.abs(w), 0.0) * big)
        along = (g64[:, idx[:, k]].T * dC).sum(axis=1)              # sum_ch dC[s, ch] * grid[ch, tap]
        for a in range(3):
            dfrac[:, a] += np.where(ok, dw[a], 0.0) * along
    dp = np.zeros_like(dfrac)
    for a, (co, size, slope) in enumerate(coordinates(points, bound, dims)):
        dp[:, a] = np.where(inner(co, size), dfrac[:, a] * slope, 0.0)
    return np.ascontiguousarray(g.T), A, dp


# ------------------------------------------------------------------------------------------------ decoders
def _W(params, key):
    return as64(params[key + '.weight'])


def xyz_forward(params, name, points, c):
    arg = DN.fourier_argument(points, params[name + '.embedder._B'])
    emb = np.sin(arg)
    h, xs, pres = emb, [], []
    for i in range(N_BLOCKS):
        xs.append(h)
        pres.append(DN.linear(params, f'{name}.pts_linears.{i}', h))
        h = DN.relu(pres[i]) + DN.linear(params, f'{name}.fc_c.{i}', c)
        if i == SKIP:
            h = DN.skip_concat(emb, h)
    return dict(arg=arg, emb=emb, xs=xs, pres=pres, h=h, c=c, out=DN.linear(params, name + '.output_linear', h))


def feat_forward(params, name, c):
    h, xs, pres = c, [], []
    for i in range(N_BLOCKS):
        xs.append(h)
        pres.append(DN.linear(params, f'{name}.pts_linears.{i}', h))
        h = DN.relu(pres[i])
        if i == SKIP:
            h = DN.skip_concat(c, h)
    return dict(xs=xs, pres=pres, h=h, c=c, out=DN.linear(params, name + '.output_linear', h))


def sample_scale(v):
    """|v| with every non-zero entry of a row replaced by the row's largest: [P, n].  A layer's input x[s, :] and its output
    cotangent delta[s, :] are themselves sums whose terms cancel (a hidden activation a thousand times below its neighbours
    still carries their rounding), so the error of an entry scales with the largest entry of its sample, not with itself --
    the reason the grid scale takes max_ch |dC|.  Exact zeros stay zero: an entry that contributes nothing has no error."""
    v = np.abs(v)
    return v.max(axis=1, keepdims=True) * (v != 0)


def weight_scale(delta, x):
    """A of a weight gradient: sum_s sample_scale(delta)[s, i] * sample_scale(x)[s, j].  With the plain sum |delta| * |x| the
    float32 oracle itself sits at 7.5e-5 of A on single-sample elements of the coarse decoder's nearly dead units (1e-6
    elsewhere), and one such element sets the bar of its whole family; with this scale it sits at 4e-8 to 2e-7 everywhere.
    A stays 0 exactly where no sample contributes, and A >= sum |delta| * |x| >= |g|."""
    return sample_scale(delta).T @ sample_scale(x)


def _layer(g, A, key, delta, x):
    g[key + '.weight'], A[key + '.weight'] = weight_grad(key, delta, x), weight_scale(delta, x)
    g[key + '.bias'], A[key + '.bias'] = delta.sum(axis=0), sample_scale(delta).sum(axis=0)


def xyz_backward(params, name, fw, d_out, points):
    """(g, A) of the decoder's parameters, dc [P, c_dim], dp [P, 3] through the embedding"""
    g, A = {}, {}
    _layer(g, A, name + '.output_linear', d_out, fw['h'])
    dh = d_out @ _W(params, name + '.output_linear')
    n_emb = fw['emb'].shape[1]
    d_emb, dc = np.zeros_like(fw['emb']), np.zeros_like(fw['c'])
    for i in reversed(range(N_BLOCKS)):
        if i == SKIP:
            d_emb, dh = d_emb + dh[:, :n_emb], dh[:, n_emb:]
        _layer(g, A, f'{name}.fc_c.{i}', dh, fw['c'])
        dc += dh @ _W(params, f'{name}.fc_c.{i}')
        delta = dh * (fw['pres'][i] > 0)
        _layer(g, A, f'{name}.pts_linears.{i}', delta, fw['xs'][i])
        dh = delta @ _W(params, f'{name}.pts_linears.{i}')
    d_arg = (d_emb + dh) * embedding_slope(fw['arg'])
    B = as64(params[name + '.embedder._B'])
    p32 = as64(points).astype(F32).astype(F64)
    g[name + '.embedder._B'], A[name + '.embedder._B'] = p32.T @ d_arg, weight_scale(p32, d_arg)
    return g, A, dc, d_arg @ B.T


def feat_backward(params, name, fw, d_out):
    g, A = {}, {}
    _layer(g, A, name + '.output_linear', d_out, fw['h'])
    dh = d_out @ _W(params, name + '.output_linear')
    n_c = fw['c'].shape[1]
    dc = np.zeros_like(fw['c'])
    for i in reversed(range(N_BLOCKS)):
        if i == SKIP:
            dc, dh = dc + dh[:, :n_c], dh[:, n_c:]
        delta = dh * (fw['pres'][i] > 0)
        _layer(g, A, f'{name}.pts_linears.{i}', delta, fw['xs'][i])
        dh = delta @ _W(params, f'{name}.pts_linears.{i}')
    return g, A, dc + dh


# ------------------------------------------------------------------------------------------------ the stage
def forward(params, grids, points, stage, bound, coarse_enlarge=2):
    """{decoder: its forward record} of the stage (features, layer inputs, pre-activations, output)"""
    points, bound = as64(points), as64(bound)
    if stage == 'coarse':
        return {'coarse_decoder': feat_forward(params, 'coarse_decoder', DN.interp(grids['grid_coarse'], points, bound * coarse_enlarge))}
    c_mid = DN.interp(grids['grid_middle'], points, bound)
    fw = {'middle_decoder': xyz_forward(params, 'middle_decoder', points, c_mid)}
    if stage == 'middle':
        return fw
    c_fine = DN.fine_features(DN.interp(grids['grid_fine'], points, bound), c_mid)
    fw['fine_decoder'] = xyz_forward(params, 'fine_decoder', points, c_fine)
    if stage == 'color':
        fw['color_decoder'] = colour_forward(params, grids, points, bound)
    return fw


def colour_forward(params, grids, points, bound):
    return xyz_forward(params, 'color_decoder', points, DN.interp(grids['grid_color'], points, bound))


def preactivations(params, grids, points, stage, bound):
    """{decoder of the stage: float64 [P, 5, 32]} hidden pre-activations"""
    fw = forward(params, grids, points, stage, bound)
    return {name: np.stack(fw[name]['pres'], axis=1) for name in STAGE_DECODERS[stage]}


def backward(params, grids, rays_o, rays_d, z_vals, d_raw, stage, bound, coarse_enlarge=2):
    """(g, A): dicts over 'grid_*' ([32, V]; A [V]), the decoders' parameter names, 'rays_o' and 'rays_d' ([N, 3]; A [N]);
    A also holds 'dC_max'"""
    points = BN.sample_points(rays_o, rays_d, z_vals)
    bound = as64(bound)
    N, S = np.asarray(z_vals).shape
    d_raw = contributing(as64(d_raw).reshape(N * S, 4))
    keep = DN.inside_bound(points, bound)
    d_occ = (d_raw[:, 3] * occupancy_mask(keep))[:, None]
    fw = forward(params, grids, points, stage, bound, coarse_enlarge)
    g, A = {}, {}
    dp = np.zeros((N * S, 3), dtype=F64)

    dC_max = [0.0]

    def grid(name, dC, lookup_bound):
        dC_max[0] = max(dC_max[0], float(np.abs(dC).max()))
        g[name], A[name], dpg = grid_backward(grids[name], points, lookup_bound, dC)
        return dpg

    def merge(gA):
        g.update(gA[0])
        A.update(gA[1])

    if stage == 'coarse':
        *gA, dc = feat_backward(params, 'coarse_decoder', fw['coarse_decoder'], d_occ)
        merge(gA)
        dp += grid('grid_coarse', dc, bound * coarse_enlarge)
    else:
        *gA, dc_mid, dpe = xyz_backward(params, 'middle_decoder', fw['middle_decoder'], d_occ, points)
        merge(gA)
        dp += dpe
        if stage in ('fine', 'color'):
            *gA, dc, dpe = xyz_backward(params, 'fine_decoder', fw['fine_decoder'], d_occ, points)
            merge(gA)
            dp += dpe + grid('grid_fine', dc[:, :32], bound)
            dc_mid = dc_mid + fine_middle_feature_grad(dc[:, 32:])
        dp += grid('grid_middle', dc_mid, bound)
        if stage != 'middle' and runs_colour(stage):
            d_rgb = d_raw[:, :3] * colour_mask(keep)[:, None]
            fw_col = fw['color_decoder'] if 'color_decoder' in fw else colour_forward(params, grids, points, bound)
            *gA, dc, dpe = xyz_backward(params, 'color_decoder', fw_col, colour_output_cotangent(d_rgb), points)
            merge(gA)
            dp += dpe + grid('grid_color', dc, bound)
    dp3 = dp.reshape(N, S, 3)
    big = np.abs(dp3).max(axis=2)
    zw = ray_weights(as64(z_vals))
    g['rays_o'], A['rays_o'] = dp3.sum(axis=1), big.sum(axis=1)
    g['rays_d'], A['rays_d'] = (dp3 * zw[:, :, None]).sum(axis=1), (big * np.abs(as64(z_vals))).sum(axis=1)
    A['dC_max'] = dC_max[0]                     # the largest |feature cotangent| of the call (a scalar, not a scale array)
    return g, A
