// Block-sparse TSDF volume: the depth fusion of Mesher.get_bound_from_frames (Mesher.py:214-279, Open3D's
// ScalableTSDFVolume.integrate + extract_triangle_mesh) as HIP kernels.  Conventions and arithmetic: enslam_hip.h.
//
//   touch      one thread per sampled pixel: its world point in float64, the stamp of this frame stored into every unit
//              within sdf_trunc of it (plain stores: all racing stores write the same value)
//   integrate  one workgroup per (touched block, x slab): 256 threads = one (y, z) plane of 16 x 16 voxels, z along the
//              lanes, so the tsdf / weight / colour rows are read and written as whole 64-byte runs
//   count      one workgroup per block (in table order): an 18^3 tile of the block and its one-voxel rim in LDS (tsdf, NaN
//              where nothing was observed), the validity of the 17^3 cells on it, then per voxel the vertex mask of its
//              three owned edges and the case of its cell; per-block vertex and triangle totals (ballots, no atomics)
//   scan       one block: exclusive offsets of the block totals in place, and the grand totals
//   verts      per voxel the first output index of its vertices (kept for the face pass), positions and colours
//   faces      per cell the case table's triangles, corners looked up through the block table
//
// Every output position is a prefix sum of counts in (table index, lattice) order: deterministic to the bit, and
// independent of the order in which frames opened the blocks.  Case table: mc_tables.hpp (a corner is "occupied" iff its
// tsdf < 0, so the triangles' normals point towards positive tsdf, the free space).
#include "../../include/enslam_hip.h"
#include "common.hpp"
#include "mc_tables.hpp"

namespace {

constexpr int TS_B = 16;                                // voxels per block edge
constexpr int TS_V = TS_B * TS_B * TS_B;                // voxels per block
constexpr int TS_THREADS = 256;                         // one (y, z) plane
constexpr int TS_T = TS_B + 2;                          // tile edge: the block and a rim of one voxel
constexpr int TS_C = TS_B + 1;                          // cells per tile edge (lowest corners -1 .. 15)
constexpr int TS_SCAN_THREADS = 1024;
constexpr int64_t TS_MAX_TABLE = 1LL << 27;             // table entries
constexpr int32_t TS_MAX_MESH_BLOCKS = 100000;          // 5 * 4096 * blocks triangles stay in int32
constexpr int32_t TS_MAX_UNIT = (1 << 26);              // |unit| * 16 + 16 stays in int32

struct TsTable {
    int32_t lo[3], nu[3];
    int64_t n;                                          // nu[0] * nu[1] * nu[2]
};

int ts_table(const int32_t* lo, const int32_t* nu, TsTable& t) {
    if (!nu) return ENSLAM_EINVAL;
    t.n = 1;
    for (int a = 0; a < 3; ++a) {
        t.lo[a] = lo ? lo[a] : 0;
        t.nu[a] = nu[a];
        if (nu[a] < 1 || nu[a] > TS_MAX_TABLE) return ENSLAM_EINVAL;
        if (t.lo[a] < -TS_MAX_UNIT || (int64_t)t.lo[a] + nu[a] > TS_MAX_UNIT) return ENSLAM_EUNSUPPORTED;
        t.n *= nu[a];
        if (t.n > TS_MAX_TABLE) return ENSLAM_EUNSUPPORTED;
    }
    return ENSLAM_OK;
}

bool ts_finite(double x) { return x == x && x - x == 0.0; }

struct TsCam {
    double fx, fy, cx, cy;
    double m[12];                                       // c2w (touch) or w2c (integrate), rows of [3,4]
};

int ts_cam(const double* cam, const double* pose, TsCam& c) {
    if (!cam || !pose) return ENSLAM_EINVAL;
    for (int k = 0; k < 4; ++k)
        if (!ts_finite(cam[k])) return ENSLAM_EINVAL;
    if (cam[0] == 0.0 || cam[1] == 0.0) return ENSLAM_EINVAL;
    c.fx = cam[0];
    c.fy = cam[1];
    c.cx = cam[2];
    c.cy = cam[3];
    for (int k = 0; k < 12; ++k) {
        if (!ts_finite(pose[k])) return ENSLAM_EINVAL;
        c.m[k] = pose[k];
    }
    return ENSLAM_OK;
}

// number of lanes below this one whose bit in m is set
ENS_DEV int ts_lanes_below(uint64_t m) {
    return (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

// Exclusive prefix over the 256 threads (in thread order) of a per-thread count 0..7, plus the total.  `red` holds 4 ints per
// call site; the caller separates reuses with a barrier.
ENS_DEV int ts_prefix3(int c, int* red, int& total) {
    const uint64_t b0 = __ballot(c & 1), b1 = __ballot(c & 2), b2 = __ballot(c & 4);
    const int lane_pre = ts_lanes_below(b0) + 2 * ts_lanes_below(b1) + 4 * ts_lanes_below(b2);
    const int wave_tot = __popcll(b0) + 2 * __popcll(b1) + 4 * __popcll(b2);
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) red[w] = wave_tot;
    __syncthreads();
    int off = 0;
    total = 0;
#pragma unroll
    for (int k = 0; k < TS_THREADS / 64; ++k) {
        off += k < w ? red[k] : 0;
        total += red[k];
    }
    return off + lane_pre;
}

// ---------------------------------------------------------------------------------------------------------------- touch
__global__ __launch_bounds__(TS_THREADS) void ts_touch_kernel(const float* __restrict__ depth, int H, int W, int stride, int ws,
                                                              int ns, TsCam c, double trunc, double L, TsTable t, int32_t stamp,
                                                              int32_t* __restrict__ stamps, int32_t* __restrict__ outside) {
    const int n = blockIdx.x * TS_THREADS + threadIdx.x;
    bool out = false;
    if (n < ns) {
        const int j = (n / ws) * stride, i = (n % ws) * stride;
        const double d = (double)depth[(int64_t)j * W + i];
        if (d > 0.0) {
            const double c0 = ((double)i - c.cx) / c.fx * d, c1 = -((double)j - c.cy) / c.fy * d, c2 = -d;
            double ulo[3], uhi[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const double p = ((c0 * c.m[4 * k] + c1 * c.m[4 * k + 1]) + c2 * c.m[4 * k + 2]) + c.m[4 * k + 3];
                ulo[k] = floor((p - trunc) / L);
                uhi[k] = floor((p + trunc) / L);
            }
            // sdf_trunc <= L: at most three units per axis.  The range test is made in float64, so a far-away point is
            // "outside" before anything is converted to an index.
            for (int dx = 0; dx < 3; ++dx)
                for (int dy = 0; dy < 3; ++dy)
                    for (int dz = 0; dz < 3; ++dz) {
                        const double u[3] = {ulo[0] + dx, ulo[1] + dy, ulo[2] + dz};
                        if (!(u[0] <= uhi[0] && u[1] <= uhi[1] && u[2] <= uhi[2])) continue;
                        bool in = true;
#pragma unroll
                        for (int k = 0; k < 3; ++k) in = in && u[k] >= (double)t.lo[k] && u[k] < (double)t.lo[k] + (double)t.nu[k];
                        if (!in) {
                            out = true;
                            continue;
                        }
                        const int64_t e = (((int64_t)((int)u[0] - t.lo[0])) * t.nu[1] + ((int)u[1] - t.lo[1])) * t.nu[2] +
                                          ((int)u[2] - t.lo[2]);
                        stamps[e] = stamp;
                    }
        }
    }
    const int cnt = __syncthreads_count(out ? 1 : 0);
    if (threadIdx.x == 0) outside[blockIdx.x] = cnt;
}

// ------------------------------------------------------------------------------------------------------------ integrate
__global__ __launch_bounds__(TS_THREADS) void ts_integrate_kernel(const float* __restrict__ depth, const float* __restrict__ color,
                                                                  const double* __restrict__ mult, int H, int W, TsCam c, double vl,
                                                                  double trunc, TsTable t, const int32_t* __restrict__ t_block,
                                                                  const int32_t* __restrict__ t_index, int32_t n_blocks,
                                                                  float* __restrict__ tsdf, float* __restrict__ weight,
                                                                  float* __restrict__ vcolor, int32_t* __restrict__ counts) {
    const int item = blockIdx.x >> 4, lx = blockIdx.x & 15;
    const int ly = threadIdx.x >> 4, lz = threadIdx.x & 15;
    const int32_t bid = t_block[item];
    const int64_t e = t_index[item];
    bool done = false;
    if (bid >= 0 && bid < n_blocks && e >= 0 && e < t.n) {
        const int uz = (int)(e % t.nu[2]), uy = (int)((e / t.nu[2]) % t.nu[1]), ux = (int)(e / ((int64_t)t.nu[2] * t.nu[1]));
        const int g[3] = {(t.lo[0] + ux) * TS_B + lx, (t.lo[1] + uy) * TS_B + ly, (t.lo[2] + uz) * TS_B + lz};
        const double p0 = ((double)g[0] + 0.5) * vl, p1 = ((double)g[1] + 0.5) * vl, p2 = ((double)g[2] + 0.5) * vl;
        const double x = ((c.m[0] * p0 + c.m[1] * p1) + c.m[2] * p2) + c.m[3];
        const double y = ((c.m[4] * p0 + c.m[5] * p1) + c.m[6] * p2) + c.m[7];
        const double z = ((c.m[8] * p0 + c.m[9] * p1) + c.m[10] * p2) + c.m[11];
        const double zc = -z;
        if (zc > 0.0) {
            const double uf = (x * c.fx / zc + c.cx) + 0.5, vf = ((-y) * c.fy / zc + c.cy) + 0.5;
            if (uf >= 1e-4 && uf < (double)W - 1e-4 && vf >= 1e-4 && vf < (double)H - 1e-4) {
                const int u = (int)uf, v = (int)vf;
                const int64_t pix = (int64_t)v * W + u;
                const double d = (double)depth[pix];
                if (d > 0.0) {
                    const double sdf = (d - zc) * mult[pix];
                    if (!(sdf <= -trunc)) {
                        const double q = sdf / trunc;
                        const float tt = (float)(q < 1.0 ? q : 1.0);
                        const int64_t o = (int64_t)bid * TS_V + (lx * TS_B + ly) * TS_B + lz;
                        const float w = weight[o], w1 = w + 1.0f;
                        tsdf[o] = (tsdf[o] * w + tt) / w1;
                        if (vcolor) {
#pragma unroll
                            for (int k = 0; k < 3; ++k) vcolor[3 * o + k] = (vcolor[3 * o + k] * w + color[3 * pix + k]) / w1;
                        }
                        weight[o] = w1;
                        done = true;
                    }
                }
            }
        }
    }
    const int cnt = __syncthreads_count(done ? 1 : 0);
    if (threadIdx.x == 0) counts[blockIdx.x] = cnt;
}

// ----------------------------------------------------------------------------------------------------------- extraction
struct TsVol {
    const int32_t* table;         // [t.n] block id or -1
    const int32_t* s_block;       // [n_blocks] block ids in ascending table index
    const int32_t* s_index;       // [n_blocks] their table indices
    const float* tsdf;
    const float* weight;
    int32_t n_blocks;
};

struct TsWork {
    uint8_t* vmask;    // [n_blocks * 4096]  bits 0-2: the +x / +y / +z edge of the voxel carries a vertex
    uint8_t* cases;    // [n_blocks * 4096]  case of the cell at the voxel (0: no valid cell)
    int32_t* vbase;    // [n_blocks * 4096]  first vertex index of the voxel (written where vmask != 0)
    int32_t* blk_v;    // [n_blocks]  vertex count per sorted block, then its exclusive offset
    int32_t* blk_f;    // [n_blocks]  triangle count per sorted block, then its exclusive offset
};

int64_t ts_align(int64_t b) { return (b + 255) & ~(int64_t)255; }

TsWork ts_carve(void* ws, int64_t nb) {
    char* b = (char*)ws;
    TsWork w;
    w.vmask = (uint8_t*)b;  b += ts_align(nb * TS_V);
    w.cases = (uint8_t*)b;  b += ts_align(nb * TS_V);
    w.vbase = (int32_t*)b;  b += ts_align(4 * nb * TS_V);
    w.blk_v = (int32_t*)b;  b += ts_align(4 * nb);
    w.blk_f = (int32_t*)b;
    return w;
}

int64_t ts_workspace_bytes(int64_t nb) { return 2 * ts_align(nb * TS_V) + ts_align(4 * nb * TS_V) + 2 * ts_align(4 * nb); }

// unit coordinates inside the table of table index e
ENS_DEV void ts_unit(const TsTable& t, int64_t e, int& ux, int& uy, int& uz) {
    uz = (int)(e % t.nu[2]);
    uy = (int)((e / t.nu[2]) % t.nu[1]);
    ux = (int)(e / ((int64_t)t.nu[2] * t.nu[1]));
}

// block id of the unit (ux, uy, uz) (table coordinates), -1 when outside the table or absent
ENS_DEV int32_t ts_block_at(const TsVol& v, const TsTable& t, int ux, int uy, int uz) {
    if (ux < 0 || uy < 0 || uz < 0 || ux >= t.nu[0] || uy >= t.nu[1] || uz >= t.nu[2]) return -1;
    const int32_t b = v.table[((int64_t)ux * t.nu[1] + uy) * t.nu[2] + uz];
    return b < v.n_blocks ? b : -1;
}

// flat voxel address (block id * 4096 + local) of the voxel (lx + dx, ly + dy, lz + dz), d in {0, 1}, of the block at table
// unit (ux, uy, uz); -1 when it falls into an absent block
ENS_DEV int64_t ts_voxel_at(const TsVol& v, const TsTable& t, int32_t bid, int ux, int uy, int uz, int lx, int ly, int lz) {
    int32_t b = bid;
    if (lx >= TS_B || ly >= TS_B || lz >= TS_B) {
        b = ts_block_at(v, t, ux + (lx >= TS_B), uy + (ly >= TS_B), uz + (lz >= TS_B));
        if (b < 0) return -1;
    }
    return (int64_t)b * TS_V + (((lx & 15) * TS_B + (ly & 15)) * TS_B + (lz & 15));
}

__global__ __launch_bounds__(TS_THREADS) void ts_count_kernel(TsVol v, TsTable t, TsWork w) {
    __shared__ float tile[TS_T * TS_T * TS_T];           // tsdf of the block and its rim; NaN: absent or weight <= 0
    __shared__ uint8_t cellv[TS_C * TS_C * TS_C];        // validity of the cell whose lowest corner is tile point (x, y, z)
    __shared__ int32_t nb[27];
    __shared__ int red[2][TS_THREADS / 64];
    const int s = blockIdx.x;
    const int32_t bid = v.s_block[s];
    if (bid < 0 || bid >= v.n_blocks || v.s_index[s] < 0 || v.s_index[s] >= t.n) {      // uniform over the workgroup
        if (threadIdx.x == 0) w.blk_v[s] = w.blk_f[s] = 0;
        return;
    }
    int ux, uy, uz;
    ts_unit(t, v.s_index[s], ux, uy, uz);
    if (threadIdx.x < 27) {
        const int k = threadIdx.x;
        nb[k] = ts_block_at(v, t, ux + k / 9 - 1, uy + (k / 3) % 3 - 1, uz + k % 3 - 1);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < TS_T * TS_T * TS_T; i += TS_THREADS) {
        const int tz = i % TS_T, ty = (i / TS_T) % TS_T, tx = i / (TS_T * TS_T);
        // tile coordinate 0 is local -1 (the unit below), 1..16 the block, 17 local 16 (the unit above)
        const int kx = (tx + TS_B - 1) >> 4, ky = (ty + TS_B - 1) >> 4, kz = (tz + TS_B - 1) >> 4;
        const int32_t b = nb[(kx * 3 + ky) * 3 + kz];
        float val = __builtin_nanf("");
        if (b >= 0) {
            const int64_t o = (int64_t)b * TS_V + ((((tx - 1) & 15) * TS_B + ((ty - 1) & 15)) * TS_B + ((tz - 1) & 15));
            if (v.weight[o] > 0.0f) val = v.tsdf[o];
        }
        tile[i] = val;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < TS_C * TS_C * TS_C; i += TS_THREADS) {
        const int cz = i % TS_C, cy = (i / TS_C) % TS_C, cx = i / (TS_C * TS_C);
        bool ok = true;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const float a = tile[((cx + (k & 1)) * TS_T + cy + ((k >> 1) & 1)) * TS_T + cz + ((k >> 2) & 1)];
            ok = ok && a == a;
        }
        cellv[i] = ok ? 1 : 0;
    }
    __syncthreads();
    const int ly = threadIdx.x >> 4, lz = threadIdx.x & 15;
    int sum_v = 0, sum_f = 0;
    for (int lx = 0; lx < TS_B; ++lx) {
        const int p = ((lx + 1) * TS_T + ly + 1) * TS_T + lz + 1;                 // the voxel in the tile
        const int stride[3] = {TS_T * TS_T, TS_T, 1};
        const float a = tile[p];
        int vm = 0, cs = 0;
        if (a == a) {
            // cell whose lowest corner is the voxel itself: tile point (lx + 1, ly + 1, lz + 1)
            const int c = ((lx + 1) * TS_C + ly + 1) * TS_C + lz + 1;
            const int cst[3] = {TS_C * TS_C, TS_C, 1};
#pragma unroll
            for (int ax = 0; ax < 3; ++ax) {
                const float b = tile[p + stride[ax]];
                if (b == b && (a < 0.0f) != (b < 0.0f)) {
                    const int o1 = cst[(ax + 1) % 3], o2 = cst[(ax + 2) % 3];
                    if (cellv[c] | cellv[c - o1] | cellv[c - o2] | cellv[c - o1 - o2]) vm |= 1 << ax;
                }
            }
            if (cellv[c]) {
#pragma unroll
                for (int k = 0; k < 8; ++k)
                    cs |= (tile[p + (k & 1) * stride[0] + ((k >> 1) & 1) * stride[1] + ((k >> 2) & 1)] < 0.0f ? 1 : 0) << k;
            }
        }
        const int64_t o = (int64_t)bid * TS_V + (lx * TS_B + ly) * TS_B + lz;
        w.vmask[o] = (uint8_t)vm;
        w.cases[o] = (uint8_t)cs;
        int tv, tf;
        ts_prefix3(__popc(vm), red[0], tv);
        ts_prefix3(mc_tri_count[cs], red[1], tf);
        sum_v += tv;
        sum_f += tf;
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        w.blk_v[s] = sum_v;
        w.blk_f[s] = sum_f;
    }
}

// One block: per-block counts -> exclusive offsets (in place); counts[0..1] = total vertices, total triangles.
__global__ __launch_bounds__(TS_SCAN_THREADS) void ts_scan_kernel(TsWork w, int32_t n, int32_t* __restrict__ counts) {
    __shared__ int sv[TS_SCAN_THREADS], sf[TS_SCAN_THREADS];
    const int chunk = (n + TS_SCAN_THREADS - 1) / TS_SCAN_THREADS;
    const int lo = min((int)threadIdx.x * chunk, n);
    const int hi = min(lo + chunk, n);
    int v = 0, f = 0;
    for (int i = lo; i < hi; ++i) {
        v += w.blk_v[i];
        f += w.blk_f[i];
    }
    sv[threadIdx.x] = v;
    sf[threadIdx.x] = f;
    __syncthreads();
    for (int o = 1; o < TS_SCAN_THREADS; o <<= 1) {       // inclusive Hillis-Steele scan
        const int av = threadIdx.x >= o ? sv[threadIdx.x - o] : 0;
        const int af = threadIdx.x >= o ? sf[threadIdx.x - o] : 0;
        __syncthreads();
        sv[threadIdx.x] += av;
        sf[threadIdx.x] += af;
        __syncthreads();
    }
    int ov = sv[threadIdx.x] - v, of = sf[threadIdx.x] - f;
    for (int i = lo; i < hi; ++i) {
        const int cv = w.blk_v[i], cf = w.blk_f[i];
        w.blk_v[i] = ov;
        w.blk_f[i] = of;
        ov += cv;
        of += cf;
    }
    if (threadIdx.x == TS_SCAN_THREADS - 1) {
        counts[0] = sv[threadIdx.x];
        counts[1] = sf[threadIdx.x];
    }
}

// Vertex of the +a edge of voxel g: centre(g) + t_a / (t_a - t_b) * voxel_length along a, float64; colour: the same
// interpolation of the two voxels' colours, clipped to [0, 1] and rounded to uint8.
__global__ __launch_bounds__(TS_THREADS) void ts_verts_kernel(TsVol v, TsTable t, TsWork w, const float* __restrict__ vcolor,
                                                              double vl, int32_t n_verts, double* __restrict__ verts,
                                                              uint8_t* __restrict__ colors) {
    __shared__ int red[TS_THREADS / 64];
    const int s = blockIdx.x;
    const int32_t bid = v.s_block[s];
    if (bid < 0 || bid >= v.n_blocks || v.s_index[s] < 0 || v.s_index[s] >= t.n) return;  // uniform over the workgroup
    int ux, uy, uz;
    ts_unit(t, v.s_index[s], ux, uy, uz);
    const int ly = threadIdx.x >> 4, lz = threadIdx.x & 15;
    int base = w.blk_v[s];
    for (int lx = 0; lx < TS_B; ++lx) {
        const int64_t o = (int64_t)bid * TS_V + (lx * TS_B + ly) * TS_B + lz;
        const int vm = w.vmask[o];
        int total;
        int k = base + ts_prefix3(__popc(vm), red, total);
        base += total;
        if (vm) {
            w.vbase[o] = k;
            const int l[3] = {lx, ly, lz};
            const double ctr[3] = {((double)((t.lo[0] + ux) * TS_B + lx) + 0.5) * vl, ((double)((t.lo[1] + uy) * TS_B + ly) + 0.5) * vl,
                                   ((double)((t.lo[2] + uz) * TS_B + lz) + 0.5) * vl};
            const double ta = (double)v.tsdf[o];
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                if (!(vm & (1 << a))) continue;
                const int64_t q = ts_voxel_at(v, t, bid, ux, uy, uz, l[0] + (a == 0), l[1] + (a == 1), l[2] + (a == 2));
                if (q >= 0 && k < n_verts) {               // q < 0 cannot happen for a counted vertex
                    const double tb = (double)v.tsdf[q];
                    const double frac = ta / (ta - tb);
#pragma unroll
                    for (int c = 0; c < 3; ++c) verts[3 * (int64_t)k + c] = c == a ? ctr[c] + frac * vl : ctr[c];
                    if (colors) {
#pragma unroll
                        for (int c = 0; c < 3; ++c) {
                            const double ca = (double)vcolor[3 * o + c], cb = (double)vcolor[3 * q + c];
                            double col = ca + frac * (cb - ca);
                            col = col < 0.0 ? 0.0 : (col > 1.0 ? 1.0 : col);
                            colors[3 * (int64_t)k + c] = (uint8_t)floor(col * 255.0 + 0.5);
                        }
                    }
                }
                ++k;
            }
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(TS_THREADS) void ts_faces_kernel(TsVol v, TsTable t, TsWork w, int32_t n_faces,
                                                              int32_t* __restrict__ faces) {
    __shared__ int red[TS_THREADS / 64];
    const int s = blockIdx.x;
    const int32_t bid = v.s_block[s];
    if (bid < 0 || bid >= v.n_blocks || v.s_index[s] < 0 || v.s_index[s] >= t.n) return;  // uniform over the workgroup
    int ux, uy, uz;
    ts_unit(t, v.s_index[s], ux, uy, uz);
    const int ly = threadIdx.x >> 4, lz = threadIdx.x & 15;
    int base = w.blk_f[s];
    for (int lx = 0; lx < TS_B; ++lx) {
        const int64_t o = (int64_t)bid * TS_V + (lx * TS_B + ly) * TS_B + lz;
        const int cs = w.cases[o];
        const int nt = mc_tri_count[cs];
        int total;
        const int first = base + ts_prefix3(nt, red, total);
        base += total;
        for (int k = 0; k < nt && first + k < n_faces; ++k) {
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const int e = mc_tri_edges[cs][3 * k + j];
                const int c0 = mc_edge_c0[e], a = e >> 2;
                const int64_t q = ts_voxel_at(v, t, bid, ux, uy, uz, lx + (c0 & 1), ly + ((c0 >> 1) & 1), lz + ((c0 >> 2) & 1));
                // q >= 0: every corner of a valid cell lies in an allocated block
                faces[3 * (int64_t)(first + k) + j] = q >= 0 ? w.vbase[q] + __popc(w.vmask[q] & ((1 << a) - 1)) : 0;
            }
        }
        __syncthreads();
    }
}

int ts_vol(const int32_t* table, int32_t n_blocks, const int32_t* s_block, const int32_t* s_index,
           const float* tsdf, const float* weight, TsVol& v) {
    if (n_blocks < 0) return ENSLAM_EINVAL;
    if (n_blocks > TS_MAX_MESH_BLOCKS) return ENSLAM_EUNSUPPORTED;
    if (!table || (n_blocks > 0 && (!s_block || !s_index || !tsdf || !weight))) return ENSLAM_EINVAL;
    v.table = table;
    v.s_block = s_block;
    v.s_index = s_index;
    v.tsdf = tsdf;
    v.weight = weight;
    v.n_blocks = n_blocks;
    return ENSLAM_OK;
}

}  // namespace

extern "C" {

int enslam_tsdf_touch(const float* depth, int32_t H, int32_t W, int32_t stride, const double* cam_host, const double* c2w_host,
                      double sdf_trunc, double voxel_length, const int32_t* unit_lo_host, const int32_t* nu_host, int32_t stamp,
                      int32_t* stamps, int32_t* outside_partials, void* stream) {
    TsTable t;
    TsCam c;
    int rc = ts_table(unit_lo_host, nu_host, t);
    if (rc != ENSLAM_OK) return rc;
    if (!unit_lo_host) return ENSLAM_EINVAL;
    rc = ts_cam(cam_host, c2w_host, c);
    if (rc != ENSLAM_OK) return rc;
    if (!depth || !stamps || !outside_partials || H < 1 || W < 1 || stride < 1 || (int64_t)H * W > (1LL << 30)) return ENSLAM_EINVAL;
    if (!ts_finite(sdf_trunc) || !ts_finite(voxel_length) || voxel_length <= 0.0 || sdf_trunc <= 0.0 ||
        sdf_trunc > TS_B * voxel_length)
        return ENSLAM_EINVAL;
    const int hs = (H + stride - 1) / stride, ws = (W + stride - 1) / stride;
    const int ns = hs * ws;
    ts_touch_kernel<<<(ns + TS_THREADS - 1) / TS_THREADS, TS_THREADS, 0, (hipStream_t)stream>>>(
        depth, H, W, stride, ws, ns, c, sdf_trunc, (double)TS_B * voxel_length, t, stamp, stamps, outside_partials);
    return hipGetLastError() == hipSuccess ? ENSLAM_OK : ENSLAM_ELAUNCH;
}

int enslam_tsdf_integrate(const float* depth, const float* color, const double* mult, int32_t H, int32_t W, const double* cam_host,
                          const double* w2c_host, double voxel_length, double sdf_trunc, const int32_t* unit_lo_host,
                          const int32_t* nu_host, int32_t n_touched, const int32_t* touched_block, const int32_t* touched_index,
                          int32_t n_blocks, float* tsdf, float* weight, float* vcolor, int32_t* voxel_counts, void* stream) {
    TsTable t;
    TsCam c;
    int rc = ts_table(unit_lo_host, nu_host, t);
    if (rc != ENSLAM_OK) return rc;
    if (!unit_lo_host) return ENSLAM_EINVAL;
    rc = ts_cam(cam_host, w2c_host, c);
    if (rc != ENSLAM_OK) return rc;
    if (!depth || !mult || H < 1 || W < 1 || (int64_t)H * W > (1LL << 30) || n_touched < 0 || n_blocks < 0 || n_touched > n_blocks)
        return ENSLAM_EINVAL;
    if ((color == nullptr) != (vcolor == nullptr)) return ENSLAM_EINVAL;
    if (!ts_finite(sdf_trunc) || !ts_finite(voxel_length) || voxel_length <= 0.0 || sdf_trunc <= 0.0 ||
        sdf_trunc > TS_B * voxel_length)
        return ENSLAM_EINVAL;
    if (n_touched > (1 << 26)) return ENSLAM_EUNSUPPORTED;
    if (n_touched == 0) return ENSLAM_OK;
    if (!touched_block || !touched_index || !tsdf || !weight || !voxel_counts) return ENSLAM_EINVAL;
    ts_integrate_kernel<<<n_touched * TS_B, TS_THREADS, 0, (hipStream_t)stream>>>(depth, color, mult, H, W, c, voxel_length, sdf_trunc,
                                                                                   t, touched_block, touched_index, n_blocks, tsdf,
                                                                                   weight, vcolor, voxel_counts);
    return hipGetLastError() == hipSuccess ? ENSLAM_OK : ENSLAM_ELAUNCH;
}

int enslam_tsdf_mesh_workspace(int32_t n_blocks, int64_t* bytes_host) {
    if (n_blocks < 0 || !bytes_host) return ENSLAM_EINVAL;
    if (n_blocks > TS_MAX_MESH_BLOCKS) return ENSLAM_EUNSUPPORTED;
    *bytes_host = ts_workspace_bytes(n_blocks > 0 ? n_blocks : 1);
    return ENSLAM_OK;
}

int enslam_tsdf_mesh_count(const int32_t* table, const int32_t* nu_host, int32_t n_blocks,
                           const int32_t* sorted_block, const int32_t* sorted_index, const float* tsdf, const float* weight,
                           void* workspace, int32_t* counts, void* stream) {
    TsTable t;
    TsVol v;
    int rc = ts_table(nullptr, nu_host, t);
    if (rc != ENSLAM_OK) return rc;
    rc = ts_vol(table, n_blocks, sorted_block, sorted_index, tsdf, weight, v);
    if (rc != ENSLAM_OK) return rc;
    if (!workspace || !counts) return ENSLAM_EINVAL;
    const TsWork w = ts_carve(workspace, n_blocks > 0 ? n_blocks : 1);
    hipStream_t s = (hipStream_t)stream;
    if (n_blocks > 0) ts_count_kernel<<<n_blocks, TS_THREADS, 0, s>>>(v, t, w);
    ts_scan_kernel<<<1, TS_SCAN_THREADS, 0, s>>>(w, n_blocks, counts);
    return hipGetLastError() == hipSuccess ? ENSLAM_OK : ENSLAM_ELAUNCH;
}

int enslam_tsdf_mesh_emit(const int32_t* table, const int32_t* unit_lo_host, const int32_t* nu_host, int32_t n_blocks,
                          const int32_t* sorted_block, const int32_t* sorted_index, const float* tsdf,
                          const float* weight, const float* vcolor, double voxel_length, void* workspace, int32_t n_verts,
                          int32_t n_faces, double* verts, int32_t* faces, uint8_t* colors, void* stream) {
    TsTable t;
    TsVol v;
    int rc = ts_table(unit_lo_host, nu_host, t);
    if (rc != ENSLAM_OK) return rc;
    if (!unit_lo_host) return ENSLAM_EINVAL;
    rc = ts_vol(table, n_blocks, sorted_block, sorted_index, tsdf, weight, v);
    if (rc != ENSLAM_OK) return rc;
    if (!workspace || n_verts < 0 || n_faces < 0 || (n_verts > 0 && !verts) || (n_faces > 0 && !faces) || (colors && !vcolor) ||
        !ts_finite(voxel_length) || voxel_length <= 0.0)
        return ENSLAM_EINVAL;
    if (n_verts == 0 || n_blocks == 0) return ENSLAM_OK;    // no crossing edge: no vertex and no triangle
    const TsWork w = ts_carve(workspace, n_blocks);
    hipStream_t s = (hipStream_t)stream;
    ts_verts_kernel<<<n_blocks, TS_THREADS, 0, s>>>(v, t, w, vcolor, voxel_length, n_verts, verts, colors);
    if (n_faces > 0) ts_faces_kernel<<<n_blocks, TS_THREADS, 0, s>>>(v, t, w, n_faces, faces);
    return hipGetLastError() == hipSuccess ? ENSLAM_OK : ENSLAM_ELAUNCH;
}

}  // extern "C"
