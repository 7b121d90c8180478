// Marching cubes on a float32 lattice [nx, ny, nz] (z fastest): the iso-surface step of Mesher.get_mesh
// (Mesher.py:495-520, skimage.measure.marching_cubes) as a count / scan / emit pipeline.
//
//   count  one thread per lattice point p: its vertex mask (bit a: the +a edge it owns crosses the level) and the case
//          of the cell whose lowest corner it is; per 256-point tile, the vertex and triangle totals (ballots, no atomics)
//   scan   one block: exclusive offsets of the tile totals in place, and the two grand totals
//   verts  per point: the first output index of its vertices (kept for the face pass) and the vertices themselves
//   faces  per cell: the case table's triangles, each corner looked up as (owner point's first index + rank of the axis)
//
// Every output position is a prefix sum of counts in lattice order, so the result is deterministic to the bit.
// Case table and conventions: mc_tables.hpp (tools/gen_mc_tables.py).
#include "../../include/enslam_hip.h"
#include "common.hpp"
#include "mc_tables.hpp"

namespace {

constexpr int MC_TILE = 256;                            // points per tile = threads per block
constexpr int MC_MAX_GRID = 2048;                       // grid-stride cap
constexpr int MC_SCAN_THREADS = 1024;
constexpr int64_t MC_MAX_POINTS = 512LL * 512 * 512;    // counts stay in int32: <= 3 * 512^3 vertices, <= 5 * 511^3 faces

struct McDims {
    int32_t nx, ny, nz;
    int64_t n, sx, sy;                                  // points, strides of x and y (z stride 1)
};

struct McWork {
    uint8_t* vmask;    // [n]  bits 0-2: the +x / +y / +z edge of the point carries a vertex
    uint8_t* cases;    // [n]  case of the cell at the point (0 on the upper faces, where no cell starts)
    int32_t* vbase;    // [n]  first vertex index of the point (written where vmask != 0)
    int32_t* tile_v;   // [tiles]  vertex count per tile, then its exclusive offset
    int32_t* tile_f;   // [tiles]  triangle count per tile, then its exclusive offset
};

int64_t mc_align(int64_t b) { return (b + 255) & ~(int64_t)255; }
int64_t mc_tiles(int64_t n) { return (n + MC_TILE - 1) / MC_TILE; }

McWork mc_carve(void* ws, int64_t n) {
    char* b = (char*)ws;
    const int64_t t = mc_tiles(n);
    McWork w;
    w.vmask = (uint8_t*)b;  b += mc_align(n);
    w.cases = (uint8_t*)b;  b += mc_align(n);
    w.vbase = (int32_t*)b;  b += mc_align(4 * n);
    w.tile_v = (int32_t*)b; b += mc_align(4 * t);
    w.tile_f = (int32_t*)b;
    return w;
}

int64_t mc_workspace_bytes(int64_t n) { return 2 * mc_align(n) + mc_align(4 * n) + 2 * mc_align(4 * mc_tiles(n)); }

int mc_grid(int64_t tiles) { return (int)(tiles < MC_MAX_GRID ? tiles : MC_MAX_GRID); }

// number of lanes below this one whose bit in m is set (v_mbcnt_lo / v_mbcnt_hi)
ENS_DEV int lanes_below(uint64_t m) {
    return (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

// Exclusive prefix over the block (in lattice order) of a per-thread count 0..7 given by its three bits, plus the block's
// total.  `red` holds 4 ints per call site; the caller separates reuses with a barrier.
ENS_DEV int block_prefix3(int c, int* red, int& total) {
    const uint64_t b0 = __ballot(c & 1), b1 = __ballot(c & 2), b2 = __ballot(c & 4);
    const int lane_pre = lanes_below(b0) + 2 * lanes_below(b1) + 4 * lanes_below(b2);
    const int wave_tot = __popcll(b0) + 2 * __popcll(b1) + 4 * __popcll(b2);
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) red[w] = wave_tot;
    __syncthreads();
    int off = 0;
    total = 0;
#pragma unroll
    for (int k = 0; k < MC_TILE / 64; ++k) {
        off += k < w ? red[k] : 0;
        total += red[k];
    }
    return off + lane_pre;
}

ENS_DEV void mc_coords(int64_t p, const McDims& d, int& ix, int& iy, int& iz) {
    iz = (int)(p % d.nz);
    const int64_t r = p / d.nz;
    iy = (int)(r % d.ny);
    ix = (int)(r / d.ny);
}

__global__ __launch_bounds__(MC_TILE) void mc_count_kernel(const float* __restrict__ vol, McDims d, double level, McWork w,
                                                           int64_t tiles) {
    __shared__ int red[2][MC_TILE / 64];
    for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const int64_t p = t * MC_TILE + threadIdx.x;
        int vm = 0, nt = 0;
        if (p < d.n) {
            int ix, iy, iz;
            mc_coords(p, d, ix, iy, iz);
            const bool hx = ix + 1 < d.nx, hy = iy + 1 < d.ny, hz = iz + 1 < d.nz;
            const bool o0 = (double)vol[p] > level;
            const bool ox = hx && (double)vol[p + d.sx] > level;
            const bool oy = hy && (double)vol[p + d.sy] > level;
            const bool oz = hz && (double)vol[p + 1] > level;
            vm = (hx && ox != o0 ? 1 : 0) | (hy && oy != o0 ? 2 : 0) | (hz && oz != o0 ? 4 : 0);
            int cs = 0;
            if (hx && hy && hz) {
                const bool oxy = (double)vol[p + d.sx + d.sy] > level;
                const bool oxz = (double)vol[p + d.sx + 1] > level;
                const bool oyz = (double)vol[p + d.sy + 1] > level;
                const bool oxyz = (double)vol[p + d.sx + d.sy + 1] > level;
                cs = (int)o0 | (int)ox << 1 | (int)oy << 2 | (int)oxy << 3 | (int)oz << 4 | (int)oxz << 5 | (int)oyz << 6 |
                     (int)oxyz << 7;
                nt = mc_tri_count[cs];
            }
            w.vmask[p] = (uint8_t)vm;
            w.cases[p] = (uint8_t)cs;
        }
        int tv, tf;
        block_prefix3((vm & 1) + ((vm >> 1) & 1) + ((vm >> 2) & 1), red[0], tv);
        block_prefix3(nt, red[1], tf);
        if (threadIdx.x == 0) {
            w.tile_v[t] = tv;
            w.tile_f[t] = tf;
        }
        __syncthreads();
    }
}

// One block: tile counts -> exclusive offsets (in place); counts[0..1] = total vertices, total triangles.
__global__ __launch_bounds__(MC_SCAN_THREADS) void mc_scan_kernel(McWork w, int64_t tiles, int32_t* __restrict__ counts) {
    __shared__ int sv[MC_SCAN_THREADS], sf[MC_SCAN_THREADS];
    const int64_t chunk = (tiles + MC_SCAN_THREADS - 1) / MC_SCAN_THREADS;
    const int64_t lo = threadIdx.x * chunk;
    const int64_t hi = lo + chunk < tiles ? lo + chunk : tiles;
    int v = 0, f = 0;
    for (int64_t i = lo; i < hi; ++i) {
        v += w.tile_v[i];
        f += w.tile_f[i];
    }
    sv[threadIdx.x] = v;
    sf[threadIdx.x] = f;
    __syncthreads();
    for (int o = 1; o < MC_SCAN_THREADS; o <<= 1) {       // inclusive Hillis-Steele scan
        const int av = threadIdx.x >= o ? sv[threadIdx.x - o] : 0;
        const int af = threadIdx.x >= o ? sf[threadIdx.x - o] : 0;
        __syncthreads();
        sv[threadIdx.x] += av;
        sf[threadIdx.x] += af;
        __syncthreads();
    }
    int ov = sv[threadIdx.x] - v, of = sf[threadIdx.x] - f;
    for (int64_t i = lo; i < hi; ++i) {
        const int cv = w.tile_v[i], cf = w.tile_f[i];
        w.tile_v[i] = ov;
        w.tile_f[i] = of;
        ov += cv;
        of += cf;
    }
    if (threadIdx.x == MC_SCAN_THREADS - 1) {
        counts[0] = sv[threadIdx.x];
        counts[1] = sf[threadIdx.x];
    }
}

struct McGeom {
    double origin[3], spacing[3];
};

// Vertex of the +a edge of point (ix, iy, iz): origin + (index + t) * spacing with t = (level - v0) / (v1 - v0), float64
// (what the reference computes after skimage: verts + [x0, y0, z0]); -ffp-contract=off keeps the order.
__global__ __launch_bounds__(MC_TILE) void mc_verts_kernel(const float* __restrict__ vol, McDims d, double level, McGeom g,
                                                           McWork w, int64_t tiles, double* __restrict__ verts) {
    __shared__ int red[MC_TILE / 64];
    for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const int64_t p = t * MC_TILE + threadIdx.x;
        const int vm = p < d.n ? w.vmask[p] : 0;
        int unused;
        const int base = w.tile_v[t] + block_prefix3((vm & 1) + ((vm >> 1) & 1) + ((vm >> 2) & 1), red, unused);
        if (vm) {
            w.vbase[p] = base;
            int ix, iy, iz;
            mc_coords(p, d, ix, iy, iz);
            const double idx[3] = {(double)ix, (double)iy, (double)iz};
            const int64_t stride[3] = {d.sx, d.sy, 1};
            const double v0 = (double)vol[p];
            int64_t k = base;
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                if (!(vm & (1 << a))) continue;
                const double v1 = (double)vol[p + stride[a]];
                const double tt = (level - v0) / (v1 - v0);
                double* out = verts + 3 * k;
#pragma unroll
                for (int c = 0; c < 3; ++c) out[c] = g.origin[c] + (idx[c] + (c == a ? tt : 0.0)) * g.spacing[c];
                ++k;
            }
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(MC_TILE) void mc_faces_kernel(McDims d, McWork w, int64_t tiles, int32_t* __restrict__ faces) {
    __shared__ int red[MC_TILE / 64];
    for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const int64_t p = t * MC_TILE + threadIdx.x;
        const int cs = p < d.n ? w.cases[p] : 0;
        const int nt = mc_tri_count[cs];
        int unused;
        const int64_t base = (int64_t)w.tile_f[t] + block_prefix3(nt, red, unused);
        for (int k = 0; k < nt; ++k) {
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const int e = mc_tri_edges[cs][3 * k + j];
                const int c0 = mc_edge_c0[e], a = e >> 2;
                const int64_t q = p + (c0 & 1) * d.sx + ((c0 >> 1) & 1) * d.sy + ((c0 >> 2) & 1);
                faces[3 * (base + k) + j] = w.vbase[q] + __popc(w.vmask[q] & ((1 << a) - 1));
            }
        }
        __syncthreads();
    }
}

int mc_dims(int32_t nx, int32_t ny, int32_t nz, McDims& d) {
    if (nx < 2 || ny < 2 || nz < 2) return ENSLAM_EINVAL;
    d.nx = nx;
    d.ny = ny;
    d.nz = nz;
    d.n = (int64_t)nx * ny * nz;
    d.sy = nz;
    d.sx = (int64_t)ny * nz;
    return d.n > MC_MAX_POINTS ? ENSLAM_EUNSUPPORTED : ENSLAM_OK;
}

bool mc_finite(double x) { return x == x && x - x == 0.0; }

}  // namespace

extern "C" {

int enslam_marching_cubes_workspace(int32_t nx, int32_t ny, int32_t nz, int64_t* bytes_host) {
    McDims d;
    const int rc = mc_dims(nx, ny, nz, d);
    if (rc != ENSLAM_OK) return rc;
    if (!bytes_host) return ENSLAM_EINVAL;
    *bytes_host = mc_workspace_bytes(d.n);
    return ENSLAM_OK;
}

int enslam_marching_cubes_count(const float* volume, int32_t nx, int32_t ny, int32_t nz, double level, void* workspace,
                                int32_t* counts, void* stream) {
    McDims d;
    const int rc = mc_dims(nx, ny, nz, d);
    if (rc != ENSLAM_OK) return rc;
    if (!volume || !workspace || !counts || !mc_finite(level)) return ENSLAM_EINVAL;
    const McWork w = mc_carve(workspace, d.n);
    const int64_t tiles = mc_tiles(d.n);
    hipStream_t s = (hipStream_t)stream;
    mc_count_kernel<<<mc_grid(tiles), MC_TILE, 0, s>>>(volume, d, level, w, tiles);
    mc_scan_kernel<<<1, MC_SCAN_THREADS, 0, s>>>(w, tiles, counts);
    return hipGetLastError() == hipSuccess ? ENSLAM_OK : ENSLAM_ELAUNCH;
}

int enslam_marching_cubes_emit(const float* volume, int32_t nx, int32_t ny, int32_t nz, double level,
                               const double* origin_host, const double* spacing_host, void* workspace, int32_t n_verts,
                               int32_t n_faces, double* verts, int32_t* faces, void* stream) {
    McDims d;
    const int rc = mc_dims(nx, ny, nz, d);
    if (rc != ENSLAM_OK) return rc;
    if (!volume || !workspace || !origin_host || !spacing_host || !mc_finite(level) || n_verts < 0 || n_faces < 0 ||
        (n_verts > 0 && !verts) || (n_faces > 0 && !faces))
        return ENSLAM_EINVAL;
    McGeom g;
    for (int c = 0; c < 3; ++c) {
        if (!mc_finite(origin_host[c]) || !mc_finite(spacing_host[c])) return ENSLAM_EINVAL;
        g.origin[c] = origin_host[c];
        g.spacing[c] = spacing_host[c];
    }
    if (n_verts == 0) return ENSLAM_OK;                 // no crossing edge: no vertex and no triangle
    const McWork w = mc_carve(workspace, d.n);
    const int64_t tiles = mc_tiles(d.n);
    hipStream_t s = (hipStream_t)stream;
    mc_verts_kernel<<<mc_grid(tiles), MC_TILE, 0, s>>>(volume, d, level, g, w, tiles, verts);
    if (n_faces > 0) mc_faces_kernel<<<mc_grid(tiles), MC_TILE, 0, s>>>(d, w, tiles, faces);
    return hipGetLastError() == hipSuccess ? ENSLAM_OK : ENSLAM_ELAUNCH;
}

}  // extern "C"
