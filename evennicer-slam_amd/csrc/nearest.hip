// Exact nearest neighbour in float64 (the cKDTree queries of the reference's src/tools/eval_recon.py:24-43 and the
// correspondence search of its ICP alignment): for every query the nearest reference point, its distance
// sqrt((dx*dx + dy*dy) + dz*dz) evaluated in that order (unfused: -ffp-contract=off), ties to the smallest index.
//
// build  (once per reference set; every launch is independent of the data)
//   bbox     per axis the smallest and largest coordinate: wave reduction, then integer maxima on order-preserving keys
//   plan     one thread: the cell edge h and the grid dimensions -- the smallest h (bisection) with at most `cap` cells,
//            cap = min(2 N, 2^24).  A flat or zero-size box gives dimension 1 on that axis.
//   count    per point: its cell, one integer add on the cell's counter
//   scan     one block: inclusive prefix sum of the counters, shifted: cursor[c] = first slot of cell c
//   scatter  per point: slot = cursor[cell]++; coordinates and the original index go to the slot.  Afterwards cursor[c] is
//            the END of cell c, so cell c is [c ? cursor[c-1] : 0, cursor[c]).  The order inside a cell depends on the
//            schedule; the result of a query does not (the index tie-break below).
// query
//   shells   one thread per query walks the Chebyshev shells r = 0 .. max_rings-1 of cells around its own cell (a query
//            outside the box starts from the clamped cell).  After shell r every unvisited point lies in a cell with
//            |cell - own| >= r + 1 on some axis, so it is at least  lb(r) = h * min over axes and sides that still have
//            unvisited cells of (own + r + 1 - t) and (t - (own - r)),  t = the query's coordinate in cells clamped into the
//            grid (clamping only lowers the bound: valid for queries outside the box).  The thread stops when its best
//            distance is <= lb(r) less a slack of 1e-6 cells (the cell coordinates carry a rounding error below 1e-8 cells:
//            4e-16 relative at most 2^24 cells), or when lb(r) >= max_dist, or when no unvisited cell is left.
//   tail     queries still open after max_rings shells are appended to a list; a workgroup per 256 of them streams the
//            whole reference through LDS in float64.  max_rings = 0: every query takes this route and no grid is needed.
//
// Ties.  Candidates are compared on the squared distance; two squared distances one rounding apart can share their square
// root, and the contract breaks ties on the DISTANCE.  A candidate within 1e-15 relative of the best is therefore compared
// on the square roots, equal roots on the index (nn_consider): the result is the smallest index among the points at the
// smallest distance, in whatever order the points are visited.
#include "../../include/enslam_hip.h"
#include "common.hpp"

namespace {

constexpr int NN_BLOCK = 256;
constexpr int NN_MAX_GRID = 4096;                       // grid-stride cap of the per-point kernels
constexpr int NN_SCAN_THREADS = 1024;
constexpr int NN_TILE = 512;                            // reference points per LDS tile of the tail kernel (12 KB)
constexpr int64_t NN_MAX_POINTS = (int64_t)1 << 26;
constexpr int64_t NN_MAX_CELLS = (int64_t)1 << 24;
constexpr double NN_SLACK_CELLS = 1e-6;

struct NnGrid {                     // written by the plan kernel
    double lo[3];
    double inv_h, h;
    int32_t dim[3];
    int32_t n_cells;
};

struct NnScalars {                  // zeroed at the start of a build
    uint64_t key_hi[3];             // largest key of  x
    uint64_t key_lo[3];             // largest key of -x
    NnGrid grid;
};

struct NnWork {
    NnScalars* sc;
    uint32_t* cursor;               // [cap]
    double* sorted;                 // [N,3]
    int32_t* sorted_idx;            // [N]
    int64_t cap, zero_bytes;
};

int64_t nn_align(int64_t b) { return (b + 255) & ~(int64_t)255; }
int64_t nn_cap(int64_t N) { return 2 * N < NN_MAX_CELLS ? (2 * N < 8 ? 8 : 2 * N) : NN_MAX_CELLS; }

int64_t nn_carve(void* ws, int64_t N, NnWork& w) {
    char* b = (char*)ws;
    int64_t o = 0;
    w.cap = nn_cap(N);
    w.sc = (NnScalars*)(b + o);         o += 256;
    w.cursor = (uint32_t*)(b + o);      o += nn_align(4 * w.cap);
    w.zero_bytes = o;
    w.sorted = (double*)(b + o);        o += nn_align(24 * N);
    w.sorted_idx = (int32_t*)(b + o);   o += nn_align(4 * N);
    return o;
}
static_assert(sizeof(NnScalars) <= 256, "the scalars have 256 bytes of the workspace");

// query scratch: the open count (int32, 256 bytes), then the open list int32 [M]
int64_t nn_query_bytes(int64_t M) { return 256 + nn_align(4 * (M > 0 ? M : 1)); }

int nn_grid_size(int64_t n) {
    const int64_t t = (n + NN_BLOCK - 1) / NN_BLOCK;
    return (int)(t < 1 ? 1 : (t < NN_MAX_GRID ? t : NN_MAX_GRID));
}

// order-preserving map of a float64 onto uint64; key 0 is below every number
ENS_DEV uint64_t nn_key(double x) {
    const uint64_t b = __builtin_bit_cast(uint64_t, x);
    return b >> 63 ? ~b : b | ((uint64_t)1 << 63);
}
ENS_DEV double nn_unkey(uint64_t k) { return __builtin_bit_cast(double, k >> 63 ? k & ~((uint64_t)1 << 63) : ~k); }

ENS_DEV uint64_t nn_wave_max(uint64_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const uint64_t u = (uint64_t)__shfl_xor((unsigned long long)v, o);
        v = u > v ? u : v;
    }
    return v;
}

__global__ __launch_bounds__(NN_BLOCK) void nn_bbox_kernel(const double* __restrict__ ref, int64_t N, NnScalars* sc) {
    uint64_t hi[3] = {0, 0, 0}, lo[3] = {0, 0, 0};
    for (int64_t i = (int64_t)blockIdx.x * NN_BLOCK + threadIdx.x; i < N; i += (int64_t)gridDim.x * NN_BLOCK) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const double x = ref[3 * i + a];
            const uint64_t kh = nn_key(x), kl = nn_key(-x);
            hi[a] = kh > hi[a] ? kh : hi[a];
            lo[a] = kl > lo[a] ? kl : lo[a];
        }
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        hi[a] = nn_wave_max(hi[a]);
        lo[a] = nn_wave_max(lo[a]);
    }
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            if (hi[a]) atomicMax((unsigned long long*)&sc->key_hi[a], (unsigned long long)hi[a]);
            if (lo[a]) atomicMax((unsigned long long*)&sc->key_lo[a], (unsigned long long)lo[a]);
        }
    }
}

// cells of the axes for edge h: floor(e / h) + 1 each, saturated so that the product cannot overflow
ENS_DEV int64_t nn_cells_for(const double e[3], double h, int32_t dim[3]) {
    int64_t prod = 1;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double c = floor(e[a] / h) + 1.0;
        const int64_t d = c < (double)(NN_MAX_CELLS + 1) ? (int64_t)c : NN_MAX_CELLS + 1;
        dim[a] = (int32_t)d;
        prod = prod * d > NN_MAX_CELLS + 1 ? NN_MAX_CELLS + 1 : prod * d;
    }
    return prod;
}

__global__ void nn_plan_kernel(NnScalars* sc, int64_t cap) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    NnGrid g;
    double e[3], emax = 0.0;
    for (int a = 0; a < 3; ++a) {
        g.lo[a] = -nn_unkey(sc->key_lo[a]);
        e[a] = nn_unkey(sc->key_hi[a]) - g.lo[a];
        if (!(e[a] >= 0.0) || !(e[a] < __builtin_huge_val())) e[a] = 0.0;       // not reached with finite input
        emax = e[a] > emax ? e[a] : emax;
    }
    double h = 1.0;
    if (emax > 0.0) {
        // h = emax gives at most 2 cells per axis (8 <= cap); bisect towards the smallest h that still fits
        double fits = emax, small = 0.0;
        for (int it = 0; it < 64; ++it) {
            const double mid = 0.5 * (fits + small);
            int32_t d[3];
            if (mid > 0.0 && nn_cells_for(e, mid, d) <= cap) fits = mid; else small = mid;
        }
        h = fits;
    }
    const int64_t n = nn_cells_for(e, h, g.dim);
    g.h = h;
    g.inv_h = 1.0 / h;
    g.n_cells = (int32_t)n;
    sc->grid = g;
}

// the coordinate in cells and the cell (clamped into the grid) on one axis
ENS_DEV int nn_axis_cell(double x, double lo, double inv_h, int dim, double& t) {
    t = (x - lo) * inv_h;
    const double f = floor(t);
    return f >= (double)(dim - 1) ? dim - 1 : (f > 0.0 ? (int)f : 0);          // a NaN lands in cell 0
}

ENS_DEV int64_t nn_cell_of(const NnGrid& g, double x, double y, double z) {
    double t;
    const int cx = nn_axis_cell(x, g.lo[0], g.inv_h, g.dim[0], t);
    const int cy = nn_axis_cell(y, g.lo[1], g.inv_h, g.dim[1], t);
    const int cz = nn_axis_cell(z, g.lo[2], g.inv_h, g.dim[2], t);
    return ((int64_t)cz * g.dim[1] + cy) * g.dim[0] + cx;
}

__global__ __launch_bounds__(NN_BLOCK) void nn_count_kernel(const double* __restrict__ ref, int64_t N, NnWork w) {
    const NnGrid g = w.sc->grid;
    for (int64_t i = (int64_t)blockIdx.x * NN_BLOCK + threadIdx.x; i < N; i += (int64_t)gridDim.x * NN_BLOCK) {
        const int64_t c = nn_cell_of(g, ref[3 * i], ref[3 * i + 1], ref[3 * i + 2]);
        if (c < w.cap) atomicAdd(w.cursor + c, 1u);                             // c < n_cells <= cap: the test guards the store
    }
}

// one block: counts -> first slots (exclusive prefix sum in place)
__global__ __launch_bounds__(NN_SCAN_THREADS) void nn_scan_kernel(NnWork w) {
    __shared__ uint32_t sm[NN_SCAN_THREADS];
    int64_t n = w.sc->grid.n_cells;
    n = n < w.cap ? n : w.cap;
    const int64_t chunk = (n + NN_SCAN_THREADS - 1) / NN_SCAN_THREADS;
    const int64_t lo = threadIdx.x * chunk;
    const int64_t hi = lo + chunk < n ? lo + chunk : n;
    uint32_t c = 0;
    for (int64_t i = lo; i < hi; ++i) c += w.cursor[i];
    sm[threadIdx.x] = c;
    __syncthreads();
    for (int o = 1; o < NN_SCAN_THREADS; o <<= 1) {                             // inclusive Hillis-Steele scan
        const uint32_t a = threadIdx.x >= o ? sm[threadIdx.x - o] : 0;
        __syncthreads();
        sm[threadIdx.x] += a;
        __syncthreads();
    }
    uint32_t off = sm[threadIdx.x] - c;
    for (int64_t i = lo; i < hi; ++i) {
        const uint32_t k = w.cursor[i];
        w.cursor[i] = off;
        off += k;
    }
}

__global__ __launch_bounds__(NN_BLOCK) void nn_scatter_kernel(const double* __restrict__ ref, int64_t N, NnWork w) {
    const NnGrid g = w.sc->grid;
    for (int64_t i = (int64_t)blockIdx.x * NN_BLOCK + threadIdx.x; i < N; i += (int64_t)gridDim.x * NN_BLOCK) {
        const double x = ref[3 * i], y = ref[3 * i + 1], z = ref[3 * i + 2];
        const int64_t c = nn_cell_of(g, x, y, z);
        if (c >= w.cap) continue;
        const int64_t s = atomicAdd(w.cursor + c, 1u);
        if (s < N) {                                    // the counts sum to N: the test guards the store
            w.sorted[3 * s] = x;
            w.sorted[3 * s + 1] = y;
            w.sorted[3 * s + 2] = z;
            w.sorted_idx[s] = (int32_t)i;
        }
    }
}

// ---- the comparison -------------------------------------------------------------------------------------------------------
struct NnBest {
    double d2, lo, hi;              // the smallest squared distance so far and d2 * (1 -+ 1e-15)
    int32_t idx;
};
ENS_DEV NnBest nn_best_init() {
    const double inf = __builtin_huge_val();
    return NnBest{inf, inf, inf, 0x7fffffff};
}
ENS_DEV void nn_consider(NnBest& b, double qx, double qy, double qz, double rx, double ry, double rz, int32_t idx) {
    const double dx = qx - rx, dy = qy - ry, dz = qz - rz;
    const double d2 = (dx * dx + dy * dy) + dz * dz;
    if (!(d2 <= b.hi)) return;
    if (d2 < b.lo) {
        b.idx = idx;
    } else {                                            // within rounding of the best: the square roots decide, then the index
        const double s = sqrt(d2), sb = sqrt(b.d2);
        if (s < sb || (s == sb && idx < b.idx)) b.idx = idx;
        if (!(d2 < b.d2)) return;
    }
    b.d2 = d2;
    b.lo = d2 * (1.0 - 1e-15);
    b.hi = d2 * (1.0 + 1e-15);
}

ENS_DEV void nn_store(const NnBest& b, double max_dist, double* __restrict__ dist, int32_t* __restrict__ idx, int64_t m) {
    const double d = sqrt(b.d2);
    const bool ok = b.idx != 0x7fffffff && d < max_dist;
    dist[m] = ok ? d : __builtin_huge_val();
    idx[m] = ok ? b.idx : -1;
}

// ---- shells ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NN_BLOCK) void nn_shell_kernel(const double* __restrict__ query, int64_t M, NnWork w, int64_t N,
                                                            double max_dist, int max_rings, double* __restrict__ dist,
                                                            int32_t* __restrict__ idx, int32_t* open_count,
                                                            int32_t* __restrict__ open_list) {
    const NnGrid g = w.sc->grid;
    const int64_t m = (int64_t)blockIdx.x * NN_BLOCK + threadIdx.x;
    if (m >= M) return;
    const double qx = query[3 * m], qy = query[3 * m + 1], qz = query[3 * m + 2];
    const double q[3] = {qx, qy, qz};
    int c[3];
    double t[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        c[a] = nn_axis_cell(q[a], g.lo[a], g.inv_h, g.dim[a], t[a]);
        t[a] = t[a] > 0.0 ? (t[a] < (double)g.dim[a] ? t[a] : (double)g.dim[a]) : 0.0;       // clamped into the grid
    }
    NnBest best = nn_best_init();
    bool done = false;
    for (int r = 0; r < max_rings && !done; ++r) {
        const int z0 = c[2] - r < 0 ? 0 : c[2] - r, z1 = c[2] + r >= g.dim[2] ? g.dim[2] - 1 : c[2] + r;
        const int y0 = c[1] - r < 0 ? 0 : c[1] - r, y1 = c[1] + r >= g.dim[1] ? g.dim[1] - 1 : c[1] + r;
        const int x0 = c[0] - r < 0 ? 0 : c[0] - r, x1 = c[0] + r >= g.dim[0] ? g.dim[0] - 1 : c[0] + r;
        for (int z = z0; z <= z1; ++z) {
            for (int y = y0; y <= y1; ++y) {
                const bool face = z == c[2] - r || z == c[2] + r || y == c[1] - r || y == c[1] + r;
                // a row on a face of the shell is one run of cells; an inner row has the two end cells (one for r = 0)
                const int runs = face || r == 0 ? 1 : 2;
                for (int k = 0; k < runs; ++k) {
                    int xa, xb;
                    if (face) { xa = x0; xb = x1; }
                    else { xa = xb = k == 0 ? c[0] - r : c[0] + r; }
                    if (xa < 0 || xb >= g.dim[0]) continue;
                    const int64_t row = ((int64_t)z * g.dim[1] + y) * g.dim[0];
                    const int64_t ca = row + xa, cb = row + xb;
                    if (cb >= w.cap) continue;          // cb < n_cells <= cap: the test guards the loads
                    int64_t s = ca ? w.cursor[ca - 1] : 0, e = w.cursor[cb];
                    e = e < N ? e : N;
                    for (; s < e; ++s)
                        nn_consider(best, qx, qy, qz, w.sorted[3 * s], w.sorted[3 * s + 1], w.sorted[3 * s + 2], w.sorted_idx[s]);
                }
            }
        }
        // the lower bound of everything outside the shells visited so far
        double lb = __builtin_huge_val();
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            if (c[a] + r + 1 <= g.dim[a] - 1) lb = fmin(lb, (double)(c[a] + r + 1) - t[a]);
            if (c[a] - r - 1 >= 0) lb = fmin(lb, t[a] - (double)(c[a] - r));
        }
        if (lb == __builtin_huge_val()) {
            done = true;                                // the shells covered the grid
        } else {
            lb = (lb - NN_SLACK_CELLS) * g.h;
            done = lb > 0.0 && (best.d2 <= lb * lb || lb >= max_dist);
        }
    }
    if (done) {
        nn_store(best, max_dist, dist, idx, m);
    } else {
        const int slot = atomicAdd(open_count, 1);
        if (slot < M) open_list[slot] = (int32_t)m;
    }
}

// ---- brute force ----------------------------------------------------------------------------------------------------------
// open_list == nullptr: every query.  A workgroup per 256 listed queries; the reference goes through LDS in its own order,
// so the first minimum needs no tie-break beyond nn_consider's.
__global__ __launch_bounds__(NN_BLOCK) void nn_tail_kernel(const double* __restrict__ ref, int64_t N,
                                                           const double* __restrict__ query, int64_t M, double max_dist,
                                                           const int32_t* open_count, const int32_t* __restrict__ open_list,
                                                           double* __restrict__ dist, int32_t* __restrict__ idx,
                                                           int32_t* __restrict__ n_tail) {
    __shared__ double tile[3 * NN_TILE];
    int64_t count = open_list ? (int64_t)*open_count : M;
    count = count < M ? count : M;
    if (n_tail && blockIdx.x == 0 && threadIdx.x == 0) *n_tail = (int32_t)count;
    const int64_t first = (int64_t)blockIdx.x * NN_BLOCK;
    if (first >= count) return;                         // uniform over the workgroup
    const int64_t e = first + threadIdx.x;
    const bool live = e < count;
    int64_t m = live ? (open_list ? (int64_t)open_list[e] : e) : 0;
    if (m < 0 || m >= M) m = 0;
    const double qx = query[3 * m], qy = query[3 * m + 1], qz = query[3 * m + 2];
    NnBest best = nn_best_init();
    for (int64_t base = 0; base < N; base += NN_TILE) {
        const int n = (int)(N - base < NN_TILE ? N - base : NN_TILE);
        __syncthreads();
        for (int i = threadIdx.x; i < 3 * n; i += NN_BLOCK) tile[i] = ref[3 * base + i];
        __syncthreads();
        if (live) {
            for (int i = 0; i < n; ++i) nn_consider(best, qx, qy, qz, tile[3 * i], tile[3 * i + 1], tile[3 * i + 2], (int32_t)(base + i));
        }
    }
    if (live) nn_store(best, max_dist, dist, idx, m);
}

int nn_sizes(int64_t n_ref, int64_t n_query) {
    if (n_ref < 0 || n_query < 0 || n_ref > NN_MAX_POINTS || n_query > NN_MAX_POINTS) return ENSLAM_EINVAL;
    return ENSLAM_OK;
}

}  // namespace

extern "C" {

int enslam_nn_workspace(int64_t n_ref, int64_t n_query, int64_t* grid_bytes_host, int64_t* query_bytes_host) {
    if (nn_sizes(n_ref, n_query) != ENSLAM_OK) return ENSLAM_EINVAL;
    NnWork w;
    if (grid_bytes_host) *grid_bytes_host = nn_carve(nullptr, n_ref, w);
    if (query_bytes_host) *query_bytes_host = nn_query_bytes(n_query);
    return ENSLAM_OK;
}

int enslam_nn_build(const double* ref, int64_t n_ref, void* grid_workspace, void* stream) {
    if (nn_sizes(n_ref, 0) != ENSLAM_OK || n_ref == 0 || !ref || !grid_workspace) return ENSLAM_EINVAL;
    NnWork w;
    nn_carve(grid_workspace, n_ref, w);
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(w.sc, 0, (size_t)w.zero_bytes, s) != hipSuccess) return ENSLAM_ELAUNCH;
    const int grid = nn_grid_size(n_ref);
    nn_bbox_kernel<<<grid, NN_BLOCK, 0, s>>>(ref, n_ref, w.sc);
    nn_plan_kernel<<<1, 64, 0, s>>>(w.sc, w.cap);
    nn_count_kernel<<<grid, NN_BLOCK, 0, s>>>(ref, n_ref, w);
    nn_scan_kernel<<<1, NN_SCAN_THREADS, 0, s>>>(w);
    nn_scatter_kernel<<<grid, NN_BLOCK, 0, s>>>(ref, n_ref, w);
    return hipGetLastError() == hipSuccess ? ENSLAM_OK : ENSLAM_ELAUNCH;
}

int enslam_nn_query(const double* ref, int64_t n_ref, const double* query, int64_t n_query, double max_dist,
                    int32_t max_rings, void* grid_workspace, void* query_workspace, double* dist, int32_t* idx,
                    int32_t* n_tail, void* stream) {
    if (nn_sizes(n_ref, n_query) != ENSLAM_OK || n_ref == 0 || !ref || max_rings < 0 || max_dist != max_dist)
        return ENSLAM_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    if (n_query == 0) {
        if (n_tail && hipMemsetAsync(n_tail, 0, 4, s) != hipSuccess) return ENSLAM_ELAUNCH;
        return ENSLAM_OK;
    }
    if (!query || !dist || !idx || (max_rings > 0 && (!grid_workspace || !query_workspace))) return ENSLAM_EINVAL;
    const unsigned blocks = (unsigned)((n_query + NN_BLOCK - 1) / NN_BLOCK);
    if (max_rings == 0) {
        nn_tail_kernel<<<blocks, NN_BLOCK, 0, s>>>(ref, n_ref, query, n_query, max_dist, nullptr, nullptr, dist, idx, n_tail);
        return hipGetLastError() == hipSuccess ? ENSLAM_OK : ENSLAM_ELAUNCH;
    }
    NnWork w;
    nn_carve(grid_workspace, n_ref, w);
    int32_t* open_count = (int32_t*)query_workspace;
    int32_t* open_list = (int32_t*)((char*)query_workspace + 256);
    if (hipMemsetAsync(open_count, 0, 4, s) != hipSuccess) return ENSLAM_ELAUNCH;
    nn_shell_kernel<<<blocks, NN_BLOCK, 0, s>>>(query, n_query, w, n_ref, max_dist, max_rings, dist, idx, open_count, open_list);
    nn_tail_kernel<<<blocks, NN_BLOCK, 0, s>>>(ref, n_ref, query, n_query, max_dist, open_count, open_list, dist, idx, n_tail);
    return hipGetLastError() == hipSuccess ? ENSLAM_OK : ENSLAM_ELAUNCH;
}

}  // extern "C"
