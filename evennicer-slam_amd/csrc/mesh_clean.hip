// Mesh cleaning on the device: the tail of Mesher.get_mesh (Mesher.py:469-510; mesher.py face_components / face_areas /
// filter_components / drop_unreferenced): drop faces by a vertex mask, label the edge-connected components of the triangle
// mesh, sum the face areas per component, keep the components above a threshold (or the largest), compact faces and vertices.
//
//   init    per face: index check, mask drop (a face goes iff none of its vertices is kept), parent[f] = f, the face area in
//           float64 (unfused, as numpy computes it) and the largest area of the mesh (integer maximum of the bit patterns)
//   link    per live face and edge: the undirected edge (sorted vertex pair, one 64-bit key) is looked up in an open-addressing
//           table (linear probing, insertion by 64-bit compare-and-swap); an integer minimum on the slot's face word returns a
//           face that registered the edge earlier, and the two faces are united.  Union-find over faces: a root is only ever
//           hooked under a SMALLER root (compare-and-swap on the root's own word), finds halve their path.  Parent words only
//           decrease along a path, so the root of a finished tree is the smallest face index of the component: the label
//           is canonical, whatever the schedule.  Every access to the table and the parents is an agent-scope atomic; a
//           stale parent is still an ancestor and a failed compare-and-swap returns the current word, so no step relies on
//           seeing another workgroup's store in time.  Nothing waits for another thread.
//   labels  per face: label = find(f); the face area joins its component's sum in FIXED POINT (below)
//   areas   per root: the component's area back in float64, the largest of them, the component count
//   best    (largest_only) the smallest label among the components with the largest area
//   keep    per face: keep flag, marks on its vertices, kept faces per 256-face tile (ballots)
//   vcount  per vertex tile: marked vertices;  scan: one block, exclusive offsets of both tile arrays and the totals
//   emit    vertices and faces at (tile offset + rank in tile): original order, no atomics for positions
// The launch count is fixed (no iteration to convergence): a long thin component costs deeper finds, not more launches.
//
// Fixed-point area sums.  Float atomics would make the sums depend on arrival order.  With A the largest face area and e the
// exponent with A in [2^(e-1), 2^e), every area is scaled by 2^(80-e) and truncated to an integer below 2^80, split into two
// 40-bit limbs; each limb has its own 64-bit accumulator per component.  A limb is below 2^40 and a component has at most
// 2^24 faces (MCL_MAX_FACES), so a limb sum stays below 2^64: no carries, no overflow, and integer adds commute, so the sums
// are the same bits in every run.  A face area of at least A * 2^-27 enters exactly (53-bit mantissa), a smaller one loses less
// than A * 2^-80: a component's sum is below the exact sum of its float64 areas by less than 2^24 * 2^-80 A = 2^-56 A --
// closer to the exact sum than np.bincount's running float64 sum.  Non-finite areas count as zero.
#include "../../include/enslam_hip.h"
#include "common.hpp"

namespace {

constexpr int MCL_TILE = 256;                           // faces / vertices per tile = threads per block
constexpr int MCL_MAX_GRID = 2048;                      // grid-stride cap
constexpr int MCL_SCAN_THREADS = 1024;
constexpr int64_t MCL_MAX_FACES = (int64_t)1 << 24;     // limb sums stay below 2^64 (header above)
constexpr int64_t MCL_MAX_VERTS = (int64_t)1 << 26;
constexpr uint64_t MCL_EMPTY = ~(uint64_t)0;            // no edge has this key: vertex indices are below 2^31
constexpr uint32_t MCL_NO_FACE = ~(uint32_t)0;
constexpr int MCL_LIMB = 40;
constexpr uint64_t MCL_LIMB_MASK = ((uint64_t)1 << MCL_LIMB) - 1;

#define MCL_RLX __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT

struct MclScalars {                 // zeroed at the start of every call
    uint64_t amax_bits;             // bit pattern of the largest face area
    uint64_t best_bits;             // bit pattern of the largest component area
    uint32_t best_inv;              // 0x7fffffff - (smallest label with that area)
    int32_t n_comp;                 // components after the mask drop
};

struct MclWork {
    MclScalars* sc;
    uint64_t* acc;      // [F][2]  limb sums of the component whose label is the face index
    uint8_t* vused;     // [V]     vertex referenced by a kept face
    uint64_t* keys;     // [cap]   edge table: sorted vertex pair, MCL_EMPTY = free
    uint32_t* vals;     // [cap]   smallest face that registered the edge so far
    int32_t* parent;    // [F]
    int32_t* labels;    // [F]     -1 for dropped faces
    double* area;       // [F]     face areas; after the `areas` pass, at a root: the component's area
    uint8_t* fkeep;     // [F]     live after the mask drop, then: kept
    int32_t* vremap;    // [V]     new index of a kept vertex
    int32_t* tile_f;    // [tiles(F)]
    int32_t* tile_v;    // [tiles(V)]
    int64_t cap;        // power of two, >= 4 F: at most 3 F distinct edges, load <= 0.75
    int64_t zero_bytes, table_bytes;
};

int64_t mcl_align(int64_t b) { return (b + 255) & ~(int64_t)255; }
__host__ __device__ inline int64_t mcl_tiles(int64_t n) { return (n + MCL_TILE - 1) / MCL_TILE; }
int64_t mcl_cap(int64_t F) {
    int64_t c = 1024;
    while (c < 4 * F) c <<= 1;
    return c;
}

// lays the workspace out; with ws == nullptr only the sizes are meaningful.  Returns the total bytes.
int64_t mcl_carve(void* ws, int64_t V, int64_t F, MclWork& w) {
    char* b = (char*)ws;
    int64_t o = 0;
    w.cap = mcl_cap(F);
    w.sc = (MclScalars*)(b + o);  o += 256;
    w.acc = (uint64_t*)(b + o);   o += mcl_align(16 * F);
    w.vused = (uint8_t*)(b + o);  o += mcl_align(V);
    w.zero_bytes = o;
    w.keys = (uint64_t*)(b + o);  o += mcl_align(8 * w.cap);
    w.vals = (uint32_t*)(b + o);  o += mcl_align(4 * w.cap);
    w.table_bytes = o - w.zero_bytes;
    w.parent = (int32_t*)(b + o); o += mcl_align(4 * F);
    w.labels = (int32_t*)(b + o); o += mcl_align(4 * F);
    w.area = (double*)(b + o);    o += mcl_align(8 * F);
    w.fkeep = (uint8_t*)(b + o);  o += mcl_align(F);
    w.vremap = (int32_t*)(b + o); o += mcl_align(4 * V);
    w.tile_f = (int32_t*)(b + o); o += mcl_align(4 * mcl_tiles(F));
    w.tile_v = (int32_t*)(b + o); o += mcl_align(4 * mcl_tiles(V));
    return o;
}

int mcl_grid(int64_t tiles) { return (int)(tiles < 1 ? 1 : (tiles < MCL_MAX_GRID ? tiles : MCL_MAX_GRID)); }

int mcl_sizes(int32_t n_verts, int32_t n_faces) {
    if (n_verts < 0 || n_faces < 0) return ENSLAM_EINVAL;
    return (n_faces > MCL_MAX_FACES || n_verts > MCL_MAX_VERTS) ? ENSLAM_EUNSUPPORTED : ENSLAM_OK;
}

ENS_DEV int mcl_lanes_below(uint64_t m) {
    return (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

// Exclusive prefix over the block (in thread order) of a per-thread flag, plus the block's total.  `red` holds one int per
// wave; the caller separates reuses with a barrier.
ENS_DEV int mcl_block_prefix(bool flag, int* red, int& total) {
    const uint64_t b = __ballot(flag);
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) red[w] = __popcll(b);
    __syncthreads();
    int off = 0;
    total = 0;
#pragma unroll
    for (int k = 0; k < MCL_TILE / 64; ++k) {
        off += k < w ? red[k] : 0;
        total += red[k];
    }
    return off + mcl_lanes_below(b);
}

ENS_DEV uint64_t mcl_wave_max(uint64_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const uint64_t u = (uint64_t)__shfl_xor((unsigned long long)v, o);
        v = u > v ? u : v;
    }
    return v;
}
ENS_DEV uint64_t mcl_wave_sum(uint64_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += (uint64_t)__shfl_xor((unsigned long long)v, o);
    return v;
}

// ---- union-find over faces ------------------------------------------------------------------------------------------------
ENS_DEV int mcl_find(int32_t* parent, int x) {
    int px = __hip_atomic_load(parent + x, MCL_RLX);
    while (px != x) {
        const int g = __hip_atomic_load(parent + px, MCL_RLX);
        if (g != px) __hip_atomic_store(parent + x, g, MCL_RLX);       // path halving: x is no root and never becomes one again
        x = px;
        px = g;
    }
    return x;
}

ENS_DEV void mcl_unite(int32_t* parent, int a, int b) {
    a = mcl_find(parent, a);
    b = mcl_find(parent, b);
    while (a != b) {
        if (a < b) { const int t = a; a = b; b = t; }                  // hook the larger root under the smaller
        int expect = a;
        if (__hip_atomic_compare_exchange_strong(parent + a, &expect, b, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return;
        a = mcl_find(parent, expect);                                  // a had been hooked meanwhile: go on from its parent
        b = mcl_find(parent, b);
    }
}

ENS_DEV uint64_t mcl_hash(uint64_t k) {                                 // the 64-bit finaliser of MurmurHash3
    k ^= k >> 33;
    k *= 0xff51afd7ed558ccdULL;
    k ^= k >> 33;
    k *= 0xc4ceb9fe1a85ec53ULL;
    k ^= k >> 33;
    return k;
}

// One thread per face.  live == nullptr: every face takes part.
__global__ __launch_bounds__(MCL_TILE) void mcl_link_kernel(const int32_t* __restrict__ faces, int64_t F,
                                                            const uint8_t* __restrict__ live, uint64_t* keys, uint32_t* vals,
                                                            int64_t cap, int32_t* parent) {
    for (int64_t f = (int64_t)blockIdx.x * MCL_TILE + threadIdx.x; f < F; f += (int64_t)gridDim.x * MCL_TILE) {
        if (live && !live[f]) continue;
        const uint32_t v[3] = {(uint32_t)faces[3 * f], (uint32_t)faces[3 * f + 1], (uint32_t)faces[3 * f + 2]};
#pragma unroll
        for (int e = 0; e < 3; ++e) {
            const uint32_t a = v[e], b = v[e == 2 ? 0 : e + 1];
            const uint64_t key = a < b ? ((uint64_t)a << 32 | b) : ((uint64_t)b << 32 | a);
            int64_t s = (int64_t)(mcl_hash(key) & (uint64_t)(cap - 1));
            for (;;) {                                  // ends: the table has more slots than the mesh has edges
                uint64_t cur = __hip_atomic_load(keys + s, MCL_RLX);
                if (cur == MCL_EMPTY) {
                    __hip_atomic_compare_exchange_strong(keys + s, &cur, key, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    if (cur == MCL_EMPTY) break;        // inserted (cur keeps the expected value on success)
                }
                if (cur == key) break;
                s = (s + 1) & (cap - 1);
            }
            const uint32_t other = __hip_atomic_fetch_min(vals + s, (uint32_t)f, MCL_RLX);
            if (other != MCL_NO_FACE && other != (uint32_t)f) mcl_unite(parent, (int)f, (int)other);
        }
    }
}

__global__ __launch_bounds__(MCL_TILE) void mcl_iota_kernel(int32_t* parent, int64_t F) {
    for (int64_t f = (int64_t)blockIdx.x * MCL_TILE + threadIdx.x; f < F; f += (int64_t)gridDim.x * MCL_TILE) parent[f] = (int32_t)f;
}

__global__ __launch_bounds__(MCL_TILE) void mcl_flatten_kernel(int32_t* parent, int64_t F, int32_t* __restrict__ labels) {
    for (int64_t f = (int64_t)blockIdx.x * MCL_TILE + threadIdx.x; f < F; f += (int64_t)gridDim.x * MCL_TILE)
        labels[f] = mcl_find(parent, (int)f);
}

// ---- areas ----------------------------------------------------------------------------------------------------------------
// 0.5 * |(v1 - v0) x (v2 - v0)| as numpy evaluates face_areas: np.cross, then sqrt((x^2 + y^2) + z^2); -ffp-contract=off
ENS_DEV double mcl_face_area(const double* __restrict__ verts, int i0, int i1, int i2) {
    const double* p0 = verts + 3 * (int64_t)i0;
    const double* p1 = verts + 3 * (int64_t)i1;
    const double* p2 = verts + 3 * (int64_t)i2;
    const double ax = p1[0] - p0[0], ay = p1[1] - p0[1], az = p1[2] - p0[2];
    const double bx = p2[0] - p0[0], by = p2[1] - p0[1], bz = p2[2] - p0[2];
    const double cx = ay * bz - az * by, cy = az * bx - ax * bz, cz = ax * by - ay * bx;
    return 0.5 * sqrt((cx * cx + cy * cy) + cz * cz);
}

// exponent e with x in [2^(e-1), 2^e) for the positive finite float64 whose bits are given
ENS_DEV int mcl_exponent(uint64_t bits) {
    const int E = (int)(bits >> 52);
    return E ? E - 1022 : (64 - __clzll((long long)bits)) - 1074;
}

// a * 2^(80 - e) truncated, as two 40-bit limbs (a <= the mesh's largest area, so the value is below 2^80)
ENS_DEV void mcl_limbs(double a, int e, uint64_t& l0, uint64_t& l1) {
    const uint64_t bits = __builtin_bit_cast(uint64_t, a);
    const int E = (int)(bits >> 52);
    const uint64_t frac = bits & (((uint64_t)1 << 52) - 1);
    const uint64_t M = E ? frac | ((uint64_t)1 << 52) : frac;           // a = M * 2^((E ? E : 1) - 1075)
    const int shift = (E ? E : 1) - 1075 + 80 - e;
    if (shift >= MCL_LIMB) {
        l0 = 0;
        l1 = M << (shift - MCL_LIMB);
    } else if (shift >= 0) {
        l0 = (M << shift) & MCL_LIMB_MASK;
        l1 = M >> (MCL_LIMB - shift);
    } else {
        const uint64_t v = shift > -64 ? M >> (-shift) : 0;
        l0 = v & MCL_LIMB_MASK;
        l1 = v >> MCL_LIMB;
    }
}

__global__ __launch_bounds__(MCL_TILE) void mcl_init_kernel(const double* __restrict__ verts, int32_t V,
                                                            const int32_t* __restrict__ faces, int64_t F,
                                                            const uint8_t* __restrict__ vkeep, MclWork w) {
    uint64_t amax = 0;
    for (int64_t f = (int64_t)blockIdx.x * MCL_TILE + threadIdx.x; f < F; f += (int64_t)gridDim.x * MCL_TILE) {
        const int i0 = faces[3 * f], i1 = faces[3 * f + 1], i2 = faces[3 * f + 2];
        bool live = (uint32_t)i0 < (uint32_t)V && (uint32_t)i1 < (uint32_t)V && (uint32_t)i2 < (uint32_t)V;
        if (live && vkeep) live = (vkeep[i0] | vkeep[i1] | vkeep[i2]) != 0;
        double a = 0.0;
        if (live) {
            a = mcl_face_area(verts, i0, i1, i2);
            if (!(a < __builtin_huge_val())) a = 0.0;                   // NaN / inf
        }
        w.parent[f] = (int32_t)f;
        w.fkeep[f] = live ? 1 : 0;
        w.area[f] = a;
        const uint64_t bits = __builtin_bit_cast(uint64_t, a);          // a >= 0: the bit patterns order as the values
        amax = bits > amax ? bits : amax;
    }
    amax = mcl_wave_max(amax);
    if ((threadIdx.x & 63) == 0 && amax) __hip_atomic_fetch_max(&w.sc->amax_bits, amax, MCL_RLX);
}

__global__ __launch_bounds__(MCL_TILE) void mcl_labels_kernel(MclWork w, int64_t F) {
    const uint64_t amax = w.sc->amax_bits;
    const int e = amax ? mcl_exponent(amax) : 0;
    const int lane = threadIdx.x & 63;
    const int64_t tiles = mcl_tiles(F);
    for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {           // whole waves stay in the loop: shuffles below
        const int64_t f = t * MCL_TILE + threadIdx.x;
        int lab = -1;
        uint64_t l0 = 0, l1 = 0;
        if (f < F) {
            if (w.fkeep[f]) {
                lab = mcl_find(w.parent, (int)f);
                const double a = w.area[f];
                if (a > 0.0) mcl_limbs(a, e, l0, l1);
            }
            w.labels[f] = lab;
        }
        // one pair of adds per wave and label: neighbouring faces mostly share their component
        bool todo = lab >= 0 && (l0 | l1) != 0;
        uint64_t m = __ballot(todo);
        while (m) {
            const int leader = __ffsll((long long)m) - 1;
            const int L = __shfl(lab, leader);
            const bool mine = todo && lab == L;
            const uint64_t s0 = mcl_wave_sum(mine ? l0 : 0), s1 = mcl_wave_sum(mine ? l1 : 0);
            if (lane == leader) {
                if (s0) __hip_atomic_fetch_add(w.acc + 2 * (int64_t)L, s0, MCL_RLX);
                if (s1) __hip_atomic_fetch_add(w.acc + 2 * (int64_t)L + 1, s1, MCL_RLX);
            }
            todo = todo && !mine;
            m = __ballot(todo);
        }
    }
}

__global__ __launch_bounds__(MCL_TILE) void mcl_areas_kernel(MclWork w, int64_t F) {
    const uint64_t amax = w.sc->amax_bits;
    const int k = 80 - (amax ? mcl_exponent(amax) : 0);
    const int64_t tiles = mcl_tiles(F);
    uint64_t best = 0;
    int roots = 0;
    for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const int64_t f = t * MCL_TILE + threadIdx.x;
        const bool root = f < F && w.labels[f] == (int32_t)f;           // dropped faces carry -1
        if (root) {
            const double s = ldexp((double)w.acc[2 * f + 1], MCL_LIMB - k) + ldexp((double)w.acc[2 * f], -k);
            w.area[f] = s;                                              // face areas are not read after the labels pass
            const uint64_t bits = __builtin_bit_cast(uint64_t, s);
            best = bits > best ? bits : best;
        }
        roots += __popcll(__ballot(root));
    }
    best = mcl_wave_max(best);
    if ((threadIdx.x & 63) == 0) {
        if (best) __hip_atomic_fetch_max(&w.sc->best_bits, best, MCL_RLX);
        if (roots) __hip_atomic_fetch_add(&w.sc->n_comp, roots, MCL_RLX);
    }
}

__global__ __launch_bounds__(MCL_TILE) void mcl_best_kernel(MclWork w, int64_t F) {
    const uint64_t best = w.sc->best_bits;
    for (int64_t f = (int64_t)blockIdx.x * MCL_TILE + threadIdx.x; f < F; f += (int64_t)gridDim.x * MCL_TILE)
        if (w.labels[f] == (int32_t)f && __builtin_bit_cast(uint64_t, w.area[f]) == best)
            __hip_atomic_fetch_max(&w.sc->best_inv, 0x7fffffffu - (uint32_t)f, MCL_RLX);
}

__global__ __launch_bounds__(MCL_TILE) void mcl_keep_kernel(const int32_t* __restrict__ faces, MclWork w, int64_t F,
                                                            double min_area, int largest_only) {
    __shared__ int red[MCL_TILE / 64];
    const int32_t best = (int32_t)(0x7fffffffu - w.sc->best_inv);       // 0x7fffffff when there is no component
    const int64_t tiles = mcl_tiles(F);
    for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const int64_t f = t * MCL_TILE + threadIdx.x;
        bool keep = false;
        if (f < F) {
            const int lab = w.labels[f];
            if (lab >= 0) keep = largest_only ? lab == best : w.area[lab] > min_area;
            w.fkeep[f] = keep ? 1 : 0;
            if (keep) {
#pragma unroll
                for (int j = 0; j < 3; ++j) w.vused[faces[3 * f + j]] = 1;      // live faces have their indices in [0, V)
            }
        }
        int total;
        mcl_block_prefix(keep, red, total);
        if (threadIdx.x == 0) w.tile_f[t] = total;
        __syncthreads();
    }
}

__global__ __launch_bounds__(MCL_TILE) void mcl_vcount_kernel(MclWork w, int64_t V) {
    __shared__ int red[MCL_TILE / 64];
    const int64_t tiles = mcl_tiles(V);
    for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const int64_t v = t * MCL_TILE + threadIdx.x;
        int total;
        mcl_block_prefix(v < V && w.vused[v], red, total);
        if (threadIdx.x == 0) w.tile_v[t] = total;
        __syncthreads();
    }
}

// One block: both tile arrays -> exclusive offsets (in place); counts = {kept vertices, kept faces, components}.
__global__ __launch_bounds__(MCL_SCAN_THREADS) void mcl_scan_kernel(MclWork w, int64_t tiles_v, int64_t tiles_f,
                                                                    int32_t* __restrict__ counts) {
    __shared__ int sm[MCL_SCAN_THREADS];
    for (int pass = 0; pass < 2; ++pass) {
        int32_t* tile = pass ? w.tile_f : w.tile_v;
        const int64_t tiles = pass ? tiles_f : tiles_v;
        const int64_t chunk = (tiles + MCL_SCAN_THREADS - 1) / MCL_SCAN_THREADS;
        const int64_t lo = threadIdx.x * chunk;
        const int64_t hi = lo + chunk < tiles ? lo + chunk : tiles;
        int c = 0;
        for (int64_t i = lo; i < hi; ++i) c += tile[i];
        sm[threadIdx.x] = c;
        __syncthreads();
        for (int o = 1; o < MCL_SCAN_THREADS; o <<= 1) {                // inclusive Hillis-Steele scan
            const int a = threadIdx.x >= o ? sm[threadIdx.x - o] : 0;
            __syncthreads();
            sm[threadIdx.x] += a;
            __syncthreads();
        }
        int off = sm[threadIdx.x] - c;
        for (int64_t i = lo; i < hi; ++i) {
            const int n = tile[i];
            tile[i] = off;
            off += n;
        }
        if (threadIdx.x == MCL_SCAN_THREADS - 1) counts[pass] = sm[threadIdx.x];
        __syncthreads();
    }
    if (threadIdx.x == 0) counts[2] = w.sc->n_comp;
}

__global__ __launch_bounds__(MCL_TILE) void mcl_emit_verts_kernel(const double* __restrict__ verts, MclWork w, int64_t V,
                                                                  int32_t n_out, double* __restrict__ verts_out,
                                                                  int32_t* __restrict__ index_out) {
    __shared__ int red[MCL_TILE / 64];
    const int64_t tiles = mcl_tiles(V);
    for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const int64_t v = t * MCL_TILE + threadIdx.x;
        const bool used = v < V && w.vused[v];
        int unused;
        const int pos = w.tile_v[t] + mcl_block_prefix(used, red, unused);
        if (used && pos < n_out) {                      // n_out is the count call's total: the bound only guards a wrong caller
            w.vremap[v] = pos;
#pragma unroll
            for (int c = 0; c < 3; ++c) verts_out[3 * (int64_t)pos + c] = verts[3 * v + c];
            if (index_out) index_out[pos] = (int32_t)v;
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(MCL_TILE) void mcl_emit_faces_kernel(const int32_t* __restrict__ faces, MclWork w, int64_t F,
                                                                  int32_t n_out, int32_t* __restrict__ faces_out) {
    __shared__ int red[MCL_TILE / 64];
    const int64_t tiles = mcl_tiles(F);
    for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const int64_t f = t * MCL_TILE + threadIdx.x;
        const bool keep = f < F && w.fkeep[f];
        int unused;
        const int pos = w.tile_f[t] + mcl_block_prefix(keep, red, unused);
        if (keep && pos < n_out) {
#pragma unroll
            for (int j = 0; j < 3; ++j) faces_out[3 * (int64_t)pos + j] = w.vremap[faces[3 * f + j]];
        }
        __syncthreads();
    }
}

bool mcl_ok() { return hipGetLastError() == hipSuccess; }

}  // namespace

extern "C" {

int enslam_mesh_clean_workspace(int32_t n_verts, int32_t n_faces, int64_t* bytes_host) {
    const int rc = mcl_sizes(n_verts, n_faces);
    if (rc != ENSLAM_OK) return rc;
    if (!bytes_host) return ENSLAM_EINVAL;
    MclWork w;
    *bytes_host = mcl_carve(nullptr, n_verts, n_faces, w);
    return ENSLAM_OK;
}

int enslam_mesh_components(const int32_t* faces, int32_t n_faces, int32_t n_verts, void* workspace, int32_t* labels_out,
                           void* stream) {
    const int rc = mcl_sizes(n_verts, n_faces);
    if (rc != ENSLAM_OK) return rc;
    if (n_faces == 0) return ENSLAM_OK;
    if (!faces || !workspace || !labels_out) return ENSLAM_EINVAL;
    MclWork w;
    mcl_carve(workspace, n_verts, n_faces, w);
    hipStream_t s = (hipStream_t)stream;
    const int grid = mcl_grid(mcl_tiles(n_faces));
    if (hipMemsetAsync(w.keys, 0xFF, (size_t)w.table_bytes, s) != hipSuccess) return ENSLAM_ELAUNCH;
    mcl_iota_kernel<<<grid, MCL_TILE, 0, s>>>(w.parent, n_faces);
    mcl_link_kernel<<<grid, MCL_TILE, 0, s>>>(faces, n_faces, nullptr, w.keys, w.vals, w.cap, w.parent);
    mcl_flatten_kernel<<<grid, MCL_TILE, 0, s>>>(w.parent, n_faces, labels_out);
    return mcl_ok() ? ENSLAM_OK : ENSLAM_ELAUNCH;
}

int enslam_mesh_clean_count(const double* vertices, int32_t n_verts, const int32_t* faces, int32_t n_faces,
                            const uint8_t* vertex_keep, double min_area, int32_t largest_only, void* workspace, int32_t* counts,
                            void* stream) {
    const int rc = mcl_sizes(n_verts, n_faces);
    if (rc != ENSLAM_OK) return rc;
    if (!counts || !workspace || min_area != min_area || (n_faces > 0 && !faces) || (n_verts > 0 && !vertices))
        return ENSLAM_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    MclWork w;
    mcl_carve(workspace, n_verts, n_faces, w);
    if (hipMemsetAsync(w.sc, 0, (size_t)w.zero_bytes, s) != hipSuccess) return ENSLAM_ELAUNCH;
    const int64_t tf = mcl_tiles(n_faces), tv = mcl_tiles(n_verts);
    if (n_faces > 0) {
        const int grid = mcl_grid(tf);
        if (hipMemsetAsync(w.keys, 0xFF, (size_t)w.table_bytes, s) != hipSuccess) return ENSLAM_ELAUNCH;
        mcl_init_kernel<<<grid, MCL_TILE, 0, s>>>(vertices, n_verts, faces, n_faces, vertex_keep, w);
        mcl_link_kernel<<<grid, MCL_TILE, 0, s>>>(faces, n_faces, w.fkeep, w.keys, w.vals, w.cap, w.parent);
        mcl_labels_kernel<<<grid, MCL_TILE, 0, s>>>(w, n_faces);
        mcl_areas_kernel<<<grid, MCL_TILE, 0, s>>>(w, n_faces);
        if (largest_only) mcl_best_kernel<<<grid, MCL_TILE, 0, s>>>(w, n_faces);
        mcl_keep_kernel<<<grid, MCL_TILE, 0, s>>>(faces, w, n_faces, min_area, largest_only ? 1 : 0);
    }
    if (n_verts > 0) mcl_vcount_kernel<<<mcl_grid(tv), MCL_TILE, 0, s>>>(w, n_verts);
    mcl_scan_kernel<<<1, MCL_SCAN_THREADS, 0, s>>>(w, tv, tf, counts);
    return mcl_ok() ? ENSLAM_OK : ENSLAM_ELAUNCH;
}

int enslam_mesh_clean_emit(const double* vertices, int32_t n_verts, const int32_t* faces, int32_t n_faces, void* workspace,
                           int32_t n_verts_out, int32_t n_faces_out, double* vertices_out, int32_t* faces_out,
                           int32_t* vertex_index_out, void* stream) {
    const int rc = mcl_sizes(n_verts, n_faces);
    if (rc != ENSLAM_OK) return rc;
    if (!workspace || n_verts_out < 0 || n_faces_out < 0 || n_verts_out > n_verts || n_faces_out > n_faces ||
        (n_faces > 0 && !faces) || (n_verts > 0 && !vertices) || (n_verts_out > 0 && !vertices_out) ||
        (n_faces_out > 0 && !faces_out))
        return ENSLAM_EINVAL;
    if (n_verts_out == 0 || n_faces_out == 0) return ENSLAM_OK;        // a kept face keeps three vertices and the reverse
    MclWork w;
    mcl_carve(workspace, n_verts, n_faces, w);
    hipStream_t s = (hipStream_t)stream;
    mcl_emit_verts_kernel<<<mcl_grid(mcl_tiles(n_verts)), MCL_TILE, 0, s>>>(vertices, w, n_verts, n_verts_out, vertices_out,
                                                                           vertex_index_out);
    mcl_emit_faces_kernel<<<mcl_grid(mcl_tiles(n_faces)), MCL_TILE, 0, s>>>(faces, w, n_faces, n_faces_out, faces_out);
    return mcl_ok() ? ENSLAM_OK : ENSLAM_ELAUNCH;
}

}  // extern "C"
