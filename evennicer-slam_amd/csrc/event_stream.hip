// Time-stamped event streams (enslam_event_stream_*, enslam_event_accumulate; enslam_hip.h holds the model).
//
// Simulator side: the sensor of event_sim.hip, but every event leaves with a time stamp from linear level-crossing
// interpolation inside its sub-step (as ESIM does).  A stream is struct-of-arrays (t float64, x / y uint16, p uint8) in
// pixel-major order: row-major pixels, time-ordered within a pixel.  Two launches per interval, one thread per pixel on the
// 64 x 4 tile of event_sim.hip:
//   count  walks the sub-steps exactly as event_sim.hip does and writes the unsaturated per-pixel total (int64); L_ref is
//          only read
//   emit   walks them again and writes the pixel's run at its offset (the caller's inclusive prefix sum of the counts), the
//          saturated uint8 (-, +) image and the new L_ref
// The counts and L_ref come from es_update of event_sim_core.hpp, the one event_sim.hip calls: the stream route adds the
// time stamps and derives nothing again.  Consecutive pixels own adjacent runs, so a wave's stores fall into one compact
// region.  No atomics, no LDS, no cross-lane traffic: two runs are bit-identical.  Every store of the emit pass is guarded
// by the end of the pixel's own run and by the capacity of the arrays.
//
// Accumulator side: any stream, in any order, into count images per time bin.  One thread per event: the sensor bounds are
// checked before any address is formed, the bin comes from a binary search of the ascending edges (staged in LDS while
// B + 1 <= 2048), and the count is one integer atomicAdd on a uint32; a second pass saturates to uint8.  Integer sums do
// not depend on the order of arrival: the result is bit-reproducible and the same for every order of the stream.  The two
// drop counters are summed per workgroup in LDS, then one global integer add per workgroup and counter.
#include "../../include/enslam_hip.h"
#include "common.hpp"

#include "event_sim_core.hpp"

namespace {

constexpr int EA_BLOCK = 256;
constexpr int EA_LDS_EDGES = 2048;                      // 16 KiB of float64 edges
constexpr int64_t EA_MAX_CELLS = (int64_t)1 << 30;      // B * H * W

// The events of one sub-step s (1-based) of K: R is L_ref before es_update, S the state after it, pos0 / neg0 the counts
// before it.  Event k crosses X_k = R +- k * C at f_k (es_cross_fraction) and leaves at es_stamp of it: event_sim_core.hpp.
ES_HD void es_emit_substep(const EsStreamOut& O, int64_t& at, int64_t end, int y, int x, int s, int K, double R,
                           const EsSensor& S, double pos0, double neg0, double cp, double cn, double L_prev, double L) {
    const double n_pos = S.pos - pos0, n_neg = S.neg - neg0;
    const bool up = n_pos > 0.0;
    const double n = up ? n_pos : n_neg, c = up ? cp : cn;
    const double D = L - L_prev;
    for (double k = 1.0; k <= n && at < end; k += 1.0) {
        es_put(O, at, es_stamp(O, s, K, es_cross_fraction(R, k, c, up, L_prev, D)), y, x, up);
        ++at;
    }
}

ES_HD int64_t es_image_pixel_count(const EsImageArgs& A, int y, int x) {
    const int64_t o = (int64_t)y * A.c.W + x;
    const double La = A.L_prev ? A.L_prev[o] : es_image_level(A, A.prev, o);
    const double Lb = A.L_cur ? A.L_cur[o] : es_image_level(A, A.cur, o);
    EsSensor S;
    double cp, cn;
    es_load(A.c, o, S, cp, cn);
    const double dL = Lb - La;
    for (int s = 1; s <= A.c.K; ++s) {
        const double L = La + ((double)s / (double)A.c.K) * dL;
        es_update(S, L, cp, cn);
    }
    return es_total(S);
}

ES_HD void es_image_pixel_emit(const EsImageArgs& A, const EsStreamOut& O, int y, int x) {
    const int64_t o = (int64_t)y * A.c.W + x;
    const double La = A.L_prev ? A.L_prev[o] : es_image_level(A, A.prev, o);
    const double Lb = A.L_cur ? A.L_cur[o] : es_image_level(A, A.cur, o);
    EsSensor S;
    double cp, cn, L = Lb, L_before = La;
    int64_t at, end;
    es_load(A.c, o, S, cp, cn);
    es_run(O, o, at, end);
    const double dL = Lb - La;
    for (int s = 1; s <= A.c.K; ++s) {
        L = La + ((double)s / (double)A.c.K) * dL;
        const double R = S.ref, pos0 = S.pos, neg0 = S.neg;
        es_update(S, L, cp, cn);
        es_emit_substep(O, at, end, y, x, s, A.c.K, R, S, pos0, neg0, cp, cn, L_before, L);
        L_before = L;
    }
    es_store(A.c, o, S, L);
}

// poses: [K,12], the sub-steps
ES_HD int64_t es_room_pixel_count(const EsRoomArgs& A, int y, int x) {
    const int64_t o = (int64_t)y * A.c.W + x;
    EsSensor S;
    double cp, cn;
    es_load(A.c, o, S, cp, cn);
#pragma clang loop unroll(disable)
    for (int s = 0; s < A.c.K; ++s) es_update(S, es_room_level(A, A.poses + 12 * s, y, x), cp, cn);
    return es_total(S);
}

// poses: [K+1,12], row 0 the previous frame's (rendered for L_prev only), rows 1..K the sub-steps
ES_HD void es_room_pixel_emit(const EsRoomArgs& A, const EsStreamOut& O, int y, int x) {
    const int64_t o = (int64_t)y * A.c.W + x;
    EsSensor S;
    double cp, cn;
    int64_t at, end;
    es_load(A.c, o, S, cp, cn);
    es_run(O, o, at, end);
    double L_before = es_room_level(A, A.poses, y, x), L = L_before;
#pragma clang loop unroll(disable)
    for (int s = 1; s <= A.c.K; ++s) {
        L = es_room_level(A, A.poses + 12 * s, y, x);
        const double R = S.ref, pos0 = S.pos, neg0 = S.neg;
        es_update(S, L, cp, cn);
        es_emit_substep(O, at, end, y, x, s, A.c.K, R, S, pos0, neg0, cp, cn, L_before, L);
        L_before = L;
    }
    es_store(A.c, o, S, L);
}

__global__ __launch_bounds__(ES_BLOCK) void event_stream_images_count_kernel(EsImageArgs A, int64_t* counts) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= A.c.W || y >= A.c.H) return;
    counts[(int64_t)y * A.c.W + x] = es_image_pixel_count(A, y, x);
}

__global__ __launch_bounds__(ES_BLOCK) void event_stream_images_emit_kernel(EsImageArgs A, EsStreamOut O) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= A.c.W || y >= A.c.H) return;
    es_image_pixel_emit(A, O, y, x);
}

__global__ __launch_bounds__(ES_BLOCK) void event_stream_boxroom_count_kernel(EsRoomArgs A, int64_t* counts) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= A.c.W || y >= A.c.H) return;
    counts[(int64_t)y * A.c.W + x] = es_room_pixel_count(A, y, x);
}

__global__ __launch_bounds__(ES_BLOCK) void event_stream_boxroom_emit_kernel(EsRoomArgs A, EsStreamOut O) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= A.c.W || y >= A.c.H) return;
    es_room_pixel_emit(A, O, y, x);
}

struct EaArgs {
    const double* t;
    const uint16_t* x;
    const uint16_t* y;
    const uint8_t* p;
    int64_t N;
    const double* edges;            // [B+1]
    int32_t B, H, W, edges_in_lds;
    uint32_t* acc;                  // [B,H,W,2]
    unsigned long long* dropped;    // [2]: by time, by sensor
};

__global__ __launch_bounds__(EA_BLOCK) void event_accumulate_kernel(EaArgs A) {
    __shared__ double s_edges[EA_LDS_EDGES];
    __shared__ unsigned s_drop[2];
    if (threadIdx.x < 2) s_drop[threadIdx.x] = 0u;
    if (A.edges_in_lds)
        for (int i = threadIdx.x; i <= A.B; i += EA_BLOCK) s_edges[i] = A.edges[i];
    __syncthreads();
    const int64_t i = (int64_t)blockIdx.x * EA_BLOCK + threadIdx.x;
    if (i < A.N) {
        const unsigned ex = A.x[i], ey = A.y[i];
        if (ex >= (unsigned)A.W || ey >= (unsigned)A.H) {
            atomicAdd(&s_drop[1], 1u);
        } else {
            const double tv = A.t[i];
            int lo = 0, hi = A.B + 1;                   // the first j in 0..B with tv <= edges[j]; B + 1 when there is none
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                const double e = A.edges_in_lds ? s_edges[mid] : A.edges[mid];
                if (tv <= e) hi = mid; else lo = mid + 1;
            }
            if (lo == 0 || lo > A.B) {                  // at or before edges[0], after edges[B], or not a number
                atomicAdd(&s_drop[0], 1u);
            } else {                                    // edges[lo - 1] < tv <= edges[lo]
                const int64_t cell = ((int64_t)(lo - 1) * A.H + (int64_t)ey) * A.W + (int64_t)ex;
                atomicAdd(&A.acc[2 * cell + (A.p[i] ? 1 : 0)], 1u);
            }
        }
    }
    __syncthreads();
    if (threadIdx.x < 2 && s_drop[threadIdx.x]) atomicAdd(&A.dropped[threadIdx.x], (unsigned long long)s_drop[threadIdx.x]);
}

// one thread per cell: the two uint32 counts of a cell as one 8-byte load, the two saturated bytes as one 2-byte store
__global__ __launch_bounds__(EA_BLOCK) void event_saturate_kernel(const uint32_t* __restrict__ acc, uint8_t* __restrict__ counts,
                                                                  int64_t cells) {
    const int64_t c = (int64_t)blockIdx.x * EA_BLOCK + threadIdx.x;
    if (c >= cells) return;
    const uint2 v = reinterpret_cast<const uint2*>(acc)[c];
    const unsigned neg = v.x > 255u ? 255u : v.x, pos = v.y > 255u ? 255u : v.y;
    reinterpret_cast<uint16_t*>(counts)[c] = (uint16_t)(neg | (pos << 8));
}

}  // namespace

extern "C" {

int enslam_event_stream_images_count(const enslam_event_sim_plan* plan, const uint8_t* prev, const uint8_t* cur,
                                     const double* lut, const double* L_prev, const double* L_cur, const double* c_pos_map,
                                     const double* c_neg_map, const double* L_ref, int64_t* counts, void* stream) {
    int rc = es_stream_plan(plan);
    if (rc != ENSLAM_OK) return rc;
    if (!counts) return ENSLAM_EINVAL;
    EsImageArgs A;                  // the count kernel only reads L_ref and has no event image: es_store is never called
    rc = es_image_args(plan, prev, cur, lut, L_prev, L_cur, c_pos_map, c_neg_map, const_cast<double*>(L_ref),
                       reinterpret_cast<uint8_t*>(counts), A);
    if (rc != ENSLAM_OK) return rc;
    A.c.events = nullptr;
    event_stream_images_count_kernel<<<es_grid(A.c), ES_BLOCK, 0, (hipStream_t)stream>>>(A, counts);
    return hipGetLastError() == hipSuccess ? ENSLAM_OK : ENSLAM_ELAUNCH;
}

int enslam_event_stream_images_emit(const enslam_event_sim_plan* plan, const uint8_t* prev, const uint8_t* cur,
                                    const double* lut, const double* L_prev, const double* L_cur, const double* c_pos_map,
                                    const double* c_neg_map, double* L_ref, uint8_t* events, const int64_t* ends, int64_t total,
                                    double t_a, double t_b, double* t, uint16_t* x, uint16_t* y, uint8_t* p, void* stream) {
    int rc = es_stream_plan(plan);
    if (rc != ENSLAM_OK) return rc;
    EsImageArgs A;
    EsStreamOut O;
    rc = es_image_args(plan, prev, cur, lut, L_prev, L_cur, c_pos_map, c_neg_map, L_ref, events, A);
    if (rc != ENSLAM_OK) return rc;
    rc = es_stream_out(ends, total, t_a, t_b, t, x, y, p, O);
    if (rc != ENSLAM_OK) return rc;
    event_stream_images_emit_kernel<<<es_grid(A.c), ES_BLOCK, 0, (hipStream_t)stream>>>(A, O);
    return hipGetLastError() == hipSuccess ? ENSLAM_OK : ENSLAM_ELAUNCH;
}

int enslam_event_stream_boxroom_count(const enslam_event_sim_plan* plan, const double* poses, const double* c_pos_map,
                                      const double* c_neg_map, const double* L_ref, int64_t* counts, void* stream) {
    int rc = es_stream_plan(plan);
    if (rc != ENSLAM_OK) return rc;
    if (!counts) return ENSLAM_EINVAL;
    EsRoomArgs A;
    rc = es_room_args(plan, poses, c_pos_map, c_neg_map, const_cast<double*>(L_ref), reinterpret_cast<uint8_t*>(counts), nullptr,
                      nullptr, A);
    if (rc != ENSLAM_OK) return rc;
    A.c.events = nullptr;
    event_stream_boxroom_count_kernel<<<es_grid(A.c), ES_BLOCK, 0, (hipStream_t)stream>>>(A, counts);
    return hipGetLastError() == hipSuccess ? ENSLAM_OK : ENSLAM_ELAUNCH;
}

int enslam_event_stream_boxroom_emit(const enslam_event_sim_plan* plan, const double* poses, const double* c_pos_map,
                                     const double* c_neg_map, double* L_ref, uint8_t* events, const int64_t* ends, int64_t total,
                                     double t_a, double t_b, double* t, uint16_t* x, uint16_t* y, uint8_t* p, void* stream) {
    int rc = es_stream_plan(plan);
    if (rc != ENSLAM_OK) return rc;
    EsRoomArgs A;
    EsStreamOut O;
    rc = es_room_args(plan, poses, c_pos_map, c_neg_map, L_ref, events, nullptr, nullptr, A);
    if (rc != ENSLAM_OK) return rc;
    rc = es_stream_out(ends, total, t_a, t_b, t, x, y, p, O);
    if (rc != ENSLAM_OK) return rc;
    event_stream_boxroom_emit_kernel<<<es_grid(A.c), ES_BLOCK, 0, (hipStream_t)stream>>>(A, O);
    return hipGetLastError() == hipSuccess ? ENSLAM_OK : ENSLAM_ELAUNCH;
}

int enslam_event_accumulate(const double* t, const uint16_t* x, const uint16_t* y, const uint8_t* p, int64_t N,
                            const double* edges_host, const double* edges, int32_t B, int32_t H, int32_t W, uint32_t* acc,
                            uint8_t* counts, uint64_t* dropped, void* stream) {
    if (!edges_host || !edges || !acc || !counts || !dropped || N < 0) return ENSLAM_EINVAL;
    if (N > 0 && (!t || !x || !y || !p)) return ENSLAM_EINVAL;
    if (B <= 0 || H <= 0 || W <= 0) return ENSLAM_EINVAL;
    if (((uintptr_t)acc & 7) || ((uintptr_t)counts & 1) || ((uintptr_t)dropped & 7)) return ENSLAM_EINVAL;
    if (N > ES_MAX_EVENTS || (int64_t)B * H > EA_MAX_CELLS || (int64_t)B * H * W > EA_MAX_CELLS) return ENSLAM_EUNSUPPORTED;
    for (int32_t b = 0; b < B; ++b)
        if (!(edges_host[b] <= edges_host[b + 1])) return ENSLAM_EINVAL;            // descending, or not a number
    const int64_t cells = (int64_t)B * H * W;
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(acc, 0, (size_t)cells * 2 * sizeof(uint32_t), st) != hipSuccess) return ENSLAM_ELAUNCH;
    if (hipMemsetAsync(dropped, 0, 2 * sizeof(uint64_t), st) != hipSuccess) return ENSLAM_ELAUNCH;
    if (N > 0) {
        EaArgs A;
        A.t = t; A.x = x; A.y = y; A.p = p; A.N = N; A.edges = edges; A.B = B; A.H = H; A.W = W;
        A.edges_in_lds = B + 1 <= EA_LDS_EDGES;
        A.acc = acc; A.dropped = reinterpret_cast<unsigned long long*>(dropped);
        event_accumulate_kernel<<<(unsigned)((N + EA_BLOCK - 1) / EA_BLOCK), EA_BLOCK, 0, st>>>(A);
        if (hipGetLastError() != hipSuccess) return ENSLAM_ELAUNCH;
    }
    event_saturate_kernel<<<(unsigned)((cells + EA_BLOCK - 1) / EA_BLOCK), EA_BLOCK, 0, st>>>(acc, counts, cells);
    return hipGetLastError() == hipSuccess ? ENSLAM_OK : ENSLAM_ELAUNCH;
}

}  // extern "C"
