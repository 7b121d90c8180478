// Time-stamped event streams (enslam_event_stream_*, enslam_event_accumulate; enslam_hip.h holds the model).
//
// Simulator side: the sensor of event_sim.hip, but every event leaves with a time stamp from linear level-crossing
// interpolation inside its sub-step (as ESIM does).  A stream is struct-of-arrays (t float64, x / y uint16, p uint8) in
// pixel-major order: row-major pixels, time-ordered within a pixel.  Two launches per interval, two passes of the one kernel
// of event_sim_core.hpp (one thread per pixel on its 64 x 4 tile, either source):
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

// count: the unsaturated per-pixel total; L_ref is only read.  O(1) per sub-step, no walk.
struct EsCountPass {
    static constexpr bool STAMPS = false, FRAME = false;
    using State = EsSensor;
    int64_t* counts;
    ES_HD void begin(const EsCommon& C, int64_t o, State& S, double& cp, double& cn) const { es_load(C, o, S, cp, cn); }
    ES_HD void substep(const EsCommon&, State& S, int64_t, int, int, int, double cp, double cn, double, double L) const {
        es_update(S, L, cp, cn);
    }
    ES_HD void end(const EsCommon&, int64_t o, const State& S, double) const { counts[o] = es_total(S); }
};

// emit: the pixel's run at its offset, the saturated count image and the new L_ref
struct EsEmitPass {
    static constexpr bool STAMPS = true, FRAME = false;
    struct State {
        EsSensor S;
        int64_t at, end;
    };
    EsStreamOut O;
    ES_HD void begin(const EsCommon& C, int64_t o, State& P, double& cp, double& cn) const {
        es_load(C, o, P.S, cp, cn);
        es_run(O, o, P.at, P.end);
    }
    ES_HD void substep(const EsCommon& C, State& P, int64_t, int y, int x, int s, double cp, double cn, double L_prev, double L) const {
        const double R = P.S.ref, pos0 = P.S.pos, neg0 = P.S.neg;
        es_update(P.S, L, cp, cn);
        es_emit_substep(O, P.at, P.end, y, x, s, C.K, R, P.S, pos0, neg0, cp, cn, L_prev, L);
    }
    ES_HD void end(const EsCommon& C, int64_t o, const State& P, double L_last) const { es_store(C, o, P.S, L_last); }
};

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
    EsImageSrc A;
    const int rc = es_image_count_args(plan, prev, cur, lut, L_prev, L_cur, c_pos_map, c_neg_map, L_ref, counts, A);
    return rc != ENSLAM_OK ? rc : es_launch(A, EsCountPass{counts}, stream);
}

int enslam_event_stream_images_emit(const enslam_event_sim_plan* plan, const uint8_t* prev, const uint8_t* cur,
                                    const double* lut, const double* L_prev, const double* L_cur, const double* c_pos_map,
                                    const double* c_neg_map, double* L_ref, uint8_t* events, const int64_t* ends, int64_t total,
                                    double t_a, double t_b, double* t, uint16_t* x, uint16_t* y, uint8_t* p, void* stream) {
    int rc = es_stream_plan(plan);
    if (rc != ENSLAM_OK) return rc;
    EsImageSrc A;
    EsEmitPass E;
    rc = es_image_args(plan, prev, cur, lut, L_prev, L_cur, c_pos_map, c_neg_map, L_ref, events, A);
    if (rc != ENSLAM_OK) return rc;
    rc = es_stream_out(ends, total, t_a, t_b, t, x, y, p, E.O);
    return rc != ENSLAM_OK ? rc : es_launch(A, E, stream);
}

// poses: [K,12], the sub-steps
int enslam_event_stream_boxroom_count(const enslam_event_sim_plan* plan, const double* poses, const double* c_pos_map,
                                      const double* c_neg_map, const double* L_ref, int64_t* counts, void* stream) {
    EsRoomSrc A;
    const int rc = es_room_count_args(plan, poses, false, c_pos_map, c_neg_map, L_ref, counts, A);
    return rc != ENSLAM_OK ? rc : es_launch(A, EsCountPass{counts}, stream);
}

// poses: [K+1,12], row 0 the previous frame's (rendered for L_prev only), rows 1..K the sub-steps
int enslam_event_stream_boxroom_emit(const enslam_event_sim_plan* plan, const double* poses, const double* c_pos_map,
                                     const double* c_neg_map, double* L_ref, uint8_t* events, const int64_t* ends, int64_t total,
                                     double t_a, double t_b, double* t, uint16_t* x, uint16_t* y, uint8_t* p, void* stream) {
    int rc = es_stream_plan(plan);
    if (rc != ENSLAM_OK) return rc;
    EsRoomSrc A;
    EsEmitPass E;
    rc = es_room_args(plan, poses, true, c_pos_map, c_neg_map, L_ref, events, nullptr, nullptr, A);
    if (rc != ENSLAM_OK) return rc;
    rc = es_stream_out(ends, total, t_a, t_b, t, x, y, p, E.O);
    return rc != ENSLAM_OK ? rc : es_launch(A, E, stream);
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
