// Event-stream denoising (enslam_event_pixel_counts, enslam_event_filter_*; enslam_hip.h holds the model): hot-pixel mask,
// refractory filter and background-activity (neighbour-support) filter on a stream t float64, x / y uint16, p uint8.
//
// Four entries, five kernels.  The order of the live events (pixel, then t, then stream position) is the caller's: torch's
// stable sorts and a cumsum of the counts, skipped where the order flags of the first entry allow.
//   classify  one thread per event: class of stage 0 and the flat pixel id (bounds first, then the time, then the mask), one
//             integer atomicAdd into counts[H,W], and the two order flags: every live event looks back for the previous live
//             one (through at most EF_LOOKBACK dead events; beyond that both flags are reported as violated, which only costs a sort)
//             and compares; violations are ORed per workgroup in LDS, then one global atomicOr per workgroup that saw one
//   walk      one thread per pixel over its run of `order`: ESIM's rule t - t_last >= rho in a register, REFRACTORY classes,
//             the passing times and event indices stored compactly at the front of the run, the per-pixel count, t_last.
//             Linear in the run.  An entry of `order` is used only if it is inside [0, N) and that event is live AND of this
//             pixel, so a wrong order cannot make two threads write one class.
//   support   one thread per slot of the compact runs (s_event = -1 marks an unused slot): up to eight binary searches for the
//             largest passing time <= t in the neighbours' compact runs, then the neighbour's carried t_seen; UNSUPPORTED
//             classes.  Reads the OLD t_seen: the state update is the next launch.
//   seen      one thread per pixel: t_seen = max(t_seen, t_last) where the pixel passed an event (its last passing time)
//   compact   one thread per event: a kept event goes to slot ends[i] - 1 of the outputs (the caller's inclusive prefix sum
//             of the keep flags), which preserves the stream order
// Only integer atomics, and none whose result depends on the order of arrival: two runs are bit-identical.  Run bounds are
// clamped to [0, n_live], counts to the run, output slots to the capacity: no load or store leaves an array whatever `order`,
// `starts` and `ends` hold.
#include "../../include/enslam_hip.h"
#include "common.hpp"

#include <cfloat>
#include <cmath>

namespace {

constexpr int EF_BLOCK = 256;
constexpr int EF_LOOKBACK = 32;
constexpr int64_t EF_MAX_EVENTS = 2147483647;           // 2^31 - 1
constexpr int64_t EF_MAX_PIXELS = (int64_t)1 << 28;

struct EfClassifyArgs {
    const double* t;
    const uint16_t* x;
    const uint16_t* y;
    int64_t N;
    int32_t H, W;
    const uint8_t* hot;             // [H,W] or NULL
    uint8_t* cls;                   // [N]
    int32_t* pix;                   // [N]
    int32_t* counts;                // [H,W]
    uint32_t* flags;                // [1]
};

// class of stage 0 and the flat pixel id (-1 outside the sensor) of event i
__device__ __forceinline__ int ef_stage0(const EfClassifyArgs& A, int64_t i, int32_t& o, double& tv) {
    const unsigned ex = A.x[i], ey = A.y[i];
    o = -1;
    tv = 0.0;
    if (ex >= (unsigned)A.W || ey >= (unsigned)A.H) return ENSLAM_EVENT_SENSOR;
    o = (int32_t)(ey * (unsigned)A.W + ex);
    tv = A.t[i];
    if (!(fabs(tv) <= DBL_MAX)) return ENSLAM_EVENT_TIME;         // NaN, +inf, -inf
    if (A.hot && A.hot[o]) return ENSLAM_EVENT_HOT;
    return ENSLAM_EVENT_KEPT;
}

__global__ __launch_bounds__(EF_BLOCK) void event_filter_classify_kernel(EfClassifyArgs A) {
    __shared__ unsigned s_flags;
    if (threadIdx.x == 0) s_flags = 0u;
    __syncthreads();
    const int64_t i = (int64_t)blockIdx.x * EF_BLOCK + threadIdx.x;
    if (i < A.N) {
        int32_t o;
        double tv;
        const int c = ef_stage0(A, i, o, tv);
        A.cls[i] = (uint8_t)c;
        A.pix[i] = o;
        if (c != ENSLAM_EVENT_SENSOR && c != ENSLAM_EVENT_TIME) atomicAdd(&A.counts[o], 1);
        if (c == ENSLAM_EVENT_KEPT) {
            unsigned bad = 0u;
            int64_t j = i - 1;
            int steps = 0;
            for (; j >= 0 && steps <= EF_LOOKBACK; --j, ++steps) {       // looks through at most EF_LOOKBACK dead events
                int32_t oj;
                double tj;
                if (ef_stage0(A, j, oj, tj) == ENSLAM_EVENT_KEPT) {
                    if (tv < tj) bad |= ENSLAM_EVENT_NOT_TIME_ORDERED;
                    if (o < oj || (o == oj && tv < tj)) bad |= ENSLAM_EVENT_NOT_PIXEL_MAJOR;
                    break;
                }
            }
            if (j >= 0 && steps > EF_LOOKBACK) bad = ENSLAM_EVENT_NOT_TIME_ORDERED | ENSLAM_EVENT_NOT_PIXEL_MAJOR;
            if (bad) atomicOr(&s_flags, bad);
        }
    }
    __syncthreads();
    if (threadIdx.x == 0 && s_flags) atomicOr(A.flags, s_flags);
}

struct EfStageArgs {
    const double* t;
    int64_t N, n_live, P;           // P = H * W
    int32_t H, W;
    double rho, dt;
    const int32_t* pix;             // [N]
    const int32_t* order;           // [n_live]
    const int64_t* starts;          // [P + 1]
    uint8_t* cls;                   // [N]
    double* t_last;                 // [P]
    double* t_seen;                 // [P]
    double* s_times;                // [n_live]
    int32_t* s_event;               // [n_live]
    int32_t* s_count;               // [P]
};

// the run of pixel o in `order`, clamped: 0 <= a <= b <= n_live
__device__ __forceinline__ void ef_run(const EfStageArgs& A, int64_t o, int64_t& a, int64_t& b) {
    a = A.starts[o];
    b = A.starts[o + 1];
    a = a < 0 ? 0 : (a > A.n_live ? A.n_live : a);
    b = b < a ? a : (b > A.n_live ? A.n_live : b);
}

__global__ __launch_bounds__(EF_BLOCK) void event_filter_walk_kernel(EfStageArgs A) {
    const int64_t o = (int64_t)blockIdx.x * EF_BLOCK + threadIdx.x;
    if (o >= A.P) return;
    int64_t a, b;
    ef_run(A, o, a, b);
    double tl = A.t_last[o];
    int64_t n = 0;
    for (int64_t k = a; k < b; ++k) {
        const int64_t i = A.order[k];
        if (i < 0 || i >= A.N) continue;
        if (A.pix[i] != (int32_t)o || A.cls[i] != ENSLAM_EVENT_KEPT) continue;
        const double tv = A.t[i];
        if (tv - tl >= A.rho) {                                 // +inf for t_last = -inf
            tl = tv;
            A.s_times[a + n] = tv;                              // n <= k - a: inside the run
            A.s_event[a + n] = (int32_t)i;
            ++n;
        } else {
            A.cls[i] = ENSLAM_EVENT_REFRACTORY;
        }
    }
    A.s_count[o] = (int32_t)n;
    A.t_last[o] = tl;
}

__global__ __launch_bounds__(EF_BLOCK) void event_filter_support_kernel(EfStageArgs A) {
    const int64_t k = (int64_t)blockIdx.x * EF_BLOCK + threadIdx.x;
    if (k >= A.n_live) return;
    const int64_t i = A.s_event[k];
    if (i < 0 || i >= A.N) return;                              // an unused slot
    const int32_t o = A.pix[i];
    if (o < 0 || (int64_t)o >= A.P) return;
    const double tv = A.s_times[k];
    const int y = o / A.W, x = o - y * A.W;
    bool supported = false;
    for (int dy = -1; dy <= 1 && !supported; ++dy) {
        const int ny = y + dy;
        if (ny < 0 || ny >= A.H) continue;
        for (int dx = -1; dx <= 1 && !supported; ++dx) {
            const int nx = x + dx;
            if ((dx == 0 && dy == 0) || nx < 0 || nx >= A.W) continue;
            const int64_t q = (int64_t)ny * A.W + nx;
            int64_t a, b;
            ef_run(A, q, a, b);
            int64_t cnt = A.s_count[q];
            cnt = cnt < 0 ? 0 : (cnt > b - a ? b - a : cnt);
            int64_t lo = 0, hi = cnt;                           // the number of passing times <= tv in the neighbour's run
            while (lo < hi) {
                const int64_t mid = (lo + hi) >> 1;
                if (A.s_times[a + mid] <= tv) lo = mid + 1; else hi = mid;
            }
            if (lo > 0 && tv - A.s_times[a + lo - 1] <= A.dt) supported = true;
            if (!supported) {
                const double ts = A.t_seen[q];
                if (ts <= tv && tv - ts <= A.dt) supported = true;
            }
        }
    }
    if (!supported) A.cls[i] = ENSLAM_EVENT_UNSUPPORTED;
}

__global__ __launch_bounds__(EF_BLOCK) void event_filter_seen_kernel(EfStageArgs A) {
    const int64_t o = (int64_t)blockIdx.x * EF_BLOCK + threadIdx.x;
    if (o >= A.P) return;
    if (A.s_count[o] > 0) {
        const double tl = A.t_last[o], ts = A.t_seen[o];
        if (tl > ts) A.t_seen[o] = tl;
    }
}

struct EfCompactArgs {
    const double* t;
    const uint16_t* x;
    const uint16_t* y;
    const uint8_t* p;
    int64_t N, n_out;
    const uint8_t* cls;
    const int64_t* ends;
    double* to;
    uint16_t* xo;
    uint16_t* yo;
    uint8_t* po;
};

__global__ __launch_bounds__(EF_BLOCK) void event_filter_compact_kernel(EfCompactArgs A) {
    const int64_t i = (int64_t)blockIdx.x * EF_BLOCK + threadIdx.x;
    if (i >= A.N || A.cls[i] != ENSLAM_EVENT_KEPT) return;
    const int64_t j = A.ends[i] - 1;
    if (j < 0 || j >= A.n_out) return;
    A.to[j] = A.t[i];
    A.xo[j] = A.x[i];
    A.yo[j] = A.y[i];
    A.po[j] = A.p[i];
}

inline unsigned ef_blocks(int64_t n) { return (unsigned)((n + EF_BLOCK - 1) / EF_BLOCK); }

inline bool ef_misaligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) != 0; }

// the refusals every entry shares: EINVAL first, then EUNSUPPORTED
int ef_sizes(int64_t N, int32_t H, int32_t W) {
    if (N < 0 || H <= 0 || W <= 0) return ENSLAM_EINVAL;
    if (N > EF_MAX_EVENTS || H > 65536 || W > 65536 || (int64_t)H * W > EF_MAX_PIXELS) return ENSLAM_EUNSUPPORTED;
    return ENSLAM_OK;
}

int ef_stage_args(const double* t, int64_t N, int32_t H, int32_t W, double rho, double dt, const int32_t* pix,
                  const int32_t* order, int64_t n_live, const int64_t* starts, uint8_t* cls, double* t_last, double* t_seen,
                  double* s_times, int32_t* s_event, int32_t* s_count, EfStageArgs& A) {
    if (!starts || !t_last || !t_seen || !s_count || n_live < 0 || n_live > N) return ENSLAM_EINVAL;
    if (N > 0 && (!t || !pix || !cls)) return ENSLAM_EINVAL;
    if (n_live > 0 && (!order || !s_times || !s_event)) return ENSLAM_EINVAL;
    if (!(rho >= 0.0) || !std::isfinite(rho) || !(dt >= 0.0) || !std::isfinite(dt)) return ENSLAM_EINVAL;
    if (ef_misaligned(t, 8) || ef_misaligned(pix, 4) || ef_misaligned(order, 4) || ef_misaligned(starts, 8) ||
        ef_misaligned(t_last, 8) || ef_misaligned(t_seen, 8) || ef_misaligned(s_times, 8) || ef_misaligned(s_event, 4) ||
        ef_misaligned(s_count, 4))
        return ENSLAM_EINVAL;
    A.t = t; A.N = N; A.n_live = n_live; A.P = (int64_t)H * W; A.H = H; A.W = W; A.rho = rho; A.dt = dt;
    A.pix = pix; A.order = order; A.starts = starts; A.cls = cls; A.t_last = t_last; A.t_seen = t_seen;
    A.s_times = s_times; A.s_event = s_event; A.s_count = s_count;
    return ENSLAM_OK;
}

}  // namespace

extern "C" {

int enslam_event_pixel_counts(const double* t, const uint16_t* x, const uint16_t* y, int64_t N, int32_t H, int32_t W,
                              const uint8_t* hot_mask, uint8_t* cls, int32_t* pix, int32_t* counts, uint32_t* flags,
                              void* stream) {
    if (!counts || !flags) return ENSLAM_EINVAL;
    int rc = ef_sizes(N, H, W);
    if (rc == ENSLAM_EINVAL) return rc;
    if (N > 0 && (!t || !x || !y || !cls || !pix)) return ENSLAM_EINVAL;
    if (ef_misaligned(t, 8) || ef_misaligned(x, 2) || ef_misaligned(y, 2) || ef_misaligned(pix, 4) || ef_misaligned(counts, 4) ||
        ef_misaligned(flags, 4))
        return ENSLAM_EINVAL;
    if (rc != ENSLAM_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(counts, 0, (size_t)H * W * sizeof(int32_t), st) != hipSuccess) return ENSLAM_ELAUNCH;
    if (hipMemsetAsync(flags, 0, sizeof(uint32_t), st) != hipSuccess) return ENSLAM_ELAUNCH;
    if (N == 0) return ENSLAM_OK;
    EfClassifyArgs A;
    A.t = t; A.x = x; A.y = y; A.N = N; A.H = H; A.W = W; A.hot = hot_mask; A.cls = cls; A.pix = pix; A.counts = counts;
    A.flags = flags;
    event_filter_classify_kernel<<<ef_blocks(N), EF_BLOCK, 0, st>>>(A);
    return hipGetLastError() == hipSuccess ? ENSLAM_OK : ENSLAM_ELAUNCH;
}

int enslam_event_filter_walk(const double* t, int64_t N, int32_t H, int32_t W, double rho, const int32_t* pix,
                             const int32_t* order, int64_t n_live, const int64_t* starts, uint8_t* cls, double* t_last,
                             double* s_times, int32_t* s_event, int32_t* s_count, void* stream) {
    int rc = ef_sizes(N, H, W);
    if (rc == ENSLAM_EINVAL) return rc;
    EfStageArgs A;
    const int rc2 = ef_stage_args(t, N, H, W, rho, 0.0, pix, order, n_live, starts, cls, t_last, t_last, s_times, s_event, s_count, A);
    if (rc2 != ENSLAM_OK) return rc2;
    if (rc != ENSLAM_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (n_live > 0 && hipMemsetAsync(s_event, 0xFF, (size_t)n_live * sizeof(int32_t), st) != hipSuccess) return ENSLAM_ELAUNCH;
    event_filter_walk_kernel<<<ef_blocks(A.P), EF_BLOCK, 0, st>>>(A);
    return hipGetLastError() == hipSuccess ? ENSLAM_OK : ENSLAM_ELAUNCH;
}

int enslam_event_filter_support(int64_t N, int32_t H, int32_t W, int32_t support, double dt, const int32_t* pix,
                                int64_t n_live, const int64_t* starts, uint8_t* cls, const double* t_last, double* t_seen,
                                const double* s_times, const int32_t* s_event, const int32_t* s_count, void* stream) {
    int rc = ef_sizes(N, H, W);
    if (rc == ENSLAM_EINVAL) return rc;
    EfStageArgs A;
    static const double t_dummy = 0.0;                          // `t` and `order` are not read by these kernels
    static const int32_t o_dummy = 0;
    const int rc2 = ef_stage_args(&t_dummy, N, H, W, 0.0, dt, pix, &o_dummy, n_live, starts, cls, const_cast<double*>(t_last), t_seen,
                                  const_cast<double*>(s_times), const_cast<int32_t*>(s_event), const_cast<int32_t*>(s_count), A);
    if (rc2 != ENSLAM_OK) return rc2;
    if (rc != ENSLAM_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (support && n_live > 0) {
        event_filter_support_kernel<<<ef_blocks(n_live), EF_BLOCK, 0, st>>>(A);
        if (hipGetLastError() != hipSuccess) return ENSLAM_ELAUNCH;
    }
    event_filter_seen_kernel<<<ef_blocks(A.P), EF_BLOCK, 0, st>>>(A);
    return hipGetLastError() == hipSuccess ? ENSLAM_OK : ENSLAM_ELAUNCH;
}

int enslam_event_filter_compact(const double* t, const uint16_t* x, const uint16_t* y, const uint8_t* p, int64_t N,
                                const uint8_t* cls, const int64_t* ends, int64_t n_out, double* t_out, uint16_t* x_out,
                                uint16_t* y_out, uint8_t* p_out, void* stream) {
    if (N < 0 || n_out < 0 || n_out > N) return ENSLAM_EINVAL;
    if (N > 0 && (!t || !x || !y || !p || !cls || !ends)) return ENSLAM_EINVAL;
    if (n_out > 0 && (!t_out || !x_out || !y_out || !p_out)) return ENSLAM_EINVAL;
    if (ef_misaligned(t, 8) || ef_misaligned(x, 2) || ef_misaligned(y, 2) || ef_misaligned(ends, 8) || ef_misaligned(t_out, 8) ||
        ef_misaligned(x_out, 2) || ef_misaligned(y_out, 2))
        return ENSLAM_EINVAL;
    if (N > EF_MAX_EVENTS) return ENSLAM_EUNSUPPORTED;
    if (N == 0 || n_out == 0) return ENSLAM_OK;
    EfCompactArgs A;
    A.t = t; A.x = x; A.y = y; A.p = p; A.N = N; A.n_out = n_out; A.cls = cls; A.ends = ends; A.to = t_out; A.xo = x_out;
    A.yo = y_out; A.po = p_out;
    event_filter_compact_kernel<<<ef_blocks(N), EF_BLOCK, 0, (hipStream_t)stream>>>(A);
    return hipGetLastError() == hipSuccess ? ENSLAM_OK : ENSLAM_ELAUNCH;
}

}  // extern "C"
