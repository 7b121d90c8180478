// The event-camera simulator's kernel, written once (enslam_hip.h holds the model).  A launch is a level SOURCE times a PASS:
//   sources  where a pixel's level at sub-step s = 1..K comes from: EsImageSrc (two decoded images or two host level images)
//            and EsRoomSrc (the analytic room rendered at K poses), both in this file
//   passes   what is done with the levels, each beside the entries that launch it: EsFramePass (event_sim.hip), EsCountPass
//            and EsEmitPass (event_stream.hip), EnPass<MODE> (event_noise.hip)
// es_pixel holds the only sub-step loop, event_pixels_kernel the only tile arithmetic, es_launch the only launch.  The
// arithmetic the passes share is here as well, each piece written once so that all files round alike: the sensor update, the
// level of an image pixel, the analytic room, and the fraction and time of a crossing.  Everything per pixel is host-callable
// too, so that a CPU build can step through one pixel.
#pragma once
#include <cmath>
#include <cstdint>
#include <hip/hip_runtime.h>
#include "../../include/enslam_hip.h"

namespace {

constexpr int ES_BLOCK = 256;
constexpr int ES_MAX_SUBSTEPS = 64;
constexpr int64_t ES_MAX_PIXELS = (int64_t)1 << 28;

#define ES_HD __host__ __device__ __forceinline__

struct EsSensor {                   // one pixel's state across the sub-steps of an interval
    double ref, pos, neg;
};

// the per-pixel update of the model at one sub-step
ES_HD void es_update(EsSensor& S, double L, double cp, double cn) {
    const double d = L - S.ref;
    if (d >= cp) {
        const double n = floor(d / cp);
        S.pos += n;
        S.ref += n * cp;
    } else if (-d >= cn) {
        const double n = floor(-d / cn);
        S.neg += n;
        S.ref -= n * cn;
    }
}

ES_HD uint8_t es_sat(double n) { return n >= 255.0 ? (uint8_t)255 : (uint8_t)n; }

ES_HD double es_luminance(double r, double g, double b) { return (0.299 * r + 0.587 * g) + 0.114 * b; }

struct EsCommon {
    int32_t H, W, K, init;
    double eps, c_pos, c_neg;
    const double* c_pos_map;
    const double* c_neg_map;
    double* L_ref;
    uint8_t* events;
};

// sensor state in, sensor state and counts out: the head of every pass, the tail of those that write the count image
ES_HD void es_load(const EsCommon& C, int64_t o, EsSensor& S, double& cp, double& cn) {
    S.ref = C.init ? 0.0 : C.L_ref[o];
    S.pos = 0.0;
    S.neg = 0.0;
    cp = C.c_pos_map ? C.c_pos_map[o] : C.c_pos;
    cn = C.c_neg_map ? C.c_neg_map[o] : C.c_neg;
}

ES_HD void es_store(const EsCommon& C, int64_t o, const EsSensor& S, double L_last) {
    C.L_ref[o] = C.init ? L_last : S.ref;
    if (C.events) {
        const unsigned neg = C.init ? 0u : es_sat(S.neg), pos = C.init ? 0u : es_sat(S.pos);
        reinterpret_cast<uint16_t*>(C.events)[o] = (uint16_t)(neg | (pos << 8));       // (-, +) as one 2-byte store
    }
}

// ---- the two level sources ----------------------------------------------------------------------------------------------------
// A source has a per-pixel record Pixel, begin (fills it), start (the level the first sub-step starts from; evaluated only by
// the passes that stamp events), level (of sub-step s = 1..K) and frame (what the source writes itself behind a pass that
// asks for it, from the last sub-step).

// images: L_a and L_b of the two frames, sub-step s at L_a + (s / K) * (L_b - L_a)
struct EsImageSrc {
    EsCommon c;
    int32_t channels;
    const uint8_t* prev;
    const uint8_t* cur;
    const double* lut;
    const double* L_prev;
    const double* L_cur;

    struct Pixel {
        double La, dL;
    };
    ES_HD void begin(Pixel& p, int64_t o) const;
    ES_HD double start(const Pixel& p, int, int) const { return p.La; }
    ES_HD double level(const Pixel& p, int s, int, int) const { return p.La + ((double)s / (double)c.K) * p.dL; }
    ES_HD void frame(const Pixel&, int64_t) const {}
};

ES_HD double es_image_level(const EsImageSrc& A, const uint8_t* img, int64_t o) {
    if (A.channels == 1) return A.lut[img[o]];
    const uint8_t* s = img + 3 * o;
    return log(es_luminance((double)s[0] / 255.0, (double)s[1] / 255.0, (double)s[2] / 255.0) + A.c.eps);
}

ES_HD void EsImageSrc::begin(Pixel& p, int64_t o) const {
    p.La = L_prev ? L_prev[o] : es_image_level(*this, prev, o);
    const double Lb = L_cur ? L_cur[o] : es_image_level(*this, cur, o);
    p.dL = Lb - p.La;
}

// boxroom: synthetic.BoxRoom rendered in the kernel at the pose of every sub-step.  The poses are read at a wave-uniform
// address from a kernel-argument pointer: scalar loads, one copy per wave.
struct EsRoomSrc {
    EsCommon c;
    double fx, fy, cx, cy;
    double room_lo[3], room_hi[3], box_lo[3], box_hi[3];
    double freq[9], phase[3];
    int32_t has_box;
    const double* pose_prev;        // [12], the previous frame's pose; NULL where no pass asks for `start`
    const double* poses;            // [K,12], the sub-steps
    double* color_out;              // [H,W,3] or NULL
    float* depth_out;               // [H,W] or NULL

    struct Pixel {                  // colour and ray parameter under the last pose rendered
        double col[3], t;
    };
    ES_HD void begin(Pixel& p, int64_t) const { p.col[0] = p.col[1] = p.col[2] = p.t = 0.0; }
    ES_HD double start(Pixel& p, int y, int x) const;
    ES_HD double level(Pixel& p, int s, int y, int x) const;
    ES_HD void frame(const Pixel& p, int64_t o) const {
        if (color_out) {
            double* co = color_out + 3 * o;
            co[0] = p.col[0]; co[1] = p.col[1]; co[2] = p.col[2];
            depth_out[o] = (float)p.t;
        }
    }
};

// BoxRoom.render of one pixel under the pose P (the 12 values of c2w[:3,:4], row-major): colour and the ray parameter
ES_HD void es_room_pixel(const EsRoomSrc& A, const double* __restrict__ P, int y, int x, double (&col)[3], double& t) {
    const double dir[3] = {((double)x - A.cx) / A.fx, -((double)y - A.cy) / A.fy, -1.0};
    double o[3], d[3], dc[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        d[a] = (dir[0] * P[4 * a] + dir[1] * P[4 * a + 1]) + dir[2] * P[4 * a + 2];
        o[a] = P[4 * a + 3];
        dc[a] = fabs(d[a]) < 1e-12 ? 1e-12 : d[a];              // BoxRoom.intersect's clamp (the hit point uses d itself)
    }
    double t_wall = 0.0, t1 = 0.0, t2 = 0.0;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double u = (A.room_lo[a] - o[a]) / dc[a], v = (A.room_hi[a] - o[a]) / dc[a];
        const double far = u > v ? u : v;
        t_wall = a == 0 ? far : (far < t_wall ? far : t_wall);
    }
    t = t_wall;
    if (A.has_box) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const double u = (A.box_lo[a] - o[a]) / dc[a], v = (A.box_hi[a] - o[a]) / dc[a];
            const double lo = u < v ? u : v, hi = u > v ? u : v;
            t1 = a == 0 ? lo : (lo > t1 ? lo : t1);
            t2 = a == 0 ? hi : (hi < t2 ? hi : t2);
        }
        if (t1 < t2 && t1 > 0.0 && t1 < t_wall) t = t1;
    }
    double p[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) p[a] = o[a] + d[a] * t;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const double arg = ((p[0] * A.freq[3 * c] + p[1] * A.freq[3 * c + 1]) + p[2] * A.freq[3 * c + 2]) + A.phase[c];
        col[c] = 0.5 + 0.45 * sin(arg);
    }
}

ES_HD double es_room_level(const EsRoomSrc& A, EsRoomSrc::Pixel& p, const double* __restrict__ P, int y, int x) {
    es_room_pixel(A, P, y, x, p.col, p.t);
    return log(es_luminance(p.col[0], p.col[1], p.col[2]) + A.c.eps);
}

ES_HD double EsRoomSrc::start(Pixel& p, int y, int x) const { return es_room_level(*this, p, pose_prev, y, x); }
ES_HD double EsRoomSrc::level(Pixel& p, int s, int y, int x) const { return es_room_level(*this, p, poses + 12 * (s - 1), y, x); }

// ---- one pixel, one kernel, one launch ----------------------------------------------------------------------------------------
// A pass has a per-pixel State, begin (loads it and the pixel's thresholds), substep (s of K at the level L, the level before
// being L_prev) and end (stores; L_last is the level of sub-step K).  STAMPS says whether it reads L_prev, FRAME whether the
// source's frame is written behind it.
//
// The loop is not unrolled: its trip count is a kernel argument, and copies of the room's render only cost registers
// (DESIGN.md 4.S has the resource table).
template <class Src, class Pass>
ES_HD void es_pixel(const Src& src, const Pass& pass, int y, int x) {
    const EsCommon& C = src.c;
    const int64_t o = (int64_t)y * C.W + x;
    typename Src::Pixel px;
    typename Pass::State st;
    double cp, cn;
    src.begin(px, o);
    pass.begin(C, o, st, cp, cn);
    double L_prev = Pass::STAMPS ? src.start(px, y, x) : 0.0, L = L_prev;
#pragma clang loop unroll(disable)
    for (int s = 1; s <= C.K; ++s) {
        L = src.level(px, s, y, x);
        pass.substep(C, st, o, y, x, s, cp, cn, L_prev, L);
        L_prev = L;
    }
    pass.end(C, o, st, L);
    if (Pass::FRAME) src.frame(px, o);
}

// 64 x 4 pixel tiles, a wave = 64 consecutive pixels of one row
template <class Src, class Pass>
__global__ __launch_bounds__(ES_BLOCK) void event_pixels_kernel(Src src, Pass pass) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= src.c.W || y >= src.c.H) return;
    es_pixel(src, pass, y, x);
}

template <class Src, class Pass>
inline int es_launch(const Src& src, const Pass& pass, void* stream) {
    const dim3 grid((unsigned)((src.c.W + 63) / 64), (unsigned)((src.c.H + 3) / 4));
    event_pixels_kernel<<<grid, ES_BLOCK, 0, (hipStream_t)stream>>>(src, pass);
    return hipGetLastError() == hipSuccess ? ENSLAM_OK : ENSLAM_ELAUNCH;
}

// ---- what the entries check before they launch (no device work) ---------------------------------------------------------------
inline bool es_pos_finite(double x) { return x > 0.0 && x - x == 0.0; }
inline bool es_finite(double x) { return x == x && x - x == 0.0; }

// Checks what both routes share and fills C.
inline int es_common(const enslam_event_sim_plan* plan, const double* c_pos_map, const double* c_neg_map, double* L_ref,
              uint8_t* events, EsCommon& C) {
    if (!plan || !L_ref) return ENSLAM_EINVAL;
    const enslam_event_sim_plan& P = *plan;
    if (!events && !P.init) return ENSLAM_EINVAL;
    if ((uintptr_t)events & 1) return ENSLAM_EINVAL;           // a pixel's two counts are stored as one 16-bit word
    if (P.H <= 0 || P.W <= 0 || P.K <= 0) return ENSLAM_EINVAL;
    if (!es_pos_finite(P.eps)) return ENSLAM_EINVAL;
    if (!P.init && ((!c_pos_map && !es_pos_finite(P.c_pos)) || (!c_neg_map && !es_pos_finite(P.c_neg)))) return ENSLAM_EINVAL;
    if (P.K > ES_MAX_SUBSTEPS || (int64_t)P.H * P.W > ES_MAX_PIXELS) return ENSLAM_EUNSUPPORTED;
    C.H = P.H; C.W = P.W; C.K = P.K; C.init = P.init != 0;
    C.eps = P.eps; C.c_pos = P.c_pos; C.c_neg = P.c_neg;
    C.c_pos_map = c_pos_map; C.c_neg_map = c_neg_map;
    C.L_ref = L_ref; C.events = events;
    return ENSLAM_OK;
}

// The images route's checks on top of es_common; fills A.
inline int es_image_args(const enslam_event_sim_plan* plan, const uint8_t* prev, const uint8_t* cur, const double* lut,
                         const double* L_prev, const double* L_cur, const double* c_pos_map, const double* c_neg_map,
                         double* L_ref, uint8_t* events, EsImageSrc& A) {
    const int rc = es_common(plan, c_pos_map, c_neg_map, L_ref, events, A.c);
    if (rc != ENSLAM_OK) return rc;
    if ((L_prev == nullptr) != (L_cur == nullptr)) return ENSLAM_EINVAL;
    if (!L_prev) {
        if (!prev || !cur) return ENSLAM_EINVAL;
        if (plan->channels != 1 && plan->channels != 3) return ENSLAM_EINVAL;
        if (plan->channels == 1 && !lut) return ENSLAM_EINVAL;
    }
    A.channels = plan->channels;
    A.prev = prev; A.cur = cur; A.lut = lut; A.L_prev = L_prev; A.L_cur = L_cur;
    return ENSLAM_OK;
}

// The analytic route's checks on top of es_common; fills A.  poses: [K,12] the sub-steps, or (with_prev) [K+1,12] with the
// previous frame's pose as row 0.
inline int es_room_args(const enslam_event_sim_plan* plan, const double* poses, bool with_prev, const double* c_pos_map,
                        const double* c_neg_map, double* L_ref, uint8_t* events, double* color_out, float* depth_out,
                        EsRoomSrc& A) {
    const int rc = es_common(plan, c_pos_map, c_neg_map, L_ref, events, A.c);
    if (rc != ENSLAM_OK) return rc;
    if (!poses || (color_out == nullptr) != (depth_out == nullptr)) return ENSLAM_EINVAL;
    const enslam_event_sim_plan& P = *plan;
    if (!es_finite(P.fx) || !es_finite(P.fy) || !es_finite(P.cx) || !es_finite(P.cy) || P.fx == 0.0 || P.fy == 0.0)
        return ENSLAM_EINVAL;
    A.fx = P.fx; A.fy = P.fy; A.cx = P.cx; A.cy = P.cy;
    for (int a = 0; a < 3; ++a) {
        A.room_lo[a] = P.room_lo[a]; A.room_hi[a] = P.room_hi[a]; A.box_lo[a] = P.box_lo[a]; A.box_hi[a] = P.box_hi[a];
        A.phase[a] = P.phase[a];
    }
    for (int k = 0; k < 9; ++k) A.freq[k] = P.freq[k];
    A.has_box = P.has_box != 0;
    A.pose_prev = with_prev ? poses : nullptr;
    A.poses = with_prev ? poses + 12 : poses;
    A.color_out = color_out; A.depth_out = depth_out;
    return ENSLAM_OK;
}

// ---- time-stamped events: shared by event_stream.hip and event_noise.hip ------------------------------------------------------
constexpr int64_t ES_COUNT_CAP = (int64_t)1 << 33;      // per-pixel total written by a count pass is limited to this: 2^28
                                                        // pixels cannot overflow the int64 prefix sum, and one pixel at the
                                                        // cap already puts the total above what emit accepts
constexpr int64_t ES_MAX_EVENTS = 2147483647;           // 2^31 - 1

struct EsStreamOut {
    const int64_t* ends;            // [H*W] inclusive prefix sum of the count pass
    int64_t capacity;               // events the four arrays hold
    double t_a, t_b;
    double* t;
    uint16_t* x;
    uint16_t* y;
    uint8_t* p;
};

ES_HD int64_t es_total(const EsSensor& S) {
    const double n = S.pos + S.neg;
    return n >= (double)ES_COUNT_CAP ? ES_COUNT_CAP : (int64_t)n;
}

// the pixel's run [begin, end) in the stream arrays
ES_HD void es_run(const EsStreamOut& O, int64_t o, int64_t& begin, int64_t& end) {
    begin = o ? O.ends[o - 1] : 0;
    end = O.ends[o];
    if (end > O.capacity) end = O.capacity;
    if (begin < 0) begin = 0;
}

// Event k of a sub-step crosses X_k = R +- k * C at f_k = (X_k - L_prev) / D, D = L - L_prev, limited to [0, 1] (a quotient
// that is not a number counts as 0).
ES_HD double es_cross_fraction(double R, double k, double c, bool up, double L_prev, double D) {
    const double step = k * c;
    const double X = up ? R + step : R - step;
    double f = (X - L_prev) / D;
    if (!(f >= 0.0)) f = 0.0;
    if (f > 1.0) f = 1.0;
    return f;
}

// the time of the fraction f of sub-step s (1-based) of K: t_a + (((s - 1) + f) / K) * (t_b - t_a)
ES_HD double es_stamp(const EsStreamOut& O, int s, int K, double f) {
    const double u = ((double)(s - 1) + f) / (double)K;
    return O.t_a + u * (O.t_b - O.t_a);
}

ES_HD void es_put(const EsStreamOut& O, int64_t at, double t, int y, int x, bool up) {
    O.t[at] = t;
    O.x[at] = (uint16_t)x;
    O.y[at] = (uint16_t)y;
    O.p[at] = up ? (uint8_t)1 : (uint8_t)0;
}

// what the stream entries add to the plan's checks: no first-frame mode, coordinates that fit uint16
inline int es_stream_plan(const enslam_event_sim_plan* plan) {
    if (!plan) return ENSLAM_EINVAL;
    if (plan->init) return ENSLAM_EINVAL;
    if (plan->H > 65536 || plan->W > 65536) return ENSLAM_EUNSUPPORTED;
    return ENSLAM_OK;
}

// The head of the four count entries: es_stream_plan, the counts, then the route's own checks.  A count pass only reads
// L_ref and has no event image (es_store is never called): `counts` stands in for it in the checks alone.
inline int es_image_count_args(const enslam_event_sim_plan* plan, const uint8_t* prev, const uint8_t* cur, const double* lut,
                               const double* L_prev, const double* L_cur, const double* c_pos_map, const double* c_neg_map,
                               const double* L_ref, int64_t* counts, EsImageSrc& A) {
    int rc = es_stream_plan(plan);
    if (rc != ENSLAM_OK) return rc;
    if (!counts) return ENSLAM_EINVAL;
    rc = es_image_args(plan, prev, cur, lut, L_prev, L_cur, c_pos_map, c_neg_map, const_cast<double*>(L_ref),
                       reinterpret_cast<uint8_t*>(counts), A);
    A.c.events = nullptr;
    return rc;
}

inline int es_room_count_args(const enslam_event_sim_plan* plan, const double* poses, bool with_prev, const double* c_pos_map,
                              const double* c_neg_map, const double* L_ref, int64_t* counts, EsRoomSrc& A) {
    int rc = es_stream_plan(plan);
    if (rc != ENSLAM_OK) return rc;
    if (!counts) return ENSLAM_EINVAL;
    rc = es_room_args(plan, poses, with_prev, c_pos_map, c_neg_map, const_cast<double*>(L_ref), reinterpret_cast<uint8_t*>(counts),
                      nullptr, nullptr, A);
    A.c.events = nullptr;
    return rc;
}

inline int es_stream_out(const int64_t* ends, int64_t total, double t_a, double t_b, double* t, uint16_t* x, uint16_t* y,
                         uint8_t* p, EsStreamOut& O) {
    if (!ends || total < 0) return ENSLAM_EINVAL;
    if (total > 0 && (!t || !x || !y || !p)) return ENSLAM_EINVAL;
    if (!es_finite(t_a) || !es_finite(t_b) || t_b < t_a) return ENSLAM_EINVAL;
    if (total > ES_MAX_EVENTS) return ENSLAM_EUNSUPPORTED;
    O.ends = ends; O.capacity = total; O.t_a = t_a; O.t_b = t_b;
    O.t = t; O.x = x; O.y = y; O.p = p;
    return ENSLAM_OK;
}

}  // namespace
