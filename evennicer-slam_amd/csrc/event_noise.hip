// The noisy event sensor (enslam_event_noisy_*; enslam_hip.h holds the model): refractory period (ESIM's rule), leak (v2e's
// rule) and shot noise on top of the sensor of event_sim.hip and the time stamps of event_stream.hip.
//
// One more pass of the kernel of event_sim_core.hpp (one thread per pixel on its 64 x 4 tile, either source).  A pixel walks
// its sub-steps; at each it leaks, runs the closed form es_update (the one event_sim.hip calls), draws its at most two
// shot-noise candidates from one Philox4x32-10 block keyed by (seed) and counted by (pixel, interval, sub-step, 0), and then
// walks the signal candidates k = 1..n in order with the noise candidates held in registers and interleaved where their times
// fall; every candidate passes the refractory filter t - t_last >= rho.  The fraction and the time of a candidate are
// es_cross_fraction / es_stamp of event_sim_core.hpp, the ones event_stream.hip calls.  en_substep is one function templated
// on "count only" or "emit", so both passes decide alike (a sub-step walks at most EN_WALK_CAP candidates; a pixel beyond
// reports the count cap, which the emit entry's total refuses); EnPass<MODE> wraps it, three instances per source:
//   count  reads both states, writes the emitted total per pixel (int64)
//   image  one launch: writes the uint8 image of emitted events and both states, no stream
//   emit   as image, and the pixel's run at its offset; every store is guarded by the end of the run and by the capacity
// No LDS (group segment 0 in all six instances), no atomics, no cross-lane traffic: two runs are bit-identical.  Philox is
// 32-bit integer arithmetic (__umulhi and the low product); with q = 0 the block is skipped by a branch on a kernel argument,
// uniform across the launch.  No local array is indexed dynamically, so nothing goes to scratch.
#include "../../include/enslam_hip.h"
#include "common.hpp"

#include "event_sim_core.hpp"

namespace {

// A sub-step walks at most this many signal candidates of a pixel: the walk is serial, and a threshold that is tiny against
// the level change would otherwise keep one launch busy for 2^31 turns per thread.  256 times what the uint8 image can show.
constexpr int64_t EN_WALK_CAP = 65536;

struct EnArgs {
    double rho, g, q;               // refractory period (s), leak per sub-step in thresholds, shot probability per sub-step
    uint32_t key0, key1, interval;
    const double* t_last_in;        // [H,W]
    double* t_last_out;             // [H,W] or NULL (count)
};

ES_HD uint32_t en_mulhi(uint32_t a, uint32_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __umulhi(a, b);
#else
    return (uint32_t)(((uint64_t)a * (uint64_t)b) >> 32);
#endif
}

// Philox4x32-10 (Salmon et al., SC 2011): counter c[4], key k[2]; the counter is replaced by the block
ES_HD void en_philox(uint32_t& c0, uint32_t& c1, uint32_t& c2, uint32_t& c3, uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = en_mulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const uint32_t hi1 = en_mulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0;
        c1 = lo1;
        c2 = hi0 ^ c3 ^ k1;
        c3 = lo0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
}

ES_HD double en_uniform(uint32_t w) { return ((double)w + 0.5) * (1.0 / 4294967296.0); }     // exact in float64

struct EnPixel {                    // what a pixel carries through its sub-steps
    EsSensor S;                     // ref: L_ref; pos / neg: EMITTED events
    double t_last;
    int64_t at, end;
    bool over;                      // a sub-step had more candidates than one walk takes
};

// one candidate through the refractory filter
template <bool EMIT>
ES_HD void en_fire(const EnArgs& N, const EsStreamOut& O, EnPixel& P, int y, int x, double t, bool up) {
    if (t - P.t_last >= N.rho) {
        P.t_last = t;
        P.S.pos += up ? 1.0 : 0.0;                  // both counts every time: a select between the two members' addresses
        P.S.neg += up ? 0.0 : 1.0;                  // would move the whole EnPixel out of registers (adding 0.0 is exact)
        if (EMIT) {
            if (P.at < P.end) es_put(O, P.at, t, y, x, up);
            ++P.at;
        }
    }
}

// Sub-step s (1-based) of K at the level L, the level before being L_prev.
template <bool EMIT>
ES_HD void en_substep(const EnArgs& N, const EsStreamOut& O, EnPixel& P, int64_t o, int y, int x, int s, int K, double cp, double cn,
                      double L_prev, double L) {
    if (N.g > 0.0) P.S.ref = P.S.ref - N.g * cp;
    const double R = P.S.ref;
    EsSensor U;
    U.ref = R; U.pos = 0.0; U.neg = 0.0;
    es_update(U, L, cp, cn);
    P.S.ref = U.ref;
    const bool up = U.pos > 0.0;
    double n = up ? U.pos : U.neg;
    if (n > (double)EN_WALK_CAP) { n = (double)EN_WALK_CAP; P.over = true; }
    const double c = up ? cp : cn, D = L - L_prev;
    // the noise candidates in the order they leave: a, then b
    bool has_a = false, has_b = false, up_a = false, up_b = true;
    double t_a = 0.0, t_b = 0.0;
    if (N.q > 0.0) {
        uint32_t w0 = (uint32_t)o, w1 = N.interval, w2 = (uint32_t)s, w3 = 0u;
        en_philox(w0, w1, w2, w3, N.key0, N.key1);
        const bool has_neg = en_uniform(w0) < N.q, has_pos = en_uniform(w2) < N.q;
        const double t_neg = es_stamp(O, s, K, en_uniform(w1)), t_pos = es_stamp(O, s, K, en_uniform(w3));
        const bool pos_first = has_pos && (!has_neg || t_pos < t_neg);
        has_a = has_neg || has_pos;
        has_b = has_neg && has_pos;
        up_a = pos_first;
        up_b = !pos_first;
        t_a = pos_first ? t_pos : t_neg;
        t_b = pos_first ? t_neg : t_pos;
    }
    for (double k = 1.0; k <= n; k += 1.0) {
        const double t = es_stamp(O, s, K, es_cross_fraction(R, k, c, up, L_prev, D));
        if (has_a && t_a < t) {
            en_fire<EMIT>(N, O, P, y, x, t_a, up_a);
            has_a = false;
            if (has_b && t_b < t) {
                en_fire<EMIT>(N, O, P, y, x, t_b, up_b);
                has_b = false;
            }
        } else if (!has_a && has_b && t_b < t) {
            en_fire<EMIT>(N, O, P, y, x, t_b, up_b);
            has_b = false;
        }
        en_fire<EMIT>(N, O, P, y, x, t, up);
    }
    if (has_a) en_fire<EMIT>(N, O, P, y, x, t_a, up_a);
    if (has_b) en_fire<EMIT>(N, O, P, y, x, t_b, up_b);
}

enum { EN_COUNT = 0, EN_IMAGE = 1, EN_EMIT = 2 };

template <int MODE>
struct EnPass {
    static constexpr bool STAMPS = true, FRAME = false;
    using State = EnPixel;
    EnArgs N;
    EsStreamOut O;
    int64_t* counts;                // [H,W] (count) or NULL
    ES_HD void begin(const EsCommon& C, int64_t o, State& P, double& cp, double& cn) const {
        es_load(C, o, P.S, cp, cn);
        P.t_last = N.t_last_in[o];
        P.at = 0; P.end = 0; P.over = false;
        if (MODE == EN_EMIT) es_run(O, o, P.at, P.end);
    }
    ES_HD void substep(const EsCommon& C, State& P, int64_t o, int y, int x, int s, double cp, double cn, double L_prev, double L) const {
        en_substep<MODE == EN_EMIT>(N, O, P, o, y, x, s, C.K, cp, cn, L_prev, L);
    }
    ES_HD void end(const EsCommon& C, int64_t o, const State& P, double L_last) const {
        if (MODE == EN_COUNT) {
            counts[o] = P.over ? ES_COUNT_CAP : es_total(P.S);
        } else {
            es_store(C, o, P.S, L_last);
            N.t_last_out[o] = P.t_last;
        }
    }
};

inline bool en_rate(double v) { return v >= 0.0 && v - v == 0.0; }      // not negative, finite

int en_args(const enslam_event_noise* noise, const double* t_last_in, double* t_last_out, EnArgs& N) {
    if (!noise || !t_last_in) return ENSLAM_EINVAL;
    if (!en_rate(noise->refractory) || !en_rate(noise->leak) || !en_rate(noise->shot) || noise->shot > 1.0) return ENSLAM_EINVAL;
    N.rho = noise->refractory; N.g = noise->leak; N.q = noise->shot;
    N.key0 = (uint32_t)(noise->seed & 0xFFFFFFFFull); N.key1 = (uint32_t)(noise->seed >> 32);
    N.interval = noise->interval;
    N.t_last_in = t_last_in; N.t_last_out = t_last_out;
    return ENSLAM_OK;
}

int en_count_out(double t_a, double t_b, EsStreamOut& O) {
    if (!es_finite(t_a) || !es_finite(t_b) || t_b < t_a) return ENSLAM_EINVAL;
    O.ends = nullptr; O.capacity = 0; O.t_a = t_a; O.t_b = t_b;
    O.t = nullptr; O.x = nullptr; O.y = nullptr; O.p = nullptr;
    return ENSLAM_OK;
}

// the five stream pointers: all of them (t, x, y, p may be NULL together while total = 0), or none with total = 0 -- the
// count-image-only form (image = true)
int en_emit_out(const int64_t* ends, int64_t total, double t_a, double t_b, double* t, uint16_t* x, uint16_t* y, uint8_t* p,
                EsStreamOut& O, bool& image) {
    const int given = (t != nullptr) + (x != nullptr) + (y != nullptr) + (p != nullptr);
    if (given != 0 && given != 4) return ENSLAM_EINVAL;
    image = !ends;
    if (image) {
        if (given || total != 0) return ENSLAM_EINVAL;
        return en_count_out(t_a, t_b, O);
    }
    return es_stream_out(ends, total, t_a, t_b, t, x, y, p, O);
}

// what the two count entries check behind their source, in this order; fills the pass
int en_count_pass(const enslam_event_noise* noise, const double* t_last, double t_a, double t_b, int64_t* counts, EnPass<EN_COUNT>& E) {
    const int rc = en_args(noise, t_last, nullptr, E.N);
    if (rc != ENSLAM_OK) return rc;
    E.counts = counts;
    return en_count_out(t_a, t_b, E.O);
}

// what the two emit entries check behind their source, in this order, and the launch of the form the pointers ask for
template <class Src>
int en_launch_emit(const Src& A, const enslam_event_noise* noise, double* t_last, const int64_t* ends, int64_t total, double t_a,
                   double t_b, double* t, uint16_t* x, uint16_t* y, uint8_t* p, void* stream) {
    EnPass<EN_EMIT> E;
    bool image = false;
    int rc = en_args(noise, t_last, t_last, E.N);
    if (rc != ENSLAM_OK) return rc;
    rc = en_emit_out(ends, total, t_a, t_b, t, x, y, p, E.O, image);
    if (rc != ENSLAM_OK) return rc;
    E.counts = nullptr;
    return image ? es_launch(A, EnPass<EN_IMAGE>{E.N, E.O, nullptr}, stream) : es_launch(A, E, stream);
}

}  // namespace

extern "C" {

int64_t enslam_event_noise_bytes(void) { return (int64_t)sizeof(enslam_event_noise); }

int enslam_event_noisy_images_count(const enslam_event_sim_plan* plan, const uint8_t* prev, const uint8_t* cur,
                                    const double* lut, const double* L_prev, const double* L_cur, const double* c_pos_map,
                                    const double* c_neg_map, const double* L_ref, int64_t* counts,
                                    const enslam_event_noise* noise, double t_a, double t_b, const double* t_last, void* stream) {
    EsImageSrc A;
    EnPass<EN_COUNT> E;
    int rc = es_image_count_args(plan, prev, cur, lut, L_prev, L_cur, c_pos_map, c_neg_map, L_ref, counts, A);
    if (rc != ENSLAM_OK) return rc;
    rc = en_count_pass(noise, t_last, t_a, t_b, counts, E);
    return rc != ENSLAM_OK ? rc : es_launch(A, E, stream);
}

int enslam_event_noisy_images_emit(const enslam_event_sim_plan* plan, const uint8_t* prev, const uint8_t* cur,
                                   const double* lut, const double* L_prev, const double* L_cur, const double* c_pos_map,
                                   const double* c_neg_map, double* L_ref, uint8_t* events, const int64_t* ends, int64_t total,
                                   double t_a, double t_b, double* t, uint16_t* x, uint16_t* y, uint8_t* p,
                                   const enslam_event_noise* noise, double* t_last, void* stream) {
    int rc = es_stream_plan(plan);
    if (rc != ENSLAM_OK) return rc;
    EsImageSrc A;
    rc = es_image_args(plan, prev, cur, lut, L_prev, L_cur, c_pos_map, c_neg_map, L_ref, events, A);
    return rc != ENSLAM_OK ? rc : en_launch_emit(A, noise, t_last, ends, total, t_a, t_b, t, x, y, p, stream);
}

// poses: [K+1,12], row 0 the previous frame's (rendered for L_prev only), rows 1..K the sub-steps -- in both entries
int enslam_event_noisy_boxroom_count(const enslam_event_sim_plan* plan, const double* poses, const double* c_pos_map,
                                     const double* c_neg_map, const double* L_ref, int64_t* counts,
                                     const enslam_event_noise* noise, double t_a, double t_b, const double* t_last, void* stream) {
    EsRoomSrc A;
    EnPass<EN_COUNT> E;
    int rc = es_room_count_args(plan, poses, true, c_pos_map, c_neg_map, L_ref, counts, A);
    if (rc != ENSLAM_OK) return rc;
    rc = en_count_pass(noise, t_last, t_a, t_b, counts, E);
    return rc != ENSLAM_OK ? rc : es_launch(A, E, stream);
}

int enslam_event_noisy_boxroom_emit(const enslam_event_sim_plan* plan, const double* poses, const double* c_pos_map,
                                    const double* c_neg_map, double* L_ref, uint8_t* events, const int64_t* ends, int64_t total,
                                    double t_a, double t_b, double* t, uint16_t* x, uint16_t* y, uint8_t* p,
                                    const enslam_event_noise* noise, double* t_last, void* stream) {
    int rc = es_stream_plan(plan);
    if (rc != ENSLAM_OK) return rc;
    EsRoomSrc A;
    rc = es_room_args(plan, poses, true, c_pos_map, c_neg_map, L_ref, events, nullptr, nullptr, A);
    return rc != ENSLAM_OK ? rc : en_launch_emit(A, noise, t_last, ends, total, t_a, t_b, t, x, y, p, stream);
}

}  // extern "C"
