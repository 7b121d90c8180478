// Event-camera simulator (enslam_event_sim_images, enslam_event_sim_boxroom; enslam_hip.h holds the model): a contrast-
// threshold sensor.  Per pixel one reference level L_ref (float64, carried between intervals); an interval is visited at K
// sub-steps, and at each the pixel fires floor(|L - L_ref| / C) events of the sign of the change and moves L_ref by as many
// thresholds.
//
// Two routes to L at a sub-step (the sources of event_sim_core.hpp), one thread per pixel, one launch per interval:
//   images   L_a, L_b of two decoded uint8 images (a 256-entry host-computed table for grey, luminance + log for RGB, or two
//            host-computed level images), sub-step s at L_a + (s / K) * (L_b - L_a)
//   boxroom  synthetic.BoxRoom rendered in the kernel at K host-interpolated poses; the frame of the last pose (colour
//            float64, depth float32) is written as well when asked for, so a simulated frame costs this one launch
//
// Launch shape (as frame_prep.hip): 64 x 4 pixel tiles, a wave = 64 consecutive pixels of one row.  A wave's event store is
// one 2-byte store per lane into 128 consecutive bytes; the colour store is three 8-byte stores per lane that together fill
// 1536 consecutive bytes (whole cache lines, merged in L2); L_ref is read and written once, 512 bytes per wave.  Counts and
// L_ref live in registers across the sub-steps.  The poses are read at a wave-uniform address from a const __restrict__
// kernel-argument pointer: scalar loads, one copy per wave.  No LDS, no atomics, no cross-lane traffic: two runs are
// bit-identical.
//
// Precision: float64 throughout, every operation in the order the model states (-ffp-contract=off: no fused multiply-adds).
// What is not pinned bit for bit is the device's sin and log (an ulp or two of the host's); the grey table and the host-level
// option keep them out of the images route where a test wants bit equality.
// The sources, the per-pixel driver and the kernel live in event_sim_core.hpp, shared with event_stream.hip (the same sensor
// with time-stamped events) and event_noise.hip (the noisy sensor); this file adds the frame pass and its two entries.
#include "../../include/enslam_hip.h"
#include "common.hpp"

#include "event_sim_core.hpp"

namespace {

// frame: the count image of the interval and the new L_ref; aware of the first frame (init: no events, L_ref := L)
struct EsFramePass {
    static constexpr bool STAMPS = false, FRAME = true;
    using State = EsSensor;
    ES_HD void begin(const EsCommon& C, int64_t o, State& S, double& cp, double& cn) const { es_load(C, o, S, cp, cn); }
    ES_HD void substep(const EsCommon& C, State& S, int64_t, int, int, int, double cp, double cn, double, double L) const {
        if (!C.init) es_update(S, L, cp, cn);
    }
    ES_HD void end(const EsCommon& C, int64_t o, const State& S, double L_last) const { es_store(C, o, S, L_last); }
};

}  // namespace

extern "C" {

int64_t enslam_event_sim_plan_bytes(void) { return (int64_t)sizeof(enslam_event_sim_plan); }

int enslam_event_sim_max_substeps(void) { return ES_MAX_SUBSTEPS; }

int enslam_event_sim_images(const enslam_event_sim_plan* plan, const uint8_t* prev, const uint8_t* cur, const double* lut,
                            const double* L_prev, const double* L_cur, const double* c_pos_map, const double* c_neg_map,
                            double* L_ref, uint8_t* events, void* stream) {
    EsImageSrc A;
    const int rc = es_image_args(plan, prev, cur, lut, L_prev, L_cur, c_pos_map, c_neg_map, L_ref, events, A);
    return rc != ENSLAM_OK ? rc : es_launch(A, EsFramePass{}, stream);
}

int enslam_event_sim_boxroom(const enslam_event_sim_plan* plan, const double* poses, const double* c_pos_map,
                             const double* c_neg_map, double* L_ref, uint8_t* events, double* color_out, float* depth_out,
                             void* stream) {
    EsRoomSrc A;
    const int rc = es_room_args(plan, poses, false, c_pos_map, c_neg_map, L_ref, events, color_out, depth_out, A);
    return rc != ENSLAM_OK ? rc : es_launch(A, EsFramePass{}, stream);
}

}  // extern "C"
