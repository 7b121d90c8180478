// Event-camera simulator (enslam_event_sim_images, enslam_event_sim_boxroom; enslam_hip.h holds the model): a contrast-
// threshold sensor.  Per pixel one reference level L_ref (float64, carried between intervals); an interval is visited at K
// sub-steps, and at each the pixel fires floor(|L - L_ref| / C) events of the sign of the change and moves L_ref by as many
// thresholds.
//
// Two routes to L at a sub-step, one kernel each, one thread per pixel, one launch per interval:
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
// The per-pixel helpers live in event_sim_core.hpp, shared with event_stream.hip (the same sensor with time-stamped events);
// they are host-callable too, so that a CPU build can step through one pixel.
#include "../../include/enslam_hip.h"
#include "common.hpp"

#include "event_sim_core.hpp"

namespace {

__global__ __launch_bounds__(ES_BLOCK) void event_sim_images_kernel(EsImageArgs A) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= A.c.W || y >= A.c.H) return;
    es_image_pixel(A, y, x);
}

__global__ __launch_bounds__(ES_BLOCK) void event_sim_boxroom_kernel(EsRoomArgs A) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= A.c.W || y >= A.c.H) return;
    es_room_pixel_interval(A, y, x);
}

}  // namespace

extern "C" {

int64_t enslam_event_sim_plan_bytes(void) { return (int64_t)sizeof(enslam_event_sim_plan); }

int enslam_event_sim_max_substeps(void) { return ES_MAX_SUBSTEPS; }

int enslam_event_sim_images(const enslam_event_sim_plan* plan, const uint8_t* prev, const uint8_t* cur, const double* lut,
                            const double* L_prev, const double* L_cur, const double* c_pos_map, const double* c_neg_map,
                            double* L_ref, uint8_t* events, void* stream) {
    EsImageArgs A;
    const int rc = es_image_args(plan, prev, cur, lut, L_prev, L_cur, c_pos_map, c_neg_map, L_ref, events, A);
    if (rc != ENSLAM_OK) return rc;
    event_sim_images_kernel<<<es_grid(A.c), ES_BLOCK, 0, (hipStream_t)stream>>>(A);
    return hipGetLastError() == hipSuccess ? ENSLAM_OK : ENSLAM_ELAUNCH;
}

int enslam_event_sim_boxroom(const enslam_event_sim_plan* plan, const double* poses, const double* c_pos_map,
                             const double* c_neg_map, double* L_ref, uint8_t* events, double* color_out, float* depth_out,
                             void* stream) {
    EsRoomArgs A;
    const int rc = es_room_args(plan, poses, c_pos_map, c_neg_map, L_ref, events, color_out, depth_out, A);
    if (rc != ENSLAM_OK) return rc;
    event_sim_boxroom_kernel<<<es_grid(A.c), ES_BLOCK, 0, (hipStream_t)stream>>>(A);
    return hipGetLastError() == hipSuccess ? ENSLAM_OK : ENSLAM_ELAUNCH;
}

}  // extern "C"
