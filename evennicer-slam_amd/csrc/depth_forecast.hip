// Depth forecast: a measured depth image forward-warped into another camera pose and another image size -- the guidance
// depth of the tracker's reduced-resolution render on a frame for which the sensor delivered no RGB-D image (slam.py, schedule
// 'reference' with event.depth_on_event_frames: 'forecast').  A z-buffered point splat, of the family of mesh_depth.hip.
//
// THE MODEL.  depth is float32 [H,W]; fx, fy, cx, cy are the intrinsics of the full-resolution image; M is the 3 x 4 float64
// matrix (row-major, M[4 r + c]) that takes source-camera coordinates to target-camera coordinates (both cameras look down -z);
// the output is float32 [Ho,Wo].  Every operation below is a float64 operation in the order written, none contracted.
//
//   source   pixel (row j, column i) with d = depth[j,i] finite and > 0 is the camera-space point
//                p = (d px, d py, -d),   px = (i - cx) / fx,   py = -(j - cy) / fy.
//            Zeros, negative values, NaN and infinities are no points.
//   move     q_r = ((M[4r] p_0 + M[4r+1] p_1) + M[4r+2] p_2) + M[4r+3],   z = -q_2.
//            The point is kept iff z > z_near and z rounded to float32 is finite.
//   project  u = cx + fx (q_0 / z),   v = cy - fy (q_1 / z)   -- its position in the full-resolution target image.
//   target   pixel (jo, io) stands for the full-resolution position (jo sy, io sx) with sx = (W - 1) / (Wo - 1) and
//            sy = (H - 1) / (Ho - 1): the strided centres of tracker.image_rays_from_camera_tensor.  An axis with Wo = 1
//            (Ho = 1) has sx = 1 (sy = 1) and stands for position 0.
//   vote     io = floor(u / sx + 0.5), jo = floor(v / sy + 0.5).  The point votes for (jo, io) iff 0 <= io <= Wo - 1,
//            0 <= jo <= Ho - 1 (a NaN or infinite u, v fails this), |u - io sx| <= radius and |v - jo sy| <= radius.
//   combine  votes are combined by an unsigned integer minimum on the bit pattern of (float)z (positive floats order as their
//            bits): the nearest surface wins and the image is the same bits in every run.
//   finish   a pixel without a vote is 0.0 -- what the renderer reads as "no guidance".
//   fill     with fill = 1 a pixel without a vote takes the LARGEST voted value among its (up to) 8 neighbours of the
//            voted image, 0.0 when none of them has a vote either.  One round, reading the unfilled image: a hole that
//            a parallax opened shows the background, not the surface that moved off it.
//
//   memset   the vote image (workspace) with the bit pattern 0xFFFFFFFF
//   splat    one thread per source pixel
//   finish   one thread per target pixel: vote image -> output, with or without the fill
// Memory-bound; at the workload's sizes (680 x 1200 -> 102 x 180, 260 x 346 -> 39 x 51) a target pixel receives a handful
// of votes, and most candidates that lose are kept off the atomic by a plain read first.  No LDS.
#include "../../include/enslam_hip.h"
#include "common.hpp"

namespace {

constexpr int DF_BLOCK = 256;
constexpr uint32_t DF_NONE = 0xFFFFFFFFu;
constexpr int64_t DF_MAX_PIXELS = (int64_t)1 << 30;

struct DfArgs {
    const float* depth;
    uint32_t* votes;                // [Ho,Wo] bit patterns
    double m[12];
    double fx, fy, cx, cy, sx, sy, radius, z_near;
    int32_t H, W, Ho, Wo;
};

__global__ __launch_bounds__(DF_BLOCK) void df_splat_kernel(DfArgs A) {
    const int64_t e = (int64_t)blockIdx.x * DF_BLOCK + threadIdx.x;
    if (e >= (int64_t)A.H * A.W) return;
    const int j = (int)(e / A.W), i = (int)(e - (int64_t)j * A.W);
    const double d = (double)A.depth[e];
    if (!(d > 0.0) || !(d - d == 0.0)) return;
    const double px = ((double)i - A.cx) / A.fx, py = -((double)j - A.cy) / A.fy;
    const double p0 = d * px, p1 = d * py, p2 = -d;
    double q[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) q[r] = ((A.m[4 * r] * p0 + A.m[4 * r + 1] * p1) + A.m[4 * r + 2] * p2) + A.m[4 * r + 3];
    const double z = -q[2];
    if (!(z > A.z_near)) return;
    const float zf = (float)z;
    if (!(zf - zf == 0.0f)) return;
    const double u = A.cx + A.fx * (q[0] / z), v = A.cy - A.fy * (q[1] / z);
    const double fi = floor(u / A.sx + 0.5), fj = floor(v / A.sy + 0.5);
    if (!(fi >= 0.0 && fi <= (double)(A.Wo - 1)) || !(fj >= 0.0 && fj <= (double)(A.Ho - 1))) return;
    if (!(fabs(u - fi * A.sx) <= A.radius) || !(fabs(v - fj * A.sy) <= A.radius)) return;
    const uint32_t bits = __float_as_uint(zf);
    uint32_t* px_out = A.votes + (int64_t)(int)fj * A.Wo + (int)fi;
    // a candidate behind what the pixel already holds stays off the atomic (a stale read only costs a redundant atomic)
    if (bits < *px_out) atomicMin(px_out, bits);
}

__global__ __launch_bounds__(DF_BLOCK) void df_finish_kernel(const uint32_t* __restrict__ votes, uint32_t* __restrict__ out,
                                                             int Ho, int Wo, int fill) {
    const int64_t e = (int64_t)blockIdx.x * DF_BLOCK + threadIdx.x;
    if (e >= (int64_t)Ho * Wo) return;
    uint32_t b = votes[e];
    if (b == DF_NONE) {
        b = 0u;
        if (fill) {
            const int jo = (int)(e / Wo), io = (int)(e - (int64_t)jo * Wo);
            for (int dj = -1; dj <= 1; ++dj)
                for (int di = -1; di <= 1; ++di) {
                    const int jj = jo + dj, ii = io + di;
                    if (jj < 0 || jj >= Ho || ii < 0 || ii >= Wo) continue;
                    const uint32_t nb = votes[(int64_t)jj * Wo + ii];
                    if (nb != DF_NONE && nb > b) b = nb;
                }
        }
    }
    out[e] = b;
}

bool df_finite(double x) { return x == x && x - x == 0.0; }

}  // namespace

extern "C" {

int enslam_depth_forecast(const float* depth, int32_t H, int32_t W, double fx, double fy, double cx, double cy,
                          const double* m_host, int32_t Ho, int32_t Wo, double radius, double z_near, int32_t fill,
                          void* workspace, float* depth_out, void* stream) {
    if (H <= 0 || W <= 0 || Ho <= 0 || Wo <= 0 || !m_host || !depth || !depth_out || !workspace) return ENSLAM_EINVAL;
    if ((fill != 0 && fill != 1) || ((uintptr_t)workspace & 3) || ((uintptr_t)depth_out & 3) || ((uintptr_t)depth & 3))
        return ENSLAM_EINVAL;
    if (!df_finite(fx) || !df_finite(fy) || !df_finite(cx) || !df_finite(cy) || fx == 0.0 || fy == 0.0) return ENSLAM_EINVAL;
    if (!df_finite(radius) || radius < 0.0 || !df_finite(z_near) || z_near < 0.0) return ENSLAM_EINVAL;
    for (int k = 0; k < 12; ++k)
        if (!df_finite(m_host[k])) return ENSLAM_EINVAL;
    // a source axis of one pixel cannot be spread over several target pixels (the spacing would be 0)
    if ((Wo > 1 && W == 1) || (Ho > 1 && H == 1)) return ENSLAM_EINVAL;
    if ((int64_t)H * W > DF_MAX_PIXELS || (int64_t)Ho * Wo > DF_MAX_PIXELS) return ENSLAM_EUNSUPPORTED;
    DfArgs A;
    A.depth = depth;
    A.votes = (uint32_t*)workspace;
    for (int k = 0; k < 12; ++k) A.m[k] = m_host[k];
    A.fx = fx; A.fy = fy; A.cx = cx; A.cy = cy;
    A.sx = Wo > 1 ? (double)(W - 1) / (double)(Wo - 1) : 1.0;
    A.sy = Ho > 1 ? (double)(H - 1) / (double)(Ho - 1) : 1.0;
    A.radius = radius; A.z_near = z_near;
    A.H = H; A.W = W; A.Ho = Ho; A.Wo = Wo;
    hipStream_t s = (hipStream_t)stream;
    const int64_t n_src = (int64_t)H * W, n_dst = (int64_t)Ho * Wo;
    if (hipMemsetAsync(workspace, 0xFF, 4 * (size_t)n_dst, s) != hipSuccess) return ENSLAM_ELAUNCH;
    df_splat_kernel<<<(unsigned)((n_src + DF_BLOCK - 1) / DF_BLOCK), DF_BLOCK, 0, s>>>(A);
    df_finish_kernel<<<(unsigned)((n_dst + DF_BLOCK - 1) / DF_BLOCK), DF_BLOCK, 0, s>>>(A.votes, (uint32_t*)depth_out, Ho, Wo, fill);
    return hipGetLastError() == hipSuccess ? ENSLAM_OK : ENSLAM_ELAUNCH;
}

}  // extern "C"
