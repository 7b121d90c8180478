// Frame preparation: the raw decoded images of one frame -> the tensors the dataset readers hand out (enslam_frame_prepare,
// enslam_hip.h; the host route is datasets.py: undistort, the cv2-style resize, / 255., crop_size, crop_edge).
//
// One launch, one thread per OUTPUT pixel.  Nothing is staged in memory: a thread walks back through the stages and
// recomputes the taps of the earlier ones, including their intermediate uint8 rounding --
//
//   output pixel -> (crop_edge shift) -> crop_size: 2x2 taps of the depth-size image (align_corners, colour float64,
//   events float32) -> cv2-style resize: 2x2 taps of the raw-size image each (half-pixel centres, float64; events rounded
//   to uint8) -> undistort: 2x2 raw taps each (float64, zero border, rounded to uint8)
//
// at most 4 * 4 * 4 raw reads per channel when every stage is switched on, 1 when none is (a Replica frame).  The images
// are 90 k - 816 k pixels: launch count, not bandwidth, is what a frame costs.
//
// Precision: every stage repeats the host route's operations in its order (-ffp-contract=off, no fused multiply-adds).
//   undistort   datasets.undistort / distort_points term by term, numpy float64; np.rint = rint (half to even)
//   resizes     torch's CPU upsample_bilinear2d for C = 3 (its generic N-d kernel): per axis
//               src = fma(scale, dst + 0.5, -0.5) clamped at 0 (half-pixel) or scale * dst (align_corners),
//               i0 = min(floorf(src), in - 1) -- floorf of the value ROUNDED TO FLOAT32, as ATen's guard_index_and_lambda
//               does for float64 too --, l1 = clamp(src - i0, 0, 1), l0 = 1 - l1, i1 = min(i0 + 1, in - 1), and
//               out = ((ly0 lx0) a + (ly0 lx1) b + (ly1 lx0) c) + (ly1 lx1) d, summed in this order.  ATen's kernel fuses
//               some of these operations in a build-dependent way; the residue is an ulp or two of the result (measured
//               against torch's CPU kernel: 3.4e-16 on values <= 1), exact where the weights are dyadic
//   depth       torch's `nearest`: min(floorf(dst * float32(in) / out), in - 1); float32(raw) / float32(png_depth_scale)
//               * float32(scale)
// The helpers are host-callable as well so that a CPU build can step through one pixel (gdb on a CPU build is the
// debugger of this project); the library only ever calls them from the kernel.
#include "../../include/enslam_hip.h"
#include "common.hpp"

namespace {

constexpr int FP_BLOCK = 256;
constexpr int64_t FP_MAX_PIXELS = (int64_t)1 << 28;

#define FP_HD __host__ __device__ __forceinline__

struct FpArgs {
    enslam_frame_plan p;
    const uint8_t* color;
    const void* depth;
    const uint8_t* event;           // NULL: zero events
    double* color_out;
    float* depth_out;
    void* event_out;                // NULL: no event outputs
    int64_t* mask_out;
    int32_t Ho, Wo;                 // outputs
    int32_t crop;                   // crop_size given
    double hp_cy, hp_cx;            // half-pixel scales raw colour -> depth size (float64: in / out)
    double hp_ey, hp_ex;            // raw events -> depth size
    double ac_y, ac_x;              // align_corners scales depth size -> crop_size, float64
    float acf_y, acf_x;             // the same in float32 (events)
    float nn_y, nn_x;               // nearest scales (float32: in / out)
};

struct FpImg {
    const uint8_t* px;
    int h, w, C;
    bool undist;
    int ch[3];                      // channels carried through the chain
};

// One axis of ATen's bilinear index computation in its float64 instantiation.
FP_HD void fp_axis(double scale, bool align, int dst, int in, int& i0, int& i1, double& l0, double& l1) {
    // half-pixel centres: ONE rounding, written as the fused multiply-add that ATen's x86-64 kernels (built with FMA and
    // contraction) make of  scale * (dst + 0.5) - 0.5;  unfused, the weights sit up to an ulp of the position (7e-15 at
    // column 40) away from the host route's
    double src = align ? scale * (double)dst : fma(scale, (double)dst + 0.5, -0.5);
    if (!align && src < 0.0) src = 0.0;
    int k = (int)floorf((float)src);
    k = k > in - 1 ? in - 1 : (k < 0 ? 0 : k);
    const double l = src - (double)k;
    l1 = l < 0.0 ? 0.0 : (l > 1.0 ? 1.0 : l);
    l0 = 1.0 - l1;
    i0 = k;
    i1 = k + 1 > in - 1 ? in - 1 : k + 1;
}

// ... and in its float32 instantiation (align_corners only: the events through crop_size)
FP_HD void fp_axis_f(float scale, int dst, int in, int& i0, int& i1, float& l0, float& l1) {
    const float src = scale * (float)dst;
    int k = (int)floorf(src);
    k = k > in - 1 ? in - 1 : (k < 0 ? 0 : k);
    const float l = src - (float)k;
    l1 = l < 0.f ? 0.f : (l > 1.f ? 1.f : l);
    l0 = 1.f - l1;
    i0 = k;
    i1 = k + 1 > in - 1 ? in - 1 : k + 1;
}

FP_HD double fp_round_u8(double v) {
    const double r = rint(v);
    return r < 0.0 ? 0.0 : (r > 255.0 ? 255.0 : r);       // a NaN (degenerate lens model) passes through to the 0 below
}

// N channels of pixel (v, u) of the undistorted image (or of the raw image without a lens model), as float64 integers.
template <int N>
FP_HD void fp_u8(const enslam_frame_plan& P, const FpImg& I, int v, int u, double (&o)[N]) {
    if (!I.undist) {
        const uint8_t* s = I.px + ((int64_t)v * I.w + u) * I.C;
#pragma unroll
        for (int c = 0; c < N; ++c) o[c] = (double)s[I.ch[c]];
        return;
    }
    // datasets.distort_points on ((u - cx) / fx, (v - cy) / fy)
    const double k1 = P.dist[0], k2 = P.dist[1], p1 = P.dist[2], p2 = P.dist[3], k3 = P.dist[4], k4 = P.dist[5], k5 = P.dist[6],
                 k6 = P.dist[7];
    const double x = ((double)u - P.cx) / P.fx, y = ((double)v - P.cy) / P.fy;
    const double r2 = x * x + y * y;
    const double radial = (1.0 + r2 * (k1 + r2 * (k2 + r2 * k3))) / (1.0 + r2 * (k4 + r2 * (k5 + r2 * k6)));
    const double xd = (x * radial + ((2.0 * p1) * x) * y) + p2 * (r2 + (2.0 * x) * x);
    const double yd = (y * radial + p1 * (r2 + (2.0 * y) * y)) + ((2.0 * p2) * x) * y;
    const double mx = P.fx * xd + P.cx, my = P.fy * yd + P.cy;
#pragma unroll
    for (int c = 0; c < N; ++c) o[c] = 0.0;
    // all four taps outside (or a position that is not a number): the zero border.  Inside this window floor() fits an int.
    if (!(mx > -1.0 && mx < (double)I.w && my > -1.0 && my < (double)I.h)) return;
    const double fxl = floor(mx), fyl = floor(my);
    const int x0 = (int)fxl, y0 = (int)fyl;               // -1 .. w - 1, -1 .. h - 1
    const double ax = mx - fxl, ay = my - fyl;
    const double w00 = (1.0 - ay) * (1.0 - ax), w01 = (1.0 - ay) * ax, w10 = ay * (1.0 - ax), w11 = ay * ax;
    const bool okx0 = x0 >= 0, okx1 = x0 + 1 < I.w, oky0 = y0 >= 0, oky1 = y0 + 1 < I.h;
    const int xa = okx0 ? x0 : 0, xb = okx1 ? x0 + 1 : I.w - 1, ya = oky0 ? y0 : 0, yb = oky1 ? y0 + 1 : I.h - 1;
    const uint8_t* ra = I.px + (int64_t)ya * I.w * I.C;
    const uint8_t* rb = I.px + (int64_t)yb * I.w * I.C;
#pragma unroll
    for (int c = 0; c < N; ++c) {
        const int k = I.ch[c];
        const double t00 = (oky0 && okx0) ? (double)ra[xa * I.C + k] : 0.0;
        const double t01 = (oky0 && okx1) ? (double)ra[xb * I.C + k] : 0.0;
        const double t10 = (oky1 && okx0) ? (double)rb[xa * I.C + k] : 0.0;
        const double t11 = (oky1 && okx1) ? (double)rb[xb * I.C + k] : 0.0;
        const double s = ((w00 * t00 + w01 * t01) + w10 * t10) + w11 * t11;
        const double r = fp_round_u8(s);
        o[c] = r == r ? r : 0.0;
    }
}

// The 2 x 2 blend  ((w00 * a + w01 * b) + w10 * c) + w11 * d,  w_ij = ly_i * lx_j,  fed one tap at a time (k = 0..3 = a, b,
// c, d) without keeping the four taps.  The taps are walked by loops that stay loops: unrolled through all three stages the
// undistortion would be laid out 16 times per instantiation.
template <int N, typename T>
struct FpBlend {
    T acc[N] = {};
    FP_HD void add(int k, const T (&v)[N], const T (&ly)[2], const T (&lx)[2]) {
        const T w = ly[k >> 1] * lx[k & 1];
#pragma unroll
        for (int c = 0; c < N; ++c) acc[c] = k == 0 ? w * v[c] : acc[c] + w * v[c];
    }
};

// N channels of pixel (y, x) of the DEPTH-SIZE image: the cv2-style resize of the undistorted image, float64.
// COLOR: values / 255. before the resize, no rounding; otherwise uint8 values, rounded half-to-even after it.
template <int N, bool COLOR>
FP_HD void fp_sized(const FpArgs& A, const FpImg& I, double sy, double sx, int y, int x, double (&o)[N]) {
    if (I.h == A.p.H && I.w == A.p.W) {
        fp_u8<N>(A.p, I, y, x, o);
#pragma unroll
        for (int c = 0; c < N; ++c) o[c] = COLOR ? o[c] / 255.0 : o[c];
        return;
    }
    int y0, y1, x0, x1;
    double ly[2], lx[2];
    fp_axis(sy, false, y, I.h, y0, y1, ly[0], ly[1]);
    fp_axis(sx, false, x, I.w, x0, x1, lx[0], lx[1]);
    FpBlend<N, double> B;
#pragma clang loop unroll(disable)
    for (int k = 0; k < 4; ++k) {
        double v[N];
        fp_u8<N>(A.p, I, (k & 2) ? y1 : y0, (k & 1) ? x1 : x0, v);
#pragma unroll
        for (int c = 0; c < N; ++c) v[c] = COLOR ? v[c] / 255.0 : v[c];
        B.add(k, v, ly, lx);
    }
#pragma unroll
    for (int c = 0; c < N; ++c) o[c] = COLOR ? B.acc[c] : fp_round_u8(B.acc[c]);
}

// colour of pixel (py, px) of the image the crop_edge cut is taken from
template <int N>
FP_HD void fp_color(const FpArgs& A, const FpImg& I, int py, int px, double (&o)[N]) {
    if (!A.crop) {
        fp_sized<N, true>(A, I, A.hp_cy, A.hp_cx, py, px, o);
        return;
    }
    int y0, y1, x0, x1;
    double ly[2], lx[2];
    fp_axis(A.ac_y, true, py, A.p.H, y0, y1, ly[0], ly[1]);
    fp_axis(A.ac_x, true, px, A.p.W, x0, x1, lx[0], lx[1]);
    FpBlend<N, double> B;
#pragma clang loop unroll(disable)
    for (int k = 0; k < 4; ++k) {
        double v[N];
        fp_sized<N, true>(A, I, A.hp_cy, A.hp_cx, (k & 2) ? y1 : y0, (k & 1) ? x1 : x0, v);
        B.add(k, v, ly, lx);
    }
#pragma unroll
    for (int c = 0; c < N; ++c) o[c] = B.acc[c];
}

// events (-, +) of that pixel: uint8 values without crop_size, float32 with it
FP_HD void fp_event(const FpArgs& A, const FpImg& I, int py, int px, float (&o)[2]) {
    double v[2];
    if (!A.crop) {
        fp_sized<2, false>(A, I, A.hp_ey, A.hp_ex, py, px, v);
        o[0] = (float)v[0];
        o[1] = (float)v[1];
        return;
    }
    int y0, y1, x0, x1;
    float ly[2], lx[2];
    fp_axis_f(A.acf_y, py, A.p.H, y0, y1, ly[0], ly[1]);
    fp_axis_f(A.acf_x, px, A.p.W, x0, x1, lx[0], lx[1]);
    FpBlend<2, float> B;
#pragma clang loop unroll(disable)
    for (int k = 0; k < 4; ++k) {
        fp_sized<2, false>(A, I, A.hp_ey, A.hp_ex, (k & 2) ? y1 : y0, (k & 1) ? x1 : x0, v);
        const float f[2] = {(float)v[0], (float)v[1]};
        B.add(k, f, ly, lx);
    }
    o[0] = B.acc[0];
    o[1] = B.acc[1];
}

FP_HD int fp_nearest(float scale, int dst, int in, int out) {
    if (in == out) return dst;
    if (out == 2 * in) return dst >> 1;
    const int k = (int)floorf((float)dst * scale);
    return k > in - 1 ? in - 1 : k;
}

FP_HD void fp_pixel(const FpArgs& A, int oy, int ox) {
    const enslam_frame_plan& P = A.p;
    const int py = oy + P.crop_edge, px = ox + P.crop_edge;
    const int64_t o = (int64_t)oy * A.Wo + ox;

    FpImg I;
    I.px = A.color; I.h = P.h0; I.w = P.w0; I.C = P.channels; I.undist = P.has_dist != 0;
    I.ch[0] = 0; I.ch[1] = 1; I.ch[2] = 2;
    double* co = A.color_out + 3 * o;
    if (P.channels == 1) {
        double g[1];
        fp_color<1>(A, I, py, px, g);
        co[0] = g[0]; co[1] = g[0]; co[2] = g[0];
    } else {
        double c[3];
        fp_color<3>(A, I, py, px, c);
        co[0] = c[0]; co[1] = c[1]; co[2] = c[2];
    }

    const int dy = A.crop ? fp_nearest(A.nn_y, py, P.H, P.crop_h) : py;
    const int dx = A.crop ? fp_nearest(A.nn_x, px, P.W, P.crop_w) : px;
    const int64_t di = (int64_t)dy * P.W + dx;
    const float raw = P.depth_int32 ? (float)((const int32_t*)A.depth)[di] : (float)((const uint16_t*)A.depth)[di];
    A.depth_out[o] = (raw / (float)P.png_depth_scale) * (float)P.scale;

    if (!A.event_out) return;
    float e[2] = {0.f, 0.f};
    if (A.event) {
        FpImg E;
        E.px = A.event; E.h = P.he; E.w = P.we; E.C = 3; E.undist = P.has_dist != 0 && P.undistort_events != 0;
        E.ch[0] = P.ev_neg; E.ch[1] = P.ev_pos; E.ch[2] = 0;
        fp_event(A, E, py, px, e);
    }
    if (A.crop) {
        float* eo = (float*)A.event_out + 2 * o;
        eo[0] = e[0]; eo[1] = e[1];
    } else {
        uint8_t* eo = (uint8_t*)A.event_out + 2 * o;
        eo[0] = (uint8_t)e[0]; eo[1] = (uint8_t)e[1];
    }
    A.mask_out[o] = (e[0] != 0.f || e[1] != 0.f) ? 1 : 0;
}

__global__ __launch_bounds__(FP_BLOCK) void frame_prepare_kernel(FpArgs A) {
    // 64 x 4 pixel tiles: a wave covers 64 consecutive pixels of one row, whose taps share cache lines
    const int ox = blockIdx.x * 64 + (threadIdx.x & 63), oy = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (ox >= A.Wo || oy >= A.Ho) return;
    fp_pixel(A, oy, ox);
}

bool fp_finite(double x) { return x == x && x - x == 0.0; }

// Checks the plan and the pointers and fills the derived fields of A.  No device work.
int fp_setup(const enslam_frame_plan* plan, const uint8_t* color_raw, const void* depth_raw, const uint8_t* event_raw,
             double* color_out, float* depth_out, void* event_out, int64_t* mask_out, FpArgs& A) {
    if (!plan || !color_raw || !depth_raw || !color_out || !depth_out) return ENSLAM_EINVAL;
    if ((event_out == nullptr) != (mask_out == nullptr)) return ENSLAM_EINVAL;
    const enslam_frame_plan& P = *plan;
    if (P.channels != 1 && P.channels != 3) return ENSLAM_EINVAL;
    if (P.h0 < 1 || P.w0 < 1 || P.H < 1 || P.W < 1 || P.crop_edge < 0) return ENSLAM_EINVAL;
    if ((P.crop_h > 0) != (P.crop_w > 0) || P.crop_h < 0 || P.crop_w < 0) return ENSLAM_EINVAL;
    if (event_raw && event_out) {
        if (P.he < 1 || P.we < 1 || P.ev_neg < 0 || P.ev_neg > 2 || P.ev_pos < 0 || P.ev_pos > 2) return ENSLAM_EINVAL;
        if ((int64_t)P.he * P.we > FP_MAX_PIXELS) return ENSLAM_EUNSUPPORTED;
    }
    if (P.has_dist) {
        if (!fp_finite(P.fx) || !fp_finite(P.fy) || !fp_finite(P.cx) || !fp_finite(P.cy) || P.fx == 0.0 || P.fy == 0.0)
            return ENSLAM_EINVAL;
        for (int i = 0; i < 8; ++i)
            if (!fp_finite(P.dist[i])) return ENSLAM_EINVAL;
    }
    if (!fp_finite(P.png_depth_scale) || P.png_depth_scale == 0.0 || !fp_finite(P.scale)) return ENSLAM_EINVAL;
    const int Hs = P.crop_h > 0 ? P.crop_h : P.H, Ws = P.crop_w > 0 ? P.crop_w : P.W;
    if ((int64_t)P.h0 * P.w0 > FP_MAX_PIXELS || (int64_t)P.H * P.W > FP_MAX_PIXELS || (int64_t)Hs * Ws > FP_MAX_PIXELS)
        return ENSLAM_EUNSUPPORTED;
    if (2 * (int64_t)P.crop_edge >= Hs || 2 * (int64_t)P.crop_edge >= Ws) return ENSLAM_EINVAL;
    A.p = P;
    A.color = color_raw; A.depth = depth_raw; A.event = event_out ? event_raw : nullptr;
    A.color_out = color_out; A.depth_out = depth_out; A.event_out = event_out; A.mask_out = mask_out;
    A.Ho = Hs - 2 * P.crop_edge; A.Wo = Ws - 2 * P.crop_edge;
    A.crop = P.crop_h > 0;
    // ATen's area_pixel_compute_scale / compute_scales_value
    A.hp_cy = (double)P.h0 / (double)P.H; A.hp_cx = (double)P.w0 / (double)P.W;
    A.hp_ey = (double)P.he / (double)P.H; A.hp_ex = (double)P.we / (double)P.W;
    A.ac_y = Hs > 1 ? (double)(P.H - 1) / (double)(Hs - 1) : 0.0;
    A.ac_x = Ws > 1 ? (double)(P.W - 1) / (double)(Ws - 1) : 0.0;
    A.acf_y = Hs > 1 ? (float)(P.H - 1) / (float)(Hs - 1) : 0.f;
    A.acf_x = Ws > 1 ? (float)(P.W - 1) / (float)(Ws - 1) : 0.f;
    A.nn_y = (float)P.H / (float)Hs; A.nn_x = (float)P.W / (float)Ws;
    return ENSLAM_OK;
}

}  // namespace

extern "C" {

int64_t enslam_frame_plan_bytes(void) { return (int64_t)sizeof(enslam_frame_plan); }

int enslam_frame_prepare(const enslam_frame_plan* plan, const uint8_t* color_raw, const void* depth_raw,
                         const uint8_t* event_raw, double* color_out, float* depth_out, void* event_out, int64_t* mask_out,
                         void* stream) {
    FpArgs A;
    const int rc = fp_setup(plan, color_raw, depth_raw, event_raw, color_out, depth_out, event_out, mask_out, A);
    if (rc != ENSLAM_OK) return rc;
    const dim3 grid((unsigned)((A.Wo + 63) / 64), (unsigned)((A.Ho + 3) / 4));
    frame_prepare_kernel<<<grid, FP_BLOCK, 0, (hipStream_t)stream>>>(A);
    return hipGetLastError() == hipSuccess ? ENSLAM_OK : ENSLAM_ELAUNCH;
}

}  // extern "C"
