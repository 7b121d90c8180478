// Per-iteration frame report (frame_vis.py; enslam_hip.h holds the pixel rules): the sheet of input / generated / residual
// panels of the reference's src/utils/Visualizer.py as one uint8 image, the frame's depth-L1 and colour-error sums, and
// the mean SSIM of two images.  Everything a pixel decides is float32 with separate IEEE operations (this file is built
// without fast-math and with -ffp-contract=off, like the rest of the library), so a numpy float32 restatement gives the
// same bytes; every sum is float64, taken per workgroup and then over the workgroups in index order -- no float atomics.
//
//   fr_max_kernel     partial maxima of gt_depth (fmaxf: a NaN is skipped), at most FR_MAX_PARTS workgroups
//   fr_panels_kernel  the whole sheet: a thread owns FR_PX consecutive pixels of the flattened sheet (12 bytes, three dword
//                     stores), finds for each the panel it lies in, or white for gutters and title strips; the threads of
//                     the colour-residual panel, which hold everything a frame pixel contributes, also add the statistics
//   fr_sum_kernel     the second stage of both sums: thread t adds its run of partials in index order, thread k < K then
//                     the 256 run sums in index order
//   ss_kernel         SSIM (Wang et al. 2004: 11 x 11 Gaussian window, sigma 1.5, K1 0.01, K2 0.03, population covariance,
//                     data range 1): one workgroup per SS_TH x SS_TW tile of output pixels and channel; both images' tile
//                     and 5-pixel halo staged in LDS as float32, the horizontal pass of the five moments x, y, xx, yy, xy
//                     into LDS as float64 (the float32 form of E[x^2] - mu^2 cancels against C2 = 9e-4), then the vertical
//                     pass and the quotient.  LDS: 2 * 26 * 42 * 4 + 5 * 26 * 32 * 8 = 42016 bytes.
#include "../../include/enslam_hip.h"
#include "common.hpp"
#define ENS_LUT_QUALIFIER __device__ const
#include "plasma_lut.hpp"

namespace {

constexpr int FR_BLOCK = 256;
constexpr int FR_PX = 4;                                // sheet pixels per thread
constexpr int FR_MAX_PARTS = 256;                       // workgroups of the depth maximum
constexpr int64_t FR_HEAD = FR_MAX_PARTS * 4;           // bytes in front of the statistics partials
constexpr int FR_STATS = 4;                             // n_valid, sum |depth residual|, sum colour error^2 all / valid
constexpr uint32_t FR_WHITE = 0xFFFFFFu;

constexpr int SS_TH = ENSLAM_SSIM_TILE_H, SS_TW = ENSLAM_SSIM_TILE_W, SS_R = 5, SS_K = 2 * SS_R + 1;
constexpr int SS_IH = SS_TH + 2 * SS_R, SS_IW = SS_TW + 2 * SS_R;
constexpr double SS_C1 = 0.01 * 0.01, SS_C2 = 0.03 * 0.03;

struct FrArgs {
    const float* gt_depth;          // [H,W]
    const float* gt_color;          // [H,W,3]
    const float* depth;             // [H,W]
    const float* color;             // [H,W,3]
    const float* gt_event;          // [h,w,2] or NULL
    const float* pred_event;        // [h,w,2] or NULL
    int32_t H, W, h, w, rows, gutter, title, SW;
    int64_t n_px;                   // pixels of the sheet
    const float* max_part;          // [n_max]
    int32_t n_max;
    uint8_t* sheet;
    double* part;                   // [workgroups][FR_STATS]
};

struct SsArgs {
    const float* x;
    const float* y;
    int32_t H, W, C;
    double g[SS_K];                 // the normalised 1-D window
    double* part;                   // [C][tiles_y][tiles_x]
    double* map;                    // [H-10,W-10,C] or NULL
};

__global__ __launch_bounds__(FR_BLOCK) void fr_max_kernel(int64_t n, const float* __restrict__ gd, float* __restrict__ part) {
    __shared__ float red[FR_BLOCK / 64];
    float m = -INFINITY;
    for (int64_t i = (int64_t)blockIdx.x * FR_BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * FR_BLOCK) m = fmaxf(m, gd[i]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) part[blockIdx.x] = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}

ENS_DEV uint32_t fr_depth_rgb(float v, float maxd, const uint32_t* lut) {
    if (maxd == 0.f) return lut[0];
    const float u = v / maxd;
    if (u != u) return FR_WHITE;
    const int idx = u < 0.f ? 0 : (u >= 1.f ? 255 : (int)(u * 256.0f));
    return lut[idx];
}

ENS_DEV float fr_clip01(float c) {                      // a NaN gives 0
    c = c > 0.f ? c : 0.f;
    return c < 1.f ? c : 1.f;
}

ENS_DEV uint32_t fr_level(float c) { return (uint32_t)(uint8_t)(fr_clip01(c) * 255.0f + 0.5f); }

ENS_DEV uint32_t fr_event_level(float e) {
    float v = e * 50.0f;
    v = v > 0.f ? v : 0.f;
    v = v < 255.f ? v : 255.f;
    return (uint32_t)(uint8_t)v;
}

// r | g << 8 | b << 16 of sheet pixel e; the colour-residual panel adds its frame pixel to acc
ENS_DEV uint32_t fr_pixel(const FrArgs& A, int64_t e, float maxd, const uint32_t* lut, double (&acc)[FR_STATS]) {
    const uint32_t eu = (uint32_t)e;                     // fewer than 2^31 sheet pixels: 32-bit division
    const int row = (int)(eu / (uint32_t)A.SW), col = (int)(eu - (uint32_t)row * (uint32_t)A.SW);
    const int ry = row - A.gutter, cx = col - A.gutter;
    if (ry < 0 || cx < 0) return FR_WHITE;
    const int ph = A.H + A.gutter + A.title, pw = A.W + A.gutter;
    const int r = ry / ph, c = cx / pw;
    const int y = ry - r * ph - A.title, x = cx - c * pw;
    if (r >= A.rows || c >= 3 || y < 0 || y >= A.H || x >= A.W) return FR_WHITE;
    const int64_t p = (int64_t)y * A.W + x;
    if (r == 0) {
        if (c == 0) return fr_depth_rgb(A.gt_depth[p], maxd, lut);
        if (c == 1) return fr_depth_rgb(A.depth[p], maxd, lut);
        const float gd = A.gt_depth[p];
        const float res = gd == 0.f ? 0.f : fabsf(gd - A.depth[p]);
        return fr_depth_rgb(res, maxd, lut);
    }
    if (r == 1) {
        if (c < 2) {
            const float* s = (c == 0 ? A.gt_color : A.color) + 3 * p;
            return fr_level(s[0]) | fr_level(s[1]) << 8 | fr_level(s[2]) << 16;
        }
        const float gd = A.gt_depth[p];
        const bool valid = gd > 0.f;
        uint32_t out = 0;
        double sq = 0.0;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            const float g = A.gt_color[3 * p + ch], q = A.color[3 * p + ch];
            const float res = gd == 0.f ? 0.f : fabsf(g - q);
            out |= fr_level(res) << (8 * ch);
            const float err = fr_clip01(g) - fr_clip01(q);
            sq += (double)err * (double)err;
        }
        acc[2] += sq;
        if (valid) {
            acc[0] += 1.0;
            acc[1] += (double)fabsf(gd - A.depth[p]);
            acc[3] += sq;
        }
        return out;
    }
    // events at their own resolution: the nearest source pixel
    const int sy = (int)(((int64_t)(2 * y + 1) * A.h) / (2 * (int64_t)A.H));
    const int sx = (int)(((int64_t)(2 * x + 1) * A.w) / (2 * (int64_t)A.W));
    const int64_t q = 2 * ((int64_t)sy * A.w + sx);
    if (c == 0) return fr_event_level(A.gt_event[q]) | fr_event_level(A.gt_event[q + 1]) << 8;
    if (c == 1) return fr_event_level(A.pred_event[q]) | fr_event_level(A.pred_event[q + 1]) << 8;
    uint32_t out = 0;
#pragma unroll
    for (int ch = 0; ch < 2; ++ch) {
        const int a = (int)fr_event_level(A.gt_event[q + ch]), b = (int)fr_event_level(A.pred_event[q + ch]);
        out |= (uint32_t)(a > b ? a - b : b - a) << (8 * ch);
    }
    return out;
}

__global__ __launch_bounds__(FR_BLOCK) void fr_panels_kernel(FrArgs A) {
    __shared__ uint32_t lut[256];
    __shared__ float mred[FR_BLOCK / 64];
    __shared__ double sred[FR_BLOCK / 64][FR_STATS];
    const int tid = threadIdx.x;
    lut[tid] = ENS_PLASMA_LUT[3 * tid] | (uint32_t)ENS_PLASMA_LUT[3 * tid + 1] << 8 | (uint32_t)ENS_PLASMA_LUT[3 * tid + 2] << 16;
    float m = tid < A.n_max ? A.max_part[tid] : -INFINITY;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
    if ((tid & 63) == 0) mred[tid >> 6] = m;
    __syncthreads();
    const float maxd = fmaxf(fmaxf(mred[0], mred[1]), fmaxf(mred[2], mred[3]));

    double acc[FR_STATS] = {0.0, 0.0, 0.0, 0.0};
    const int64_t e0 = ((int64_t)blockIdx.x * FR_BLOCK + tid) * FR_PX;
    if (e0 + FR_PX <= A.n_px) {
        uint32_t px[FR_PX];
#pragma unroll
        for (int k = 0; k < FR_PX; ++k) px[k] = fr_pixel(A, e0 + k, maxd, lut, acc);
        uint32_t* dst = reinterpret_cast<uint32_t*>(A.sheet + 3 * e0);          // 12 * thread: dword aligned
        dst[0] = px[0] | px[1] << 24;
        dst[1] = px[1] >> 8 | px[2] << 16;
        dst[2] = px[2] >> 16 | px[3] << 8;
    } else {
        for (int64_t e = e0; e < A.n_px; ++e) {
            const uint32_t v = fr_pixel(A, e, maxd, lut, acc);
            A.sheet[3 * e] = (uint8_t)v;
            A.sheet[3 * e + 1] = (uint8_t)(v >> 8);
            A.sheet[3 * e + 2] = (uint8_t)(v >> 16);
        }
    }
#pragma unroll
    for (int k = 0; k < FR_STATS; ++k) acc[k] = wave_sum(acc[k]);
    if ((tid & 63) == 0) {
#pragma unroll
        for (int k = 0; k < FR_STATS; ++k) sred[tid >> 6][k] = acc[k];
    }
    __syncthreads();
    if (tid < FR_STATS) A.part[(int64_t)blockIdx.x * FR_STATS + tid] = ((sred[0][tid] + sred[1][tid]) + sred[2][tid]) + sred[3][tid];
}

// out[k] = (sum over i of part[i * K + k]) / divisor, and out[K + k] the same (every term is non-negative: the sum of the
// absolute values is the sum) when with_abs.
template <int K>
__global__ __launch_bounds__(FR_BLOCK) void fr_sum_kernel(const double* __restrict__ part, int64_t n, double divisor, int with_abs,
                                                         double* __restrict__ out) {
    __shared__ double run[FR_BLOCK][K];
    const int64_t len = (n + FR_BLOCK - 1) / FR_BLOCK;
    const int64_t lo = threadIdx.x * len, hi = lo + len < n ? lo + len : n;
    double acc[K];
#pragma unroll
    for (int k = 0; k < K; ++k) acc[k] = 0.0;
    for (int64_t i = lo; i < hi; ++i) {
#pragma unroll
        for (int k = 0; k < K; ++k) acc[k] += part[i * K + k];
    }
#pragma unroll
    for (int k = 0; k < K; ++k) run[threadIdx.x][k] = acc[k];
    __syncthreads();
    if (threadIdx.x < K) {
        double s = 0.0;
        for (int t = 0; t < FR_BLOCK; ++t) s += run[t][threadIdx.x];
        out[threadIdx.x] = s / divisor;
        if (with_abs) out[K + threadIdx.x] = s / divisor;
    }
}

__global__ __launch_bounds__(FR_BLOCK) void ss_kernel(SsArgs A) {
    __shared__ float sx[SS_IH][SS_IW], sy[SS_IH][SS_IW];
    __shared__ double hm[5][SS_IH][SS_TW];
    __shared__ double red[FR_BLOCK / 64];
    const int tid = threadIdx.x, ch = blockIdx.z;
    const int y0 = blockIdx.y * SS_TH, x0 = blockIdx.x * SS_TW;         // first output pixel = first input pixel of the tile
    for (int i = tid; i < SS_IH * SS_IW; i += FR_BLOCK) {
        const int r = i / SS_IW, c = i - r * SS_IW;
        const int gy = y0 + r, gx = x0 + c;
        float a = 0.f, b = 0.f;
        if (gy < A.H && gx < A.W) {
            const int64_t p = ((int64_t)gy * A.W + gx) * A.C + ch;
            a = A.x[p];
            b = A.y[p];
        }
        sx[r][c] = a;
        sy[r][c] = b;
    }
    __syncthreads();
    for (int i = tid; i < SS_IH * SS_TW; i += FR_BLOCK) {
        const int r = i / SS_TW, c = i - r * SS_TW;
        double m[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int k = 0; k < SS_K; ++k) {
            const double a = (double)sx[r][c + k], b = (double)sy[r][c + k], w = A.g[k];
            m[0] += w * a;
            m[1] += w * b;
            m[2] += w * (a * a);
            m[3] += w * (b * b);
            m[4] += w * (a * b);
        }
#pragma unroll
        for (int j = 0; j < 5; ++j) hm[j][r][c] = m[j];
    }
    __syncthreads();
    double acc = 0.0;
    for (int i = tid; i < SS_TH * SS_TW; i += FR_BLOCK) {
        const int r = i / SS_TW, c = i - r * SS_TW;
        const int oy = y0 + r, ox = x0 + c;
        if (oy >= A.H - 2 * SS_R || ox >= A.W - 2 * SS_R) continue;
        double m[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int k = 0; k < SS_K; ++k) {
            const double w = A.g[k];
#pragma unroll
            for (int j = 0; j < 5; ++j) m[j] += w * hm[j][r + k][c];
        }
        const double ux = m[0], uy = m[1];
        const double vx = m[2] - ux * ux, vy = m[3] - uy * uy, vxy = m[4] - ux * uy;
        const double num = (2.0 * (ux * uy) + SS_C1) * (2.0 * vxy + SS_C2);
        const double den = ((ux * ux + uy * uy) + SS_C1) * ((vx + vy) + SS_C2);
        const double s = num / den;
        if (A.map) A.map[((int64_t)oy * (A.W - 2 * SS_R) + ox) * A.C + ch] = s;
        acc += s;
    }
    acc = wave_sum(acc);
    if ((tid & 63) == 0) red[tid >> 6] = acc;
    __syncthreads();
    if (tid == 0) A.part[((int64_t)ch * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}

// sheet size and launch shape; ENSLAM_OK or the error code
int fr_shape(int32_t H, int32_t W, int32_t rows, int32_t gutter, int32_t title, int64_t& SH, int64_t& SW, int64_t& blocks) {
    if (H <= 0 || W <= 0 || (rows != 2 && rows != 3) || gutter < 0 || title < 0) return ENSLAM_EINVAL;
    SH = (int64_t)rows * H + (int64_t)(rows + 1) * gutter + (int64_t)rows * title;
    SW = 3 * (int64_t)W + 4 * (int64_t)gutter;
    if (SH > INT32_MAX || SW > INT32_MAX || SH * SW > ((int64_t)1 << 31)) return ENSLAM_EUNSUPPORTED;
    blocks = (SH * SW + (int64_t)FR_BLOCK * FR_PX - 1) / ((int64_t)FR_BLOCK * FR_PX);
    return ENSLAM_OK;
}

int ss_shape(int32_t H, int32_t W, int32_t C, int64_t& tx, int64_t& ty) {
    if (H <= 0 || W <= 0 || (C != 1 && C != 3)) return ENSLAM_EINVAL;
    if (H < SS_K || W < SS_K) return ENSLAM_EINVAL;
    if ((int64_t)H * W > ((int64_t)1 << 28)) return ENSLAM_EUNSUPPORTED;
    tx = (W - 2 * SS_R + SS_TW - 1) / SS_TW;
    ty = (H - 2 * SS_R + SS_TH - 1) / SS_TH;
    if (ty > 65535) return ENSLAM_EUNSUPPORTED;
    return ENSLAM_OK;
}

}  // namespace

extern "C" {

int enslam_vis_panels_workspace(int32_t H, int32_t W, int32_t rows, int32_t gutter, int32_t title, int64_t* bytes_host) {
    int64_t SH, SW, blocks;
    if (!bytes_host) return ENSLAM_EINVAL;
    const int rc = fr_shape(H, W, rows, gutter, title, SH, SW, blocks);
    if (rc != ENSLAM_OK) return rc;
    *bytes_host = FR_HEAD + blocks * FR_STATS * 8;
    return ENSLAM_OK;
}

int enslam_vis_panels(const float* gt_depth, const float* gt_color, const float* depth, const float* color,
                      const float* gt_event, const float* pred_event, int32_t H, int32_t W, int32_t h, int32_t w,
                      int32_t gutter, int32_t title, void* workspace, int64_t workspace_bytes, uint8_t* sheet, double* stats,
                      void* stream) {
    if ((gt_event != nullptr) != (pred_event != nullptr)) return ENSLAM_EINVAL;
    const int rows = gt_event ? 3 : 2;
    int64_t SH, SW, blocks;
    const int rc = fr_shape(H, W, rows, gutter, title, SH, SW, blocks);
    if (rc != ENSLAM_OK) return rc;
    if (!gt_depth || !gt_color || !depth || !color || !workspace || !sheet || !stats) return ENSLAM_EINVAL;
    if (gt_event && (h <= 0 || w <= 0)) return ENSLAM_EINVAL;
    if (workspace_bytes < FR_HEAD + blocks * FR_STATS * 8 || ((uintptr_t)workspace & 7) || ((uintptr_t)sheet & 3)) return ENSLAM_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    const int64_t n = (int64_t)H * W;
    int64_t n_max = (n + 4 * FR_BLOCK - 1) / (4 * FR_BLOCK);
    n_max = n_max > FR_MAX_PARTS ? FR_MAX_PARTS : n_max;
    FrArgs A;
    A.gt_depth = gt_depth; A.gt_color = gt_color; A.depth = depth; A.color = color;
    A.gt_event = gt_event; A.pred_event = pred_event;
    A.H = H; A.W = W; A.h = gt_event ? h : 1; A.w = gt_event ? w : 1; A.rows = rows; A.gutter = gutter; A.title = title;
    A.SW = (int32_t)SW; A.n_px = SH * SW;
    A.max_part = (const float*)workspace; A.n_max = (int32_t)n_max;
    A.sheet = sheet;
    A.part = (double*)((char*)workspace + FR_HEAD);
    fr_max_kernel<<<(unsigned)n_max, FR_BLOCK, 0, s>>>(n, gt_depth, (float*)workspace);
    fr_panels_kernel<<<(unsigned)blocks, FR_BLOCK, 0, s>>>(A);
    fr_sum_kernel<FR_STATS><<<1, FR_BLOCK, 0, s>>>(A.part, blocks, 1.0, 1, stats);
    return hipGetLastError() == hipSuccess ? ENSLAM_OK : ENSLAM_ELAUNCH;
}

int enslam_ssim_workspace(int32_t H, int32_t W, int32_t C, int64_t* bytes_host) {
    int64_t tx, ty;
    if (!bytes_host) return ENSLAM_EINVAL;
    const int rc = ss_shape(H, W, C, tx, ty);
    if (rc != ENSLAM_OK) return rc;
    *bytes_host = tx * ty * C * 8;
    return ENSLAM_OK;
}

int enslam_ssim(const float* x, const float* y, int32_t H, int32_t W, int32_t C, void* workspace, int64_t workspace_bytes,
                double* mean_out, double* map_out, void* stream) {
    int64_t tx, ty;
    const int rc = ss_shape(H, W, C, tx, ty);
    if (rc != ENSLAM_OK) return rc;
    if (!x || !y || !workspace || !mean_out || workspace_bytes < tx * ty * C * 8 || ((uintptr_t)workspace & 7)) return ENSLAM_EINVAL;
    SsArgs A;
    A.x = x; A.y = y; A.H = H; A.W = W; A.C = C;
    double sum = 0.0;
    for (int k = 0; k < SS_K; ++k) {
        A.g[k] = exp(-((double)(k - SS_R) * (double)(k - SS_R)) / (2.0 * 1.5 * 1.5));
        sum += A.g[k];
    }
    for (int k = 0; k < SS_K; ++k) A.g[k] /= sum;
    A.part = (double*)workspace;
    A.map = map_out;
    hipStream_t s = (hipStream_t)stream;
    ss_kernel<<<dim3((unsigned)tx, (unsigned)ty, (unsigned)C), FR_BLOCK, 0, s>>>(A);
    const double count = (double)(H - 2 * SS_R) * (double)(W - 2 * SS_R) * (double)C;
    fr_sum_kernel<1><<<1, FR_BLOCK, 0, s>>>(A.part, tx * ty * C, count, 0, mean_out);
    return hipGetLastError() == hipSuccess ? ENSLAM_OK : ENSLAM_ELAUNCH;
}

}  // extern "C"
