// Event-generation-model loss (enslam_event_model_loss; enslam_hip.h holds the model): predicted event image of a colour pair
// from the contrast-threshold model, its L2 distance to the recorded one raw and Gaussian-blurred, and the gradient in the
// current colour -- two launches.
//
//   tile    one 256-thread workgroup per EM_TILE x EM_TILE tile and event channel (grid z).  It stages the residual r in LDS
//           on the tile grown by 2 R_max in EXTENDED coordinates: position s holds r[reflect(s)] for -R_max <= s <= n - 1 +
//           R_max (what a reflect-padded blur of an in-image pixel can read) and 0 elsewhere.  Per Gaussian kernel, out of LDS:
//             rows     h[sy][x]  = sum_t tap[t] ext[sy][x - R + t]        sy in tile +- 2R, x in tile +- R
//             columns  v[y][x]   = sum_t tap[t] h[y - R + t][x]           y, x in tile +- R; 0 outside the image  (= B r)
//             columns' a[y][x]   = (B_y^T v)[y][x]                        y in the tile, x in tile +- R
//             rows'    out[y][x] = (B_x^T a)[y][x]                        the thread's own pixel                  (= B^T B r)
//           The adjoint passes gather: in one dimension (B^T v)[p] = C(p) + [1 <= p <= R] C(-p) + [n-1-R <= p <= n-2] C(2(n-1)-p)
//           with C(s) = sum_t tap[t] v[s + R - t] over the in-image v only.  Every v a pixel needs lies within R of it and
//           inside the image, so inside the staged region.
//           The channel of a pixel's active hinge writes its gradient (+ where d >= 0, which writes the zeros too; - where
//           d < 0): exactly one workgroup writes each gradient pixel.  r^2 and (B_i r)^2 are squared and added in float64,
//           reduced by a fixed tree per workgroup, one partial row per workgroup.
//           On request the same two forward passes run on gt and on pred first (B_i gt, B_i pred for the figure writer).
//   finish  one workgroup: term j = the partial rows added in workgroup order; loss = term 0 + sum_i w_i term i.
// No float atomics, no fences: two runs give the same bits.  Every global index is a reflected or guarded in-image index.
#include "../../include/enslam_hip.h"
#include "common.hpp"
#include "kernels.hpp"

#include <cmath>

namespace {

constexpr int EM_TILE = ENSLAM_EVENT_MODEL_TILE;
constexpr int EM_BLOCK = EM_TILE * EM_TILE;
constexpr int EM_KMAX = ENSLAM_EVENT_MODEL_MAX_KSIZE;
constexpr int EM_NK = ENSLAM_EVENT_MODEL_MAX_KERNELS;
constexpr int EM_RMAX = EM_KMAX / 2;
constexpr int EM_E = EM_TILE + 4 * EM_RMAX;            // staged side at the largest kernel
constexpr int EM_V = EM_TILE + 2 * EM_RMAX;
static_assert(EM_BLOCK == 256, "one thread per tile pixel, four waves");
static_assert((EM_E * EM_E + EM_E * EM_V + EM_V * EM_V + EM_TILE * EM_V + EM_NK * EM_KMAX) * 4 + EM_BLOCK * 8 <= 65536, "LDS");

enum { EM_STAGE_R = 0, EM_STAGE_GT = 1, EM_STAGE_PRED = 2 };

struct EmArgs {
    const float* cur;
    const float* prev;
    const float* gt;
    int h, w, K, rmax;
    float c_neg, c_pos, eps;
    int ksize[EM_NK];
    float wk[EM_NK];
    float taps[EM_NK][EM_KMAX];
    float* pred;
    float* grad;
    double* partials;               // [tiles * 2][K + 1]
    float* blur_gt;                 // [K,h,w,2] or NULL
    float* blur_pred;
};

__device__ __forceinline__ float em_luma(const float* p) { return (0.299f * p[0] + 0.587f * p[1]) + 0.114f * p[2]; }

// torch.clamp(y, min=0) of the model's statement (event_model.luminance): a NaN stays a NaN (fmaxf would turn it into 0 and a
// render that is not a number into a finite loss with a zero gradient)
__device__ __forceinline__ float em_clamp0(float y) { return y < 0.f ? 0.f : y; }

__device__ __forceinline__ float em_logdiff(const EmArgs& A, int64_t o, float& ycur_raw) {
    ycur_raw = em_luma(A.cur + 3 * o);
    const float yc = em_clamp0(ycur_raw), yp = em_clamp0(em_luma(A.prev + 3 * o));
    return logf(yc + A.eps) - logf(yp + A.eps);
}

__device__ __forceinline__ float em_pred(const EmArgs& A, float d, int c) {
    if (d != d) return d;                               // (a NaN is no side of the hinge: it goes through, as in torch.clamp)
    return c ? (d > 0.f ? d / A.c_pos : 0.f) : (d < 0.f ? -d / A.c_neg : 0.f);
}

__device__ __forceinline__ int em_reflect(int s, int n) { return s < 0 ? -s : (s >= n ? 2 * (n - 1) - s : s); }

// ext[E x E] of the tile at (y0, x0), E = EM_TILE + 4 rm: extended position (sy, sx) = (y0 - 2 rm + j, x0 - 2 rm + m)
__device__ void em_stage(const EmArgs& A, float* ext, int y0, int x0, int c, int what) {
    const int rm = A.rmax, E = EM_TILE + 4 * rm;
    for (int e = threadIdx.x; e < E * E; e += EM_BLOCK) {
        const int j = e / E, m = e - j * E;
        const int sy = y0 - 2 * rm + j, sx = x0 - 2 * rm + m;
        float val = 0.f;
        if (sy >= -rm && sy <= A.h - 1 + rm && sx >= -rm && sx <= A.w - 1 + rm) {
            const int64_t o = (int64_t)em_reflect(sy, A.h) * A.w + em_reflect(sx, A.w);
            const float g = A.gt[2 * o + c];
            if (what == EM_STAGE_GT) {
                val = g;
            } else {
                float yraw;
                const float p = em_pred(A, em_logdiff(A, o, yraw), c);
                val = what == EM_STAGE_PRED ? p : p - g;
            }
        }
        ext[e] = val;
    }
}

// v = B_i ext on tile +- R (0 outside the image); leaves with a barrier behind it
__device__ void em_blur(const EmArgs& A, const float* ext, float* hb, float* v, const float* tap, int k, int y0, int x0) {
    const int rm = A.rmax, E = EM_TILE + 4 * rm, R = k / 2, dl = 2 * (rm - R);
    const int Vi = EM_TILE + 2 * R, Hi = EM_TILE + 4 * R;
    for (int e = threadIdx.x; e < Hi * Vi; e += EM_BLOCK) {
        const int j = e / Vi, m = e - j * Vi;
        const float* src = ext + (j + dl) * E + m + dl;
        float acc = 0.f;
        for (int t = 0; t < k; ++t) acc += tap[t] * src[t];
        hb[e] = acc;
    }
    __syncthreads();
    for (int e = threadIdx.x; e < Vi * Vi; e += EM_BLOCK) {
        const int j = e / Vi, m = e - j * Vi;
        const int y = y0 - R + j, x = x0 - R + m;
        float acc = 0.f;
        if (y >= 0 && y < A.h && x >= 0 && x < A.w)
            for (int t = 0; t < k; ++t) acc += tap[t] * hb[(j + t) * Vi + m];
        v[e] = acc;
    }
    __syncthreads();
}

// C(s) of the header for one dimension of length n: sum_t tap[t] src[(q - lo) * stride], q = s + R - t inside the image and
// inside the staged rows [lo, lo + len)
__device__ __forceinline__ float em_corr(const float* src, int stride, const float* tap, int k, int s, int n, int lo, int len) {
    const int R = k / 2;
    float acc = 0.f;
    for (int t = 0; t < k; ++t) {
        const int q = s + R - t;
        if (q >= 0 && q < n && q >= lo && q < lo + len) acc += tap[t] * src[(q - lo) * stride];
    }
    return acc;
}

// (B^T src)[p] in one dimension
__device__ __forceinline__ float em_adjoint(const float* src, int stride, const float* tap, int k, int p, int n, int lo, int len) {
    const int R = k / 2;
    float acc = em_corr(src, stride, tap, k, p, n, lo, len);
    if (p >= 1 && p <= R) acc += em_corr(src, stride, tap, k, -p, n, lo, len);
    if (p <= n - 2 && p >= n - 1 - R) acc += em_corr(src, stride, tap, k, 2 * (n - 1) - p, n, lo, len);
    return acc;
}

__device__ double em_block_sum(double* red, double x) {
    red[threadIdx.x] = x;
    __syncthreads();
    for (int s = EM_BLOCK / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    const double out = red[0];
    __syncthreads();
    return out;
}

__global__ __launch_bounds__(EM_BLOCK) void event_model_tile_kernel(EmArgs A) {
    __shared__ float s_ext[EM_E * EM_E];
    __shared__ float s_h[EM_E * EM_V];
    __shared__ float s_v[EM_V * EM_V];
    __shared__ float s_a[EM_TILE * EM_V];
    __shared__ float s_tap[EM_NK * EM_KMAX];
    __shared__ double s_red[EM_BLOCK];
    const int tid = threadIdx.x, c = blockIdx.z;
    const int x0 = blockIdx.x * EM_TILE, y0 = blockIdx.y * EM_TILE;
    const int tx = tid % EM_TILE, ty = tid / EM_TILE, px = x0 + tx, py = y0 + ty;
    const bool inside = px < A.w && py < A.h;
    const int64_t o = inside ? (int64_t)py * A.w + px : 0;
    const int64_t npix = (int64_t)A.h * A.w;
    const int rm = A.rmax, E = EM_TILE + 4 * rm;
    if (tid < EM_NK * EM_KMAX) s_tap[tid] = A.taps[tid / EM_KMAX][tid % EM_KMAX];

    if (A.blur_gt && A.K > 0) {
        for (int what = EM_STAGE_GT; what <= EM_STAGE_PRED; ++what) {
            __syncthreads();
            em_stage(A, s_ext, y0, x0, c, what);
            __syncthreads();
            float* dst = what == EM_STAGE_GT ? A.blur_gt : A.blur_pred;
            for (int i = 0; i < A.K; ++i) {
                const int k = A.ksize[i], R = k / 2, Vi = EM_TILE + 2 * R;
                em_blur(A, s_ext, s_h, s_v, s_tap + i * EM_KMAX, k, y0, x0);
                if (inside) dst[2 * (i * npix + o) + c] = s_v[(ty + R) * Vi + tx + R];
                __syncthreads();
            }
        }
    }
    __syncthreads();
    em_stage(A, s_ext, y0, x0, c, EM_STAGE_R);
    __syncthreads();

    float d = 0.f, yraw = 0.f, r0 = 0.f;
    if (inside) {
        d = em_logdiff(A, o, yraw);
        A.pred[2 * o + c] = em_pred(A, d, c);
        r0 = s_ext[(ty + 2 * rm) * E + tx + 2 * rm];
    }
    const int64_t row = ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * 2 + c;
    double* part = A.partials + row * (A.K + 1);
    double tot = em_block_sum(s_red, (double)r0 * (double)r0);
    if (tid == 0) part[0] = tot;
    float g = 2.f * r0;
    for (int i = 0; i < A.K; ++i) {
        const int k = A.ksize[i], R = k / 2, Vi = EM_TILE + 2 * R;
        const float* tap = s_tap + i * EM_KMAX;
        em_blur(A, s_ext, s_h, s_v, tap, k, y0, x0);
        const float vi = inside ? s_v[(ty + R) * Vi + tx + R] : 0.f;
        tot = em_block_sum(s_red, (double)vi * (double)vi);
        if (tid == 0) part[i + 1] = tot;
        for (int e = tid; e < EM_TILE * Vi; e += EM_BLOCK) {            // columns': a[y][x], y in the tile, x in tile +- R
            const int j = e / Vi, m = e - j * Vi;
            const int y = y0 + j;
            s_a[e] = y < A.h ? em_adjoint(s_v + m, Vi, tap, k, y, A.h, y0 - R, Vi) : 0.f;
        }
        __syncthreads();
        if (inside) g += (2.f * A.wk[i]) * em_adjoint(s_a + ty * Vi, 1, tap, k, px, A.w, x0 - R, Vi);
        __syncthreads();
    }

    // the channel of the active hinge owns the pixel's gradient: + writes where d >= 0 (the zeros of a tie too), - where d < 0
    if (inside && (c == 1) == !(d < 0.f)) {
        float s = 0.f;
        if (yraw >= 0.f) {
            const float den = yraw + A.eps;
            if (d > 0.f) s = g / (A.c_pos * den);
            else if (d < 0.f) s = -g / (A.c_neg * den);
            else if (d != d) s = d;                     // (NaN from the previous frame's luminance)
        } else if (yraw != yraw) {
            s = yraw;                                   // a NaN colour has a NaN gradient: the failure reaches the pose
        }
        A.grad[3 * o + 0] = 0.299f * s;
        A.grad[3 * o + 1] = 0.587f * s;
        A.grad[3 * o + 2] = 0.114f * s;
    }
}

struct EmFinishArgs {
    const double* partials;
    int64_t rows;
    int K;
    float wk[EM_NK];
    double* sums;                   // [K + 2]
};

__global__ __launch_bounds__(64) void event_model_finish_kernel(EmFinishArgs A) {
    __shared__ double s_term[EM_NK + 1];
    const int j = threadIdx.x;
    if (j <= A.K) {
        double acc = 0.0;
        for (int64_t r = 0; r < A.rows; ++r) acc += A.partials[r * (A.K + 1) + j];
        s_term[j] = acc;
        A.sums[j] = acc;
    }
    __syncthreads();
    if (j == 0) {
        double loss = s_term[0];
        for (int i = 0; i < A.K; ++i) loss += (double)A.wk[i] * s_term[i + 1];
        A.sums[A.K + 1] = loss;
    }
}

}  // namespace

int64_t ens_event_model_workspace_bytes(int h, int w, int K) {
    const int64_t tiles = (int64_t)((h + EM_TILE - 1) / EM_TILE) * ((w + EM_TILE - 1) / EM_TILE);
    return tiles * 2 * (K + 1) * (int64_t)sizeof(double);
}

int ens_launch_event_model(const EventModelJob& J, hipStream_t st) {
    EmArgs A;
    A.cur = J.cur; A.prev = J.prev; A.gt = J.gt; A.h = J.h; A.w = J.w; A.K = J.K;
    A.c_neg = J.c_neg; A.c_pos = J.c_pos; A.eps = J.eps;
    A.rmax = 0;
    for (int i = 0; i < EM_NK; ++i) {
        A.ksize[i] = i < J.K ? J.ksizes[i] : 1;
        A.wk[i] = i < J.K ? J.weights[i] : 0.f;
        for (int t = 0; t < EM_KMAX; ++t) A.taps[i][t] = (i < J.K && t < J.ksizes[i]) ? J.taps[i * EM_KMAX + t] : 0.f;
        if (i < J.K && J.ksizes[i] / 2 > A.rmax) A.rmax = J.ksizes[i] / 2;
    }
    A.pred = J.pred; A.grad = J.grad; A.partials = (double*)J.workspace; A.blur_gt = J.blur_gt; A.blur_pred = J.blur_pred;
    const dim3 grid((unsigned)((J.w + EM_TILE - 1) / EM_TILE), (unsigned)((J.h + EM_TILE - 1) / EM_TILE), 2);
    event_model_tile_kernel<<<grid, EM_BLOCK, 0, st>>>(A);
    if (hipGetLastError() != hipSuccess) return ENSLAM_ELAUNCH;
    EmFinishArgs F;
    F.partials = A.partials; F.rows = (int64_t)grid.x * grid.y * 2; F.K = J.K; F.sums = J.sums;
    for (int i = 0; i < EM_NK; ++i) F.wk[i] = A.wk[i];
    event_model_finish_kernel<<<1, 64, 0, st>>>(F);
    return hipGetLastError() == hipSuccess ? ENSLAM_OK : ENSLAM_ELAUNCH;
}
