// Event network on the device: UNet_2heads(6, 2, 2), bilinear, float32 -- forward, the gradient with respect to the input
// image and the gradients of the parameters (event.py: UNet_2heads; reference event_net/unet_model.py:72-122, unet_parts.py).
//
// The network is written down once, as a table (EN_CONV: per convolution its level and where its one or two inputs come
// from).  One planner lays out the workspace from it, and one forward walk and one backward walk launch the kernels from
// it, per image.  Two routes bind the walks:
//   folded         eval-mode BatchNorm, one image (enslam_eventnet_forward / _backward / _backward_weights).  Every
//                  conv - BN - ReLU triple is one 3x3 convolution with folded weights w' = w * gamma / sqrt(var + eps),
//                  b' = beta - mean * gamma / sqrt(var + eps) (event.py folds in float64 and rounds once; fold_pack does it on
//                  the device for live parameters), bias and ReLU in the convolution's epilogue.
//   training mode  batch statistics, B images (enslam_eventnet_train_forward / _train_backward).  The convolutions run
//                  unfolded and write the raw z; the BatchNorm kernels, which alone see the whole batch, follow each one.
// Activations are channels-last ([H*W][C], images one after the other) so the reduction axis of a tap is contiguous; the
// public tensors stay [B,C,H,W] (en_pack_x / en_unpack_gx / the heads convert).
//
//   conv3x3_kernel   implicit GEMM  out[p][n] = sum_{tap, c} in[p + tap][c] * w[(tap, c)][n]  on v_mfma_f32_32x32x2_f32
//                    (exact f32, an fmaf chain in k order).  One workgroup (4 waves as 2 x 2) owns 64 pixels x 64 output
//                    channels, one 32 x 32 accumulator tile per wave; the reduction runs in chunks of 32 k staged in LDS
//                    (A transposed [k][pixel], row stride 65; B [k][n]), the next chunk's global loads issued before the
//                    current chunk's MFMAs.  The input may be two sources read in place: the skip and the up-sampled
//                    deep feature with its centred zero padding (torch.cat / F.pad are not materialised).  The input
//                    gradient is the SAME kernel on weights packed flipped and transposed: the incoming gradient is
//                    masked at load by saved_out > 0 (relu'(0) = 0 as in torch), and where the forward read two sources
//                    the result goes to two destinations.  Layers with few pixels split the reduction over
//                    blockIdx.z; conv3x3_reduce_kernel sums the partials in split order: no atomics, results are
//                    bit-reproducible.
//   pool2 / up2      nn.MaxPool2d(2) and x2 bilinear up-sampling (align_corners=True) with their backward passes as
//                    gathers (pool: the window's first maximum in row-major order takes the gradient, torch's tie rule;
//                    up: torch's float32 source-coordinate expression, so the interpolation weights are F.interpolate's).
//   heads            the two 1x1 heads fused (sigmoid on head 2), and their backward into the 64-channel features.
//
// The weight gradients (of the packed image on the folded route, of the parameters in training mode):
//   conv3x3_wgrad_kernel   implicit GEMM  dWf[tap * Cin + c][n] = sum_p in[p + tap][c] * G[p][n],  G = g where saved_out > 0,
//                    on the same MFMA.  One workgroup (4 waves as 2 x 2) owns 64 weight rows x 64 output channels; the
//                    reduction runs over the pixels in chunks of 32 staged in LDS, both operands as [pixel][row] (both are
//                    channels-last in memory: no transpose), the next chunk's loads issued before the current chunk's
//                    MFMAs.  The input is read as the forward reads it (zero outside the image per tap, two sources in
//                    place).  The workgroups of the first row tile also sum G's columns: the bias gradient.  Layers with
//                    few output tiles split the PIXEL axis over blockIdx.z; conv3x3_wgrad_reduce_kernel sums the partials
//                    in split order (no atomics).
//   heads_wgrad      gradients of the heads block, a fixed-order two-stage reduction over the pixels.
//
// The BatchNorm kernels (enslam_eventnet_bn_*) and the unfolded weights' packing have their own notes further down; the
// planner, the two walks and the whole-network entries of both routes are the last section of this file.
#include "../../include/enslam_hip.h"
#include "common.hpp"
#include <algorithm>

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int EN_TM = 64;             // pixels per workgroup
constexpr int EN_TN = 64;             // output channels per workgroup
constexpr int EN_KC = 32;             // reduction chunk
constexpr int EN_LDA = EN_TM + 1;     // LDS row stride of the A chunk (floats)
constexpr int EN_THREADS = 256;
constexpr int EN_SPLIT_BELOW = 256;   // layers with fewer output tiles than this split the reduction ...
constexpr int EN_SPLIT_TARGET = 512;  // ... to about this many workgroups
constexpr int EN_NCONV = 26;
constexpr int EN_HEADS_FLOATS = 264;  // W1 [2][64] | W2 [2][64] | b1 [2] | b2 [2] | pad

struct ConvArgs {
    const float* w;       // [9 * (C0 + C1)][N]
    const float* bias;    // [N] or null
    const float* s0;      // [H * W][C0]
    const float* s1;      // [sH1 * sW1][C1]: conv pixel (y, x) reads (y - soy, x - sox), zero outside; null iff C1 == 0
    const float* mask;    // layout of s0 or null: s0's values count only where mask > 0
    float* d0;            // [H * W][N0]
    float* d1;            // [dH1 * dW1][N - N0]: conv pixel (y, x) writes (y - doy, x - dox), dropped outside; null iff N0 == N
    float* part;          // [splits][H * W][N]
    int H, W, C0, C1, sH1, sW1, soy, sox;
    int N, N0, dH1, dW1, doy, dox;
    int relu, acc0, acc1;
    int nchunks, cps;     // chunks in all / per split
};

ENS_DEV f32x16 mfma32(float a, float b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0); }
// C/D map of the 32x32 f32 MFMA: column lane & 31, row (v & 3) + 8 (v >> 2) + 4 (lane >> 5)
ENS_DEV int c_row(int v, int lane) { return (v & 3) + 8 * (v >> 2) + 4 * (lane >> 5); }

ENS_DEV void conv_emit(const ConvArgs& a, int p, int n, float v) {
    if (a.bias) v = v + a.bias[n];
    if (a.relu) v = v > 0.f ? v : 0.f;
    float* q;
    int acc;
    if (n < a.N0) {
        q = a.d0 + (int64_t)p * a.N0 + n;
        acc = a.acc0;
    } else {
        const int y = p / a.W - a.doy, x = p % a.W - a.dox;
        if (y < 0 || y >= a.dH1 || x < 0 || x >= a.dW1) return;
        q = a.d1 + ((int64_t)y * a.dW1 + x) * (a.N - a.N0) + (n - a.N0);
        acc = a.acc1;
    }
    *q = acc ? *q + v : v;
}

__global__ __launch_bounds__(EN_THREADS) void conv3x3_kernel(ConvArgs a) {
    __shared__ float As[EN_KC * EN_LDA];
    __shared__ __attribute__((aligned(16))) float Bs[EN_KC * EN_TN];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, wm = wave & 1, wn = wave >> 1;
    const int r = lane & 31, h = lane >> 5;
    const int P = a.H * a.W, Cin = a.C0 + a.C1, K = 9 * Cin;
    const int p0 = blockIdx.x * EN_TM, n0 = blockIdx.y * EN_TN;
    // loader roles.  A: 4 channels (kq) of pixels t >> 3 and 32 + (t >> 3); B: 4 columns (bc) of rows t >> 4 and 16 + (t >> 4)
    const int kq = t & 7, apx = t >> 3, brow = t >> 4, bc = (t & 15) * 4;
    int ay[2], ax[2];
    bool aok[2];
    for (int i = 0; i < 2; ++i) {
        const int p = p0 + apx + 32 * i;
        aok[i] = p < P;
        ay[i] = aok[i] ? p / a.W : 0;
        ax[i] = aok[i] ? p % a.W : 0;
    }
    const bool bok = n0 + bc < a.N;        // N is a multiple of 4
    f32x4 av[2], bv[2];
    auto load = [&](int ch) {
        const int k4 = ch * EN_KC + 4 * kq;
        const int tap = k4 / Cin, c = k4 - tap * Cin;
        const int dy = tap / 3 - 1, dx = tap % 3 - 1;
        for (int i = 0; i < 2; ++i) {
            f32x4 v = splat4(0.f);
            const int yy = ay[i] + dy, xx = ax[i] + dx;
            if (k4 < K && aok[i] && yy >= 0 && yy < a.H && xx >= 0 && xx < a.W) {
                if (c < a.C0) {
                    const int64_t idx = ((int64_t)yy * a.W + xx) * a.C0 + c;
                    v = ld4(a.s0 + idx);
                    if (a.mask) {
                        const f32x4 m = ld4(a.mask + idx);
                        for (int e = 0; e < 4; ++e) v[e] = m[e] > 0.f ? v[e] : 0.f;
                    }
                } else {
                    const int y1 = yy - a.soy, x1 = xx - a.sox;
                    if (y1 >= 0 && y1 < a.sH1 && x1 >= 0 && x1 < a.sW1)
                        v = ld4(a.s1 + ((int64_t)y1 * a.sW1 + x1) * a.C1 + (c - a.C0));
                }
            }
            av[i] = v;
            const int k = ch * EN_KC + brow + 16 * i;
            bv[i] = (k < K && bok) ? ld4(a.w + (int64_t)k * a.N + n0 + bc) : splat4(0.f);
        }
    };
    f32x16 acc;
    for (int v = 0; v < 16; ++v) acc[v] = 0.f;
    const int c_begin = blockIdx.z * a.cps;
    const int c_end = min(c_begin + a.cps, a.nchunks);
    if (c_begin < c_end) load(c_begin);
    for (int ch = c_begin; ch < c_end; ++ch) {
        __syncthreads();                       // every wave has finished reading the previous chunk
        for (int i = 0; i < 2; ++i) {
            for (int e = 0; e < 4; ++e) As[(4 * kq + e) * EN_LDA + apx + 32 * i] = av[i][e];
            *reinterpret_cast<f32x4*>(&Bs[(brow + 16 * i) * EN_TN + bc]) = bv[i];
        }
        __syncthreads();
        if (ch + 1 < c_end) load(ch + 1);      // in flight under this chunk's MFMAs
        for (int kk = 0; kk < EN_KC; kk += 2)
            acc = mfma32(As[(kk + h) * EN_LDA + 32 * wm + r], Bs[(kk + h) * EN_TN + 32 * wn + r], acc);
    }
    const int n = n0 + 32 * wn + r;
    if (n >= a.N) return;
    const bool split = gridDim.z > 1;
    for (int v = 0; v < 16; ++v) {
        const int p = p0 + 32 * wm + c_row(v, lane);
        if (p >= P) continue;
        if (split) a.part[((int64_t)blockIdx.z * P + p) * a.N + n] = acc[v];
        else conv_emit(a, p, n, acc[v]);
    }
}

__global__ __launch_bounds__(256) void conv3x3_reduce_kernel(ConvArgs a, int splits) {
    const int64_t PN = (int64_t)a.H * a.W * a.N;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= PN) return;
    float s = a.part[i];
    for (int k = 1; k < splits; ++k) s = s + a.part[k * PN + i];     // fixed order
    conv_emit(a, (int)(i / a.N), (int)(i % a.N), s);
}

// ---------------------------------------------------------------------------------------------------------------
// 2x2 max pool, [H][W][C] -> [H/2][W/2][C] (floor).  The first maximum in row-major order wins (ATen: val > max).
// ---------------------------------------------------------------------------------------------------------------
ENS_DEV int pool_argmax(const float* in, int W, int C, int oy, int ox, int c, float& best) {
    int arg = 0;
    best = in[((int64_t)(2 * oy) * W + 2 * ox) * C + c];
    for (int k = 1; k < 4; ++k) {
        const float v = in[((int64_t)(2 * oy + (k >> 1)) * W + 2 * ox + (k & 1)) * C + c];
        if (v > best || v != v) { best = v; arg = k; }
    }
    return arg;
}

__global__ __launch_bounds__(256) void pool2_fwd_kernel(const float* __restrict__ in, int H, int W, int C,
                                                        float* __restrict__ out) {
    const int Ho = H / 2, Wo = W / 2;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)Ho * Wo * C) return;
    const int c = (int)(i % C), q = (int)(i / C);
    float best;
    pool_argmax(in, W, C, q / Wo, q % Wo, c, best);
    out[i] = best;
}

// d_in[H][W][C] (=, or += with acc) g_out[H/2][W/2][C] where the pixel is its window's first maximum; 0 elsewhere
__global__ __launch_bounds__(256) void pool2_bwd_kernel(const float* __restrict__ in, int H, int W, int C,
                                                        const float* __restrict__ g_out, float* __restrict__ d_in, int acc) {
    const int Ho = H / 2, Wo = W / 2;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)H * W * C) return;
    const int c = (int)(i % C), p = (int)(i / C), y = p / W, x = p % W;
    float g = 0.f;
    if (y < 2 * Ho && x < 2 * Wo) {
        float best;
        const int arg = pool_argmax(in, W, C, y / 2, x / 2, c, best);
        if (arg == 2 * (y & 1) + (x & 1)) g = g_out[((int64_t)(y / 2) * Wo + x / 2) * C + c];
    }
    d_in[i] = acc ? d_in[i] + g : g;
}

// ---------------------------------------------------------------------------------------------------------------
// x2 bilinear up-sampling, align_corners=True, [h][w][C] -> [2h][2w][C].  ATen (UpSample.h): scale = (in - 1) / (out - 1)
// in float32 (0 when out == 1), src = scale * dst, i0 = floor(src), i1 = i0 + (i0 < in - 1), l1 = src - i0, l0 = 1 - l1;
// value = l0y * (l0x * v00 + l1x * v01) + l1y * (l0x * v10 + l1x * v11).
// ---------------------------------------------------------------------------------------------------------------
ENS_DEV float up_scale(int in, int out) { return out > 1 ? (float)(in - 1) / (float)(out - 1) : 0.f; }
ENS_DEV void up_src(float scale, int dst, int in, int& i0, int& i1, float& l0, float& l1) {
    const float src = scale * (float)dst;
    i0 = min((int)floorf(src), in - 1);
    i1 = i0 + (i0 < in - 1 ? 1 : 0);
    l1 = fminf(fmaxf(src - (float)i0, 0.f), 1.f);
    l0 = 1.f - l1;
}

__global__ __launch_bounds__(256) void up2_fwd_kernel(const float* __restrict__ in, int h, int w, int C,
                                                      float* __restrict__ out) {
    const int Ho = 2 * h, Wo = 2 * w;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)Ho * Wo * C) return;
    const int c = (int)(i % C), q = (int)(i / C), Y = q / Wo, X = q % Wo;
    int y0, y1, x0, x1;
    float ly0, ly1, lx0, lx1;
    up_src(up_scale(h, Ho), Y, h, y0, y1, ly0, ly1);
    up_src(up_scale(w, Wo), X, w, x0, x1, lx0, lx1);
    const float v00 = in[((int64_t)y0 * w + x0) * C + c], v01 = in[((int64_t)y0 * w + x1) * C + c];
    const float v10 = in[((int64_t)y1 * w + x0) * C + c], v11 = in[((int64_t)y1 * w + x1) * C + c];
    out[i] = ly0 * (lx0 * v00 + lx1 * v01) + ly1 * (lx0 * v10 + lx1 * v11);
}

// the output rows whose stencil can touch input row i: floor(scale * Y) in {i - 1, i}, with one row of slack either side
ENS_DEV void up_range(float scale, int i, int out, int& lo, int& hi) {
    if (scale <= 0.f) { lo = 0; hi = out - 1; return; }
    lo = max(0, (int)floorf((float)(i - 1) / scale) - 1);
    hi = min(out - 1, (int)ceilf((float)(i + 1) / scale) + 1);
}

// d_in[h][w][C] (=, or += with acc) the gather of g_out[2h][2w][C]: output pixels in ascending (Y, X) order
__global__ __launch_bounds__(256) void up2_bwd_kernel(const float* __restrict__ g_out, int h, int w, int C,
                                                      float* __restrict__ d_in, int acc) {
    const int Ho = 2 * h, Wo = 2 * w;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)h * w * C) return;
    const int c = (int)(i % C), p = (int)(i / C), y = p / w, x = p % w;
    const float sy = up_scale(h, Ho), sx = up_scale(w, Wo);
    int Ylo, Yhi, Xlo, Xhi;
    up_range(sy, y, Ho, Ylo, Yhi);
    up_range(sx, x, Wo, Xlo, Xhi);
    float s = 0.f;
    for (int Y = Ylo; Y <= Yhi; ++Y) {
        int y0, y1, x0, x1;
        float ly0, ly1, lx0, lx1;
        up_src(sy, Y, h, y0, y1, ly0, ly1);
        const float wy = (y0 == y ? ly0 : 0.f) + (y1 == y ? ly1 : 0.f);
        if (y0 != y && y1 != y) continue;
        for (int X = Xlo; X <= Xhi; ++X) {
            up_src(sx, X, w, x0, x1, lx0, lx1);
            if (x0 != x && x1 != x) continue;
            const float wx = (x0 == x ? lx0 : 0.f) + (x1 == x ? lx1 : 0.f);
            s = fmaf(wy * wx, g_out[((int64_t)Y * Wo + X) * C + c], s);
        }
    }
    d_in[i] = acc ? d_in[i] + s : s;
}

// ---------------------------------------------------------------------------------------------------------------
// layout changes of the public tensors and the heads
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void en_pack_x_kernel(const float* __restrict__ x, int P, float* __restrict__ x8) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P * 8) return;
    const int c = i & 7, p = i >> 3;
    x8[i] = c < 6 ? x[(int64_t)c * P + p] : 0.f;
}

__global__ __launch_bounds__(256) void en_unpack_gx_kernel(const float* __restrict__ g8, int P, float* __restrict__ gx) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P * 6) return;
    const int c = i / P, p = i % P;
    gx[i] = g8[(int64_t)p * 8 + c];
}

// hw: W1 [2][64] | W2 [2][64] | b1 [2] | b2 [2].  events [2][P] = W1 f1 + b1, probs [2][P] = sigmoid(W2 f2 + b2)
__global__ __launch_bounds__(256) void heads_fwd_kernel(const float* __restrict__ hw, const float* __restrict__ f1,
                                                        const float* __restrict__ f2, int P, float* __restrict__ events,
                                                        float* __restrict__ probs, float* __restrict__ probs_saved) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= 2 * P) return;
    const int head = i / P, p = i % P;
    const float* f = (head ? f2 : f1) + (int64_t)p * 64;
    const float* w = hw + 128 * head;
    float s0 = 0.f, s1 = 0.f;
    for (int c = 0; c < 64; c += 4) {
        const f32x4 v = ld4(f + c);
        for (int e = 0; e < 4; ++e) { s0 = fmaf(v[e], w[c + e], s0); s1 = fmaf(v[e], w[64 + c + e], s1); }
    }
    s0 = s0 + hw[256 + 2 * head];
    s1 = s1 + hw[257 + 2 * head];
    if (head) {
        const float q0 = 1.f / (1.f + expf(-s0)), q1 = 1.f / (1.f + expf(-s1));
        probs[p] = q0;
        probs[P + p] = q1;
        probs_saved[p] = q0;
        probs_saved[P + p] = q1;
    } else {
        events[p] = s0;
        events[P + p] = s1;
    }
}

// g_f [P][64] of head `head`: W^T g (head 1: g through the sigmoid, s (1 - s) from the saved probabilities)
__global__ __launch_bounds__(256) void heads_bwd_kernel(const float* __restrict__ hw, int head, const float* __restrict__ g,
                                                        const float* __restrict__ probs, int P, float* __restrict__ g_f) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P * 64) return;
    const int c = i & 63, p = i >> 6;
    float g0 = g[p], g1 = g[P + p];
    if (head) {
        const float q0 = probs[p], q1 = probs[P + p];
        g0 = g0 * (q0 * (1.f - q0));
        g1 = g1 * (q1 * (1.f - q1));
    }
    const float* w = hw + 128 * head;
    g_f[i] = fmaf(g1, w[64 + c], g0 * w[c]);
}

// ---------------------------------------------------------------------------------------------------------------
// weight gradients
// ---------------------------------------------------------------------------------------------------------------
struct WgradArgs {
    const float* s0;      // [H * W][C0]: the convolution's input ...
    const float* s1;      // ... and its second source [sH1 * sW1][C1] at (soy, sox), zero outside; null iff C1 == 0
    const float* g;       // [H * W][N]: gradient of the convolution's output
    const float* saved;   // [H * W][N] or null: g counts only where saved > 0
    float* dw;            // [9 * (C0 + C1)][N]
    float* db;            // [N] or null
    float* part;          // [splits][9 * (C0 + C1) * N + N]
    int H, W, C0, C1, sH1, sW1, soy, sox, N;
    int nchunks, cps;     // pixel chunks in all / per split
};

constexpr int EN_WG_PC = 32;          // pixels per chunk

__global__ __launch_bounds__(EN_THREADS) void conv3x3_wgrad_kernel(WgradArgs a) {
    __shared__ __attribute__((aligned(16))) float As[EN_WG_PC * EN_TM];     // [pixel][weight row]
    __shared__ __attribute__((aligned(16))) float Bs[EN_WG_PC * EN_TN];     // [pixel][output channel]
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, wm = wave & 1, wn = wave >> 1;
    const int r = lane & 31, h = lane >> 5;
    const int P = a.H * a.W, Cin = a.C0 + a.C1, M = 9 * Cin;
    const int m0 = blockIdx.x * EN_TM, n0 = blockIdx.y * EN_TN;
    // loader roles: 4 rows / columns (q) of pixels t >> 4 and 16 + (t >> 4) of the chunk.  Cin is a multiple of 8, so the
    // four rows share a tap and a source.
    const int q = (t & 15) * 4, px = t >> 4;
    const int m4 = m0 + q;
    const bool mok = m4 < M, nok = n0 + q < a.N;           // M and N are multiples of 4
    const int tap = mok ? m4 / Cin : 0, c = mok ? m4 - tap * Cin : 0;
    const int dy = tap / 3 - 1, dx = tap % 3 - 1;
    f32x4 av[2], bv[2];
    auto load = [&](int ch) {
        for (int i = 0; i < 2; ++i) {
            const int p = ch * EN_WG_PC + px + 16 * i;
            f32x4 va = splat4(0.f), vb = splat4(0.f);
            if (p < P) {
                const int y = p / a.W, x = p - y * a.W;
                const int yy = y + dy, xx = x + dx;
                if (mok && yy >= 0 && yy < a.H && xx >= 0 && xx < a.W) {
                    if (c < a.C0) {
                        va = ld4(a.s0 + ((int64_t)yy * a.W + xx) * a.C0 + c);
                    } else {
                        const int y1 = yy - a.soy, x1 = xx - a.sox;
                        if (y1 >= 0 && y1 < a.sH1 && x1 >= 0 && x1 < a.sW1)
                            va = ld4(a.s1 + ((int64_t)y1 * a.sW1 + x1) * a.C1 + (c - a.C0));
                    }
                }
                if (nok) {
                    const int64_t idx = (int64_t)p * a.N + n0 + q;
                    vb = ld4(a.g + idx);
                    if (a.saved) {
                        const f32x4 s = ld4(a.saved + idx);
                        for (int e = 0; e < 4; ++e) vb[e] = s[e] > 0.f ? vb[e] : 0.f;
                    }
                }
            }
            av[i] = va;
            bv[i] = vb;
        }
    };
    f32x16 acc;
    for (int v = 0; v < 16; ++v) acc[v] = 0.f;
    float bsum = 0.f;                                      // column t of G, summed by the first row tile's first wave
    const bool do_bias = blockIdx.x == 0 && t < EN_TN;
    const int c_begin = blockIdx.z * a.cps;
    const int c_end = min(c_begin + a.cps, a.nchunks);
    if (c_begin < c_end) load(c_begin);
    for (int ch = c_begin; ch < c_end; ++ch) {
        __syncthreads();                       // every wave has finished reading the previous chunk
        for (int i = 0; i < 2; ++i) {
            *reinterpret_cast<f32x4*>(&As[(px + 16 * i) * EN_TM + q]) = av[i];
            *reinterpret_cast<f32x4*>(&Bs[(px + 16 * i) * EN_TN + q]) = bv[i];
        }
        __syncthreads();
        if (ch + 1 < c_end) load(ch + 1);      // in flight under this chunk's MFMAs
        for (int kk = 0; kk < EN_WG_PC; kk += 2)
            acc = mfma32(As[(kk + h) * EN_TM + 32 * wm + r], Bs[(kk + h) * EN_TN + 32 * wn + r], acc);
        if (do_bias)
            for (int kk = 0; kk < EN_WG_PC; ++kk) bsum = bsum + Bs[kk * EN_TN + t];
    }
    const int64_t MN = (int64_t)M * a.N;
    const bool split = gridDim.z > 1;
    float* dw = split ? a.part + (int64_t)blockIdx.z * (MN + a.N) : a.dw;
    float* db = split ? dw + MN : a.db;
    if (do_bias && db && n0 + t < a.N) db[n0 + t] = bsum;
    const int n = n0 + 32 * wn + r;
    if (n >= a.N) return;
    for (int v = 0; v < 16; ++v) {
        const int m = m0 + 32 * wm + c_row(v, lane);
        if (m < M) dw[(int64_t)m * a.N + n] = acc[v];
    }
}

__global__ __launch_bounds__(256) void conv3x3_wgrad_reduce_kernel(WgradArgs a, int splits) {
    const int64_t MN = (int64_t)9 * (a.C0 + a.C1) * a.N, total = MN + a.N;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    float s = a.part[i];
    for (int k = 1; k < splits; ++k) s = s + a.part[k * total + i];     // fixed order
    if (i < MN) a.dw[i] = s;
    else if (a.db) a.db[i - MN] = s;
}

// Heads block gradient, stage 1: block b sums its pixel range.  Thread t owns weight t of W1 | W2 ([2][2][64]: head, row,
// channel); the threads of channel 0 also own the row's bias.  part [blocks][260].
__global__ __launch_bounds__(256) void heads_wgrad_kernel(const float* __restrict__ g_events, const float* __restrict__ g_probs,
                                                          const float* __restrict__ probs, const float* __restrict__ f1,
                                                          const float* __restrict__ f2, int P, int per_block,
                                                          float* __restrict__ part) {
    const int t = threadIdx.x, head = t >> 7, row = (t >> 6) & 1, c = t & 63;
    const float* g = (head ? g_probs : g_events) + (int64_t)row * P;
    const float* pr = probs + (int64_t)row * P;
    const float* f = head ? f2 : f1;
    const int p_begin = blockIdx.x * per_block, p_end = min(p_begin + per_block, P);
    float sw = 0.f, sb = 0.f;
    for (int p = p_begin; p < p_end; ++p) {
        float gv = g[p];
        if (head) {
            const float qv = pr[p];
            gv = gv * (qv * (1.f - qv));
        }
        sw = fmaf(gv, f[(int64_t)p * 64 + c], sw);
        sb = sb + gv;
    }
    part[(int64_t)blockIdx.x * 260 + t] = sw;
    if (c == 0) part[(int64_t)blockIdx.x * 260 + 256 + 2 * head + row] = sb;
}

// stage 2: the partials in block order; the pad of the heads block is written as zero
__global__ __launch_bounds__(EN_HEADS_FLOATS) void heads_wgrad_reduce_kernel(const float* __restrict__ part, int blocks,
                                                                             float* __restrict__ g_heads) {
    const int t = threadIdx.x;
    float s = 0.f;
    if (t < 260) {
        s = part[t];
        for (int b = 1; b < blocks; ++b) s = s + part[(int64_t)b * 260 + t];
    }
    g_heads[t] = s;
}

// ---------------------------------------------------------------------------------------------------------------
// The packed image from live parameters, and its chain rule back to them (training: the weights change every step).
// One convolution: Wf, b, Wt of event.pack_conv from w [cout][cin][3][3], BatchNorm gamma / beta and the host's float64
// sq = sqrt(var + eps), shift = -mean, with event.fold_event_net's float64 operations in its order, rounded once:
//   s = gamma / sq,  w' = float(w * s),  b' = float(beta + shift * s).
// A workgroup moves a 32 (cout) x 32 (cin) x 9 tile through LDS so that reads and writes are both contiguous runs.
// ---------------------------------------------------------------------------------------------------------------
constexpr int EN_FT = 32;                     // tile edge in output and in input channels
constexpr int EN_FLD = EN_FT * 9 + 1;         // LDS row stride (floats): 289, odd, so columns spread over the banks

struct FoldArgs {
    const float* w;        // [cout][cin][3][3]
    const float* gamma;    // [cout]
    const float* beta;     // [cout]
    const double* sq;      // [cout]
    const double* shift;   // [cout]
    float* wf;             // [9 cinp][cout]   (forward: written; backward: the gradient, read)
    float* b;              // [cout]
    float* wt;             // [9 cout][cinp]   (forward only)
    float* dw;             // [cout][cin][3][3]                 (backward)
    double* part;          // [cinp / 32 tiles][cout]           (backward: per-tile sums of dWf * w)
    float* dgamma;         // [cout]                            (backward)
    float* dbeta;          // [cout]                            (backward)
    int cin, cinp, cout;
};
// all 26 convolutions in one launch: workgroup blockIdx.x belongs to convolution i with first[i] <= blockIdx.x < first[i + 1]
struct FoldTable {
    FoldArgs a[EN_NCONV];
    int first[EN_NCONV + 1];
};
static_assert(sizeof(FoldTable) <= 4096, "FoldTable travels as a kernel argument");

ENS_DEV int fold_locate(const FoldTable& tb, int& bx, int& by) {
    int i = 0;
    while (i + 1 < EN_NCONV && (int)blockIdx.x >= tb.first[i + 1]) ++i;
    const int local = blockIdx.x - tb.first[i], tiles = (tb.a[i].cinp + EN_FT - 1) / EN_FT;
    bx = local % tiles;
    by = local / tiles;
    return i;
}

__global__ __launch_bounds__(256) void fold_pack_kernel(FoldTable tb) {
    __shared__ float tile[EN_FT * EN_FLD];
    __shared__ double sS[EN_FT];
    int bx, by;
    const FoldArgs a = tb.a[fold_locate(tb, bx, by)];
    const int t = threadIdx.x, ci0 = bx * EN_FT, co0 = by * EN_FT;
    if (t < EN_FT) {
        const int co = co0 + t;
        const double s = co < a.cout ? (double)a.gamma[co] / a.sq[co] : 0.0;
        sS[t] = s;
        if (bx == 0 && co < a.cout) a.b[co] = (float)((double)a.beta[co] + a.shift[co] * s);
    }
    __syncthreads();
    for (int e = t; e < EN_FT * EN_FT * 9; e += 256) {
        const int row = e / (EN_FT * 9), col = e - row * (EN_FT * 9);
        const int co = co0 + row, ci = ci0 + col / 9;
        float v = 0.f;
        if (co < a.cout && ci < a.cin) v = (float)((double)a.w[((int64_t)co * a.cin + ci0) * 9 + col] * sS[row]);
        tile[row * EN_FLD + col] = v;
    }
    __syncthreads();
    for (int e = t; e < EN_FT * EN_FT * 9; e += 256) {
        const int lo = e & (EN_FT - 1), mid = (e >> 5) & (EN_FT - 1), tap = e >> 10;
        // Wf: lo = cout, mid = cin
        if (co0 + lo < a.cout && ci0 + mid < a.cinp)
            a.wf[((int64_t)tap * a.cinp + ci0 + mid) * a.cout + co0 + lo] = tile[lo * EN_FLD + mid * 9 + tap];
        // Wt: lo = cin, mid = cout, the flipped tap
        if (co0 + mid < a.cout && ci0 + lo < a.cinp)
            a.wt[((int64_t)tap * a.cout + co0 + mid) * a.cinp + ci0 + lo] = tile[mid * EN_FLD + lo * 9 + (8 - tap)];
    }
}

// dw = float(dWf * s) in w's layout, and per (cin tile, cout) the float64 sum of dWf * w in a fixed order
__global__ __launch_bounds__(256) void fold_pack_bwd_kernel(FoldTable tb) {
    __shared__ float tile[EN_FT * EN_FLD];
    __shared__ double red[256];
    __shared__ double sS[EN_FT];
    int bx, by;
    const FoldArgs a = tb.a[fold_locate(tb, bx, by)];
    const int t = threadIdx.x, ci0 = bx * EN_FT, co0 = by * EN_FT;
    if (t < EN_FT) sS[t] = co0 + t < a.cout ? (double)a.gamma[co0 + t] / a.sq[co0 + t] : 0.0;
    for (int e = t; e < EN_FT * EN_FT * 9; e += 256) {
        const int lo = e & (EN_FT - 1), mid = (e >> 5) & (EN_FT - 1), tap = e >> 10;
        float v = 0.f;
        if (co0 + lo < a.cout && ci0 + mid < a.cinp) v = a.wf[((int64_t)tap * a.cinp + ci0 + mid) * a.cout + co0 + lo];
        tile[lo * EN_FLD + mid * 9 + tap] = v;
    }
    __syncthreads();
    // 8 threads per row, each a contiguous run of 36 columns
    const int row = t >> 3, sub = t & 7, co = co0 + row;
    double acc = 0.0;
    for (int k = 0; k < 36; ++k) {
        const int col = sub * 36 + k, ci = ci0 + col / 9;
        if (co < a.cout && ci < a.cin) {
            const int64_t at = ((int64_t)co * a.cin + ci0) * 9 + col;
            const double g = (double)tile[row * EN_FLD + col];
            a.dw[at] = (float)(g * sS[row]);
            acc = acc + g * (double)a.w[at];
        }
    }
    red[t] = acc;
    __syncthreads();
    if (sub == 0 && co < a.cout) {
        double sum = red[t];
        for (int k = 1; k < 8; ++k) sum = sum + red[t + k];
        a.part[(int64_t)bx * a.cout + co] = sum;
    }
}

// dgamma = float((sum over the cin tiles + shift * db) / sq), dbeta = db; blockIdx.y is the convolution
__global__ __launch_bounds__(256) void fold_pack_bwd_finish_kernel(FoldTable tb) {
    const FoldArgs a = tb.a[blockIdx.y];
    const int co = blockIdx.x * blockDim.x + threadIdx.x, tiles = (a.cinp + EN_FT - 1) / EN_FT;
    if (co >= a.cout) return;
    double sum = a.part[co];
    for (int k = 1; k < tiles; ++k) sum = sum + a.part[(int64_t)k * a.cout + co];
    const float db = a.b[co];
    sum = sum + (double)db * a.shift[co];
    a.dgamma[co] = (float)(sum / a.sq[co]);
    a.dbeta[co] = db;
}

// heads block: pack (dir 0: parameters -> block, pad zero) or unpack (dir 1: block gradient -> parameter gradients)
__global__ __launch_bounds__(EN_HEADS_FLOATS) void heads_pack_kernel(float* w1, float* w2, float* b1, float* b2, float* block,
                                                                     int dir) {
    const int t = threadIdx.x;
    float* q = t < 128 ? w1 + t : t < 256 ? w2 + (t - 128) : t < 258 ? b1 + (t - 256) : t < 260 ? b2 + (t - 258) : nullptr;
    if (dir == 0) block[t] = q ? *q : 0.f;
    else if (q) *q = block[t];
}

// ---------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------
inline unsigned blocks_of(int64_t n) { return (unsigned)((n + 255) / 256); }
inline int tiles_of(int64_t n, int tile) { return (int)((n + tile - 1) / tile); }
bool chan_ok(int c) { return c >= 8 && c <= 1024 && c % 8 == 0; }
bool all_set(const void* const* p, int n) {
    for (int k = 0; k < n; ++k)
        if (!p[k]) return false;
    return true;
}

// The one split rule: a launch with fewer than EN_SPLIT_BELOW output tiles splits its reduction (nchunks chunks) over
// blockIdx.z, to about EN_SPLIT_TARGET workgroups; cps chunks per split.
struct Split { int nchunks, cps, splits; };
Split split_plan(int64_t tiles, int nchunks) {
    Split s = {nchunks, nchunks, 1};
    if (tiles < EN_SPLIT_BELOW) {
        const int want = (int)std::min<int64_t>(nchunks, (EN_SPLIT_TARGET + tiles - 1) / tiles);
        s.cps = (nchunks + want - 1) / want;
    }
    s.splits = (nchunks + s.cps - 1) / s.cps;
    return s;
}
// convolution: the tiles cover pixels x output channels, the reduction over 9 Cin runs in chunks of EN_KC
dim3 conv_grid(int64_t P, int Cin, int N, Split& s) {
    const int ptiles = tiles_of(P, EN_TM), ntiles = tiles_of(N, EN_TN);
    s = split_plan((int64_t)ptiles * ntiles, tiles_of(9 * Cin, EN_KC));
    return dim3(ptiles, ntiles, s.splits);
}
// weight gradient: the tiles cover the 9 Cin x N weight block, so the PIXEL axis is what splits, in chunks of EN_WG_PC pixels
dim3 wgrad_grid(int64_t P, int Cin, int N, Split& s) {
    const int mtiles = tiles_of(9 * Cin, EN_TM), ntiles = tiles_of(N, EN_TN);
    s = split_plan((int64_t)mtiles * ntiles, tiles_of(P, EN_WG_PC));
    return dim3(mtiles, ntiles, s.splits);
}
int64_t split_floats(int64_t P, int Cin, int N) {
    Split s;
    conv_grid(P, Cin, N, s);
    return s.splits > 1 ? (int64_t)s.splits * P * N : 0;
}
int64_t wgrad_floats(int64_t P, int Cin, int N) {
    Split s;
    wgrad_grid(P, Cin, N, s);
    return s.splits > 1 ? (int64_t)s.splits * ((int64_t)9 * Cin * N + N) : 0;
}

int launch_conv(ConvArgs a, hipStream_t st) {
    const int64_t P = (int64_t)a.H * a.W;
    Split s;
    const dim3 grid = conv_grid(P, a.C0 + a.C1, a.N, s);
    a.nchunks = s.nchunks;
    a.cps = s.cps;
    conv3x3_kernel<<<grid, EN_THREADS, 0, st>>>(a);
    if (s.splits > 1) conv3x3_reduce_kernel<<<blocks_of(P * a.N), 256, 0, st>>>(a, s.splits);
    return 0;
}

void launch_wgrad(WgradArgs a, hipStream_t st) {
    const int Cin = a.C0 + a.C1;
    Split s;
    const dim3 grid = wgrad_grid((int64_t)a.H * a.W, Cin, a.N, s);
    a.nchunks = s.nchunks;
    a.cps = s.cps;
    conv3x3_wgrad_kernel<<<grid, EN_THREADS, 0, st>>>(a);
    if (s.splits > 1)
        conv3x3_wgrad_reduce_kernel<<<blocks_of((int64_t)9 * Cin * a.N + a.N), 256, 0, st>>>(a, s.splits);
}

// heads: at most 256 blocks, at least 64 pixels each
int heads_wgrad_blocks(int64_t P, int& per_block) {
    per_block = (int)std::max<int64_t>(64, (P + 255) / 256);
    return (int)((P + per_block - 1) / per_block);
}

// ---------------------------------------------------------------------------------------------------------------
// The network, once.  The 26 convolutions in packing order: encoder (inc, down1..4), then per head up1..up4.  Each reads
// one or two sources (torch.cat / F.pad are not materialised: the convolution kernels read both in place):
//   SRC_X8    the packed input image (6 channels padded to 8)
//   SRC_OUT   the output of convolution `conv`
//   SRC_POOL  MaxPool2d(2) of the output of convolution `conv`
//   SRC_UP    the x2 bilinear up-sample of the output of convolution `conv`, centred in the skip's extent (the skip is at
//             most one pixel larger per axis, so the centring offset diff / 2 is zero)
// and `ch` channels come from that source.  Everything the planner and the two walks know about the wiring is read here.
// ---------------------------------------------------------------------------------------------------------------
enum SrcKind { SRC_NONE, SRC_X8, SRC_OUT, SRC_POOL, SRC_UP };
struct Source { SrcKind kind; int conv, ch; };
struct ConvDesc {
    int cout, level;              // output channels; resolution level: H >> level x W >> level
    Source src[2];
    int cin() const { return src[0].ch + src[1].ch; }
};
constexpr Source NO_SRC = {SRC_NONE, -1, 0};
const ConvDesc EN_CONV[EN_NCONV] = {
    {64, 0, {{SRC_X8, -1, 8}, NO_SRC}},                {64, 0, {{SRC_OUT, 0, 64}, NO_SRC}},
    {128, 1, {{SRC_POOL, 1, 64}, NO_SRC}},             {128, 1, {{SRC_OUT, 2, 128}, NO_SRC}},
    {256, 2, {{SRC_POOL, 3, 128}, NO_SRC}},            {256, 2, {{SRC_OUT, 4, 256}, NO_SRC}},
    {512, 3, {{SRC_POOL, 5, 256}, NO_SRC}},            {512, 3, {{SRC_OUT, 6, 512}, NO_SRC}},
    {512, 4, {{SRC_POOL, 7, 512}, NO_SRC}},            {512, 4, {{SRC_OUT, 8, 512}, NO_SRC}},
    // head 0: the skip and the up-sampled deep feature, then the stage's second convolution
    {512, 3, {{SRC_OUT, 7, 512}, {SRC_UP, 9, 512}}},   {256, 3, {{SRC_OUT, 10, 512}, NO_SRC}},
    {256, 2, {{SRC_OUT, 5, 256}, {SRC_UP, 11, 256}}},  {128, 2, {{SRC_OUT, 12, 256}, NO_SRC}},
    {128, 1, {{SRC_OUT, 3, 128}, {SRC_UP, 13, 128}}},  {64, 1, {{SRC_OUT, 14, 128}, NO_SRC}},
    {64, 0, {{SRC_OUT, 1, 64}, {SRC_UP, 15, 64}}},     {64, 0, {{SRC_OUT, 16, 64}, NO_SRC}},
    // head 1
    {512, 3, {{SRC_OUT, 7, 512}, {SRC_UP, 9, 512}}},   {256, 3, {{SRC_OUT, 18, 512}, NO_SRC}},
    {256, 2, {{SRC_OUT, 5, 256}, {SRC_UP, 19, 256}}},  {128, 2, {{SRC_OUT, 20, 256}, NO_SRC}},
    {128, 1, {{SRC_OUT, 3, 128}, {SRC_UP, 21, 128}}},  {64, 1, {{SRC_OUT, 22, 128}, NO_SRC}},
    {64, 0, {{SRC_OUT, 1, 64}, {SRC_UP, 23, 64}}},     {64, 0, {{SRC_OUT, 24, 64}, NO_SRC}}};
// each head's decoder is the convolutions first..last; the 1x1 head reads the 64-channel output of `last`.  The encoder is
// every convolution before EN_HEAD[0].first.
struct HeadDesc { int first, last; };
const HeadDesc EN_HEAD[2] = {{10, 17}, {18, 25}};

// packed image: per convolution  Wf [9 cin][cout] | b [cout] | Wt [9 cout][cin],  then the heads block
struct PackOff { int64_t wf[EN_NCONV], b[EN_NCONV], wt[EN_NCONV], heads, total; };
PackOff pack_offsets() {
    PackOff o;
    int64_t q = 0;
    for (int i = 0; i < EN_NCONV; ++i) {
        const int64_t n = (int64_t)9 * EN_CONV[i].cin() * EN_CONV[i].cout;
        o.wf[i] = q; q += n;
        o.b[i] = q; q += EN_CONV[i].cout;
        o.wt[i] = q; q += n;
    }
    o.heads = q;
    o.total = q + EN_HEADS_FLOATS;
    return o;
}

constexpr int EN_FOLD_PART = 32 * 512;        // float64 partials per convolution: at most 32 cin tiles x 512 cout
// the table's shapes and workgroup ranges; `stride` addresses per convolution in params, the first of them w.  The caller
// fills the remaining addresses.
int fold_shapes(const void* const* params, int stride, FoldTable& tb) {
    int blocks = 0;
    for (int i = 0; i < EN_NCONV; ++i) {
        FoldArgs& a = tb.a[i];
        a = FoldArgs{};
        a.w = (const float*)params[stride * i];
        a.cinp = EN_CONV[i].cin(); a.cin = i ? a.cinp : 6; a.cout = EN_CONV[i].cout;
        tb.first[i] = blocks;
        blocks += tiles_of(a.cinp, EN_FT) * tiles_of(a.cout, EN_FT);
    }
    tb.first[EN_NCONV] = blocks;
    return blocks;
}
// the folded route's table: 5 addresses per convolution (w, gamma, beta, sq float64, shift float64)
int fold_table(const void* const* params, FoldTable& tb) {
    const int blocks = fold_shapes(params, 5, tb);
    for (int i = 0; i < EN_NCONV; ++i) {
        FoldArgs& a = tb.a[i];
        a.gamma = (const float*)params[5 * i + 1]; a.beta = (const float*)params[5 * i + 2];
        a.sq = (const double*)params[5 * i + 3]; a.shift = (const double*)params[5 * i + 4];
    }
    return blocks;
}

}  // namespace

extern "C" {

size_t enslam_eventnet_pack_floats(void) { return (size_t)pack_offsets().total; }

/* params: per convolution 5 device addresses (w, gamma, beta, sq float64, shift float64), then W1, W2, b1, b2 of the heads */
int enslam_eventnet_fold_pack(const void* const* params, float* packed, void* stream) {
    if (!params || !packed) return ENSLAM_EINVAL;
    if (!all_set(params, 5 * EN_NCONV + 4)) return ENSLAM_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    const PackOff po = pack_offsets();
    FoldTable tb;
    const int blocks = fold_table(params, tb);
    for (int i = 0; i < EN_NCONV; ++i) {
        tb.a[i].wf = packed + po.wf[i]; tb.a[i].b = packed + po.b[i]; tb.a[i].wt = packed + po.wt[i];
    }
    fold_pack_kernel<<<blocks, 256, 0, st>>>(tb);
    const void* const* h = params + 5 * EN_NCONV;
    heads_pack_kernel<<<1, EN_HEADS_FLOATS, 0, st>>>((float*)h[0], (float*)h[1], (float*)h[2], (float*)h[3], packed + po.heads, 0);
    return hipGetLastError() == hipSuccess ? ENSLAM_OK : ENSLAM_ELAUNCH;
}

/* grads: per convolution 3 device addresses (dw, dgamma, dbeta), then dW1, dW2, db1, db2; scratch: float64 [26 * 16384] */
int enslam_eventnet_fold_pack_backward(const void* const* params, const float* g_packed, void* const* grads, double* scratch,
                                       void* stream) {
    if (!params || !g_packed || !grads || !scratch) return ENSLAM_EINVAL;
    if (!all_set(params, 5 * EN_NCONV + 4)) return ENSLAM_EINVAL;
    if (!all_set(grads, 3 * EN_NCONV + 4)) return ENSLAM_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    const PackOff po = pack_offsets();
    FoldTable tb;
    const int blocks = fold_table(params, tb);
    for (int i = 0; i < EN_NCONV; ++i) {
        FoldArgs& a = tb.a[i];
        a.wf = const_cast<float*>(g_packed) + po.wf[i]; a.b = const_cast<float*>(g_packed) + po.b[i];
        a.dw = (float*)grads[3 * i]; a.dgamma = (float*)grads[3 * i + 1]; a.dbeta = (float*)grads[3 * i + 2];
        a.part = scratch + (int64_t)i * EN_FOLD_PART;
    }
    fold_pack_bwd_kernel<<<blocks, 256, 0, st>>>(tb);
    fold_pack_bwd_finish_kernel<<<dim3(2, EN_NCONV), 256, 0, st>>>(tb);
    void* const* h = grads + 3 * EN_NCONV;
    heads_pack_kernel<<<1, EN_HEADS_FLOATS, 0, st>>>((float*)h[0], (float*)h[1], (float*)h[2], (float*)h[3],
                                                    const_cast<float*>(g_packed) + po.heads, 1);
    return hipGetLastError() == hipSuccess ? ENSLAM_OK : ENSLAM_ELAUNCH;
}

int enslam_eventnet_conv3x3_wgrad(int32_t H, int32_t W, int32_t C0, int32_t C1, int32_t H1, int32_t W1, int32_t oy, int32_t ox,
                                  int32_t Cn, const float* a0, const float* a1, const float* g, const float* saved, float* dw,
                                  float* db, float* scratch, int64_t scratch_floats, void* stream) {
    if (!a0 || !g || !dw || H < 1 || W < 1 || (int64_t)H * W > (1 << 21)) return ENSLAM_EINVAL;
    if (!chan_ok(C0) || !chan_ok(Cn) || (C1 != 0 && !chan_ok(C1)) || C0 + C1 > 1024) return ENSLAM_EUNSUPPORTED;
    if (C1 && (!a1 || H1 < 1 || W1 < 1 || oy < 0 || ox < 0 || oy + H1 > H || ox + W1 > W)) return ENSLAM_EINVAL;
    const int64_t need = wgrad_floats((int64_t)H * W, C0 + C1, Cn);
    if (need > 0 && (!scratch || scratch_floats < need)) return ENSLAM_EINVAL;
    WgradArgs a = {};
    a.s0 = a0; a.s1 = C1 ? a1 : nullptr; a.g = g; a.saved = saved; a.dw = dw; a.db = db; a.part = scratch;
    a.H = H; a.W = W; a.C0 = C0; a.C1 = C1; a.sH1 = H1; a.sW1 = W1; a.soy = oy; a.sox = ox; a.N = Cn;
    launch_wgrad(a, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? ENSLAM_OK : ENSLAM_ELAUNCH;
}

int enslam_eventnet_conv3x3(const float* w, const float* bias, int32_t H, int32_t W, int32_t C0, int32_t C1, int32_t H1,
                            int32_t W1, int32_t oy, int32_t ox, int32_t Cn, const float* a0, const float* a1, float* d0,
                            float* d1, int32_t relu, int32_t transposed, float* scratch, int64_t scratch_floats,
                            void* stream) {
    if (!w || !a0 || !d0 || H < 1 || W < 1 || (int64_t)H * W > (1 << 21)) return ENSLAM_EINVAL;
    if (!chan_ok(C0) || !chan_ok(Cn) || (C1 != 0 && !chan_ok(C1)) || C0 + C1 > 1024) return ENSLAM_EUNSUPPORTED;
    if (C1 && (H1 < 1 || W1 < 1 || oy < 0 || ox < 0 || oy + H1 > H || ox + W1 > W)) return ENSLAM_EINVAL;
    if (C1 && (transposed ? d1 == nullptr : a1 == nullptr)) return ENSLAM_EINVAL;
    const int Cin = transposed ? Cn : C0 + C1, N = transposed ? C0 + C1 : Cn;
    const int64_t need = split_floats((int64_t)H * W, Cin, N);
    if (need > 0 && (!scratch || scratch_floats < need)) return ENSLAM_EINVAL;
    ConvArgs a = {};
    a.w = w; a.bias = bias; a.part = scratch; a.H = H; a.W = W; a.relu = relu; a.d0 = d0;
    if (!transposed) {
        a.s0 = a0; a.s1 = C1 ? a1 : nullptr; a.C0 = C0; a.C1 = C1; a.sH1 = H1; a.sW1 = W1; a.soy = oy; a.sox = ox;
        a.N = a.N0 = Cn;
    } else {
        a.s0 = a0; a.mask = a1; a.C0 = Cn;
        a.N = C0 + C1; a.N0 = C0; a.d1 = C1 ? d1 : nullptr; a.dH1 = H1; a.dW1 = W1; a.doy = oy; a.dox = ox;
    }
    launch_conv(a, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? ENSLAM_OK : ENSLAM_ELAUNCH;
}

int enslam_eventnet_pool2(const float* in, int32_t H, int32_t W, int32_t C, const float* g_out, float* out, int32_t backward,
                          void* stream) {
    if (!in || !out || (backward && !g_out) || H < 2 || W < 2 || C < 1 || (int64_t)H * W > (1 << 21)) return ENSLAM_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    if (backward) pool2_bwd_kernel<<<blocks_of((int64_t)H * W * C), 256, 0, st>>>(in, H, W, C, g_out, out, 0);
    else pool2_fwd_kernel<<<blocks_of((int64_t)(H / 2) * (W / 2) * C), 256, 0, st>>>(in, H, W, C, out);
    return hipGetLastError() == hipSuccess ? ENSLAM_OK : ENSLAM_ELAUNCH;
}

int enslam_eventnet_up2(const float* in, int32_t h, int32_t w, int32_t C, float* out, int32_t backward, void* stream) {
    if (!in || !out || h < 1 || w < 1 || C < 1 || (int64_t)h * w > (1 << 19)) return ENSLAM_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    if (backward) up2_bwd_kernel<<<blocks_of((int64_t)h * w * C), 256, 0, st>>>(in, h, w, C, out, 0);
    else up2_fwd_kernel<<<blocks_of((int64_t)4 * h * w * C), 256, 0, st>>>(in, h, w, C, out);
    return hipGetLastError() == hipSuccess ? ENSLAM_OK : ENSLAM_ELAUNCH;
}

}  // extern "C"

// ===============================================================================================================
// Training-mode BatchNorm and batches (enslam_eventnet_bn_*, enslam_eventnet_train_*): the unfolded network.  Every
// convolution writes its raw output z [B*H*W][C]; BatchNorm's batch statistics couple the images of a batch, so its three
// kernels see all M = B*H*W rows at once, while the convolution / pooling / up-sampling / weight-gradient launchers above
// run once per image.
//
// The BatchNorm kernels are bandwidth-bound streams over a row-major [M][C] matrix.  A workgroup owns BN_ROWS consecutive rows
// of a slab of up to BN_SLAB channels: a slab's row is cw / 4 float4 loads by consecutive threads (tpr threads per row), and
// 256 / tpr rows are in flight per pass, so a wave's loads are contiguous runs of at least 32 bytes at C = 8, whole 256-byte
// rows at C = 64 and 1 KiB runs at C = 1024.  The split of M (chunks of BN_ROWS rows) depends on M alone, and every sum runs in
// a fixed order (thread-private over its rows, then over the row sub-sets in LDS, then over the chunks), all in float64: two
// runs, and two boxes, are bit-equal.
// ===============================================================================================================
namespace {

constexpr int BN_ROWS = 256;
constexpr int BN_SLAB = 256;
constexpr int BN_THREADS = 256;
constexpr int EN_BN_CHANNELS = 5888;          // the 26 BatchNorms' channels in all

struct BnGeom {
    int c0, cw, tpr, rp, c4, rs, r0, r1;
    bool active;
};
ENS_DEV BnGeom bn_geom(int M, int C) {
    BnGeom g;
    g.c0 = blockIdx.y * BN_SLAB;
    g.cw = min(BN_SLAB, C - g.c0);
    g.tpr = g.cw / 4;
    g.rp = BN_THREADS / g.tpr;
    g.active = (int)threadIdx.x < g.tpr * g.rp;
    g.c4 = threadIdx.x % g.tpr;
    g.rs = threadIdx.x / g.tpr;
    g.r0 = blockIdx.x * BN_ROWS;
    g.r1 = min(g.r0 + BN_ROWS, M);
    return g;
}
// v summed over the workgroup's row sub-sets in ascending order; the result is valid in the threads with rs == 0
ENS_DEV void bn_reduce(double (*red)[4], const BnGeom& g, double v[4]) {
    __syncthreads();
    if (g.active)
        for (int e = 0; e < 4; ++e) red[threadIdx.x][e] = v[e];
    __syncthreads();
    if (g.active && g.rs == 0)
        for (int e = 0; e < 4; ++e) {
            double s = red[g.c4][e];
            for (int k = 1; k < g.rp; ++k) s = s + red[k * g.tpr + g.c4][e];
            v[e] = s;
        }
}

// per chunk and channel: the chunk's mean and its centred sum of squares (two passes over the chunk, the second from cache).
// part [chunks][2][C]
__global__ __launch_bounds__(BN_THREADS) void bn_stats_chunk_kernel(const float* __restrict__ z, int M, int C,
                                                                    double* __restrict__ part) {
    __shared__ double red[BN_THREADS][4];
    __shared__ double smean[BN_SLAB];
    const BnGeom g = bn_geom(M, C);
    const float* base = z + g.c0 + 4 * g.c4;
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    if (g.active)
        for (int r = g.r0 + g.rs; r < g.r1; r += g.rp) {
            const f32x4 v = ld4(base + (int64_t)r * C);
            for (int e = 0; e < 4; ++e) s[e] = s[e] + (double)v[e];
        }
    bn_reduce(red, g, s);
    if (g.active && g.rs == 0)
        for (int e = 0; e < 4; ++e) smean[4 * g.c4 + e] = s[e] / (double)(g.r1 - g.r0);
    __syncthreads();
    double m[4] = {0.0, 0.0, 0.0, 0.0}, q[4] = {0.0, 0.0, 0.0, 0.0};
    if (g.active) {
        for (int e = 0; e < 4; ++e) m[e] = smean[4 * g.c4 + e];
        for (int r = g.r0 + g.rs; r < g.r1; r += g.rp) {
            const f32x4 v = ld4(base + (int64_t)r * C);
            for (int e = 0; e < 4; ++e) {
                const double d = (double)v[e] - m[e];
                q[e] = q[e] + d * d;
            }
        }
    }
    bn_reduce(red, g, q);
    if (g.active && g.rs == 0)
        for (int e = 0; e < 4; ++e) {
            const int c = g.c0 + 4 * g.c4 + e;
            part[((int64_t)blockIdx.x * 2) * C + c] = m[e];
            part[((int64_t)blockIdx.x * 2 + 1) * C + c] = q[e];
        }
}

// Chan's merge of the chunks in chunk order: mean, and the biased variance M2 / M
__global__ __launch_bounds__(256) void bn_stats_finish_kernel(const double* __restrict__ part, int M, int C,
                                                              double* __restrict__ mean, double* __restrict__ var) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    const int chunks = (M + BN_ROWS - 1) / BN_ROWS;
    double n = (double)min(BN_ROWS, M), mu = part[c], m2 = part[C + c];
    for (int k = 1; k < chunks; ++k) {
        const double nb = (double)(min((k + 1) * BN_ROWS, M) - k * BN_ROWS);
        const double mb = part[((int64_t)k * 2) * C + c], qb = part[((int64_t)k * 2 + 1) * C + c];
        const double nt = n + nb, delta = mb - mu;
        mu = mu + delta * (nb / nt);
        m2 = (m2 + qb) + (delta * delta) * (n * nb / nt);
        n = nt;
    }
    mean[c] = mu;
    var[c] = m2 / (double)M;
}

// y = relu?((float)(a * ((double)z - mean) + (double)beta)),  a = (double)gamma / sqrt(var + eps)
__global__ __launch_bounds__(BN_THREADS) void bn_apply_kernel(const float* __restrict__ z, const float* __restrict__ gamma,
                                                              const float* __restrict__ beta, const double* __restrict__ mean,
                                                              const double* __restrict__ var, double eps, int M, int C, int relu,
                                                              float* __restrict__ y) {
    __shared__ double sa[BN_SLAB], sm[BN_SLAB], sb[BN_SLAB];
    const BnGeom g = bn_geom(M, C);
    if ((int)threadIdx.x < g.cw) {
        const int c = g.c0 + threadIdx.x;
        sa[threadIdx.x] = (double)gamma[c] / sqrt(var[c] + eps);
        sm[threadIdx.x] = mean[c];
        sb[threadIdx.x] = (double)beta[c];
    }
    __syncthreads();
    if (!g.active) return;
    double a[4], m[4], b[4];
    for (int e = 0; e < 4; ++e) { a[e] = sa[4 * g.c4 + e]; m[e] = sm[4 * g.c4 + e]; b[e] = sb[4 * g.c4 + e]; }
    for (int r = g.r0 + g.rs; r < g.r1; r += g.rp) {
        const int64_t at = (int64_t)r * C + g.c0 + 4 * g.c4;
        const f32x4 v = ld4(z + at);
        f32x4 o;
        for (int e = 0; e < 4; ++e) {
            const float w = (float)(a[e] * ((double)v[e] - m[e]) + b[e]);
            o[e] = relu ? (w > 0.f ? w : 0.f) : w;
        }
        *reinterpret_cast<f32x4*>(y + at) = o;
    }
}

// per chunk and channel: sum gh and sum gh * xh,  gh = g_y where y > 0 (all of g_y without y),
// xh = ((double)z - mean) * (1 / sqrt(var + eps)).  part [chunks][2][C]
__global__ __launch_bounds__(BN_THREADS) void bn_bwd_chunk_kernel(const float* __restrict__ z, const float* __restrict__ y,
                                                                  const float* __restrict__ g_y, const double* __restrict__ mean,
                                                                  const double* __restrict__ var, double eps, int M, int C,
                                                                  double* __restrict__ part) {
    __shared__ double red[BN_THREADS][4];
    __shared__ double sm[BN_SLAB], si[BN_SLAB];
    const BnGeom g = bn_geom(M, C);
    if ((int)threadIdx.x < g.cw) {
        sm[threadIdx.x] = mean[g.c0 + threadIdx.x];
        si[threadIdx.x] = 1.0 / sqrt(var[g.c0 + threadIdx.x] + eps);
    }
    __syncthreads();
    double sb[4] = {0.0, 0.0, 0.0, 0.0}, sg[4] = {0.0, 0.0, 0.0, 0.0};
    if (g.active) {
        double m[4], inv[4];
        for (int e = 0; e < 4; ++e) { m[e] = sm[4 * g.c4 + e]; inv[e] = si[4 * g.c4 + e]; }
        for (int r = g.r0 + g.rs; r < g.r1; r += g.rp) {
            const int64_t at = (int64_t)r * C + g.c0 + 4 * g.c4;
            const f32x4 v = ld4(z + at), gv = ld4(g_y + at);
            const f32x4 yv = y ? ld4(y + at) : splat4(1.f);
            for (int e = 0; e < 4; ++e) {
                const double gh = yv[e] > 0.f ? (double)gv[e] : 0.0;
                const double xh = ((double)v[e] - m[e]) * inv[e];
                sb[e] = sb[e] + gh;
                sg[e] = sg[e] + gh * xh;
            }
        }
    }
    bn_reduce(red, g, sb);
    bn_reduce(red, g, sg);
    if (g.active && g.rs == 0)
        for (int e = 0; e < 4; ++e) {
            const int c = g.c0 + 4 * g.c4 + e;
            part[((int64_t)blockIdx.x * 2) * C + c] = sb[e];
            part[((int64_t)blockIdx.x * 2 + 1) * C + c] = sg[e];
        }
}

// the chunks in chunk order: sums [2][C] float64 (dbeta, dgamma) and their float32 roundings
__global__ __launch_bounds__(256) void bn_bwd_finish_kernel(const double* __restrict__ part, int M, int C,
                                                            double* __restrict__ sums, float* __restrict__ dgamma,
                                                            float* __restrict__ dbeta) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    const int chunks = (M + BN_ROWS - 1) / BN_ROWS;
    double sb = part[c], sg = part[C + c];
    for (int k = 1; k < chunks; ++k) {
        sb = sb + part[((int64_t)k * 2) * C + c];
        sg = sg + part[((int64_t)k * 2 + 1) * C + c];
    }
    sums[c] = sb;
    sums[C + c] = sg;
    dbeta[c] = (float)sb;
    dgamma[c] = (float)sg;
}

// g_z = (float)(a * ((gh - dbeta / M) - xh * (dgamma / M))),  a = (double)gamma * (1 / sqrt(var + eps)); g_z may be g_y
__global__ __launch_bounds__(BN_THREADS) void bn_bwd_apply_kernel(const float* __restrict__ z, const float* __restrict__ y,
                                                                  const float* g_y, const float* __restrict__ gamma,
                                                                  const double* __restrict__ mean, const double* __restrict__ var,
                                                                  double eps, const double* __restrict__ sums, int M, int C,
                                                                  float* g_z) {
    __shared__ double sm[BN_SLAB], si[BN_SLAB], sa[BN_SLAB], scb[BN_SLAB], scg[BN_SLAB];
    const BnGeom g = bn_geom(M, C);
    if ((int)threadIdx.x < g.cw) {
        const int c = g.c0 + threadIdx.x;
        const double inv = 1.0 / sqrt(var[c] + eps);
        sm[threadIdx.x] = mean[c];
        si[threadIdx.x] = inv;
        sa[threadIdx.x] = (double)gamma[c] * inv;
        scb[threadIdx.x] = sums[c] / (double)M;
        scg[threadIdx.x] = sums[C + c] / (double)M;
    }
    __syncthreads();
    if (!g.active) return;
    double m[4], inv[4], a[4], cb[4], cg[4];
    for (int e = 0; e < 4; ++e) {
        const int k = 4 * g.c4 + e;
        m[e] = sm[k]; inv[e] = si[k]; a[e] = sa[k]; cb[e] = scb[k]; cg[e] = scg[k];
    }
    for (int r = g.r0 + g.rs; r < g.r1; r += g.rp) {
        const int64_t at = (int64_t)r * C + g.c0 + 4 * g.c4;
        const f32x4 v = ld4(z + at), gv = *reinterpret_cast<const f32x4*>(g_y + at);
        const f32x4 yv = y ? ld4(y + at) : splat4(1.f);
        f32x4 o;
        for (int e = 0; e < 4; ++e) {
            const double gh = yv[e] > 0.f ? (double)gv[e] : 0.0;
            const double xh = ((double)v[e] - m[e]) * inv[e];
            o[e] = (float)(a[e] * ((gh - cb[e]) - xh * cg[e]));
        }
        *reinterpret_cast<f32x4*>(g_z + at) = o;
    }
}

struct BnRunArgs {
    float* rm[EN_NCONV];
    float* rv[EN_NCONV];
    int first[EN_NCONV];          // the layer's first channel in the concatenated batch statistics
    int C[EN_NCONV], M[EN_NCONV];
};
// running <- (1 - m) running + m batch in float64, rounded once; the variance unbiased (var M / (M - 1)).  blockIdx.y: layer
__global__ __launch_bounds__(256) void bn_running_kernel(BnRunArgs a, const double* __restrict__ mean,
                                                         const double* __restrict__ var, double momentum) {
    const int i = blockIdx.y, c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= a.C[i]) return;
    const double M = (double)a.M[i], bm = mean[a.first[i] + c], bv = var[a.first[i] + c] * (M / (M - 1.0));
    a.rm[i][c] = (float)((1.0 - momentum) * (double)a.rm[i][c] + momentum * bm);
    a.rv[i][c] = (float)((1.0 - momentum) * (double)a.rv[i][c] + momentum * bv);
}

bool bn_shape_ok(int64_t M, int C) { return M >= 2 && M <= (1 << 24); }
bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
int64_t bn_chunks(int64_t M) { return (M + BN_ROWS - 1) / BN_ROWS; }
int64_t bn_part_doubles(int64_t M, int C) { return 2 * bn_chunks(M) * C; }
dim3 bn_grid(int64_t M, int C) { return dim3((unsigned)bn_chunks(M), (unsigned)((C + BN_SLAB - 1) / BN_SLAB)); }

void launch_bn_stats(const float* z, int M, int C, double* mean, double* var, double* part, hipStream_t st) {
    bn_stats_chunk_kernel<<<bn_grid(M, C), BN_THREADS, 0, st>>>(z, M, C, part);
    bn_stats_finish_kernel<<<(C + 255) / 256, 256, 0, st>>>(part, M, C, mean, var);
}
void launch_bn_apply(const float* z, const float* gamma, const float* beta, const double* mean, const double* var, double eps,
                     int M, int C, int relu, float* y, hipStream_t st) {
    bn_apply_kernel<<<bn_grid(M, C), BN_THREADS, 0, st>>>(z, gamma, beta, mean, var, eps, M, C, relu, y);
}
// scratch: part [2 chunks C] then sums [2 C]
void launch_bn_backward(const float* z, const float* y, const float* g_y, const float* gamma, const double* mean,
                        const double* var, double eps, int M, int C, float* g_z, float* dgamma, float* dbeta, double* scratch,
                        hipStream_t st) {
    double* sums = scratch + bn_part_doubles(M, C);
    bn_bwd_chunk_kernel<<<bn_grid(M, C), BN_THREADS, 0, st>>>(z, y, g_y, mean, var, eps, M, C, scratch);
    bn_bwd_finish_kernel<<<(C + 255) / 256, 256, 0, st>>>(scratch, M, C, sums, dgamma, dbeta);
    bn_bwd_apply_kernel<<<bn_grid(M, C), BN_THREADS, 0, st>>>(z, y, g_y, gamma, mean, var, eps, sums, M, C, g_z);
}

// ---------------------------------------------------------------------------------------------------------------
// the unfolded weights in the convolution launchers' layouts, and the weight gradient back in the parameter's layout
// ---------------------------------------------------------------------------------------------------------------
// fold_pack_kernel without the fold: Wf [9 cinp][cout] and Wt [9 cout][cinp] of w [cout][cin][3][3], copied bit for bit
__global__ __launch_bounds__(256) void train_pack_kernel(FoldTable tb) {
    __shared__ float tile[EN_FT * EN_FLD];
    int bx, by;
    const FoldArgs a = tb.a[fold_locate(tb, bx, by)];
    const int t = threadIdx.x, ci0 = bx * EN_FT, co0 = by * EN_FT;
    for (int e = t; e < EN_FT * EN_FT * 9; e += 256) {
        const int row = e / (EN_FT * 9), col = e - row * (EN_FT * 9);
        const int co = co0 + row, ci = ci0 + col / 9;
        float v = 0.f;
        if (co < a.cout && ci < a.cin) v = a.w[((int64_t)co * a.cin + ci0) * 9 + col];
        tile[row * EN_FLD + col] = v;
    }
    __syncthreads();
    for (int e = t; e < EN_FT * EN_FT * 9; e += 256) {
        const int lo = e & (EN_FT - 1), mid = (e >> 5) & (EN_FT - 1), tap = e >> 10;
        if (co0 + lo < a.cout && ci0 + mid < a.cinp)
            a.wf[((int64_t)tap * a.cinp + ci0 + mid) * a.cout + co0 + lo] = tile[lo * EN_FLD + mid * 9 + tap];
        if (co0 + mid < a.cout && ci0 + lo < a.cinp)
            a.wt[((int64_t)tap * a.cout + co0 + mid) * a.cinp + ci0 + lo] = tile[mid * EN_FLD + lo * 9 + (8 - tap)];
    }
}

// dw [cout][cin][3][3] from the gradient in Wf's layout [9 cinp][cout]; blockIdx.x: cin tile, blockIdx.y: cout tile
__global__ __launch_bounds__(256) void train_unpack_dw_kernel(const float* __restrict__ gwf, int cin, int cinp, int cout,
                                                              float* __restrict__ dw) {
    __shared__ float tile[EN_FT * EN_FLD];
    const int t = threadIdx.x, ci0 = blockIdx.x * EN_FT, co0 = blockIdx.y * EN_FT;
    for (int e = t; e < EN_FT * EN_FT * 9; e += 256) {
        const int lo = e & (EN_FT - 1), mid = (e >> 5) & (EN_FT - 1), tap = e >> 10;
        float v = 0.f;
        if (co0 + lo < cout && ci0 + mid < cinp) v = gwf[((int64_t)tap * cinp + ci0 + mid) * cout + co0 + lo];
        tile[lo * EN_FLD + mid * 9 + tap] = v;
    }
    __syncthreads();
    for (int e = t; e < EN_FT * EN_FT * 9; e += 256) {
        const int row = e / (EN_FT * 9), col = e - row * (EN_FT * 9);
        const int co = co0 + row, ci = ci0 + col / 9;
        if (co < cout && ci < cin) dw[((int64_t)co * cin + ci0) * 9 + col] = tile[row * EN_FLD + col];
    }
}

// acc += add: the per-image weight-gradient partials, summed in image order
__global__ __launch_bounds__(256) void train_add_kernel(float* __restrict__ acc, const float* __restrict__ add, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) acc[i] = acc[i] + add[i];
}

// ---------------------------------------------------------------------------------------------------------------
// The workspace of a batch of B images (float offsets; every region a multiple of 64 floats, so the float64 regions are
// 8-byte aligned), from the description.  A convolution's saved output is y[conv] on both routes.  The folded route
// (bn == false, B == 1) fuses bias and ReLU into the convolution's epilogue, so z[conv] IS y[conv]; the training-mode route
// keeps the raw z and the BatchNorm + ReLU y, and the unfolded weights, BatchNorm statistics and gradient staging besides.
// ---------------------------------------------------------------------------------------------------------------
struct Plan {
    int B, H[5], W[5];
    int64_t P[5];
    int first[EN_NCONV];          // first channel of each BatchNorm in the concatenated statistics
    int64_t x8, z[EN_NCONV], y[EN_NCONV];
    int64_t in[EN_NCONV][2];      // where the convolution's two sources are read: x8, a y[], or the pooled / up-sampled copy
    int64_t df[EN_NCONV];         // the summed gradient of an output that more than one layer reads (else -1)
    int64_t probs, t[3], part, wscr_floats, total;
    int64_t wf[EN_NCONV], wt[EN_NCONV], wscr, gw, gwtmp, heads, hgrad, dummy, stat, bnscr;      // bn only
};
bool size_ok(int H, int W) { return H >= 16 && W >= 16 && (int64_t)H * W <= (1 << 21); }
// the batch statistics of the deepest level need two values per channel
bool train_size_ok(int B, int H, int W) {
    return B >= 1 && B <= 8 && H >= 16 && W >= 16 && (int64_t)B * H * W <= (1 << 21) && (int64_t)B * (H / 16) * (W / 16) >= 2;
}
Plan make_plan(int B, int H, int W, bool bn) {
    Plan pl = {};
    pl.B = B;
    for (int l = 0; l < 5; ++l) {
        pl.H[l] = l ? pl.H[l - 1] / 2 : H;
        pl.W[l] = l ? pl.W[l - 1] / 2 : W;
        pl.P[l] = (int64_t)pl.H[l] * pl.W[l];
    }
    int64_t q = 0, part = 0, wscr = 0, gw = 0, bnscr = 0;
    auto take = [&](int64_t n) { const int64_t at = q; q += (n + 63) / 64 * 64; return at; };
    int readers[EN_NCONV] = {}, ch = 0;
    for (const ConvDesc& c : EN_CONV)
        for (const Source& s : c.src)
            if (s.conv >= 0) ++readers[s.conv];
    pl.x8 = take(B * pl.P[0] * 8);
    for (int i = 0; i < EN_NCONV; ++i) {
        const ConvDesc& c = EN_CONV[i];
        const int cin = c.cin(), cout = c.cout;
        const int64_t P = pl.P[c.level], n = B * P * cout, nw = (int64_t)9 * cin * cout;
        pl.y[i] = take(n);
        pl.z[i] = bn ? take(n) : pl.y[i];
        pl.df[i] = readers[i] > 1 ? take(n) : -1;
        for (int s = 0; s < 2; ++s) {
            const Source& sc = c.src[s];
            pl.in[i][s] = sc.kind == SRC_X8     ? pl.x8
                          : sc.kind == SRC_OUT  ? pl.y[sc.conv]
                          : sc.kind == SRC_POOL ? take(B * P * sc.ch)
                          : sc.kind == SRC_UP   ? take(B * 4 * pl.P[EN_CONV[sc.conv].level] * sc.ch)
                                                : -1;
        }
        if (bn) {
            pl.wf[i] = take(nw);
            pl.wt[i] = take(nw);
        }
        pl.first[i] = ch;
        ch += cout;
        part = std::max(part, std::max(split_floats(P, cin, cout), split_floats(P, cout, cin)));
        wscr = std::max(wscr, wgrad_floats(P, cin, cout));
        gw = std::max(gw, nw);
        bnscr = std::max(bnscr, bn_part_doubles(B * P, cout) + 2 * cout);
    }
    pl.probs = take(B * 2 * pl.P[0]);
    // transient gradients: at most P0 * 64 floats each per image (level l has P0 / 4^l pixels and at most 64 * 2^l channels)
    for (int k = 0; k < 3; ++k) pl.t[k] = take(B * pl.P[0] * 64);
    pl.part = take(part);
    // scratch of the weight gradients: the largest split-partial block of the 26 convolutions, or the heads'
    int per_block;
    pl.wscr_floats = std::max(wscr, (int64_t)B * heads_wgrad_blocks(pl.P[0], per_block) * 260);
    if (bn) {
        pl.wscr = take(pl.wscr_floats);
        pl.gw = take(gw);
        pl.gwtmp = take(gw);
        pl.heads = take(EN_HEADS_FLOATS);
        pl.hgrad = take(EN_HEADS_FLOATS);
        pl.dummy = take(2 * 1024);
        pl.stat = take(2 * 2 * EN_BN_CHANNELS);         // float64 mean [5888] | var [5888]
        pl.bnscr = take(2 * bnscr);                      // float64
    }
    pl.total = q;
    return pl;
}

// ---------------------------------------------------------------------------------------------------------------
// The two walks over the description.  Every launch is per image (BatchNorm alone sees the whole batch); with B == 1 each loop
// body runs once.  A route binds where the weights live and what surrounds a convolution:
//   folded (enslam_eventnet_forward / _backward / _backward_weights): weights in the packed image, bias + ReLU in the
//     convolution's epilogue; the backward masks the incoming gradient by the saved output at load (relu'(0) = 0 as in torch).
//   training mode (enslam_eventnet_train_*): the unfolded copies in the workspace, BatchNorm statistics + apply after every
//     convolution; the backward runs BatchNorm + ReLU backwards in place first, and needs no mask.
// ---------------------------------------------------------------------------------------------------------------
struct Route {
    const float *wf[EN_NCONV], *bias[EN_NCONV], *wt[EN_NCONV], *heads;
    int relu;
};
Route packed_route(const float* packed, const PackOff& po) {
    Route r;
    for (int i = 0; i < EN_NCONV; ++i) {
        r.wf[i] = packed + po.wf[i]; r.bias[i] = packed + po.b[i]; r.wt[i] = packed + po.wt[i];
    }
    r.heads = packed + po.heads;
    r.relu = 1;
    return r;
}
Route workspace_route(const float* ws, const Plan& pl) {
    Route r;
    for (int i = 0; i < EN_NCONV; ++i) {
        r.wf[i] = ws + pl.wf[i]; r.bias[i] = nullptr; r.wt[i] = ws + pl.wt[i];
    }
    r.heads = ws + pl.heads;
    r.relu = 0;
    return r;
}

// a convolution's geometry: its level's extent, the channels of its two sources, and the extent of the up-sampled one
struct ConvGeom { int H, W, C0, C1, lk, sH1, sW1; int64_t P; };
ConvGeom conv_geom(const Plan& pl, const ConvDesc& c) {
    ConvGeom g = {pl.H[c.level], pl.W[c.level], c.src[0].ch, c.src[1].ch, -1, 0, 0, pl.P[c.level]};
    const Source& s = c.src[0].kind == SRC_POOL ? c.src[0] : c.src[1];      // src[0] is never SRC_UP, src[1] nothing else
    if (s.conv >= 0) g.lk = EN_CONV[s.conv].level;
    if (c.src[1].kind == SRC_UP) {
        g.sH1 = 2 * pl.H[g.lk];
        g.sW1 = 2 * pl.W[g.lk];
    }
    return g;
}

// after(i): what follows convolution i's B launches into z[i] (training mode: BatchNorm over the whole batch, z[i] -> y[i])
template <class After>
void walk_forward(const Plan& pl, const Route& r, float* ws, const float* x, float* events, float* probs, hipStream_t st,
                  After after) {
    const int B = pl.B;
    const int64_t P0 = pl.P[0];
    for (int b = 0; b < B; ++b)
        en_pack_x_kernel<<<blocks_of(P0 * 8), 256, 0, st>>>(x + b * 6 * P0, (int)P0, ws + pl.x8 + b * P0 * 8);
    for (int i = 0; i < EN_NCONV; ++i) {
        const ConvDesc& c = EN_CONV[i];
        const ConvGeom cg = conv_geom(pl, c);
        const float *s0 = ws + pl.in[i][0], *s1 = cg.C1 ? ws + pl.in[i][1] : nullptr;
        if (c.src[0].kind == SRC_POOL) {
            const float* from = ws + pl.y[c.src[0].conv];
            for (int b = 0; b < B; ++b)
                pool2_fwd_kernel<<<blocks_of(cg.P * cg.C0), 256, 0, st>>>(from + b * pl.P[cg.lk] * cg.C0, pl.H[cg.lk], pl.W[cg.lk],
                                                                          cg.C0, ws + pl.in[i][0] + b * cg.P * cg.C0);
        }
        if (c.src[1].kind == SRC_UP) {
            const float* from = ws + pl.y[c.src[1].conv];
            const int64_t n = pl.P[cg.lk] * cg.C1;
            for (int b = 0; b < B; ++b)
                up2_fwd_kernel<<<blocks_of(4 * n), 256, 0, st>>>(from + b * n, pl.H[cg.lk], pl.W[cg.lk], cg.C1,
                                                                 ws + pl.in[i][1] + b * 4 * n);
        }
        for (int b = 0; b < B; ++b) {
            ConvArgs a = {};
            a.w = r.wf[i]; a.bias = r.bias[i];
            a.s0 = s0 + b * cg.P * cg.C0;
            a.s1 = s1 ? s1 + (int64_t)b * cg.sH1 * cg.sW1 * cg.C1 : nullptr;
            a.d0 = ws + pl.z[i] + b * cg.P * c.cout; a.part = ws + pl.part;
            a.H = cg.H; a.W = cg.W; a.C0 = cg.C0; a.C1 = cg.C1; a.sH1 = cg.sH1; a.sW1 = cg.sW1;
            a.N = a.N0 = c.cout; a.relu = r.relu;
            launch_conv(a, st);
        }
        after(i);
    }
    for (int b = 0; b < B; ++b)
        heads_fwd_kernel<<<blocks_of(2 * P0), 256, 0, st>>>(r.heads, ws + pl.y[EN_HEAD[0].last] + b * P0 * 64,
                                                            ws + pl.y[EN_HEAD[1].last] + b * P0 * 64, (int)P0, events + b * 2 * P0,
                                                            probs + b * 2 * P0, ws + pl.probs + b * 2 * P0);
}

// the heads block's gradient: per image into scratch [B][blocks][260], summed in that order into dst [EN_HEADS_FLOATS]
void launch_heads_wgrad(const Plan& pl, const float* ws, const float* g_events, const float* g_probs, float* scratch, float* dst,
                        hipStream_t st) {
    const int64_t P0 = pl.P[0];
    int per_block;
    const int blocks = heads_wgrad_blocks(P0, per_block);
    for (int b = 0; b < pl.B; ++b)
        heads_wgrad_kernel<<<blocks, 256, 0, st>>>(g_events + b * 2 * P0, g_probs + b * 2 * P0, ws + pl.probs + b * 2 * P0,
                                                   ws + pl.y[EN_HEAD[0].last] + b * P0 * 64,
                                                   ws + pl.y[EN_HEAD[1].last] + b * P0 * 64, (int)P0, per_block,
                                                   scratch + (int64_t)b * blocks * 260);
    heads_wgrad_reduce_kernel<<<1, EN_HEADS_FLOATS, 0, st>>>(scratch, pl.B * blocks, dst);
}

// The backward walk: each head's decoder from its last convolution down, then the encoder.  g is the gradient of the current
// convolution's output.  It travels through the transients tA / tB (a transposed convolution writes the one it does not
// read); the up-sampled source's gradient goes through tC and up2_bwd; an output that several layers read collects its
// gradient in df[]: the first writer of this walk stores, the later ones add (the skips: acc0 = head; the bottleneck's
// up2_bwd likewise; pool2_bwd always comes after a skip and adds).  Per layer the order is fixed:
//   before(i, g)      folded: returns the saved output, the ReLU mask of g.  Training mode: BatchNorm + ReLU backwards in
//                     place, g becomes the gradient of z[i]; returns null.
//   wgrad(i, b, a)    image b's weight gradient from a (sources, g, mask, shapes filled in); it reads g before the transposed
//                     convolution overwrites a transient.  The route supplies the destination, or skips an unwanted one.
//   the transposed convolution, into the sources' gradients.  g_x == null skips the first layer's and the unpack.
template <class Before, class Wgrad>
void walk_backward(const Plan& pl, const Route& r, float* ws, const float* g_events, const float* g_probs, float* g_x,
                   hipStream_t st, Before before, Wgrad wgrad) {
    const int B = pl.B;
    const int64_t P0 = pl.P[0];
    float *tA = ws + pl.t[0], *tB = ws + pl.t[1], *tC = ws + pl.t[2], *g = nullptr;
    bool stored[EN_NCONV] = {};
    auto add_to = [&](int k) { const int acc = stored[k]; stored[k] = true; return acc; };
    auto back = [&](int i) {
        const ConvDesc& c = EN_CONV[i];
        const ConvGeom cg = conv_geom(pl, c);
        const int k0 = c.src[0].conv, k1 = c.src[1].conv;
        const int64_t n_out = cg.P * c.cout;
        if (pl.df[i] >= 0) g = ws + pl.df[i];
        const float* mask = before(i, g);
        for (int b = 0; b < B; ++b) {
            WgradArgs a = {};
            a.s0 = ws + pl.in[i][0] + b * cg.P * cg.C0;
            a.s1 = cg.C1 ? ws + pl.in[i][1] + (int64_t)b * cg.sH1 * cg.sW1 * cg.C1 : nullptr;
            a.g = g + b * n_out; a.saved = mask ? mask + b * n_out : nullptr;
            a.H = cg.H; a.W = cg.W; a.C0 = cg.C0; a.C1 = cg.C1; a.sH1 = cg.sH1; a.sW1 = cg.sW1; a.N = c.cout;
            wgrad(i, b, a);
        }
        // d(sources) from g: C0 channels to d0 (a skip's straight into its df), the up-sampled source's C1 to tC
        const bool skip = c.src[0].kind == SRC_OUT && pl.df[k0] >= 0;
        float* d0 = skip ? ws + pl.df[k0] : g == tA ? tB : tA;
        const int acc0 = skip ? add_to(k0) : 0;
        if (c.src[0].kind != SRC_X8 || g_x)
            for (int b = 0; b < B; ++b) {
                ConvArgs a = {};
                a.w = r.wt[i];
                a.s0 = g + b * n_out; a.mask = mask ? mask + b * n_out : nullptr; a.C0 = c.cout;
                a.d0 = d0 + b * cg.P * cg.C0;
                a.d1 = cg.C1 ? tC + (int64_t)b * cg.sH1 * cg.sW1 * cg.C1 : nullptr;
                a.part = ws + pl.part;
                a.H = cg.H; a.W = cg.W; a.N = c.cin(); a.N0 = cg.C0; a.dH1 = cg.sH1; a.dW1 = cg.sW1; a.acc0 = acc0;
                launch_conv(a, st);
            }
        if (c.src[0].kind == SRC_POOL) {
            const int64_t n = pl.P[cg.lk] * cg.C0;
            const int acc = add_to(k0);
            for (int b = 0; b < B; ++b)
                pool2_bwd_kernel<<<blocks_of(n), 256, 0, st>>>(ws + pl.y[k0] + b * n, pl.H[cg.lk], pl.W[cg.lk], cg.C0,
                                                               d0 + b * cg.P * cg.C0, ws + pl.df[k0] + b * n, acc);
        }
        if (c.src[1].kind == SRC_UP) {
            const int64_t n = pl.P[cg.lk] * cg.C1;
            float* dst = pl.df[k1] >= 0 ? ws + pl.df[k1] : tA;
            const int acc = pl.df[k1] >= 0 ? add_to(k1) : 0;
            for (int b = 0; b < B; ++b)
                up2_bwd_kernel<<<blocks_of(n), 256, 0, st>>>(tC + b * 4 * n, pl.H[cg.lk], pl.W[cg.lk], cg.C1, dst + b * n, acc);
            g = tA;
        } else {
            g = d0;
        }
    };
    for (int hd = 0; hd < 2; ++hd) {
        for (int b = 0; b < B; ++b)
            heads_bwd_kernel<<<blocks_of(P0 * 64), 256, 0, st>>>(r.heads, hd, (hd ? g_probs : g_events) + b * 2 * P0,
                                                                 ws + pl.probs + b * 2 * P0, (int)P0, tA + b * P0 * 64);
        g = tA;
        for (int i = EN_HEAD[hd].last; i >= EN_HEAD[hd].first; --i) back(i);
    }
    for (int i = EN_HEAD[0].first - 1; i >= 0; --i) back(i);
    if (g_x)
        for (int b = 0; b < B; ++b)
            en_unpack_gx_kernel<<<blocks_of(P0 * 6), 256, 0, st>>>(g + b * P0 * 8, (int)P0, g_x + b * 6 * P0);
}

}  // namespace

extern "C" {

int enslam_eventnet_bn_stats(const float* z, int64_t M, int32_t C, double* mean, double* var, double* scratch,
                             int64_t scratch_doubles, void* stream) {
    if (!z || !mean || !var || !scratch || !aligned16(z)) return ENSLAM_EINVAL;
    if (!chan_ok(C)) return ENSLAM_EUNSUPPORTED;
    if (!bn_shape_ok(M, C) || scratch_doubles < bn_part_doubles(M, C)) return ENSLAM_EINVAL;
    launch_bn_stats(z, (int)M, C, mean, var, scratch, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? ENSLAM_OK : ENSLAM_ELAUNCH;
}

int enslam_eventnet_bn_apply(const float* z, const float* gamma, const float* beta, const double* mean, const double* var,
                             double eps, int64_t M, int32_t C, int32_t relu, float* y, void* stream) {
    if (!z || !gamma || !beta || !mean || !var || !y || !aligned16(z) || !aligned16(y)) return ENSLAM_EINVAL;
    if (!chan_ok(C)) return ENSLAM_EUNSUPPORTED;
    if (!bn_shape_ok(M, C) || !(eps >= 0.0)) return ENSLAM_EINVAL;
    launch_bn_apply(z, gamma, beta, mean, var, eps, (int)M, C, relu, y, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? ENSLAM_OK : ENSLAM_ELAUNCH;
}

int enslam_eventnet_bn_backward(const float* z, const float* y, const float* g_y, const float* gamma, const double* mean,
                                const double* var, double eps, int64_t M, int32_t C, float* g_z, float* dgamma, float* dbeta,
                                double* scratch, int64_t scratch_doubles, void* stream) {
    if (!z || !g_y || !gamma || !mean || !var || !g_z || !dgamma || !dbeta || !scratch) return ENSLAM_EINVAL;
    if (!aligned16(z) || !aligned16(g_y) || !aligned16(g_z) || (y && !aligned16(y))) return ENSLAM_EINVAL;
    if (!chan_ok(C)) return ENSLAM_EUNSUPPORTED;
    if (!bn_shape_ok(M, C) || !(eps >= 0.0) || scratch_doubles < bn_part_doubles(M, C) + 2 * C) return ENSLAM_EINVAL;
    launch_bn_backward(z, y, g_y, gamma, mean, var, eps, (int)M, C, g_z, dgamma, dbeta, scratch, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? ENSLAM_OK : ENSLAM_ELAUNCH;
}

// ---- the folded route: frozen BatchNorm, one image ----

size_t enslam_eventnet_workspace_floats(int32_t H, int32_t W) {
    if (!size_ok(H, W)) return 0;
    return (size_t)make_plan(1, H, W, false).total;
}

int enslam_eventnet_forward(const float* packed, const float* x, int32_t H, int32_t W, float* workspace, float* events,
                            float* probs, void* stream) {
    if (!packed || !x || !workspace || !events || !probs) return ENSLAM_EINVAL;
    if (!size_ok(H, W)) return ENSLAM_EINVAL;
    const Plan pl = make_plan(1, H, W, false);
    walk_forward(pl, packed_route(packed, pack_offsets()), workspace, x, events, probs, (hipStream_t)stream, [](int) {});
    return hipGetLastError() == hipSuccess ? ENSLAM_OK : ENSLAM_ELAUNCH;
}

}  // extern "C"

namespace {
// g_packed == null: the input gradient only (enslam_eventnet_backward).  Otherwise every layer's weight gradient goes
// straight into g_packed, whose Wt blocks (the same weights again) are zeroed.
int run_backward(const float* packed, float* ws, const float* g_events, const float* g_probs, float* g_x, float* g_packed,
                 float* scratch, int H, int W, hipStream_t st) {
    const Plan pl = make_plan(1, H, W, false);
    const PackOff po = pack_offsets();
    if (g_packed) launch_heads_wgrad(pl, ws, g_events, g_probs, scratch, g_packed + po.heads, st);
    walk_backward(
        pl, packed_route(packed, po), ws, g_events, g_probs, g_x, st, [&](int i, float*) { return ws + pl.y[i]; },
        [&](int i, int, WgradArgs a) {
            if (!g_packed) return;
            a.dw = g_packed + po.wf[i]; a.db = g_packed + po.b[i]; a.part = scratch;
            launch_wgrad(a, st);
            // the launch's status is read by hipGetLastError below
            (void)hipMemsetAsync(g_packed + po.wt[i], 0, sizeof(float) * 9 * EN_CONV[i].cin() * EN_CONV[i].cout, st);
        });
    return hipGetLastError() == hipSuccess ? ENSLAM_OK : ENSLAM_ELAUNCH;
}
int64_t wgrad_scratch_floats(int H, int W) { return (make_plan(1, H, W, false).wscr_floats + 63) / 64 * 64; }
}  // namespace

extern "C" {

int enslam_eventnet_backward(const float* packed, float* workspace, const float* g_events, const float* g_probs,
                             float* g_x, int32_t H, int32_t W, void* stream) {
    if (!packed || !workspace || !g_events || !g_probs || !g_x) return ENSLAM_EINVAL;
    if (!size_ok(H, W)) return ENSLAM_EINVAL;
    return run_backward(packed, workspace, g_events, g_probs, g_x, nullptr, nullptr, H, W, (hipStream_t)stream);
}

size_t enslam_eventnet_wgrad_scratch_floats(int32_t H, int32_t W) {
    if (!size_ok(H, W)) return 0;
    return (size_t)wgrad_scratch_floats(H, W);
}

int enslam_eventnet_backward_weights(const float* packed, float* workspace, const float* g_events, const float* g_probs,
                                     float* g_x, float* g_packed, float* scratch, int64_t scratch_floats, int32_t H, int32_t W,
                                     void* stream) {
    if (!packed || !workspace || !g_events || !g_probs || !g_packed || !scratch) return ENSLAM_EINVAL;
    if (!size_ok(H, W)) return ENSLAM_EINVAL;
    if (scratch_floats < wgrad_scratch_floats(H, W)) return ENSLAM_EINVAL;
    return run_backward(packed, workspace, g_events, g_probs, g_x, g_packed, scratch, H, W, (hipStream_t)stream);
}

int enslam_eventnet_heads_wgrad(const float* workspace, const float* g_events, const float* g_probs, float* g_heads,
                                float* scratch, int64_t scratch_floats, int32_t H, int32_t W, void* stream) {
    if (!workspace || !g_events || !g_probs || !g_heads || !scratch) return ENSLAM_EINVAL;
    if (!size_ok(H, W)) return ENSLAM_EINVAL;
    const Plan pl = make_plan(1, H, W, false);
    int per_block;
    if (scratch_floats < (int64_t)heads_wgrad_blocks(pl.P[0], per_block) * 260) return ENSLAM_EINVAL;
    launch_heads_wgrad(pl, workspace, g_events, g_probs, scratch, g_heads, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? ENSLAM_OK : ENSLAM_ELAUNCH;
}

// ---- the training-mode route: batch statistics, B images ----

int enslam_eventnet_bn_running(void* const* buffers, const double* batch_mean, const double* batch_var, int32_t B, int32_t H,
                               int32_t W, double momentum, void* stream) {
    if (!buffers || !batch_mean || !batch_var || !train_size_ok(B, H, W)) return ENSLAM_EINVAL;
    if (!(momentum >= 0.0 && momentum <= 1.0) || !all_set(buffers, 2 * EN_NCONV)) return ENSLAM_EINVAL;
    const Plan pl = make_plan(B, H, W, true);
    BnRunArgs a;
    for (int i = 0; i < EN_NCONV; ++i) {
        a.rm[i] = (float*)buffers[2 * i];
        a.rv[i] = (float*)buffers[2 * i + 1];
        a.first[i] = pl.first[i];
        a.C[i] = EN_CONV[i].cout;
        a.M[i] = (int)(B * pl.P[EN_CONV[i].level]);
    }
    bn_running_kernel<<<dim3(2, EN_NCONV), 256, 0, (hipStream_t)stream>>>(a, batch_mean, batch_var, momentum);
    return hipGetLastError() == hipSuccess ? ENSLAM_OK : ENSLAM_ELAUNCH;
}

size_t enslam_eventnet_bn_workspace_floats(int32_t B, int32_t H, int32_t W) {
    if (!train_size_ok(B, H, W)) return 0;
    return (size_t)make_plan(B, H, W, true).total;
}

int64_t enslam_eventnet_bn_saved_offset(int32_t B, int32_t H, int32_t W, int32_t conv) {
    if (!train_size_ok(B, H, W) || conv < 0 || conv >= EN_NCONV) return -1;
    return make_plan(B, H, W, true).y[conv];
}

/* params: per convolution 3 device addresses (w, gamma, beta), then W1, W2, b1, b2 of the heads */
int enslam_eventnet_train_forward(const void* const* params, const float* x, int32_t B, int32_t H, int32_t W, double eps,
                                  float* workspace, float* events, float* probs, double* batch_mean, double* batch_var,
                                  void* stream) {
    if (!params || !x || !workspace || !events || !probs || !batch_mean || !batch_var) return ENSLAM_EINVAL;
    if (!all_set(params, 3 * EN_NCONV + 4)) return ENSLAM_EINVAL;
    if (!train_size_ok(B, H, W) || !(eps >= 0.0)) return ENSLAM_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    const Plan pl = make_plan(B, H, W, true);
    float* ws = workspace;
    double* mean = reinterpret_cast<double*>(ws + pl.stat);
    double* var = mean + EN_BN_CHANNELS;
    double* bnscr = reinterpret_cast<double*>(ws + pl.bnscr);
    FoldTable tb;
    const int blocks = fold_shapes(params, 3, tb);
    for (int i = 0; i < EN_NCONV; ++i) {
        tb.a[i].wf = ws + pl.wf[i]; tb.a[i].wt = ws + pl.wt[i];
    }
    train_pack_kernel<<<blocks, 256, 0, st>>>(tb);
    const void* const* h = params + 3 * EN_NCONV;
    heads_pack_kernel<<<1, EN_HEADS_FLOATS, 0, st>>>((float*)h[0], (float*)h[1], (float*)h[2], (float*)h[3], ws + pl.heads, 0);
    walk_forward(pl, workspace_route(ws, pl), ws, x, events, probs, st, [&](int i) {
        const int M = (int)(B * pl.P[EN_CONV[i].level]), cout = EN_CONV[i].cout;
        launch_bn_stats(ws + pl.z[i], M, cout, mean + pl.first[i], var + pl.first[i], bnscr, st);
        launch_bn_apply(ws + pl.z[i], (const float*)params[3 * i + 1], (const float*)params[3 * i + 2], mean + pl.first[i],
                        var + pl.first[i], eps, M, cout, 1, ws + pl.y[i], st);
    });
    (void)hipMemcpyAsync(batch_mean, mean, sizeof(double) * EN_BN_CHANNELS, hipMemcpyDeviceToDevice, st);
    (void)hipMemcpyAsync(batch_var, var, sizeof(double) * EN_BN_CHANNELS, hipMemcpyDeviceToDevice, st);
    return hipGetLastError() == hipSuccess ? ENSLAM_OK : ENSLAM_ELAUNCH;
}

/* grads: per convolution 3 device addresses (dw, dgamma, dbeta), then dW1, dW2, db1, db2; a null address skips that gradient
   (the heads' four are wanted together or not at all) */
int enslam_eventnet_train_backward(const void* const* params, float* workspace, const float* g_events, const float* g_probs,
                                   int32_t B, int32_t H, int32_t W, double eps, float* g_x, void* const* grads, void* stream) {
    if (!params || !workspace || !g_events || !g_probs || !grads) return ENSLAM_EINVAL;
    if (!all_set(params, 3 * EN_NCONV + 4)) return ENSLAM_EINVAL;
    void* const* h = grads + 3 * EN_NCONV;
    for (int k = 1; k < 4; ++k)
        if ((h[k] != nullptr) != (h[0] != nullptr)) return ENSLAM_EINVAL;
    if (!train_size_ok(B, H, W) || !(eps >= 0.0)) return ENSLAM_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    const Plan pl = make_plan(B, H, W, true);
    float* ws = workspace;
    const double* mean = reinterpret_cast<const double*>(ws + pl.stat);
    const double* var = mean + EN_BN_CHANNELS;
    double* bnscr = reinterpret_cast<double*>(ws + pl.bnscr);
    if (h[0]) {
        launch_heads_wgrad(pl, ws, g_events, g_probs, ws + pl.wscr, ws + pl.hgrad, st);
        heads_pack_kernel<<<1, EN_HEADS_FLOATS, 0, st>>>((float*)h[0], (float*)h[1], (float*)h[2], (float*)h[3], ws + pl.hgrad, 1);
    }
    walk_backward(
        pl, workspace_route(ws, pl), ws, g_events, g_probs, g_x, st,
        [&](int i, float* g) -> const float* {
            float* dg = grads[3 * i + 1] ? (float*)grads[3 * i + 1] : ws + pl.dummy;
            float* db = grads[3 * i + 2] ? (float*)grads[3 * i + 2] : ws + pl.dummy + 1024;
            launch_bn_backward(ws + pl.z[i], ws + pl.y[i], g, (const float*)params[3 * i + 1], mean + pl.first[i],
                               var + pl.first[i], eps, (int)(B * pl.P[EN_CONV[i].level]), EN_CONV[i].cout, g, dg, db, bnscr, st);
            return nullptr;
        },
        // d(w of convolution i): per image in Wf's layout, summed in image order, then moved to the parameter's layout
        [&](int i, int b, WgradArgs a) {
            if (!grads[3 * i]) return;
            const int cin = EN_CONV[i].cin(), cout = EN_CONV[i].cout;
            const int64_t n = (int64_t)9 * cin * cout;
            a.dw = ws + (b ? pl.gwtmp : pl.gw); a.part = ws + pl.wscr;
            launch_wgrad(a, st);
            if (b) train_add_kernel<<<blocks_of(n), 256, 0, st>>>(ws + pl.gw, ws + pl.gwtmp, n);
            if (b == B - 1)
                train_unpack_dw_kernel<<<dim3(tiles_of(cin, EN_FT), tiles_of(cout, EN_FT)), 256, 0, st>>>(
                    ws + pl.gw, i ? cin : 6, cin, cout, (float*)grads[3 * i]);
        });
    return hipGetLastError() == hipSuccess ? ENSLAM_OK : ENSLAM_ELAUNCH;
}

}  // extern "C"
