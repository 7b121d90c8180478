// iMAP mode (configs/imap.yaml): the 256-wide decoder and density compositing.
//
// Decoder (reference src/conv_onet/models/decoder.py:91-203 with c_dim 0, hidden 256, 4 blocks, no skips, colour,
// fourier embedding):  e = sin(p . B) (B [3,93], p in world coordinates, float32), h1..h4 = relu(W_l h + b_l)
// (93->256, then 256->256 three times), raw = Wo h4 + bo (4 outputs, no activation).  All arithmetic is float32; the
// products run on v_mfma_f32_32x32x2_f32, which is exact f32 (an fmaf chain), so only the summation order differs from
// torch's GEMMs.
//
//   imap_fwd_kernel    64 points per workgroup (4 waves).  The layer inputs live transposed in LDS ([k][point], row
//                      stride 65: conflict-free for the A-operand reads and the C-tile writes); every wave computes 64
//                      output columns x 64 points as 2x2 32x32 MFMA tiles and reads its B operand (the transposed
//                      weights of enslam_imap_pack) from L2.  The layer's result is held in accumulators across a
//                      barrier and written back over its own input, so one 66.5 KB buffer serves all layers (two
//                      workgroups per CU).  With `save` it also writes e and h1..h4 to the workspace (backward).
//   imap_bwd_chain     same tiling, top down: dOut -> dPre3 = (dOut Wo) * [h4 > 0] -> ... -> dPre0 -> de -> dz =
//                      de * cos(p . B) -> dp.  Writes every dPre_l and dz to the workspace.  relu'(0) = 0 as in torch.
//   imap_dw_kernel     dW_l = dPre_l^T in_l, dWo = dOut^T h4, dB = p^T dz, and the bias sums, as one list of
//                      "X^T Y over points" jobs: one wave per 64x64 output tile and point slice, partials per slice.
//   imap_reduce        sums the slices in a fixed order: the parameter gradients are deterministic (no atomics).
//
// Density compositing (reference src/common.py:256-297, occupancy=False): one thread per ray, at most 64 samples.
#include "../../include/enslam_hip.h"
#include "common.hpp"

namespace {

constexpr int IM_H = 256;          // hidden width
constexpr int IM_E = 93;           // embedding width
constexpr int IM_EP = 96;          // embedding width padded to the MFMA k step / workspace row
constexpr int IM_TM = 64;          // points per workgroup
constexpr int IM_LD = IM_TM + 1;   // LDS row stride (floats)
constexpr int IM_THREADS = 256;

// packed forward weights (enslam_imap_pack): B [3][96] | WT0 [96][256] | b0 | (WTl [256][256] | bl) x 3 | Wo [4][256] | bo
constexpr int64_t PK_B = 0;
constexpr int64_t PK_W0 = PK_B + 3 * IM_EP;
constexpr int64_t PK_B0 = PK_W0 + IM_EP * IM_H;
constexpr int64_t PK_L1 = PK_B0 + IM_H;
constexpr int64_t PK_LSTRIDE = IM_H * IM_H + IM_H;
constexpr int64_t PK_WO = PK_L1 + 3 * PK_LSTRIDE;
constexpr int64_t PK_BO = PK_WO + 4 * IM_H;
constexpr int64_t PK_FLOATS = PK_BO + 4;

// backward workspace, per point (floats): e [96] | h1..h4 [4][256] | dPre0..3 [4][256] | dz [96] | dOut [4] | p [4]
constexpr int64_t WS_PER_POINT = IM_EP + 4 * IM_H + 4 * IM_H + IM_EP + 4 + 4;
constexpr int IM_MAX_SLICES = 64;
constexpr int IM_PARAM_FLOATS = 3 * IM_E + IM_H * IM_E + IM_H + 3 * (IM_H * IM_H + IM_H) + 4 * IM_H + 4;   // 222747

typedef float f32x16 __attribute__((ext_vector_type(16)));

ENS_DEV f32x16 mfma32(float a, float b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0); }

struct ImBound {
    double lo[3], hi[3];
    int on;
};

ENS_DEV bool im_outside(const ImBound& b, double x, double y, double z) {
    // Renderer.eval_points: strict inequalities, evaluated in the points' precision (the host rounds the bound to float32
    // for float32 points, as torch's comparison with a 0-dim float64 bound does)
    return !((x < b.hi[0]) && (x > b.lo[0]) && (y < b.hi[1]) && (y > b.lo[1]) && (z < b.hi[2]) && (z > b.lo[2]));
}

// z = p . B[:,k] in the order of the reference's x @ B (three products summed left to right), no contraction
ENS_DEV float im_arg(const float* p, const float* B, int k, int ldb) {
    const float a0 = p[0] * B[k], a1 = p[1] * B[ldb + k], a2 = p[2] * B[2 * ldb + k];
    return (a0 + a1) + a2;
}

struct Ws {
    float* e;        // [P][96]
    float* h[4];     // [P][256] each: h1..h4 (post-relu)
    float* dpre[4];  // [P][256] each: dPre0..dPre3
    float* dz;       // [P][96]
    float* dout;     // [P][4]
    float* pf;       // [P][4]: points as float32
    float* part;     // [slices][IM_PARAM_FLOATS]
};

__host__ __device__ inline Ws ws_carve(float* base, int64_t P) {
    Ws w;
    w.e = base;
    float* q = base + P * IM_EP;
    for (int l = 0; l < 4; ++l) { w.h[l] = q; q += P * IM_H; }
    for (int l = 0; l < 4; ++l) { w.dpre[l] = q; q += P * IM_H; }
    w.dz = q; q += P * IM_EP;
    w.dout = q; q += P * 4;
    w.pf = q; q += P * 4;
    w.part = q;
    return w;
}

// 64 points x 64 output columns (this wave's) of in[K][64] (LDS, transposed) times B operand rows of length ldb
// (bw[k * ldb + n], n contiguous, guarded by n < n_valid).
ENS_DEV void tile_mm(const float* Hs, int K, const float* __restrict__ bw, int ldb, int n0, int n_valid, int lane,
                     f32x16 acc[2][2]) {
    const int r = lane & 31, h = lane >> 5;
    for (int i = 0; i < 2; ++i)
        for (int j = 0; j < 2; ++j)
            for (int v = 0; v < 16; ++v) acc[i][j][v] = 0.f;
    const bool ok0 = n0 + r < n_valid, ok1 = n0 + 32 + r < n_valid;
    for (int k = 0; k < K; k += 2) {
        const int kk = k + h;
        const float a0 = Hs[kk * IM_LD + r], a1 = Hs[kk * IM_LD + 32 + r];
        const float b0 = ok0 ? bw[(int64_t)kk * ldb + n0 + r] : 0.f;
        const float b1 = ok1 ? bw[(int64_t)kk * ldb + n0 + 32 + r] : 0.f;
        acc[0][0] = mfma32(a0, b0, acc[0][0]);
        acc[0][1] = mfma32(a0, b1, acc[0][1]);
        acc[1][0] = mfma32(a1, b0, acc[1][0]);
        acc[1][1] = mfma32(a1, b1, acc[1][1]);
    }
}

// C/D map of the 32x32 f32 MFMA: column lane & 31, row (v & 3) + 8 (v >> 2) + 4 (lane >> 5)
ENS_DEV int c_row(int v, int lane) { return (v & 3) + 8 * (v >> 2) + 4 * (lane >> 5); }

__global__ __launch_bounds__(IM_THREADS) void imap_pack_kernel(const float* __restrict__ B, const float* __restrict__ W0,
                                                               const float* __restrict__ b0, const float* __restrict__ W1,
                                                               const float* __restrict__ b1, const float* __restrict__ W2,
                                                               const float* __restrict__ b2, const float* __restrict__ W3,
                                                               const float* __restrict__ b3, const float* __restrict__ Wo,
                                                               const float* __restrict__ bo, float* __restrict__ pk) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= PK_FLOATS) return;
    float v;
    if (i < PK_W0) {
        const int c = (int)(i / IM_EP), k = (int)(i % IM_EP);
        v = k < IM_E ? B[c * IM_E + k] : 0.f;
    } else if (i < PK_B0) {
        const int k = (int)((i - PK_W0) / IM_H), n = (int)((i - PK_W0) % IM_H);
        v = k < IM_E ? W0[n * IM_E + k] : 0.f;
    } else if (i < PK_L1) {
        v = b0[i - PK_B0];
    } else if (i < PK_WO) {
        const int l = (int)((i - PK_L1) / PK_LSTRIDE);
        const int64_t o = (i - PK_L1) % PK_LSTRIDE;
        const float* W = l == 0 ? W1 : (l == 1 ? W2 : W3);
        const float* b = l == 0 ? b1 : (l == 1 ? b2 : b3);
        if (o < IM_H * IM_H) {
            const int k = (int)(o / IM_H), n = (int)(o % IM_H);
            v = W[n * IM_H + k];
        } else {
            v = b[o - IM_H * IM_H];
        }
    } else if (i < PK_BO) {
        v = Wo[i - PK_WO];
    } else {
        v = bo[i - PK_BO];
    }
    pk[i] = v;
}

// points float64 [P,3] -> raw float32 [P,4]; with `save`, e / h1..h4 / p into the workspace (backward recompute)
__global__ __launch_bounds__(IM_THREADS) void imap_fwd_kernel(int64_t P, const double* __restrict__ pts,
                                                              const float* __restrict__ pk, ImBound bd,
                                                              float* __restrict__ raw, Ws ws, int save) {
    __shared__ float Hs[IM_H * IM_LD];
    __shared__ float ps[IM_TM][3];
    __shared__ int outside[IM_TM];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int64_t p0 = (int64_t)blockIdx.x * IM_TM;
    if (t < IM_TM) {
        const int64_t p = p0 + t;
        double x = 0., y = 0., z = 0.;
        if (p < P) { x = pts[p * 3]; y = pts[p * 3 + 1]; z = pts[p * 3 + 2]; }
        ps[t][0] = (float)x; ps[t][1] = (float)y; ps[t][2] = (float)z;
        outside[t] = bd.on && im_outside(bd, x, y, z);
        if (save && p < P) {
            ws.pf[p * 4] = (float)x; ws.pf[p * 4 + 1] = (float)y; ws.pf[p * 4 + 2] = (float)z; ws.pf[p * 4 + 3] = 0.f;
        }
    }
    __syncthreads();
    // embedding, k fastest (coalesced workspace rows)
    for (int idx = t; idx < IM_TM * IM_EP; idx += IM_THREADS) {
        const int m = idx / IM_EP, k = idx % IM_EP;
        const float e = k < IM_E ? sinf(im_arg(ps[m], pk + PK_B, k, IM_EP)) : 0.f;
        Hs[k * IM_LD + m] = e;
        if (save && p0 + m < P) ws.e[(p0 + m) * IM_EP + k] = e;
    }
    __syncthreads();
    const int n0 = wave * 64;
    for (int l = 0; l < 4; ++l) {
        const float* WT = l == 0 ? pk + PK_W0 : pk + PK_L1 + (l - 1) * PK_LSTRIDE;
        const float* bias = l == 0 ? pk + PK_B0 : WT + IM_H * IM_H;
        f32x16 acc[2][2];
        tile_mm(Hs, l == 0 ? IM_EP : IM_H, WT, IM_H, n0, IM_H, lane, acc);
        __syncthreads();                      // every wave has read this layer's input
        for (int j = 0; j < 2; ++j) {
            const int n = n0 + 32 * j + (lane & 31);
            const float bn = bias[n];
            for (int i = 0; i < 2; ++i)
                for (int v = 0; v < 16; ++v) {
                    const int m = 32 * i + c_row(v, lane);
                    const float s = acc[i][j][v] + bn;
                    const float hv = s > 0.f ? s : 0.f;
                    Hs[n * IM_LD + m] = hv;
                    if (save && p0 + m < P) ws.h[l][(p0 + m) * IM_H + n] = hv;
                }
        }
        __syncthreads();
    }
    // output layer: thread (m, o)
    {
        const int m = t & 63, o = t >> 6;
        const float* wo = pk + PK_WO + o * IM_H;
        float s = 0.f;
#pragma unroll 8
        for (int k = 0; k < IM_H; ++k) s += Hs[k * IM_LD + m] * wo[k];
        s += pk[PK_BO + o];
        if (o == 3 && outside[m]) s = 100.f;
        if (p0 + m < P) raw[(p0 + m) * 4 + o] = s;
    }
}

// top-down dX chain of one 64-point tile; needs the workspace of imap_fwd_kernel(save)
__global__ __launch_bounds__(IM_THREADS) void imap_bwd_chain_kernel(int64_t P, const float* __restrict__ pk,
                                                                    const float* __restrict__ W0, const float* __restrict__ W1,
                                                                    const float* __restrict__ W2, const float* __restrict__ W3,
                                                                    ImBound bd, const double* __restrict__ pts,
                                                                    const float* __restrict__ d_raw, Ws ws,
                                                                    float* __restrict__ d_pts) {
    __shared__ float D[IM_H * IM_LD];
    __shared__ float ps[IM_TM][3];
    __shared__ float dos[IM_TM][4];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int64_t p0 = (int64_t)blockIdx.x * IM_TM;
    if (t < IM_TM) {
        const int64_t p = p0 + t;
        double x = 0., y = 0., z = 0.;
        float g[4] = {0.f, 0.f, 0.f, 0.f};
        if (p < P) {
            x = pts[p * 3]; y = pts[p * 3 + 1]; z = pts[p * 3 + 2];
            for (int o = 0; o < 4; ++o) g[o] = d_raw[p * 4 + o];
            if (bd.on && im_outside(bd, x, y, z)) g[3] = 0.f;     // sigma was overwritten with 100
            for (int o = 0; o < 4; ++o) ws.dout[p * 4 + o] = g[o];
        }
        ps[t][0] = (float)x; ps[t][1] = (float)y; ps[t][2] = (float)z;
        for (int o = 0; o < 4; ++o) dos[t][o] = g[o];
    }
    __syncthreads();
    // dPre3 = (dOut Wo) * [h4 > 0]: thread = column n
    {
        const int n = t;
        const float* wo = pk + PK_WO;
        const float w0 = wo[n], w1 = wo[IM_H + n], w2 = wo[2 * IM_H + n], w3 = wo[3 * IM_H + n];
        for (int m = 0; m < IM_TM; ++m) {
            const int64_t p = p0 + m;
            float g = 0.f;
            if (p < P && ws.h[3][p * IM_H + n] > 0.f)
                g = ((dos[m][0] * w0 + dos[m][1] * w1) + dos[m][2] * w2) + dos[m][3] * w3;
            D[n * IM_LD + m] = g;
            if (p < P) ws.dpre[3][p * IM_H + n] = g;
        }
    }
    __syncthreads();
    const int n0 = wave * 64;
    for (int l = 3; l >= 1; --l) {
        const float* W = l == 3 ? W3 : (l == 2 ? W2 : W1);
        f32x16 acc[2][2];
        tile_mm(D, IM_H, W, IM_H, n0, IM_H, lane, acc);      // dh_l = dPre_l W_l   ([m][k] = sum_n dPre[m][n] W[n][k])
        __syncthreads();
        const float* hin = ws.h[l - 1];
        for (int j = 0; j < 2; ++j) {
            const int k = n0 + 32 * j + (lane & 31);
            for (int i = 0; i < 2; ++i)
                for (int v = 0; v < 16; ++v) {
                    const int m = 32 * i + c_row(v, lane);
                    const int64_t p = p0 + m;
                    const float g = (p < P && hin[p * IM_H + k] > 0.f) ? acc[i][j][v] : 0.f;
                    D[k * IM_LD + m] = g;
                    if (p < P) ws.dpre[l - 1][p * IM_H + k] = g;
                }
        }
        __syncthreads();
    }
    // de = dPre0 W0 (64 x 93): six 32x32 tiles over four waves, then dz = de * cos(p . B)
    f32x16 acc[2];
    int tiles[2] = {wave, wave + 4};
    const int r = lane & 31, h = lane >> 5;
    for (int q = 0; q < 2; ++q) {
        for (int v = 0; v < 16; ++v) acc[q][v] = 0.f;
        if (tiles[q] >= 6) continue;
        const int mi = tiles[q] & 1, kt = tiles[q] >> 1;
        const int kcol = kt * 32 + r;
        const bool ok = kcol < IM_E;
#pragma unroll 4
        for (int n = 0; n < IM_H; n += 2) {
            const int nn = n + h;
            const float a = D[nn * IM_LD + mi * 32 + r];
            const float b = ok ? W0[nn * IM_E + kcol] : 0.f;
            acc[q] = mfma32(a, b, acc[q]);
        }
    }
    __syncthreads();
    for (int q = 0; q < 2; ++q) {
        if (tiles[q] >= 6) continue;
        const int mi = tiles[q] & 1, kt = tiles[q] >> 1;
        const int k = kt * 32 + r;
        for (int v = 0; v < 16; ++v) {
            const int m = mi * 32 + c_row(v, lane);
            float g = 0.f;
            if (k < IM_E) g = acc[q][v] * cosf(im_arg(ps[m], pk + PK_B, k, IM_EP));
            D[k * IM_LD + m] = g;
            if (p0 + m < P) ws.dz[(p0 + m) * IM_EP + k] = g;
        }
    }
    __syncthreads();
    // dp[m][c] = sum_k dz[m][k] B[c][k]
    if (t < IM_TM * 3) {
        const int m = t & 63, c = t >> 6;
        const float* Bc = pk + PK_B + c * IM_EP;
        float s = 0.f;
        for (int k = 0; k < IM_E; ++k) s += D[k * IM_LD + m] * Bc[k];
        if (p0 + m < P) d_pts[(p0 + m) * 3 + c] = s;
    }
}

// ---------------------------------------------------------------------------------------------- weight gradients
struct DwJob {
    const float* X;      // [P][ldx], columns 0..n1-1
    const float* Y;      // [P][ldy], columns 0..n2-1
    int ldx, n1, ldy, n2;
    int tiles_j;         // ceil(n2 / 64)
    int tile0;           // first flat tile index of this job
    int out_off;         // offset of this job's [n1][n2] result in the parameter-gradient layout
    int bias_off;        // offset of the [n1] column sums of X, or -1
};
constexpr int IM_JOBS = 6;
struct DwJobs {
    DwJob j[IM_JOBS];
    int n_tiles;
};

// gradient layout (IM_PARAM_FLOATS): B [3,93] | W0 [256,93] | b0 | W1 | b1 | W2 | b2 | W3 | b3 | Wo [4,256] | bo
constexpr int G_B = 0;
constexpr int G_W0 = G_B + 3 * IM_E;
constexpr int G_B0 = G_W0 + IM_H * IM_E;
constexpr int G_W1 = G_B0 + IM_H;
constexpr int G_LSTRIDE = IM_H * IM_H + IM_H;
constexpr int G_WO = G_W1 + 3 * G_LSTRIDE;
constexpr int G_BO = G_WO + 4 * IM_H;

// one wave: a 64x64 tile of X^T Y over the points of slice blockIdx.y
__global__ __launch_bounds__(64) void imap_dw_kernel(int64_t P, int slices, DwJobs jobs, float* __restrict__ part) {
    const int tile = blockIdx.x, s = blockIdx.y, lane = threadIdx.x;
    int ji = 0;
    while (ji + 1 < IM_JOBS && tile >= jobs.j[ji + 1].tile0) ++ji;
    const DwJob J = jobs.j[ji];
    const int lt = tile - J.tile0;
    const int i0 = (lt / J.tiles_j) * 64, j0 = (lt % J.tiles_j) * 64;
    int64_t per = (P + slices - 1) / slices;
    per = (per + 1) & ~(int64_t)1;
    const int64_t m_beg = s * per, m_end = m_beg + per < P ? m_beg + per : P;
    const int r = lane & 31, h = lane >> 5;
    const bool xa = i0 + r < J.n1, xb = i0 + 32 + r < J.n1;
    const bool ya = j0 + r < J.n2, yb = j0 + 32 + r < J.n2;
    f32x16 acc[2][2];
    for (int i = 0; i < 2; ++i)
        for (int j = 0; j < 2; ++j)
            for (int v = 0; v < 16; ++v) acc[i][j][v] = 0.f;
    float bs0 = 0.f, bs1 = 0.f;
    for (int64_t m = m_beg; m < m_end; m += 2) {
        const int64_t mm = m + h;
        const bool ok = mm < m_end;
        const float* xr = J.X + mm * J.ldx + i0;
        const float* yr = J.Y + mm * J.ldy + j0;
        const float a0 = (ok && xa) ? xr[r] : 0.f, a1 = (ok && xb) ? xr[32 + r] : 0.f;
        const float b0 = (ok && ya) ? yr[r] : 0.f, b1 = (ok && yb) ? yr[32 + r] : 0.f;
        bs0 += a0;
        bs1 += a1;
        acc[0][0] = mfma32(a0, b0, acc[0][0]);
        acc[0][1] = mfma32(a0, b1, acc[0][1]);
        acc[1][0] = mfma32(a1, b0, acc[1][0]);
        acc[1][1] = mfma32(a1, b1, acc[1][1]);
    }
    float* out = part + (int64_t)s * IM_PARAM_FLOATS;
    // A[i][k] = X[m][i0 + i]: accumulator rows are X's columns (the parameter's output index), columns are Y's
    for (int i = 0; i < 2; ++i)
        for (int j = 0; j < 2; ++j) {
            const int col = j0 + 32 * j + r;
            if (col >= J.n2) continue;
            for (int v = 0; v < 16; ++v) {
                const int row = i0 + 32 * i + c_row(v, lane);
                if (row < J.n1) out[J.out_off + row * J.n2 + col] = acc[i][j][v];
            }
        }
    if (J.bias_off >= 0 && j0 == 0) {
        bs0 += __shfl_xor(bs0, 32);
        bs1 += __shfl_xor(bs1, 32);
        if (h == 0) {
            if (xa) out[J.bias_off + i0 + r] = bs0;
            if (xb) out[J.bias_off + i0 + 32 + r] = bs1;
        }
    }
}

__constant__ int c_goffs[12] = {G_B, G_W0, G_B0, G_W1, G_W1 + IM_H * IM_H, G_W1 + G_LSTRIDE,
                                G_W1 + G_LSTRIDE + IM_H * IM_H, G_W1 + 2 * G_LSTRIDE, G_W1 + 2 * G_LSTRIDE + IM_H * IM_H,
                                G_WO, G_BO, IM_PARAM_FLOATS};

struct GradPtrs {
    float* g[11];
};

__global__ __launch_bounds__(256) void imap_reduce_kernel(int slices, const float* __restrict__ part, GradPtrs gp,
                                                          int accumulate) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= IM_PARAM_FLOATS) return;
    float s = 0.f;
    for (int q = 0; q < slices; ++q) s += part[(int64_t)q * IM_PARAM_FLOATS + e];
    int t = 0;
    while (e >= c_goffs[t + 1]) ++t;
    float* dst = gp.g[t] + (e - c_goffs[t]);
    *dst = accumulate ? *dst + s : s;
}

int im_slices(int64_t P) {
    int64_t s = P / 1024;
    return (int)(s < 1 ? 1 : (s > IM_MAX_SLICES ? IM_MAX_SLICES : s));
}

bool im_bound(const double* bound_host, ImBound& b) {
    b.on = bound_host != nullptr;
    for (int c = 0; c < 3; ++c) {
        b.lo[c] = b.on ? bound_host[2 * c] : 0.;
        b.hi[c] = b.on ? bound_host[2 * c + 1] : 0.;
    }
    return true;
}

// ---------------------------------------------------------------------------------------------- density compositing
constexpr int DC_THREADS = 64;
constexpr int DC_MAX_S = 64;

// per-sample quantities of raw2outputs_nerf_color(occupancy=False), float32 as in the reference
ENS_DEV float dc_dd(const double* z, int s, int S) { return s + 1 < S ? (float)(z[s + 1] - z[s]) : 1e10f; }

ENS_DEV float dc_norm(const float* d) {
    const float x = d[0], y = d[1], z = d[2];
    return sqrtf((x * x + y * y) + z * z);
}

__global__ __launch_bounds__(DC_THREADS) void composite_density_fwd_kernel(int N, int S, const float* __restrict__ raw,
                                                                           const double* __restrict__ zv,
                                                                           const float* __restrict__ rays_d,
                                                                           double* __restrict__ depth, double* __restrict__ var,
                                                                           float* __restrict__ rgb, float* __restrict__ wts) {
    const int n = blockIdx.x * DC_THREADS + threadIdx.x;
    if (n >= N) return;
    const float nd = dc_norm(rays_d + (int64_t)n * 3);
    const float* rr = raw + (int64_t)n * S * 4;
    const double* z = zv + (int64_t)n * S;
    float T = 1.f, c0 = 0.f, c1 = 0.f, c2 = 0.f;
    double D = 0.;
    for (int s = 0; s < S; ++s) {
        const float dist = dc_dd(z, s, S) * nd;
        const float sg = rr[s * 4 + 3] > 0.f ? rr[s * 4 + 3] : 0.f;
        const float a = 1.f - expf(-(sg * dist));
        const float w = a * T;
        T = T * ((1.f - a) + 1e-10f);
        c0 += w * rr[s * 4];
        c1 += w * rr[s * 4 + 1];
        c2 += w * rr[s * 4 + 2];
        D += (double)w * z[s];
        if (wts) wts[(int64_t)n * S + s] = w;
    }
    // the variance needs the depth: second walk, recomputing the weights bit for bit
    double V = 0.;
    T = 1.f;
    for (int s = 0; s < S; ++s) {
        const float dist = dc_dd(z, s, S) * nd;
        const float sg = rr[s * 4 + 3] > 0.f ? rr[s * 4 + 3] : 0.f;
        const float a = 1.f - expf(-(sg * dist));
        const float w = a * T;
        T = T * ((1.f - a) + 1e-10f);
        const double d = z[s] - D;
        V += (double)w * d * d;
    }
    depth[n] = D;
    var[n] = V;
    rgb[n * 3] = c0;
    rgb[n * 3 + 1] = c1;
    rgb[n * 3 + 2] = c2;
}

// Backward as torch's autograd takes it: weights -> (alpha, cumprod); cumprod's backward is torch's no-zero formula
// (reverse cumulative sum of grad * output, divided by the input), so a running product that underflowed to 0 gives
// what torch gives there.  d rays_d = d|d| * d / |d| (0 for |d| = 0, as torch's norm backward).
__global__ __launch_bounds__(DC_THREADS) void composite_density_bwd_kernel(int N, int S, const float* __restrict__ raw,
                                                                           const double* __restrict__ zv,
                                                                           const float* __restrict__ rays_d,
                                                                           const double* __restrict__ depth,
                                                                           const double* __restrict__ gD,
                                                                           const double* __restrict__ gV,
                                                                           const float* __restrict__ gC,
                                                                           float* __restrict__ d_raw, float* __restrict__ d_rd) {
    __shared__ float sT[DC_MAX_S][DC_THREADS];
    __shared__ float sA[DC_MAX_S][DC_THREADS];
    const int tid = threadIdx.x;
    const int n = blockIdx.x * DC_THREADS + tid;
    if (n >= N) return;
    const float* rd = rays_d + (int64_t)n * 3;
    const float nd = dc_norm(rd);
    const float* rr = raw + (int64_t)n * S * 4;
    const double* z = zv + (int64_t)n * S;
    const double D = depth[n];
    const double gd = gD ? gD[n] : 0., gv = gV ? gV[n] : 0.;
    const float g0 = gC ? gC[n * 3] : 0.f, g1 = gC ? gC[n * 3 + 1] : 0.f, g2 = gC ? gC[n * 3 + 2] : 0.f;
    float T = 1.f;
    double swz = 0.;
    for (int s = 0; s < S; ++s) {
        const float dist = dc_dd(z, s, S) * nd;
        const float sg = rr[s * 4 + 3] > 0.f ? rr[s * 4 + 3] : 0.f;
        const float a = 1.f - expf(-(sg * dist));
        sT[s][tid] = T;
        sA[s][tid] = a;
        swz += (double)(a * T) * (z[s] - D);
        T = T * ((1.f - a) + 1e-10f);
    }
    const double gDe = gd + gv * (-2. * swz);        // the depth's share of the variance's gradient
    float R = 0.f, gnd = 0.f;
    float* dr = d_raw + (int64_t)n * S * 4;
    for (int s = S - 1; s >= 0; --s) {
        const float Ts = sT[s][tid], a = sA[s][tid];
        const float w = a * Ts;
        const double dz = z[s] - D;
        const float gw = ((float)(gDe * z[s]) + (float)(gv * dz * dz)) + ((g0 * rr[s * 4] + g1 * rr[s * 4 + 1]) + g2 * rr[s * 4 + 2]);
        const float f = (1.f - a) + 1e-10f;
        const float df = R / f;                       // d cumprod input f_s = sum_{k > s} gT_k T_k / f_s
        R += (gw * a) * Ts;
        const float ga = gw * Ts - df;
        const float dd = dc_dd(z, s, S);
        const float dist = dd * nd;
        const float sraw = rr[s * 4 + 3];
        const float sg = sraw > 0.f ? sraw : 0.f;
        const float gx = ga * expf(-(sg * dist));     // alpha = 1 - exp(-x)
        dr[s * 4] = w * g0;
        dr[s * 4 + 1] = w * g1;
        dr[s * 4 + 2] = w * g2;
        dr[s * 4 + 3] = sraw > 0.f ? gx * dist : 0.f;
        gnd += (gx * sg) * dd;
    }
    if (d_rd) {
        const float k = nd > 0.f ? gnd / nd : 0.f;
        d_rd[n * 3] = k * rd[0];
        d_rd[n * 3 + 1] = k * rd[1];
        d_rd[n * 3 + 2] = k * rd[2];
    }
}

}  // namespace

extern "C" {

size_t enslam_imap_packed_floats(void) { return (size_t)PK_FLOATS; }

size_t enslam_imap_workspace_floats(int64_t n_points) {
    if (n_points < 0) return 0;
    return (size_t)(n_points * WS_PER_POINT + (int64_t)im_slices(n_points) * IM_PARAM_FLOATS);
}

int enslam_imap_pack(const float* const* params, float* packed, void* stream) {
    if (!params || !packed) return ENSLAM_EINVAL;
    for (int i = 0; i < 11; ++i)
        if (!params[i]) return ENSLAM_EINVAL;
    const int blocks = (int)((PK_FLOATS + 255) / 256);
    imap_pack_kernel<<<blocks, 256, 0, (hipStream_t)stream>>>(params[0], params[1], params[2], params[3], params[4], params[5],
                                                              params[6], params[7], params[8], params[9], params[10], packed);
    return hipGetLastError() == hipSuccess ? ENSLAM_OK : ENSLAM_ELAUNCH;
}

int enslam_imap_fwd(int64_t n_points, const double* points, const float* packed, const double* bound_host, float* raw,
                    void* stream) {
    if (n_points < 0 || (n_points > 0 && (!points || !packed || !raw))) return ENSLAM_EINVAL;
    if (n_points == 0) return ENSLAM_OK;
    if ((n_points + IM_TM - 1) / IM_TM > INT32_MAX) return ENSLAM_EUNSUPPORTED;
    ImBound b;
    im_bound(bound_host, b);
    Ws none = {};
    imap_fwd_kernel<<<(unsigned)((n_points + IM_TM - 1) / IM_TM), IM_THREADS, 0, (hipStream_t)stream>>>(
        n_points, points, packed, b, raw, none, 0);
    return hipGetLastError() == hipSuccess ? ENSLAM_OK : ENSLAM_ELAUNCH;
}

int enslam_imap_bwd(int64_t n_points, const double* points, const float* const* params, const float* packed,
                    const double* bound_host, const float* d_raw, float* workspace, int32_t accumulate, float* const* grads,
                    float* d_points, void* stream) {
    if (n_points < 0 || !params || !grads) return ENSLAM_EINVAL;
    for (int i = 0; i < 11; ++i)
        if (!params[i] || !grads[i]) return ENSLAM_EINVAL;
    if (n_points > 0 && (!points || !packed || !d_raw || !workspace || !d_points)) return ENSLAM_EINVAL;
    if ((n_points + IM_TM - 1) / IM_TM > INT32_MAX) return ENSLAM_EUNSUPPORTED;
    hipStream_t s = (hipStream_t)stream;
    ImBound b;
    im_bound(bound_host, b);
    const int64_t P = n_points;
    const int slices = im_slices(P);
    Ws ws = ws_carve(workspace, P);
    GradPtrs gp;
    for (int i = 0; i < 11; ++i) gp.g[i] = grads[i];
    if (P > 0) {
        const unsigned blocks = (unsigned)((P + IM_TM - 1) / IM_TM);
        // (the recompute's raw output lands in the dz rows, which the chain overwrites: no extra buffer)
        imap_fwd_kernel<<<blocks, IM_THREADS, 0, s>>>(P, points, packed, b, ws.dz, ws, 1);
        imap_bwd_chain_kernel<<<blocks, IM_THREADS, 0, s>>>(P, packed, params[1], params[3], params[5], params[7], b,
                                                            points, d_raw, ws, d_points);
        DwJobs jobs;
        int tile = 0;
        auto add = [&](int q, const float* X, int ldx, int n1, const float* Y, int ldy, int n2, int out_off, int bias_off) {
            DwJob& J = jobs.j[q];
            J.X = X; J.Y = Y; J.ldx = ldx; J.n1 = n1; J.ldy = ldy; J.n2 = n2;
            J.tiles_j = (n2 + 63) / 64;
            J.tile0 = tile;
            J.out_off = out_off;
            J.bias_off = bias_off;
            tile += ((n1 + 63) / 64) * J.tiles_j;
        };
        add(0, ws.pf, 4, 3, ws.dz, IM_EP, IM_E, G_B, -1);
        add(1, ws.dpre[0], IM_H, IM_H, ws.e, IM_EP, IM_E, G_W0, G_B0);
        for (int l = 1; l < 4; ++l) {
            const int off = G_W1 + (l - 1) * G_LSTRIDE;
            add(1 + l, ws.dpre[l], IM_H, IM_H, ws.h[l - 1], IM_H, IM_H, off, off + IM_H * IM_H);
        }
        add(5, ws.dout, 4, 4, ws.h[3], IM_H, IM_H, G_WO, G_BO);
        jobs.n_tiles = tile;
        imap_dw_kernel<<<dim3(tile, slices), 64, 0, s>>>(P, slices, jobs, ws.part);
        imap_reduce_kernel<<<(IM_PARAM_FLOATS + 255) / 256, 256, 0, s>>>(slices, ws.part, gp, accumulate);
    } else if (!accumulate) {
        for (int i = 0; i < 11; ++i) {
            static const int sizes[11] = {3 * IM_E, IM_H * IM_E, IM_H, IM_H * IM_H, IM_H, IM_H * IM_H, IM_H, IM_H * IM_H, IM_H,
                                          4 * IM_H, 4};
            if (hipMemsetAsync(grads[i], 0, sizes[i] * sizeof(float), s) != hipSuccess) return ENSLAM_ELAUNCH;
        }
    }
    return hipGetLastError() == hipSuccess ? ENSLAM_OK : ENSLAM_ELAUNCH;
}

int enslam_composite_density_fwd(int32_t n_rays, int32_t n_samples, const float* raw, const double* z_vals,
                                 const float* rays_d, double* depth, double* var, float* rgb, float* weights, void* stream) {
    if (n_rays < 0 || n_samples < 1 || n_samples > DC_MAX_S) return ENSLAM_EINVAL;
    if (n_rays == 0) return ENSLAM_OK;
    if (!raw || !z_vals || !rays_d || !depth || !var || !rgb) return ENSLAM_EINVAL;
    composite_density_fwd_kernel<<<(n_rays + DC_THREADS - 1) / DC_THREADS, DC_THREADS, 0, (hipStream_t)stream>>>(
        n_rays, n_samples, raw, z_vals, rays_d, depth, var, rgb, weights);
    return hipGetLastError() == hipSuccess ? ENSLAM_OK : ENSLAM_ELAUNCH;
}

int enslam_composite_density_bwd(int32_t n_rays, int32_t n_samples, const float* raw, const double* z_vals,
                                 const float* rays_d, const double* depth, const double* g_depth, const double* g_var,
                                 const float* g_rgb, float* d_raw, float* d_rays_d, void* stream) {
    if (n_rays < 0 || n_samples < 1 || n_samples > DC_MAX_S) return ENSLAM_EINVAL;
    if (n_rays == 0) return ENSLAM_OK;
    if (!raw || !z_vals || !rays_d || !depth || !d_raw) return ENSLAM_EINVAL;
    composite_density_bwd_kernel<<<(n_rays + DC_THREADS - 1) / DC_THREADS, DC_THREADS, 0, (hipStream_t)stream>>>(
        n_rays, n_samples, raw, z_vals, rays_d, depth, g_depth, g_var, g_rgb, d_raw, d_rays_d);
    return hipGetLastError() == hipSuccess ? ENSLAM_OK : ENSLAM_ELAUNCH;
}

}  // extern "C"
