// Event motion compensation by contrast maximisation (enslam_event_cmax_eval, enslam_event_cmax_rigid_eval and
// enslam_event_cmax_reg_eval; enslam_hip.h
// holds the models and fixes the order of every float64 operation): the image of warped events of a stream under a candidate motion, the variance of its blur and
// the gradient of that variance in the motion.  One evaluation is a fixed chain of launches on one stream:
//
//   zero     one thread per pixel: the IWE, the drop counters and stats start from zero.  A kernel, not memsets: captured as
//            memset nodes, the three did not zero their buffers again from the second replay of the graph on
//            (tests/test_hip_event_cmax_rigid.py replays one captured evaluation over refilled outputs)
//   vote     one thread per event: sensor check, time check, (rigid: depth check,) warp, the float64 range check, then up to
//            four 64-bit integer atomic adds of llrint(w 2^32) into the int64 IWE (corners of weight 0 are not sent).  The drop
//            counters are summed per workgroup in LDS, then one global integer add per workgroup and counter.
//   rows     one thread per pixel: r = the row pass of the zero-padded blur (of the IWE times 2^-32, or of J - mu)
//   columns  one thread per pixel: the column pass; for J also the first level of SUM(J) (256 consecutive pixels per
//            workgroup, halving tree in LDS, one partial per workgroup)
//   upper    one workgroup: the partials 256 at a time through the same tree, thread 0 adds the results in ascending order
//            and writes mu, f or the gradient
//   centre   one thread per pixel: J - mu, and the first level of SUM((J - mu)^2)
//   gather   one thread per event: the same warp, the four D values of its corners, its P products into the block tree in LDS
//   reg      (enslam_event_cmax_reg_eval with a regulariser only) one thread per event, after everything above: the same warp
//            and the same checks once more, then the event's |divergence| or |deformation| of the header and, with want_grad,
//            its P derivatives through the block tree in LDS ((1 + P) x 256 doubles, 14 KB for rigid; 2 KB without the
//            gradient), one row of 1 + P partials per workgroup.  Its own launch and not a part of the gather, because R is
//            wanted without the gradient too and the gather only runs with it; the pass reads the stream (and the depth at the
//            checked pixel) and nothing of the image, about 18 bytes per event.
//   reg_upper  one workgroup: the upper levels of those partials, divided by M = N minus the drop counters, which it reads on
//            the device (the vote that wrote them is earlier on the same stream: no read-back, no fence)
// Integer atomics for the image, fixed trees for every float64 sum, no float atomics, no fences: two runs give the same
// bits, and the numpy route of event_cmax.py, which performs the same operations in the same order, gives them too.
// The three models share one warp (cm_warp<MODEL>), one vote and one gather; the kernels are templates of the model only so
// that the factors Bu, Bv and the gather's LDS tree have the model's own size (rigid: 6 x 256 doubles = 12 KB).
// Every address comes from a checked value: the event's own x, y against the sensor before anything else (the rigid model
// reads its depth at that checked pixel and nowhere else), the warped position against (-1, W) x (-1, H) in float64 before floor() and the conversion, every corner against the image.
#include "../../include/enslam_hip.h"
#include "common.hpp"

#include <cmath>

namespace {

constexpr int CM_BLOCK = 256;
constexpr int CM_KMAX = ENSLAM_CMAX_MAX_KSIZE;
constexpr int CM_PMAX = 6;
constexpr int CM_RIGID = ENSLAM_CMAX_RIGID;                 // the third model: refused by enslam_event_cmax_eval
constexpr int64_t CM_MAX_EVENTS = 2147483647;
constexpr int64_t CM_MAX_PIXELS = (int64_t)1 << 28;
constexpr double CM_TWO32 = 4294967296.0;
constexpr double CM_INV_TWO32 = 1.0 / 4294967296.0;

struct CmStream {
    const double* t;
    const uint16_t* x;
    const uint16_t* y;
    const uint8_t* p;
    const float* depth;                                     // [H,W], the rigid model's; nullptr otherwise
    int64_t N;
    int32_t H, W, model, sign_votes;
    double fx, fy, cx, cy, t_ref;
    double theta[CM_PMAX];
};

struct CmBlur {
    int32_t H, W, k;
    double taps[CM_KMAX];
};

// what the header calls a vote: the cell (x0, y0), the fractions and the factors of the gradient
template <int P>
struct CmWarp {
    int x0, y0;
    double a, b, oa, ob, mx, my, s;
    double Bu[P], Bv[P];
    double dt, u, v, rho;                                   // what the regulariser takes (flow: not set; rotation: rho = 0.0)
};

constexpr int cm_params(int model) { return model == ENSLAM_CMAX_FLOW ? 2 : model == ENSLAM_CMAX_ROTATION ? 3 : 6; }

enum { CM_OK = -1 };

// CM_OK, or the drop counter of event i.  The operations and their order are the header's.
template <int MODEL>
__device__ __forceinline__ int cm_warp(const CmStream& S, int64_t i, CmWarp<cm_params(MODEL)>& Q) {
    const unsigned ex = S.x[i], ey = S.y[i];
    if (ex >= (unsigned)S.W || ey >= (unsigned)S.H) return ENSLAM_CMAX_DROP_SENSOR;
    const double tv = S.t[i];
    if (!std::isfinite(tv)) return ENSLAM_CMAX_DROP_TIME;
    const double xd = (double)ex, yd = (double)ey;
    const double dt = tv - S.t_ref;
    double du, dv;
    Q.dt = dt;
    if constexpr (MODEL == ENSLAM_CMAX_FLOW) {
        Q.Bu[0] = 1.0 / S.fx; Q.Bu[1] = 0.0;
        Q.Bv[0] = 0.0; Q.Bv[1] = 1.0 / S.fy;
        du = S.theta[0] / S.fx;
        dv = S.theta[1] / S.fy;
    } else {
        const double u = (xd - S.cx) / S.fx, v = (yd - S.cy) / S.fy;
        const double uv = u * v, pu = 1.0 + u * u, pv = 1.0 + v * v;
        Q.Bu[0] = uv; Q.Bu[1] = -pu; Q.Bu[2] = v;
        Q.Bv[0] = pv; Q.Bv[1] = -uv; Q.Bv[2] = -u;
        du = (uv * S.theta[0] - pu * S.theta[1]) + v * S.theta[2];
        dv = (pv * S.theta[0] - uv * S.theta[1]) - u * S.theta[2];
        Q.u = u; Q.v = v; Q.rho = 0.0;
        if constexpr (MODEL == CM_RIGID) {
            const float z = S.depth[(int64_t)ey * S.W + ex];            // ex < W, ey < H: checked above
            if (!(std::isfinite(z) && z > 0.0f)) return ENSLAM_CMAX_DROP_DEPTH;
            const double rho = 1.0 / (double)z;
            Q.rho = rho;
            Q.Bu[3] = -rho; Q.Bu[4] = 0.0; Q.Bu[5] = u * rho;
            Q.Bv[3] = 0.0; Q.Bv[4] = -rho; Q.Bv[5] = v * rho;
            du = du + rho * (u * S.theta[5] - S.theta[3]);
            dv = dv + rho * (v * S.theta[5] - S.theta[4]);
        }
    }
    Q.mx = -(dt * S.fx);
    Q.my = -(dt * S.fy);
    const double xw = xd + Q.mx * du, yw = yd + Q.my * dv;
    if (!(xw > -1.0 && xw < (double)S.W && yw > -1.0 && yw < (double)S.H)) return ENSLAM_CMAX_DROP_WARP;
    const double fx0 = floor(xw), fy0 = floor(yw);            // in [-1, W - 1] x [-1, H - 1]: the conversion is safe
    Q.x0 = (int)fx0;
    Q.y0 = (int)fy0;
    Q.a = xw - fx0;
    Q.b = yw - fy0;
    Q.oa = 1.0 - Q.a;
    Q.ob = 1.0 - Q.b;
    Q.s = (S.sign_votes && !S.p[i]) ? -1.0 : 1.0;
    return CM_OK;
}

template <int P>
__device__ __forceinline__ bool cm_corner(const CmStream& S, const CmWarp<P>& Q, int c, int64_t& cell) {
    const int px = Q.x0 + (c & 1), py = Q.y0 + (c >> 1);
    if (px < 0 || px >= S.W || py < 0 || py >= S.H) return false;
    cell = (int64_t)py * S.W + px;
    return true;
}

__global__ __launch_bounds__(CM_BLOCK) void cmax_zero_kernel(long long* __restrict__ iwe, int64_t npix, unsigned long long* __restrict__ dropped,
                                                             int n_dropped, double* __restrict__ stats, int n_stats,
                                                             double* __restrict__ reg_stats, int n_reg) {
    const int64_t o = (int64_t)blockIdx.x * CM_BLOCK + threadIdx.x;
    if (o < npix) iwe[o] = 0;
    if (blockIdx.x == 0) {
        if ((int)threadIdx.x < n_dropped) dropped[threadIdx.x] = 0ull;
        if ((int)threadIdx.x < n_stats) stats[threadIdx.x] = 0.0;
        if ((int)threadIdx.x < n_reg) reg_stats[threadIdx.x] = 0.0;
    }
}

// dropped has three counters, four for the rigid model: only that model returns the fourth, and a counter of 0 is not sent
template <int MODEL>
__global__ __launch_bounds__(CM_BLOCK) void cmax_vote_kernel(CmStream S, unsigned long long* iwe, unsigned long long* dropped) {
    __shared__ unsigned s_drop[4];
    if (threadIdx.x < 4) s_drop[threadIdx.x] = 0u;
    __syncthreads();
    const int64_t i = (int64_t)blockIdx.x * CM_BLOCK + threadIdx.x;
    if (i < S.N) {
        CmWarp<cm_params(MODEL)> Q;
        const int why = cm_warp<MODEL>(S, i, Q);
        if (why != CM_OK) {
            atomicAdd(&s_drop[why], 1u);
        } else {
            const double w[4] = {Q.oa * Q.ob, Q.a * Q.ob, Q.oa * Q.b, Q.a * Q.b};
            for (int c = 0; c < 4; ++c) {
                int64_t cell;
                if (!cm_corner(S, Q, c, cell)) continue;
                long long q = llrint(w[c] * CM_TWO32);
                if (q == 0) continue;
                if (Q.s < 0.0) q = -q;
                atomicAdd(&iwe[cell], (unsigned long long)q);       // two's complement: the wrapped sum is the signed sum
            }
        }
    }
    __syncthreads();
    if (threadIdx.x < 4 && s_drop[threadIdx.x]) atomicAdd(&dropped[threadIdx.x], (unsigned long long)s_drop[threadIdx.x]);
}

// the halving tree of the header over the workgroup's 256 values; every thread gets the result
__device__ __forceinline__ double cm_block_sum(double* red, double v) {
    red[threadIdx.x] = v;
    __syncthreads();
    for (int s = CM_BLOCK / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    const double out = red[0];
    __syncthreads();
    return out;
}

__device__ __forceinline__ double cm_value(const long long* src, int64_t o) { return (double)src[o] * CM_INV_TWO32; }
__device__ __forceinline__ double cm_value(const double* src, int64_t o) { return src[o]; }

template <typename T>
__global__ __launch_bounds__(CM_BLOCK) void cmax_rows_kernel(CmBlur B, const T* __restrict__ src, double* __restrict__ dst) {
    const int64_t o = (int64_t)blockIdx.x * CM_BLOCK + threadIdx.x;
    if (o >= (int64_t)B.H * B.W) return;
    const int y = (int)(o / B.W), x = (int)(o - (int64_t)y * B.W), R = B.k / 2;
    double acc = 0.0;
    for (int i = 0; i < B.k; ++i) {
        const int xs = x - R + i;
        const double val = (xs >= 0 && xs < B.W) ? cm_value(src, (int64_t)y * B.W + xs) : 0.0;
        acc += B.taps[i] * val;
    }
    dst[o] = acc;
}

// the column pass; SUM: also the workgroup's partial of SUM(dst)
template <bool SUM>
__global__ __launch_bounds__(CM_BLOCK) void cmax_cols_kernel(CmBlur B, const double* __restrict__ src, double* __restrict__ dst,
                                                             double* __restrict__ partials) {
    __shared__ double s_red[CM_BLOCK];
    const int64_t o = (int64_t)blockIdx.x * CM_BLOCK + threadIdx.x;
    const bool inside = o < (int64_t)B.H * B.W;
    double acc = 0.0;
    if (inside) {
        const int y = (int)(o / B.W), x = (int)(o - (int64_t)y * B.W), R = B.k / 2;
        for (int i = 0; i < B.k; ++i) {
            const int ys = y - R + i;
            const double val = (ys >= 0 && ys < B.H) ? src[(int64_t)ys * B.W + x] : 0.0;
            acc += B.taps[i] * val;
        }
        dst[o] = acc;
    }
    if (SUM) {
        const double tot = cm_block_sum(s_red, acc);
        if (threadIdx.x == 0) partials[blockIdx.x] = tot;
    }
}

__global__ __launch_bounds__(CM_BLOCK) void cmax_centre_kernel(const double* __restrict__ J, const double* __restrict__ stats,
                                                               int64_t npix, double* __restrict__ C, double* __restrict__ partials) {
    __shared__ double s_red[CM_BLOCK];
    const int64_t o = (int64_t)blockIdx.x * CM_BLOCK + threadIdx.x;
    double sq = 0.0;
    if (o < npix) {
        const double c = J[o] - stats[0];
        C[o] = c;
        sq = c * c;
    }
    const double tot = cm_block_sum(s_red, sq);
    if (threadIdx.x == 0) partials[blockIdx.x] = tot;
}

// The upper levels of SUM for `cols` interleaved columns of n partials: 256 at a time through the tree, the results added in
// ascending order.  out[c] = scale_first ? scale * sum : sum / scale.
__global__ __launch_bounds__(CM_BLOCK) void cmax_upper_kernel(const double* __restrict__ partials, int64_t n, int cols, double scale,
                                                              int scale_first, double* __restrict__ out) {
    __shared__ double s_red[CM_BLOCK];
    for (int c = 0; c < cols; ++c) {
        double acc = 0.0;
        for (int64_t base = 0; base < n; base += CM_BLOCK) {
            const int64_t i = base + threadIdx.x;
            acc += cm_block_sum(s_red, i < n ? partials[i * cols + c] : 0.0);
        }
        if (threadIdx.x == 0) out[c] = scale_first ? scale * acc : acc / scale;
    }
}

template <int MODEL>
__global__ __launch_bounds__(CM_BLOCK) void cmax_gather_kernel(CmStream S, const double* __restrict__ D, double* __restrict__ partials) {
    constexpr int P = cm_params(MODEL);
    __shared__ double s_red[P * CM_BLOCK];
    const int64_t i = (int64_t)blockIdx.x * CM_BLOCK + threadIdx.x;
    double g[P] = {};
    if (i < S.N) {
        CmWarp<P> Q;
        if (cm_warp<MODEL>(S, i, Q) == CM_OK) {
            const double dwx[4] = {-Q.ob, Q.ob, -Q.b, Q.b}, dwy[4] = {-Q.oa, -Q.a, Q.oa, Q.a};
            double Gx = 0.0, Gy = 0.0;
            for (int c = 0; c < 4; ++c) {
                int64_t cell;
                if (!cm_corner(S, Q, c, cell)) continue;
                const double d = D[cell];
                Gx += d * dwx[c];
                Gy += d * dwy[c];
            }
            for (int k = 0; k < P; ++k) g[k] = Q.s * (Gx * (Q.mx * Q.Bu[k]) + Gy * (Q.my * Q.Bv[k]));
        }
    }
    for (int k = 0; k < P; ++k) s_red[k * CM_BLOCK + threadIdx.x] = g[k];
    __syncthreads();
    for (int s = CM_BLOCK / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s)
            for (int k = 0; k < P; ++k) s_red[k * CM_BLOCK + threadIdx.x] += s_red[k * CM_BLOCK + threadIdx.x + s];
        __syncthreads();
    }
    if ((int)threadIdx.x < P) partials[(int64_t)blockIdx.x * P + threadIdx.x] = s_red[threadIdx.x * CM_BLOCK];
}

// The collapse regulariser of the header: per event that reaches CM_OK, r = |d| with d the divergence of the warp's flow or
// det(dx'/dx) - 1, and with GRAD its P derivatives, through the block tree; one row of COLS = 1 + P (GRAD) or 1 partials per
// workgroup.  Rotation is the rho = 0 case of rigid (S.theta[3..5] are 0.0 for it); flow has no launch (R = 0 exactly).
template <int MODEL, bool GRAD>
__global__ __launch_bounds__(CM_BLOCK) void cmax_reg_kernel(CmStream S, int kind, double* __restrict__ partials) {
    constexpr int P = cm_params(MODEL), COLS = GRAD ? 1 + P : 1;
    __shared__ double s_red[COLS * CM_BLOCK];
    const int64_t i = (int64_t)blockIdx.x * CM_BLOCK + threadIdx.x;
    double out[COLS] = {};
    if (i < S.N) {
        CmWarp<P> Q;
        if (cm_warp<MODEL>(S, i, Q) == CM_OK) {
            const double u = Q.u, v = Q.v, rho = Q.rho, dt = Q.dt;
            const double c11 = (v * S.theta[0] - (2.0 * u) * S.theta[1]) + rho * S.theta[5];
            const double c22 = ((2.0 * v) * S.theta[0] - u * S.theta[1]) + rho * S.theta[5];
            const double c12 = u * S.theta[0] + S.theta[2];
            const double c21 = -(v * S.theta[1]) - S.theta[2];
            const double dt2 = dt * dt;
            const bool deform = kind == ENSLAM_CMAX_REG_DEFORMATION;
            double d = -(dt * (c11 + c22));
            if (deform) d = d + dt2 * (c11 * c22 - c12 * c21);
            out[0] = fabs(d);
            if constexpr (GRAD) {
                const double sg = d > 0.0 ? 1.0 : (d < 0.0 ? -1.0 : 0.0);
                const double e11[6] = {v, -(2.0 * u), 0.0, 0.0, 0.0, rho}, e22[6] = {2.0 * v, -u, 0.0, 0.0, 0.0, rho};
                const double e12[6] = {u, 0.0, 1.0, 0.0, 0.0, 0.0}, e21[6] = {0.0, -v, -1.0, 0.0, 0.0, 0.0};
                for (int k = 0; k < P; ++k) {
                    double dd = -(dt * (e11[k] + e22[k]));
                    if (deform) dd = dd + dt2 * ((e11[k] * c22 + c11 * e22[k]) - (e12[k] * c21 + c12 * e21[k]));
                    out[1 + k] = sg * dd;
                }
            }
        }
    }
    for (int c = 0; c < COLS; ++c) s_red[c * CM_BLOCK + threadIdx.x] = out[c];
    __syncthreads();
    for (int s = CM_BLOCK / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s)
            for (int c = 0; c < COLS; ++c) s_red[c * CM_BLOCK + threadIdx.x] += s_red[c * CM_BLOCK + threadIdx.x + s];
        __syncthreads();
    }
    if ((int)threadIdx.x < COLS) partials[(int64_t)blockIdx.x * COLS + threadIdx.x] = s_red[threadIdx.x * CM_BLOCK];
}

// cmax_upper_kernel for the regulariser: column 0 of the n rows is R's, the others dR's; the divisor M = N - the drop counters
// is taken from the device (the vote kernel is complete: it precedes this launch on the stream).  out = (R, M, dR...): the
// columns a call without the gradient does not have keep the zero kernel's 0.0, and M = 0 gives 0.0 throughout.
__global__ __launch_bounds__(CM_BLOCK) void cmax_reg_upper_kernel(const double* __restrict__ partials, int64_t n, int cols, int64_t N,
                                                                  const unsigned long long* __restrict__ dropped, int n_dropped,
                                                                  double* __restrict__ out) {
    __shared__ double s_red[CM_BLOCK];
    unsigned long long M = (unsigned long long)N;
    for (int j = 0; j < n_dropped; ++j) M -= dropped[j];
    for (int c = 0; c < cols; ++c) {
        double acc = 0.0;
        for (int64_t base = 0; base < n; base += CM_BLOCK) {
            const int64_t i = base + threadIdx.x;
            acc += cm_block_sum(s_red, i < n ? partials[i * cols + c] : 0.0);
        }
        if (threadIdx.x == 0) out[c == 0 ? 0 : 1 + c] = M ? acc / (double)M : 0.0;
    }
    if (threadIdx.x == 0) out[1] = (double)M;
}

int64_t cm_blocks(int64_t n) { return (n + CM_BLOCK - 1) / CM_BLOCK; }

int cm_sizes(int32_t H, int32_t W, int64_t N) {
    if (N < 0 || H <= 0 || W <= 0) return ENSLAM_EINVAL;
    if (N > CM_MAX_EVENTS || H > 65536 || W > 65536 || (int64_t)H * W > CM_MAX_PIXELS) return ENSLAM_EUNSUPPORTED;
    return ENSLAM_OK;
}

// three float64 images (J or D, the row pass, J - mu) and the partials of the widest first level: `cols` per workgroup of
// events, P for the gather and 1 + P for the regulariser's pass
int64_t cm_workspace_bytes(int32_t H, int32_t W, int64_t N, int32_t cols) {
    const int64_t npix = (int64_t)H * W, a = cm_blocks(npix), b = cm_blocks(N) * cols;
    return (3 * npix + (a > b ? a : b)) * (int64_t)sizeof(double);
}

bool cm_finite(double v) { return std::isfinite(v); }

// the launches that depend on the model
void cm_vote(int model, const CmStream& S, unsigned blocks, int64_t* iwe, uint64_t* dropped, hipStream_t st) {
    unsigned long long* I = reinterpret_cast<unsigned long long*>(iwe);
    unsigned long long* X = reinterpret_cast<unsigned long long*>(dropped);
    if (model == ENSLAM_CMAX_FLOW) cmax_vote_kernel<ENSLAM_CMAX_FLOW><<<blocks, CM_BLOCK, 0, st>>>(S, I, X);
    else if (model == ENSLAM_CMAX_ROTATION) cmax_vote_kernel<ENSLAM_CMAX_ROTATION><<<blocks, CM_BLOCK, 0, st>>>(S, I, X);
    else cmax_vote_kernel<CM_RIGID><<<blocks, CM_BLOCK, 0, st>>>(S, I, X);
}

void cm_gather(int model, const CmStream& S, unsigned blocks, const double* D, double* partials, hipStream_t st) {
    if (model == ENSLAM_CMAX_FLOW) cmax_gather_kernel<ENSLAM_CMAX_FLOW><<<blocks, CM_BLOCK, 0, st>>>(S, D, partials);
    else if (model == ENSLAM_CMAX_ROTATION) cmax_gather_kernel<ENSLAM_CMAX_ROTATION><<<blocks, CM_BLOCK, 0, st>>>(S, D, partials);
    else cmax_gather_kernel<CM_RIGID><<<blocks, CM_BLOCK, 0, st>>>(S, D, partials);
}

void cm_reg(int model, bool grad, const CmStream& S, unsigned blocks, int kind, double* partials, hipStream_t st) {
    if (model == ENSLAM_CMAX_ROTATION) {
        if (grad) cmax_reg_kernel<ENSLAM_CMAX_ROTATION, true><<<blocks, CM_BLOCK, 0, st>>>(S, kind, partials);
        else cmax_reg_kernel<ENSLAM_CMAX_ROTATION, false><<<blocks, CM_BLOCK, 0, st>>>(S, kind, partials);
    } else {
        if (grad) cmax_reg_kernel<CM_RIGID, true><<<blocks, CM_BLOCK, 0, st>>>(S, kind, partials);
        else cmax_reg_kernel<CM_RIGID, false><<<blocks, CM_BLOCK, 0, st>>>(S, kind, partials);
    }
}

enum CmEntry { CM_ENTRY_PAIR, CM_ENTRY_RIGID, CM_ENTRY_REG };

// The one validating body of the three *_eval entries.  CM_ENTRY_PAIR: model is the caller's ENSLAM_CMAX_FLOW or
// ENSLAM_CMAX_ROTATION and depth is not looked at.  CM_ENTRY_RIGID: the model is CM_RIGID whatever `model` says, depth is its
// image and dropped has four counters.  CM_ENTRY_REG: any of the three models, depth NULL unless rigid, and reg_kind /
// reg_stats, which the other two pass as ENSLAM_CMAX_REG_NONE / nullptr.
int cm_eval(CmEntry entry, int32_t reg_kind, double* reg_stats, const double* t, const uint16_t* x, const uint16_t* y, const uint8_t* p, int64_t N, int32_t H, int32_t W,
            double fx, double fy, double cx, double cy, int32_t model, const float* depth, const double* theta_host, double t_ref,
            int32_t sign_votes, int32_t k, const double* taps_host, void* workspace, int64_t workspace_bytes, int64_t* iwe,
            double* blurred, double* stats, uint64_t* dropped, int32_t want_grad, void* stream) {
    const bool reg = entry == CM_ENTRY_REG;
    if (!theta_host || !taps_host || !workspace || !iwe || !stats || !dropped || (reg && !reg_stats)) return ENSLAM_EINVAL;
    if (entry == CM_ENTRY_RIGID) model = CM_RIGID;
    else if (model != ENSLAM_CMAX_FLOW && model != ENSLAM_CMAX_ROTATION && !(reg && model == CM_RIGID)) return ENSLAM_EINVAL;
    const bool rigid = model == CM_RIGID;
    if (N > 0 && (!t || !x || !y || !p || (rigid && !depth))) return ENSLAM_EINVAL;
    if (reg && ((!rigid && depth) || (reg_kind != ENSLAM_CMAX_REG_NONE && reg_kind != ENSLAM_CMAX_REG_DIVERGENCE &&
                                      reg_kind != ENSLAM_CMAX_REG_DEFORMATION)))
        return ENSLAM_EINVAL;
    if (k <= 0 || k % 2 == 0) return ENSLAM_EINVAL;
    int rc = cm_sizes(H, W, N);
    if (rc == ENSLAM_EINVAL) return rc;
    const int P = cm_params(model);
    if (!cm_finite(fx) || !cm_finite(fy) || !cm_finite(cx) || !cm_finite(cy) || !cm_finite(t_ref) || fx == 0.0 || fy == 0.0)
        return ENSLAM_EINVAL;
    for (int i = 0; i < P; ++i)
        if (!cm_finite(theta_host[i])) return ENSLAM_EINVAL;
    if (rc != ENSLAM_OK) return rc;
    if (k > CM_KMAX) return ENSLAM_EUNSUPPORTED;
    for (int i = 0; i < k; ++i)
        if (!cm_finite(taps_host[i])) return ENSLAM_EINVAL;
    if (workspace_bytes < cm_workspace_bytes(H, W, N, reg ? 1 + P : P) || ((uintptr_t)workspace & 7u)) return ENSLAM_EINVAL;
    if (((uintptr_t)iwe & 7u) || ((uintptr_t)blurred & 7u) || ((uintptr_t)stats & 7u) || ((uintptr_t)dropped & 7u) ||
        ((uintptr_t)reg_stats & 7u))
        return ENSLAM_EINVAL;

    const int64_t npix = (int64_t)H * W, pix_blocks = cm_blocks(npix), ev_blocks = cm_blocks(N);
    double* bufA = (double*)workspace;                      // J when the caller wants none, then D
    double* bufR = bufA + npix;                             // the row pass
    double* bufC = bufR + npix;                             // J - mu
    double* partials = bufC + npix;
    double* J = blurred ? blurred : bufA;
    hipStream_t st = (hipStream_t)stream;

    CmStream S;
    S.t = t; S.x = x; S.y = y; S.p = p; S.depth = rigid ? depth : nullptr; S.N = N; S.H = H; S.W = W; S.model = model; S.sign_votes = sign_votes;
    S.fx = fx; S.fy = fy; S.cx = cx; S.cy = cy; S.t_ref = t_ref;
    for (int i = 0; i < CM_PMAX; ++i) S.theta[i] = i < P ? theta_host[i] : 0.0;
    CmBlur B;
    B.H = H; B.W = W; B.k = k;
    for (int i = 0; i < CM_KMAX; ++i) B.taps[i] = i < k ? taps_host[i] : 0.0;

    cmax_zero_kernel<<<(unsigned)pix_blocks, CM_BLOCK, 0, st>>>(reinterpret_cast<long long*>(iwe), npix,
                                                                 reinterpret_cast<unsigned long long*>(dropped), rigid ? 4 : 3, stats, 2 + P,
                                                                 reg_stats, reg ? 2 + P : 0);
    if (N > 0) cm_vote(model, S, (unsigned)ev_blocks, iwe, dropped, st);
    cmax_rows_kernel<long long><<<(unsigned)pix_blocks, CM_BLOCK, 0, st>>>(B, reinterpret_cast<const long long*>(iwe), bufR);
    cmax_cols_kernel<true><<<(unsigned)pix_blocks, CM_BLOCK, 0, st>>>(B, bufR, J, partials);
    cmax_upper_kernel<<<1, CM_BLOCK, 0, st>>>(partials, pix_blocks, 1, (double)npix, 0, stats);
    cmax_centre_kernel<<<(unsigned)pix_blocks, CM_BLOCK, 0, st>>>(J, stats, npix, bufC, partials);
    cmax_upper_kernel<<<1, CM_BLOCK, 0, st>>>(partials, pix_blocks, 1, (double)npix, 0, stats + 1);
    if (want_grad) {
        cmax_rows_kernel<double><<<(unsigned)pix_blocks, CM_BLOCK, 0, st>>>(B, bufC, bufR);
        cmax_cols_kernel<false><<<(unsigned)pix_blocks, CM_BLOCK, 0, st>>>(B, bufR, bufA, nullptr);
        if (N > 0) cm_gather(model, S, (unsigned)ev_blocks, bufA, partials, st);
        cmax_upper_kernel<<<1, CM_BLOCK, 0, st>>>(partials, ev_blocks, P, 2.0 / (double)npix, 1, stats + 2);
    }
    if (reg && reg_kind != ENSLAM_CMAX_REG_NONE) {
        // after the last reader of `partials`; flow launches no pass: no partials, R = 0.0 exactly, M still reported
        const bool pass = N > 0 && model != ENSLAM_CMAX_FLOW;
        const int cols = want_grad ? 1 + P : 1;
        if (pass) cm_reg(model, want_grad != 0, S, (unsigned)ev_blocks, reg_kind, partials, st);
        cmax_reg_upper_kernel<<<1, CM_BLOCK, 0, st>>>(partials, pass ? ev_blocks : 0, cols, N,
                                                      reinterpret_cast<const unsigned long long*>(dropped), rigid ? 4 : 3, reg_stats);
    }
    return hipGetLastError() == hipSuccess ? ENSLAM_OK : ENSLAM_ELAUNCH;
}

}  // namespace

extern "C" {

int enslam_event_cmax_workspace(int32_t H, int32_t W, int64_t N, int32_t P, int64_t* bytes_host) {
    if (!bytes_host || P < 2 || P > 3) return ENSLAM_EINVAL;
    const int rc = cm_sizes(H, W, N);
    if (rc != ENSLAM_OK) return rc;
    *bytes_host = cm_workspace_bytes(H, W, N, P);
    return ENSLAM_OK;
}

int enslam_event_cmax_rigid_workspace(int32_t H, int32_t W, int64_t N, int64_t* bytes_host) {
    if (!bytes_host) return ENSLAM_EINVAL;
    const int rc = cm_sizes(H, W, N);
    if (rc != ENSLAM_OK) return rc;
    *bytes_host = cm_workspace_bytes(H, W, N, cm_params(CM_RIGID));
    return ENSLAM_OK;
}

int enslam_event_cmax_eval(const double* t, const uint16_t* x, const uint16_t* y, const uint8_t* p, int64_t N, int32_t H, int32_t W,
                           double fx, double fy, double cx, double cy, int32_t model, const double* theta_host, double t_ref,
                           int32_t sign_votes, int32_t k, const double* taps_host, void* workspace, int64_t workspace_bytes,
                           int64_t* iwe, double* blurred, double* stats, uint64_t* dropped, int32_t want_grad, void* stream) {
    return cm_eval(CM_ENTRY_PAIR, ENSLAM_CMAX_REG_NONE, nullptr, t, x, y, p, N, H, W, fx, fy, cx, cy, model, nullptr, theta_host, t_ref, sign_votes, k, taps_host, workspace,
                   workspace_bytes, iwe, blurred, stats, dropped, want_grad, stream);
}

int enslam_event_cmax_rigid_eval(const double* t, const uint16_t* x, const uint16_t* y, const uint8_t* p, int64_t N, int32_t H,
                                 int32_t W, double fx, double fy, double cx, double cy, const float* depth, const double* theta_host,
                                 double t_ref, int32_t sign_votes, int32_t k, const double* taps_host, void* workspace,
                                 int64_t workspace_bytes, int64_t* iwe, double* blurred, double* stats, uint64_t* dropped,
                                 int32_t want_grad, void* stream) {
    return cm_eval(CM_ENTRY_RIGID, ENSLAM_CMAX_REG_NONE, nullptr, t, x, y, p, N, H, W, fx, fy, cx, cy, 0, depth, theta_host, t_ref, sign_votes, k, taps_host, workspace,
                   workspace_bytes, iwe, blurred, stats, dropped, want_grad, stream);
}

int enslam_event_cmax_reg_workspace(int32_t H, int32_t W, int64_t N, int32_t model, int64_t* bytes_host) {
    if (!bytes_host || (model != ENSLAM_CMAX_FLOW && model != ENSLAM_CMAX_ROTATION && model != ENSLAM_CMAX_RIGID)) return ENSLAM_EINVAL;
    const int rc = cm_sizes(H, W, N);
    if (rc != ENSLAM_OK) return rc;
    *bytes_host = cm_workspace_bytes(H, W, N, 1 + cm_params(model));
    return ENSLAM_OK;
}

int enslam_event_cmax_reg_eval(const double* t, const uint16_t* x, const uint16_t* y, const uint8_t* p, int64_t N, int32_t H, int32_t W,
                               double fx, double fy, double cx, double cy, int32_t model, const float* depth, const double* theta_host,
                               double t_ref, int32_t sign_votes, int32_t k, const double* taps_host, void* workspace,
                               int64_t workspace_bytes, int64_t* iwe, double* blurred, double* stats, uint64_t* dropped,
                               int32_t reg_kind, double* reg_stats, int32_t want_grad, void* stream) {
    return cm_eval(CM_ENTRY_REG, reg_kind, reg_stats, t, x, y, p, N, H, W, fx, fy, cx, cy, model, depth, theta_host, t_ref, sign_votes, k,
                   taps_host, workspace, workspace_bytes, iwe, blurred, stats, dropped, want_grad, stream);
}

}  // extern "C"
