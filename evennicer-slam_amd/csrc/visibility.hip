// Visibility of points in a set of cameras: the projection loop shared by Mesher.point_masks (Mesher.py:53-211, float32)
// and Mapper.keyframe_selection_overlap (Mapper.py:218-241, float64), one thread per point, the cameras read as
// wave-uniform data.
//
//   max    (depth test only) per camera the largest bilinear depth sample over ALL points of the call, the reference's
//          torch.max(depth_sample): wave maximum, then one atomic max per wave and camera on an order-preserving key
//   mask   per point the class (0 unseen, 1 seen, 2 forecast) and per camera the count of points that pass its seen test
//
// Integer adds and a maximum do not depend on the launch order, so the outputs are deterministic to the bit.  The
// arithmetic follows the reference's statements one by one in T (the Makefile's -ffp-contract=off keeps them unfused).
#include "../../include/enslam_hip.h"
#include "common.hpp"

namespace {

constexpr int VIS_BLOCK = 256;

template <typename T>
struct VisArgs {
    int64_t n;                      // points of this call
    const float* points;            // [n,3] or NULL: lattice
    const float *ax, *ay, *az;      // lattice axes
    int64_t first, syz;             // first linear lattice index of the call; ny * nz
    int32_t nz, ny;
    int32_t K;
    const T* w2c;                   // [K,12]: the upper three rows of the world-to-camera matrix
    T fx, fy, cx, cy, z_eps;
    float u_lo[2], u_hi[2], v_hi[2];    // edge, W - edge, H - edge for {seen, forecast}
    int32_t H, W;
    const float* limit;             // [K] or NULL
    const float* depth;             // [K,H,W] or NULL
    uint32_t* max_key;              // [K] (depth test)
    uint8_t* classes;               // [n] or NULL
    int32_t* counts;                // [K] or NULL
};

// order-preserving map of a float onto uint32 (larger float <=> larger key; a NaN with the sign bit clear tops +inf, so a
// NaN sample makes the maximum NaN as torch.max does); key 0 is below every float
ENS_DEV uint32_t vis_key(float f) {
    const uint32_t b = __float_as_uint(f);
    return b & 0x80000000u ? ~b : b | 0x80000000u;
}
ENS_DEV float vis_unkey(uint32_t k) { return __uint_as_float(k & 0x80000000u ? k & 0x7fffffffu : ~k); }

template <typename T>
ENS_DEV bool vis_point(const VisArgs<T>& a, int64_t i, T& x, T& y, T& z) {
    if (i >= a.n) return false;
    if (a.points) {
        x = (T)a.points[3 * i];
        y = (T)a.points[3 * i + 1];
        z = (T)a.points[3 * i + 2];
    } else {                                            // Mesher.lattice_volume's order: x slowest, z fastest
        const int64_t lin = a.first + i;
        x = (T)a.ax[lin / a.syz];
        y = (T)a.ay[(lin / a.nz) % a.ny];
        z = (T)a.az[lin % a.nz];
    }
    return true;
}

template <typename T>
struct VisProj {
    float u, v;                     // the reference compares uv as float32 in both paths
    T z, pd;                        // uvz.z + z_eps, and -cam.z (the projected depth)
};

// cam = w2c[:3,:3] p + w2c[:3,3]; cam.x *= -1; uvz = K cam; z = uvz.z + z_eps; uv = uvz.xy / z
template <typename T>
ENS_DEV VisProj<T> vis_project(const VisArgs<T>& a, const T* __restrict__ m, T x, T y, T z) {
    T c0 = m[0] * x + m[1] * y + m[2] * z + m[3];
    const T c1 = m[4] * x + m[5] * y + m[6] * z + m[7];
    const T c2 = m[8] * x + m[9] * y + m[10] * z + m[11];
    c0 = -c0;
    VisProj<T> p;
    p.z = c2 + a.z_eps;
    p.u = (float)((a.fx * c0 + a.cx * c2) / p.z);
    p.v = (float)((a.fy * c1 + a.cy * c2) / p.z);
    p.pd = -c2;
    return p;
}

// F.grid_sample(depth[k], (u / (W-1) * 2 - 1, v / (H-1) * 2 - 1), bilinear, padding_mode='zeros', align_corners=True):
// float32 throughout, corners outside the image (and NaN coordinates) contribute zero
ENS_DEV float vis_sample(const float* __restrict__ img, int H, int W, float u, float v) {
    const float gx = u / (float)(W - 1) * 2.0f - 1.0f, gy = v / (float)(H - 1) * 2.0f - 1.0f;
    const float ix = ((gx + 1.0f) / 2.0f) * (float)(W - 1), iy = ((gy + 1.0f) / 2.0f) * (float)(H - 1);
    const float x0 = floorf(ix), y0 = floorf(iy), x1 = x0 + 1.0f, y1 = y0 + 1.0f;
    const bool bx0 = x0 >= 0.0f && x0 <= (float)(W - 1), bx1 = x1 >= 0.0f && x1 <= (float)(W - 1);
    const bool by0 = y0 >= 0.0f && y0 <= (float)(H - 1), by1 = y1 >= 0.0f && y1 <= (float)(H - 1);
    const int jx0 = bx0 ? (int)x0 : 0, jx1 = bx1 ? (int)x1 : 0, jy0 = by0 ? (int)y0 : 0, jy1 = by1 ? (int)y1 : 0;
    float out = 0.0f;
    if (bx0 && by0) out += img[(int64_t)jy0 * W + jx0] * ((x1 - ix) * (y1 - iy));
    if (bx1 && by0) out += img[(int64_t)jy0 * W + jx1] * ((ix - x0) * (y1 - iy));
    if (bx0 && by1) out += img[(int64_t)jy1 * W + jx0] * ((x1 - ix) * (iy - y0));
    if (bx1 && by1) out += img[(int64_t)jy1 * W + jx1] * ((ix - x0) * (iy - y0));
    return out;
}

ENS_DEV uint32_t wave_max_u32(uint32_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const uint32_t w = (uint32_t)__shfl_xor((int)v, o, 64);
        v = w > v ? w : v;
    }
    return v;
}

template <typename T>
__global__ __launch_bounds__(VIS_BLOCK) void vis_max_kernel(VisArgs<T> a) {
    const int64_t i = (int64_t)blockIdx.x * VIS_BLOCK + threadIdx.x;
    T x = 0, y = 0, z = 0;
    const bool live = vis_point(a, i, x, y, z);
    const int64_t hw = (int64_t)a.H * a.W;
    for (int k = 0; k < a.K; ++k) {
        uint32_t key = 0;
        if (live) {
            const VisProj<T> p = vis_project(a, a.w2c + 12 * (int64_t)k, x, y, z);
            key = vis_key(vis_sample(a.depth + k * hw, a.H, a.W, p.u, p.v));
        }
        key = wave_max_u32(key);
        // most waves cannot raise the maximum: a plain read first keeps them off the atomic (a stale read only costs a
        // redundant atomic, never a wrong maximum)
        if ((threadIdx.x & 63) == 0 && key > a.max_key[k]) atomicMax(a.max_key + k, key);
    }
}

template <typename T>
__global__ __launch_bounds__(VIS_BLOCK) void vis_mask_kernel(VisArgs<T> a) {
    const int64_t i = (int64_t)blockIdx.x * VIS_BLOCK + threadIdx.x;
    T x = 0, y = 0, z = 0;
    const bool live = vis_point(a, i, x, y, z);
    const int64_t hw = (int64_t)a.H * a.W;
    bool seen = false, fore = false;
    for (int k = 0; k < a.K; ++k) {
        // forecast excludes seen: a wave whose lanes are all seen has nothing more to learn (the counts need every camera)
        if (!a.counts && __ballot(live && !seen) == 0) break;
        bool s = false;
        if (live) {
            const VisProj<T> p = vis_project(a, a.w2c + 12 * (int64_t)k, x, y, z);
            const bool front = p.z < (T)0;
            s = front && p.u < a.u_hi[0] && p.u > a.u_lo[0] && p.v < a.v_hi[0] && p.v > a.u_lo[0];
            bool f = front && p.u < a.u_hi[1] && p.u > a.u_lo[1] && p.v < a.v_hi[1] && p.v > a.u_lo[1];
            if (a.limit) {
                const bool near = p.pd < (T)a.limit[k];
                s = s && near;
                f = f && near;
            }
            if (a.depth) {
                const T d = (T)vis_sample(a.depth + k * hw, a.H, a.W, p.u, p.v);
                s = s && p.pd < d + (T)2.4 && d - (T)2.4 < p.pd;
                f = f && p.pd < (T)vis_unkey(a.max_key[k]);
            }
            seen = seen || s;
            fore = fore || f;
        }
        if (a.counts) {
            const uint64_t b = __ballot(s);
            if ((threadIdx.x & 63) == 0 && b) atomicAdd(a.counts + k, (int)__popcll(b));
        }
    }
    if (live && a.classes) a.classes[i] = seen ? 1 : fore ? 2 : 0;
}

int64_t vis_ws_bytes(int32_t K) { return (4 * (int64_t)(K > 0 ? K : 1) + 255) & ~(int64_t)255; }

template <typename T>
int vis_launch(VisArgs<T> a, const void* w2c, double fx, double fy, double cx, double cy, double z_eps, void* workspace,
               hipStream_t s) {
    a.w2c = (const T*)w2c;
    a.fx = (T)fx;
    a.fy = (T)fy;
    a.cx = (T)cx;
    a.cy = (T)cy;
    a.z_eps = (T)z_eps;
    const unsigned blocks = (unsigned)((a.n + VIS_BLOCK - 1) / VIS_BLOCK);
    if (a.depth) {
        a.max_key = (uint32_t*)workspace;
        if (hipMemsetAsync(workspace, 0, 4 * (size_t)a.K, s) != hipSuccess) return ENSLAM_ELAUNCH;
        vis_max_kernel<T><<<blocks, VIS_BLOCK, 0, s>>>(a);
    }
    vis_mask_kernel<T><<<blocks, VIS_BLOCK, 0, s>>>(a);
    return hipGetLastError() == hipSuccess ? ENSLAM_OK : ENSLAM_ELAUNCH;
}

bool vis_finite(double x) { return x == x && x - x == 0.0; }

}  // namespace

extern "C" {

int enslam_visibility_workspace(int32_t n_cams, int64_t* bytes_host) {
    if (n_cams < 0 || !bytes_host) return ENSLAM_EINVAL;
    *bytes_host = vis_ws_bytes(n_cams);
    return ENSLAM_OK;
}

int enslam_visibility(int32_t real64, int64_t n_points, const float* points, const float* ax, const float* ay,
                      const float* az, int32_t nx, int32_t ny, int32_t nz, int64_t lattice_first, int32_t n_cams,
                      const void* w2c, double fx, double fy, double cx, double cy, int32_t H, int32_t W, int32_t edge_seen,
                      int32_t edge_forecast, double z_eps, const float* limit, const float* depth, void* workspace,
                      uint8_t* classes, int32_t* counts, void* stream) {
    if ((real64 != 0 && real64 != 1) || n_points < 0 || n_cams < 0 || H <= 0 || W <= 0) return ENSLAM_EINVAL;
    if (!vis_finite(fx) || !vis_finite(fy) || !vis_finite(cx) || !vis_finite(cy) || !vis_finite(z_eps)) return ENSLAM_EINVAL;
    if (n_cams > 0 && !w2c) return ENSLAM_EINVAL;
    if (depth && (!workspace || H < 2 || W < 2)) return ENSLAM_EINVAL;
    if (n_points > 0 && !points) {
        if (!ax || !ay || !az || nx <= 0 || ny <= 0 || nz <= 0 || lattice_first < 0) return ENSLAM_EINVAL;
        if (lattice_first + n_points > (int64_t)nx * ny * nz) return ENSLAM_EINVAL;
    }
    if ((n_points + VIS_BLOCK - 1) / VIS_BLOCK > INT32_MAX) return ENSLAM_EUNSUPPORTED;
    hipStream_t s = (hipStream_t)stream;
    if (counts && n_cams > 0 && hipMemsetAsync(counts, 0, 4 * (size_t)n_cams, s) != hipSuccess) return ENSLAM_ELAUNCH;
    if (n_points == 0) return ENSLAM_OK;
    if (n_cams == 0) {                                  // no camera sees anything
        if (classes && hipMemsetAsync(classes, 0, (size_t)n_points, s) != hipSuccess) return ENSLAM_ELAUNCH;
        return ENSLAM_OK;
    }
    if (!classes && !counts) return ENSLAM_OK;
    const float es[2] = {(float)edge_seen, (float)edge_forecast};
    const float wh[2] = {(float)(W - edge_seen), (float)(W - edge_forecast)};
    const float hh[2] = {(float)(H - edge_seen), (float)(H - edge_forecast)};
    if (real64) {
        VisArgs<double> a = {n_points, points, ax, ay, az, lattice_first, (int64_t)ny * nz, nz, ny, n_cams, nullptr, 0, 0, 0, 0, 0,
                             {es[0], es[1]}, {wh[0], wh[1]}, {hh[0], hh[1]}, H, W, limit, depth, nullptr, classes, counts};
        return vis_launch<double>(a, w2c, fx, fy, cx, cy, z_eps, workspace, s);
    }
    VisArgs<float> a = {n_points, points, ax, ay, az, lattice_first, (int64_t)ny * nz, nz, ny, n_cams, nullptr, 0, 0, 0, 0, 0,
                        {es[0], es[1]}, {wh[0], wh[1]}, {hh[0], hh[1]}, H, W, limit, depth, nullptr, classes, counts};
    return vis_launch<float>(a, w2c, fx, fy, cx, cy, z_eps, workspace, s);
}

}  // extern "C"
