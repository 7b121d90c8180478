// The triangle rasteriser of mesh_depth.hip (depth images) and scene_raster.hip (the visibility buffer), held once: the two
// differ only in what a covered pixel receives and in culling, which a Sink supplies.
//
// The camera looks down -z; pixel (row j, column i) sees the direction d = ((i - cx) / fx, -(j - cy) / fy, -1).  With a, b, c
// the vertices in camera space (cam = w2c p), n0 = b x c, n1 = c x a, n2 = a x b and det = a . n0, d meets the triangle's
// plane at  t d = (s0 a + s1 b + s2 c) t / det,  s_i = d . n_i: inside iff s0, s1, s2 share a sign (zeros count), and then
// t = det / (s0 + s1 + s2), kept when z_near < t <= z_far.  The form is homogeneous: a triangle that crosses the camera
// plane needs no clipping, and a hit behind the camera has t < 0.  Degenerate triangles hit nothing.  Everything is float64
// up to the rounding of t to float32, and every expression keeps its order and parentheses: the bits are the contract
// (tests/recon_edge_cases.py).
//
//   small   one thread per (triangle, view): the pixel box from the projected vertices (the whole image when a vertex is
//           at or behind the camera plane); a box of at most TRI_SMALL pixels is rasterised by the thread, a larger one is
//           appended to a list (when the list is full the thread rasterises it after all)
//   large   a workgroup per listed (triangle, view), grid-stride over the list: 256 threads share the box
//
// A Sink is a small struct passed by value with
//   static constexpr bool CULLS   and, when it is true, a member  cull:  1 keeps det > 0, 2 keeps det < 0, 0 both
//   void put(int k, int j, int i, uint32_t depth_bits, uint32_t face) const   the float32 bit pattern of t at a covered pixel
#pragma once
#include "../../include/enslam_hip.h"
#include "common.hpp"

namespace {

constexpr int TRI_BLOCK = 256;
constexpr int TRI_SMALL = 256;                          // pixels a single thread rasterises
constexpr int TRI_LARGE_GRID = 2048;
constexpr int64_t TRI_LIST_CAP = (int64_t)1 << 22;      // listed (triangle, view) pairs: 32 MB

struct TriArgs {
    const double* verts;
    const int32_t* faces;
    const double* w2c;              // [K,12]
    int64_t F;
    int32_t V, K, H, W;
    double fx, fy, cx, cy, z_near, z_far;
    int32_t* list_count;
    int64_t* list;                  // [list_cap] entries  view * F + triangle
    int64_t list_cap;
};

struct TriSetup {
    double n0[3], n1[3], n2[3], det;
    int i0, i1, j0, j1;             // inclusive pixel box
};

ENS_DEV void tri_cross(const double* a, const double* b, double* o) {
    o[0] = a[1] * b[2] - a[2] * b[1];
    o[1] = a[2] * b[0] - a[0] * b[2];
    o[2] = a[0] * b[1] - a[1] * b[0];
}

// floor / ceil of a pixel coordinate clamped into [-1, n] first (the value may be huge)
ENS_DEV int tri_pix(double x, int n) { return (int)(x < -1.0 ? -1.0 : (x > (double)n ? (double)n : x)); }

// camera-space vertices of face f in view k; false for an index outside [0, V)
ENS_DEV bool tri_face(const TriArgs& A, int64_t f, int k, int (&vi)[3], double (&p)[3][3]) {
    vi[0] = A.faces[3 * f]; vi[1] = A.faces[3 * f + 1]; vi[2] = A.faces[3 * f + 2];
    if ((uint32_t)vi[0] >= (uint32_t)A.V || (uint32_t)vi[1] >= (uint32_t)A.V || (uint32_t)vi[2] >= (uint32_t)A.V) return false;
    const double* m = A.w2c + 12 * (int64_t)k;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const double* w = A.verts + 3 * (int64_t)vi[j];
        const double x = w[0], y = w[1], z = w[2];
#pragma unroll
        for (int r = 0; r < 3; ++r) p[j][r] = ((m[4 * r] * x + m[4 * r + 1] * y) + m[4 * r + 2] * z) + m[4 * r + 3];
    }
    return true;
}

// The edge normals and the pixel box of triangle f in view k.  Returns false when the triangle cannot be hit or is culled.
template <class Sink>
ENS_DEV bool tri_setup(const TriArgs& A, const Sink& S, int64_t f, int k, TriSetup& T) {
    int vi[3];
    double p[3][3];
    if (!tri_face(A, f, k, vi, p)) return false;
    tri_cross(p[1], p[2], T.n0);
    tri_cross(p[2], p[0], T.n1);
    tri_cross(p[0], p[1], T.n2);
    T.det = (p[0][0] * T.n0[0] + p[0][1] * T.n0[1]) + p[0][2] * T.n0[2];
    // the triangle's normal (b - a) x (c - a) = n0 + n1 + n2: zero for a repeated vertex (n1 = -n0 and n2 = 0 to the bit)
    const double nx = T.n0[0] + T.n1[0] + T.n2[0], ny = T.n0[1] + T.n1[1] + T.n2[1], nz = T.n0[2] + T.n1[2] + T.n2[2];
    if ((nx == 0.0 && ny == 0.0 && nz == 0.0) || !(T.det != 0.0) || !(T.det - T.det == 0.0)) return false;
    if constexpr (Sink::CULLS)
        if ((S.cull == 1 && !(T.det > 0.0)) || (S.cull == 2 && !(T.det < 0.0))) return false;
    const double za = -p[0][2], zb = -p[1][2], zc = -p[2][2];          // depths
    const double zmin = fmin(za, fmin(zb, zc)), zmax = fmax(za, fmax(zb, zc));
    if (!(zmax > A.z_near) || !(zmin <= A.z_far)) return false;         // every hit has its depth in [zmin, zmax]
    T.i0 = 0; T.i1 = A.W - 1; T.j0 = 0; T.j1 = A.H - 1;
    if (zmin > 0.0) {                                   // all in front: the projection of the triangle is inside the box
        double u0 = __builtin_huge_val(), u1 = -u0, w0 = u0, w1 = -u0;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const double u = A.cx + A.fx * (p[j][0] / -p[j][2]), w = A.cy - A.fy * (p[j][1] / -p[j][2]);
            u0 = fmin(u0, u); u1 = fmax(u1, u);
            w0 = fmin(w0, w); w1 = fmax(w1, w);
        }
        // one thousandth of a pixel covers the rounding of the projection
        const int i0 = tri_pix(floor(u0 - 1e-3), A.W), i1 = tri_pix(ceil(u1 + 1e-3), A.W);
        const int j0 = tri_pix(floor(w0 - 1e-3), A.H), j1 = tri_pix(ceil(w1 + 1e-3), A.H);
        T.i0 = i0 < 0 ? 0 : i0; T.i1 = i1 > A.W - 1 ? A.W - 1 : i1;
        T.j0 = j0 < 0 ? 0 : j0; T.j1 = j1 > A.H - 1 ? A.H - 1 : j1;
        if (T.i0 > T.i1 || T.j0 > T.j1) return false;
    }
    return true;
}

// whether the ray of pixel (j, i) hits the triangle, and then its depth t
ENS_DEV bool tri_cover(const TriArgs& A, const TriSetup& T, int j, int i, double& t) {
    const double dx = ((double)i - A.cx) / A.fx, dy = -((double)j - A.cy) / A.fy;
    const double s0 = (dx * T.n0[0] + dy * T.n0[1]) - T.n0[2];
    const double s1 = (dx * T.n1[0] + dy * T.n1[1]) - T.n1[2];
    const double s2 = (dx * T.n2[0] + dy * T.n2[1]) - T.n2[2];
    const bool inside = (s0 >= 0.0 && s1 >= 0.0 && s2 >= 0.0) || (s0 <= 0.0 && s1 <= 0.0 && s2 <= 0.0);
    const double S = (s0 + s1) + s2;
    if (!inside || S == 0.0) return false;
    t = T.det / S;
    return t > A.z_near && t <= A.z_far;
}

template <class Sink>
ENS_DEV void tri_pixel(const TriArgs& A, const Sink& S, const TriSetup& T, uint32_t f, int k, int j, int i) {
    double t;
    if (tri_cover(A, T, j, i, t)) S.put(k, j, i, __float_as_uint((float)t), f);
}

template <class Sink>
__global__ __launch_bounds__(TRI_BLOCK) void tri_small_kernel(TriArgs A, Sink S) {
    const int64_t e = (int64_t)blockIdx.x * TRI_BLOCK + threadIdx.x;
    if (e >= A.F * A.K) return;
    const int k = (int)(e / A.F);
    const int64_t f = e - (int64_t)k * A.F;
    TriSetup T;
    if (!tri_setup(A, S, f, k, T)) return;
    const int64_t box = (int64_t)(T.i1 - T.i0 + 1) * (T.j1 - T.j0 + 1);
    if (box > TRI_SMALL) {
        const int64_t slot = atomicAdd(A.list_count, 1);
        if (slot < A.list_cap) {
            A.list[slot] = e;
            return;
        }
    }
    for (int j = T.j0; j <= T.j1; ++j)
        for (int i = T.i0; i <= T.i1; ++i) tri_pixel(A, S, T, (uint32_t)f, k, j, i);
}

template <class Sink>
__global__ __launch_bounds__(TRI_BLOCK) void tri_large_kernel(TriArgs A, Sink S) {
    int64_t count = *A.list_count;
    count = count < A.list_cap ? count : A.list_cap;
    for (int64_t s = blockIdx.x; s < count; s += gridDim.x) {
        const int64_t e = A.list[s];
        if (e < 0 || e >= A.F * A.K) continue;
        const int k = (int)(e / A.F);
        const int64_t f = e - (int64_t)k * A.F;
        TriSetup T;
        if (!tri_setup(A, S, f, k, T)) continue;
        const int bw = T.i1 - T.i0 + 1;
        const uint32_t box = (uint32_t)bw * (uint32_t)(T.j1 - T.j0 + 1);               // H * W <= 2^31
        for (uint32_t q = threadIdx.x; q < box; q += TRI_BLOCK)
            tri_pixel(A, S, T, (uint32_t)f, k, T.j0 + (int)(q / (uint32_t)bw), T.i0 + (int)(q % (uint32_t)bw));
    }
}

// the small and the large pass over A.F triangles and A.K views, the list counter being zero
template <class Sink>
void tri_launch(const TriArgs& A, const Sink& S, hipStream_t s) {
    tri_small_kernel<<<(unsigned)((A.F * A.K + TRI_BLOCK - 1) / TRI_BLOCK), TRI_BLOCK, 0, s>>>(A, S);
    tri_large_kernel<<<TRI_LARGE_GRID, TRI_BLOCK, 0, s>>>(A, S);
}

bool tri_finite(double x) { return x == x && x - x == 0.0; }

int64_t tri_list_cap(int64_t F, int64_t K) { return F * K < TRI_LIST_CAP ? (F * K < 1 ? 1 : F * K) : TRI_LIST_CAP; }

// the refusals both entries share, in their order: counts and image size, the camera, the depth range
int tri_refuse(int32_t n_verts, int32_t n_faces, int32_t n_points, int32_t n_views, int32_t H, int32_t W, double fx, double fy,
               double cx, double cy, double z_near, double z_far) {
    if (n_verts < 0 || n_faces < 0 || n_points < 0 || n_views < 0 || H <= 0 || W <= 0) return ENSLAM_EINVAL;
    // the list counter is an int32, a box is counted in 32 bits, a point id keeps 31
    if ((int64_t)n_views * H * W > ((int64_t)1 << 31) || (int64_t)n_faces * n_views > INT32_MAX ||
        (int64_t)n_points * n_views > INT32_MAX)
        return ENSLAM_EUNSUPPORTED;
    if (!tri_finite(fx) || !tri_finite(fy) || !tri_finite(cx) || !tri_finite(cy) || fx == 0.0 || fy == 0.0) return ENSLAM_EINVAL;
    if (!tri_finite(z_near) || z_far != z_far || z_near < 0.0 || !(z_far > z_near)) return ENSLAM_EINVAL;
    return ENSLAM_OK;
}

}  // namespace
