// Depth images of a triangle mesh from K cameras (the off-screen depth renders of the reference's
// src/tools/eval_recon.py:131-210): pixel (row j, column i) of view k holds the smallest camera-space depth t in
// (z_near, z_far] at which the ray through ((i - cx) / fx, -(j - cy) / fy, -1) meets a triangle, 0.0 where none does.
// Both sides of a triangle count, edges are inclusive, degenerate triangles hit nothing.  Float64 up to the rounding of t.
//
// With a, b, c the vertices in camera space (cam = w2c p, the camera looks down -z), n0 = b x c, n1 = c x a, n2 = a x b and
// det = a . n0, a ray direction d meets the triangle's plane at  t d = (s0 a + s1 b + s2 c) t / det,  s_i = d . n_i:
// inside iff s0, s1, s2 share a sign (zeros count), and then  t = det / (s0 + s1 + s2).  The form is homogeneous: a
// triangle that crosses the camera plane needs no clipping, and a hit behind the camera has t < 0.
//
//   fill    the images with the bit pattern 0xFFFFFFFF
//   small   one thread per (triangle, view): the pixel box from the projected vertices (the whole image when a vertex is
//           at or behind the camera plane); a box of at most MD_SMALL pixels is rasterised by the thread, a larger one is
//           appended to a list (when the list is full the thread rasterises it after all)
//   large   a workgroup per listed (triangle, view), grid-stride over the list: 256 threads share the box
//   finish  0xFFFFFFFF -> 0.0
// Depths are combined by an unsigned integer minimum on the float32 bit pattern (positive floats order as their bits), so
// the images are the same bits in every run and do not depend on how the views are batched.
#include "../../include/enslam_hip.h"
#include "common.hpp"

namespace {

constexpr int MD_BLOCK = 256;
constexpr int MD_SMALL = 256;                           // pixels a single thread rasterises
constexpr int MD_LARGE_GRID = 2048;
constexpr int64_t MD_LIST_CAP = (int64_t)1 << 22;       // listed (triangle, view) pairs: 32 MB
constexpr uint32_t MD_NONE = 0xFFFFFFFFu;

struct MdArgs {
    const double* verts;
    const int32_t* faces;
    const double* w2c;              // [K,12]
    int64_t F;
    int32_t V, K, H, W;
    double fx, fy, cx, cy, z_near, z_far;
    uint32_t* img;                  // [K,H,W] bit patterns
    int32_t* list_count;
    int64_t* list;                  // [list_cap] entries  view * F + triangle
    int64_t list_cap;
};

struct MdTri {
    double n0[3], n1[3], n2[3], det;
    int i0, i1, j0, j1;             // inclusive pixel box; empty when i0 > i1
};

ENS_DEV void md_cross(const double* a, const double* b, double* o) {
    o[0] = a[1] * b[2] - a[2] * b[1];
    o[1] = a[2] * b[0] - a[0] * b[2];
    o[2] = a[0] * b[1] - a[1] * b[0];
}

// floor / ceil of a pixel coordinate clamped into [-1, n] first (the value may be huge)
ENS_DEV int md_pix(double x, int n) { return (int)(x < -1.0 ? -1.0 : (x > (double)n ? (double)n : x)); }

// The edge normals and the pixel box of triangle f in view k.  Returns false when the triangle cannot be hit.
ENS_DEV bool md_setup(const MdArgs& A, int64_t f, int k, MdTri& T) {
    const int v0 = A.faces[3 * f], v1 = A.faces[3 * f + 1], v2 = A.faces[3 * f + 2];
    if ((uint32_t)v0 >= (uint32_t)A.V || (uint32_t)v1 >= (uint32_t)A.V || (uint32_t)v2 >= (uint32_t)A.V) return false;
    const double* m = A.w2c + 12 * (int64_t)k;
    const int vi[3] = {v0, v1, v2};
    double p[3][3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const double* w = A.verts + 3 * (int64_t)vi[j];
        const double x = w[0], y = w[1], z = w[2];
#pragma unroll
        for (int r = 0; r < 3; ++r) p[j][r] = ((m[4 * r] * x + m[4 * r + 1] * y) + m[4 * r + 2] * z) + m[4 * r + 3];
    }
    md_cross(p[1], p[2], T.n0);
    md_cross(p[2], p[0], T.n1);
    md_cross(p[0], p[1], T.n2);
    T.det = (p[0][0] * T.n0[0] + p[0][1] * T.n0[1]) + p[0][2] * T.n0[2];
    // the triangle's normal (b - a) x (c - a) = n0 + n1 + n2: zero for a repeated vertex (n1 = -n0 and n2 = 0 to the bit)
    const double nx = T.n0[0] + T.n1[0] + T.n2[0], ny = T.n0[1] + T.n1[1] + T.n2[1], nz = T.n0[2] + T.n1[2] + T.n2[2];
    if ((nx == 0.0 && ny == 0.0 && nz == 0.0) || !(T.det != 0.0) || !(T.det - T.det == 0.0)) return false;
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
        const int i0 = md_pix(floor(u0 - 1e-3), A.W), i1 = md_pix(ceil(u1 + 1e-3), A.W);
        const int j0 = md_pix(floor(w0 - 1e-3), A.H), j1 = md_pix(ceil(w1 + 1e-3), A.H);
        T.i0 = i0 < 0 ? 0 : i0; T.i1 = i1 > A.W - 1 ? A.W - 1 : i1;
        T.j0 = j0 < 0 ? 0 : j0; T.j1 = j1 > A.H - 1 ? A.H - 1 : j1;
        if (T.i0 > T.i1 || T.j0 > T.j1) return false;
    }
    return true;
}

ENS_DEV void md_pixel(const MdArgs& A, const MdTri& T, int k, int j, int i) {
    const double dx = ((double)i - A.cx) / A.fx, dy = -((double)j - A.cy) / A.fy;
    const double s0 = (dx * T.n0[0] + dy * T.n0[1]) - T.n0[2];
    const double s1 = (dx * T.n1[0] + dy * T.n1[1]) - T.n1[2];
    const double s2 = (dx * T.n2[0] + dy * T.n2[1]) - T.n2[2];
    const bool inside = (s0 >= 0.0 && s1 >= 0.0 && s2 >= 0.0) || (s0 <= 0.0 && s1 <= 0.0 && s2 <= 0.0);
    const double S = (s0 + s1) + s2;
    if (!inside || S == 0.0) return;
    const double t = T.det / S;
    if (!(t > A.z_near) || !(t <= A.z_far)) return;
    const uint32_t bits = __float_as_uint((float)t);
    uint32_t* px = A.img + ((int64_t)k * A.H + j) * A.W + i;
    // most candidates lie behind what the pixel already holds: a plain read first keeps them off the atomic (a stale read
    // only costs a redundant atomic)
    if (bits < *px) atomicMin(px, bits);
}

__global__ __launch_bounds__(MD_BLOCK) void md_small_kernel(MdArgs A) {
    const int64_t e = (int64_t)blockIdx.x * MD_BLOCK + threadIdx.x;
    if (e >= A.F * A.K) return;
    const int k = (int)(e / A.F);
    const int64_t f = e - (int64_t)k * A.F;
    MdTri T;
    if (!md_setup(A, f, k, T)) return;
    const int64_t box = (int64_t)(T.i1 - T.i0 + 1) * (T.j1 - T.j0 + 1);
    if (box > MD_SMALL) {
        const int64_t slot = atomicAdd(A.list_count, 1);
        if (slot < A.list_cap) {
            A.list[slot] = e;
            return;
        }
    }
    for (int j = T.j0; j <= T.j1; ++j)
        for (int i = T.i0; i <= T.i1; ++i) md_pixel(A, T, k, j, i);
}

__global__ __launch_bounds__(MD_BLOCK) void md_large_kernel(MdArgs A) {
    int64_t count = *A.list_count;
    count = count < A.list_cap ? count : A.list_cap;
    for (int64_t s = blockIdx.x; s < count; s += gridDim.x) {
        const int64_t e = A.list[s];
        if (e < 0 || e >= A.F * A.K) continue;
        const int k = (int)(e / A.F);
        MdTri T;
        if (!md_setup(A, e - (int64_t)k * A.F, k, T)) continue;
        const int bw = T.i1 - T.i0 + 1;
        const uint32_t box = (uint32_t)bw * (uint32_t)(T.j1 - T.j0 + 1);               // H * W <= 2^31
        for (uint32_t q = threadIdx.x; q < box; q += MD_BLOCK)
            md_pixel(A, T, k, T.j0 + (int)(q / (uint32_t)bw), T.i0 + (int)(q % (uint32_t)bw));
    }
}

__global__ __launch_bounds__(MD_BLOCK) void md_finish_kernel(uint32_t* img, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * MD_BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * MD_BLOCK)
        if (img[i] == MD_NONE) img[i] = 0u;
}

bool md_finite(double x) { return x == x && x - x == 0.0; }

int64_t md_list_cap(int64_t F, int64_t K) { return F * K < MD_LIST_CAP ? (F * K < 1 ? 1 : F * K) : MD_LIST_CAP; }

int md_sizes(int32_t n_verts, int32_t n_faces, int32_t n_views, int32_t H, int32_t W) {
    if (n_verts < 0 || n_faces < 0 || n_views < 0 || H <= 0 || W <= 0) return ENSLAM_EINVAL;
    // the list counter is an int32 and a box is counted in 32 bits
    if ((int64_t)n_views * H * W > ((int64_t)1 << 31) || (int64_t)n_faces * n_views > INT32_MAX) return ENSLAM_EUNSUPPORTED;
    return ENSLAM_OK;
}

}  // namespace

extern "C" {

int enslam_mesh_depth_workspace(int32_t n_faces, int32_t n_views, int64_t* bytes_host) {
    if (n_faces < 0 || n_views < 0 || !bytes_host) return ENSLAM_EINVAL;
    *bytes_host = 256 + 8 * md_list_cap(n_faces, n_views);
    return ENSLAM_OK;
}

int enslam_mesh_depth(const double* vertices, int32_t n_verts, const int32_t* faces, int32_t n_faces, const double* w2c,
                      int32_t n_views, int32_t H, int32_t W, double fx, double fy, double cx, double cy, double z_near,
                      double z_far, void* workspace, float* depth_out, void* stream) {
    const int rc = md_sizes(n_verts, n_faces, n_views, H, W);
    if (rc != ENSLAM_OK) return rc;
    if (!md_finite(fx) || !md_finite(fy) || !md_finite(cx) || !md_finite(cy) || fx == 0.0 || fy == 0.0) return ENSLAM_EINVAL;
    if (!md_finite(z_near) || z_far != z_far || z_near < 0.0 || !(z_far > z_near)) return ENSLAM_EINVAL;
    if (n_views == 0) return ENSLAM_OK;
    if (!depth_out || !w2c) return ENSLAM_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    const int64_t n_px = (int64_t)n_views * H * W;
    if (n_faces == 0 || n_verts == 0)
        return hipMemsetAsync(depth_out, 0, 4 * (size_t)n_px, s) == hipSuccess ? ENSLAM_OK : ENSLAM_ELAUNCH;
    if (!vertices || !faces || !workspace) return ENSLAM_EINVAL;
    MdArgs A;
    A.verts = vertices; A.faces = faces; A.w2c = w2c;
    A.F = n_faces; A.V = n_verts; A.K = n_views; A.H = H; A.W = W;
    A.fx = fx; A.fy = fy; A.cx = cx; A.cy = cy; A.z_near = z_near; A.z_far = z_far;
    A.img = (uint32_t*)depth_out;
    A.list_count = (int32_t*)workspace;
    A.list = (int64_t*)((char*)workspace + 256);
    A.list_cap = md_list_cap(n_faces, n_views);
    if (hipMemsetAsync(depth_out, 0xFF, 4 * (size_t)n_px, s) != hipSuccess) return ENSLAM_ELAUNCH;
    if (hipMemsetAsync(A.list_count, 0, 4, s) != hipSuccess) return ENSLAM_ELAUNCH;
    const unsigned blocks = (unsigned)(((int64_t)n_faces * n_views + MD_BLOCK - 1) / MD_BLOCK);
    md_small_kernel<<<blocks, MD_BLOCK, 0, s>>>(A);
    md_large_kernel<<<MD_LARGE_GRID, MD_BLOCK, 0, s>>>(A);
    const int64_t fin = (n_px + MD_BLOCK - 1) / MD_BLOCK;
    md_finish_kernel<<<(unsigned)(fin < 4096 ? fin : 4096), MD_BLOCK, 0, s>>>(A.img, n_px);
    return hipGetLastError() == hipSuccess ? ENSLAM_OK : ENSLAM_ELAUNCH;
}

}  // extern "C"
