// Colour images of a triangle mesh and a point set from K cameras: the headless renderer of the SLAM visualiser (the
// Open3D window of the reference's src/tools/viz.py).  The conventions are those of mesh_depth.hip: the camera looks down
// -z, pixel (row j, column i) sees the direction d = ((i - cx) / fx, -(j - cy) / fy, -1), vertices and matrices are float64.
//
// Visibility buffer: one uint64 per pixel and view, high word = the float32 bit pattern of the depth t, low word = the
// primitive (the face index f, or 0x80000000 | p for point p), combined with an unsigned 64-bit atomicMin: the nearest
// primitive wins, on equal float32 depth the smaller id, and a face beats a point.  The images are therefore the same bits
// in every run and do not depend on how the views are batched.
//
//   fill     the buffer with 0xFF bytes (nothing)
//   small    \ the rasteriser of tri_raster.hpp (the one mesh_depth.hip runs; the arithmetic is set out there) with culling;
//   large    / a covered pixel takes the minimum of what it holds and (bit pattern of t, face)
//   points   one thread per (point, view): a point of camera depth z = -p_z in (z_near, z_far] covers the point_size x
//            point_size pixel square whose first column is ceil(u - point_size / 2) and first row ceil(w - point_size / 2),
//            u = cx + fx (p_x / z), w = cy - fy (p_y / z), clipped to the image, at the constant depth z
//   resolve  one thread per pixel: a face's s_i again in float64, barycentrics s_i / S, vertex colours and vertex normals
//            interpolated, shade = ambient + (1 - ambient) |n^ . d^| (two-sided); a point's colour unshaded; the background
// Culling: 1 keeps det > 0 (the stored normal (b - a) x (c - a) points away from the eye), 2 keeps det < 0, 0 both.
//
// Vertex normals (Open3D's compute_vertex_normals): per vertex the unnormalised face normals (b - a) x (c - a) of its
// incident faces summed in ascending face order from a CSR incidence -- no float atomics -- then normalised; a zero sum
// stays zero.
#include "tri_raster.hpp"

namespace {

constexpr uint64_t SR_NONE = ~(uint64_t)0;
constexpr uint32_t SR_POINT = 0x80000000u;
constexpr int64_t SR_HEAD = 256;                        // bytes in front of the visibility buffer: the list counter

struct SrArgs : TriArgs {           // F is 0 without a mesh
    const uint8_t* vcol;            // [V,3] or NULL
    const double* vnrm;             // [V,3] or NULL
    const double* pts;              // [P,3]
    const uint8_t* pcol;            // [P,3]
    int32_t P, psize;
    double ambient;
    uint32_t background;            // r | g << 8 | b << 16
    uint64_t* vis;                  // [K,H,W]
    uint8_t* rgb;                   // [K,H,W,3]
    float* depth;                   // [K,H,W] or NULL
    int32_t* id;                    // [K,H,W] or NULL
};

ENS_DEV void sr_put(uint64_t* px, uint32_t depth_bits, uint32_t prim) {
    const uint64_t key = ((uint64_t)depth_bits << 32) | prim;
    // most candidates lie behind what the pixel already holds: a plain read first keeps them off the atomic (a stale read
    // only costs a redundant atomic)
    if (key < *px) atomicMin((unsigned long long*)px, (unsigned long long)key);
}

struct SrSink {
    static constexpr bool CULLS = true;
    uint64_t* vis;
    int32_t H, W, cull;
    ENS_DEV void put(int k, int j, int i, uint32_t bits, uint32_t face) const { sr_put(vis + ((int64_t)k * H + j) * W + i, bits, face); }
};

__global__ __launch_bounds__(TRI_BLOCK) void sr_point_kernel(SrArgs A) {
    const int64_t e = (int64_t)blockIdx.x * TRI_BLOCK + threadIdx.x;
    if (e >= (int64_t)A.P * A.K) return;
    const int k = (int)(e / A.P);
    const int32_t p = (int32_t)(e - (int64_t)k * A.P);
    const double* m = A.w2c + 12 * (int64_t)k;
    const double* w = A.pts + 3 * (int64_t)p;
    double c[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) c[r] = ((m[4 * r] * w[0] + m[4 * r + 1] * w[1]) + m[4 * r + 2] * w[2]) + m[4 * r + 3];
    const double z = -c[2];
    if (!(z > A.z_near) || !(z <= A.z_far)) return;
    const double half = 0.5 * (double)A.psize;
    const double a = ceil((A.cx + A.fx * (c[0] / z)) - half), b = ceil((A.cy - A.fy * (c[1] / z)) - half);
    // the square [a, a + psize) x [b, b + psize) against the image (a NaN fails every comparison)
    if (!(a < (double)A.W) || !(a + (double)A.psize > 0.0) || !(b < (double)A.H) || !(b + (double)A.psize > 0.0)) return;
    const int i0 = a < 0.0 ? 0 : (int)a, j0 = b < 0.0 ? 0 : (int)b;
    const double ae = a + (double)(A.psize - 1), be = b + (double)(A.psize - 1);
    const int i1 = ae > (double)(A.W - 1) ? A.W - 1 : (int)ae, j1 = be > (double)(A.H - 1) ? A.H - 1 : (int)be;
    const uint32_t bits = __float_as_uint((float)z);
    for (int j = j0; j <= j1; ++j)
        for (int i = i0; i <= i1; ++i) sr_put(A.vis + ((int64_t)k * A.H + j) * A.W + i, bits, SR_POINT | (uint32_t)p);
}

ENS_DEV uint8_t sr_level(double x) {
    const double v = floor(x + 0.5);
    return (uint8_t)(v < 0.0 ? 0.0 : (v > 255.0 ? 255.0 : v));                // a NaN gives 0
}

__global__ __launch_bounds__(TRI_BLOCK) void sr_resolve_kernel(SrArgs A) {
    const int64_t e = (int64_t)blockIdx.x * TRI_BLOCK + threadIdx.x;
    const int64_t hw = (int64_t)A.H * A.W;
    if (e >= hw * A.K) return;
    const uint64_t key = A.vis[e];
    const uint32_t prim = (uint32_t)key;
    uint8_t out[3] = {(uint8_t)A.background, (uint8_t)(A.background >> 8), (uint8_t)(A.background >> 16)};
    float depth = 0.f;
    int32_t id = -1;
    if (key != SR_NONE) {
        depth = __uint_as_float((uint32_t)(key >> 32));
        if (prim & SR_POINT) {
            const uint32_t p = prim & ~SR_POINT;
            id = -2 - (int32_t)p;
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) out[ch] = A.pcol[3 * (int64_t)p + ch];
        } else {
            id = (int32_t)prim;
            const int k = (int)(e / hw);
            const int64_t r = e - (int64_t)k * hw;
            const int j = (int)(r / A.W), i = (int)(r - (int64_t)j * A.W);
            int vi[3];
            double p[3][3], n0[3], n1[3], n2[3];
            tri_face(A, prim, k, vi, p);                                        // in range: the face made it into the buffer
            tri_cross(p[1], p[2], n0);
            tri_cross(p[2], p[0], n1);
            tri_cross(p[0], p[1], n2);
            const double dx = ((double)i - A.cx) / A.fx, dy = -((double)j - A.cy) / A.fy;
            const double s0 = (dx * n0[0] + dy * n0[1]) - n0[2];
            const double s1 = (dx * n1[0] + dy * n1[1]) - n1[2];
            const double s2 = (dx * n2[0] + dy * n2[1]) - n2[2];
            const double S = (s0 + s1) + s2;
            const double b0 = s0 / S, b1 = s1 / S, b2 = s2 / S;
            double n[3] = {0.0, 0.0, 0.0};
            if (A.vnrm) {
                const double *na = A.vnrm + 3 * (int64_t)vi[0], *nb = A.vnrm + 3 * (int64_t)vi[1], *nc = A.vnrm + 3 * (int64_t)vi[2];
#pragma unroll
                for (int c = 0; c < 3; ++c) n[c] = (b0 * na[c] + b1 * nb[c]) + b2 * nc[c];
            }
            if (n[0] == 0.0 && n[1] == 0.0 && n[2] == 0.0) {                    // the face normal, in world space
                const double *va = A.verts + 3 * (int64_t)vi[0], *vb = A.verts + 3 * (int64_t)vi[1], *vc = A.verts + 3 * (int64_t)vi[2];
                const double e1[3] = {vb[0] - va[0], vb[1] - va[1], vb[2] - va[2]};
                const double e2[3] = {vc[0] - va[0], vc[1] - va[1], vc[2] - va[2]};
                tri_cross(e1, e2, n);
            }
            // the pixel direction in world space: the rotation of w2c transposed
            const double* m = A.w2c + 12 * (int64_t)k;
            double dw[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) dw[c] = (m[c] * dx + m[4 + c] * dy) - m[8 + c];
            const double dot = (n[0] * dw[0] + n[1] * dw[1]) + n[2] * dw[2];
            const double nn = sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]);
            const double dd = sqrt((dw[0] * dw[0] + dw[1] * dw[1]) + dw[2] * dw[2]);
            const double len = nn * dd;
            const double shade = A.ambient + (1.0 - A.ambient) * (len > 0.0 ? fabs(dot) / len : 0.0);
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                double c = 0.7;
                if (A.vcol)
                    c = (b0 * ((double)A.vcol[3 * (int64_t)vi[0] + ch] / 255.0) + b1 * ((double)A.vcol[3 * (int64_t)vi[1] + ch] / 255.0)) +
                        b2 * ((double)A.vcol[3 * (int64_t)vi[2] + ch] / 255.0);
                out[ch] = sr_level((255.0 * c) * shade);
            }
        }
    }
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) A.rgb[3 * e + ch] = out[ch];
    if (A.depth) A.depth[e] = depth;
    if (A.id) A.id[e] = id;
}

// one thread per vertex: the face normals of off[v] .. off[v + 1] summed in the order of the list
__global__ __launch_bounds__(TRI_BLOCK) void sr_normals_kernel(const double* verts, int32_t V, const int32_t* faces, int32_t F,
                                                              const int64_t* off, const int32_t* inc, int64_t n_inc, double* out) {
    const int32_t v = (int32_t)((int64_t)blockIdx.x * TRI_BLOCK + threadIdx.x);
    if (v >= V) return;
    double acc[3] = {0.0, 0.0, 0.0};
    int64_t lo = off[v], hi = off[v + 1];
    lo = lo < 0 ? 0 : lo;
    hi = hi > n_inc ? n_inc : hi;
    for (int64_t s = lo; s < hi; ++s) {
        const int32_t f = inc[s];
        if ((uint32_t)f >= (uint32_t)F) continue;
        const int32_t ia = faces[3 * (int64_t)f], ib = faces[3 * (int64_t)f + 1], ic = faces[3 * (int64_t)f + 2];
        if ((uint32_t)ia >= (uint32_t)V || (uint32_t)ib >= (uint32_t)V || (uint32_t)ic >= (uint32_t)V) continue;
        const double *a = verts + 3 * (int64_t)ia, *b = verts + 3 * (int64_t)ib, *c = verts + 3 * (int64_t)ic;
        const double e1[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]};
        const double e2[3] = {c[0] - a[0], c[1] - a[1], c[2] - a[2]};
        double fn[3];
        tri_cross(e1, e2, fn);
        acc[0] += fn[0]; acc[1] += fn[1]; acc[2] += fn[2];
    }
    const double len = sqrt((acc[0] * acc[0] + acc[1] * acc[1]) + acc[2] * acc[2]);
    if (len > 0.0) { acc[0] /= len; acc[1] /= len; acc[2] /= len; }
    out[3 * (int64_t)v] = acc[0]; out[3 * (int64_t)v + 1] = acc[1]; out[3 * (int64_t)v + 2] = acc[2];
}

int64_t sr_vis_bytes(int64_t K, int64_t H, int64_t W) { return (8 * K * H * W + 255) / 256 * 256; }

}  // namespace

extern "C" {

int enslam_scene_normals(const double* vertices, int32_t n_verts, const int32_t* faces, int32_t n_faces,
                         const int64_t* vf_offsets, const int32_t* vf_faces, int64_t n_incident, double* normals_out,
                         void* stream) {
    if (n_verts < 0 || n_faces < 0 || n_incident < 0) return ENSLAM_EINVAL;
    if (n_verts == 0) return ENSLAM_OK;
    if (!vertices || !vf_offsets || !normals_out || (n_incident > 0 && (!faces || !vf_faces))) return ENSLAM_EINVAL;
    sr_normals_kernel<<<(unsigned)((n_verts + TRI_BLOCK - 1) / TRI_BLOCK), TRI_BLOCK, 0, (hipStream_t)stream>>>(
        vertices, n_verts, faces, n_faces, vf_offsets, vf_faces, n_incident, normals_out);
    return hipGetLastError() == hipSuccess ? ENSLAM_OK : ENSLAM_ELAUNCH;
}

int enslam_scene_raster_workspace(int32_t n_faces, int32_t n_views, int32_t H, int32_t W, int64_t* bytes_host) {
    if (n_faces < 0 || n_views < 0 || H <= 0 || W <= 0 || !bytes_host) return ENSLAM_EINVAL;
    if ((int64_t)n_views * H * W > ((int64_t)1 << 31)) return ENSLAM_EUNSUPPORTED;
    *bytes_host = SR_HEAD + sr_vis_bytes(n_views, H, W) + 8 * tri_list_cap(n_faces, n_views);
    return ENSLAM_OK;
}

int enslam_scene_raster(const double* vertices, int32_t n_verts, const int32_t* faces, int32_t n_faces,
                        const uint8_t* vertex_colors, const double* vertex_normals, const double* points, int32_t n_points,
                        const uint8_t* point_colors, int32_t point_size, const double* w2c, int32_t n_views, int32_t H,
                        int32_t W, double fx, double fy, double cx, double cy, double z_near, double z_far, int32_t cull,
                        double ambient, uint32_t background, int32_t passes, void* workspace, int64_t workspace_bytes,
                        uint8_t* rgb_out, float* depth_out, int32_t* id_out, void* stream) {
    const int rc = tri_refuse(n_verts, n_faces, n_points, n_views, H, W, fx, fy, cx, cy, z_near, z_far);
    if (rc != ENSLAM_OK) return rc;
    if (passes < 1 || passes > 7 || cull < 0 || cull > 2 || point_size < 1 || point_size > 64 || !(ambient >= 0.0) || !(ambient <= 1.0)) return ENSLAM_EINVAL;
    if (n_views == 0) return ENSLAM_OK;
    const int64_t vis_bytes = sr_vis_bytes(n_views, H, W);
    if (!rgb_out || !w2c || !workspace || workspace_bytes < SR_HEAD + vis_bytes + 8) return ENSLAM_EINVAL;
    const bool mesh = n_faces > 0 && n_verts > 0;
    if (mesh && (!vertices || !faces)) return ENSLAM_EINVAL;
    if (n_points > 0 && (!points || !point_colors)) return ENSLAM_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    const int64_t n_px = (int64_t)n_views * H * W;
    SrArgs A;
    A.verts = vertices; A.faces = faces; A.vcol = vertex_colors; A.vnrm = vertex_normals;
    A.pts = points; A.pcol = point_colors; A.w2c = w2c;
    A.F = mesh ? n_faces : 0; A.V = n_verts; A.P = n_points; A.K = n_views; A.H = H; A.W = W;
    A.psize = point_size;
    A.fx = fx; A.fy = fy; A.cx = cx; A.cy = cy; A.z_near = z_near; A.z_far = z_far; A.ambient = ambient;
    A.background = background;
    A.list_count = (int32_t*)workspace;
    A.vis = (uint64_t*)((char*)workspace + SR_HEAD);
    A.list = (int64_t*)((char*)workspace + SR_HEAD + vis_bytes);
    const int64_t room = (workspace_bytes - SR_HEAD - vis_bytes) / 8, want = tri_list_cap(n_faces, n_views);
    A.list_cap = room < want ? room : want;
    A.rgb = rgb_out; A.depth = depth_out; A.id = id_out;
    if (passes & 1) {
        if (hipMemsetAsync(A.vis, 0xFF, 8 * (size_t)n_px, s) != hipSuccess) return ENSLAM_ELAUNCH;
        if (hipMemsetAsync(A.list_count, 0, 4, s) != hipSuccess) return ENSLAM_ELAUNCH;
    }
    if (mesh && (passes & 1)) tri_launch(A, SrSink{A.vis, H, W, cull}, s);
    if (n_points > 0 && (passes & 2)) {
        const unsigned blocks = (unsigned)(((int64_t)n_points * n_views + TRI_BLOCK - 1) / TRI_BLOCK);
        sr_point_kernel<<<blocks, TRI_BLOCK, 0, s>>>(A);
    }
    if (passes & 4) sr_resolve_kernel<<<(unsigned)((n_px + TRI_BLOCK - 1) / TRI_BLOCK), TRI_BLOCK, 0, s>>>(A);
    return hipGetLastError() == hipSuccess ? ENSLAM_OK : ENSLAM_ELAUNCH;
}

}  // extern "C"
