// Depth images of a triangle mesh from K cameras (the off-screen depth renders of the reference's
// src/tools/eval_recon.py:131-210): pixel (row j, column i) of view k holds the smallest camera-space depth t in
// (z_near, z_far] at which the ray through ((i - cx) / fx, -(j - cy) / fy, -1) meets a triangle, 0.0 where none does.
// Both sides of a triangle count, edges are inclusive, degenerate triangles hit nothing.  Float64 up to the rounding of t.
//
//   fill    the images with the bit pattern 0xFFFFFFFF
//   small   \ the rasteriser of tri_raster.hpp (the arithmetic is set out there) without culling; a covered pixel takes
//   large   / the minimum of what it holds and the bit pattern of t
//   finish  0xFFFFFFFF -> 0.0
// Depths are combined by an unsigned integer minimum on the float32 bit pattern (positive floats order as their bits), so
// the images are the same bits in every run and do not depend on how the views are batched.
#include "tri_raster.hpp"

namespace {

constexpr uint32_t MD_NONE = 0xFFFFFFFFu;

struct MdSink {
    static constexpr bool CULLS = false;
    uint32_t* img;                  // [K,H,W] bit patterns
    int32_t H, W;
    ENS_DEV void put(int k, int j, int i, uint32_t bits, uint32_t) const {
        uint32_t* px = img + ((int64_t)k * H + j) * W + i;
        // most candidates lie behind what the pixel already holds: a plain read first keeps them off the atomic (a stale read
        // only costs a redundant atomic)
        if (bits < *px) atomicMin(px, bits);
    }
};

__global__ __launch_bounds__(TRI_BLOCK) void md_finish_kernel(uint32_t* img, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * TRI_BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * TRI_BLOCK)
        if (img[i] == MD_NONE) img[i] = 0u;
}

}  // namespace

extern "C" {

int enslam_mesh_depth_workspace(int32_t n_faces, int32_t n_views, int64_t* bytes_host) {
    if (n_faces < 0 || n_views < 0 || !bytes_host) return ENSLAM_EINVAL;
    *bytes_host = 256 + 8 * tri_list_cap(n_faces, n_views);
    return ENSLAM_OK;
}

int enslam_mesh_depth(const double* vertices, int32_t n_verts, const int32_t* faces, int32_t n_faces, const double* w2c,
                      int32_t n_views, int32_t H, int32_t W, double fx, double fy, double cx, double cy, double z_near,
                      double z_far, void* workspace, float* depth_out, void* stream) {
    const int rc = tri_refuse(n_verts, n_faces, 0, n_views, H, W, fx, fy, cx, cy, z_near, z_far);
    if (rc != ENSLAM_OK) return rc;
    if (n_views == 0) return ENSLAM_OK;
    if (!depth_out || !w2c) return ENSLAM_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    const int64_t n_px = (int64_t)n_views * H * W;
    if (n_faces == 0 || n_verts == 0)
        return hipMemsetAsync(depth_out, 0, 4 * (size_t)n_px, s) == hipSuccess ? ENSLAM_OK : ENSLAM_ELAUNCH;
    if (!vertices || !faces || !workspace) return ENSLAM_EINVAL;
    TriArgs A;
    A.verts = vertices; A.faces = faces; A.w2c = w2c;
    A.F = n_faces; A.V = n_verts; A.K = n_views; A.H = H; A.W = W;
    A.fx = fx; A.fy = fy; A.cx = cx; A.cy = cy; A.z_near = z_near; A.z_far = z_far;
    A.list_count = (int32_t*)workspace;
    A.list = (int64_t*)((char*)workspace + 256);
    A.list_cap = tri_list_cap(n_faces, n_views);
    const MdSink sink{(uint32_t*)depth_out, H, W};
    if (hipMemsetAsync(depth_out, 0xFF, 4 * (size_t)n_px, s) != hipSuccess) return ENSLAM_ELAUNCH;
    if (hipMemsetAsync(A.list_count, 0, 4, s) != hipSuccess) return ENSLAM_ELAUNCH;
    tri_launch(A, sink, s);
    const int64_t fin = (n_px + TRI_BLOCK - 1) / TRI_BLOCK;
    md_finish_kernel<<<(unsigned)(fin < 4096 ? fin : 4096), TRI_BLOCK, 0, s>>>(sink.img, n_px);
    return hipGetLastError() == hipSuccess ? ENSLAM_OK : ENSLAM_ELAUNCH;
}

}  // extern "C"
