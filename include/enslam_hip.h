/*
 * enslam_hip.h -- C ABI of the MI355X (gfx950) volume-rendering hot path.
 *
 * The reference (cs-vision/EvenNICER-SLAM) has no FFI on this path: its boundary
 * is a Python object protocol.  This library is what a
 * Python (ctypes) host binds instead of the PyTorch op sequence; each entry
 * point names the reference code it replaces (paths relative to the reference
 * checkout).  All pointers are DEVICE pointers unless marked "host".  Nothing
 * here allocates, frees, synchronises or takes ownership: the caller owns every
 * buffer, every call is stream-ordered on `stream` (a hipStream_t passed as
 * void*), re-entrant, and returns 0 on success or a negative ENSLAM_E* code.
 *
 * Memory layouts
 *   rays_o, rays_d      float32 [N,3]
 *   gt_depth            float32 [N]            (may be NULL: no depth guidance)
 *   z_vals              float64 [N,S]          sorted sample distances
 *   grid (reference)    float32 [1,32,D,H,W]   "channel-major", as the callers hold it
 *   grid (kernel)       float32 [D*H*W,32]     "voxel-major": one voxel corner = 128 contiguous bytes
 *   raw                 float32 [N*S,4]        (r,g,b,occ) after the out-of-bound mask
 *   depth, var          float64 [N];   rgb float32 [N,3]
 *   packed MLP          float32 [enslam_packed_floats(kind)]   (see enslam_pack_mlp)
 */
#ifndef ENSLAM_HIP_H
#define ENSLAM_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ENSLAM_ABI_VERSION 1

/* error codes */
#define ENSLAM_OK 0
#define ENSLAM_EINVAL (-1)      /* bad argument (NULL where required, unsupported size) */
#define ENSLAM_ELAUNCH (-2)     /* hipLaunch / hipMemsetAsync reported an error */
#define ENSLAM_EUNSUPPORTED (-3)

/* stages of NICE.forward, src/conv_onet/models/decoder.py:312-342 */
#define ENSLAM_STAGE_COARSE 0
#define ENSLAM_STAGE_MIDDLE 1
#define ENSLAM_STAGE_FINE 2
#define ENSLAM_STAGE_COLOR 3

/* decoder kinds (index into the arrays below) */
#define ENSLAM_MLP_COARSE 0     /* MLP_no_xyz, decoder.py:206-274 */
#define ENSLAM_MLP_MIDDLE 1     /* MLP,        decoder.py:91-203  */
#define ENSLAM_MLP_FINE 2       /* MLP with concat_feature (c_dim 64) */
#define ENSLAM_MLP_COLOR 3      /* MLP with 4 outputs */

/* Parameter tensors of one decoder, in the reference's state_dict layout
 * (row-major nn.Linear weights [out,in]).  Used as input by enslam_pack_mlp and
 * as OUTPUT (gradient tensors of the same shapes) by enslam_unpack_mlp_grads. */
typedef struct enslam_mlp_params {
    float *W[5];    /* pts_linears.{i}.weight  [32,K_i]; K = 93,32,32,125,32 (coarse: 32,32,32,64,32) */
    float *b[5];    /* pts_linears.{i}.bias    [32] */
    float *Wc[5];   /* fc_c.{i}.weight         [32,c_dim] (c_dim 32; fine 64); NULL for coarse */
    float *bc[5];   /* fc_c.{i}.bias           [32]; NULL for coarse */
    float *Wo;      /* output_linear.weight    [n_out,32]  (n_out 1; color 4) */
    float *bo;      /* output_linear.bias      [n_out] */
    float *B;       /* embedder._B             [3,93]; NULL for coarse */
} enslam_mlp_params;

/* One feature grid in voxel-major layout. */
typedef struct enslam_grid {
    float *data;    /* [D*H*W,32] (const for the forward; accumulation target for gradients) */
    int32_t D, H, W;
} enslam_grid;

/* Everything a render call reads.  grids/packed are indexed by ENSLAM_MLP_*.
 * Entries the stage does not use may be NULL. */
typedef struct enslam_scene {
    double bound[6];         /* host: x_lo,x_hi,y_lo,y_hi,z_lo,z_hi  (Renderer.bound, Renderer.py:20)   */
    double coarse_bound[6];  /* host: bound * coarse_bound_enlarge (EvenNICER_SLAM.py:182)             */
    enslam_grid grids[4];    /* coarse, middle, fine, color                                            */
    const float *packed[4];  /* packed decoders (enslam_pack_mlp)                                       */
} enslam_scene;

int enslam_abi_version(void);
const char *enslam_arch(void);          /* "gfx950" */

/* number of float32 in the packed form of decoder `kind` (forward + transposed sections) and
 * in its gradient accumulator (forward section only). */
size_t enslam_packed_floats(int kind);
size_t enslam_packed_grad_floats(int kind);

/* Re-layout one decoder's parameters for the MFMA kernels (zero-padded K, transposed copies for
 * the backward).  `packed` must have been zero-filled once by the caller; padding is never written.
 * Replaces nothing in the reference (layout glue for decoder.py:149-159 parameters). */
int enslam_pack_mlp(int kind, const enslam_mlp_params *params, float *packed, void *stream);
/* The same for several decoders in ONE launch (host arrays of length n <= 3). */
int enslam_pack_mlp_multi(int32_t n, const int32_t *kinds, const enslam_mlp_params *params, float *const *packed,
                          void *stream);

/* Inverse for gradients: packed_grad (accumulated by enslam_render_bwd) -> tensors shaped like the
 * reference parameters.  Pointers in `grads` that are NULL are skipped. */
int enslam_unpack_mlp_grads(int kind, const float *packed_grad, const enslam_mlp_params *grads, void *stream);
/* The same for several decoders in ONE launch (host arrays of length n <= 4). */
int enslam_unpack_mlp_grads_multi(int32_t n, const int32_t *kinds, const float *const *packed_grads,
                                  const enslam_mlp_params *grads, void *stream);

/* [C,V] -> [V,C] and back (C = 32).  Replaces the implicit layout of F.grid_sample's input
 * (decoder.py:173-174).  `to` reads the caller's grid; `from` writes a gradient the caller's
 * autograd expects ([1,32,D,H,W]). */
int enslam_grid_to_voxel_major(const float *src, float *dst, int64_t n_voxels, void *stream);
int enslam_grid_from_voxel_major(const float *src, float *dst, int64_t n_voxels, void *stream);
/* The same for up to 4 grids in ONE launch (n <= 4; src/dst/n_voxels are host arrays of length n). */
int enslam_grids_convert(int32_t n, const float *const *src, float *const *dst, const int64_t *n_voxels,
                         int32_t to_voxel_major, void *stream);

/* Sparse layout path.  A batch touches only a few percent of a grid; blocks of 64 consecutive voxels are the unit.
 * enslam_mark_blocks: flags[k][b] = 1 for every block of grid k (stage's grids) holding a corner that a sample of
 *   the batch reads (flags: uint8 [ceil(V_k/64)], caller-zeroed; entries of unused grids may be NULL).
 * enslam_grids_convert_sparse, to_voxel_major != 0: converts blocks with need && !valid and sets valid (valid: uint8
 *   bitmap that lives with the voxel-major copy; zero it when the source grid changes).
 *   to_voxel_major == 0 (gradients back to [32,V]): blocks with need are transposed, all others written as zeros.
 * enslam_zero_blocks: zero-fills the flagged blocks of voxel-major buffers (gradient accumulators) and, in the same
 *   launch, the flat float range [flat, flat + n_flat) (the small decoder / ray accumulators; may be NULL / 0). */
int enslam_mark_blocks(int32_t stage, int32_t n_rays, int32_t n_samples, const float *rays_o, const float *rays_d,
                       const double *z_vals, const enslam_scene *scene, uint8_t *const *flags, void *stream);
/* enslam_mark_blocks / enslam_bucket_pack / enslam_bucket_unpack at a finer block granularity: block_voxels in {64, 32, 16, 8}
 * voxels per flag (flags uint8 [ceil(n_voxels / block_voxels)] per grid, pos and bucket slots accordingly).  The bucket of a
 * ray-sharded step carries the union over ranks of the touched blocks; measured on one real step (room0, 1000 rays): 6.52 MB at
 * 64 voxels per block, 3.35 MB at 16 (the non-zero entries are 1.45 MB).  New functionality (the reference has no multi-GPU
 * path). */
int enslam_mark_blocks_g(int32_t stage, int32_t n_rays, int32_t n_samples, const float *rays_o, const float *rays_d,
                         const double *z_vals, const enslam_scene *scene, uint8_t *const *flags, int32_t block_voxels,
                         void *stream);
int enslam_bucket_pack_g(int32_t n_grids, const float *const *grid_grad, int32_t channels, const int64_t *n_voxels,
                         const int32_t *layout, const uint8_t *flags, const int32_t *pos, int32_t n_small,
                         const float *const *small, const int64_t *small_numel, int64_t small_base, float *bucket,
                         int32_t block_voxels, void *stream);
int enslam_bucket_unpack_g(int32_t n_grids, float *const *grid_grad, int32_t channels, const int64_t *n_voxels,
                           const int32_t *layout, const uint8_t *flags, const int32_t *pos, int32_t n_small,
                           float *const *small, const int64_t *small_numel, int64_t small_base, const float *bucket,
                           int32_t block_voxels, void *stream);
int enslam_grids_convert_sparse(int32_t n, const float *const *src, float *const *dst, const int64_t *n_voxels,
                                const uint8_t *const *need, uint8_t *const *valid, int32_t to_voxel_major,
                                void *stream);
int enslam_zero_blocks(int32_t n, float *const *dst, const int64_t *n_voxels, const uint8_t *const *need,
                       float *flat, int64_t n_flat, void *stream);

/* Tracker glue (RGB-D part).
 * enslam_pose_rays_fwd: camera tensor float32 [7] = (qr,qi,qj,qk, tx,ty,tz), pixels (pix_i = column, pix_j = row,
 *   float32 [n]) -> rays_o, rays_d float32 [n,3]: quad2rotation + get_camera_from_tensor (common.py:189-229) and
 *   get_rays_from_uv (:74-89) in one launch.  enslam_pose_rays_bwd: ray gradients (either may be NULL) ->
 *   g_camera_tensor float32 [7] (written, not accumulated); one workgroup, float64 sums, deterministic.
 * enslam_tracker_loss_fwd/bwd: Tracker.py:179-195 with handle_dynamic off:
 *   sum_{gt_depth>0} |gt_depth - depth| / sqrt(uncertainty + 1e-10)  +  w_color * sum_{gt_depth>0} |gt_color - color|
 *   (colour term when color/gt_color are given); the uncertainty carries no gradient (:179). */
int enslam_pose_rays_fwd(int32_t n, const float *camera_tensor, const float *pix_i, const float *pix_j, float fx,
                         float fy, float cx, float cy, float *rays_o, float *rays_d, void *stream);
/* Pixel samples of a frame behind the caller's single torch.randint draw (common.py:125-141, get_sample_uv / select_uv):
 * pixel_index int64 [n] in [0, window_h * window_w) of the window starting at (h0, w0) of an image_h x image_w frame ->
 * pix_i (column) / pix_j (row) float32 [n], depth_out float32 [n] from depth float32 [image_h, image_w], color_out [n,3] from
 * color [image_h, image_w, 3] (float32, or float64 with color_is_f64: the dataset readers hand out float64 colours).  The
 * caller keeps indices inside the window (they come from randint(window_h * window_w)); nothing is range-checked on the device. */
int enslam_gather_pixels(int32_t n, const int64_t *pixel_index, int32_t h0, int32_t w0, int32_t window_w, int32_t image_w,
                         int32_t image_h, const float *depth, const void *color, int32_t color_is_f64, float *pix_i,
                         float *pix_j, float *depth_out, void *color_out, void *stream);
int enslam_pose_rays_bwd(int32_t n, const float *camera_tensor, const float *pix_i, const float *pix_j, float fx,
                         float fy, float cx, float cy, const float *g_rays_o, const float *g_rays_d,
                         float *g_camera_tensor, void *stream);
int enslam_tracker_loss_fwd(int32_t n, const double *depth, const double *uncertainty, const float *color,
                            const float *gt_depth, const float *gt_color, float w_color, double *loss, void *stream);
int enslam_tracker_loss_bwd(int32_t n, const double *depth, const double *uncertainty, const float *color,
                            const float *gt_depth, const float *gt_color, float w_color, const double *g_loss,
                            double *g_depth, float *g_color, void *stream);

/* Mapper glue.  torch.optim.Adam (defaults) on voxel-major grids [V,32], restricted to the voxels whose
 * mask byte is 1 -- how Mapper.optimize_map optimises val_grad = val[mask] (Mapper.py:328-361, 573-575) without the
 * val[mask] = val_grad re-materialisation (:448-458, :596-602).  Per grid i: param / grad / exp_avg / exp_avg_sq are
 * float32 [n_voxels[i]*32]; mask uint8 [n_voxels[i]] or NULL (all voxels); lr[i] (float64) and step[i] (int32) are
 * DEVICE scalars (learning rate; Adam step count t >= 1 of this update, t <= 0: only clear the gradients) so that a captured
 * launch follows stage changes.  The gradients are cleared (everywhere, masked or not) by the same launch. */
int enslam_adam_masked(int32_t n, float *const *param, float *const *grad, float *const *exp_avg,
                       float *const *exp_avg_sq, const uint8_t *const *mask, const int64_t *n_voxels,
                       const double *const *lr, const int32_t *const *step, double beta1, double beta2, double eps,
                       void *stream);

/* The same Adam update for up to 72 small dense tensors (the decoder parameters the mapper optimises,
 * Mapper.py:363-369) in one launch; lr (float64) and step (int32, count of this update) are device scalars. */
int enslam_adam_tensors(int32_t n, float *const *param, const float *const *grad, float *const *exp_avg,
                        float *const *exp_avg_sq, const int64_t *numel, const double *lr, const int32_t *step,
                        double beta1, double beta2, double eps, void *stream);
/* enslam_adam_tensors for jobs of ONE workgroup (at most 1024 parameters in one tensor -- a camera tensor): *step holds the count
 * BEFORE this step; the launch uses *step + 1 and stores it back, so no separate increment launch precedes it.  More than one
 * workgroup: ENSLAM_EUNSUPPORTED. */
int enslam_adam_tensors_step(int32_t n, float *const *param, const float *const *grad, float *const *exp_avg,
                             float *const *exp_avg_sq, const int64_t *numel, const double *lr, int32_t *step, double beta1,
                             double beta2, double eps, void *stream);

/* Gradient bucket of the ray-sharded step (new functionality, SURVEY.md 8e: the reference has no multi-GPU path; the
 * tensors are the leaf gradients of Mapper.py:573-575).  Packs into / unpacks from one flat all-reduce buffer:
 *   - of up to 4 feature-grid gradients with `channels` channels each -- layout[g] 0: [channels, n_voxels[g]] (the
 *     reference's [1,C,D,H,W]), 1: voxel-major [n_voxels[g], channels] -- only the 64-voxel blocks whose flag is set.
 *     flags (uint8) and pos (int32, the INCLUSIVE prefix sum of flags) run over the blocks of all grids concatenated,
 *     ceil(n_voxels[g] / 64) per grid; flagged block b occupies bucket floats [(pos[b]-1) * channels * 64, +channels*64)
 *     in the gradient's own layout ([channels][64] or [64][channels]); voxels past the end of a grid travel as zeros;
 *   - then n_small (<= 72) dense tensors, concatenated from float offset small_base on.
 * The flags must be the union over ranks (so every rank lays the bucket out identically); unpack writes only the
 * flagged blocks and the small tensors. */
int enslam_bucket_pack(int32_t n_grids, const float *const *grid_grad, int32_t channels, const int64_t *n_voxels,
                       const int32_t *layout, const uint8_t *flags, const int32_t *pos, int32_t n_small,
                       const float *const *small, const int64_t *small_numel, int64_t small_base, float *bucket,
                       void *stream);
int enslam_bucket_unpack(int32_t n_grids, float *const *grid_grad, int32_t channels, const int64_t *n_voxels,
                         const int32_t *layout, const uint8_t *flags, const int32_t *pos, int32_t n_small,
                         float *const *small, const int64_t *small_numel, int64_t small_base, const float *bucket,
                         void *stream);

/* The small independent jobs around a render call in ONE launch each (they are 4-6 us kernels when issued separately):
 * enslam_step_prepare = enslam_pack_mlp_multi (n_dec decoders) + enslam_grids_convert_sparse to voxel-major (n_conv
 *   grids) + enslam_zero_blocks (n_zero accumulators and the flat range); any of the three parts may be empty.
 * enslam_step_finish  = enslam_grids_convert_sparse back to [32,V] (gradients) + enslam_unpack_mlp_grads_multi.
 * The finish launch is one family, each member the next wider one with its extra arguments fixed:
 *   enslam_step_finish           = enslam_step_finish_rays with n_rays = 0 (no ray arguments)
 *   enslam_step_finish_rays      = enslam_step_finish_rays_prev with prev = NULL
 *   enslam_step_finish_rays_prev = enslam_step_finish_partials with grad_partials = NULL, except for the NULL hand-off below
 *   enslam_step_finish_partials  = enslam_step_finish_native with n_move = 0 (move_need, move_prev unused)
 * One rule differs.  With a ray role asked for (n_rays > 0, stage above COARSE) the two narrow members that take rays,
 * enslam_step_finish_rays and enslam_step_finish_rays_prev, REQUIRE the hand-off: dgrid_ws NULL is ENSLAM_EINVAL (after the
 * sample count has been checked).  The two wide members, enslam_step_finish_partials and enslam_step_finish_native, read a
 * NULL dgrid_ws as "no ray role": the ray arguments, scene and sample count are then not looked at, as with n_rays = 0.
 * Common to all: n_rays < 0 (and n_move < 0, or n_move > 0 without both move pointers) is ENSLAM_EINVAL; then prev, when given,
 * needs need and every need[i] / prev[i] (ENSLAM_EINVAL); then, with a ray role, n_samples not in {16, 32, 48, 64} is
 * ENSLAM_EUNSUPPORTED, and a scene that lacks the stage's grids, a NULL ray pointer or half a work list ENSLAM_EINVAL; the
 * conversion and unpack arguments are checked last. */
int enslam_step_prepare(int32_t n_dec, const int32_t *kinds, const enslam_mlp_params *params, float *const *packed,
                        int32_t n_conv, const float *const *src, float *const *dst, const int64_t *n_voxels,
                        const uint8_t *const *need, uint8_t *const *valid, int32_t n_zero, float *const *zero_dst,
                        const int64_t *zero_voxels, const uint8_t *const *zero_need, float *flat, int64_t n_flat,
                        void *stream);
int enslam_step_finish(int32_t n_conv, const float *const *src, float *const *dst, const int64_t *n_voxels,
                       const uint8_t *const *need, int32_t n_dec, const int32_t *kinds,
                       const float *const *packed_grads, const enslam_mlp_params *grads, void *stream);
/* enslam_step_finish with enslam_ray_grad_bwd riding in the same launch (both depend only on enslam_decoder_bwd):
 * one dependent launch fewer per step.  stage COARSE or n_rays == 0: plain enslam_step_finish.  Otherwise dgrid_ws (the
 * hand-off enslam_decoder_bwd left) is required, see above. */
int enslam_step_finish_rays(int32_t n_conv, const float *const *src, float *const *dst, const int64_t *n_voxels,
                            const uint8_t *const *need, int32_t n_dec, const int32_t *kinds,
                            const float *const *packed_grads, const enslam_mlp_params *grads, int32_t stage,
                            int32_t n_rays, int32_t n_samples, const float *rays_o, const float *rays_d,
                            const double *z_vals, const enslam_scene *scene, float *dgrid_ws, float *g_rays_o,
                            float *g_rays_d, const int32_t *work_list, const int32_t *work_count, void *stream);
/* enslam_step_finish_rays into PERSISTENT gradient tensors: dst[i] is the same memory from call to call (the dense
 * gradient of a grid inside a captured hipGraph step) and prev[i] (uint8 per 64-voxel block, as need[i]; all zero and
 * dst[i] all zero before the first call) holds the blocks the previous call wrote.  Blocks touched neither then nor now
 * keep their zeros and are not written; the others are written / cleared as in enslam_step_finish_rays, and need[i] is
 * MOVED to prev[i] on the way (need[i] is all zero afterwards: a captured step keeps its flags in memory that nothing
 * re-zeroes between replays; read the touched blocks from prev[i]).  The result in dst is identical; the 48 MB zero-fill of room0's three dense gradients
 * becomes ~6 MB.  prev NULL: enslam_step_finish_rays.  Replaces nothing in the reference: autograd allocates a fresh dense
 * gradient per backward there (Mapper.py:573-575 then reads three mostly-zero 16 MB tensors). */
int enslam_step_finish_rays_prev(int32_t n_conv, const float *const *src, float *const *dst, const int64_t *n_voxels,
                                 const uint8_t *const *need, uint8_t *const *prev, int32_t n_dec, const int32_t *kinds,
                                 const float *const *packed_grads, const enslam_mlp_params *grads, int32_t stage,
                                 int32_t n_rays, int32_t n_samples, const float *rays_o, const float *rays_d,
                                 const double *z_vals, const enslam_scene *scene, float *dgrid_ws, float *g_rays_o,
                                 float *g_rays_d, const int32_t *work_list, const int32_t *work_count, void *stream);

/* enslam_step_finish_rays_prev (prev NULL: no persistent destinations) which, for every decoder i with grad_partials[i] != NULL,
 * forms the gradient as the SUM of the per-workgroup partial images enslam_decoder_bwd_partials left there instead of reading
 * packed_grads[i] (grad_partials NULL: none).  Unlike there, dgrid_ws NULL means "no ray-gradient role", as n_rays == 0 does. */
int enslam_step_finish_partials(int32_t n_conv, const float *const *src, float *const *dst, const int64_t *n_voxels,
                                const uint8_t *const *need, uint8_t *const *prev, int32_t n_dec, const int32_t *kinds,
                                const float *const *packed_grads, const float *const *grad_partials,
                                const enslam_mlp_params *grads, int32_t stage, int32_t n_rays, int32_t n_samples,
                                const float *rays_o, const float *rays_d, const double *z_vals, const enslam_scene *scene,
                                float *dgrid_ws, float *g_rays_o, float *g_rays_d, const int32_t *work_list,
                                const int32_t *work_count, void *stream);

/* enslam_step_finish_partials plus the flag hand-over for gradients that live in the kernels' own layout (feature grids given
 * as channels_last_3d tensors: their storage IS [V][32], nothing is converted on the way in and the gradient buffer the backward
 * adds into IS the tensor autograd receives, so no transposed-back copy exists whose launch could carry the flags): for the
 * n_move block flags at move_need (uint8, the flags this step's sampler marked, all such grids back to back) the launch does
 * move_prev[b] = move_need[b]; move_need[b] = 0.  `move_prev` is what the next step's enslam_sample_prepare clears the
 * persistent gradient by (zero_need) and what the gradient bucket reads.  n_move = 0: enslam_step_finish_partials. */
int enslam_step_finish_native(int32_t n_conv, const float *const *src, float *const *dst, const int64_t *n_voxels,
                              const uint8_t *const *need, uint8_t *const *prev, int32_t n_dec, const int32_t *kinds,
                              const float *const *packed_grads, const float *const *grad_partials,
                              const enslam_mlp_params *grads, int32_t stage, int32_t n_rays, int32_t n_samples,
                              const float *rays_o, const float *rays_d, const double *z_vals, const enslam_scene *scene,
                              float *dgrid_ws, float *g_rays_o, float *g_rays_d, const int32_t *work_list,
                              const int32_t *work_count, uint8_t *move_need, uint8_t *move_prev, int64_t n_move, void *stream);

/* enslam_sample_rays_g and enslam_step_prepare (without its conversion role) as ONE launch, for render calls whose
 * feature grids all arrive in the kernels' own layout: with nothing to convert, no prepare role waits for the sampler's
 * block marks, and the decoder packing / accumulator clearing run under the sampler's latency (a ray's wave is one dependent
 * chain of float64 divisions and a 21-step shuffle sort).  Arguments: enslam_sample_rays_g's, then enslam_step_prepare's
 * (n_dec .. packed, n_zero .. n_flat); the sampler arguments are checked as there (mark_block_voxels in every call).
 * n_rays = 0 runs the prepare roles alone: unlike enslam_sample_rays_g, which returns ENSLAM_OK for n_rays = 0 before it looks
 * at a pointer or at the marking, this call goes on, still needs bound_host and still checks the marking arguments.
 *   Replaces Renderer.render_batch_ray lines 83-171 (sampling) of the reference; the prepare roles replace nothing. */
int enslam_sample_prepare(int32_t n_rays, int32_t n_lin, int32_t n_surf, const float *rays_o, const float *rays_d,
                          const float *gt_depth, const double *bound_host, const float *t_lin, const double *t_surf,
                          int32_t lindisp, const float *t_rand, float *scratch, int32_t depth_max_given, double *z_vals,
                          int32_t mark_stage, const enslam_scene *mark_scene, uint8_t *const *mark_flags,
                          int32_t mark_block_voxels, uint8_t *const *mark_flags64, int32_t n_dec, const int32_t *kinds,
                          const enslam_mlp_params *params, float *const *packed, int32_t n_zero, float *const *zero_dst,
                          const int64_t *zero_voxels, const uint8_t *const *zero_need, float *flat, int64_t n_flat,
                          void *stream);

/* Head of the tracker's camera iteration in one launch (one workgroup; any n): for the n window pixels `pixel_index` (int64,
 * row-major inside the window that starts at (H0, W0) and is window_w wide -- the single torch.randint draw of
 * common.get_sample_uv) it writes their column / row as floats (pix_i, pix_j), their depth and colour samples (gt_depth,
 * gt_color as float32 [n,3]), their rays from the camera tensor [qr,qi,qj,qk,tx,ty,tz] (rays_o, rays_d: enslam_pose_rays_fwd's
 * arithmetic) and -- prefilter != 0 -- the in-bound mask  inside[k] = min_axis max_side((bound - o) / d) >= gt_depth[k]  in
 * float64, with depth_max = {max over the inside rays of gt_depth (0 if none), that * 1.2f}: the sampler's batch maxima when the
 * rays the reference drops are rendered but masked (prefilter == 0: maxima over all rays, inside untouched).
 * draw_counter (optional, int32 [1] on the device): pixel_index then holds n_draws rows of n indices drawn ahead (one
 * torch.randint per frame instead of one per iteration -- under hipGraph replay every captured randint costs its launch plus two
 * fill launches for the generator's seed and offset); the call takes row *draw_counter % n_draws and increments the counter.
 * An index outside [0, (image_h - H0) * window_w) is clamped into it (no read ever leaves the images).
 *   Replaces Tracker.optimize_cam_in_batch lines 160-174 (get_samples with the camera tensor's pose, the `inside_mask` filter)
 *   and common.get_camera_from_tensor (common.py:189-229) for this use. */
int enslam_tracker_rays(int32_t n, const float *camera_tensor, const int64_t *pixel_index, int32_t H0, int32_t W0,
                        int32_t window_w, int32_t image_w, int32_t image_h, const float *depth_image, const void *color_image,
                        int32_t color_is_f64, float fx, float fy, float cx, float cy, const double *bound_host,
                        int32_t prefilter, float *pix_i, float *pix_j, float *rays_o, float *rays_d, float *gt_depth,
                        float *gt_color, uint8_t *inside, float *depth_max, int32_t *draw_counter, int32_t n_draws,
                        void *stream);

/* enslam_render_loss_fwd with the TRACKER's loss in place of the mapper's (batches of up to enslam_tracker_tail_max_rays()
 * rays; more, or the coarse stage: ENSLAM_EUNSUPPORTED, reported where the sample count is, before the scene and the pointers
 * are looked at; tmp_scratch is required as gt_depth, loss and raw_out are): behind the decoder kernel two launches of 16
 * rays per workgroup (one without handle_dynamic) -- compositing with
 *   tmp = |gt_depth - depth| / sqrt(var + 1e-10),
 * then, every workgroup taking the median of tmp over the inside rays for itself (the lower median of torch.median; by counting
 * ranks in LDS up to 1024 rays, a bitonic network above),
 *   keep = inside & (handle_dynamic ? tmp < 10 * median : 1),
 *   loss += sum_{keep & gt_depth > 0} tmp + w_color * sum_{keep & gt_depth > 0} |gt_color - color|   (gt_color NULL: depth term)
 * with d(loss)/d(raw) for a unit loss gradient in d_raw_unit and the work list of active tiles, the variance treated as a
 * constant.  inside NULL: every ray.  tmp_scratch: float64 [n_rays].  *loss must be 0 on entry.
 *   Replaces Tracker.optimize_cam_in_batch lines 176-195 around Renderer.render_batch_ray. */
int enslam_tracker_tail_max_rays(void);
/* The number of 16-sample tiles from which a forward-only colour-stage call (enslam_eval_points, or enslam_render_fwd with
 * raw_out and act_ws NULL) runs on the weight-stationary decoder kernel; below it the call runs on the ring kernel.  The
 * two kernels give the same bits. */
int64_t enslam_fwd_res_min_tiles(void);
/* The workgroup count of the persistent decoder backward (one per compute unit): the upper bound of the workgroups of one
 * decoder role, i.e. of the rows of a partial buffer (enslam_bwd_partial_floats).  A batch of more than 4 * this many
 * 16-sample tiles makes a role walk several rounds. */
int enslam_bwd_max_workgroups(void);
int enslam_render_tracker_loss_fwd(int32_t stage, int32_t n_rays, int32_t n_samples, const float *rays_o, const float *rays_d,
                                   const double *z_vals, const enslam_scene *scene, double *depth, double *var, float *rgb,
                                   float *raw_out, float *act_ws, int32_t act_light, const float *gt_depth,
                                   const float *gt_color, float w_color, const uint8_t *inside, int32_t handle_dynamic,
                                   double *tmp_scratch, double *loss, float *d_raw_unit, int32_t *work_list,
                                   int32_t *work_count, void *stream);

/* The tail of enslam_render_tracker_loss_fwd on its own, on a raw [n_rays, n_samples, 4] of the caller's (1 <= n_samples <= 64;
 * a work list needs n_samples % 16 == 0, else ENSLAM_EINVAL; more than enslam_tracker_tail_max_rays() rays:
 * ENSLAM_EUNSUPPORTED): the same launches with the same arguments, outputs and *loss == 0 on entry as there.
 * loss_only != 0 (valid with handle_dynamic != 0 only, else ENSLAM_EINVAL): the compositing launch is skipped and the second
 * launch (median, mask, loss, unit gradients, work list) runs on the depth, var, rgb and tmp_scratch the caller filled.
 * A NaN in tmp is outside the contract: its ray is not kept (tmp < 10 * median is false), up to 1024 rays it counts among the
 * inside rays but ranks above every finite value like +inf (torch.median would return NaN; with one or two inside rays the
 * NaN itself can become the median, and then nothing is kept), and above 1024 rays the sorting network's order, hence the
 * median, is unspecified. */
int enslam_tracker_tail(int32_t n_rays, int32_t n_samples, const float *raw, const double *z_vals, double *depth, double *var,
                        float *rgb, const float *gt_depth, const float *gt_color, float w_color, const uint8_t *inside,
                        int32_t handle_dynamic, double *tmp_scratch, double *loss, float *d_raw_unit, int32_t *work_list,
                        int32_t *work_count, int32_t loss_only, void *stream);

/* Sample distances along rays (mark_scene / mark_flags non-NULL: also does enslam_mark_blocks' work for stage mark_stage
 * on the samples it has just placed -- one launch less per render call).
 *   Replaces Renderer.render_batch_ray lines 83-171
 * (src/utils/Renderer.py): near/far from gt_depth and the AABB exit, n_lin linear samples,
 * n_surf near-surface samples (gt_depth>0: [0.95d,1.05d]; else [0.001,max d]), ascending merge.
 *   t_lin   float32 [n_lin]  = torch.linspace(0,1,n_lin)
 *   t_surf  float64 [n_surf] = torch.linspace(0,1,n_surf).double()   (ignored if n_surf == 0)
 *   t_rand  float32 [N,n_lin] or NULL (perturb == 0)
 *   scratch float32 [2]: {max(gt_depth), fl32(max(gt_depth)*1.2f)} (batch-global, Renderer.py:110,145).
 *           depth_max_given == 0: computed here over this call's gt_depth and written to scratch;
 *           depth_max_given != 0: read from scratch (a ray-sharded caller supplies the max of the WHOLE batch,
 *           so that every shard samples exactly what the unsharded reference would).
 *   z_vals  float64 [N, n_lin + n_surf] (n_surf forced to 0 when gt_depth is NULL)
 * n_lin >= 1 and at most 64 samples per ray, judged on the count that is written (n_lin alone when gt_depth is NULL):
 * ENSLAM_EINVAL otherwise, without a launch.
 * Bit-exact with the reference's float64/float32 evaluation order on every ray whose intermediates are numbers.
 * Outside the contract: a face distance 0/0 (an origin exactly on a face of the bound with a zero direction component along
 * that axis), a gt_depth that is not finite, and lindisp != 0 with near == 0 or far == 0 (a depth <= 0, an origin outside the
 * bound).  torch's max / min hand a NaN on; the comparisons here do not (t0 > t1 ? t0 : t1, fmaxf), so such a ray's own row of
 * z_vals is unspecified, and a gt_depth that is not finite makes the batch maxima, hence scratch and every depth-guided row
 * of the call, unspecified.  In no other way does such a ray touch another ray's row, and nothing outside z_vals' [N, S]
 * is written. */
int enslam_sample_rays(int32_t n_rays, int32_t n_lin, int32_t n_surf, const float *rays_o, const float *rays_d,
                       const float *gt_depth, const double *bound_host, const float *t_lin, const double *t_surf,
                       int32_t lindisp, const float *t_rand, float *scratch, int32_t depth_max_given, double *z_vals,
                       int32_t mark_stage, const enslam_scene *mark_scene, uint8_t *const *mark_flags, void *stream);
/* enslam_sample_rays whose block marking works at mark_block_voxels in {64, 32, 16, 8} voxels per flag (mark_flags sized
 * accordingly) and, for the finer ones, optionally leaves the 64-voxel form in mark_flags64 as well (NULL: not wanted): the flags
 * of a ray-sharded step's gradient bucket (enslam_bucket_pack_g) and what the finish launch keeps, from ONE launch.
 * enslam_sample_rays is this call with mark_block_voxels = 64 and mark_flags64 = NULL.  A mark_block_voxels outside {64, 32, 16, 8} is
 * ENSLAM_EINVAL, with or without marking and for n_rays = 0 too; no pointer and no marking argument is looked at when n_rays = 0 (ENSLAM_OK). */
int enslam_sample_rays_g(int32_t n_rays, int32_t n_lin, int32_t n_surf, const float *rays_o, const float *rays_d,
                         const float *gt_depth, const double *bound, const float *t_lin, const double *t_surf,
                         int32_t lindisp, const float *t_rand, float *scratch, int32_t depth_max_given, double *z_vals,
                         int32_t mark_stage, const enslam_scene *mark_scene, uint8_t *const *mark_flags,
                         int32_t mark_block_voxels, uint8_t *const *mark_flags64, void *stream);

/* Forward of Renderer.render_batch_ray lines 173-181 + eval_points (Renderer.py:24-62) +
 * NICE.forward (decoder.py:312-342) + raw2outputs_nerf_color (common.py:256-297, occupancy):
 * points, bound mask, trilinear gather, decoders, alpha compositing.  S must be 16, 32, 48 or 64 (64: tile-per-wave
 * forward only, i.e. up to 32768 rays per call; ENSLAM_EUNSUPPORTED beyond).
 * raw_out (may be NULL) receives the per-sample (r,g,b,occ) needed by enslam_render_bwd. */
int enslam_render_fwd(int32_t stage, int32_t n_rays, int32_t n_samples, const float *rays_o, const float *rays_d,
                      const double *z_vals, const enslam_scene *scene, double *depth, double *var, float *rgb,
                      float *raw_out, float *act_ws, int32_t act_light, void *stream);

/* float32 count of the activation workspace `act_ws` for a batch (0 for the coarse stage, which always
 * recomputes).  When enslam_render_fwd is given a workspace of this size it also writes, per 16-sample tile and
 * decoder, the operands the backward needs (embedding, grid features, hidden activations, ReLU masks), and
 * enslam_decoder_bwd / enslam_render_bwd given the same buffer read them instead of recomputing the decoder
 * forward.  NULL in both places selects recomputation (no extra memory, slower backward).
 * act_light != 0 (same value in the size query, the forward and the backward): the backward will be asked for no
 * decoder-parameter gradient (tracker iterations, mapper stages with fixed decoders), so only the sample
 * coordinates, the ReLU masks and the trilinear cell records are kept: 1.8 KB instead of 22 KB per tile and decoder. */
size_t enslam_activation_floats(int32_t stage, int32_t n_rays, int32_t n_samples, int32_t act_light);
/* float32 count of the scratch buffer `dgrid_ws` the backward needs when it runs from `act_ws` AND ray gradients
 * are requested (decoder kernel -> ray-gradient kernel hand-off: feature gradient and embedding position gradient per
 * tile and decoder).  dgrid_ws may be NULL when g_rays_o is NULL.  act_ws needs every grid below 2^29 voxels. */
size_t enslam_grid_handoff_floats(int32_t stage, int32_t n_rays, int32_t n_samples);

/* Forward of Renderer.eval_points (Renderer.py:24-62) on explicit points p float64 [P,3].
 * apply_mask = 0 gives the bare decoder call NICE.forward (decoder.py:312-342, as Mesher.py:308 uses it). */
int enslam_eval_points(int32_t stage, int64_t n_points, const double *points, const enslam_scene *scene,
                       int32_t apply_mask, float *raw_out, void *stream);

/* Marching cubes (the skimage.measure.marching_cubes call of Mesher.py:495-520) on a float32 lattice volume
 * [nx, ny, nz], z fastest: the reference's z.reshape(ny, nx, nz).transpose(1, 0, 2) indexed [ix, iy, iz].
 * A corner is occupied iff value > level; an edge carries a vertex iff its ends differ; each lattice point owns its
 * +x, +y and +z edges.
 *   vertices float64 [V,3]: owner point in linear [ix, iy, iz] order, then axis x < y < z; position
 *            origin + (index + t) * spacing, t = (level - a) / (b - a), float64
 *   faces    int32 [F,3]:   cell in linear order, then the case table's order (csrc/mc_tables.hpp, generated by
 *            tools/gen_mc_tables.py); right-hand normals point from occupied to free.  Deterministic: no atomics.
 * Two calls on one stream with the same workspace: the count call leaves {V, F} in counts (device int32 [2]); the caller
 * reads them back, allocates exactly and passes them to the emit call.  Every dimension >= 2, nx*ny*nz <= 512^3
 * (ENSLAM_EUNSUPPORTED beyond), a finite level, origin_host / spacing_host (host float64 [3]) finite. */
int enslam_marching_cubes_workspace(int32_t nx, int32_t ny, int32_t nz, int64_t *bytes_host);
int enslam_marching_cubes_count(const float *volume, int32_t nx, int32_t ny, int32_t nz, double level, void *workspace,
                                int32_t *counts, void *stream);
int enslam_marching_cubes_emit(const float *volume, int32_t nx, int32_t ny, int32_t nz, double level,
                               const double *origin_host, const double *spacing_host, void *workspace, int32_t n_verts,
                               int32_t n_faces, double *verts, int32_t *faces, void *stream);

/* Visibility of points in K cameras: the projection loop of Mesher.point_masks (src/utils/Mesher.py:88-190) and of
 * Mapper.keyframe_selection_overlap (src/Mapper.py:218-241).  One thread per point; the cameras are wave-uniform data.
 * Per camera k, in float32 (real64 = 0, the Mesher's points.float() path) or float64 (real64 = 1, the Mapper's numpy path):
 *   cam = w2c[k][:3,:3] p + w2c[k][:3,3]; cam.x *= -1; uvz = K cam; z = uvz.z + z_eps; (u, v) = float32(uvz.xy / z)
 *   inside(edge) = edge < u < W - edge  and  edge < v < H - edge  and  z < 0                      (all strict)
 *   seen_k     = inside(edge_seen)     [and -cam.z < limit[k]]  [and  sample - 2.4 < -cam.z < sample + 2.4]
 *   forecast_k = inside(edge_forecast) [and -cam.z < limit[k]]  [and  -cam.z < max_sample[k]]
 * where sample is the bilinear sample of depth[k] at (u, v) with zero padding (F.grid_sample, align_corners=True) and
 * max_sample[k] the largest sample of camera k over ALL points of the call, in view or not (the reference's
 * torch.max(depth_sample) per chunk of points: chunk in the caller to match it chunk for chunk).
 *   points   float32 [P,3], or NULL for a lattice: point i is (ax[ix], ay[iy], az[iz]) of the linear index
 *            lattice_first + i = (ix * ny + iy) * nz + iz  (Mesher.lattice_volume's order); ax/ay/az float32 [nx]/[ny]/[nz]
 *   w2c      float32 (real64 = 0) or float64 (real64 = 1) [K,12]: the upper three rows of each world-to-camera matrix
 *   limit    float32 [K] or NULL;  depth float32 [K,H,W] or NULL (needs workspace, H and W >= 2)
 *   classes  uint8 [P] or NULL: 0 unseen, 1 seen by some camera, 2 forecast by some camera and seen by none
 *   counts   int32 [K] or NULL: points that pass seen_k (zeroed by the call).  With counts NULL a wave leaves the camera
 *            loop once all its points are seen.
 * Integer adds and a maximum: the outputs do not depend on the launch order.  P = 0 and K = 0 are valid. */
int enslam_visibility_workspace(int32_t n_cams, int64_t *bytes_host);
int enslam_visibility(int32_t real64, int64_t n_points, const float *points, const float *ax, const float *ay,
                      const float *az, int32_t nx, int32_t ny, int32_t nz, int64_t lattice_first, int32_t n_cams,
                      const void *w2c, double fx, double fy, double cx, double cy, int32_t H, int32_t W, int32_t edge_seen,
                      int32_t edge_forecast, double z_eps, const float *limit, const float *depth, void *workspace,
                      uint8_t *classes, int32_t *counts, void *stream);

/* Mesh cleaning: the tail of Mesher.get_mesh (src/utils/Mesher.py:469-510) on a triangle mesh, vertices float64 [V,3] and
 * faces int32 [F,3] with indices in [0, V) -- any such mesh, boundary edges and edges of three or more faces included.
 *   adjacency  two faces are adjacent iff they share an undirected edge (the same unordered pair of vertex indices); faces
 *              that share only a vertex are not
 *   labels     int32 [F]: the smallest face index of the face's edge-connected component (canonical: it does not depend on
 *              scheduling, and it numbers the components in the order of their first faces)
 *   mask drop  vertex_keep uint8 [V] or NULL (keep all): a face goes iff none of its three vertices is kept
 *   areas      0.5 * |(v1 - v0) x (v2 - v0)| per face in float64, unfused; summed per component in 80-bit fixed point scaled
 *              by the mesh's largest face area (integer adds: the same bits in every run; a sum is below the exact sum of
 *              its float64 areas by less than 2^-56 of the largest face area).  Non-finite areas count as zero.
 *   keep rule  largest_only = 0: the components with area > min_area (strict); else the one with the largest area, ties to
 *              the smallest label
 *   output     kept faces in their original order, the vertices a kept face references in their original order, face
 *              indices remapped; vertex_index_out int32 [V_out] or NULL: the original index of each kept vertex.  Output
 *              positions are prefix sums: no order depends on scheduling.
 * Two calls on one stream with the same workspace, as for marching cubes: the count call leaves {kept vertices, kept faces,
 * components after the mask drop} in counts (device int32 [3]); the caller reads them back, allocates exactly and passes
 * them to the emit call with the same vertices and faces.  The components call is the labelling alone (no mask, indices are
 * only compared, never used as addresses).  Limits: n_faces <= 2^24, n_verts <= 2^26 (ENSLAM_EUNSUPPORTED beyond); negative
 * counts, NULL where data is required and a NaN min_area: ENSLAM_EINVAL.  A vertex index outside [0, V) is the caller's error:
 * the cleaning calls drop such a face, nothing reports it.  Zero faces or vertices are valid (empty result). */
int enslam_mesh_clean_workspace(int32_t n_verts, int32_t n_faces, int64_t *bytes_host);
int enslam_mesh_components(const int32_t *faces, int32_t n_faces, int32_t n_verts, void *workspace, int32_t *labels_out,
                           void *stream);
int enslam_mesh_clean_count(const double *vertices, int32_t n_verts, const int32_t *faces, int32_t n_faces,
                            const uint8_t *vertex_keep, double min_area, int32_t largest_only, void *workspace,
                            int32_t *counts, void *stream);
int enslam_mesh_clean_emit(const double *vertices, int32_t n_verts, const int32_t *faces, int32_t n_faces, void *workspace,
                           int32_t n_verts_out, int32_t n_faces_out, double *vertices_out, int32_t *faces_out,
                           int32_t *vertex_index_out, void *stream);

/* Exact nearest neighbour in float64 (the cKDTree queries of src/tools/eval_recon.py:24-43 and the correspondence search of
 * its ICP alignment).  ref float64 [N,3], query float64 [M,3]; outputs dist float64 [M], idx int32 [M]:
 *   dist[m] = sqrt((dx*dx + dy*dy) + dz*dz) of the nearest reference point, float64 in this order, unfused -- the bits of
 *             numpy's np.sqrt(((q - r) ** 2).sum(-1)); among reference points at bit-equal distance the smallest index wins
 *   max_dist  a query with no reference point at distance < max_dist gets idx = -1 and dist = +inf (pass +inf for none)
 *   max_rings the query walks this many Chebyshev shells of a uniform cell grid over the reference (about 2 N cells, at
 *             most 2^24, counting-sorted on the device by the build call); queries still open after that are finished by a
 *             brute-force kernel (the reference through LDS, a workgroup per 256 queries).  0: brute force alone, the
 *             build call and both workspaces are not needed.  The result does not depend on max_rings.
 *   n_tail    device int32 [1] or NULL: the number of queries the brute-force kernel finished
 * The build call sorts `ref` into grid_workspace; any number of query calls with the same ref and n_ref may follow on the
 * same stream.  query_workspace is scratch of one query call.  Every call enqueues a fixed set of launches, whatever the
 * data, and never waits for the device.  Limits: N, M <= 2^26; beyond them, N = 0, a negative max_rings or a NaN max_dist:
 * ENSLAM_EINVAL.  M = 0 is valid (nothing is written but n_tail).  Coordinates must be finite (the caller checks). */
int enslam_nn_workspace(int64_t n_ref, int64_t n_query, int64_t *grid_bytes_host, int64_t *query_bytes_host);
int enslam_nn_build(const double *ref, int64_t n_ref, void *grid_workspace, void *stream);
int enslam_nn_query(const double *ref, int64_t n_ref, const double *query, int64_t n_query, double max_dist,
                    int32_t max_rings, void *grid_workspace, void *query_workspace, double *dist, int32_t *idx,
                    int32_t *n_tail, void *stream);

/* Depth images of a triangle mesh from K cameras (the off-screen depth renders of src/tools/eval_recon.py:131-210).
 * vertices float64 [V,3], faces int32 [F,3], w2c float64 [K,12] (the upper three rows of each world-to-camera matrix, the
 * convention of the visibility entry: the camera looks down -z); depth_out float32 [K,H,W].
 *   pixel (row j, column i) = the smallest camera-space depth t, z_near < t <= z_far, at which the ray through
 *   ((i - cx) / fx, -(j - cy) / fy, -1) meets a triangle; 0.0 where none does.  Both sides of a triangle count, edges are
 *   inclusive, degenerate triangles and triangles whose plane holds the camera centre hit nothing, a face with a vertex
 *   index outside [0, V) is dropped.  Float64 up to the rounding of t to float32.
 * The depths are combined by an integer minimum: the images are the same bits in every run and do not depend on how the
 * views are split over calls.  A fixed set of launches per call.  Limits: K*H*W <= 2^31 and F*K < 2^31
 * (ENSLAM_EUNSUPPORTED beyond); 0 <= z_near < z_far, finite intrinsics with fx, fy != 0 (ENSLAM_EINVAL otherwise).
 * F = 0 gives zero images, K = 0 is valid. */
int enslam_mesh_depth_workspace(int32_t n_faces, int32_t n_views, int64_t *bytes_host);
int enslam_mesh_depth(const double *vertices, int32_t n_verts, const int32_t *faces, int32_t n_faces, const double *w2c,
                      int32_t n_views, int32_t H, int32_t W, double fx, double fy, double cx, double cy, double z_near,
                      double z_far, void *workspace, float *depth_out, void *stream);

/* Colour images of a triangle mesh and a point set from K cameras: the headless renderer of the SLAM visualiser (the Open3D
 * window of src/tools/viz.py).  Conventions, arithmetic and limits of the triangle test are those of enslam_mesh_depth.
 *   vertices float64 [V,3], faces int32 [F,3]; vertex_colors uint8 [V,3] or NULL (0.7 grey); vertex_normals float64 [V,3] or
 *   NULL (the face normal; also used where the interpolated normal is zero); points float64 [P,3], point_colors uint8 [P,3];
 *   w2c float64 [K,12]; rgb_out uint8 [K,H,W,3]; depth_out float32 [K,H,W] or NULL (0 where empty); id_out int32 [K,H,W] or
 *   NULL (the face index, -2 - p for point p, -1 where empty).
 * Visibility: per pixel the primitive with the smallest (float32 depth, id), a face's id being its index and a point's
 * 0x80000000 | p -- an unsigned 64-bit integer minimum, so the images are the same bits in every run and do not depend on
 * how the views are split over calls.  cull: 0 both sides, 1 keeps triangles with det = a . (b x c) > 0 in camera space (the
 * stored normal (b - a) x (c - a) points away from the eye: what the reference shows after it reverses the faces and hides
 * back faces), 2 keeps det < 0.  A point of camera depth z = -p_z in (z_near, z_far] covers the point_size x point_size
 * pixels whose first column is ceil(u - point_size / 2) and first row ceil(w - point_size / 2), u = cx + fx p_x / z,
 * w = cy - fy p_y / z, at the constant depth z.  A face pixel is floor(255 c shade + 0.5) with c the barycentric mix of the
 * vertex colours / 255 and shade = ambient + (1 - ambient) |n^ . d^| (two-sided); a point pixel is the point's colour; an
 * empty pixel is `background` (r | g << 8 | b << 16).
 * workspace_bytes: at least 264 + 8 K H W rounded up to 256; what lies beyond holds the list of triangles whose pixel box
 * exceeds 256 pixels (8 bytes each, enslam_scene_raster_workspace gives room for all that can be used); a triangle that
 * finds the list full is rasterised by its own thread: the images do not depend on the size.
 * passes: 7 for an image.  The bits select the fill and the triangle pass (1), the point pass (2) and the resolve pass (4):
 * three calls with 1, 2 and 4 on one workspace give the image of one call with 7 (tools/bench_viz.py times them so).
 * A fixed set of launches per call.  Limits: K*H*W <= 2^31, F*K < 2^31, P*K < 2^31 (ENSLAM_EUNSUPPORTED beyond); 0 <= z_near
 * < z_far, finite intrinsics with fx, fy != 0, cull in 0..2, passes in 1..7, 1 <= point_size <= 64, 0 <= ambient <= 1 (ENSLAM_EINVAL
 * otherwise).  F = 0 and / or P = 0 are valid (the background shows), K = 0 is valid.
 *
 * enslam_scene_normals: Open3D's compute_vertex_normals.  vf_offsets int64 [V+1] and vf_faces int32 [n_incident] list, per
 * vertex, its incident faces; the unnormalised face normals (b - a) x (c - a) are summed in the order of the list (ascending
 * face index gives a result that is reproducible to the bit), then normalised; a zero sum stays zero.  normals_out float64
 * [V,3]. */
int enslam_scene_normals(const double *vertices, int32_t n_verts, const int32_t *faces, int32_t n_faces,
                         const int64_t *vf_offsets, const int32_t *vf_faces, int64_t n_incident, double *normals_out,
                         void *stream);
int enslam_scene_raster_workspace(int32_t n_faces, int32_t n_views, int32_t H, int32_t W, int64_t *bytes_host);
int enslam_scene_raster(const double *vertices, int32_t n_verts, const int32_t *faces, int32_t n_faces,
                        const uint8_t *vertex_colors, const double *vertex_normals, const double *points, int32_t n_points,
                        const uint8_t *point_colors, int32_t point_size, const double *w2c, int32_t n_views, int32_t H,
                        int32_t W, double fx, double fy, double cx, double cy, double z_near, double z_far, int32_t cull,
                        double ambient, uint32_t background, int32_t passes, void *workspace, int64_t workspace_bytes,
                        uint8_t *rgb_out, float *depth_out, int32_t *id_out, void *stream);

/* Frame preparation (the per-frame work of src/utils/datasets.py between the image decoders and the tracker): one launch
 * turns the raw decoded images of one frame into the tensors the readers hand out.
 *   color_raw  uint8 [h0,w0,C], C = 3 or C = 1 (grey, replicated to three channels)
 *   depth_raw  uint16 (depth_int32 = 0) or int32 (depth_int32 = 1) [H,W]
 *   event_raw  uint8 [he,we,3] or NULL (frame 0: all-zero events and mask)
 *   color_out  float64 [H',W',3]; depth_out float32 [H',W']; mask_out int64 [H',W'];
 *   event_out  [H',W',2] = (-, +): uint8 without crop_size, float32 with it; NULL (with mask_out NULL): no event outputs
 *   (H',W') = (crop_h, crop_w) when crop_h > 0, else (H, W), less crop_edge on every side.
 * Stages, in the order and precision of the host route (datasets.py):
 *   1 undistort (has_dist: colour; undistort_events: the event image too; never the depth): per destination pixel the
 *     inverse map of OpenCV's rational-radial + tangential model in float64, bilinear taps with a zero border in float64,
 *     one round-half-to-even to uint8
 *   2 colour / 255., then a half-pixel-centre bilinear resize to (H,W) in float64 when (h0,w0) differs
 *   3 events: the same resize from (he,we), rounded half-to-even to uint8
 *   4 crop_size: colour bilinear align_corners in float64, events the same in float32, depth torch's `nearest`
 *   5 the crop_edge cut
 *   6 depth = float32(raw) / float32(png_depth_scale) * float32(scale), two float32 operations
 *   7 mask = any event channel != 0
 * ev_neg / ev_pos: the channels of event_raw that hold the negative / positive events (1, 2 for Replica's (0,-,+) pngs,
 * 1, 0 for RPG's (+,-,0)).  ENSLAM_EINVAL without a launch: a NULL plan / colour / depth pointer, event_out without
 * mask_out (or the reverse), C not 1 or 3, a size < 1, an event channel outside 0..2, a crop_edge that leaves no pixel,
 * non-finite or zero intrinsics with has_dist, a png_depth_scale of 0.  More than 2^28 pixels in any image:
 * ENSLAM_EUNSUPPORTED. */
typedef struct enslam_frame_plan {
    int32_t h0, w0, channels;       /* raw colour image */
    int32_t he, we;                 /* raw event image (ignored when event_raw is NULL) */
    int32_t H, W;                   /* raw depth image */
    int32_t depth_int32;
    int32_t has_dist, undistort_events;
    int32_t crop_h, crop_w;         /* cam.crop_size, 0 0 for none */
    int32_t crop_edge;
    int32_t ev_neg, ev_pos;
    int32_t reserved;
    double fx, fy, cx, cy;
    double dist[8];                 /* k1 k2 p1 p2 k3 k4 k5 k6 */
    double png_depth_scale, scale;
} enslam_frame_plan;
int64_t enslam_frame_plan_bytes(void);               /* sizeof(enslam_frame_plan): binding self-check */
int enslam_frame_prepare(const enslam_frame_plan *plan, const uint8_t *color_raw, const void *depth_raw,
                         const uint8_t *event_raw, double *color_out, float *depth_out, void *event_out,
                         int64_t *mask_out, void *stream);

/* Block-sparse TSDF volume (Mesher.get_bound_from_frames, Mesher.py:214-279: Open3D's ScalableTSDFVolume.integrate and
 * extract_triangle_mesh; tsdf.py holds the arrays and does the allocation).
 *   units   16^3 voxels, anchored at the world origin: unit = floor(p / (16 * voxel_length)) per axis.  The block table
 *           (device int32 [nu0 * nu1 * nu2], z fastest, -1 = absent, otherwise a block id < n_blocks) covers the integer unit
 *           box [unit_lo, unit_lo + nu) (host int32 [3] each); at most 2^27 entries (ENSLAM_EUNSUPPORTED beyond).
 *   blocks  tsdf / weight float32 [n_blocks,4096], vcolor float32 [n_blocks,4096,3] or NULL, voxel (lx, ly, lz) of a block at
 *           (lx * 16 + ly) * 16 + lz.  0 < sdf_trunc <= 16 * voxel_length (ENSLAM_EINVAL otherwise).
 *   cam_host host float64 [4] = fx, fy, cx, cy; poses host float64 [12] = the rows of a [3,4] matrix, in the reference's camera
 *           axes (x right, y up, looking along -z).
 * enslam_tsdf_touch: for every pixel on rows / columns 0, stride, 2 stride, ... with depth > 0 (depth float32 [H,W]) the world
 *   point P = c2w . (depth * [(i - cx) / fx, -(j - cy) / fy, -1]) in float64, products summed left to right and the translation
 *   added last; stamps[unit] = stamp for every unit from floor((P - sdf_trunc) / L) to floor((P + sdf_trunc) / L) per axis,
 *   L = 16 * voxel_length (plain stores of one value).  Units outside the table are ignored; outside_partials (int32
 *   [ceil(ceil(H / stride) * ceil(W / stride) / 256)]) receives per workgroup the number of pixels that had one.
 * enslam_tsdf_integrate: Open3D's UniformTSDFVolume integration with the depth-to-distance multiplier, over the voxels of the
 *   n_touched blocks touched_block (ids) / touched_index (their table indices), every voxel evaluated on its own in float64
 *   (Open3D steps the camera point incrementally in float32):
 *     centre = (g + 0.5) * voxel_length, g the global integer voxel index; (x, y, z) = w2c . centre; zc = -z > 0 required;
 *     u_f = x * fx / zc + cx + 0.5, v_f = (-y) * fy / zc + cy + 0.5; inside iff 1e-4 <= u_f < W - 1e-4 (v likewise);
 *     (u, v) = trunc(u_f, v_f); d = depth[v,u] > 0 required; sdf = (d - zc) * mult[v,u] (mult float64 [H,W], the length of
 *     the pixel's un-normalised ray, made by the host); skipped if sdf <= -sdf_trunc; t = (float) min(1, sdf / sdf_trunc);
 *     float32: tsdf = (tsdf * w + t) / (w + 1), vcolor likewise from color[v,u] (float32 [H,W,3]; color and vcolor are both
 *     given or both NULL), w += 1.
 *   voxel_counts (int32 [n_touched * 16]) receives the number of voxels updated per (block, x slab).
 * Extraction (the pattern of enslam_marching_cubes_*): sorted_block / sorted_index int32 [n_blocks] are the block ids and
 *   their table indices in ascending table index.  A cell is the 8 voxels g + {0,1}^3, valid iff all lie in allocated blocks
 *   with weight > 0; a corner is "occupied" iff tsdf < 0 (zero level, normals towards positive tsdf).  A voxel owns its +x / +y /
 *   +z edges; an edge carries a vertex iff both ends have weight > 0 and different signs and one of the up to four cells sharing
 *   it is valid.  Vertex: centre(a) + t_a / (t_a - t_b) * voxel_length along the axis (float64); colour: the same interpolation
 *   of the two voxels' colours, clipped to [0, 1], floor(255 c + 0.5).  Order: blocks by table index, voxels in lattice order,
 *   edges x, y, z; faces by cell, then case-table order.  counts: device int32 [2] = vertices, triangles.  At most 100000
 *   blocks (ENSLAM_EUNSUPPORTED beyond).  colors uint8 [V,3] may be NULL. */
int enslam_tsdf_touch(const float *depth, int32_t H, int32_t W, int32_t stride, const double *cam_host, const double *c2w_host,
                      double sdf_trunc, double voxel_length, const int32_t *unit_lo_host, const int32_t *nu_host,
                      int32_t stamp, int32_t *stamps, int32_t *outside_partials, void *stream);
int enslam_tsdf_integrate(const float *depth, const float *color, const double *mult, int32_t H, int32_t W,
                          const double *cam_host, const double *w2c_host, double voxel_length, double sdf_trunc,
                          const int32_t *unit_lo_host, const int32_t *nu_host, int32_t n_touched, const int32_t *touched_block,
                          const int32_t *touched_index, int32_t n_blocks, float *tsdf, float *weight, float *vcolor,
                          int32_t *voxel_counts, void *stream);
int enslam_tsdf_mesh_workspace(int32_t n_blocks, int64_t *bytes_host);
int enslam_tsdf_mesh_count(const int32_t *table, const int32_t *nu_host, int32_t n_blocks, const int32_t *sorted_block,
                           const int32_t *sorted_index, const float *tsdf, const float *weight, void *workspace,
                           int32_t *counts, void *stream);
int enslam_tsdf_mesh_emit(const int32_t *table, const int32_t *unit_lo_host, const int32_t *nu_host, int32_t n_blocks,
                          const int32_t *sorted_block, const int32_t *sorted_index, const float *tsdf, const float *weight,
                          const float *vcolor, double voxel_length, void *workspace, int32_t n_verts, int32_t n_faces,
                          double *verts, int32_t *faces, uint8_t *colors, void *stream);

/* Hand-derived backward of enslam_render_fwd (replaces autograd of the reference ops).
 *   g_depth float64 [N], g_var float64 [N] or NULL, g_rgb float32 [N,3] or NULL
 *   grad_grids[k].data : voxel-major accumulators (caller-zeroed) or NULL to skip that grid
 *   grad_packed[k]     : packed-layout accumulators (caller-zeroed, enslam_packed_grad_floats) or NULL
 *   g_rays_o/g_rays_d  : float32 [N,3] accumulators (caller-zeroed) or NULL
 *   d_raw              : float32 [N*S,4] workspace
 * Gradients follow the reference's autograd exactly: none through the out-of-bound occupancy
 * overwrite (Renderer.py:58), none to grid_middle / positions through the fine decoder's
 * concatenated middle feature (decoder.py:184-186), none to z_vals. */
int enslam_render_bwd(int32_t stage, int32_t n_rays, int32_t n_samples, const float *rays_o, const float *rays_d,
                      const double *z_vals, const enslam_scene *scene, const float *raw, const double *depth,
                      const double *g_depth, const double *g_var, const float *g_rgb,
                      const enslam_grid *grad_grids, float *const *grad_packed, float *g_rays_o, float *g_rays_d,
                      float *d_raw, const float *act_ws, int32_t act_light, float *dgrid_ws, void *stream);

/* The mapper's RGB-D loss (Mapper.py:553-562:  sum_{gt_depth>0} |gt_depth - depth| + w_color * sum |gt_color - color|)
 * fused into the compositing launches of the render (two dependent launches fewer per optimisation step).
 * enslam_render_loss_fwd   : enslam_render_fwd that also ADDS the loss of this batch into loss[0] (float64, zero on
 *   entry; one atomic per 16 rays, so the last bits depend on the order).  gt_color NULL: depth term only.  Needs raw_out;
 *   ray counts above the tile-mode limit (full-image renders) return ENSLAM_EUNSUPPORTED.  d_raw_unit (optional,
 *   float32 [N*S,4]): d(loss)/d(raw) for g_loss = 1, so that the backward can start at enslam_decoder_bwd_scaled
 *   (d_raw = d_raw_unit, d_raw_scale = g_loss) without a compositing launch.
 * enslam_composite_loss_bwd: enslam_composite_bwd with d(depth), d(rgb) derived from that loss and the device scalar
 *   g_loss = d(total)/d(loss) instead of read from memory; follow with enslam_decoder_bwd.  gt_depth and g_loss are required,
 *   rgb (the forward's) when gt_color is given; the work list arguments are enslam_composite_bwd_list's.
 * enslam_render_fwd is enslam_render_loss_fwd without the loss arguments and the list; only there may raw_out be NULL. */
int enslam_render_loss_fwd(int32_t stage, int32_t n_rays, int32_t n_samples, const float *rays_o, const float *rays_d,
                           const double *z_vals, const enslam_scene *scene, double *depth, double *var, float *rgb,
                           float *raw_out, float *act_ws, int32_t act_light, const float *gt_depth,
                           const float *gt_color, float w_color, double *loss, float *d_raw_unit, int32_t *work_list,
                           int32_t *work_count, void *stream);
int enslam_composite_loss_bwd(int32_t n_rays, int32_t n_samples, const float *raw, const double *z_vals,
                              const double *depth, const float *rgb, const float *gt_depth, const float *gt_color,
                              float w_color, const double *g_loss, float *d_raw, int32_t *work_list, int32_t *work_count,
                              void *stream);

/* The two halves of enslam_render_bwd, callable on their own.
 * enslam_composite_bwd: backward of raw2outputs_nerf_color (common.py:284-296): d(depth,var,rgb) -> d_raw [N*S,4].
 * enslam_decoder_bwd  : everything upstream of raw (decoders, gather, points), consuming d_raw.  With act_ws and
 *   (from the size query above) it reads the saved activations and cell records and leaves what the ray gradients
 *   need in dgrid_ws: follow it with enslam_ray_grad_bwd (enslam_render_bwd does).  With act_ws given and dgrid_ws NULL
 *   the kernel computes the ray gradients itself at the end of each round (costs the kernel ~10 %; worth it when nothing
 *   else would need a launch after it, e.g. tracker iterations on a fixed map).  With act_ws NULL everything, ray
 *   gradients included, is recomputed in the one kernel.  In both of these cases enslam_ray_grad_bwd must not be called.
 * enslam_ray_grad_bwd : ray gradients of the saved-activation path (fp64 sample geometry, corner re-gather,
 *   coordinate gradient, per-ray reduction) from dgrid_ws, added into g_rays_o / g_rays_d. */
int enslam_composite_bwd(int32_t n_rays, int32_t n_samples, const float *raw, const double *z_vals,
                         const double *depth, const double *g_depth, const double *g_var, const float *g_rgb,
                         float *d_raw, void *stream);
int enslam_decoder_bwd(int32_t stage, int32_t n_rays, int32_t n_samples, const float *rays_o, const float *rays_d,
                       const double *z_vals, const enslam_scene *scene, const float *d_raw, const float *act_ws,
                       int32_t act_light, float *dgrid_ws, const enslam_grid *grad_grids, float *const *grad_packed,
                       float *g_rays_o, float *g_rays_d, void *stream);
/* enslam_decoder_bwd with every d_raw value multiplied by the device scalar *d_raw_scale (NULL: 1). */
int enslam_decoder_bwd_scaled(int32_t stage, int32_t n_rays, int32_t n_samples, const float *rays_o, const float *rays_d,
                              const double *z_vals, const enslam_scene *scene, const float *d_raw,
                              const double *d_raw_scale, const float *act_ws, int32_t act_light, float *dgrid_ws,
                              const enslam_grid *grad_grids, float *const *grad_packed, float *g_rays_o,
                              float *g_rays_d, const int32_t *work_list, const int32_t *work_count, void *stream);
/* enslam_decoder_bwd_scaled whose decoder-parameter gradients leave the kernel as per-workgroup PARTIAL IMAGES instead of
 * float atomics into grad_packed: grad_partial[k] (float32 [enslam_bwd_partial_floats(k)], need not be cleared; NULL: atomics as
 * before) receives a 16-float header (word 0, int32: number of rows) and one row of enslam_packed_grad_floats(k) floats per
 * workgroup of decoder k's role; enslam_step_finish_partials sums the rows while it unpacks.  grad_packed[k] must still be
 * given (it selects which decoders get parameter gradients) but is not written for those decoders.  All workgroups of the
 * persistent backward finish within microseconds of each other; their 17.6 MB of atomics onto the same 53 k addresses ran at
 * the chip-wide float-atomic rate (10-13 us at the tail of a 137 us kernel).  Replaces nothing in the reference (autograd
 * sums the weight gradients inside its mm kernels). */
size_t enslam_bwd_partial_floats(int kind);
int enslam_decoder_bwd_partials(int32_t stage, int32_t n_rays, int32_t n_samples, const float *rays_o, const float *rays_d,
                                const double *z_vals, const enslam_scene *scene, const float *d_raw,
                                const double *d_raw_scale, const float *act_ws, int32_t act_light, float *dgrid_ws,
                                const enslam_grid *grad_grids, float *const *grad_packed, float *const *grad_partial,
                                float *g_rays_o, float *g_rays_d, const int32_t *work_list, const int32_t *work_count,
                                void *stream);
/* Work list (optional everywhere, NULL/NULL = every tile): the 16-sample tiles (ray * n_samples/16 + tile) whose d_raw is
 * not all zero -- behind a converged surface the transmittance underflows to 0 and the far tiles of most rays carry no
 * gradient.  The kernel that produces d_raw appends them ray by ray (work_list int32 [n_rays * n_samples/16], work_count
 * int32 [1], ZERO on entry): enslam_render_loss_fwd (with d_raw_unit), enslam_composite_loss_bwd,
 * enslam_composite_bwd_list.  enslam_decoder_bwd_scaled (saved-activation roles only) and enslam_step_finish_rays then
 * walk the list instead of all tiles; both must be given the same list.  The list holds whole tiles only: with a work list
 * n_samples must be a multiple of 16 (ENSLAM_EINVAL otherwise; the samples past the last whole tile would never be listed).
 * Without a list the two compositing entries take every n_samples from 1 to 64.
 * enslam_composite_bwd is enslam_composite_bwd_list with work_list = work_count = NULL. */
int enslam_composite_bwd_list(int32_t n_rays, int32_t n_samples, const float *raw, const double *z_vals,
                              const double *depth, const double *g_depth, const double *g_var, const float *g_rgb,
                              float *d_raw, int32_t *work_list, int32_t *work_count, void *stream);
int enslam_ray_grad_bwd(int32_t stage, int32_t n_rays, int32_t n_samples, const float *rays_o, const float *rays_d,
                        const double *z_vals, const enslam_scene *scene, float *dgrid_ws, float *g_rays_o,
                        float *g_rays_d, void *stream);

/* raw2outputs_nerf_color (common.py:256-297, occupancy=True) on its own: raw float32 [N,S,4], z_vals float64 [N,S]
 * -> depth/var float64 [N], rgb float32 [N,3], weights float32 [N,S] (may be NULL).  1 <= S <= 64. */
int enslam_composite_fwd(int32_t n_rays, int32_t n_samples, const float *raw, const double *z_vals, double *depth,
                         double *var, float *rgb, float *weights, void *stream);

/* Mapper's RGB-D loss, Mapper.py:553-562:  sum_{gt_depth>0} |gt_depth - depth| + w_color * sum |gt_color - color|
 * (colour term only when color/gt_color are given, i.e. in the colour stage).  One kernel each way, deterministic
 * single-block reduction (n <= ray_batch_size).  loss: float64 [1]; g_loss: float64 [1] upstream gradient (device);
 * g_depth float64 [n], g_color float32 [n,3] (NULL when there is no colour term). */
int enslam_rgbd_loss_fwd(int32_t n, const double *depth, const float *color, const float *gt_depth,
                         const float *gt_color, float w_color, double *loss, void *stream);
int enslam_rgbd_loss_bwd(int32_t n, const double *depth, const float *color, const float *gt_depth,
                         const float *gt_color, float w_color, const double *g_loss, double *g_depth,
                         float *g_color, void *stream);

/* Parity helper: base voxel index and fractions the gather uses for points p float64 [P,3]
 * (normalize_3d_coordinate, common.py:342-357, then ATen grid_sampler unnormalize/clip/floor). */
int enslam_voxel_index(int64_t n_points, const double *points, const double *bound_host, int32_t D, int32_t H,
                       int32_t W, int32_t *ix, int32_t *iy, int32_t *iz, float *fx, float *fy, float *fz,
                       void *stream);

/* Parity helper: points p = o + d*z (float64 [N*S,3]) and the strict in-bound mask (uint8 [N*S]). */
int enslam_ray_points(int32_t n_rays, int32_t n_samples, const float *rays_o, const float *rays_d,
                      const double *z_vals, const double *bound_host, double *points, uint8_t *mask, void *stream);

/* Parity helper: the device sin / cos the Fourier embedding and its backward use (decoder.py:26-30: torch.sin of
 * p @ B in float32) on n float32 arguments; either output may be NULL. */
int enslam_fourier_sincos(int64_t n, const float *x, float *sin_out, float *cos_out, void *stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Step plans: one differentiable render call (Renderer.render_batch_ray, or render_batch_ray_rgbd_loss, and its backward)
 * as TWO calls of this library instead of the six to eight entry points above, with every buffer of the call a fixed
 * offset inside three caller-allocated blobs.  A Python host pays ~200 us per direction for marshalling ~180 pointers,
 * allocating ~25 tensors and laying out accumulators; with a plan it checks a cache key, allocates three blobs and makes one
 * call.  Replaces nothing in the reference (host glue); the launches are exactly those of the entry points above.
 *
 * enslam_step_plan describes what does not change between the steps of a loop (filled by the host once per combination of
 * stage / batch size / grid set / gradient pattern); enslam_step_layout is derived from it (enslam_plan_layout).
 *   grid_mode[k]  0: kind k unused by the stage
 *                 1: values given voxel-major ([V][32]: a channels_last_3d tensor or a cached copy), no gradient
 *                 2: values voxel-major, gradient wanted: added into the gradient blob's [V][32] region of kind k (zero-filled
 *                    by the forward), which the host hands to autograd as a channels_last_3d tensor
 *                 3: values channel-major ([32][V], the reference's strides), gradient wanted: touched 64-voxel blocks
 *                    converted per step (scratch blob), gradient transposed back into a dense [32][V] region of the gradient blob
 *   par_grad[k]   decoder k's parameters get gradients (all or none); they appear in the gradient blob's parameter region at the
 *                 float offsets pgrad_off[k][..] in the order W0,b0,..,W4,b4,Wc0,bc0,..,Wc4,bc4,Wo,bo,B
 *   loss_kind     0: outputs depth / var / rgb, backward from their gradients; 1: the mapper's RGB-D loss fused into the
 *                 compositing launches (enslam_render_loss_fwd), backward from d(total)/d(loss)
 * Blobs (device memory, 256-byte aligned, sizes from the layout): scratch (lives from forward to backward), grad (lives as long
 * as any gradient the host made from it), out (depth | var | rgb | loss).  Nothing needs clearing by the caller. */
typedef struct enslam_step_plan {
    int32_t stage, n_rays, n_lin, n_surf, lindisp, act_light, need_rays, use_work_list, loss_kind, use_color;
    float w_color;
    int32_t grid_mode[4], par_grad[4];
    int32_t grid_D[4], grid_H[4], grid_W[4];
    double bound[6], coarse_bound[6];
    enslam_mlp_params params[4];       /* the callers' parameter tensors (sources of the per-step packing) */
    int64_t pgrad_off[4][23];          /* float offsets inside the gradient blob's parameter region */
    int64_t pgrad_floats;              /* size of that region */
    const float *t_lin;                /* device: [n_lin] */
    const double *t_surf;              /* device: [n_surf] */
} enslam_step_plan;

typedef struct enslam_step_layout {    /* byte offsets (-1: absent) and sizes */
    int64_t scratch_bytes, grad_bytes, out_bytes;
    int64_t s_zero_bytes;              /* scratch [0, s_zero_bytes) is cleared by the forward: block flags, packed decoders */
    int64_t s_flags[4], s_packed[4], s_z, s_dmax, s_raw, s_act, s_work, s_draw, s_dgw, s_vm[4], s_gacc[4];
    int64_t g_flat, g_flat_floats;     /* grad blob: range the forward's prepare roles clear */
    int64_t g_packed[4], g_ro, g_rd, g_counter, g_nat[4], g_params, g_dense[4];
    int64_t o_depth, o_var, o_rgb, o_loss;
    int32_t n_samples, finish_needed, inline_rays, merged;
} enslam_step_layout;

int64_t enslam_plan_struct_bytes(int32_t which);       /* sizeof(enslam_step_plan) (0) / sizeof(enslam_step_layout) (1): binding self-check */
int enslam_plan_layout(const enslam_step_plan *plan, enslam_step_layout *layout);
/* grid_values[k]: the grid's values (voxel-major for modes 1 / 2, channel-major for mode 3).  gt_color: loss_kind 1 with colour term.
 * depth_max: device float32 [2] {max, max * 1.2f} of the whole batch or NULL (taken over this call's rays). */
int enslam_plan_forward(const enslam_step_plan *plan, const enslam_step_layout *layout, void *scratch, void *grad, void *out,
                        const float *rays_o, const float *rays_d, const float *gt_depth, const float *gt_color,
                        const float *depth_max, const float *const *grid_values, void *stream);
/* g_depth / g_var (float64 [N]) / g_rgb (float32 [N,3]): gradients of the outputs, any may be NULL (loss_kind 0);
 * g_loss: device float64 [1] (loss_kind 1). */
int enslam_plan_backward(const enslam_step_plan *plan, const enslam_step_layout *layout, void *scratch, void *grad, void *out,
                         const float *rays_o, const float *rays_d, const float *gt_depth, const float *gt_color,
                         const float *const *grid_values, const double *g_depth, const double *g_var, const float *g_rgb,
                         const double *g_loss, void *stream);

/* iMAP mode (configs/imap.yaml).  Decoder: src/conv_onet/models/decoder.py:91-203 with c_dim 0, hidden 256, 4 blocks, no
 * skips, colour output, fourier embedding; float32 throughout (f32-input MFMA).  Its 11 parameter tensors, float32
 * contiguous, in this order everywhere below (params / grads):
 *   embedder._B [3,93], pts_linears.{0..3}.{weight,bias} ([256,93] [256] then [256,256] [256] x 3),
 *   output_linear.{weight,bias} ([4,256] [4]).
 * enslam_imap_pack writes the forward's weight image (enslam_imap_packed_floats floats) from them; repack after every
 * parameter change.  enslam_imap_fwd: points float64 [P,3] (cast to float32 like the reference's p.float()) -> raw
 * float32 [P,4] = (r, g, b, sigma); bound_host (host float64 [3][2]) or NULL: points not strictly inside get sigma = 100
 * (Renderer.eval_points).  enslam_imap_bwd recomputes the forward into the workspace (enslam_imap_workspace_floats(P)
 * floats, device) and writes d_points float32 [P,3] and the 11 parameter gradients (accumulate != 0: added to what grads
 * hold).  The parameter gradients are per-slice partials summed in a fixed order: deterministic, no atomics. */
size_t enslam_imap_packed_floats(void);
size_t enslam_imap_workspace_floats(int64_t n_points);
int enslam_imap_pack(const float *const *params, float *packed, void *stream);
int enslam_imap_fwd(int64_t n_points, const double *points, const float *packed, const double *bound_host, float *raw,
                    void *stream);
int enslam_imap_bwd(int64_t n_points, const double *points, const float *const *params, const float *packed,
                    const double *bound_host, const float *d_raw, float *workspace, int32_t accumulate, float *const *grads,
                    float *d_points, void *stream);

/* raw2outputs_nerf_color (common.py:256-297, occupancy=False: volume density): raw float32 [N,S,4], z_vals float64 [N,S],
 * rays_d float32 [N,3] (dists are scaled by |rays_d|) -> depth/var float64 [N], rgb float32 [N,3], weights float32 [N,S]
 * (may be NULL).  The backward also returns d_rays_d float32 [N,3] (may be NULL), the gradient through |rays_d|; g_depth /
 * g_var / g_rgb may each be NULL.  1 <= S <= 64. */
int enslam_composite_density_fwd(int32_t n_rays, int32_t n_samples, const float *raw, const double *z_vals,
                                 const float *rays_d, double *depth, double *var, float *rgb, float *weights, void *stream);
int enslam_composite_density_bwd(int32_t n_rays, int32_t n_samples, const float *raw, const double *z_vals,
                                 const float *rays_d, const double *depth, const double *g_depth, const double *g_var,
                                 const float *g_rgb, float *d_raw, float *d_rays_d, void *stream);

/* Event network (event.py: UNet_2heads(6, 2, 2), bilinear=True, eval mode, frozen weights, batch 1, float32): forward and the
 * gradient with respect to the input image, reference event_net/unet_model.py:72-122 and unet_parts.py.  Conv + BatchNorm
 * pairs arrive folded (event.py: pack_event_net folds in float64 and rounds once).  Activations are channels-last
 * ([H*W][C]) inside; x / g_x are [6,H,W], events / probs and their gradients [2,H,W].  Deterministic: no atomics, partial
 * sums reduced in a fixed order.  H, W >= 16 (four poolings).
 *   packed     float32 [enslam_eventnet_pack_floats]: per convolution, in the order inc.{0,1}, down1..4.{0,1}, then per head
 *              up1..up4.{0,1} (26 in all):  Wf [9 cin][cout] (row = tap * cin + ci, tap = 3 ky + kx; the first layer's cin 6
 *              padded to 8 with zeros) | b [cout] | Wt [9 cout][cin] (row = tap * cout + co, holding w[8 - tap][ci][co]: the
 *              input gradient is the same kernel on it);  then the heads: W1 [2][64] | W2 [2][64] | b1 [2] | b2 [2] | pad to 264.
 *   workspace  float32 [enslam_eventnet_workspace_floats]: every saved activation, gradient scratch and split-reduction
 *              partials; the backward reads what the LAST forward on this workspace left.
 * The single-operation entries exist for the tests.  conv3x3: an H x W pixel grid; the "two-part side" has C0 channels at
 * [H*W][C0] and, with C1 > 0, C1 more at [H1*W1][C1] placed at offset (oy, ox) inside the grid (zero outside it); the
 * "single side" has Cn channels.  transposed == 0: out[H*W][Cn] = act(sum in[p + tap][c] w[tap (C0 + C1) + c][n] + bias[n])
 * with a0 / a1 the two inputs and d0 the output.  transposed != 0: a0 [H*W][Cn] is the incoming gradient, counted only where
 * a1 (same layout, may be NULL) is > 0; w is [9 Cn][C0 + C1]; channels [0, C0) go to d0, the rest to d1 [H1*W1][C1].  Every
 * channel count a multiple of 8, at most 1024 (else ENSLAM_EUNSUPPORTED); bias may be NULL.  scratch: 2^22 + H W N floats
 * (N the output channel count) always suffice.  pool2: nn.MaxPool2d(2) of in [H][W][C] -> out [H/2][W/2][C]; backward != 0:
 * out [H][W][C] = gradient of in from g_out [H/2][W/2][C] (first maximum in row-major order).  up2: x2 bilinear,
 * align_corners=True, in [h][w][C] -> out [2h][2w][C]; backward != 0: in is the gradient [2h][2w][C], out [h][w][C]. */
size_t enslam_eventnet_pack_floats(void);
size_t enslam_eventnet_workspace_floats(int32_t H, int32_t W);     /* 0: unsupported size */
int enslam_eventnet_forward(const float *packed, const float *x, int32_t H, int32_t W, float *workspace, float *events,
                            float *probs, void *stream);
int enslam_eventnet_backward(const float *packed, float *workspace, const float *g_events, const float *g_probs, float *g_x,
                             int32_t H, int32_t W, void *stream);
int enslam_eventnet_conv3x3(const float *w, const float *bias, int32_t H, int32_t W, int32_t C0, int32_t C1, int32_t H1,
                            int32_t W1, int32_t oy, int32_t ox, int32_t Cn, const float *a0, const float *a1, float *d0,
                            float *d1, int32_t relu, int32_t transposed, float *scratch, int64_t scratch_floats, void *stream);
int enslam_eventnet_pool2(const float *in, int32_t H, int32_t W, int32_t C, const float *g_out, float *out, int32_t backward,
                          void *stream);
int enslam_eventnet_up2(const float *in, int32_t h, int32_t w, int32_t C, float *out, int32_t backward, void *stream);

/* Training of the event network: the gradient of the packed image.  backward_weights does everything the backward entry above
 * does (g_x may be NULL: no input gradient is built) and writes g_packed, laid out like packed: the Wf and b blocks of every
 * convolution hold the gradients of the FOLDED weights and biases (relu'(0) = 0), the heads block those of W1 | W2 | b1 | b2;
 * every Wt block and the pad are written as zero (Wt is a copy of Wf: the caller's chain rule goes through Wf alone).  Each
 * weight gradient is an implicit GEMM over the pixels on the exact-f32 MFMA; layers with few weight tiles split the pixel
 * axis and the partials, kept in scratch [at least wgrad_scratch_floats(H, W)], are summed in split order: no atomics, two
 * runs are bit-equal.  The workspace is the forward's, unchanged in layout and size.  No allocation, no synchronisation.
 * heads_wgrad writes only the heads block's gradient [264] from the workspace of the last forward (scratch: as above).
 * conv3x3_wgrad is the single-operation entry for the tests, with the conventions of the conv3x3 entry: a0 [H*W][C0] and,
 * with C1 > 0, a1 [H1*W1][C1] at (oy, ox) are the convolution's input, g [H*W][Cn] the gradient of its output, counted only
 * where saved (same layout, may be NULL) is > 0;  dw [9 (C0 + C1)][Cn] (row = tap * (C0 + C1) + c), db [Cn] (may be NULL).
 * scratch: 2^22 floats always suffice. */
/* fold_pack builds the packed image on the device from live parameters, bit-equal to event.pack_event_net: params holds, per
 * convolution in packing order, five device addresses -- w float32 [cout][cin][3][3] (the first layer's cin is 6), BatchNorm
 * gamma and beta float32 [cout], sq = sqrt(var + eps) and shift = -mean float64 [cout], both computed on the host -- and then
 * the heads' W1, W2, b1, b2 (134 addresses).  Folding is float64 (s = gamma / sq, w s, beta + shift s), rounded once.
 * fold_pack_backward is its chain rule: from g_packed (Wf, b and heads blocks; Wt is not read) to grads, per convolution dw,
 * dgamma, dbeta (float32, shaped like the parameters, overwritten) and then the heads' four (82 addresses): dw = dWf s,
 * dgamma = (sum dWf w + shift db) / sq with the sum in float64 in a fixed order, dbeta = db.  scratch: float64 [26 * 16384].  Each is one launch over all 26 convolutions. */
int enslam_eventnet_fold_pack(const void *const *params, float *packed, void *stream);
int enslam_eventnet_fold_pack_backward(const void *const *params, const float *g_packed, void *const *grads, double *scratch,
                                       void *stream);
size_t enslam_eventnet_wgrad_scratch_floats(int32_t H, int32_t W);     /* 0: unsupported size */
int enslam_eventnet_backward_weights(const float *packed, float *workspace, const float *g_events, const float *g_probs,
                                     float *g_x, float *g_packed, float *scratch, int64_t scratch_floats, int32_t H, int32_t W,
                                     void *stream);
int enslam_eventnet_heads_wgrad(const float *workspace, const float *g_events, const float *g_probs, float *g_heads,
                                float *scratch, int64_t scratch_floats, int32_t H, int32_t W, void *stream);
int enslam_eventnet_conv3x3_wgrad(int32_t H, int32_t W, int32_t C0, int32_t C1, int32_t H1, int32_t W1, int32_t oy, int32_t ox,
                                  int32_t Cn, const float *a0, const float *a1, const float *g, const float *saved, float *dw,
                                  float *db, float *scratch, int64_t scratch_floats, void *stream);

/* Training-mode BatchNorm and batches for the event network (csrc/event_net.hip): the unfolded UNet_2heads(6, 2, 2) with
 * batch statistics in the forward, their terms in the backward and torch's running-statistics rule.  Activations are
 * channels-last [M][C] float32 with M = B H W rows (image-major); C a multiple of 8, at most 1024 (else ENSLAM_EUNSUPPORTED);
 * 2 <= M <= 2^24 (else ENSLAM_EINVAL: one row has no variance); activation pointers 16-byte aligned.  No atomics, no
 * allocation, no synchronisation; M is split into chunks of 256 rows whatever the device, every sum is float64 in a fixed
 * order (a thread's rows ascending, the 256 / min(C, 256) * 4 row sub-sets of a chunk ascending, the chunks ascending), so
 * two runs are bit-equal.
 *   bn_stats     mean [C], var [C] float64: per chunk of n_k rows  mean_k = (sum z) / n_k  and  M2_k = sum (z - mean_k)^2
 *                (z widened to float64 first), merged in chunk order with Chan's formula  delta = mean_k - mean,
 *                mean += delta n_k / n,  M2 += M2_k + delta^2 n_prev n_k / n;  var = M2 / M (biased).
 *                scratch: float64 [2 ceil(M / 256) C].
 *   bn_apply     per channel in float64  a = (double)gamma / sqrt(var + eps);  per element
 *                y = (float)(a * ((double)z - mean) + (double)beta),  then max(y, 0) when relu != 0: float64 operations, one
 *                rounding to float32.
 *   bn_backward  per channel  inv = 1 / sqrt(var + eps);  per element  gh = g_y where y > 0, else 0 (y NULL: gh = g_y) and
 *                xh = ((double)z - mean) * inv;  dbeta = sum gh,  dgamma = sum gh * xh  in float64, leaving as float32 [C];
 *                g_z = (float)(((double)gamma * inv) * ((gh - dbeta / M) - xh * (dgamma / M)))  with the float64 sums.
 *                g_z may be g_y itself.  scratch: float64 [2 ceil(M / 256) C + 2 C].
 *   bn_running   all 26 BatchNorms in one launch: buffers holds, per convolution in packing order, the device addresses of
 *                running_mean and running_var (float32 [cout], 52 addresses); batch_mean / batch_var float64 [5888] are the
 *                train_forward outputs (the layers' channels concatenated in packing order).  In float64, rounded once:
 *                running <- (1 - momentum) running + momentum batch, the variance unbiased (var M / (M - 1), M = B H_l W_l).
 * train_forward / train_backward run the whole net in training mode for a batch 1 <= B <= 8 (B H W <= 2^21, H, W >= 16 and
 * B (H / 16) (W / 16) >= 2, else ENSLAM_EINVAL: the bottom level would normalise one value per channel).
 *   params     per convolution in packing order three device addresses: w float32 [cout][cin][3][3] (the first cin is 6),
 *              gamma, beta float32 [cout]; then the heads' W1, W2, b1, b2 (82 addresses).  The weights are packed into the
 *              convolution kernels' layouts on the device, once per forward, inside the workspace.
 *   workspace  float32 [enslam_eventnet_bn_workspace_floats(B, H, W)] (0: unsupported): per convolution z and
 *              y = relu(bn(z)) [B H_l W_l][cout], the packed weights, the batch statistics, gradient and reduction scratch.
 *              The backward reads what the LAST forward on this workspace left, the packed weights included.
 *              enslam_eventnet_bn_saved_offset is the float offset of convolution `conv`'s y in it (-1: bad argument).
 *   forward    x [B,6,H,W] -> events, probs [B,2,H,W]; batch_mean, batch_var float64 [5888] for bn_running.
 *   backward   g_events, g_probs [B,2,H,W] -> g_x [B,6,H,W] (may be NULL) and grads: per convolution dw, dgamma, dbeta, then
 *              the heads' four (82 addresses, float32, shaped like the parameters, overwritten).  A NULL dw skips that
 *              convolution's weight gradient, a NULL dgamma / dbeta drops the value; the heads' four are all NULL or all
 *              given.  Per-image weight-gradient partials are summed in image order. */
int enslam_eventnet_bn_stats(const float *z, int64_t M, int32_t C, double *mean, double *var, double *scratch,
                             int64_t scratch_doubles, void *stream);
int enslam_eventnet_bn_apply(const float *z, const float *gamma, const float *beta, const double *mean, const double *var,
                             double eps, int64_t M, int32_t C, int32_t relu, float *y, void *stream);
int enslam_eventnet_bn_backward(const float *z, const float *y, const float *g_y, const float *gamma, const double *mean,
                                const double *var, double eps, int64_t M, int32_t C, float *g_z, float *dgamma, float *dbeta,
                                double *scratch, int64_t scratch_doubles, void *stream);
int enslam_eventnet_bn_running(void *const *buffers, const double *batch_mean, const double *batch_var, int32_t B, int32_t H,
                               int32_t W, double momentum, void *stream);
size_t enslam_eventnet_bn_workspace_floats(int32_t B, int32_t H, int32_t W);     /* 0: unsupported size */
int64_t enslam_eventnet_bn_saved_offset(int32_t B, int32_t H, int32_t W, int32_t conv);
int enslam_eventnet_train_forward(const void *const *params, const float *x, int32_t B, int32_t H, int32_t W, double eps,
                                  float *workspace, float *events, float *probs, double *batch_mean, double *batch_var,
                                  void *stream);
int enslam_eventnet_train_backward(const void *const *params, float *workspace, const float *g_events, const float *g_probs,
                                   int32_t B, int32_t H, int32_t W, double eps, float *g_x, void *const *grads, void *stream);

/* Event-camera simulator (event_sim.py, csrc/event_sim.hip): a contrast-threshold sensor in the style of ESIM / vid2e.
 * All arithmetic is float64.
 *   luminance  Y = (0.299 R + 0.587 G) + 0.114 B of values in [0, 1] (a grey image is its own Y); L = log(Y + eps)
 *   state      one reference level per pixel, L_ref float64 [H,W], updated in place and carried between intervals
 *   interval   visited at K sub-steps s = 1..K; at each, with d = L - L_ref:
 *                d >= C_pos:        n = floor(d / C_pos),  pos += n,  L_ref += n * C_pos
 *                else -d >= C_neg:  n = floor(-d / C_neg), neg += n,  L_ref -= n * C_neg
 *              (this closed form is the definition); the counts leave saturated at 255, L_ref moves by the unsaturated n
 *   output     events uint8 [H,W,2] = (-, +)
 *   thresholds the plan's scalars c_pos / c_neg, or per pixel where c_pos_map / c_neg_map (float64 [H,W]) are not NULL
 *   init       plan.init != 0: no events; L_ref := L of the last sub-step (the first frame of a sequence).  events may
 *              be NULL then and the thresholds are not looked at.
 * One thread per pixel, one launch, no atomics: the output is deterministic.
 *
 * enslam_event_sim_images: two decoded uint8 images prev, cur [H,W,channels] (channels 1 or 3); sub-step s sees
 *   L_a + (s / K) * (L_b - L_a), in this operation order.  L of a grey value comes from `lut` (device float64 [256], computed
 *   by the host: required for channels = 1); of an RGB pixel from the three bytes / 255. and the device's log.  With L_prev
 *   and L_cur (device float64 [H,W], both or neither) the images are not read (they may be NULL) and L_a, L_b are taken from
 *   there: host-computed levels, so that no device log decides a count.
 * enslam_event_sim_boxroom: the analytic room of synthetic.BoxRoom rendered inside the kernel at K poses (device float64
 *   [K,12]: the rows of c2w[:3,:4], interpolated by the host); per pose BoxRoom.render / intersect / color_at step by step:
 *   direction ((i - cx) / fx, -(j - cy) / fy, -1) rotated ((d0 R_c0 + d1 R_c1) + d2 R_c2), the |d| < 1e-12 clamp, wall exit
 *   and box entry parameters, hit point o + d * t, colour 0.5 + 0.45 sin(((p0 f_c0 + p1 f_c1) + p2 f_c2) + phase_c),
 *   luminance, log.  color_out (float64 [H,W,3]) and depth_out (float32 [H,W]), both or neither, receive the frame of the last
 *   pose.
 * ENSLAM_EINVAL without a launch: a NULL plan / L_ref, NULL events without init, events at an odd address, images route without a source of levels
 *   (channels = 1 without lut, NULL prev or cur without L_prev / L_cur, only one of L_prev / L_cur), channels not 1 or 3,
 *   NULL poses, only one of color_out / depth_out, H, W or K <= 0, eps, c_pos or c_neg (where no map replaces it) not a
 *   positive finite number, fx or fy zero or not finite.  K above enslam_event_sim_max_substeps (64) or more than 2^28 pixels:
 *   ENSLAM_EUNSUPPORTED. */
typedef struct enslam_event_sim_plan {
    int32_t H, W, K;
    int32_t channels;               /* images route: 1 or 3 */
    int32_t init;
    int32_t has_box;                /* boxroom route: the box stands in the room */
    double eps, c_pos, c_neg;
    double fx, fy, cx, cy;          /* boxroom route */
    double room_lo[3], room_hi[3], box_lo[3], box_hi[3];
    double freq[9];                 /* [channel][axis] */
    double phase[3];
} enslam_event_sim_plan;
int64_t enslam_event_sim_plan_bytes(void);           /* sizeof(enslam_event_sim_plan): binding self-check */
int enslam_event_sim_max_substeps(void);
int enslam_event_sim_images(const enslam_event_sim_plan *plan, const uint8_t *prev, const uint8_t *cur, const double *lut,
                            const double *L_prev, const double *L_cur, const double *c_pos_map, const double *c_neg_map,
                            double *L_ref, uint8_t *events, void *stream);
int enslam_event_sim_boxroom(const enslam_event_sim_plan *plan, const double *poses, const double *c_pos_map,
                             const double *c_neg_map, double *L_ref, uint8_t *events, double *color_out, float *depth_out,
                             void *stream);

/* Time-stamped event streams (event_stream.py, csrc/event_stream.hip): the simulator's events with time stamps, and the
 * accumulator that bins any stream into the count images above.  All arithmetic is float64, no fused multiply-adds.
 *
 * Stream: struct-of-arrays of N events -- t float64 seconds, x, y uint16, p uint8 (1 = positive).
 *
 * Model.  The sensor is the one above, unchanged: the counts and the new L_ref of an interval are those of its closed form.
 *   The interval [t_a, t_b] is visited at sub-steps s = 1..K.  At sub-step s let L_prev be the level seen at sub-step s - 1
 *   (for s = 1 the previous frame's level), L_s this sub-step's level and R the value of L_ref before the update.  When the
 *   pixel fires n events there, they are the events k = 1..n:
 *     X_k = R + k * C_pos for positive events, R - k * C_neg for negative ones (the product, then the sum)
 *     f_k = (X_k - L_prev) / (L_s - L_prev), then limited to [0, 1]: below 0 or not a number gives 0, above 1 gives 1
 *     t_k = t_a + (((s - 1) + f_k) / K) * (t_b - t_a), in exactly this operation order
 *   The limit is needed: rounding puts f a few 1e-16 outside [0, 1] at single events.  Images route: L_prev at s = 1 is L_a.
 *   Analytic route: `poses` has K + 1 rows, row 0 the previous frame's pose, which the kernel renders for L_prev only.
 *   Order of the output: pixel-major -- row-major pixels, time-ordered within a pixel (sub-step, then k).
 *
 * Two launches per interval, one thread per pixel, no atomics (bit-reproducible):
 *   enslam_event_stream_*_count: the arguments of enslam_event_sim_* without the outputs; counts (device int64 [H,W]) receives
 *     the unsaturated number of events per pixel (limited to 2^33 per pixel); L_ref is only read.  The boxroom entry takes
 *     the K sub-step poses [K,12] (as enslam_event_sim_boxroom).
 *   enslam_event_stream_*_emit: `ends` (device int64 [H,W]) is the INCLUSIVE prefix sum of `counts` in row-major order, `total`
 *     its last element, read back by the caller, = the capacity of t, x, y, p (which may be NULL when total = 0).  Writes every
 *     pixel's run at its offset, the saturated events image and the new L_ref -- both bit-equal to enslam_event_sim_*'s on
 *     the same inputs.  The boxroom entry takes K + 1 poses [K+1,12]; plan.K stays K.  No store leaves a pixel's own run or
 *     the capacity, whatever `ends` holds.
 *   ENSLAM_EINVAL without a launch: what enslam_event_sim_* refuses, plan.init != 0, NULL counts / ends, total < 0, a NULL
 *     stream array with total > 0, t_a or t_b not finite or t_b < t_a.  ENSLAM_EUNSUPPORTED: total above 2^31 - 1, H or W
 *     above 65536, and what enslam_event_sim_* does not support.
 *
 * enslam_event_accumulate: N events in any order into B time bins given by ascending edges [B+1] (equal neighbours make an
 *   empty bin; edges[0] may be -inf).  An event goes to bin b where edges[b] < t <= edges[b+1]: an event at a frame's own time
 *   belongs to the interval that ends there, as f = 1 does above.  Events with x >= W or y >= H are dropped and counted in
 *   dropped[1] (checked before any address is formed, and before the time is looked at); the others outside every bin (or
 *   with a t that is not a number) are dropped and counted in dropped[0].  p != 0 counts as positive.
 *   acc (device uint32 [B,H,W,2] = (-, +), 8-byte aligned) receives the unsaturated counts, counts (device uint8 [B,H,W,2],
 *   2-byte aligned) the counts saturated at 255, dropped (device uint64 [2]) the two counters; all three are overwritten.
 *   edges_host (host) is checked, edges (device, the same values) is what the kernel reads.  One thread per event, binary
 *   search of the edges (in LDS while B + 1 <= 2048), integer atomic adds: independent of the order of the events and
 *   bit-reproducible.  Two memsets and one launch when N = 0, two launches otherwise.
 *   ENSLAM_EINVAL without a launch: NULL edges_host, edges, acc, counts or dropped, N < 0, a NULL stream array with N > 0, B, H
 *   or W <= 0, misaligned acc / counts / dropped, edges that descend or hold a NaN.  ENSLAM_EUNSUPPORTED: N above 2^31 - 1 or
 *   B * H * W above 2^30 (the Python wrapper splits the bins). */
int enslam_event_stream_images_count(const enslam_event_sim_plan *plan, const uint8_t *prev, const uint8_t *cur,
                                     const double *lut, const double *L_prev, const double *L_cur, const double *c_pos_map,
                                     const double *c_neg_map, const double *L_ref, int64_t *counts, void *stream);
int enslam_event_stream_images_emit(const enslam_event_sim_plan *plan, const uint8_t *prev, const uint8_t *cur,
                                    const double *lut, const double *L_prev, const double *L_cur, const double *c_pos_map,
                                    const double *c_neg_map, double *L_ref, uint8_t *events, const int64_t *ends, int64_t total,
                                    double t_a, double t_b, double *t, uint16_t *x, uint16_t *y, uint8_t *p, void *stream);
int enslam_event_stream_boxroom_count(const enslam_event_sim_plan *plan, const double *poses, const double *c_pos_map,
                                      const double *c_neg_map, const double *L_ref, int64_t *counts, void *stream);
int enslam_event_stream_boxroom_emit(const enslam_event_sim_plan *plan, const double *poses, const double *c_pos_map,
                                     const double *c_neg_map, double *L_ref, uint8_t *events, const int64_t *ends, int64_t total,
                                     double t_a, double t_b, double *t, uint16_t *x, uint16_t *y, uint8_t *p, void *stream);
int enslam_event_accumulate(const double *t, const uint16_t *x, const uint16_t *y, const uint8_t *p, int64_t N,
                            const double *edges_host, const double *edges, int32_t B, int32_t H, int32_t W, uint32_t *acc,
                            uint8_t *counts, uint64_t *dropped, void *stream);

/* The noisy event sensor (event_sim.EventNoise, csrc/event_noise.hip): refractory period, leak and shot noise on top of the
 * sensor and the time stamps above.  All arithmetic is float64, no fused multiply-adds.
 *
 * State beside L_ref: t_last float64 [H,W], the time of the pixel's last emitted event; -inf after a reset.
 * Parameters (struct enslam_event_noise): refractory = rho >= 0 in seconds; leak = g = lambda * delta and shot = q = r * delta,
 *   the leak rate lambda (Hz) and the shot-noise rate r (Hz per pixel and polarity) times the length of a sub-step
 *   delta = (t_b - t_a) / K, computed by the host; seed; interval, the index of the interval since the reset, supplied by the
 *   caller (no generator state is stored).
 * Per pixel with flat index o = y W + x, at sub-step s = 1..K, in this order:
 *   1 leak (v2e's rule), if g > 0: L_ref = L_ref - g * C_pos (the product, then the difference).  Under constant light this
 *     yields positive events at lambda Hz.
 *   2 signal candidates, exactly the events of the stream model above: R = L_ref, the closed form moves L_ref and gives n
 *     candidates of one polarity with X_k, f_k limited to [0, 1] and t_k in the operation order stated there.
 *   3 shot-noise candidates, if q > 0: one Philox4x32-10 block (w0, w1, w2, w3) with key (seed & 0xffffffff, seed >> 32) and
 *     counter (o, interval, s, 0); multipliers D2511F53 / CD9E8D57, Weyl constants 9E3779B9 / BB67AE85.  With
 *     u(w) = (w + 0.5) * 2^-32 (exact): a negative candidate exists iff u(w0) < q, at f = u(w1); a positive one iff u(w2) < q,
 *     at f = u(w3); both at t = t_a + (((s - 1) + f) / K) * (t_b - t_a).  Noise candidates do not move L_ref.
 *   4 merge: the signal candidates in the order k = 1..n and the noise candidates in ascending t (on equal t the negative
 *     one first) are merged two-way: the next noise candidate leaves before the next signal candidate iff its t is smaller
 *     (on equal t signal comes first).  Signal times ascend with k wherever the level moves towards the crossing, so the
 *     merged order is ascending in t.
 *   5 refractory filter (ESIM's rule) in merged order: a candidate is emitted iff t - t_last >= rho (always for t_last = -inf)
 *     and then sets t_last = t.  A suppressed signal candidate has still moved L_ref.
 * Outputs: the uint8 (-, +) image of EMITTED events saturated at 255, L_ref, t_last, and the stream of emitted events
 * (pixel-major, merged order within a pixel).  With rho = g = q = 0 and frame times that do not go backwards the image, L_ref
 * and the stream equal those of enslam_event_stream_* bit for bit.
 * Limit of the device route: the walk over the candidates is serial, so a sub-step walks at most 65536 signal candidates of a
 * pixel (256 times what the uint8 image shows; a threshold that tiny against the level change is not a sensor).  A pixel beyond
 * that reports the count cap 2^33, so the emit entry's total refuses the interval; the count-image-only form has no count pass
 * and cannot report it: there L_ref stays the closed form's, the image and t_last are those of the candidates walked.
 * Not modelled: bandwidth-limited pixels, intensity-dependent noise rates, a reference level held in reset during the
 * refractory period.
 *
 * One thread per pixel, no atomics, no LDS (bit-reproducible):
 *   enslam_event_noisy_*_count: the arguments of enslam_event_stream_*_count, then noise, t_a, t_b and t_last; counts receives
 *     the emitted events per pixel; L_ref and t_last are only read.  The boxroom entry takes K + 1 poses [K+1,12] as its emit
 *     entry does: the refractory decision needs the time stamps, those the previous frame's level.
 *   enslam_event_noisy_*_emit: the arguments of enslam_event_stream_*_emit, then noise and t_last; writes the runs, the image,
 *     L_ref and t_last.  Count-image-only form: ends, t, x, y, p all NULL and total 0 -- one launch, no prefix sum, writes
 *     the image and the two states only.
 *   ENSLAM_EINVAL without a launch: what enslam_event_stream_* refuses, a NULL noise or t_last, refractory, leak or shot
 *     negative or not finite, shot > 1 (raise K), t_a or t_b not finite or t_b < t_a, only some of ends, t, x, y, p given (t, x,
 *     y, p may be NULL together beside ends while total = 0).  ENSLAM_EUNSUPPORTED as enslam_event_stream_*. */
typedef struct enslam_event_noise {
    double refractory;              /* rho, seconds */
    double leak;                    /* g = leak rate * sub-step length */
    double shot;                    /* q = shot rate * sub-step length, at most 1 */
    uint64_t seed;
    uint32_t interval, reserved;
} enslam_event_noise;
int64_t enslam_event_noise_bytes(void);              /* sizeof(enslam_event_noise): binding self-check */
int enslam_event_noisy_images_count(const enslam_event_sim_plan *plan, const uint8_t *prev, const uint8_t *cur,
                                    const double *lut, const double *L_prev, const double *L_cur, const double *c_pos_map,
                                    const double *c_neg_map, const double *L_ref, int64_t *counts,
                                    const enslam_event_noise *noise, double t_a, double t_b, const double *t_last, void *stream);
int enslam_event_noisy_images_emit(const enslam_event_sim_plan *plan, const uint8_t *prev, const uint8_t *cur,
                                   const double *lut, const double *L_prev, const double *L_cur, const double *c_pos_map,
                                   const double *c_neg_map, double *L_ref, uint8_t *events, const int64_t *ends, int64_t total,
                                   double t_a, double t_b, double *t, uint16_t *x, uint16_t *y, uint8_t *p,
                                   const enslam_event_noise *noise, double *t_last, void *stream);
int enslam_event_noisy_boxroom_count(const enslam_event_sim_plan *plan, const double *poses, const double *c_pos_map,
                                     const double *c_neg_map, const double *L_ref, int64_t *counts,
                                     const enslam_event_noise *noise, double t_a, double t_b, const double *t_last, void *stream);
int enslam_event_noisy_boxroom_emit(const enslam_event_sim_plan *plan, const double *poses, const double *c_pos_map,
                                    const double *c_neg_map, double *L_ref, uint8_t *events, const int64_t *ends, int64_t total,
                                    double t_a, double t_b, double *t, uint16_t *x, uint16_t *y, uint8_t *p,
                                    const enslam_event_noise *noise, double *t_last, void *stream);

/* Event-stream denoising (event_filter.py, csrc/event_filter.hip): hot-pixel mask, refractory filter and background-activity
 * (neighbour-support) filter between a stream and the accumulator above.  All arithmetic is float64 comparisons and one
 * float64 subtraction: every result is exact, and the same on every route.
 *
 * Stream: the struct-of-arrays above (t float64, x, y uint16, p uint8), N events i = 0..N-1 in stream order.  Sensor H x W,
 *   flat index o = y W + x.
 * State, carried between calls, all -inf after a reset:
 *   t_last float64 [H,W]  the time of the pixel's last event that passed the refractory stage (the simulator's t_last)
 *   t_seen float64 [H,W]  the largest time of the pixel's events that passed stages 0 and 1
 * Parameters: rho >= 0, the refractory period in seconds; support on or off with dt >= 0, the support window in seconds
 *   (dt = 0 is meaningful: only equal-time neighbours support); optionally hot_mask uint8 [H,W].
 *
 * One call filters one chunk.  Every event gets exactly one class, the first that applies (ENSLAM_EVENT_* below, 0 = kept):
 *   Stage 0, classification.  SENSOR: x >= W or y >= H, decided before any address is formed and before the time is looked
 *     at.  TIME: t is not finite (NaN, +inf, -inf).  HOT: hot_mask[o] != 0.  Otherwise the event is live.
 *   Stage 1, refractory (ESIM's rule, the noisy sensor's expression).  The live events of a pixel are taken in the order of
 *     (t, i): time first, stream position on equal times.  An event passes iff t - t_last[o] >= rho (with t_last = -inf the
 *     difference is +inf: it passes) and then sets t_last[o] = t; otherwise its class is REFRACTORY.  Polarity plays no part.
 *     With rho = 0 the stage removes nothing and still maintains t_last.  The events that passed are called S.
 *   Stage 2, support (non-recursive background-activity filter), only when support is on.  An S-event at (x, y, t) is kept iff
 *     a supporting time t' exists for one of the up to eight pixels (x + dx, y + dy), (dx, dy) != (0, 0), that lie inside the
 *     sensor: t' <= t and t - t' <= dt, evaluated exactly so, where t' is the time of an S-event of that neighbour in this
 *     chunk or the carried t_seen of that neighbour (the value before this call).  Without such a t' the class is UNSUPPORTED.
 *     Equal-time neighbours support each other.  HOT, REFRACTORY, SENSOR and TIME events support nobody.  An S-event that
 *     ends up UNSUPPORTED still supports others (the classical filter writes every event's time stamp; it also keeps the
 *     stage parallel).  A pixel never supports itself.  Neighbours are spatial: (W-1, y) and (0, y+1) are adjacent in memory
 *     and are NOT neighbours.  t - t' is monotone in t', so only the largest t' <= t of each neighbour needs the test: one
 *     binary search per neighbour.
 *   Afterwards t_seen[o] = max(t_seen[o], the largest S time at o).
 * Output: the events of class 0 in stream order (the input arrays are untouched), the class array uint8 [N], and the counters
 *   n_in, sensor, time, hot, refractory, unsupported, n_out.
 * Chunks.  PRECONDITION: successive calls ascend in time -- the smallest live time of a chunk is >= the largest live time of
 *   all chunks since the reset (event_filter.EventFilter checks it and refuses).  The support kernel still tests
 *   t_seen <= t, so a violation has a defined, memory-safe result.  A stream filtered in several chunks gives exactly the
 *   one-call result whenever no time value is shared across a chunk boundary.  The one exception: an event at exactly the
 *   boundary time in the earlier chunk whose only support would be an equal-time event of the later chunk is UNSUPPORTED
 *   (the later one is supported by it, through t_seen).
 * Hot pixels are learned separately: counts[o] is the number of events of the pixel that are neither SENSOR nor TIME
 *   (integer atomics: independent of the order), and a pixel is hot iff counts[o] > max_events.
 *
 * Ordering is the caller's (torch.sort(stable=True) and torch.cumsum in functional.event_filter): `order` (device int32
 *   [n_live]) lists the live events by (o, t, i) and `starts` (device int64 [H W + 1]) is the exclusive prefix sum of the live
 *   events per pixel, so pixel o owns order[starts[o] .. starts[o+1]).  The entries are memory-safe whatever the two hold: an
 *   index outside [0, N), or of an event that is not live or not of that pixel, is skipped; run bounds are clamped to
 *   [0, n_live]; no load or store leaves an array.
 *
 * enslam_event_pixel_counts: stage 0.  One thread per event.  cls (device uint8 [N]) receives the class, pix (device int32 [N])
 *   the flat index o (-1 for SENSOR), counts (device int32 [H,W], zeroed here) the counts above, flags (device uint32 [1],
 *   zeroed here) the bits ENSLAM_EVENT_NOT_TIME_ORDERED -- some live t is smaller than the previous live event's -- and
 *   ENSLAM_EVENT_NOT_PIXEL_MAJOR -- some live (o, t) is lexicographically smaller than the previous live event's; the
 *   simulator emits pixel-major streams.  A live event separated from the previous live one by more than 32 events that are
 *   not live sets both bits (a clear bit always guarantees the order; a set bit only costs a sort).  hot_mask may be NULL: the
 *   same entry serves hot-pixel learning.  Two memsets, and one launch when N > 0.
 * enslam_event_filter_walk: stage 1.  One thread per pixel over its run, linear in the run.  Writes REFRACTORY into cls,
 *   t_last, and the workspace of stage 2: s_times (device float64 [n_live]) and s_event (device int32 [n_live]) hold the times
 *   and stream positions of the pixel's S-events compactly at the front of its run (unused slots of s_event are -1), s_count
 *   (device int32 [H,W]) their number.  One memset and one launch.
 * enslam_event_filter_support: stage 2 when `support` != 0 -- one thread per S-event, up to eight binary searches in the
 *   neighbours' compact runs, then the neighbours' t_seen; writes UNSUPPORTED into cls -- and then, in a launch of its own so
 *   that stage 2 reads the old values, the update of t_seen.  Call it with support = 0 as well: the state needs it.
 * enslam_event_filter_compact: `ends` (device int64 [N]) is the INCLUSIVE prefix sum of (cls == 0) in stream order and n_out
 *   its last element, the capacity of the outputs (which may be NULL when n_out = 0).  One thread per event; a kept event
 *   goes to slot ends[i] - 1, a slot outside [0, n_out) is skipped.  No launch when N = 0 or n_out = 0.
 * No float atomics anywhere: two runs give the same bits.
 * ENSLAM_EINVAL without a launch: a NULL counts, flags, starts, t_last, t_seen or s_count; N < 0; a NULL stream array, cls,
 *   pix or ends with N > 0; a NULL order, s_times or s_event with n_live > 0; a NULL output with n_out > 0; n_live or n_out
 *   outside [0, N]; H or W <= 0; rho or dt negative or not finite; an array not aligned to its element size.
 *   ENSLAM_EUNSUPPORTED: N above 2^31 - 1, H or W above 65536, more than 2^28 pixels. */
#define ENSLAM_EVENT_KEPT 0
#define ENSLAM_EVENT_SENSOR 1
#define ENSLAM_EVENT_TIME 2
#define ENSLAM_EVENT_HOT 3
#define ENSLAM_EVENT_REFRACTORY 4
#define ENSLAM_EVENT_UNSUPPORTED 5
#define ENSLAM_EVENT_NOT_TIME_ORDERED 1u
#define ENSLAM_EVENT_NOT_PIXEL_MAJOR 2u
int enslam_event_pixel_counts(const double *t, const uint16_t *x, const uint16_t *y, int64_t N, int32_t H, int32_t W,
                              const uint8_t *hot_mask, uint8_t *cls, int32_t *pix, int32_t *counts, uint32_t *flags,
                              void *stream);
int enslam_event_filter_walk(const double *t, int64_t N, int32_t H, int32_t W, double rho, const int32_t *pix,
                             const int32_t *order, int64_t n_live, const int64_t *starts, uint8_t *cls, double *t_last,
                             double *s_times, int32_t *s_event, int32_t *s_count, void *stream);
int enslam_event_filter_support(int64_t N, int32_t H, int32_t W, int32_t support, double dt, const int32_t *pix,
                                int64_t n_live, const int64_t *starts, uint8_t *cls, const double *t_last, double *t_seen,
                                const double *s_times, const int32_t *s_event, const int32_t *s_count, void *stream);
int enslam_event_filter_compact(const double *t, const uint16_t *x, const uint16_t *y, const uint8_t *p, int64_t N,
                                const uint8_t *cls, const int64_t *ends, int64_t n_out, double *t_out, uint16_t *x_out,
                                uint16_t *y_out, uint8_t *p_out, void *stream);

/* Per-iteration frame report (frame_vis.py, csrc/frame_report.hip): the figure of the reference's src/utils/Visualizer.py
 * as one uint8 sheet, the frame's error sums, and the mean SSIM of two images.
 *
 * enslam_vis_panels: inputs gt_depth, depth float32 [H,W], gt_color, color float32 [H,W,3] and, both or neither, gt_event,
 *   pred_event float32 [h,w,2] at their own resolution.  sheet uint8 [R H + (R + 1) g + R t, 3 W + 4 g, 3] with R = 2 rows of
 *   panels without events and 3 with them, g = gutter and t = title: panel (r, c) starts at row g + t + r (H + g + t) and
 *   column g + c (W + g); gutters and the title strip above each panel are 255 (the host draws the titles after the download).
 *   Columns are input, generated, residual; rows depth, colour, events.  Every rule is float32 with separate operations:
 *     max_depth  the maximum of gt_depth (a NaN is skipped), reduced on the device first
 *     depth      max_depth == 0: entry 0 of the table; else u = v / max_depth: NaN white, u < 0 entry 0, u >= 1 entry 255,
 *                else entry (int)(u * 256.0f) of the 256-entry plasma table (csrc/plasma_lut.hpp); the residual is
 *                |gt - pred|, 0 where gt_depth == 0, against the same max_depth
 *     colour     c' = c > 0 ? c : 0, then c' < 1 ? c' : 1 (a NaN gives 0), level (uint8)(c' * 255.0f + 0.5f); the residual is
 *                |gt - pred| per channel, 0 where gt_depth == 0, then the same
 *     events     channels (e0, e1, 0), level (uint8) of e * 50.0f limited to [0, 255] the same way; panel pixel (y, x) shows
 *                source pixel ((2 y + 1) h / (2 H), (2 x + 1) w / (2 W)) in integer arithmetic; the residual is |a - b| of the
 *                two levels (the reference subtracts the uint8 arrays, which wraps)
 *   stats (device float64 [8]): {n, L, S, Sv, n, L, S, Sv} with n the number of pixels with gt_depth > 0, L the sum over
 *   them of |gt_depth - depth| (float32, added in float64), S the sum over all pixels and channels of (c'(gt) - c'(pred))^2
 *   (the difference float32, squared and added in float64), Sv the same over the gt_depth > 0 pixels; the second four are
 *   the sums of the absolute values of the terms (all terms are non-negative, so they repeat the first four).  Sums are per
 *   workgroup, then over the workgroups in index order: no float atomics, the same bits in every run.
 *   workspace: enslam_vis_panels_workspace bytes, 8-byte aligned; sheet 4-byte aligned.  Three launches.
 *   ENSLAM_EINVAL without a launch: a NULL pointer where data is required, only one of the event images, H, W <= 0 (h, w
 *   with events), negative gutter or title, a workspace too small or misaligned.  More than 2^31 sheet pixels:
 *   ENSLAM_EUNSUPPORTED.
 *
 * enslam_ssim: mean structural similarity (Wang et al. 2004) of x, y float32 [H,W,C], C 1 or 3, data range 1: 11 x 11
 *   normalised Gaussian window of sigma 1.5 (the outer product of the normalised 11-tap window), K1 = 0.01, K2 = 0.03,
 *   population covariance, the mean over the (H - 10) x (W - 10) interior and the channels.  The five windowed moments are
 *   float64.  One workgroup per ENSLAM_SSIM_TILE_H x ENSLAM_SSIM_TILE_W tile of the interior and channel; mean_out (device
 *   float64 [1]) is the sum of the per-workgroup sums in index order, divided by the count; map_out (device float64
 *   [H-10,W-10,C]) may be NULL.  workspace: enslam_ssim_workspace bytes, 8-byte aligned.  Two launches.
 *   ENSLAM_EINVAL without a launch: NULL x, y, workspace or mean_out, H or W < 11, C not 1 or 3, a workspace too small.
 *   More than 2^28 pixels: ENSLAM_EUNSUPPORTED. */
#define ENSLAM_SSIM_TILE_H 16
#define ENSLAM_SSIM_TILE_W 32
int enslam_vis_panels_workspace(int32_t H, int32_t W, int32_t rows, int32_t gutter, int32_t title, int64_t *bytes_host);
int enslam_vis_panels(const float *gt_depth, const float *gt_color, const float *depth, const float *color,
                      const float *gt_event, const float *pred_event, int32_t H, int32_t W, int32_t h, int32_t w,
                      int32_t gutter, int32_t title, void *workspace, int64_t workspace_bytes, uint8_t *sheet, double *stats,
                      void *stream);
int enslam_ssim_workspace(int32_t H, int32_t W, int32_t C, int64_t *bytes_host);
int enslam_ssim(const float *x, const float *y, int32_t H, int32_t W, int32_t C, void *workspace, int64_t workspace_bytes,
                double *mean_out, double *map_out, void *stream);

/* Event-generation-model loss (event_model.py, csrc/event_model.hip): the tracker's event term without a network.  The
 * event image between the previous colour frame and the colour rendered at the pose under optimisation is predicted with
 * the contrast-threshold model of event_sim.py and compared with the recorded one.
 *
 * Inputs at the event resolution: cur float32 [h,w,3] (the rendered colour, carries the gradient), prev float32 [h,w,3],
 * gt float32 [h,w,2] with channels (-, +).  Scalars c_neg, c_pos, eps > 0; K <= ENSLAM_EVENT_MODEL_MAX_KERNELS Gaussian
 * kernels of odd size k_i <= ENSLAM_EVENT_MODEL_MAX_KSIZE with weight w_i.  ksizes (int32 [K]), weights (float32 [K]) and
 * taps (float32 [K][ENSLAM_EVENT_MODEL_MAX_KSIZE], row i holds the k_i taps of kernel i from its first column) are HOST
 * arrays, copied into the launch: the taps are event.gaussian_kernel1d's own numbers.  Per pixel, float32, every
 * operation on its own (no contraction):
 *     Y(a)   = max((0.299 a_R + 0.587 a_G) + 0.114 a_B, 0)
 *     d      = log(Y(cur) + eps) - log(Y(prev) + eps)
 *     pred_- = max(-d, 0) / c_neg,   pred_+ = max(d, 0) / c_pos          (d == 0: both 0, gradient 0)
 *     r      = pred - gt
 *     loss   = sum r^2 + sum_i w_i sum (B_i r)^2
 * B_i is the separable Gaussian blur with reflect padding, per channel (event.gaussian_blur): rows first, then columns.
 * Gradient: dloss/dr = 2 r + sum_i 2 w_i B_i^T B_i r with B^T the adjoint of the reflect-padded blur (a pixel p within
 * k / 2 of a border also receives what was reflected onto it: in one dimension of length n, with C the zero-padded
 * correlation of the taps, (B^T v)[p] = C(p) + [1 <= p <= k/2] C(-p) + [n - 1 - k/2 <= p <= n - 2] C(2 (n - 1) - p));
 * d pred_+ / d cur_ch = [d > 0] w_ch / (c_pos (Y(cur) + eps)), d pred_- / d cur_ch = -[d < 0] w_ch / (c_neg (Y(cur) + eps)),
 * zero where the luminance of cur was clamped (below 0).  The two max() are torch.clamp(min=0): a NaN goes through them, so a
 * colour that is not a number gives a NaN prediction, a NaN loss and a NaN gradient at that pixel, never a finite loss.
 *
 * Outputs: pred float32 [h,w,2]; sums float64 [K + 2] = the raw term sum r^2, the K blurred terms sum (B_i r)^2, then the
 * loss; grad float32 [h,w,3] = dloss/dcur; and, both or neither, blur_gt and blur_pred float32 [K,h,w,2] = B_i gt, B_i pred.
 * One workgroup per ENSLAM_EVENT_MODEL_TILE x ENSLAM_EVENT_MODEL_TILE tile and channel stages r with a halo of 2 (k_max / 2)
 * in LDS and runs the four passes out of it; squares are added in float64 per workgroup, then over the workgroups in index
 * order by a second launch: no float atomics, no fences, the same bits in every run.  workspace: enslam_event_model_workspace
 * bytes, 8-byte aligned.  Two launches, no host synchronisation: safe inside a stream capture.
 * ENSLAM_EINVAL without a launch: a NULL pointer where data is required (K > 0: ksizes, weights, taps), only one of the
 * blurred outputs, h or w <= 0, K < 0, a k that is even or <= 0, k / 2 >= min(h, w) (reflect padding is undefined), c_neg,
 * c_pos or eps not > 0 (a NaN included), a workspace too small or misaligned.  ENSLAM_EUNSUPPORTED without a launch:
 * K > ENSLAM_EVENT_MODEL_MAX_KERNELS, k > ENSLAM_EVENT_MODEL_MAX_KSIZE, h or w above 32768, more than 2^28 pixels. */
#define ENSLAM_EVENT_MODEL_TILE 16
#define ENSLAM_EVENT_MODEL_MAX_KERNELS 4
#define ENSLAM_EVENT_MODEL_MAX_KSIZE 31
int enslam_event_model_workspace(int32_t h, int32_t w, int32_t K, int64_t *bytes_host);
int enslam_event_model_loss(const float *cur, const float *prev, const float *gt, int32_t h, int32_t w, float c_neg,
                            float c_pos, float eps, int32_t K, const int32_t *ksizes, const float *weights,
                            const float *taps, void *workspace, int64_t workspace_bytes, float *pred, double *sums,
                            float *grad, float *blur_gt, float *blur_pred, void *stream);

/* Event motion compensation by contrast maximisation (event_cmax.py, csrc/event_cmax.hip; Gallego et al., CVPR 2018): every
 * event of a stream is warped along a candidate motion theta to the reference time t_ref and voted into an image of warped
 * events (IWE); the objective is the variance of the blurred IWE, returned with its gradient in theta.
 *
 * Stream: t float64 [N], x, y uint16 [N], p uint8 [N] on the device, in any order.  Pinhole intrinsics fx, fy, cx, cy (x
 * right, y down, z forward).  theta_host is a HOST float64 [P] array, P = 2 for ENSLAM_CMAX_FLOW, 3 for ENSLAM_CMAX_ROTATION.
 * ALL arithmetic is float64 and every operation stands on its own (no contraction), in exactly this order, with xd, yd the
 * event's x, y as float64:
 *     u  = (xd - cx) / fx                   v  = (yd - cy) / fy                  dt = t - t_ref
 *     FLOW      Bu = (1 / fx, 0)            Bv = (0, 1 / fy)
 *               du = theta0 / fx            dv = theta1 / fy                                       (pixels per second)
 *     ROTATION  uv = u * v                  pu = 1 + u * u                       pv = 1 + v * v
 *               Bu = (uv, -pu, v)           Bv = (pv, -uv, -u)
 *               du = (uv * w_x - pu * w_y) + v * w_z          dv = (pv * w_x - uv * w_y) - u * w_z   (theta = w, rad / s)
 *     mx = -(dt * fx)                       my = -(dt * fy)
 *     x' = xd + mx * du                     y' = yd + my * dv
 * Checks, in this order, each with its counter in dropped uint64 [3]: x >= W or y >= H -> dropped[1] (before the time is
 * looked at, as enslam_event_accumulate does); t not finite -> dropped[0]; then, in float64 and BEFORE any conversion to an
 * integer, x' > -1 && x' < W && y' > -1 && y' < H, else -> dropped[2] (no corner inside the image; a NaN fails).  No address
 * is formed from an unchecked value.
 * Vote: x0 = floor(x'), a = x' - x0, oa = 1 - a, likewise y0, b, ob.  Corners c = 0..3 at (x0, y0), (x0 + 1, y0),
 * (x0, y0 + 1), (x0 + 1, y0 + 1) with weights w_c = oa * ob, a * ob, oa * b, a * b; a corner outside [0, W) x [0, H) is
 * skipped.  q_c = llrint(w_c * 2^32), negated when sign_votes != 0 and p == 0, is added to iwe int64 [H,W] with 64-bit
 * integer atomics: integer sums do not depend on arrival order (the IWE is bit-reproducible) and N <= 2^31 - 1 votes of
 * weight <= 1 cannot overflow.  I = (float64)iwe * 2^-32.
 * Objective: J = G I, the separable Gaussian blur with ZERO padding, rows first then columns:
 *     r[y][x] = sum_{i = 0..k-1, ascending, from 0.0} taps[i] * I[y][x - k/2 + i]        (0.0 outside the image)
 *     J[y][x] = sum_{i = 0..k-1, ascending, from 0.0} taps[i] * r[y - k/2 + i][x]
 * taps_host is a HOST float64 [k] array (event.gaussian_kernel1d's own numbers), k odd, k <= ENSLAM_CMAX_MAX_KSIZE; k = 1
 * with tap 1 is no blur.  mu = SUM(J) / (H W), f = SUM((J - mu) * (J - mu)) / (H W) over the row-major pixels.
 * Gradient (want_grad != 0): D = G (J - mu) (zero padding makes the blur its own adjoint).  Per event that voted, with
 * dwx_c = -ob, ob, -b, b and dwy_c = -oa, -a, oa, a:
 *     Gx = sum over the corners inside, c ascending, from 0.0, of D_c * dwx_c;      Gy likewise with dwy_c
 *     g_k = s * (Gx * (mx * Bu_k) + Gy * (my * Bv_k)),   s = -1 for a negated vote, else 1;   g_k = 0.0 for a dropped event
 *     df / dtheta_k = (2 / (H W)) * SUM(g_k) over the events in stream order.
 * SUM, the one order of every float64 sum here: the elements in consecutive blocks of 256, the last block padded with 0.0;
 * each block reduced by the halving tree v[i] += v[i + s] for s = 128, 64, .. 1; the block results reduced 256 at a time by
 * the same tree; what is then left (one value per 65536 elements) added in ascending order from 0.0.  No float atomics.
 *
 * Outputs: iwe; blurred float64 [H,W] = J, or NULL; stats float64 [2 + P] = (mu, f, df/dtheta..., the latter 0.0 without
 * want_grad); dropped.  workspace: enslam_event_cmax_workspace bytes, 8-byte aligned.  A fixed set of launches on the stream
 * (the outputs are zeroed by a kernel, not by memsets), no host synchronisation: safe inside a stream capture, replayed any
 * number of times.  Inputs are only read.
 * ENSLAM_EINVAL without a launch: a NULL theta_host, taps_host, workspace, iwe, stats or dropped; a NULL stream array with
 * N > 0; N < 0; H or W <= 0; a non-finite theta, t_ref or intrinsic; fx or fy equal to 0; an unknown model; k even or <= 0
 * (checked before its size); a non-finite tap; a workspace too small or misaligned; iwe, blurred, stats or dropped not 8-byte
 * aligned.  ENSLAM_EUNSUPPORTED without a launch: N > 2^31 - 1, H or W > 65536, more than 2^28 pixels, k >
 * ENSLAM_CMAX_MAX_KSIZE.  enslam_event_cmax_workspace refuses the same sizes and P outside 2..3. */
#define ENSLAM_CMAX_FLOW 0
#define ENSLAM_CMAX_ROTATION 1
#define ENSLAM_CMAX_MAX_KSIZE 31
#define ENSLAM_CMAX_DROP_TIME 0
#define ENSLAM_CMAX_DROP_SENSOR 1
#define ENSLAM_CMAX_DROP_WARP 2
int enslam_event_cmax_workspace(int32_t H, int32_t W, int64_t N, int32_t P, int64_t *bytes_host);
int enslam_event_cmax_eval(const double *t, const uint16_t *x, const uint16_t *y, const uint8_t *p, int64_t N, int32_t H,
                           int32_t W, double fx, double fy, double cx, double cy, int32_t model, const double *theta_host,
                           double t_ref, int32_t sign_votes, int32_t k, const double *taps_host, void *workspace,
                           int64_t workspace_bytes, int64_t *iwe, double *blurred, double *stats, uint64_t *dropped,
                           int32_t want_grad, void *stream);

/* The rigid-motion model of the same objective: the six velocity components of a camera that moves through a scene of known
 * depth, at metric scale.  Its own entry points, because the pair above refuses a third model and P outside 2..3 and keeps
 * doing so; both *_eval entries run one validating body and one set of kernels (csrc/event_cmax.hip).
 *
 * The arguments are enslam_event_cmax_eval's without `model`, plus: depth, a device float32 [H,W] image in the sensor's own
 * resolution (only read); theta_host, a HOST float64 [6] = (w_x, w_y, w_z, v_x, v_y, v_z): the angular velocity in rad / s,
 * then the linear velocity in depth units / s, both in the pinhole frame of ROTATION (x right, y down, z forward); dropped,
 * uint64 [4].  ALL arithmetic is float64, every operation on its own, in exactly this order; u, v, uv, pu, pv, dt, mx, my are
 * ROTATION's:
 *     z   = depth[y * W + x]                (the event's own, already checked, pixel: no interpolation)
 *     rho = 1 / (float64)z
 *     Bu  = (uv, -pu,  v, -rho, 0.0, u * rho)
 *     Bv  = (pv, -uv, -u, 0.0, -rho, v * rho)
 *     du  = ((uv * w_x - pu * w_y) + v * w_z) + rho * (u * v_z - v_x)
 *     dv  = ((pv * w_x - uv * w_y) - u * w_z) + rho * (v * v_z - v_y)
 *     x'  = xd + mx * du                    y'  = yd + my * dv
 * the motion field (Longuet-Higgins and Prazdny) of a camera whose pose obeys c2w(t + dt) = c2w(t) exp(dt xi), to first order
 * in |xi| dt; an event's depth is held constant over the window.
 * Checks, in this order, each with its counter: x >= W or y >= H -> dropped[ENSLAM_CMAX_DROP_SENSOR]; t not finite ->
 * dropped[ENSLAM_CMAX_DROP_TIME]; z not finite or z <= 0 -> dropped[ENSLAM_CMAX_DROP_DEPTH] (the depth is read only after the
 * sensor check: no address comes from an unchecked value); then the float64 range check on x', y' ->
 * dropped[ENSLAM_CMAX_DROP_WARP] (a subnormal float32 z is a valid depth with rho up to 2^149: its x', far outside the
 * image, infinite or NaN, fails here).
 * The vote, the blur, mu, f, D, Gx, Gy, g_k (k = 0..5), SUM, the outputs and the capture safety are the ones above; stats is
 * float64 [2 + 6]; the workspace is the formula above with P = 6 (enslam_event_cmax_rigid_workspace).
 * The refusals are the ones above (without the model), plus ENSLAM_EINVAL for a NULL depth with N > 0 and for a non-finite
 * component of the six-element theta. */
#define ENSLAM_CMAX_DROP_DEPTH 3
int enslam_event_cmax_rigid_workspace(int32_t H, int32_t W, int64_t N, int64_t *bytes_host);
int enslam_event_cmax_rigid_eval(const double *t, const uint16_t *x, const uint16_t *y, const uint8_t *p, int64_t N, int32_t H,
                                 int32_t W, double fx, double fy, double cx, double cy, const float *depth,
                                 const double *theta_host, double t_ref, int32_t sign_votes, int32_t k,
                                 const double *taps_host, void *workspace, int64_t workspace_bytes, int64_t *iwe,
                                 double *blurred, double *stats, uint64_t *dropped, int32_t want_grad, void *stream);

/* Event-collapse regularisers of the same objective (Shiba, Aoki, Gallego: Event Collapse in Contrast Maximization Frameworks,
 * 2022): with six parameters the contrast has no useful maximum -- v_z contracts the events towards the principal point and the
 * variance rises without bound.  R, the mean over the events that voted of the absolute DIVERGENCE of the warp's flow or of
 * the absolute DEFORMATION |det(dx'/dx) - 1| of the warp, is what a caller subtracts from f with a weight (event_cmax.py).
 * A third entry, because the four above keep their signatures, workspace formulas and refusals; it runs the same validating
 * body and the same kernels, and iwe, blurred, stats and dropped are bit-equal to theirs for every reg_kind.
 *
 * The arguments are enslam_event_cmax_rigid_eval's, plus: model, ENSLAM_CMAX_FLOW, ENSLAM_CMAX_ROTATION or ENSLAM_CMAX_RIGID
 * (theta_host has the model's P = 2, 3 or 6 numbers, dropped 3 counters, 4 for RIGID; depth must be NULL unless RIGID);
 * reg_kind, ENSLAM_CMAX_REG_NONE, _DIVERGENCE or _DEFORMATION; reg_stats, float64 [2 + P] = (R, M, dR / dtheta...).
 * Per event that passes every check above (the same checks: the pass warps the event once more and reads the depth at the
 * checked pixel only), with that warp's dt, u, v, rho (ROTATION is the rho = 0.0 case of RIGID, with v_z = 0.0 and k < 3) and
 * theta = (w, v); float64, every operation on its own, in exactly this order:
 *     c11 = (v * w_x - (2 u) * w_y) + rho * v_z          e11 = ( v, -(2 u),  0, 0, 0, rho)
 *     c22 = ((2 v) * w_x - u * w_y) + rho * v_z          e22 = (2 v,    -u,  0, 0, 0, rho)
 *     c12 = u * w_x + w_z                                e12 = ( u,      0,  1, 0, 0, 0)
 *     c21 = -(v * w_y) - w_z                             e21 = ( 0,     -v, -1, 0, 0, 0)
 *     d_div = -(dt * (c11 + c22))
 *     d_def = d_div + (dt * dt) * (c11 * c22 - c12 * c21)
 *     dd_div[k] = -(dt * (e11[k] + e22[k]))
 *     dd_def[k] = dd_div[k] + (dt * dt) * ((e11[k] * c22 + c11 * e22[k]) - (e12[k] * c21 + c12 * e21[k]))
 *     r = |d|,   dr[k] = sgn(d) * dd[k]   with sgn(0) = 0.0;   r = dr[k] = 0.0 for a dropped event
 *     R = SUM(r) / M,   dR[k] = SUM(dr[k]) / M,   M = N minus the drop counters (the events that voted); M = 0: R = dR = 0.0
 * c_ij is the Jacobian of the motion field (du, dv) in (u, v), so that dx'/dx = 1 - dt c: d_div is its trace times -dt and
 * d_def = det(dx'/dx) - 1 (the factors fx / fy and fy / fx of the off-diagonal pair cancel in the product).  The depth of an
 * event is held LOCALLY CONSTANT: there is no term in the gradient of rho -- a finite difference of a depth image across an
 * occlusion edge is not a usable number.  FLOW has R = dR = 0.0 exactly (a constant flow has neither) and M as above.
 * SUM is the tree above over the events in stream order; M is read from the drop counters on the device.  dR is 0.0 without
 * want_grad; with ENSLAM_CMAX_REG_NONE nothing is added to the launches and reg_stats is all 0.0.  The launches stay one
 * capturable chain on the stream.  workspace: enslam_event_cmax_reg_workspace bytes, the formula above with 1 + P partials per
 * workgroup of events in place of P.
 * The refusals are enslam_event_cmax_rigid_eval's, plus ENSLAM_EINVAL for an unknown model, an unknown reg_kind, a depth that is
 * not NULL with FLOW or ROTATION, and a NULL or misaligned reg_stats; a NULL depth is refused for RIGID only. */
#define ENSLAM_CMAX_RIGID 2
#define ENSLAM_CMAX_REG_NONE 0
#define ENSLAM_CMAX_REG_DIVERGENCE 1
#define ENSLAM_CMAX_REG_DEFORMATION 2
int enslam_event_cmax_reg_workspace(int32_t H, int32_t W, int64_t N, int32_t model, int64_t *bytes_host);
int enslam_event_cmax_reg_eval(const double *t, const uint16_t *x, const uint16_t *y, const uint8_t *p, int64_t N, int32_t H,
                               int32_t W, double fx, double fy, double cx, double cy, int32_t model, const float *depth,
                               const double *theta_host, double t_ref, int32_t sign_votes, int32_t k, const double *taps_host,
                               void *workspace, int64_t workspace_bytes, int64_t *iwe, double *blurred, double *stats,
                               uint64_t *dropped, int32_t reg_kind, double *reg_stats, int32_t want_grad, void *stream);

/* Depth forecast (csrc/depth_forecast.hip, functional.depth_forecast): a measured depth image forward-warped into another
 * camera pose and image size by a z-buffered point splat -- the guidance depth of the tracker's reduced-resolution render on a
 * frame without an RGB-D image (slam.py, event.depth_on_event_frames: 'forecast').
 * depth float32 [H,W] (device); m_host 12 float64 on the HOST, row-major 3 x 4, source-camera to target-camera coordinates
 * (cameras look down -z); depth_out float32 [Ho,Wo] (device); workspace 4 * Ho * Wo bytes (device, the vote image).
 * Every operation is float64 in the order written, not contracted; (float)z is the only float32 rounding.
 *   A source pixel (row j, column i) with d = depth[j,i] finite and > 0 is the point p = (d px, d py, -d), px = (i - cx) / fx,
 *   py = -(j - cy) / fy.  q_r = ((M[4r] p_0 + M[4r+1] p_1) + M[4r+2] p_2) + M[4r+3], z = -q_2; kept iff z > z_near and (float)z
 *   is finite.  u = cx + fx (q_0 / z), v = cy - fy (q_1 / z).  Target pixel (jo, io) stands for the full-resolution position
 *   (jo sy, io sx), sx = (W - 1) / (Wo - 1), sy = (H - 1) / (Ho - 1) (1 for an axis of one target pixel).  io = floor(u / sx +
 *   0.5), jo = floor(v / sy + 0.5); the point votes iff 0 <= io <= Wo - 1, 0 <= jo <= Ho - 1, |u - io sx| <= radius and
 *   |v - jo sy| <= radius.  Votes combine by an unsigned integer minimum on the bits of (float)z: the same bits in every run.
 *   A pixel without a vote is 0.0; with fill = 1 it takes the LARGEST voted value among its up to 8 neighbours of the voted
 *   (unfilled) image, 0.0 when there is none.
 * One memset and two launches on the stream, no host synchronisation; the input is only read.
 * ENSLAM_EINVAL without a launch: a NULL or misaligned (4 bytes) pointer; H, W, Ho or Wo <= 0; Wo > 1 with W = 1 or Ho > 1
 * with H = 1; a non-finite intrinsic, matrix entry, radius or z_near; fx or fy equal to 0; radius < 0; z_near < 0; fill not 0
 * or 1.  ENSLAM_EUNSUPPORTED: more than 2^30 source or target pixels. */
int enslam_depth_forecast(const float *depth, int32_t H, int32_t W, double fx, double fy, double cx, double cy,
                          const double *m_host, int32_t Ho, int32_t Wo, double radius, double z_near, int32_t fill,
                          void *workspace, float *depth_out, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* ENSLAM_HIP_H */
