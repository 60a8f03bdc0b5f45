/*
 * include/csplat.h -- C-ABI of libcsplat.so, the MI355X (gfx950) hot path of cloth-splatting.
 *
 * Plain pointers and sizes only; every pointer named "device" is HBM memory owned by the caller
 * (torch tensors on the Python side), `stream` is a hipStream_t passed as void*.  All calls are
 * stream-ordered; the only host synchronisation is the 8-byte read of `num_rendered` (and the longest
 * tile list) inside csplat_forward (upstream reads num_rendered the same way): the scan kernel posts it
 * to a host-pinned mailbox that the host polls.  Return value: 0 = ok, non-zero = error
 * (text via csplat_last_error()); no C++ exception crosses this boundary.
 *
 * What each entry point replaces in the reference (/root/reference):
 *   csplat_forward / csplat_backward
 *       the `diff_gaussian_rasterization._C.rasterize_gaussians{,_backward}` calls behind
 *       GaussianRasterizer.forward, gaussian_renderer/__init__.py:16,76,156-164 (backward runs from
 *       loss.backward(), scene_reconstruction/train_utils.py:288).  Sources of that extension are an empty
 *       submodule (.gitmodules:7-9); the argument list mirrors its published rasterize_points.h.
 *   csplat_visibility_views
 *       no counterpart there: which Gaussians a view really sees (peak / summed blending weight, pixel count) and which one dominates
 *       each pixel, for an occlusion-aware `visibility_filter` (the reference uses radii > 0, train_utils.py:270-300, train.py:52-90).
 *   csplat_dist2
 *       `simple_knn._C.distCUDA2`, scene_reconstruction/gaussian_mesh.py:26,250; gaussian_model.py:20,134.
 *   csplat_knn, csplat_knn_ws, csplat_fps
 *       the host neighbour queries of the reference: cKDTree in compute_edges_index (meshnet/data_utils.py:406-412), the Open3D
 *       KD-tree of o3d_knn (utils/external.py:5-16), the numpy loop of farthest_point_sampling (meshnet/data_utils.py:134-160).
 *   csplat_track_visibility, csplat_track_mte
 *       the host-side tracking evaluation: `project` and `get_mask` of render.py:77-121 for all view-frames at once, and the
 *       align_traj + compute_mte loop of scripts/align_eval_trajs.py for all ground-truth tracks at once.
 *   csplat_obs_unproject, csplat_obs_voxel, csplat_obs_mark
 *       the host-side observation code: get_world_coords (manipulation/envs/camera_utils.py:106-133, manipulation/deform_mesh.py:168-195)
 *       and get_observable_particle_index (camera_utils.py:136-162); the voxel grid thins the cloud before node sampling.
 *   csplat_zb_mesh, csplat_zb_points, csplat_zb_mark
 *       what a depth camera sees of the mesh: the Blender renders of manipulation/fold_rendering/ and the pixel loop
 *       build_depth_from_pointcloud (manipulation/envs/camera_utils.py:7-41), as an exact z-buffer on the device.
 *   csplat_gnn_*
 *       the torch_geometric MessagePassing gather / scatter-add inside InteractionNetwork.propagate,
 *       meshnet/graph_network.py:173-174 (gather x_i, x_j: PyG __lift__), :197 (concat), :136 (aggr='add').
 */
#ifndef CSPLAT_H
#define CSPLAT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CSPLAT_ABI_VERSION 9   /* 9: feature channels and the alpha image (csplat_view.features .. dL_dfeat_in, csplat_backward_feature_scratch_bytes); 8: camera and background gradients (csplat_view.dL_dview / dL_dproj / dL_dcampos / dL_dbg, csplat_backward_camera_scratch_bytes); 7: the depth image's gradient (csplat_view.dL_ddepth, csplat_backward_depth, csplat_backward_depth_scratch_bytes); 6 (round 6): csplat_backward_views_parts / _slice_rows, csplat_gnn_edge_length_refine, csplat_rollout_head / _decode / _integrate, csplat_gnn_edge_features_ordered, csplat_gnn_rows_chain(_pack), csplat_binning_fields; round 4: csplat_view.busy_tiles / .valid, csplat_rows_dot_fwd's extra argument; 3: the binning chunk's layout (bbits, bmask); 4 (round 5): csplat_gather_words kind 2; 5: csplat_gnn_edge_mlp3* (e0_absmax, modes), csplat_absmax, csplat_linear_narrow128 */

/* scratch chunks requested through the allocator callback */
#define CSPLAT_CHUNK_GEOM 0    /* per-Gaussian state, kept for backward */
#define CSPLAT_CHUNK_BINNING 1 /* sorted tile instances, kept for backward */
#define CSPLAT_CHUNK_IMAGE 2   /* per-tile ranges, per-pixel n_contrib / final_T, kept for backward */
#define CSPLAT_CHUNK_TEMP 3    /* unsorted instances, sort ping-pong + histograms; may be freed after forward */
#define CSPLAT_CHUNK_TABLE 4   /* per-(workgroup, tile) counting table of the bucketed binning; may be freed after forward */

/* Must return a device pointer to at least `bytes` bytes, 256-byte aligned, valid until the matching
 * backward has run (GEOM/BINNING/IMAGE) or until csplat_forward returns (TEMP).  NULL = failure. */
typedef void *(*csplat_alloc_fn)(void *ctx, int chunk, size_t bytes);

int csplat_abi_version(void);
/* test hooks (results must not change beyond fp32 re-association).  bit 0: no culling -- every block mask of K5b is all ones;
 * bit 1: force the global radix-sort binning path instead of the tile-bucketed LDS sort;
 * bit 2: read R with a blocking stream synchronise instead of polling the pinned mailbox;
 * bit 3: unused (round 1's experimental four-wave forward was removed);
 * bit 4: quadruple the culling radius (sensitivity check of the culling bound);
 * bit 5: circle stage of the culling only (no exact ellipse-vs-box stage).  Bits 0 and 4 also switch the ellipse stage off;
 * bit 7: one K8 launch per view instead of one for all views of a step;
 * bit 8: bit-reproducible backward -- K7 stores one record per (list entry, quadrant) and every Gaussian sums its records in
 *        emission order instead of meeting in float atomics (csplat_backward_scratch_bytes grows accordingly: set the flag
 *        before sizing the scratch);
 * bit 9: per-view launches on per-view streams instead of one launch per stage for all views of a step;
 * bit 10: csplat_forward_views always waits for a call's counts before launching its second phase (no speculative launch with
 * the previous call's counts as capacities);
 * bit 11: tile sort by LSD radix only; bit 12: forced radix fallback of the bucket sort (both: test hooks of the sort's two paths);
 * bit 15: K6 in the row form (four survivors per step; default: sixteen per step) -- kept because its transmittance products run in list
 *         order, which the culling-exactness test holds bit for bit.
 * Bits 13, 14, 16-21 selected the shelved kernel forms of round 3 (K7 survivor columns, retire-waves flush, K6 items per wave / tile order,
 * block masks by blockIdx.y); those forms left the library in round 4 (history: commit 809fd4b) and the bits are
 * ignored.  The word is process-global and meant to be set between calls, not concurrently with them. */
#define CSPLAT_DEBUG_NO_CULLING 1u             /* bit 0 */
#define CSPLAT_DEBUG_GLOBAL_SORT 2u            /* bit 1 */
#define CSPLAT_DEBUG_NO_MAILBOX 4u             /* bit 2 */
#define CSPLAT_DEBUG_CULL_RADIUS_X4 16u        /* bit 4 */
#define CSPLAT_DEBUG_CIRCLE_ONLY 32u           /* bit 5 */
#define CSPLAT_DEBUG_PER_VIEW_K8 128u          /* bit 7 */
#define CSPLAT_DEBUG_BIT_REPRODUCIBLE 256u     /* bit 8 */
#define CSPLAT_DEBUG_PER_VIEW_LAUNCHES 512u    /* bit 9 */
#define CSPLAT_DEBUG_NO_SPECULATION 1024u      /* bit 10 */
#define CSPLAT_DEBUG_SORT_RADIX_ONLY 2048u     /* bit 11 */
#define CSPLAT_DEBUG_SORT_RADIX_FALLBACK 4096u /* bit 12 */
#define CSPLAT_DEBUG_K6_ROWS 32768u            /* bit 15 */
int csplat_debug_flags(unsigned flags);
unsigned csplat_debug_flags_query(void);
/* measurement hook (not part of the operator interface): a device buffer the batched compositing backward fills with s_memtime stamps,
 * 12 uint64 per workgroup in launch order [view][workgroup] (tools/k7_stamps.py); NULL / 0 switches it off.  A buffer of exactly
 * 8 * (ceil(P / 64) + ceil(P / 32)) uint64 is filled by the batched K1 and K8 of a P-Gaussian step instead, 8 per workgroup, K1's first
 * (tools/per_gaussian_stamps.py) */
int csplat_debug_stamps(void *device_buffer, size_t bytes);
const char *csplat_last_error(void);

/* Sizes of the chunks (bytes) so that a caller may pre-allocate instead of answering the callback lazily. */
size_t csplat_geom_bytes(int P);
size_t csplat_image_bytes(int W, int H);
size_t csplat_binning_bytes(int64_t R, int W, int H);
size_t csplat_temp_bytes(int P, int64_t R, int W, int H);
size_t csplat_backward_scratch_bytes(int P, int64_t R); /* per-Gaussian accumulation records used by csplat_backward */
/* the scratch of a backward call that takes a depth gradient (csplat_backward_depth, or any view of csplat_backward_views* with
 * dL_ddepth set -- then EVERY view of that call needs this size): the records above, 10-float (entry, block) records in the
 * bit-reproducible mode, and one float per (list segment, pixel) for the depth partials.  Never smaller than
 * csplat_backward_scratch_bytes(P, R). */
size_t csplat_backward_depth_scratch_bytes(int P, int64_t R, int W, int H);
/* the scratch of a backward call that takes a camera or background gradient (any view of csplat_backward_views* with dL_dview,
 * dL_dproj, dL_dcampos or dL_dbg set -- then EVERY view of that call needs this size): the depth layout above, then the camera slab
 * (one 35-float row per K8 workgroup) and the background slab (256 rows of 3).  Never smaller than
 * csplat_backward_depth_scratch_bytes(P, R, W, H). */
size_t csplat_backward_camera_scratch_bytes(int P, int64_t R, int W, int H);
/* the scratch of a backward call that takes a feature or alpha gradient (any view of csplat_backward_views with dL_dfeatures or
 * dL_dalpha set -- then EVERY view of that call needs this size): the camera layout above, then one float per (list segment, pixel) for
 * the feature partials and, in the bit-reproducible mode, 16-float (entry, block) records.  Never smaller than
 * csplat_backward_camera_scratch_bytes(P, R, W, H). */
size_t csplat_backward_feature_scratch_bytes(int P, int64_t R, int W, int H);

/* Byte offsets of the named sub-buffers inside a chunk (for tests / debugging; see DESIGN.md "HBM layout").
 * geom:    0 depth f32[P] | 1 xy f32[P][2] | 2 conic_opacity f32[P][4] | 3 rgb f32[P][3] | 4 cov3D f32[P][6]
 *          | 5 clamped u32[P] (bit c = channel c clamped) | 6 tiles_touched u32[P]
 *          | 7 offsets u32[P] (inclusive scan; filled only on the global radix-sort path)
 * binning: 0 keys u64[R] (sorted) | 1 ids u32[R] (sorted)   [ABI 3, behind them and not part of the offsets: the per-tile segment
 *          plan seg_offset[tiles+1] / slot_tile[slots]; the forward's checkpoints float4[slots][16 blocks][16 px] (T, colour so far
 *          at the start of every 256-entry list segment); the 16-bit block masks u16[R+1]; the tile-ordered records recA / recB
 *          float4[R+1], recC float2[R+1] (entry R = the null record); `bbits` u64[slots][16][4] = per (segment, 4x4 block) WHICH of the
 *          segment's entries the block blended (K6 writes, K7 reads); `bmask` u64[R/64+4][16] = the block masks transposed, per 64
 *          list entries and block (K5b writes, K6 reads).  R here is the LAYOUT count (csplat_view.layout_rendered >= num_rendered)]
 * image:   0 ranges i32[tiles][2] | 1 n_contrib u32[H*W] | 2 final_T f32[H*W]                               */
int csplat_geom_layout(int P, size_t *offsets8);
int csplat_binning_layout(int64_t R, int W, int H, size_t *offsets2);
/* byte offsets of ALL eleven sub-buffers of a BINNING chunk laid out for R list entries: 0 sorted keys, 1 sorted ids, 2 seg_offset[tiles + 1]
 * followed by blk_hi[tiles][16], 3 slot_tile, 4 checkpoints, 5 block masks, 6-8 the tile-ordered records, 9 bbits u64[slots][16][4] (which
 * entries of a 256-entry segment a 4x4 block blended), 10 bmask.  Diagnostics only (tools/k6_stats.py, bench.py's count of the (entry,
 * block) pairs = K7's float-atomic requests). */
int csplat_binning_fields(int64_t R, int W, int H, size_t *o11);
int csplat_image_layout(int W, int H, size_t *offsets3);

/* Forward: K1 preprocess (+ per-tile counts), K2 tile scan, K3 instance emission into tile buckets, K4 per-tile LDS sort
 * (global stable radix sort when a tile list exceeds 8192 entries), K5 segment plan, K6 compositing.
 *   means3D[P][3], shs[P][M][3] or NULL, colors_precomp[P][3] or NULL (exactly one of the two),
 *   opacities[P], scales[P][3]+rotations[P][4] or cov3D_precomp[P][6] (exactly one of the two),
 *   view/proj: the reference's transposed 4x4 matrices (flat index 4*row+col of world_view_transform /
 *   full_proj_transform, scene_reconstruction/cameras.py:63-67), campos[3], bg[3]  -- all device, fp32.
 *   D = active SH degree (0..3), M = SH coefficients per channel stored (16 for max degree 3).
 *   The rule for M and the SH pointers, for every entry point that takes them (csplat_forward*, csplat_backward*, csplat_view):
 *     - any M >= (D+1)^2 is accepted, at any 4-byte alignment of shs / dL_dsh; coefficient rows past (D+1)^2 are not read, and their
 *       gradient rows are written as zeros;
 *     - staging the SH rows through LDS (K1, K8), the one K8 launch for all views of csplat_backward_views and CSPLAT_ACC_SH need
 *       M == 16 and 16-byte aligned shs and (K8) dL_dsh.  Anything else is served by the unstaged kernels, per view, each view writing a
 *       dL_dsh of its own; a view that asks for CSPLAT_ACC_SH there is an error.
 * Outputs (device): out_color[3][H][W], out_depth[1][H][W], radii[P] (int32).
 * *num_rendered (host) receives R = number of (Gaussian, tile) instances.
 * The three kept chunks are returned through geom/binning/image (device pointers from `alloc`). */
int csplat_forward(void *stream, int P, int D, int M, const float *bg, int W, int H, const float *means3D,
                   const float *shs, const float *colors_precomp, const float *opacities, const float *scales,
                   float scale_modifier, const float *rotations, const float *cov3D_precomp, const float *view,
                   const float *proj, const float *campos, float tanfovx, float tanfovy, int prefiltered,
                   csplat_alloc_fn alloc, void *alloc_ctx, float *out_color, float *out_depth, int32_t *radii,
                   int *num_rendered, void **geom, void **binning, void **image);

/* Two-phase form of csplat_forward for callers with several independent views in flight (new; upstream renders cameras one
 * by one: /root/reference/scene_reconstruction/train_utils.py:204-260).  _begin enqueues K1 and the counting half of the
 * binning on `stream` and returns without waiting; _finish (same thread or another) reads num_rendered -- the path's only
 * host round trip --, requests the R-sized chunks from the allocator given to _begin and enqueues K3..K6 on the same
 * stream.  Issue every _begin before the first _finish and the round trips and the compositing kernels of the views
 * overlap.  At most 64 tickets may be open; a ticket is released by _finish whatever it returns.
 * csplat_forward(...) == csplat_forward_begin(...) followed by csplat_forward_finish(...). */
int csplat_forward_begin(void *stream, int P, int D, int M, const float *bg, int W, int H, const float *means3D,
                         const float *shs, const float *colors_precomp, const float *opacities, const float *scales,
                         float scale_modifier, const float *rotations, const float *cov3D_precomp, const float *view,
                         const float *proj, const float *campos, float tanfovx, float tanfovy, int prefiltered,
                         csplat_alloc_fn alloc, void *alloc_ctx, int32_t *radii, int *ticket_out);
int csplat_forward_finish(int ticket, float *out_color, float *out_depth, int *num_rendered, void **geom,
                          void **binning, void **image);

/* Batched form: V independent views of one step in ONE call each way (the reference's loop over cameras,
 * /root/reference/scene_reconstruction/train_utils.py:204-260 forward, :288 backward).  Every view names its own stream;
 * the library fences them against `join_stream` on entry and exit (events), issues every view's K1/K2 before the first
 * num_rendered read, and in the backward runs the views' K7 concurrently.  accmask (CSPLAT_ACC_*): gradient outputs of
 * this view that are ADDED to a buffer an earlier view of the same call wrote (a parameter shared by several views then
 * needs no per-view temporaries and no summation launches); when any view accumulates, K8 of all views runs on the join
 * stream in view order.  dL_dmean2D is always written, dL_dconic unless CSPLAT_K8_OUTPUTS_UNREAD lets it be skipped.  Field meanings as in csplat_forward / csplat_backward. */
enum { CSPLAT_ACC_OPACITY = 1, CSPLAT_ACC_COLOR = 2, CSPLAT_ACC_MEAN3D = 4, CSPLAT_ACC_COV3D = 8, CSPLAT_ACC_SH = 16,
       CSPLAT_ACC_SCALE = 32, CSPLAT_ACC_ROT = 64,
       /* not an accumulate bit: the view's `scratch` records are ALL ZERO on entry and the call leaves them all zero again (K8 clears
        * every record it has consumed) -- a caller that keeps the buffer from step to step on one stream then needs no clearing launch per
        * step (25.6 MB of zero fill for four views of 100k Gaussians).  Without the bit the library clears the records itself. */
       CSPLAT_SCRATCH_ZEROED = 256,
       /* not an accumulate bit either: the caller does not read dL_dconic, dL_dcolor and dL_dcov3D of this call, and the library MAY leave
        * them unwritten.  The three pointers stay required and valid (every per-view launch still writes them).  The one-launch K8 of
        * csplat_backward_views / _parts skips their stores when ALL views of the call carry the bit: each of the three buffers is then
        * either written in full or not touched at all.  A caller that passes scales and rotations (no cov3D_precomp) and SH (no
        * colors_precomp) has no use for the three and should set it.  An older caller does not, and gets every output as before. */
       CSPLAT_K8_OUTPUTS_UNREAD = 512 };
#define CSPLAT_MAX_FEATURES 6    /* ABI 9: csplat_view.n_features <= 6 (record slots 10..15 of the compositing backward) */
/* csplat_view.prefiltered is a bit word.  Bit 0 is upstream's `prefiltered` flag and is ignored, as before.
 * CSPLAT_ANTIALIAS (bit 1): antialiased rendering with opacity compensation (upstream's `antialiasing` option).  K1 widens every projected
 * covariance by 0.3 px^2; with the bit it also scales the opacity by the ratio of the footprint areas it has widened.  With
 * (a0, b, c0) = T Sigma T^T, the cov2D before the 0.3 is added:
 *     det0 = a0 c0 - b^2,   det1 = (a0 + 0.3)(c0 + 0.3) - b^2   (the determinant the conic inverts),
 *     h = sqrt(max(2.5e-5, det0 / det1)),   o' = opacity h,
 * and every later use of the view's opacity is o': conic_opacity.w, the culling radius 2 lambda ln(255 o'), the 1/255 skip, the 0.99 cap,
 * the stop rule, n_contrib, the colour, depth, feature and alpha images.  Conic, radius and tile rectangle are those of the widened cov2D,
 * unchanged.  The backward is the chain rule through h: dL/dopacity = h dL/do', and opacity dL/do' dh/d(a0, b, c0) joins the cov2D
 * gradient (b the one scalar off-diagonal entry; dh = 0 where the 2.5e-5 floor is active) before it reaches cov3D, scales, rotations,
 * means3D and the camera gradients.  It composes with the depth, camera, feature / alpha paths, launches on faith, captured steps and
 * csplat_backward_views_parts slices.  Honoured by csplat_forward_views, _deferred / _settle, _faith, csplat_backward_views and _parts
 * (the backward reads the view's `opacities`: keep them alive and unchanged until it has run); the views of one batched launch share
 * the bit (views that differ take the per-view launches; csplat_forward_views_faith refuses them).  csplat_forward / csplat_forward_begin
 * return an error when it is set: their backward cannot see it. */
#define CSPLAT_ANTIALIAS 2
typedef struct csplat_view {
    void *stream;
    int P, D, M, W, H, prefiltered;   /* prefiltered: bit 0 ignored, CSPLAT_ANTIALIAS */
    float scale_modifier, tanfovx, tanfovy;
    const float *bg, *means3D, *shs, *colors_precomp, *opacities, *scales, *rotations, *cov3D_precomp, *view, *proj, *campos;
    void *alloc_ctx;
    float *out_color, *out_depth;   /* forward outputs (caller-allocated) */
    int32_t *radii;
    int num_rendered;               /* written by the forward: R, the number of (Gaussian, tile) instances */
    int layout_rendered;            /* written by the forward, read by the backward: the list capacity (>= R) the binning chunk
                                     * was laid out for -- csplat_forward_views may size it from the previous call's counts so
                                     * as not to wait for this call's (use it for csplat_backward_scratch_bytes too) */
    void *geom, *binning, *image;   /* chunk base pointers: written by the forward, read by the backward */
    const float *dL_dpix;           /* backward inputs */
    void *scratch;
    unsigned accmask;
    float *dL_dmean2D, *dL_dconic, *dL_dopacity, *dL_dcolor, *dL_dmean3D, *dL_dcov3D, *dL_dsh, *dL_dscale, *dL_drot;
    int busy_tiles;                 /* written by the forward (0 = not known): tiles with a non-empty list -- the backward sizes the
                                     * compositing backward's grid with it (segments <= R / 256 + busy_tiles + 1) */
    const uint32_t *valid;          /* NULL, or (csplat_forward_views_faith) the device word that says whether the forward took place:
                                     * the backward of views[0..V) does nothing when it is 0 */
    const float *dL_ddepth;         /* ABI 7, backward input: the gradient of out_depth [1][H][W], NULL = none.  When any view of a
                                     * backward call has one, the call takes the depth path (extra launches, see csplat_backward_depth;
                                     * every view's scratch sized by csplat_backward_depth_scratch_bytes; not for views launched on faith;
                                     * more than 8 views: see "More than 8 views" below); when none has, the call is exactly the ABI 6 one */
    /* ABI 8, backward outputs (device, each NULL = not wanted): the gradients of the camera tensors of the view, WRITTEN (never added).
     * Notation: V = view, Pm = proj (row-vector form, flat index 4 row + col), ph = [m, 1] for a mean m; pv = ph V, hom = ph Pm,
     * ndc = hom[:2] / (hom[3] + 1e-7), Rw = V[:3,:3]^T, cov2D = J(pv) Rw Sigma Rw^T J(pv)^T, the SH direction (m - campos) / |m - campos|,
     * the depth z = pv[2], C = sum T_i alpha_i c_i + T_final bg.  The gradients are the chain rule through exactly these uses, with the
     * conventions of the Gaussian gradients: tile lists, sort order, culling and termination are constants, alpha is straight-through
     * at the 0.99 cap, the 1.3 tanfov clamp stops the gradient of a clamped axis of pv, radii are not differentiable.
     *   dL_dview[16]   sum over visible Gaussians of ph (x) dL/dpv (covariance term through J(pv), the depth term dL/dz when dL_ddepth
     *                  is set), plus (J^T dL/dT)^T on the upper 3x3 block (T = J Rw); column 3 (flat 3, 7, 11, 15) is exactly 0
     *   dL_dproj[16]   sum of ph (x) dL/dhom through the projected centre only (J uses fx = W / (2 tanfovx), not Pm); column 2 is 0
     *   dL_dcampos[3]  minus the sum of the SH-direction part of dL/dmean3D; 0 with colors_precomp
     *   dL_dbg[3]      sum_pix dL/dC_c(pix) T_final(pix)
     * The sums over Gaussians run in a fixed order (a slab row per K8 workgroup and view, then a fixed-order sum; no float atomics), so
     * they are bit-reproducible whenever their per-Gaussian inputs are (csplat_debug_flags bit 256).  Every view's scratch is sized by
     * csplat_backward_camera_scratch_bytes.  Not for views launched on faith, nor csplat_backward_views_parts with parts != 3 or
     * nslices != 1; more than 8 views: see "More than 8 views" below.  All NULL: the call is exactly the ABI 7 one. */
    float *dL_dview, *dL_dproj, *dL_dcampos, *dL_dbg;
    /* ABI 9, feature channels and the alpha image.  features [P][n_features] (device, 1 <= n_features <= CSPLAT_MAX_FEATURES; NULL and 0
     * = none; a view with P = 0 may leave it NULL whatever n_features) are composited with the colour's weights over exactly the entries the colour blends (same alpha, 0.99 cap, 1/255 skip,
     * stop rule, n_contrib), without a background term:  out_features[c][pix] = sum_i T_i alpha_i f[i][c]  ([n_features][H][W]);
     * out_alpha[pix] = 1 - T_final(pix)  ([1][H][W]; T_final = the factor of the colour's background term).  Both are written by
     * csplat_forward_views, csplat_forward_views_deferred (when not pending) and csplat_forward_views_settle, in one launch behind the
     * views' K6 on the join stream; each NULL = not wanted (not for csplat_forward_views_faith).
     * Backward inputs dL_dfeatures [n_features][H][W] and dL_dalpha [1][H][W] (NULL = none): when any view of a csplat_backward_views
     * call has one, the call takes the feature path (every view's scratch sized by csplat_backward_feature_scratch_bytes; more than 8
     * views: see below; not for views launched on faith nor csplat_backward_views_parts with parts != 3 or nslices != 1), which composes
     * with the depth and camera paths; dL/dalpha_i gains sum_c g_c (T_i f_ic - F_behind_c / (1 - alpha_i)) + g_A T_final / (1 - alpha_i).
     * dL_dfeat_in [P][n_features] (output, NULL = not wanted): sum over pixels of T_i alpha_i dL_dfeatures[c][pix], WRITTEN, or added when
     * an earlier view of the same call has the same buffer.  All NULL / 0: every call is exactly the ABI 8 one. */
    /* More than 8 views: the feature / alpha images, csplat_visibility_views and the depth, feature, alpha, camera and background
     * gradients take any number of views a call takes (csplat_forward_views: up to 64).  A call of more than 8 views runs them in
     * ceil(V / 8) groups of as equal a size as possible (9 views: 5 + 4), one group after the other on the join stream, each with the
     * launches of a call of its own views; accumulation (accmask, a shared dL_dfeat_in) spans the groups: a view adds to what a view of
     * an earlier group wrote, in view order, and the bit-reproducible mode stays bit-reproducible.  A call of up to 8 views is one group:
     * its launches are those it always made. */
    const float *features;
    int n_features;
    float *out_features, *out_alpha;
    const float *dL_dfeatures, *dL_dalpha;
    float *dL_dfeat_in;
} csplat_view;
int csplat_forward_views(int V, csplat_view *views, csplat_alloc_fn alloc, void *join_stream);
/* The same call with its one host read (the views' counts) DEFERRED.  When the second phase can be launched on the previous call's
 * capacities (speculative launch, see above), csplat_forward_views_deferred returns right behind that launch with *pending = 1:
 * layout_rendered is filled in (the capacity), num_rendered is -1; the caller does the host work that does not need the counts while
 * the GPU runs K1..K6 and then calls csplat_forward_views_settle with the SAME array on the same join stream -- before
 * csplat_backward_views and before reading num_rendered.  settle: counts fit -> num_rendered filled in, *relaunched = 0; they do not ->
 * the second phase is repeated with exact sizes (new BINNING chunks through the allocator of the call, which must still be callable;
 * layout_rendered / binning updated) and *relaunched = 1.  *pending = 0: the call was complete, nothing to settle. */
int csplat_forward_views_deferred(int V, csplat_view *views, csplat_alloc_fn alloc, void *join_stream, int *pending);
int csplat_forward_views_settle(int V, csplat_view *views, void *join_stream, int *relaunched);
int csplat_backward_views(int V, csplat_view *views, void *join_stream);
/* csplat_backward_views cut into parts (round 6; no counterpart upstream -- the reference is single-GPU): parts bit 0 = the compositing
 * backward (K7) of all views, bit 1 = the per-Gaussian backward (K8) for slice `slice` of `nslices` equal ranges of Gaussians (boundaries
 * at multiples of 32; csplat_backward_slice_rows).  A view-parallel step launches K7 once, then the K8 slices one by one, and hands the
 * finished gradient rows of slice g to its collective while slice g + 1 computes.  Only the one-launch-per-stage path can be cut (views
 * sharing P, SH, scales and the image size); parts = 3, one slice = csplat_backward_views.  The parts together equal the whole call bit for
 * bit. */
int csplat_backward_views_parts(int n_views, csplat_view *views, void *join_stream, unsigned parts, int slice, int nslices);
/* rows [*row_lo, *row_hi) of the P Gaussians whose gradients K8 slice `slice` of `nslices` finishes */
int csplat_backward_slice_rows(int P, int slice, int nslices, int64_t *row_lo, int64_t *row_hi);
/* The batched forward WITHOUT a host read, for stream capture (a training step replayed as a hipGraph; the reference times its step
 * with an event pair around exactly such a loop body, train.py:146,178): both phases are launched with the caller's capacities --
 * caps[0] list entries per view, caps[1] longest tile list, caps[2] non-empty tiles, normally a previous call's counts plus a margin --
 * and *valid (device) becomes 1 when every view's counts fitted, else 0 (the second phase then left the views untouched, and
 * csplat_backward_views, which finds views[i].valid set, does nothing).  num_rendered is NOT the count (it is set to the capacity):
 * the counts stay on the device, at csplat_image_info_offset(W, H) inside each view's IMAGE chunk (u32 x 3).  The views must qualify
 * for the one-launch-per-stage path (2..8 views sharing P, SH, opacities, scales, image size); otherwise an error is returned. */
int csplat_forward_views_faith(int V, csplat_view *views, csplat_alloc_fn alloc, void *join_stream, const uint32_t *caps, uint32_t *valid);
/* Images of more than 12288 tiles (16 x 16 pixels each; 2048 x 1536 is the largest 4:3 image within it): a view of that size has no tile-bucket
 * table and does not qualify for the one-launch-per-stage forward.  csplat_forward_views and csplat_forward_views_deferred run such views
 * one by one through the global sort, with the same results; _deferred completes the call itself (*pending = 0, nothing to settle) however
 * often the shape repeats.  csplat_forward_views_faith refuses them (the views do not qualify: the error its comment names).
 * csplat_backward_views, csplat_backward_views_parts, csplat_visibility_views and the feature / alpha images do not depend on the tile
 * count. */

/* byte offset of a view's counts (u32 x 3, see csplat_forward_views_faith) inside its IMAGE chunk */
size_t csplat_image_info_offset(int W, int H);

/* Gaussian visibility and the top-contributor map (forward only, no gradient; ABI 9, csplat_view unchanged).  With w_i(pix) = T_i alpha_i,
 * exactly the weight with which the colour image blended Gaussian i at pix (the same alpha, 0.99 cap, 1/255 skip, stop rule and n_contrib;
 * o' under CSPLAT_ANTIALIAS):
 *   weight_max[i]  = max_pix w_i(pix)       (0 where i blends nowhere)         [P] float
 *   weight_sum[i]  = sum_pix w_i(pix)                                           [P] float
 *   pixel_count[i] = number of pixels where i blended                           [P] int32
 *   top_id[pix]    = argmax_i w_i(pix), the front-most on a tie, -1 where nothing blended   [H][W] int32
 * Each pointer NULL = not wanted; every wanted output is fully written (zeros for radii == 0, -1 for a view without list entries).  No float
 * atomics: the per-entry records are joined in a fixed order (16 lanes of a block, then the 16 blocks of a tile), the per-Gaussian sums in
 * tile order, so every output is bit-reproducible in the default mode.  scratch: csplat_visibility_scratch_bytes(P, layout_rendered, W, H)
 * bytes per view when any per-Gaussian output is wanted (NULL is fine for top_id alone), no initial state.
 * csplat_visibility_views runs on the join stream, behind views that a finished csplat_forward_views (or _deferred + _settle) filled in,
 * and reads their geom, binning and image chunks.  Errors: V outside 1..64, a pending view (num_rendered < 0), a view launched on faith
 * (valid != NULL), a missing chunk or scratch.  More than 8 views: see "More than 8 views" at csplat_view. */
typedef struct csplat_visibility {
    float *weight_max;     /* [P]     NULL = not wanted */
    float *weight_sum;     /* [P]     NULL = not wanted */
    int32_t *pixel_count;  /* [P]     NULL = not wanted */
    int32_t *top_id;       /* [H][W]  NULL = not wanted */
    void *scratch;         /* csplat_visibility_scratch_bytes(P, R, W, H) bytes, or NULL when only top_id is wanted */
} csplat_visibility;
size_t csplat_visibility_scratch_bytes(int P, int64_t R, int W, int H);
int csplat_visibility_views(int V, const csplat_view *views, const csplat_visibility *outs, void *join_stream);

/* Backward: K7 compositing backward, K8 per-Gaussian backward.
 * out_color is the forward's colour image; dL_dpix[3][H][W] its gradient.  The depth image's gradient is taken by
 * csplat_backward_depth below.
 * scratch: device buffer of csplat_backward_scratch_bytes(P, R) bytes, no initial state: one 64-byte-aligned accumulation record per Gaussian (9 floats
 * used).  ABI 3: K7 adds one 36-byte partial per (list entry, 4x4 pixel BLOCK that blended it) -- the nine lanes that hold the row sums
 * issue one float-atomic request to the Gaussian's record; K8 consumes the records.  In the bit-reproducible mode (csplat_debug_flags
 * bit 8) the buffer also holds one stored 9-float record per (list entry, block), summed per Gaussian in emission order.
 * Gradient outputs (device, fully overwritten): dL_dmean2D[P][3] (NDC units, .z = 0), dL_dconic[P][4],
 * dL_dopacity[P], dL_dcolor[P][3], dL_dmean3D[P][3], dL_dcov3D[P][6], dL_dsh[P][M][3] (may be NULL when
 * colors_precomp was used), dL_dscale[P][3], dL_drot[P][4] (may be NULL when cov3D_precomp was used). */
int csplat_backward(void *stream, int P, int D, int M, int R, const float *bg, int W, int H, const float *means3D,
                    const float *shs, const float *colors_precomp, const float *scales, float scale_modifier,
                    const float *rotations, const float *cov3D_precomp, const float *view, const float *proj,
                    const float *campos, float tanfovx, float tanfovy, const int32_t *radii, const void *geom,
                    const void *binning, const void *image, const float *out_color, const float *dL_dpix, void *scratch,
                    float *dL_dmean2D,
                    float *dL_dconic, float *dL_dopacity, float *dL_dcolor, float *dL_dmean3D, float *dL_dcov3D,
                    float *dL_dsh, float *dL_dscale, float *dL_drot);
/* csplat_backward plus the gradient of the depth image dL_ddepth[1][H][W] (device; NULL = exactly csplat_backward).  The depth image is
 * D = sum_i T_i alpha_i z_i over the blended entries of a pixel (z = view-space depth, no background term; the depth fork of the
 * rasterizer that the reference pins).  Its adjoint adds g (T_i z_i - D_behind_i / (1 - alpha_i)) to dL/dalpha_i (reaching means2D,
 * conic / cov3D / scale / rotation and opacity as the colour term does) and sum_pix g T_i alpha_i (view[2], view[6], view[10]) to
 * dL/dmean3D_i.  Launches: a prepass of per-(segment, pixel) depth partials, the depth variant of K7, the depth variant of K8.
 * scratch: csplat_backward_depth_scratch_bytes(P, R, W, H) bytes, no initial state. */
int csplat_backward_depth(void *stream, int P, int D, int M, int R, const float *bg, int W, int H, const float *means3D,
                          const float *shs, const float *colors_precomp, const float *scales, float scale_modifier,
                          const float *rotations, const float *cov3D_precomp, const float *view, const float *proj,
                          const float *campos, float tanfovx, float tanfovy, const int32_t *radii, const void *geom,
                          const void *binning, const void *image, const float *out_color, const float *dL_dpix, const float *dL_ddepth,
                          void *scratch, float *dL_dmean2D, float *dL_dconic, float *dL_dopacity, float *dL_dcolor, float *dL_dmean3D,
                          float *dL_dcov3D, float *dL_dsh, float *dL_dscale, float *dL_drot);

/* distCUDA2: out[i] = mean of squared distances from point i to its 3 nearest other points. */
int csplat_dist2(void *stream, int P, const float *xyz, float *out);
/* the same result (bit for bit) in O(P * pruned candidates): Morton order + bounding-box pruning as the upstream extension
 * does; temp: csplat_dist2_temp_bytes(P) bytes of device memory, no initial state. */
size_t csplat_dist2_temp_bytes(int P);
int csplat_dist2_ws(void *stream, int P, const float *xyz, float *out, void *temp);

/* Exact k nearest neighbours WITH indices, self excluded by index (coincident points are neighbours at distance 0, as in
 * csplat_dist2).  out_d2[i*K + r], out_idx[i*K + r]: the r-th nearest other point of point i, ascending in (d2, index) -- ties in
 * d2 are broken by the smaller index, which makes the result unique.  Slots r >= P-1 (fewer than K other points): d2 = +inf,
 * idx = -1.  d2 = dx*dx + dy*dy + dz*dz with d = candidate - query, FP contraction off (the arithmetic of csplat_dist2: for
 * K = 3, (d2[0] + d2[1] + d2[2]) / 3.0f is bit-identical to it).  1 <= K <= CSPLAT_KNN_MAX_K; P = 0 is a no-op.  Indices are
 * the caller's.  csplat_knn is the brute-force form, csplat_knn_ws the Morton-order + bounding-box form (the same bits and the
 * same indices; temp: csplat_knn_temp_bytes(P, K) bytes of device memory, no initial state).  Added exports: CSPLAT_ABI_VERSION is unchanged. */
#define CSPLAT_KNN_MAX_K 32
int csplat_knn(void *stream, int P, int K, const float *xyz, float *out_d2, int32_t *out_idx);
size_t csplat_knn_temp_bytes(int P, int K);
int csplat_knn_ws(void *stream, int P, int K, const float *xyz, float *out_d2, int32_t *out_idx, void *temp);
/* Farthest-point sampling.  out_idx[0] = start; out_idx[s] = argmax_i min_{t<s} d2(i, out_idx[t]), the smallest i among equal
 * maxima (numpy's argmax rule); the same d2 arithmetic as above.  min_d2: caller-provided float[N] work array (on return: each
 * point's squared distance to the selected set).  S > N is legal and repeats indices (all min_d2 are 0, argmax is index 0).
 * One workgroup runs all S rounds; 0 <= start < N. */
int csplat_fps(void *stream, int N, int S, const float *xyz, int start, float *min_d2, int32_t *out_idx);

/* Exact k nearest neighbours between TWO clouds.  out_d2[i*K + r], out_idx[i*K + r]: the r-th nearest of `points` [N,3] to
 * query i of `queries` [Q,3], ascending in (d2, index) -- ties in d2 go to the smaller index, so the result is unique.  Nothing
 * is excluded: a query that coincides with a point finds it at distance 0.  Slots r >= N: d2 = +inf, idx = -1.
 * d2 = dx*dx + dy*dy + dz*dz with d = point - query, FP contraction off (the arithmetic of csplat_knn).
 * 1 <= K <= CSPLAT_KNN_MAX_K.  Q = 0 is a no-op; N = 0 fills every slot with (+inf, -1) (`points`, and `temp`, may then be
 * NULL).  Negative sizes, a K outside the range and NULL with non-zero sizes are errors whose text names the entry point.
 * csplat_knn_query is the brute-force form; csplat_knn_query_ws orders the points along a Morton curve, prunes by the bounding
 * boxes of 1024-point runs and orders the queries along the same curve (clamped to the points' bounding box), temp:
 * csplat_knn_query_temp_bytes(Q, N, K) bytes of device memory, no initial state.  Both forms return the same bits and the same indices for
 * every input.  Added exports: CSPLAT_ABI_VERSION is unchanged. */
int csplat_knn_query(void *stream, int Q, int N, int K, const float *queries, const float *points, float *out_d2, int32_t *out_idx);
size_t csplat_knn_query_temp_bytes(int Q, int N, int K);
int csplat_knn_query_ws(void *stream, int Q, int N, int K, const float *queries, const float *points, float *out_d2, int32_t *out_idx,
                        void *temp);

/* One direction of the Chamfer distance from a K = 1 result (d2 [Q], idx [Q]) of csplat_knn_query(queries -> points).
 * w_i = 1 when max_sq_dist < 0 (no cap) or d2[i] <= max_sq_dist, else 0.
 * csplat_chamfer_fwd: loss[0] = (1/Q) sum_i w_i d2[i].  The divisor is always Q; the sum runs in a fixed order inside one
 * workgroup (fp64 accumulation, one rounding at the end).  Q >= 1.
 * csplat_chamfer_bwd: g is a DEVICE scalar, the upstream gradient (no host value enters a launch: the path records into a
 * hipGraph).  dL_dqueries[i] = g (2/Q) w_i (q_i - p_idx[i]); dL_dpoints[j] = - the sum of the same terms over the queries with
 * idx[i] = j, in ascending i (stable sort of (idx, i), one lane sums a run: no float atomics, the result is reproducible bit
 * for bit); every row of dL_dpoints is written, exact zeros for a point nobody selected.  Either output may be NULL.
 * temp: csplat_chamfer_bwd_temp_bytes(Q, N) bytes of device memory, no initial state (needed for dL_dpoints only).  Q >= 1, N >= 1. */
int csplat_chamfer_fwd(void *stream, int Q, const float *d2, float max_sq_dist, float *loss);
size_t csplat_chamfer_bwd_temp_bytes(int Q, int N);
int csplat_chamfer_bwd(void *stream, int Q, int N, const float *queries, const float *points, const float *d2, const int32_t *idx,
                       float max_sq_dist, const float *g, float *dL_dqueries, float *dL_dpoints, void *temp);

/* Neighbourhood regularisers on a K-neighbour graph of N nodes (csplat.knn_regs): isometry, spring and local rigidity of the
 * Gaussian centres M[t] [N,3] and rotations Q[t] [N,4] ((w,x,y,z), not assumed normalised) at the T time rows of a step.
 * The graph: idx [N,K] (neighbour j of pair (i,k)), d0 [N,K] >= 0 (rest distance), w [N,K] >= 0 (weight).  Per pair and row
 *   off_t = M[t][j] - M[t][i],   d_t = |off_t|   (derivative off_t / d_t, 0 where d_t == 0)
 *   L_iso    = mean_t      mean_{i,k} (d_t - d0)            signed; |d_t - d0| with isometric_abs (sign(0) = 0)
 *   L_spring = mean_{t>=1} mean_{i,k} |d_t - d_{t-1}|       (sign(0) = 0)
 *   L_rigid  = mean_{t>=1} mean_{i,k} sqrt(w |R off_t - off_{t-1}|^2 + 1e-20),   R = rotmat(r / |r|),
 *              r = Q[t-1][j] (x) conj(Q[t][j])  (Hamilton product, the NEIGHBOUR's rotations; the normalisation is differentiated)
 *   L = lambda_isometric L_iso + lambda_spring L_spring + lambda_rigidity L_rigid;  T = 1: L_spring = L_rigid = 0.
 * A pair whose idx is outside 0 .. N-1 contributes nothing (the divisors stay N K).  1 <= K <= CSPLAT_KNN_MAX_K, N >= 1,
 * 1 <= T < 65536, N K < 2^31, T N < 2^31; weights >= 0 and finite.  Errors name the entry point.
 *
 * csplat_knn_regs_graph: built once per graph refresh.  With d2 != NULL (the squared distances of csplat_knn) it writes
 * d0 = sqrt(d2) and w = exp(-lambda_w d2) (exponent and exp in fp64, rounded once); with d2 == NULL d0 / w are the caller's.
 * Always: the REVERSE lists -- rev_offsets [N+1], rev_entries [N K]: rev_entries[rev_offsets[j] .. rev_offsets[j+1]) are the
 * pair numbers i K + k with idx[i,k] == j in ascending order (integer counts + csplat_scan, stable csplat_sort_pairs).
 * temp: csplat_knn_regs_graph_temp_bytes(N, K) bytes, no initial state, 16-byte aligned, as rev_offsets.
 *
 * csplat_knn_regs_fwd: ONE kernel launch; out4 = (L_iso, L_spring, L_rigid, L) on the device.  rotations == NULL: L_rigid = 0
 * and w is not read.  The sums run in fp64 in a fixed order (per-workgroup partials over contiguous pair ranges, joined by
 * the last workgroup in index order): the result does not depend on scheduling, stream or graph replay.
 * scratch: csplat_knn_regs_fwd_scratch_bytes() bytes, 16-byte aligned, any contents; not shared by launches that may overlap.
 *
 * csplat_knn_regs_bwd: g is a DEVICE scalar (dL/dL; the path records into a hipGraph).  Gather-only, no float atomics:
 * dL_dmeans[t][n] = the fixed-order sum over n's K own pairs and the pairs of its reverse list, every pair quantity
 * recomputed; dL_drotations[t][n] from the reverse list alone, exact zeros where it is empty.  Either output may be NULL.
 * With lambda_rigidity == 0 the rotations are not read (and may be NULL); a dL_drotations given then is cleared. */
size_t csplat_knn_regs_graph_temp_bytes(int N, int K);
int csplat_knn_regs_graph(void *stream, int N, int K, const int32_t *idx, const float *d2, double lambda_w, float *d0, float *w,
                          int32_t *rev_offsets, int32_t *rev_entries, void *temp);
size_t csplat_knn_regs_fwd_scratch_bytes(void);
int csplat_knn_regs_fwd(void *stream, int T, int N, int K, const float *means, const float *rotations, const int32_t *idx,
                        const float *d0, const float *w, float lambda_isometric, float lambda_spring, float lambda_rigidity,
                        int isometric_abs, float *out4, void *scratch);
int csplat_knn_regs_bwd(void *stream, int T, int N, int K, const float *means, const float *rotations, const int32_t *idx,
                        const float *d0, const float *w, const int32_t *rev_offsets, const int32_t *rev_entries,
                        float lambda_isometric, float lambda_spring, float lambda_rigidity, int isometric_abs, const float *g,
                        float *dL_dmeans, float *dL_drotations);

/* Separable 11-tap window of the SSIM loss (utils/loss_utils.py:30-58), zero padded: out = G (x) G * in for every one of
 * the n_images [H][W] planes.  taps11 is a HOST pointer to the 11 normalised window weights.  Self-adjoint: the backward
 * of the operator is the operator.  (SURVEY.md 8(f) "next" row N2.) */
int csplat_blur11(void *stream, int64_t n_images, int H, int W, const float *taps11, const float *in, float *out);

/* One Adam step (torch.optim.Adam semantics: no weight decay, no amsgrad, maximize = false) over n_tensors fp32 tensors in a
 * single launch per CSPLAT_ADAM_MAX_TENSORS tensors.  Host arrays of device pointers / element counts / per-tensor learning
 * rates (doubles, combined in double before the cast to fp32 as torch does; the reference keeps one parameter group per Gaussian attribute, /root/reference/scene_reconstruction/
 * gaussian_mesh.py:126-136, stepped at train_utils.py:310-319).  `step` is the 1-based step count AFTER this update. */
#define CSPLAT_ADAM_MAX_TENSORS 48
int csplat_adam_step(void *stream, int n_tensors, float *const *params, const float *const *grads, float *const *exp_avg,
                     float *const *exp_avg_sq, const int64_t *numel, const double *lr, double beta1, double beta2, double eps,
                     int64_t step);
/* The same step with NOTHING of the launch depending on a per-step host value (for a training step recorded into a hipGraph):
 * state_dev[0] (int32, device) = steps taken so far -- the kernel uses state_dev[0] + 1 for its bias corrections and a trailing
 * one-thread launch advances it; lr_dev = the tensors' learning rates as doubles in device memory; valid_dev (may be NULL) = a device
 * word: 0 there -> parameters, moments and the step count are left untouched.  One launch per CSPLAT_ADAM_MAX_TENSORS tensors
 * (all of them read the same count), then the one that advances the count. */
int csplat_adam_step_dev(void *stream, int n_tensors, float *const *params, const float *const *grads, float *const *exp_avg,
                         float *const *exp_avg_sq, const int64_t *numel, const double *lr_dev, double beta1, double beta2, double eps,
                         int *state_dev, const uint32_t *valid_dev);
/* dst[...] (float, device) = the concatenation of n <= 32 small device arrays, src[i] holding count[i] values of kind[i] (0 = float,
 * 1 = int32 / uint32 converted to float, exact below 2^24; 2 = int32 / uint32 copied BIT FOR BIT -- read the slot back as an integer:
 * instance counts exceed 2^24 on large scenes): one launch that collects a recorded step's log line -- step count, go / no-go
 * word, PSNR, loss, the views' instance counts -- for ONE copy to pinned host memory. */
int csplat_gather_words(void *stream, int n, const void *const *src, const int *kind, const int *count, float *dst);

/* Capacity-based densify / prune: replaces the boolean-mask indexing / torch.cat re-creation of every
 * parameter and Adam moment in /root/reference/scene_reconstruction/gaussian_model.py:266-341 and gaussian_mesh.py:336-431.
 *   csplat_mask_to_map: map[i] = base + (number of set mask bytes before i) where mask[i] != 0, else -1; *count_dev = number of
 *                       set bytes (device int32).  Stable.  temp: csplat_mask_to_map_temp_bytes(n) bytes, no initial state.
 *   csplat_rows_scatter: for every tensor t and source row i with map[i] >= 0: dst[t][map[i]] = src[t][i] (row_bytes[t] bytes,
 *                       a multiple of 4); src[t] == NULL writes zeros (fresh Adam moments of appended rows).  ONE launch for up
 *                       to CSPLAT_ROWS_MAX_TENSORS tensors.  Source and destination rows must not overlap (ping-pong buffers
 *                       for compaction, rows beyond the live range for appends).  src / dst / row_bytes are HOST arrays. */
#define CSPLAT_ROWS_MAX_TENSORS 32
size_t csplat_mask_to_map_temp_bytes(int64_t n);
int csplat_mask_to_map(void *stream, int64_t n, const uint8_t *mask, int32_t base, int32_t *map, int32_t *count_dev, void *temp);
int csplat_rows_scatter(void *stream, int n_tensors, const void *const *src, void *const *dst, const int64_t *row_bytes,
                        int64_t n_rows, const int32_t *map);

/* Output layer of the time-conditioned simulator MLP, T time rows at once (/root/reference/meshnet/meshnet_network.py:
 * 339 `self.output = Linear(256, n_nodes * 3)`, applied at :367 to ONE time value per render() call; a training step makes
 * T = 3 such calls, train_utils.py:204-260):
 *   forward:  y[t][r] = b[r] + sum_k W[r][k] h[t][k]               W [R][K] row-major (torch Linear.weight), h [T][K], y [T][R]
 *   backward: dW[r][k] = sum_t dy[t][r] h[t][k], db[r] = sum_t dy[t][r], dh[t][k] = sum_r dy[t][r] W[r][k]   (deterministic)
 * K must be 256, 0 <= T <= 8 (T = 0 or R = 0: nothing is written).  W, h, dW and scratch are accessed 16 bytes at a time and must be
 * 16-byte aligned (refused otherwise).  scratch: csplat_rows_dot_scratch_bytes(T) bytes, contents irrelevant, not shared between
 * concurrent calls.  Non-finite data propagate as in the sums above: a NaN in h[t] reaches y[t][:], an Inf in W[r] reaches y[:][r]. */
/* The two hidden layers in front of it (meshnet_network.py:337-338,364-366), for the same T time rows, one launch each way:
 *   forward : h1 = relu(e W1^T + b1) [T][256], h2 = relu(h1 W2^T + b2) [T][256]      e [T][K0] (the sinusoidal code, K0 <= 16),
 *             W1 [256][K0], W2 [256][256] row-major (torch Linear.weight)
 *   backward: from dh2 = dL/dh2 [T][256]: dW1 [256][K0], db1 [256], dW2 [256][256], db2 [256]   (e has no gradient: parameter-free code)
 * 1 <= T <= 8, 1 <= K0 <= 16; W2 16-byte aligned.  relu(x) = x < 0 ? 0 : x, torch.relu's values: -0.0 stays -0.0, a NaN stays a NaN (a NaN in e[t] makes rows t of h1 and h2 NaN,
 * a NaN in a row of W1 that unit of h1 in every row and all of h2), its derivative at 0 is 0.  The order of every sum does not depend
 * on T: row t of a T-row call has the bits of the same row in any other call. */
int csplat_sim_hidden_fwd(void *stream, int T, int K0, const float *e, const float *W1, const float *b1, const float *W2, const float *b2,
                          float *h1, float *h2);
/* scratch: csplat_sim_hidden_scratch_bytes(T) bytes whose first word (the ticket) is zero on entry and left at zero: one buffer of
 * csplat_sim_hidden_scratch_bytes(8) bytes serves calls of any T in a row; not shared between calls that may run concurrently */
size_t csplat_sim_hidden_scratch_bytes(int T);
int csplat_sim_hidden_bwd(void *stream, int T, int K0, const float *e, const float *W2, const float *h1, const float *h2, const float *dh2,
                          float *dW1, float *db1, float *dW2, float *db2, void *scratch);
size_t csplat_rows_dot_scratch_bytes(int T);
/* add: NULL, or [T][R] added to the result (the simulator's `mesh_predictions[time_id] + residual`, meshnet_network.py:371) */
int csplat_rows_dot_fwd(void *stream, int T, int R, int K, const float *W, const float *b, const float *h, float *y, const float *add);
int csplat_rows_dot_bwd(void *stream, int T, int R, int K, const float *W, const float *h, const float *dy, float *dW, float *db,
                        float *dh, void *scratch);

/* The cloth regularisers of the reconstruction loss with their gradient in one pass (/root/reference/scene_reconstruction/
 * train_utils.py:83-102): D [T][V][3] deformed vertices of the step's T cameras, edge_index [2][E] int64, rest_len [E]:
 *   *loss = lambda_deform * 0.5 * (mean_v |D1-D0|_2 + mean_v |D2-D1|_2)          (only when T >= 3)
 *         + lambda_rigid * mean_{t,e} | rest_len[e] - |D[t][edge_index[1][e]] - D[t][edge_index[0][e]]|_2 |
 *         + lambda_momentum * mean_v |D2 - 2 D1 + D0|_1                          (only when T >= 3)
 *   grad [T][V][3] = d loss / d D (norms have gradient 0 at 0, as torch defines them; sign(0) = 0).  The two node terms read time
 *   rows 0, 1 and 2 only, whatever T >= 3 is: rows 3 .. T-1 get the rigidity gradient alone.  With no active term (all lambdas 0, or
 *   only node terms at T < 3) *loss = 0 and grad is zeroed in either form.
 * scratch: csplat_cloth_regs_scratch_bytes(T, V, E) bytes (enough for either form), ZERO before the first call; the ticket word in its
 * last 256 bytes is left at zero by every call, so one buffer serves calls of the same (T, V, E) in a row; not shared between
 * concurrent calls.  The loss value is summed in a fixed order.  Gradient: with the CSR of the graph (dst_rowptr / src_rowptr [V+1], dst_perm / src_perm [E], int32: edge ids
 * grouped by edge_index[1] / edge_index[0], ascending within a group; the two perm lists may be NULL when E = 0) every vertex gathers
 * its edges -- deterministic, no atomics; with NULLs the edges scatter with float atomics (summation order not fixed). */
size_t csplat_cloth_regs_scratch_bytes(int T, int V, int64_t E);
int csplat_cloth_regs(void *stream, int T, int V, int64_t E, const float *D, const int64_t *edge_index, const float *rest_len,
                      float lambda_deform, float lambda_rigid, float lambda_momentum, float *loss, float *grad, void *scratch,
                      const int *dst_rowptr, const int *dst_perm, const int *src_rowptr, const int *src_perm);

/* Pixel coordinates of n world points (the `projections` by-product of render(), /root/reference/gaussian_renderer/__init__.py:
 * 166-179): hom = [p, 1] @ full_proj (device pointer to the row-major 4x4 the reference keeps as Camera.full_proj_transform),
 * ndc = hom.xy / hom.w, out = ((ndc + 1) * (W, H) - 1) / 2.  points [n][3], out_pixels [n][2]. */
int csplat_project_points(void *stream, int64_t n, const float *full_proj, int W, int H, const float *points, float *out_pixels);

/* psnr of /root/reference/utils/image_utils.py:19-21 per image: out[i] = 20 log10(1 / sqrt(mean((a_i - b_i)^2))) over the
 * n_per_image values (channels x pixels) of image i; a, b [n_images][n_per_image].  One launch; fixed summation order.
 * scratch: csplat_psnr_scratch_bytes(n_images) bytes, no initial state (the entry clears its tickets on the stream), not shared between concurrent calls. */
size_t csplat_psnr_scratch_bytes(int64_t n_images);
int csplat_psnr(void *stream, int64_t n_images, int64_t n_per_image, const float *a, const float *b, void *scratch, float *out);

/* SSIM of /root/reference/utils/loss_utils.py:40-70 (window 11, sigma 1.5, zero padding, size_average) on n_images [H][W]
 * planes (n_images = batch * channels), fused:
 *   forward:  map[i] = SSIM(x, y)[i] (optional), partial[b] = sum of the map over workgroup b's tile
 *             (csplat_ssim_partial_count() floats; mean = sum(partial) / (n_images*H*W), summed by the caller in a fixed
 *             order), and p1, p2, p3 = dSSIM/dblur(x), dSSIM/dblur(x*x), dSSIM/dblur(x*y) per pixel (all three or NULL).
 *   backward: dx[i] = g_scalar[0] * inv_n * ( blur(p1) + 2 x blur(p2) + y blur(p3) )[i]   (gradient w.r.t. x only)
 *                     + add_scale[0] * addend[i]   when addend / add_scale (device pointers) are given: the gradient of the
 *             reference's whole image loss Ll1 + lambda_dssim (1 - ssim) (train_utils.py:50-74) leaves in one pass, addend =
 *             the sign(x - y) / n that csplat_l1 wrote.
 * taps11: the 11 host floats of the 1-D window, as csplat_blur11. */
size_t csplat_ssim_partial_count(int64_t n_images, int H, int W);
int csplat_ssim_fwd(void *stream, int64_t n_images, int H, int W, const float *taps11, const float *x, const float *y,
                    float *p1, float *p2, float *p3, float *map_out, float *partial);
int csplat_ssim_bwd(void *stream, int64_t n_images, int H, int W, const float *taps11, const float *x, const float *y,
                    const float *p1, const float *p2, const float *p3, const float *g_scalar, float inv_n,
                    const float *addend, const float *add_scale, float *dx);
/* masked form of the reference's image loss (train_utils.py:61-67: `((1.0 - ssim_map) * mask_tensor).mean()`): x, y
 * [n_batch][channels][H][W], mask [n_batch][mask_channels][H][W] with mask_channels = 1 (Camera.mask, broadcast over the
 * colour channels) or = channels.  partial sums hold sum((1 - SSIM) * mask) over the workgroup's tile (the loss term is
 * sum(partial) / (n_batch*channels*H*W)); p1..p3 are pre-multiplied by the mask, so csplat_ssim_bwd (g_scalar = MINUS the
 * incoming gradient of the loss term) serves both forms. */
int csplat_ssim_fwd_masked(void *stream, int64_t n_batch, int channels, int H, int W, const float *taps11, const float *x,
                           const float *y, const float *mask, int mask_channels, float *p1, float *p2, float *p3,
                           float *map_out, float *partial);
/* The densification statistics of a training step (/root/reference/scene_reconstruction/train_utils.py:276-285:
 * `radii = torch.cat(radii_list, 0).max(dim=0).values`, `visibility_filter = torch.cat(visibility_filter_list).any(dim=0)`, the
 * viewspace-gradient sum over the step's cameras) in one launch.  mean2d_grads / radii: HOST arrays of V (<= 16) device pointers,
 * [P][3] float / [P] int32 each (a NULL gradient entry counts as zero); outputs: grad_sum [P][3], radii_max [P], visible [P] (0 / 1
 * bytes).  grad_sum or (radii_max, visible) may be NULL. */
int csplat_step_stats(void *stream, int64_t P, int V, const float *const *mean2d_grads, const int *const *radii, float *grad_sum,
                      int *radii_max, uint8_t *visible);
/* The whole image loss of a training step in two launches forward, one backward -- the reference's Ll1 + lambda_dssim * (1 - ssim) (masked:
 * mean|(x - y) m| + lambda_dssim * mean((1 - ssim_map) m)), /root/reference/scene_reconstruction/train_utils.py:50-74, the per-camera
 * PSNR it logs every step (:262-283, utils/image_utils.py:17-21, unmasked) and the sum with one more device scalar (the regularisers,
 * :76-237):
 *   out[0] = img_weight * image_loss + add_weight * add[0]   (add may be NULL)      out[1] = psnr_scale * sum_b PSNR_b
 *   out[2] = image_loss                                                              out[3] = Ll1
 * x, y [n_batch][channels][H][W]; mask NULL or [n_batch][mask_channels][H][W] (mask_channels 1 or channels).  p1..p3 (float images) and
 * sign8 (one byte per element) are what csplat_image_loss_bwd needs; all four NULL = no gradient wanted.  scratch:
 * csplat_image_loss_scratch_bytes bytes (no initial state, not shared between concurrent calls).  Bit-reproducible (workgroup
 * partials summed in index order by a one-workgroup second launch).
 * csplat_image_loss_bwd: dx = g_scalar[0] * img_weight * d(image_loss)/dx. */
size_t csplat_image_loss_scratch_bytes(int64_t n_batch, int channels, int H, int W);
int csplat_image_loss_fwd(void *stream, int64_t n_batch, int channels, int H, int W, const float *taps11, const float *x,
                          const float *y, const float *mask, int mask_channels, float lam, float img_weight, const float *add,
                          float add_weight, float psnr_scale, float *p1, float *p2, float *p3, signed char *sign8, void *scratch,
                          float *out);
int csplat_image_loss_bwd(void *stream, int64_t n_batch, int channels, int H, int W, const float *taps11, const float *x,
                          const float *y, const float *p1, const float *p2, const float *p3, const signed char *sign8,
                          const float *mask, int mask_channels, float lam, float img_weight, const float *g_scalar, float *dx);
/* l1_loss of /root/reference/utils/loss_utils.py:20-23 with its gradient in the same pass:
 *   *loss = mean_i |a[i] - b[i]|,   grad[i] = sign(a[i] - b[i]) / n   (grad may be NULL).
 * csplat_l1_masked: *loss = mean_i |(a[i] - b[i]) * m[i]|, grad[i] = sign((a-b)*m) * m / n, with the mask laid out as for
 * csplat_ssim_fwd_masked (hw = H*W values per plane).
 * scratch: csplat_l1_scratch_bytes() bytes whose last word is zero on entry (the kernel restores it), not shared between
 * calls that may run concurrently.  Deterministic (fixed summation order).  a, b, mask and grad need only their natural 4-byte
 * alignment (a contiguous view into a batch with odd plane sizes): 16-byte groups are used when all of them are 16-byte aligned,
 * element-wise accesses otherwise (csplat_l1_signs_bwd: likewise for its mask; out is 16-byte aligned). */
size_t csplat_l1_scratch_bytes(void);
int csplat_l1(void *stream, int64_t n, const float *a, const float *b, void *scratch, float *loss, float *grad);
int csplat_l1_masked(void *stream, int64_t n_batch, int channels, int64_t hw, const float *a, const float *b, const float *mask,
                     int mask_channels, void *scratch, float *loss, float *grad);
/* The same loss for a caller that runs the backward later (autograd, `loss.backward()` of train_utils.py:288): the forward keeps ONE
 * BYTE per element, sign8[i] = sign((a[i] - b[i]) * m[i]) in {-1, 0, 1}, instead of a float gradient image, and
 *   csplat_l1_signs_bwd: out[i] = g_scalar[0] * sign8[i] * m[i] / n     (g_scalar: the incoming gradient of the loss, a device scalar)
 * is the whole backward -- no separate multiply by the incoming gradient.  mask may be NULL (then mask_channels is ignored). */
int csplat_l1_signs(void *stream, int64_t n_batch, int channels, int64_t hw, const float *a, const float *b, const float *mask,
                    int mask_channels, void *scratch, float *loss, signed char *sign8);
int csplat_l1_signs_bwd(void *stream, int64_t n_batch, int channels, int64_t hw, const signed char *sign8, const float *mask,
                        int mask_channels, const float *g_scalar, float *out);
/* Depth and silhouette supervision of a training step on the rasterizer's depth image D = sum_i T_i alpha_i z_i (view-space z, no
 * background term) and alpha image A = 1 - T_final (csplat_view.out_depth / out_alpha), two launches forward and one backward.  The reference
 * has no such loss.  The n_views views of a step are all of hw = H * W pixels, n = n_views * hw, and arrive as tables of n_views device
 * pointers, one float image per view: depth (D), alpha (A), gt_depth (Z: measured z-depth in scene units), silhouette (S in [0, 1], 1 =
 * cloth), mask (M: the camera's mask, 1 = keep).  gt_depth, silhouette and mask may each be NULL: no Z = no depth term (depth may then be
 * NULL too), no S = no silhouette term, no M = 1 everywhere.  A term is on when its table is given and its weight is > 0; with no term on
 * the call returns an argument error and launches nothing.
 *   valid   = isfinite(Z) and Z > 0                    (a hole in a sensor map is 0, negative, NaN or Inf)
 *   w_d     = valid ? M : 0                            w_s = M
 *   r_d     = D - A Z   (= sum_i T_i alpha_i (z_i - Z): no division by alpha; formed with ONE fused multiply-add, so that its sign is exact)
 *   r_s     = A - S
 *   L_depth = (1/n) sum_{w_d != 0} |r_d w_d|           L_sil = (1/n) sum_{w_s != 0} |r_s w_s|
 *   out[0]  = weight * (lambda_depth L_depth + lambda_silhouette L_sil) + add_weight * add[0]   (add may be NULL)
 *   out[1]  = L_depth        out[2] = L_sil            (0 for a term that is off)
 *   d_depth = g weight lambda_depth w_d sign(r_d w_d) / n
 *   d_alpha = g weight (-lambda_depth w_d Z sign(r_d w_d) + lambda_silhouette w_s sign(r_s w_s)) / n       (g = g_scalar[0], on the device)
 * SELECTION, not multiplication: a pixel with w == 0 adds exactly 0 and gets exactly 0 gradient whatever D, A, Z hold there (NaN, Inf);
 * a NaN in D or A where w != 0 makes that term (and that pixel's gradient) NaN.  sign(0) = 0, as in csplat_l1_signs: pixels where nothing
 * blended (D = A = 0) are exact ties of r_d.  The division is by n, ALL pixels of the call (the convention of the reference's masked L1,
 * abs((x - y) * mask).mean(), utils/loss_utils.py:20-23).
 * sign8 [n_views][hw]: one byte per pixel, bits 0-1 the code of sign(r_d w_d), bits 2-3 of sign(r_s w_s) (0: -1, 1: 0, 2: +1, 3: NaN);
 * NULL = no gradient wanted, nothing is stored.  d_depth / d_alpha [n_views][hw] floats, either may be NULL.  scratch:
 * csplat_geom_loss_scratch_bytes bytes, no initial state, not shared between concurrent calls.  Bit-reproducible: workgroup partials summed
 * in index order by a one-workgroup second launch, no float atomics.  More than 16 views run as one launch per 16 (the kernel's table
 * size) with the same result.  Every image needs 4-byte alignment; 16-byte accesses are used when all of them (and d_depth / d_alpha)
 * are 16-byte aligned and hw is a multiple of 4. */
size_t csplat_geom_loss_scratch_bytes(int n_views, int64_t hw);
int csplat_geom_loss_fwd(void *stream, int n_views, int64_t hw, const float *const *depth, const float *const *alpha,
                         const float *const *gt_depth, const float *const *silhouette, const float *const *mask, float lambda_depth,
                         float lambda_silhouette, float weight, const float *add, float add_weight, unsigned char *sign8, void *scratch,
                         float *out);
int csplat_geom_loss_bwd(void *stream, int n_views, int64_t hw, const unsigned char *sign8, const float *const *gt_depth,
                         const float *const *mask, float lambda_depth, float lambda_silhouette, float weight, const float *g_scalar,
                         float *d_depth, float *d_alpha);
/* Optical-flow supervision of the Gaussians' motion between the frames of a training step, two launches forward and one backward
 * (csplat_flow_loss.hip).  Added exports: CSPLAT_ABI_VERSION is unchanged.  The reference carries flow images as far as an unfinished
 * `flow_loss` that prints (train.py:52-90); this is that term.
 * FRAMES, PAIRS, PROJECTION.  T = n_frames frames, 2 <= T <= 16, of P Gaussians.  Frame t has centres X_t [P][3] and full_t [16], row-major
 * in the reference's transposed convention, hom = [X, 1] @ full, as csplat_project_points takes it; all frames share one image size W x H.
 * Pair t = 0..T-2 is (frame t -> frame t+1) with the flow image F_t [2][H][W]: channel 0 is dx in pixels (+x to the right), channel 1 dy,
 * defined at the pixels of frame t (RAFT's convention).  Projection as gaussian_renderer._project: x = ((hom_x / w + 1) W - 1) / 2,
 * y likewise with H; pixel centres sit at the integers.
 * PER PAIR t AND GAUSSIAN i.  p_a = projection of X_t[i] with full_t, p_b = projection of X_{t+1}[i] with full_{t+1}.
 *   g = bilinear(F_t, p_a): x0 = floor(x), x1 = min(x0 + 1, W - 1), fx = x - x0, the same in y (at x = W - 1 the clamped tap weighs 0)
 *   m = M_t[floor(y + 0.5)][floor(x + 0.5)] clamped to the image; M_t [H][W] the optional camera mask of frame t, m = 1 without a table
 *   r = (p_b - p_a) - g          e = |r_x| + |r_y|
 * The pair is VALID iff visible_t[i] > 0 and visible_{t+1}[i] > 0 (int32 [P] per frame, the rasterizer's radii; the table or an entry
 * may be NULL: visible), w_a > 0 and w_b > 0, p_a and p_b finite, 0 <= x_a <= W - 1 and 0 <= y_a <= H - 1, all four taps of both
 * channels finite (a NaN / Inf flow pixel means "no flow here"), m finite and > 0, and -- when max_error > 0 -- e <= max_error.
 *   L_flow   = (1/n) sum_valid m e,  n = (T - 1) P: ALL pairs, the convention of csplat_geom_loss_fwd
 *   out[0]   = weight lambda L_flow + add_weight add[0]   (add may be NULL)        out[1] = L_flow        count[0] = valid pairs (int32)
 * SELECTION, not multiplication: an invalid pair adds exactly 0 and gets exactly 0 gradient whatever its inputs hold.  sign(0) = 0.
 * GRADIENT: the full analytic one, the sample's dependence on p_a included.  With s = m (sign r_x, sign r_y): dL/dp_b = s,
 * dL/dp_a = -(I + J_g)^T s, J_g the 2 x 2 Jacobian of the bilinear sample in its cell (floor convention); then through the projection,
 * dx/dX_k = (W/2) (full[k][0] - ndc_x full[k][3]) / w and likewise y.  The mask lookup and every validity decision are constants.  A
 * middle frame receives the sum of its role as b of pair t-1 and as a of pair t.
 * Tables are host arrays of device pointers: points and full_proj T entries, flow T-1, visible T or NULL, mask T-1 or NULL.
 * unit [T][P][3]: dL_flow/dX_t[i] (divided by n), each element written once, no atomics; NULL = no gradient wanted, nothing is stored.
 * csplat_flow_loss_bwd: d_points[t][i][c] = g_scalar[0] weight lambda unit[t][i][c] (g_scalar on the device; a unit of 0 gives 0).
 * scratch: csplat_flow_loss_scratch_bytes bytes, no initial state, not shared between concurrent calls.  Bit-reproducible: workgroup
 * partials summed in index order by a one-workgroup second launch, no float atomics.  Argument errors, before any launch: n_frames
 * outside 2..16, P < 1, W < 1 or H < 1, lambda < 0, max_error NaN, a NULL required table, entry or output, an operand that is not
 * 4-byte aligned, (T - 1) P >= 2^31. */
size_t csplat_flow_loss_scratch_bytes(int n_frames, int64_t P);
int csplat_flow_loss_fwd(void *stream, int n_frames, int64_t P, int W, int H, const float *const *points,
                         const float *const *full_proj, const float *const *flow, const int *const *visible, const float *const *mask,
                         float max_error, float lambda, float weight, const float *add, float add_weight, float *unit, void *scratch,
                         float *out, int *count);
int csplat_flow_loss_bwd(void *stream, int n_frames, int64_t P, const float *unit, float lambda, float weight, const float *g_scalar,
                         float *d_points);
/* Point tracking, the evaluation end of the pipeline (csplat_tracking.hip).  Added exports: CSPLAT_ABI_VERSION is unchanged.  They restate
 * the reference's `project` and `get_mask` (render.py:77-121) for all view-frames of a tracking run in one launch, and the `align_traj` +
 * `compute_mte` loop of scripts/align_eval_trajs.py for all ground-truth tracks in one launch (plus a one-workgroup mean).  No gradients.
 *
 * csplat_track_visibility: F view-frames (1 <= F <= 65535) of N points; every array is stacked and contiguous.  Per frame f and point i,
 * with X = points[f][i], full = full_proj[f] (row-major, the reference's transposed convention: hom = [X, 1] @ full), c = cam_center[f]:
 *   PIXEL     pixels_in == NULL: the arithmetic of csplat_project_points, x = ((hom_x / w + 1) W - 1) / 2, y likewise with H;
 *             pixels_in given: (x, y) = pixels_in[f][i], nothing is projected (the get_mask form, which receives projections)
 *   in_image  0 <= x < W and 0 <= y < H, both finite -- and, when projecting, w > 0.  The reference has no test of w: a point behind
 *             the camera is mirrored into the image there and can count as visible.  A deliberate divergence, as csplat_flow_loss_fwd's
 *   d         depth[f][(int)y][(int)x], C truncation (the reference's astype(int)); then d < min_depth gives d = far_value (render.py:
 *             171, 206: `depth[depth < 1.0] = 10e3`).  min_depth <= 0 (or NaN) switches that rule off
 *   visible   in_image and (||X - c||_2 - depth_threshold) <= d: a EUCLIDEAN distance against the rendered (alpha-weighted z) depth,
 *             as the reference compares them.  A NaN depth or a NaN point gives not visible.  depth == NULL: visible = in_image
 *   counts    counts[f] = (points in the image, points visible), int32.  Of the two forms the design allowed, the finishing launch was
 *             chosen over integer atomics: a second launch, one workgroup per frame, sums the frame's in_image and visible bytes.
 *             INTEGER sums, the same in any order; no atomics of any kind (atomics of all workgroups into the one cache line that
 *             holds counts cost 88 us of a 97 us call at 100 000 points x 12 frames)
 * Every load is unconditional with its index clamped into the arrays; an invalid point is selected out.  pixels_out [F][N][2] (NULL:
 * not stored), in_image / visible [F][N] bytes 0 / 1, counts [F][2] (NULL: not formed).  Bit-reproducible.  N == 0 returns at once.
 * Argument errors, before any launch: F outside 1..65535, N < 0 or >= 2^31, W < 1 or H < 1, W * H >= 2^31, a NULL points, full_proj,
 * cam_center, in_image or visible, depth_threshold or far_value NaN, a float operand that is not 4-byte aligned.
 *
 * csplat_track_mte: T >= 1 frames, N tracked points, G ground-truth tracks; track g is associated with point j = assoc[g] (int32; the
 * caller guarantees 0 <= j < N, the kernel clamps j so that no load can leave the arrays).  With R_k = the rotation matrix of the
 * quaternion rotations[k][j], r first, normalised inside (build_rotation, scripts/align_eval_trajs.py:9-27):
 *   t0 = gt[0][g] - traj[0][j]        aligned[0][g] = traj[0][j] + t0        aligned[k][g] = traj[k][j] + (R_k R_0^T) t0   (k >= 1)
 *   err[k][g] = ||gt[k][g] - aligned[k][g]||_2        mte[g] = (sum_k err[k][g]) / T, summed in increasing k
 *   mean[0] = (sum_g mte[g]) / G, formed by a second, one-workgroup launch in a fixed order
 * rotations == NULL: no alignment, aligned[k][g] = traj[k][j] (render.py's own `deform[gt_idxs]`).  A ZERO quaternion normalises to NaN
 * and makes its track's aligned positions, errors and the mean NaN, as in the reference; it is not guarded.  aligned [T][G][3], err
 * [T][G], mte [G], mean [1]; aligned and err may be NULL.  Bit-reproducible, no atomics.  N == 0 or G == 0 returns at once.  Argument
 * errors: T < 1, N or G < 0 or >= 2^31, a NULL traj, gt, assoc, mte or mean, an operand that is not 4-byte aligned. */
int csplat_track_visibility(void *stream, int F, int64_t N, int W, int H, const float *points, const float *pixels_in,
                            const float *full_proj, const float *cam_center, const float *depth, float depth_threshold, float min_depth,
                            float far_value, float *pixels_out, uint8_t *in_image, uint8_t *visible, int *counts);
int csplat_track_mte(void *stream, int T, int64_t N, int64_t G, const float *traj, const float *rotations, const float *gt,
                     const int *assoc, float *aligned, float *err, float *mte, float *mean);

/* Planning, the control end of the pipeline (csplat_plan.hip).  Added exports: CSPLAT_ABI_VERSION is unchanged.  What a model-predictive
 * planner needs around the batched MeshNet rollout: the reference rolls the GNN out for A candidate action sequences as one
 * block-diagonal graph (meshnet/dataloader_sim.py:248-288), takes (pos - goal).pow(2).mean() per candidate (manipulation/planning.py:425)
 * and executes the cheapest (:311).  Its MPC class is not shipped; these entries restate the cost and supply a cross-entropy-method update.
 *
 * Batched state, PyG's Batch layout: node n of candidate b is row b * N + n.  pos [B*N][3], hist [H][B*N][3] (oldest first), actions
 * [B][T][3], goal [N][3] shared by all candidates, node_w [N] or NULL (all ones), cost [B].  Plain loads and vector stores, NO atomics:
 * every output is bit-reproducible.  Every entry validates its arguments before any launch (a bad one returns non-zero and
 * csplat_last_error() names the entry) and does nothing, returning 0, for an empty problem.  Operands are 4-byte aligned.
 *
 * csplat_plan_integrate: the tail of rollout step k (0 <= k < T, by value) for all candidates, the batched twin of
 * csplat_rollout_integrate: v[b*N + grasped] = actions[b][k] (a grasped index outside [0, N) pins NOTHING); pos += v;
 * hist <- (hist[1:], v); preds[k][b*N + n] = v when preds != NULL (preds [steps][B*N][3], steps > k).  With goal != NULL also
 *   cost[b] += step_w[k] * (1 / 3N) * sum_{n,c} node_w[n] * (pos_new[b][n][c] - goal[n][c])^2
 * step_w [T], or NULL = 1 at k == T-1 and 0 before it -- an earlier step then forms no term and leaves cost untouched; with node_w == NULL
 * this is planning.py:425 on the final state.  cost is zeroed by the caller before step 0.  ONE workgroup owns a candidate's cost word and
 * sums its 3N terms in an order fixed by N alone (thread t its elements t, t + 256, .. in increasing index; a xor tree over each wave;
 * the waves in order; / 3N; * the weight; added to cost[b]): a candidate's cost is a function of its own positions, bit for bit,
 * independent of B and of b.  Elementwise arithmetic without contraction, in torch's order.  B * N < 2^29, H >= 1, T >= 1.
 *
 * csplat_plan_cost: the same term on stored positions pos [B][N][3]: cost[b] = (accumulate ? cost[b] : 0) + w * (1 / 3N) * sum ...
 * It shares the device function with csplat_plan_integrate: for equal positions and an equal weight the two give bit-equal terms, so a
 * cost formed after the rollout (w = 1, accumulate = 0) EQUALS the one accumulated under the default step_w.
 *
 * csplat_plan_select: B <= 65536 costs, K <= B: order[r] (int32) = the index of the r-th smallest cost, best[r] = that cost as stored.
 * A total order: numbers ascending with -0.0 == 0.0, +inf before every NaN, NaN last; equal costs (and all NaN) by ascending index --
 * torch.sort(cost, stable=True) truncated to K.  Each candidate's rank is counted against LDS tiles of the cost vector (B^2 compares:
 * no global sort); the ranks are a permutation, so every output slot is written once.
 *
 * csplat_plan_refit_sample: one cross-entropy-method update.  actions [B][T][3] (in/out), order [K] (the elite rows; an index outside
 * [0, B) is clamped), mu / sigma [T][3] (in/out), noise [B][T][3] (standard normal, drawn by the caller; row 0 is not read).  Per (t, c),
 * sums over the elites in the order r = 0 .. K-1:
 *   m = (sum_r a_r) / K          s = sqrt((sum_r (a_r - m)^2) / K)          a_r = actions[order[r]][t][c]
 *   mu <- alpha * mu + (1 - alpha) * m          sigma <- max(sigma_min, alpha * sigma + (1 - alpha) * s)   (a NaN stays a NaN)
 * then the new candidates: row 0 = clamp(mu, +-a_max) (the incumbent is always a candidate), row b > 0 = clamp(mu + sigma * noise[b],
 * +-a_max); a_max <= 0: no clamp.  alpha = 1 is an identity refit (of finite elites); K = 0 skips the refit altogether (order may be
 * NULL).  Two launches on the stream, refit then sample: every elite row is read before any row is overwritten.  0 <= alpha <= 1,
 * sigma_min >= 0, B * T < 2^29. */
int csplat_plan_integrate(void *stream, int B, int N, int H, int T, int k, float *v, const float *actions, int64_t grasped, float *pos,
                          float *hist, float *preds /* or NULL */, const float *goal /* or NULL: no cost */, const float *node_w /* or NULL */,
                          const float *step_w /* or NULL */, float *cost /* NULL only without a goal */);
int csplat_plan_cost(void *stream, int B, int N, const float *pos, const float *goal, const float *node_w /* or NULL */, float w,
                     int accumulate, float *cost);
int csplat_plan_select(void *stream, int B, int K, const float *cost, int32_t *order, float *best);
int csplat_plan_refit_sample(void *stream, int B, int T, int K, float *actions, const int32_t *order, float *mu, float *sigma,
                             const float *noise, float alpha, float sigma_min, float a_max);

/* Observation clouds, the sensing end of the pipeline (csplat_observation.hip): what turns depth images, silhouettes and cameras into the
 * 3-D data the Chamfer term (camera.points), the cloth-graph builders and the planner's node weights read.  They restate the reference's
 * host code: get_world_coords (manipulation/envs/camera_utils.py:106-133, manipulation/deform_mesh.py:168-195) and
 * get_observable_particle_index / _old (camera_utils.py:136-162, a full cdist matrix).  No gradients.  NO atomics of any kind: every
 * output is bit-reproducible run to run.  Float arithmetic without contraction, every operation one float32 rounding; the library is built
 * without fast-math, so `/` is the correctly rounded IEEE division and the cell below can be restated exactly in numpy float32.  Every
 * entry validates its arguments before any launch (a bad one returns non-zero and csplat_last_error() names the entry): NULL operands,
 * an output or `temp` that shares a byte with another operand, sizes out of range, operands that are not 4-byte aligned (temp: 16).
 *
 * csplat_obs_unproject: V views (1 <= V <= 65535) of H x W, V * H * W < 2^31; depth [V][H][W]; mask [V][H][W] or NULL (all ones);
 * intrinsics [V][4] = (fx, fy, cx, cy) in pixel units, pixel centres at the integers; cam_to_world [V][3][4] row-major, column-vector
 * form (p_world = R p_cam + t, t the fourth column).  Pixel (v, y, x) is SELECTED when x % stride == 0 and y % stride == 0 (stride >= 1),
 * its depth d is finite and > 0 (a hole is 0, negative, NaN or Inf: the rule of csplat_geom_loss_fwd), d <= max_depth when max_depth > 0
 * (<= 0: no maximum), and mask > 0.5 when a mask is given (a NaN mask value selects nothing).  Its point, with a = x - cx, b = y - cy:
 *   kind 0 (d is the view-space z)             p_cam = (a * d / fx, b * d / fy, d)
 *   kind 1 (d is the distance along the ray)   u = a / fx, w = b / fy, s = d / sqrt(u u + w w + 1), p_cam = (u s, w s, s)
 *   p_world[r] = R[r][0] p_cam.x + R[r][1] p_cam.y + R[r][2] p_cam.z + t[r], summed left to right
 * Selected pixels land in ascending order of their flat index (v H + y) W + x: points [cap][3], source [cap] (int32, that flat index),
 * *count_dev (device int32) = the number of selected pixels -- the FULL count, also when it exceeds cap; rows beyond cap are not written.
 * A stable compaction: selection bytes, csplat_mask_to_map, then a second pass that computes a selected pixel's point into its row.  Both
 * passes read a view's pixels row-wise, 16 bytes a lane where the view's plane allows it and scalar before and behind (odd H * W); the
 * view's 4 + 12 camera floats are uniform per workgroup.  temp: csplat_obs_unproject_temp_bytes(V, H, W) bytes of device memory, no initial state.
 * Errors besides the common ones: stride < 1, kind not 0 or 1, a NaN max_depth, cap < 0 or >= 2^31, NULL points / source with cap > 0.
 *
 * csplat_obs_voxel: M points [M][3] (0 <= M < 2^31) on a grid of cubic cells of edge voxel (finite, > 0) from `origin` (DEVICE float [3];
 * NULL: the per-axis minimum over the finite points, found on the device).  A point with a non-finite coordinate is left out:
 * inverse = -1.  Per axis the cell is c = floorf((p - o) / voxel), the subtraction and the division each rounded to float32 (no reciprocal,
 * no fused form).  Cells lie in [0, 2^21) per axis; a finite point outside (or a non-finite origin) is counted in *n_outside (device int32)
 * and gets inverse = -1.  Voxels are the occupied cells in ascending order of the key cz << 42 | cy << 21 | cx:
 *   centroid[q] = corner + (sum of (p - corner) over the voxel's points) / count[q],  corner = o + (float)c * voxel per axis;
 *                 the points of a voxel are taken in ascending index: lane l of one wave sums the l-th, (l + 64)-th, .. in that order
 *                 and a xor tree joins the 64 lanes -- an order fixed by the voxel's own points
 *   count[q] (int32), inverse[i] (int32) = the voxel of point i, *n_voxels (device int32) = K
 * centroid and count have M rows of capacity (K <= M is not known to the host); rows from K on are not written.  Built on
 * csplat_sort_pairs_u64 (stable, the point index as value), a head-flag csplat_scan_u32 and a segment reduction.  M == 0 zeroes the two
 * counters and returns.  temp: csplat_obs_voxel_temp_bytes(M) bytes of device memory, no initial state.
 *
 * csplat_obs_mark: idx [Q][K] (int32), d2 [Q][K] as csplat_knn_query returns them (K >= 1, Q * K < 2^31): flags[n] = 1 (uint8, N of them)
 * iff some entry has idx == n and (max_sq_dist < 0 or d2 <= max_sq_dist), else 0.  The entry zeroes flags on the stream, then every
 * writer stores the same byte: plain stores, no atomics.  Entries with idx outside [0, N) (the -1 of an unfilled slot) mark nothing.
 * A NaN max_sq_dist is an error.  Added exports: CSPLAT_ABI_VERSION is unchanged. */
size_t csplat_obs_unproject_temp_bytes(int V, int H, int W);
int csplat_obs_unproject(void *stream, int V, int H, int W, const float *depth, const float *mask /* or NULL */, const float *intrinsics,
                         const float *cam_to_world, int stride, float max_depth, int kind, int64_t cap, float *points, int32_t *source,
                         int32_t *count_dev, void *temp);
size_t csplat_obs_voxel_temp_bytes(int64_t M);
int csplat_obs_voxel(void *stream, int64_t M, const float *points, float voxel, const float *origin /* device, or NULL */, float *centroid,
                     int32_t *count, int32_t *inverse, int32_t *n_voxels, int32_t *n_outside, void *temp);
int csplat_obs_mark(void *stream, int64_t Q, int K, int N, const int32_t *idx, const float *d2, float max_sq_dist, uint8_t *flags);

/* Mesh z-buffer, the arrow mesh -> image (csplat_zbuffer.hip): what a depth camera would see of a triangle mesh -- depth, silhouette and
 * face-id images of V views -- and of a point cloud as one-pixel primitives.  The reference answers this on the host: Blender renders
 * (manipulation/fold_rendering/), the Python double loop build_depth_from_pointcloud (manipulation/envs/camera_utils.py:7-41) and the guess
 * of get_observable_particle_index.  An observation: no gradients.  Every output is a pure function of the inputs: coverage is exact integer
 * arithmetic, the only atomic is a 64-bit unsigned integer minimum (independent of the order of arrival), NO float atomics: every output
 * is bit-reproducible run to run.  Float arithmetic without contraction, every operation one float32 rounding, `/` and sqrt correctly rounded.
 * Every entry validates its arguments before any launch (a bad one returns non-zero and csplat_last_error() names the entry): sizes out of
 * range, NULL operands, operands that are not 4-byte aligned (screen and temp: 16), an output or `temp` that shares a byte with another
 * operand.  Sizes: 0 <= V <= 65535, H, W >= 0, V * H * W < 2^31, 0 <= N, M, F < 2^31, V * N < 2^31; V * H * W == 0 writes nothing and F == 0
 * gives images that are all holes.  NO CLIPPING: a face with a corner behind `near` is dropped whole (the cloth is in front of the camera).
 *
 * Cameras as csplat_obs_unproject takes them, mirrored: intrinsics [V][4] = (fx, fy, cx, cy) in pixel units, pixel centres at the
 * integers; world_to_cam [V][3][4] row-major, column-vector form (p_cam = R p_world + t, t the fourth column).  vertices [N][3]
 * (per_view 0: one mesh for all views) or [V][N][3] (per_view 1); faces [F][3] int32.  near finite and >= 0.
 *   Stage P, per (view, vertex): p_cam[r] = R[r][0] X + R[r][1] Y + R[r][2] Z + t[r], summed left to right;  px = (fx * x) / z + cx,
 *   py = (fy * y) / z + cy, iz = 1 / z.  The vertex is VALID when x, y, z, px, py and iz are finite, z > near, |px| <= 16384 and
 *   |py| <= 16384.  Snapped coordinates sx = rint(256 px), sy = rint(256 py) as int32, round-half-even.  screen [V][N][4] int32 =
 *   (sx, sy, float bits of iz, valid); all four are 0 for an invalid vertex.
 *   Stage D, per (view, face), in exact int64 arithmetic on the snapped corners 0, 1, 2: A = (x1 - x0)(y2 - y0) - (y1 - y0)(x2 - x0).
 *   A face with an invalid corner, a corner index outside [0, N) or A == 0 is dropped.  A < 0: corners 1 and 2 change places (the cloth is
 *   two-sided).  For pixel (X, Y), P = (256 X, 256 Y), and for each directed edge a -> b of 0 -> 1, 1 -> 2, 2 -> 0 with dx = xb - xa,
 *   dy = yb - ya:  E = dx (Py - ya) - dy (Px - xa).  The pixel is COVERED iff for all three edges E > 0, or E == 0 and (dy < 0, or
 *   dy == 0 and dx > 0): the top-left rule, every pixel of a watertight mesh has one owner per layer.  E12, E20, E01 are the weights of
 *   the (exchanged) corners 0, 1, 2 and sum to A.
 *   Depth: b_i = (float)E_i / (float)A for the face's OWN corners i = 0, 1, 2 (the exchange undone), q = b0 iz0 + b1 iz1 + b2 iz2 summed
 *   left to right, z = 1 / q: interpolating 1 / z is perspective-correct.  The nearest face wins; on equal float32 z the lower face index:
 *   the per-pixel state is one uint64 key (float bits of z) << 32 | face, all-ones = background, initialised by the call itself on every
 *   call, and the draw is atomicMin on it.
 *   Outputs per view: depth [V][H][W] = z (kind 0) or z * sqrt(u u + w w + 1), u = (X - cx) / fx, w = (Y - cy) / fy (kind 1: the
 *   distance along the pixel's ray, the inverse of csplat_obs_unproject's kind 1), 0 where no face covers the pixel (the hole convention
 *   of csplat_obs_unproject); silhouette [V][H][W] 0 or 1; face_id [V][H][W] int32, -1 on the background; bary [V][3][H][W] or NULL: the
 *   perspective-correct weights (b_i iz_i) / q in the face's corner order, 0 on the background; screen or NULL (then it lives in temp).
 * Launches: k_zb_project, k_zb_clear (16-byte stores), k_zb_draw -- one workgroup of four waves per (view, face), the waves stride over
 * the 8 x 8-pixel blocks of the bounding box clipped to the image, 64 lanes = one block, a block wholly outside one edge is skipped -- and
 * k_zb_resolve per pixel, which reads the key's z and recomputes the winner's weights with the same operations; plain stores.
 * temp: temp_bytes >= align256(8 V H W) + align256(16 V n) bytes of device memory (n = N or M, align256 rounds up to a multiple of 256;
 * csplat.zbuffer.temp_bytes computes it -- the library exports no size query and refuses a smaller temp_bytes), no initial state.
 *
 * csplat_zb_points: points [M][3] or [V][M][3] as one-pixel primitives (build_depth_from_pointcloud): the same stage P and validity; the
 * pixel is (rint(px), rint(py)), round-half-even, and a point outside the image is dropped; the same key with z = p_cam.z and the point
 * index in the low word, so the nearest point wins and a tie goes to the lower index; the same resolve writes depth [V][H][W] and
 * point_id [V][H][W] (int32, -1: none).
 *
 * csplat_zb_mark: face_id [V][H][W], faces [F][3] -> face_visible [V][F] and node_visible [V][N] (uint8): 1 iff some pixel of the view
 * holds the face, respectively a face with that corner, else 0.  The entry zeroes the flags on the stream, then every writer stores the
 * same byte: plain stores.  Ids outside [0, F) (the -1 of the background) and corners outside [0, N) mark nothing; V * F < 2^31.
 * Added exports: CSPLAT_ABI_VERSION is unchanged. */
int csplat_zb_mesh(void *stream, int V, int64_t N, int64_t F, int H, int W, const float *vertices, int per_view, const int32_t *faces,
                   const float *intrinsics, const float *world_to_cam, float near, int kind, float *depth, float *silhouette, int32_t *face_id,
                   float *bary /* or NULL */, int32_t *screen /* or NULL */, void *temp, size_t temp_bytes);
int csplat_zb_points(void *stream, int V, int64_t M, int H, int W, const float *points, int per_view, const float *intrinsics,
                     const float *world_to_cam, float near, int kind, float *depth, int32_t *point_id, void *temp, size_t temp_bytes);
int csplat_zb_mark(void *stream, int V, int64_t N, int64_t F, int H, int W, const int32_t *face_id, const int32_t *faces, uint8_t *face_visible,
                   uint8_t *node_visible);

/* Trajectory preprocessing, the step between the sensing end and the planner (csplat_traj_smooth in csplat_knn.hip, csplat_traj_features in
 * csplat_trajectory.hip): what turns a tracked cloud [T][N][3] into the smoothed positions, velocities and per-frame edge features the GNN and
 * the planner read.  They restate the reference's host code: gaussian_smoothing (meshnet/data_utils.py:267-278, one KD-tree query per point
 * per frame), the loop of process_traj (:307-348) and compute_edge_features (:443-448).  No gradients.  No atomics: every output element is
 * written by one thread in a fixed order of operations, so every output is bit-reproducible run to run.  Float arithmetic without
 * contraction, every operation one float32 rounding.  Every entry validates its arguments before any launch (a bad one returns non-zero
 * and csplat_last_error() names the entry): sizes out of range, NULL operands, operands that are not 4-byte aligned (edge_index: 8), an
 * output that shares a byte with another operand.
 *
 * csplat_traj_smooth: points [T][N][3], 1 <= K <= CSPLAT_KNN_MAX_K, sigma finite and > 0, T * N * K < 2^31.  For every frame t and point i:
 * the K nearest points of frame t to point i -- the point itself included, at distance 0 -- ordered exactly as csplat_knn_query orders them:
 * ascending in (d2, index), d2 = dx*dx + dy*dy + dz*dz with d = candidate - point, FP contraction off, ties to the smaller index.  No
 * other frame is ever read.  A candidate whose d2 is not finite (a NaN or Inf coordinate, an overflow) is nobody's neighbour; with fewer
 * than K neighbours (N < K among them) the remaining slots are (+inf, -1) as in csplat_knn_query and contribute nothing.  Weights:
 *   c = 1 / (2 sigma^2), evaluated in double from the float32 sigma, rounded once to float32 and limited to FLT_MAX;
 *   w_j = expf(-(d2_j * c)), the product rounded once to float32 (so w = 1 at d2 = 0 for every sigma; expf is the device library's);
 *   out_i = (sum_j w_j p_j) / (sum_j w_j), per axis: each product w_j p_j rounded, added in the list's ascending order beginning with its
 *   first term, one IEEE division at the end.  K = 1 returns the input bits.
 * sum_j w_j >= 1 always (a point at distance 0 is in the list), so no division is by zero.  A point with a non-finite coordinate has an
 * empty list and is written through unchanged.  out [T][N][3]; out_d2 [T][N][K] and out_idx [T][N][K] (int32) are optional (NULL: not
 * wanted), each on its own.  T = 0 or N = 0 is a no-op without a launch.  One launch: the brute-force search of csplat_knn_query with the
 * frame on the grid's second axis (frames beyond the axis limit are looped over) and the weighted mean formed from the K-best registers, K
 * gathers from the frame.  Only the brute-force form exists, O(T N^2): tracked clouds are hundreds to a few thousand points.
 *
 * csplat_traj_features: pos [T][N][3], edge_index [2][E] (int64, entries in 0 .. N-1), T * N < 2^31, T * E < 2^31, inv_dt finite; ONE launch for
 * all frames:
 *   vel[0][i] = 0;  vel[t][i] = (pos[t][i] - pos[t-1][i]) * inv_dt, the difference and the product each rounded once
 *   disp[t][e] = pos[t][edge_index[1][e]] - pos[t][edge_index[0][e]]  (receiver minus sender: the sign of the reference's
 *                compute_edge_features, the OPPOSITE of csplat_gnn_edge_features / rollout.edge_features)
 *   norm[t][e] = sqrtf(dx*dx + dy*dy + dz*dz), contraction off
 * vel [T][N][3] is optional (NULL: not wanted); disp [T][E][3] and norm [T][E] are wanted together or not at all.  An edge_index entry
 * outside 0 .. N-1 gives a NaN row and reads nothing (the Python surface checks the range).  T = 0 or N = 0 is a no-op without a launch, and
 * so is a call that has nothing to write (E = 0 without vel); E = 0 with vel writes the velocities alone.
 * Added exports: CSPLAT_ABI_VERSION is unchanged. */
int csplat_traj_smooth(void *stream, int T, int N, int K, const float *points, float sigma, float *out, float *out_d2 /* or NULL */,
                       int32_t *out_idx /* or NULL */);
int csplat_traj_features(void *stream, int T, int N, int64_t E, const float *pos, const int64_t *edge_index, float inv_dt, float *vel /* or NULL */,
                         float *disp, float *norm);

/* Delaunay triangulation of a planar cloud, the mesh between the sampled nodes and the network's edges (csplat_delaunay.hip, predicates in
 * csplat_delaunay_predicates.h).  It restates what the reference does on the host: scipy.spatial.Delaunay followed by the loop over simplices
 * with the length filter (meshnet/data_utils.py:371-405, compute_edges_index with delaunay=True, the default of every MeshNet script), and
 * compute_mesh (:419-440), from which scene_reconstruction/gaussian_mesh.py:52,204 builds the Gaussians' mesh.  No gradients.
 *
 * points [N][2] float32 (the projected coordinates), 0 <= N < 2^24.  A point with a non-finite coordinate is skipped; so is a point whose
 * two coordinates equal those of a lower-indexed point (-0.0 == 0.0).  Skipped points are in no face and are counted.  Among the rest the
 * output is the triangulation of their convex hull in which no point is strictly inside a face's circumcircle.  Ties are broken by raising
 * the lifted height x^2 + y^2 of point p by a symbolic eps_p, eps_0 >> eps_1 >> ... > 0: when the exact in-circle determinant of (a, b, c, d)
 * is zero, its sign is that of the first non-zero cofactor, taken in ascending point index over the four; the cofactors are +orient(b,c,d),
 * -orient(a,c,d), +orient(a,b,d), -orient(a,b,c) for a, b, c, d.  Orientation is not perturbed: a collinear triple is never a face.  The
 * result is therefore a pure function of the coordinates and the index order, unique also on a regular grid where every quad is
 * cocircular (this rule replaces Qhull's joggle and its arbitrary choice among cocircular points).  All points collinear, or fewer than
 * three usable: zero faces, no error.
 *
 * Brute force, one wave per point i and no dependence between points: from the exact nearest other point j0 (ties to the lower index; that
 * edge is in every Delaunay triangulation) the walk takes, among the points strictly left of i -> j, the one that no other beats under the
 * perturbed in-circle test, emits the face and goes on with the edge (i, k), until it closes on j0 or nothing is left of the edge (the
 * hull); then it walks the other way from j0.  Each face is found by its three vertices; only the walk of its lowest index writes it.
 * The walk counts what each point owns and keeps the first sixteen faces and edges per point; one scan lays the output out; only points
 * that own more walk a second time to write; one ordering pass.  O(N^2) per walk, made for hundreds to a few thousand points.  Every
 * decision of the walk -- nearest neighbour, orientation, in-circle -- is an exact predicate on the float32 inputs over the whole finite
 * float32 range, denormals and 60-binade exponent gaps included: an fp64 evaluation with a forward error bound as filter, then an exact
 * stage in fp64 expansion arithmetic (two-sum; two-product by explicit fma; nothing else contracts).  No float atomics: every output is
 * bit-reproducible.
 *
 * The length filter of the reference's loop is part of the entry: len = sqrtf(du*du + dv*dv) in float32 without contraction; an edge of a
 * simplex is dropped when len > (float)norm_threshold; a face is kept when none of its three edges is dropped; kept edges come back once
 * each.  has_threshold = 0 keeps everything (norm_threshold is not read); a NaN threshold is an error.
 *
 * Outputs on the device: faces [2N][3] int32, the first counters[0] rows written: each face rotated so that its lowest index is first,
 * counter-clockwise in the input plane, the rows in lexicographic order.  edges [3N][2] int32, the first counters[1] rows written: i < j,
 * sorted by (i, j).  counters [5] int64: kept faces, kept edges, skipped points, exact decisions (how many decisions of the counting walk
 * the exact stage took: per-point partials summed in a fixed order), status.  status bit 0: a walk exceeded N steps; bit 1: the two walks
 * disagreed or an output would leave its capacity (nothing is written outside).  A non-zero status means the outputs are not to be used.
 * temp: what csplat_delaunay_temp_bytes reports, 256-byte aligned, no initial state.  csplat_delaunay_temp_bytes returns 0 and stores the
 * size, or refuses N like the entry does.  N = 0 zeroes the counters without a launch.
 *
 * Refused before any launch, with return 2 and csplat_last_error() naming the entry: N outside 0 .. 2^24 - 1, has_threshold other than 0 or
 * 1, a NaN threshold, NULL operands, points not 8-byte aligned, faces / edges not 4-byte aligned, counters not 8-byte aligned, temp not
 * 256-byte aligned, an output or temp that shares a byte with another operand.
 * Added exports: CSPLAT_ABI_VERSION is unchanged. */
int csplat_delaunay_temp_bytes(int N, size_t *bytes);
int csplat_delaunay(void *stream, int N, const float *points, int has_threshold, double norm_threshold, int32_t *faces, int32_t *edges,
                    int64_t *counters, void *temp);

/* MeshNet training transition (csplat_train_sim.hip): the state update between the predictions of one unrolled training step, the
 * reference's update_prediction (train_meshnet_sim.py:322-359), forward and backward, one launch each.  H = input_sequence_length, c a
 * component 0..2; every operation is float32 and rounded once, no contraction:
 *   pa[n][c]      = pred_acc[n][c] * ostd[c] + omean[c]   (Normalizer.inverse folded in: one multiply, one add, each rounded; pred_acc[n][c]
 *                   itself when omean / ostd are NULL -- they are given together or not at all)
 *   vn[n]         = velocity[n] + velocity_noise[n]       (velocity[n] itself when the noise is NULL)
 *   nv[n][c]      = old_actions[n][c] != 0 ? old_actions[n][c] : vn[n][3(H-1)+c] + pa[n][c]
 *   new_pos[n][c] = (actions[n][c] == 0 ? init_position[n][c] + nv[n][c] : init_position[n][c]) + actions[n][c]
 *   hist[n][0 : 3(H-1)] = vn[n][3 : 3H]                    (a shift; H = 1 shifts nothing)
 *   hist[n][3(H-1)+c]   = actions[n][c] != 0 ? actions[n][c] : vn[n][3(H-1)+c]
 *   edge_feat[e]  = (d, |d|), d = new_pos[row] - new_pos[col], row / col = edge_index[0 / 1][e]: bit-equal to csplat_gnn_edge_features on
 *                   new_pos (|d| = sqrtf(fma(dz, dz, fma(dx, dx, dy * dy))), the form that kernel's object code has)
 * The quirks are the reference's: the masks are per component (a grasped node whose action has one component exactly 0 integrates the
 * predicted velocity in that component), and the last history slot receives the OLD last velocity with the next action's non-zero
 * components written over it, not nv.  velocity, velocity_noise, hist [N][3H]; pred_acc, init_position, old_actions, actions, new_pos [N][3];
 * omean, ostd [3]; edge_index [2][E] int64 with entries in 0 .. N-1 (an entry outside gives a NaN row and reads nothing; the Python surface
 * checks the range); edge_feat [E][4], 16-byte aligned.  Each of hist, edge_feat, new_pos may be NULL: not wanted.  Edge threads recompute
 * their two endpoint positions from the node inputs with the same rounded operations, so the forward is ONE launch.
 *
 * csplat_train_update_bwd, ONE launch, one thread per node, gathers
 *   gp[n] = g_new_pos[n] + sum_{e: row = n} (g_d[e] + g_len[e] d[e] / |d[e]|) - sum_{e: col = n} (the same)
 * with (d[e], |d[e]|) = edge_feat[e] as the forward left it and (g_d[e], g_len[e]) = g_edge_feat[e]; the length term is 0 for a zero-length
 * edge, as with torch.norm.  The sums run over the CSR by source, then the CSR by destination (csplat_gnn_build_csr's rowptr [N+1] / perm [E],
 * ascending edge id inside a row), in that fixed order.  g_init_position = gp;
 * g_pred_acc[n][c] = (actions[n][c] == 0 && old_actions[n][c] == 0) ? gp[n][c] (times ostd[c] when folded) : 0.  Nothing flows to velocity,
 * the noise or the actions, and hist carries no gradient.  g_edge_feat or g_new_pos may be NULL (no such gradient arrived), and so may
 * either output.  No atomics: two runs give equal bits.
 *
 * Both entries refuse, before any launch, with return 2 and csplat_last_error() naming the entry: negative sizes, H outside 1 .. 16, NULL
 * or misaligned operands, omean without ostd, an output that shares a byte with an input or with another output, N * 3H or 4E beyond 2^31.
 * N = 0 or nothing wanted is a no-op that returns 0.
 * Added exports: CSPLAT_ABI_VERSION is unchanged. */
int csplat_train_update_fwd(void *stream, int N, int64_t E, int H, const float *velocity, const float *velocity_noise /* or NULL */,
                            const float *pred_acc, const float *omean /* or NULL */, const float *ostd /* or NULL */, const float *init_position,
                            const float *old_actions, const float *actions, const int64_t *edge_index, float *hist /* or NULL */,
                            float *edge_feat /* or NULL */, float *new_pos /* or NULL */);
int csplat_train_update_bwd(void *stream, int N, int64_t E, const float *edge_feat, const float *g_edge_feat /* or NULL */,
                            const float *g_new_pos /* or NULL */, const float *old_actions, const float *actions, const float *ostd /* or NULL */,
                            const int32_t *src_rowptr, const int32_t *src_perm, const int32_t *dst_rowptr, const int32_t *dst_perm,
                            float *g_pred_acc /* or NULL */, float *g_init_position /* or NULL */);

/* MeshNet sample data set (csplat_dataset.hip): the samples of the reference's SamplesClothSimDataset (meshnet/dataloader_sim.py: __getitem__
 * :148-182, _data_to_graph :352-412, followed by FaceToEdge / Cartesian / Distance and PyG's collate) assembled on the device, a whole
 * block-diagonal batch in ONE launch, and the arithmetic of its validate (train_meshnet_sim.py:303-308) in one launch.
 *
 * The store: all trajectories packed back to back in device buffers.  Trajectory j has T_j frames of N_j nodes and E_j edges:
 *   pos, velocity [sum T_j N_j][3], node_type [sum T_j N_j]  frame-major inside a trajectory: node i of frame t is row NODE_BASE + t N_j + i
 *   actions [sum T_j][3]                                     frame t is row FRAME_BASE + t
 *   edges (int64)                                            trajectory j's [2][E_j] block begins at word 2 * EDGE_BASE: stored once, not
 *                                                            per frame; entries in 0 .. N_j - 1
 *   table (int64) [n_traj][CSPLAT_DATASET_TABLE_WORDS]       NODE_BASE (node rows in front), FRAME_BASE (frames in front), EDGE_BASE (edges
 *                                                            in front), N, E, T, GRASPED (the grasped node g_j; outside 0 .. N-1: none)
 * store_rows, store_frames, store_edges are the three sums (what the buffers hold).
 *
 * desc (int32) [B][4] = (trajectory j, time index t, first output node row r, first output edge row e0) of every sample, 16-byte aligned;
 * action_override [B][F][3] or NULL.  n_rows / n_edges are the batch's totals (sum N_j / sum E_j over the samples), max_items the largest
 * N_j (3H + 4 + 9F) + E_j of a sample (it sizes the grid; a larger sample is still written whole).  H = input sequence length, F = future
 * sequence length, a[f] = action_override[b][f] when given, else actions_j[t - 1 + f].  Sample b writes, bit for bit (i a node, g = g_j):
 *   out_velocity[r + i][3h : 3h + 3]   = vel_j[t - H + h][i], h = 0 .. H-1 (oldest first); the grasped row's last three columns are
 *                                        vel_j[t][g] (_data_to_graph:363-365: the grasped node already carries its target velocity)
 *   out_node_types[r + i]              = node_type_j[t - 1][i]
 *   out_positions[r + i]               = pos_j[t - 1][i]; the grasped row is pos_j[t - 1][g] + a[0], one float32 add per component
 *   out_target_velocities[r + i][f]    = vel_j[t + f][i],  out_pos_target[r + i][f] = pos_j[t + f][i],  f = 0 .. F-1
 *   out_particle_actions[r + i][f]     = 0; the grasped row is a[f]
 *   out_edge_index[0 / 1][e0 + e]      = edges_j[0 / 1][e] + r          (out_edge_index is [2][n_edges])
 *   out_edge_features[e0 + e]          = (d, |d|), d = p[row] - p[col] on the OUTPUT positions p (the moved grasped node included), bit-equal
 *                                        to csplat_gnn_edge_features on out_positions (|d| = sqrtf(fma(dz, dz, fma(dx, dx, dy * dy))), the
 *                                        form that kernel's object code has); [n_edges][4], 16-byte aligned
 * Float arithmetic without contraction.  Plain loads and stores, every output element written by exactly one thread, no atomics: two runs
 * give equal bits.  An edges entry outside 0 .. N_j - 1 gives that edge a NaN feature row and reads nothing out of range.  A window that
 * leaves its trajectory (t < H or t + F > T_j) is the caller's error -- the Python surface refuses it; here every float of that sample is
 * NaN and nothing is read.  A sample whose rows would leave the outputs (r + N_j > n_rows, e0 + E_j > n_edges), whose j is not a
 * trajectory or whose trajectory leaves the store is skipped: nothing outside the operands is ever touched.
 *
 * csplat_dataset_rollout_error: pos0 [N][3], pred [S][N][3] (the predicted displacement of every step), gt [S][N][3] (the true positions of
 * steps 1 .. S) -> err [S]:
 *   at_s[i] = ((pos0[i] + pred[0][i]) + pred[1][i]) + ... + pred[s][i]   added in this order, each sum rounded
 *   err[s]  = (sum_i (at_s[i] - gt[s][i])^2) / (float)(3 N)              i over the 3 N components
 * The sum has a fixed order: thread q of 256 adds its components q, q + 256, ... in ascending order beginning from 0, then the 256 partial
 * sums are joined by a halving tree (slot q += slot q + 128, then + 64, ... + 1).  One workgroup per step, no atomics: two runs give
 * equal bits.  S = 0 is a no-op; N = 0 with S > 0 is refused.  S * N * 3 < 2^31.
 *
 * Both entries refuse, before any launch, with return 2 and csplat_last_error() naming the entry: negative sizes, H outside 1 .. 16,
 * F < 1, NULL or misaligned operands, an output that shares a byte with another operand, row counts beyond 2^31 (n_rows * 3H, n_rows * 3F,
 * 4 * n_edges, the store's sums).  B = 0 or an empty batch is a no-op that returns 0.
 * Added exports: CSPLAT_ABI_VERSION is unchanged. */
#define CSPLAT_DATASET_TABLE_WORDS 8
enum { CSPLAT_DATASET_NODE_BASE = 0, CSPLAT_DATASET_FRAME_BASE, CSPLAT_DATASET_EDGE_BASE, CSPLAT_DATASET_N, CSPLAT_DATASET_E, CSPLAT_DATASET_T,
       CSPLAT_DATASET_GRASPED };
int csplat_dataset_batch(void *stream, int B, int H, int F, int n_traj, int64_t store_rows, int64_t store_frames, int64_t store_edges,
                         const float *pos, const float *velocity, const float *node_type, const float *actions, const int64_t *edges,
                         const int64_t *table, const int32_t *desc, const float *action_override /* or NULL */, int64_t n_rows, int64_t n_edges,
                         int64_t max_items, float *out_velocity, float *out_node_types, float *out_positions, float *out_target_velocities,
                         float *out_pos_target, float *out_particle_actions, int64_t *out_edge_index, float *out_edge_features);
int csplat_dataset_rollout_error(void *stream, int S, int N, const float *pos0, const float *pred, const float *gt, float *err);

/* Camera data set (csplat_camera_dataset.hip): the ground-truth images and masks of a training step's cameras -- the reference's MDNerfDataset
 * (scene_reconstruction/dataset.py:46-123), whose items carry float images from the host -- gathered out of a device-resident store in ONE
 * launch.
 *
 * The store: one 16-byte aligned device buffer of n_slots slots.  A slot holds 3 image planes, then 1 mask plane when has_mask = 1; plane p
 * of slot s begins at byte (s * (3 + has_mask) + p) * pitch.  pitch is a multiple of 16 bytes and at least H * W elements long, so every
 * plane begins 16-byte aligned; the bytes behind the H * W elements of a plane are never read.  storage:
 *   CSPLAT_CAMERA_UINT8    an element is one byte, the 8-bit level u of an image or m of a mask (the loader's own quantisation,
 *                          csplat/scene_io.py: image = uint8 / 255.0, mask = 1.0 - uint8 / 255.0)
 *   CSPLAT_CAMERA_FLOAT32  an element is one float32 word
 * slots (int32, device) [n] names the slot of every camera of the step.  Camera i writes, bit for bit:
 *   gt[i][c][y][x]   = (float)u / 255.0f, one correctly rounded division (torch's uint8_tensor / 255.0; a multiply by the reciprocal
 *                      differs at 126 of the 256 levels)                                         | the stored word (float32 storage)
 *   mask[i][0][y][x] = 1.0f - (float)m / 255.0f, two roundings (torch's 1.0 - uint8_tensor / 255.0) | the stored word
 * gt is [n][3][H][W], mask [n][1][H][W] (NULL exactly when has_mask = 0).  float32 storage copies words: NaN payloads, -0.0 and denormals
 * arrive as stored.  Float arithmetic without contraction.  Plain loads and stores, every output element written by exactly one thread,
 * no atomics: two runs give equal bits.  A slots entry outside 0 .. n_slots - 1 is the caller's error -- the Python surface refuses it;
 * here every float of that camera is NaN and nothing is read.
 *
 * Refused before any launch, with return 2 and csplat_last_error() naming the entry: negative sizes, another storage or has_mask value, a
 * pitch that is not a multiple of 16 or shorter than a plane, H * W or n_slots beyond 2^31, NULL slots / gt / store (with n_slots > 0), a
 * mask output that does not go with has_mask, a store that is not 16-byte aligned or slots / gt / mask that are not 4-byte aligned, an
 * output that shares a byte with another operand.  n = 0 or H * W = 0 is a no-op that returns 0.
 * Added exports: CSPLAT_ABI_VERSION is unchanged. */
#define CSPLAT_CAMERA_UINT8 0
#define CSPLAT_CAMERA_FLOAT32 1
int csplat_camera_batch(void *stream, int n, int H, int W, int storage, int has_mask, int64_t n_slots, int64_t pitch, const void *store,
                        const int32_t *slots, float *gt, float *mask /* or NULL */);

/* Fused mesh -> Gaussian transform (SURVEY.md 8(f) "next" row N1): MultiGaussianMesh.get_xyz + get_rotation,
 * scene_reconstruction/gaussian_mesh.py:151-188.  face_vertex_ids[P][3] (int64, device) = mesh.face[:, face_ids].T.
 *   csplat_mesh_rest       per-Gaussian constants of the REST face (in-plane basis, normal, in-plane coordinates) into
 *                          `rest` (csplat_mesh_rest_bytes(P) bytes); recompute when the mesh / face assignment changes
 *   csplat_mesh_transform_fwd   out_xyz[P][3] = barycentric centre on the deformed vertices; out_quat[P][4] =
 *                          normalize(rotation) (x) quaternion(Kabsch(rest face -> deformed face)), roma XYZW convention
 *   csplat_mesh_transform_bwd   gradients w.r.t. vertices[V][3] (atomically scattered, zeroed here), bary[P][3], rotation[P][4] */
size_t csplat_mesh_rest_bytes(int P);
int csplat_mesh_rest(void *stream, int P, const int64_t *face_vertex_ids, const float *rest_vertices, void *rest);
int csplat_mesh_transform_fwd(void *stream, int P, const int64_t *face_vertex_ids, const float *vertices, const float *bary,
                              const float *rotation, const void *rest, float *out_xyz, float *out_quat);
int csplat_mesh_transform_bwd(void *stream, int P, int V, const int64_t *face_vertex_ids, const float *vertices,
                              const float *bary, const float *rotation, const void *rest, const float *g_xyz,
                              const float *g_quat, float *d_vertices, float *d_bary, float *d_rotation);
/* The same for the T cameras of a training step in one launch each way (the reference calls get_xyz / get_rotation once per
 * render(), train_utils.py:204-260): vertices [T][V][3] -> out_xyz [T][P][3], out_quat [T][P][4]; backward takes g_xyz
 * [T][P][3] / g_quat [T][P][4] (either may be NULL) and returns d_vertices [T][V][3] and d_bary / d_rotation summed over the
 * cameras in camera order.  Vertex gradients: with vertex_rowptr [V+1] / vertex_corners [3P] (int32; the (Gaussian, corner)
 * pairs incident to each vertex as 3 * gaussian + corner, grouped by vertex: a stable sort of face_vertex_ids) and
 * corner_scratch (T*P*9 floats, contents irrelevant) they are gathered in that fixed order -- deterministic, no atomics; with NULLs they are
 * scattered with float atomics. */
int csplat_mesh_transform_fwd_views(void *stream, int T, int P, int V, const int64_t *face_vertex_ids, const float *vertices,
                                    const float *bary, const float *rotation, const void *rest, float *out_xyz, float *out_quat);
int csplat_mesh_transform_bwd_views(void *stream, int T, int P, int V, const int64_t *face_vertex_ids, const float *vertices,
                                    const float *bary, const float *rotation, const void *rest, const float *g_xyz,
                                    const float *g_quat, float *d_vertices, float *d_bary, float *d_rotation,
                                    const int *vertex_rowptr, const int *vertex_corners, float *corner_scratch);

/* ---- in-library kernel timing (HIP events on the launch stream; used by bench.py's roofline leg) ------
 * mask bit k enables bracketing of kernel class k with a start/stop event pair on the stream it is launched on:
 *   0 K1 preprocess | 1 K2 scan | 2 K3 key emission | 3 K4 radix sort (all passes) | 4 K5 tile ranges
 *   5 K6 compositing fwd | 6 K7 compositing bwd | 7 K8 preprocess bwd | 8 distCUDA2 | 9 GNN kernels
 *   10 depth partials prepass | 11 K7 of the depth path | 12 K8 of the depth path (csplat_backward_depth, dL_ddepth)
 *   13 K8 of the camera path | 14 the camera path's background partials and fixed-order sums (csplat_view.dL_dview .. dL_dbg)
 *   15 the feature / alpha forward pass | 16 feature partials prepass | 17 K7 of the feature path | 18 feature gradient extraction
 *   (csplat_view.features .. dL_dfeat_in) | 19 the visibility walk and per-Gaussian reduce (csplat_visibility_views)
 *   20 csplat_geom_loss_fwd (both launches) | 21 csplat_geom_loss_bwd
 * csplat_prof_read synchronises the recorded events of class k, returns their summed duration (ms) and the
 * number of brackets, and recycles the events. */
int csplat_prof_enable(unsigned mask);
int csplat_prof_read(int kernel_class, double *ms_total, int64_t *launches);

/* ---- MeshNet message passing (meshnet/graph_network.py:151-222) ------------------------------------
 * Graph structure is passed as two CSR orderings of the E directed edges, built once per graph by
 * csplat_gnn_build_csr: for key in {dst = edge_index[1], src = edge_index[0]}:
 *   rowptr[N+1] (int32) and perm[E] (int32) listing edge ids grouped by key, ascending edge id inside a row
 *   (=> a fixed, reproducible summation order; no float atomics on this path).
 * Rows of L floats move as float4 (16 B per lane) when L % 4 == 0, as scalars otherwise: with such an L every float operand of
 * csplat_gnn_edge_combine_fwd / _bwd, csplat_gnn_segment_sum and csplat_gnn_gather_rows must be 16-byte aligned (refused otherwise,
 * before anything is launched). */
size_t csplat_gnn_csr_temp_bytes(int N, int64_t E); /* temp of csplat_gnn_build_csr: no initial state */
int csplat_gnn_build_csr(void *stream, int N, int64_t E, const int64_t *keys /* device, [E] */, int32_t *rowptr,
                         int32_t *perm, void *temp);

/* edge pre-activation of the first edge-MLP layer with the concat folded away:
 *   out[e][:] = relu?( xa[dst[e]][:] + xb[src[e]][:] + ec[e][:] )          (ec already holds e@W_e^T + b)
 * xa = x @ W_i^T, xb = x @ W_j^T are node-level products (N x L); may run in place (out == ec). */
int csplat_gnn_edge_combine_fwd(void *stream, int N, int64_t E, int L, const int64_t *edge_index /* [2][E] */,
                                const float *xa, const float *xb, const float *ec, int relu, float *out);
/* backward of the above w.r.t. xa, xb (gradient w.r.t. ec is g itself, masked by relu):
 *   g_masked = g * (out > 0) if relu;  dxa[n] = sum_{e: dst(e)=n} g_masked[e];  dxb[n] = sum_{e: src(e)=n} g_masked[e] */
int csplat_gnn_edge_combine_bwd(void *stream, int N, int64_t E, int L, const float *g, const float *out, int relu,
                                const int32_t *rowptr_dst, const int32_t *perm_dst, const int32_t *rowptr_src,
                                const int32_t *perm_src, float *g_masked, float *dxa, float *dxb);
/* aggr='add': agg[n][:] = sum_{e in row n} msg[perm[e]][:]   (deterministic segmented sum, compensated: the float64 sum to an ulp).
 * A row whose running sum leaves the finite range -- a message of +-Inf, an overflow, a NaN -- gives what the plain sequence of
 * float32 adds gives (index_add_): +-Inf stays +-Inf, Inf - Inf and NaN are NaN. */
int csplat_gnn_segment_sum(void *stream, int N, int64_t E, int L, const float *msg, const int32_t *rowptr,
                           const int32_t *perm, float *agg);
/* its backward: dmsg[e][:] = dagg[key[e]][:]   (row gather) */
int csplat_gnn_gather_rows(void *stream, int64_t E, int L, const float *rows, const int64_t *keys, float *out);
/* the same pass also leaves *absmax = max |value| over the gathered rows (L a multiple of 4; what csplat_gnn_edge_mlp3's mode 0 scales by) */
int csplat_gnn_gather_rows_absmax(void *stream, int64_t E, int L, const float *rows, const int64_t *keys, float *out, float *absmax);
/* Edge features of one rollout step (PyG Cartesian(norm=False) + Distance(norm=False), the `transformer(graph)` of
 * /root/reference/train_meshnet_sim.py:152 and dataloader_sim.py): out[e] = (pos[row] - pos[col], |pos[row] - pos[col]|) with
 * row = edge_index[0][e], col = edge_index[1][e]; pos [N][3], out [E][4] (16-byte aligned). */
int csplat_gnn_edge_features(void *stream, int64_t E, const float *pos, const int64_t *edge_index, float *out);
/* A chain of 128-wide Linears on node rows with pre-packed 16-bit-piece weights (the node update's machinery; round 6):
 *   mode 0: out_a = x Wa^T, out_b = x Wb^T           -- the first processor layer's x_i / x_j products (graph_network.py:178-199)
 *   mode 1: out_a = relu(W1 relu(W0 x + b0) + b1)    -- the decoder's two hidden layers (graph_network.py:295-332); out_b unused
 * x, out_* [N][128] fp32, 16-byte aligned, outputs not aliasing x; image = csplat_gnn_rows_chain_pack(mode, first, second) of
 * csplat_gnn_node_update_image_bytes() bytes, packed and used under one csplat_gnn_edge_mlp3_mode. */
int csplat_gnn_rows_chain_pack(void *stream, int mode, const float *Wfirst, const float *Wsecond, void *image);
int csplat_gnn_rows_chain(void *stream, int64_t N, int mode, const float *x, const void *image, const float *b0, const float *b1,
                          float *out_a, float *out_b);
/* csplat_gnn_edge_features for the edges in another order: row r of out = the features of edge order[r] (the rollout encodes its edges in the
 * destination order of GraphCSR.agg_plan: a permuted read of the [E] index pairs instead of a gather of [E][4] rows afterwards). */
int csplat_gnn_edge_features_ordered(void *stream, int64_t E, const float *pos, const int64_t *edge_index, const int64_t *order, float *out,
                                     float *absmax /* or NULL: receives max |value| (as csplat_absmax: atomicMax on the bits; zeroed by the caller) */);
/* Head and tail of ONE rollout step of ClothMeshSimulator around the network's launches (round 6: a recorded step holds library kernels only).
 *   head:      feats[n] = normalise(cat(hist[0][n], .., hist[H-1][n], one_hot(node_type[n], T)))   (/root/reference/meshnet/cloth_network.py:72-110;
 *              mean / std [3H + T] or both NULL = IdentityNormalizer); also *counter += 1 (the step's number + 1, device side)
 *   decode:    v[n] = last_v[n] + denormalise(W h[n] + b)   (the decoder's last Linear 128 -> D <= 4 and cloth_network.py:163-193); *fine = 0
 *              when a row is not finite (the fp16-piece arithmetic's overflow signal, meshnet/graph_network.py)
 *   integrate: v[grasped] = actions[*counter - 1]; preds[*counter - 1] = v; pos += v; hist <- (hist[1:], v)
 *              (/root/reference/train_meshnet_sim.py:176,256-262).  hist [H][N][D], pos / v [N][D], actions / preds [steps][..].
 * head: N >= 0 (the counter goes up at N = 0 too; counter may be NULL), 1 <= H <= 16, 0 <= T <= 16, a node type outside 0 .. T-1 has
 * an all-zero one-hot; the absmax word is only ever raised (atomicMax on the bits of max |stored feature|): zero it before a step.
 * decode: 1 <= D <= 4, h and W 16-byte aligned; *fine is only ever cleared, by a row of v that holds a NaN or an Inf; every other row is
 * unaffected.  integrate: H >= 1, *counter >= 1 (the head ran); a grasped index outside [0, N) pins NOTHING (callers that give -1
 * Python's meaning must resolve it first: meshnet.rollout takes its generic step for such an index). */
int csplat_rollout_head(void *stream, int N, int H, int T, const float *hist, const int32_t *node_type, const float *mean, const float *stdv,
                        float *feats, int32_t *counter, float *absmax /* or NULL: max |feature|, as csplat_absmax */);
int csplat_rollout_decode(void *stream, int N, int D, const float *h, const float *W, const float *b, const float *omean, const float *ostd,
                          const float *last_v, float *v, int32_t *fine);
int csplat_rollout_integrate(void *stream, int N, int H, int D, float *v, const float *actions, const int32_t *counter, int64_t grasped,
                             float *pos, float *hist, float *preds, float *absmax2 /* or NULL: two words set to zero for the next step's head / edge features */);
/* The `real_world` branch of the rollout (/root/reference/train_meshnet_sim.py:211-250: per rollout step, ten iterations of a fresh
 * torch.optim.Adam(lr = 1e-3) on the predicted velocities against sum_e w_e (|(pos + v)[row_e] - (pos + v)[col_e]| - rest_len_e)^2).
 * v [N][3] is updated in place; edge_w [E] or NULL (the reference zeroes ONE deviation: `length_deviation[grasped_particle] *= 0`);
 * the CSR orderings by destination (edge_index[1]) and by source (edge_index[0]) as csplat_gnn_build_csr leaves them; scratch = 9 N
 * floats, contents irrelevant.  iters = 0, and a node without edges at any iters, leave v as it is bit for bit.  One launch per iteration (gradient gathered per node over both orderings -- no atomics -- and the Adam step of the node's own
 * coordinates in the same pass), nothing read back. */
int csplat_gnn_edge_length_refine(void *stream, int N, int64_t E, const float *pos, float *v, const int64_t *edge_index, const float *rest_len,
                                  const float *edge_w, const int32_t *dst_rowptr, const int32_t *dst_perm, const int32_t *src_rowptr,
                                  const int32_t *src_perm, int iters, double lr, double beta1, double beta2, double eps, float *scratch);

/* The 128-wide Linear layers of the MeshNet MLPs for inference (replaces the cuBLAS sgemm behind nn.Linear at
 * /root/reference/meshnet/graph_network.py:198,221 when no autograd graph is recorded), with everything that follows the
 * product fused into the accumulators:
 *   out[m][:] = LN?( relu?( alpha * (A[m][:] @ W^T) + bias + gather_a[index_a[m]][:] + gather_b[index_b[m]][:]
 *                           + add_pre[m][:] ) ) + add_post[m][:]
 * A [M][128], W [128][128] row-major (torch Linear.weight), bias [128] or NULL, gather_* [*][128] with int64 row indices
 * (both or neither), ln_gamma / ln_beta [128] (both or neither; biased variance, ln_eps), add_pre / add_post [M][128] or
 * NULL (not together with the gathers), out [M][128]; out may alias A (and add_post may then alias both).
 * fp32 throughout (v_mfma_f32_32x32x2_f32: exact fp32 products, fp32 accumulate). A, W and out 16-byte aligned. */
/* The node update of one InteractionNetwork layer (/root/reference/meshnet/graph_network.py:203-222, two hidden layers of
 * width 128) in one launch, optionally followed by the next layer's node-level products:
 *   h = relu(agg @ Wa^T + x @ Wx^T + b0);  h = relu(h @ W2^T + b2);  x_new = LayerNorm(h @ W3^T + b3) + x;
 *   xa_next = x_new @ Wi_next^T;  xb_next = x_new @ Wj_next^T          (Wi_next, Wj_next both NULL: skipped)
 * agg, x, x_new, xa_next, xb_next [N][128]; all weights [128][128] row-major, contiguous (Wa / Wx are the two column
 * blocks of the first Linear's weight, cut by the caller); exact fp32 MFMA.  x_new must not alias agg or x. */
int csplat_gnn_node_update(void *stream, int64_t N, const float *agg, const float *x, const float *Wa, const float *Wx,
                           const float *b0, const float *W2, const float *b2, const float *W3, const float *b3,
                           const float *ln_gamma, const float *ln_beta, float ln_eps, const float *Wi_next,
                           const float *Wj_next, float *x_new, float *xa_next, float *xb_next);

/* The same node update on 16-bit pieces -- by csplat_gnn_edge_mlp3_mode: 0 (default) two fp16 pieces per operand, three products, everything run
 * at a fixed 2^-4 scale (values up to ~1e6 in magnitude fit; 1e-5 of the output scale against fp64 held from 1e-2 to 300 times the rollout's
 * magnitudes in tests/test_knn_gnn_gpu.py); 1 three bf16 pieces, six products (fp32's exponent range) -- with the six weight matrices
 * PRE-PACKED as MFMA A operands (pack under the mode the launch will run in): csplat_gnn_node_update_pack lays Wa, Wx, W2, W3 and the
 * next layer's Wi, Wj (both NULL: none; all [128][128] row-major, contiguous) out in `image` (csplat_gnn_node_update_image_bytes() bytes
 * of device memory, 16-byte aligned) -- once per weight version; csplat_gnn_node_update_packed is the launch (has_next = the image holds
 * Wi / Wj and xa_next / xb_next are written).  23 us (mode 0) / 30 us (mode 1) against 44 for csplat_gnn_node_update at N = 1e4.
 * piece_ptr != NULL: `agg` holds the PIECES csplat_gnn_edge_mlp3's fused aggregation left, node v's aggregate = the sum of pieces
 * piece_ptr[v] .. piece_ptr[v + 1] - 1 in that order (int32 [N + 1]) -- formed while the rows are loaded, no csplat_gnn_segment_sum launch. */
size_t csplat_gnn_node_update_image_bytes(void);
int csplat_gnn_node_update_pack(void *stream, const float *Wa, const float *Wx, const float *W2, const float *W3, const float *Wi_next,
                                const float *Wj_next, void *image);
int csplat_gnn_node_update_packed(void *stream, int64_t N, const float *agg, const float *x, const void *image, const float *b0,
                                  const float *b2, const float *b3, const float *ln_gamma, const float *ln_beta, float ln_eps,
                                  int has_next, float *x_new, float *xa_next, float *xb_next, const int32_t *piece_ptr);

/* LayerNorm(128) of the MeshNet MLPs under autograd (/root/reference/meshnet/graph_network.py:86-97,139-150: every edge / node
 * MLP ends in nn.LayerNorm), single HBM passes over [M][128] rows:
 *   csplat_ln128_fwd   y = (x - mean) * rstd * gamma + beta; stats[row] = (mean, rstd)  (biased variance, as torch)
 *   csplat_ln128_bwd   dx; dgamma[128] = sum_rows g * xhat; dbeta[128] = sum_rows g  (fixed summation order: deterministic);
 *                      dxsum[128] (or NULL) = column sums of dx: the bias gradient of the Linear layer whose output was normalised;
 *                      g_rows[M] (or NULL): row r of the incoming gradient is g[g_rows[r]] -- the backward of the segmented sum
 *                      that follows the edge LayerNorm (every edge reads its destination node's row) without a gathered copy;
 *                      x_normalized != 0: `x` holds xhat = (x - mean) * rstd itself (what csplat_linear128_ex's LayerNorm
 *                      epilogue leaves with gamma = 1, beta = 0), stats only supplies rstd
 *   csplat_relu_mask_bias128   gm = out > 0 ? g : 0 and dbias[128] = column sums of gm: ReLU backward + bias gradient of a
 *                      Linear + ReLU layer in one pass (out NULL: no mask; gm NULL: sums only)
 * partials: 3 x csplat_ln128_partial_floats(M) floats of scratch (1 x for csplat_relu_mask_bias128).
 * Alignment (refused otherwise, before anything is launched): x, y, g, dx, out, gm, gamma, beta and partials 16 bytes, stats 8 bytes. */
size_t csplat_ln128_partial_floats(int64_t M);
int csplat_ln128_fwd(void *stream, int64_t M, const float *x, const float *gamma, const float *beta, float eps, float *y, float *stats);
int csplat_ln128_bwd(void *stream, int64_t M, const float *g, const float *x, const float *stats, const float *gamma, float *dx,
                     float *dgamma, float *dbeta, float *dxsum, const int64_t *g_rows, int x_normalized, float *partials);
int csplat_relu_mask_bias128(void *stream, int64_t M, const float *g, const float *out, float *gm, float *dbias, float *partials);

/* Weight gradient of a 128 -> 128 Linear layer under autograd: dW[o][i] = sum_e g[e][o] * x[e][i], g and x [M][128] row-major,
 * dW [128][128] (torch Linear.weight layout).  Exact-fp32 MFMA, split over row slices, partial results summed in slice order
 * (deterministic).  workspace: csplat_dw128_workspace_bytes(M) bytes, no initial state. */
size_t csplat_dw128_workspace_bytes(int64_t M);
int csplat_dw128(void *stream, int64_t M, const float *g, const float *x, float *dW, void *workspace);
/* the same with dbias[128] = column sums of g (the bias gradient, from the g rows the product reads anyway) and, when x_relu != 0,
 * max(x, 0) in place of x (a layer whose saved input is the PRE-activation of the ReLU in front of it) */
int csplat_dw128_bias(void *stream, int64_t M, const float *g, const float *x, int x_relu, float *dW, float *dbias, void *workspace);

/* how csplat_linear128 forms its products: 0 = v_mfma_f32_32x32x2_f32 (exact fp32 products); 1 = three bf16 pieces per
 * operand and the six significant partial products on v_mfma_f32_32x32x16_bf16 (fp32 accumulate; error ~3 x 2^-24 relative
 * per term -- measured rms error vs fp64 1.2e-7, the fp32-MFMA path and the library sgemm 1.5e-7 --; 6/16 of the
 * matrix-core time).  Default 1.  Applies to the persistent (edge-level) kernel. */
int csplat_linear128_mode(unsigned mode);
unsigned csplat_linear128_mode_query(void);   /* the mode currently in force */
int csplat_linear128(void *stream, int64_t M, const float *A, const float *W, const float *bias, float alpha, int relu,
                     const float *gather_a, const int64_t *index_a, const float *gather_b, const int64_t *index_b,
                     const float *ln_gamma, const float *ln_beta, float ln_eps, const float *add_pre,
                     const float *add_post, float *out);
/* The same product for the autograd path, where the weight is seldom a contiguous [128][128] matrix of its own: W is read as
 * W[j * ldw + k] (w_transposed = 0: a Linear.weight, or a 128-column slice of a wider one, ldw = its row stride) or as W[k * ldw + j]
 * (w_transposed = 1: the transpose, i.e. the input-gradient product g @ W, without materialising W^T); and `mask` [M][128] (or NULL)
 * zeroes the outputs whose mask entry is not positive, after everything else: the ReLU backward of the layer whose saved
 * output is handed in, folded into the GEMM that produces its incoming gradient.  ln_stats [M][2] (or NULL): with a LayerNorm
 * epilogue, the (mean, rstd) of every row -- what csplat_ln128_bwd needs, so that training can take the fused epilogue too.
 * Alignment (both entries; refused otherwise, before anything is launched): A, W, out, bias, add_pre, add_post and mask 16 bytes,
 * ln_stats 8 bytes.
 * Non-finite data: a NaN or +-Inf in a row of A makes that row's outputs non-finite and no other; with the fp32 products an Inf gives
 * the +-Inf torch.nn.functional.linear gives, with the bf16 split (x - bf16(x) = Inf - Inf) it gives NaN. */
int csplat_linear128_ex(void *stream, int64_t M, const float *A, const float *W, int ldw, int w_transposed, const float *bias,
                        float alpha, int relu, const float *gather_a, const int64_t *index_a, const float *gather_b,
                        const int64_t *index_b, const float *ln_gamma, const float *ln_beta, float ln_eps,
                        const float *add_pre, const float *add_post, const float *mask, float *ln_stats, float *out);

/* out[M,128] = (ReLU)(x[M,K] W^T + bias) for a narrow input, 1 <= K <= 32: the first Linear of the encoders' MLPs
 * (/root/reference/meshnet/graph_network.py:48-111, build_mlp's NN-0 on 4 edge / 8 node features).  W is [128][ldw >= K] row-major as
 * nn.Linear stores it, x is [M][ldx >= K]; bias may be NULL; out is dense [M][128], 16-byte aligned. */
int csplat_linear_narrow128(void *stream, int64_t M, int K, const float *x, int ldx, const float *W, int ldw, const float *bias, int relu,
                            float *out);

/* The WHOLE edge MLP of an InteractionNetwork layer in one launch (inference; csplat_edge_mlp.hip) -- replaces the three csplat_linear128
 * calls of rounds 1-4 for /root/reference/meshnet/graph_network.py:178-199 (`message`: LN(MLP(cat[x_i, x_j, e]))):
 *     out[e] = LayerNorm( W2 relu( W1 relu( alpha * W0 e0[e] + b0 + xa[index_a[e]] + xb[index_b[e]] ) + b1 ) + b2 ) * gamma + beta
 * e0 / out [E][128] fp32 (out != e0), xa / xb [N][128] (the node-level x_i / x_j column-block products of the first Linear; N < 2^23),
 * index_a / index_b int64 [E], alpha a power of two (the edge scale 2^l of SURVEY F7).  `image` = the three weight matrices as
 * csplat_gnn_edge_mlp3_pack lays them out (csplat_gnn_edge_mlp3_image_bytes() bytes of device memory, 16-byte aligned): per wave of the
 * kernel the 16-bit pieces of its 32 output rows of the three W as MFMA A operands, in the order the kernel loads them into registers.
 * Pack once per weight version AND mode: W_l is read as W_l[j * ld_l + k] (a Linear.weight or a 128-column slice of a wider one).
 * csplat_gnn_edge_mlp3_mode(mode) selects the arithmetic and returns the previous mode (any other value only queries):
 *   0 (default)  two fp16 pieces per operand, three products.  The values are brought into fp16's range by ONE power of two per launch,
 *                taken from e0_absmax = the device word csplat_absmax leaves (max |e0| over the launch's rows or over a superset of them;
 *                NULL = 1.0).  Per row, in units of max(max_j |out|, 1), against fp64 (fp32 itself: 5e-7): 4e-7 .. 9e-7 for rows whose inner
 *                activations are within 2^6 of the launch's scale max |e0| x alpha; 3e-5 .. 5e-5 at 2^12 (the OTHER rows of a launch that
 *                holds one edge row 2^12 above them); 1e-4 at 2^14 (rows without edge features at alpha 16384) and up to O(1) beyond.  An
 *                inner activation 2^12 ABOVE the edge rows' scale, or an understated e0_absmax, leaves fp16's range: a NaN row, never a
 *                wrong finite one.  Table: tests/test_edge_mlp_cpu.py; the arithmetic: header of csplat_edge_mlp.hip.
 *   1            three bf16 pieces per operand, six products: fp32's exponent range, 7e-7 against fp64; e0_absmax is not read.
 * csplat_absmax(n, x, out): *out = max |x[i]| over the elements that are not NaN (fmaxf ignores a NaN; 0 for n = 0 and when all are NaN;
 * Inf for an Inf) -- n a multiple of 4, x 16-byte aligned; one pass, asynchronous on `stream`.
 * Fused aggregation (mode 0; pieces != NULL, out may be NULL and is not written): the rows are in DESTINATION order (index_a
 * non-decreasing: the caller permuted e0 / index_a / index_b by the CSR order), and instead of E message rows the launch writes their sums
 * over runs of equal index_a, cut additionally every 8 rows: piece p = sum of the rows of run p, [npieces][128] fp32, numbered in row
 * order; group_piece0[g] = number of the first piece of rows 8g .. 8g + 7 (int32 [ceil(E / 8)]).  A node's aggregate (graph_network.py:
 * 201-222, aggr = 'add') is the sum of its consecutive pieces -- csplat_gnn_segment_sum over the piece rows; one writer per piece, fixed
 * order of addition: deterministic.  Replaces the E x 128 write here and the E x 128 read of the segmented sum by ~(E / 8 + N) x 128. */
int csplat_gnn_edge_mlp3_mode(int mode);
size_t csplat_gnn_edge_mlp3_image_bytes(void);
int csplat_gnn_edge_mlp3_pack(void *stream, const float *W0, int ld0, const float *W1, int ld1, const float *W2, int ld2, void *image);
int csplat_absmax(void *stream, int64_t n, const float *x, float *out);
int csplat_gnn_edge_mlp3(void *stream, int64_t E, const float *e0, float alpha, const float *e0_absmax, const float *xa,
                         const int64_t *index_a, const float *xb, const int64_t *index_b, const void *image, const float *b0,
                         const float *b1, const float *b2, const float *ln_gamma, const float *ln_beta, float ln_eps, float *out,
                         const int32_t *group_piece0, float *pieces);

/* The same kernel as a stand-alone operator on NARROW input rows -- the encoders' MLPs (/root/reference/meshnet/graph_network.py:48-111:
 * build_mlp(K -> 128 -> 128 -> 128) + LayerNorm) in ONE launch:
 *     out[m] = LayerNorm( W2 relu( W1 relu( W0 x[m] + b0 ) + b1 ) + b2 ) * gamma + beta
 * x [M][K] fp32 (K a multiple of 4, 4 .. 128; M <= 2^22), out [M][128].  `image` = csplat_gnn_edge_mlp3_pack(W0 PADDED with zero columns
 * to [128][128], W1, W2) under mode 0; x_absmax = csplat_absmax of x (or of a superset; NULL = 1.0).  Mode 0 (fp16 pieces) only. */
int csplat_gnn_mlp3_rows(void *stream, int64_t M, const float *x, int K, const float *x_absmax, const void *image, const float *b0,
                         const float *b1, const float *b2, const float *ln_gamma, const float *ln_beta, float ln_eps, float *out);

/* The per-step activations of the Gaussian parameters as render() consumes them (/root/reference/scene_reconstruction/
 * gaussian_model.py:96-121 via gaussian_renderer/__init__.py:92-118): opacity[P] = sigmoid(opacity_raw), scales[P][3] = exp(scaling_raw),
 * shs[P][16][3] = cat(features_dc[P][1][3], features_rest[P][15][3]) in one launch, and their backward in one launch (any incoming
 * gradient may be NULL = zero). */
int csplat_gauss_act_fwd(void *stream, int64_t P, const float *opacity_raw, const float *scaling_raw, const float *features_dc,
                         const float *features_rest, float *opacity, float *scales, float *shs);
int csplat_gauss_act_bwd(void *stream, int64_t P, const float *opacity, const float *scales, const float *g_opacity,
                         const float *g_scales, const float *g_shs, float *d_opacity_raw, float *d_scaling_raw,
                         float *d_features_dc, float *d_features_rest);

/* The two device-wide primitives the library is built on (csrc/csplat_sort.hip), as entry points of their own so that a test can reach
 * them: the rasterizer's tile sort and tiles_touched scan, the k-NN Morton sorts, the Chamfer backward's (index, query) sort, the GNN CSR
 * build and csplat_mask_to_map all run on them.  Added exports: CSPLAT_ABI_VERSION is unchanged.
 *
 * csplat_sort_pairs_u64: stable LSD radix sort of n (u64 key, u32 value) pairs, 8 bits per pass, ceil(end_bit / 8) passes.
 *   The order is that of key bits [0, 8 * ceil(end_bit / 8)) -- whole digits, NOT [0, end_bit): for end_bit = 10 the bits 10..15 take
 *   part.  Key bits at or above 8 * ceil(end_bit / 8) travel with their key into keys_out and do not affect the order.  Pairs whose
 *   ordered bits are equal keep their input order.  1 <= end_bit <= 64; n >= 0 (n = 0: a no-op that accepts NULL pointers); n below 2^32.
 *   The inputs are not written; keys_out / vals_out [n] must not be the inputs (refused) nor overlap them.
 *   temp: csplat_sort_pairs_temp_bytes(n) bytes of device memory (a second key and value buffer and the 256 x ceil(n / 4096) digit table).
 * csplat_scan_u32: out[i] = in[0] + ... + in[i] modulo 2^32, n >= 0 (n = 0: a no-op that accepts NULL pointers).  `out` must not be `in`
 *   (refused) nor overlap it.  temp: csplat_scan_u32_temp_bytes(n) bytes of device memory.
 * Errors (non-zero, text from csplat_last_error names the entry point) are raised before any launch. */
size_t csplat_sort_pairs_temp_bytes(int64_t n);
int csplat_sort_pairs_u64(void *stream, int64_t n, int end_bit, const uint64_t *keys_in, const uint32_t *vals_in, uint64_t *keys_out,
                          uint32_t *vals_out, void *temp);
size_t csplat_scan_u32_temp_bytes(int64_t n);
int csplat_scan_u32(void *stream, int64_t n, const uint32_t *in, uint32_t *out, void *temp);

#ifdef __cplusplus
}
#endif
#endif /* CSPLAT_H */
