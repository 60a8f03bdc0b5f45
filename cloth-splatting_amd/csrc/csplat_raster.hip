// csplat_raster.hip -- the depth-aware differentiable Gaussian rasterizer for gfx950 (MI355X).
//
// Replaces the CUDA extension behind GaussianRasterizer.forward / backward
// (the reference's gaussian_renderer/__init__.py:16,76,156-164; backward via
// scene_reconstruction/train_utils.py:288).
//
// One translation unit in parts.  The device code of every stage but K7 lives in a part, csplat_raster_*.h: each is included below exactly
// once, in this order, compiles only here, and opens and closes the anonymous namespace itself.  K7 and the host code stay in this file:
// its SHA-1 is what bench.py and the profile collectors key the committed K7 counters by, and __FILE__ is what a caller reads in an error
// text (csplat_last_error).  "needs" = the earlier parts a part uses names of.  Kernel inventory = SURVEY.md 2.1 K1..K8.
//
// csplat_raster_math.h      needs: --
//      constants, Geom / Cam / ProjJac, the quaternion -> cov3D -> cov2D chain, antialiasing helpers, tile_rect, SH row staging
// csplat_raster_k1.h        needs: math
//   K1 k_preprocess        per-Gaussian cull / projection / cov3D / cov2D / conic / radius / rect / SH->RGB
// csplat_raster_binning.h   needs: math, k1 (K1Table)
//   K2 (csplat_sort.hip)   inclusive scan of tiles_touched
//   K3 k_emit_keys         (tile<<32 | depth bits, id) per touched tile
//   K4 (csplat_sort.hip)   stable radix sort
//   K5 k_tile_ranges       [first,last) per tile; k_seg_plan (SEG = 256-entry segments of every tile list);
//      k_tile_count .. k_tile_sort   the tile-bucketed path that stands in for K2-K5 up to BUCKET_TILES tiles: the in-LDS tile sort
// csplat_raster_k5b_k6.h    needs: binning
//      k_block_masks       per list entry: which of the tile's sixteen 4x4 pixel blocks it can reach + tile-ordered records
//   K6 k_composite_fwd     front-to-back compositing of RGB + depth: one wavefront per 4x4 block, four survivors per step
// (this file)               needs: math, binning (SEG), k5b_k6
//   K7 k_composite_bwd     per (segment, quadrant) workgroup, forward-ordered replay from the checkpoints, factored moment reduction
//                          reduction, LDS records, one atomic per (entry, quadrant)
// csplat_raster_extended.h  needs: math, binning (SEG), k5b_k6 (ALPHA_MIN), K7
//      the depth-gradient, feature / alpha and visibility paths (listed below), but for their K1 / K8 kernels
// csplat_raster_k8.h        needs: math, K7 (ACC_STRIDE)
//   K8 k_preprocess_bwd    conic->cov2D->cov3D/mean, mean2D(NDC)->mean3D, colour->SH, cov3D->(scale,quat); the batched K8 kernels
//                          (body: csplat_k8_views_body.h), k_bg_partials, k_cam_sum
// (this file)               needs: every part
//      from the "---- layouts" rule to the end, the host code: the chunk layouts and their typed views (Geom, ImageView, BinView,
//      TempView, ScratchView), the two-phase forward and the extended forward passes, then the backward: one view's launches
//      (backward_one, launch_k8), the batched ones (launch_k8_views, backward_views_depth / _colour), the one way in (backward_views_impl)
//      and the exported entries
//
// Every stage has a `_views` form: all views of a step (at most RASTER_MAX_VIEWS) in one launch, blockIdx.y = view.
// The extended paths, each launched only when a view asks for it (csplat_view, include/csplat.h):
//   antialiasing           k_preprocess_aa, k_preprocess_bwd_aa (+ _views): K1 / K8 with the opacity compensation       (k1, k8)
//   depth gradient         k_depth_bwd_partials, k_depth_composite_bwd_views, k_preprocess_bwd_depth (+ _views)         (extended, k8)
//   camera / background    k_preprocess_bwd_cam (+ _views), k_bg_partials, k_cam_sum                                    (k8)
//   features, alpha        k_feature_fwd_views, k_feature_bwd_partials, k_feature_composite_bwd_views, k_feature_grads  (extended)
//   visibility             k_visibility_walk_views, k_visibility_reduce_views                                           (extended)
//   bit-reproducible mode  k_composite_bwd_rows<true>, *_det, k_*det_reduce*: ordered sums instead of float atomics (debug flag 256)
// Build-time switches, given to build.sh as -D...: CSPLAT_SEG (csplat_raster_binning.h), CSPLAT_K7X (K7, this file).
//
// Index-deciding arithmetic (radius, tile rectangle, sort key) is compiled with FP contraction OFF and is
// written in the same association order as oracle/raster_ref.c, so tile/bin indices are bit-exact.
#include "csplat_common.h"

#include <atomic>
#include <cstring>
#include <chrono>
#include <mutex>
#include <type_traits>

#include "csplat_raster_math.h"
#include "csplat_raster_k1.h"
#include "csplat_raster_binning.h"
#include "csplat_raster_k5b_k6.h"

namespace {

// ------------------------------------------------------------------------------------------- K7
// per-Gaussian gradient accumulator filled by K7 and consumed by K8 (one 64-byte record per Gaussian):
//   rounds 1-5: 0 dmean2D.x  1 dmean2D.y  2 dconic.a  3 dconic.b  4 dconic.c  5 dopacity  6..8 dcolour  9..15 pad
//   round 6:    0 Mx  1 My  2 Mxx  3 Mxy  4 Myy  5 M0 (= dopacity)  6..8 dcolour -- moments of G dL/dalpha (moments_to_gradients, K8)
constexpr int ACC_STRIDE = 16;

// ---- K7's chains across the four survivor rows of a group (round 4).  v_permlane16_swap(x, x) hands every lane the two values of its
// row PAIR (even row's, odd row's); one v_permlane32_swap of the pair's product / sum hands it the totals of both pairs.  The prefix a row
// needs is then two row-masked DPP operations away -- 2 swaps + 2 masked ops per chain instead of an all-gather of the four values
// (3 swaps), four dependent operations and three row selects.  The product / sum of a group associates as (f0 f1)(f2 f3) instead of
// front to back: K7's T and S differ from a sequential walk in the last bit (K7 takes every blend decision from n_contrib, not from T).
#define CSPLAT_ROWMASK_OP(OP, dst, src0, src1, RM)                                                                                  \
    asm("s_nop 1\n\tv_" OP "_f32_dpp %0, %1, %2 quad_perm:[0,1,2,3] row_mask:" RM " bank_mask:0xf" : "+v"(dst) : "v"(src0), "v"(src1))
// Tin: the pixel's transmittance in front of the group (same in the pixel's four lanes) -> in front of the lane's own survivor, behind the group
__device__ __forceinline__ void rows_scan_mul(float f, float Tin, float &Tr, float &Tout) {
    const auto s16 = __builtin_amdgcn_permlane16_swap(__float_as_uint(f), __float_as_uint(f), false, false);
    const float ev = __uint_as_float(s16[0]), od = __uint_as_float(s16[1]);       // the pair's even / odd row
    const float pr = ev * od;
    const auto s32 = __builtin_amdgcn_permlane32_swap(__float_as_uint(pr), __float_as_uint(pr), false, false);
    const float lo = __uint_as_float(s32[0]), hi = __uint_as_float(s32[1]);       // rows 0-1, rows 2-3
    float base = Tin;
    CSPLAT_ROWMASK_OP("mul", base, lo, Tin, "0xc");                               // rows 2, 3: behind the first pair
    Tr = base;
    CSPLAT_ROWMASK_OP("mul", Tr, ev, base, "0xa");                                // odd rows: behind the pair's even row
    Tout = (Tin * lo) * hi;
}
// inclusive: Sr = Sin + the addends up to and including the lane's own survivor
__device__ __forceinline__ void rows_scan_add(float g, float Sin, float &Sr, float &Sout) {
    const auto s16 = __builtin_amdgcn_permlane16_swap(__float_as_uint(g), __float_as_uint(g), false, false);
    const float ev = __uint_as_float(s16[0]), od = __uint_as_float(s16[1]);
    const float pr = ev + od;
    const auto s32 = __builtin_amdgcn_permlane32_swap(__float_as_uint(pr), __float_as_uint(pr), false, false);
    const float lo = __uint_as_float(s32[0]), hi = __uint_as_float(s32[1]);
    float base = Sin;
    CSPLAT_ROWMASK_OP("add", base, lo, Sin, "0xc");
    float incl = ev;
    CSPLAT_ROWMASK_OP("add", incl, od, ev, "0xa");
    Sr = base + incl;
    Sout = (Sin + lo) + hi;
}
// grid: one 4-wave workgroup per (segment slot, group of four live blocks); wave w = one 4x4 block.  The four waves of a workgroup
// share nothing but the launch geometry: no LDS records, no barrier.
// Round 4, first step: a wave's survivors are the entries of the segment its block BLENDED (bbits, written by K6 -- see bbits_flush), not
// the entries that reach the block: the four ballot words arrive with one scalar load, the whole segment's survivor list is laid out in
// the wave's LDS ring before the first group (no mask loads, no ingest inside the loop, a counted loop), and every group of four does
// arithmetic that lands in a gradient: 280 -> 259 us for the four views of a step.
// Second step: the nine row sums of a survivor go STRAIGHT to the Gaussian's 64-byte record (one global float atomic request per (entry,
// block): the nine lanes that hold the sums address one record).  Rounds 1-3 added them into an LDS record per list entry first (shared
// by the workgroup's four blocks, ds_add_f32), zeroed before and flushed behind a barrier -- a quarter of the global requests, but: an
// LDS float atomic per group on a unit the CU's 32 waves share, 9 KB of zeroing and ten flush rounds per workgroup, and every wave waiting
// at the barrier for the slowest of its four blocks (8.7 k of a live wave's 46 k cycles, tools/k7_stamps.py).  259 -> 241 us (same-box
// A/B, three alternations).  DET (csplat_debug_flags bit 8, bit-reproducible): the sums are STORED, one 9-float record per (list entry,
// block) -- each pair is visited exactly once -- and k_det_reduce adds every Gaussian's records in emission order.
#ifndef CSPLAT_K7X
#define CSPLAT_K7X 0
#endif
constexpr int RING7 = SEG;     // a segment's survivors of one block, padded to a multiple of four: at most SEG
// DEPTH (the depth-gradient path, k_depth_composite_bwd_views; never the default launches): the pixel's depth gradient g = dL_ddepth[pix]
// adds g (T_i z_i - D_behind_i / (1 - alpha_i)) to dL/dalpha, with D_behind_i = (sum of the partials dpart of this and the later segments
// of the tile, k_depth_bwd_partials) - (the in-segment prefix of T alpha z through entry i), and the block's sum of g T_i alpha_i goes to
// record slot 9 (dL/dz of the Gaussian, K8).  With DEPTH = false every added line below is compiled out.
// FEAT (the feature / alpha path, k_feature_composite_bwd_views, always with DEPTH; never the default launches): with the pixel's feature
// gradients gf_c = dL_dfeat[c][pix] (c < nf <= 6), wf_i = sum_c gf_c f[id_i][c] and the alpha image's gradient gA = dL_dalpha[pix], adds
// Tr_i wf_i - (Fsuf - gA T_final - SF_i) / (1 - alpha_i) to dL/dalpha, where Fsuf = the prepass partials (k_feature_bwd_partials: T alpha wf
// summed per segment) of this and the tile's later segments and SF_i = the in-segment prefix of T alpha wf through entry i; the block's
// sums of gf_c T_i alpha_i go to record slots 10 + c (dL/df of the Gaussian: k_feature_grads).  Lanes 6, 7, 10, 13, 14, 15 of a row -- free
// in the default record layout -- carry them, so an (entry, block) pair is still ONE atomic request to one 64-byte record.
template <bool DET, bool DEPTH = false, bool FEAT = false>
__device__ __forceinline__ void composite_bwd_body(int tiles, int W, int H, int gx, const int2 *__restrict__ ranges,
                                                   const uint32_t *__restrict__ ids_sorted,
                                                   const unsigned long long *__restrict__ bbits, const float4 *__restrict__ recA,
                                                   const float4 *__restrict__ recB, const float2 *__restrict__ recC,
                                                   uint32_t null_rec, const int *__restrict__ seg_offset,
                                                   const int *__restrict__ slot_tile, const float4 *__restrict__ ckpt,
                                                   const float *__restrict__ final_T, const uint32_t *__restrict__ n_contrib,
                                                   const float *__restrict__ out_color, const float *__restrict__ dL_dpix,
                                                   float *__restrict__ acc, float *__restrict__ det,
                                                   unsigned long long *stamp = nullptr, int wg = (int)blockIdx.x,
                                                   const float *__restrict__ dL_ddepth = nullptr, const float *__restrict__ dpart = nullptr,
                                                   const float *__restrict__ features = nullptr, int nf = 0,
                                                   const float *__restrict__ dL_dfeat = nullptr, const float *__restrict__ dL_dalpha = nullptr,
                                                   const float *__restrict__ wpart = nullptr) {
    static_assert(!FEAT || DEPTH, "the feature path is instantiated on the depth path");
    constexpr int DS = FEAT ? 16 : (DEPTH ? 10 : 9);                // floats per stored (entry, block) record in the DET mode
    using TT = std::conditional_t<FEAT, TripF, Trip>;
    __shared__ int s_ring[4][RING7];
    __shared__ float4 s_ra[4][64], s_rb[4][64];                     // one batch of 64 survivors' records per wave (see `stage`)
    __shared__ float s_rc[4][64];
    constexpr bool IDS = !DET || FEAT;                              // the survivors' Gaussian ids are staged
    __shared__ uint32_t s_rid[IDS ? 4 : 1][IDS ? 64 : 1];
    __shared__ float s_rz[DEPTH ? 4 : 1][DEPTH ? 64 : 1];          // (DEPTH) the survivors' view-space depths
    __shared__ float s_rf[FEAT ? 4 : 1][FEAT ? CSPLAT_MAX_FEATURES : 1][FEAT ? 64 : 1];   // (FEAT) the survivors' feature rows
    // in-kernel stamps (csplat_debug_stamps; tools/k7_stamps.py): wave 0 of every workgroup leaves s_memtime at the phase boundaries
    unsigned long long *my_stamp = stamp ? stamp + ((size_t)blockIdx.y * gridDim.x + (size_t)wg) * 12 : nullptr;
    auto mark = [&](int k) {
        if (my_stamp && threadIdx.x == 0) {
            asm volatile("" ::: "memory");
            my_stamp[k] = (unsigned long long)__builtin_amdgcn_s_memtime();
            asm volatile("" ::: "memory");
        }
    };
    mark(0);
    const int slot = ((wg >> 5) << 3) + (wg & 7), quad = (wg >> 3) & 3;     // the 4 workgroups of a slot share blockIdx % 8
    if (slot >= seg_offset[tiles]) return;
    const int tile = slot_tile[slot];
    const int seg = slot - seg_offset[tile];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63, r = lane >> 4, l16 = lane & 15;
    const int seg_lo = seg * SEG;
    // (round 3) K6 leaves every block's largest n_contrib (blk_hi).  The blocks of the tile that still blend something at or behind this
    // segment -- blk_hi > seg_lo -- are PACKED four to a workgroup in index order: workgroup `quad` of the slot takes the live blocks
    // 4 quad .. 4 quad + 3, whichever quadrant of the tile they lie in (they only share the segment's LDS records).
    const uint32_t *blk_hi = reinterpret_cast<const uint32_t *>(seg_offset) + tiles + 1 + tile * 16;
    uint32_t livemask = 0u;
#pragma unroll
    for (int b = 0; b < 16; b++) livemask |= ((int)blk_hi[b] > seg_lo ? 1u : 0u) << b;
    const int n_live = __builtin_popcount(livemask);
    if (4 * quad >= n_live) return;                                      // (workgroup-uniform)
    const int kth = 4 * quad + __builtin_amdgcn_readfirstlane(w);
    uint32_t m_ = livemask;
    for (int i = 0; i < kth && m_; i++) m_ &= m_ - 1u;
    const bool has_block = kth < n_live;
    const int blk = has_block ? __builtin_ctz(m_) : 0;
    // the entries of this segment the block blended: four 64-bit words, one scalar load
    constexpr int NW = SEG / 64;
    const unsigned long long *bw = bbits + ((size_t)slot * 16 + (size_t)blk) * NW;
    unsigned long long sw[NW];
#pragma unroll
    for (int c = 0; c < NW; c++) sw[c] = has_block ? bw[c] : 0ull;
    const int px = (tile % gx) * CSPLAT_TILE + (blk & 3) * 4 + (l16 & 3);
    const int py = (tile / gx) * CSPLAT_TILE + (blk >> 2) * 4 + (l16 >> 2);
    const bool inside = px < W && py < H;
    const int pix = py * W + px;
    const float fx = (float)px, fy = (float)py;
    const int2 range = ranges[tile];
    const uint32_t rx = (uint32_t)range.x;
    mark(1);                                                            // the scalar chain (slot -> tile -> range, blk_hi, bbits) has returned
    // ONE memory round trip for everything a wave needs before its first group: the pixel's constants, its checkpoint and (below, `stage`)
    // the records + ids of its first 64 survivors are requested together
    unsigned long long any_ = 0ull;
#pragma unroll
    for (int c = 0; c < NW; c++) any_ |= sw[c];
    const bool live = any_ != 0ull;
    const size_t HW = (size_t)H * W;
    int ncontrib = 0;
    float dp0 = 0.f, dp1 = 0.f, dp2 = 0.f, oc0 = 0.f, oc1 = 0.f, oc2 = 0.f;
    float4 ck = make_float4(1.f, 0.f, 0.f, 0.f);
    if (live) {
        if (inside) {
            ncontrib = (int)n_contrib[pix];
            dp0 = dL_dpix[pix]; dp1 = dL_dpix[HW + pix]; dp2 = dL_dpix[2 * HW + pix];
            oc0 = out_color[pix]; oc1 = out_color[HW + pix]; oc2 = out_color[2 * HW + pix];
        }
        ck = ckpt[(size_t)slot * 256 + blk * 16 + l16];
    }
    float gz = 0.f, Dsuf = 0.f;         // (DEPTH) the pixel's dL/ddepth; T alpha z summed over this and the tile's later segments
    if constexpr (DEPTH) {
        if (live && dL_ddepth) {
            if (inside) gz = dL_ddepth[pix];
            const int s_end = seg_offset[tile + 1];
            for (int s2 = slot; s2 < s_end; s2++) Dsuf += dpart[(size_t)s2 * 256 + blk * 16 + l16];
        }
    }
    float gf[FEAT ? CSPLAT_MAX_FEATURES : 1], OFA = 0.f;  // (FEAT) the pixel's feature gradients; Fsuf - gA T_final
    if constexpr (FEAT) {
#pragma unroll
        for (int c = 0; c < CSPLAT_MAX_FEATURES; c++) gf[c] = 0.f;
        if (live) {
            float Fsuf = 0.f, gA = 0.f;
            if (inside) {
                if (dL_dfeat)
#pragma unroll
                    for (int c = 0; c < CSPLAT_MAX_FEATURES; c++) gf[c] = c < nf ? dL_dfeat[c * HW + pix] : 0.f;
                if (dL_dalpha) gA = dL_dalpha[pix] * final_T[pix];
            }
            if (dL_dfeat) {
                const int s_end = seg_offset[tile + 1];
                for (int s2 = slot; s2 < s_end; s2++) Fsuf += wpart[(size_t)s2 * 256 + blk * 16 + l16];
            }
            OFA = Fsuf - gA;
        }
    }
    // the wave's survivor list: list positions of the set bits, in order, padded with -1 to a multiple of four (wave-private LDS)
    int *ring = s_ring[w];
    int total = 0;
    if (live) {
#pragma unroll
        for (int c = 0; c < NW; c++) {
            const unsigned long long cur = sw[c];
            if ((cur >> lane) & 1ull) {
                const int rank = (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(cur >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)cur, 0u));
                ring[total + rank] = seg_lo + 64 * c + lane;
            }
            total += (int)__popcll(cur);
        }
        const int pad = (-total) & 3;
        if (lane < pad) ring[total + lane] = -1;
        total += pad;
    }
    mark(2);
    if (live) {
        // ---- the survivors' RECORDS go through LDS, 64 survivors (16 groups) a batch: lane i requests survivor i's record (x, y, conic,
        // opacity, colour -- 36 bytes -- and the Gaussian's id) and parks it in the wave's strip; the group loop then contains NO vector
        // load, only LDS reads (row r reads slot 4k + r: a broadcast) and the atomics.  Why: vmcnt counts loads and atomics together, IN
        // ORDER -- a record requested behind an atomic cannot be used before that atomic has retired, and under load a float atomic stays
        // counted for ~3,000 cycles (MI355X_MICROARCH.md, cycle constants).  With the records fetched from global memory two groups
        // ahead, every group waited for the atomic of the group before the last: 1,670 cycles per group for ~350 of arithmetic
        // (tools/k7_stamps.py).  The first batch's requests travel with the pixel constants and the checkpoint: one round trip in all
        // before the first group; later batches (a block that blended more than 64 of the segment's 256 entries) wait once per batch.
        float4 *ra = s_ra[w], *rb = s_rb[w];
        float *rc = s_rc[w];
        uint32_t *rid = s_rid[IDS ? w : 0];
        auto stage = [&](int b0) {      // survivors b0 .. b0 + 63 -> the strip
            const int idx = b0 + lane;
            const int pos = idx < total ? ring[idx] : -1;
            const uint32_t ri = pos >= 0 ? rx + (uint32_t)pos : null_rec;
            const float4 A = recA[ri], B = recB[ri];
            const float C = reinterpret_cast<const float *>(recC)[2 * (size_t)ri];      // (c.y, the depth, is K6's)
            uint32_t id = 0u;
            if (IDS) id = ids_sorted[pos >= 0 ? rx + (uint32_t)pos : rx];
            ra[lane] = A; rb[lane] = B; rc[lane] = C;
            if (IDS) rid[lane] = id;
            if constexpr (DEPTH) s_rz[w][lane] = reinterpret_cast<const float *>(recC)[2 * (size_t)ri + 1];
            if constexpr (FEAT)
#pragma unroll
                for (int c = 0; c < CSPLAT_MAX_FEATURES; c++) s_rf[w][c][lane] = c < nf ? features[(size_t)id * nf + c] : 0.f;
        };
        stage(0);
        const float OD = oc0 * dp0 + oc1 * dp1 + oc2 * dp2;
        float T = 1.f, S = 0.f;
        float SD = 0.f;                 // (DEPTH) in-segment running sum of T alpha z
        float SF = 0.f;                 // (FEAT) in-segment running sum of T alpha wf
        if (ncontrib > seg_lo) {
            T = ck.x;
            S = ck.y * dp0 + ck.z * dp1 + ck.w * dp2;
        }
        if (my_stamp && threadIdx.x == 0) { asm volatile("" :: "v"(S), "v"(T)); }
        mark(3);                                                        // the pixel constants, the checkpoint and the first batch have arrived
        // after the moment reduction (processN) nine lanes of a row hold a record entry each: lane 4 j + t of the row = block pixel
        // (column t, row j).  Record: 0 Mx  1 My  2 Mxx  3 Mxy  4 Myy  5 M0  6..8 colour (K8: moments -> dL/dmean2D, dL/dconic)
        const bool lq0 = (l16 & 3) == 0, lq1 = (l16 & 3) == 1, lq2 = (l16 & 3) == 2;
        constexpr int RED_T[16] = {5, 0, 2, 7, 4, -1, -1, -1, 1, 3, -1, 8, 6, -1, -1, -1};
        int red_t_ = -1;
#pragma unroll
        for (int q = 0; q < 16; q++) red_t_ = l16 == q ? RED_T[q] : red_t_;
        if constexpr (DEPTH) red_t_ = l16 == 5 ? 9 : red_t_;          // (lane 5 of a row carries the depth sum: slot 9, same 64-byte record)
        // (FEAT) lanes 6, 7, 10, 13, 14, 15 of a row carry the feature sums of channels 0..5: slots 10..15
        const int fch = !FEAT ? -1 : (l16 == 6 ? 0 : (l16 == 7 ? 1 : (l16 == 10 ? 2 : (l16 == 13 ? 3 : (l16 == 14 ? 4 : (l16 == 15 ? 5 : -1))))));
        if constexpr (FEAT) red_t_ = (fch >= 0 && fch < nf) ? 10 + fch : red_t_;
        const bool red_active = red_t_ >= 0;
        const int red_t = red_active ? red_t_ : 0;
        int base = 0;                   // first survivor of the batch in the strip
        // (every LDS read of the loop is unconditional, with a clamped slot: the compiler's lgkmcnt bookkeeping assumes the path on which
        //  a conditional read was NOT issued, and then waits for the youngest ones)
        auto fetch = [&](TT &t, int k) {
            const int sl = 4 * k + r;
            t.pos = ring[base + sl];
            t.a = ra[sl]; t.b = rb[sl]; t.c.x = rc[sl];
            if (!DET) t.id = rid[sl];
            if constexpr (DEPTH) t.c.y = s_rz[w][sl];
            if constexpr (FEAT) {
                float wf = 0.f;
#pragma unroll
                for (int c = 0; c < CSPLAT_MAX_FEATURES; c++) wf += gf[c] * s_rf[w][c][sl];
                t.wf = wf;
            }
        };
        // N groups at once, statement by statement: a group is one dependent chain of ~110 vector instructions (~10 cycles from one to the
        // next: ~1,200 cycles a group for a wave on its own, tools/k7_stamps.py -- the same with the atomics removed); groups k and k + 1
        // only meet where T and S pass from one to the other, so written side by side the two chains fill each other's waits.
        auto processN = [&](auto NC, const TT *const *t) {
            constexpr int N = decltype(NC)::value;
            float dx[N], dy[N], G[N], al[N], F[N], gdot[N], Tr[N], Sr[N], dcc[N], tot[N];
            bool act[N];
#pragma unroll
            for (int u = 0; u < N; u++) {
                dx[u] = t[u]->a.x - fx; dy[u] = t[u]->a.y - fy;
                const float power = -0.5f * (t[u]->a.z * dx[u] * dx[u] + t[u]->b.x * dy[u] * dy[u]) - t[u]->a.w * dx[u] * dy[u];
                G[u] = __expf(power);
                const float a = fminf(0.99f, t[u]->b.y * G[u]);
                act[u] = t[u]->pos < ncontrib && power <= 0.f && a >= ALPHA_MIN;   // (padding: pos = -1, opacity 0 -> a = 0)
                al[u] = act[u] ? a : 0.f;
                F[u] = 1.f - al[u];
                gdot[u] = t[u]->b.z * dp0 + t[u]->b.w * dp1 + t[u]->c.x * dp2;
            }
#pragma unroll
            for (int u = 0; u < N; u++) rows_scan_mul(F[u], T, Tr[u], T);
#pragma unroll
            for (int u = 0; u < N; u++) dcc[u] = al[u] * Tr[u];
#pragma unroll
            for (int u = 0; u < N; u++) rows_scan_add(gdot[u] * dcc[u], S, Sr[u], S);
            float SDr[N], zs[N];
            if constexpr (DEPTH) {
#pragma unroll
                for (int u = 0; u < N; u++) rows_scan_add(act[u] ? dcc[u] * t[u]->c.y : 0.f, SD, SDr[u], SD);
#pragma unroll
                for (int u = 0; u < N; u++) {   // the block's sum of g T alpha over the row's 16 pixels (dL/dz of the survivor)
                    float v = gz * dcc[u];
                    v += __shfl_xor(v, 1, 16); v += __shfl_xor(v, 2, 16); v += __shfl_xor(v, 4, 16); v += __shfl_xor(v, 8, 16);
                    zs[u] = v;
                }
            }
            float SFr[N];
            if constexpr (FEAT) {
#pragma unroll
                for (int u = 0; u < N; u++) rows_scan_add(act[u] ? dcc[u] * t[u]->wf : 0.f, SF, SFr[u], SF);
            }
#pragma unroll
            for (int u = 0; u < N; u++) {
                float dL_dalpha = act[u] ? Tr[u] * gdot[u] - (OD - Sr[u]) * __builtin_amdgcn_rcpf(F[u]) : 0.f;
                if constexpr (DEPTH) dL_dalpha += act[u] ? gz * (Tr[u] * t[u]->c.y - (Dsuf - SDr[u]) * __builtin_amdgcn_rcpf(F[u])) : 0.f;
                if constexpr (FEAT) dL_dalpha += act[u] ? Tr[u] * t[u]->wf - (OFA - SFr[u]) * __builtin_amdgcn_rcpf(F[u]) : 0.f;
                // Round 6: the row's lanes no longer form the nine GRADIENT values and reduce each over the 16 pixels (14 multiplications + a
                // 4-level butterfly of ~24 DPP operations); they reduce the MOMENTS of m = G dL/dalpha about the Gaussian's centre,
                //   M0 = sum m, Mx = sum m dx, My = sum m dy, Mxx = sum m dx^2, Mxy = sum m dx dy, Myy = sum m dy^2,
                // which factor over the 4 x 4 block (dx depends on the pixel column only, dy on the row only): first over the rows j at a
                // fixed column (values m, m dy, m dy^2 and colour 0 -- a two-level transposing fold on the 4-lane banks), then over the
                // columns with the weights 1, dx, dx^2 (two quad_perm levels); colours 1 and 2 take a five-step reduction of their own.
                // 7 multiplications + 19 DPP adds + 3 selects; K8 turns the summed moments into dL/dmean2D and dL/dconic once per
                // Gaussian: dL/dmean2D = -0.5 o (a Mx + b My, c My + b Mx), dL/dconic = -0.5 o (Mxx, Mxy, Myy), dL/dopacity = M0.
                const float gda = G[u] * dL_dalpha;
                const float c0v = dcc[u] * dp0, c1v = dcc[u] * dp1, c2v = dcc[u] * dp2;
                float a1, a2, P, Q, R, X, b1, b2;
                asm("v_mul_f32 %0, %8, %10\n\t"                                                               // a1 = m dy
                    "v_mul_f32 %1, %0, %10\n\t"                                                               // a2 = m dy^2
                    "v_add_f32_dpp %2, %8, %8 row_ror:8 row_mask:0xf bank_mask:0x3\n\t"                       // P (rows 0, 1) = m      + partner row's
                    "v_add_f32_dpp %5, %12, %12 row_ror:8 row_mask:0xf bank_mask:0x3\n\t"                     // X (rows 0, 1) = colour 1
                    "v_add_f32_dpp %5, %13, %13 row_ror:8 row_mask:0xf bank_mask:0xc\n\t"                     // X (rows 2, 3) = colour 2
                    "v_add_f32_dpp %2, %0, %0 row_ror:8 row_mask:0xf bank_mask:0xc\n\t"                       // P (rows 2, 3) = m dy
                    "v_add_f32_dpp %3, %1, %1 row_ror:8 row_mask:0xf bank_mask:0x3\n\t"                       // Q (rows 0, 1) = m dy^2
                    "v_add_f32_dpp %3, %11, %11 row_ror:8 row_mask:0xf bank_mask:0xc\n\t"                     // Q (rows 2, 3) = colour 0
                    "v_add_f32_dpp %4, %2, %2 row_ror:12 row_mask:0xf bank_mask:0x5\n\t"                      // R (rows 0, 2) = P over all four rows
                    "v_add_f32_dpp %5, %5, %5 row_half_mirror row_mask:0xf bank_mask:0xf\n\t"                 // X: the half's pairs
                    "v_add_f32_dpp %4, %3, %3 row_ror:4 row_mask:0xf bank_mask:0xa\n\t"                       // R (rows 1, 3) = Q over all four rows
                    "v_mul_f32 %6, %4, %9\n\t"                                                                // b1 = R dx
                    "v_mul_f32 %7, %6, %9\n\t"                                                                // b2 = R dx^2
                    "v_add_f32_dpp %5, %5, %5 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"
                    "v_add_f32_dpp %4, %4, %4 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"
                    "v_add_f32_dpp %6, %6, %6 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"
                    "v_add_f32_dpp %7, %7, %7 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"
                    "v_add_f32_dpp %5, %5, %5 quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf\n\t"
                    "v_add_f32_dpp %4, %4, %4 quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf\n\t"
                    "v_add_f32_dpp %6, %6, %6 quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf\n\t"
                    "v_add_f32_dpp %7, %7, %7 quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf"
                    : "=&v"(a1), "=&v"(a2), "=&v"(P), "=&v"(Q), "=&v"(R), "=&v"(X), "=&v"(b1), "=&v"(b2)
                    : "v"(gda), "v"(dx[u]), "v"(dy[u]), "v"(c0v), "v"(c1v), "v"(c2v));
                // column t of the block's lane grid keeps: t = 0 the plain sums, t = 1 the dx-weighted, t = 2 the dx^2-weighted, t = 3 colours 1 / 2
                tot[u] = lq0 ? R : (lq1 ? b1 : (lq2 ? b2 : X));
                if constexpr (DEPTH) tot[u] = l16 == 5 ? zs[u] : tot[u];
                if constexpr (FEAT) {   // the block's sums of gf_c T alpha over the row's 16 pixels (dL/df_c of the survivor)
                    float fsel = tot[u];
#pragma unroll
                    for (int c = 0; c < CSPLAT_MAX_FEATURES; c++) {
                        const float fsum = row_total(gf[c] * dcc[u]);
                        fsel = fch == c ? fsum : fsel;
                    }
                    tot[u] = fsel;
                }
            }
            // (every survivor of the list was blended at one of the block's pixels: the row always has something to add, padding aside)
#pragma unroll
            for (int u = 0; u < N; u++)
                if (red_active && t[u]->pos >= 0) {
                    if (DET) det[((size_t)(rx + (uint32_t)t[u]->pos) * 16 + (size_t)blk) * DS + red_t] = tot[u];   // one (entry, block) pair is visited exactly once
                    else if (CSPLAT_K7X != 1) atomicAdd(acc + (size_t)t[u]->id * ACC_STRIDE + red_t, tot[u]);                      // nine lanes, one 64-byte record
                    else asm volatile("" :: "v"(tot[u]));        // (elimination build CSPLAT_K7X=1: the sums are formed, nothing is sent)
                }
        };
        auto process = [&](const TT &t0) { const TT *t[1] = {&t0}; processN(std::integral_constant<int, 1>{}, t); };
        auto process2 = [&](const TT &t0, const TT &t1) { const TT *t[2] = {&t0, &t1}; processN(std::integral_constant<int, 2>{}, t); };
        bool first = true;
        // (round 6, tried and dropped: requesting the NEXT batch's records before this batch's atomics are issued -- vmcnt retires in order and
        //  a load queued behind a float atomic waits for it -- costs ten registers across the batch (44 bytes of scratch at the 64-register
        //  bound) and changed nothing: 214-215 against 210-217 us, profiles/r06_k7_elimination.txt)
        for (; base < total && CSPLAT_K7X != 4; base += 64) {
            if (!first) stage(base);
            const int ngroups = min(64, total - base) >> 2, last_g = ngroups - 1;
            // two groups in flight: group k + 2 is read from the strip when group k has been composited
            TT ta, tb;
            fetch(ta, 0);
            fetch(tb, min(1, last_g));
            if (first) {
                if (my_stamp && threadIdx.x == 0) { asm volatile("" :: "v"(ta.a.x), "v"(ta.c.x)); }
                mark(4);                                                // strip -> the first group's records have arrived
            }
            first = false;
            int k = 0;
            for (; k + 1 < ngroups; k += 2) {       // (a fetch past the end re-reads the last group: never processed)
                process2(ta, tb);
                fetch(ta, min(k + 2, last_g));
                fetch(tb, min(k + 3, last_g));
            }
            if (k < ngroups) process(ta);
        }
    }
    mark(5);                                                            // this wave's groups are done
    if (my_stamp && threadIdx.x == 0) { my_stamp[8] = (unsigned long long)total; my_stamp[9] = 1ull; }
}

// (four survivors x 16 pixels per step.  The survivor-column forms of round 3 -- 16 survivors per step, DPP row scans, MFMA reduction:
// 29 % fewer VALU instructions but 112 VGPRs = 4 waves per SIMD, and slower -- left the library in round 4; they are in the history at
// commit 809fd4b and described in DESIGN section 6)
template <bool DET>
__global__ __launch_bounds__(256) void k_composite_bwd_rows(int tiles, int W, int H, int gx, const int2 *__restrict__ ranges,
                                                             const uint32_t *__restrict__ ids_sorted,
                                                             const unsigned long long *__restrict__ bbits, const float4 *__restrict__ recA,
                                                             const float4 *__restrict__ recB, const float2 *__restrict__ recC,
                                                             uint32_t null_rec, const int *__restrict__ seg_offset,
                                                             const int *__restrict__ slot_tile, const float4 *__restrict__ ckpt,
                                                             const float *__restrict__ final_T, const uint32_t *__restrict__ n_contrib,
                                                             const float *__restrict__ out_color, const float *__restrict__ dL_dpix,
                                                             float *__restrict__ acc, float *__restrict__ det) {
    composite_bwd_body<DET>(tiles, W, H, gx, ranges, ids_sorted, bbits, recA, recB, recC, null_rec, seg_offset, slot_tile, ckpt, final_T,
                            n_contrib, out_color, dL_dpix, acc, det, nullptr);
}

// K7 for ALL views of a step in one launch (blockIdx.y = view), preceded by one launch that clears every view's records
struct B2View {
    const int2 *ranges;
    const uint32_t *ids_sorted;
    const unsigned long long *bbits;
    const float4 *recA, *recB;
    const float2 *recC;
    const int *seg_offset, *slot_tile;
    const float4 *ckpt;
    const float *final_T;
    const uint32_t *n_contrib;
    const float *out_color, *dL_dpix;
    float *acc;
    uint32_t R;
    float *det;        // bit-reproducible mode: the (entry, block) records behind the per-Gaussian ones, else NULL
};
struct B2Table { B2View v[RASTER_MAX_VIEWS]; unsigned long long *stamp; const uint32_t *valid; };
__global__ __launch_bounds__(256, 8) void k_composite_bwd_rows_views(int tiles, int W, int H, int gx, B2Table tab) {
    if (tab.valid && *tab.valid == 0u) return;     // (a forward launched on faith whose counts did not fit: its chunks hold nothing)
    const B2View &w = tab.v[blockIdx.y];
    composite_bwd_body<false>(tiles, W, H, gx, w.ranges, w.ids_sorted, w.bbits, w.recA, w.recB, w.recC, w.R, w.seg_offset, w.slot_tile, w.ckpt,
                              w.final_T, w.n_contrib, w.out_color, w.dL_dpix, w.acc, nullptr, tab.stamp);
}
// the same launch in the bit-reproducible mode (round 6: the batched and the recorded step take the mode too, so that an eager and a
// replayed step can be compared bit for bit)
__global__ __launch_bounds__(256) void k_composite_bwd_rows_views_det(int tiles, int W, int H, int gx, B2Table tab) {
    if (tab.valid && *tab.valid == 0u) return;
    const B2View &w = tab.v[blockIdx.y];
    composite_bwd_body<true>(tiles, W, H, gx, w.ranges, w.ids_sorted, w.bbits, w.recA, w.recB, w.recC, w.R, w.seg_offset, w.slot_tile, w.ckpt,
                             w.final_T, w.n_contrib, w.out_color, w.dL_dpix, w.acc, w.det, nullptr);
}
__global__ __launch_bounds__(256) void k_zero_det_views(B2Table tab) {
    if (tab.valid && *tab.valid == 0u) return;
    const B2View &w = tab.v[blockIdx.y];
    float4 *p = reinterpret_cast<float4 *>(w.det);
    const int64_t n4 = ((int64_t)(w.R > 0 ? w.R : 1) * 16 * 9 + 3) / 4;        // (the layout's field is a multiple of 256 bytes: the tail is ours)
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) p[i] = make_float4(0.f, 0.f, 0.f, 0.f);
}
__global__ __launch_bounds__(256) void k_zero_acc_views(int64_t n4, B2Table tab) {
    float4 *p = reinterpret_cast<float4 *>(tab.v[blockIdx.y].acc);
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) p[i] = make_float4(0.f, 0.f, 0.f, 0.f);
}

// DET mode, second half: Gaussian i sums the records of its tile instances in emission order (tiles y-major, x; quadrants
// 0..3): a fixed order, whatever the scheduling of K7.  The instance of Gaussian i in a tile's sorted list is found by
// binary search on the unique (depth bits, id) key.
__global__ __launch_bounds__(256) void k_det_reduce(int P, Cam cam, const float2 *__restrict__ xy, const float *__restrict__ depth,
                                                     const int32_t *__restrict__ radii, const int2 *__restrict__ ranges,
                                                     const uint64_t *__restrict__ keys_sorted, const uint32_t *__restrict__ ids_sorted,
                                                     const float *__restrict__ det, float *__restrict__ acc) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= P) return;
    float s[9];
#pragma unroll
    for (int t = 0; t < 9; t++) s[t] = 0.f;
    const int rad = radii[i];
    if (rad > 0) {
        const float2 p = xy[i];
        int minx, miny, maxx, maxy;
        tile_rect(p.x, p.y, rad, cam, minx, miny, maxx, maxy);
        const uint64_t want = ((uint64_t)__float_as_uint(depth[i]) << 32) | (uint32_t)i;
        for (int y = miny; y < maxy; y++)
            for (int x = minx; x < maxx; x++) {
                const int2 rg = ranges[y * cam.gx + x];
                int lo = rg.x, hi = rg.y;
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    const uint64_t k = ((keys_sorted[mid] & 0xFFFFFFFFull) << 32) | ids_sorted[mid];
                    if (k < want) lo = mid + 1; else hi = mid;
                }
                for (int q = 0; q < 16; q++)
#pragma unroll
                    for (int t = 0; t < 9; t++) s[t] += det[((size_t)lo * 16 + q) * 9 + t];
            }
    }
#pragma unroll
    for (int t = 0; t < 9; t++) acc[(size_t)i * ACC_STRIDE + t] = s[t];
}

struct DetView { Cam cam; const float2 *xy; const float *depth; const int32_t *radii; const int2 *ranges; const uint64_t *keys_sorted;
                 const uint32_t *ids_sorted; const float *det; float *acc; };
struct DetTable { DetView v[RASTER_MAX_VIEWS]; const uint32_t *valid; };
// NF floats per stored record: 9, or 10 on the depth path (slot 9 = dL/dz)
template <int NF>
__device__ __forceinline__ void det_reduce_views_body(int P, const DetTable &tab) {
    if (tab.valid && *tab.valid == 0u) return;
    const DetView &w = tab.v[blockIdx.y];
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= P) return;
    float s[NF];
#pragma unroll
    for (int t = 0; t < NF; t++) s[t] = 0.f;
    const int rad = w.radii[i];
    if (rad > 0) {
        const float2 p = w.xy[i];
        int minx, miny, maxx, maxy;
        tile_rect(p.x, p.y, rad, w.cam, minx, miny, maxx, maxy);
        const uint64_t want = ((uint64_t)__float_as_uint(w.depth[i]) << 32) | (uint32_t)i;
        for (int y = miny; y < maxy; y++)
            for (int x = minx; x < maxx; x++) {
                const int2 rg = w.ranges[y * w.cam.gx + x];
                int lo = rg.x, hi = rg.y;
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    const uint64_t k = ((w.keys_sorted[mid] & 0xFFFFFFFFull) << 32) | w.ids_sorted[mid];
                    if (k < want) lo = mid + 1; else hi = mid;
                }
                for (int q = 0; q < 16; q++)
#pragma unroll
                    for (int t = 0; t < NF; t++) s[t] += w.det[((size_t)lo * 16 + q) * NF + t];
            }
    }
#pragma unroll
    for (int t = 0; t < NF; t++) w.acc[(size_t)i * ACC_STRIDE + t] = s[t];
}
__global__ __launch_bounds__(256) void k_det_reduce_views(int P, DetTable tab) { det_reduce_views_body<9>(P, tab); }

}  // namespace

#include "csplat_raster_extended.h"
#include "csplat_raster_k8.h"

namespace {

// csplat_debug_flags: the CSPLAT_DEBUG_* bits of csplat.h.  (bits 13, 14, 16-21 selected the shelved kernel forms of round 3; they left the
// library in round 4 and are ignored)
unsigned g_debug_flags = 0;
bool dbg(unsigned bits) { return (g_debug_flags & bits) != 0; }
// K5b's exact ellipse-against-block stage is off under any of these
constexpr unsigned DBG_NO_ELLIPSE_STAGE = CSPLAT_DEBUG_NO_CULLING | CSPLAT_DEBUG_CULL_RADIUS_X4 | CSPLAT_DEBUG_CIRCLE_ONLY;

// ------------------------------------------------------------------------------------------- layouts
// The saved state of a view lives in chunks the caller allocates (GEOM, IMAGE, BINNING, TEMP): every field 256-byte aligned, in enum
// order.  ONE function per chunk knows the sizes (*_offsets) and one hands out typed pointers (*_view): nothing else indexes a layout.
size_t lay_out(const size_t *sz, int n, size_t *off) {
    size_t o = 0;
    for (int k = 0; k < n; k++) { off[k] = o; o += align256(sz[k]); }
    return o;
}
int tiles_of(int W, int H) { return cdiv(W, CSPLAT_TILE) * cdiv(H, CSPLAT_TILE); }
int64_t max_slots(int64_t R, int tiles) { return R / SEG + tiles + 1; }

enum { G_DEPTH, G_XY, G_CONIC, G_RGB, G_COV3D, G_CLAMPED, G_TOUCHED, G_OFFSETS, G_CUT2, G_SCANTMP, G_PACK, G_NFIELDS };
size_t geom_offsets(int P, size_t *off) {
    const size_t n = (size_t)(P > 0 ? P : 1);
    const size_t sz[G_NFIELDS] = {n * 4, n * 8, n * 16, n * 12, n * 24, n * 4, n * 4, n * 4, n * 4,
                                  csplat_scan_temp_bytes(P), n * 48};
    return lay_out(sz, G_NFIELDS, off);
}
Geom geom_view(const void *base, int P) {
    size_t off[G_NFIELDS];
    geom_offsets(P, off);
    char *b = (char *)base;
    Geom g;
    g.depth = (float *)(b + off[G_DEPTH]); g.xy = (float2 *)(b + off[G_XY]);
    g.conic_opacity = (float4 *)(b + off[G_CONIC]); g.rgb = (float *)(b + off[G_RGB]);
    g.cov3D = (float *)(b + off[G_COV3D]); g.clamped = (uint32_t *)(b + off[G_CLAMPED]);
    g.tiles_touched = (uint32_t *)(b + off[G_TOUCHED]); g.offsets = (uint32_t *)(b + off[G_OFFSETS]);
    g.cut2 = (float *)(b + off[G_CUT2]);
    g.scan_tmp = (void *)(b + off[G_SCANTMP]);
    g.pack = (float4 *)(b + off[G_PACK]);
    return g;
}
// image: ranges int2[tiles] | n_contrib u32[H][W] | final_T f32[H][W] | info u32: [0] R, [1] longest list, [2] non-empty tiles; word 64: the
//        number of non-empty tiles, their ids in tile order; word 64 + tiles + 4: the same ids, longest list first (K6's launch order)
enum { I_RANGES, I_NCONTRIB, I_FINALT, I_INFO, I_NFIELDS };
struct ImageView { int2 *ranges; uint32_t *n_contrib; float *final_T; uint32_t *info; };
size_t image_offsets(int W, int H, size_t *off) {
    const size_t tiles = (size_t)tiles_of(W, H), X = (size_t)W * H;
    const size_t sz[I_NFIELDS] = {tiles * 8, X * 4, X * 4, 256 + 2 * (tiles + 4) * 4};
    return lay_out(sz, I_NFIELDS, off);
}
ImageView image_view(const void *base, int W, int H) {
    size_t off[I_NFIELDS];
    image_offsets(W, H, off);
    char *b = (char *)base;
    return {(int2 *)(b + off[I_RANGES]), (uint32_t *)(b + off[I_NCONTRIB]), (float *)(b + off[I_FINALT]), (uint32_t *)(b + off[I_INFO])};
}
// per-(counting workgroup, tile) table of the bucketed binning path; requested as its own TEMP-class chunk
size_t bucket_table_bytes(int P, int tiles) { return align256(((size_t)cdiv(P > 0 ? P : 1, BUCKET_G) + 1) * tiles * 4); }
// binning (the field numbers are ABI: csplat_binning_fields hands all eleven offsets out, in this order):
//   B_KEYS keys_sorted u64[R] | B_IDS ids_sorted u32[R] | B_SEG seg_offset i32[tiles+1] + blk_hi u32[tiles][16] (largest n_contrib of every
//   4x4 pixel block, written by K6: K7 drops the (segment, quadrant) workgroups behind it on ONE scalar load; the kernels find it behind
//   seg_offset themselves) | B_SLOT slot_tile i32[slots]
//   | B_CKPT ckpt float4[slots][16 blocks][16 pixels]   (slots = R/SEG + tiles + 1 bounds sum_t ceil(n_t/SEG))
//   | B_MASK mask16 u16[R+1] | B_RECA recA float4[R+1] | B_RECB recB float4[R+1] | B_RECC recC float2[R+1]   (entry R = the null record)
//   | B_BBITS bbits u64[slots][16 blocks][SEG / 64]: per segment and block, which of the segment's 256 entries the block BLENDED (K6 -> K7)
//   | B_BMASK bmask u64[R / 64 + 4][16 blocks]: mask16 TRANSPOSED -- per 64 list entries (global index >> 6) and block, which entries
//     reach the block (K5b -> K6, one scalar 8-byte load per chunk instead of 64 mask loads and a ballot)
enum { B_KEYS, B_IDS, B_SEG, B_SLOT, B_CKPT, B_MASK, B_RECA, B_RECB, B_RECC, B_BBITS, B_BMASK, B_NFIELDS };
struct BinView {
    uint64_t *keys_sorted; uint32_t *ids_sorted; int *seg_offset, *slot_tile; float4 *ckpt; uint16_t *mask16; float4 *recA, *recB; float2 *recC;
    unsigned long long *bbits, *bmask;
};
size_t binning_offsets(int64_t R, int tiles, size_t *off) {
    const size_t n = (size_t)(R > 0 ? R : 1), slots = (size_t)max_slots(R, tiles);
    const size_t sz[B_NFIELDS] = {n * 8, n * 4, (size_t)(tiles + 1) * 4 + (size_t)tiles * 16 * 4, slots * 4, slots * 256 * 16, (n + 1) * 2,
                                  (n + 1) * 16, (n + 1) * 16, (n + 1) * 8, slots * 16 * (SEG / 8), ((n + 63) / 64 + 4) * 16 * 8};
    return lay_out(sz, B_NFIELDS, off);
}
BinView binning_view(const void *base, int64_t R, int tiles) {
    size_t off[B_NFIELDS];
    binning_offsets(R, tiles, off);
    char *b = (char *)base;
    BinView v;
    v.keys_sorted = (uint64_t *)(b + off[B_KEYS]); v.ids_sorted = (uint32_t *)(b + off[B_IDS]);
    v.seg_offset = (int *)(b + off[B_SEG]); v.slot_tile = (int *)(b + off[B_SLOT]); v.ckpt = (float4 *)(b + off[B_CKPT]);
    v.mask16 = (uint16_t *)(b + off[B_MASK]); v.recA = (float4 *)(b + off[B_RECA]); v.recB = (float4 *)(b + off[B_RECB]);
    v.recC = (float2 *)(b + off[B_RECC]); v.bbits = (unsigned long long *)(b + off[B_BBITS]);
    v.bmask = (unsigned long long *)(b + off[B_BMASK]);
    return v;
}
// temp: the unsorted keys and ids, the radix sort's ping-pong copies and its table (the bucketed path uses keys_u only)
enum { T_KEYS_U, T_IDS_U, T_KEYS_T, T_IDS_T, T_SORT, T_NFIELDS };
struct TempView { uint64_t *keys_u; uint32_t *ids_u; uint64_t *keys_t; uint32_t *ids_t; void *sort_tmp; };
size_t temp_offsets(int64_t R, size_t *off) {
    const size_t n = (size_t)(R > 0 ? R : 1);
    const size_t sz[T_SORT] = {n * 8, n * 4, n * 8, n * 4};
    off[T_SORT] = lay_out(sz, T_SORT, off);
    return off[T_SORT] + csplat_sort_temp_bytes(R);
}
TempView temp_view(void *base, int64_t R) {
    size_t off[T_NFIELDS];
    temp_offsets(R, off);
    char *b = (char *)base;
    return {(uint64_t *)(b + off[T_KEYS_U]), (uint32_t *)(b + off[T_IDS_U]), (uint64_t *)(b + off[T_KEYS_T]), (uint32_t *)(b + off[T_IDS_T]),
            (void *)(b + off[T_SORT])};
}

// the list capacity the view's BINNING chunk (and its scratch) was laid out for
int layout_R(const csplat_view &w) { return w.layout_rendered > 0 ? w.layout_rendered : w.num_rendered; }
// backward scratch.  Four nested layouts, one per path of the backward, each a prefix of the next in enum order:
//   colour   S_ACC records f32[P][ACC_STRIDE] | S_DET (entry, block) records f32[R][16][9]
//   depth    S_ACC | S_DET f32[R][16][10] (slot 9 = dL/dz) | S_DPART depth partials f32[slots][256], one per (segment, pixel)
//   camera   the depth layout | S_CAMSLAB f32[ceil(P / 32)][CAM_NC] (at most one row per 32 Gaussians: the batched K8's workgroup)
//            | S_BGSLAB f32[BG_BLOCKS][3]
//   feature  the camera layout | S_WPART feature partials f32[slots][256] | S_FDET (entry, block) records f32[R][16][16]
// The (entry, block) records exist in the bit-reproducible mode only (else 0 bytes).  The feature layout still carries the depth layout's
// 10-float region, unused: its K7 writes S_FDET.  A camera call whose K7 is the colour one keeps its 9-float records in S_DET.
enum ScratchPath { SP_COLOUR, SP_DEPTH, SP_CAMERA, SP_FEATURE };
enum { S_ACC, S_DET, S_DPART, S_CAMSLAB, S_BGSLAB, S_WPART, S_FDET, S_NFIELDS };
constexpr int S_LAST[] = {S_DET, S_DPART, S_BGSLAB, S_FDET};      // every path's last field
size_t scratch_offsets(ScratchPath path, int P, int64_t R, int W, int H, bool det_mode, size_t *off) {
    const size_t p = (size_t)(P > 0 ? P : 1), det = det_mode ? (size_t)(R > 0 ? R : 1) * 16 * 4 : 0;
    const size_t part = (size_t)max_slots(R, tiles_of(W, H)) * 256 * 4;
    const size_t sz[S_NFIELDS] = {p * ACC_STRIDE * 4, det * (path == SP_COLOUR ? 9 : 10), part, (size_t)cdiv(p, 32) * CAM_NC * 4,
                                  (size_t)BG_BLOCKS * 3 * 4, part, det * 16};
    return lay_out(sz, S_LAST[path] + 1, off);
}
// det: the (entry, block) records the path's K7 writes (NULL outside the bit-reproducible mode), det_bytes: their field, to be cleared;
// a field the path does not lay out is NULL, and so is every field of a view without scratch
struct ScratchView { float *acc, *det, *dpart, *cam_slab, *bg_slab, *wpart; size_t det_bytes; };
ScratchView scratch_view(const csplat_view &w, ScratchPath path) {
    size_t off[S_NFIELDS + 1];
    const bool det_mode = dbg(CSPLAT_DEBUG_BIT_REPRODUCIBLE);
    const int last = S_LAST[path], d = path == SP_FEATURE ? S_FDET : S_DET;
    off[last + 1] = scratch_offsets(path, w.P, layout_R(w), w.W, w.H, det_mode, off);
    auto at = [&](int f) { return w.scratch && f <= last ? (float *)((char *)w.scratch + off[f]) : nullptr; };
    return {at(S_ACC), det_mode ? at(d) : nullptr, at(S_DPART), at(S_CAMSLAB), at(S_BGSLAB), at(S_WPART), det_mode ? off[d + 1] - off[d] : 0};
}

// camera constants stay in HBM (80 bytes, read through the scalar cache by every wave): no host round trip
int make_cam(Cam &c, const float *view, const float *proj, const float *campos, float tanfovx, float tanfovy, int W, int H) {
    c.view = view; c.proj = proj; c.campos = campos;
    c.tanfovx = tanfovx; c.tanfovy = tanfovy;
    c.fx = (float)W / (2.0f * tanfovx); c.fy = (float)H / (2.0f * tanfovy);
    c.W = W; c.H = H; c.gx = cdiv(W, CSPLAT_TILE); c.gy = cdiv(H, CSPLAT_TILE);
    return 0;
}
void make_cam(Cam &c, const csplat_view &w) { make_cam(c, w.view, w.proj, w.campos, w.tanfovx, w.tanfovy, w.W, w.H); }

// ---- a finished view (csplat_view) as the backward and the extended passes read it
// segments of the view: <= R / SEG + (non-empty tiles) + 1 with the EXACT counts the forward read -- the layout's bound (capacity / SEG +
// all tiles + 1) launches twice as many workgroups that find no segment
int64_t k7_slots(const csplat_view &w, int tiles) {
    return (w.busy_tiles > 0 && w.num_rendered > 0) ? (int64_t)w.num_rendered / SEG + w.busy_tiles + 1 : max_slots(layout_R(w), tiles);
}
// what every walk over a view's tile lists reads (FeatFwdView, VisView, B2View): the fields have the chunk views' names
template <typename T>
void fill_list_view(const BinView &b, const ImageView &im, T &k) {
    k.ranges = im.ranges; k.n_contrib = im.n_contrib;
    k.ids_sorted = b.ids_sorted; k.seg_offset = b.seg_offset; k.ckpt = b.ckpt; k.bbits = b.bbits; k.recA = b.recA; k.recB = b.recB;
}
// the view's K7 record (tiles: of its image) and, in the bit-reproducible mode (sv.det), what the fixed-order sum of its (entry, block)
// records reads
void fill_k7_view(const csplat_view &w, const ScratchView &sv, int tiles, B2View &k, DetView &e) {
    const BinView b = binning_view(w.binning, layout_R(w), tiles);
    const ImageView im = image_view(w.image, w.W, w.H);
    fill_list_view(b, im, k);
    k.final_T = im.final_T; k.slot_tile = b.slot_tile; k.recC = b.recC;
    k.out_color = w.out_color; k.dL_dpix = w.dL_dpix; k.acc = sv.acc; k.R = (uint32_t)layout_R(w); k.det = sv.det;
    if (!sv.det || w.P <= 0) return;      // (a view without Gaussians has no chunks: nothing sums its records)
    make_cam(e.cam, w);
    const Geom g = geom_view(w.geom, w.P);
    e.xy = g.xy; e.depth = g.depth; e.radii = w.radii; e.ranges = k.ranges; e.keys_sorted = b.keys_sorted; e.ids_sorted = k.ids_sorted;
    e.det = k.det; e.acc = k.acc;
}

// Mailboxes for the one host read of the forward (R and the longest tile list): 64 slots of host-pinned, device-mapped
// memory.  The scan kernel stores the two words, fences at system scope and stores a per-call tag; the host spins on the
// tag.  A blocking hipStreamSynchronize costs tens of microseconds of wake-up latency during which the GPU idles.
struct Mailboxes {
    volatile uint32_t *host = nullptr;
    uint32_t *dev = nullptr;
    std::atomic<uint32_t> next{1};
    bool tried = false;
};
Mailboxes g_mail;
std::mutex g_mail_mu;
constexpr int MAIL_SLOTS = 64, MAIL_WORDS = 16;

bool mail_init() {
    std::lock_guard<std::mutex> lk(g_mail_mu);
    if (!g_mail.tried) {
        g_mail.tried = true;
        void *h = nullptr, *d = nullptr;
        if (hipHostMalloc(&h, MAIL_SLOTS * MAIL_WORDS * 4, hipHostMallocMapped | hipHostMallocPortable) == hipSuccess &&
            hipHostGetDevicePointer(&d, h, 0) == hipSuccess) {
            memset(h, 0, MAIL_SLOTS * MAIL_WORDS * 4);
            g_mail.host = (volatile uint32_t *)h;
            g_mail.dev = (uint32_t *)d;
        }
        (void)hipGetLastError();
    }
    return g_mail.host != nullptr;
}

unsigned long long *g_stamp_buf = nullptr;     // csplat_debug_stamps: 12 u64 per K7 workgroup (rows form, batched launch)
size_t g_stamp_words = 0;
// ... or, when the buffer holds EXACTLY 8 u64 per workgroup of the batched K1 (P / 64) and, behind them, of the batched K8 (P / 32): those
// two kernels' stamps (k_preprocess_views_stamps, k_preprocess_bwd_views_stamps; tools/per_gaussian_stamps.py) and not K7's
unsigned long long *per_gaussian_stamps(int P) {
    return (g_stamp_buf && g_stamp_words == 8u * ((size_t)cdiv(P, 64) + (size_t)cdiv(P, 32))) ? g_stamp_buf : nullptr;
}

// `mode` argument of the tile sort kernels: bit 0 ids < 2^24, bit 1 radix only, bit 2 fallback limit 1
int tsort_mode(int P) { return (P < (1 << 24) ? 1 : 0) | (dbg(CSPLAT_DEBUG_SORT_RADIX_ONLY) ? 2 : 0) | (dbg(CSPLAT_DEBUG_SORT_RADIX_FALLBACK) ? 4 : 0); }

int higher_msb(uint32_t n) {  // number of bits needed to represent tile ids < n (upstream getHigherMsb)
    int b = 0;
    while ((1u << b) < n && b < 31) b++;
    return b == 0 ? 1 : b;
}

// events for cross-stream ordering (no timing): a ring; a wait captures the record that precedes it, so reuse is safe
hipEvent_t pooled_event() {
    constexpr int N = 256;
    static hipEvent_t ring[N];
    static std::atomic<unsigned> next{0};
    static std::mutex mu;
    const unsigned k = next.fetch_add(1) % N;
    std::lock_guard<std::mutex> lk(mu);
    if (!ring[k] && hipEventCreateWithFlags(&ring[k], hipEventDisableTiming) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    return ring[k];
}

}  // namespace

extern "C" {

int csplat_abi_version(void) { return CSPLAT_ABI_VERSION; }
int csplat_debug_flags(unsigned flags) { g_debug_flags = flags; return 0; }
unsigned csplat_debug_flags_query(void) { return g_debug_flags; }
// measurement hook: a device buffer that the batched row-form K7 fills with s_memtime stamps (12 u64 per workgroup, launch order
// [view][workgroup]); NULL switches it off.  Not part of the operator interface.
int csplat_debug_stamps(void *buf, size_t bytes) { g_stamp_buf = (unsigned long long *)buf; g_stamp_words = bytes / 8; return 0; }
}  // extern "C"
// (the stamp buffer for the library's other translation units: nullptr unless one of at least `need_words` words was handed over)
unsigned long long *csplat_stamp_buffer(size_t need_words) { return (g_stamp_buf && g_stamp_words >= need_words) ? g_stamp_buf : nullptr; }
extern "C" {
const char *csplat_last_error(void) { return g_csplat_err; }

size_t csplat_geom_bytes(int P) { size_t off[G_NFIELDS]; return geom_offsets(P, off); }
size_t csplat_image_bytes(int W, int H) { size_t off[I_NFIELDS]; return image_offsets(W, H, off); }
size_t csplat_binning_bytes(int64_t R, int W, int H) { size_t off[B_NFIELDS]; return binning_offsets(R, tiles_of(W, H), off); }
size_t csplat_temp_bytes(int P, int64_t R, int W, int H) { (void)P; (void)W; (void)H; size_t off[T_NFIELDS]; return temp_offsets(R, off); }
// backward scratch of the four paths (scratch_offsets)
static size_t scratch_bytes(ScratchPath path, int P, int64_t R, int W, int H) {
    size_t off[S_NFIELDS];
    return scratch_offsets(path, P, R, W, H, dbg(CSPLAT_DEBUG_BIT_REPRODUCIBLE), off);
}
size_t csplat_backward_scratch_bytes(int P, int64_t R) { return scratch_bytes(SP_COLOUR, P, R, 0, 0); }
size_t csplat_backward_depth_scratch_bytes(int P, int64_t R, int W, int H) { return scratch_bytes(SP_DEPTH, P, R, W, H); }
size_t csplat_backward_camera_scratch_bytes(int P, int64_t R, int W, int H) { return scratch_bytes(SP_CAMERA, P, R, W, H); }
size_t csplat_backward_feature_scratch_bytes(int P, int64_t R, int W, int H) { return scratch_bytes(SP_FEATURE, P, R, W, H); }
int csplat_geom_layout(int P, size_t *o8) { size_t off[G_NFIELDS]; geom_offsets(P, off); for (int k = 0; k < 8; k++) o8[k] = off[k]; return 0; }
// every sub-buffer of the BINNING chunk (csplat.h: csplat_binning_fields): 0 keys 1 ids 2 seg_offset + blk_hi 3 slot_tile 4 checkpoints
// 5 masks 6-8 records A / B / C 9 bbits 10 bmask; o11[11] = byte offsets for a chunk laid out for R list entries (diagnostics: tools/,
// bench.py's count of K7's atomic requests)
static_assert(B_NFIELDS == 11 && B_KEYS == 0 && B_IDS == 1 && I_RANGES == 0 && I_NCONTRIB == 1 && I_FINALT == 2, "field numbers csplat.h documents");
int csplat_binning_fields(int64_t R, int W, int H, size_t *o11) { binning_offsets(R, tiles_of(W, H), o11); return 0; }
int csplat_binning_layout(int64_t R, int W, int H, size_t *o2) {
    size_t off[B_NFIELDS];
    binning_offsets(R, tiles_of(W, H), off);
    o2[0] = off[B_KEYS]; o2[1] = off[B_IDS];
    return 0;
}
int csplat_image_layout(int W, int H, size_t *o3) {
    size_t off[I_NFIELDS];
    image_offsets(W, H, off);
    o3[0] = off[I_RANGES]; o3[1] = off[I_NCONTRIB]; o3[2] = off[I_FINALT];
    return 0;
}

// ---- two-phase forward.  begin: K1 + the counting half of the binning, everything that does not need num_rendered;
// finish: reads num_rendered (mailbox poll), allocates the R-sized chunks, K3..K6.  A caller with several independent
// views issues every begin (each on its own stream) before the first finish, so the one host round trip per view and
// the under-filled compositing kernels of different views overlap.  csplat_forward = begin + finish.
// antialiasing (csplat_view.prefiltered & CSPLAT_ANTIALIAS; bit 0, upstream's prefiltered, is ignored): K1 stores o' = o h
// (k_preprocess_aa / k_preprocess_views_aa); K8 takes its AA variant and reads the raw opacities
static bool aa_of(const csplat_view &w) { return (w.prefiltered & CSPLAT_ANTIALIAS) != 0; }

// A forward between its two phases: the call's arguments as a csplat_view, and what begin_prepare derived from them.  The outputs that
// arrive late are NOT read from `w`: the flat finish receives out_color / out_depth itself, the batched second phase takes them from
// the caller's array (p2_launch).
struct FwdTicket {
    bool used;              // (static storage: starts false; claimed in begin_prepare, given back by release_ticket)
    csplat_view w;
    csplat_alloc_fn alloc;
    hipStream_t s;
    Cam cam;
    Geom g;
    ImageView im;
    void *gbase, *ibase;
    uint32_t *table;
    int tiles, nb;
    bool can_bucket, use_mail;
    uint32_t tag;           // the mailbox triple: tag, host and device address of the slot
    volatile uint32_t *mb_host;
    uint32_t *mb_dev;
};
constexpr int MAX_TICKETS = 64;
static FwdTicket g_tickets[MAX_TICKETS];
static std::mutex g_ticket_mu;
// the ONE place a ticket is given back
static void release_ticket(int tk) {
    std::lock_guard<std::mutex> lk(g_ticket_mu);
    g_tickets[tk].used = false;
}

// allocation + bookkeeping of a forward: nothing is launched
static int begin_prepare(const csplat_view &w, csplat_alloc_fn alloc, int *ticket_out) {
    const int P = w.P, W = w.W, H = w.H;
    CSPLAT_REQUIRE(P >= 0 && W > 0 && H > 0, "csplat_forward: bad sizes");
    CSPLAT_REQUIRE(ticket_out != nullptr, "csplat_forward_begin: ticket_out missing");
    // (an empty input, P == 0, legitimately arrives with NULL data pointers)
    CSPLAT_REQUIRE(P == 0 || (w.shs != nullptr) != (w.colors_precomp != nullptr), "provide exactly one of shs / colors_precomp");
    CSPLAT_REQUIRE(P == 0 || (w.cov3D_precomp != nullptr) != (w.scales != nullptr && w.rotations != nullptr),
                   "provide exactly one of (scales, rotations) / cov3D_precomp");
    CSPLAT_REQUIRE(w.shs == nullptr || (w.D >= 0 && w.D <= 3 && w.M >= (w.D + 1) * (w.D + 1)), "SH degree / coefficient count mismatch");
    CSPLAT_REQUIRE(alloc != nullptr, "allocator callback missing");
    Cam cam;
    make_cam(cam, w);

    void *gbase = alloc(w.alloc_ctx, CSPLAT_CHUNK_GEOM, csplat_geom_bytes(P));
    void *ibase = alloc(w.alloc_ctx, CSPLAT_CHUNK_IMAGE, csplat_image_bytes(W, H));
    CSPLAT_REQUIRE(gbase && ibase, "allocator returned NULL");
    const int tiles = cam.gx * cam.gy;
    const bool can_bucket = tiles <= BUCKET_TILES && !dbg(CSPLAT_DEBUG_GLOBAL_SORT);
    uint32_t *table = nullptr;
    if (can_bucket) {
        table = (uint32_t *)alloc(w.alloc_ctx, CSPLAT_CHUNK_TABLE, bucket_table_bytes(P, tiles));
        CSPLAT_REQUIRE(table, "allocator returned NULL");
    }
    int tk = -1;
    {
        std::lock_guard<std::mutex> lk(g_ticket_mu);
        for (int i = 0; i < MAX_TICKETS && tk < 0; i++)
            if (!g_tickets[i].used) tk = i;
        if (tk >= 0) g_tickets[tk].used = true;
    }
    CSPLAT_REQUIRE(tk >= 0, "csplat_forward_begin: more than 64 forwards begun and not finished");
    FwdTicket &t = g_tickets[tk];
    t.w = w; t.alloc = alloc; t.s = (hipStream_t)w.stream;
    t.cam = cam; t.g = geom_view(gbase, P); t.im = image_view(ibase, W, H); t.gbase = gbase; t.ibase = ibase; t.table = table;
    t.tiles = tiles; t.nb = cdiv(P > 0 ? P : 1, BUCKET_G); t.can_bucket = can_bucket;
    t.use_mail = false; t.tag = 0; t.mb_host = nullptr; t.mb_dev = nullptr;
    if (can_bucket && !dbg(CSPLAT_DEBUG_NO_MAILBOX) && mail_init()) {
        t.use_mail = true;
        t.tag = g_mail.next.fetch_add(1);
        if (t.tag == 0) t.tag = g_mail.next.fetch_add(1);
        const int slot = (int)(t.tag % MAIL_SLOTS);
        t.mb_host = g_mail.host + slot * MAIL_WORDS;
        t.mb_dev = g_mail.dev + slot * MAIL_WORDS;
    }
    *ticket_out = tk;
    return 0;
}

static int nocull_mode() { return dbg(CSPLAT_DEBUG_NO_CULLING) ? 1 : dbg(CSPLAT_DEBUG_CULL_RADIUS_X4) ? 2 : 0; }

// K1 + the counting half of the binning of ONE view, on its stream
static int begin_launch(const FwdTicket &t) {
    hipStream_t s = t.s;
    const csplat_view &w = t.w;
    const int P = w.P, tiles = t.tiles, nb = t.nb;
    if (!t.can_bucket) HIP_TRY(hipMemsetAsync(t.im.ranges, 0, (size_t)tiles * 8, s));
    if (P > 0) {
        ProfScope ps(PROF_K1, s);
        auto form = [&](auto staged) {        // staged: the SH rows go through LDS
            constexpr bool STAGE = decltype(staged)::value;
            auto go = [&](auto kernel) {
                kernel<<<cdiv(P, 256), 256, 0, s>>>(P, w.D, w.M, w.means3D, w.shs, w.colors_precomp, w.opacities, w.scales, w.scale_modifier,
                                                    w.rotations, w.cov3D_precomp, t.cam, t.g, w.radii, nocull_mode());
            };
            if (aa_of(w)) go(k_preprocess_aa<STAGE>);
            else go(k_preprocess<STAGE>);
        };
        if (w.shs != nullptr && w.M == 16 && ((uintptr_t)w.shs & 15u) == 0) form(std::true_type{});
        else form(std::false_type{});
        LAUNCH_CHECK();
    }
    if (t.can_bucket) {
        ProfScope ps(PROF_K2, s);
        if (P > 0) {
            k_tile_count<<<nb, BUCKET_G, (size_t)tiles * 4, s>>>(P, tiles, t.g.xy, w.radii, t.cam, t.table);
            LAUNCH_CHECK();
        } else {
            HIP_TRY(hipMemsetAsync(t.table, 0, (size_t)nb * tiles * 4, s));
        }
        uint32_t *tile_cnt = t.table + (size_t)nb * tiles;   // last row of the chunk: per-tile totals
        k_tile_colscan<<<cdiv(tiles, 256), 256, 0, s>>>(tiles, nb, t.table, tile_cnt);
        LAUNCH_CHECK();
        k_tile_scan<<<1, 1024, 0, s>>>(tiles, tile_cnt, t.im.ranges, t.im.info, t.mb_dev, t.tag);
        LAUNCH_CHECK();
    }
    return 0;
}

// the same for V views that share the Gaussians (P, SH, opacities, scales; own means / rotations / cameras): four launches on
// `join` in all, then every view's stream waits for them.  false = the views do not qualify (the caller launches per view).
static bool begin_views_compatible(int V, const int *tk) {
    // (V == 1 qualifies too since round 5: a camera-by-camera caller -- the reference's own loop, train_utils.py:259-272 -- then gets the
    //  speculative second phase as well instead of a blocking read of its counts per camera)
    if (V < 1 || V > RASTER_MAX_VIEWS || dbg(CSPLAT_DEBUG_PER_VIEW_LAUNCHES)) return false;
    const FwdTicket &ta = g_tickets[tk[0]];
    const csplat_view &a = ta.w;
    if (a.P <= 0 || !ta.can_bucket || !a.shs || a.colors_precomp || a.cov3D_precomp || !a.scales || !a.rotations) return false;
    for (int i = 1; i < V; i++) {
        const csplat_view &w = g_tickets[tk[i]].w;
        if (w.P != a.P || w.D != a.D || w.M != a.M || w.W != a.W || w.H != a.H || w.shs != a.shs || w.opacities != a.opacities ||
            w.scales != a.scales || w.scale_modifier != a.scale_modifier || w.colors_precomp || w.cov3D_precomp || !w.rotations ||
            !g_tickets[tk[i]].can_bucket || aa_of(w) != aa_of(a))
            return false;
    }
    return true;
}
static int begin_launch_views(int V, const int *tk, hipStream_t join) {
    const FwdTicket &ta = g_tickets[tk[0]];
    const csplat_view &a = ta.w;
    const int P = a.P, tiles = ta.tiles, nb = ta.nb;
    K1Table tab;
    tab.n = V;
    for (int i = 0; i < V; i++) {
        const FwdTicket &t = g_tickets[tk[i]];
        K1View &k = tab.v[i];
        k.means3D = t.w.means3D; k.rotations = t.w.rotations; k.cam = t.cam; k.g = t.g; k.radii = t.w.radii; k.table = t.table;
        k.info = t.im.info; k.mailbox = t.mb_dev; k.ranges = t.im.ranges; k.tag = t.tag;
    }
    {
        ProfScope ps(PROF_K1, join);
        auto form = [&](auto staged) {
            constexpr bool STAGE = decltype(staged)::value;
            auto go = [&](auto kernel, auto... extra) {
                kernel<<<cdiv(P, K1V_G), 256, 0, join>>>(P, a.D, a.M, a.shs, a.opacities, a.scales, a.scale_modifier, tab, nocull_mode(), extra...);
            };
            if (aa_of(a)) go(k_preprocess_views_aa<STAGE>);
            else if (STAGE && per_gaussian_stamps(P)) go(k_preprocess_views_stamps, per_gaussian_stamps(P));   // (staged rows, no AA only)
            else go(k_preprocess_views<STAGE>);
        };
        if (a.M == 16 && ((uintptr_t)a.shs & 15u) == 0) form(std::true_type{});
        else form(std::false_type{});
        LAUNCH_CHECK();
    }
    {
        ProfScope ps(PROF_K2, join);
        k_tile_count_views<<<dim3(nb, V), BUCKET_G, (size_t)tiles * 4, join>>>(P, tiles, tab);
        LAUNCH_CHECK();
        k_tile_colscan_views<<<dim3(cdiv(tiles, 256), V), 256, 0, join>>>(tiles, nb, tab);
        LAUNCH_CHECK();
        k_tile_scan_views<<<V, 1024, 0, join>>>(tiles, nb, tab);
        LAUNCH_CHECK();
    }
    return 0;
}

// the flat begin: its arguments as a csplat_view (everything else zero; the outputs arrive with csplat_forward_finish)
int csplat_forward_begin(void *stream, int P, int D, int M, const float *bg, int W, int H, const float *means3D,
                         const float *shs, const float *colors_precomp, const float *opacities, const float *scales,
                         float scale_modifier, const float *rotations, const float *cov3D_precomp, const float *view,
                         const float *proj, const float *campos, float tanfovx, float tanfovy, int prefiltered,
                         csplat_alloc_fn alloc, void *alloc_ctx, int32_t *radii, int *ticket_out) {
    CSPLAT_REQUIRE(!(prefiltered & CSPLAT_ANTIALIAS), "csplat_forward / csplat_forward_begin: CSPLAT_ANTIALIAS needs a csplat_view entry point "
                                                      "(csplat_forward_views*), whose backward knows the bit");
    csplat_view w;
    memset(&w, 0, sizeof(w));
    w.stream = stream;
    w.P = P; w.D = D; w.M = M; w.W = W; w.H = H; w.prefiltered = prefiltered;
    w.scale_modifier = scale_modifier; w.tanfovx = tanfovx; w.tanfovy = tanfovy;
    w.bg = bg; w.means3D = means3D; w.shs = shs; w.colors_precomp = colors_precomp; w.opacities = opacities; w.scales = scales;
    w.rotations = rotations; w.cov3D_precomp = cov3D_precomp; w.view = view; w.proj = proj; w.campos = campos;
    w.alloc_ctx = alloc_ctx; w.radii = radii;
    if (int rc = begin_prepare(w, alloc, ticket_out)) return rc;
    const int rc = begin_launch(g_tickets[*ticket_out]);
    if (rc) release_ticket(*ticket_out);
    return rc;
}

// the one host read of a forward: R and the longest tile list of a view whose first phase has been launched
static int finish_read(const FwdTicket &t, uint32_t host_info[3], hipStream_t launched_on = nullptr) {
    hipStream_t s = launched_on ? launched_on : t.s;     // the stream the first phase was launched on
    host_info[0] = host_info[1] = host_info[2] = 0;
    if (t.can_bucket) {
        bool got = false;
        if (t.use_mail) {   // spin on the tag (bounded: fall back to a stream synchronise after 2 s)
            const auto t0 = std::chrono::steady_clock::now();
            unsigned spins = 0;
            while (!(got = (t.mb_host[2] == t.tag))) {
                if ((++spins & 0x3FFu) == 0 &&
                    std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > 2.0) break;
            }
            if (got) { host_info[0] = t.mb_host[0]; host_info[1] = t.mb_host[1]; host_info[2] = t.mb_host[3]; }
        }
        if (!got) {
            HIP_TRY(hipMemcpyAsync(host_info, t.im.info, 12, hipMemcpyDeviceToHost, s));
            HIP_TRY(hipStreamSynchronize(s));
        }
    } else if (t.w.P > 0) {
        ProfScope ps(PROF_K2, s);
        if (int rc = csplat_inclusive_scan_u32(s, t.g.tiles_touched, t.g.offsets, t.w.P, t.g.scan_tmp)) return rc;
        HIP_TRY(hipMemcpyAsync(host_info, t.g.offsets + (t.w.P - 1), 4, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        host_info[1] = 0xFFFFFFFFu;
        host_info[2] = 0xFFFFFFFFu;
    }
    // list positions, tile ranges and the int `num_rendered` of the ABI are 32-bit (as upstream's): refuse instead of wrapping
    CSPLAT_REQUIRE(host_info[0] <= 0x7FFFFFFFu, "csplat_forward: more than 2^31 - 1 tile instances (Gaussian x tile pairs) in one view");
    return 0;
}
// The tile sort's instantiations: keys per lane held in registers -- the launch takes the smallest that holds its longest list (the exact
// count, or the speculative capacity Lcap), so a launch of short lists is not charged the registers of an 8192-key one -- and, up to 6
// keys per lane (two workgroups' LDS fits a CU up to there), the two-workgroups-per-CU form (see k_tile_sort).
#define TSORT_FOR_ITEMS(X) X(2) X(4) X(6) X(8)
static int tsort_items(uint32_t longest) {
    const uint32_t items = (longest + TSORT_THREADS - 1) / TSORT_THREADS;
    return items <= 2 ? 2 : items <= 4 ? 4 : items <= 6 ? 6 : 8;
}
// busy: non-empty tiles of the whole launch (exact, or the capacity a speculative launch was sized for)
static bool tsort_dense(int items, uint64_t busy) {
    static int s_cus = 0;
    if (s_cus <= 0) {
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&s_cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || s_cus <= 0)
            s_cus = 256;
        (void)hipGetLastError();
    }
    return items <= 6 && 2 * busy > 5 * (uint64_t)s_cus;
}
// longest tile list the in-LDS sort takes (64 KB of keys + 17 KB of counters when the device grants 96 KB per workgroup)
static uint32_t tile_sort_cap() {
    static int s_lds_big = -1;
    if (s_lds_big < 0) {
        bool ok = true;
#define X(I) ok = ok && hipFuncSetAttribute((const void *)k_tile_sort<I, false>, hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024) == hipSuccess && \
                  hipFuncSetAttribute((const void *)k_tile_sort<I, I <= 6>, hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024) == hipSuccess &&  \
                  hipFuncSetAttribute((const void *)k_tile_sort_views<I, false>, hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024) == hipSuccess && \
                  hipFuncSetAttribute((const void *)k_tile_sort_views<I, I <= 6>, hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024) == hipSuccess;
        TSORT_FOR_ITEMS(X)
#undef X
        s_lds_big = ok;
        (void)hipGetLastError();   // a refusal must not poison the launch checks below
    }
    return s_lds_big ? (uint32_t)BUCKET_CAP : 5120u;
}
// `longest`: no tile list of the launch is longer (LDS and the keys per lane are sized from it); `busy`: its non-empty tiles
static void tile_sort_launch(hipStream_t s, int tiles, uint32_t longest, uint32_t busy, const ImageView &im, const uint64_t *comp,
                             const BinView &b, int mode) {
    const size_t lds = tsort_lds_bytes((int)longest);
    const int grid = tiles < TSORT_GRID ? tiles : TSORT_GRID, items = tsort_items(longest);
    const bool dense = tsort_dense(items, busy);
    switch (items) {
#define X(I) case I:                                                                                                                        \
        if (dense) k_tile_sort<I, I <= 6><<<grid, TSORT_THREADS, lds, s>>>(im.ranges, comp, b.keys_sorted, b.ids_sorted, im.info, tiles, mode); \
        else k_tile_sort<I, false><<<grid, TSORT_THREADS, lds, s>>>(im.ranges, comp, b.keys_sorted, b.ids_sorted, im.info, tiles, mode);    \
        break;
        TSORT_FOR_ITEMS(X)
#undef X
    }
}
static void tile_sort_views_launch(hipStream_t s, int tiles, int V, uint32_t Lcap, uint32_t Bcap, const P2Table &tab, int mode) {
    const size_t lds = tsort_lds_bytes((int)Lcap);
    const dim3 grid(tiles < TSORT_GRID ? tiles : TSORT_GRID, V);
    const int items = tsort_items(Lcap);
    const bool dense = tsort_dense(items, (uint64_t)V * (Bcap < (uint32_t)tiles ? Bcap : (uint32_t)tiles));
    switch (items) {
#define X(I) case I:                                                                                           \
        if (dense) k_tile_sort_views<I, I <= 6><<<grid, TSORT_THREADS, lds, s>>>(tab, tiles, mode);            \
        else k_tile_sort_views<I, false><<<grid, TSORT_THREADS, lds, s>>>(tab, tiles, mode);                   \
        break;
        TSORT_FOR_ITEMS(X)
#undef X
    }
}

// ---- second phase of ALL views in one launch per stage on `join` (see P2Table), as named steps: p2_qualifies, caps_from_history,
// p2_launch, p2_settle.  The entries further down compose them.
// Capacities of a batched second phase: list entries per view, longest tile list, non-empty tiles (per view)
struct Caps { uint32_t R[RASTER_MAX_VIEWS], longest, busy; };

// What the last batched call saw, per image size: the capacities the next one is launched with BEFORE its counts are read.
// (a short ring: a process that alternates between scenes of different density -- bench.py --mode scenes -- is served by the largest
// of its recent calls with the same shape instead of failing the speculation at every switch)
struct SpecHist { int W = 0, H = 0, P = 0; uint32_t R = 0, longest = 0, busy = 0; };
constexpr int SPEC_RING = 8;
static SpecHist g_spec_ring[SPEC_RING];
static int g_spec_next = 0;
static std::mutex g_spec_mu;
// info[i]: the three counts view i's first phase left (finish_read)
static void remember(int P, int W, int H, int V, const uint32_t (*info)[3]) {
    std::lock_guard<std::mutex> lk(g_spec_mu);
    SpecHist &e = g_spec_ring[g_spec_next];
    g_spec_next = (g_spec_next + 1) % SPEC_RING;
    e.W = W; e.H = H; e.P = P; e.R = 0; e.longest = 0; e.busy = 0;
    for (int i = 0; i < V; i++) {
        e.R = info[i][0] > e.R ? info[i][0] : e.R;
        e.longest = info[i][1] > e.longest ? info[i][1] : e.longest;
        e.busy = info[i][2] > e.busy ? info[i][2] : e.busy;
    }
}
// Speculative capacities: in a training loop the counts of consecutive steps differ by a few per cent, and waiting for them leaves the
// GPU idle for a host round trip (~40 us of a 1 ms step).  With the largest recent counts of the shape + 1/8 as capacities the second
// phase is queued straight behind the first; the counts are read AFTER that (the GPU is busy with the phase by then), and a view whose
// counts do not fit was left untouched by the kernels (p2_live) -- the phase is then repeated with exact sizes (p2_settle).
// false = the ring has no entry of the shape.
static bool caps_from_history(int P, int W, int H, int tiles, int V, Caps &c) {
    SpecHist hist;
    {
        std::lock_guard<std::mutex> lk(g_spec_mu);
        for (const SpecHist &e : g_spec_ring)
            if (e.R > 0 && e.W == W && e.H == H && e.P == P) {
                hist.R = e.R > hist.R ? e.R : hist.R;
                hist.longest = e.longest > hist.longest ? e.longest : hist.longest;
                hist.busy = e.busy > hist.busy ? e.busy : hist.busy;
            }
    }
    if (hist.R == 0) return false;
    const uint64_t want = (uint64_t)hist.R + hist.R / 8 + 4096;
    const uint32_t rc32 = (uint32_t)(want > 0x7FFFFF00ull ? 0x7FFFFF00ull : want), cap = tile_sort_cap();
    for (int i = 0; i < V; i++) c.R[i] = rc32;
    c.longest = hist.longest + hist.longest / 4 + 64;
    c.longest = c.longest > cap ? cap : c.longest;
    c.busy = hist.busy + hist.busy / 8 + 16;          // non-empty tiles: sizes the compositing forward's grid
    c.busy = c.busy > (uint32_t)tiles ? (uint32_t)tiles : c.busy;
    return true;
}

// A call whose speculative second phase has been launched but whose counts have not been read yet (csplat_forward_views_deferred):
// what csplat_forward_views_settle needs to finish it.  Keyed by the caller's view array.
struct PendingViews {
    bool parked = false;
    const csplat_view *key = nullptr;
    int V = 0, tk[RASTER_MAX_VIEWS];
    Caps caps;
};
constexpr int MAX_PENDING = 8;
static PendingViews g_pending[MAX_PENDING];
static std::mutex g_pending_mu;

// The tickets a call has opened.  Whatever way the call ends, the destructor gives back those it still owns: a ticket leaves the set
// only into a pending slot (park; settle takes them back with adopt) or into csplat_forward_finish, which releases its own (hand_over).
namespace {     // (its member functions stay out of the library's exports)
struct TicketSet {
    int tk[MAX_TICKETS], n = 0, handed = 0;         // tk[handed..n) are this call's to release
    TicketSet() = default;
    TicketSet(const TicketSet &) = delete;
    TicketSet &operator=(const TicketSet &) = delete;
    ~TicketSet() {
        for (int i = handed; i < n; i++) release_ticket(tk[i]);
    }
    // begin_prepare for views[0..V), up to the first refusal
    int prepare(int V, const csplat_view *v, csplat_alloc_fn alloc) {
        for (; n < V; n++)
            if (int rc = begin_prepare(v[n], alloc, &tk[n])) return rc;
        return 0;
    }
    int hand_over() { return tk[handed++]; }
    // false = no free pending slot (the set keeps its tickets)
    bool park(const csplat_view *key, const Caps &caps) {
        std::lock_guard<std::mutex> lk(g_pending_mu);
        for (PendingViews &p : g_pending)
            if (!p.parked) {
                p.parked = true; p.key = key; p.V = n; p.caps = caps;
                for (int i = 0; i < n; i++) p.tk[i] = tk[i];
                n = handed = 0;
                return true;
            }
        return false;
    }
    void adopt(const PendingViews &p) {
        for (n = 0; n < p.V; n++) tk[n] = p.tk[n];
    }
};
}  // namespace

// the checks a call passes before its second phase can be one launch per stage; false: the caller finishes view by view
static bool p2_qualifies(int V, const int *tk) {
    if (V < 1 || V > RASTER_MAX_VIEWS || dbg(CSPLAT_DEBUG_PER_VIEW_LAUNCHES)) return false;
    const FwdTicket &a = g_tickets[tk[0]];
    for (int i = 0; i < V; i++) {
        const FwdTicket &t = g_tickets[tk[i]];
        if (!t.can_bucket || t.w.P != a.w.P || t.w.W != a.w.W || t.w.H != a.w.H || t.w.P <= 0) return false;
    }
    return true;
}

// lays the chunks of every view out for `caps.R[i]` list entries and launches the five stages of the second phase on `join`, writing
// the images v[i].out_color / out_depth name NOW.  spec: the capacities are a guess, the kernels check the counts against them;
// valid != nullptr: K6's first wave leaves 1 there when every view's counts fitted the capacities, else 0 (csplat_forward_views_faith)
static int p2_launch(int V, const int *tk, csplat_view *v, hipStream_t join, const Caps &caps, int spec, uint32_t *valid) {
    const FwdTicket &a = g_tickets[tk[0]];
    const int P = a.w.P, W = a.w.W, H = a.w.H, tiles = a.tiles, nb = a.nb;
    const uint32_t Lcap = caps.longest, Bcap = caps.busy;
    P2Table tab;
    tab.valid = valid; tab.nviews = V;
    uint32_t maxR = 0;
    for (int i = 0; i < V; i++) {
        const FwdTicket &t = g_tickets[tk[i]];
        const uint32_t R = caps.R[i];
        maxR = R > maxR ? R : maxR;
        void *bbase = t.alloc(t.w.alloc_ctx, CSPLAT_CHUNK_BINNING, csplat_binning_bytes(R, W, H));
        void *tbase = t.alloc(t.w.alloc_ctx, CSPLAT_CHUNK_TEMP, csplat_temp_bytes(P, R, W, H));
        CSPLAT_REQUIRE(bbase && tbase, "allocator returned NULL");
        const BinView b = binning_view(bbase, R, tiles);
        P2View &k = tab.v[i];
        k.g = t.g; k.cam = t.cam; k.radii = t.w.radii; k.table = t.table; k.ranges = t.im.ranges;
        k.keys_u = temp_view(tbase, R).keys_u;
        k.keys_sorted = b.keys_sorted; k.ids_sorted = b.ids_sorted; k.seg_offset = b.seg_offset; k.slot_tile = b.slot_tile;
        k.ckpt = b.ckpt; k.mask16 = b.mask16; k.bbits = b.bbits; k.bmask = b.bmask; k.recA = b.recA; k.recB = b.recB; k.recC = b.recC;
        k.bg = t.w.bg; k.final_T = t.im.final_T; k.n_contrib = t.im.n_contrib; k.out_color = v[i].out_color; k.out_depth = v[i].out_depth;
        k.R = R; k.info = t.im.info; k.Lcap = Lcap; k.Bcap = Bcap; k.spec = spec;
        v[i].layout_rendered = (int)R; v[i].geom = t.gbase; v[i].binning = bbase; v[i].image = t.ibase;
    }
    {
        ProfScope ps(PROF_K3, join);
        k_emit_bucket_views<<<dim3(nb + 1, V), BUCKET_G, (size_t)tiles * 4, join>>>(P, tiles, tab);
        LAUNCH_CHECK();
    }
    {
        ProfScope ps(PROF_K4, join);
        tile_sort_views_launch(join, tiles, V, Lcap, Bcap, tab, tsort_mode(P));
        LAUNCH_CHECK();
    }
    {
        ProfScope ps(PROF_K5, join);
        const int exact = dbg(DBG_NO_ELLIPSE_STAGE) ? 0 : 1, nbm = cdiv((int64_t)maxR + 1, 256);
        if (V == 1 || V == 2 || V == 4 || V == 8)         // one view per XCD (see k_block_masks_views)
            k_block_masks_views<<<dim3((unsigned)(((int64_t)nbm * V + 7) / 8 * 8)), 256, 0, join>>>(tab, exact, V);
        else
            k_block_masks_views<<<dim3(nbm, V), 256, 0, join>>>(tab, exact, 0);
        LAUNCH_CHECK();
    }
    {
        ProfScope ps(PROF_K6, join);
        // Waves for the NON-EMPTY tiles only (Bcap of them, longest list first) + K6_EXTRA waves that paint the empty tiles' pixels: on
        // scene_1 nine tiles in ten are empty, and launching 16 waves for each of them cost ~50 us of the launch (the same launch on a
        // scene of 500 Gaussians: 51 us).  What is left is ~17 k waves with work for 8192 wave slots, 40-75 us each in the row form
        // (four survivors a step): the launch is as long as a few of those in a row on the unluckiest slot.  Hence the SURVIVOR-COLUMN
        // form by default (sixteen survivors a step: a quarter of the steps, each longer; 96 VGPRs, which no longer matters with two
        // waves per slot to place): 158 -> 137 us for four views, step 0.685 -> 0.665 ms (same box, three alternations).  Bit 15 of
        // csplat_debug_flags selects the row form.
        const int total = cdiv(tiles, 8) * 128, bg_ = cdiv((int)Bcap, 8) * 128, busy_grid = bg_ < total ? bg_ : total;
        if (!dbg(CSPLAT_DEBUG_K6_ROWS))
            k_composite_fwd_views<false><<<dim3(busy_grid + K6_EXTRA, V), 64, 0, join>>>(tiles, W, H, tab, busy_grid);
        else
            k_composite_fwd_views<true><<<dim3(busy_grid + K6_EXTRA, V), 64, 0, join>>>(tiles, W, H, tab, busy_grid);
        LAUNCH_CHECK();
    }
    return 0;
}

// The one host read of a batched call: the counts of every view, behind the speculative launch when there was one (`speculated`: its
// capacities).  They fit: accepted as launched.  They do not, or nothing was launched yet: the phase is launched with exact sizes
// (*relaunched = 1 when given) -- unless a list is too long for the in-LDS sort or a view is empty: P2_PER_VIEW, the caller goes view
// by view.  The ring learns the counts (remember) whenever they were compared with capacities, and before every exact launch.
enum P2Result { P2_DONE, P2_PER_VIEW };
static int p2_settle(int V, const int *tk, csplat_view *v, hipStream_t join, const Caps *speculated, int *relaunched, P2Result *how) {
    const csplat_view &a = g_tickets[tk[0]].w;
    *how = P2_PER_VIEW;
    uint32_t info[RASTER_MAX_VIEWS][3];
    for (int i = 0; i < V; i++)
        if (int rc = finish_read(g_tickets[tk[i]], info[i], join)) return rc;
    auto accept = [&]() {
        for (int i = 0; i < V; i++) { v[i].num_rendered = (int)info[i][0]; v[i].busy_tiles = (int)info[i][2]; }
        *how = P2_DONE;
    };
    if (speculated) {
        bool fits = true;
        for (int i = 0; i < V; i++)
            fits = fits && info[i][0] - 1u < speculated->R[i] && info[i][1] <= speculated->longest && info[i][2] <= speculated->busy;
        remember(a.P, a.W, a.H, V, info);
        if (fits) { accept(); return 0; }
    }
    const uint32_t cap = tile_sort_cap();
    Caps exact;
    exact.longest = exact.busy = 0;
    for (int i = 0; i < V; i++) {
        if (info[i][1] > cap || info[i][0] == 0) return 0;      // a list too long for the in-LDS sort, an empty view: view by view
        exact.longest = info[i][1] > exact.longest ? info[i][1] : exact.longest;
        exact.busy = info[i][2] > exact.busy ? info[i][2] : exact.busy;
        exact.R[i] = info[i][0];
    }
    remember(a.P, a.W, a.H, V, info);
    if (int rc = p2_launch(V, tk, v, join, exact, 0, nullptr)) return rc;
    if (relaunched) *relaunched = 1;
    accept();
    return 0;
}

int csplat_forward_finish(int ticket, float *out_color, float *out_depth, int *num_rendered, void **geom_out,
                          void **binning_out, void **image_out) {
    CSPLAT_REQUIRE(ticket >= 0 && ticket < MAX_TICKETS && g_tickets[ticket].used, "csplat_forward_finish: unknown ticket");
    const FwdTicket t = g_tickets[ticket];
    release_ticket(ticket);     // released whatever happens below: the slot is free before the first launch
    hipStream_t s = t.s;
    const int P = t.w.P, W = t.w.W, H = t.w.H, tiles = t.tiles, nb = t.nb;
    const Cam &cam = t.cam;
    const Geom &g = t.g;
    int2 *ranges = t.im.ranges;
    const int32_t *radii = t.w.radii;
    uint32_t host_info[3] = {0, 0, 0};   // R, longest tile list, non-empty tiles
    if (int rc = finish_read(t, host_info)) return rc;
    const uint32_t R = host_info[0];
    const uint32_t cap = tile_sort_cap();
    const bool bucketed = t.can_bucket && host_info[1] <= cap;
    *num_rendered = (int)R;
    void *bbase = t.alloc(t.w.alloc_ctx, CSPLAT_CHUNK_BINNING, csplat_binning_bytes(R, W, H));
    CSPLAT_REQUIRE(bbase, "allocator returned NULL");
    const BinView b = binning_view(bbase, R, tiles);
    if (R > 0) {
        void *tbase = t.alloc(t.w.alloc_ctx, CSPLAT_CHUNK_TEMP, csplat_temp_bytes(P, R, W, H));
        CSPLAT_REQUIRE(tbase, "allocator returned NULL");
        const TempView tmp = temp_view(tbase, R);
        if (bucketed) {
            {
                ProfScope ps(PROF_K3, s);
                k_emit_bucket<<<nb, BUCKET_G, (size_t)tiles * 4, s>>>(P, tiles, g.xy, g.depth, radii, cam, t.table, ranges, tmp.keys_u);
                LAUNCH_CHECK();
            }
            ProfScope ps(PROF_K4, s);
            tile_sort_launch(s, tiles, host_info[1], host_info[2], t.im, tmp.keys_u, b, tsort_mode(P));
            LAUNCH_CHECK();
        } else {
            // a tile list longer than the LDS sort takes: the global stable radix sort (upstream's pipeline shape)
            if (t.can_bucket) {   // (the bucket path was attempted: the P-scan has not run yet)
                ProfScope ps(PROF_K2, s);
                if (int rc = csplat_inclusive_scan_u32(s, g.tiles_touched, g.offsets, P, g.scan_tmp)) return rc;
            }
            {
                ProfScope ps(PROF_K3, s);
                k_emit_keys<<<cdiv(P, 256), 256, 0, s>>>(P, g.xy, g.depth, g.offsets, radii, cam, tmp.keys_u, tmp.ids_u);
                LAUNCH_CHECK();
            }
            const int end_bit = 32 + higher_msb((uint32_t)tiles);
            {
                ProfScope ps(PROF_K4, s);
                if (int rc = csplat_sort_pairs(s, tmp.keys_u, tmp.ids_u, b.keys_sorted, b.ids_sorted, tmp.keys_t, tmp.ids_t, R, end_bit, tmp.sort_tmp))
                    return rc;
            }
            {
                ProfScope ps(PROF_K5, s);
                HIP_TRY(hipMemsetAsync(ranges, 0, (size_t)tiles * 8, s));
                k_tile_ranges<<<cdiv(R, 256), 256, 0, s>>>(R, b.keys_sorted, ranges);
                LAUNCH_CHECK();
            }
        }
    }
    {
        ProfScope ps(PROF_K5, s);
        k_seg_plan<<<1, 1024, 0, s>>>(tiles, ranges, b.seg_offset, b.slot_tile);
        LAUNCH_CHECK();
    }
    {
        ProfScope ps(PROF_K5, s);
        k_block_masks<<<cdiv((int64_t)R + 1, 256), 256, 0, s>>>((int64_t)R, cam.gx, b.keys_sorted, b.ids_sorted, g.pack, b.mask16, b.recA, b.recB,
                                                                 b.recC, dbg(DBG_NO_ELLIPSE_STAGE) ? 0 : 1, b.bmask);
        LAUNCH_CHECK();
    }
    {
        ProfScope ps(PROF_K6, s);
        if (dbg(CSPLAT_DEBUG_K6_ROWS))       // (bit 15: the row form, four survivors a step; default: the survivor-column form, 74 -> 67 us alone)
            k_composite_fwd<true><<<cdiv(tiles, 8) * 128, 64, 0, s>>>(tiles, W, H, cam.gx, ranges, b.mask16, b.recA, b.recB, b.recC, R, t.w.bg, b.seg_offset,
                                                                      b.ckpt, t.im.final_T, t.im.n_contrib, out_color, out_depth, b.bbits, b.bmask);
        else
            k_composite_fwd<false><<<cdiv(tiles, 8) * 128, 64, 0, s>>>(tiles, W, H, cam.gx, ranges, b.mask16, b.recA, b.recB, b.recC, R, t.w.bg, b.seg_offset,
                                                                       b.ckpt, t.im.final_T, t.im.n_contrib, out_color, out_depth, b.bbits, b.bmask);
        LAUNCH_CHECK();
    }
    *geom_out = t.gbase; *binning_out = bbase; *image_out = t.ibase;
    return 0;
}

int csplat_forward(void *stream, int P, int D, int M, const float *bg, int W, int H, const float *means3D,
                   const float *shs, const float *colors_precomp, const float *opacities, const float *scales,
                   float scale_modifier, const float *rotations, const float *cov3D_precomp, const float *view,
                   const float *proj, const float *campos, float tanfovx, float tanfovy, int prefiltered,
                   csplat_alloc_fn alloc, void *alloc_ctx, float *out_color, float *out_depth, int32_t *radii,
                   int *num_rendered, void **geom_out, void **binning_out, void **image_out) {
    int ticket = -1;
    if (int rc = csplat_forward_begin(stream, P, D, M, bg, W, H, means3D, shs, colors_precomp, opacities, scales, scale_modifier,
                                      rotations, cov3D_precomp, view, proj, campos, tanfovx, tanfovy, prefiltered, alloc,
                                      alloc_ctx, radii, &ticket))
        return rc;
    return csplat_forward_finish(ticket, out_color, out_depth, num_rendered, geom_out, binning_out, image_out);
}

// The single-view K8 of `w` on `k8s`: one of k_preprocess_bwd / _depth / _cam<DEPTH> / _aa<DEPTH, CAM>, each with the SH rows staged in
// LDS (128 threads) or not (256).  depth: record slot 9 -> dL/dmean3D (csplat_view.dL_ddepth); cam_slab != NULL: the camera-gradient
// form, one slab row per workgroup, summed by k_cam_sum (*cam_rows = the number of rows); an antialiased view takes the AA variant of
// whichever form the call takes.
static int launch_k8(hipStream_t k8s, const csplat_view &w, bool depth, float *cam_slab, int *cam_rows) {
    ProfScope ps(cam_slab ? PROF_K8_CAM : depth ? PROF_K8_DEPTH : PROF_K8, k8s);
    const bool stage = w.shs != nullptr && w.dL_dsh != nullptr && w.M == 16 && (((uintptr_t)w.shs | (uintptr_t)w.dL_dsh) & 15u) == 0;
    CSPLAT_REQUIRE(stage || !(w.accmask & CSPLAT_ACC_SH), "accumulating dL_dsh needs M == 16 and 16-byte aligned buffers");
    Cam cam;
    make_cam(cam, w);
    const Geom g = geom_view(w.geom, w.P);
    auto form = [&](auto staged) {
        constexpr bool STAGE = decltype(staged)::value;
        constexpr int NT = STAGE ? 128 : 256;
        const int grid = cdiv(w.P, NT);
        auto go = [&](auto kernel, auto... extra) {
            kernel<<<grid, NT, 0, k8s>>>(w.P, w.D, w.M, w.means3D, w.shs, w.scales, w.scale_modifier, w.rotations, w.cov3D_precomp != nullptr, cam,
                                         g, w.radii, (const float *)w.scratch, w.dL_dmean2D, w.dL_dconic, w.dL_dopacity, w.dL_dcolor,
                                         w.dL_dmean3D, w.dL_dcov3D, w.dL_dsh, w.dL_dscale, w.dL_drot, w.accmask, extra...);
        };
        if (aa_of(w)) {
            if (cam_slab && depth) go(k_preprocess_bwd_aa<STAGE, NT, true, true>, cam_slab, w.opacities);
            else if (cam_slab) go(k_preprocess_bwd_aa<STAGE, NT, false, true>, cam_slab, w.opacities);
            else if (depth) go(k_preprocess_bwd_aa<STAGE, NT, true, false>, cam_slab, w.opacities);
            else go(k_preprocess_bwd_aa<STAGE, NT, false, false>, cam_slab, w.opacities);
        } else if (cam_slab) {
            if (depth) go(k_preprocess_bwd_cam<STAGE, NT, true>, cam_slab);
            else go(k_preprocess_bwd_cam<STAGE, NT, false>, cam_slab);
        } else if (depth) {
            go(k_preprocess_bwd_depth<STAGE, NT>);
        } else {
            go(k_preprocess_bwd<STAGE, NT>);
        }
        if (cam_slab && cam_rows) *cam_rows = grid;
    };
    if (stage) form(std::true_type{});
    else form(std::false_type{});
    LAUNCH_CHECK();
    return 0;
}

// One view's backward: K7 on `s` (with_k7; false = the caller launched K7 of all views as one batch), K8 on `k8s` (with_k8; after an
// event wait when the streams differ; false = the caller runs one K8 over all views afterwards).  depth_k8 / cam_k8: K8's form (launch_k8).
// A view without Gaussians has nothing to do, whatever else it lacks.  accmask see k_preprocess_bwd.
static int backward_one(const csplat_view &w, ScratchPath path, hipStream_t s, hipStream_t k8s, bool with_k7, bool with_k8, bool depth_k8,
                        bool cam_k8, int *cam_rows) {
    if (w.P <= 0) return 0;
    CSPLAT_REQUIRE(w.geom && w.binning && w.image && w.out_color, "csplat_backward: missing saved state");
    CSPLAT_REQUIRE(w.dL_dmean2D && w.dL_dconic && w.dL_dopacity && w.dL_dcolor && w.dL_dmean3D && w.dL_dcov3D, "missing gradient outputs");
    CSPLAT_REQUIRE(w.scratch != nullptr, "csplat_backward: scratch (csplat_backward_scratch_bytes) missing");
    const int P = w.P, R = layout_R(w), tiles = tiles_of(w.W, w.H);
    const ScratchView sv = (with_k7 || cam_k8) ? scratch_view(w, path) : ScratchView{};
    if (with_k7) {
        B2View k;
        DetView e;
        fill_k7_view(w, sv, tiles, k, e);
        if (sv.det) HIP_TRY(hipMemsetAsync(sv.det, 0, sv.det_bytes, s));
        else if (!(w.accmask & CSPLAT_SCRATCH_ZEROED)) HIP_TRY(hipMemsetAsync(sv.acc, 0, (size_t)P * ACC_STRIDE * 4, s));
        ProfScope ps(PROF_K7, s);
        if (R > 0) {
            const unsigned grid = (unsigned)cdiv(max_slots(R, tiles), 8) * 32u;
            auto go = [&](auto kernel) {
                kernel<<<grid, 256, 0, s>>>(tiles, w.W, w.H, cdiv(w.W, CSPLAT_TILE), k.ranges, k.ids_sorted, k.bbits, k.recA, k.recB, k.recC, k.R,
                                            k.seg_offset, k.slot_tile, k.ckpt, k.final_T, k.n_contrib, k.out_color, k.dL_dpix, k.acc, k.det);
            };
            if (sv.det) go(k_composite_bwd_rows<true>);
            else go(k_composite_bwd_rows<false>);
            LAUNCH_CHECK();
        }
        if (sv.det) {   // fixed-order sum of every Gaussian's instance records (writes all of acc)
            k_det_reduce<<<cdiv(P, 256), 256, 0, s>>>(P, e.cam, e.xy, e.depth, e.radii, e.ranges, e.keys_sorted, e.ids_sorted, e.det, e.acc);
            LAUNCH_CHECK();
        }
    }
    if (!with_k8) return 0;
    if (with_k7 && k8s != s) {
        hipEvent_t ev = pooled_event();
        CSPLAT_REQUIRE(ev != nullptr, "csplat_backward_views: no event");
        HIP_TRY(hipEventRecord(ev, s));
        HIP_TRY(hipStreamWaitEvent(k8s, ev, 0));
    }
    return launch_k8(k8s, w, depth_k8, cam_k8 ? sv.cam_slab : nullptr, cam_rows);
}

// ---- batched entry points: V independent views, one stream each, fenced against `join_stream`
static int fence_in(int V, const csplat_view *v, hipStream_t join) {
    hipEvent_t ev = pooled_event();
    CSPLAT_REQUIRE(ev != nullptr, "csplat_*_views: no event");
    HIP_TRY(hipEventRecord(ev, join));
    for (int i = 0; i < V; i++) {
        bool seen = (hipStream_t)v[i].stream == join;
        for (int j = 0; j < i && !seen; j++) seen = v[j].stream == v[i].stream;
        if (!seen) HIP_TRY(hipStreamWaitEvent((hipStream_t)v[i].stream, ev, 0));
    }
    return 0;
}
static int fence_out(int V, const csplat_view *v, hipStream_t join) {
    for (int i = 0; i < V; i++) {
        bool seen = (hipStream_t)v[i].stream == join;
        for (int j = 0; j < i && !seen; j++) seen = v[j].stream == v[i].stream;
        if (seen) continue;
        hipEvent_t ev = pooled_event();
        CSPLAT_REQUIRE(ev != nullptr, "csplat_*_views: no event");
        HIP_TRY(hipEventRecord(ev, (hipStream_t)v[i].stream));
        HIP_TRY(hipStreamWaitEvent(join, ev, 0));
    }
    return 0;
}

// the per-view tail of a forward call: every ticket of the set is finished (csplat_forward_finish releases its own) or, after an
// error, left to the set to release
static int finish_views_one_by_one(int V, csplat_view *v, TicketSet &ts, hipStream_t join, bool fenced, int rc) {
    for (int i = 0; i < ts.n && rc == 0; i++) {
        csplat_view &w = v[i];
        rc = csplat_forward_finish(ts.hand_over(), w.out_color, w.out_depth, &w.num_rendered, &w.geom, &w.binning, &w.image);
        w.layout_rendered = w.num_rendered;
    }
    // (also on the error path: the side streams may hold work on torch-owned chunks that the caller frees on its own stream as
    // soon as the error propagates)
    if (fenced) { const int r2 = fence_out(V, v, join); if (rc == 0) rc = r2; }
    return rc;
}

// csplat_forward_views (pending == nullptr) and csplat_forward_views_deferred: prepare; then, for views that share their Gaussians, K1
// of all views and the second phase -- speculate and settle, or settle alone (no history of the shape, speculation switched off by
// csplat_debug_flags bit 10); the deferred call parks itself behind the speculative launch instead of settling.  Everything else, and
// a call whose counts p2_settle hands back, goes view by view on the views' own streams.
static int forward_views_impl(int V, csplat_view *v, csplat_alloc_fn alloc, void *join_stream, int *pending) {
    CSPLAT_REQUIRE(V >= 0 && V <= MAX_TICKETS && (V == 0 || v != nullptr), "csplat_forward_views: bad view count");
    hipStream_t join = (hipStream_t)join_stream;
    TicketSet ts;
    if (pending) *pending = 0;
    int rc = ts.prepare(V, v, alloc);
    bool fenced = false;
    if (rc == 0 && begin_views_compatible(V, ts.tk)) {
        // first phase of all views in four launches on the join stream ...
        rc = begin_launch_views(V, ts.tk, join);
        // ... and, when every tile list fits the in-LDS sort, the second phase in five more, also on the join stream: no
        // side stream is involved at all
        P2Result how = P2_PER_VIEW;
        if (rc == 0 && p2_qualifies(V, ts.tk)) {
            const FwdTicket &a = g_tickets[ts.tk[0]];
            Caps caps;
            const bool spec = caps_from_history(a.w.P, a.w.W, a.w.H, a.tiles, V, caps) && !dbg(CSPLAT_DEBUG_NO_SPECULATION);
            if (spec) rc = p2_launch(V, ts.tk, v, join, caps, 1, nullptr);
            if (rc == 0 && spec && pending) {   // deferred: the caller reads the counts later (settle), the GPU has its work
                for (int i = 0; i < V; i++) { v[i].num_rendered = -1; v[i].busy_tiles = 0; }
                if (ts.park(v, caps)) {
                    *pending = 1;
                    return 0;
                }                               // (no free slot: settle right here)
            }
            if (rc == 0) rc = p2_settle(V, ts.tk, v, join, spec ? &caps : nullptr, nullptr, &how);
        }
        if (rc || how == P2_DONE) return rc;
        rc = fence_in(V, v, join);     // otherwise the views' streams branch off here
        fenced = rc == 0;
    } else if (rc == 0) {
        rc = fence_in(V, v, join);
        fenced = rc == 0;
        for (int i = 0; i < V && rc == 0; i++) rc = begin_launch(g_tickets[ts.tk[i]]);
    }
    return finish_views_one_by_one(V, v, ts, join, fenced, rc);
}

// ABI 9: the feature / alpha images of a finished forward (csplat_view.out_features / out_alpha), on the join stream behind every view's
// K6.  Nothing is launched when no view asks for them.  One launch per group of views (view_group): a call of up to 8 views is one launch.
static bool feat_out_wanted(const csplat_view &w) { return w.out_features || w.out_alpha; }
// The per-view tables of the extended paths hold RASTER_MAX_VIEWS views: a call of more views runs in ceil(V / 8) groups of as equal a size as
// possible, one after the other on the join stream, in view order.  Group g is views [lo, hi); a call of up to 8 views is one group.
static int view_groups(int V) { return V > RASTER_MAX_VIEWS ? cdiv(V, RASTER_MAX_VIEWS) : 1; }
static_assert(RASTER_MAX_VIEWS == 8, "csplat.h and the CSPLAT_REQUIRE texts of the grouped paths promise groups of at most 8 views");
static void view_group(int V, int g, int *lo, int *hi) {
    const int ng = view_groups(V);
    *lo = (int)((int64_t)V * g / ng);
    *hi = (int)((int64_t)V * (g + 1) / ng);
}
static int feature_forward_group(int V, csplat_view *v, hipStream_t join) {
    bool any = false;
    for (int i = 0; i < V; i++) any = any || feat_out_wanted(v[i]);
    if (!any) return 0;
    CSPLAT_REQUIRE(V <= RASTER_MAX_VIEWS, "csplat_forward_views: feature / alpha images are rendered for at most 8 views per launch");
    FeatFwdTable t;
    memset(&t, 0, sizeof(t));
    int maxtiles = 0;
    for (int i = 0; i < V; i++) {
        const csplat_view &w = v[i];
        // (a view without Gaussians may leave features NULL whatever its n_features: an empty [0][F] array has no storage)
        CSPLAT_REQUIRE(w.n_features >= 0 && w.n_features <= CSPLAT_MAX_FEATURES &&
                       ((w.n_features == 0) == (w.features == nullptr) || (w.P <= 0 && w.features == nullptr)),
                       "csplat_forward_views: n_features must be 0..6, with features set exactly when it is not 0");
        CSPLAT_REQUIRE(!w.out_features || w.n_features > 0, "csplat_forward_views: out_features without features");
        FeatFwdView &f = t.v[i];
        const int gx = cdiv(w.W, CSPLAT_TILE), tiles = tiles_of(w.W, w.H);
        f.W = w.W; f.H = w.H; f.gx = gx; f.nf = w.n_features; f.features = w.features;
        f.out_features = w.out_features; f.out_alpha = w.out_alpha;
        if (!feat_out_wanted(w)) continue;
        maxtiles = tiles > maxtiles ? tiles : maxtiles;
        if (w.P <= 0 || w.num_rendered <= 0) continue;       // (no list entry: feat = 0, alpha = 0)
        CSPLAT_REQUIRE(w.image && w.binning, "csplat_forward_views: missing chunks");
        const ImageView im = image_view(w.image, w.W, w.H);
        fill_list_view(binning_view(w.binning, layout_R(w), tiles), im, f);
        f.final_T = im.final_T;
        f.tiles = tiles;
    }
    if (maxtiles == 0) return 0;
    ProfScope ps(PROF_K6_FEAT, join);
    k_feature_fwd_views<<<dim3((unsigned)maxtiles, V), 256, 0, join>>>(t);
    LAUNCH_CHECK();
    return 0;
}
static int feature_forward(int V, csplat_view *v, hipStream_t join) {
    for (int g = 0, ng = view_groups(V); g < ng; g++) {
        int lo, hi;
        view_group(V, g, &lo, &hi);
        if (int rc = feature_forward_group(hi - lo, v + lo, join)) return rc;
    }
    return 0;
}

int csplat_forward_views(int V, csplat_view *v, csplat_alloc_fn alloc, void *join_stream) {
    const int rc = forward_views_impl(V, v, alloc, join_stream, nullptr);
    return rc ? rc : feature_forward(V, v, (hipStream_t)join_stream);
}

// Gaussian visibility and the top-contributor map of finished forward views: the per-entry records (max, sum, count) of the walk, back to
// back in the scratch, each array 256-byte aligned.
size_t csplat_visibility_scratch_bytes(int P, int64_t R, int W, int H) {
    (void)P; (void)W; (void)H;
    const size_t n = R > 0 ? (size_t)R : 0;
    return 3 * align256(n * 4 + 4);
}
static int visibility_views_group(int V, const csplat_view *v, const csplat_visibility *outs, hipStream_t join) {
    VisTable t;
    VisRedTable r;
    memset(&t, 0, sizeof(t));
    memset(&r, 0, sizeof(r));
    int maxtiles = 0, maxP = 0;
    for (int i = 0; i < V; i++) {
        const csplat_view &w = v[i];
        const csplat_visibility &o = outs[i];
        const bool per_g = o.weight_max || o.weight_sum || o.pixel_count;
        if (!per_g && !o.top_id) continue;
        CSPLAT_REQUIRE(w.num_rendered >= 0, "csplat_visibility_views: the view's forward is still pending (settle it first)");
        CSPLAT_REQUIRE(w.valid == nullptr, "csplat_visibility_views: views launched on faith have no visibility pass");
        CSPLAT_REQUIRE(w.P >= 0 && w.W > 0 && w.H > 0, "csplat_visibility_views: bad view size");
        const int gx = cdiv(w.W, CSPLAT_TILE), tiles = tiles_of(w.W, w.H);
        const bool lists = w.P > 0 && w.num_rendered > 0;
        CSPLAT_REQUIRE(!lists || (w.geom && w.binning && w.image), "csplat_visibility_views: missing chunks");
        CSPLAT_REQUIRE(!lists || !per_g || o.scratch, "csplat_visibility_views: per-Gaussian outputs need the scratch");
        CSPLAT_REQUIRE(!per_g || w.P == 0 || w.radii, "csplat_visibility_views: per-Gaussian outputs need the view's radii");
        VisView &f = t.v[i];
        f.W = w.W; f.H = w.H; f.gx = gx; f.top_id = o.top_id;
        VisRedView &g = r.v[i];
        g.P = per_g ? w.P : 0;
        g.weight_max = o.weight_max; g.weight_sum = o.weight_sum; g.pixel_count = o.pixel_count; g.radii = w.radii;
        maxtiles = tiles > maxtiles ? tiles : maxtiles;      // (the walk also writes top_id = -1 of a view without list entries)
        maxP = g.P > maxP ? g.P : maxP;
        if (!lists) continue;
        const BinView b = binning_view(w.binning, layout_R(w), tiles);
        fill_list_view(b, image_view(w.image, w.W, w.H), f);
        f.tiles = tiles;
        if (per_g) {
            const size_t a = align256((size_t)layout_R(w) * 4 + 4);
            f.rec_max = (float *)o.scratch; f.rec_sum = (float *)((char *)o.scratch + a); f.rec_cnt = (int32_t *)((char *)o.scratch + 2 * a);
            make_cam(g.cam, w);
            const Geom gm = geom_view(w.geom, w.P);
            g.xy = gm.xy; g.depth = gm.depth; g.ranges = f.ranges; g.keys_sorted = b.keys_sorted; g.ids_sorted = f.ids_sorted;
            g.rec_max = f.rec_max; g.rec_sum = f.rec_sum; g.rec_cnt = f.rec_cnt; g.tiles = tiles;
        }
    }
    if (maxtiles == 0) return 0;
    ProfScope ps(PROF_VISIBILITY, join);
    k_visibility_walk_views<<<dim3((unsigned)maxtiles, V), 256, 0, join>>>(t);
    LAUNCH_CHECK();
    if (maxP > 0) {
        k_visibility_reduce_views<<<dim3((unsigned)cdiv(maxP, 16), V), 256, 0, join>>>(r);
        LAUNCH_CHECK();
    }
    return 0;
}
int csplat_visibility_views(int V, const csplat_view *v, const csplat_visibility *outs, void *join_stream) {
    CSPLAT_REQUIRE(V >= 1 && V <= MAX_TICKETS && v != nullptr && outs != nullptr, "csplat_visibility_views: 1 to 64 views and their outputs");
    for (int g = 0, ng = view_groups(V); g < ng; g++) {      // (a group of at most 8 views per walk / reduce pair)
        int lo, hi;
        view_group(V, g, &lo, &hi);
        if (int rc = visibility_views_group(hi - lo, v + lo, outs + lo, (hipStream_t)join_stream)) return rc;
    }
    return 0;
}

// csplat_forward_views WITHOUT any host read: both phases are launched with the caller's capacities (caps[0] list entries per view,
// caps[1] longest tile list, caps[2] non-empty tiles) and *valid (device) receives 1 when every view's counts fitted them, else 0 -- in
// which case the second phase left the views untouched and csplat_backward_views (views[i].valid = valid) does nothing either.  Nothing
// here waits for the GPU or reads from it: the call can be recorded into a hipGraph (stream capture) and replayed.  The views must
// qualify for the one-launch-per-stage path (2..8 views sharing P, SH, opacities, scales and the image size), else an error.
int csplat_forward_views_faith(int V, csplat_view *v, csplat_alloc_fn alloc, void *join_stream, const uint32_t *caps, uint32_t *valid) {
    CSPLAT_REQUIRE(V >= 2 && V <= RASTER_MAX_VIEWS && v != nullptr && caps != nullptr && valid != nullptr, "csplat_forward_views_faith: bad arguments");
    for (int i = 0; i < V; i++)
        CSPLAT_REQUIRE(!feat_out_wanted(v[i]), "csplat_forward_views_faith: views launched on faith render no feature or alpha image");
    CSPLAT_REQUIRE(caps[0] > 0 && caps[0] <= 0x7FFFFF00u && caps[1] > 0 && caps[1] <= tile_sort_cap() && caps[2] > 0,
                   "csplat_forward_views_faith: capacities out of range");
    hipStream_t join = (hipStream_t)join_stream;
    TicketSet ts;
    if (int rc = ts.prepare(V, v, alloc)) return rc;
    CSPLAT_REQUIRE(begin_views_compatible(V, ts.tk), "csplat_forward_views_faith: the views do not qualify for the one-launch-per-stage path");
    if (int rc = begin_launch_views(V, ts.tk, join)) return rc;
    Caps c;
    for (int i = 0; i < V; i++) c.R[i] = caps[0];
    const uint32_t tiles = (uint32_t)g_tickets[ts.tk[0]].tiles;
    c.longest = caps[1];
    c.busy = caps[2] > tiles ? tiles : caps[2];
    if (int rc = p2_launch(V, ts.tk, v, join, c, 1, valid)) return rc;
    for (int i = 0; i < V; i++) { v[i].num_rendered = (int)caps[0]; v[i].busy_tiles = 0; v[i].valid = valid; }
    return 0;
}
// byte offset, inside the IMAGE chunk, of the three counts a view's first phase leaves (u32: tile instances, longest tile list, non-empty
// tiles) -- what a caller that launched on faith reads, at a time of its choosing, to size the next launch
size_t csplat_image_info_offset(int W, int H) { size_t off[I_NFIELDS]; image_offsets(W, H, off); return off[I_INFO]; }

// csplat_forward_views with the one host read DEFERRED.  When the second phase can be launched speculatively (capacities from the
// previous call of the same shape) the call returns right behind that launch with *pending = 1: views[i].layout_rendered is the capacity,
// views[i].num_rendered is -1, and the caller does whatever host work it has (the GPU is busy with K1..K6) before it calls
// csplat_forward_views_settle with the SAME array.  *pending = 0: the call was complete (first call of a shape, views that do not qualify).
int csplat_forward_views_deferred(int V, csplat_view *v, csplat_alloc_fn alloc, void *join_stream, int *pending) {
    CSPLAT_REQUIRE(pending != nullptr, "csplat_forward_views_deferred: pending missing");
    const int rc = forward_views_impl(V, v, alloc, join_stream, pending);
    return (rc || *pending) ? rc : feature_forward(V, v, (hipStream_t)join_stream);      // (pending: settle renders them)
}

// Reads the counts of a pending call.  They fit the capacities: num_rendered is filled in, nothing else changes (*relaunched = 0).
// They do not: the second phase is repeated with exact sizes -- new BINNING chunks through the allocator of the call, layout_rendered /
// binning updated -- and *relaunched = 1: whatever the caller derived from layout_rendered must be rebuilt.
static int forward_views_settle_impl(int V, csplat_view *v, void *join_stream, int *relaunched);
int csplat_forward_views_settle(int V, csplat_view *v, void *join_stream, int *relaunched) {
    const int rc = forward_views_settle_impl(V, v, join_stream, relaunched);
    return rc ? rc : feature_forward(V, v, (hipStream_t)join_stream);
}
static int forward_views_settle_impl(int V, csplat_view *v, void *join_stream, int *relaunched) {
    CSPLAT_REQUIRE(v != nullptr && relaunched != nullptr, "csplat_forward_views_settle: bad arguments");
    *relaunched = 0;
    PendingViews pend;
    {
        std::lock_guard<std::mutex> lk(g_pending_mu);
        int slot = -1;
        for (int i = 0; i < MAX_PENDING && slot < 0; i++)
            if (g_pending[i].parked && g_pending[i].key == v && g_pending[i].V == V) slot = i;
        CSPLAT_REQUIRE(slot >= 0, "csplat_forward_views_settle: no pending call for this view array");
        pend = g_pending[slot];
        g_pending[slot].parked = false;
    }
    hipStream_t join = (hipStream_t)join_stream;
    TicketSet ts;
    ts.adopt(pend);
    P2Result how;
    int rc = p2_settle(V, ts.tk, v, join, &pend.caps, relaunched, &how);
    if (rc || how == P2_DONE) return rc;
    // the exact counts do not qualify for the batched phase (a list too long for the in-LDS sort, an empty view): view by view
    *relaunched = 1;
    rc = fence_in(V, v, join);
    return finish_views_one_by_one(V, v, ts, join, rc == 0, rc);
}

// Can ONE K8 serve all views?  Same Gaussians (P, D, M, scale modifier, SH and scale tensors), SH staging applicable, and every
// gradient output either the SAME buffer in all views (then views after the first must have been asked to add into it) or
// a DIFFERENT buffer in every view.  Fills the table and returns true; anything else keeps the per-view launches.
static bool k8_views_table(int V, const csplat_view *v, K8Table &tab) {
    if (V < 2 || V > RASTER_MAX_VIEWS || dbg(CSPLAT_DEBUG_PER_VIEW_K8)) return false;
    const csplat_view &a = v[0];
    if (a.P <= 0 || a.cov3D_precomp || !a.shs || !a.dL_dsh || a.M != 16 || !a.scales || !a.rotations || !a.dL_dscale || !a.dL_drot ||
        ((((uintptr_t)a.shs | (uintptr_t)a.dL_dsh) & 15u) != 0))
        return false;
    for (int i = 1; i < V; i++) {
        const csplat_view &w = v[i];
        if (w.P != a.P || w.D != a.D || w.M != a.M || w.scale_modifier != a.scale_modifier || w.shs != a.shs || w.dL_dsh != a.dL_dsh ||
            w.scales != a.scales || w.cov3D_precomp || !w.rotations || !w.dL_dscale || !w.dL_drot || !(w.accmask & CSPLAT_ACC_SH))
            return false;
        if (aa_of(w) != aa_of(a) || (aa_of(a) && w.opacities != a.opacities)) return false;     // (the AA K8 reads ONE opacity tensor)
    }
    if (aa_of(a) && !a.opacities) return false;
    unsigned sharedmask = 0;
    auto classify = [&](auto get, unsigned bit) {      // -> false when the buffers are neither all equal nor all different
        bool all_same = true, all_diff = true;
        for (int i = 0; i < V; i++)
            for (int j = i + 1; j < V; j++) {
                if (get(v[i]) == get(v[j])) all_diff = false; else all_same = false;
            }
        if (all_same) {
            for (int i = 1; i < V; i++)
                if (bit && !(v[i].accmask & bit)) return false;
            sharedmask |= bit;
            return true;
        }
        return all_diff;
    };
    if (!classify([](const csplat_view &w) { return (const void *)w.dL_dopacity; }, CSPLAT_ACC_OPACITY)) return false;
    if (!classify([](const csplat_view &w) { return (const void *)w.dL_dcolor; }, CSPLAT_ACC_COLOR)) return false;
    if (!classify([](const csplat_view &w) { return (const void *)w.dL_dmean3D; }, CSPLAT_ACC_MEAN3D)) return false;
    if (!classify([](const csplat_view &w) { return (const void *)w.dL_dcov3D; }, CSPLAT_ACC_COV3D)) return false;
    if (!classify([](const csplat_view &w) { return (const void *)w.dL_dscale; }, CSPLAT_ACC_SCALE)) return false;
    if (!classify([](const csplat_view &w) { return (const void *)w.dL_drot; }, CSPLAT_ACC_ROT)) return false;
    for (int i = 0; i < V; i++)      // mean2D / conic are per-view by construction
        for (int j = i + 1; j < V; j++)
            if (v[i].dL_dmean2D == v[j].dL_dmean2D || v[i].dL_dconic == v[j].dL_dconic || v[i].scratch == v[j].scratch) return false;
    tab.n = V;
    tab.sharedmask = sharedmask;
    tab.unread = CSPLAT_K8_OUTPUTS_UNREAD;
    for (int i = 0; i < V; i++) tab.unread &= v[i].accmask;
    tab.valid = v[0].valid;
    for (int i = 0; i < V; i++) {
        const csplat_view &w = v[i];
        if (!w.geom || !w.scratch || !w.dL_dmean2D || !w.dL_dconic || !w.dL_dopacity || !w.dL_dcolor || !w.dL_dmean3D || !w.dL_dcov3D ||
            !w.means3D || !w.radii)
            return false;
        K8View &k = tab.v[i];
        make_cam(k.cam, w);
        k.g = geom_view(w.geom, w.P);
        k.radii = w.radii; k.acc = (const float *)w.scratch; k.means3D = w.means3D; k.rotations = w.rotations;
        k.dL_dmean2D = w.dL_dmean2D; k.dL_dconic = w.dL_dconic; k.dL_dopacity = w.dL_dopacity; k.dL_dcolor = w.dL_dcolor;
        k.dL_dmean3D = w.dL_dmean3D; k.dL_dcov3D = w.dL_dcov3D; k.dL_dscale = w.dL_dscale; k.dL_drot = w.dL_drot;
        k.accmask = w.accmask;
    }
    return true;
}

// ---- the camera-gradient path (ABI 8: csplat_view.dL_dview / dL_dproj / dL_dcampos / dL_dbg).  The compositing backward is the call's
// own (default or depth); only K8 changes, to its CAM variant (when a view / projection / centre gradient is asked for), and two small
// launches follow on the join stream, behind every view's K8: k_bg_partials (when a background gradient is asked for) and k_cam_sum.
static bool cam_k8_wanted(const csplat_view &w) { return w.dL_dview || w.dL_dproj || w.dL_dcampos; }
static int cam_tail(int V, const csplat_view *v, ScratchPath path, hipStream_t join, const int *rows) {
    BgTable bt;
    CamSumTable ct;
    bool any_bg = false;
    for (int i = 0; i < V; i++) {
        const csplat_view &w = v[i];
        const ScratchView sv = scratch_view(w, path);
        BgView &b = bt.v[i];
        b.slab = nullptr; b.final_T = nullptr; b.dL_dpix = w.dL_dpix; b.npix = w.W * w.H;
        if (w.dL_dbg && w.dL_dpix && w.scratch) {
            b.final_T = w.image ? image_view(w.image, w.W, w.H).final_T : nullptr;
            b.slab = sv.bg_slab;
            any_bg = true;
        }
        CamSumView &c = ct.v[i];
        c.slab = sv.cam_slab; c.rows = w.scratch ? rows[i] : 0;
        c.bg_slab = b.slab; c.bg_rows = b.slab ? BG_BLOCKS : 0;
        c.dL_dview = w.dL_dview; c.dL_dproj = w.dL_dproj; c.dL_dcampos = w.dL_dcampos; c.dL_dbg = w.dL_dbg;
    }
    ProfScope ps(PROF_CAM_SUM, join);
    if (any_bg) {
        k_bg_partials<<<dim3(BG_BLOCKS, V), 256, 0, join>>>(bt);
        LAUNCH_CHECK();
    }
    k_cam_sum<<<dim3(1, V), 256, 0, join>>>(ct);
    LAUNCH_CHECK();
    return 0;
}

// The batched K8 (k8_views_table filled `tab`) on the join stream: k_preprocess_bwd_views / _depth / _cam<DEPTH> / _aa<DEPTH, CAM>.  depth:
// the call takes the depth / feature path; cam_k8: the camera form, one slab row per workgroup and view (cam_rows[i] = their number), whole
// calls only; every other form runs the workgroups of slice `slice` of `nslices`.
static int launch_k8_views(int V, const csplat_view *v, ScratchPath path, const K8Table &tab, bool depth, bool cam_k8, int slice, int nslices,
                           hipStream_t join, int *cam_rows) {
    ProfScope ps(cam_k8 ? PROF_K8_CAM : depth ? PROF_K8_DEPTH : PROF_K8, join);
    const csplat_view &a = v[0];
    const int nb = cdiv(a.P, 32);
    const int b_lo = cam_k8 ? 0 : (int)((int64_t)nb * slice / nslices), b_hi = cam_k8 ? nb : (int)((int64_t)nb * (slice + 1) / nslices);
    CamSlabs sl{};       // (stays empty without cam_k8: the antialiased kernel takes the argument on every path)
    for (int i = 0; i < V && cam_k8; i++) { sl.p[i] = scratch_view(v[i], path).cam_slab; cam_rows[i] = nb; }
    if (b_hi <= b_lo) return 0;
    auto go = [&](auto kernel, auto... extra) {
        kernel<<<b_hi - b_lo, 128, 0, join>>>(a.P, a.D, a.M, a.shs, a.scales, a.scale_modifier, 0, a.dL_dsh, tab, b_lo, extra...);
    };
    if (aa_of(a)) {
        if (depth && cam_k8) go(k_preprocess_bwd_views_aa<128, 4, true, true>, sl, a.opacities);
        else if (depth) go(k_preprocess_bwd_views_aa<128, 4, true, false>, sl, a.opacities);
        else if (cam_k8) go(k_preprocess_bwd_views_aa<128, 4, false, true>, sl, a.opacities);
        else go(k_preprocess_bwd_views_aa<128, 4, false, false>, sl, a.opacities);
    } else if (cam_k8) {
        if (depth) go(k_preprocess_bwd_views_cam<128, 4, true>, sl);
        else go(k_preprocess_bwd_views_cam<128, 4, false>, sl);
    } else if (depth) {
        go(k_preprocess_bwd_views_depth<128, 4>);
    } else {
        // (the flagship form: with every view's CSPLAT_K8_OUTPUTS_UNREAD the three outputs' running sums leave the registers as well)
        if (tab.unread && per_gaussian_stamps(a.P)) go(k_preprocess_bwd_views_stamps<128, 4>, per_gaussian_stamps(a.P) + (size_t)cdiv(a.P, 64) * 8);
        else if (tab.unread) go(k_preprocess_bwd_views<128, 4, true>);
        else go(k_preprocess_bwd_views<128, 4, false>);
    }
    LAUNCH_CHECK();
    return 0;
}

// What the launches of a group of views depend on.  backward_views_impl sets, once per call, which gradients the CALL takes (cam: camera /
// background at all, cam_k8: K8 in its camera form, feat: feature / alpha) and the scratch layout that follows (path); plan_group sets,
// once per group, the rest: the parts wanted; `shared` = some view adds into another view's buffers, so every K8 runs on the join stream,
// in view order; one_k8 = ONE K8 serves all views (tab).
struct GroupPlan {
    bool want_k7, want_k8, whole, shared, one_k8, det_mode, cam, cam_k8, feat;
    ScratchPath path;
    K8Table tab;
};
static void plan_group(int V, const csplat_view *v, unsigned parts, int nslices, GroupPlan &g) {
    g.want_k7 = (parts & 1u) != 0; g.want_k8 = (parts & 2u) != 0; g.whole = parts == 3u && nslices == 1;
    g.shared = false;
    for (int i = 0; i < V; i++) g.shared |= (v[i].accmask & ~(unsigned)(CSPLAT_SCRATCH_ZEROED | CSPLAT_K8_OUTPUTS_UNREAD)) != 0u;
    g.one_k8 = g.shared && k8_views_table(V, v, g.tab);
    g.det_mode = dbg(CSPLAT_DEBUG_BIT_REPRODUCIBLE);
}
// the fixed-order sum of every Gaussian's (entry, block) records (bit-reproducible mode): one launch of `kernel` per view, in view order
static int det_reduce_each(int V, const csplat_view *v, const DetTable &dt, void (*kernel)(int, DetTable), hipStream_t join) {
    for (int i = 0; i < V; i++) {
        if (v[i].P <= 0) continue;
        DetTable one;
        one.valid = nullptr;
        one.v[0] = dt.v[i];
        kernel<<<dim3((unsigned)cdiv(v[i].P, 256), 1), 256, 0, join>>>(v[i].P, one);
        LAUNCH_CHECK();
    }
    return 0;
}

static bool feat_wanted(const csplat_view &w) { return w.dL_dfeatures || w.dL_dalpha; }
// The depth-gradient path (some view has dL_ddepth) and the feature path (g.feat): every stage runs on the join stream -- clearing, the
// prepass of depth / feature partials, the depth (feature) K7 of all views in one launch (views without a depth gradient take it with zero
// depth terms), the depth K8.  earlier[0 .. n_earlier): the views of the call's earlier groups, whose dL_dfeat_in this group adds to.
static int backward_views_depth(int V, csplat_view *v, hipStream_t join, GroupPlan &g, int slice, int nslices, const csplat_view *earlier,
                                int n_earlier) {
    CSPLAT_REQUIRE(V <= RASTER_MAX_VIEWS, "csplat_backward_views: a depth, feature or alpha gradient is taken for at most 8 views per group");
    CSPLAT_REQUIRE(!v[0].valid, "csplat_backward_views: views launched on faith take no depth, feature or alpha gradient");
    CSPLAT_REQUIRE(!g.feat || g.whole, "csplat_backward_views_parts: feature / alpha gradients are taken by the whole call only");
    CSPLAT_REQUIRE(g.whole || g.one_k8, "csplat_backward_views_parts: only the one-launch-per-stage path can be cut into parts");
    const bool feat = g.feat, det_mode = g.det_mode;
    if (g.want_k7) {
        DepthTable dtab;
        FeatTable ftab;
        ftab.n = V;
        bool any_fgrad = false, any_depth = false;
        DetTable dt;
        dt.valid = nullptr;
        int64_t slots = 0;
        int Pmax = 0;
        for (int i = 0; i < V; i++) {
            const csplat_view &w = v[i];
            // (a view without Gaussians has no chunks nor radii: its tables keep tiles = 0 and nothing reads them)
            CSPLAT_REQUIRE(w.P <= 0 || (w.geom && w.binning && w.image && w.out_color && w.scratch && w.dL_dpix && w.radii),
                           "csplat_backward_views: missing saved state, scratch or dL_dpix");
            DepthView &d = dtab.v[i];
            const int tiles = tiles_of(w.W, w.H);
            const ScratchView sv = scratch_view(w, g.path);
            fill_k7_view(w, sv, tiles, d.b, dt.v[i]);
            d.dL_ddepth = w.dL_ddepth;
            d.dpart = sv.dpart;
            d.W = w.W; d.H = w.H; d.gx = cdiv(w.W, CSPLAT_TILE);
            d.tiles = (w.P > 0 && w.num_rendered > 0) ? tiles : 0;
            any_depth = any_depth || w.dL_ddepth;
            if (feat) {
                CSPLAT_REQUIRE(w.n_features >= 0 && w.n_features <= CSPLAT_MAX_FEATURES &&
                               ((w.n_features == 0) == (w.features == nullptr) || (w.P <= 0 && w.features == nullptr)),
                               "csplat_backward_views: n_features must be 0..6, with features set exactly when it is not 0");
                CSPLAT_REQUIRE(!w.dL_dfeatures || w.n_features > 0, "csplat_backward_views: dL_dfeatures without features");
                FeatView &f = ftab.v[i];
                f.d = d;
                f.radii = w.radii; f.features = w.features; f.nf = w.n_features; f.dL_dfeat = w.dL_dfeatures; f.dL_dalpha = w.dL_dalpha;
                f.wpart = sv.wpart;
                f.dL_dfeat_in = w.n_features > 0 ? w.dL_dfeat_in : nullptr; f.P = w.P; f.accmask = w.accmask;
                for (int j = 0; j < n_earlier && f.dL_dfeat_in; j++)
                    if (earlier[j].n_features > 0 && earlier[j].dL_dfeat_in == f.dL_dfeat_in) f.accmask |= FEAT_ADD_IN;
                any_fgrad = any_fgrad || w.dL_dfeatures;
            }
            if (w.P <= 0) continue;
            Pmax = w.P > Pmax ? w.P : Pmax;
            // (the records start at zero: the bit-reproducible mode writes every one of them, CSPLAT_SCRATCH_ZEROED promises them)
            if (det_mode) HIP_TRY(hipMemsetAsync(sv.det, 0, sv.det_bytes, join));
            else if (!(w.accmask & CSPLAT_SCRATCH_ZEROED)) HIP_TRY(hipMemsetAsync(sv.acc, 0, (size_t)w.P * ACC_STRIDE * 4, join));
            const int64_t sl = k7_slots(w, tiles);
            slots = sl > slots ? sl : slots;
        }
        const unsigned items = (unsigned)cdiv(slots, 8) * 32u;
        if (slots > 0 && (any_depth || !feat)) {
            ProfScope ps(PROF_K7_DEPTH_PARTIALS, join);
            k_depth_bwd_partials<<<dim3((unsigned)slots, V), 256, 0, join>>>(dtab);
            LAUNCH_CHECK();
        }
        if (feat) {
            if (slots > 0) {
                if (any_fgrad) {
                    ProfScope ps(PROF_K7_FEAT_PARTIALS, join);
                    k_feature_bwd_partials<<<dim3((unsigned)slots, V), 256, 0, join>>>(ftab);
                    LAUNCH_CHECK();
                }
                ProfScope ps(PROF_K7_FEAT, join);
                if (det_mode) k_feature_composite_bwd_views<true><<<dim3(items, V), 256, 0, join>>>(ftab);
                else k_feature_composite_bwd_views<false><<<dim3(items, V), 256, 0, join>>>(ftab);
                LAUNCH_CHECK();
            }
            if (det_mode)
                if (int rc = det_reduce_each(V, v, dt, k_feature_det_reduce_views, join)) return rc;
            if (Pmax > 0) {     // the feature gradients leave the records before K8 reads (and may clear) them
                ProfScope ps(PROF_FEAT_GRADS, join);
                k_feature_grads<<<dim3((unsigned)cdiv(Pmax, 256), 1), 256, 0, join>>>(ftab);
                LAUNCH_CHECK();
            }
        } else {
            if (slots > 0) {
                ProfScope ps(PROF_K7_DEPTH, join);
                if (det_mode) k_depth_composite_bwd_views<true><<<dim3(items, V), 256, 0, join>>>(dtab);
                else k_depth_composite_bwd_views<false><<<dim3(items, V), 256, 0, join>>>(dtab);
                LAUNCH_CHECK();
            }
            if (det_mode)
                if (int rc = det_reduce_each(V, v, dt, k_depth_det_reduce_views, join)) return rc;
        }
    }
    if (!g.want_k8) return 0;
    int cam_rows[RASTER_MAX_VIEWS] = {0};
    if (g.one_k8) {
        if (int rc = launch_k8_views(V, v, g.path, g.tab, true, g.cam_k8, slice, nslices, join, cam_rows)) return rc;
    } else {
        for (int i = 0; i < V; i++)       // per-view K8 on the join stream, in view order (views may add into one another's buffers)
            if (int rc = backward_one(v[i], g.path, join, join, false, true, v[i].dL_ddepth != nullptr, g.cam_k8, &cam_rows[i])) return rc;
    }
    return g.cam ? cam_tail(V, v, g.path, join, cam_rows) : 0;
}

// the colour path (no view has a depth, feature or alpha gradient)
static int backward_views_colour(int V, csplat_view *v, hipStream_t join, GroupPlan &g, int slice, int nslices) {
    CSPLAT_REQUIRE(!g.cam || V <= RASTER_MAX_VIEWS, "csplat_backward_views: camera / background gradients are taken for at most 8 views per group");
    int cam_rows[RASTER_MAX_VIEWS] = {0};
    const bool shared = g.shared, one_k8 = g.one_k8, det_mode = g.det_mode;
    // K7 of all views in ONE launch on the join stream (plus one launch clearing the records) when the views are alike
    bool batch_k7 = V >= 2 && V <= RASTER_MAX_VIEWS && !dbg(CSPLAT_DEBUG_PER_VIEW_LAUNCHES);
    for (int i = 0; i < V && batch_k7; i++)
        batch_k7 = v[i].P == v[0].P && v[i].P > 0 && v[i].W == v[0].W && v[i].H == v[0].H && v[i].num_rendered > 0 && v[i].geom &&
                   v[i].binning && v[i].image && v[i].out_color && v[i].scratch && v[i].dL_dpix;
    // one launch per stage for all views: everything runs on the join stream, the views' own streams are not involved and need
    // neither the entry nor the exit fence (six event / wait calls, ~25 us of host time per step)
    const bool lone = V == 1 && (hipStream_t)v[0].stream == join;      // one view on the caller's stream: nothing to fence
    const bool side_streams = !(batch_k7 && one_k8) && !lone;
    CSPLAT_REQUIRE(g.whole || (batch_k7 && one_k8), "csplat_backward_views_parts: only the one-launch-per-stage path can be cut into parts");
    CSPLAT_REQUIRE(!(V > 0 && v[0].valid) || !side_streams, "csplat_backward_views: views launched on faith need the one-launch-per-stage path");
    if (side_streams)
        if (int rc = fence_in(V, v, join)) return rc;
    // from here on side streams may hold work on caller-owned buffers: whatever fails, the exit fence is still issued
    auto body = [&]() -> int {
        if (batch_k7 && g.want_k7) {
            const int W = v[0].W, H = v[0].H, P = v[0].P, gx = cdiv(W, CSPLAT_TILE), tiles = tiles_of(W, H);
            B2Table bt;
            DetTable dt;
            dt.valid = v[0].valid;
            int64_t slots = 0;
            for (int i = 0; i < V; i++) {
                fill_k7_view(v[i], scratch_view(v[i], g.path), tiles, bt.v[i], dt.v[i]);
                const int64_t sl = k7_slots(v[i], tiles);
                slots = sl > slots ? sl : slots;
            }
            {   // (measurement hook, off unless csplat_debug_stamps handed over a buffer large enough for this launch)
                const size_t need = (size_t)V * ((size_t)cdiv(slots, 8) * 32u) * 12;
                bt.stamp = (g_stamp_buf && g_stamp_words >= need) ? g_stamp_buf : nullptr;
                bt.valid = v[0].valid;
            }
            bool zeroed = true;      // every view's records are zero already (CSPLAT_SCRATCH_ZEROED) and K8 will leave them so: no clearing launch
            for (int i = 0; i < V; i++) zeroed = zeroed && (v[i].accmask & CSPLAT_SCRATCH_ZEROED);
            if (det_mode) {          // (k_det_reduce_views writes every record: nothing to clear but the (entry, block) records)
                k_zero_det_views<<<dim3(1024, V), 256, 0, join>>>(bt);
                LAUNCH_CHECK();
            } else if (!zeroed) {
                const int64_t n4 = (int64_t)P * ACC_STRIDE / 4;
                k_zero_acc_views<<<dim3((unsigned)(cdiv(n4, 256) > 1024 ? 1024 : cdiv(n4, 256)), V), 256, 0, join>>>(n4, bt);
                LAUNCH_CHECK();
            }
            ProfScope ps(PROF_K7, join);       // (the bracket bench.py's roofline reads: K7's launch alone, not the record clearing in front of it)
            const unsigned items = (unsigned)cdiv(slots, 8) * 32u;
            if (det_mode) {
                k_composite_bwd_rows_views_det<<<dim3(items, V), 256, 0, join>>>(tiles, W, H, gx, bt);
                LAUNCH_CHECK();
                k_det_reduce_views<<<dim3((unsigned)cdiv(P, 256), V), 256, 0, join>>>(P, dt);
            } else
                k_composite_bwd_rows_views<<<dim3(items, V), 256, 0, join>>>(tiles, W, H, gx, bt);
            LAUNCH_CHECK();
        }
        for (int i = 0; i < V && !(batch_k7 && one_k8); i++) {
            const csplat_view &w = v[i];
            if (int rc = backward_one(w, g.path, (hipStream_t)w.stream, (shared || batch_k7) ? join : (hipStream_t)w.stream, !batch_k7, !one_k8,
                                      false, g.cam_k8, &cam_rows[i]))
                return rc;
        }
        if (one_k8 && g.want_k8) {   // every view's K7 is queued on its own stream: the join stream waits for all of them, then ONE K8
            for (int i = 0; i < V && !batch_k7; i++) {
                if ((hipStream_t)v[i].stream == join) continue;
                hipEvent_t ev = pooled_event();
                CSPLAT_REQUIRE(ev != nullptr, "csplat_backward_views: no event");
                HIP_TRY(hipEventRecord(ev, (hipStream_t)v[i].stream));
                HIP_TRY(hipStreamWaitEvent(join, ev, 0));
            }
            return launch_k8_views(V, v, g.path, g.tab, false, g.cam_k8, slice, nslices, join, cam_rows);
        }
        return 0;
    };
    const int rc = body();
    const int r2 = side_streams ? fence_out(V, v, join) : 0;
    if (!rc && !r2 && g.cam) return cam_tail(V, v, g.path, join, cam_rows);     // (behind every view's K8: the exit fence has joined their streams)
    return rc ? rc : r2;
}

// The only way into the backward.  The path (colour, depth, feature; camera or not) is the call's.  A call of more than 8 views that takes
// the depth, feature or camera path runs in groups of at most 8 views (view_group), one after the other on the join stream, each as a call
// of its own views would run: every group writes or adds into the call's gradient buffers as the views' accmask says (an accumulating view
// of a later group adds to what an earlier group wrote), dL_dfeat_in included.  A call of up to 8 views is one group: its launches are those
// of the ungrouped call.  The colour path without camera gradients takes any number of views as one group.
static int backward_views_impl(int V, csplat_view *v, void *join_stream, unsigned parts, int slice, int nslices) {
    CSPLAT_REQUIRE(V >= 0 && (V == 0 || v != nullptr), "csplat_backward_views: bad view count");
    CSPLAT_REQUIRE(parts >= 1 && parts <= 3 && nslices >= 1 && slice >= 0 && slice < nslices, "csplat_backward_views_parts: bad parts / slice");
    GroupPlan g;
    bool depth = false;
    g.cam = g.cam_k8 = g.feat = false;
    for (int i = 0; i < V; i++) {
        g.cam_k8 = g.cam_k8 || cam_k8_wanted(v[i]);
        g.cam = g.cam || cam_k8_wanted(v[i]) || v[i].dL_dbg != nullptr;
        g.feat = g.feat || feat_wanted(v[i]);
        depth = depth || v[i].dL_ddepth != nullptr;
    }
    if (g.cam) {
        CSPLAT_REQUIRE(parts == 3u && nslices == 1, "csplat_backward_views_parts: camera / background gradients are taken by the whole call only");
        CSPLAT_REQUIRE(!(V > 0 && v[0].valid), "csplat_backward_views: views launched on faith take no camera / background gradient");
        for (int i = 0; i < V; i++)
            CSPLAT_REQUIRE(v[i].scratch, "csplat_backward_views: camera gradients need scratch of csplat_backward_camera_scratch_bytes");
    }
    for (int i = 0; i < V; i++)
        CSPLAT_REQUIRE(!aa_of(v[i]) || v[i].opacities || v[i].P <= 0, "csplat_backward_views: CSPLAT_ANTIALIAS needs the view's opacities");
    if (g.feat) {
        CSPLAT_REQUIRE(!(V > 0 && v[0].valid), "csplat_backward_views: views launched on faith take no feature or alpha gradient");
        for (int i = 0; i < V; i++)
            CSPLAT_REQUIRE(v[i].scratch, "csplat_backward_views: feature / alpha gradients need scratch of csplat_backward_feature_scratch_bytes");
    }
    g.path = g.feat ? SP_FEATURE : g.cam ? SP_CAMERA : depth ? SP_DEPTH : SP_COLOUR;
    hipStream_t join = (hipStream_t)join_stream;
    for (int k = 0, ng = g.path == SP_COLOUR ? 1 : view_groups(V); k < ng; k++) {
        int lo = 0, hi = V;
        if (ng > 1) view_group(V, k, &lo, &hi);
        plan_group(hi - lo, v + lo, parts, nslices, g);
        const int rc = (g.feat || depth) ? backward_views_depth(hi - lo, v + lo, join, g, slice, nslices, v, lo)
                                         : backward_views_colour(hi - lo, v + lo, join, g, slice, nslices);
        if (rc) return rc;
    }
    return 0;
}

int csplat_backward_views(int V, csplat_view *v, void *join_stream) { return backward_views_impl(V, v, join_stream, 3u, 0, 1); }
// csplat_backward_views cut into parts (round 6: the gradient exchange of a view-parallel step starts before the backward has ended).
// parts bit 0: the compositing backward (K7) of all views; bit 1: the per-Gaussian backward (K8) for SLICE `slice` of `nslices` equal
// ranges of Gaussians (boundaries at multiples of 32: csplat_backward_slice_rows) -- a caller launches K7 once, then the K8 slices one by
// one, and may hand the gradient rows of slice g to its collective while slice g + 1 computes.  Only the one-launch-per-stage path can be
// cut (the views share P, SH, scales and the image size, as csplat_forward_views_faith requires); parts == 3 with one slice is
// csplat_backward_views.  The sum of the parts is the whole call bit for bit: every Gaussian's arithmetic is the same in any slicing.
int csplat_backward_views_parts(int V, csplat_view *v, void *join_stream, unsigned parts, int slice, int nslices) {
    return backward_views_impl(V, v, join_stream, parts, slice, nslices);
}
// rows [*row_lo, *row_hi) of the P Gaussians that K8 slice `slice` of `nslices` finishes
int csplat_backward_slice_rows(int P, int slice, int nslices, int64_t *row_lo, int64_t *row_hi) {
    CSPLAT_REQUIRE(P >= 0 && nslices >= 1 && slice >= 0 && slice < nslices && row_lo && row_hi, "csplat_backward_slice_rows: bad arguments");
    const int64_t nb = cdiv(P, 32);
    const int64_t lo = nb * slice / nslices * 32, hi = nb * (slice + 1) / nslices * 32;
    *row_lo = lo < P ? lo : P; *row_hi = hi < P ? hi : P;
    return 0;
}

// ---- the single-view C entry points: their arguments as a csplat_view (everything else zero: no accumulation, no antialiasing, no extras),
// then a call of one view on its own stream
static csplat_view pack_view(void *stream, int P, int D, int M, int R, const float *bg, int W, int H, const float *means3D, const float *shs,
                             const float *colors_precomp, const float *scales, float scale_modifier, const float *rotations,
                             const float *cov3D_precomp, const float *view, const float *proj, const float *campos, float tanfovx,
                             float tanfovy, const int32_t *radii, const void *geom, const void *binning, const void *image,
                             const float *out_color, const float *dL_dpix, const float *dL_ddepth, void *scratch, float *dL_dmean2D,
                             float *dL_dconic, float *dL_dopacity, float *dL_dcolor, float *dL_dmean3D, float *dL_dcov3D, float *dL_dsh,
                             float *dL_dscale, float *dL_drot) {
    csplat_view w;
    memset(&w, 0, sizeof(w));
    w.stream = stream;
    w.P = P; w.D = D; w.M = M; w.W = W; w.H = H;
    w.scale_modifier = scale_modifier; w.tanfovx = tanfovx; w.tanfovy = tanfovy;
    w.bg = bg; w.means3D = means3D; w.shs = shs; w.colors_precomp = colors_precomp; w.scales = scales; w.rotations = rotations;
    w.cov3D_precomp = cov3D_precomp; w.view = view; w.proj = proj; w.campos = campos;
    w.out_color = const_cast<float *>(out_color); w.radii = const_cast<int32_t *>(radii);
    w.num_rendered = R; w.layout_rendered = R;
    w.geom = const_cast<void *>(geom); w.binning = const_cast<void *>(binning); w.image = const_cast<void *>(image);
    w.dL_dpix = dL_dpix; w.dL_ddepth = dL_ddepth; w.scratch = scratch;
    w.dL_dmean2D = dL_dmean2D; w.dL_dconic = dL_dconic; w.dL_dopacity = dL_dopacity; w.dL_dcolor = dL_dcolor; w.dL_dmean3D = dL_dmean3D;
    w.dL_dcov3D = dL_dcov3D; w.dL_dsh = dL_dsh; w.dL_dscale = dL_dscale; w.dL_drot = dL_drot;
    return w;
}
int csplat_backward(void *stream, int P, int D, int M, int R, const float *bg, int W, int H, const float *means3D,
                    const float *shs, const float *colors_precomp, const float *scales, float scale_modifier,
                    const float *rotations, const float *cov3D_precomp, const float *view, const float *proj,
                    const float *campos, float tanfovx, float tanfovy, const int32_t *radii, const void *geom,
                    const void *binning, const void *image, const float *out_color, const float *dL_dpix, void *scratch,
                    float *dL_dmean2D,
                    float *dL_dconic, float *dL_dopacity, float *dL_dcolor, float *dL_dmean3D, float *dL_dcov3D,
                    float *dL_dsh, float *dL_dscale, float *dL_drot) {
    return csplat_backward_depth(stream, P, D, M, R, bg, W, H, means3D, shs, colors_precomp, scales, scale_modifier, rotations, cov3D_precomp,
                                 view, proj, campos, tanfovx, tanfovy, radii, geom, binning, image, out_color, dL_dpix, nullptr, scratch,
                                 dL_dmean2D, dL_dconic, dL_dopacity, dL_dcolor, dL_dmean3D, dL_dcov3D, dL_dsh, dL_dscale, dL_drot);
}
// csplat_backward with the depth image's gradient (NULL dL_ddepth = the call is csplat_backward's: the colour path)
int csplat_backward_depth(void *stream, int P, int D, int M, int R, const float *bg, int W, int H, const float *means3D,
                          const float *shs, const float *colors_precomp, const float *scales, float scale_modifier,
                          const float *rotations, const float *cov3D_precomp, const float *view, const float *proj,
                          const float *campos, float tanfovx, float tanfovy, const int32_t *radii, const void *geom,
                          const void *binning, const void *image, const float *out_color, const float *dL_dpix, const float *dL_ddepth,
                          void *scratch, float *dL_dmean2D, float *dL_dconic, float *dL_dopacity, float *dL_dcolor, float *dL_dmean3D,
                          float *dL_dcov3D, float *dL_dsh, float *dL_dscale, float *dL_drot) {
    csplat_view w = pack_view(stream, P, D, M, R, bg, W, H, means3D, shs, colors_precomp, scales, scale_modifier, rotations, cov3D_precomp, view,
                              proj, campos, tanfovx, tanfovy, radii, geom, binning, image, out_color, dL_dpix, dL_ddepth, scratch, dL_dmean2D,
                              dL_dconic, dL_dopacity, dL_dcolor, dL_dmean3D, dL_dcov3D, dL_dsh, dL_dscale, dL_drot);
    return backward_views_impl(1, &w, stream, 3u, 0, 1);
}

}  // extern "C"
