// csplat_raster_extended.h -- part of csplat_raster.hip, included there once, behind that file's K7 section.
// The backward passes of the extended outputs, each launched only when a view asks for it: the depth-gradient K7 wrappers and their
// prepass, the feature / alpha kernels (forward and backward), the visibility walk and reduce.
// Uses from csplat_raster.hip's K7 section: composite_bwd_body, det_reduce_views_body, B2View, DetTable, ACC_STRIDE; from
// csplat_raster_k5b_k6.h: ALPHA_MIN; from csplat_raster_binning.h: SEG; from csplat_raster_math.h: Cam, RASTER_MAX_VIEWS, tile_rect.
#pragma once

namespace {

// ------------------------------------------------------------------------------------------- K7, depth-gradient path
// Launched only when a depth gradient is given (csplat_view.dL_ddepth); the default K7 / K8 launches are untouched.
// The forward's checkpoints hold (T, colour so far) at every segment start but no depth, so a prepass computes, per (segment, pixel),
// the segment's partial depth  dpart = sum over its blended entries of T alpha z  (T from the checkpoint, entries from K6's bbits words,
// the same alpha / threshold / n_contrib tests as K7); the depth K7 then needs only sums of partials for D_behind (composite_bwd_body).
struct DepthView {
    B2View b;
    const float *dL_ddepth;   // [H][W], NULL: this view has no depth gradient (its depth terms are zero)
    float *dpart;             // [slots][256] (segment, pixel of the tile in block-major order, as the checkpoints)
    int W, H, gx, tiles;      // tiles = 0: the view has no list entries -- nothing to do
};
struct DepthTable { DepthView v[RASTER_MAX_VIEWS]; };
__global__ __launch_bounds__(256) void k_depth_bwd_partials(DepthTable tab) {
    const DepthView &w = tab.v[blockIdx.y];
    if (!w.dL_ddepth || w.tiles == 0) return;
    const int slot = blockIdx.x;
    const int *seg_offset = w.b.seg_offset;
    if (slot >= seg_offset[w.tiles]) return;
    const int tile = w.b.slot_tile[slot];
    const int seg_lo = (slot - seg_offset[tile]) * SEG;
    const int blk = threadIdx.x >> 4, l16 = threadIdx.x & 15;
    const uint32_t *blk_hi = reinterpret_cast<const uint32_t *>(seg_offset) + w.tiles + 1 + tile * 16;
    const int px = (tile % w.gx) * CSPLAT_TILE + (blk & 3) * 4 + (l16 & 3);
    const int py = (tile / w.gx) * CSPLAT_TILE + (blk >> 2) * 4 + (l16 >> 2);
    float D = 0.f;
    if ((int)blk_hi[blk] > seg_lo && px < w.W && py < w.H) {
        const int nc = (int)w.b.n_contrib[py * w.W + px];
        if (nc > seg_lo) {
            float T = w.b.ckpt[(size_t)slot * 256 + threadIdx.x].x;
            const uint32_t rx = (uint32_t)w.b.ranges[tile].x;
            const float fx = (float)px, fy = (float)py;
            constexpr int NW = SEG / 64;
            const unsigned long long *bw = w.b.bbits + ((size_t)slot * 16 + (size_t)blk) * NW;
            for (int c = 0; c < NW; c++) {
                unsigned long long m = bw[c];
                while (m) {
                    const int pos = seg_lo + 64 * c + __builtin_ctzll(m);
                    m &= m - 1ull;
                    if (pos >= nc) { c = NW; break; }
                    const uint32_t ri = rx + (uint32_t)pos;
                    const float4 A = w.b.recA[ri], B = w.b.recB[ri];
                    const float z = reinterpret_cast<const float *>(w.b.recC)[2 * (size_t)ri + 1];
                    const float dx = A.x - fx, dy = A.y - fy;
                    const float power = -0.5f * (A.z * dx * dx + B.x * dy * dy) - A.w * dx * dy;
                    const float a = fminf(0.99f, B.y * __expf(power));
                    if (power > 0.f || a < ALPHA_MIN) continue;
                    D += a * T * z;
                    T *= 1.f - a;
                }
            }
        }
    }
    w.dpart[(size_t)slot * 256 + threadIdx.x] = D;
}
template <bool DET>
__global__ __launch_bounds__(256) void k_depth_composite_bwd_views(DepthTable tab) {
    const DepthView &w = tab.v[blockIdx.y];
    if (w.tiles == 0) return;
    const B2View &b = w.b;
    composite_bwd_body<DET, true>(w.tiles, w.W, w.H, w.gx, b.ranges, b.ids_sorted, b.bbits, b.recA, b.recB, b.recC, b.R, b.seg_offset,
                                  b.slot_tile, b.ckpt, b.final_T, b.n_contrib, b.out_color, b.dL_dpix, b.acc, b.det, nullptr,
                                  (int)blockIdx.x, w.dL_ddepth, w.dpart);
}
__global__ __launch_bounds__(256) void k_depth_det_reduce_views(int P, DetTable tab) { det_reduce_views_body<10>(P, tab); }

// ------------------------------------------------------------------------------------------- feature channels and the alpha image
// (ABI 9: csplat_view.features / out_features / out_alpha and their gradients.)  Launched only when a view asks for them; K6, K7 and K8
// of the default, depth and camera paths are untouched.
// Forward: a pass BEHIND K6, one thread per pixel and one workgroup per tile.  The pixel walks its tile's segments; each segment starts
// from K6's checkpointed T and visits the entries its block blended (K6's bbits words), with K7's blend test (alpha, 1/255, n_contrib):
// feat[c] = sum T alpha f[id][c] over exactly the entries the colour blended, front to back.  alpha = 1 - final_T, the factor of the colour's
// background term.  (K6 itself is not touched: a feature variant of it would carry F more accumulators through its transmittance chain.)
struct FeatFwdView {
    const int2 *ranges;
    const uint32_t *ids_sorted;
    const unsigned long long *bbits;
    const float4 *recA, *recB;
    const int *seg_offset;
    const float4 *ckpt;
    const float *final_T;
    const uint32_t *n_contrib;
    const float *features;    // [P][nf], NULL when nf = 0
    float *out_features;      // [nf][H][W], NULL: not asked for
    float *out_alpha;         // [H][W], NULL: not asked for
    int nf, W, H, gx, tiles;  // tiles = 0: the view has no list entries (feat = 0, alpha = 0)
};
struct FeatFwdTable { FeatFwdView v[RASTER_MAX_VIEWS]; };
// one pixel's walk over the blended entries of one segment (slot) from transmittance T: calls f(T alpha, list position) per blended entry
template <typename Fn>
__device__ __forceinline__ void walk_segment(const float4 *__restrict__ recA, const float4 *__restrict__ recB,
                                             const unsigned long long *__restrict__ bbits, int slot, int blk, int seg_lo, int nc,
                                             uint32_t rx, float fx, float fy, float T, Fn &&f) {
    constexpr int NW = SEG / 64;
    const unsigned long long *bw = bbits + ((size_t)slot * 16 + (size_t)blk) * NW;
    for (int c = 0; c < NW; c++) {
        unsigned long long m = bw[c];
        while (m) {
            const int pos = seg_lo + 64 * c + __builtin_ctzll(m);
            m &= m - 1ull;
            if (pos >= nc) return;
            const uint32_t ri = rx + (uint32_t)pos;
            const float4 A = recA[ri], B = recB[ri];
            const float dx = A.x - fx, dy = A.y - fy;
            const float power = -0.5f * (A.z * dx * dx + B.x * dy * dy) - A.w * dx * dy;
            const float a = fminf(0.99f, B.y * __expf(power));
            if (power > 0.f || a < ALPHA_MIN) continue;
            f(a * T, ri);
            T *= 1.f - a;
        }
    }
}
__global__ __launch_bounds__(256) void k_feature_fwd_views(FeatFwdTable tab) {
    const FeatFwdView &w = tab.v[blockIdx.y];
    const int tile = blockIdx.x;
    const int ntiles = w.gx * ((w.H + CSPLAT_TILE - 1) / CSPLAT_TILE);
    if (tile >= ntiles) return;
    const int blk = threadIdx.x >> 4, l16 = threadIdx.x & 15;
    const int px = (tile % w.gx) * CSPLAT_TILE + (blk & 3) * 4 + (l16 & 3);
    const int py = (tile / w.gx) * CSPLAT_TILE + (blk >> 2) * 4 + (l16 >> 2);
    if (px >= w.W || py >= w.H) return;
    const int pix = py * w.W + px;
    float acc[CSPLAT_MAX_FEATURES];
#pragma unroll
    for (int c = 0; c < CSPLAT_MAX_FEATURES; c++) acc[c] = 0.f;
    float alpha = 0.f;
    if (w.tiles > 0) {
        alpha = 1.f - w.final_T[pix];
        const int nc = (int)w.n_contrib[pix];
        if (w.nf > 0 && nc > 0) {
            const int s0 = w.seg_offset[tile], s1 = w.seg_offset[tile + 1];
            const uint32_t rx = (uint32_t)w.ranges[tile].x;
            const float *feat = w.features;
            const int nf = w.nf;
            for (int slot = s0; slot < s1; slot++) {
                const int seg_lo = (slot - s0) * SEG;
                if (nc <= seg_lo) break;
                walk_segment(w.recA, w.recB, w.bbits, slot, blk, seg_lo, nc, rx, (float)px, (float)py,
                             w.ckpt[(size_t)slot * 256 + threadIdx.x].x, [&](float wt, uint32_t ri) {
                                 const float *fr = feat + (size_t)w.ids_sorted[ri] * nf;
#pragma unroll
                                 for (int c = 0; c < CSPLAT_MAX_FEATURES; c++)
                                     if (c < nf) acc[c] += wt * fr[c];
                             });
            }
        }
    }
    const size_t HW = (size_t)w.H * w.W;
    if (w.out_features)
#pragma unroll
        for (int c = 0; c < CSPLAT_MAX_FEATURES; c++)
            if (c < w.nf) w.out_features[c * HW + pix] = acc[c];
    if (w.out_alpha) w.out_alpha[pix] = alpha;
}

// Backward.  K7 needs, per entry, what lies behind it in every channel, weighted by the pixel's feature gradients; a prepass (as the depth
// path's) leaves per (segment, pixel) wpart = sum over the segment's blended entries of T alpha wf, wf = sum_c dL/dfeat_c f[id][c] -- one
// float per (segment, pixel) whatever F, in backward scratch only; the forward keeps nothing for it.
struct FeatView {
    DepthView d;
    const int32_t *radii;
    const float *features;    // [P][nf]
    const float *dL_dfeat;    // [nf][H][W], NULL: no feature gradient in this view
    const float *dL_dalpha;   // [H][W], NULL: no alpha gradient in this view
    float *wpart;             // [slots][256]
    float *dL_dfeat_in;       // [P][nf] (written, or added when an earlier view of the call has the same buffer), NULL: not wanted
    int nf, P;
    unsigned accmask;         // the view's CSPLAT_ACC_* / CSPLAT_SCRATCH_ZEROED / CSPLAT_K8_OUTPUTS_UNREAD bits, plus FEAT_ADD_IN
};
// not an ABI bit: an earlier group of views of the same call (backward_views_impl) already wrote dL_dfeat_in -- add to it
constexpr unsigned FEAT_ADD_IN = 1u << 31;
struct FeatTable { FeatView v[RASTER_MAX_VIEWS]; int n; };
__global__ __launch_bounds__(256) void k_feature_bwd_partials(FeatTable tab) {
    const FeatView &fv = tab.v[blockIdx.y];
    const DepthView &w = fv.d;
    if (!fv.dL_dfeat || w.tiles == 0) return;
    const int slot = blockIdx.x;
    const int *seg_offset = w.b.seg_offset;
    if (slot >= seg_offset[w.tiles]) return;
    const int tile = w.b.slot_tile[slot];
    const int seg_lo = (slot - seg_offset[tile]) * SEG;
    const int blk = threadIdx.x >> 4, l16 = threadIdx.x & 15;
    const uint32_t *blk_hi = reinterpret_cast<const uint32_t *>(seg_offset) + w.tiles + 1 + tile * 16;
    const int px = (tile % w.gx) * CSPLAT_TILE + (blk & 3) * 4 + (l16 & 3);
    const int py = (tile / w.gx) * CSPLAT_TILE + (blk >> 2) * 4 + (l16 >> 2);
    float S = 0.f;
    if ((int)blk_hi[blk] > seg_lo && px < w.W && py < w.H) {
        const int pix = py * w.W + px;
        const int nc = (int)w.b.n_contrib[pix];
        if (nc > seg_lo) {
            const int nf = fv.nf;
            const size_t HW = (size_t)w.H * w.W;
            float gf[CSPLAT_MAX_FEATURES];
#pragma unroll
            for (int c = 0; c < CSPLAT_MAX_FEATURES; c++) gf[c] = c < nf ? fv.dL_dfeat[c * HW + pix] : 0.f;
            const float *feat = fv.features;
            walk_segment(w.b.recA, w.b.recB, w.b.bbits, slot, blk, seg_lo, nc, (uint32_t)w.b.ranges[tile].x, (float)px, (float)py,
                         w.b.ckpt[(size_t)slot * 256 + threadIdx.x].x, [&](float wt, uint32_t ri) {
                             const float *fr = feat + (size_t)w.b.ids_sorted[ri] * nf;
                             float wf = 0.f;
#pragma unroll
                             for (int c = 0; c < CSPLAT_MAX_FEATURES; c++)
                                 if (c < nf) wf += gf[c] * fr[c];
                             S += wt * wf;
                         });
        }
    }
    fv.wpart[(size_t)slot * 256 + threadIdx.x] = S;
}
template <bool DET>
__global__ __launch_bounds__(256) void k_feature_composite_bwd_views(FeatTable tab) {
    const FeatView &fv = tab.v[blockIdx.y];
    const DepthView &w = fv.d;
    if (w.tiles == 0) return;
    const B2View &b = w.b;
    composite_bwd_body<DET, true, true>(w.tiles, w.W, w.H, w.gx, b.ranges, b.ids_sorted, b.bbits, b.recA, b.recB, b.recC, b.R, b.seg_offset,
                                        b.slot_tile, b.ckpt, b.final_T, b.n_contrib, b.out_color, b.dL_dpix, b.acc, b.det, nullptr,
                                        (int)blockIdx.x, w.dL_ddepth, w.dpart, fv.features, fv.nf, fv.dL_dfeat, fv.dL_dalpha, fv.wpart);
}
__global__ __launch_bounds__(256) void k_feature_det_reduce_views(int P, DetTable tab) { det_reduce_views_body<16>(P, tab); }
// record slots 10 .. 10 + nf - 1 of every view -> dL_dfeat_in, the views in call order (a buffer shared with an earlier view of the call
// is added to: a fixed order).  Runs between K7 and K8; slots 12..15 are cleared here when the records must be left zero (K8's
// clear_record takes 0..11).
__global__ __launch_bounds__(256) void k_feature_grads(FeatTable tab) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    for (int vi = 0; vi < tab.n; vi++) {
        const FeatView &fv = tab.v[vi];
        if (i >= fv.P) continue;
        float *acc = fv.d.b.acc + (size_t)i * ACC_STRIDE;
        const bool vis = fv.radii[i] > 0;
        if (fv.dL_dfeat_in) {
            bool add = (fv.accmask & FEAT_ADD_IN) != 0u;      // (a view of an earlier group of the call wrote the buffer)
            for (int vj = 0; vj < vi; vj++) add = add || tab.v[vj].dL_dfeat_in == fv.dL_dfeat_in;
            float *out = fv.dL_dfeat_in + (size_t)i * fv.nf;
            for (int c = 0; c < fv.nf; c++) {
                const float g = vis ? acc[10 + c] : 0.f;
                out[c] = add ? out[c] + g : g;
            }
        }
        if (vis && (fv.accmask & CSPLAT_SCRATCH_ZEROED))
            *reinterpret_cast<float4 *>(acc + 12) = make_float4(0.f, 0.f, 0.f, 0.f);
    }
}

// ------------------------------------------------------------------------------------------- Gaussian visibility, top-contributor map
// (csplat_visibility_views.)  Forward-only, launched only when asked for; K1..K8 and the feature kernels are untouched.  w_i(pix) = T_i alpha_i is
// the colour's blending weight (walk_segment's test: alpha with the 0.99 cap, 1/255 skip, n_contrib).  No float atomics: every sum runs in
// a fixed order, so the outputs are bit-reproducible in the default mode.
// Walk: one workgroup per tile, the pixels as in the feature forward.  The 16 lanes of a 4x4 block (one 16-lane row of a wave) step through
// their block's bbits positions in lockstep (the walk ends at the row's largest n_contrib; a lane past its own contributes 0) and join
// their weights per entry with DPP row scans (max, sum, count).  The 16 blocks of the tile meet in LDS: the sum as one slot per (block,
// entry), added in block order; max and count are order-free LDS atomics.  One (max, sum, count) record per LIST ENTRY leaves per segment,
// zeros included, so that every position of every list is written.  The pixel's top contributor (strictly larger weight, front to back:
// a tie keeps the front-most) stays in registers.
struct VisView {
    const int2 *ranges;
    const uint32_t *ids_sorted;
    const unsigned long long *bbits;
    const float4 *recA, *recB;
    const int *seg_offset;
    const float4 *ckpt;
    const uint32_t *n_contrib;
    int32_t *top_id;           // [H][W], NULL: not wanted
    float *rec_max, *rec_sum;  // [R] per list entry (scratch), NULL: no per-Gaussian output wanted
    int32_t *rec_cnt;
    int W, H, gx, tiles;       // tiles = 0: the view has no list entries (top_id = -1 everywhere)
};
struct VisTable { VisView v[RASTER_MAX_VIEWS]; };
static_assert(SEG == 256, "the visibility join keeps one list entry per thread of a segment");
// inclusive scans over the 16 lanes of a DPP row (row_shr 1, 2, 4, 8; lanes shifted in from outside the row read 0): lane 15 of the row then
// holds the row's sum / max / count, formed in the same order in every run
template <int N> __device__ __forceinline__ float row_shr_f(float x) { return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0x110 + N, 0xF, 0xF, true)); }
template <int N> __device__ __forceinline__ int row_shr_i(int x) { return __builtin_amdgcn_update_dpp(0, x, 0x110 + N, 0xF, 0xF, true); }
__device__ __forceinline__ void row16_join(float &mx, float &sm, int &cn) {     // (mx >= 0: the 0 shifted in is neutral)
    mx = fmaxf(mx, row_shr_f<1>(mx)); sm += row_shr_f<1>(sm); cn += row_shr_i<1>(cn);
    mx = fmaxf(mx, row_shr_f<2>(mx)); sm += row_shr_f<2>(sm); cn += row_shr_i<2>(cn);
    mx = fmaxf(mx, row_shr_f<4>(mx)); sm += row_shr_f<4>(sm); cn += row_shr_i<4>(cn);
    mx = fmaxf(mx, row_shr_f<8>(mx)); sm += row_shr_f<8>(sm); cn += row_shr_i<8>(cn);
}
__global__ __launch_bounds__(256) void k_visibility_walk_views(VisTable tab) {
    const VisView &w = tab.v[blockIdx.y];
    const int tile = blockIdx.x;
    const int ntiles = w.gx * ((w.H + CSPLAT_TILE - 1) / CSPLAT_TILE);
    if (tile >= ntiles) return;                                         // (uniform in the workgroup)
    __shared__ float s_sum[16][SEG];
    __shared__ uint32_t s_max[SEG];
    __shared__ int s_cnt[SEG];
    const int blk = threadIdx.x >> 4, l16 = threadIdx.x & 15;
    const int px = (tile % w.gx) * CSPLAT_TILE + (blk & 3) * 4 + (l16 & 3);
    const int py = (tile / w.gx) * CSPLAT_TILE + (blk >> 2) * 4 + (l16 >> 2);
    const bool inside = px < w.W && py < w.H;
    const int pix = py * w.W + px;
    const bool recs = w.rec_sum != nullptr;
    float best = 0.f;
    int best_id = -1;
    if (w.tiles > 0) {
        const int nc = inside ? (int)w.n_contrib[pix] : 0;
        int ncr = nc;                                                   // the row's (block's) largest n_contrib
#pragma unroll
        for (int o = 8; o >= 1; o >>= 1) ncr = max(ncr, __shfl_xor(ncr, o, 16));
        const int s0 = w.seg_offset[tile], s1 = w.seg_offset[tile + 1];
        const uint32_t rx = (uint32_t)w.ranges[tile].x;
        const int len = w.ranges[tile].y - (int)rx;
        constexpr int NW = SEG / 64;
        for (int slot = s0; slot < s1; slot++) {                        // (every segment, in every thread: the join below syncs)
            const int seg_lo = (slot - s0) * SEG;
            if (recs) {
                float4 *z = reinterpret_cast<float4 *>(&s_sum[blk][l16 * 16]);
                const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
                z[0] = zero; z[1] = zero; z[2] = zero; z[3] = zero;
                s_max[threadIdx.x] = 0u;
                s_cnt[threadIdx.x] = 0;
                __syncthreads();
            }
            if (ncr > seg_lo) {                                         // (uniform in the row; K6 wrote this block's bbits / checkpoints)
                float T = nc > seg_lo ? w.ckpt[(size_t)slot * 256 + threadIdx.x].x : 0.f;
                const unsigned long long *bw = w.bbits + ((size_t)slot * 16 + (size_t)blk) * NW;
                const float fx = (float)px, fy = (float)py;
                int c = 0;
                unsigned long long m = bw[0];
                auto next = [&](int &p) -> bool {                       // the block's next blended position below ncr, in list order
                    while (m == 0ull) {
                        if (++c >= NW) return false;
                        m = bw[c];
                    }
                    p = seg_lo + 64 * c + __builtin_ctzll(m);
                    m &= m - 1ull;
                    return p < ncr;
                };
                int pos = 0;
                bool have = next(pos);
                float4 A = make_float4(0.f, 0.f, 0.f, 0.f), B = A;
                if (have) { A = w.recA[rx + (uint32_t)pos]; B = w.recB[rx + (uint32_t)pos]; }
                while (have) {
                    int npos = 0;
                    const bool nhave = next(npos);                      // (the next entry's records are loaded before this one is used)
                    float4 nA = A, nB = B;
                    if (nhave) { nA = w.recA[rx + (uint32_t)npos]; nB = w.recB[rx + (uint32_t)npos]; }
                    const float dx = A.x - fx, dy = A.y - fy;
                    const float power = -0.5f * (A.z * dx * dx + B.x * dy * dy) - A.w * dx * dy;
                    const float a = fminf(0.99f, B.y * __expf(power));
                    const bool bl = pos < nc && !(power > 0.f || a < ALPHA_MIN);
                    const float wt = bl ? a * T : 0.f;
                    if (bl) {
                        if (wt > best) { best = wt; best_id = (int)w.ids_sorted[rx + (uint32_t)pos]; }
                        T *= 1.f - a;
                    }
                    if (recs) {
                        float mx = wt, sm = wt;
                        int cn = bl ? 1 : 0;
                        row16_join(mx, sm, cn);
                        if (l16 == 15) {
                            s_sum[blk][pos - seg_lo] = sm;
                            if (cn > 0) {
                                atomicMax(&s_max[pos - seg_lo], __float_as_uint(mx));     // (non-negative floats order as their bits)
                                atomicAdd(&s_cnt[pos - seg_lo], cn);
                            }
                        }
                    }
                    pos = npos; A = nA; B = nB; have = nhave;
                }
            }
            if (recs) {
                __syncthreads();
                const int e = seg_lo + (int)threadIdx.x;
                if (e < len) {
                    float s = 0.f;
#pragma unroll
                    for (int b = 0; b < 16; b++) s += s_sum[b][threadIdx.x];
                    w.rec_max[rx + e] = __uint_as_float(s_max[threadIdx.x]);
                    w.rec_sum[rx + e] = s;
                    w.rec_cnt[rx + e] = s_cnt[threadIdx.x];
                }
                __syncthreads();
            }
        }
    }
    if (inside && w.top_id) w.top_id[pix] = best_id;
}
// Per Gaussian, one 16-lane row: its records in the tiles of its rectangle (the entry found by binary search on the unique (depth bits, id)
// key, as det_reduce_views_body does), lane l16 taking the tiles l16, l16 + 16, ... in y-major order, then the row's fixed-order join.
// Every output row is written, zeros for radii == 0.
struct VisRedView {
    Cam cam;
    const float2 *xy;
    const float *depth;
    const int32_t *radii;
    const int2 *ranges;
    const uint64_t *keys_sorted;
    const uint32_t *ids_sorted;
    const float *rec_max, *rec_sum;
    const int32_t *rec_cnt;
    float *weight_max, *weight_sum;   // [P], each NULL = not wanted
    int32_t *pixel_count;
    int P, tiles;                     // tiles = 0: no list entries (zeros); P = 0: nothing asked of this view
};
struct VisRedTable { VisRedView v[RASTER_MAX_VIEWS]; };
__global__ __launch_bounds__(256) void k_visibility_reduce_views(VisRedTable tab) {
    const VisRedView &w = tab.v[blockIdx.y];
    const int i = blockIdx.x * 16 + (int)(threadIdx.x >> 4);            // 16 lanes (one DPP row) per Gaussian
    const int l16 = threadIdx.x & 15;
    if (i >= w.P) return;                                               // (uniform in the row)
    float m = 0.f, s = 0.f;
    int n = 0;
    const int rad = w.tiles > 0 ? w.radii[i] : 0;
    if (rad > 0) {
        const float2 p = w.xy[i];
        int minx, miny, maxx, maxy;
        tile_rect(p.x, p.y, rad, w.cam, minx, miny, maxx, maxy);
        const uint64_t want = ((uint64_t)__float_as_uint(w.depth[i]) << 32) | (uint32_t)i;
        const int nx = maxx - minx, nt = nx * (maxy - miny);
        for (int k = l16; k < nt; k += 16) {                            // lane l16: the rectangle's tiles k = l16 (mod 16), y-major
            const int y = miny + k / nx, x = minx + k % nx;
            const int2 rg = w.ranges[y * w.cam.gx + x];
            int lo = rg.x, hi = rg.y;
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                const uint64_t key = ((w.keys_sorted[mid] & 0xFFFFFFFFull) << 32) | w.ids_sorted[mid];
                if (key < want) lo = mid + 1; else hi = mid;
            }
            if (lo >= rg.y || w.ids_sorted[lo] != (uint32_t)i) continue;
            m = fmaxf(m, w.rec_max[lo]);
            s += w.rec_sum[lo];
            n += w.rec_cnt[lo];
        }
    }
    row16_join(m, s, n);
    if (l16 != 15) return;
    if (w.weight_max) w.weight_max[i] = m;
    if (w.weight_sum) w.weight_sum[i] = s;
    if (w.pixel_count) w.pixel_count[i] = n;
}

}  // namespace
