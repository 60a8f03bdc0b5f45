// csplat_raster_k5b_k6.h -- part of csplat_raster.hip, included there once, behind csplat_raster_binning.h.
// The forward compositing on 4x4 pixel blocks: the row helpers, K5b (k_block_masks*), the blended-bit words (bbits) and K6 in its two forms
// (k_composite_fwd*: one wave per block, and the survivor-column form).
// Uses from csplat_raster_binning.h: SEG, INFO_BUSY, P2View, P2Table, p2_live, box_hit, dpp_mov; nothing of the two parts before it directly.
// Macros: CSPLAT_WORD_TO_LANE is defined and undefined inside block_masks_body.  CSPLAT_ROW_SCAN4 is never undefined and so stays
// defined to the end of the translation unit, as it always has; its readers (row_scan4_mul, row_scan4_add, row_scan4_min) are all here.
#pragma once

namespace {

// =================================================================================================== K5b / K6 / K7, block form
// The compositing kernels work on 4x4 PIXEL BLOCKS (16 per tile) instead of 8x8 quadrants: a wavefront owns ONE block and
// advances through the block's survivors FOUR AT A TIME -- DPP row r (16 lanes = the 16 pixels of the block) evaluates
// survivor r of the group.  On scene_1 a projected Gaussian covers ~16 of the 64 pixels of a quadrant (26 % of the lanes
// did useful work per survivor); it covers ~8 of the 16 pixels of the blocks it reaches, and a quadrant's survivor reaches
// 2.2 of the 4 blocks: ~1.8x fewer wave-instructions per (pixel, Gaussian) pair, 4x more waves, 4x shorter serial chains.
//   * the per-pixel transmittance chain crosses the four rows: every lane all-gathers the four (1 - alpha) factors of its
//     pixel (three v_permlane{16,32}_swap) and forms the running products in the sequential order T*F0*F1*F2*F3 -- the
//     same association as a one-entry-at-a-time walk, so skipping culled entries (factor 1) cannot change a bit of T;
//   * which entries reach which block is decided ONCE per view by k_block_masks (exact ellipse-vs-box test, one lane per
//     tile-list entry, 16 boxes): a 16-bit mask per entry plus a tile-ordered copy of what compositing reads (40 B, so the
//     walkers read contiguous records instead of gathering five arrays by Gaussian id).  Since round 4 the same masks also leave
//     TRANSPOSED (bmask[chunk][block]: the sixteen ballots of a wave's 64 entries): K6's wave takes its block's word of a chunk with one
//     scalar load; K7 no longer looks at the masks at all -- it walks what K6 found BLENDED (bbits);
//   * K7 runs FORWARD through a 256-entry segment: with S_k = sum_{j<=k} (c_j . dL/dC) alpha_j T_j (restarted from the
//     forward's checkpoint) the upstream back-to-front recurrence collapses to
//         dL/dalpha_k = T_k (c_k . dL/dC) - (out_colour . dL/dC - S_k) / (1 - alpha_k),
//     the same identity the depth-split restart already used once per segment;
//   * what a survivor's 16-lane row sums over its pixels are the MOMENTS of m = G dL/dalpha about the Gaussian's centre + three colour
//     sums (round 6; rounds 2-5: the nine gradient values, by a 4-level butterfly): they factor over the 4 x 4 block, 19 DPP adds + 3
//     selects per survivor row (processN), and go, nine lanes at once, to the Gaussian's 64-byte record as ONE global float-atomic
//     request per (entry, block) -- requests are priced per 64 bytes at the memory side (MI355X_MICROARCH.md "Global float atomics"),
//     and their rate is what binds the kernel (profiles/r06_k7_elimination.txt); K8 turns the moments into gradients.
constexpr float T_EPS = 0.0001f;
constexpr float ALPHA_MIN = 1.f / 255.f;

struct Row4 { float v0, v1, v2, v3; };
// every lane receives the values its pixel position holds in rows 0..3 (rows = 16-lane groups)
__device__ __forceinline__ Row4 rows_allgather(float f) {
    const auto s16 = __builtin_amdgcn_permlane16_swap(__float_as_uint(f), __float_as_uint(f), false, false);   // [f0 f0 f2 f2], [f1 f1 f3 f3]
    const auto ev = __builtin_amdgcn_permlane32_swap(s16[0], s16[0], false, false);                           // f0 x4, f2 x4
    const auto od = __builtin_amdgcn_permlane32_swap(s16[1], s16[1], false, false);                           // f1 x4, f3 x4
    return {__uint_as_float(ev[0]), __uint_as_float(od[0]), __uint_as_float(ev[1]), __uint_as_float(od[1])};
}
__device__ __forceinline__ float rows_sum(float f) { const Row4 g = rows_allgather(f); return ((g.v0 + g.v1) + g.v2) + g.v3; }
// row r of the wave takes the r-th argument: three DPP moves with a row mask (lanes of the other rows keep the old value)
__device__ __forceinline__ float rowsel(int, float a, float b, float c, float d) {
    int x = __float_as_int(a);
    x = __builtin_amdgcn_update_dpp(x, __float_as_int(b), 0xE4, 0x2, 0xF, false);
    x = __builtin_amdgcn_update_dpp(x, __float_as_int(c), 0xE4, 0x4, 0xF, false);
    x = __builtin_amdgcn_update_dpp(x, __float_as_int(d), 0xE4, 0x8, 0xF, false);
    return __int_as_float(x);
}

// ------------------------------------------------------------------------------------------- K5b
__device__ __forceinline__ void block_masks_body(int64_t R, int64_t null_at, int gx, const uint64_t *__restrict__ keys_sorted,
                                                 const uint32_t *__restrict__ ids_sorted, const float4 *__restrict__ pack,
                                                 uint16_t *__restrict__ mask16, float4 *__restrict__ recA,
                                                 float4 *__restrict__ recB, float2 *__restrict__ recC, int exact, int64_t block,
                                                 unsigned long long *__restrict__ bmask) {
    const int64_t i = block * 256 + threadIdx.x;
    // (workgroup-uniform: nothing of this workgroup's range is in use -- no list entry, not the list's last chunk, not the null record)
    if (block * 256 > (R | 63) && !(block * 256 <= null_at && null_at < block * 256 + 256)) return;
    if (i == null_at) {   // the null record behind the list (at the list's CAPACITY): opacity 0, pads incomplete groups of four
        mask16[i] = 0;
        recA[i] = make_float4(0.f, 0.f, 0.f, 0.f); recB[i] = make_float4(0.f, 0.f, 0.f, 0.f); recC[i] = make_float2(0.f, 0.f);
    }
    uint32_t m = 0;
    if (i < R) {
    const uint32_t tile = (uint32_t)(keys_sorted[i] >> 32), id = ids_sorted[i];
    const float4 pa = pack[3 * (size_t)id], pb = pack[3 * (size_t)id + 1], pc = pack[3 * (size_t)id + 2];
    const float2 c = make_float2(pa.x, pa.y);
    const float4 co = make_float4(pa.z, pa.w, pb.x, pb.y);
    const float cut = pc.z;
    const float x0 = (float)((tile % (uint32_t)gx) * CSPLAT_TILE), y0 = (float)((tile / (uint32_t)gx) * CSPLAT_TILE);
#pragma unroll
    for (int by = 0; by < 4; by++)
#pragma unroll
        for (int bx = 0; bx < 4; bx++)
            if (box_hit(c, cut, co, x0 + 4.f * bx, x0 + 4.f * bx + 3.f, y0 + 4.f * by, y0 + 4.f * by + 3.f, exact)) m |= 1u << (by * 4 + bx);
    mask16[i] = (uint16_t)m;
    recA[i] = pa;
    recB[i] = pb;
    recC[i] = make_float2(pc.x, pc.y);
    }
    // the wave's 64 entries are list chunk i >> 6: the sixteen ballots ARE the chunk's per-block words; lane b of the wave stores block b's
    // (entries at or behind the list's end contribute 0; K6 masks its last chunk by the list length anyway)
    if (bmask && (i >> 6) <= (R >> 6)) {
        uint32_t lo = 0u, hi = 0u;
        // (v_writelane_b32 with a literal lane: block b's ballot -- an SGPR pair -- lands in lane b of (lo, hi))
#define CSPLAT_WORD_TO_LANE(b)                                                                                                      \
        {                                                                                                                           \
            const unsigned long long wb_ = __builtin_amdgcn_ballot_w64((m >> b) & 1u);                                              \
            asm("v_writelane_b32 %0, %2, " #b "\n\tv_writelane_b32 %1, %3, " #b                                                     \
                : "+v"(lo), "+v"(hi) : "s"((uint32_t)wb_), "s"((uint32_t)(wb_ >> 32)));                                             \
        }
        CSPLAT_WORD_TO_LANE(0) CSPLAT_WORD_TO_LANE(1) CSPLAT_WORD_TO_LANE(2) CSPLAT_WORD_TO_LANE(3)
        CSPLAT_WORD_TO_LANE(4) CSPLAT_WORD_TO_LANE(5) CSPLAT_WORD_TO_LANE(6) CSPLAT_WORD_TO_LANE(7)
        CSPLAT_WORD_TO_LANE(8) CSPLAT_WORD_TO_LANE(9) CSPLAT_WORD_TO_LANE(10) CSPLAT_WORD_TO_LANE(11)
        CSPLAT_WORD_TO_LANE(12) CSPLAT_WORD_TO_LANE(13) CSPLAT_WORD_TO_LANE(14) CSPLAT_WORD_TO_LANE(15)
#undef CSPLAT_WORD_TO_LANE
        const int lane = threadIdx.x & 63;
        if (lane < 16) bmask[(size_t)(i >> 6) * 16 + lane] = ((unsigned long long)hi << 32) | lo;
    }
}
__global__ __launch_bounds__(256) void k_block_masks(int64_t R, int gx, const uint64_t *__restrict__ keys_sorted,
                                                      const uint32_t *__restrict__ ids_sorted, const float4 *__restrict__ pack,
                                                      uint16_t *__restrict__ mask16, float4 *__restrict__ recA,
                                                      float4 *__restrict__ recB, float2 *__restrict__ recC, int exact,
                                                      unsigned long long *__restrict__ bmask) {
    block_masks_body(R, R, gx, keys_sorted, ids_sorted, pack, mask16, recA, recB, recC, exact, blockIdx.x, bmask);
}
// xcd_views = V (1, 2, 4 or 8) on a 1-D grid: a workgroup's XCD is blockIdx.x % 8 and XCD x serves ONLY view x % V.  The list entries of
// a tile gather their Gaussians' 48-byte records in depth order (random), and a Gaussian recurs in the tiles next to and below it -- one
// tile row later, ~2 MB of gathers per view: inside one XCD's 4 MB L2 when that L2 sees one view, outside it when the workgroups of all
// the step's views interleave on every XCD.  xcd_views = 0: blockIdx.y = view.
__global__ __launch_bounds__(256) void k_block_masks_views(P2Table tab, int exact, int xcd_views) {
    int view = blockIdx.y;
    int64_t block = blockIdx.x;
    if (xcd_views > 0) {
        const int xcd = blockIdx.x & 7;
        view = xcd % xcd_views;
        block = (int64_t)(blockIdx.x >> 3) * (8 / xcd_views) + xcd / xcd_views;
    }
    const P2View &w = tab.v[view];
    if (!p2_live(w)) return;
    block_masks_body(w.spec ? (int64_t)w.info[0] : (int64_t)w.R, (int64_t)w.R, w.cam.gx, w.keys_sorted, w.ids_sorted, w.g.pack, w.mask16,
                     w.recA, w.recB, w.recC, exact, block, w.bmask);
}

// The survivors of block `blk` among list positions [lo, hi) of one tile, as a stream of GROUPS OF FOUR that never cross a
// SEG boundary (incomplete groups are padded with -1).  A 64-entry chunk of masks is turned into list positions with one
// ballot + mbcnt and appended to a small ring in LDS (wave-private); group k is ring[4k .. 4k+3], so row r of the wave reads
// its survivor with one ds_read_b32.  All counters are wave-uniform (SGPRs); the mask of the next chunk is prefetched.
constexpr int RING = 128;   // >= 3 groups in flight (12; K7 keeps 2) + one chunk (64) + padding (3)
constexpr int RING16 = 256; // groups of sixteen: 3 x 16 in flight + one chunk + padding (15)
template <int G, int RN>
struct BlockStreamT {
    const uint16_t *m16;     // the tile's masks (already offset by range.x)
    int *ring;
    int cbase, hi, blk, lane, tail;
    uint32_t m_next;
    __device__ __forceinline__ uint32_t load(int base) const { const int e = base + lane; return e < hi ? (uint32_t)m16[e] : 0u; }
    __device__ __forceinline__ void start(const uint16_t *masks, int lo, int hi_, int blk_, int lane_, int *ring_) {
        m16 = masks; hi = hi_; blk = blk_; lane = lane_; ring = ring_; cbase = lo; tail = 0;
        m_next = load(lo);
    }
    // (the caller has already requested the first chunk: first = load(lo))
    __device__ __forceinline__ void start(const uint16_t *masks, int lo, int hi_, int blk_, int lane_, int *ring_, uint32_t first) {
        m16 = masks; hi = hi_; blk = blk_; lane = lane_; ring = ring_; cbase = lo; tail = 0;
        m_next = first;
    }
    __device__ __forceinline__ void ingest() {   // one chunk
        const uint32_t m = m_next;
        m_next = load(cbase + 64);
        const bool hit = (m >> blk) & 1u;
        const unsigned long long cur = __builtin_amdgcn_ballot_w64(hit);
        if (hit) {
            const int rank = (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(cur >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)cur, 0u));
            ring[(tail + rank) & (RN - 1)] = cbase + lane;
        }
        tail += (int)__popcll(cur);
        cbase += 64;
        if ((cbase & (SEG - 1)) == 0 || cbase >= hi) {   // the segment (or the list) ends here: complete the group
            const int pad = (-tail) & (G - 1);
            if (lane < pad) ring[(tail + lane) & (RN - 1)] = -1;
            tail += pad;
        }
    }
    // list position of survivor `slot` of group k (-1 = padding); false when the stream ends before group k
    __device__ __forceinline__ bool group(int k, int slot, int &pos) {
        while (G * k + G > tail && cbase < hi) ingest();
        if (G * k >= tail) return false;
        pos = ring[(G * k + slot) & (RN - 1)];
        return true;
    }
};
typedef BlockStreamT<4, RING> BlockStream;

// The same stream fed from K5b's TRANSPOSED masks (round 4): bmask[chunk][block] is the ballot a wave of BlockStreamT forms from 64 mask
// loads -- here it arrives by ONE scalar load per chunk (two chunks ahead), so the stream issues no vector-memory instruction at all and
// the only loads of K6's loop are the step's records.  Chunks of bmask are aligned to the GLOBAL list index; a tile's list starts at any
// rx, so tile-relative chunk j is bits o.. of word g0 + j joined with bits ..o-1 of word g0 + j + 1 (o = rx & 63: a funnel shift on the
// scalar unit) -- segment boundaries (multiples of 256 tile-relative entries) then fall between chunks as before.
// (the words are read through a CONSTANT-address-space pointer: nothing writes bmask while K6 runs, and only then does the compiler keep
//  the loads on the scalar unit inside the loop -- behind the loop's stores a plain global pointer gets a vector load + v_readfirstlane
//  and an s_waitcnt vmcnt(0) on the spot)
typedef const __attribute__((address_space(4))) unsigned long long *const_u64_ptr;
template <int G, int RN>
struct WordStreamT {
    const_u64_ptr bw;                // word of global chunk g0 for this block; + 16 per chunk
    int *ring;
    int cbase, hi, lane, tail, o, j;
    unsigned long long wa, wb, wc;
    __device__ __forceinline__ void start(const unsigned long long *bmask, uint32_t rx, int hi_, int blk, int lane_, int *ring_) {
        bw = (const_u64_ptr)(bmask + ((size_t)(rx >> 6) * 16 + (size_t)blk));
        o = (int)(rx & 63u); hi = hi_; lane = lane_; ring = ring_; cbase = 0; tail = 0; j = 0;
        wa = bw[0]; wb = bw[16]; wc = bw[32];
    }
    __device__ __forceinline__ void ingest() {   // one tile-relative chunk
        unsigned long long cur = o ? (wa >> o) | (wb << (64 - o)) : wa;
        const int rem = hi - cbase;
        if (rem < 64) cur &= (1ull << rem) - 1ull;
        wa = wb; wb = wc; j++;
        wc = bw[(size_t)(j + 2) * 16];
        if (__builtin_amdgcn_inverse_ballot_w64(cur)) {
            const int rank = (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(cur >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)cur, 0u));
            ring[(tail + rank) & (RN - 1)] = cbase + lane;
        }
        tail += (int)__popcll(cur);
        cbase += 64;
        if ((cbase & (SEG - 1)) == 0 || cbase >= hi) {   // the segment (or the list) ends here: complete the group
            const int pad = (-tail) & (G - 1);
            if (lane < pad) ring[(tail + lane) & (RN - 1)] = -1;
            tail += pad;
        }
    }
    // list position of survivor `slot` of group k (-1 = padding, and -1 with `false` when the stream ends before group k)
    __device__ __forceinline__ bool group(int k, int slot, int &pos) {
        while (G * k + G > tail && cbase < hi) ingest();
        const bool ok = G * k < tail;
        pos = ok ? ring[(G * k + slot) & (RN - 1)] : -1;
        return ok;
    }
};

struct Trip { float4 a, b; float2 c; int pos; uint32_t id; };   // the lane's survivor of a group (row r's), pos = list position or -1
struct TripF { float4 a, b; float2 c; int pos; uint32_t id; float wf; };   // (K7's feature path) + sum_c gf_c f_c of the survivor at the pixel

// ---- which entries a block BLENDED (round 4).  K5b's masks say which entries can REACH a 4x4 block (ellipse vs box); K6 finds out which
// of them any pixel of the block actually blends -- alpha >= 1/255 at some pixel centre that is still open -- and K7 only ever does
// arithmetic for those: a survivor that no pixel blended has factor 1 and addend 0 at all sixteen pixels (bit for bit: same exp, same
// tests), so dropping it changes no bit of T, S or any gradient.  K6 marks a blended survivor with ONE BIT in a 256-bit LDS strip (the
// segment's list positions); when its walk leaves a segment the strip is stored as four 64-bit words bbits[slot][block][0..3] -- the
// TRANSPOSE of mask16 restricted to what was blended -- and K7's waves read their segment's survivor set with one scalar 32-byte load
// instead of four vector loads of masks + ballots.  Segments a block's walk skipped (no survivor) get zero words; K7 never looks behind
// the block's last blended entry (blk_hi).
// (the strip is kept as 8 x 32 BITS, set with ds_or_b32: the flush is then one LDS read and one 4-byte store by eight lanes -- ballots
// over a byte strip, four 64-bit selects and their addresses cost the survivor-column K6 22 VGPRs at the flush point, i.e. its fifth wave)
__device__ __forceinline__ void bbits_mark(uint32_t *s_bits, int pos) { atomicOr(&s_bits[(pos & (SEG - 1)) >> 5], 1u << (pos & 31)); }
__device__ __forceinline__ void bbits_flush(uint32_t *s_bits, unsigned long long *__restrict__ bbits, size_t slot, int blk, int lane) {
    if (lane < SEG / 32) {
        reinterpret_cast<uint32_t *>(bbits)[(slot * 16 + (size_t)blk) * (SEG / 32) + lane] = s_bits[lane];
        s_bits[lane] = 0u;
    }
}
__device__ __forceinline__ void bbits_zero(unsigned long long *__restrict__ bbits, size_t slot, int blk, int lane) {
    if (lane < SEG / 32) reinterpret_cast<uint32_t *>(bbits)[(slot * 16 + (size_t)blk) * (SEG / 32) + lane] = 0u;
}

// ------------------------------------------------------------------------------------------- K6
// grid: 16 single-wave workgroups per tile; the 16 blocks of a tile have the same blockIdx % 8 (same XCD, shared L2 lines)
__device__ __forceinline__ void composite_fwd_body(int tiles, int W, int H, int gx, const int2 *__restrict__ ranges,
                                                   const uint16_t *__restrict__ mask16, const float4 *__restrict__ recA,
                                                   const float4 *__restrict__ recB, const float2 *__restrict__ recC,
                                                   uint32_t null_rec, const float *__restrict__ bg,
                                                   int *seg_offset, float4 *__restrict__ ckpt,
                                                   float *__restrict__ final_T, uint32_t *__restrict__ n_contrib,
                                                   float *__restrict__ out_color, float *__restrict__ out_depth, int wg,
                                                   unsigned long long *__restrict__ bbits,
                                                   const uint32_t *__restrict__ order = nullptr) {
    __shared__ int s_ring[RING];
    __shared__ uint32_t s_hit[SEG / 32];
    // item (wg >> 7) * 8 + (wg & 7), block (wg >> 3) & 15: the 16 blocks of an item share blockIdx % 8 (one XCD).  order: a permutation
    // of the tiles, longest list first, the empty tiles (background only) last (k_tile_scan)
    const int item = ((wg >> 7) << 3) + (wg & 7), blk = (wg >> 3) & 15;
    if (item >= tiles) return;
    const int tile = order ? (int)order[item] : item;
    const int lane = threadIdx.x, r = lane >> 4, l16 = lane & 15;
    const int px = (tile % gx) * CSPLAT_TILE + (blk & 3) * 4 + (l16 & 3);
    const int py = (tile / gx) * CSPLAT_TILE + (blk >> 2) * 4 + (l16 >> 2);
    const bool inside = px < W && py < H;
    const int pix = py * W + px;
    const float fx = (float)px, fy = (float)py;
    const int2 range = ranges[tile];
    const int n = range.y - range.x;
    const uint32_t rx = (uint32_t)range.x;
    bool done = !inside;
    float T = 1.f, C0 = 0.f, C1 = 0.f, C2 = 0.f, Dp = 0.f;   // T: the pixel's (same in its 4 lanes); C*, Dp: this row's share
    uint32_t last = 0;
    if (n > 0 && __builtin_amdgcn_ballot_w64(!done) != 0ull) {
        const int seg0 = seg_offset[tile];
        BlockStream st;
        st.start(mask16 + rx, 0, n, blk, lane, s_ring);
        int seg_written = -1;
        if (lane < SEG / 32) s_hit[lane] = 0u;
        auto fetch = [&](Trip &t, int k) -> bool {
            if (!st.group(k, r, t.pos)) return false;
            const uint32_t ri = t.pos >= 0 ? rx + (uint32_t)t.pos : null_rec;
            t.a = recA[ri]; t.b = recB[ri]; t.c = recC[ri];
            return true;
        };
        auto process = [&](const Trip &t) {
            const int seg = __builtin_amdgcn_readfirstlane(t.pos) / SEG;   // (a group's first entry is never padding)
            if (seg != seg_written) {
                // entering a new 256-entry segment: checkpoint (T, colour so far) for the depth-split backward, for every
                // segment start passed since the last one (segments without a survivor of this block get the same state)
                const float t0 = rows_sum(C0), t1 = rows_sum(C1), t2 = rows_sum(C2);
                if (r == 0)
                    for (int s = seg_written + 1; s <= seg; s++)
                        ckpt[(size_t)(seg0 + s) * 256 + blk * 16 + l16] = make_float4(T, t0, t1, t2);
                C0 = r == 0 ? t0 : 0.f; C1 = r == 0 ? t1 : 0.f; C2 = r == 0 ? t2 : 0.f;
                if (seg_written >= 0) bbits_flush(s_hit, bbits, (size_t)(seg0 + seg_written), blk, lane);
                for (int s = seg_written + 1; s < seg; s++) bbits_zero(bbits, (size_t)(seg0 + s), blk, lane);
                seg_written = seg;
            }
            const float dx = t.a.x - fx, dy = t.a.y - fy;
            const float power = -0.5f * (t.a.z * dx * dx + t.b.x * dy * dy) - t.a.w * dx * dy;
            const float a = fminf(0.99f, t.b.y * __expf(power));
            const float al = (!done && power <= 0.f && a >= ALPHA_MIN) ? a : 0.f;
            const float F = 1.f - al;
            const Row4 g = rows_allgather(F);
            const float P1 = T * g.v0, P2 = P1 * g.v1, P3 = P2 * g.v2, P4 = P3 * g.v3;
            const float Tr = rowsel(r, T, P1, P2, P3);
            const bool blend = al > 0.f && Tr * F >= T_EPS;     // (Tr * F is this row's P_{r+1}, bit for bit)
            const float wgt = blend ? al * Tr : 0.f;
            C0 += t.b.z * wgt; C1 += t.b.w * wgt; C2 += t.c.x * wgt; Dp += t.c.y * wgt;
            last = blend ? (uint32_t)(t.pos + 1) : last;
            {   // the row's survivor was blended at one of its 16 pixels: its byte in the segment's strip
                const unsigned long long bal = __builtin_amdgcn_ballot_w64(blend);
                if (l16 == 0 && ((bal >> (lane & 48)) & 0xFFFFull) != 0ull) bbits_mark(s_hit, t.pos);
            }
            // the products only decrease: the pixel's T after the group is the last one still above the threshold
            T = P4 >= T_EPS ? P4 : (P3 >= T_EPS ? P3 : (P2 >= T_EPS ? P2 : (P1 >= T_EPS ? P1 : T)));
            done = done || !(P4 >= T_EPS);
        };
        // software pipeline, three groups in flight: the records of group k+3 are requested when group k has been composited
        Trip ta, tb, tc;
        bool va = fetch(ta, 0), vb = fetch(tb, 1), vc = fetch(tc, 2);
        int k = 3;
        while (va) {
            process(ta);
            if (__builtin_amdgcn_ballot_w64(!done) == 0ull) break;
            va = fetch(ta, k++);
            if (!vb) break;
            process(tb);
            if (__builtin_amdgcn_ballot_w64(!done) == 0ull) break;
            vb = fetch(tb, k++);
            if (!vc) break;
            process(tc);
            if (__builtin_amdgcn_ballot_w64(!done) == 0ull) break;
            vc = fetch(tc, k++);
        }
        if (seg_written >= 0) bbits_flush(s_hit, bbits, (size_t)(seg0 + seg_written), blk, lane);
    }
    C0 = rows_sum(C0); C1 = rows_sum(C1); C2 = rows_sum(C2); Dp = rows_sum(Dp);
    {
        const Row4 g = rows_allgather(__uint_as_float(last));
        last = max(max(__float_as_uint(g.v0), __float_as_uint(g.v1)), max(__float_as_uint(g.v2), __float_as_uint(g.v3)));
    }
    {   // the block's largest n_contrib, for K7's workgroups (seg_offset[tiles + 1 ...] = blk_hi[tile][blk])
        uint32_t m = inside ? last : 0u;
#pragma unroll
        for (int o = 1; o < 16; o <<= 1) m = max(m, (uint32_t)__shfl_xor((int)m, o, 64));
        if (lane == 0) reinterpret_cast<uint32_t *>(seg_offset)[tiles + 1 + tile * 16 + blk] = m;
    }
    if (inside && r == 0) {
        final_T[pix] = T;
        n_contrib[pix] = last;
        const size_t HW = (size_t)H * W;
        out_color[pix] = C0 + T * bg[0];
        out_color[HW + pix] = C1 + T * bg[1];
        out_color[2 * HW + pix] = C2 + T * bg[2];
        out_depth[pix] = Dp;
    }
}
template <int CTRL>
__device__ __forceinline__ float dpp_add(float v) {
    return v + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, false));
}
// One level of a row scan (x[lane] op= x[lane - N] inside every DPP row of 16; lanes without a source keep their value) for FOUR
// independent registers at once: the four instructions are independent, so three of them cover the two wait states a DPP read
// needs after a VALU write of the same register (FIRST: the registers were last written by ordinary VALU code -> s_nop 1).
#define CSPLAT_ROW_SCAN4(OP, N, FIRST, a, b, c, d)                                                                                  \
    asm(FIRST "v_" OP "_f32_dpp %0, %0, %0 row_shr:" #N " row_mask:0xf bank_mask:0xf\n\t"                                          \
              "v_" OP "_f32_dpp %1, %1, %1 row_shr:" #N " row_mask:0xf bank_mask:0xf\n\t"                                          \
              "v_" OP "_f32_dpp %2, %2, %2 row_shr:" #N " row_mask:0xf bank_mask:0xf\n\t"                                          \
              "v_" OP "_f32_dpp %3, %3, %3 row_shr:" #N " row_mask:0xf bank_mask:0xf"                                               \
        : "+v"(a), "+v"(b), "+v"(c), "+v"(d))
__device__ __forceinline__ void row_scan4_mul(float (&x)[4]) {
    CSPLAT_ROW_SCAN4("mul", 1, "s_nop 1\n\t", x[0], x[1], x[2], x[3]);
    CSPLAT_ROW_SCAN4("mul", 2, "", x[0], x[1], x[2], x[3]);
    CSPLAT_ROW_SCAN4("mul", 4, "", x[0], x[1], x[2], x[3]);
    CSPLAT_ROW_SCAN4("mul", 8, "", x[0], x[1], x[2], x[3]);
}
__device__ __forceinline__ void row_scan4_add(float (&x)[4]) {
    CSPLAT_ROW_SCAN4("add", 1, "s_nop 1\n\t", x[0], x[1], x[2], x[3]);
    CSPLAT_ROW_SCAN4("add", 2, "", x[0], x[1], x[2], x[3]);
    CSPLAT_ROW_SCAN4("add", 4, "", x[0], x[1], x[2], x[3]);
    CSPLAT_ROW_SCAN4("add", 8, "", x[0], x[1], x[2], x[3]);
}
// ------------------------------------------------------------------------------------------- K6, survivor-column form (round 3)
// The lane mapping of composite_bwd16_body for the forward: a step takes SIXTEEN consecutive survivors of the block, lane l holds
// survivor l & 15 and the four pixels of block row l >> 4.  The transmittance of a pixel in front of every survivor is a 4-level
// row_shr product scan along its DPP row (+ one shift, one row_newbcast) instead of an all-gather of four factors + a row select per
// group of four, a lane accumulates colour and depth for ITS survivor only (summed over the row's lanes once per tile and at the
// segment checkpoints), and the serial chain a wave walks -- what bounds this kernel: one wave per block goes through the whole
// tile list -- is a quarter as many steps long.  The products of a step associate as a scan tree, not front to back: final_T and the
// alpha / transmittance decisions can differ from a sequential walk in the last bit (the tests hold n_contrib to the oracle up to
// counted threshold ties and final_T to 1e-4, as they do for v_exp_f32 against expf).  Measured (profiles/r03*): 45 %
// fewer VALU instructions than the row form (composite_fwd_body) but 96-106 VGPRs against 62, i.e. 4-5 waves per SIMD against 8.  While
// the launch still handed 16 waves to every empty tile it lost (188-197 us against 182 us for the four views of a step); launched for
// the non-empty tiles only -- ~17 k long waves for 8192 slots, where the length of a wave is what counts and not how many fit -- it
// wins: 137 against 158 us.  It is the DEFAULT; csplat_debug_flags bit 15 selects the row form.
__device__ __forceinline__ void row_scan4_min(float (&x)[4]) {
    CSPLAT_ROW_SCAN4("min", 1, "s_nop 1\n\t", x[0], x[1], x[2], x[3]);
    CSPLAT_ROW_SCAN4("min", 2, "", x[0], x[1], x[2], x[3]);
    CSPLAT_ROW_SCAN4("min", 4, "", x[0], x[1], x[2], x[3]);
    CSPLAT_ROW_SCAN4("min", 8, "", x[0], x[1], x[2], x[3]);
}
// sum over the 16 lanes of every DPP row, result in all of them
__device__ __forceinline__ float row_total(float v) {
    v = dpp_add<0xB1>(v); v = dpp_add<0x4E>(v); v = dpp_add<0x141>(v); v = dpp_add<0x140>(v);
    return v;
}
__device__ __forceinline__ void composite_fwd16_body(int tiles, int W, int H, int gx, const int2 *__restrict__ ranges,
                                                     const uint16_t *__restrict__ mask16, const float4 *__restrict__ recA,
                                                     const float4 *__restrict__ recB, const float2 *__restrict__ recC,
                                                     uint32_t null_rec, const float *__restrict__ bg,
                                                     int *seg_offset, float4 *__restrict__ ckpt,
                                                     float *__restrict__ final_T, uint32_t *__restrict__ n_contrib,
                                                     float *__restrict__ out_color, float *__restrict__ out_depth,
                                                     unsigned long long *__restrict__ bbits,
                                                     const unsigned long long *__restrict__ bmask,
                                                     const uint32_t *__restrict__ order = nullptr) {
    __shared__ int s_ring[RING16];
    __shared__ uint32_t s_hit[SEG / 32];
    const int wg = blockIdx.x;
    const int item = ((wg >> 7) << 3) + (wg & 7), blk = (wg >> 3) & 15;
    if (item >= tiles) return;
    const int tile = order ? (int)order[item] : item;
    const int lane = threadIdx.x, sv = lane & 15, q = lane >> 4;
    const int px0 = (tile % gx) * CSPLAT_TILE + (blk & 3) * 4;
    const int py = (tile / gx) * CSPLAT_TILE + (blk >> 2) * 4 + q;
    const float fy = (float)py;
    const int2 range = ranges[tile];
    const int n = range.y - range.x;
    const uint32_t rx = (uint32_t)range.x;
    // A pixel that is DONE (outside the image, or its walk has ended: T fell below 1e-4) keeps working transmittance 0 -- every weight it
    // forms is 0 by arithmetic, no select -- and its final T waits in s_Tend; which pixels are done is a LANE MASK per pixel column
    // (m_done[j], an SGPR pair: the decisions of a step are scalar-unit logic on compare results, selects take the masks directly).
    __shared__ float s_Tend[16];
    bool inside[4];
    unsigned long long m_done[4];
    float T[4], C0[4], C1[4], C2[4], Dp[4], fx[4];
    uint32_t last[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
        inside[j] = px0 + j < W && py < H;
        m_done[j] = __builtin_amdgcn_ballot_w64(!inside[j]);
        T[j] = inside[j] ? 1.f : 0.f; C0[j] = C1[j] = C2[j] = Dp[j] = 0.f;      // T: the pixel's (same in its 16 lanes); C*, Dp: this lane's survivors' share
        last[j] = 0u;
        fx[j] = (float)(px0 + j);
    }
    int seg0 = 0, seg_written = -1;
    if (n > 0 && (m_done[0] & m_done[1] & m_done[2] & m_done[3]) != ~0ull) {
        seg0 = seg_offset[tile];
        WordStreamT<16, RING16> st;
        st.start(bmask, rx, n, blk, lane, s_ring);
        if (lane < SEG / 32) s_hit[lane] = 0u;
        // (the three loads are issued whether or not the stream still has a step: s_waitcnt vmcnt counts in order, and a load the
        //  compiler must assume was NOT issued makes it wait for the youngest ones -- see K7's loop)
        auto fetch = [&](Trip &t, int k) -> bool {
            const bool ok = st.group(k, sv, t.pos);
            const uint32_t ri = t.pos >= 0 ? rx + (uint32_t)t.pos : null_rec;
            t.a = recA[ri]; t.b = recB[ri]; t.c = recC[ri];
            return ok;
        };
        auto process = [&](const Trip &t) {
            const int seg = __builtin_amdgcn_readfirstlane(t.pos) / SEG;   // (a group's first entry is never padding)
            if (seg != seg_written) {
                // entering a new 256-entry segment: checkpoint (T, colour so far) of every pixel for the depth-split backward, for
                // every segment start passed since the last one.  The colour so far is spread over the row's lanes: sum it, keep
                // the total in lane 0 of the row
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    const float t0 = row_total(C0[j]), t1 = row_total(C1[j]), t2 = row_total(C2[j]);
                    if (sv == 0)
                        for (int s_ = seg_written + 1; s_ <= seg; s_++)
                            ckpt[(size_t)(seg0 + s_) * 256 + blk * 16 + q * 4 + j] = make_float4(T[j], t0, t1, t2);
                    C0[j] = sv == 0 ? t0 : 0.f; C1[j] = sv == 0 ? t1 : 0.f; C2[j] = sv == 0 ? t2 : 0.f;
                }
                if (seg_written >= 0) bbits_flush(s_hit, bbits, (size_t)(seg0 + seg_written), blk, lane);
                for (int s_ = seg_written + 1; s_ < seg; s_++) bbits_zero(bbits, (size_t)(seg0 + s_), blk, lane);
                seg_written = seg;
            }
            const float dy = t.a.y - fy;
            float al[4], inc[4];
            unsigned long long m_live[4];
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const float dx = t.a.x - fx[j];
                const float power = -0.5f * (t.a.z * dx * dx + t.b.x * dy * dy) - t.a.w * dx * dy;
                const float a = fminf(0.99f, t.b.y * __expf(power));
                m_live[j] = __builtin_amdgcn_ballot_w64(power <= 0.f) & __builtin_amdgcn_ballot_w64(a >= ALPHA_MIN);
                al[j] = __builtin_amdgcn_inverse_ballot_w64(m_live[j]) ? a : 0.f;
                inc[j] = 1.f - al[j];
            }
            row_scan4_mul(inc);                                          // the pixel's factor up to and including every survivor
            float Tr[4], P[4], Pend[4];
#pragma unroll
            for (int j = 0; j < 4; j++) { Tr[j] = T[j]; P[j] = T[j] * inc[j]; }
            // transmittance in front of the lane's survivor (T x the scan of the lane to the left; survivor 0 of the row keeps T) and
            // behind the step's last survivor (row_newbcast:15)
            asm("s_nop 1\n\t"
                "v_mul_f32_dpp %0, %4, %0 row_shr:1 row_mask:0xf bank_mask:0xf\n\t"
                "v_mul_f32_dpp %1, %5, %1 row_shr:1 row_mask:0xf bank_mask:0xf\n\t"
                "v_mul_f32_dpp %2, %6, %2 row_shr:1 row_mask:0xf bank_mask:0xf\n\t"
                "v_mul_f32_dpp %3, %7, %3 row_shr:1 row_mask:0xf bank_mask:0xf"
                : "+v"(Tr[0]), "+v"(Tr[1]), "+v"(Tr[2]), "+v"(Tr[3]) : "v"(inc[0]), "v"(inc[1]), "v"(inc[2]), "v"(inc[3]));
            asm("s_nop 1\n\t"
                "v_mov_b32_dpp %0, %4 row_newbcast:15 row_mask:0xf bank_mask:0xf\n\t"
                "v_mov_b32_dpp %1, %5 row_newbcast:15 row_mask:0xf bank_mask:0xf\n\t"
                "v_mov_b32_dpp %2, %6 row_newbcast:15 row_mask:0xf bank_mask:0xf\n\t"
                "v_mov_b32_dpp %3, %7 row_newbcast:15 row_mask:0xf bank_mask:0xf"
                : "=&v"(Pend[0]), "=&v"(Pend[1]), "=&v"(Pend[2]), "=&v"(Pend[3]) : "v"(P[0]), "v"(P[1]), "v"(P[2]), "v"(P[3]));
            unsigned long long m_end[4], any_end = 0ull, m_bl = 0ull;
#pragma unroll
            for (int j = 0; j < 4; j++) {
                m_end[j] = __builtin_amdgcn_ballot_w64(!(Pend[j] >= T_EPS)) & ~m_done[j];       // the pixel's walk ends inside this step
                any_end |= m_end[j];
            }
            if (any_end == 0ull) {
                // no pixel of the block ends in this step: every product of an open pixel is above the threshold (they only decrease
                // along the row), so a survivor is blended exactly where its alpha passed -- and a done pixel's weight is 0 x anything
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    const float wgt = al[j] * Tr[j];
                    C0[j] += t.b.z * wgt; C1[j] += t.b.w * wgt; C2[j] += t.c.x * wgt; Dp[j] += t.c.y * wgt;
                    const unsigned long long mb = m_live[j] & ~m_done[j];
                    m_bl |= mb;
                    last[j] = __builtin_amdgcn_inverse_ballot_w64(mb) ? (uint32_t)(t.pos + 1) : last[j];
                    T[j] = Pend[j];
                }
            } else {
                float cand[4];
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    const unsigned long long mb = m_live[j] & ~m_done[j] & __builtin_amdgcn_ballot_w64(P[j] >= T_EPS);
                    m_bl |= mb;
                    const float wgt = __builtin_amdgcn_inverse_ballot_w64(mb) ? al[j] * Tr[j] : 0.f;
                    C0[j] += t.b.z * wgt; C1[j] += t.b.w * wgt; C2[j] += t.c.x * wgt; Dp[j] += t.c.y * wgt;
                    last[j] = __builtin_amdgcn_inverse_ballot_w64(mb) ? (uint32_t)(t.pos + 1) : last[j];
                    // the T an ending pixel keeps: the last product above the threshold (the products only decrease) = the row's smallest candidate
                    cand[j] = __builtin_amdgcn_inverse_ballot_w64(m_end[j]) ? (P[j] >= T_EPS ? P[j] : T[j]) : 3.0e38f;
                }
                row_scan4_min(cand);
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    const float mend = dpp_mov<0x15F, 0xF>(cand[j], cand[j]);
                    const bool ended = __builtin_amdgcn_inverse_ballot_w64(m_end[j]);
                    if (ended && sv == 0) s_Tend[q * 4 + j] = mend;
                    m_done[j] |= m_end[j];
                    T[j] = __builtin_amdgcn_inverse_ballot_w64(m_done[j]) ? 0.f : Pend[j];
                }
            }
            {   // survivor sv was blended at one of the block's 16 pixels (its four lanes, four pixels each): its bit in the strip
                const uint32_t any16 = (uint32_t)(m_bl | (m_bl >> 16) | (m_bl >> 32) | (m_bl >> 48)) & 0xFFFFu;
                if (lane < 16 && ((any16 >> lane) & 1u)) bbits_mark(s_hit, t.pos);
            }
        };
        // software pipeline, two steps in flight (a step is ~16 survivors x 4 pixels of arithmetic: one step ahead covers the fetch)
        Trip ta, tb;
        bool va = fetch(ta, 0), vb = fetch(tb, 1);
        int k = 2;
        auto all_done = [&]() { return (m_done[0] & m_done[1] & m_done[2] & m_done[3]) == ~0ull; };
        while (va) {
            process(ta);
            if (all_done()) break;
            va = fetch(ta, k++);
            if (!vb) break;
            process(tb);
            if (all_done()) break;
            vb = fetch(tb, k++);
        }
    }
#pragma unroll
    for (int j = 0; j < 4; j++)         // the pixels whose walk ended: the transmittance they kept
        if (inside[j] && __builtin_amdgcn_inverse_ballot_w64(m_done[j])) T[j] = s_Tend[q * 4 + j];
    uint32_t hi_ = 0u;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        C0[j] = row_total(C0[j]); C1[j] = row_total(C1[j]); C2[j] = row_total(C2[j]); Dp[j] = row_total(Dp[j]);
        uint32_t m = last[j];
#pragma unroll
        for (int o = 1; o < 16; o <<= 1) m = max(m, (uint32_t)__shfl_xor((int)m, o, 64));
        last[j] = m;
        hi_ = max(hi_, inside[j] ? m : 0u);
    }
    {   // the block's largest n_contrib, for K7's workgroups (seg_offset[tiles + 1 ...] = blk_hi[tile][blk])
#pragma unroll
        for (int o = 16; o < 64; o <<= 1) hi_ = max(hi_, (uint32_t)__shfl_xor((int)hi_, o, 64));
        if (lane == 0) reinterpret_cast<uint32_t *>(seg_offset)[tiles + 1 + tile * 16 + blk] = hi_;
    }
    if (sv < 4) {   // lane j of every row writes pixel j of that row
        const size_t HW = (size_t)H * W;
        float t_ = T[0], c0 = C0[0], c1 = C1[0], c2 = C2[0], dp = Dp[0];
        uint32_t la = last[0];
        bool in_ = inside[0];
#pragma unroll
        for (int j = 1; j < 4; j++)
            if (sv == j) { t_ = T[j]; c0 = C0[j]; c1 = C1[j]; c2 = C2[j]; dp = Dp[j]; la = last[j]; in_ = inside[j]; }
        if (in_) {
            const int pix = py * W + px0 + sv;
            final_T[pix] = t_;
            n_contrib[pix] = la;
            out_color[pix] = c0 + t_ * bg[0];
            out_color[HW + pix] = c1 + t_ * bg[1];
            out_color[2 * HW + pix] = c2 + t_ * bg[2];
            out_depth[pix] = dp;
        }
    }
    // (the last segment's strip leaves here, where nothing else is live: flushed right behind the loop it cost the kernel 18 VGPRs)
    if (seg_written >= 0) bbits_flush(s_hit, bbits, (size_t)(seg0 + seg_written), blk, lane);
}
template <bool ROWS>
__global__ __launch_bounds__(64) void k_composite_fwd(int tiles, int W, int H, int gx, const int2 *__restrict__ ranges,
                                                       const uint16_t *__restrict__ mask16, const float4 *__restrict__ recA,
                                                       const float4 *__restrict__ recB, const float2 *__restrict__ recC,
                                                       uint32_t null_rec, const float *__restrict__ bg,
                                                       int *seg_offset, float4 *__restrict__ ckpt,
                                                       float *__restrict__ final_T, uint32_t *__restrict__ n_contrib,
                                                       float *__restrict__ out_color, float *__restrict__ out_depth,
                                                       unsigned long long *__restrict__ bbits,
                                                       const unsigned long long *__restrict__ bmask) {
    if (ROWS)
        composite_fwd_body(tiles, W, H, gx, ranges, mask16, recA, recB, recC, null_rec, bg, seg_offset, ckpt, final_T, n_contrib, out_color,
                           out_depth, (int)blockIdx.x, bbits);
    else
        composite_fwd16_body(tiles, W, H, gx, ranges, mask16, recA, recB, recC, null_rec, bg, seg_offset, ckpt, final_T, n_contrib, out_color,
                             out_depth, bbits, bmask);
}
// the waves behind the first busy_grid of a K6 launch: the tiles of the launch-order list that got no waves of their own -- the empty
// ones -- receive what K6 writes for a tile without a list (background colour, T = 1, no contributor, blk_hi = 0), 256 pixels a pass
constexpr int K6_EXTRA = 256;
__device__ __forceinline__ void paint_empty_tiles(int tiles, int W, int H, int gx, const uint32_t *__restrict__ order, int busy_grid,
                                                  const float *__restrict__ bg, int *seg_offset, float *__restrict__ final_T,
                                                  uint32_t *__restrict__ n_contrib, float *__restrict__ out_color,
                                                  float *__restrict__ out_depth) {
    const int lane = threadIdx.x;
    const size_t HW = (size_t)H * W;
    const float b0 = bg[0], b1 = bg[1], b2 = bg[2];
    uint32_t *blk_hi = reinterpret_cast<uint32_t *>(seg_offset) + tiles + 1;
    for (int pos = (busy_grid >> 7 << 3) + ((int)blockIdx.x - busy_grid); pos < tiles; pos += (int)gridDim.x - busy_grid) {
        const int tile = (int)order[pos];
        if (lane < 16) blk_hi[tile * 16 + lane] = 0u;
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const int px = (tile % gx) * CSPLAT_TILE + (lane & 15), py = (tile / gx) * CSPLAT_TILE + 4 * q + (lane >> 4);
            if (px < W && py < H) {
                const int pix = py * W + px;
                final_T[pix] = 1.f;
                n_contrib[pix] = 0u;
                out_color[pix] = b0; out_color[HW + pix] = b1; out_color[2 * HW + pix] = b2;
                out_depth[pix] = 0.f;
            }
        }
    }
}
// blockIdx.x < busy_grid: one wave per (item, block) of the first busy_grid / 16 entries of the launch-order list (the non-empty tiles,
// longest list first: every one of them is among the entries, p2_live: info[2] <= Bcap); the waves behind paint what is left of the list,
// the empty tiles.  (Round 3 measured the alternatives that left the library in round 4: 16 waves for every tile in tile order, and
// 1024 n persistent waves per view walking the items -- DESIGN section 6.)
template <bool ROWS>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(5))) void k_composite_fwd_views(int tiles, int W, int H, P2Table tab, int busy_grid) {
    if (tab.valid && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) {
        // the verdict of a launch on faith (csplat_forward_views_faith): every view's counts fitted the capacities its second phase was
        // laid out for -- what the backward's kernels and the optimizer step read before they touch anything
        bool ok = true;
        for (int i = 0; i < tab.nviews; i++) ok = ok && p2_live(tab.v[i]);
        *tab.valid = ok ? 1u : 0u;
    }
    const P2View &w = tab.v[blockIdx.y];
    if (!p2_live(w)) return;
    const uint32_t *order = w.info + INFO_BUSY + tiles + 4;
    if ((int)blockIdx.x >= busy_grid) {
        paint_empty_tiles(tiles, W, H, w.cam.gx, order, busy_grid, w.bg, w.seg_offset, w.final_T, w.n_contrib, w.out_color, w.out_depth);
        return;
    }
    if (ROWS)
        composite_fwd_body(tiles, W, H, w.cam.gx, w.ranges, w.mask16, w.recA, w.recB, w.recC, w.R, w.bg, w.seg_offset, w.ckpt, w.final_T,
                           w.n_contrib, w.out_color, w.out_depth, (int)blockIdx.x, w.bbits, order);
    else
        composite_fwd16_body(tiles, W, H, w.cam.gx, w.ranges, w.mask16, w.recA, w.recB, w.recC, w.R, w.bg, w.seg_offset, w.ckpt, w.final_T,
                             w.n_contrib, w.out_color, w.out_depth, w.bbits, w.bmask, order);
}

}  // namespace
