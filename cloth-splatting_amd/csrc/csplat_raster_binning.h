// csplat_raster_binning.h -- part of csplat_raster.hip, included there once, behind csplat_raster_k1.h.
// From Gaussians to sorted tile lists: K3 (k_emit_keys), K5 (k_tile_ranges), the tile-bucketed path (k_tile_count, k_tile_colscan,
// k_tile_scan, k_emit_bucket, k_tile_sort, each with its _views form), box_hit and the segment plan (k_seg_plan*).
// Uses from csplat_raster_math.h: Cam, Geom, RASTER_MAX_VIEWS, tile_rect; from csplat_raster_k1.h: K1View, K1Table.
// Defines CSPLAT_SEG (unless the build line did: build.sh -DCSPLAT_SEG=...) and leaves it defined; its one reader is SEG, here.  SEG itself
// is read by every part behind this one except csplat_raster_k8.h, and by the host code of csplat_raster.hip.
#pragma once

namespace {

// ------------------------------------------------------------------------------------------- K3
__global__ __launch_bounds__(256) void k_emit_keys(int P, const float2 *__restrict__ xy, const float *__restrict__ depth,
                                                    const uint32_t *__restrict__ offsets,
                                                    const int32_t *__restrict__ radii, Cam cam,
                                                    uint64_t *__restrict__ keys, uint32_t *__restrict__ ids) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P) return;
    const int rad = radii[i];
    if (rad <= 0) return;
    uint32_t off = (i == 0) ? 0u : offsets[i - 1];
    const float2 p = xy[i];
    int minx, miny, maxx, maxy;
    tile_rect(p.x, p.y, rad, cam, minx, miny, maxx, maxy);
    const uint32_t dbits = __float_as_uint(depth[i]);
    for (int y = miny; y < maxy; y++)
        for (int x = minx; x < maxx; x++) {
            keys[off] = ((uint64_t)(uint32_t)(y * cam.gx + x) << 32) | dbits;
            ids[off] = (uint32_t)i;
            off++;
        }
}

// ------------------------------------------------------------------------------------------- K5
__global__ __launch_bounds__(256) void k_tile_ranges(int64_t R, const uint64_t *__restrict__ keys, int2 *__restrict__ ranges) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= R) return;
    const uint32_t t = (uint32_t)(keys[i] >> 32);
    if (i == 0) ranges[t].x = 0;
    else {
        const uint32_t tp = (uint32_t)(keys[i - 1] >> 32);
        if (tp != t) { ranges[tp].y = (int)i; ranges[t].x = (int)i; }
    }
    if (i == R - 1) ranges[t].y = (int)R;
}

// ---- tile-bucketed binning (default path) ------------------------------------------------------------------------
// One MSD "radix" pass whose digit is the tile id, without any global atomic:
//   k_tile_count   workgroup b (1024 Gaussians) histograms its instances per tile in LDS -> table[b][tile]
//   k_tile_colscan per tile: exclusive scan over the workgroups, in place (each workgroup's offset inside the tile's list)
//   k_tile_scan    exclusive scan of the per-tile totals: tile ranges, R and the longest list
//   k_emit_bucket  workgroup b reloads its bases into LDS and drops every instance at base[tile]++ (LDS atomic)
//   k_tile_sort    each tile's list ordered by (depth bits, Gaussian id) with a stable LSD radix sort in LDS + registers.
//                  The composite key is unique, so the result is exactly the stable (tile | depth) radix order of the
//                  upstream pipeline.
constexpr int BUCKET_CAP = 8192;    // longest tile list the LDS sort takes (64 KB); longer lists -> global radix sort
constexpr int BUCKET_TILES = 12288; // most tiles the per-workgroup LDS histogram takes (48 KB)
constexpr int BUCKET_G = 1024;      // Gaussians per counting workgroup

__device__ __forceinline__ void tile_count_body(int P, int tiles, const float2 *__restrict__ xy,
                                                const int32_t *__restrict__ radii, const Cam &cam,
                                                uint32_t *__restrict__ table) {
    extern __shared__ uint32_t s_hist[];
    for (int t = threadIdx.x; t < tiles; t += BUCKET_G) s_hist[t] = 0u;
    __syncthreads();
    const int i = blockIdx.x * BUCKET_G + threadIdx.x;
    if (i < P) {
        const int rad = radii[i];
        if (rad > 0) {
            const float2 p = xy[i];
            int minx, miny, maxx, maxy;
            tile_rect(p.x, p.y, rad, cam, minx, miny, maxx, maxy);
            for (int y = miny; y < maxy; y++)
                for (int x = minx; x < maxx; x++) atomicAdd(&s_hist[y * cam.gx + x], 1u);
        }
    }
    __syncthreads();
    uint32_t *row = table + (size_t)blockIdx.x * tiles;
    for (int t = threadIdx.x; t < tiles; t += BUCKET_G) row[t] = s_hist[t];
}
__global__ __launch_bounds__(BUCKET_G) void k_tile_count(int P, int tiles, const float2 *__restrict__ xy,
                                                          const int32_t *__restrict__ radii, Cam cam,
                                                          uint32_t *__restrict__ table) {
    tile_count_body(P, tiles, xy, radii, cam, table);
}
__global__ __launch_bounds__(BUCKET_G) void k_tile_count_views(int P, int tiles, K1Table tab) {
    const K1View &w = tab.v[blockIdx.y];
    tile_count_body(P, tiles, w.g.xy, w.radii, w.cam, w.table);
}

// per tile (one lane each, coalesced across tiles): exclusive prefix over the nb counting workgroups, in place;
// the column total goes to cnt[tile]
__device__ __forceinline__ void tile_colscan_body(int tiles, int nb, uint32_t *__restrict__ table, uint32_t *__restrict__ cnt) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= tiles) return;
    uint32_t run = 0;
    int b = 0;
    for (; b + 8 <= nb; b += 8) {   // 8 independent loads in flight
        uint32_t v[8];
#pragma unroll
        for (int u = 0; u < 8; u++) v[u] = table[(size_t)(b + u) * tiles + t];
#pragma unroll
        for (int u = 0; u < 8; u++) { table[(size_t)(b + u) * tiles + t] = run; run += v[u]; }
    }
    for (; b < nb; b++) { const uint32_t v = table[(size_t)b * tiles + t]; table[(size_t)b * tiles + t] = run; run += v; }
    cnt[t] = run;
}
__global__ __launch_bounds__(256) void k_tile_colscan(int tiles, int nb, uint32_t *__restrict__ table, uint32_t *__restrict__ cnt) {
    tile_colscan_body(tiles, nb, table, cnt);
}
__global__ __launch_bounds__(256) void k_tile_colscan_views(int tiles, int nb, K1Table tab) {
    uint32_t *table = tab.v[blockIdx.y].table;
    tile_colscan_body(tiles, nb, table, table + (size_t)nb * tiles);
}

// single workgroup: exclusive scan of the per-tile totals -> tile ranges, R, longest list
constexpr int INFO_BUSY = 64;   // word offset of the non-empty-tile list inside the info block: [count, tile ids ...]
constexpr int LPT_BINS = 512;   // bins of the longest-list-first order (list length / 16, BUCKET_CAP / 16 = 512)
constexpr int TSCAN_ITEMS = BUCKET_TILES / 1024;   // consecutive tiles per thread of the tile scan, at most
__device__ __forceinline__ void tile_scan_body(int tiles, const uint32_t *__restrict__ cnt, int2 *__restrict__ ranges,
                                               uint32_t *__restrict__ info, volatile uint32_t *mailbox, uint32_t tag) {
    // ONE scan over the tiles of two running sums packed in 64 bits: low word = instances (the tile ranges), high word = number of
    // non-empty tiles (their compact list: the tile sort launches over it instead of over a grid that is ~90 % empty on scene_1).
    // A thread takes `per` CONSECUTIVE tiles (tiles <= BUCKET_TILES on the bucketed path, the only caller: at most TSCAN_ITEMS), so the
    // counts are read from memory once, in one round trip, the workgroup scans once (two barriers, where 1024 tiles a round took three
    // rounds of three on the 2500 tiles of an 800 x 800 image), and the counts stay in registers for the longest-first pass below --
    // which walks the tiles, not the busy list, so nothing written here is read back.
    __shared__ unsigned long long s_w[17];
    __shared__ uint32_t s_max[16];
    __shared__ uint32_t s_bin[LPT_BINS + 1];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    uint32_t *busy = info + INFO_BUSY;
    uint32_t *lpt = busy + tiles + 4;
    const int per = (tiles + 1023) / 1024, t0 = threadIdx.x * per;
    uint32_t c[TSCAN_ITEMS];
#pragma unroll
    for (int k = 0; k < TSCAN_ITEMS; k++) c[k] = (k < per && t0 + k < tiles) ? cnt[t0 + k] : 0u;
    for (int i = threadIdx.x; i <= LPT_BINS; i += 1024) s_bin[i] = 0u;
    uint32_t mx = 0;
    unsigned long long v0 = 0ull;
#pragma unroll
    for (int k = 0; k < TSCAN_ITEMS; k++) { mx = max(mx, c[k]); v0 += (unsigned long long)c[k] | ((unsigned long long)(c[k] ? 1u : 0u) << 32); }
    unsigned long long inc = v0;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const unsigned long long o = __shfl_up(inc, d, 64); if (lane >= d) inc += o; }
    if (lane == 63) s_w[w] = inc;
    __syncthreads();                                       // (also: the zeroed bins)
    if (w == 0) {
        unsigned long long v = lane < 16 ? s_w[lane] : 0ull, vi = v;
#pragma unroll
        for (int d = 1; d < 16; d <<= 1) { const unsigned long long o = __shfl_up(vi, d, 64); if (lane >= d) vi += o; }
        if (lane < 16) s_w[lane] = vi - v;
        if (lane == 15) s_w[16] = vi;
    }
    __syncthreads();
    const unsigned long long carry = s_w[16];
    {
        unsigned long long exl = s_w[w] + inc - v0;
#pragma unroll
        for (int k = 0; k < TSCAN_ITEMS; k++) {
            const int t = t0 + k;
            if (k < per && t < tiles) {
                const uint32_t ex = (uint32_t)exl, nz = (uint32_t)(exl >> 32);
                ranges[t] = c[k] ? make_int2((int)ex, (int)(ex + c[k])) : make_int2(0, 0);
                if (c[k]) {
                    busy[1 + nz] = (uint32_t)t;
                    // length bins of the longest-first order below (a counting sort on length / 16)
                    atomicAdd(&s_bin[LPT_BINS - 1 - min(c[k] >> 4, (uint32_t)(LPT_BINS - 1))], 1u);
                } else {
                    lpt[tiles - 1 - (t - (int)nz)] = (uint32_t)t;   // launch-order list: empty tiles from the end
                }
                exl += (unsigned long long)c[k] | ((unsigned long long)(c[k] ? 1u : 0u) << 32);
            }
        }
    }
    __syncthreads();
    // the non-empty tiles once more, LONGEST LIST FIRST (a counting sort on length / 16): the launch order of the compositing forward.
    // Its waves -- one per (tile, 4x4 block), ~14 k of them with work on scene_1 for 8192 wave slots, 40-75 us each -- are handed out in
    // grid order to whichever slot frees: in tile order the longest lists (the middle of the image) start in the middle of the launch and
    // the slots that draw three of them in a row set the kernel's duration while the others idle (4.5 of 8 waves resident on average);
    // longest first, what is still running at the end are the short lists.  The tile sort walks the same list.
    {
        if (w == 0) {                                      // exclusive scan of the bins by one wave: 8 consecutive bins per lane
            uint32_t v[LPT_BINS / 64], run = 0;
#pragma unroll
            for (int k = 0; k < LPT_BINS / 64; k++) { v[k] = s_bin[lane * (LPT_BINS / 64) + k]; run += v[k]; }
            uint32_t binc = run;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) { const uint32_t o = (uint32_t)__shfl_up((int)binc, d, 64); if (lane >= d) binc += o; }
            uint32_t base = binc - run;
#pragma unroll
            for (int k = 0; k < LPT_BINS / 64; k++) { s_bin[lane * (LPT_BINS / 64) + k] = base; base += v[k]; }
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < TSCAN_ITEMS; k++)
            if (c[k]) lpt[atomicAdd(&s_bin[LPT_BINS - 1 - min(c[k] >> 4, (uint32_t)(LPT_BINS - 1))], 1u)] = (uint32_t)(t0 + k);
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) mx = max(mx, (uint32_t)__shfl_xor((int)mx, d, 64));
    if (lane == 0) s_max[w] = mx;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t m = 0;
        for (int k = 0; k < 16; k++) m = max(m, s_max[k]);
        info[0] = (uint32_t)carry;
        info[1] = m;
        info[2] = (uint32_t)(carry >> 32);               // non-empty tiles
        busy[0] = (uint32_t)(carry >> 32);
        if (mailbox) {   // host-mapped pinned memory: the host polls the tag instead of blocking in a stream synchronise
            mailbox[0] = (uint32_t)carry;
            mailbox[1] = m;
            mailbox[3] = (uint32_t)(carry >> 32);
            __threadfence_system();
            mailbox[2] = tag;
        }
    }
}
__global__ __launch_bounds__(1024) void k_tile_scan(int tiles, const uint32_t *__restrict__ cnt, int2 *__restrict__ ranges,
                                                     uint32_t *__restrict__ info, volatile uint32_t *mailbox, uint32_t tag) {
    tile_scan_body(tiles, cnt, ranges, info, mailbox, tag);
}
__global__ __launch_bounds__(1024) void k_tile_scan_views(int tiles, int nb, K1Table tab) {
    const K1View &w = tab.v[blockIdx.x];
    tile_scan_body(tiles, w.table + (size_t)nb * tiles, w.ranges, w.info, w.mailbox, w.tag);
}

__device__ __forceinline__ void emit_bucket_body(int P, int tiles, const float2 *__restrict__ xy,
                                                 const float *__restrict__ depth, const int32_t *__restrict__ radii,
                                                 const Cam &cam, const uint32_t *__restrict__ table,
                                                 const int2 *__restrict__ ranges, uint64_t *__restrict__ comp) {
    extern __shared__ uint32_t s_base[];
    const uint32_t *row = table + (size_t)blockIdx.x * tiles;
    for (int t = threadIdx.x; t < tiles; t += BUCKET_G) s_base[t] = (uint32_t)ranges[t].x + row[t];
    __syncthreads();
    const int i = blockIdx.x * BUCKET_G + threadIdx.x;
    if (i >= P) return;
    const int rad = radii[i];
    if (rad <= 0) return;
    const float2 p = xy[i];
    int minx, miny, maxx, maxy;
    tile_rect(p.x, p.y, rad, cam, minx, miny, maxx, maxy);
    const uint64_t v = ((uint64_t)__float_as_uint(depth[i]) << 32) | (uint32_t)i;
    for (int y = miny; y < maxy; y++)
        for (int x = minx; x < maxx; x++) comp[atomicAdd(&s_base[y * cam.gx + x], 1u)] = v;
}
__global__ __launch_bounds__(BUCKET_G) void k_emit_bucket(int P, int tiles, const float2 *__restrict__ xy,
                                                           const float *__restrict__ depth, const int32_t *__restrict__ radii,
                                                           Cam cam, const uint32_t *__restrict__ table,
                                                           const int2 *__restrict__ ranges, uint64_t *__restrict__ comp) {
    emit_bucket_body(P, tiles, xy, depth, radii, cam, table, ranges, comp);
}

// The second phase of the forward (after the one host read of the instance counts) for ALL views of a step, one launch per
// stage (blockIdx.y = view): the GPU's dispatcher packs the views' workgroups instead of 4 x 5 launches staggered by the
// host's launch rate.
struct P2View {
    Geom g;
    Cam cam;
    const int32_t *radii;
    const uint32_t *table;
    int2 *ranges;
    uint64_t *keys_u, *keys_sorted;
    uint32_t *ids_sorted;
    int *seg_offset, *slot_tile;
    float4 *ckpt;
    uint16_t *mask16;
    unsigned long long *bbits;  // [slots][16 blocks][4]: which entries of a segment each block blended (K6 -> K7)
    unsigned long long *bmask;  // [chunks][16 blocks]: which entries of a 64-entry list chunk reach each block (K5b -> K6)
    float4 *recA, *recB;
    float2 *recC;
    const float *bg;
    float *final_T;
    uint32_t *n_contrib;
    float *out_color, *out_depth;
    uint32_t R;                 // list capacity the binning chunk was laid out for (the null record sits at index R)
    // speculative launch (finish_views_batched): the host has not read the counts yet and sized the chunks from the previous call;
    // every kernel of the second phase checks the counts the scan left in `info` against those capacities and leaves the view
    // alone when they do not fit (the host notices the same way and repeats the phase with exact sizes)
    const uint32_t *info;       // [0] tile instances, [1] longest tile list, [2] non-empty tiles
    uint32_t Lcap;              // longest tile list the sort's LDS was sized for
    uint32_t Bcap;              // non-empty tiles the compositing forward's grid was sized for
    int spec;
};
struct P2Table { P2View v[RASTER_MAX_VIEWS]; uint32_t *valid; int nviews; };     // valid: see csplat_forward_views_faith (NULL otherwise)
__device__ __forceinline__ bool p2_live(const P2View &w) { return !w.spec || (w.info[0] - 1u < w.R && w.info[1] <= w.Lcap && w.info[2] <= w.Bcap); }
__device__ __forceinline__ void seg_plan_body(int tiles, const int2 *__restrict__ ranges, int *__restrict__ seg_offset,
                                              int *__restrict__ slot_tile);
// (the LAST workgroup of every view does not emit: it lays out the view's 256-entry segments -- the former k_seg_plan launch; both only
// need the tile ranges)
__global__ __launch_bounds__(BUCKET_G) void k_emit_bucket_views(int P, int tiles, P2Table tab) {
    const P2View &w = tab.v[blockIdx.y];
    if (!p2_live(w)) return;
    if (blockIdx.x == gridDim.x - 1) { seg_plan_body(tiles, w.ranges, w.seg_offset, w.slot_tile); return; }
    emit_bucket_body(P, tiles, w.g.xy, w.g.depth, w.radii, w.cam, w.table, w.ranges, w.keys_u);
}

constexpr int TSORT_THREADS = 1024;
constexpr int TSORT_WAVES = TSORT_THREADS / 64;
constexpr int TSORT_NB = 4 * TSORT_THREADS;               // interpolation buckets: every thread owns 4 consecutive ones
constexpr int TSORT_GRID = 512;                           // workgroups per view striding over the non-empty tiles
constexpr int TSORT_LONG = 64;                            // most keys in one bucket before the tile takes the radix fallback
constexpr int TSORT_WORDS = TSORT_NB + 4 + 256 + 8 + 2 + 2 + TSORT_WAVES + 2;   // u32 words of LDS behind the keys
__host__ __device__ inline size_t tsort_lds_bytes(int longest) {
    const int items = (longest > 0 ? longest : 1) + TSORT_THREADS - 1;
    return (size_t)(items / TSORT_THREADS) * TSORT_THREADS * 8 + (size_t)TSORT_WORDS * 4;
}

// One tile's (depth bits << 32 | Gaussian id) keys put into ascending order entirely in LDS + registers.  The result is the
// unique sorted order of the (unique) composite keys, i.e. exactly the stable (tile | depth) radix order of the upstream
// pipeline -- however it is reached:
//   * default (round 3): an INTERPOLATION BUCKET sort.  A tile holds 1 .. 8192 keys whose depths span a narrow range; the
//     depth bits (positive floats: unsigned order = numeric order) are mapped monotonically onto 4096 buckets between the tile's
//     own minimum and maximum, every key takes a slot in its bucket with ONE LDS atomic (the order inside a bucket is whatever
//     the atomics made it), an exclusive scan of the bucket counts gives the bucket starts, the keys are dropped at start +
//     slot, and every key then counts the keys of its bucket that are smaller (its rank: ~1 independent LDS read per key) and
//     moves to start + rank.  Buckets are ordered and complete and the composite keys unique, so the outcome does not depend
//     on the atomic order: bit-identical to the radix sort, in 8 barriers instead of ~6 per radix pass x 3 passes.
//   * fallback (a bucket with more than TSORT_LONG keys: depths piled onto a few buckets by an outlier; all depths equal;
//     csplat_debug_flags bit 11): the round-2 stable LSD radix sort -- keys live in registers between passes (lane l of wave w
//     owns positions w*64*items + i*64 + l), every pass ranks the 8-bit digit with 8 ballots per key and per-wave LDS counters.
// mode: bit 0 = ids < 2^24 (radix: skip byte 3), bit 1 = radix only, bit 2 = bucket limit 1 (tests the fallback path)
template <int ITEMS>
__device__ __forceinline__ void tile_sort_body(const int2 *__restrict__ ranges, const uint64_t *__restrict__ comp,
                                               uint64_t *__restrict__ keys_sorted,
                                               uint32_t *__restrict__ ids_sorted, int mode, int tile) {
    extern __shared__ uint64_t s_key[];                 // [m] keys, then the counters
    const int2 r = ranges[tile];
    const int n = r.y - r.x;
    if (n <= 0) return;
    const int skip_byte3 = mode & 1;
    const int items = (n + TSORT_THREADS - 1) / TSORT_THREADS;
    uint32_t *s_cnt = reinterpret_cast<uint32_t *>(s_key + (size_t)items * TSORT_THREADS);   // [TSORT_NB] buckets / [TSORT_WAVES][256]
    uint32_t *s_dig = s_cnt + TSORT_NB + 4;                                                   // [256] + [4] (+ 4 spare)
    // (lane and wave are re-derived for every tile behind an empty asm: hoisted out of the callers' tile loop, what depends on them alone
    //  -- a dozen offsets and masks -- stays live across the whole sort and no longer fits the 64 registers of two workgroups per CU)
    int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    asm volatile("" : "+v"(lane), "+v"(w));
    const int wbase = w * items * 64;
    const uint64_t lt = (1ull << lane) - 1ull;
    uint64_t key[ITEMS];
    uint32_t rank[ITEMS];
#pragma unroll
    for (int i = 0; i < ITEMS; i++) {
        const int idx = wbase + i * 64 + lane;
        key[i] = (i < items && idx < n) ? comp[r.x + idx] : ~0ull;
    }
    uint32_t *s_diff = s_dig + 264;                                                           // [2]
    uint32_t *s_mm = s_diff + 2;                                                              // [2] min, max of the depth bits
    uint32_t *s_wtot = s_mm + 2;                                                              // [TSORT_WAVES]
    const uint64_t hi = (uint64_t)(uint32_t)tile << 32;
    if (!(mode & 2)) {
        // ---- interpolation bucket sort
        uint32_t dmin = ~0u, dmax = 0u;
#pragma unroll
        for (int i = 0; i < ITEMS; i++) {
            const int idx = wbase + i * 64 + lane;
            if (i < items && idx < n) { const uint32_t d = (uint32_t)(key[i] >> 32); dmin = min(dmin, d); dmax = max(dmax, d); }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            dmin = min(dmin, (uint32_t)__shfl_xor((int)dmin, o, 64));
            dmax = max(dmax, (uint32_t)__shfl_xor((int)dmax, o, 64));
        }
        if (threadIdx.x == 0) { s_mm[0] = ~0u; s_mm[1] = 0u; }
        reinterpret_cast<uint4 *>(s_cnt)[threadIdx.x] = make_uint4(0u, 0u, 0u, 0u);
        __syncthreads();
        if (lane == 0) { atomicMin(&s_mm[0], dmin); atomicMax(&s_mm[1], dmax); }
        __syncthreads();
        dmin = s_mm[0]; dmax = s_mm[1];
        if (dmax != dmin) {                                   // (workgroup-uniform)
            // monotone map of the depth bits onto [0, TSORT_NB): uint -> float conversion, a positive scale and truncation
            // are all non-decreasing, so bucket order never contradicts depth order
            const float scale = (float)TSORT_NB / ((float)(dmax - dmin) + 1.0f);
            uint32_t bs[ITEMS];                         // bucket << 16 | slot inside the bucket
#pragma unroll
            for (int i = 0; i < ITEMS; i++) {
                const int idx = wbase + i * 64 + lane;
                if (i < items && idx < n) {
                    const uint32_t b = min((uint32_t)(TSORT_NB - 1), (uint32_t)((float)((uint32_t)(key[i] >> 32) - dmin) * scale));
                    bs[i] = (b << 16) | atomicAdd(&s_cnt[b], 1u);
                }
            }
            __syncthreads();
            // exclusive scan of the bucket counts: 4 buckets per thread, a wave scan, the wave totals
            const uint4 c = reinterpret_cast<const uint4 *>(s_cnt)[threadIdx.x];
            const uint32_t tot = c.x + c.y + c.z + c.w;
            uint32_t inc = tot;
#pragma unroll
            for (int dd = 1; dd < 64; dd <<= 1) { const uint32_t o = __shfl_up(inc, dd, 64); if (lane >= dd) inc += o; }
            if (lane == 63) s_wtot[w] = inc;
            __syncthreads();
            uint32_t ex = inc - tot;
            for (int k = 0; k < w; k++) ex += s_wtot[k];
            reinterpret_cast<uint4 *>(s_cnt)[threadIdx.x] = make_uint4(ex, ex + c.x, ex + c.x + c.y, ex + c.x + c.y + c.z);
            if (threadIdx.x == 0) s_cnt[TSORT_NB] = (uint32_t)n;
            __syncthreads();
#pragma unroll
            for (int i = 0; i < ITEMS; i++) {
                const int idx = wbase + i * 64 + lane;
                if (i < items && idx < n) s_key[s_cnt[bs[i] >> 16] + (bs[i] & 0xFFFFu)] = key[i];
            }
            __syncthreads();
            // inside a bucket the order is whatever the atomics made it: every key finds its RANK among the keys of its bucket
            // (independent LDS reads, a bucket holds ~1 key on average; the composite keys are unique) ...
            const int limit = (mode & 4) ? 1 : TSORT_LONG;
            bool long_run = false;
            uint32_t dst[ITEMS];
#pragma unroll
            for (int i = 0; i < ITEMS; i++) {
                const int idx = wbase + i * 64 + lane;
                if (i < items && idx < n) {
                    const uint32_t b = bs[i] >> 16;
                    const uint32_t lo = s_cnt[b], cb = s_cnt[b + 1] - lo;     // (s_cnt[TSORT_NB] = n)
                    uint32_t rk = 0;
                    if (cb > (uint32_t)limit) long_run = true;
                    else
#pragma unroll 1
                        for (uint32_t j = 0; j < cb; j++) rk += s_key[lo + j] < key[i] ? 1u : 0u;     // (cb ~ 1: unrolled, it costs 30 registers)
                    dst[i] = lo + rk;
                }
            }
            if (!__syncthreads_or(long_run)) {
                // ... and moves there (the keys are still in registers: in place, behind a barrier)
#pragma unroll
                for (int i = 0; i < ITEMS; i++) {
                    const int idx = wbase + i * 64 + lane;
                    if (i < items && idx < n) s_key[dst[i]] = key[i];
                }
                __syncthreads();
#pragma unroll
                for (int i = 0; i < ITEMS; i++) {
                    const int idx = wbase + i * 64 + lane;
                    if (i < items && idx < n) {
                        const uint64_t k = s_key[idx];
                        keys_sorted[r.x + idx] = hi | (k >> 32);
                        ids_sorted[r.x + idx] = (uint32_t)k;
                    }
                }
                return;
            }
            // (fallback: key[] still holds the tile's keys; the composite key is unique, so the radix sort below gives the
            // same order whatever order they are in)
        }
    }
    // ---- stable LSD radix sort (fallback)
    // digits on which every key of the tile agrees need no pass (a stable pass over a constant digit is the identity):
    // typically the exponent byte of the depth, and more on short lists.  One OR-reduction of (key ^ first key).
    __syncthreads();
    if (threadIdx.x < 2) s_diff[threadIdx.x] = 0u;
    __syncthreads();
    {
        const uint64_t k0 = comp[r.x];
        uint64_t dv = 0ull;
#pragma unroll
        for (int i = 0; i < ITEMS; i++) {
            const int idx = wbase + i * 64 + lane;
            if (i < items && idx < n) dv |= key[i] ^ k0;
        }
        uint32_t lo = (uint32_t)dv, hi32 = (uint32_t)(dv >> 32);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { lo |= (uint32_t)__shfl_xor((int)lo, o, 64); hi32 |= (uint32_t)__shfl_xor((int)hi32, o, 64); }
        if (lane == 0) { atomicOr(&s_diff[0], lo); atomicOr(&s_diff[1], hi32); }
    }
    __syncthreads();
    const uint64_t diffbits = (uint64_t)s_diff[0] | ((uint64_t)s_diff[1] << 32);
    auto pass = [&](int shift) {
        for (int t = threadIdx.x; t < TSORT_WAVES * 256; t += TSORT_THREADS) s_cnt[t] = 0u;
        __syncthreads();
#pragma unroll
        for (int i = 0; i < ITEMS; i++) {
            if (i < items) {   // workgroup-uniform
                const int idx = wbase + i * 64 + lane;
                const bool valid = idx < n;
                const uint32_t d = (uint32_t)(key[i] >> shift) & 0xFF;
                unsigned long long peers = __builtin_amdgcn_ballot_w64(valid);
#pragma unroll
                for (int b = 0; b < 8; b++) {
                    const unsigned long long mb = __builtin_amdgcn_ballot_w64(valid && ((d >> b) & 1));
                    peers &= ((d >> b) & 1) ? mb : ~mb;
                }
                const uint32_t prev = s_cnt[w * 256 + d];
                rank[i] = prev + (uint32_t)__popcll(peers & lt);
                __builtin_amdgcn_wave_barrier();
                if (valid && (peers & lt) == 0ull) s_cnt[w * 256 + d] = prev + (uint32_t)__popcll(peers);
                __builtin_amdgcn_wave_barrier();
            }
        }
        __syncthreads();
        uint32_t tot = 0;   // (the per-wave counts are read again below instead of kept: 16 registers of the fallback the bucket path would pay for)
        if (threadIdx.x < 256) {
#pragma unroll
            for (int k = 0; k < TSORT_WAVES; k++) tot += s_cnt[k * 256 + threadIdx.x];
            uint32_t inc = tot;   // inclusive scan of the digit totals over 4 waves of 64 digits
#pragma unroll
            for (int dd = 1; dd < 64; dd <<= 1) { const uint32_t o = __shfl_up(inc, dd, 64); if (lane >= dd) inc += o; }
            if (lane == 63) s_dig[256 + w] = inc;
            s_dig[threadIdx.x] = inc - tot;
        }
        __syncthreads();
        if (threadIdx.x < 256) {
            uint32_t run = s_dig[threadIdx.x];
            for (int k = 0; k < w; k++) run += s_dig[256 + k];
#pragma unroll
            for (int k = 0; k < TSORT_WAVES; k++) { const uint32_t ck = s_cnt[k * 256 + threadIdx.x]; s_cnt[k * 256 + threadIdx.x] = run; run += ck; }
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < ITEMS; i++) {
            if (i < items) {
                const int idx = wbase + i * 64 + lane;
                if (idx < n) {
                    const uint32_t d = (uint32_t)(key[i] >> shift) & 0xFF;
                    s_key[s_cnt[w * 256 + d] + rank[i]] = key[i];
                }
            }
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < ITEMS; i++) {
            const int idx = wbase + i * 64 + lane;
            if (i < items && idx < n) key[i] = s_key[idx];
        }
        __syncthreads();
    };
    auto varies = [&](int byte) { return ((diffbits >> (byte * 8)) & 0xFFull) != 0ull && !(byte == 3 && skip_byte3); };   // workgroup-uniform
    // The key is (depth bits, Gaussian id) and the id only breaks ties between EQUAL depths, which are rare (exact clones right
    // after a densification step, coplanar centres): sort on the depth bytes alone (3 passes on a typical tile instead of 6),
    // then put the runs of equal depth into id order.  Short runs are fixed in place by the lane that owns the run's first
    // element; a run longer than TIE_RUN (or a tile whose depths are all equal) falls back to the full LSD sort over every
    // varying byte -- the composite key is unique, so the result is the same whatever order the keys are in by then.
    constexpr int TIE_RUN = 8;
    bool full = (diffbits >> 32) == 0ull;        // no depth byte varies: nothing but the ids to sort on
    if (!full) {
        for (int byte = 4; byte < 8; byte++)
            if (varies(byte)) pass(byte * 8);
        // (s_key now holds the keys in depth order, key[] = this lane's elements of it)
        bool long_run = false;
#pragma unroll
        for (int i = 0; i < ITEMS; i++) {
            const int idx = wbase + i * 64 + lane;
            if (i < items && idx + 1 < n) {
                const uint32_t d = (uint32_t)(key[i] >> 32);
                const bool starts = (idx == 0 || (uint32_t)(s_key[idx - 1] >> 32) != d) && (uint32_t)(s_key[idx + 1] >> 32) == d;
                if (starts) {
                    int j = idx + 2;
                    while (j < n && j - idx <= TIE_RUN && (uint32_t)(s_key[j] >> 32) == d) j++;
                    if (j - idx > TIE_RUN) long_run = true;
                    else
                        for (int a2 = idx + 1; a2 < j; a2++) {          // insertion sort of the run by id (low word)
                            const uint64_t v = s_key[a2];
                            int b2 = a2 - 1;
                            while (b2 >= idx && s_key[b2] > v) { s_key[b2 + 1] = s_key[b2]; b2--; }
                            s_key[b2 + 1] = v;
                        }
                }
            }
        }
        full = __syncthreads_or(long_run);
        if (!full) {
#pragma unroll
            for (int i = 0; i < ITEMS; i++) {
                const int idx = wbase + i * 64 + lane;
                if (i < items && idx < n) key[i] = s_key[idx];
            }
        }
    }
    if (full)
        for (int byte = 0; byte < 8; byte++)
            if (varies(byte)) pass(byte * 8);
#pragma unroll
    for (int i = 0; i < ITEMS; i++) {
        const int idx = wbase + i * 64 + lane;
        if (i < items && idx < n) {
            keys_sorted[r.x + idx] = hi | (key[i] >> 32);
            ids_sorted[r.x + idx] = (uint32_t)key[i];
        }
    }
}
// ITEMS = keys per lane the instantiation holds in registers (the host picks the smallest that takes the launch's longest list:
// tile_sort_launch).  The workgroups stride over the non-empty tiles LONGEST LIST FIRST (the order the tile scan leaves for K6).
// DENSE: compiled for 8 waves per SIMD (64 VGPRs), so that TWO workgroups share a CU.  A tile's sort is a chain of ~10 workgroup barriers
// and a second workgroup fills the waits, but the 64-register code takes a fifth longer per tile (MI355X, 800 x 800 scene_1: 14.4 against
// 12.0 us for the 267 tiles of one view, 20.5 / 20.9 for two views, 26.2 / 28.3 for three, 31.1 / 34.6 for four): the host takes it for
// launches of more than 2.5 non-empty tiles per CU (tsort_dense).
template <int ITEMS, bool DENSE>
__global__ __launch_bounds__(TSORT_THREADS, DENSE ? 8 : 4) void k_tile_sort(const int2 *__restrict__ ranges, const uint64_t *__restrict__ comp,
                                                              uint64_t *__restrict__ keys_sorted,
                                                              uint32_t *__restrict__ ids_sorted, const uint32_t *__restrict__ info, int tiles, int mode) {
    const uint32_t *busy = info + INFO_BUSY, *lpt = busy + tiles + 4;
    const int nbusy = (int)busy[0];
    for (int b = blockIdx.x; b < nbusy; b += gridDim.x) {
        tile_sort_body<ITEMS>(ranges, comp, keys_sorted, ids_sorted, mode, (int)lpt[b]);
        __syncthreads();
    }
}
template <int ITEMS, bool DENSE>
__global__ __launch_bounds__(TSORT_THREADS, DENSE ? 8 : 4) void k_tile_sort_views(P2Table tab, int tiles, int mode) {
    // (workgroups are handed out in the order of their linear index: view = index % views puts the longest lists of EVERY view in
    //  front, where blockIdx.y = view started the last view's longest lists behind all the others' short ones)
    const int lin = blockIdx.y * gridDim.x + blockIdx.x, nv = gridDim.y;
    const P2View &w = tab.v[lin % nv];
    if (!p2_live(w)) return;
    const uint32_t *busy = w.info + INFO_BUSY, *lpt = busy + tiles + 4;
    const int nbusy = (int)busy[0];
    for (int b = lin / nv; b < nbusy; b += gridDim.x) {
        tile_sort_body<ITEMS>(w.ranges, w.keys_u, w.keys_sorted, w.ids_sorted, mode, (int)lpt[b]);
        __syncthreads();
    }
}

template <int CTRL, int RMASK>
__device__ __forceinline__ float dpp_mov(float v, float old) {
    return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(old), __float_as_int(v), CTRL, RMASK, 0xF, false));
}
// min / max over the 64 lanes, result broadcast to every lane (through an SGPR)
__device__ __forceinline__ float wave_min(float v) {
    v = fminf(v, dpp_mov<0xB1, 0xF>(v, v)); v = fminf(v, dpp_mov<0x4E, 0xF>(v, v));
    v = fminf(v, dpp_mov<0x141, 0xF>(v, v)); v = fminf(v, dpp_mov<0x140, 0xF>(v, v));
    const float r0 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 0));
    const float r1 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 16));
    const float r2 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 32));
    const float r3 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 48));
    return fminf(fminf(r0, r1), fminf(r2, r3));
}
__device__ __forceinline__ float wave_max(float v) { return -wave_min(-v); }

// Wave-level culling.  A list entry can only change a pixel if alpha = opacity*exp(power) >= 1/255, and
// power <= -0.5*d^2/lambda_max(cov2D); so it is irrelevant to EVERY pixel of an axis-aligned box whose distance to
// the centre satisfies d^2 > cut2 = 2*lambda_max*ln(255*opacity) (K1 stores cut2 with a safety margin).  Lane l
// tests entry l of a 64-entry group against the wave's box of still-live pixels; the ballot is the work list.
//
// Second, exact stage (scene_1: a quarter of the circle test's survivors reach no pixel -- the projected Gaussians are
// anisotropic and the circle of radius sqrt(cut2) over-covers their ellipse): alpha >= 1/255 <=> q(d) = A dx^2 + 2B dx dy
// + C dy^2 <= tau = 2 ln(255 opacity), so the entry is irrelevant to the whole box if the MINIMUM of q over the box
// exceeds tau.  q is convex: the minimum is 0 if the centre is inside, else it lies on one of the (at most two) edges
// facing the centre, where q is a 1-D quadratic whose minimiser is clamped to the edge.  ~35 VALU per entry per chunk,
// against ~26 per survivor and pixel row saved.  Margins: 1e-3 relative + 1e-3 absolute on tau, 1e-5 of the sum of the
// absolute terms of q (cancellation); culling must stay exact (tests compare against the un-culled run bit for bit).
__device__ __forceinline__ bool box_hit(float2 c, float cut2, float4 co, float bx0, float bx1, float by0, float by1, bool exact) {
    const float lx = bx0 - c.x, hx = bx1 - c.x, ly = by0 - c.y, hy = by1 - c.y;     // the box relative to the centre
    const float ex = fmaxf(lx, fminf(0.f, hx)), ey = fmaxf(ly, fminf(0.f, hy));     // nearest point of the box, per axis
    if (!(ex * ex + ey * ey <= cut2)) return false;
    if (!exact || cut2 > 1.0e30f) return true;
    const float A = co.x, B = co.y, C = co.z;
    float qmin = 0.f, sabs = 0.f;
    if (ex != 0.f || ey != 0.f) {
        float q1 = 3.0e38f, s1 = 0.f, q2 = 3.0e38f, s2 = 0.f;
        if (ex != 0.f) {
            const float dy = fminf(fmaxf(-B * ex * __builtin_amdgcn_rcpf(fmaxf(C, 1e-30f)), ly), hy);
            const float t0 = A * ex * ex, t1 = 2.f * B * ex * dy, t2 = C * dy * dy;
            q1 = t0 + t1 + t2; s1 = t0 + fabsf(t1) + t2;
        }
        if (ey != 0.f) {
            const float dx = fminf(fmaxf(-B * ey * __builtin_amdgcn_rcpf(fmaxf(A, 1e-30f)), lx), hx);
            const float t0 = C * ey * ey, t1 = 2.f * B * ey * dx, t2 = A * dx * dx;
            q2 = t0 + t1 + t2; s2 = t0 + fabsf(t1) + t2;
        }
        const bool first = q1 <= q2;
        qmin = first ? q1 : q2; sabs = first ? s1 : s2;
    }
    const float tau = 2.f * __logf(255.f * co.w);
    return qmin - 1e-5f * sabs <= tau * 1.001f + 1e-3f;
}

#ifndef CSPLAT_SEG
#define CSPLAT_SEG 256
#endif
constexpr int SEG = CSPLAT_SEG;   // tile-list entries per backward segment (multiple of 64)

// per-tile segment plan: seg_offset[t] = first segment slot of tile t (exclusive scan of ceil(n_t / SEG)),
// slot_tile[slot] = owning tile.  One workgroup; tiles are few (2500 at 800x800).
__device__ __forceinline__ void seg_plan_body(int tiles, const int2 *__restrict__ ranges, int *__restrict__ seg_offset,
                                              int *__restrict__ slot_tile) {
    __shared__ int s_w[17];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int carry = 0;
    for (int base = 0; base < tiles; base += 1024) {
        const int t = base + threadIdx.x;
        int ns = 0;
        if (t < tiles) { const int2 r = ranges[t]; ns = (r.y - r.x + SEG - 1) / SEG; }
        int inc = ns;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) { const int o = __shfl_up(inc, d, 64); if (lane >= d) inc += o; }
        if (lane == 63) s_w[w] = inc;
        __syncthreads();
        if (w == 0) {
            int v = lane < 16 ? s_w[lane] : 0, vi = v;
#pragma unroll
            for (int d = 1; d < 16; d <<= 1) { const int o = __shfl_up(vi, d, 64); if (lane >= d) vi += o; }
            if (lane < 16) s_w[lane] = vi - v;
            if (lane == 15) s_w[16] = vi;
        }
        __syncthreads();
        const int ex = carry + s_w[w] + inc - ns;
        if (t < tiles) {
            seg_offset[t] = ex;
            for (int k = 0; k < ns; k++) slot_tile[ex + k] = t;
        }
        carry += s_w[16];
        __syncthreads();
    }
    if (threadIdx.x == 0) seg_offset[tiles] = carry;
}
__global__ __launch_bounds__(1024) void k_seg_plan(int tiles, const int2 *__restrict__ ranges, int *__restrict__ seg_offset,
                                                    int *__restrict__ slot_tile) {
    seg_plan_body(tiles, ranges, seg_offset, slot_tile);
}
__global__ __launch_bounds__(1024) void k_seg_plan_views(int tiles, P2Table tab) {
    const P2View &w = tab.v[blockIdx.x];
    if (!p2_live(w)) return;
    seg_plan_body(tiles, w.ranges, w.seg_offset, w.slot_tile);
}

}  // namespace
