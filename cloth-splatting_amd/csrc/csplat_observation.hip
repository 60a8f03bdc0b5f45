// csplat_observation.hip -- observation clouds, the sensing end of the pipeline (gfx950, wave64; include/csplat.h, csplat_obs_unproject,
// csplat_obs_voxel and csplat_obs_mark, states the semantics).  The reference does this on the host with numpy: get_world_coords
// (manipulation/envs/camera_utils.py:106-133, manipulation/deform_mesh.py:168-195) and get_observable_particle_index (camera_utils.py:136-162,
// a full cdist matrix).
//   k_obs_select      one thread per four pixels of a view (blockIdx.y): the selection byte of each -- a pure stream over depth (and mask)
//   (csplat_mask_to_map: selection bytes -> the output row of every selected pixel, stable, and their number)
//   k_obs_points      the same walk again: a selected pixel's point and flat index into its row
//   k_obs_min_part / k_obs_min_final   the per-axis minimum over the finite points, when no origin is given (a minimum: the same in any order)
//   k_obs_keys        one thread per point: its cell and the sort key cz << 42 | cy << 21 | cx (two keys above every cell's for the rest)
//   (csplat_sort_pairs_u64: stable, the point index as value; csplat_scan_u32 over the head flags)
//   k_obs_heads       head flag of every sorted entry        k_obs_segments   inverse[], the first entry of every voxel
//   k_obs_centroids   one wave per voxel: lane l sums the offsets from the cell corner of the entries l, l + 64, .. of its segment in
//                     increasing order, a xor tree joins the lanes -- an order fixed by the segment alone
//   k_obs_voxel_counts   one thread: K and the number of points outside the cell range, from the sorted keys
//   k_obs_mark        one thread per four (index, distance) entries: plain byte stores of the value 1
// No atomics of any kind; every output is bit-reproducible.  Float arithmetic without contraction: every operation is one float32 rounding,
// so that a numpy float32 restatement gives the same cells and the same selection.
// Algorithmic bytes: unproject, per pixel: 4 (depth) [+ 4 mask] read and 1 written, then 4 + 4 (depth, row) read and, per selected pixel,
// 16 written; voxel, per point: 12 read and 12 written around an 8-pass sort of 12-byte pairs, 12 gathered; mark, per entry: 8 read.
#include "csplat_common.h"
#include "csplat_device.h"

#pragma clang fp contract(off)

namespace {

constexpr int OB_THREADS = 256, OB_MIN_BLOCKS = 256;
constexpr int OB_CELL_BITS = 21;
constexpr uint64_t OB_KEY_RANGE = (uint64_t)1 << 63, OB_KEY_NONFINITE = OB_KEY_RANGE | 1u;      // above every cell's key, in this order

template <typename T> struct ObsQuad { T v[4]; };

// elements [p0, p0 + 4) of a plane of n 4-byte values: one 16-byte load when the four lie inside the plane on a 16-byte boundary, scalar
// loads of those inside it otherwise (`fill` for the others).  p0 may be negative: the first slot of a plane that begins off the boundary
template <typename T>
__device__ __forceinline__ ObsQuad<T> obs_load4(const T *__restrict__ plane, int64_t p0, int64_t n, T fill) {
    ObsQuad<T> q;
    const uintptr_t addr = (uintptr_t)plane + (uintptr_t)(p0 * 4);
    if (p0 >= 0 && p0 + 4 <= n && (addr & 15) == 0) {
        const uint4 w = *reinterpret_cast<const uint4 *>(addr);
        const uint32_t u[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
        for (int e = 0; e < 4; e++) __builtin_memcpy(&q.v[e], &u[e], 4);
    } else {
#pragma unroll
        for (int e = 0; e < 4; e++) {
            const int64_t p = p0 + e;
            q.v[e] = (p >= 0 && p < n) ? plane[p] : fill;
        }
    }
    return q;
}

// how many elements the slots of a plane are shifted down so that slot boundaries fall on 16 bytes (0 .. 3; the plane is 4-byte aligned)
__device__ __host__ __forceinline__ int obs_shift(const void *plane) { return (int)(((uintptr_t)plane & 15) >> 2); }

// grid (slots of a view, V views): v = blockIdx.y is uniform
template <bool MASKED>
__global__ __launch_bounds__(OB_THREADS) void k_obs_select(int W, int64_t HW, const float *__restrict__ depth, const float *__restrict__ mask,
                                                           int stride, float max_depth, uint8_t *__restrict__ sel) {
    const int64_t base = (int64_t)blockIdx.y * HW;
    const float *__restrict__ plane = depth + base;
    const int64_t p0 = 4 * ((int64_t)blockIdx.x * OB_THREADS + threadIdx.x) - obs_shift(plane);
    if (p0 >= HW) return;
    const ObsQuad<float> d = obs_load4<float>(plane, p0, HW, 0.f);
    ObsQuad<float> m;
    if (MASKED) m = obs_load4<float>(mask + base, p0, HW, 0.f);
    const int64_t first = p0 < 0 ? 0 : p0;
    int y = (int)(first / W), x = (int)(first - (int64_t)y * W);
#pragma unroll
    for (int e = 0; e < 4; e++) {
        const int64_t p = p0 + e;
        if (p < first || p >= HW) continue;
        bool on = d.v[e] > 0.f && d.v[e] < __builtin_inff();                      // a hole is 0, negative, NaN or Inf
        on = on && (max_depth <= 0.f || d.v[e] <= max_depth);
        if (MASKED) on = on && m.v[e] > 0.5f;
        if (stride > 1) on = on && (x % stride == 0) && (y % stride == 0);
        sel[base + p] = on ? 1 : 0;
        if (++x == W) { x = 0; y++; }
    }
}

// intr = (fx, fy, cx, cy), c2w = 3 x 4 row-major camera-to-world, both wave-uniform
template <int KIND>
__device__ __forceinline__ void obs_point(int x, int y, float d, const float *__restrict__ intr, const float *__restrict__ c2w, float out[3]) {
    float cx, cy, cz;
    if (KIND == 0) {
        cx = ((float)x - intr[2]) * d / intr[0];
        cy = ((float)y - intr[3]) * d / intr[1];
        cz = d;
    } else {
        const float a = ((float)x - intr[2]) / intr[0], b = ((float)y - intr[3]) / intr[1];
        const float s = d / sqrtf(a * a + b * b + 1.f);
        cx = a * s;
        cy = b * s;
        cz = s;
    }
#pragma unroll
    for (int r = 0; r < 3; r++) out[r] = c2w[4 * r] * cx + c2w[4 * r + 1] * cy + c2w[4 * r + 2] * cz + c2w[4 * r + 3];
}

template <int KIND>
__global__ __launch_bounds__(OB_THREADS) void k_obs_points(int W, int64_t HW, const float *__restrict__ depth, const float *__restrict__ intrinsics,
                                                           const float *__restrict__ cam_to_world, const int32_t *__restrict__ map, int64_t cap,
                                                           float *__restrict__ points, int32_t *__restrict__ source) {
    const int v = blockIdx.y;
    const int64_t base = (int64_t)v * HW;
    const float *__restrict__ plane = depth + base;
    const int64_t p0 = 4 * ((int64_t)blockIdx.x * OB_THREADS + threadIdx.x) - obs_shift(plane);
    if (p0 >= HW) return;
    const ObsQuad<int32_t> row = obs_load4<int32_t>(map + base, p0, HW, -1);
    if (row.v[0] < 0 && row.v[1] < 0 && row.v[2] < 0 && row.v[3] < 0) return;      // nothing selected in this slot: no depth load
    const ObsQuad<float> d = obs_load4<float>(plane, p0, HW, 0.f);
    const float *__restrict__ intr = intrinsics + 4 * v, *__restrict__ c2w = cam_to_world + 12 * v;
    const int64_t first = p0 < 0 ? 0 : p0;
    int y = (int)(first / W), x = (int)(first - (int64_t)y * W);
#pragma unroll
    for (int e = 0; e < 4; e++) {
        const int64_t p = p0 + e;
        if (p < first || p >= HW) continue;
        const int64_t to = row.v[e];
        if (to >= 0 && to < cap) {
            float w[3];
            obs_point<KIND>(x, y, d.v[e], intr, c2w, w);
            points[3 * to] = w[0];
            points[3 * to + 1] = w[1];
            points[3 * to + 2] = w[2];
            source[to] = (int32_t)(base + p);
        }
        if (++x == W) { x = 0; y++; }
    }
}

// ---- voxel grid
__device__ __forceinline__ void obs_block_min3(float m[3], float *__restrict__ out) {
    __shared__ float s_min[3][OB_THREADS / 64];
#pragma unroll
    for (int a = 0; a < 3; a++) block_stash(s_min[a], wave_min(m[a]));
    __syncthreads();
    if (threadIdx.x < 3) {                              // thread a joins axis a, from slot 0 on
        float r = s_min[threadIdx.x][0];
        for (int k = 1; k < OB_THREADS / 64; k++) r = fminf(r, s_min[threadIdx.x][k]);
        out[threadIdx.x] = r;
    }
}

// part[blockIdx.x] = the per-axis minimum over this workgroup's share of the points whose three coordinates are finite (+inf: none)
__global__ __launch_bounds__(OB_THREADS) void k_obs_min_part(int64_t M, const float *__restrict__ points, float *__restrict__ part) {
    float m[3] = {__builtin_inff(), __builtin_inff(), __builtin_inff()};
    for (int64_t i = (int64_t)blockIdx.x * OB_THREADS + threadIdx.x; i < M; i += (int64_t)gridDim.x * OB_THREADS) {
        const float x = points[3 * i], y = points[3 * i + 1], z = points[3 * i + 2];
        if (finite_f32(x) && finite_f32(y) && finite_f32(z)) { m[0] = fminf(m[0], x); m[1] = fminf(m[1], y); m[2] = fminf(m[2], z); }
    }
    obs_block_min3(m, part + 3 * blockIdx.x);
}

__global__ __launch_bounds__(OB_THREADS) void k_obs_min_final(int n_parts, const float *__restrict__ part, float *__restrict__ origin) {
    float m[3] = {__builtin_inff(), __builtin_inff(), __builtin_inff()};
    for (int i = threadIdx.x; i < n_parts; i += OB_THREADS) {
        m[0] = fminf(m[0], part[3 * i]); m[1] = fminf(m[1], part[3 * i + 1]); m[2] = fminf(m[2], part[3 * i + 2]);
    }
    obs_block_min3(m, origin);
}

// the cell of one coordinate: floorf((p - o) / voxel), the subtraction and the division each one float32 rounding (IEEE division: the
// library is built without fast-math and hipcc's default is the correctly rounded form).  Outside [0, 2^21), or NaN: -1
__device__ __forceinline__ int64_t obs_cell(float p, float o, float voxel) {
    const float c = floorf(__fdiv_rn(__fsub_rn(p, o), voxel));
    return (c >= 0.f && c < (float)(1 << OB_CELL_BITS)) ? (int64_t)c : -1;
}

__global__ __launch_bounds__(OB_THREADS) void k_obs_keys(int64_t M, const float *__restrict__ points, const float *__restrict__ origin, float voxel,
                                                         uint64_t *__restrict__ keys, uint32_t *__restrict__ vals) {
    const int64_t i = (int64_t)blockIdx.x * OB_THREADS + threadIdx.x;
    if (i >= M) return;
    const float x = points[3 * i], y = points[3 * i + 1], z = points[3 * i + 2];
    uint64_t key = OB_KEY_NONFINITE;
    if (finite_f32(x) && finite_f32(y) && finite_f32(z)) {
        const int64_t cx = obs_cell(x, origin[0], voxel), cy = obs_cell(y, origin[1], voxel), cz = obs_cell(z, origin[2], voxel);
        key = (cx < 0 || cy < 0 || cz < 0) ? OB_KEY_RANGE
                                           : ((uint64_t)cz << (2 * OB_CELL_BITS)) | ((uint64_t)cy << OB_CELL_BITS) | (uint64_t)cx;
    }
    keys[i] = key;
    vals[i] = (uint32_t)i;
}

__global__ __launch_bounds__(OB_THREADS) void k_obs_heads(int64_t M, const uint64_t *__restrict__ skeys, uint32_t *__restrict__ heads) {
    const int64_t j = (int64_t)blockIdx.x * OB_THREADS + threadIdx.x;
    if (j >= M) return;
    const uint64_t k = skeys[j];
    heads[j] = (k < OB_KEY_RANGE && (j == 0 || skeys[j - 1] != k)) ? 1u : 0u;
}

// seg = the inclusive scan of heads: entry j of a cell belongs to voxel seg[j] - 1.  start[q] = the first sorted entry of voxel q, start[K] =
// the number of entries that have a cell; every slot has one writer
__global__ __launch_bounds__(OB_THREADS) void k_obs_segments(int64_t M, const uint64_t *__restrict__ skeys, const uint32_t *__restrict__ svals,
                                                             const uint32_t *__restrict__ seg, int32_t *__restrict__ inverse,
                                                             uint32_t *__restrict__ start) {
    const int64_t j = (int64_t)blockIdx.x * OB_THREADS + threadIdx.x;
    if (j >= M) return;
    const uint64_t k = skeys[j];
    const bool has = k < OB_KEY_RANGE;
    const uint32_t q = seg[j];
    inverse[svals[j]] = has ? (int32_t)q - 1 : -1;
    if (has && (j == 0 || skeys[j - 1] != k)) start[q - 1] = (uint32_t)j;
    if (has && (j == M - 1 || skeys[j + 1] >= OB_KEY_RANGE)) start[q] = (uint32_t)(j + 1);
    if (j == 0 && !has) start[0] = 0u;
}

// one wave per voxel; counters[0] = K is read from the device (the host does not know it)
__global__ __launch_bounds__(OB_THREADS) void k_obs_centroids(int64_t M, const float *__restrict__ points, const float *__restrict__ origin, float voxel,
                                                              const uint64_t *__restrict__ skeys, const uint32_t *__restrict__ svals,
                                                              const uint32_t *__restrict__ seg, const uint32_t *__restrict__ start,
                                                              float *__restrict__ centroid, int32_t *__restrict__ count) {
    const int64_t q = (int64_t)blockIdx.x * (OB_THREADS / 64) + (threadIdx.x >> 6);
    const int64_t K = seg[M - 1];
    if (q >= K) return;                                                            // (wave-uniform)
    const int lane = threadIdx.x & 63;
    const uint32_t lo = start[q], hi = start[q + 1];
    const uint64_t key = skeys[lo];
    const uint32_t cell_mask = (1u << OB_CELL_BITS) - 1u;
    const float corner[3] = {origin[0] + (float)(uint32_t)(key & cell_mask) * voxel,
                             origin[1] + (float)(uint32_t)((key >> OB_CELL_BITS) & cell_mask) * voxel,
                             origin[2] + (float)(uint32_t)((key >> (2 * OB_CELL_BITS)) & cell_mask) * voxel};
    float s[3] = {0.f, 0.f, 0.f};
    for (uint32_t j = lo + lane; j < hi; j += 64) {
        const int64_t i = svals[j];
        s[0] += points[3 * i] - corner[0];
        s[1] += points[3 * i + 1] - corner[1];
        s[2] += points[3 * i + 2] - corner[2];
    }
    wave_sum_each(s[0], s[1], s[2]);
    if (lane < 3) {
        const float n = (float)(hi - lo);
        const float sum = lane == 0 ? s[0] : (lane == 1 ? s[1] : s[2]);
        centroid[3 * q + lane] = corner[lane] + sum / n;
    }
    if (lane == 3) count[q] = (int32_t)(hi - lo);
}

// the first sorted entry whose key is >= k (M: none)
__device__ __forceinline__ int64_t obs_lower_bound(const uint64_t *__restrict__ skeys, int64_t M, uint64_t k) {
    int64_t lo = 0, hi = M;
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (skeys[mid] < k) lo = mid + 1; else hi = mid;
    }
    return lo;
}

__global__ void k_obs_voxel_counts(int64_t M, const uint64_t *__restrict__ skeys, const uint32_t *__restrict__ seg, int32_t *__restrict__ n_voxels,
                                   int32_t *__restrict__ n_outside) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    *n_voxels = (int32_t)seg[M - 1];
    *n_outside = (int32_t)(obs_lower_bound(skeys, M, OB_KEY_NONFINITE) - obs_lower_bound(skeys, M, OB_KEY_RANGE));
}

// ---- observable nodes: every writer stores the value 1 into flags zeroed on the stream before the launch
template <bool VEC>
__global__ __launch_bounds__(OB_THREADS) void k_obs_mark(int64_t total, int N, const int32_t *__restrict__ idx, const float *__restrict__ d2,
                                                         float max_sq_dist, uint8_t *__restrict__ flags) {
    const int64_t e0 = 4 * ((int64_t)blockIdx.x * OB_THREADS + threadIdx.x);
    if (e0 >= total) return;
    int32_t n[4];
    float d[4];
    if (VEC && e0 + 4 <= total) {
        const int4 a = *reinterpret_cast<const int4 *>(idx + e0);
        const float4 b = *reinterpret_cast<const float4 *>(d2 + e0);
        n[0] = a.x; n[1] = a.y; n[2] = a.z; n[3] = a.w;
        d[0] = b.x; d[1] = b.y; d[2] = b.z; d[3] = b.w;
    } else {
#pragma unroll
        for (int e = 0; e < 4; e++) {
            const bool live = e0 + e < total;
            n[e] = live ? idx[e0 + e] : -1;
            d[e] = live ? d2[e0 + e] : 0.f;
        }
    }
#pragma unroll
    for (int e = 0; e < 4; e++)
        if (n[e] >= 0 && n[e] < N && (max_sq_dist < 0.f || d[e] <= max_sq_dist)) flags[n[e]] = 1;
}

// do [a, a + na) and [b, b + nb) share a byte?  (a NULL or empty range shares none)
bool obs_overlap(const void *a, size_t na, const void *b, size_t nb) {
    if (!a || !b || na == 0 || nb == 0) return false;
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + nb && y < x + na;
}

struct ObsRange { const void *p; size_t n; };

// no output may share a byte with another operand; inputs may share among themselves.  `n_out` leading ranges are the outputs
bool obs_any_overlap(const ObsRange *r, int n, int n_out) {
    for (int i = 0; i < n_out; i++)
        for (int j = i + 1; j < n; j++)
            if (obs_overlap(r[i].p, r[i].n, r[j].p, r[j].n)) return true;
    return false;
}

struct UnprojectCarve { size_t sel, map, mtm, total; };
UnprojectCarve unproject_carve(int64_t n) {
    UnprojectCarve c;
    c.sel = 0;
    c.map = c.sel + align256((size_t)n);
    c.mtm = c.map + align256((size_t)n * 4);
    c.total = c.mtm + align256(csplat_mask_to_map_temp_bytes(n));
    return c;
}

struct VoxelCarve { size_t keys, vals, skeys, svals, heads, seg, start, origin, parts, sort, scan, total; };
VoxelCarve voxel_carve(int64_t M) {
    const size_t m = (size_t)(M > 0 ? M : 0);
    VoxelCarve c;
    size_t at = 0;
    auto take = [&](size_t bytes) { const size_t o = at; at += align256(bytes); return o; };
    c.keys = take(m * 8); c.vals = take(m * 4); c.skeys = take(m * 8); c.svals = take(m * 4);
    c.heads = take(m * 4); c.seg = take(m * 4); c.start = take((m + 1) * 4);
    c.origin = take(3 * 4); c.parts = take((size_t)OB_MIN_BLOCKS * 3 * 4);
    c.sort = take(csplat_sort_pairs_temp_bytes(M)); c.scan = take(csplat_scan_u32_temp_bytes(M));
    c.total = at;
    return c;
}

}  // namespace

extern "C" size_t csplat_obs_unproject_temp_bytes(int V, int H, int W) {
    if (V < 1 || H < 1 || W < 1) return 0;
    return unproject_carve((int64_t)V * H * W).total;
}

extern "C" int csplat_obs_unproject(void *stream, int V, int H, int W, const float *depth, const float *mask, const float *intrinsics,
                                    const float *cam_to_world, int stride, float max_depth, int kind, int64_t cap, float *points,
                                    int32_t *source, int32_t *count_dev, void *temp) {
    CSPLAT_REQUIRE(V >= 1 && V <= 65535, "csplat_obs_unproject: 1 <= V <= 65535");
    CSPLAT_REQUIRE(H >= 1 && W >= 1 && (int64_t)V * H * W < ((int64_t)1 << 31), "csplat_obs_unproject: H and W are >= 1, V * H * W < 2^31");
    CSPLAT_REQUIRE(stride >= 1, "csplat_obs_unproject: stride is >= 1");
    CSPLAT_REQUIRE(kind == 0 || kind == 1, "csplat_obs_unproject: kind is 0 (view-space z) or 1 (distance along the ray)");
    CSPLAT_REQUIRE(max_depth == max_depth, "csplat_obs_unproject: max_depth is a number (<= 0: none)");
    CSPLAT_REQUIRE(cap >= 0 && cap < ((int64_t)1 << 31), "csplat_obs_unproject: 0 <= cap < 2^31");
    CSPLAT_REQUIRE(depth && intrinsics && cam_to_world && count_dev && temp, "csplat_obs_unproject: a NULL operand");
    CSPLAT_REQUIRE(cap == 0 || (points && source), "csplat_obs_unproject: NULL points or source with cap > 0");
    CSPLAT_REQUIRE((((uintptr_t)depth | (uintptr_t)mask | (uintptr_t)intrinsics | (uintptr_t)cam_to_world | (uintptr_t)points |
                     (uintptr_t)source | (uintptr_t)count_dev) & 3u) == 0 && ((uintptr_t)temp & 15u) == 0,
                   "csplat_obs_unproject: operands must be 4-byte aligned, temp 16-byte aligned");
    const int64_t HW = (int64_t)H * W, n = (int64_t)V * HW;
    const UnprojectCarve c = unproject_carve(n);
    const ObsRange r[] = {{points, (size_t)cap * 12}, {source, (size_t)cap * 4}, {count_dev, 4}, {temp, c.total},
                          {depth, (size_t)n * 4}, {mask, (size_t)n * 4}, {intrinsics, (size_t)V * 16}, {cam_to_world, (size_t)V * 48}};
    CSPLAT_REQUIRE(!obs_any_overlap(r, 8, 4), "csplat_obs_unproject: an output or temp overlaps another operand");
    hipStream_t s = (hipStream_t)stream;
    uint8_t *sel = (uint8_t *)((char *)temp + c.sel);
    int32_t *map = (int32_t *)((char *)temp + c.map);
    const dim3 grid((unsigned)cdiv(HW + 3, 4 * OB_THREADS), (unsigned)V);      // (+ 3: the slots of a plane that begins off a 16-byte boundary)
    if (mask)
        k_obs_select<true><<<grid, OB_THREADS, 0, s>>>(W, HW, depth, mask, stride, max_depth, sel);
    else
        k_obs_select<false><<<grid, OB_THREADS, 0, s>>>(W, HW, depth, mask, stride, max_depth, sel);
    LAUNCH_CHECK();
    if (int rc = csplat_mask_to_map(stream, n, sel, 0, map, count_dev, (char *)temp + c.mtm)) return rc;
    if (cap == 0) return 0;
    if (kind == 0)
        k_obs_points<0><<<grid, OB_THREADS, 0, s>>>(W, HW, depth, intrinsics, cam_to_world, map, cap, points, source);
    else
        k_obs_points<1><<<grid, OB_THREADS, 0, s>>>(W, HW, depth, intrinsics, cam_to_world, map, cap, points, source);
    LAUNCH_CHECK();
    return 0;
}

extern "C" size_t csplat_obs_voxel_temp_bytes(int64_t M) { return voxel_carve(M).total; }

extern "C" int csplat_obs_voxel(void *stream, int64_t M, const float *points, float voxel, const float *origin, float *centroid, int32_t *count,
                                int32_t *inverse, int32_t *n_voxels, int32_t *n_outside, void *temp) {
    CSPLAT_REQUIRE(M >= 0 && M < ((int64_t)1 << 31), "csplat_obs_voxel: 0 <= M < 2^31");
    CSPLAT_REQUIRE(voxel > 0.f && voxel < __builtin_inff(), "csplat_obs_voxel: voxel is a finite size > 0");
    CSPLAT_REQUIRE(n_voxels && n_outside, "csplat_obs_voxel: a NULL counter");
    CSPLAT_REQUIRE((((uintptr_t)n_voxels | (uintptr_t)n_outside) & 3u) == 0, "csplat_obs_voxel: operands must be 4-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    if (M == 0) {
        HIP_TRY(hipMemsetAsync(n_voxels, 0, 4, s));
        HIP_TRY(hipMemsetAsync(n_outside, 0, 4, s));
        return 0;
    }
    CSPLAT_REQUIRE(points && centroid && count && inverse && temp, "csplat_obs_voxel: a NULL operand");
    CSPLAT_REQUIRE((((uintptr_t)points | (uintptr_t)origin | (uintptr_t)centroid | (uintptr_t)count | (uintptr_t)inverse) & 3u) == 0 &&
                       ((uintptr_t)temp & 15u) == 0, "csplat_obs_voxel: operands must be 4-byte aligned, temp 16-byte aligned");
    const VoxelCarve c = voxel_carve(M);
    const ObsRange r[] = {{centroid, (size_t)M * 12}, {count, (size_t)M * 4}, {inverse, (size_t)M * 4}, {n_voxels, 4}, {n_outside, 4},
                          {temp, c.total}, {points, (size_t)M * 12}, {origin, 12}};
    CSPLAT_REQUIRE(!obs_any_overlap(r, 8, 6), "csplat_obs_voxel: an output or temp overlaps another operand");
    char *t = (char *)temp;
    uint64_t *keys = (uint64_t *)(t + c.keys), *skeys = (uint64_t *)(t + c.skeys);
    uint32_t *vals = (uint32_t *)(t + c.vals), *svals = (uint32_t *)(t + c.svals);
    uint32_t *heads = (uint32_t *)(t + c.heads), *seg = (uint32_t *)(t + c.seg), *start = (uint32_t *)(t + c.start);
    const unsigned blocks = (unsigned)cdiv(M, OB_THREADS);
    if (!origin) {
        float *o = (float *)(t + c.origin), *parts = (float *)(t + c.parts);
        const int n_parts = (int)(blocks < (unsigned)OB_MIN_BLOCKS ? blocks : (unsigned)OB_MIN_BLOCKS);
        k_obs_min_part<<<n_parts, OB_THREADS, 0, s>>>(M, points, parts);
        LAUNCH_CHECK();
        k_obs_min_final<<<1, OB_THREADS, 0, s>>>(n_parts, parts, o);
        LAUNCH_CHECK();
        origin = o;
    }
    k_obs_keys<<<blocks, OB_THREADS, 0, s>>>(M, points, origin, voxel, keys, vals);
    LAUNCH_CHECK();
    if (int rc = csplat_sort_pairs_u64(stream, M, 64, keys, vals, skeys, svals, t + c.sort)) return rc;
    k_obs_heads<<<blocks, OB_THREADS, 0, s>>>(M, skeys, heads);
    LAUNCH_CHECK();
    if (int rc = csplat_scan_u32(stream, M, heads, seg, t + c.scan)) return rc;
    k_obs_segments<<<blocks, OB_THREADS, 0, s>>>(M, skeys, svals, seg, inverse, start);
    LAUNCH_CHECK();
    // K <= M is known on the device only: one wave per possible voxel, the waves beyond K leave at once
    k_obs_centroids<<<(unsigned)cdiv(M, OB_THREADS / 64), OB_THREADS, 0, s>>>(M, points, origin, voxel, skeys, svals, seg, start, centroid, count);
    LAUNCH_CHECK();
    k_obs_voxel_counts<<<1, 64, 0, s>>>(M, skeys, seg, n_voxels, n_outside);
    LAUNCH_CHECK();
    return 0;
}

extern "C" int csplat_obs_mark(void *stream, int64_t Q, int K, int N, const int32_t *idx, const float *d2, float max_sq_dist, uint8_t *flags) {
    CSPLAT_REQUIRE(Q >= 0 && Q < ((int64_t)1 << 31) && K >= 1 && Q * (int64_t)K < ((int64_t)1 << 31), "csplat_obs_mark: Q >= 0, K >= 1, Q * K < 2^31");
    CSPLAT_REQUIRE(N >= 0, "csplat_obs_mark: N is >= 0");
    CSPLAT_REQUIRE(max_sq_dist == max_sq_dist, "csplat_obs_mark: max_sq_dist is a number (< 0: none)");
    if (N == 0) return 0;
    CSPLAT_REQUIRE(flags, "csplat_obs_mark: NULL flags");
    const int64_t total = Q * (int64_t)K;
    CSPLAT_REQUIRE(total == 0 || (idx && d2), "csplat_obs_mark: a NULL operand");
    CSPLAT_REQUIRE((((uintptr_t)idx | (uintptr_t)d2) & 3u) == 0, "csplat_obs_mark: operands must be 4-byte aligned");
    CSPLAT_REQUIRE(!obs_overlap(flags, (size_t)N, idx, (size_t)total * 4) && !obs_overlap(flags, (size_t)N, d2, (size_t)total * 4),
                   "csplat_obs_mark: flags overlaps another operand");
    hipStream_t s = (hipStream_t)stream;
    HIP_TRY(hipMemsetAsync(flags, 0, (size_t)N, s));
    if (total == 0) return 0;
    const unsigned blocks = (unsigned)cdiv(total, 4 * OB_THREADS);
    if ((((uintptr_t)idx | (uintptr_t)d2) & 15u) == 0)
        k_obs_mark<true><<<blocks, OB_THREADS, 0, s>>>(total, N, idx, d2, max_sq_dist, flags);
    else
        k_obs_mark<false><<<blocks, OB_THREADS, 0, s>>>(total, N, idx, d2, max_sq_dist, flags);
    LAUNCH_CHECK();
    return 0;
}
