// csplat_knn.hip -- exact nearest-neighbour searches for gfx950: simple_knn._C.distCUDA2 (the CUDA extension called
// from scene_reconstruction/gaussian_mesh.py and gaussian_model.py), k-NN with indices inside one cloud and between two clouds,
// farthest-point sampling, the one-sided Chamfer distance and trajectory smoothing.
//
// Every search is one query per lane against candidates that the whole wave reads at the same address (an LDS or cache broadcast), the
// best entries kept in registers.  The distance is dx*dx + dy*dy + dz*dz with FP contraction off, the association order of
// oracle/knn_ref.c, so every form returns the oracle's bits.  The building blocks, each defined once:
//   knn_d2 / knn_box_d2     squared distance query-to-candidate / query-to-bounding-box
//   best3_insert            the list of a distCUDA2 lane: three sorted distances in three registers
//   KBest<CAP>              the list of a k-NN lane: K (d2, index) pairs, CAP in {4, 8, 16, 32}; init, worst, offer, offer4, store
//   ExclSelf / ExclNone / ExclNonFinite   which candidates a scan leaves out
//   knn_scan_slabs          brute force: all N candidates through LDS in KNN_SLAB-point slabs, four per step
//   knn_scan_sorted         a stretch [lo, hi) of the Morton-sorted float4 copy of the points, four per step
//   knn_scan_boxes          every KNN_BOX run of that copy whose box is not beyond the lane's worst entry, a seeded stretch left out
//   block_minmax6_store     a workgroup's min / max of three coordinates
//   k_bbox_partial, k_morton<SHIFT>, k_knn_boxes + knn_order_points   the host pass that makes the sorted copy and its boxes
//   PairSortWs / KnnWs / KnnQueryWs / ChamferWs   the layouts of the `temp` buffers
// Which entry uses which:
//   csplat_dist2            k_dist2            best3_insert, a slab loop of its own (one candidate per step; in the shared scan it measured 1 % slower)
//   csplat_dist2_ws         k_knn_search       best3_insert, knn_order_points, a box loop of its own (a reject bound from +-3 curve neighbours, no stretch left out)
//   csplat_knn              k_knn_brute        KBest, a slab loop of its own (knn_scan_slabs with the query's own point left out: 0.5 % slower)
//   csplat_knn_ws           k_knn_search_k     KBest, knn_order_points, knn_scan_sorted + knn_scan_boxes(ExclSelf) around the wave's own position
//   csplat_knn_query        k_knn_query_brute  KBest, knn_scan_slabs(ExclNone)
//   csplat_knn_query_ws     k_knn_query_search KBest, knn_order_points + the queries' own sort, knn_scan_sorted + knn_scan_boxes(ExclNone)
//                                              around a binary search of the wave's first query code
//   csplat_traj_smooth      k_traj_smooth      KBest, knn_scan_slabs(ExclNonFinite) per frame, then the weighted mean from the list
//   csplat_fps, csplat_chamfer_fwd / _bwd      kernels of their own (k_fps, k_chamfer_*); the Chamfer backward sorts through a PairSortWs
#include "csplat_common.h"
#include "csplat_device.h"

namespace {
constexpr int KNN_THREADS = 256;
constexpr int KNN_SLAB = 1024;
constexpr int KNN_BOX = 1024;
constexpr int KNN_IDX_NONE = 0x7fffffff;   // index of an empty slot and of a left-out candidate: never precedes anything

// squared distance from the query (x, y, z) to the candidate (cx, cy, cz).  The pragma is lexical: it has to stand in here.
__device__ __forceinline__ float knn_d2(float cx, float cy, float cz, float x, float y, float z) {
#pragma clang fp contract(off)
    const float dx = cx - x, dy = cy - y, dz = cz - z;
    return dx * dx + dy * dy + dz * dz;
}

// squared distance from the query to the box bx = (min x, y, z, max x, y, z); 0 inside
__device__ __forceinline__ float knn_box_d2(float px, float py, float pz, const float *__restrict__ bx) {
#pragma clang fp contract(off)
    float ex = 0.f, ey = 0.f, ez = 0.f;     // distance from the query to the box, per axis
    if (px < bx[0] || px > bx[3]) ex = fminf(fabsf(px - bx[0]), fabsf(px - bx[3]));
    if (py < bx[1] || py > bx[4]) ey = fminf(fabsf(py - bx[1]), fabsf(py - bx[4]));
    if (pz < bx[2] || pz > bx[5]) ez = fminf(fabsf(pz - bx[2]), fabsf(pz - bx[5]));
    return ex * ex + ey * ey + ez * ez;
}

// ---- the list of a lane.  distCUDA2 keeps the three smallest distances (b0 <= b1 <= b2) in three registers, no indices: it needs
// their mean only.
__device__ __forceinline__ void best3_insert(float d, float &b0, float &b1, float &b2) {
    const float n2 = fminf(b2, fmaxf(b1, d));
    const float n1 = fminf(b1, fmaxf(b0, d));
    const float n0 = fminf(b0, d);
    b0 = n0; b1 = n1; b2 = n2;
}

// KBest<CAP>: the K best (d2, index) pairs in registers, CAP in {4, 8, 16, 32}, every access through a fully unrolled loop (a
// runtime-indexed private array would go to scratch memory).  Slots [0, CAP-K) hold the pair (-inf, -1), which no candidate can
// precede, so the K real entries sit in slots [CAP-K, CAP) and slot CAP-1 is always the K-th best -- the skip test and the box
// rejection use the exact bound for every K, not the bound of the rounded-up capacity.  Pairs are ordered by (d2, index): the
// result does not depend on the order in which candidates arrive, which is what lets the Morton-ordered form return the same bits
// and indices as the brute-force one.
template <int CAP> struct KBest {
    float d[CAP];
    int id[CAP];
    __device__ __forceinline__ void init(int K) {   // K = 0: a list that accepts nothing (lanes without a query)
#pragma unroll
        for (int r = 0; r < CAP; r++) {
            const bool dead = r < CAP - K;
            d[r] = dead ? -INFINITY : INFINITY;
            id[r] = dead ? -1 : KNN_IDX_NONE;
        }
    }
    __device__ __forceinline__ float worst() const { return d[CAP - 1]; }
    __device__ __forceinline__ bool before(float cd, int ci, int r) const { return cd < d[r] || (cd == d[r] && ci < id[r]); }
    // sorted insert; a pair that does not precede the worst entry changes nothing
    __device__ __forceinline__ void insert(float cd, int ci) {
        bool here = before(cd, ci, CAP - 1);
#pragma unroll
        for (int r = CAP - 1; r > 0; r--) {
            const bool above = before(cd, ci, r - 1);   // the candidate goes above slot r: slot r takes its upper neighbour
            d[r] = above ? d[r - 1] : (here ? cd : d[r]);
            id[r] = above ? id[r - 1] : (here ? ci : id[r]);
            here = above;
        }
        d[0] = here ? cd : d[0];
        id[0] = here ? ci : id[0];
    }
    // one candidate against one query per lane.  The wave tests the candidate against every lane's K-th best first and skips the
    // insert together; `<=` (not the full pair order) keeps the test at one compare -- an equal distance enters the insert, which
    // then decides by index.
    __device__ __forceinline__ void offer(float cd, int ci, bool excl) {
        cd = excl ? INFINITY : cd;
        ci = excl ? KNN_IDX_NONE : ci;
        if (__builtin_amdgcn_ballot_w64(cd <= worst()) != 0ull) insert(cd, ci);
    }
    // four candidates at once: one wave-wide test and one branch for the four (after the first few hundred candidates almost every
    // group is skipped whole), then the single-candidate path for a group in which some lane still needs one
    __device__ __forceinline__ void offer4(const float (&cd)[4], const int (&ci)[4], const bool (&excl)[4]) {
        const float w = worst();
        const bool any = (!excl[0] && cd[0] <= w) || (!excl[1] && cd[1] <= w) || (!excl[2] && cd[2] <= w) || (!excl[3] && cd[3] <= w);
        if (__builtin_amdgcn_ballot_w64(any) == 0ull) return;
#pragma unroll
        for (int u = 0; u < 4; u++) offer(cd[u], ci[u], excl[u]);
    }
    __device__ __forceinline__ void store(int K, size_t row, float *__restrict__ out_d2, int32_t *__restrict__ out_idx) const {
#pragma unroll
        for (int s = 0; s < CAP; s++) {
            const int r = s - (CAP - K);
            if (r >= 0) {
                out_d2[row * K + r] = d[s];                              // an empty slot still holds +inf
                out_idx[row * K + r] = id[s] == KNN_IDX_NONE ? -1 : id[s];
            }
        }
    }
};

// ---- which candidates a scan leaves out, from the candidate's position in the array the scan walks and its squared distance.  A
// left-out candidate is offered as (+inf, KNN_IDX_NONE): it changes nothing.
struct ExclSelf { int self; __device__ __forceinline__ bool operator()(int pos, float) const { return pos == self; } };   // the query's own point
struct ExclNone { __device__ __forceinline__ bool operator()(int, float) const { return false; } };
struct ExclNonFinite { __device__ __forceinline__ bool operator()(int, float d) const { return !finite_f32(d); } };

// ---- the scans.  Each takes the lane's list BY VALUE and returns it (`b = knn_scan_...(b, ...)`).  With a `List &` parameter the
// compiler keeps a second copy of the whole list live across the inner loop, `__restrict__` or not: measured, KBest<32> +24 VGPRs and
// one occupancy step down.
//
// brute force: pts[0 .. N) against the query (x, y, z) of every lane, through LDS in slabs of KNN_SLAB points (every lane reads the
// same LDS word -> broadcast, no bank conflicts).  All KNN_THREADS lanes of the workgroup must call it together (barriers).  N = 0:
// nothing is read.
template <class List, class Excl>
__device__ __forceinline__ List knn_scan_slabs(List b, const float *__restrict__ pts, int N, float x, float y, float z, Excl excl) {
    __shared__ float s_p[KNN_SLAB * 3];
    for (int base = 0; base < N; base += KNN_SLAB) {
        const int cnt = min(KNN_SLAB, N - base);
        __syncthreads();
        for (int k = threadIdx.x; k < cnt * 3; k += KNN_THREADS) s_p[k] = pts[(size_t)base * 3 + k];
        __syncthreads();
        int j = 0;
        for (; j + 4 <= cnt; j += 4) {
            float d[4];
            int ci[4];
            bool ex[4];
#pragma unroll
            for (int u = 0; u < 4; u++) {
                d[u] = knn_d2(s_p[3 * (j + u)], s_p[3 * (j + u) + 1], s_p[3 * (j + u) + 2], x, y, z);
                ci[u] = base + j + u;
                ex[u] = excl(ci[u], d[u]);
            }
            b.offer4(d, ci, ex);
        }
        for (; j < cnt; j++) {
            const float d = knn_d2(s_p[3 * j], s_p[3 * j + 1], s_p[3 * j + 2], x, y, z);
            b.offer(d, base + j, excl(base + j, d));
        }
    }
    return b;
}

// ---- pruned forms.  spts: the points in Morton order, .w = the caller's index.  Positions [lo, hi) of it (what `excl` sees);
// wave-uniform addresses: one broadcast load per candidate.
template <class List, class Excl>
__device__ __forceinline__ List knn_scan_sorted(List b, const float4 *__restrict__ spts, int lo, int hi, float x, float y, float z, Excl excl) {
    int j = lo;
    for (; j + 4 <= hi; j += 4) {
        float d[4];
        int ci[4];
        bool ex[4];
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const float4 c = spts[j + u];
            d[u] = knn_d2(c.x, c.y, c.z, x, y, z);
            ci[u] = (int)__float_as_uint(c.w);
            ex[u] = excl(j + u, d[u]);         // by position: the test does not wait for the load
        }
        b.offer4(d, ci, ex);
    }
    for (; j < hi; j++) {
        const float4 c = spts[j];
        const float d = knn_d2(c.x, c.y, c.z, x, y, z);
        b.offer(d, (int)__float_as_uint(c.w), excl(j, d));
    }
    return b;
}

// every box (a run of KNN_BOX positions of spts) that is not farther than the lane's current worst entry, leaving out the stretch
// [wlo, whi) that seeded the lists.  Rejection is strict (`>`): a box at exactly the K-th distance may hold an equal distance with a
// smaller index.  The wave skips a box together; lanes that do not need it scan along.
template <class List, class Excl>
__device__ __forceinline__ List knn_scan_boxes(List b, const float4 *__restrict__ spts, const float *__restrict__ boxes, int nbox, int N,
                                               float x, float y, float z, int wlo, int whi, Excl excl) {
    for (int bi = 0; bi < nbox; bi++) {
        const bool need = !(knn_box_d2(x, y, z, boxes + 6 * bi) > b.worst());   // lanes without a query hold -inf and never need a box
        if (__builtin_amdgcn_ballot_w64(need) == 0ull) continue;
        const int lo = bi * KNN_BOX, hi = min(N, lo + KNN_BOX);
        b = knn_scan_sorted(b, spts, lo, min(hi, wlo), x, y, z, excl);
        b = knn_scan_sorted(b, spts, max(lo, whi), hi, x, y, z, excl);
    }
    return b;
}

// ---- distCUDA2, brute force: the mean of the three smallest squared distances to the other points.  Self is excluded by index, so
// coincident points contribute 0 exactly as upstream.  One candidate per step with a plain insert -- no ballot, nothing to skip -- so
// the slab loop is its own: through knn_scan_slabs (four per step and a tail) it measured 1 % slower at P = 4000 and 10 000.
__global__ __launch_bounds__(KNN_THREADS) void k_dist2(int P, const float *__restrict__ pts, float *__restrict__ out) {
#pragma clang fp contract(off)
    __shared__ float s_p[KNN_SLAB * 3];
    const int i = blockIdx.x * KNN_THREADS + threadIdx.x;
    const bool live = i < P;
    const float x = live ? pts[3 * i] : 0.f, y = live ? pts[3 * i + 1] : 0.f, z = live ? pts[3 * i + 2] : 0.f;
    float b0 = INFINITY, b1 = INFINITY, b2 = INFINITY;
    for (int base = 0; base < P; base += KNN_SLAB) {
        const int cnt = min(KNN_SLAB, P - base);
        __syncthreads();
        for (int k = threadIdx.x; k < cnt * 3; k += KNN_THREADS) s_p[k] = pts[(size_t)base * 3 + k];
        __syncthreads();
        const int self = i - base;  // index of this lane's own point inside the slab, if any
#pragma unroll 4
        for (int j = 0; j < cnt; j++) {
            const float d = knn_d2(s_p[3 * j], s_p[3 * j + 1], s_p[3 * j + 2], x, y, z);
            best3_insert((j == self) ? INFINITY : d, b0, b1, b2);
        }
    }
    if (live) out[i] = (b0 + b1 + b2) / 3.0f;
}

// ---- the point-ordering pass of the pruned forms (the brute-force kernels are O(P^2): 4.9 ms at P = 1e5, 0.5 s at 1e6).
// Same pruning as the upstream extension: points are ordered along a Morton curve and every run of KNN_BOX consecutive points
// gets its bounding box.

// the workgroup's (256 lanes) minimum of mn[0..3) and maximum of mx[0..3) over all lanes: dst[0..3) = min, dst[3..6) = max
__device__ __forceinline__ void block_minmax6_store(const float (&mn)[3], const float (&mx)[3], float *__restrict__ dst) {
    __shared__ float s[6][4];
    for (int a = 0; a < 3; a++) {
        float lo = mn[a], hi = mx[a];      // (its own loop: minimum and maximum in step; one after the other, wave_min then wave_max, timed above the parent)
        for (int o = 32; o > 0; o >>= 1) { lo = fminf(lo, __shfl_xor(lo, o, 64)); hi = fmaxf(hi, __shfl_xor(hi, o, 64)); }
        if ((threadIdx.x & 63) == 0) { s[a][threadIdx.x >> 6] = lo; s[3 + a][threadIdx.x >> 6] = hi; }
    }
    __syncthreads();
    if (threadIdx.x < 6) {
        const float *r = s[threadIdx.x];
        dst[threadIdx.x] = threadIdx.x < 3 ? fminf(fminf(r[0], r[1]), fminf(r[2], r[3])) : fmaxf(fmaxf(r[0], r[1]), fmaxf(r[2], r[3]));
    }
}

__global__ __launch_bounds__(256) void k_bbox_partial(int P, const float *__restrict__ pts, float *__restrict__ part) {
    float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int i = blockIdx.x * 256 + threadIdx.x; i < P; i += gridDim.x * 256)
        for (int a = 0; a < 3; a++) { const float v = pts[3 * i + a]; mn[a] = fminf(mn[a], v); mx[a] = fmaxf(mx[a], v); }
    block_minmax6_store(mn, mx, part + blockIdx.x * 6);
}

__device__ __forceinline__ uint64_t spread21(uint32_t v) {   // bit i -> bit 3 i
    uint64_t x = v & 0x1FFFFFu;
    x = (x | x << 32) & 0x1F00000000FFFFull;
    x = (x | x << 16) & 0x1F0000FF0000FFull;
    x = (x | x << 8) & 0x100F00F00F00F00Full;
    x = (x | x << 4) & 0x10C30C30C30C30C3ull;
    x = (x | x << 2) & 0x1249249249249249ull;
    return x;
}

// the queries are ordered by the upper 31 bits of their 63-bit code (10 levels of the octree and one bit more): four passes of the
// radix sort instead of eight, and no coarser a grouping than that for any cloud of fewer than 2^30 queries
constexpr int KNN_QUERY_CODE_SHIFT = 32, KNN_QUERY_CODE_BITS = 63 - KNN_QUERY_CODE_SHIFT;

// 63-bit Morton codes (>> SHIFT) of pts in the bounding box that `part` holds (the partials of k_bbox_partial); a point outside
// the box clamps to its faces.  SHIFT = 0: the points themselves.  SHIFT = KNN_QUERY_CODE_SHIFT: the queries of the two-cloud search
// in the POINTS' box -- their codes only group nearby queries in one wave, the search is exact for any order.
template <int SHIFT>
__global__ __launch_bounds__(256) void k_morton(int P, int nparts, const float *__restrict__ pts, const float *__restrict__ part,
                                                uint64_t *__restrict__ codes, uint32_t *__restrict__ ids) {
    __shared__ float s_box[6];
    if (threadIdx.x < 6) {
        float v = part[threadIdx.x];
        for (int b = 1; b < nparts; b++) v = threadIdx.x < 3 ? fminf(v, part[b * 6 + threadIdx.x]) : fmaxf(v, part[b * 6 + threadIdx.x]);
        s_box[threadIdx.x] = v;
    }
    __syncthreads();
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= P) return;
    uint32_t q[3];
    for (int a = 0; a < 3; a++) {
        const float ext = s_box[3 + a] - s_box[a];
        const float t = ext > 0.f ? (pts[3 * (size_t)i + a] - s_box[a]) / ext : 0.f;
        q[a] = (uint32_t)fminf(fmaxf(t * 2097151.f, 0.f), 2097151.f);
    }
    codes[i] = (spread21(q[0]) | spread21(q[1]) << 1 | spread21(q[2]) << 2) >> SHIFT;
    ids[i] = (uint32_t)i;
}

// sorted copy of the points (x, y, z, original index) + one bounding box per KNN_BOX run
__global__ __launch_bounds__(256) void k_knn_boxes(int P, const float *__restrict__ pts, const uint32_t *__restrict__ ids,
                                                   float4 *__restrict__ spts, float *__restrict__ boxes) {
    const int base = blockIdx.x * KNN_BOX;
    float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int j = threadIdx.x; j < KNN_BOX && base + j < P; j += 256) {
        const uint32_t id = ids[base + j];
        const float x = pts[3 * id], y = pts[3 * id + 1], z = pts[3 * id + 2];
        spts[base + j] = make_float4(x, y, z, __uint_as_float(id));
        mn[0] = fminf(mn[0], x); mn[1] = fminf(mn[1], y); mn[2] = fminf(mn[2], z);
        mx[0] = fmaxf(mx[0], x); mx[1] = fmaxf(mx[1], y); mx[2] = fmaxf(mx[2], z);
    }
    block_minmax6_store(mn, mx, boxes + blockIdx.x * 6);
}

// ---- distCUDA2, pruned form: a query first bounds its 3rd-nearest distance with its +-3 curve neighbours (`reject`), restarts, and
// then scans only the boxes whose distance to it exceeds neither that bound nor the current 3rd best -- a loop of its own: no stretch
// is left out.  The result is the same multiset of three smallest squared distances, summed in ascending order as before:
// bit-identical to the brute-force kernel (tested).
__global__ __launch_bounds__(256) void k_knn_search(int P, int nbox, const float4 *__restrict__ spts, const float *__restrict__ boxes,
                                                    float *__restrict__ out) {
#pragma clang fp contract(off)
    const int i = blockIdx.x * 256 + threadIdx.x;
    const bool live = i < P;
    const float4 p = spts[live ? i : P - 1];
    float b0 = INFINITY, b1 = INFINITY, b2 = INFINITY;
    if (live) {
        for (int j = max(0, i - 3); j <= min(P - 1, i + 3); j++) {
            if (j == i) continue;
            const float4 c = spts[j];
            best3_insert(knn_d2(c.x, c.y, c.z, p.x, p.y, p.z), b0, b1, b2);
        }
    }
    const float reject = b2;
    b0 = b1 = b2 = INFINITY;
    for (int b = 0; b < nbox; b++) {
        const float *bx = boxes + 6 * b;        // knn_box_d2 spelled out: through the helper this kernel measured 2 % slower at P = 100 000
        float ex = 0.f, ey = 0.f, ez = 0.f;
        if (p.x < bx[0] || p.x > bx[3]) ex = fminf(fabsf(p.x - bx[0]), fabsf(p.x - bx[3]));
        if (p.y < bx[1] || p.y > bx[4]) ey = fminf(fabsf(p.y - bx[1]), fabsf(p.y - bx[4]));
        if (p.z < bx[2] || p.z > bx[5]) ez = fminf(fabsf(p.z - bx[2]), fabsf(p.z - bx[5]));
        const float dist = ex * ex + ey * ey + ez * ez;
        const bool need = live && !(dist > reject || dist > b2);
        if (__builtin_amdgcn_ballot_w64(need) == 0ull) continue;   // the wave skips the box together; lanes that do not need it scan along
        const int lo = b * KNN_BOX, hi = min(P, lo + KNN_BOX);
#pragma unroll 4
        for (int j = lo; j < hi; j++) {          // wave-uniform address: one broadcast load per candidate
            const float4 c = spts[j];
            const float d = knn_d2(c.x, c.y, c.z, p.x, p.y, p.z);
            best3_insert((j == i) ? INFINITY : d, b0, b1, b2);
        }
    }
    if (live) out[__float_as_uint(p.w)] = (b0 + b1 + b2) / 3.0f;
}

// ---- the `temp` buffers.  PairSortWs: what one csplat_sort_pairs call of n (u64 key, u32 value) pairs needs; the sorted pairs land
// in keys_o / vals_o.
struct WsCarve {
    size_t o = 0;
    size_t take(size_t b) { const size_t at = o; o += align256(b); return at; }
};
struct PairSortWs {
    size_t keys, vals, keys_o, vals_o, keys_t, vals_t, stab;
    void carve(WsCarve &c, size_t n) {
        keys = c.take(n * 8); vals = c.take(n * 4); keys_o = c.take(n * 8); vals_o = c.take(n * 4);
        keys_t = c.take(n * 8); vals_t = c.take(n * 4); stab = c.take(csplat_sort_temp_bytes((int64_t)n));
    }
    uint64_t *k(char *t) const { return (uint64_t *)(t + keys); }
    uint32_t *v(char *t) const { return (uint32_t *)(t + vals); }
    uint64_t *k_sorted(char *t) const { return (uint64_t *)(t + keys_o); }
    uint32_t *v_sorted(char *t) const { return (uint32_t *)(t + vals_o); }
    int sort(hipStream_t s, char *t, int64_t n, int end_bit) const {
        return csplat_sort_pairs(s, k(t), v(t), k_sorted(t), v_sorted(t), (uint64_t *)(t + keys_t), (uint32_t *)(t + vals_t), n, end_bit, t + stab);
    }
};

// the pruned forms' buffer for a cloud of P points: the bounding-box partials, the (code, index) sort, the sorted copy, the boxes
struct KnnWs { size_t part; PairSortWs sort; size_t spts, boxes, total; };
KnnWs knn_ws(int P) {
    KnnWs w;
    WsCarve c;
    const size_t n = (size_t)(P > 0 ? P : 1);
    w.part = c.take(256 * 6 * 4);
    w.sort.carve(c, n);
    w.spts = c.take(n * 16); w.boxes = c.take((size_t)cdiv((int)n, KNN_BOX) * 6 * 4);
    w.total = c.o;
    return w;
}

// the two-cloud form: the points' side as above, unchanged, then the queries' (code, index) sort
struct KnnQueryWs { KnnWs pts; PairSortWs qsort; size_t total; };
KnnQueryWs knn_query_ws(int Q, int N) {
    KnnQueryWs w;
    w.pts = knn_ws(N);
    WsCarve c{w.pts.total};
    w.qsort.carve(c, (size_t)(Q > 0 ? Q : 1));
    w.total = c.o;
    return w;
}

struct ChamferWs { PairSortWs sort; size_t total; };
ChamferWs chamfer_ws(int Q) {
    ChamferWs w;
    WsCarve c;
    w.sort.carve(c, (size_t)(Q > 0 ? Q : 1));
    w.total = c.o;
    return w;
}

// Orders the N >= 1 points for a pruned search: bounding box, Morton codes, radix sort, then the sorted float4 copy at temp + w.spts and
// one box per KNN_BOX run at temp + w.boxes.  The sorted codes stay at w.sort.k_sorted(temp), the box partials at temp + w.part.
int knn_order_points(hipStream_t s, int N, const float *points, char *t, const KnnWs &w, int *nparts, int *nbox) {
    *nparts = N < 256 * 256 ? cdiv(N, 256) : 256;
    *nbox = cdiv(N, KNN_BOX);
    k_bbox_partial<<<*nparts, 256, 0, s>>>(N, points, (float *)(t + w.part));
    LAUNCH_CHECK();
    k_morton<0><<<cdiv(N, 256), 256, 0, s>>>(N, *nparts, points, (const float *)(t + w.part), w.sort.k(t), w.sort.v(t));
    LAUNCH_CHECK();
    if (int rc = w.sort.sort(s, t, N, 63)) return rc;
    k_knn_boxes<<<*nbox, 256, 0, s>>>(N, points, w.sort.v_sorted(t), (float4 *)(t + w.spts), (float *)(t + w.boxes));
    LAUNCH_CHECK();
    return 0;
}
}  // namespace

#define KNN_BY_CAPACITY(K, LAUNCH)                                  \
    do {                                                            \
        if ((K) <= 4) { LAUNCH(4); } else if ((K) <= 8) { LAUNCH(8); } else if ((K) <= 16) { LAUNCH(16); } else { LAUNCH(32); } \
    } while (0)

extern "C" int csplat_dist2(void *stream, int P, const float *xyz, float *out) {
    CSPLAT_REQUIRE(P >= 0, "csplat_dist2: bad P");
    if (P == 0) return 0;
    ProfScope ps(PROF_KNN, (hipStream_t)stream);
    k_dist2<<<cdiv(P, KNN_THREADS), KNN_THREADS, 0, (hipStream_t)stream>>>(P, xyz, out);
    LAUNCH_CHECK();
    return 0;
}

extern "C" size_t csplat_dist2_temp_bytes(int P) { return knn_ws(P).total; }

// workspace form: Morton order + box pruning (exact; same bits as csplat_dist2).  temp: csplat_dist2_temp_bytes(P) bytes.
extern "C" int csplat_dist2_ws(void *stream, int P, const float *xyz, float *out, void *temp) {
    CSPLAT_REQUIRE(P >= 0, "csplat_dist2_ws: bad P");
    if (P == 0) return 0;
    CSPLAT_REQUIRE(xyz && out && temp, "csplat_dist2_ws: NULL argument");
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps(PROF_KNN, s);
    const KnnWs w = knn_ws(P);
    char *t = (char *)temp;
    int nparts, nbox;
    if (int rc = knn_order_points(s, P, xyz, t, w, &nparts, &nbox)) return rc;
    k_knn_search<<<cdiv(P, 256), 256, 0, s>>>(P, nbox, (const float4 *)(t + w.spts), (const float *)(t + w.boxes), out);
    LAUNCH_CHECK();
    return 0;
}

// ---- exact k-NN with indices inside one cloud (csplat_knn / csplat_knn_ws)
namespace {
template <int CAP>
__global__ __launch_bounds__(KNN_THREADS) void k_knn_brute(int P, int K, const float *__restrict__ pts, float *__restrict__ out_d2,
                                                           int32_t *__restrict__ out_idx) {
    const int i = blockIdx.x * KNN_THREADS + threadIdx.x;
    const bool live = i < P;
    const float x = live ? pts[3 * (size_t)i] : 0.f, y = live ? pts[3 * (size_t)i + 1] : 0.f, z = live ? pts[3 * (size_t)i + 2] : 0.f;
    KBest<CAP> b;
    b.init(live ? K : 0);
    // the slab loop of knn_scan_slabs, spelled out with the query's own point left out: through the shared scan this kernel measured
    // 0.4 to 0.5 % slower at P = 100 000 in every run (profiles/knn_refactor_before_after.txt); so it is the former kernel to the instruction
    __shared__ float s_p[KNN_SLAB * 3];
    for (int base = 0; base < P; base += KNN_SLAB) {
        const int cnt = min(KNN_SLAB, P - base);
        __syncthreads();
        for (int k = threadIdx.x; k < cnt * 3; k += KNN_THREADS) s_p[k] = pts[(size_t)base * 3 + k];
        __syncthreads();
        const int self = i - base;
        int j = 0;
        for (; j + 4 <= cnt; j += 4) {
            float d[4];
            int ci[4];
            bool me[4];
#pragma unroll
            for (int u = 0; u < 4; u++) {
                d[u] = knn_d2(s_p[3 * (j + u)], s_p[3 * (j + u) + 1], s_p[3 * (j + u) + 2], x, y, z);
                ci[u] = base + j + u;
                me[u] = j + u == self;
            }
            b.offer4(d, ci, me);
        }
        for (; j < cnt; j++) b.offer(knn_d2(s_p[3 * j], s_p[3 * j + 1], s_p[3 * j + 2], x, y, z), base + j, j == self);
    }
    if (live) b.store(K, (size_t)i, out_d2, out_idx);
}

// pruned form.  A wave first takes its own stretch of the curve (its 64 queries and K positions either side: at least K other
// points whenever P > K, so every lane starts with a finite K-th distance), then the boxes, leaving that stretch out.
template <int CAP>
__global__ __launch_bounds__(256) void k_knn_search_k(int P, int K, int nbox, const float4 *__restrict__ spts, const float *__restrict__ boxes,
                                                      float *__restrict__ out_d2, int32_t *__restrict__ out_idx) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    const bool live = i < P;
    const float4 p = spts[live ? i : P - 1];
    KBest<CAP> b;
    b.init(live ? K : 0);
    const int w0 = __builtin_amdgcn_readfirstlane(i & ~63);
    const int wlo = max(0, w0 - K), whi = min(P, w0 + 64 + K);   // [wlo, whi)
    b = knn_scan_sorted(b, spts, wlo, whi, p.x, p.y, p.z, ExclSelf{i});
    b = knn_scan_boxes(b, spts, boxes, nbox, P, p.x, p.y, p.z, wlo, whi, ExclSelf{i});
    if (live) b.store(K, (size_t)__float_as_uint(p.w), out_d2, out_idx);
}

// ---- farthest-point sampling: S selections are a serial chain, so one workgroup stays resident for all of them.  Each round
// lowers every point's distance to the selected set by the newest selection, reduces (value, index) to the workgroup's argmax --
// equal values go to the smaller index, numpy's argmax rule -- and every lane reads the winner's coordinates back as one
// wave-uniform load.  REG: N <= 1024 * FPS_REG points and their distances stay in registers; otherwise they stream from memory
// (12 N + 4 N bytes a round, L2-resident at the sizes this is for).  One barrier a round: the LDS exchange is double-buffered.
constexpr int FPS_THREADS = 1024, FPS_REG = 8, FPS_WAVES = FPS_THREADS / 64;

template <bool REG>
__global__ __launch_bounds__(FPS_THREADS) void k_fps(int N, int S, const float *__restrict__ pts, int start, float *__restrict__ min_d2,
                                                     int32_t *__restrict__ out_idx) {
#pragma clang fp contract(off)
    __shared__ float s_v[2][FPS_WAVES];
    __shared__ int s_i[2][FPS_WAVES];
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    float px[FPS_REG], py[FPS_REG], pz[FPS_REG], md[FPS_REG];
    if (REG) {
#pragma unroll
        for (int m = 0; m < FPS_REG; m++) {
            const int i = t + FPS_THREADS * m;
            const bool in = i < N;
            px[m] = in ? pts[3 * i] : 0.f; py[m] = in ? pts[3 * i + 1] : 0.f; pz[m] = in ? pts[3 * i + 2] : 0.f;
            md[m] = INFINITY;
        }
    } else {
        for (int i = t; i < N; i += FPS_THREADS) min_d2[i] = INFINITY;
    }
    if (t == 0) out_idx[0] = start;
    int cur = start;
    for (int s = 1; s <= S; s++) {     // round S only folds the last selection into min_d2
        const float cx = pts[3 * (size_t)cur], cy = pts[3 * (size_t)cur + 1], cz = pts[3 * (size_t)cur + 2];
        float bv = -1.f;               // below every squared distance: the first point offered is taken
        int bi = KNN_IDX_NONE;
        if (REG) {
#pragma unroll
            for (int m = 0; m < FPS_REG; m++) {
                const int i = t + FPS_THREADS * m;
                const float dx = px[m] - cx, dy = py[m] - cy, dz = pz[m] - cz;
                md[m] = fminf(md[m], dx * dx + dy * dy + dz * dz);
                if (i < N && md[m] > bv) { bv = md[m]; bi = i; }   // ascending i: strict `>` keeps the smallest index
            }
        } else {
            for (int i = t; i < N; i += FPS_THREADS) {
                const float dx = pts[3 * (size_t)i] - cx, dy = pts[3 * (size_t)i + 1] - cy, dz = pts[3 * (size_t)i + 2] - cz;
                const float m = fminf(min_d2[i], dx * dx + dy * dy + dz * dz);
                min_d2[i] = m;
                if (m > bv) { bv = m; bi = i; }
            }
        }
        if (s == S) break;
        for (int o = 32; o > 0; o >>= 1) {
            const float ov = __shfl_xor(bv, o, 64);
            const int oi = __shfl_xor(bi, o, 64);
            if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
        }
        if (lane == 0) { s_v[s & 1][wv] = bv; s_i[s & 1][wv] = bi; }
        __syncthreads();
        bv = s_v[s & 1][lane & (FPS_WAVES - 1)];
        bi = s_i[s & 1][lane & (FPS_WAVES - 1)];
        for (int o = FPS_WAVES / 2; o > 0; o >>= 1) {
            const float ov = __shfl_xor(bv, o, 64);
            const int oi = __shfl_xor(bi, o, 64);
            if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
        }
        cur = __builtin_amdgcn_readfirstlane(bi);
        if (t == 0) out_idx[s] = cur;
    }
    if (REG) {
#pragma unroll
        for (int m = 0; m < FPS_REG; m++) {
            const int i = t + FPS_THREADS * m;
            if (i < N) min_d2[i] = md[m];
        }
    }
}
}  // namespace

extern "C" int csplat_knn(void *stream, int P, int K, const float *xyz, float *out_d2, int32_t *out_idx) {
    CSPLAT_REQUIRE(P >= 0, "csplat_knn: bad P");
    CSPLAT_REQUIRE(K >= 1 && K <= CSPLAT_KNN_MAX_K, "csplat_knn: K outside 1 .. CSPLAT_KNN_MAX_K");
    if (P == 0) return 0;
    CSPLAT_REQUIRE(xyz && out_d2 && out_idx, "csplat_knn: NULL argument");
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps(PROF_KNN, s);
#define LAUNCH(CAP) k_knn_brute<CAP><<<cdiv(P, KNN_THREADS), KNN_THREADS, 0, s>>>(P, K, xyz, out_d2, out_idx)
    KNN_BY_CAPACITY(K, LAUNCH);
#undef LAUNCH
    LAUNCH_CHECK();
    return 0;
}

extern "C" size_t csplat_knn_temp_bytes(int P, int K) { (void)K; return knn_ws(P).total; }

// workspace form: Morton order + box pruning (exact; the same bits and indices as csplat_knn).  temp: csplat_knn_temp_bytes(P, K) bytes.
extern "C" int csplat_knn_ws(void *stream, int P, int K, const float *xyz, float *out_d2, int32_t *out_idx, void *temp) {
    CSPLAT_REQUIRE(P >= 0, "csplat_knn_ws: bad P");
    CSPLAT_REQUIRE(K >= 1 && K <= CSPLAT_KNN_MAX_K, "csplat_knn_ws: K outside 1 .. CSPLAT_KNN_MAX_K");
    if (P == 0) return 0;
    CSPLAT_REQUIRE(xyz && out_d2 && out_idx && temp, "csplat_knn_ws: NULL argument");
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps(PROF_KNN, s);
    const KnnWs w = knn_ws(P);
    char *t = (char *)temp;
    int nparts, nbox;
    if (int rc = knn_order_points(s, P, xyz, t, w, &nparts, &nbox)) return rc;
#define LAUNCH(CAP) k_knn_search_k<CAP><<<cdiv(P, 256), 256, 0, s>>>(P, K, nbox, (const float4 *)(t + w.spts), (const float *)(t + w.boxes), out_d2, out_idx)
    KNN_BY_CAPACITY(K, LAUNCH);
#undef LAUNCH
    LAUNCH_CHECK();
    return 0;
}

extern "C" int csplat_fps(void *stream, int N, int S, const float *xyz, int start, float *min_d2, int32_t *out_idx) {
    CSPLAT_REQUIRE(N >= 0 && S >= 0, "csplat_fps: bad N or S");
    if (S == 0) return 0;
    CSPLAT_REQUIRE(N >= 1, "csplat_fps: S > 0 needs at least one point");
    CSPLAT_REQUIRE(start >= 0 && start < N, "csplat_fps: start outside 0 .. N-1");
    CSPLAT_REQUIRE(xyz && min_d2 && out_idx, "csplat_fps: NULL argument");
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps(PROF_KNN, s);
    if (N <= FPS_THREADS * FPS_REG) k_fps<true><<<1, FPS_THREADS, 0, s>>>(N, S, xyz, start, min_d2, out_idx);
    else k_fps<false><<<1, FPS_THREADS, 0, s>>>(N, S, xyz, start, min_d2, out_idx);
    LAUNCH_CHECK();
    return 0;
}

// ---- two-cloud search (csplat_knn_query / csplat_knn_query_ws) and the one-sided Chamfer distance on top of it (csplat_chamfer_fwd /
// csplat_chamfer_bwd).  The pruned form orders the POINTS as csplat_knn_ws does and sorts the queries by their own codes behind that.
namespace {
// one query per lane; nothing is excluded.  N = 0: the list stays empty and every slot is stored as (+inf, -1) -- `points` is never read.
template <int CAP>
__global__ __launch_bounds__(KNN_THREADS) void k_knn_query_brute(int Q, int N, int K, const float *__restrict__ qry, const float *__restrict__ pts,
                                                                 float *__restrict__ out_d2, int32_t *__restrict__ out_idx) {
    const int i = blockIdx.x * KNN_THREADS + threadIdx.x;
    const bool live = i < Q;
    const float x = live ? qry[3 * (size_t)i] : 0.f, y = live ? qry[3 * (size_t)i + 1] : 0.f, z = live ? qry[3 * (size_t)i + 2] : 0.f;
    KBest<CAP> b;
    b.init(live ? K : 0);
    b = knn_scan_slabs(b, pts, N, x, y, z, ExclNone{});
    if (live) b.store(K, (size_t)i, out_d2, out_idx);
}

// pruned form.  Lane i takes the i-th query of the queries' Morton order (qids), so a wave's queries are neighbours in space.
// The wave seeds its lists from a stretch of the sorted points around the place where its first query's code would be inserted
// (binary search in the sorted codes; K + KNN_QUERY_SEED positions either side: at least min(K, N) points), then scans the
// boxes, leaving that stretch out.  The result is stored at the caller's query index.
// A wave scans the UNION of the boxes its queries need, one candidate after the other, so its time is that union's size whatever
// the number of lanes at work: with few queries a wave takes only `lanes` of them (a power of two, 1 .. 64; the other lanes hold
// lists that accept nothing) -- smaller unions, and enough waves to fill the machine.  knn_query_lanes() chooses it.
constexpr int KNN_QUERY_SEED = 32, KNN_QUERY_MIN_WAVES = 4096;

inline int knn_query_lanes(int Q) {
    int lanes = 64;
    while (lanes > 1 && Q / lanes < KNN_QUERY_MIN_WAVES) lanes >>= 1;
    return lanes;
}

template <int CAP>
__global__ __launch_bounds__(256) void k_knn_query_search(int Q, int N, int K, int nbox, int lanes, const float *__restrict__ qry,
                                                          const uint64_t *__restrict__ qcodes, const uint32_t *__restrict__ qids,
                                                          const uint64_t *__restrict__ pcodes, const float4 *__restrict__ spts,
                                                          const float *__restrict__ boxes, float *__restrict__ out_d2, int32_t *__restrict__ out_idx) {
    const int lane = threadIdx.x & 63;
    const int w0 = __builtin_amdgcn_readfirstlane((blockIdx.x * 4 + (threadIdx.x >> 6)) * lanes);   // the wave's first query
    if (w0 >= Q) return;                         // a wave without a query (no barrier in this kernel)
    const int i = w0 + lane;
    const bool live = lane < lanes && i < Q;
    const size_t qi = qids[live ? i : Q - 1];
    const float px = qry[3 * qi], py = qry[3 * qi + 1], pz = qry[3 * qi + 2];
    KBest<CAP> b;
    b.init(live ? K : 0);
    const uint64_t code0 = qcodes[w0] << KNN_QUERY_CODE_SHIFT;
    int lo = 0, hi = N;                          // first position whose code is not below code0, in [0, N]
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (pcodes[mid] < code0) lo = mid + 1; else hi = mid;
    }
    const int pos = __builtin_amdgcn_readfirstlane(lo);
    const int wlo = max(0, pos - K - KNN_QUERY_SEED), whi = min(N, pos + K + KNN_QUERY_SEED);   // [wlo, whi)
    b = knn_scan_sorted(b, spts, wlo, whi, px, py, pz, ExclNone{});
    b = knn_scan_boxes(b, spts, boxes, nbox, N, px, py, pz, wlo, whi, ExclNone{});
    if (live) b.store(K, qi, out_d2, out_idx);
}

// ---- one direction of the Chamfer distance from a K = 1 result.  w_i = 1 when the cap is off (< 0) or d2[i] <= cap.
constexpr int CHAMFER_THREADS = 1024, CHAMFER_WAVES = CHAMFER_THREADS / 64;

__device__ __forceinline__ float chamfer_weight(float d2, float cap) { return (cap < 0.f || d2 <= cap) ? 1.f : 0.f; }

// loss[0] = (1/Q) sum_i w_i d2[i]: ONE workgroup, a fixed order (lane t takes i = t, t + 1024, ...; lanes, then waves, join in a
// fixed tree), accumulated in fp64 so that the only rounding is the last conversion.
__global__ __launch_bounds__(CHAMFER_THREADS) void k_chamfer_fwd(int Q, const float *__restrict__ d2, float cap, float *__restrict__ loss) {
    __shared__ double s_w[CHAMFER_WAVES];
    double acc = 0.0;
    for (int i = threadIdx.x; i < Q; i += CHAMFER_THREADS) {
        const float d = d2[i];
        acc += chamfer_weight(d, cap) != 0.f ? (double)d : 0.0;
    }
    block_sum<CHAMFER_THREADS>(s_w, acc);
    if (threadIdx.x == 0) loss[0] = (float)(acc / (double)Q);
}

// the term both gradients are made of: t_i = g (2/Q) w_i (q_i - p_idx[i])
// (an index outside 0 .. N-1 is not a result of csplat_knn_query on a non-empty cloud: its term is zero and nothing is read)
__device__ __forceinline__ void chamfer_term(int i, int N, float c, float cap, const float *__restrict__ qry, const float *__restrict__ pts,
                                             const float *__restrict__ d2, const int32_t *__restrict__ idx, float (&t)[3]) {
#pragma clang fp contract(off)
    const int j = idx[i];
    if ((unsigned)j >= (unsigned)N) { t[0] = t[1] = t[2] = 0.f; return; }
    const float cw = c * chamfer_weight(d2[i], cap);
    for (int a = 0; a < 3; a++) t[a] = cw * (qry[3 * (size_t)i + a] - pts[3 * (size_t)j + a]);
}

__global__ __launch_bounds__(256) void k_chamfer_bwd_queries(int Q, int N, const float *__restrict__ qry, const float *__restrict__ pts,
                                                             const float *__restrict__ d2, const int32_t *__restrict__ idx, float cap,
                                                             const float *__restrict__ g, float *__restrict__ dq) {
#pragma clang fp contract(off)
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= Q) return;
    const float c = g[0] * (2.0f / (float)Q);
    float t[3];
    chamfer_term(i, N, c, cap, qry, pts, d2, idx, t);
    for (int a = 0; a < 3; a++) dq[3 * (size_t)i + a] = t[a];
}

__global__ __launch_bounds__(256) void k_chamfer_keys(int Q, const int32_t *__restrict__ idx, uint64_t *__restrict__ keys, uint32_t *__restrict__ vals) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= Q) return;
    keys[i] = (uint64_t)(uint32_t)idx[i];
    vals[i] = (uint32_t)i;
}

// keys / vals: (idx, i) sorted by idx, equal idx in ascending i (the sort is stable).  The lane at the first position of a run
// sums the run's terms in that order and writes the point's row; rows nobody selected keep the zeros they were cleared to.
__global__ __launch_bounds__(256) void k_chamfer_bwd_points(int Q, int N, const uint64_t *__restrict__ keys, const uint32_t *__restrict__ vals,
                                                            const float *__restrict__ qry, const float *__restrict__ pts, const float *__restrict__ d2,
                                                            const int32_t *__restrict__ idx, float cap, const float *__restrict__ g,
                                                            float *__restrict__ dp) {
#pragma clang fp contract(off)
    const int s = blockIdx.x * 256 + threadIdx.x;
    if (s >= Q) return;
    const uint64_t j = keys[s];
    if (s > 0 && keys[s - 1] == j) return;       // not a run start
    if (j >= (uint64_t)N) return;                // (an index outside the cloud: not a result of csplat_knn_query; nothing is written)
    const float c = g[0] * (2.0f / (float)Q);
    float acc[3] = {0.f, 0.f, 0.f};
    for (int r = s; r < Q && keys[r] == j; r++) {
        float t[3];
        chamfer_term((int)vals[r], N, c, cap, qry, pts, d2, idx, t);
        for (int a = 0; a < 3; a++) acc[a] = acc[a] + t[a];
    }
    for (int a = 0; a < 3; a++) dp[3 * (size_t)j + a] = -acc[a];
}
}  // namespace

extern "C" int csplat_knn_query(void *stream, int Q, int N, int K, const float *queries, const float *points, float *out_d2,
                                int32_t *out_idx) {
    CSPLAT_REQUIRE(Q >= 0 && N >= 0, "csplat_knn_query: bad Q or N");
    CSPLAT_REQUIRE(K >= 1 && K <= CSPLAT_KNN_MAX_K, "csplat_knn_query: K outside 1 .. CSPLAT_KNN_MAX_K");
    if (Q == 0) return 0;
    CSPLAT_REQUIRE(queries && out_d2 && out_idx && (points || N == 0), "csplat_knn_query: NULL argument");
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps(PROF_KNN, s);
#define LAUNCH(CAP) k_knn_query_brute<CAP><<<cdiv(Q, KNN_THREADS), KNN_THREADS, 0, s>>>(Q, N, K, queries, points, out_d2, out_idx)
    KNN_BY_CAPACITY(K, LAUNCH);
#undef LAUNCH
    LAUNCH_CHECK();
    return 0;
}

extern "C" size_t csplat_knn_query_temp_bytes(int Q, int N, int K) { (void)K; return knn_query_ws(Q, N).total; }

extern "C" int csplat_knn_query_ws(void *stream, int Q, int N, int K, const float *queries, const float *points, float *out_d2,
                                   int32_t *out_idx, void *temp) {
    CSPLAT_REQUIRE(Q >= 0 && N >= 0, "csplat_knn_query_ws: bad Q or N");
    CSPLAT_REQUIRE(K >= 1 && K <= CSPLAT_KNN_MAX_K, "csplat_knn_query_ws: K outside 1 .. CSPLAT_KNN_MAX_K");
    if (Q == 0) return 0;
    CSPLAT_REQUIRE(queries && out_d2 && out_idx && (points || N == 0) && (temp || N == 0), "csplat_knn_query_ws: NULL argument");
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps(PROF_KNN, s);
    if (N == 0) {                                // nothing to order: the brute-force kernel stores the empty lists
#define LAUNCH(CAP) k_knn_query_brute<CAP><<<cdiv(Q, KNN_THREADS), KNN_THREADS, 0, s>>>(Q, N, K, queries, points, out_d2, out_idx)
        KNN_BY_CAPACITY(K, LAUNCH);
#undef LAUNCH
        LAUNCH_CHECK();
        return 0;
    }
    const KnnQueryWs wq = knn_query_ws(Q, N);
    const KnnWs &w = wq.pts;
    char *t = (char *)temp;
    int nparts, nbox;
    if (int rc = knn_order_points(s, N, points, t, w, &nparts, &nbox)) return rc;
    k_morton<KNN_QUERY_CODE_SHIFT><<<cdiv(Q, 256), 256, 0, s>>>(Q, nparts, queries, (const float *)(t + w.part), wq.qsort.k(t), wq.qsort.v(t));
    LAUNCH_CHECK();
    if (int rc = wq.qsort.sort(s, t, Q, KNN_QUERY_CODE_BITS)) return rc;
    const int lanes = knn_query_lanes(Q);
#define LAUNCH(CAP)                                                                                                                          \
    k_knn_query_search<CAP><<<cdiv(cdiv(Q, lanes), 4), 256, 0, s>>>(Q, N, K, nbox, lanes, queries, wq.qsort.k_sorted(t), wq.qsort.v_sorted(t), \
                                                                    w.sort.k_sorted(t), (const float4 *)(t + w.spts), (const float *)(t + w.boxes), out_d2, out_idx)
    KNN_BY_CAPACITY(K, LAUNCH);
#undef LAUNCH
    LAUNCH_CHECK();
    return 0;
}

extern "C" int csplat_chamfer_fwd(void *stream, int Q, const float *d2, float max_sq_dist, float *loss) {
    CSPLAT_REQUIRE(Q >= 1, "csplat_chamfer_fwd: Q must be >= 1 (the loss divides by it)");
    CSPLAT_REQUIRE(d2 && loss, "csplat_chamfer_fwd: NULL argument");
    CSPLAT_REQUIRE(!(max_sq_dist != max_sq_dist), "csplat_chamfer_fwd: max_sq_dist is NaN");
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps(PROF_KNN, s);
    k_chamfer_fwd<<<1, CHAMFER_THREADS, 0, s>>>(Q, d2, max_sq_dist, loss);
    LAUNCH_CHECK();
    return 0;
}

extern "C" size_t csplat_chamfer_bwd_temp_bytes(int Q, int N) { (void)N; return chamfer_ws(Q).total; }

extern "C" int csplat_chamfer_bwd(void *stream, int Q, int N, const float *queries, const float *points, const float *d2,
                                  const int32_t *idx, float max_sq_dist, const float *g, float *dL_dqueries, float *dL_dpoints,
                                  void *temp) {
    CSPLAT_REQUIRE(Q >= 1 && N >= 1, "csplat_chamfer_bwd: Q and N must be >= 1");
    CSPLAT_REQUIRE(queries && points && d2 && idx && g, "csplat_chamfer_bwd: NULL argument");
    CSPLAT_REQUIRE(!dL_dpoints || temp, "csplat_chamfer_bwd: dL_dpoints needs temp");
    CSPLAT_REQUIRE(!(max_sq_dist != max_sq_dist), "csplat_chamfer_bwd: max_sq_dist is NaN");
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps(PROF_KNN, s);
    if (dL_dqueries) {
        k_chamfer_bwd_queries<<<cdiv(Q, 256), 256, 0, s>>>(Q, N, queries, points, d2, idx, max_sq_dist, g, dL_dqueries);
        LAUNCH_CHECK();
    }
    if (dL_dpoints) {
        const ChamferWs w = chamfer_ws(Q);
        char *t = (char *)temp;
        int bits = 1;
        while (bits < 32 && ((uint64_t)1 << bits) < (uint64_t)N) bits++;
        HIP_TRY(hipMemsetAsync(dL_dpoints, 0, (size_t)N * 3 * sizeof(float), s));
        k_chamfer_keys<<<cdiv(Q, 256), 256, 0, s>>>(Q, idx, w.sort.k(t), w.sort.v(t));
        LAUNCH_CHECK();
        if (int rc = w.sort.sort(s, t, Q, bits)) return rc;
        k_chamfer_bwd_points<<<cdiv(Q, 256), 256, 0, s>>>(Q, N, w.sort.k_sorted(t), w.sort.v_sorted(t), queries, points, d2, idx, max_sq_dist, g, dL_dpoints);
        LAUNCH_CHECK();
    }
    return 0;
}

// ---- trajectory smoothing (csplat_traj_smooth; include/csplat.h "Trajectory preprocessing" states the semantics): the reference's
// gaussian_smoothing (meshnet/data_utils.py:267-278, one KD-tree query per point per frame in Python) for all T frames of a tracked
// cloud in ONE launch.  This is k_knn_query_brute with the frame on the grid's second axis (queries and points are the same frame; a
// wave never reads another frame) and an epilogue that forms the weighted mean straight from the K-best registers -- K gathers from
// the frame, which the slab scan has just pulled through the cache -- so no index array leaves the kernel unless the caller asks for
// it.  A candidate whose squared distance is not finite is left out (ExclNonFinite): it changes nothing.  The sum runs over the list
// in its ascending (d2, index) order, one float32 rounding per operation: bit-reproducible, no atomics.  Brute force only, O(T N^2):
// tracked clouds are hundreds to a few thousand points (profiles/trajectory_cost.txt shows where that stops being the right tool).
namespace {
template <int CAP>
__global__ __launch_bounds__(KNN_THREADS) void k_traj_smooth(int T, int N, int K, const float *__restrict__ pts, float neg_scale,
                                                             float *__restrict__ out, float *__restrict__ out_d2, int32_t *__restrict__ out_idx) {
#pragma clang fp contract(off)                                   // (the weighted mean below; knn_d2 has its own)
    const int i = blockIdx.x * KNN_THREADS + threadIdx.x;
    const bool live = i < N;
    for (int t = blockIdx.y; t < T; t += gridDim.y) {            // uniform per workgroup: the scan's barriers stay together
        const float *__restrict__ frame = pts + (size_t)t * N * 3;
        const float x = live ? frame[3 * (size_t)i] : 0.f, y = live ? frame[3 * (size_t)i + 1] : 0.f, z = live ? frame[3 * (size_t)i + 2] : 0.f;
        KBest<CAP> b;
        b.init(live ? K : 0);
        b = knn_scan_slabs(b, frame, N, x, y, z, ExclNonFinite{});
        if (live) {
            const size_t row = (size_t)t * N + i;
            float ax = -0.f, ay = -0.f, az = -0.f, sw = 0.f;      // -0 is the identity of +: the sum is that of its terms alone (K = 1 returns a -0 as -0)
#pragma unroll
            for (int s = 0; s < CAP; s++) {
                const int r = s - (CAP - K);
                if (r < 0) continue;
                const bool filled = b.id[s] != KNN_IDX_NONE;
                if (out_d2) out_d2[row * K + r] = b.d[s];                 // an empty slot still holds +inf
                if (out_idx) out_idx[row * K + r] = filled ? b.id[s] : -1;
                if (filled) {
                    const float w = expf(b.d[s] * neg_scale);
                    const float *__restrict__ q = frame + 3 * (size_t)b.id[s];
                    ax = ax + w * q[0]; ay = ay + w * q[1]; az = az + w * q[2];
                    sw = sw + w;
                }
            }
            // a non-finite coordinate: every distance was a NaN or Inf, the list is empty and the point goes through as it is
            const bool whole = finite_f32(x) && finite_f32(y) && finite_f32(z);
            out[3 * row] = whole ? ax / sw : x;
            out[3 * row + 1] = whole ? ay / sw : y;
            out[3 * row + 2] = whole ? az / sw : z;
        }
    }
}

bool traj_overlap(const void *a, size_t na, const void *b, size_t nb) {
    if (!a || !b || na == 0 || nb == 0) return false;
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + nb && y < x + na;
}
}  // namespace

extern "C" int csplat_traj_smooth(void *stream, int T, int N, int K, const float *points, float sigma, float *out, float *out_d2,
                                  int32_t *out_idx) {
    CSPLAT_REQUIRE(T >= 0 && N >= 0, "csplat_traj_smooth: bad T or N");
    CSPLAT_REQUIRE(K >= 1 && K <= CSPLAT_KNN_MAX_K, "csplat_traj_smooth: K outside 1 .. CSPLAT_KNN_MAX_K");
    CSPLAT_REQUIRE(sigma > 0.f && sigma < __builtin_inff(), "csplat_traj_smooth: sigma is a finite number > 0");
    CSPLAT_REQUIRE((int64_t)T * N * K < ((int64_t)1 << 31), "csplat_traj_smooth: T * N * K must stay below 2^31");
    if (T == 0 || N == 0) return 0;
    CSPLAT_REQUIRE(points && out, "csplat_traj_smooth: NULL points or out");
    CSPLAT_REQUIRE((((uintptr_t)points | (uintptr_t)out | (uintptr_t)out_d2 | (uintptr_t)out_idx) & 3u) == 0,
                   "csplat_traj_smooth: operands must be 4-byte aligned");
    const size_t rows = (size_t)T * N, nb = rows * 3 * 4, kb = rows * K * 4;
    CSPLAT_REQUIRE(!traj_overlap(out, nb, points, nb) && !traj_overlap(out_d2, kb, points, nb) && !traj_overlap(out_idx, kb, points, nb) &&
                       !traj_overlap(out, nb, out_d2, kb) && !traj_overlap(out, nb, out_idx, kb) && !traj_overlap(out_d2, kb, out_idx, kb),
                   "csplat_traj_smooth: an output overlaps another operand");
    // the weight's scale: 1 / (2 sigma^2) in double from the float32 sigma, rounded once to float32, at most FLT_MAX (0 * scale stays 0)
    const double inv = 1.0 / (2.0 * (double)sigma * (double)sigma);
    const float neg_scale = -(inv < (double)__FLT_MAX__ ? (float)inv : __FLT_MAX__);
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps(PROF_KNN, s);
    const dim3 grid(cdiv(N, KNN_THREADS), T < 65535 ? T : 65535);
#define LAUNCH(CAP) k_traj_smooth<CAP><<<grid, KNN_THREADS, 0, s>>>(T, N, K, points, neg_scale, out, out_d2, out_idx)
    KNN_BY_CAPACITY(K, LAUNCH);
#undef LAUNCH
    LAUNCH_CHECK();
    return 0;
}
