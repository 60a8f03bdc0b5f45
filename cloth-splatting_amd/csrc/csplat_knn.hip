// csplat_knn.hip -- simple_knn._C.distCUDA2 for gfx950: exact 3-nearest-neighbour mean squared distance.
//
// Replaces the CUDA extension called at /root/reference/scene_reconstruction/gaussian_mesh.py:250 and
// gaussian_model.py:134.  A single k-select kernel: one query point per lane, candidate
// points streamed through LDS in 1024-point slabs (every lane reads the same LDS word -> broadcast, no bank
// conflicts), the three best squared distances kept in registers.  Self is excluded by index, so coincident
// points contribute 0 exactly as upstream.  The distance is evaluated as dx*dx + dy*dy + dz*dz with FP
// contraction off, the association order of oracle/knn_ref.c: the result is bit-identical to the oracle.
#include "csplat_common.h"

namespace {
constexpr int KNN_THREADS = 256;
constexpr int KNN_SLAB = 1024;

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
            const float dx = s_p[3 * j] - x, dy = s_p[3 * j + 1] - y, dz = s_p[3 * j + 2] - z;
            float d = dx * dx + dy * dy + dz * dz;
            d = (j == self) ? INFINITY : d;
            // insert into the sorted triple (b0 <= b1 <= b2)
            const float n2 = fminf(b2, fmaxf(b1, d));
            const float n1 = fminf(b1, fmaxf(b0, d));
            const float n0 = fminf(b0, d);
            b0 = n0; b1 = n1; b2 = n2;
        }
    }
    if (live) out[i] = (b0 + b1 + b2) / 3.0f;
}

// ---- accelerated exact form for large P (the brute-force kernel above is O(P^2): 4.9 ms at P = 1e5, 0.5 s at 1e6).
// Same pruning as the upstream extension: points are ordered along a Morton curve, every run of KNN_BOX consecutive points
// gets its bounding box, a query first bounds its 3rd-nearest distance with its +-3 curve neighbours and then scans only the
// boxes whose distance to the query does not exceed the current 3rd best.  The result is the same multiset of three smallest
// squared distances, summed in ascending order as before: bit-identical to the brute-force kernel (tested).
constexpr int KNN_BOX = 1024;

__global__ __launch_bounds__(256) void k_bbox_partial(int P, const float *__restrict__ pts, float *__restrict__ part) {
    float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int i = blockIdx.x * 256 + threadIdx.x; i < P; i += gridDim.x * 256)
        for (int a = 0; a < 3; a++) { const float v = pts[3 * i + a]; mn[a] = fminf(mn[a], v); mx[a] = fmaxf(mx[a], v); }
    __shared__ float s[6][4];
    for (int a = 0; a < 3; a++) {
        float lo = mn[a], hi = mx[a];
        for (int o = 32; o > 0; o >>= 1) { lo = fminf(lo, __shfl_xor(lo, o, 64)); hi = fmaxf(hi, __shfl_xor(hi, o, 64)); }
        if ((threadIdx.x & 63) == 0) { s[a][threadIdx.x >> 6] = lo; s[3 + a][threadIdx.x >> 6] = hi; }
    }
    __syncthreads();
    if (threadIdx.x < 6) {
        const float *r = s[threadIdx.x];
        part[blockIdx.x * 6 + threadIdx.x] = threadIdx.x < 3 ? fminf(fminf(r[0], r[1]), fminf(r[2], r[3]))
                                                             : fmaxf(fmaxf(r[0], r[1]), fmaxf(r[2], r[3]));
    }
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
        const float t = ext > 0.f ? (pts[3 * i + a] - s_box[a]) / ext : 0.f;
        q[a] = (uint32_t)fminf(fmaxf(t * 2097151.f, 0.f), 2097151.f);
    }
    codes[i] = spread21(q[0]) | spread21(q[1]) << 1 | spread21(q[2]) << 2;
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
    __shared__ float s[6][4];
    for (int a = 0; a < 3; a++) {
        float lo = mn[a], hi = mx[a];
        for (int o = 32; o > 0; o >>= 1) { lo = fminf(lo, __shfl_xor(lo, o, 64)); hi = fmaxf(hi, __shfl_xor(hi, o, 64)); }
        if ((threadIdx.x & 63) == 0) { s[a][threadIdx.x >> 6] = lo; s[3 + a][threadIdx.x >> 6] = hi; }
    }
    __syncthreads();
    if (threadIdx.x < 6) {
        const float *r = s[threadIdx.x];
        boxes[blockIdx.x * 6 + threadIdx.x] = threadIdx.x < 3 ? fminf(fminf(r[0], r[1]), fminf(r[2], r[3]))
                                                              : fmaxf(fmaxf(r[0], r[1]), fmaxf(r[2], r[3]));
    }
}

__device__ __forceinline__ void best3_insert(float d, float &b0, float &b1, float &b2) {
    const float n2 = fminf(b2, fmaxf(b1, d));
    const float n1 = fminf(b1, fmaxf(b0, d));
    const float n0 = fminf(b0, d);
    b0 = n0; b1 = n1; b2 = n2;
}

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
            const float dx = c.x - p.x, dy = c.y - p.y, dz = c.z - p.z;
            best3_insert(dx * dx + dy * dy + dz * dz, b0, b1, b2);
        }
    }
    const float reject = b2;
    b0 = b1 = b2 = INFINITY;
    for (int b = 0; b < nbox; b++) {
        const float *bx = boxes + 6 * b;
        float ex = 0.f, ey = 0.f, ez = 0.f;     // distance from the query to the box, per axis
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
            const float dx = c.x - p.x, dy = c.y - p.y, dz = c.z - p.z;
            float d = dx * dx + dy * dy + dz * dz;
            d = (j == i) ? INFINITY : d;
            best3_insert(d, b0, b1, b2);
        }
    }
    if (live) out[__float_as_uint(p.w)] = (b0 + b1 + b2) / 3.0f;
}
}  // namespace

extern "C" int csplat_dist2(void *stream, int P, const float *xyz, float *out) {
    CSPLAT_REQUIRE(P >= 0, "csplat_dist2: bad P");
    if (P == 0) return 0;
    ProfScope ps(PROF_KNN, (hipStream_t)stream);
    k_dist2<<<cdiv(P, KNN_THREADS), KNN_THREADS, 0, (hipStream_t)stream>>>(P, xyz, out);
    LAUNCH_CHECK();
    return 0;
}

// workspace form: Morton order + box pruning (exact; same bits as csplat_dist2).  temp: csplat_dist2_temp_bytes(P) bytes.
namespace {
struct KnnWs { size_t part, codes, ids, codes_o, ids_o, codes_t, ids_t, stab, spts, boxes, total; };
KnnWs knn_ws(int P) {
    KnnWs w;
    size_t o = 0;
    auto take = [&](size_t b) { const size_t at = o; o += align256(b); return at; };
    const size_t n = (size_t)(P > 0 ? P : 1);
    w.part = take(256 * 6 * 4);
    w.codes = take(n * 8); w.ids = take(n * 4); w.codes_o = take(n * 8); w.ids_o = take(n * 4);
    w.codes_t = take(n * 8); w.ids_t = take(n * 4); w.stab = take(csplat_sort_temp_bytes((int64_t)n));
    w.spts = take(n * 16); w.boxes = take((size_t)cdiv((int)n, KNN_BOX) * 6 * 4);
    w.total = o;
    return w;
}
}  // namespace

extern "C" size_t csplat_dist2_temp_bytes(int P) { return knn_ws(P).total; }

extern "C" int csplat_dist2_ws(void *stream, int P, const float *xyz, float *out, void *temp) {
    CSPLAT_REQUIRE(P >= 0, "csplat_dist2_ws: bad P");
    if (P == 0) return 0;
    CSPLAT_REQUIRE(xyz && out && temp, "csplat_dist2_ws: NULL argument");
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps(PROF_KNN, s);
    const KnnWs w = knn_ws(P);
    char *t = (char *)temp;
    float *part = (float *)(t + w.part);
    uint64_t *codes = (uint64_t *)(t + w.codes), *codes_o = (uint64_t *)(t + w.codes_o), *codes_t = (uint64_t *)(t + w.codes_t);
    uint32_t *ids = (uint32_t *)(t + w.ids), *ids_o = (uint32_t *)(t + w.ids_o), *ids_t = (uint32_t *)(t + w.ids_t);
    float4 *spts = (float4 *)(t + w.spts);
    float *boxes = (float *)(t + w.boxes);
    const int nparts = P < 256 * 256 ? cdiv(P, 256) : 256, nbox = cdiv(P, KNN_BOX);
    k_bbox_partial<<<nparts, 256, 0, s>>>(P, xyz, part);
    LAUNCH_CHECK();
    k_morton<<<cdiv(P, 256), 256, 0, s>>>(P, nparts, xyz, part, codes, ids);
    LAUNCH_CHECK();
    if (int rc = csplat_sort_pairs(s, codes, ids, codes_o, ids_o, codes_t, ids_t, P, 63, t + w.stab)) return rc;
    k_knn_boxes<<<nbox, 256, 0, s>>>(P, xyz, ids_o, spts, boxes);
    LAUNCH_CHECK();
    k_knn_search<<<cdiv(P, 256), 256, 0, s>>>(P, nbox, spts, boxes, out);
    LAUNCH_CHECK();
    return 0;
}

// ================================================================================================================================
// Exact k-NN with indices (csplat_knn / csplat_knn_ws) and farthest-point sampling (csplat_fps).  Nothing above is touched: the
// pruned form reuses k_bbox_partial / k_morton / the radix sort / k_knn_boxes and the workspace layout of csplat_dist2_ws.
//
// The K best (d2, index) pairs of a query live in registers: KBest<CAP> with CAP in {4, 8, 16, 32}, every access through a fully
// unrolled loop (a runtime-indexed private array would go to scratch memory).  Slots [0, CAP-K) hold the pair (-inf, -1), which no
// candidate can precede, so the K real entries sit in slots [CAP-K, CAP) and slot CAP-1 is always the K-th best -- the skip test
// and the box rejection use the exact bound for every K, not the bound of the rounded-up capacity.  Pairs are ordered by
// (d2, index): the result does not depend on the order in which candidates arrive, which is what lets the Morton-ordered form
// return the same bits and indices as the brute-force one.
namespace {
constexpr int KNN_IDX_NONE = 0x7fffffff;   // index of an empty slot and of the query itself: never precedes anything

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

// one candidate against one query per lane.  The wave tests the candidate against every lane's K-th best first and skips the
// insert together; `<=` (not the full pair order) keeps the test at one compare -- an equal distance enters the insert, which
// then decides by index.
template <int CAP>
__device__ __forceinline__ void knn_offer(KBest<CAP> &b, float d, int ci, bool self) {
    d = self ? INFINITY : d;
    ci = self ? KNN_IDX_NONE : ci;
    if (__builtin_amdgcn_ballot_w64(d <= b.worst()) != 0ull) b.insert(d, ci);
}

// four candidates at once: one wave-wide test and one branch for the four (after the first few hundred candidates almost every
// group is skipped whole), then the single-candidate path for a group in which some lane still needs one
template <int CAP>
__device__ __forceinline__ void knn_offer4(KBest<CAP> &b, const float (&d)[4], const int (&ci)[4], const bool (&self)[4]) {
    const float w = b.worst();
    const bool any = (!self[0] && d[0] <= w) || (!self[1] && d[1] <= w) || (!self[2] && d[2] <= w) || (!self[3] && d[3] <= w);
    if (__builtin_amdgcn_ballot_w64(any) == 0ull) return;
#pragma unroll
    for (int u = 0; u < 4; u++) knn_offer(b, d[u], ci[u], self[u]);
}

template <int CAP>
__global__ __launch_bounds__(KNN_THREADS) void k_knn_brute(int P, int K, const float *__restrict__ pts, float *__restrict__ out_d2,
                                                           int32_t *__restrict__ out_idx) {
#pragma clang fp contract(off)
    __shared__ float s_p[KNN_SLAB * 3];
    const int i = blockIdx.x * KNN_THREADS + threadIdx.x;
    const bool live = i < P;
    const float x = live ? pts[3 * (size_t)i] : 0.f, y = live ? pts[3 * (size_t)i + 1] : 0.f, z = live ? pts[3 * (size_t)i + 2] : 0.f;
    KBest<CAP> b;
    b.init(live ? K : 0);
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
                const float dx = s_p[3 * (j + u)] - x, dy = s_p[3 * (j + u) + 1] - y, dz = s_p[3 * (j + u) + 2] - z;
                d[u] = dx * dx + dy * dy + dz * dz;
                ci[u] = base + j + u;
                me[u] = j + u == self;
            }
            knn_offer4(b, d, ci, me);
        }
        for (; j < cnt; j++) {
            const float dx = s_p[3 * j] - x, dy = s_p[3 * j + 1] - y, dz = s_p[3 * j + 2] - z;
            knn_offer(b, dx * dx + dy * dy + dz * dz, base + j, j == self);
        }
    }
    if (live) b.store(K, (size_t)i, out_d2, out_idx);
}

// pruned form.  spts: the points in Morton order, .w = the caller's index.  A wave first takes its own stretch of the curve
// (its 64 queries and K positions either side: at least K other points whenever P > K, so every lane starts with a finite
// K-th distance), then scans the boxes that are not farther than a lane's current K-th best, leaving that stretch out.
// Rejection is strict (`>`): a box at exactly the K-th distance may hold an equal distance with a smaller index.
template <int CAP>
__global__ __launch_bounds__(256) void k_knn_search_k(int P, int K, int nbox, const float4 *__restrict__ spts, const float *__restrict__ boxes,
                                                      float *__restrict__ out_d2, int32_t *__restrict__ out_idx) {
#pragma clang fp contract(off)
    const int i = blockIdx.x * 256 + threadIdx.x;
    const bool live = i < P;
    const float4 p = spts[live ? i : P - 1];
    KBest<CAP> b;
    b.init(live ? K : 0);
    auto scan = [&](int lo, int hi) {
        int j = lo;                              // wave-uniform addresses: one broadcast load per candidate
        for (; j + 4 <= hi; j += 4) {
            float d[4];
            int ci[4];
            bool me[4];
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const float4 c = spts[j + u];
                const float dx = c.x - p.x, dy = c.y - p.y, dz = c.z - p.z;
                d[u] = dx * dx + dy * dy + dz * dz;
                ci[u] = (int)__float_as_uint(c.w);
                me[u] = j + u == i;
            }
            knn_offer4(b, d, ci, me);
        }
        for (; j < hi; j++) {
            const float4 c = spts[j];
            const float dx = c.x - p.x, dy = c.y - p.y, dz = c.z - p.z;
            knn_offer(b, dx * dx + dy * dy + dz * dz, (int)__float_as_uint(c.w), j == i);
        }
    };
    const int w0 = __builtin_amdgcn_readfirstlane(i & ~63);
    const int wlo = max(0, w0 - K), whi = min(P, w0 + 64 + K);   // [wlo, whi)
    scan(wlo, whi);
    for (int bi = 0; bi < nbox; bi++) {
        const float *bx = boxes + 6 * bi;
        float ex = 0.f, ey = 0.f, ez = 0.f;     // distance from the query to the box, per axis
        if (p.x < bx[0] || p.x > bx[3]) ex = fminf(fabsf(p.x - bx[0]), fabsf(p.x - bx[3]));
        if (p.y < bx[1] || p.y > bx[4]) ey = fminf(fabsf(p.y - bx[1]), fabsf(p.y - bx[4]));
        if (p.z < bx[2] || p.z > bx[5]) ez = fminf(fabsf(p.z - bx[2]), fabsf(p.z - bx[5]));
        const float dist = ex * ex + ey * ey + ez * ez;
        const bool need = !(dist > b.worst());   // lanes without a query hold -inf and never need a box
        if (__builtin_amdgcn_ballot_w64(need) == 0ull) continue;
        const int lo = bi * KNN_BOX, hi = min(P, lo + KNN_BOX);
        scan(lo, min(hi, wlo));
        scan(max(lo, whi), hi);
    }
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

#define KNN_BY_CAPACITY(K, LAUNCH)                                  \
    do {                                                            \
        if ((K) <= 4) { LAUNCH(4); } else if ((K) <= 8) { LAUNCH(8); } else if ((K) <= 16) { LAUNCH(16); } else { LAUNCH(32); } \
    } while (0)

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
    float *part = (float *)(t + w.part);
    uint64_t *codes = (uint64_t *)(t + w.codes), *codes_o = (uint64_t *)(t + w.codes_o), *codes_t = (uint64_t *)(t + w.codes_t);
    uint32_t *ids = (uint32_t *)(t + w.ids), *ids_o = (uint32_t *)(t + w.ids_o), *ids_t = (uint32_t *)(t + w.ids_t);
    float4 *spts = (float4 *)(t + w.spts);
    float *boxes = (float *)(t + w.boxes);
    const int nparts = P < 256 * 256 ? cdiv(P, 256) : 256, nbox = cdiv(P, KNN_BOX);
    k_bbox_partial<<<nparts, 256, 0, s>>>(P, xyz, part);
    LAUNCH_CHECK();
    k_morton<<<cdiv(P, 256), 256, 0, s>>>(P, nparts, xyz, part, codes, ids);
    LAUNCH_CHECK();
    if (int rc = csplat_sort_pairs(s, codes, ids, codes_o, ids_o, codes_t, ids_t, P, 63, t + w.stab)) return rc;
    k_knn_boxes<<<nbox, 256, 0, s>>>(P, xyz, ids_o, spts, boxes);
    LAUNCH_CHECK();
#define LAUNCH(CAP) k_knn_search_k<CAP><<<cdiv(P, 256), 256, 0, s>>>(P, K, nbox, spts, boxes, out_d2, out_idx)
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

// ================================================================================================================================
// Two-cloud search (csplat_knn_query / csplat_knn_query_ws) and the one-sided Chamfer distance on top of it (csplat_chamfer_fwd /
// csplat_chamfer_bwd).  Nothing above is touched: KBest, knn_offer / knn_offer4 and the CAP dispatch are used as they are, the
// pruned form orders the POINTS with k_bbox_partial / k_morton / the radix sort / k_knn_boxes in the workspace layout of
// csplat_dist2_ws and appends its own query-side arrays behind it.
namespace {
// one query per lane, slabs of `points` through LDS as in k_knn_brute; nothing is excluded.  N = 0: the list stays empty and
// every slot is stored as (+inf, -1) -- `points` is never read.
template <int CAP>
__global__ __launch_bounds__(KNN_THREADS) void k_knn_query_brute(int Q, int N, int K, const float *__restrict__ qry, const float *__restrict__ pts,
                                                                 float *__restrict__ out_d2, int32_t *__restrict__ out_idx) {
#pragma clang fp contract(off)
    __shared__ float s_p[KNN_SLAB * 3];
    const int i = blockIdx.x * KNN_THREADS + threadIdx.x;
    const bool live = i < Q;
    const float x = live ? qry[3 * (size_t)i] : 0.f, y = live ? qry[3 * (size_t)i + 1] : 0.f, z = live ? qry[3 * (size_t)i + 2] : 0.f;
    KBest<CAP> b;
    b.init(live ? K : 0);
    for (int base = 0; base < N; base += KNN_SLAB) {
        const int cnt = min(KNN_SLAB, N - base);
        __syncthreads();
        for (int k = threadIdx.x; k < cnt * 3; k += KNN_THREADS) s_p[k] = pts[(size_t)base * 3 + k];
        __syncthreads();
        int j = 0;
        for (; j + 4 <= cnt; j += 4) {
            float d[4];
            int ci[4];
            const bool me[4] = {false, false, false, false};
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const float dx = s_p[3 * (j + u)] - x, dy = s_p[3 * (j + u) + 1] - y, dz = s_p[3 * (j + u) + 2] - z;
                d[u] = dx * dx + dy * dy + dz * dz;
                ci[u] = base + j + u;
            }
            knn_offer4(b, d, ci, me);
        }
        for (; j < cnt; j++) {
            const float dx = s_p[3 * j] - x, dy = s_p[3 * j + 1] - y, dz = s_p[3 * j + 2] - z;
            knn_offer(b, dx * dx + dy * dy + dz * dz, base + j, false);
        }
    }
    if (live) b.store(K, (size_t)i, out_d2, out_idx);
}

// the queries are ordered by the upper 31 bits of their 63-bit code (10 levels of the octree and one bit more): four passes of the
// radix sort instead of eight, and no coarser a grouping than that for any cloud of fewer than 2^30 queries
constexpr int KNN_QUERY_CODE_SHIFT = 32, KNN_QUERY_CODE_BITS = 63 - KNN_QUERY_CODE_SHIFT;

// Morton codes of the queries in the POINTS' bounding box (part: the partials of k_bbox_partial over the points); a query outside
// the box clamps to its faces.  The codes only group nearby queries in one wave -- the search is exact for any order.
__global__ __launch_bounds__(256) void k_morton_query(int Q, int nparts, const float *__restrict__ qry, const float *__restrict__ part,
                                                      uint64_t *__restrict__ codes, uint32_t *__restrict__ ids) {
    __shared__ float s_box[6];
    if (threadIdx.x < 6) {
        float v = part[threadIdx.x];
        for (int b = 1; b < nparts; b++) v = threadIdx.x < 3 ? fminf(v, part[b * 6 + threadIdx.x]) : fmaxf(v, part[b * 6 + threadIdx.x]);
        s_box[threadIdx.x] = v;
    }
    __syncthreads();
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= Q) return;
    uint32_t q[3];
    for (int a = 0; a < 3; a++) {
        const float ext = s_box[3 + a] - s_box[a];
        const float t = ext > 0.f ? (qry[3 * (size_t)i + a] - s_box[a]) / ext : 0.f;
        q[a] = (uint32_t)fminf(fmaxf(t * 2097151.f, 0.f), 2097151.f);
    }
    codes[i] = (spread21(q[0]) | spread21(q[1]) << 1 | spread21(q[2]) << 2) >> KNN_QUERY_CODE_SHIFT;
    ids[i] = (uint32_t)i;
}

// pruned form.  Lane i takes the i-th query of the queries' Morton order (qids), so a wave's queries are neighbours in space.
// The wave seeds its lists from a stretch of the sorted points around the place where its first query's code would be inserted
// (binary search in the sorted codes; K + KNN_QUERY_SEED positions either side: at least min(K, N) points), then scans the
// boxes that are not farther than a lane's current K-th best, leaving that stretch out.  Rejection is strict as in
// k_knn_search_k.  The result is stored at the caller's query index.
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
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63;
    const int w0 = __builtin_amdgcn_readfirstlane((blockIdx.x * 4 + (threadIdx.x >> 6)) * lanes);   // the wave's first query
    if (w0 >= Q) return;                         // a wave without a query (no barrier in this kernel)
    const int i = w0 + lane;
    const bool live = lane < lanes && i < Q;
    const size_t qi = qids[live ? i : Q - 1];
    const float px = qry[3 * qi], py = qry[3 * qi + 1], pz = qry[3 * qi + 2];
    KBest<CAP> b;
    b.init(live ? K : 0);
    auto scan = [&](int lo, int hi) {
        int j = lo;                              // wave-uniform addresses: one broadcast load per candidate
        for (; j + 4 <= hi; j += 4) {
            float d[4];
            int ci[4];
            const bool me[4] = {false, false, false, false};
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const float4 c = spts[j + u];
                const float dx = c.x - px, dy = c.y - py, dz = c.z - pz;
                d[u] = dx * dx + dy * dy + dz * dz;
                ci[u] = (int)__float_as_uint(c.w);
            }
            knn_offer4(b, d, ci, me);
        }
        for (; j < hi; j++) {
            const float4 c = spts[j];
            const float dx = c.x - px, dy = c.y - py, dz = c.z - pz;
            knn_offer(b, dx * dx + dy * dy + dz * dz, (int)__float_as_uint(c.w), false);
        }
    };
    const uint64_t code0 = qcodes[w0] << KNN_QUERY_CODE_SHIFT;
    int lo = 0, hi = N;                          // first position whose code is not below code0, in [0, N]
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (pcodes[mid] < code0) lo = mid + 1; else hi = mid;
    }
    const int pos = __builtin_amdgcn_readfirstlane(lo);
    const int wlo = max(0, pos - K - KNN_QUERY_SEED), whi = min(N, pos + K + KNN_QUERY_SEED);   // [wlo, whi)
    scan(wlo, whi);
    for (int bi = 0; bi < nbox; bi++) {
        const float *bx = boxes + 6 * bi;
        float ex = 0.f, ey = 0.f, ez = 0.f;     // distance from the query to the box, per axis
        if (px < bx[0] || px > bx[3]) ex = fminf(fabsf(px - bx[0]), fabsf(px - bx[3]));
        if (py < bx[1] || py > bx[4]) ey = fminf(fabsf(py - bx[1]), fabsf(py - bx[4]));
        if (pz < bx[2] || pz > bx[5]) ez = fminf(fabsf(pz - bx[2]), fabsf(pz - bx[5]));
        const float dist = ex * ex + ey * ey + ez * ez;
        const bool need = !(dist > b.worst());   // lanes without a query hold -inf and never need a box
        if (__builtin_amdgcn_ballot_w64(need) == 0ull) continue;
        const int blo = bi * KNN_BOX, bhi = min(N, blo + KNN_BOX);
        scan(blo, min(bhi, wlo));
        scan(max(blo, whi), bhi);
    }
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
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0;
        for (int w = 0; w < CHAMFER_WAVES; w++) t += s_w[w];
        loss[0] = (float)(t / (double)Q);
    }
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

struct KnnQueryWs { size_t codes, ids, codes_o, ids_o, codes_t, ids_t, stab, total; };
KnnQueryWs knn_query_ws(int Q, int N) {
    KnnQueryWs w;
    size_t o = knn_ws(N).total;                  // the points' side: the layout of csplat_dist2_ws, unchanged
    auto take = [&](size_t b) { const size_t at = o; o += align256(b); return at; };
    const size_t n = (size_t)(Q > 0 ? Q : 1);
    w.codes = take(n * 8); w.ids = take(n * 4); w.codes_o = take(n * 8); w.ids_o = take(n * 4);
    w.codes_t = take(n * 8); w.ids_t = take(n * 4); w.stab = take(csplat_sort_temp_bytes((int64_t)n));
    w.total = o;
    return w;
}

struct ChamferWs { size_t keys, vals, keys_o, vals_o, keys_t, vals_t, stab, total; };
ChamferWs chamfer_ws(int Q) {
    ChamferWs w;
    size_t o = 0;
    auto take = [&](size_t b) { const size_t at = o; o += align256(b); return at; };
    const size_t n = (size_t)(Q > 0 ? Q : 1);
    w.keys = take(n * 8); w.vals = take(n * 4); w.keys_o = take(n * 8); w.vals_o = take(n * 4);
    w.keys_t = take(n * 8); w.vals_t = take(n * 4); w.stab = take(csplat_sort_temp_bytes((int64_t)n));
    w.total = o;
    return w;
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
    const KnnWs w = knn_ws(N);
    const KnnQueryWs wq = knn_query_ws(Q, N);
    char *t = (char *)temp;
    float *part = (float *)(t + w.part);
    uint64_t *codes = (uint64_t *)(t + w.codes), *codes_o = (uint64_t *)(t + w.codes_o), *codes_t = (uint64_t *)(t + w.codes_t);
    uint32_t *ids = (uint32_t *)(t + w.ids), *ids_o = (uint32_t *)(t + w.ids_o), *ids_t = (uint32_t *)(t + w.ids_t);
    float4 *spts = (float4 *)(t + w.spts);
    float *boxes = (float *)(t + w.boxes);
    uint64_t *qcodes = (uint64_t *)(t + wq.codes), *qcodes_o = (uint64_t *)(t + wq.codes_o), *qcodes_t = (uint64_t *)(t + wq.codes_t);
    uint32_t *qids = (uint32_t *)(t + wq.ids), *qids_o = (uint32_t *)(t + wq.ids_o), *qids_t = (uint32_t *)(t + wq.ids_t);
    const int nparts = N < 256 * 256 ? cdiv(N, 256) : 256, nbox = cdiv(N, KNN_BOX);
    k_bbox_partial<<<nparts, 256, 0, s>>>(N, points, part);
    LAUNCH_CHECK();
    k_morton<<<cdiv(N, 256), 256, 0, s>>>(N, nparts, points, part, codes, ids);
    LAUNCH_CHECK();
    if (int rc = csplat_sort_pairs(s, codes, ids, codes_o, ids_o, codes_t, ids_t, N, 63, t + w.stab)) return rc;
    k_knn_boxes<<<nbox, 256, 0, s>>>(N, points, ids_o, spts, boxes);
    LAUNCH_CHECK();
    k_morton_query<<<cdiv(Q, 256), 256, 0, s>>>(Q, nparts, queries, part, qcodes, qids);
    LAUNCH_CHECK();
    if (int rc = csplat_sort_pairs(s, qcodes, qids, qcodes_o, qids_o, qcodes_t, qids_t, Q, KNN_QUERY_CODE_BITS, t + wq.stab)) return rc;
    const int lanes = knn_query_lanes(Q);
#define LAUNCH(CAP) k_knn_query_search<CAP><<<cdiv(cdiv(Q, lanes), 4), 256, 0, s>>>(Q, N, K, nbox, lanes, queries, qcodes_o, qids_o, codes_o, spts, boxes, out_d2, out_idx)
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
        uint64_t *keys = (uint64_t *)(t + w.keys), *keys_o = (uint64_t *)(t + w.keys_o), *keys_t = (uint64_t *)(t + w.keys_t);
        uint32_t *vals = (uint32_t *)(t + w.vals), *vals_o = (uint32_t *)(t + w.vals_o), *vals_t = (uint32_t *)(t + w.vals_t);
        int bits = 1;
        while (bits < 32 && ((uint64_t)1 << bits) < (uint64_t)N) bits++;
        HIP_TRY(hipMemsetAsync(dL_dpoints, 0, (size_t)N * 3 * sizeof(float), s));
        k_chamfer_keys<<<cdiv(Q, 256), 256, 0, s>>>(Q, idx, keys, vals);
        LAUNCH_CHECK();
        if (int rc = csplat_sort_pairs(s, keys, vals, keys_o, vals_o, keys_t, vals_t, Q, bits, t + w.stab)) return rc;
        k_chamfer_bwd_points<<<cdiv(Q, 256), 256, 0, s>>>(Q, N, keys_o, vals_o, queries, points, d2, idx, max_sq_dist, g, dL_dpoints);
        LAUNCH_CHECK();
    }
    return 0;
}

// ================================================================================================================================
// Trajectory smoothing (csplat_traj_smooth; include/csplat.h "Trajectory preprocessing" states the semantics): the reference's
// gaussian_smoothing (meshnet/data_utils.py:267-278, one KD-tree query per point per frame in Python) for all T frames of a tracked
// cloud in ONE launch.  Nothing above is touched: this is k_knn_query_brute with the frame on the grid's second axis (queries and
// points are the same frame; a wave never reads another frame) and an epilogue that forms the weighted mean straight from the K-best
// registers -- K gathers from the frame, which the slab loop has just pulled through the cache -- so no index array leaves the kernel
// unless the caller asks for it.  A candidate whose squared distance is not finite is offered as knn_offer's `self` case: it changes
// nothing.  The sum runs over the list in its ascending (d2, index) order, one float32 rounding per operation: bit-reproducible, no
// atomics.  Brute force only, O(T N^2): tracked clouds are hundreds to a few thousand points (profiles/trajectory_cost.txt shows
// where that stops being the right tool).
namespace {
__device__ __forceinline__ bool traj_finite(float v) { return fabsf(v) < __builtin_inff(); }   // (false for a NaN)

template <int CAP>
__global__ __launch_bounds__(KNN_THREADS) void k_traj_smooth(int T, int N, int K, const float *__restrict__ pts, float neg_scale,
                                                             float *__restrict__ out, float *__restrict__ out_d2, int32_t *__restrict__ out_idx) {
#pragma clang fp contract(off)
    __shared__ float s_p[KNN_SLAB * 3];
    const int i = blockIdx.x * KNN_THREADS + threadIdx.x;
    const bool live = i < N;
    for (int t = blockIdx.y; t < T; t += gridDim.y) {            // uniform per workgroup: the barriers below stay together
        const float *__restrict__ frame = pts + (size_t)t * N * 3;
        const float x = live ? frame[3 * (size_t)i] : 0.f, y = live ? frame[3 * (size_t)i + 1] : 0.f, z = live ? frame[3 * (size_t)i + 2] : 0.f;
        KBest<CAP> b;
        b.init(live ? K : 0);
        for (int base = 0; base < N; base += KNN_SLAB) {
            const int cnt = min(KNN_SLAB, N - base);
            __syncthreads();
            for (int k = threadIdx.x; k < cnt * 3; k += KNN_THREADS) s_p[k] = frame[(size_t)base * 3 + k];
            __syncthreads();
            int j = 0;
            for (; j + 4 <= cnt; j += 4) {
                float d[4];
                int ci[4];
                bool none[4];
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    const float dx = s_p[3 * (j + u)] - x, dy = s_p[3 * (j + u) + 1] - y, dz = s_p[3 * (j + u) + 2] - z;
                    d[u] = dx * dx + dy * dy + dz * dz;
                    ci[u] = base + j + u;
                    none[u] = !traj_finite(d[u]);
                }
                knn_offer4(b, d, ci, none);
            }
            for (; j < cnt; j++) {
                const float dx = s_p[3 * j] - x, dy = s_p[3 * j + 1] - y, dz = s_p[3 * j + 2] - z;
                const float d = dx * dx + dy * dy + dz * dz;
                knn_offer(b, d, base + j, !traj_finite(d));
            }
        }
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
            const bool whole = traj_finite(x) && traj_finite(y) && traj_finite(z);
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
