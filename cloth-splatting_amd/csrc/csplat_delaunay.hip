// csplat_delaunay.hip -- Delaunay triangulation of a planar point cloud (gfx950, wave64; include/csplat.h "Delaunay triangulation" states
// the definitions).  The reference triangulates on the host (scipy.spatial.Delaunay, meshnet/data_utils.py:371-405 and :419-440); here the
// cloud stays on the device.  Brute force, like the exact k-NN of csplat_knn.hip: made for clouds of hundreds to a few thousand points.
//   k_dl_usable   one thread per point: finite, and no lower-indexed point has the same coordinates
//   k_dl_walk     one wave per point i, no dependence between points: the exact nearest point j0, then the faces around i one after the
//                 other -- among the points strictly left of i -> j the one that no other beats under the in-circle test with the symbolic
//                 tie rule -- until the ring closes on j0 or the hull ends it, then the other way round from j0.  The 64 lanes share the
//                 candidates; their winners are joined by a butterfly in which both partners evaluate the same expression.  The first
//                 run counts the faces and edges that point i owns (it is their lowest index) and keeps up to DL_SLAB of each in the
//                 point's slab; a scan turns the counts into segments; the second run walks again only for the points that own more
//                 than a slab holds (none in a cloth-like cloud) and writes their segments
//   k_dl_order    one wave per point: its slab or segment sorted by the second vertex, which makes the whole list lexicographic
//   k_dl_finish   one workgroup: the counters, summed over the points in a fixed order
// Every decision is an exact predicate (csplat_delaunay_predicates.h), so the three walks that find a face agree on it.  No float
// atomics, no atomics on data at all (one integer atomicOr raises the status word): every output is bit-reproducible.
#include "csplat_common.h"
#include "csplat_device.h"
#include "csplat_delaunay_predicates.h"

#pragma clang fp contract(off)

namespace {

constexpr int DL_THREADS = 256;
constexpr int DL_WAVES = DL_THREADS / CSPLAT_WAVE;
constexpr int DL_MAX_N = 1 << 24;
constexpr uint32_t DL_SLAB = 16;     // faces, and edges, of a point kept by the counting walk (a point of a triangulation has six neighbours on average)
enum { DL_FACES = 0, DL_EDGES, DL_SKIPPED, DL_EXACT, DL_STATUS, DL_COUNTERS };
enum { DL_STATUS_STEPS = 1, DL_STATUS_LAYOUT = 2 };

__device__ __forceinline__ float2 dl_point(const float *__restrict__ pts, int i) { return reinterpret_cast<const float2 *>(pts)[i]; }
__device__ __forceinline__ dp_pt dl_wide(float2 v) { return dp_pt{(double)v.x, (double)v.y}; }

// the reference's length of an edge: float32, every operation rounded once
__device__ __forceinline__ float dl_length(float2 a, float2 b) {
    const float du = a.x - b.x, dv = a.y - b.y;
    return sqrtf(du * du + dv * dv);
}

__global__ __launch_bounds__(DL_THREADS) void k_dl_usable(int N, const float *__restrict__ pts, uint8_t *__restrict__ ok) {
    const int i = blockIdx.x * DL_THREADS + threadIdx.x;
    if (i >= N) return;
    const float2 p = dl_point(pts, i);
    bool good = fabsf(p.x) < __builtin_inff() && fabsf(p.y) < __builtin_inff();      // false for a NaN
    for (int j = 0; good && j < i; j++) {
        const float2 q = dl_point(pts, j);
        if (q.x == p.x && q.y == p.y) good = false;                                   // -0.0 == 0.0
    }
    ok[i] = good ? 1 : 0;
}

// Among the usable points strictly left of u -> v: the one that no other beats.  -1: there is none.  Every lane returns the same index.
// `exact` counts this lane's exact-stage decisions.  Before the butterfly's step `off` a lane's winner depends on lane mod 2 off only, so the
// step takes at most `off` different decisions, pair (r, r + off) for r < off: lane r counts it, the other lanes that repeat it do not.
__device__ int dl_apex(int N, const float *__restrict__ pts, const uint8_t *__restrict__ ok, int lane, int u, int v, dp_pt pu, dp_pt pv, unsigned &exact) {
    int best = -1;
    dp_pt pb = pu;
    for (int k = lane; k < N; k += CSPLAT_WAVE) {
        if (!ok[k] || k == u || k == v) continue;
        const dp_pt pk = dl_wide(dl_point(pts, k));
        if (dp_orient(pu, pv, pk, exact) <= 0) continue;
        if (best < 0 || dp_incircle(pu, pv, pb, pk, u, v, best, k, exact) > 0) {
            best = k;
            pb = pk;
        }
    }
    for (int off = CSPLAT_WAVE / 2; off > 0; off >>= 1) {
        const int other = __shfl_xor(best, off, CSPLAT_WAVE);
        if (other >= 0 && other != best) {
            if (best < 0) {
                best = other;
            } else {
                const int lo = best < other ? best : other, hi = best < other ? other : best;
                unsigned ex = 0;
                const bool hi_wins = dp_incircle(pu, pv, dl_wide(dl_point(pts, lo)), dl_wide(dl_point(pts, hi)), u, v, lo, hi, ex) > 0;
                best = hi_wins ? hi : lo;
                if (lane < off) exact += ex;
            }
        }
    }
    return best;
}

// the usable point nearest to point i (not i itself), ties to the lower index; -1: there is none
__device__ int dl_nearest(int N, const float *__restrict__ pts, const uint8_t *__restrict__ ok, int lane, int i, dp_pt pi, unsigned &exact) {
    int best = -1;
    dp_pt pb = pi;
    for (int k = lane; k < N; k += CSPLAT_WAVE) {
        if (!ok[k] || k == i) continue;
        const dp_pt pk = dl_wide(dl_point(pts, k));
        if (best < 0 || dp_nearer(pi, pk, pb, exact) < 0) {      // strictly nearer: ascending k keeps the lower index of a tie
            best = k;
            pb = pk;
        }
    }
    for (int off = CSPLAT_WAVE / 2; off > 0; off >>= 1) {
        const int other = __shfl_xor(best, off, CSPLAT_WAVE);
        if (other >= 0 && other != best) {
            if (best < 0) {
                best = other;
            } else {
                const int lo = best < other ? best : other, hi = best < other ? other : best;
                unsigned ex = 0;
                const bool hi_wins = dp_nearer(pi, dl_wide(dl_point(pts, hi)), dl_wide(dl_point(pts, lo)), ex) < 0;
                best = hi_wins ? hi : lo;
                if (lane < off) exact += ex;
            }
        }
    }
    return best;
}

struct DlOut {
    bool write;
    int lane, i;
    float thr;
    float2 fi;
    uint32_t f_at, f_end, e_at, e_end, f_cap, e_cap;
    int2 *__restrict__ faces, *__restrict__ slab_f;
    int *__restrict__ edges, *__restrict__ slab_e;
    uint32_t nf, ne;
    int bad;
};

// the face (i, a, b), counter-clockwise: owned by the walk of its lowest index, kept when none of its three edges is longer than thr
__device__ __forceinline__ void dl_face(DlOut &o, int a, int b, float2 fa, float2 fb) {
    if (a < o.i || b < o.i) return;
    if (dl_length(o.fi, fa) > o.thr || dl_length(fa, fb) > o.thr || dl_length(fb, o.fi) > o.thr) return;
    if (o.write && o.lane == 0) {
        const uint32_t at = o.f_at + o.nf;
        if (at < o.f_end && at < o.f_cap) o.faces[at] = make_int2(a, b);
        else o.bad |= DL_STATUS_LAYOUT;
    } else if (o.lane == 0 && o.nf < DL_SLAB) {
        o.slab_f[o.nf] = make_int2(a, b);
    }
    o.nf++;
}

// the edge (i, a): owned by its lower end, kept when it is not longer than thr
__device__ __forceinline__ void dl_edge(DlOut &o, int a, float2 fa) {
    if (a < o.i || dl_length(o.fi, fa) > o.thr) return;
    if (o.write && o.lane == 0) {
        const uint32_t at = o.e_at + o.ne;
        if (at < o.e_end && at < o.e_cap) o.edges[at] = a;
        else o.bad |= DL_STATUS_LAYOUT;
    } else if (o.lane == 0 && o.ne < DL_SLAB) {
        o.slab_e[o.ne] = a;
    }
    o.ne++;
}

// counts [2N]: faces of point i at [i], edges at [N + i];  scan [2N]: the inclusive scan of counts (read when `write`);  slab_f, slab_e
// [N][DL_SLAB]: what the counting walk keeps of point i.  The writing walk leaves at once for a point whose slabs hold everything.
__global__ __launch_bounds__(DL_THREADS) void k_dl_walk(int N, const float *__restrict__ pts, const uint8_t *__restrict__ ok, float thr, int write,
                                                        uint32_t *__restrict__ counts, const uint32_t *__restrict__ scan, uint32_t *__restrict__ exact_out,
                                                        int2 *__restrict__ faces, int *__restrict__ edges, int2 *__restrict__ slab_f,
                                                        int *__restrict__ slab_e, uint32_t f_cap, uint32_t e_cap, int *status) {
    const int lane = threadIdx.x & (CSPLAT_WAVE - 1), i = blockIdx.x * DL_WAVES + (threadIdx.x / CSPLAT_WAVE);
    if (i >= N) return;                                                               // the whole wave
    if (write && counts[i] <= DL_SLAB && counts[N + i] <= DL_SLAB) return;            // the whole wave, too
    DlOut o;
    o.slab_f = slab_f + (size_t)i * DL_SLAB, o.slab_e = slab_e + (size_t)i * DL_SLAB;
    o.write = write != 0, o.lane = lane, o.i = i, o.thr = thr, o.fi = dl_point(pts, i);
    o.faces = faces, o.edges = edges, o.f_cap = f_cap, o.e_cap = e_cap, o.nf = o.ne = 0, o.bad = 0;
    o.f_at = o.f_end = o.e_at = o.e_end = 0;
    if (o.write) {
        const uint32_t all_faces = scan[N - 1];
        o.f_at = i ? scan[i - 1] : 0, o.f_end = scan[i];
        o.e_at = scan[N + i - 1] - all_faces, o.e_end = scan[N + i] - all_faces;
    }
    unsigned exact = 0;
    if (ok[i]) {
        const dp_pt pi = dl_wide(o.fi);
        const int j0 = dl_nearest(N, pts, ok, lane, i, pi, exact);
        if (j0 >= 0) {
            const float2 f0 = dl_point(pts, j0);
            int steps = 0, j = j0;
            float2 fj = f0;
            bool closed = false;
            for (;;) {                                                                // counter-clockwise: the apex left of i -> j
                const int k = dl_apex(N, pts, ok, lane, i, j, pi, dl_wide(fj), exact);
                if (k < 0) break;
                if (++steps > N) {
                    o.bad |= DL_STATUS_STEPS;
                    closed = true;
                    break;
                }
                const float2 fk = dl_point(pts, k);
                dl_face(o, j, k, fj, fk);
                if (k == j0) {
                    closed = true;
                    break;
                }
                dl_edge(o, k, fk);
                j = k, fj = fk;
            }
            if (!closed) {                                                            // i is on the hull: the other way, the apex left of j -> i
                j = j0, fj = f0;
                for (;;) {
                    const int k = dl_apex(N, pts, ok, lane, j, i, dl_wide(fj), pi, exact);
                    if (k < 0) break;
                    if (++steps > N) {
                        o.bad |= DL_STATUS_STEPS;
                        break;
                    }
                    const float2 fk = dl_point(pts, k);
                    dl_face(o, k, j, fk, fj);
                    dl_edge(o, k, fk);
                    j = k, fj = fk;
                }
            }
            if (steps > 0) dl_edge(o, j0, f0);                                        // (i, j0) is an edge of a face unless every point is collinear
        }
    }
    exact = wave_sum(exact);
    if (lane == 0) {
        if (o.write) {
            if (o.nf != o.f_end - o.f_at || o.ne != o.e_end - o.e_at) o.bad |= DL_STATUS_LAYOUT;
        } else {
            counts[i] = o.nf;
            counts[N + i] = o.ne;
            exact_out[i] = exact;
        }
        if (o.bad) atomicOr(status, o.bad);
    }
}

__global__ __launch_bounds__(DL_THREADS) void k_dl_order(int N, const uint32_t *__restrict__ scan, const int2 *__restrict__ faces, const int *__restrict__ edges,
                                                         const int2 *__restrict__ slab_f, const int *__restrict__ slab_e, uint32_t f_cap, uint32_t e_cap,
                                                         int32_t *__restrict__ out_faces, int32_t *__restrict__ out_edges) {
    const int lane = threadIdx.x & (CSPLAT_WAVE - 1), i = blockIdx.x * DL_WAVES + (threadIdx.x / CSPLAT_WAVE);
    if (i >= N) return;
    const uint32_t all_faces = scan[N - 1];
    uint32_t at = i ? scan[i - 1] : 0, owned = scan[i] - at;
    uint32_t n = at < f_cap ? (owned < f_cap - at ? owned : f_cap - at) : 0;          // never beyond the output's capacity
    const int2 *__restrict__ src_f = owned <= DL_SLAB ? slab_f + (size_t)i * DL_SLAB : faces + at;
    for (uint32_t f = lane; f < n; f += CSPLAT_WAVE) {                                // second vertices are distinct: the ranks are too
        const int2 me = src_f[f];
        uint32_t rank = 0;
        for (uint32_t g = 0; g < n; g++) rank += src_f[g].x < me.x;
        int32_t *dst = out_faces + 3 * (size_t)(at + rank);
        dst[0] = i, dst[1] = me.x, dst[2] = me.y;
    }
    at = scan[N + i - 1] - all_faces, owned = scan[N + i] - all_faces - at;
    n = at < e_cap ? (owned < e_cap - at ? owned : e_cap - at) : 0;
    const int *__restrict__ src_e = owned <= DL_SLAB ? slab_e + (size_t)i * DL_SLAB : edges + at;
    for (uint32_t f = lane; f < n; f += CSPLAT_WAVE) {
        const int me = src_e[f];
        uint32_t rank = 0;
        for (uint32_t g = 0; g < n; g++) rank += src_e[g] < me;
        int32_t *dst = out_edges + 2 * (size_t)(at + rank);
        dst[0] = i, dst[1] = me;
    }
}

__global__ __launch_bounds__(DL_THREADS) void k_dl_finish(int N, const uint8_t *__restrict__ ok, const uint32_t *__restrict__ scan, const uint32_t *__restrict__ exact,
                                                          uint32_t f_cap, uint32_t e_cap, int64_t *__restrict__ counters) {
    __shared__ unsigned long long s_skip[DL_THREADS], s_exact[DL_THREADS];
    unsigned long long skip = 0, ex = 0;
    for (int i = threadIdx.x; i < N; i += DL_THREADS) skip += ok[i] ? 0 : 1, ex += exact[i];
    s_skip[threadIdx.x] = skip, s_exact[threadIdx.x] = ex;
    __syncthreads();
    for (int half = DL_THREADS / 2; half > 0; half >>= 1) {
        if ((int)threadIdx.x < half) s_skip[threadIdx.x] += s_skip[threadIdx.x + half], s_exact[threadIdx.x] += s_exact[threadIdx.x + half];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const uint32_t nf = scan[N - 1], ne = scan[2 * (size_t)N - 1] - nf;
        counters[DL_FACES] = nf < f_cap ? nf : f_cap;
        counters[DL_EDGES] = ne < e_cap ? ne : e_cap;
        counters[DL_SKIPPED] = (int64_t)s_skip[0];
        counters[DL_EXACT] = (int64_t)s_exact[0];
        if (nf > f_cap || ne > e_cap) counters[DL_STATUS] |= DL_STATUS_LAYOUT;
    }
}

struct DlTemp {
    size_t ok, counts, scan, exact, faces, edges, slab_f, slab_e, scan_temp, total;
};

DlTemp dl_layout(int N) {
    DlTemp t;
    size_t at = 0;
    const size_t n = (size_t)N;
    t.ok = at, at += align256(n);
    t.counts = at, at += align256(2 * n * sizeof(uint32_t));
    t.scan = at, at += align256(2 * n * sizeof(uint32_t));
    t.exact = at, at += align256(n * sizeof(uint32_t));
    t.faces = at, at += align256(2 * n * sizeof(int2));
    t.edges = at, at += align256(3 * n * sizeof(int));
    t.slab_f = at, at += align256(n * DL_SLAB * sizeof(int2));
    t.slab_e = at, at += align256(n * DL_SLAB * sizeof(int));
    t.scan_temp = at, at += align256(csplat_scan_temp_bytes(2 * (int64_t)N));
    t.total = at;
    return t;
}

bool dl_overlap(const void *a, size_t na, const void *b, size_t nb) {
    if (!a || !b || na == 0 || nb == 0) return false;
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + nb && y < x + na;
}

}  // namespace

extern "C" int csplat_delaunay_temp_bytes(int N, size_t *bytes) {
    CSPLAT_REQUIRE(N >= 0 && N < DL_MAX_N, "csplat_delaunay_temp_bytes: N must lie in 0 .. 2^24 - 1");
    CSPLAT_REQUIRE(bytes, "csplat_delaunay_temp_bytes: NULL bytes");
    *bytes = N ? dl_layout(N).total : 0;
    return 0;
}

extern "C" int csplat_delaunay(void *stream, int N, const float *points, int has_threshold, double norm_threshold, int32_t *faces, int32_t *edges,
                               int64_t *counters, void *temp) {
    CSPLAT_REQUIRE(N >= 0 && N < DL_MAX_N, "csplat_delaunay: N must lie in 0 .. 2^24 - 1");
    CSPLAT_REQUIRE(has_threshold == 0 || has_threshold == 1, "csplat_delaunay: has_threshold is 0 or 1");
    CSPLAT_REQUIRE(!has_threshold || norm_threshold == norm_threshold, "csplat_delaunay: norm_threshold is NaN");
    CSPLAT_REQUIRE(counters && ((uintptr_t)counters & 7u) == 0, "csplat_delaunay: counters is NULL or not 8-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    if (N == 0) {
        HIP_TRY(hipMemsetAsync(counters, 0, DL_COUNTERS * sizeof(int64_t), s));
        return 0;
    }
    CSPLAT_REQUIRE(points && faces && edges && temp, "csplat_delaunay: NULL points, faces, edges or temp");
    CSPLAT_REQUIRE(((uintptr_t)points & 7u) == 0 && (((uintptr_t)faces | (uintptr_t)edges) & 3u) == 0 && ((uintptr_t)temp & 255u) == 0,
                   "csplat_delaunay: points must be 8-byte aligned, faces and edges 4-byte aligned, temp 256-byte aligned");
    const DlTemp t = dl_layout(N);
    const size_t n = (size_t)N, pb = n * 8, fb = 2 * n * 12, eb = 3 * n * 8, cb = DL_COUNTERS * sizeof(int64_t);
    CSPLAT_REQUIRE(!dl_overlap(faces, fb, points, pb) && !dl_overlap(edges, eb, points, pb) && !dl_overlap(counters, cb, points, pb) &&
                       !dl_overlap(temp, t.total, points, pb) && !dl_overlap(faces, fb, edges, eb) && !dl_overlap(faces, fb, counters, cb) &&
                       !dl_overlap(faces, fb, temp, t.total) && !dl_overlap(edges, eb, counters, cb) && !dl_overlap(edges, eb, temp, t.total) &&
                       !dl_overlap(counters, cb, temp, t.total),
                   "csplat_delaunay: an output or temp overlaps another operand");
    // (float)norm_threshold: a double beyond the float32 range becomes +-inf, and no length is greater than +inf
    const float thr = has_threshold ? (float)norm_threshold : __builtin_inff();
    char *base = (char *)temp;
    uint8_t *ok = (uint8_t *)(base + t.ok);
    uint32_t *counts = (uint32_t *)(base + t.counts), *scan = (uint32_t *)(base + t.scan), *exact = (uint32_t *)(base + t.exact);
    int2 *tf = (int2 *)(base + t.faces);
    int *te = (int *)(base + t.edges), *se = (int *)(base + t.slab_e);
    int2 *sf = (int2 *)(base + t.slab_f);
    const uint32_t f_cap = 2u * (uint32_t)N, e_cap = 3u * (uint32_t)N;
    int *status = (int *)(counters + DL_STATUS);
    HIP_TRY(hipMemsetAsync(counters, 0, cb, s));
    k_dl_usable<<<cdiv(N, DL_THREADS), DL_THREADS, 0, s>>>(N, points, ok);
    LAUNCH_CHECK();
    const int waves = cdiv(N, DL_WAVES);
    k_dl_walk<<<waves, DL_THREADS, 0, s>>>(N, points, ok, thr, 0, counts, scan, exact, tf, te, sf, se, f_cap, e_cap, status);
    LAUNCH_CHECK();
    if (int rc = csplat_inclusive_scan_u32(s, counts, scan, 2 * (int64_t)N, base + t.scan_temp)) return rc;
    k_dl_walk<<<waves, DL_THREADS, 0, s>>>(N, points, ok, thr, 1, counts, scan, exact, tf, te, sf, se, f_cap, e_cap, status);
    LAUNCH_CHECK();
    k_dl_order<<<waves, DL_THREADS, 0, s>>>(N, scan, tf, te, sf, se, f_cap, e_cap, faces, edges);
    LAUNCH_CHECK();
    k_dl_finish<<<1, DL_THREADS, 0, s>>>(N, ok, scan, exact, f_cap, e_cap, counters);
    LAUNCH_CHECK();
    return 0;
}
