// csplat_knn_regs.hip -- the neighbourhood regularisers of the Gaussians' kNN graph (isometry, spring, local rigidity), fused:
// csplat_knn_regs_graph (rest lengths, weights, reverse lists), csplat_knn_regs_fwd (one launch), csplat_knn_regs_bwd (one launch,
// gather-only).  Definition: include/csplat.h.  The per-pair arithmetic lives in csplat_knn_regs_math.h.
//
// Traffic: a pair reads two 12-byte centres (and one 16-byte rotation) per time row.  Pairs are laid out node-major and both the k-NN
// output and the Gaussians are spatially coherent, so a workgroup's contiguous node range gathers rows that mostly share L2 lines; the
// algorithmic bytes are T * N * 28 read + the graph (12 * N * K), all cache resident at the sizes of a training step.
#include "csplat_common.h"
#include "csplat_knn_regs_math.h"

namespace {
constexpr int KR_THREADS = 256, KR_WAVES = KR_THREADS / 64;
constexpr int KR_FWD_MAX_BLOCKS = 1024;

// ---- graph: d0 = sqrt(d2), w = exp(-lambda_w d2) (the exponent and exp in fp64: one rounding), sort keys (neighbour, pair) and the
// neighbours' counts.  An index outside 0 .. N-1 (the -1 of a short k-NN row) is keyed N: it sorts behind every list and is counted nowhere.
__global__ __launch_bounds__(KR_THREADS) void k_knn_regs_keys(int64_t NK, int N, const int32_t *__restrict__ idx, const float *__restrict__ d2,
                                                              double lambda_w, float *__restrict__ d0, float *__restrict__ w,
                                                              uint64_t *__restrict__ keys, uint32_t *__restrict__ vals, uint32_t *__restrict__ counts) {
    const int64_t p = (int64_t)blockIdx.x * KR_THREADS + threadIdx.x;
    if (p >= NK) return;
    const int j = idx[p];
    const bool in = (unsigned)j < (unsigned)N;
    keys[p] = in ? (uint64_t)j : (uint64_t)N;
    vals[p] = (uint32_t)p;
    if (in) atomicAdd(counts + j + 1, 1u);       // (integer: the sum does not depend on the order)
    if (d2) {
        const float x = d2[p];
        d0[p] = sqrtf(x);
        w[p] = (float)exp(-lambda_w * (double)x);
    }
}

// ---- forward: one thread per pair, the T rows in order; three fp64 sums per workgroup, joined by the workgroup that arrives last
// (ticket) in a fixed order: thread k takes partials k, k + 256, ... ascending, then the lanes' and waves' fixed tree.  The geometry of
// the launch depends on N * K alone, so neither scheduling nor stream nor replay can change a bit.
// (its own loops, not block_sum of csplat_device.h: with the three sums in step the forward timed 1-2 us above the parent's runs)
__device__ __forceinline__ void kr_block_sum3(double (&acc)[3], double (*s_red)[KR_WAVES]) {
    for (int m = 0; m < 3; m++) {
        double v = acc[m];
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
        if ((threadIdx.x & 63) == 0) s_red[m][threadIdx.x >> 6] = v;
    }
    __syncthreads();
    for (int m = 0; m < 3; m++) {
        double v = 0.0;
        for (int k = 0; k < KR_WAVES; k++) v += s_red[m][k];
        acc[m] = v;
    }
    __syncthreads();
}

__global__ __launch_bounds__(KR_THREADS) void k_knn_regs_fwd(int T, int N, int K, int64_t NK, int64_t chunk, const float *__restrict__ M,
                                                             const float *__restrict__ Q, const int32_t *__restrict__ idx,
                                                             const float *__restrict__ d0, const float *__restrict__ w, float lam_iso,
                                                             float lam_spring, float lam_rigid, int iso_abs, double *__restrict__ partial,
                                                             unsigned *__restrict__ ticket, float *__restrict__ out) {
#pragma clang fp contract(off)
    __shared__ double s_red[3][KR_WAVES];
    __shared__ bool s_last;
    double acc[3] = {0.0, 0.0, 0.0};
    const int64_t p0 = (int64_t)blockIdx.x * chunk, p1 = p0 + chunk < NK ? p0 + chunk : NK;
    const float4 *q4 = reinterpret_cast<const float4 *>(Q);
    for (int64_t p = p0 + threadIdx.x; p < p1; p += KR_THREADS) {
        const int i = (int)((uint32_t)p / (uint32_t)K), j = idx[p];
        if ((unsigned)j >= (unsigned)N) continue;
        const float rest = d0[p], wt = Q ? w[p] : 0.f;
        float prev[3] = {0.f, 0.f, 0.f}, pd = 0.f, pq[4] = {0.f, 0.f, 0.f, 0.f};
        for (int t = 0; t < T; t++) {
            const float *mi = M + ((size_t)t * N + i) * 3, *mj = M + ((size_t)t * N + j) * 3;
            float off[3], q[4] = {0.f, 0.f, 0.f, 0.f};
            for (int a = 0; a < 3; a++) off[a] = mj[a] - mi[a];
            const float d = kr_len(off);
            const float x = d - rest;
            acc[0] += (double)(iso_abs ? fabsf(x) : x);
            if (Q) { const float4 v = q4[(size_t)t * N + j]; q[0] = v.x; q[1] = v.y; q[2] = v.z; q[3] = v.w; }
            if (t >= 1) {
                acc[1] += (double)fabsf(d - pd);
                if (Q) {
                    KrRot k;
                    float e[3];
                    kr_rot(pq, q, k);
                    acc[2] += (double)kr_rigid_value(k.R, off, prev, wt, e);
                }
            }
            for (int a = 0; a < 3; a++) prev[a] = off[a];
            for (int a = 0; a < 4; a++) pq[a] = q[a];
            pd = d;
        }
    }
    kr_block_sum3(acc, s_red);
    if (threadIdx.x == 0) {
        for (int m = 0; m < 3; m++) partial[3 * (size_t)blockIdx.x + m] = acc[m];
        __threadfence();
        s_last = atomicAdd(ticket, 1u) == gridDim.x - 1;
    }
    __syncthreads();
    if (!s_last) return;
    __threadfence();
    for (int m = 0; m < 3; m++) {
        double v = 0.0;
        for (unsigned k = threadIdx.x; k < gridDim.x; k += KR_THREADS) v += __builtin_nontemporal_load(partial + 3 * (size_t)k + m);
        acc[m] = v;
    }
    kr_block_sum3(acc, s_red);
    if (threadIdx.x == 0) {
        const double n0 = (double)T * (double)NK, n1 = (double)(T - 1) * (double)NK;
        const double iso = acc[0] / n0, spring = T > 1 ? acc[1] / n1 : 0.0, rigid = T > 1 ? acc[2] / n1 : 0.0;
        out[0] = (float)iso;
        out[1] = (float)spring;
        out[2] = (float)rigid;
        out[3] = (float)(((double)lam_iso * iso + (double)lam_spring * spring) + (double)lam_rigid * rigid);
        *ticket = 0u;
    }
}

// ---- backward: G lanes per (node, time row).  The lanes walk the node's items -- its K own pairs (the node is the pair's i: -f), then
// its reverse list in ascending (i, k) (the node is the pair's j: +f, and the pair's share of dQ) -- item m on lane m % G in ascending m,
// and join in a fixed xor tree.  Every pair quantity is recomputed from M and Q: nothing is stored between the passes, nothing is
// scattered, no float atomics.  One lane writes the node's rows; a row of dQ with an empty reverse list is the exact zero it started as.
template <int G>
__global__ __launch_bounds__(KR_THREADS) void k_knn_regs_bwd(int T, int N, int K, const float *__restrict__ M, const float *__restrict__ Q,
                                                             const int32_t *__restrict__ idx, const float *__restrict__ d0,
                                                             const float *__restrict__ w, const int32_t *__restrict__ rev_off,
                                                             const int32_t *__restrict__ rev_ent, float lam_iso, float lam_spring,
                                                             float lam_rigid, int iso_abs, const float *__restrict__ g,
                                                             float *__restrict__ dM, float *__restrict__ dQ) {
#pragma clang fp contract(off)
    const int t = blockIdx.y, lane = threadIdx.x % G;
    const int64_t node64 = (int64_t)blockIdx.x * (KR_THREADS / G) + threadIdx.x / G;
    const bool live = node64 < N;
    const int node = live ? (int)node64 : 0;
    const int64_t NK = (int64_t)N * K;
    const float up = g[0];
    KrCoef c;
    c.iso = up * (float)((double)lam_iso / ((double)T * (double)NK));
    c.spring = T > 1 ? up * (float)((double)lam_spring / ((double)(T - 1) * (double)NK)) : 0.f;
    c.rigid = (T > 1 && Q) ? up * (float)((double)lam_rigid / ((double)(T - 1) * (double)NK)) : 0.f;
    c.iso_abs = iso_abs;
    float am[3] = {0.f, 0.f, 0.f}, aq[4] = {0.f, 0.f, 0.f, 0.f};
    if (live) {
        const int r0 = rev_off[node], r1 = rev_off[node + 1];
        const int items = K + (r1 - r0);
        for (int m = lane; m < items; m += G) {
            float f[3];
            if (m < K) {
                const int64_t p = (int64_t)node * K + m;
                const int j = idx[p];
                if ((unsigned)j >= (unsigned)N) continue;
                kr_pair_row_grad(T, t, N, node, j, d0[p], c.rigid != 0.f ? w[p] : 0.f, M, Q, c, f, nullptr);
                for (int a = 0; a < 3; a++) am[a] -= f[a];
            } else {
                const int64_t p = (int64_t)(uint32_t)rev_ent[r0 + (m - K)];
                if (p >= NK) continue;
                kr_pair_row_grad(T, t, N, (int)((uint32_t)p / (uint32_t)K), node, d0[p], c.rigid != 0.f ? w[p] : 0.f, M, Q, c, f, dQ ? aq : nullptr);
                for (int a = 0; a < 3; a++) am[a] += f[a];
            }
        }
    }
    for (int o = G / 2; o > 0; o >>= 1) {      // (its own loop, not wave_sum<G> of csplat_device.h: one row of the cost table timed above the parent)
        for (int a = 0; a < 3; a++) am[a] += __shfl_xor(am[a], o, 64);
        if (dQ)
            for (int a = 0; a < 4; a++) aq[a] += __shfl_xor(aq[a], o, 64);
    }
    if (live && lane == 0) {
        if (dM) {
            float *pm = dM + ((size_t)t * N + node) * 3;
            for (int a = 0; a < 3; a++) pm[a] = am[a];
        }
        if (dQ) reinterpret_cast<float4 *>(dQ)[(size_t)t * N + node] = make_float4(aq[0], aq[1], aq[2], aq[3]);
    }
}

struct KnnRegsWs { size_t counts, scan, keys, vals, keys_o, keys_t, vals_t, stab, total; };
KnnRegsWs knn_regs_ws(int N, int K) {
    KnnRegsWs s;
    size_t o = 0;
    auto take = [&](size_t b) { const size_t at = o; o += align256(b); return at; };
    const size_t n = (size_t)(N > 0 ? N : 1), nk = n * (size_t)(K > 0 ? K : 1);
    s.counts = take((n + 1) * 4); s.scan = take(csplat_scan_temp_bytes((int64_t)n + 1));
    s.keys = take(nk * 8); s.vals = take(nk * 4); s.keys_o = take(nk * 8); s.keys_t = take(nk * 8); s.vals_t = take(nk * 4);
    s.stab = take(csplat_sort_temp_bytes((int64_t)nk));
    s.total = o;
    return s;
}

bool kr_sizes_ok(int T, int N, int K) {
    return T >= 1 && T < 65536 && N >= 1 && K >= 1 && K <= CSPLAT_KNN_MAX_K && (int64_t)N * K < ((int64_t)1 << 31) &&
           (int64_t)T * N < ((int64_t)1 << 31);
}
bool kr_weight_ok(float x) { return x >= 0.f && x <= 3.0e38f; }      // (false for a NaN)
}  // namespace

extern "C" size_t csplat_knn_regs_graph_temp_bytes(int N, int K) { return knn_regs_ws(N, K).total; }

extern "C" int csplat_knn_regs_graph(void *stream, int N, int K, const int32_t *idx, const float *d2, double lambda_w, float *d0, float *w,
                                     int32_t *rev_offsets, int32_t *rev_entries, void *temp) {
    CSPLAT_REQUIRE(kr_sizes_ok(1, N, K), "csplat_knn_regs_graph: need N >= 1, 1 <= K <= CSPLAT_KNN_MAX_K, N * K < 2^31");
    CSPLAT_REQUIRE(idx && rev_offsets && rev_entries && temp, "csplat_knn_regs_graph: NULL argument");
    CSPLAT_REQUIRE(!d2 || (d0 && w), "csplat_knn_regs_graph: d2 without d0 / w");
    CSPLAT_REQUIRE(!d2 || lambda_w >= 0.0, "csplat_knn_regs_graph: lambda_w is negative or NaN");
    CSPLAT_REQUIRE((((uintptr_t)rev_offsets | (uintptr_t)temp) & 15u) == 0, "csplat_knn_regs_graph: rev_offsets and temp must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    const KnnRegsWs ws = knn_regs_ws(N, K);
    char *t = (char *)temp;
    const int64_t NK = (int64_t)N * K;
    uint32_t *counts = (uint32_t *)(t + ws.counts), *vals = (uint32_t *)(t + ws.vals), *vals_t = (uint32_t *)(t + ws.vals_t);
    uint64_t *keys = (uint64_t *)(t + ws.keys), *keys_o = (uint64_t *)(t + ws.keys_o), *keys_t = (uint64_t *)(t + ws.keys_t);
    HIP_TRY(hipMemsetAsync(counts, 0, ((size_t)N + 1) * 4, s));
    k_knn_regs_keys<<<cdiv(NK, KR_THREADS), KR_THREADS, 0, s>>>(NK, N, idx, d2, lambda_w, d0, w, keys, vals, counts);
    LAUNCH_CHECK();
    // counts[0] = 0, counts[j + 1] = the pairs naming j: the inclusive scan IS the offsets [N + 1]
    if (int rc = csplat_inclusive_scan_u32(s, counts, (uint32_t *)rev_offsets, (int64_t)N + 1, t + ws.scan)) return rc;
    int bits = 1;
    while (bits < 32 && ((uint64_t)1 << bits) <= (uint64_t)N) bits++;        // keys are 0 .. N
    // stable: equal neighbours stay in ascending pair number = ascending (i, k)
    return csplat_sort_pairs(s, keys, vals, keys_o, (uint32_t *)rev_entries, keys_t, vals_t, NK, bits, t + ws.stab);
}

extern "C" size_t csplat_knn_regs_fwd_scratch_bytes(void) { return align256((size_t)KR_FWD_MAX_BLOCKS * 3 * sizeof(double)) + 256; }

extern "C" int csplat_knn_regs_fwd(void *stream, int T, int N, int K, const float *means, const float *rotations, const int32_t *idx,
                                   const float *d0, const float *w, float lambda_isometric, float lambda_spring, float lambda_rigidity,
                                   int isometric_abs, float *out4, void *scratch) {
    CSPLAT_REQUIRE(kr_sizes_ok(T, N, K), "csplat_knn_regs_fwd: need 1 <= T < 65536, N >= 1, 1 <= K <= CSPLAT_KNN_MAX_K, N * K and T * N < 2^31");
    CSPLAT_REQUIRE(means && idx && d0 && out4 && scratch && (!rotations || w), "csplat_knn_regs_fwd: NULL argument");
    CSPLAT_REQUIRE(kr_weight_ok(lambda_isometric) && kr_weight_ok(lambda_spring) && kr_weight_ok(lambda_rigidity),
                   "csplat_knn_regs_fwd: a weight is negative or not finite");
    CSPLAT_REQUIRE((((uintptr_t)rotations | (uintptr_t)scratch) & 15u) == 0, "csplat_knn_regs_fwd: rotations and scratch must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    const int64_t NK = (int64_t)N * K;
    const int64_t tiles = (NK + KR_THREADS - 1) / KR_THREADS;
    const int blocks = (int)(tiles < KR_FWD_MAX_BLOCKS ? tiles : KR_FWD_MAX_BLOCKS);
    const int64_t chunk = ((tiles + blocks - 1) / blocks) * KR_THREADS;
    double *partial = (double *)scratch;
    unsigned *ticket = (unsigned *)((char *)scratch + csplat_knn_regs_fwd_scratch_bytes() - 256);
    HIP_TRY(hipMemsetAsync(ticket, 0, 4, s));
    k_knn_regs_fwd<<<blocks, KR_THREADS, 0, s>>>(T, N, K, NK, chunk, means, rotations, idx, d0, w, lambda_isometric, lambda_spring,
                                                 lambda_rigidity, isometric_abs ? 1 : 0, partial, ticket, out4);
    LAUNCH_CHECK();
    return 0;
}

extern "C" int csplat_knn_regs_bwd(void *stream, int T, int N, int K, const float *means, const float *rotations, const int32_t *idx,
                                   const float *d0, const float *w, const int32_t *rev_offsets, const int32_t *rev_entries,
                                   float lambda_isometric, float lambda_spring, float lambda_rigidity, int isometric_abs, const float *g,
                                   float *dL_dmeans, float *dL_drotations) {
    CSPLAT_REQUIRE(kr_sizes_ok(T, N, K), "csplat_knn_regs_bwd: need 1 <= T < 65536, N >= 1, 1 <= K <= CSPLAT_KNN_MAX_K, N * K and T * N < 2^31");
    CSPLAT_REQUIRE(means && idx && d0 && rev_offsets && rev_entries && g && (dL_dmeans || dL_drotations), "csplat_knn_regs_bwd: NULL argument");
    CSPLAT_REQUIRE(kr_weight_ok(lambda_isometric) && kr_weight_ok(lambda_spring) && kr_weight_ok(lambda_rigidity),
                   "csplat_knn_regs_bwd: a weight is negative or not finite");
    CSPLAT_REQUIRE(lambda_rigidity == 0.f || (rotations && w), "csplat_knn_regs_bwd: lambda_rigidity > 0 needs rotations and w");
    CSPLAT_REQUIRE((((uintptr_t)rotations | (uintptr_t)dL_drotations) & 15u) == 0, "csplat_knn_regs_bwd: rotations and dL_drotations must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    const float *Q = lambda_rigidity != 0.f ? rotations : nullptr;          // (no rigidity term: the rotations are not read)
    if (dL_drotations && !Q) {                                              // ... and their gradient is zero
        HIP_TRY(hipMemsetAsync(dL_drotations, 0, (size_t)T * N * 4 * sizeof(float), s));
        dL_drotations = nullptr;
    }
    if (!dL_dmeans && !dL_drotations) return 0;
    // a group of 4 lanes per (node, row) up to K = 8 (own pairs + a reverse list of about K), 16 above
    if (K <= 8) {
        const dim3 grid(cdiv(N, KR_THREADS / 4), T);
        k_knn_regs_bwd<4><<<grid, KR_THREADS, 0, s>>>(T, N, K, means, Q, idx, d0, w, rev_offsets, rev_entries, lambda_isometric, lambda_spring,
                                                      lambda_rigidity, isometric_abs ? 1 : 0, g, dL_dmeans, dL_drotations);
    } else {
        const dim3 grid(cdiv(N, KR_THREADS / 16), T);
        k_knn_regs_bwd<16><<<grid, KR_THREADS, 0, s>>>(T, N, K, means, Q, idx, d0, w, rev_offsets, rev_entries, lambda_isometric, lambda_spring,
                                                       lambda_rigidity, isometric_abs ? 1 : 0, g, dL_dmeans, dL_drotations);
    }
    LAUNCH_CHECK();
    return 0;
}
