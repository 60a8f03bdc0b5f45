// csplat_plan.hip -- the planning end of the pipeline: what a model-predictive planner needs AROUND the batched MeshNet rollout (gfx950,
// wave64; include/csplat.h, "Planning", states the semantics).  The reference plans by rolling the GNN out for A candidate action
// sequences in one block-diagonal graph (meshnet/dataloader_sim.py:248-288), takes (pos - goal).pow(2).mean() per candidate
// (manipulation/planning.py:425) and picks the cheapest (:311).  Candidates are stacked PyG-style: node n of candidate b is row b*N + n.
//   k_plan_integrate   one workgroup per candidate: the rollout step's tail for every candidate (pin the grasped node to the step's
//                      action, predictions row, positions, history shift -- the batched twin of k_rollout_integrate, csplat_gnn.hip) and,
//                      with a goal, the step's term of the candidate's cost
//   k_plan_cost        one workgroup per candidate: the same cost term on stored positions
//   k_plan_select      one thread per candidate: its rank by counting against LDS tiles of the cost vector; ranks < K are stored
//   k_plan_refit       one thread per (t, c): mean and deviation of the K elite rows in the order r = 0 .. K-1, the smoothed mu / sigma
//   k_plan_sample      one thread per element: the new candidates from mu, sigma and the caller's noise; row 0 is the incumbent
// A candidate's cost word belongs to ONE workgroup, which sums the candidate's 3N terms in an order fixed by N alone (each thread its
// residue class of PL_THREADS in increasing index, a xor tree over the wave, the waves in order): a candidate's cost is a function of its
// own positions, bit for bit, whatever B and b are, and the same through k_plan_integrate and k_plan_cost.  No atomics anywhere.
// Every access is 4 bytes per lane at consecutive addresses (a candidate's 3N floats start at a multiple of 12 bytes: no wider access is
// aligned for every N).  Algorithmic bytes per candidate element and step, integrate: v, pos read and written, H history rows moved, the
// predictions row, the goal and a third of a node weight -- (4 + 2H + 3) * 4 bytes at most; cost: 3 * 4 bytes.
#include <initializer_list>

#include "csplat_common.h"
#include "csplat_device.h"

namespace {

constexpr int PL_THREADS = 256, PL_SEL_TILE = 1024, PL_BATCH = 8;

// Elementwise arithmetic in torch's order ((pos + v) - goal, squared, weighted; alpha * mu + (1 - alpha) * m): no contraction, as the
// rollout kernels of csplat_gnn.hip
#pragma clang fp contract(off)

__device__ __forceinline__ float plan_term(float p, float g, float w) {
    const float d = p - g;
    return w * (d * d);
}

// cost[b] = (keep ? cost[b] : 0) + w * (sum / 3N), by thread 0 of the candidate's workgroup
__device__ __forceinline__ void plan_cost_store(float acc, int n3, float w, bool keep, float *__restrict__ cost_b) {
    __shared__ float s_sum[PL_THREADS / 64];
    block_sum<PL_THREADS>(s_sum, acc);
    if (threadIdx.x == 0) {
        const float mean = acc / (float)n3;
        const float term = w * mean;
        *cost_b = keep ? *cost_b + term : term;
    }
}

// grid B.  COST: the launch carries the step's cost term (goal given and the step's weight in play)
template <bool COST>
__global__ __launch_bounds__(PL_THREADS) void k_plan_integrate(int N, int H, int T, int k, long long BN3, float *__restrict__ v,
                                                               const float *__restrict__ actions, long long grasped,
                                                               float *__restrict__ pos, float *__restrict__ hist,
                                                               float *__restrict__ preds, const float *__restrict__ goal,
                                                               const float *__restrict__ node_w, const float *__restrict__ step_w,
                                                               float *__restrict__ cost) {
    const int b = blockIdx.x, n3 = 3 * N;
    const long long base = (long long)b * n3;
    const float *__restrict__ act = actions + ((long long)b * T + k) * 3;
    float acc = 0.f;
    for (int j = threadIdx.x; j < n3; j += PL_THREADS) {
        const int n = j / 3, c = j - 3 * n;
        const long long i = base + j;
        const float val = (long long)n == grasped ? act[c] : v[i];
        v[i] = val;
        if (preds) preds[(long long)k * BN3 + i] = val;
        const float p = pos[i] + val;
        pos[i] = p;
        for (int h = 0; h + 1 < H; h++) hist[(long long)h * BN3 + i] = hist[(long long)(h + 1) * BN3 + i];
        hist[(long long)(H - 1) * BN3 + i] = val;
        if (COST) acc = acc + plan_term(p, goal[j], node_w ? node_w[n] : 1.f);
    }
    if (COST) plan_cost_store(acc, n3, step_w ? step_w[k] : 1.f, true, cost + b);
}

// grid B: the cost term of stored positions
__global__ __launch_bounds__(PL_THREADS) void k_plan_cost(int N, const float *__restrict__ pos, const float *__restrict__ goal,
                                                          const float *__restrict__ node_w, float w, int accumulate,
                                                          float *__restrict__ cost) {
    const int b = blockIdx.x, n3 = 3 * N;
    const long long base = (long long)b * n3;
    float acc = 0.f;
    for (int j = threadIdx.x; j < n3; j += PL_THREADS) {
        const int n = j / 3;
        acc = acc + plan_term(pos[base + j], goal[j], node_w ? node_w[n] : 1.f);
    }
    plan_cost_store(acc, n3, w, accumulate != 0, cost + b);
}

// a key whose unsigned order is torch.sort's order of floats: -inf < ... < -0 == +0 < ... < +inf < every NaN, all NaN equal
__device__ __forceinline__ unsigned plan_key(float x) {
    if (x != x) return 0xFFFFFFFFu;
    const unsigned u = x == 0.f ? 0u : __float_as_uint(x);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// rank[i] = the number of j with (key[j], j) < (key[i], i): a permutation of 0 .. B-1, the stable sort's.  Tiles of PL_SEL_TILE keys
// through LDS; every lane reads the same 16 bytes at a time (a broadcast).  An entry past B carries the largest key and an index above
// every i: it is never counted
__global__ __launch_bounds__(PL_THREADS) void k_plan_select(int B, int K, const float *__restrict__ cost, int *__restrict__ order,
                                                            float *__restrict__ best) {
    __shared__ uint4 s_key[PL_SEL_TILE / 4];
    unsigned *s_k = reinterpret_cast<unsigned *>(s_key);
    const int gi = blockIdx.x * PL_THREADS + threadIdx.x;
    const int i = gi < B ? gi : B - 1;
    const float mine = cost[i];
    const unsigned ki = plan_key(mine);
    int rank = 0;
    for (int t0 = 0; t0 < B; t0 += PL_SEL_TILE) {
        __syncthreads();
        for (int q = threadIdx.x; q < PL_SEL_TILE; q += PL_THREADS) s_k[q] = t0 + q < B ? plan_key(cost[t0 + q]) : 0xFFFFFFFFu;
        __syncthreads();
        const int lim = B - t0 < PL_SEL_TILE ? B - t0 : PL_SEL_TILE;
        for (int q = 0; q < lim; q += 4) {
            const uint4 kk = s_key[q >> 2];
            const int j = t0 + q;
            rank += (kk.x < ki || (kk.x == ki && j < i)) ? 1 : 0;
            rank += (kk.y < ki || (kk.y == ki && j + 1 < i)) ? 1 : 0;
            rank += (kk.z < ki || (kk.z == ki && j + 2 < i)) ? 1 : 0;
            rank += (kk.w < ki || (kk.w == ki && j + 3 < i)) ? 1 : 0;
        }
    }
    if (gi < B && rank < K) {
        order[rank] = i;
        best[rank] = mine;
    }
}

// one thread per (t, c) = column j of the [B][3T] action matrix: the elite rows PL_BATCH at a time (all of a batch's loads are requested
// before the first is used), summed in the order r = 0 .. K-1.  An index outside [0, B) is clamped: no load leaves the array
__global__ __launch_bounds__(PL_THREADS) void k_plan_refit(int B, int T3, int K, const float *__restrict__ actions,
                                                           const int *__restrict__ order, float *__restrict__ mu,
                                                           float *__restrict__ sigma, float alpha, float sigma_min) {
    const int j = blockIdx.x * PL_THREADS + threadIdx.x;
    if (j >= T3) return;
    float m = 0.f, s = 0.f;
    for (int pass = 0; pass < 2; pass++) {
        float sum = 0.f;
        for (int r0 = 0; r0 < K; r0 += PL_BATCH) {
            float a[PL_BATCH];
#pragma unroll
            for (int q = 0; q < PL_BATCH; q++) {
                int row = order[r0 + q < K ? r0 + q : K - 1];
                row = row < 0 ? 0 : (row > B - 1 ? B - 1 : row);
                a[q] = actions[(long long)row * T3 + j];
            }
#pragma unroll
            for (int q = 0; q < PL_BATCH; q++) {
                const float d = a[q] - m;
                const float x = pass == 0 ? a[q] : d * d;
                sum = r0 + q < K ? sum + x : sum;
            }
        }
        if (pass == 0) m = sum / (float)K;
        else s = sqrtf(sum / (float)K);
    }
    const float one_minus = 1.f - alpha;
    mu[j] = alpha * mu[j] + one_minus * m;
    const float sg = alpha * sigma[j] + one_minus * s;
    sigma[j] = sg < sigma_min ? sigma_min : sg;          // (a NaN stays a NaN, as torch.clamp)
}

__device__ __forceinline__ float plan_clamp(float x, float a_max) {
    return a_max > 0.f ? (x < -a_max ? -a_max : (x > a_max ? a_max : x)) : x;
}

// one thread per element of the [B][3T] action matrix
__global__ __launch_bounds__(PL_THREADS) void k_plan_sample(long long total, int T3, float *__restrict__ actions,
                                                            const float *__restrict__ mu, const float *__restrict__ sigma,
                                                            const float *__restrict__ noise, float a_max) {
    const long long i = (long long)blockIdx.x * PL_THREADS + threadIdx.x;
    if (i >= total) return;
    const int j = (int)(i % T3);
    const float m = mu[j];
    const float x = i < T3 ? m : m + sigma[j] * noise[i];
    actions[i] = plan_clamp(x, a_max);
}
#pragma clang fp contract(fast)

inline bool plan_aligned4(std::initializer_list<const void *> ps) {
    uintptr_t u = 0;
    for (const void *p : ps) u |= (uintptr_t)p;
    return (u & 3u) == 0;
}

}  // namespace

extern "C" int csplat_plan_integrate(void *stream, int B, int N, int H, int T, int k, float *v, const float *actions, int64_t grasped,
                                     float *pos, float *hist, float *preds, const float *goal, const float *node_w, const float *step_w,
                                     float *cost) {
    CSPLAT_REQUIRE(B >= 0 && N >= 0 && (int64_t)B * N < ((int64_t)1 << 29), "csplat_plan_integrate: B, N >= 0 and B * N < 2^29");
    CSPLAT_REQUIRE(H >= 1 && T >= 1 && k >= 0 && k < T, "csplat_plan_integrate: H >= 1, T >= 1, 0 <= k < T");
    if (B == 0 || N == 0) return 0;
    CSPLAT_REQUIRE(v && actions && pos && hist, "csplat_plan_integrate: a NULL operand (v, actions, pos, hist)");
    CSPLAT_REQUIRE(!goal || cost, "csplat_plan_integrate: a goal needs the cost array");
    CSPLAT_REQUIRE(plan_aligned4({v, actions, pos, hist, preds, goal, node_w, step_w, cost}),
                   "csplat_plan_integrate: operands must be 4-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    const long long BN3 = (long long)B * N * 3;
    // step_w == NULL: the weight is 1 at the last step and 0 before it -- the earlier steps form no cost term at all
    const bool with_cost = goal && (step_w || k == T - 1);
    if (with_cost)
        k_plan_integrate<true><<<(unsigned)B, PL_THREADS, 0, s>>>(N, H, T, k, BN3, v, actions, (long long)grasped, pos, hist, preds, goal,
                                                                  node_w, step_w, cost);
    else
        k_plan_integrate<false><<<(unsigned)B, PL_THREADS, 0, s>>>(N, H, T, k, BN3, v, actions, (long long)grasped, pos, hist, preds, goal,
                                                                   node_w, step_w, cost);
    LAUNCH_CHECK();
    return 0;
}

extern "C" int csplat_plan_cost(void *stream, int B, int N, const float *pos, const float *goal, const float *node_w, float w,
                                int accumulate, float *cost) {
    CSPLAT_REQUIRE(B >= 0 && N >= 0 && (int64_t)B * N < ((int64_t)1 << 29), "csplat_plan_cost: B, N >= 0 and B * N < 2^29");
    CSPLAT_REQUIRE(w == w, "csplat_plan_cost: the weight is a number");
    if (B == 0 || N == 0) return 0;
    CSPLAT_REQUIRE(pos && goal && cost, "csplat_plan_cost: a NULL operand (pos, goal, cost)");
    CSPLAT_REQUIRE(plan_aligned4({pos, goal, node_w, cost}), "csplat_plan_cost: operands must be 4-byte aligned");
    k_plan_cost<<<(unsigned)B, PL_THREADS, 0, (hipStream_t)stream>>>(N, pos, goal, node_w, w, accumulate, cost);
    LAUNCH_CHECK();
    return 0;
}

extern "C" int csplat_plan_select(void *stream, int B, int K, const float *cost, int *order, float *best) {
    CSPLAT_REQUIRE(B >= 0 && B <= 65536, "csplat_plan_select: 0 <= B <= 65536");
    CSPLAT_REQUIRE(K >= 0 && K <= B, "csplat_plan_select: 0 <= K <= B");
    if (B == 0 || K == 0) return 0;
    CSPLAT_REQUIRE(cost && order && best, "csplat_plan_select: a NULL operand (cost, order, best)");
    CSPLAT_REQUIRE(plan_aligned4({cost, order, best}), "csplat_plan_select: operands must be 4-byte aligned");
    k_plan_select<<<(unsigned)cdiv(B, PL_THREADS), PL_THREADS, 0, (hipStream_t)stream>>>(B, K, cost, order, best);
    LAUNCH_CHECK();
    return 0;
}

extern "C" int csplat_plan_refit_sample(void *stream, int B, int T, int K, float *actions, const int *order, float *mu, float *sigma,
                                        const float *noise, float alpha, float sigma_min, float a_max) {
    CSPLAT_REQUIRE(B >= 0 && T >= 0 && (int64_t)B * T < ((int64_t)1 << 29), "csplat_plan_refit_sample: B, T >= 0 and B * T < 2^29");
    CSPLAT_REQUIRE(K >= 0 && K <= B, "csplat_plan_refit_sample: 0 <= K <= B");
    CSPLAT_REQUIRE(alpha >= 0.f && alpha <= 1.f && sigma_min >= 0.f && a_max == a_max,
                   "csplat_plan_refit_sample: 0 <= alpha <= 1, sigma_min >= 0, a_max is a number");
    if (B == 0 || T == 0) return 0;
    CSPLAT_REQUIRE(actions && mu && sigma && (noise || B == 1), "csplat_plan_refit_sample: a NULL operand (actions, mu, sigma, noise)");
    CSPLAT_REQUIRE(K == 0 || order, "csplat_plan_refit_sample: K > 0 needs the elite indices");
    CSPLAT_REQUIRE(plan_aligned4({actions, order, mu, sigma, noise}), "csplat_plan_refit_sample: operands must be 4-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    const int T3 = 3 * T;
    // two launches on the stream: every elite row is read before any row is written
    if (K > 0) {
        k_plan_refit<<<(unsigned)cdiv(T3, PL_THREADS), PL_THREADS, 0, s>>>(B, T3, K, actions, order, mu, sigma, alpha, sigma_min);
        LAUNCH_CHECK();
    }
    const long long total = (long long)B * T3;
    k_plan_sample<<<(unsigned)cdiv(total, PL_THREADS), PL_THREADS, 0, s>>>(total, T3, actions, mu, sigma, noise, a_max);
    LAUNCH_CHECK();
    return 0;
}
