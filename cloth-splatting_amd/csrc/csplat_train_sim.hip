// csplat_train_sim.hip -- the state transition of the unrolled MeshNet training loss (gfx950, wave64; include/csplat.h "MeshNet training
// transition" states the semantics).  The reference advances the graph state between the predictions of one training step with
// update_prediction (train_meshnet_sim.py:322-359): a dozen indexing operations and two PyG transforms, with an autograd graph through
// index_select and norm behind them.  Here:
//   k_train_update_fwd   ONE launch: the first N threads take the nodes (history shift, last slot, new position), the next E the edges.
//                        An edge thread RECOMPUTES its two endpoint positions from the node inputs with the same rounded operations (the
//                        same bits) instead of waiting for the node threads: at E / N = 30 that is 36 gathered floats per edge out of a
//                        node table of 72 + 24 H bytes per node -- 1 MB at N = 10^4, resident in L2 -- against a dependent kernel boundary
//                        and a second host launch in a step that is bound by the host.  (Chosen from those figures, not from an A/B run.)
//   k_train_update_bwd   ONE launch, one thread per node: the gradient of the node's position gathered over its out-edges (CSR by source)
//                        and then its in-edges (CSR by destination), each in ascending edge id, as k_edge_len_adam gathers.  The edge
//                        vector and its length are read back from the forward's edge_feat row.  No atomics: bit-reproducible.
// Float arithmetic without contraction, every operation one float32 rounding, so a float32 restatement gives the same bits.  Written with
// PLAIN operators under the pragma below, not with the __fmul_rn / __fadd_rn intrinsics: those are inline functions of a header that is
// compiled before the pragma, their instructions carry the contraction flag, and a product that feeds a sum (pred * std + mean) came out
// as one v_fma through them.  The squared length is the one exception, spelled out: csplat_gnn_edge_features (compiled with contraction)
// evaluates it as fma(dz, dz, fma(dx, dx, dy * dy)), and the edge features here are bit-equal to that kernel run on new_pos.
// Algorithmic bytes: forward 24 H N + 72 N read, 12 H N + 12 N written, 16 E + 288 E gathered (L2), 16 E written; backward 32 E x 2
// gathered, 36 N read, 24 N written.
#include "csplat_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int TRAIN_SIM_THREADS = 256;

struct TrainNodeIn {
    const float *__restrict__ vel, *__restrict__ noise, *__restrict__ pred, *__restrict__ omean, *__restrict__ ostd, *__restrict__ init,
        *__restrict__ old_act, *__restrict__ act;
    int H;
};

// vn[n][3 (H - 1) + c]: the newest velocity with the noise on it
__device__ __forceinline__ float train_last_velocity(const TrainNodeIn &in, int64_t n, int c) {
    const int64_t i = n * (3 * in.H) + 3 * (in.H - 1) + c;
    return in.noise ? in.vel[i] + in.noise[i] : in.vel[i];
}

// new_pos[n][c] from the node inputs: node and edge threads both call this, so both hold the same bits
__device__ __forceinline__ float train_new_pos(const TrainNodeIn &in, int64_t n, int c, float last) {
    const int64_t i = 3 * n + c;
    const float a = in.act[i], o = in.old_act[i], p0 = in.init[i];
    float acc = in.pred[i];
    if (in.ostd) acc = acc * in.ostd[c] + in.omean[c];          // (a product and a sum, each rounded: contraction is off)
    const float nv = o != 0.f ? o : last + acc;
    return (a == 0.f ? p0 + nv : p0) + a;
}

__global__ __launch_bounds__(TRAIN_SIM_THREADS) void k_train_update_fwd(int N, int64_t n_edge, int64_t E, TrainNodeIn in,
                                                                       const int64_t *__restrict__ edge_index, float *__restrict__ hist,
                                                                       float *__restrict__ edge_feat, float *__restrict__ new_pos) {
    const int64_t g = (int64_t)blockIdx.x * TRAIN_SIM_THREADS + threadIdx.x;
    if (g < N) {
        const int W = 3 * in.H;
        const int64_t row = g * W;
        if (hist)
            for (int k = 3; k < W; k++) hist[row + k - 3] = in.noise ? in.vel[row + k] + in.noise[row + k] : in.vel[row + k];
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const float last = train_last_velocity(in, g, c), a = in.act[3 * g + c];
            if (hist) hist[row + W - 3 + c] = a != 0.f ? a : last;
            if (new_pos) new_pos[3 * g + c] = train_new_pos(in, g, c, last);
        }
        return;
    }
    const int64_t e = g - N;
    if (e >= n_edge) return;
    const int64_t r = edge_index[e], q = edge_index[E + e];
    // an index outside 0 .. N-1 is the caller's error (the Python surface checks the range): its row is NaN and nothing outside the inputs is read
    const bool inside = (uint64_t)r < (uint64_t)N && (uint64_t)q < (uint64_t)N;
    float d[3];
#pragma unroll
    for (int c = 0; c < 3; c++)
        d[c] = inside ? train_new_pos(in, r, c, train_last_velocity(in, r, c)) - train_new_pos(in, q, c, train_last_velocity(in, q, c))
                      : __builtin_nanf("");
    // (the squared length as csplat_gnn_edge_features' object code forms it)
    const float len = sqrtf(__fmaf_rn(d[2], d[2], __fmaf_rn(d[0], d[0], d[1] * d[1])));
    reinterpret_cast<float4 *>(edge_feat)[e] = make_float4(d[0], d[1], d[2], len);
}

// one edge's term of gp: g_d + g_len d / |d| (the length term is 0 at a zero-length edge, as torch.norm's backward)
__device__ __forceinline__ void train_edge_term(const float4 ef, const float4 ge, float t[3]) {
    const bool has_length = ef.w > 0.f;
    const float k = has_length ? ge.w / ef.w : 0.f;
    t[0] = ge.x + (has_length ? k * ef.x : 0.f);
    t[1] = ge.y + (has_length ? k * ef.y : 0.f);
    t[2] = ge.z + (has_length ? k * ef.z : 0.f);
}

__global__ __launch_bounds__(TRAIN_SIM_THREADS) void k_train_update_bwd(int N, int64_t E, const float4 *__restrict__ edge_feat,
                                                                       const float4 *__restrict__ g_edge, const float *__restrict__ g_pos,
                                                                       const float *__restrict__ old_act, const float *__restrict__ act,
                                                                       const float *__restrict__ ostd, const int32_t *__restrict__ src_rowptr,
                                                                       const int32_t *__restrict__ src_perm, const int32_t *__restrict__ dst_rowptr,
                                                                       const int32_t *__restrict__ dst_perm, float *__restrict__ g_pred,
                                                                       float *__restrict__ g_init) {
    const int64_t n = (int64_t)blockIdx.x * TRAIN_SIM_THREADS + threadIdx.x;
    if (n >= N) return;
    float gp[3];
#pragma unroll
    for (int c = 0; c < 3; c++) gp[c] = g_pos ? g_pos[3 * n + c] : 0.f;
    if (g_edge) {
        // (row pointers and edge ids are clamped to the edge list: a broken CSR reads nothing outside edge_feat / g_edge)
        int64_t s = src_rowptr[n], end = src_rowptr[n + 1];
        s = s < 0 ? 0 : s; end = end > E ? E : end;
        for (int64_t i = s; i < end; i++) {          // edges with row == n: new_pos[n] enters d with +
            const int64_t id = src_perm[i];
            if ((uint64_t)id >= (uint64_t)E) continue;
            float t[3];
            train_edge_term(edge_feat[id], g_edge[id], t);
#pragma unroll
            for (int c = 0; c < 3; c++) gp[c] = gp[c] + t[c];
        }
        s = dst_rowptr[n]; end = dst_rowptr[n + 1];
        s = s < 0 ? 0 : s; end = end > E ? E : end;
        for (int64_t i = s; i < end; i++) {          // edges with col == n: new_pos[n] enters d with -
            const int64_t id = dst_perm[i];
            if ((uint64_t)id >= (uint64_t)E) continue;
            float t[3];
            train_edge_term(edge_feat[id], g_edge[id], t);
#pragma unroll
            for (int c = 0; c < 3; c++) gp[c] = gp[c] - t[c];
        }
    }
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const int64_t i = 3 * n + c;
        if (g_init) g_init[i] = gp[c];
        if (g_pred) {
            const bool free_node = act[i] == 0.f && old_act[i] == 0.f;
            g_pred[i] = free_node ? (ostd ? gp[c] * ostd[c] : gp[c]) : 0.f;
        }
    }
}

// do [a, a + na) and [b, b + nb) share a byte?  (a NULL or empty range shares none)
bool train_sim_overlap(const void *a, size_t na, const void *b, size_t nb) {
    if (!a || !b || na == 0 || nb == 0) return false;
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + nb && y < x + na;
}

struct Range {
    const void *p;
    size_t bytes;
};

// no output may share a byte with an input or with another output
bool train_sim_outputs_alias(const Range *out, int n_out, const Range *in, int n_in) {
    for (int i = 0; i < n_out; i++) {
        for (int j = 0; j < n_in; j++)
            if (train_sim_overlap(out[i].p, out[i].bytes, in[j].p, in[j].bytes)) return true;
        for (int j = i + 1; j < n_out; j++)
            if (train_sim_overlap(out[i].p, out[i].bytes, out[j].p, out[j].bytes)) return true;
    }
    return false;
}

}  // namespace

extern "C" int csplat_train_update_fwd(void *stream, int N, int64_t E, int H, const float *velocity, const float *velocity_noise,
                                       const float *pred_acc, const float *omean, const float *ostd, const float *init_position,
                                       const float *old_actions, const float *actions, const int64_t *edge_index, float *hist, float *edge_feat,
                                       float *new_pos) {
    CSPLAT_REQUIRE(N >= 0 && E >= 0, "csplat_train_update_fwd: bad N or E");
    CSPLAT_REQUIRE(H >= 1 && H <= 16, "csplat_train_update_fwd: H must lie in 1 .. 16");
    CSPLAT_REQUIRE((int64_t)N * 3 * H < ((int64_t)1 << 31) && E < ((int64_t)1 << 29), "csplat_train_update_fwd: N * 3H and 4E must stay below 2^31");
    CSPLAT_REQUIRE((omean == nullptr) == (ostd == nullptr), "csplat_train_update_fwd: omean and ostd are given together or not at all");
    const int64_t n_edge = edge_feat ? E : 0;
    if (N == 0 || (!hist && !new_pos && n_edge == 0)) return 0;
    CSPLAT_REQUIRE(velocity && pred_acc && init_position && old_actions && actions && (edge_index || n_edge == 0),
                   "csplat_train_update_fwd: NULL operand");
    CSPLAT_REQUIRE((((uintptr_t)velocity | (uintptr_t)velocity_noise | (uintptr_t)pred_acc | (uintptr_t)omean | (uintptr_t)ostd |
                     (uintptr_t)init_position | (uintptr_t)old_actions | (uintptr_t)actions | (uintptr_t)hist | (uintptr_t)new_pos) & 3u) == 0 &&
                       ((uintptr_t)edge_index & 7u) == 0 && ((uintptr_t)edge_feat & 15u) == 0,
                   "csplat_train_update_fwd: float operands must be 4-byte aligned, edge_index 8-byte, edge_feat 16-byte aligned");
    const size_t hb = (size_t)N * 3 * H * 4, nb = (size_t)N * 12;
    const Range out[3] = {{hist, hb}, {edge_feat, (size_t)n_edge * 16}, {new_pos, nb}};
    const Range in[9] = {{velocity, hb}, {velocity_noise, hb}, {pred_acc, nb}, {omean, 12}, {ostd, 12}, {init_position, nb}, {old_actions, nb},
                         {actions, nb}, {edge_index, n_edge ? (size_t)E * 16 : 0}};
    CSPLAT_REQUIRE(!train_sim_outputs_alias(out, 3, in, 9), "csplat_train_update_fwd: an output overlaps another operand");
    const TrainNodeIn node = {velocity, velocity_noise, pred_acc, omean, ostd, init_position, old_actions, actions, H};
    k_train_update_fwd<<<cdiv((int64_t)N + n_edge, TRAIN_SIM_THREADS), TRAIN_SIM_THREADS, 0, (hipStream_t)stream>>>(N, n_edge, E, node, edge_index, hist,
                                                                                                                 edge_feat, new_pos);
    LAUNCH_CHECK();
    return 0;
}

extern "C" int csplat_train_update_bwd(void *stream, int N, int64_t E, const float *edge_feat, const float *g_edge_feat, const float *g_new_pos,
                                       const float *old_actions, const float *actions, const float *ostd, const int32_t *src_rowptr,
                                       const int32_t *src_perm, const int32_t *dst_rowptr, const int32_t *dst_perm, float *g_pred_acc,
                                       float *g_init_position) {
    CSPLAT_REQUIRE(N >= 0 && E >= 0, "csplat_train_update_bwd: bad N or E");
    CSPLAT_REQUIRE((int64_t)N * 3 < ((int64_t)1 << 31) && E < ((int64_t)1 << 29), "csplat_train_update_bwd: 3N and 4E must stay below 2^31");
    if (N == 0 || (!g_pred_acc && !g_init_position)) return 0;
    const bool edges = g_edge_feat && E > 0;
    if (!edges) g_edge_feat = nullptr;
    CSPLAT_REQUIRE(!g_pred_acc || (old_actions && actions), "csplat_train_update_bwd: g_pred_acc needs old_actions and actions");
    CSPLAT_REQUIRE(!edges || (edge_feat && src_rowptr && src_perm && dst_rowptr && dst_perm), "csplat_train_update_bwd: NULL operand");
    CSPLAT_REQUIRE((((uintptr_t)g_new_pos | (uintptr_t)old_actions | (uintptr_t)actions | (uintptr_t)ostd | (uintptr_t)src_rowptr |
                     (uintptr_t)src_perm | (uintptr_t)dst_rowptr | (uintptr_t)dst_perm | (uintptr_t)g_pred_acc | (uintptr_t)g_init_position) & 3u) == 0 &&
                       (((uintptr_t)edge_feat | (uintptr_t)g_edge_feat) & 15u) == 0,
                   "csplat_train_update_bwd: operands must be 4-byte aligned, edge_feat and g_edge_feat 16-byte aligned");
    const size_t nb = (size_t)N * 12, eb = edges ? (size_t)E * 16 : 0, pb = edges ? (size_t)E * 4 : 0, rb = edges ? ((size_t)N + 1) * 4 : 0;
    const Range out[2] = {{g_pred_acc, nb}, {g_init_position, nb}};
    const Range in[10] = {{edge_feat, eb}, {g_edge_feat, eb}, {g_new_pos, nb}, {old_actions, g_pred_acc ? nb : 0}, {actions, g_pred_acc ? nb : 0},
                          {ostd, 12}, {src_rowptr, rb}, {src_perm, pb}, {dst_rowptr, rb}, {dst_perm, pb}};
    CSPLAT_REQUIRE(!train_sim_outputs_alias(out, 2, in, 10), "csplat_train_update_bwd: an output overlaps another operand");
    k_train_update_bwd<<<cdiv(N, TRAIN_SIM_THREADS), TRAIN_SIM_THREADS, 0, (hipStream_t)stream>>>(
        N, E, (const float4 *)edge_feat, (const float4 *)g_edge_feat, g_new_pos, old_actions, actions, ostd, src_rowptr, src_perm, dst_rowptr, dst_perm,
        g_pred_acc, g_init_position);
    LAUNCH_CHECK();
    return 0;
}
