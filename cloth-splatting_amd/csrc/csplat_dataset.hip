// csplat_dataset.hip -- the MeshNet sample data set on the device (gfx950, wave64; include/csplat.h "MeshNet sample data set" states the
// semantics).  The reference assembles every training sample on the host (meshnet/dataloader_sim.py: __getitem__ :148-182, _data_to_graph
// :352-412, then FaceToEdge / Cartesian / Distance and PyG's collate): about a dozen small operations per sample.  Here the trajectories
// live packed in device buffers and
//   k_dataset_batch          ONE launch writes a whole block-diagonal batch.  The grid is (work items, samples); a sample's work items are
//                            the FLOATS of its node outputs, one array after the other, then its edges -- so consecutive lanes write
//                            consecutive floats of the wide rows (velocity is 3 H floats wide, the targets 3 F) and read runs of 3 N
//                            consecutive floats of a stored frame.  An edge thread forms its two endpoint positions itself (the stored
//                            position, plus the action for the grasped node: the same rounded add the node thread does, the same bits)
//                            instead of waiting for the node threads, as k_train_update_fwd does
//   k_dataset_rollout_error  the per-step error of a validation rollout, one workgroup per step: each thread walks its elements in
//                            ascending order, the workgroup's 256 partial sums are joined by a fixed tree in LDS.  Step s re-adds the
//                            predictions 0 .. s (S^2 / 2 passes over an L2-resident array in all) instead of a second launch or a ticket
// Plain loads and stores, every output element written by exactly one thread, no atomics: bit-reproducible.  Float arithmetic without
// contraction, every operation one float32 rounding; the squared edge length is the one exception, spelled out as csplat_train_sim.hip
// spells it, so that the edge features are bit-equal to csplat_gnn_edge_features on the output positions.
// Algorithmic bytes per sample: (12 H + 4 + 12 + 24 F) N read, (12 H + 4 + 12 + 36 F) N written, 16 E + 24 E gathered (L2), 32 E written.
#include "csplat_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int DATASET_THREADS = 256;
constexpr int DATASET_TABLE_WORDS = CSPLAT_DATASET_TABLE_WORDS;      // int64 words per trajectory (include/csplat.h names them)
constexpr int DATASET_MAX_GRID_X = 16384;   // workgroups along the work items; the kernel strides over what is beyond

struct DatasetStore {
    const float *__restrict__ pos, *__restrict__ vel, *__restrict__ node_type, *__restrict__ actions;
    const int64_t *__restrict__ edges, *__restrict__ table;
    int64_t rows, steps, n_edges;      // what is stored: sum T N node rows, sum T frames, sum E edges
    int n_traj;
};

struct DatasetOut {
    float *__restrict__ velocity, *__restrict__ node_types, *__restrict__ positions, *__restrict__ target_vel, *__restrict__ pos_target,
        *__restrict__ particle_actions;
    int64_t *__restrict__ edge_index;
    float *__restrict__ edge_features;
    int64_t rows, n_edges;             // of the whole batch
};

__global__ __launch_bounds__(DATASET_THREADS) void k_dataset_batch(int B, int H, int F, DatasetStore st, const int32_t *__restrict__ desc,
                                                                  const float *__restrict__ action_override, DatasetOut out) {
    const float nan = __builtin_nanf("");
    for (int b = blockIdx.y; b < B; b += gridDim.y) {
        const int4 d = reinterpret_cast<const int4 *>(desc)[b];
        const int j = d.x;
        const int64_t t = d.y, r = d.z, e0 = d.w;
        if ((unsigned)j >= (unsigned)st.n_traj) continue;
        const int64_t *__restrict__ row = st.table + (int64_t)j * DATASET_TABLE_WORDS;
        const int64_t nb = row[CSPLAT_DATASET_NODE_BASE], ab = row[CSPLAT_DATASET_FRAME_BASE], eb = row[CSPLAT_DATASET_EDGE_BASE],
                      N = row[CSPLAT_DATASET_N], E = row[CSPLAT_DATASET_E], T = row[CSPLAT_DATASET_T], g = row[CSPLAT_DATASET_GRASPED];
        // a sample whose rows would leave the outputs, or whose trajectory leaves the store, writes and reads nothing (the Python surface
        // builds descriptors and table from its own records: this is a broken caller)
        if (N < 0 || E < 0 || T < 0 || r < 0 || e0 < 0 || r + N > out.rows || e0 + E > out.n_edges) continue;
        if (nb < 0 || ab < 0 || eb < 0 || N * T > st.rows - nb || T > st.steps - ab || E > st.n_edges - eb) continue;
        // a window that leaves its trajectory is the Python surface's error: every float of the sample is NaN and nothing is read
        const bool inside = t >= H && t + F <= T;
        const int W = 3 * H, G = 3 * F;
        const int64_t n_vel = N * W, n_pos = 3 * N, n_fut = N * G;
        const int64_t work = n_vel + N + n_pos + 3 * n_fut + E;
        const float *__restrict__ act = action_override ? action_override + (int64_t)b * G : st.actions + (inside ? (ab + t - 1) * 3 : 0);
        const int64_t now = nb + (t - 1) * N;          // the node row of frame t - 1's node 0
        for (int64_t w = (int64_t)blockIdx.x * DATASET_THREADS + threadIdx.x; w < work; w += (int64_t)gridDim.x * DATASET_THREADS) {
            int64_t k = w;
            if (k < n_vel) {                 // velocity[r + i][3 h + a] = vel[t - H + h][i][a]; the grasped row's last slot: vel[t][g]
                const int64_t i = k / W;
                const int c = (int)(k - i * W), h = c / 3, a = c - 3 * h;
                const int64_t frame = (i == g && h == H - 1) ? t : t - H + h;
                out.velocity[r * W + k] = inside ? st.vel[(nb + frame * N + i) * 3 + a] : nan;
                continue;
            }
            k -= n_vel;
            if (k < N) {
                out.node_types[r + k] = inside ? st.node_type[now + k] : nan;
                continue;
            }
            k -= N;
            if (k < n_pos) {                 // positions[r + i] = pos[t - 1][i], the grasped row moved by a[0]
                const int64_t i = k / 3;
                const int a = (int)(k - 3 * i);
                float p = nan;
                if (inside) {
                    p = st.pos[now * 3 + k];
                    if (i == g) p = p + act[a];
                }
                out.positions[r * 3 + k] = p;
                continue;
            }
            k -= n_pos;
            if (k < 2 * n_fut) {             // target_velocities / pos_target [r + i][f] = vel / pos [t + f][i]
                const bool velocity = k < n_fut;
                if (!velocity) k -= n_fut;
                const int64_t i = k / G;
                const int c = (int)(k - i * G), f = c / 3, a = c - 3 * f;
                const int64_t at = (nb + (t + f) * N + i) * 3 + a;
                (velocity ? out.target_vel : out.pos_target)[r * G + k] = inside ? (velocity ? st.vel[at] : st.pos[at]) : nan;
                continue;
            }
            k -= 2 * n_fut;
            if (k < n_fut) {                 // particle_actions[r + i][f] = 0, the grasped row a[f]
                const int64_t i = k / G;
                const int c = (int)(k - i * G);
                out.particle_actions[r * G + k] = inside ? (i == g ? act[c] : 0.f) : nan;
                continue;
            }
            k -= n_fut;                      // edge k
            const int64_t s = st.edges[2 * eb + k], q = st.edges[2 * eb + E + k];
            out.edge_index[e0 + k] = s + r;
            out.edge_index[out.n_edges + e0 + k] = q + r;
            // a node index outside 0 .. N-1 is the caller's error (the Python surface checks the range): its row is NaN and nothing is read
            const bool ok = inside && (uint64_t)s < (uint64_t)N && (uint64_t)q < (uint64_t)N;
            float dd[3];
#pragma unroll
            for (int a = 0; a < 3; a++) {
                float ps = nan, pq = nan;
                if (ok) {
                    ps = st.pos[(now + s) * 3 + a];
                    pq = st.pos[(now + q) * 3 + a];
                    if (s == g) ps = ps + act[a];
                    if (q == g) pq = pq + act[a];
                }
                dd[a] = ps - pq;
            }
            // (the squared length as csplat_gnn_edge_features' object code forms it)
            const float len = sqrtf(__fmaf_rn(dd[2], dd[2], __fmaf_rn(dd[0], dd[0], dd[1] * dd[1])));
            reinterpret_cast<float4 *>(out.edge_features)[e0 + k] = make_float4(dd[0], dd[1], dd[2], len);
        }
    }
}

__global__ __launch_bounds__(DATASET_THREADS) void k_dataset_rollout_error(int S, int64_t n, const float *__restrict__ pos0,
                                                                          const float *__restrict__ pred, const float *__restrict__ gt,
                                                                          float *__restrict__ err) {
    __shared__ float s_sum[DATASET_THREADS];
    const int tid = threadIdx.x;
    for (int s = blockIdx.x; s < S; s += gridDim.x) {
        float part = 0.f;
        for (int64_t i = tid; i < n; i += DATASET_THREADS) {
            float at = pos0[i];
            for (int k = 0; k <= s; k++) at = at + pred[(int64_t)k * n + i];
            const float d = at - gt[(int64_t)s * n + i];
            part = part + d * d;
        }
        s_sum[tid] = part;
        __syncthreads();
        for (int half = DATASET_THREADS / 2; half > 0; half >>= 1) {
            if (tid < half) s_sum[tid] = s_sum[tid] + s_sum[tid + half];
            __syncthreads();
        }
        if (tid == 0) err[s] = s_sum[0] / (float)n;
        __syncthreads();
    }
}

struct Range {
    const void *p;
    size_t bytes;
};

// do two ranges share a byte?  (a NULL or empty range shares none)
bool dataset_overlap(const Range &a, const Range &b) {
    if (!a.p || !b.p || a.bytes == 0 || b.bytes == 0) return false;
    const uintptr_t x = (uintptr_t)a.p, y = (uintptr_t)b.p;
    return x < y + b.bytes && y < x + a.bytes;
}

// no output may share a byte with an input or with another output
bool dataset_outputs_alias(const Range *out, int n_out, const Range *in, int n_in) {
    for (int i = 0; i < n_out; i++) {
        for (int j = 0; j < n_in; j++)
            if (dataset_overlap(out[i], in[j])) return true;
        for (int j = i + 1; j < n_out; j++)
            if (dataset_overlap(out[i], out[j])) return true;
    }
    return false;
}

}  // namespace

extern "C" int csplat_dataset_batch(void *stream, int B, int H, int F, int n_traj, int64_t store_rows, int64_t store_frames, int64_t store_edges,
                                    const float *pos, const float *velocity, const float *node_type, const float *actions, const int64_t *edges,
                                    const int64_t *table, const int32_t *desc, const float *action_override, int64_t n_rows, int64_t n_edges,
                                    int64_t max_items, float *out_velocity, float *out_node_types, float *out_positions,
                                    float *out_target_velocities, float *out_pos_target, float *out_particle_actions, int64_t *out_edge_index,
                                    float *out_edge_features) {
    CSPLAT_REQUIRE(B >= 0 && n_traj >= 0 && store_rows >= 0 && store_frames >= 0 && store_edges >= 0 && n_rows >= 0 && n_edges >= 0 && max_items >= 0,
                   "csplat_dataset_batch: a negative size");
    CSPLAT_REQUIRE(H >= 1 && H <= 16, "csplat_dataset_batch: H must lie in 1 .. 16");
    CSPLAT_REQUIRE(F >= 1 && F < (1 << 20), "csplat_dataset_batch: F must be >= 1 (and below 2^20)");
    const int64_t lim = (int64_t)1 << 31;
    CSPLAT_REQUIRE(n_rows < lim && n_rows * 3 * H < lim && n_rows * 3 * F < lim && n_edges < ((int64_t)1 << 29) && store_rows < lim &&
                       store_frames < lim && store_edges < lim && (int64_t)B * 3 * F < lim,
                   "csplat_dataset_batch: row counts (rows * 3H, rows * 3F, 4 * edges, stored rows, frames and edges, B * 3F) must stay below 2^31");
    if (B == 0 || (n_rows == 0 && n_edges == 0)) return 0;
    CSPLAT_REQUIRE(pos && velocity && node_type && actions && table && desc && (edges || n_edges == 0), "csplat_dataset_batch: NULL operand");
    CSPLAT_REQUIRE((n_rows == 0 || (out_velocity && out_node_types && out_positions && out_target_velocities && out_pos_target && out_particle_actions)) &&
                       (n_edges == 0 || (out_edge_index && out_edge_features)),
                   "csplat_dataset_batch: NULL output");
    CSPLAT_REQUIRE((((uintptr_t)pos | (uintptr_t)velocity | (uintptr_t)node_type | (uintptr_t)actions | (uintptr_t)action_override |
                     (uintptr_t)out_velocity | (uintptr_t)out_node_types | (uintptr_t)out_positions | (uintptr_t)out_target_velocities |
                     (uintptr_t)out_pos_target | (uintptr_t)out_particle_actions) & 3u) == 0 &&
                       (((uintptr_t)edges | (uintptr_t)table | (uintptr_t)out_edge_index) & 7u) == 0 &&
                       (((uintptr_t)desc | (uintptr_t)out_edge_features) & 15u) == 0,
                   "csplat_dataset_batch: float operands must be 4-byte aligned, edges, table and edge_index 8-byte, desc and edge_features 16-byte aligned");
    const size_t rows = (size_t)n_rows, ne = (size_t)n_edges;
    const Range out[8] = {{out_velocity, rows * 12 * H}, {out_node_types, rows * 4}, {out_positions, rows * 12}, {out_target_velocities, rows * 12 * F},
                          {out_pos_target, rows * 12 * F}, {out_particle_actions, rows * 12 * F}, {out_edge_index, ne * 16}, {out_edge_features, ne * 16}};
    const Range in[8] = {{pos, (size_t)store_rows * 12}, {velocity, (size_t)store_rows * 12}, {node_type, (size_t)store_rows * 4},
                         {actions, (size_t)store_frames * 12}, {edges, (size_t)store_edges * 16}, {table, (size_t)n_traj * DATASET_TABLE_WORDS * 8},
                         {desc, (size_t)B * 16}, {action_override, (size_t)B * 12 * F}};
    CSPLAT_REQUIRE(!dataset_outputs_alias(out, 8, in, 8), "csplat_dataset_batch: an output overlaps another operand");
    const DatasetStore st = {pos, velocity, node_type, actions, edges, table, store_rows, store_frames, store_edges, n_traj};
    const DatasetOut o = {out_velocity, out_node_types, out_positions, out_target_velocities, out_pos_target, out_particle_actions, out_edge_index,
                          out_edge_features, n_rows, n_edges};
    int64_t gx = (max_items + DATASET_THREADS - 1) / DATASET_THREADS;
    gx = gx < 1 ? 1 : (gx > DATASET_MAX_GRID_X ? DATASET_MAX_GRID_X : gx);
    const dim3 grid((unsigned)gx, (unsigned)(B < 65535 ? B : 65535));
    k_dataset_batch<<<grid, DATASET_THREADS, 0, (hipStream_t)stream>>>(B, H, F, st, desc, action_override, o);
    LAUNCH_CHECK();
    return 0;
}

extern "C" int csplat_dataset_rollout_error(void *stream, int S, int N, const float *pos0, const float *pred, const float *gt, float *err) {
    CSPLAT_REQUIRE(S >= 0 && N >= 0, "csplat_dataset_rollout_error: bad S or N");
    CSPLAT_REQUIRE((int64_t)S * N * 3 < ((int64_t)1 << 31), "csplat_dataset_rollout_error: S * N * 3 must stay below 2^31");
    if (S == 0) return 0;
    CSPLAT_REQUIRE(N >= 1, "csplat_dataset_rollout_error: the mean over no node is undefined");
    CSPLAT_REQUIRE(pos0 && pred && gt && err, "csplat_dataset_rollout_error: NULL operand");
    CSPLAT_REQUIRE((((uintptr_t)pos0 | (uintptr_t)pred | (uintptr_t)gt | (uintptr_t)err) & 3u) == 0,
                   "csplat_dataset_rollout_error: operands must be 4-byte aligned");
    const size_t nb = (size_t)N * 12;
    const Range out[1] = {{err, (size_t)S * 4}};
    const Range in[3] = {{pos0, nb}, {pred, nb * S}, {gt, nb * S}};
    CSPLAT_REQUIRE(!dataset_outputs_alias(out, 1, in, 3), "csplat_dataset_rollout_error: err overlaps another operand");
    k_dataset_rollout_error<<<S < 65535 ? S : 65535, DATASET_THREADS, 0, (hipStream_t)stream>>>(S, (int64_t)N * 3, pos0, pred, gt, err);
    LAUNCH_CHECK();
    return 0;
}
