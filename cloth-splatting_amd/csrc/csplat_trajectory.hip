// csplat_trajectory.hip -- trajectory features (gfx950, wave64; include/csplat.h "Trajectory preprocessing", csplat_traj_features,
// states the semantics).  The reference forms them on the host, frame by frame (meshnet/data_utils.py: process_traj :307-348 and
// compute_edge_features :443-448); here one launch covers every frame of a tracked cloud:
//   k_traj_features   one thread per node of a frame (its finite-difference velocity) or per edge of a frame (its displacement and
//                     length); the first T * N threads take the nodes, the next T * E the edges
// Plain loads and stores, every output element written by exactly one thread: bit-reproducible.  Float arithmetic without contraction,
// every operation one float32 rounding, so a numpy float32 restatement gives the same bits.  (csplat_traj_smooth, the smoothing that
// comes before this, lives in csplat_knn.hip beside the k-NN kernel it extends.)
// Algorithmic bytes per frame: 24 N read and 12 N written (velocity), 16 E + 24 E gathered and 16 E written (edges).
#include "csplat_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int TRAJ_THREADS = 256;

__global__ __launch_bounds__(TRAJ_THREADS) void k_traj_features(int T, int N, int64_t E, int64_t n_node, int64_t n_edge, const float *__restrict__ pos,
                                                                const int64_t *__restrict__ edge_index, float inv_dt, float *__restrict__ vel,
                                                                float *__restrict__ disp, float *__restrict__ norm) {
    const int64_t g = (int64_t)blockIdx.x * TRAJ_THREADS + threadIdx.x;
    if (g < n_node) {                            // node g = t N + i
        const bool first = g < N;
#pragma unroll
        for (int a = 0; a < 3; a++) vel[3 * g + a] = first ? 0.f : __fmul_rn(__fsub_rn(pos[3 * g + a], pos[3 * (g - N) + a]), inv_dt);
        return;
    }
    const int64_t h = g - n_node;                // edge h = t E + e
    if (h >= n_edge) return;
    const int64_t t = h / E, e = h - t * E;
    const int64_t s = edge_index[e], r = edge_index[E + e];
    float d[3];
    // an index outside 0 .. N-1 is the caller's error (the Python surface checks the range): its row is NaN and nothing outside pos is read
    const bool inside = (uint64_t)s < (uint64_t)N && (uint64_t)r < (uint64_t)N;
    const float *__restrict__ frame = pos + (size_t)t * N * 3;
#pragma unroll
    for (int a = 0; a < 3; a++) d[a] = inside ? __fsub_rn(frame[3 * r + a], frame[3 * s + a]) : __builtin_nanf("");
#pragma unroll
    for (int a = 0; a < 3; a++) disp[3 * h + a] = d[a];
    norm[h] = sqrtf(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
}

// do [a, a + na) and [b, b + nb) share a byte?  (a NULL or empty range shares none)
bool traj_feat_overlap(const void *a, size_t na, const void *b, size_t nb) {
    if (!a || !b || na == 0 || nb == 0) return false;
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + nb && y < x + na;
}

}  // namespace

extern "C" int csplat_traj_features(void *stream, int T, int N, int64_t E, const float *pos, const int64_t *edge_index, float inv_dt, float *vel,
                                    float *disp, float *norm) {
    CSPLAT_REQUIRE(T >= 0 && N >= 0 && E >= 0, "csplat_traj_features: bad T, N or E");
    CSPLAT_REQUIRE((int64_t)T * N < ((int64_t)1 << 31) && E < ((int64_t)1 << 31) && (int64_t)T * E < ((int64_t)1 << 31),
                   "csplat_traj_features: T * N and T * E must stay below 2^31");
    CSPLAT_REQUIRE(inv_dt == inv_dt && fabsf(inv_dt) < __builtin_inff(), "csplat_traj_features: inv_dt is a finite number");
    CSPLAT_REQUIRE((disp == nullptr) == (norm == nullptr), "csplat_traj_features: disp and norm are wanted together or not at all");
    // N = 0: no node an edge could name;  otherwise the node part runs when vel is wanted and the edge part when E > 0 and disp / norm are
    const int64_t n_node = vel ? (int64_t)T * N : 0, n_edge = disp ? (int64_t)T * E : 0;
    if (T == 0 || N == 0 || n_node + n_edge == 0) return 0;
    CSPLAT_REQUIRE(pos && (edge_index || n_edge == 0), "csplat_traj_features: NULL pos or edge_index");
    CSPLAT_REQUIRE((((uintptr_t)pos | (uintptr_t)vel | (uintptr_t)disp | (uintptr_t)norm) & 3u) == 0 && ((uintptr_t)edge_index & 7u) == 0,
                   "csplat_traj_features: float operands must be 4-byte aligned, edge_index 8-byte aligned");
    const size_t pb = (size_t)T * N * 12, eb = (size_t)n_edge * 12, nb = (size_t)n_edge * 4, ib = n_edge ? (size_t)E * 16 : 0, vb = (size_t)n_node * 12;
    CSPLAT_REQUIRE(!traj_feat_overlap(vel, vb, pos, pb) && !traj_feat_overlap(disp, eb, pos, pb) && !traj_feat_overlap(norm, nb, pos, pb) &&
                       !traj_feat_overlap(vel, vb, edge_index, ib) && !traj_feat_overlap(disp, eb, edge_index, ib) &&
                       !traj_feat_overlap(norm, nb, edge_index, ib) && !traj_feat_overlap(vel, vb, disp, eb) &&
                       !traj_feat_overlap(vel, vb, norm, nb) && !traj_feat_overlap(disp, eb, norm, nb),
                   "csplat_traj_features: an output overlaps another operand");
    hipStream_t s = (hipStream_t)stream;
    k_traj_features<<<cdiv(n_node + n_edge, TRAJ_THREADS), TRAJ_THREADS, 0, s>>>(T, N, E, n_node, n_edge, pos, edge_index, inv_dt, vel, disp, norm);
    LAUNCH_CHECK();
    return 0;
}
