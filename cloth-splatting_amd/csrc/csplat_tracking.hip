// csplat_tracking.hip -- point tracking, the evaluation end of the pipeline (gfx950, wave64; include/csplat.h, csplat_track_visibility and
// csplat_track_mte, states the semantics).  The reference does this on the host: `project` and `get_mask` per frame with a device -> host
// copy each (render.py:77-121), `align_traj` + `compute_mte` in a Python loop over the ground-truth tracks (scripts/align_eval_trajs.py).
//   k_track_visibility   one thread per (view-frame f = blockIdx.y, point i): pixel, in_image, the depth lookup, visible
//   k_track_counts       one workgroup per frame: counts[f] = the sums of the frame's in_image and visible bytes, 16 at a time.  (Two
//                        integer atomics per workgroup of k_track_visibility, the first form, all landed in the one cache line that holds
//                        counts: 88 us of a 97 us launch at 100 000 points x 12 frames; this launch replaced them)
//   k_track_mte          one thread per ground-truth track g: its associated point's trajectory aligned by the reference's rule, the
//                        per-frame errors and their mean over the frames, summed in increasing k
//   k_track_mean         one workgroup: the mean of mte[G] in a fixed order
// Every load is unconditional with its index clamped into the arrays; an invalid point is selected out, never branched around.  No float
// atomics, no atomics at all: every output is bit-reproducible.
// Algorithmic bytes: visibility, per (f, i): 12 (point) [+ 8 pixels_in] + 4 (depth tap) read, 8 (pixel) + 2 (bytes) written;
// mte, per (k, g): 12 (gt) + 12 (traj row) + 16 (quaternion) read, 12 (aligned) + 4 (err) written.
#include "csplat_common.h"
#include "csplat_device.h"

namespace {

constexpr int TK_THREADS = 256, TK_BATCH = 8, TK_COUNT_THREADS = 1024;

// 0 <= x < W, 0 <= y < H, both finite; `front` carries w > 0 when the pixel was projected here
__device__ __forceinline__ bool track_in_image(float x, float y, bool front, float W, float H) {
    return front && finite_f32(x) && finite_f32(y) && x >= 0.f && x < W && y >= 0.f && y < H;
}

// the depth tap of a pixel: C truncation, as the reference's astype(int).  A point that is not in the image reads pixel (0, 0); the
// clamp keeps the tap inside the image whatever the pixel holds (x < W in float32 already gives (int)x <= W - 1)
__device__ __forceinline__ int64_t track_tap(float x, float y, bool in, int W, int H) {
    int xi = in ? (int)x : 0, yi = in ? (int)y : 0;
    xi = xi < 0 ? 0 : (xi > W - 1 ? W - 1 : xi);
    yi = yi < 0 ? 0 : (yi > H - 1 ? H - 1 : yi);
    return (int64_t)yi * W + xi;
}

// the reference's `depth[depth < 1.0] = 10e3`, then `(dist - thr) <= depth`; a NaN on either side compares false
__device__ __forceinline__ bool track_depth_test(float dist, float thr, float d, float min_depth, float far_value) {
    const float dd = (min_depth > 0.f && d < min_depth) ? far_value : d;
    return (dist - thr) <= dd;
}

// grid (workgroups over N, F frames): f = blockIdx.y is uniform, so the frame's 16 + 3 matrix floats are scalar loads
template <bool PROJECT, bool HAS_DEPTH>
__global__ __launch_bounds__(TK_THREADS) void k_track_visibility(int64_t N, int W, int H, const float *__restrict__ points,
                                                                 const float *__restrict__ pixels_in, const float *__restrict__ full_proj,
                                                                 const float *__restrict__ cam_center, const float *__restrict__ depth,
                                                                 float thr, float min_depth, float far_value, float *__restrict__ pixels_out,
                                                                 uint8_t *__restrict__ in_image, uint8_t *__restrict__ visible) {
    const int f = blockIdx.y;
    const int64_t gi = (int64_t)blockIdx.x * TK_THREADS + threadIdx.x;
    const bool live = gi < N;
    const int64_t i = live ? gi : N - 1;
    const int64_t row = (int64_t)f * N + i;
    const float *__restrict__ full = full_proj + 16 * (int64_t)f;
    const float *__restrict__ cam = cam_center + 3 * (int64_t)f;
    const float Wf = (float)W, Hf = (float)H;

    // round 1: the point (and its given pixel)
    const float px = points[3 * row], py = points[3 * row + 1], pz = points[3 * row + 2];
    PixelProj p;
    if (PROJECT) {
        p = project_pixel(px, py, pz, full, Wf, Hf);
    } else {
        p.x = pixels_in[2 * row];
        p.y = pixels_in[2 * row + 1];
        p.w = 1.f;
    }
    const bool in = track_in_image(p.x, p.y, p.w > 0.f, Wf, Hf);

    // round 2: the depth tap
    bool vis = in;
    if (HAS_DEPTH) {
        const float d = depth[(int64_t)f * W * H + track_tap(p.x, p.y, in, W, H)];
        const float dx = px - cam[0], dy = py - cam[1], dz = pz - cam[2];
        const float dist = sqrtf(dx * dx + dy * dy + dz * dz);
        vis = in && track_depth_test(dist, thr, d, min_depth, far_value);
    }

    if (live) {
        if (pixels_out) {
            pixels_out[2 * row] = p.x;
            pixels_out[2 * row + 1] = p.y;
        }
        in_image[row] = in ? 1 : 0;
        visible[row] = vis ? 1 : 0;
    }
}

// the ones among n bytes that are 0 or 1, this thread's share: single bytes up to the first 16-byte boundary, 16 at a time, single bytes
__device__ __forceinline__ int track_count_ones(const uint8_t *__restrict__ p, int64_t n) {
    int c = 0;
    int64_t head = (int64_t)((16 - ((uintptr_t)p & 15)) & 15);
    head = head < n ? head : n;
    for (int64_t i = threadIdx.x; i < head; i += TK_COUNT_THREADS) c += p[i];
    const int64_t nv = (n - head) / 16;
    const uint4 *__restrict__ v = reinterpret_cast<const uint4 *>(p + head);
    for (int64_t i = threadIdx.x; i < nv; i += TK_COUNT_THREADS) {
        const uint4 w = v[i];
        c += __popc(w.x) + __popc(w.y) + __popc(w.z) + __popc(w.w);
    }
    for (int64_t i = head + 16 * nv + threadIdx.x; i < n; i += TK_COUNT_THREADS) c += p[i];
    return c;
}

// grid F, 1024 threads (a frame has one workgroup: the more loads it keeps in flight the better): counts[f] = (points in the image, points visible) of frame f -- integer sums, the same whatever the order
__global__ __launch_bounds__(TK_COUNT_THREADS) void k_track_counts(int64_t N, const uint8_t *__restrict__ in_image,
                                                             const uint8_t *__restrict__ visible, int *__restrict__ counts) {
    __shared__ int s_cnt[2][TK_COUNT_THREADS / 64];
    const int f = blockIdx.x;
    int ci = track_count_ones(in_image + (int64_t)f * N, N), cv = track_count_ones(visible + (int64_t)f * N, N);
    block_sum<TK_COUNT_THREADS>(s_cnt, ci, cv);
    if (threadIdx.x == 0) {
        counts[2 * f] = ci;
        counts[2 * f + 1] = cv;
    }
}

struct TrackRot { float m[9]; };

// build_rotation of scripts/align_eval_trajs.py:9-27: q = (r, x, y, z) / |q|.  A zero quaternion gives 0 / 0 = NaN, as there
__device__ __forceinline__ TrackRot track_rotation(float q0, float q1, float q2, float q3) {
    const float norm = sqrtf(q0 * q0 + q1 * q1 + q2 * q2 + q3 * q3);
    const float r = q0 / norm, x = q1 / norm, y = q2 / norm, z = q3 / norm;
    TrackRot R;
    R.m[0] = 1.f - 2.f * (y * y + z * z); R.m[1] = 2.f * (x * y - r * z);       R.m[2] = 2.f * (x * z + r * y);
    R.m[3] = 2.f * (x * y + r * z);       R.m[4] = 1.f - 2.f * (x * x + z * z); R.m[5] = 2.f * (y * z - r * x);
    R.m[6] = 2.f * (x * z - r * y);       R.m[7] = 2.f * (y * z + r * x);       R.m[8] = 1.f - 2.f * (x * x + y * y);
    return R;
}

// (R_k R_0^T) t: the relative rotation first, then the translation, in the reference's order
__device__ __forceinline__ void track_rel_apply(const TrackRot &Rk, const TrackRot &R0, float tx, float ty, float tz, float out[3]) {
#pragma unroll
    for (int a = 0; a < 3; a++) {
        float rel[3];
#pragma unroll
        for (int b = 0; b < 3; b++) rel[b] = Rk.m[3 * a] * R0.m[3 * b] + Rk.m[3 * a + 1] * R0.m[3 * b + 1] + Rk.m[3 * a + 2] * R0.m[3 * b + 2];
        out[a] = rel[0] * tx + rel[1] * ty + rel[2] * tz;
    }
}

template <bool ALIGN>
__global__ __launch_bounds__(TK_THREADS) void k_track_mte(int T, int64_t N, int64_t G, const float *__restrict__ traj,
                                                          const float *__restrict__ rotations, const float *__restrict__ gt,
                                                          const int *__restrict__ assoc, float *__restrict__ aligned,
                                                          float *__restrict__ err, float *__restrict__ mte) {
    const int64_t g = (int64_t)blockIdx.x * TK_THREADS + threadIdx.x;
    if (g >= G) return;
    int64_t j = assoc[g];
    j = j < 0 ? 0 : (j > N - 1 ? N - 1 : j);
    const float *__restrict__ p0 = traj + 3 * j, *__restrict__ g0 = gt + 3 * g;
    const float tx = ALIGN ? g0[0] - p0[0] : 0.f, ty = ALIGN ? g0[1] - p0[1] : 0.f, tz = ALIGN ? g0[2] - p0[2] : 0.f;
    TrackRot R0;
    if (ALIGN) {
        const float *__restrict__ q = rotations + 4 * j;
        R0 = track_rotation(q[0], q[1], q[2], q[3]);
    }
    // TK_BATCH frames at a time: all of a batch's loads are requested before the first one is used (a frame per round trip otherwise: the
    // thread walks T frames alone).  A frame past the end reads frame T-1 again -- in bounds -- and is selected out
    float sum = 0.f;
    for (int k0 = 0; k0 < T; k0 += TK_BATCH) {
        float P[TK_BATCH][3], Y[TK_BATCH][3], Q[TK_BATCH][4];
#pragma unroll
        for (int b = 0; b < TK_BATCH; b++) {
            const int kk = k0 + b < T ? k0 + b : T - 1;
            const float *__restrict__ p = traj + 3 * ((int64_t)kk * N + j), *__restrict__ y = gt + 3 * ((int64_t)kk * G + g);
            P[b][0] = p[0]; P[b][1] = p[1]; P[b][2] = p[2];
            Y[b][0] = y[0]; Y[b][1] = y[1]; Y[b][2] = y[2];
            if (ALIGN) {
                const float *__restrict__ q = rotations + 4 * ((int64_t)kk * N + j);
                Q[b][0] = q[0]; Q[b][1] = q[1]; Q[b][2] = q[2]; Q[b][3] = q[3];
            }
        }
#pragma unroll
        for (int b = 0; b < TK_BATCH; b++) {
            const int k = k0 + b;
            const bool live = k < T;
            float s[3] = {0.f, 0.f, 0.f};
            if (ALIGN) {
                const TrackRot Rk = track_rotation(Q[b][0], Q[b][1], Q[b][2], Q[b][3]);
                track_rel_apply(Rk, R0, tx, ty, tz, s);
                if (k == 0) { s[0] = tx; s[1] = ty; s[2] = tz; }          // frame 0 takes the translation itself
            }
            const float ax = P[b][0] + s[0], ay = P[b][1] + s[1], az = P[b][2] + s[2];
            const float ex = Y[b][0] - ax, ey = Y[b][1] - ay, ez = Y[b][2] - az;
            const float e = sqrtf(ex * ex + ey * ey + ez * ez);
            if (aligned && live) {
                float *o = aligned + 3 * ((int64_t)k * G + g);
                o[0] = ax; o[1] = ay; o[2] = az;
            }
            if (err && live) err[(int64_t)k * G + g] = e;
            sum = live ? sum + e : sum;                                   // in increasing k
        }
    }
    mte[g] = sum / (float)T;
}

// the second (one-workgroup) launch: a fixed tree over mte[G] in index order -- each thread walks its residue class
__global__ __launch_bounds__(TK_THREADS) void k_track_mean(int64_t G, const float *__restrict__ mte, float *__restrict__ mean) {
    __shared__ float s_sum[TK_THREADS / 64];
    float ts = 0.f;
    for (int64_t i = threadIdx.x; i < G; i += TK_THREADS) ts += mte[i];
    block_sum<TK_THREADS>(s_sum, ts);
    if (threadIdx.x == 0) mean[0] = ts / (float)G;
}

}  // namespace

extern "C" int csplat_track_visibility(void *stream, int F, int64_t N, int W, int H, const float *points, const float *pixels_in,
                                       const float *full_proj, const float *cam_center, const float *depth, float depth_threshold,
                                       float min_depth, float far_value, float *pixels_out, uint8_t *in_image, uint8_t *visible,
                                       int *counts) {
    CSPLAT_REQUIRE(F >= 1 && F <= 65535, "csplat_track_visibility: 1 <= F <= 65535");
    CSPLAT_REQUIRE(N >= 0 && N < ((int64_t)1 << 31), "csplat_track_visibility: 0 <= N < 2^31");
    CSPLAT_REQUIRE(W >= 1 && H >= 1 && (int64_t)W * H < ((int64_t)1 << 31), "csplat_track_visibility: W and H are >= 1, W * H < 2^31");
    CSPLAT_REQUIRE(depth_threshold == depth_threshold && far_value == far_value, "csplat_track_visibility: depth_threshold and far_value are numbers");
    hipStream_t s = (hipStream_t)stream;
    if (N == 0) {
        if (counts) HIP_TRY(hipMemsetAsync(counts, 0, (size_t)F * 2 * sizeof(int), s));
        return 0;
    }
    CSPLAT_REQUIRE(points && full_proj && cam_center && in_image && visible, "csplat_track_visibility: a NULL operand");
    CSPLAT_REQUIRE((((uintptr_t)points | (uintptr_t)pixels_in | (uintptr_t)full_proj | (uintptr_t)cam_center | (uintptr_t)depth |
                     (uintptr_t)pixels_out | (uintptr_t)counts) & 3u) == 0, "csplat_track_visibility: operands must be 4-byte aligned");
    const dim3 grid((unsigned)((N + TK_THREADS - 1) / TK_THREADS), (unsigned)F);
#define TK_LAUNCH(P_, D_)                                                                                                              \
    k_track_visibility<P_, D_><<<grid, TK_THREADS, 0, s>>>(N, W, H, points, pixels_in, full_proj, cam_center, depth, depth_threshold, \
                                                           min_depth, far_value, pixels_out, in_image, visible)
    if (pixels_in) {
        if (depth) TK_LAUNCH(false, true); else TK_LAUNCH(false, false);
    } else {
        if (depth) TK_LAUNCH(true, true); else TK_LAUNCH(true, false);
    }
#undef TK_LAUNCH
    LAUNCH_CHECK();
    if (counts) {
        k_track_counts<<<(unsigned)F, TK_COUNT_THREADS, 0, s>>>(N, in_image, visible, counts);
        LAUNCH_CHECK();
    }
    return 0;
}

extern "C" int csplat_track_mte(void *stream, int T, int64_t N, int64_t G, const float *traj, const float *rotations, const float *gt,
                                const int *assoc, float *aligned, float *err, float *mte, float *mean) {
    CSPLAT_REQUIRE(T >= 1, "csplat_track_mte: T is >= 1");
    CSPLAT_REQUIRE(N >= 0 && N < ((int64_t)1 << 31) && G >= 0 && G < ((int64_t)1 << 31), "csplat_track_mte: 0 <= N, G < 2^31");
    if (N == 0 || G == 0) return 0;
    CSPLAT_REQUIRE(traj && gt && assoc && mte && mean, "csplat_track_mte: a NULL operand");
    CSPLAT_REQUIRE((((uintptr_t)traj | (uintptr_t)rotations | (uintptr_t)gt | (uintptr_t)assoc | (uintptr_t)aligned | (uintptr_t)err |
                     (uintptr_t)mte | (uintptr_t)mean) & 3u) == 0, "csplat_track_mte: operands must be 4-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    const unsigned blocks = (unsigned)((G + TK_THREADS - 1) / TK_THREADS);
    if (rotations)
        k_track_mte<true><<<blocks, TK_THREADS, 0, s>>>(T, N, G, traj, rotations, gt, assoc, aligned, err, mte);
    else
        k_track_mte<false><<<blocks, TK_THREADS, 0, s>>>(T, N, G, traj, rotations, gt, assoc, aligned, err, mte);
    LAUNCH_CHECK();
    k_track_mean<<<1, TK_THREADS, 0, s>>>(G, mte, mean);
    LAUNCH_CHECK();
    return 0;
}
