// csplat_flow_loss.hip -- optical-flow supervision of the Gaussians' motion between the frames of a training step (gfx950, wave64;
// include/csplat.h, csplat_flow_loss_fwd, states the semantics).  The reference carries flow images to its train step and stops at an
// unfinished `flow_loss` that prints (train.py:52-90); there is no counterpart kernel.
//   k_flow_loss_fwd      one thread per (frame t, Gaussian i): both pairs frame t takes part in -- as b of pair t-1, as a of pair t --
//                        through flow_cell() / flow_pair(), so that a pair is judged by the same code in both roles; writes the
//                        unit gradient dL_flow/dX_t[i] once (no atomics) and one (sum, count) partial per workgroup
//   k_flow_loss_finish   one workgroup sums the partials in index order: bit-reproducible, no float atomics
//   k_flow_loss_bwd      d_points = g weight lambda unit
// Algorithmic bytes per (t, i): <= 3 points (36) + 3 visibility words (12) + 16 flow taps + 2 mask taps (72) read, 12 written.
#include "csplat_common.h"
#include "csplat_device.h"

namespace {

constexpr int FL_THREADS = 256, FL_FRAMES = 16;

// frame t's slots; F / M of slot t belong to PAIR t (t -> t+1), so slot T-1 of them stays empty
struct FlowTable {
    const float *X[FL_FRAMES], *full[FL_FRAMES], *F[FL_FRAMES], *M[FL_FRAMES];
    const int *vis[FL_FRAMES];
};

// where pair's `a` end samples the flow image and the mask: the four taps of its cell (floor convention, the upper tap clamped to the
// image so that its weight is 0 at x = W-1) and the nearest pixel.  Outside the image (or not a number) every index is 0: the loads
// stay inside the image whatever the point holds, and flow_pair() selects the pair out
struct FlowCell { int64_t i00, i01, i10, i11, im; float fx, fy; bool inside; };
__device__ __forceinline__ FlowCell flow_cell(const PixelProj &a, int W, int H) {
    FlowCell c;
    c.inside = a.x >= 0.f && a.x <= (float)(W - 1) && a.y >= 0.f && a.y <= (float)(H - 1);
    const float xs = c.inside ? a.x : 0.f, ys = c.inside ? a.y : 0.f;
    const float xf = floorf(xs), yf = floorf(ys);
    int x0 = (int)xf, y0 = (int)yf;
    x0 = x0 < 0 ? 0 : (x0 > W - 1 ? W - 1 : x0);
    y0 = y0 < 0 ? 0 : (y0 > H - 1 ? H - 1 : y0);
    const int x1 = x0 + 1 < W ? x0 + 1 : W - 1, y1 = y0 + 1 < H ? y0 + 1 : H - 1;
    c.fx = xs - xf;
    c.fy = ys - yf;
    int xm = (int)floorf(xs + 0.5f), ym = (int)floorf(ys + 0.5f);
    xm = xm < 0 ? 0 : (xm > W - 1 ? W - 1 : xm);
    ym = ym < 0 ? 0 : (ym > H - 1 ? H - 1 : ym);
    c.i00 = (int64_t)y0 * W + x0; c.i01 = (int64_t)y0 * W + x1;
    c.i10 = (int64_t)y1 * W + x0; c.i11 = (int64_t)y1 * W + x1;
    c.im = (int64_t)ym * W + xm;
    return c;
}
struct FlowTaps { float u00, u01, u10, u11, v00, v01, v10, v11, m; };
template <bool HAS_M>
__device__ __forceinline__ FlowTaps flow_gather(const float *__restrict__ F, const float *__restrict__ M, const FlowCell &c, int64_t hw) {
    FlowTaps t;
    t.u00 = F[c.i00]; t.u01 = F[c.i01]; t.u10 = F[c.i10]; t.u11 = F[c.i11];
    t.v00 = F[hw + c.i00]; t.v01 = F[hw + c.i01]; t.v10 = F[hw + c.i10]; t.v11 = F[hw + c.i11];
    t.m = HAS_M ? M[c.im] : 1.f;
    return t;
}

// ONE pair (a -> b) from its two projections, visibilities, taps and mask weight.  SELECTION: an invalid pair returns value 0 and both
// gradients exactly 0, whatever its inputs hold.  ga = dL/dp_a = -(I + J_g)^T s, gb = dL/dp_b = s, s = m (sign r_x, sign r_y)
struct FlowPair { bool valid; float value, gax, gay, gbx, gby; };
__device__ __forceinline__ FlowPair flow_pair(const PixelProj &a, const PixelProj &b, int vis_a, int vis_b, const FlowCell &c, const FlowTaps &t,
                                              float max_error) {
    const float fx = c.fx, fy = c.fy, ex = 1.f - fx, ey = 1.f - fy;
    const float gu = ey * (ex * t.u00 + fx * t.u01) + fy * (ex * t.u10 + fx * t.u11);
    const float gv = ey * (ex * t.v00 + fx * t.v01) + fy * (ex * t.v10 + fx * t.v11);
    const float rx = (b.x - a.x) - gu, ry = (b.y - a.y) - gv;
    const float e = fabsf(rx) + fabsf(ry);
    bool ok = vis_a > 0 && vis_b > 0 && a.w > 0.f && b.w > 0.f;
    ok = ok && finite_f32(a.x) && finite_f32(a.y) && finite_f32(b.x) && finite_f32(b.y) && c.inside;
    ok = ok && finite_f32(t.u00) && finite_f32(t.u01) && finite_f32(t.u10) && finite_f32(t.u11);
    ok = ok && finite_f32(t.v00) && finite_f32(t.v01) && finite_f32(t.v10) && finite_f32(t.v11);
    ok = ok && finite_f32(t.m) && t.m > 0.f;
    ok = ok && !(max_error > 0.f && !(e <= max_error));
    const float sx = t.m * (float)((rx > 0.f) - (rx < 0.f)), sy = t.m * (float)((ry > 0.f) - (ry < 0.f));
    // J_g in the cell: d(gu, gv) / d(x, y)
    const float ux = ey * (t.u01 - t.u00) + fy * (t.u11 - t.u10), uy = ex * (t.u10 - t.u00) + fx * (t.u11 - t.u01);
    const float vx = ey * (t.v01 - t.v00) + fy * (t.v11 - t.v10), vy = ex * (t.v10 - t.v00) + fx * (t.v11 - t.v01);
    FlowPair p;
    p.valid = ok;
    p.value = ok ? t.m * e : 0.f;
    p.gbx = ok ? sx : 0.f;
    p.gby = ok ? sy : 0.f;
    p.gax = ok ? -(sx + ux * sx + vx * sy) : 0.f;
    p.gay = ok ? -(sy + uy * sx + vy * sy) : 0.f;
    return p;
}

// grid (workgroups over P, T frames): t = blockIdx.y is uniform, so the 16 matrix floats of a frame are scalar loads.  partial: n_parts
// floats (sum of m e) then n_parts ints (valid pairs), at blockIdx.y * gridDim.x + blockIdx.x.  unit [T][P][3] or NULL
template <bool HAS_M>
__global__ __launch_bounds__(FL_THREADS) void k_flow_loss_fwd(int T, int64_t P, int W, int H, FlowTable tab, float max_error, float inv_n,
                                                              int64_t n_parts, float *__restrict__ partial, float *__restrict__ unit) {
    __shared__ float s_sum[FL_THREADS / 64];
    __shared__ int s_cnt[FL_THREADS / 64];
    const int t = blockIdx.y;
    const bool has_a = t < T - 1, has_b = t > 0;          // the pair this frame opens / the pair it closes
    const int tp = has_b ? t - 1 : t, tn = has_a ? t + 1 : t;      // (an absent neighbour reads this frame again: in bounds, selected out)
    const int ta = has_a ? t : t - 1;                      // pair whose flow the a role samples (T >= 2: pair t-1 exists when pair t does not)
    const int64_t gi = (int64_t)blockIdx.x * FL_THREADS + threadIdx.x;
    const bool live = gi < P;
    const int64_t i = live ? gi : P - 1;
    const float Wf = (float)W, Hf = (float)H;
    const int64_t hw = (int64_t)W * H;

    // round 1: the three points and their visibilities
    const float *__restrict__ Xp = tab.X[tp], *__restrict__ Xc = tab.X[t], *__restrict__ Xn = tab.X[tn];
    const float px = Xp[3 * i], py = Xp[3 * i + 1], pz = Xp[3 * i + 2];
    const float cx = Xc[3 * i], cy = Xc[3 * i + 1], cz = Xc[3 * i + 2];
    const float nx = Xn[3 * i], ny = Xn[3 * i + 1], nz = Xn[3 * i + 2];
    const int *__restrict__ Vp = tab.vis[tp], *__restrict__ Vc = tab.vis[t], *__restrict__ Vn = tab.vis[tn];
    // (a NULL entry reads a word of its frame's points instead and drops it: a load inside a branch on the pointer waits for its own
    //  round trip, three of them in a row in the first form of this kernel)
    const int lp = (Vp ? Vp : reinterpret_cast<const int *>(Xp))[i], lc = (Vc ? Vc : reinterpret_cast<const int *>(Xc))[i],
              ln = (Vn ? Vn : reinterpret_cast<const int *>(Xn))[i];
    const int vp = Vp ? lp : 1, vc = Vc ? lc : 1, vn = Vn ? ln : 1;
    const PixelProj pp = project_pixel(px, py, pz, tab.full[tp], Wf, Hf);
    const PixelProj pc = project_pixel(cx, cy, cz, tab.full[t], Wf, Hf);
    const PixelProj pn = project_pixel(nx, ny, nz, tab.full[tn], Wf, Hf);

    // round 2: every tap of both pairs before the first one is used
    const FlowCell cell_a = flow_cell(pc, W, H), cell_b = flow_cell(pp, W, H);
    const FlowTaps taps_a = flow_gather<HAS_M>(tab.F[ta], tab.M[ta], cell_a, hw);
    const FlowTaps taps_b = flow_gather<HAS_M>(tab.F[tp], tab.M[tp], cell_b, hw);

    const FlowPair as_a = flow_pair(pc, pn, vc, vn, cell_a, taps_a, max_error);      // pair t:   this frame -> the next
    const FlowPair as_b = flow_pair(pp, pc, vp, vc, cell_b, taps_b, max_error);      // pair t-1: the previous -> this frame
    const bool on_a = has_a && live, on_b = has_b && live;

    if (unit && live) {
        const float gx = (on_a ? as_a.gax : 0.f) + (on_b ? as_b.gbx : 0.f);
        const float gy = (on_a ? as_a.gay : 0.f) + (on_b ? as_b.gby : 0.f);
        const bool any = (on_a && as_a.valid) || (on_b && as_b.valid);
        // dx/dX_k = (W/2) (full[k][0] - ndc_x full[k][3]) / w, likewise y.  A frame whose pairs are both invalid gets exactly 0: its w and
        // ndc may hold anything
        const float *__restrict__ fc = tab.full[t];
        const float kx = 0.5f * Wf * gx, ky = 0.5f * Hf * gy;
        float *o = unit + ((int64_t)t * P + i) * 3;
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const float d = (kx * (fc[4 * k] - pc.ndx * fc[4 * k + 3]) + ky * (fc[4 * k + 1] - pc.ndy * fc[4 * k + 3])) / pc.w;
            o[k] = any ? d * inv_n : 0.f;
        }
    }

    float acc = on_a ? as_a.value : 0.f;
    int cnt = (on_a && as_a.valid) ? 1 : 0;
    wave_sum_each(acc, cnt);
    block_stash(s_sum, acc, s_cnt, cnt);
    __syncthreads();
    if (threadIdx.x == 0) {
        const float ts = block_join<FL_THREADS>(s_sum, 0.f, OpSum{});
        const int tc = block_join<FL_THREADS>(s_cnt, 0, OpSum{});
        const int64_t at = (int64_t)blockIdx.y * gridDim.x + blockIdx.x;
        partial[at] = ts;
        reinterpret_cast<int *>(partial + n_parts)[at] = tc;
    }
}

// the second (one-workgroup) launch: a fixed tree over the partials in index order -- any number of them, each thread walks its residue
// class -- then out[2] = {weight lambda L_flow + add_weight add[0], L_flow}, count[0] = valid pairs
__global__ __launch_bounds__(FL_THREADS) void k_flow_loss_finish(int64_t n_parts, const float *__restrict__ partial, float n_pairs, float scale,
                                                                 const float *__restrict__ add, float add_weight, float *__restrict__ out,
                                                                 int *__restrict__ count) {
    __shared__ float s_sum[FL_THREADS / 64];
    __shared__ int s_cnt[FL_THREADS / 64];
    const int *__restrict__ counts = reinterpret_cast<const int *>(partial + n_parts);
    float ts = 0.f;
    int tc = 0;
    for (int64_t i = threadIdx.x; i < n_parts; i += FL_THREADS) { ts += partial[i]; tc += counts[i]; }
    wave_sum_each(ts, tc);
    block_stash(s_sum, ts, s_cnt, tc);
    __syncthreads();
    if (threadIdx.x == 0) {
        const float ss = block_join<FL_THREADS>(s_sum, 0.f, OpSum{});
        const int sc = block_join<FL_THREADS>(s_cnt, 0, OpSum{});
        const float l = ss / n_pairs;
        out[0] = scale * l + (add ? add_weight * add[0] : 0.f);
        out[1] = l;
        count[0] = sc;
    }
}

// backward, one launch: d_points[j] = g[0] scale unit[j] over the T P 3 floats; a unit of 0 (no valid pair) stays exactly 0 whatever g holds
__global__ __launch_bounds__(FL_THREADS) void k_flow_loss_bwd(int64_t n, const float *__restrict__ unit, const float *__restrict__ g, float scale,
                                                              float *__restrict__ d_points) {
    const int64_t j = (int64_t)blockIdx.x * FL_THREADS + threadIdx.x;
    if (j >= n) return;
    const float u = unit[j];
    d_points[j] = u != 0.f ? g[0] * scale * u : 0.f;
}

int64_t flow_blocks(int64_t P) { return (P + FL_THREADS - 1) / FL_THREADS; }

}  // namespace

extern "C" size_t csplat_flow_loss_scratch_bytes(int n_frames, int64_t P) {
    const int64_t T = n_frames > 1 ? n_frames : 1, blocks = flow_blocks(P > 0 ? P : 1);
    return align256((size_t)T * (size_t)blocks * 8);          // a float and an int per workgroup
}

extern "C" int csplat_flow_loss_fwd(void *stream, int n_frames, int64_t P, int W, int H, const float *const *points,
                                    const float *const *full_proj, const float *const *flow, const int *const *visible,
                                    const float *const *mask, float max_error, float lambda, float weight, const float *add, float add_weight,
                                    float *unit, void *scratch, float *out, int *count) {
    CSPLAT_REQUIRE(n_frames >= 2 && n_frames <= FL_FRAMES, "csplat_flow_loss_fwd: 2 <= n_frames <= 16");
    CSPLAT_REQUIRE(P >= 1 && W >= 1 && H >= 1, "csplat_flow_loss_fwd: P, W and H are >= 1");
    CSPLAT_REQUIRE(lambda >= 0.f, "csplat_flow_loss_fwd: lambda is >= 0");
    CSPLAT_REQUIRE(max_error == max_error, "csplat_flow_loss_fwd: max_error is a number (<= 0: no cap)");
    CSPLAT_REQUIRE(points && full_proj && flow && scratch && out && count, "csplat_flow_loss_fwd: a NULL table or output");
    CSPLAT_REQUIRE((int64_t)(n_frames - 1) * P < ((int64_t)1 << 31), "csplat_flow_loss_fwd: (n_frames - 1) * P must stay below 2^31");
    FlowTable tab;
    memset(&tab, 0, sizeof(tab));
    uintptr_t bits = (uintptr_t)add | (uintptr_t)unit | (uintptr_t)scratch | (uintptr_t)out | (uintptr_t)count;
    for (int t = 0; t < n_frames; t++) {
        CSPLAT_REQUIRE(points[t] && full_proj[t], "csplat_flow_loss_fwd: a NULL entry in `points` or `full_proj`");
        tab.X[t] = points[t];
        tab.full[t] = full_proj[t];
        tab.vis[t] = visible ? visible[t] : nullptr;          // (an entry may be NULL: visible)
        bits |= (uintptr_t)tab.X[t] | (uintptr_t)tab.full[t] | (uintptr_t)tab.vis[t];
        if (t < n_frames - 1) {
            CSPLAT_REQUIRE(flow[t] && (!mask || mask[t]), "csplat_flow_loss_fwd: a NULL entry in `flow` or in a `mask` table that is given");
            tab.F[t] = flow[t];
            tab.M[t] = mask ? mask[t] : nullptr;
            bits |= (uintptr_t)tab.F[t] | (uintptr_t)tab.M[t];
        }
    }
    CSPLAT_REQUIRE((bits & 3u) == 0, "csplat_flow_loss_fwd: operands must be 4-byte aligned");
    const int64_t gx = flow_blocks(P), n_parts = gx * n_frames;
    const float n_pairs = (float)((int64_t)(n_frames - 1) * P);
    const dim3 grid((unsigned)gx, (unsigned)n_frames);
    float *partial = (float *)scratch;
    if (mask)
        k_flow_loss_fwd<true><<<grid, FL_THREADS, 0, (hipStream_t)stream>>>(n_frames, P, W, H, tab, max_error, 1.0f / n_pairs, n_parts, partial, unit);
    else
        k_flow_loss_fwd<false><<<grid, FL_THREADS, 0, (hipStream_t)stream>>>(n_frames, P, W, H, tab, max_error, 1.0f / n_pairs, n_parts, partial, unit);
    LAUNCH_CHECK();
    k_flow_loss_finish<<<1, FL_THREADS, 0, (hipStream_t)stream>>>(n_parts, partial, n_pairs, weight * lambda, add, add_weight, out, count);
    LAUNCH_CHECK();
    return 0;
}

extern "C" int csplat_flow_loss_bwd(void *stream, int n_frames, int64_t P, const float *unit, float lambda, float weight,
                                    const float *g_scalar, float *d_points) {
    CSPLAT_REQUIRE(n_frames >= 2 && n_frames <= FL_FRAMES, "csplat_flow_loss_bwd: 2 <= n_frames <= 16");
    CSPLAT_REQUIRE(P >= 1 && lambda >= 0.f, "csplat_flow_loss_bwd: P is >= 1 and lambda is >= 0");
    CSPLAT_REQUIRE(unit && g_scalar && d_points, "csplat_flow_loss_bwd: a NULL operand");
    CSPLAT_REQUIRE((int64_t)(n_frames - 1) * P < ((int64_t)1 << 31), "csplat_flow_loss_bwd: (n_frames - 1) * P must stay below 2^31");
    CSPLAT_REQUIRE((((uintptr_t)unit | (uintptr_t)g_scalar | (uintptr_t)d_points) & 3u) == 0, "csplat_flow_loss_bwd: operands must be 4-byte aligned");
    const int64_t n = (int64_t)n_frames * P * 3;
    k_flow_loss_bwd<<<(unsigned)((n + FL_THREADS - 1) / FL_THREADS), FL_THREADS, 0, (hipStream_t)stream>>>(n, unit, g_scalar, weight * lambda, d_points);
    LAUNCH_CHECK();
    return 0;
}
