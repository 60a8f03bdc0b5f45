// csplat_raster_k1.h -- part of csplat_raster.hip, included there once, behind csplat_raster_math.h.
// K1, the per-Gaussian forward: preprocess_body and the k_preprocess* kernels, K1View / K1Table of the batched form.
// Uses from csplat_raster_math.h: the constants, Geom, Cam, ProjJac, the projection / covariance / antialiasing helpers, tile_rect,
// stage_sh_rows.  Its macro S is defined and undefined inside preprocess_body.
#pragma once

namespace {

// ------------------------------------------------------------------------------------------- K1
// s_shrows: the workgroup's SH rows in LDS when STAGE (filled by the caller: once per workgroup, also when it serves
// several views).  AA (k_preprocess_aa / k_preprocess_views_aa): the stored opacity is o' = o h (aa_factor) -- conic_opacity.w, the pack
// record, cut2 and everything downstream see o'; the conic, radius and tile rectangle still come from the dilated cov2D.
// What a thread reads of its Gaussian from global memory: requested by k1_request at the top of every K1 kernel, in front of the SH staging
// loads, so that all of a wave's loads are in flight together -- one memory round trip.  (Read where they are used, means3D, then scales
// and rotations behind the near-plane test, then the opacity behind two more tests, each waited for the one before: four round trips.)
struct K1In {
    float p[3];     // means3D
    float sq[7];    // cov3D_precomp (0..5) when that pointer is set (uniform across the launch), else scales (0..2) and rotations (3..6)
    float op;       // opacities[i]
};
// i may lie past P (the last workgroup): such a thread requests the last Gaussian's values and preprocess_body leaves before using them.
__device__ __forceinline__ void k1_request(int P, const float *__restrict__ means3D, const float *__restrict__ opacities,
                                           const float *__restrict__ scales, const float *__restrict__ rotations,
                                           const float *__restrict__ cov3D_precomp, int i, K1In &in) {
    const int il = min(i, P - 1);
#pragma unroll
    for (int k = 0; k < 3; k++) in.p[k] = means3D[3 * il + k];
    if (cov3D_precomp) {
#pragma unroll
        for (int k = 0; k < 6; k++) in.sq[k] = cov3D_precomp[6 * il + k];
        in.sq[6] = 0.f;
    } else {
#pragma unroll
        for (int k = 0; k < 3; k++) in.sq[k] = scales[3 * il + k];
#pragma unroll
        for (int k = 0; k < 4; k++) in.sq[3 + k] = rotations[4 * il + k];
    }
    in.op = opacities[il];
}

// stage_sh_rows with all of the thread's loads requested before the first LDS write (its loop waits for each 16-byte load before it asks
// for the next: ROWS * 12 / NT dependent round trips in front of the barrier).  The batched K1 and K8 kernels stage through this one.
template <int NT, int ROWS>
__device__ __forceinline__ void stage_sh_rows_batched(const float *__restrict__ src, int rows, float *s_rows) {
    constexpr int N = (ROWS * 12 + NT - 1) / NT;
    const float4 *src4 = reinterpret_cast<const float4 *>(src);
    const int n = rows * 12;                    // (rows >= 1: a slot past n requests the last one again and writes nothing)
    float4 v[N];
#pragma unroll
    for (int k = 0; k < N; k++) v[k] = src4[min((int)threadIdx.x + k * NT, n - 1)];
#pragma unroll
    for (int k = 0; k < N; k++) {
        const int t = (int)threadIdx.x + k * NT;
        if (t < n) {
            const int row = t / 12, c = (t - row * 12) * 4;
            float *d = s_rows + row * SH_ROW + c;
            d[0] = v[k].x; d[1] = v[k].y; d[2] = v[k].z; d[3] = v[k].w;
        }
    }
}

// Measurement hook of the batched K1 and K8 (csplat_debug_stamps, tools/per_gaussian_stamps.py): thread 0 of a workgroup leaves s_memtime in
// its 8 words of the buffer once `dep` has arrived -- where a wave's life goes between its loads.  Only the *_stamps kernels carry a
// StampMark; every other kernel passes NoMark and compiles to what it was.
struct NoMark {
    __device__ __forceinline__ void operator()(int, float) const {}
};
struct StampMark {
    unsigned long long *at;
    __device__ __forceinline__ void operator()(int k, float dep) const {
        if (threadIdx.x == 0) {
            asm volatile("" ::"v"(dep) : "memory");
            at[k] = (unsigned long long)__builtin_amdgcn_s_memtime();
            asm volatile("" ::: "memory");
        }
    }
};

template <bool STAGE, bool AA = false, class MK = NoMark>
__device__ __forceinline__ void preprocess_body(int P, int D, int M, const K1In &in, const float *__restrict__ shs,
                                                const float *__restrict__ colors_precomp, float scale_mod, bool cov_precomp,
                                                const Cam &cam, const Geom &g, int32_t *__restrict__ radii, int nocull,
                                                const float *s_shrows, int i, int srow, const MK &mark = MK()) {
#pragma clang fp contract(off)
    if (i >= P) return;
    float depth = 0.f, px = 0.f, py = 0.f, cut = -1.f;
    float4 co = {0.f, 0.f, 0.f, 0.f};
    float rgb[3] = {0.f, 0.f, 0.f};
    float c6[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    uint32_t clampbits = 0, touched = 0;
    int rad = 0;

    const float p[3] = {in.p[0], in.p[1], in.p[2]};
    mark(2, p[2]);
    float pv[3];
    view_point(p, cam.view, pv);
    do {
        if (pv[2] <= NEAR_Z) break;
        const float *pr = cam.proj;
        const float hx = pr[0] * p[0] + pr[4] * p[1] + pr[8] * p[2] + pr[12];
        const float hy = pr[1] * p[0] + pr[5] * p[1] + pr[9] * p[2] + pr[13];
        const float hw = pr[3] * p[0] + pr[7] * p[1] + pr[11] * p[2] + pr[15];
        const float pw = 1.0f / (hw + 0.0000001f);
        const float ndcx = hx * pw, ndcy = hy * pw;
        if (cov_precomp) {
#pragma unroll
            for (int k = 0; k < 6; k++) c6[k] = in.sq[k];
        } else {
            const float s[3] = {in.sq[0], in.sq[1], in.sq[2]};
            const float q[4] = {in.sq[3], in.sq[4], in.sq[5], in.sq[6]};
            mark(3, q[3]);
            cov3d_from_scale_rot(s, scale_mod, q, c6);
        }
        ProjJac pj;
        proj_jacobian(pv, cam, pj);
        float a, b, c;
        float aa_h = 1.f;
        if constexpr (AA) {
            float a0, c0;
            cov2d_undilated(c6, pj, a0, b, c0);
            a = a0 + AA_DILATE; c = c0 + AA_DILATE;
            aa_h = aa_factor(a0, b, c0);
        } else {
            cov2d_from_cov3d(c6, pj, a, b, c);
        }
        const float det = a * c - b * b;
        if (det == 0.0f) break;
        const float det_inv = 1.f / det;
        const float mid = 0.5f * (a + c);
        const float sq = sqrtf(fmaxf(0.1f, mid * mid - det));
        const float lam1 = mid + sq, lam2 = mid - sq;
        const float my_radius = ceilf(3.f * sqrtf(fmaxf(lam1, lam2)));
        const float ix = ((ndcx + 1.0f) * (float)cam.W - 1.0f) * 0.5f;
        const float iy = ((ndcy + 1.0f) * (float)cam.H - 1.0f) * 0.5f;
        const int r = (int)my_radius;
        int minx, miny, maxx, maxy;
        tile_rect(ix, iy, r, cam, minx, miny, maxx, maxy);
        if ((maxx - minx) * (maxy - miny) == 0) break;

        if (colors_precomp) {
#pragma unroll
            for (int k = 0; k < 3; k++) rgb[k] = colors_precomp[3 * i + k];
        } else {
            const float *sh = STAGE ? (const float *)(s_shrows + srow * SH_ROW) : shs + (size_t)i * M * 3;
            const float d0 = p[0] - cam.campos[0], d1 = p[1] - cam.campos[1], d2 = p[2] - cam.campos[2];
            const float len = sqrtf(d0 * d0 + d1 * d1 + d2 * d2);
            const float x = d0 / len, y = d1 / len, z = d2 / len;
#pragma unroll
            for (int ch = 0; ch < 3; ch++) {
#define S(k) sh[(k) * 3 + ch]
                float res = SH_C0 * S(0);
                if (D > 0) {
                    res = res - SH_C1 * y * S(1) + SH_C1 * z * S(2) - SH_C1 * x * S(3);
                    if (D > 1) {
                        const float xx = x * x, yy = y * y, zz = z * z, xy = x * y, yz = y * z, xz = x * z;
                        res = res + SH_C2[0] * xy * S(4) + SH_C2[1] * yz * S(5) + SH_C2[2] * (2.f * zz - xx - yy) * S(6) +
                              SH_C2[3] * xz * S(7) + SH_C2[4] * (xx - yy) * S(8);
                        if (D > 2) {
                            res = res + SH_C3[0] * y * (3.f * xx - yy) * S(9) + SH_C3[1] * xy * z * S(10) +
                                  SH_C3[2] * y * (4.f * zz - xx - yy) * S(11) +
                                  SH_C3[3] * z * (2.f * zz - 3.f * xx - 3.f * yy) * S(12) +
                                  SH_C3[4] * x * (4.f * zz - xx - yy) * S(13) + SH_C3[5] * z * (xx - yy) * S(14) +
                                  SH_C3[6] * x * (xx - 3.f * yy) * S(15);
                        }
                    }
                }
#undef S
                res += 0.5f;
                if (res < 0.f) clampbits |= (1u << ch);
                rgb[ch] = fmaxf(res, 0.f);
            }
        }
        depth = pv[2];
        rad = r;
        px = ix; py = iy;
        float op = in.op;
        mark(4, op);
        if constexpr (AA) op = op * aa_h;
        co = make_float4(c * det_inv, -b * det_inv, a * det_inv, op);
        touched = (uint32_t)((maxy - miny) * (maxx - minx));
        // culling radius: alpha >= 1/255 needs d^2 <= 2*lambda_max*ln(255*opacity).  lam1 >= lambda_max (the max(0.1,.)
        // above only enlarges it); the margin covers the rounding of det (cancellation in a*c - b*b scales the stored
        // conic uniformly) and of the per-pixel power evaluation.
        const float cancel = 4e-7f * (a * c + b * b) / det;
        cut = cancel < 0.25f ? 2.f * lam1 * logf(255.f * op) * (1.0001f + 2.f * cancel) + 0.01f : 3.0e38f;
        if (nocull == 1) cut = 3.0e38f;
        if (nocull == 2) cut = cut * 4.f + 4.f;
    } while (0);

    g.depth[i] = depth;
    radii[i] = rad;
    g.xy[i] = make_float2(px, py);
    g.conic_opacity[i] = co;
#pragma unroll
    for (int k = 0; k < 3; k++) g.rgb[3 * i + k] = rgb[k];
#pragma unroll
    for (int k = 0; k < 6; k++) g.cov3D[6 * i + k] = c6[k];
    g.clamped[i] = clampbits;
    g.tiles_touched[i] = touched;
    g.cut2[i] = cut;
    g.pack[3 * (size_t)i] = make_float4(px, py, co.x, co.y);
    g.pack[3 * (size_t)i + 1] = make_float4(co.z, co.w, rgb[0], rgb[1]);
    g.pack[3 * (size_t)i + 2] = make_float4(rgb[2], depth, cut, 0.f);
    mark(5, 0.f);
}

template <bool STAGE>
__global__ __launch_bounds__(256) void k_preprocess(int P, int D, int M, const float *__restrict__ means3D,
                                                     const float *__restrict__ shs,
                                                     const float *__restrict__ colors_precomp,
                                                     const float *__restrict__ opacities,
                                                     const float *__restrict__ scales, float scale_mod,
                                                     const float *__restrict__ rotations,
                                                     const float *__restrict__ cov3D_precomp, Cam cam, Geom g,
                                                     int32_t *__restrict__ radii, int nocull) {
    __shared__ float s_shrows[STAGE ? 256 * SH_ROW : 1];
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    K1In in;
    k1_request(P, means3D, opacities, scales, rotations, cov3D_precomp, i, in);      // in front of the staging loads: one round trip
    if (STAGE) {
        const int base = blockIdx.x * 256;
        stage_sh_rows<256>(shs + (size_t)base * 48, min(256, P - base), s_shrows);
        __syncthreads();
    }
    preprocess_body<STAGE>(P, D, M, in, shs, colors_precomp, scale_mod, cov3D_precomp != nullptr, cam, g, radii, nocull, s_shrows, i,
                           (int)threadIdx.x);
}
// (the antialiased K1: k_preprocess with o' = o h; a kernel of its own so that k_preprocess is compiled exactly as before)
template <bool STAGE>
__global__ __launch_bounds__(256) void k_preprocess_aa(int P, int D, int M, const float *__restrict__ means3D,
                                                        const float *__restrict__ shs,
                                                        const float *__restrict__ colors_precomp,
                                                        const float *__restrict__ opacities,
                                                        const float *__restrict__ scales, float scale_mod,
                                                        const float *__restrict__ rotations,
                                                        const float *__restrict__ cov3D_precomp, Cam cam, Geom g,
                                                        int32_t *__restrict__ radii, int nocull) {
    __shared__ float s_shrows[STAGE ? 256 * SH_ROW : 1];
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    K1In in;
    k1_request(P, means3D, opacities, scales, rotations, cov3D_precomp, i, in);      // in front of the staging loads: one round trip
    if (STAGE) {
        const int base = blockIdx.x * 256;
        stage_sh_rows<256>(shs + (size_t)base * 48, min(256, P - base), s_shrows);
        __syncthreads();
    }
    preprocess_body<STAGE, true>(P, D, M, in, shs, colors_precomp, scale_mod, cov3D_precomp != nullptr, cam, g, radii, nocull, s_shrows, i,
                                 (int)threadIdx.x);
}

// The first phase of the forward (K1 + the three counting kernels) for ALL views of a step, one launch each (blockIdx.y =
// view): a 4-view step otherwise spends 16 launches (~10 us of host time each, the GPU idling in between) before its one
// host read.  Views share the Gaussians' view-independent inputs; means / rotations / cameras / outputs come per view.
struct K1View {
    const float *means3D, *rotations;
    Cam cam;
    Geom g;
    int32_t *radii;
    uint32_t *table, *info, *mailbox;
    int2 *ranges;
    uint32_t tag;
};
struct K1Table { int n; K1View v[RASTER_MAX_VIEWS]; };

// (the 192-byte SH row of a Gaussian is staged ONCE per workgroup and evaluated for every view's direction)
constexpr int K1V_G = 64;
// 64 Gaussians per workgroup, wave w takes the views w, w + 4, ...: the views of a Gaussian run side by side instead of one after the
// other in one thread (P / 256 = 391 workgroups of four dependent load -> project -> SH rounds each: 1.2 waves per SIMD, 25 us for
// the four views of the bench), the stores of a wave go to ONE view's arrays at consecutive indices
template <bool STAGE, bool AA, class MK>
__device__ __forceinline__ void preprocess_views(int P, int D, int M, const float *__restrict__ shs, const float *__restrict__ opacities,
                                                 const float *__restrict__ scales, float scale_mod, const K1Table &tab, int nocull,
                                                 float *s_shrows, const MK &mark) {
    mark(0, 0.f);
    const int base = blockIdx.x * K1V_G;
    const int lane = threadIdx.x & 63;
    if (tab.n <= 0) return;
    // (the wave's number through readfirstlane: known to be the same in all lanes, its views' table entries arrive by scalar loads)
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    // the wave's first view's loads in front of the staging loads (a wave without a view, V < 4, requests the last view's and drops them)
    K1In in;
    {
        const K1View &w0 = tab.v[min(wave, tab.n - 1)];
        k1_request(P, w0.means3D, opacities, scales, w0.rotations, nullptr, base + lane, in);
    }
    if (STAGE) {
        stage_sh_rows_batched<256, K1V_G>(shs + (size_t)base * 48, min(K1V_G, P - base), s_shrows);
        __syncthreads();
    }
    mark(1, 0.f);
    for (int vi = wave; vi < tab.n; vi += 4) {
        const K1View &w = tab.v[vi];
        preprocess_body<STAGE, AA>(P, D, M, in, shs, nullptr, scale_mod, false, w.cam, w.g, w.radii, nocull, s_shrows, base + lane, lane, mark);
        // (V > 4) the next view's means and rotations, one batch; scales and the opacity are the same in every view
        if (vi + 4 < tab.n) k1_request(P, tab.v[vi + 4].means3D, opacities, scales, tab.v[vi + 4].rotations, nullptr, base + lane, in);
    }
}
template <bool STAGE>
__global__ __launch_bounds__(256) void k_preprocess_views(int P, int D, int M, const float *__restrict__ shs,
                                                           const float *__restrict__ opacities,
                                                           const float *__restrict__ scales, float scale_mod, K1Table tab,
                                                           int nocull) {
    __shared__ float s_shrows[STAGE ? K1V_G * SH_ROW : 1];
    preprocess_views<STAGE, false>(P, D, M, shs, opacities, scales, scale_mod, tab, nocull, s_shrows, NoMark());
}
template <bool STAGE>
__global__ __launch_bounds__(256) void k_preprocess_views_aa(int P, int D, int M, const float *__restrict__ shs,
                                                              const float *__restrict__ opacities,
                                                              const float *__restrict__ scales, float scale_mod, K1Table tab,
                                                              int nocull) {
    __shared__ float s_shrows[STAGE ? K1V_G * SH_ROW : 1];
    preprocess_views<STAGE, true>(P, D, M, shs, opacities, scales, scale_mod, tab, nocull, s_shrows, NoMark());
}
// (k_preprocess_views<true> with stamps: words 0..5 of the workgroup's 8 = entry, behind the staging barrier, means3D arrived, scales and
//  rotations arrived, the opacity arrived, the last store issued -- the last four for view 0, and only where thread 0's Gaussian got there)
__global__ __launch_bounds__(256) void k_preprocess_views_stamps(int P, int D, int M, const float *__restrict__ shs,
                                                                  const float *__restrict__ opacities,
                                                                  const float *__restrict__ scales, float scale_mod, K1Table tab,
                                                                  int nocull, unsigned long long *stamp_buf) {
    __shared__ float s_shrows[K1V_G * SH_ROW];
    preprocess_views<true, false>(P, D, M, shs, opacities, scales, scale_mod, tab, nocull, s_shrows, StampMark{stamp_buf + (size_t)blockIdx.x * 8});
}

}  // namespace
