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
template <bool STAGE, bool AA = false>
__device__ __forceinline__ void preprocess_body(int P, int D, int M, const float *__restrict__ means3D,
                                                const float *__restrict__ shs,
                                                const float *__restrict__ colors_precomp,
                                                const float *__restrict__ opacities,
                                                const float *__restrict__ scales, float scale_mod,
                                                const float *__restrict__ rotations,
                                                const float *__restrict__ cov3D_precomp, const Cam &cam, const Geom &g,
                                                int32_t *__restrict__ radii, int nocull, const float *s_shrows, int i, int srow) {
#pragma clang fp contract(off)
    if (i >= P) return;
    float depth = 0.f, px = 0.f, py = 0.f, cut = -1.f;
    float4 co = {0.f, 0.f, 0.f, 0.f};
    float rgb[3] = {0.f, 0.f, 0.f};
    float c6[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    uint32_t clampbits = 0, touched = 0;
    int rad = 0;

    const float p[3] = {means3D[3 * i], means3D[3 * i + 1], means3D[3 * i + 2]};
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
        if (cov3D_precomp) {
#pragma unroll
            for (int k = 0; k < 6; k++) c6[k] = cov3D_precomp[6 * i + k];
        } else {
            const float s[3] = {scales[3 * i], scales[3 * i + 1], scales[3 * i + 2]};
            const float q[4] = {rotations[4 * i], rotations[4 * i + 1], rotations[4 * i + 2], rotations[4 * i + 3]};
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
        float op = opacities[i];
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
    if (STAGE) {
        const int base = blockIdx.x * 256;
        stage_sh_rows<256>(shs + (size_t)base * 48, min(256, P - base), s_shrows);
        __syncthreads();
    }
    preprocess_body<STAGE>(P, D, M, means3D, shs, colors_precomp, opacities, scales, scale_mod, rotations, cov3D_precomp, cam, g, radii,
                           nocull, s_shrows, (int)(blockIdx.x * blockDim.x + threadIdx.x), (int)threadIdx.x);
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
    if (STAGE) {
        const int base = blockIdx.x * 256;
        stage_sh_rows<256>(shs + (size_t)base * 48, min(256, P - base), s_shrows);
        __syncthreads();
    }
    preprocess_body<STAGE, true>(P, D, M, means3D, shs, colors_precomp, opacities, scales, scale_mod, rotations, cov3D_precomp, cam, g,
                                 radii, nocull, s_shrows, (int)(blockIdx.x * blockDim.x + threadIdx.x), (int)threadIdx.x);
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
template <bool STAGE>
__global__ __launch_bounds__(256) void k_preprocess_views(int P, int D, int M, const float *__restrict__ shs,
                                                           const float *__restrict__ opacities,
                                                           const float *__restrict__ scales, float scale_mod, K1Table tab,
                                                           int nocull) {
    // 64 Gaussians per workgroup, wave w takes the views w, w + 4, ...: the views of a Gaussian run side by side instead of one after the
    // other in one thread (P / 256 = 391 workgroups of four dependent load -> project -> SH rounds each: 1.2 waves per SIMD, 25 us for
    // the four views of the bench), the stores of a wave go to ONE view's arrays at consecutive indices
    __shared__ float s_shrows[STAGE ? K1V_G * SH_ROW : 1];
    const int base = blockIdx.x * K1V_G;
    if (STAGE) {
        stage_sh_rows<256>(shs + (size_t)base * 48, min(K1V_G, P - base), s_shrows);
        __syncthreads();
    }
    const int lane = threadIdx.x & 63;
    for (int vi = threadIdx.x >> 6; vi < tab.n; vi += 4) {
        const K1View &w = tab.v[vi];
        preprocess_body<STAGE>(P, D, M, w.means3D, shs, nullptr, opacities, scales, scale_mod, w.rotations, nullptr, w.cam, w.g, w.radii, nocull,
                               s_shrows, base + lane, lane);
    }
}
template <bool STAGE>
__global__ __launch_bounds__(256) void k_preprocess_views_aa(int P, int D, int M, const float *__restrict__ shs,
                                                              const float *__restrict__ opacities,
                                                              const float *__restrict__ scales, float scale_mod, K1Table tab,
                                                              int nocull) {
    __shared__ float s_shrows[STAGE ? K1V_G * SH_ROW : 1];
    const int base = blockIdx.x * K1V_G;
    if (STAGE) {
        stage_sh_rows<256>(shs + (size_t)base * 48, min(K1V_G, P - base), s_shrows);
        __syncthreads();
    }
    const int lane = threadIdx.x & 63;
    for (int vi = threadIdx.x >> 6; vi < tab.n; vi += 4) {
        const K1View &w = tab.v[vi];
        preprocess_body<STAGE, true>(P, D, M, w.means3D, shs, nullptr, opacities, scales, scale_mod, w.rotations, nullptr, w.cam, w.g, w.radii,
                                     nocull, s_shrows, base + lane, lane);
    }
}

}  // namespace
