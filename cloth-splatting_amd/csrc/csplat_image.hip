// csplat_image.hip -- image-space losses: the separable 11-tap Gaussian window (csplat_blur11), the fused L1 loss
// (csplat_l1) and the fused SSIM (csplat_ssim_fwd / _bwd).  The window: SSIM loss (utils/loss_utils.py:30-58: five grouped
// 11x11 conv2d per SSIM evaluation; the window is the outer product of a 1-D Gaussian with itself).  "Next" row N2 of
// sits right after the rasterizer in every train step.  One kernel does both passes through an LDS tile:
// HBM-bound, 4 B read + 4 B written per pixel (the grouped-conv path measured 1.2-1.8 ms per call on 5x3x3x800x800;
// this is a 46 MB round trip).  The window is symmetric and the padding is zero, so the operator is self-adjoint: the
// backward of blur is the same kernel applied to the incoming gradient.
// Sums: the L1, the image loss and the geometry loss leave one partial per workgroup, added in index order by a second, one-workgroup
// launch (no ticket, no float atomics); the standalone SSIM hands its partials to the caller.  Only k_psnr still has a ticket.
#include "csplat_common.h"
#include "csplat_device.h"
#include <math.h>
#include <stdlib.h>

namespace {
// ---- the tile the blur, the SSIM and the image loss share: IL_T threads per 64 x 16 tile of one plane (blockIdx.z).  il_load puts N maps
// with their 5-pixel halo into LDS; a thread then owns a STRIP: il_hrow makes 4 consecutive outputs of a halo row from 14 loaded values,
// il_vcol 2 consecutive rows of a column from 12 -- the sums of one output per thread and pass, tap order k = 0 .. 10, at half the
// instructions (round 5: 80.2 / 54.9 us at [3,3,800,800] -> 76.1 / 48.1 us; 256 threads with 8 x 1 / 1 x 4 strips were slower than either).
constexpr int BW = 64, BH = 16, R5 = 5;
struct Taps { float w[11]; };
constexpr int IL_T = 512, IL_HR = BH + 2 * R5, IL_XP = BW + 2 * R5 + 2, IL_HP = BW + 4;      // 26 halo rows; pitches 76 / 68 floats
constexpr int IL_HS = 4, IL_VS = 2;            // outputs per horizontal / vertical strip: 26 x 16 = 416 and 64 x 8 = 512 strips for 512 threads
constexpr int IL_NS = BW / IL_HS, IL_NV = IL_HS + 10;      // strips per halo row; values a horizontal strip loads per map
static_assert(IL_NS * IL_HR <= IL_T && BW * (BH / IL_VS) == IL_T, "one strip per thread");
static_assert(BW == 64 && BH == 16, "the strip assignment below is written for 64 x 16 tiles");

// the tile at (x0, y0) of plane `img` of N maps with its halo, zero outside the image; ends with the barrier
template <int N, class... Src>
__device__ __forceinline__ void il_load(int H, int W, size_t img, int x0, int y0, float (&dst)[N][IL_HR][IL_XP], const Src *__restrict__... src) {
    static_assert(sizeof...(Src) == N, "one source per map");
    for (int t = threadIdx.x; t < IL_HR * (BW + 2 * R5); t += IL_T) {
        const int ry = t / (BW + 2 * R5), rx = t - ry * (BW + 2 * R5);
        const int y = y0 + ry - R5, x = x0 + rx - R5;
        const bool in = y >= 0 && y < H && x >= 0 && x < W;
        const size_t o = img + (size_t)y * W + x;
        int q = 0;
        ((dst[q++][ry][rx] = in ? src[o] : 0.f), ...);
    }
    __syncthreads();
}
// horizontal 11-tap pass of one row strip: out[o] = sum_k w[k] v[o + k], o = 0 .. IL_HS - 1
__device__ __forceinline__ void il_hrow(const Taps &taps, const float (&v)[IL_NV], float *dst) {
    float a[IL_HS];
#pragma unroll
    for (int o = 0; o < IL_HS; o++) {
        float t = 0.f;
#pragma unroll
        for (int k = 0; k < 11; k++) t += taps.w[k] * v[o + k];
        a[o] = t;
    }
    static_assert(IL_HS == 4, "one 16-byte store per strip");
    reinterpret_cast<float4 *>(dst)[0] = make_float4(a[0], a[1], a[2], a[3]);
}
// the same for a map as it was loaded: the strip's IL_NV values from LDS, its IL_HS sums back
__device__ __forceinline__ void il_hmap(const Taps &taps, const float *src, float *dst) {
    float v[IL_NV];
#pragma unroll
    for (int k = 0; k < IL_NV; k++) v[k] = src[k];
    il_hrow(taps, v, dst);
}
// vertical 11-tap pass of one column strip: out[r] = sum_k w[k] s[(row0 + r + k) * IL_HP], r = 0 .. IL_VS - 1
__device__ __forceinline__ void il_vcol(const Taps &taps, const float *s, float (&out)[IL_VS]) {
    float v[IL_VS + 10];
#pragma unroll
    for (int j = 0; j < IL_VS + 10; j++) v[j] = s[j * IL_HP];
#pragma unroll
    for (int r = 0; r < IL_VS; r++) {
        float t = 0.f;
#pragma unroll
        for (int k = 0; k < 11; k++) t += taps.w[k] * v[r + k];
        out[r] = t;
    }
}
// the mask plane of image plane blockIdx.z: one per image (mask_channels == 1) or one per channel
__device__ __forceinline__ size_t il_mask_plane(const float *mask, int mask_channels, int channels) {
    return mask ? (mask_channels == 1 ? blockIdx.z / channels : blockIdx.z) : 0;
}

__global__ __launch_bounds__(IL_T) void k_blur11(int H, int W, Taps taps, const float *__restrict__ in, float *__restrict__ out) {
    __shared__ __attribute__((aligned(16))) float s_in[1][IL_HR][IL_XP];
    __shared__ __attribute__((aligned(16))) float s_h[1][IL_HR][IL_HP];
    const size_t img = (size_t)blockIdx.z * H * W;
    const int x0 = blockIdx.x * BW, y0 = blockIdx.y * BH;
    il_load(H, W, img, x0, y0, s_in, in);
    if (threadIdx.x < IL_HR * IL_NS) {
        const int ry = threadIdx.x / IL_NS, c0 = (threadIdx.x % IL_NS) * IL_HS;
        il_hmap(taps, &s_in[0][ry][c0], &s_h[0][ry][c0]);
    }
    __syncthreads();
    const int rx = threadIdx.x & 63, r0 = (threadIdx.x >> 6) * IL_VS, x = x0 + rx;
    float a[IL_VS];
    il_vcol(taps, &s_h[0][r0][rx], a);
#pragma unroll
    for (int r = 0; r < IL_VS; r++) {
        const int y = y0 + r0 + r;
        if (y < H && x < W) out[img + (size_t)y * W + x] = a[r];
    }
}

// ---- fused SSIM (utils/loss_utils.py:40-70, size_average form) and the WHOLE image loss of a train step (train_utils.py:50-74 + the PSNR
// the reference logs every step, :262-283): Ll1 + lambda (1 - SSIM) [masked: mean|(x - y) m| + lambda mean((1 - S) m)].  ONE tile body each
// way, instantiated twice.  Forward: loads an x / y tile with its halo, runs the five separable 11x11 windows (x^2, y^2, xy formed once
// per loaded value), evaluates the SSIM map, its three partial derivatives (w.r.t. mu1 = blur(x), s11 = blur(x^2), s12 = blur(xy)) and the
// workgroup's sum of the map.  Backward: blurs the three partials (the window is self-adjoint) and combines g (b1 + 2x b2 + y b3).  The
// composed form is a cat, a blur launch and ~25 elementwise launches forward, ~50 backward, each a full-image HBM round trip.
//   L1 = false (k_ssim_fwd / k_ssim_bwd, the standalone SSIM): one partial sum per workgroup, the optional map, the optional addend.
//   L1 = true  (k_image_loss_fwd / _bwd, what every train step runs): the tile already holds x and y, so the L1 term, the sign byte of
//              its gradient and the squared error of the PSNR ride on the last phase; three partial sums per workgroup, summed in index
//              order by k_image_loss_finish: bit-reproducible, no float atomics.
// What these kernels wait for is a tile's LIFE (load, barrier, pass, barrier, pass, stores) with three tiles resident per CU (51 KB of LDS
// each): at 84 VGPRs (5 waves per SIMD: two tiles per CU) the forward took 92.6 us against 76.1 -- hence __launch_bounds__(IL_T, 6).
constexpr float SSIM_C1 = 0.01f * 0.01f, SSIM_C2 = 0.03f * 0.03f;

// partial [L1 ? 3 : 1][workgroups]: sum S (masked: sum (1 - S) m), then sum |(x - y) m| and sum (x - y)^2
template <bool L1>
__device__ __forceinline__ void ssim_tile_fwd(int H, int W, const Taps &taps, const float *__restrict__ X, const float *__restrict__ Y,
                                              float *__restrict__ P1, float *__restrict__ P2, float *__restrict__ P3,
                                              signed char *__restrict__ sign8, float *__restrict__ map_out, const float *__restrict__ mask,
                                              int mask_channels, int channels, float *__restrict__ partial) {
    constexpr int NQ = L1 ? 3 : 1;
    __shared__ __attribute__((aligned(16))) float s_x[IL_HR][IL_XP];
    __shared__ __attribute__((aligned(16))) float s_y[IL_HR][IL_XP];
    __shared__ __attribute__((aligned(16))) float s_h[5][IL_HR][IL_HP];
    __shared__ float s_red[NQ][IL_T / 64];
    const size_t img = (size_t)blockIdx.z * H * W;
    const int x0 = blockIdx.x * BW, y0 = blockIdx.y * BH;
    // (this body's own halo loop, not il_load: with the one index il_load forms for all its maps the compiler arranges the address
    //  arithmetic of the two loads differently -- three instructions fewer, but not the listing every train step has run since round 5)
    for (int t = threadIdx.x; t < IL_HR * (BW + 2 * R5); t += IL_T) {
        const int ry = t / (BW + 2 * R5), rx = t - ry * (BW + 2 * R5);
        const int y = y0 + ry - R5, x = x0 + rx - R5;
        const bool in = y >= 0 && y < H && x >= 0 && x < W;       // zero padding (of the images AND of their products)
        s_x[ry][rx] = in ? X[img + (size_t)y * W + x] : 0.f;
        s_y[ry][rx] = in ? Y[img + (size_t)y * W + x] : 0.f;
    }
    __syncthreads();
    if (threadIdx.x < IL_HR * IL_NS) {                    // strip = (halo row, IL_HS columns)
        const int ry = threadIdx.x / IL_NS, c0 = (threadIdx.x % IL_NS) * IL_HS;
        float xv[IL_NV], yv[IL_NV], v[IL_NV];
#pragma unroll
        for (int k = 0; k < IL_NV; k++) { xv[k] = s_x[ry][c0 + k]; yv[k] = s_y[ry][c0 + k]; }
        il_hrow(taps, xv, &s_h[0][ry][c0]);
        il_hrow(taps, yv, &s_h[1][ry][c0]);
#pragma unroll
        for (int k = 0; k < IL_NV; k++) v[k] = xv[k] * xv[k];
        il_hrow(taps, v, &s_h[2][ry][c0]);
#pragma unroll
        for (int k = 0; k < IL_NV; k++) v[k] = yv[k] * yv[k];
        il_hrow(taps, v, &s_h[3][ry][c0]);
#pragma unroll
        for (int k = 0; k < IL_NV; k++) v[k] = xv[k] * yv[k];
        il_hrow(taps, v, &s_h[4][ry][c0]);
    }
    __syncthreads();
    float acc_s = 0.f, acc_l = 0.f, acc_q = 0.f;
    {                                                   // strip = (column, IL_VS rows)
        const int rx = threadIdx.x & 63, r0 = (threadIdx.x >> 6) * IL_VS;
        float m1[IL_VS], m2[IL_VS], q11[IL_VS], q22[IL_VS], q12[IL_VS];
        il_vcol(taps, &s_h[0][r0][rx], m1);
        il_vcol(taps, &s_h[1][r0][rx], m2);
        il_vcol(taps, &s_h[2][r0][rx], q11);
        il_vcol(taps, &s_h[3][r0][rx], q22);
        il_vcol(taps, &s_h[4][r0][rx], q12);
        const int x = x0 + rx;
        const size_t plane = il_mask_plane(mask, mask_channels, channels);
#pragma unroll
        for (int r = 0; r < IL_VS; r++) {
            const int y = y0 + r0 + r;
            if (y < H && x < W) {
                const float mu1 = m1[r], mu2 = m2[r], s11 = q11[r], s22 = q22[r], s12 = q12[r];
                const float mu1_sq = mu1 * mu1, mu2_sq = mu2 * mu2, mu12 = mu1 * mu2;
                const float A1 = 2.f * mu12 + SSIM_C1, A2 = 2.f * (s12 - mu12) + SSIM_C2;
                const float B1 = mu1_sq + mu2_sq + SSIM_C1, B2 = (s11 - mu1_sq) + (s22 - mu2_sq) + SSIM_C2;
                const float inv = 1.f / (B1 * B2);
                const float S = A1 * A2 * inv;
                const size_t o = img + (size_t)y * W + x;
                if constexpr (!L1) { if (map_out) map_out[o] = S; }
                // masked form (train_utils.py:64-67): the reduced quantity is sum((1 - S) * m) and the partials carry the weight m
                float m = 1.f;
                if (mask) {
                    m = mask[(plane * H + y) * W + x];
                    acc_s += (1.f - S) * m;
                } else acc_s += S;
                if constexpr (L1) {
                    const float d0 = s_x[r0 + r + R5][rx + R5] - s_y[r0 + r + R5][rx + R5];
                    const float d = d0 * m;                               // (utils/loss_utils.py:21-22: |(x - y) m|; the PSNR is unmasked)
                    acc_l += fabsf(d);
                    acc_q += d0 * d0;
                    if (sign8) sign8[o] = (signed char)(d > 0.f ? 1 : (d < 0.f ? -1 : 0));
                }
                if (P1) {
                    P1[o] = m * (2.f * mu2 * (A2 - A1) * inv - S * 2.f * mu1 * (B2 - B1) * inv);   // dS/dmu1
                    P2[o] = m * (-S / B2);                                                         // dS/ds11
                    P3[o] = m * (2.f * A1 * inv);                                                  // dS/ds12
                }
            }
        }
    }
    if constexpr (L1) wave_sum_each(acc_s, acc_l, acc_q); else wave_sum_each(acc_s);
    if constexpr (L1) block_stash(s_red[0], acc_s, s_red[1], acc_l, s_red[2], acc_q); else block_stash(s_red[0], acc_s);
    __syncthreads();
    if (threadIdx.x == 0) {
        const size_t nwg = (size_t)gridDim.y * gridDim.x * gridDim.z;
        const size_t me = ((size_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
        for (int q = 0; q < NQ; q++) partial[q * nwg + me] = block_join<IL_T>(s_red[q], 0.f, OpSum{});
    }
}

// dX = gscalar[0] g_ssim (b1 + 2 x b2 + y b3), plus gscalar[0] g_l1 sign m (L1) or add_scale[0] addend (the standalone SSIM, optional)
template <bool L1>
__device__ __forceinline__ void ssim_tile_bwd(int H, int W, const Taps &taps, const float *__restrict__ X, const float *__restrict__ Y,
                                              const float *__restrict__ P1, const float *__restrict__ P2, const float *__restrict__ P3,
                                              const signed char *__restrict__ sign8, const float *__restrict__ mask, int mask_channels,
                                              int channels, const float *__restrict__ gscalar, float g_l1, float g_ssim,
                                              const float *__restrict__ addend, const float *__restrict__ add_scale, float *__restrict__ dX) {
    __shared__ __attribute__((aligned(16))) float s_p[3][IL_HR][IL_XP];
    __shared__ __attribute__((aligned(16))) float s_h[3][IL_HR][IL_HP];
    const size_t img = (size_t)blockIdx.z * H * W;
    const int x0 = blockIdx.x * BW, y0 = blockIdx.y * BH;
    il_load(H, W, img, x0, y0, s_p, P1, P2, P3);
    if (threadIdx.x < IL_HR * IL_NS) {
        const int ry = threadIdx.x / IL_NS, c0 = (threadIdx.x % IL_NS) * IL_HS;
#pragma unroll
        for (int q = 0; q < 3; q++) il_hmap(taps, &s_p[q][ry][c0], &s_h[q][ry][c0]);
    }
    __syncthreads();
    const float gs = gscalar[0] * g_ssim, gl = L1 ? gscalar[0] * g_l1 : 0.f;
    const float ga = !L1 && addend ? add_scale[0] : 0.f;
    const int rx = threadIdx.x & 63, r0 = (threadIdx.x >> 6) * IL_VS;
    float b1[IL_VS], b2[IL_VS], b3[IL_VS];
    il_vcol(taps, &s_h[0][r0][rx], b1);
    il_vcol(taps, &s_h[1][r0][rx], b2);
    il_vcol(taps, &s_h[2][r0][rx], b3);
    const int x = x0 + rx;
    const size_t plane = il_mask_plane(mask, mask_channels, channels);
#pragma unroll
    for (int r = 0; r < IL_VS; r++) {
        const int y = y0 + r0 + r;
        if (y < H && x < W) {
            const size_t o = img + (size_t)y * W + x;
            if constexpr (L1) {
                const float m = mask ? mask[(plane * H + y) * W + x] : 1.f;
                dX[o] = gs * (b1[r] + 2.f * X[o] * b2[r] + Y[o] * b3[r]) + gl * (float)sign8[o] * m;
            } else {
                const float d = gs * (b1[r] + 2.f * X[o] * b2[r] + Y[o] * b3[r]);
                dX[o] = addend ? d + ga * addend[o] : d;
            }
        }
    }
}

__global__ __launch_bounds__(IL_T, 6) void k_ssim_fwd(int H, int W, Taps taps, const float *__restrict__ X, const float *__restrict__ Y,
                                                     float *__restrict__ P1, float *__restrict__ P2, float *__restrict__ P3,
                                                     float *__restrict__ map_out, float *__restrict__ partial,
                                                     const float *__restrict__ mask, int mask_channels, int channels) {
    ssim_tile_fwd<false>(H, W, taps, X, Y, P1, P2, P3, nullptr, map_out, mask, mask_channels, channels, partial);
}
__global__ __launch_bounds__(IL_T, 6) void k_ssim_bwd(int H, int W, Taps taps, const float *__restrict__ X, const float *__restrict__ Y,
                                                     const float *__restrict__ P1, const float *__restrict__ P2,
                                                     const float *__restrict__ P3, const float *__restrict__ gscalar, float inv_n,
                                                     const float *__restrict__ addend, const float *__restrict__ add_scale,
                                                     float *__restrict__ dX) {
    ssim_tile_bwd<false>(H, W, taps, X, Y, P1, P2, P3, nullptr, nullptr, 1, 1, gscalar, 0.f, inv_n, addend, add_scale, dX);
}
__global__ __launch_bounds__(IL_T, 6) void k_image_loss_fwd(int H, int W, Taps taps, const float *__restrict__ X, const float *__restrict__ Y,
                                                           float *__restrict__ P1, float *__restrict__ P2, float *__restrict__ P3,
                                                           signed char *__restrict__ sign8, const float *__restrict__ mask, int mask_channels,
                                                           int channels, float *__restrict__ partial) {
    ssim_tile_fwd<true>(H, W, taps, X, Y, P1, P2, P3, sign8, nullptr, mask, mask_channels, channels, partial);
}
__global__ __launch_bounds__(IL_T, 6) void k_image_loss_bwd(int H, int W, Taps taps, const float *__restrict__ X, const float *__restrict__ Y,
                                                           const float *__restrict__ P1, const float *__restrict__ P2,
                                                           const float *__restrict__ P3, const signed char *__restrict__ sign8,
                                                           const float *__restrict__ mask, int mask_channels, int channels,
                                                           const float *__restrict__ gscalar, float g_l1, float g_ssim, float *__restrict__ dX) {
    ssim_tile_bwd<true>(H, W, taps, X, Y, P1, P2, P3, sign8, mask, mask_channels, channels, gscalar, g_l1, g_ssim, nullptr, nullptr, dX);
}

// the second (one-workgroup) launch of the image loss: sums the workgroup partials in index order.  NOT a ticket in the kernel above:
// a device-scope release on gfx950 writes the XCD's dirty L2 lines back, and ~6000 workgroups each fencing while all of them stream the
// three partial-derivative images out cost 4x the kernel itself (measured 268-351 us against 75 + 4 for the two launches).
__global__ __launch_bounds__(IL_T) void k_image_loss_finish(size_t per_plane, int planes, int channels, int H, int W, int masked, float lam,
                                                            float img_weight, const float *__restrict__ add, float add_weight,
                                                            float psnr_scale, const float *__restrict__ partial, float *__restrict__ out) {
    __shared__ float s_red[IL_T / 64];
    const size_t nwg = per_plane * planes;
    // (ONE workgroup pulls ~135 KB of partials: 16-byte loads, four of them in flight per thread -- with 4-byte loads in a dependent
    //  `t += p[i]` loop the five sums of a 3-camera step took 12.8 us)
    auto range_sum = [&](const float *p, size_t lo, size_t hi) -> float {     // fixed-order sum of p[lo, hi)
        float t = 0.f;
        size_t a0 = lo + (((16u - (unsigned)((uintptr_t)(p + lo) & 15u)) & 15u) >> 2);      // first 16-byte-aligned element of p[lo ..
        if (a0 > hi) a0 = hi;
        const size_t n4 = (hi - a0) >> 2;
        const float4 *p4 = reinterpret_cast<const float4 *>(p + a0);
        size_t i = threadIdx.x;
        for (; i + 3 * IL_T < n4; i += 4 * IL_T) {
            const float4 u0 = p4[i], u1 = p4[i + IL_T], u2 = p4[i + 2 * IL_T], u3 = p4[i + 3 * IL_T];
            t += ((u0.x + u0.y) + (u0.z + u0.w)) + ((u1.x + u1.y) + (u1.z + u1.w));
            t += ((u2.x + u2.y) + (u2.z + u2.w)) + ((u3.x + u3.y) + (u3.z + u3.w));
        }
        for (; i < n4; i += IL_T) { const float4 u = p4[i]; t += (u.x + u.y) + (u.z + u.w); }
        for (size_t j = lo + threadIdx.x; j < a0; j += IL_T) t += p[j];                    // <= 3 elements in front ...
        for (size_t j = a0 + (n4 << 2) + threadIdx.x; j < hi; j += IL_T) t += p[j];        // ... and behind the float4 body
        __syncthreads();                                      // (s_red still holds the call before this one)
        block_sum<IL_T, true>(s_red, t);
        return t;
    };
    const float ssim_sum = range_sum(partial, 0, nwg);
    const float l1_sum = range_sum(partial + nwg, 0, nwg);
    const int n_batch = planes / channels;
    double psnr_sum = 0.0;         // (a float sum of 21 845 images' PSNR, added one by one, is off by 1e-6 of its value)
    for (int b = 0; b < n_batch; b++) {
        const float q = range_sum(partial + 2 * nwg, (size_t)b * channels * per_plane, (size_t)(b + 1) * channels * per_plane);
        const float mse = q / ((float)channels * (float)H * (float)W);
        psnr_sum += (double)(20.f * log10f(1.f / sqrtf(mse)));
    }
    if (threadIdx.x == 0) {
        const float n = (float)planes * (float)H * (float)W;
        const float l1 = l1_sum / n;
        const float image_loss = masked ? l1 + lam * (ssim_sum / n) : l1 + lam * (1.f - ssim_sum / n);
        out[0] = img_weight * image_loss + (add ? add_weight * add[0] : 0.f);
        out[1] = psnr_scale * (float)psnr_sum;
        out[2] = image_loss;
        out[3] = l1;
    }
}

// ---- fused L1 loss: mean |a - b| and its gradient sign(a - b) / n in ONE pass (utils/loss_utils.py:20-23 is three
// elementwise launches forward and three backward).  Deterministic: one partial per workgroup, summed in index order by
// k_l1_finish, a second one-workgroup launch -- no ticket, no float atomics.
constexpr int L1_BLOCKS = 256, L1_THREADS = 1024;  // one fat workgroup per CU; their partials are summed by k_l1_finish
__global__ __launch_bounds__(L1_THREADS) void k_l1(int64_t n, const float *__restrict__ a, const float *__restrict__ b,
                                                    float inv_n, float *__restrict__ partial, float *__restrict__ grad,
                                                    const float *__restrict__ mask, int64_t hw, int channels, int mask_channels,
                                                    signed char *__restrict__ sign8) {
    __shared__ float s_red[L1_THREADS / 64];
    float acc = 0.f;
    auto sg = [&](float d) { return d > 0.f ? inv_n : (d < 0.f ? -inv_n : 0.f); };
    auto s8 = [&](float d) { return (signed char)(d > 0.f ? 1 : (d < 0.f ? -1 : 0)); };   // the backward's input when the caller asks for 1 byte per element
    // masked form (utils/loss_utils.py:21-22): mean |(a - b) * m|, m one plane per image (mask_channels == 1) or per channel
    auto moff = [&](int64_t e) {
        const int64_t plane = e / hw;
        return (mask_channels == 1 ? plane / channels : plane) * hw + (e - plane * hw);
    };
    // 16-byte groups need a 4-pixel group inside one image plane AND 16-byte-aligned operands (a contiguous view into a batch whose plane
    // size is not a multiple of 4 floats starts anywhere); otherwise every element takes the scalar form below, as in k_psnr / adam_span
    const bool al = ((((uintptr_t)a | (uintptr_t)b | (uintptr_t)grad | (uintptr_t)mask) & 15u) == 0);
    const int64_t n4 = ((mask && (hw & 3)) || !al) ? 0 : n >> 2;
    auto one = [&](int64_t i, const float4 x, const float4 y) {
        float d0 = x.x - y.x, d1 = x.y - y.y, d2 = x.z - y.z, d3 = x.w - y.w;
        if (mask) {
            const float4 m = *reinterpret_cast<const float4 *>(mask + moff(i << 2));
            d0 *= m.x; d1 *= m.y; d2 *= m.z; d3 *= m.w;
            acc += (fabsf(d0) + fabsf(d1)) + (fabsf(d2) + fabsf(d3));
            if (grad) reinterpret_cast<float4 *>(grad)[i] = make_float4(sg(d0) * m.x, sg(d1) * m.y, sg(d2) * m.z, sg(d3) * m.w);
        } else {
            acc += (fabsf(d0) + fabsf(d1)) + (fabsf(d2) + fabsf(d3));
            if (grad) reinterpret_cast<float4 *>(grad)[i] = make_float4(sg(d0), sg(d1), sg(d2), sg(d3));
        }
        if (sign8) reinterpret_cast<char4 *>(sign8)[i] = make_char4(s8(d0), s8(d1), s8(d2), s8(d3));
    };
    const int64_t stride = (int64_t)gridDim.x * L1_THREADS;
    int64_t i = (int64_t)blockIdx.x * L1_THREADS + threadIdx.x;
    for (; i + 3 * stride < n4; i += 4 * stride) {   // four independent pairs of 16-byte loads in flight (two: 24.6 us for 4 x 3 x 800^2)
        const float4 x0 = reinterpret_cast<const float4 *>(a)[i], y0 = reinterpret_cast<const float4 *>(b)[i];
        const float4 x1 = reinterpret_cast<const float4 *>(a)[i + stride], y1 = reinterpret_cast<const float4 *>(b)[i + stride];
        const float4 x2 = reinterpret_cast<const float4 *>(a)[i + 2 * stride], y2 = reinterpret_cast<const float4 *>(b)[i + 2 * stride];
        const float4 x3 = reinterpret_cast<const float4 *>(a)[i + 3 * stride], y3 = reinterpret_cast<const float4 *>(b)[i + 3 * stride];
        one(i, x0, y0);
        one(i + stride, x1, y1);
        one(i + 2 * stride, x2, y2);
        one(i + 3 * stride, x3, y3);
    }
    for (; i + stride < n4; i += 2 * stride) {   // two independent pairs of 16-byte loads in flight
        const float4 x0 = reinterpret_cast<const float4 *>(a)[i], y0 = reinterpret_cast<const float4 *>(b)[i];
        const float4 x1 = reinterpret_cast<const float4 *>(a)[i + stride], y1 = reinterpret_cast<const float4 *>(b)[i + stride];
        one(i, x0, y0);
        one(i + stride, x1, y1);
    }
    if (i < n4) one(i, reinterpret_cast<const float4 *>(a)[i], reinterpret_cast<const float4 *>(b)[i]);
    // tail: n not a multiple of 4 (<= 3 elements, all on workgroup 0), or every element when the planes or the operands are not 16-byte-aligned
    for (int64_t i = (n4 << 2) + (int64_t)blockIdx.x * L1_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * L1_THREADS) {
        float d = a[i] - b[i];
        float m = 1.f;
        if (mask) { m = mask[moff(i)]; d *= m; }
        acc += fabsf(d);
        if (grad) grad[i] = sg(d) * m;
        if (sign8) sign8[i] = s8(d);
    }
    block_sum<L1_THREADS>(s_red, acc);
    // one partial per workgroup; k_l1_finish (a second, one-workgroup launch) sums them in index order.  Rounds 1-4 had the LAST workgroup
    // to arrive do that behind a ticket: a device-scope release per workgroup, and on gfx950 a release writes the XCD's dirty L2 lines back
    // -- here the sign bytes this kernel has just stored and the image the compositing kernel wrote in front of it -- which made ~10 us of
    // fixed cost on a kernel that streams its 69 MB in ~14 us (24.8 us for four views, 15 us for ONE view: profiles/r04g, r05g).
    if (threadIdx.x == 0) partial[blockIdx.x] = acc;
}
__global__ __launch_bounds__(L1_BLOCKS) void k_l1_finish(int nparts, const float *__restrict__ partial, float inv_n, float *__restrict__ loss) {
    __shared__ float s[L1_BLOCKS];
    s[threadIdx.x] = (int)threadIdx.x < nparts ? partial[threadIdx.x] : 0.f;
    __syncthreads();
    if (threadIdx.x == 0) {       // groups of 16 in index order, then the group sums in index order: a fixed tree
        float tt = 0.f;
        for (int g = 0; g < L1_BLOCKS / 16; g++) {
            float t = 0.f;
            for (int k = 0; k < 16; k++) t += s[16 * g + k];
            tt += t;
        }
        *loss = tt * inv_n;
    }
}
// ---- geometry loss of a train step: depth and silhouette supervision on the rasterizer's depth image D = sum T alpha z and alpha image
// A = 1 - T_final (include/csplat.h, csplat_geom_loss_fwd, states the semantics).  No counterpart in the reference, whose losses never
// touch `depth`.  The views of a step arrive as per-view pointer tables (as k_step_stats takes them): the rasterizer's images are separate
// allocations, a stacked form would cost a copy of each every step.  One pass over all pixels writes ONE BYTE per pixel -- two 2-bit codes of
// sign(r_d w_d) and sign(r_s w_s) -- and two partial sums per workgroup; k_geom_loss_finish (one workgroup) sums them in index order, as
// k_l1_finish does: no ticket, no float atomics.  Algorithmic bytes per pixel: <= 5 floats read + 1 byte written forward (D, A, Z, S, M),
// 1 byte + <= 2 floats read (Z, M) + 2 floats written backward.
constexpr int GL_THREADS = 256, GL_MAX_BLOCKS = 1024, GL_VIEWS = 16;      // workgroups per view <= GL_MAX_BLOCKS; views per launch <= GL_VIEWS
struct GeomTable {
    const float *D[GL_VIEWS], *A[GL_VIEWS], *Z[GL_VIEWS], *S[GL_VIEWS], *M[GL_VIEWS];
};
// 2-bit code of sign(r * w): 0 -> -1, 1 -> 0, 2 -> +1, 3 -> NaN.  From the two signs, not from the rounded product (which may underflow to 0)
__device__ __forceinline__ unsigned geom_code(float r, float w) {
    if (r != r || w != w) return 3u;
    const int sr = (r > 0.f) - (r < 0.f), sw = (w > 0.f) - (w < 0.f);
    return (unsigned)(sr * sw + 1);
}
__device__ __forceinline__ float geom_sign(unsigned code) { return code == 3u ? __builtin_nanf("") : (float)((int)code - 1); }
// a sensor map's hole is 0, negative, NaN or Inf
__device__ __forceinline__ bool geom_valid(float z) { return z > 0.f && z < __builtin_inff(); }

// one pixel: adds its two terms to acc_d / acc_s and returns its byte.  SELECTION: a pixel of weight 0 adds exactly 0 and gets the code of
// sign 0, whatever D, A, Z hold there (NaN, Inf); D, Z, S are only looked at when their term is on
// (selects, not branches: a load that is only used inside a divergent branch is sunk into it by the compiler, one dword at a time -- the
//  first form of this kernel had 21 4-byte loads where five 16-byte ones were written)
template <bool HAS_Z, bool HAS_S>
__device__ __forceinline__ unsigned geom_pixel(float d, float a, float z, float s, float m, float &acc_d, float &acc_s) {
    unsigned code_d = 1u, code_s = 1u;
    if (HAS_Z) {
        const float w = geom_valid(z) ? m : 0.f;
        const bool on = w != 0.f;
        const float r = fmaf(-a, z, d);           // ONE rounding: the sign is the exact sign of D - A Z (a separate multiply may flip it near a tie)
        acc_d += on ? fabsf(r * w) : 0.f;
        code_d = on ? geom_code(r, w) : 1u;
    }
    if (HAS_S) {
        const bool on = m != 0.f;
        const float r = a - s;
        acc_s += on ? fabsf(r * m) : 0.f;
        code_s = on ? geom_code(r, m) : 1u;
    }
    return code_d | (code_s << 2);
}

// grid (workgroups per view, views of this launch).  partial [2][n_parts]: the depth sums, then the silhouette sums, at
// (view0 + blockIdx.y) * gridDim.x + blockIdx.x.  vec: every pointer of the call is 16-byte aligned and hw % 4 == 0
template <bool HAS_Z, bool HAS_S, bool HAS_M>
__global__ __launch_bounds__(GL_THREADS) void k_geom_loss_fwd(int64_t hw, GeomTable tab, int view0, int64_t n_parts, int vec,
                                                              float *__restrict__ partial, unsigned char *__restrict__ sign8) {
    __shared__ float s_red[2][GL_THREADS / 64];
    const int v = blockIdx.y;
    const float *__restrict__ D = tab.D[v], *__restrict__ A = tab.A[v], *__restrict__ Z = tab.Z[v], *__restrict__ S = tab.S[v],
                *__restrict__ M = tab.M[v];
    unsigned char *sg = sign8 ? sign8 + (int64_t)(view0 + v) * hw : nullptr;
    float acc_d = 0.f, acc_s = 0.f;
    const int64_t stride = (int64_t)gridDim.x * GL_THREADS;
    if (vec) {
        const int64_t n4 = hw >> 2;
        const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f), one = make_float4(1.f, 1.f, 1.f, 1.f);
        for (int64_t i = (int64_t)blockIdx.x * GL_THREADS + threadIdx.x; i < n4; i += stride) {
            const float4 a = reinterpret_cast<const float4 *>(A)[i];
            const float4 d = HAS_Z ? reinterpret_cast<const float4 *>(D)[i] : zero, z = HAS_Z ? reinterpret_cast<const float4 *>(Z)[i] : zero;
            const float4 s = HAS_S ? reinterpret_cast<const float4 *>(S)[i] : zero, m = HAS_M ? reinterpret_cast<const float4 *>(M)[i] : one;
            const unsigned c0 = geom_pixel<HAS_Z, HAS_S>(d.x, a.x, z.x, s.x, m.x, acc_d, acc_s);
            const unsigned c1 = geom_pixel<HAS_Z, HAS_S>(d.y, a.y, z.y, s.y, m.y, acc_d, acc_s);
            const unsigned c2 = geom_pixel<HAS_Z, HAS_S>(d.z, a.z, z.z, s.z, m.z, acc_d, acc_s);
            const unsigned c3 = geom_pixel<HAS_Z, HAS_S>(d.w, a.w, z.w, s.w, m.w, acc_d, acc_s);
            if (sg) reinterpret_cast<uchar4 *>(sg)[i] = make_uchar4((unsigned char)c0, (unsigned char)c1, (unsigned char)c2, (unsigned char)c3);
        }
    } else {
        for (int64_t i = (int64_t)blockIdx.x * GL_THREADS + threadIdx.x; i < hw; i += stride) {
            const unsigned c = geom_pixel<HAS_Z, HAS_S>(HAS_Z ? D[i] : 0.f, A[i], HAS_Z ? Z[i] : 0.f, HAS_S ? S[i] : 0.f, HAS_M ? M[i] : 1.f,
                                                        acc_d, acc_s);
            if (sg) sg[i] = (unsigned char)c;
        }
    }
    block_sum<GL_THREADS>(s_red, acc_d, acc_s);
    if (threadIdx.x == 0) {
        const int64_t at = (int64_t)(view0 + v) * gridDim.x + blockIdx.x;
        partial[at] = acc_d;
        partial[n_parts + at] = acc_s;
    }
}

// the second (one-workgroup) launch: a fixed tree over the partials in index order -- any number of them, each thread walks its residue
// class -- then out[3] = {weight * (lam_d L_depth + lam_s L_sil) + add_weight * add[0], L_depth, L_sil}
__global__ __launch_bounds__(GL_THREADS) void k_geom_loss_finish(int64_t n_parts, const float *__restrict__ partial, float n_pixels, float lam_d,
                                                                 float lam_s, float weight, const float *__restrict__ add, float add_weight,
                                                                 float *__restrict__ out) {
    __shared__ float s_red[2][GL_THREADS / 64];
    float td = 0.f, ts = 0.f;
    for (int64_t i = threadIdx.x; i < n_parts; i += GL_THREADS) { td += partial[i]; ts += partial[n_parts + i]; }
    block_sum<GL_THREADS>(s_red, td, ts);
    if (threadIdx.x == 0) {
        const float ld = td / n_pixels, ls = ts / n_pixels;
        out[0] = weight * (lam_d * ld + lam_s * ls) + (add ? add_weight * add[0] : 0.f);
        out[1] = ld;
        out[2] = ls;
    }
}

// backward, one launch: dD = g lam_d w_d sign_d / n, dA = g (-lam_d w_d Z sign_d + lam_s w_s sign_s) / n from the sign bytes, Z and M; a pixel
// of weight 0 gets exactly 0 (selection: its Z may be NaN).  dD / dA [views][hw], either may be NULL.  scale_d / scale_s = lam / n
template <bool HAS_Z, bool HAS_S, bool HAS_M>
__global__ __launch_bounds__(GL_THREADS) void k_geom_loss_bwd(int64_t hw, GeomTable tab, int view0, int vec, const unsigned char *__restrict__ sign8,
                                                              const float *__restrict__ g, float scale_d, float scale_s,
                                                              float *__restrict__ dD, float *__restrict__ dA) {
    const int v = blockIdx.y;
    const float *__restrict__ Z = tab.Z[v], *__restrict__ M = tab.M[v];      // (only these two tables are read here)
    const int64_t base = (int64_t)(view0 + v) * hw;
    const unsigned char *sg = sign8 + base;
    float *od = dD ? dD + base : nullptr, *oa = dA ? dA + base : nullptr;
    const float sc_d = g[0] * scale_d, sc_s = g[0] * scale_s;
    auto one = [&](unsigned code, float z, float m, float &gd, float &ga) {
        gd = 0.f; ga = 0.f;
        if (HAS_Z) {
            const float w = geom_valid(z) ? m : 0.f;
            const float t = sc_d * w * geom_sign(code & 3u);
            gd = w != 0.f ? t : 0.f;              // (selects: see geom_pixel)
            ga = w != 0.f ? -t * z : 0.f;
        }
        if (HAS_S) ga += m != 0.f ? sc_s * m * geom_sign((code >> 2) & 3u) : 0.f;
    };
    const int64_t stride = (int64_t)gridDim.x * GL_THREADS;
    if (vec) {
        const int64_t n4 = hw >> 2;
        const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f), ones = make_float4(1.f, 1.f, 1.f, 1.f);
        for (int64_t i = (int64_t)blockIdx.x * GL_THREADS + threadIdx.x; i < n4; i += stride) {
            const uchar4 c = reinterpret_cast<const uchar4 *>(sg)[i];
            const float4 z = HAS_Z ? reinterpret_cast<const float4 *>(Z)[i] : zero, m = HAS_M ? reinterpret_cast<const float4 *>(M)[i] : ones;
            float4 gd, ga;
            one(c.x, z.x, m.x, gd.x, ga.x);
            one(c.y, z.y, m.y, gd.y, ga.y);
            one(c.z, z.z, m.z, gd.z, ga.z);
            one(c.w, z.w, m.w, gd.w, ga.w);
            if (od) reinterpret_cast<float4 *>(od)[i] = gd;
            if (oa) reinterpret_cast<float4 *>(oa)[i] = ga;
        }
    } else {
        for (int64_t i = (int64_t)blockIdx.x * GL_THREADS + threadIdx.x; i < hw; i += stride) {
            float gd, ga;
            one(sg[i], HAS_Z ? Z[i] : 0.f, HAS_M ? M[i] : 1.f, gd, ga);
            if (od) od[i] = gd;
            if (oa) oa[i] = ga;
        }
    }
}

// ---- PSNR per image (utils/image_utils.py psnr: mse over all channels and pixels of an image, 20 log10(1 / sqrt(mse))).
// The reference logs it every training step; as torch ops it is ~10 launches.  gridDim.y = image, PSNR_BLOCKS slices per
// image, last slice of an image (ticket) sums the slice partials in fixed order.
constexpr int PSNR_BLOCKS = 64;
__global__ __launch_bounds__(1024) void k_psnr(int64_t n, const float *__restrict__ a, const float *__restrict__ b,
                                               float *__restrict__ partial, unsigned *__restrict__ ticket, float *__restrict__ out) {
    __shared__ float s_red[16];
    __shared__ bool s_last;
    const float *pa = a + (size_t)blockIdx.y * n, *pb = b + (size_t)blockIdx.y * n;
    float acc = 0.f;
    if ((((uintptr_t)pa | (uintptr_t)pb) & 15u) == 0) {
        const int64_t n4 = n >> 2;
        for (int64_t i = (int64_t)blockIdx.x * 1024 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 1024) {
            const float4 x = reinterpret_cast<const float4 *>(pa)[i], y = reinterpret_cast<const float4 *>(pb)[i];
            const float d0 = x.x - y.x, d1 = x.y - y.y, d2 = x.z - y.z, d3 = x.w - y.w;
            acc += (d0 * d0 + d1 * d1) + (d2 * d2 + d3 * d3);
        }
        if (blockIdx.x == 0)
            for (int64_t i = (n4 << 2) + threadIdx.x; i < n; i += 1024) { const float d = pa[i] - pb[i]; acc += d * d; }
    } else {
        for (int64_t i = (int64_t)blockIdx.x * 1024 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 1024) {
            const float d = pa[i] - pb[i];
            acc += d * d;
        }
    }
    block_sum<1024>(s_red, acc);
    if (threadIdx.x == 0) {
        partial[blockIdx.y * PSNR_BLOCKS + blockIdx.x] = acc;
        __threadfence();
        s_last = atomicAdd(ticket + blockIdx.y, 1u) == gridDim.x - 1;
    }
    __syncthreads();
    if (s_last && threadIdx.x == 0) {
        __threadfence();
        float t = 0.f;
        for (unsigned k = 0; k < gridDim.x; k++) t += __builtin_nontemporal_load(partial + blockIdx.y * PSNR_BLOCKS + k);
        const float mse = t / (float)n;
        out[blockIdx.y] = 20.f * log10f(1.f / sqrtf(mse));
        ticket[blockIdx.y] = 0u;
    }
}
}  // namespace

// ---- what every launch of a tile kernel starts from: one workgroup per 64 x 16 tile and plane (the plane rides in blockIdx.z, hence
// fewer than 65536 of them per launch) and the window's taps by value
static dim3 tile_grid(int64_t planes, int H, int W) { return dim3(cdiv(W, BW), cdiv(H, BH), (unsigned)planes); }
struct TileLaunch { Taps taps; dim3 grid; };
static int tile_launch(const char *who, const float *taps11, int64_t planes, int H, int W, TileLaunch *tl) {
    if (!(taps11 && planes >= 0 && planes < 65536 && H > 0 && W > 0)) {
        snprintf(g_csplat_err, sizeof(g_csplat_err), "%s: bad arguments (the taps, H, W > 0, fewer than 65536 planes per launch) (%s:%d)", who,
                 __FILE__, __LINE__);
        return 2;
    }
    memcpy(tl->taps.w, taps11, sizeof(tl->taps.w));
    tl->grid = tile_grid(planes, H, W);
    return 0;
}

extern "C" int csplat_blur11(void *stream, int64_t n_images, int H, int W, const float *taps11, const float *in, float *out) {
    CSPLAT_REQUIRE(in && out && in != out, "csplat_blur11: bad arguments");
    TileLaunch tl;
    if (int rc = tile_launch("csplat_blur11", taps11, n_images, H, W, &tl)) return rc;
    if (n_images == 0) return 0;
    k_blur11<<<tl.grid, IL_T, 0, (hipStream_t)stream>>>(H, W, tl.taps, in, out);
    LAUNCH_CHECK();
    return 0;
}

extern "C" size_t csplat_l1_scratch_bytes(void) { return (size_t)(L1_BLOCKS + 1) * 4; }   // the workgroup partials

// backward of the fused L1 when the forward kept one BYTE per element (csplat_l1_signs): out[i] = g[0] * sign[i] * m[i] / n -- the
// upstream gradient g is a device scalar, so the reference's three elementwise backward launches (and the multiply by the incoming
// gradient that a stored float gradient image needs) are this one pass: 1 (+4 masked) bytes read, 4 written per element
__global__ __launch_bounds__(256) void k_l1_bwd(int64_t n, const signed char *__restrict__ sign8, const float *__restrict__ g, float inv_n,
                                                const float *__restrict__ mask, int64_t hw, int channels, int mask_channels,
                                                float *__restrict__ out) {
    const float sc = g[0] * inv_n;
    auto moff = [&](int64_t e) {
        const int64_t plane = e / hw;
        return (mask_channels == 1 ? plane / channels : plane) * hw + (e - plane * hw);
    };
    const int64_t n4 = ((mask && (hw & 3)) || ((uintptr_t)mask & 15u)) ? 0 : n >> 2;      // (a misaligned mask: scalar form, as k_l1)
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += stride) {
        const char4 s = reinterpret_cast<const char4 *>(sign8)[i];
        float4 o = make_float4(sc * (float)s.x, sc * (float)s.y, sc * (float)s.z, sc * (float)s.w);
        if (mask) {
            const float4 m = *reinterpret_cast<const float4 *>(mask + moff(i << 2));
            o.x *= m.x; o.y *= m.y; o.z *= m.z; o.w *= m.w;
        }
        reinterpret_cast<float4 *>(out)[i] = o;
    }
    for (int64_t i = (n4 << 2) + (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride)
        out[i] = sc * (float)sign8[i] * (mask ? mask[moff(i)] : 1.f);
}

static int l1_launch(void *stream, int64_t n, const float *a, const float *b, void *scratch, float *loss, float *grad,
                     const float *mask, int64_t hw, int channels, int mask_channels, signed char *sign8 = nullptr) {
    CSPLAT_REQUIRE(n > 0 && a && b && scratch && loss, "csplat_l1: bad arguments");
    CSPLAT_REQUIRE((((uintptr_t)a | (uintptr_t)b | (uintptr_t)grad | (uintptr_t)mask) & 3u) == 0, "csplat_l1: operands must be 4-byte aligned");
    const bool al = ((((uintptr_t)a | (uintptr_t)b | (uintptr_t)grad | (uintptr_t)mask) & 15u) == 0);      // else k_l1 takes its scalar form
    float *partial = (float *)scratch;
    const int64_t units = ((mask && (hw & 3)) || !al) ? n : n / 4;
    const int64_t work = (units + L1_THREADS - 1) / L1_THREADS;
    const int grid = (int)(work < 1 ? 1 : (work > L1_BLOCKS ? L1_BLOCKS : work));
    CSPLAT_REQUIRE(((uintptr_t)sign8 & 3u) == 0, "csplat_l1: the sign buffer must be 4-byte aligned");
    k_l1<<<grid, L1_THREADS, 0, (hipStream_t)stream>>>(n, a, b, 1.0f / (float)n, partial, grad, mask, hw, channels, mask_channels, sign8);
    LAUNCH_CHECK();
    k_l1_finish<<<1, L1_BLOCKS, 0, (hipStream_t)stream>>>(grid, partial, 1.0f / (float)n, loss);
    LAUNCH_CHECK();
    return 0;
}

extern "C" int csplat_l1(void *stream, int64_t n, const float *a, const float *b, void *scratch, float *loss, float *grad) {
    return l1_launch(stream, n, a, b, scratch, loss, grad, nullptr, 1, 1, 1);
}

extern "C" int csplat_l1_masked(void *stream, int64_t n_batch, int channels, int64_t hw, const float *a, const float *b,
                                const float *mask, int mask_channels, void *scratch, float *loss, float *grad) {
    CSPLAT_REQUIRE(n_batch > 0 && channels > 0 && hw > 0 && mask, "csplat_l1_masked: bad arguments");
    CSPLAT_REQUIRE(mask_channels == 1 || mask_channels == channels, "csplat_l1_masked: the mask has 1 plane per image or one per channel");
    return l1_launch(stream, n_batch * channels * hw, a, b, scratch, loss, grad, mask, hw, channels, mask_channels);
}

extern "C" int csplat_l1_signs(void *stream, int64_t n_batch, int channels, int64_t hw, const float *a, const float *b, const float *mask,
                               int mask_channels, void *scratch, float *loss, signed char *sign8) {
    CSPLAT_REQUIRE(n_batch > 0 && channels > 0 && hw > 0 && sign8, "csplat_l1_signs: bad arguments");
    CSPLAT_REQUIRE(!mask || mask_channels == 1 || mask_channels == channels, "csplat_l1_signs: the mask has 1 plane per image or one per channel");
    return l1_launch(stream, n_batch * channels * hw, a, b, scratch, loss, nullptr, mask, hw, channels, mask ? mask_channels : 1, sign8);
}
extern "C" int csplat_l1_signs_bwd(void *stream, int64_t n_batch, int channels, int64_t hw, const signed char *sign8, const float *mask,
                                   int mask_channels, const float *g_scalar, float *out) {
    CSPLAT_REQUIRE(n_batch > 0 && channels > 0 && hw > 0 && sign8 && g_scalar && out, "csplat_l1_signs_bwd: bad arguments");
    CSPLAT_REQUIRE(((uintptr_t)out & 15u) == 0 && (((uintptr_t)sign8 | (uintptr_t)mask) & 3u) == 0, "csplat_l1_signs_bwd: operands must be aligned");
    const int64_t n = n_batch * channels * hw;
    const int64_t work = (n / 4 + 255) / 256;
    const int grid = (int)(work < 1 ? 1 : (work > 4096 ? 4096 : work));
    k_l1_bwd<<<grid, 256, 0, (hipStream_t)stream>>>(n, sign8, g_scalar, 1.0f / (float)n, mask, hw, channels, mask ? mask_channels : 1, out);
    LAUNCH_CHECK();
    return 0;
}

// ---- geometry loss (k_geom_loss_fwd + k_geom_loss_finish / k_geom_loss_bwd; include/csplat.h states the semantics)
static int geom_blocks(int64_t hw, bool vec) {
    const int64_t work = ((vec ? hw >> 2 : hw) + GL_THREADS - 1) / GL_THREADS;
    return (int)(work < 1 ? 1 : (work > GL_MAX_BLOCKS ? GL_MAX_BLOCKS : work));
}
// 16-byte accesses need every pointer of the call 16-byte aligned and 4-pixel groups that stay inside a view; all need 4-byte alignment
static int geom_alignment(int n_views, int64_t hw, const float *const *const tabs[], int n_tabs, bool *vec) {
    uintptr_t bits = 0;
    for (int t = 0; t < n_tabs; t++)
        if (tabs[t])
            for (int v = 0; v < n_views; v++) {
                CSPLAT_REQUIRE(tabs[t][v], "csplat_geom_loss: a NULL view in a table that is given");
                bits |= (uintptr_t)tabs[t][v];
            }
    CSPLAT_REQUIRE((bits & 3u) == 0, "csplat_geom_loss: operands must be 4-byte aligned");
    *vec = (bits & 15u) == 0 && (hw & 3) == 0;
    return 0;
}
extern "C" size_t csplat_geom_loss_scratch_bytes(int n_views, int64_t hw) {
    return align256((size_t)2 * (size_t)(n_views > 0 ? n_views : 1) * geom_blocks(hw > 0 ? hw : 1, false) * 4);      // [2][views * workgroups]
}
extern "C" int csplat_geom_loss_fwd(void *stream, int n_views, int64_t hw, const float *const *depth, const float *const *alpha,
                                    const float *const *gt_depth, const float *const *silhouette, const float *const *mask,
                                    float lambda_depth, float lambda_silhouette, float weight, const float *add, float add_weight,
                                    unsigned char *sign8, void *scratch, float *out) {
    CSPLAT_REQUIRE(n_views > 0 && hw > 0 && alpha && scratch && out, "csplat_geom_loss_fwd: bad arguments");
    CSPLAT_REQUIRE(lambda_depth >= 0.f && lambda_silhouette >= 0.f, "csplat_geom_loss_fwd: the weights are >= 0");
    if (!(lambda_depth > 0.f)) gt_depth = nullptr;             // a term is on when its weight is > 0 and its data are given
    if (!(lambda_silhouette > 0.f)) silhouette = nullptr;
    CSPLAT_REQUIRE(gt_depth || silhouette, "csplat_geom_loss_fwd: no term is on (both tables NULL or both weights 0)");
    CSPLAT_REQUIRE(!gt_depth || depth, "csplat_geom_loss_fwd: the depth term needs the depth images");
    CSPLAT_REQUIRE((int64_t)n_views * hw < ((int64_t)1 << 40), "csplat_geom_loss_fwd: too many pixels");
    const float *const *const tabs[5] = {gt_depth ? depth : nullptr, alpha, gt_depth, silhouette, mask};
    bool vec = false;
    if (int rc = geom_alignment(n_views, hw, tabs, 5, &vec)) return rc;
    CSPLAT_REQUIRE(((uintptr_t)sign8 & 3u) == 0, "csplat_geom_loss_fwd: the sign bytes must be 4-byte aligned");
    const int gx = geom_blocks(hw, vec);
    const int64_t n_parts = (int64_t)n_views * gx;
    float *partial = (float *)scratch;
    ProfScope ps(PROF_GEOM_LOSS_FWD, (hipStream_t)stream);
    for (int v0 = 0; v0 < n_views; v0 += GL_VIEWS) {          // more views than a table holds: one launch per GL_VIEWS, the partials of all
        const int nv = n_views - v0 < GL_VIEWS ? n_views - v0 : GL_VIEWS;      // launches side by side, summed in index order below
        GeomTable tab;
        memset(&tab, 0, sizeof(tab));
        for (int v = 0; v < nv; v++) {
            tab.A[v] = alpha[v0 + v];
            if (gt_depth) { tab.D[v] = depth[v0 + v]; tab.Z[v] = gt_depth[v0 + v]; }
            if (silhouette) tab.S[v] = silhouette[v0 + v];
            if (mask) tab.M[v] = mask[v0 + v];
        }
        const dim3 grid(gx, nv);
#define GEOM_FWD(Z_, S_, M_) k_geom_loss_fwd<Z_, S_, M_><<<grid, GL_THREADS, 0, (hipStream_t)stream>>>(hw, tab, v0, n_parts, vec ? 1 : 0, partial, sign8)
        switch ((gt_depth ? 4 : 0) | (silhouette ? 2 : 0) | (mask ? 1 : 0)) {       // (no term on was refused above)
        case 2: GEOM_FWD(false, true, false); break;
        case 3: GEOM_FWD(false, true, true); break;
        case 4: GEOM_FWD(true, false, false); break;
        case 5: GEOM_FWD(true, false, true); break;
        case 6: GEOM_FWD(true, true, false); break;
        default: GEOM_FWD(true, true, true); break;
        }
#undef GEOM_FWD
        LAUNCH_CHECK();
    }
    k_geom_loss_finish<<<1, GL_THREADS, 0, (hipStream_t)stream>>>(n_parts, partial, (float)n_views * (float)hw, gt_depth ? lambda_depth : 0.f,
                                                                  silhouette ? lambda_silhouette : 0.f, weight, add, add_weight, out);
    LAUNCH_CHECK();
    return 0;
}
extern "C" int csplat_geom_loss_bwd(void *stream, int n_views, int64_t hw, const unsigned char *sign8, const float *const *gt_depth,
                                    const float *const *mask, float lambda_depth, float lambda_silhouette, float weight,
                                    const float *g_scalar, float *d_depth, float *d_alpha) {
    CSPLAT_REQUIRE(n_views > 0 && hw > 0 && sign8 && g_scalar && (d_depth || d_alpha), "csplat_geom_loss_bwd: bad arguments");
    CSPLAT_REQUIRE(lambda_depth >= 0.f && lambda_silhouette >= 0.f, "csplat_geom_loss_bwd: the weights are >= 0");
    if (!(lambda_depth > 0.f)) gt_depth = nullptr;
    const bool sil = lambda_silhouette > 0.f;
    CSPLAT_REQUIRE(gt_depth || sil, "csplat_geom_loss_bwd: no term is on (no depth table and no silhouette weight)");
    const float *const *const tabs[2] = {gt_depth, mask};
    bool vec = false;
    if (int rc = geom_alignment(n_views, hw, tabs, 2, &vec)) return rc;
    CSPLAT_REQUIRE((((uintptr_t)sign8 | (uintptr_t)d_depth | (uintptr_t)d_alpha) & 3u) == 0, "csplat_geom_loss_bwd: operands must be 4-byte aligned");
    vec = vec && (((uintptr_t)d_depth | (uintptr_t)d_alpha) & 15u) == 0;
    const int gx = geom_blocks(hw, vec);
    const float inv_n = 1.0f / ((float)n_views * (float)hw);
    ProfScope ps(PROF_GEOM_LOSS_BWD, (hipStream_t)stream);
    for (int v0 = 0; v0 < n_views; v0 += GL_VIEWS) {
        const int nv = n_views - v0 < GL_VIEWS ? n_views - v0 : GL_VIEWS;
        GeomTable tab;
        memset(&tab, 0, sizeof(tab));
        for (int v = 0; v < nv; v++) {
            if (gt_depth) tab.Z[v] = gt_depth[v0 + v];
            if (mask) tab.M[v] = mask[v0 + v];
        }
        const dim3 grid(gx, nv);
#define GEOM_BWD(Z_, S_, M_)                                                                                                              \
    k_geom_loss_bwd<Z_, S_, M_><<<grid, GL_THREADS, 0, (hipStream_t)stream>>>(hw, tab, v0, vec ? 1 : 0, sign8, g_scalar, weight * lambda_depth * inv_n, \
                                                                              weight * lambda_silhouette * inv_n, d_depth, d_alpha)
        switch ((gt_depth ? 4 : 0) | (sil ? 2 : 0) | (mask ? 1 : 0)) {
        case 2: GEOM_BWD(false, true, false); break;
        case 3: GEOM_BWD(false, true, true); break;
        case 4: GEOM_BWD(true, false, false); break;
        case 5: GEOM_BWD(true, false, true); break;
        case 6: GEOM_BWD(true, true, false); break;
        default: GEOM_BWD(true, true, true); break;
        }
#undef GEOM_BWD
        LAUNCH_CHECK();
    }
    return 0;
}

static size_t tiles_per_plane(int H, int W) { const dim3 g = tile_grid(1, H, W); return (size_t)g.x * g.y; }
extern "C" size_t csplat_ssim_partial_count(int64_t n_images, int H, int W) { return (size_t)n_images * tiles_per_plane(H, W); }

static int ssim_fwd_launch(void *stream, int64_t n_images, int H, int W, const float *taps11, const float *x, const float *y,
                           float *p1, float *p2, float *p3, float *map_out, float *partial, const float *mask, int mask_channels,
                           int channels) {
    CSPLAT_REQUIRE(x && y && partial, "csplat_ssim_fwd: bad arguments");
    TileLaunch tl;
    if (int rc = tile_launch("csplat_ssim_fwd", taps11, n_images, H, W, &tl)) return rc;
    CSPLAT_REQUIRE((p1 != nullptr) == (p2 != nullptr) && (p1 != nullptr) == (p3 != nullptr), "csplat_ssim_fwd: all three partials or none");
    if (n_images == 0) return 0;
    k_ssim_fwd<<<tl.grid, IL_T, 0, (hipStream_t)stream>>>(H, W, tl.taps, x, y, p1, p2, p3, map_out, partial, mask, mask_channels, channels);
    LAUNCH_CHECK();
    return 0;
}

extern "C" int csplat_ssim_fwd(void *stream, int64_t n_images, int H, int W, const float *taps11, const float *x, const float *y,
                               float *p1, float *p2, float *p3, float *map_out, float *partial) {
    return ssim_fwd_launch(stream, n_images, H, W, taps11, x, y, p1, p2, p3, map_out, partial, nullptr, 1, 1);
}

// masked form: partial sums hold sum((1 - S) * m), the three partial-derivative images are pre-multiplied by m, so that
// csplat_ssim_bwd serves both forms unchanged.  n_images = batch * channels planes; mask [batch, mask_channels, H, W].
extern "C" int csplat_ssim_fwd_masked(void *stream, int64_t n_batch, int channels, int H, int W, const float *taps11, const float *x,
                                      const float *y, const float *mask, int mask_channels, float *p1, float *p2, float *p3,
                                      float *map_out, float *partial) {
    CSPLAT_REQUIRE(n_batch >= 0 && channels > 0 && mask, "csplat_ssim_fwd_masked: bad arguments");
    CSPLAT_REQUIRE(mask_channels == 1 || mask_channels == channels, "csplat_ssim_fwd_masked: the mask has 1 plane per image or one per channel");
    return ssim_fwd_launch(stream, n_batch * channels, H, W, taps11, x, y, p1, p2, p3, map_out, partial, mask, mask_channels, channels);
}

extern "C" int csplat_ssim_bwd(void *stream, int64_t n_images, int H, int W, const float *taps11, const float *x, const float *y,
                               const float *p1, const float *p2, const float *p3, const float *g_scalar, float inv_n,
                               const float *addend, const float *add_scale, float *dx) {
    CSPLAT_REQUIRE(x && y && p1 && p2 && p3 && g_scalar && dx, "csplat_ssim_bwd: bad arguments");
    TileLaunch tl;
    if (int rc = tile_launch("csplat_ssim_bwd", taps11, n_images, H, W, &tl)) return rc;
    if (n_images == 0) return 0;
    CSPLAT_REQUIRE((addend == nullptr) == (add_scale == nullptr), "csplat_ssim_bwd: addend and add_scale go together");
    k_ssim_bwd<<<tl.grid, IL_T, 0, (hipStream_t)stream>>>(H, W, tl.taps, x, y, p1, p2, p3, g_scalar, inv_n, addend, add_scale, dx);
    LAUNCH_CHECK();
    return 0;
}

// image loss of a train step (k_image_loss_fwd + k_image_loss_finish / k_image_loss_bwd).  out[4] = {img_weight * image_loss +
// add_weight * add[0], psnr_scale * sum_b PSNR_b, image_loss, Ll1}; scratch: csplat_image_loss_scratch_bytes (no initial state).
// p1..p3 / sign8 may be NULL when no gradient will be asked for.
extern "C" size_t csplat_image_loss_scratch_bytes(int64_t n_batch, int channels, int H, int W) {
    const size_t planes = (size_t)(n_batch > 0 ? n_batch : 1) * channels;
    return align256(3 * planes * tiles_per_plane(H, W) * 4);      // [3][workgroups] partial sums
}
extern "C" int csplat_image_loss_fwd(void *stream, int64_t n_batch, int channels, int H, int W, const float *taps11, const float *x,
                                     const float *y, const float *mask, int mask_channels, float lam, float img_weight, const float *add,
                                     float add_weight, float psnr_scale, float *p1, float *p2, float *p3, signed char *sign8, void *scratch,
                                     float *out) {
    CSPLAT_REQUIRE(n_batch > 0 && channels > 0 && x && y && scratch && out, "csplat_image_loss_fwd: bad arguments");
    TileLaunch tl;
    if (int rc = tile_launch("csplat_image_loss_fwd", taps11, n_batch * channels, H, W, &tl)) return rc;
    CSPLAT_REQUIRE((p1 != nullptr) == (p2 != nullptr) && (p1 != nullptr) == (p3 != nullptr) && (p1 != nullptr) == (sign8 != nullptr),
                   "csplat_image_loss_fwd: the three partials and the sign bytes go together");
    CSPLAT_REQUIRE(!mask || mask_channels == 1 || mask_channels == channels, "csplat_image_loss_fwd: the mask has 1 plane per image or one per channel");
    float *partial = (float *)scratch;
    k_image_loss_fwd<<<tl.grid, IL_T, 0, (hipStream_t)stream>>>(H, W, tl.taps, x, y, p1, p2, p3, sign8, mask, mask ? mask_channels : 1, channels, partial);
    LAUNCH_CHECK();
    k_image_loss_finish<<<1, IL_T, 0, (hipStream_t)stream>>>((size_t)tl.grid.x * tl.grid.y, (int)tl.grid.z, channels, H, W, mask ? 1 : 0, lam, img_weight,
                                                             add, add_weight, psnr_scale, partial, out);
    LAUNCH_CHECK();
    return 0;
}
extern "C" int csplat_image_loss_bwd(void *stream, int64_t n_batch, int channels, int H, int W, const float *taps11, const float *x,
                                     const float *y, const float *p1, const float *p2, const float *p3, const signed char *sign8,
                                     const float *mask, int mask_channels, float lam, float img_weight, const float *g_scalar, float *dx) {
    CSPLAT_REQUIRE(n_batch > 0 && channels > 0 && x && y && p1 && p2 && p3 && sign8 && g_scalar && dx, "csplat_image_loss_bwd: bad arguments");
    TileLaunch tl;
    if (int rc = tile_launch("csplat_image_loss_bwd", taps11, n_batch * channels, H, W, &tl)) return rc;
    const float inv_n = 1.0f / ((float)(n_batch * channels) * (float)H * (float)W);
    k_image_loss_bwd<<<tl.grid, IL_T, 0, (hipStream_t)stream>>>(H, W, tl.taps, x, y, p1, p2, p3, sign8, mask, mask ? mask_channels : 1, channels,
                                                                g_scalar, img_weight * inv_n, -lam * img_weight * inv_n, dx);
    LAUNCH_CHECK();
    return 0;
}

extern "C" size_t csplat_psnr_scratch_bytes(int64_t n_images) { return (size_t)(n_images > 0 ? n_images : 1) * (PSNR_BLOCKS + 1) * 4; }

extern "C" int csplat_psnr(void *stream, int64_t n_images, int64_t n_per_image, const float *a, const float *b, void *scratch,
                           float *out) {
    CSPLAT_REQUIRE(n_images >= 0 && n_images < 65536 && n_per_image > 0, "csplat_psnr: bad sizes");
    if (n_images == 0) return 0;
    CSPLAT_REQUIRE(a && b && scratch && out, "csplat_psnr: NULL");
    float *partial = (float *)scratch;
    unsigned *ticket = (unsigned *)scratch + n_images * PSNR_BLOCKS;
    HIP_TRY(hipMemsetAsync(ticket, 0, (size_t)n_images * 4, (hipStream_t)stream));
    const int64_t work = (n_per_image / 4 + 1023) / 1024;
    dim3 grid((unsigned)(work < 1 ? 1 : (work > PSNR_BLOCKS ? PSNR_BLOCKS : work)), (unsigned)n_images);
    k_psnr<<<grid, 1024, 0, (hipStream_t)stream>>>(n_per_image, a, b, partial, ticket, out);
    LAUNCH_CHECK();
    return 0;
}
