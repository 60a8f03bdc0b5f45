// csplat_raster_k8.h -- part of csplat_raster.hip, included there once, behind csplat_raster_extended.h, last of the parts.
// K8, the per-Gaussian backward: the camera partials, preprocess_bwd_body and the k_preprocess_bwd* kernels, the batched K8 kernels
// (their body is csplat_k8_views_body.h, included into each of the four), and the fixed-order sums of the camera path (k_bg_partials,
// k_cam_sum).
// Uses from csplat_raster_math.h: the constants, Geom, Cam, ProjJac, the projection / covariance / antialiasing helpers, stage_sh_rows;
// from csplat_raster.hip's K7 section: ACC_STRIDE (the record K7 fills).  Its macros PUT, S, GS, CSPLAT_K8_ARGS and CSPLAT_K8_PASS are
// defined and undefined here.
#pragma once

namespace {

// ------------------------------------------------------------------------------------------- K8
// K7's per-Gaussian record (round 6) holds the MOMENTS of m = G dL/dalpha over the pixels the Gaussian was blended at, about its centre:
// 0 Mx  1 My  2 Mxx  3 Mxy  4 Myy  5 M0  6..8 dL/dcolour.  With conic (a, b, c) and opacity o the pixel-level gradients upstream sums
// pixel by pixel are linear in them:  dL/dmean2D = -0.5 o (a Mx + b My, c My + b Mx)  (pixel units),  dL/dconic = -0.5 o (Mxx, Mxy, Myy),
// dL/dopacity = M0.  In place: a9[0..4] become (dmean2D.x, dmean2D.y, dconic.a, dconic.b, dconic.c), a9[5..8] stay.
__device__ __forceinline__ void moments_to_gradients(float (&a9)[9], const float4 co) {
    const float h = -0.5f * co.w;
    const float mx = a9[0], my = a9[1];
    a9[0] = h * (co.x * mx + co.y * my);
    a9[1] = h * (co.z * my + co.y * mx);
    a9[2] *= h; a9[3] *= h; a9[4] *= h;
}
// CSPLAT_SCRATCH_ZEROED: the record K8 has just read goes back to zero (12 of its 16 floats: the 9 in use, as three 16-byte stores)
__device__ __forceinline__ void clear_record(const float *acc, int i) {
    float4 *p = reinterpret_cast<float4 *>(const_cast<float *>(acc) + (size_t)i * ACC_STRIDE);
    const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
    p[0] = z; p[1] = z; p[2] = z;
}
// ---- camera partials (the camera-gradient path: csplat_view.dL_dview / dL_dproj / dL_dcampos).  One slab row per (workgroup, view):
// 0..15 dL/dview (flat 4 row + col; column 3 is unused by the kernels and stays 0) | 16..31 dL/dproj (column 2 unused, 0) | 32..34 dL/dcampos.
// No float atomics: the rows are summed in a fixed order (cam_block_sum, then k_cam_sum), so the sums are as reproducible as their inputs.
constexpr int CAM_NC = 35;
constexpr int CAM_PARTS = 8;          // first level of cam_block_sum: CAM_PARTS x CAM_NC partial sums over contiguous row ranges
__device__ __forceinline__ void cam_partials_zero(float *row) {
#pragma unroll
    for (int k = 0; k < CAM_NC; k++) row[k] = 0.f;
}
// dL/dview = ph (x) dL/dpv (ph = [m, 1], pv = ph view) plus, on the upper 3x3 block, the term through Rw = view[:3,:3]^T in T = J Rw:
// dL/dview[4 r + k] += (J^T dL/dT)[k][r].  J: J00 = fx / tz, J02 = -fx tx / tz^2, J11 = fy / tz, J12 = -fy ty / tz^2 (tx, ty clamped).
__device__ __forceinline__ void cam_partials_view(float *row, const float p[3], const float dpv[3], float J00, float J02, float J11, float J12,
                                                  const float dT0[3], const float dT1[3]) {
#pragma unroll
    for (int r = 0; r < 3; r++) {
        row[4 * r] = p[r] * dpv[0] + J00 * dT0[r];
        row[4 * r + 1] = p[r] * dpv[1] + J11 * dT1[r];
        row[4 * r + 2] = p[r] * dpv[2] + (J02 * dT0[r] + J12 * dT1[r]);
        row[4 * r + 3] = 0.f;
    }
    row[12] = dpv[0]; row[13] = dpv[1]; row[14] = dpv[2]; row[15] = 0.f;
}
// dL/dproj = ph (x) dL/dhom, hom = ph proj, ndc = hom[:2] / (hom[3] + 1e-7): dL/dhom = (g.x m_w, g.y m_w, 0, -(hom0 g.x + hom1 g.y) m_w^2)
__device__ __forceinline__ void cam_partials_proj(float *row, const float p[3], float dh0, float dh1, float dh3) {
#pragma unroll
    for (int r = 0; r < 3; r++) {
        row[16 + 4 * r] = p[r] * dh0; row[16 + 4 * r + 1] = p[r] * dh1; row[16 + 4 * r + 2] = 0.f; row[16 + 4 * r + 3] = p[r] * dh3;
    }
    row[28] = dh0; row[29] = dh1; row[30] = 0.f; row[31] = dh3;
}
// rows [0, nrows) of s[.][CAM_NC] (LDS) summed per column in a fixed order -> out[CAM_NC] (global): CAM_PARTS contiguous row ranges, then
// the parts in order.  Every thread of the workgroup calls it (it synchronises).
template <int NT>
__device__ __forceinline__ void cam_block_sum(const float *s, int nrows, float *s_part, float *out) {
    __syncthreads();
    const int chunk = (nrows + CAM_PARTS - 1) / CAM_PARTS;
    for (int t = threadIdx.x; t < CAM_PARTS * CAM_NC; t += NT) {
        const int part = t / CAM_NC, c = t - part * CAM_NC;
        const int r0 = part * chunk, r1 = min(nrows, r0 + chunk);
        float a = 0.f;
        for (int r = r0; r < r1; r++) a += s[r * CAM_NC + c];
        s_part[t] = a;
    }
    __syncthreads();
    if (threadIdx.x < CAM_NC) {
        float a = 0.f;
#pragma unroll
        for (int q = 0; q < CAM_PARTS; q++) a += s_part[q * CAM_NC + threadIdx.x];
        out[threadIdx.x] = a;
    }
}

// DEPTH (k_preprocess_bwd_depth, the depth-gradient path only): record slot 9 holds dL/dz of the view-space depth z = view[2] x + view[6] y +
// view[10] z + view[14] (summed g T alpha, K7), which adds dL/dz (view[2], view[6], view[10]) to dL/dmean3D
// CAM (k_preprocess_bwd_cam, the camera-gradient path only): every thread writes its Gaussian's camera partials (cam_partials_*) to its LDS
// row, the workgroup sums them in a fixed order into slab row blockIdx.x (cam_block_sum).  The Gaussian's own gradients are computed by
// exactly the same expressions: the partials only read values the body has formed (never a product that feeds a sum), so no FMA
// contraction of the default arithmetic changes.
// AA (k_preprocess_bwd_aa, antialiasing only): record slot 5 holds dL/do' of the view's o' = o h; dL/dopacity = h dL/do' and o dL/do' dh
// (aa_backward) joins the cov2D gradient before it is turned into the cov3D / scale / rotation / mean (and, with CAM, camera) gradients.
// aa_opacities = the raw opacities o.
template <bool STAGE, int NT, bool DEPTH, bool CAM = false, bool AA = false>
__device__ __forceinline__ void preprocess_bwd_body(int P, int D, int M, const float *__restrict__ means3D,
                                                         const float *__restrict__ shs, const float *__restrict__ scales,
                                                         float scale_mod, const float *__restrict__ rotations,
                                                         int use_precomp_cov, Cam cam, Geom g,
                                                         const int32_t *__restrict__ radii, const float *__restrict__ acc,
                                                         float *__restrict__ dL_dmean2D, float *__restrict__ dL_dconic,
                                                         float *__restrict__ dL_dopacity, float *__restrict__ dL_dcolor,
                                                         float *__restrict__ dL_dmean3D, float *__restrict__ dL_dcov3D,
                                                         float *__restrict__ dL_dsh, float *__restrict__ dL_dscale,
                                                         float *__restrict__ dL_drot, unsigned accmask, float *__restrict__ cam_slab = nullptr,
                                                         const float *__restrict__ aa_opacities = nullptr) {
    // accmask (CSPLAT_ACC_*): outputs that are ADDED to instead of written -- several views of one step share the
    // gradient buffer of a shared parameter (csplat_backward_views), which replaces autograd's per-view temporaries
    // and its V-1 summation launches per parameter.
#define PUT(ptr, idx, val, bit) do { float *p_ = (ptr) + (idx); *p_ = (accmask & (bit)) ? *p_ + (val) : (val); } while (0)
    // STAGE: SH coefficients in / SH gradients out go through LDS so that HBM sees contiguous 16-byte accesses (the
    // lane-per-Gaussian 4-byte stores at a 192-byte stride wrote 2.7x the algorithmic bytes)
    __shared__ float s_in[STAGE ? NT * SH_ROW : 1];
    __shared__ float s_out[STAGE ? NT * SH_ROW : 1];
    __shared__ float s_cam[CAM ? NT * CAM_NC : 1];
    __shared__ float s_cpart[CAM ? CAM_PARTS * CAM_NC : 1];
    float *const crow = s_cam + (CAM ? threadIdx.x * CAM_NC : 0);     // (CAM) this thread's partials
    const int i = blockIdx.x * NT + threadIdx.x;
    const int rows = min(NT, P - blockIdx.x * NT);
    if (STAGE) {
        stage_sh_rows<NT>(shs + (size_t)blockIdx.x * NT * 48, rows, s_in);
        for (int k = 0; k < 48; k++) s_out[threadIdx.x * SH_ROW + k] = 0.f;
        __syncthreads();
    }
    if (i < P) {
    const bool vis = radii[i] > 0;
    float a9[9];
#pragma unroll
    for (int k = 0; k < 9; k++) a9[k] = vis ? acc[(size_t)i * ACC_STRIDE + k] : 0.f;
    float dz = 0.f;
    if constexpr (DEPTH) dz = vis ? acc[(size_t)i * ACC_STRIDE + 9] : 0.f;
    if (vis && (accmask & CSPLAT_SCRATCH_ZEROED)) clear_record(acc, i);      // (consumed: the caller's buffer is all zero again for its next step)
    moments_to_gradients(a9, vis ? g.conic_opacity[i] : make_float4(0.f, 0.f, 0.f, 0.f));
    a9[0] *= (float)cam.W; a9[1] *= (float)cam.H;      // (K7 leaves dL/dmean2D without the pixel <- NDC factors 2 * 0.5 W, 2 * 0.5 H)
    dL_dmean2D[3 * i] = a9[0]; dL_dmean2D[3 * i + 1] = a9[1]; dL_dmean2D[3 * i + 2] = 0.f;
    dL_dconic[4 * i] = a9[2]; dL_dconic[4 * i + 1] = a9[3]; dL_dconic[4 * i + 2] = 0.f; dL_dconic[4 * i + 3] = a9[4];
    if constexpr (!AA) PUT(dL_dopacity, i, a9[5], CSPLAT_ACC_OPACITY);     // (AA: h dL/do', below)
    PUT(dL_dcolor, 3 * i, a9[6], CSPLAT_ACC_COLOR); PUT(dL_dcolor, 3 * i + 1, a9[7], CSPLAT_ACC_COLOR);
    PUT(dL_dcolor, 3 * i + 2, a9[8], CSPLAT_ACC_COLOR);

    float dmean[3] = {0.f, 0.f, 0.f};
    float g6[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (!vis) {
        if constexpr (AA) PUT(dL_dopacity, i, 0.f, CSPLAT_ACC_OPACITY);
#pragma unroll
        for (int k = 0; k < 3; k++) PUT(dL_dmean3D, 3 * i + k, 0.f, CSPLAT_ACC_MEAN3D);
#pragma unroll
        for (int k = 0; k < 6; k++) PUT(dL_dcov3D, 6 * i + k, 0.f, CSPLAT_ACC_COV3D);
        if (dL_dsh && !STAGE) for (int k = 0; k < M * 3; k++) dL_dsh[(size_t)i * M * 3 + k] = 0.f;
        if (dL_dscale) for (int k = 0; k < 3; k++) PUT(dL_dscale, 3 * i + k, 0.f, CSPLAT_ACC_SCALE);
        if (dL_drot) for (int k = 0; k < 4; k++) PUT(dL_drot, 4 * i + k, 0.f, CSPLAT_ACC_ROT);
        if constexpr (CAM) cam_partials_zero(crow);
    } else {
    const float p[3] = {means3D[3 * i], means3D[3 * i + 1], means3D[3 * i + 2]};
    const float *view = cam.view, *proj = cam.proj;

    // ---- conic -> cov2D -> cov3D and view-space mean
    {
        float pv[3];
        view_point(p, view, pv);
        ProjJac pj;
        proj_jacobian(pv, cam, pj);
        float c6[6];
#pragma unroll
        for (int k = 0; k < 6; k++) c6[k] = g.cov3D[6 * i + k];
        float a, b, c;
        float aa_ga = 0.f, aa_gb = 0.f, aa_gc = 0.f;     // (AA) o dL/do' dh/d(a0, b, c0)
        if constexpr (AA) {
            float a0, c0;
            cov2d_undilated(c6, pj, a0, b, c0);
            a = a0 + AA_DILATE; c = c0 + AA_DILATE;
            const float h = aa_backward(a0, b, c0, aa_opacities[i] * a9[5], aa_ga, aa_gb, aa_gc);
            PUT(dL_dopacity, i, h * a9[5], CSPLAT_ACC_OPACITY);
        } else {
            cov2d_from_cov3d(c6, pj, a, b, c);
        }
        const float denom = a * c - b * b;
        const float denom2inv = 1.0f / ((denom * denom) + 0.0000001f);
        const float gcx = a9[2], gcy = a9[3], gcz = a9[4];
        float dL_da = 0.f, dL_db = 0.f, dL_dc = 0.f;
        const float *t0 = pj.t0, *t1 = pj.t1;
        if (denom2inv != 0.f) {
            dL_da = denom2inv * (-c * c * gcx + 2.f * b * c * gcy + (denom - a * c) * gcz);
            dL_dc = denom2inv * (-a * a * gcz + 2.f * a * b * gcy + (denom - a * c) * gcx);
            dL_db = denom2inv * 2.f * (b * c * gcx - (denom + 2.f * b * b) * gcy + a * b * gcz);
            if constexpr (AA) { dL_da += aa_ga; dL_db += aa_gb; dL_dc += aa_gc; }
            g6[0] = t0[0] * t0[0] * dL_da + t0[0] * t1[0] * dL_db + t1[0] * t1[0] * dL_dc;
            g6[3] = t0[1] * t0[1] * dL_da + t0[1] * t1[1] * dL_db + t1[1] * t1[1] * dL_dc;
            g6[5] = t0[2] * t0[2] * dL_da + t0[2] * t1[2] * dL_db + t1[2] * t1[2] * dL_dc;
            g6[1] = 2.f * t0[0] * t0[1] * dL_da + (t0[0] * t1[1] + t0[1] * t1[0]) * dL_db + 2.f * t1[0] * t1[1] * dL_dc;
            g6[2] = 2.f * t0[0] * t0[2] * dL_da + (t0[0] * t1[2] + t0[2] * t1[0]) * dL_db + 2.f * t1[0] * t1[2] * dL_dc;
            g6[4] = 2.f * t0[2] * t0[1] * dL_da + (t0[1] * t1[2] + t0[2] * t1[1]) * dL_db + 2.f * t1[1] * t1[2] * dL_dc;
        }
        const float Vm[3][3] = {{c6[0], c6[1], c6[2]}, {c6[1], c6[3], c6[4]}, {c6[2], c6[4], c6[5]}};
        float dT0[3], dT1[3];
#pragma unroll
        for (int r = 0; r < 3; r++) {
            const float Vt0 = Vm[r][0] * t0[0] + Vm[r][1] * t0[1] + Vm[r][2] * t0[2];
            const float Vt1 = Vm[r][0] * t1[0] + Vm[r][1] * t1[1] + Vm[r][2] * t1[2];
            dT0[r] = 2.f * Vt0 * dL_da + Vt1 * dL_db;
            dT1[r] = 2.f * Vt1 * dL_dc + Vt0 * dL_db;
        }
        const float dJ00 = view[0] * dT0[0] + view[4] * dT0[1] + view[8] * dT0[2];
        const float dJ02 = view[2] * dT0[0] + view[6] * dT0[1] + view[10] * dT0[2];
        const float dJ11 = view[1] * dT1[0] + view[5] * dT1[1] + view[9] * dT1[2];
        const float dJ12 = view[2] * dT1[0] + view[6] * dT1[1] + view[10] * dT1[2];
        const float tz = 1.f / pj.tz, tz2 = tz * tz, tz3 = tz2 * tz;
        const float xg = pj.x_in ? 1.f : 0.f, yg = pj.y_in ? 1.f : 0.f;
        const float dtx = xg * -cam.fx * tz2 * dJ02;
        const float dty = yg * -cam.fy * tz2 * dJ12;
        const float dtz = -cam.fx * tz2 * dJ00 - cam.fy * tz2 * dJ11 + (2.f * cam.fx * pj.tx) * tz3 * dJ02 +
                          (2.f * cam.fy * pj.ty) * tz3 * dJ12;
        dmean[0] += view[0] * dtx + view[1] * dty + view[2] * dtz;
        dmean[1] += view[4] * dtx + view[5] * dty + view[6] * dtz;
        dmean[2] += view[8] * dtx + view[9] * dty + view[10] * dtz;
        if constexpr (CAM) {
            const float dpv[3] = {dtx, dty, dtz + dz};
            cam_partials_view(crow, p, dpv, cam.fx * tz, -(cam.fx * pj.tx) * tz2, cam.fy * tz, -(cam.fy * pj.ty) * tz2, dT0, dT1);
        }
    }
    // ---- mean2D (NDC) -> mean3D
    {
        const float hw = proj[3] * p[0] + proj[7] * p[1] + proj[11] * p[2] + proj[15];
        const float m_w = 1.0f / (hw + 0.0000001f);
        const float mul1 = (proj[0] * p[0] + proj[4] * p[1] + proj[8] * p[2] + proj[12]) * m_w * m_w;
        const float mul2 = (proj[1] * p[0] + proj[5] * p[1] + proj[9] * p[2] + proj[13]) * m_w * m_w;
        const float gx2 = a9[0], gy2 = a9[1];
        dmean[0] += (proj[0] * m_w - proj[3] * mul1) * gx2 + (proj[1] * m_w - proj[3] * mul2) * gy2;
        dmean[1] += (proj[4] * m_w - proj[7] * mul1) * gx2 + (proj[5] * m_w - proj[7] * mul2) * gy2;
        dmean[2] += (proj[8] * m_w - proj[11] * mul1) * gx2 + (proj[9] * m_w - proj[11] * mul2) * gy2;
        if constexpr (CAM) cam_partials_proj(crow, p, gx2 * m_w, gy2 * m_w, -(mul1 * gx2 + mul2 * gy2));
    }
    if constexpr (CAM) { crow[32] = 0.f; crow[33] = 0.f; crow[34] = 0.f; }
    // ---- colour -> SH (+ view direction -> mean3D)
    if (shs && dL_dsh) {
        const float *sh = STAGE ? (const float *)(s_in + threadIdx.x * SH_ROW) : shs + (size_t)i * M * 3;
        float *gsh = STAGE ? s_out + threadIdx.x * SH_ROW : dL_dsh + (size_t)i * M * 3;
        const uint32_t cl = g.clamped[i];
        const float vx = p[0] - cam.campos[0], vy = p[1] - cam.campos[1], vz = p[2] - cam.campos[2];
        const float sum2 = vx * vx + vy * vy + vz * vz;
        const float len = sqrtf(sum2);
        const float x = vx / len, y = vy / len, z = vz / len;
        float ddx = 0.f, ddy = 0.f, ddz = 0.f;
        for (int k = (D + 1) * (D + 1) * 3; k < M * 3; k++) gsh[k] = 0.f;
#pragma unroll
        for (int ch = 0; ch < 3; ch++) {
            const float dRGB = ((cl >> ch) & 1u) ? 0.f : a9[6 + ch];
            float dx_ = 0.f, dy_ = 0.f, dz_ = 0.f;
#define S(k) sh[(k) * 3 + ch]
#define GS(k) gsh[(k) * 3 + ch]
            GS(0) = SH_C0 * dRGB;
            if (D > 0) {
                GS(1) = -SH_C1 * y * dRGB;
                GS(2) = SH_C1 * z * dRGB;
                GS(3) = -SH_C1 * x * dRGB;
                dx_ = -SH_C1 * S(3); dy_ = -SH_C1 * S(1); dz_ = SH_C1 * S(2);
                if (D > 1) {
                    const float xx = x * x, yy = y * y, zz = z * z, xy = x * y, yz = y * z, xz = x * z;
                    GS(4) = SH_C2[0] * xy * dRGB;
                    GS(5) = SH_C2[1] * yz * dRGB;
                    GS(6) = SH_C2[2] * (2.f * zz - xx - yy) * dRGB;
                    GS(7) = SH_C2[3] * xz * dRGB;
                    GS(8) = SH_C2[4] * (xx - yy) * dRGB;
                    dx_ += SH_C2[0] * y * S(4) + SH_C2[2] * 2.f * -x * S(6) + SH_C2[3] * z * S(7) + SH_C2[4] * 2.f * x * S(8);
                    dy_ += SH_C2[0] * x * S(4) + SH_C2[1] * z * S(5) + SH_C2[2] * 2.f * -y * S(6) + SH_C2[4] * 2.f * -y * S(8);
                    dz_ += SH_C2[1] * y * S(5) + SH_C2[2] * 4.f * z * S(6) + SH_C2[3] * x * S(7);
                    if (D > 2) {
                        GS(9) = SH_C3[0] * y * (3.f * xx - yy) * dRGB;
                        GS(10) = SH_C3[1] * xy * z * dRGB;
                        GS(11) = SH_C3[2] * y * (4.f * zz - xx - yy) * dRGB;
                        GS(12) = SH_C3[3] * z * (2.f * zz - 3.f * xx - 3.f * yy) * dRGB;
                        GS(13) = SH_C3[4] * x * (4.f * zz - xx - yy) * dRGB;
                        GS(14) = SH_C3[5] * z * (xx - yy) * dRGB;
                        GS(15) = SH_C3[6] * x * (xx - 3.f * yy) * dRGB;
                        dx_ += SH_C3[0] * S(9) * 6.f * xy + SH_C3[1] * S(10) * yz + SH_C3[2] * S(11) * -2.f * xy +
                               SH_C3[3] * S(12) * -6.f * xz + SH_C3[4] * S(13) * (-3.f * xx + 4.f * zz - yy) +
                               SH_C3[5] * S(14) * 2.f * xz + SH_C3[6] * S(15) * 3.f * (xx - yy);
                        dy_ += SH_C3[0] * S(9) * 3.f * (xx - yy) + SH_C3[1] * S(10) * xz +
                               SH_C3[2] * S(11) * (-3.f * yy + 4.f * zz - xx) + SH_C3[3] * S(12) * -6.f * yz +
                               SH_C3[4] * S(13) * -2.f * xy + SH_C3[5] * S(14) * -2.f * yz + SH_C3[6] * S(15) * -6.f * xy;
                        dz_ += SH_C3[1] * S(10) * xy + SH_C3[2] * S(11) * 8.f * yz +
                               SH_C3[3] * S(12) * 3.f * (2.f * zz - xx - yy) + SH_C3[4] * S(13) * 8.f * xz +
                               SH_C3[5] * S(14) * (xx - yy);
                    }
                }
            }
#undef S
#undef GS
            ddx += dx_ * dRGB; ddy += dy_ * dRGB; ddz += dz_ * dRGB;
        }
        const float invsum32 = 1.0f / sqrtf(sum2 * sum2 * sum2);
        dmean[0] += ((sum2 - vx * vx) * ddx - vy * vx * ddy - vz * vx * ddz) * invsum32;
        dmean[1] += (-vx * vy * ddx + (sum2 - vy * vy) * ddy - vz * vy * ddz) * invsum32;
        dmean[2] += (-vx * vz * ddx - vy * vz * ddy + (sum2 - vz * vz) * ddz) * invsum32;
        if constexpr (CAM) {   // dL/dcampos = -(the direction's part of dL/dmean3D) = -(dd - d (d . dd)) / |m - campos|
            const float dd = x * ddx + y * ddy + z * ddz, il = 1.f / len;
            crow[32] = (x * dd - ddx) * il; crow[33] = (y * dd - ddy) * il; crow[34] = (z * dd - ddz) * il;
        }
    }
    if constexpr (DEPTH) { dmean[0] += dz * view[2]; dmean[1] += dz * view[6]; dmean[2] += dz * view[10]; }
#pragma unroll
    for (int k = 0; k < 3; k++) PUT(dL_dmean3D, 3 * i + k, dmean[k], CSPLAT_ACC_MEAN3D);
#pragma unroll
    for (int k = 0; k < 6; k++) PUT(dL_dcov3D, 6 * i + k, g6[k], CSPLAT_ACC_COV3D);

    // ---- cov3D -> scale, quaternion
    if (!use_precomp_cov && dL_dscale && dL_drot) {
        const float q[4] = {rotations[4 * i], rotations[4 * i + 1], rotations[4 * i + 2], rotations[4 * i + 3]};
        float R[3][3];
        quat_to_rot(q, R);
        const float s[3] = {scale_mod * scales[3 * i], scale_mod * scales[3 * i + 1], scale_mod * scales[3 * i + 2]};
        const float dS[3][3] = {{g6[0], 0.5f * g6[1], 0.5f * g6[2]},
                                {0.5f * g6[1], g6[3], 0.5f * g6[4]},
                                {0.5f * g6[2], 0.5f * g6[4], g6[5]}};
        float dA[3][3];
#pragma unroll
        for (int r = 0; r < 3; r++)
#pragma unroll
            for (int k = 0; k < 3; k++)
                dA[r][k] = 2.f * (dS[r][0] * R[0][k] * s[k] + dS[r][1] * R[1][k] * s[k] + dS[r][2] * R[2][k] * s[k]);
#pragma unroll
        for (int k = 0; k < 3; k++) PUT(dL_dscale, 3 * i + k, dA[0][k] * R[0][k] + dA[1][k] * R[1][k] + dA[2][k] * R[2][k], CSPLAT_ACC_SCALE);
        float dR[3][3];
#pragma unroll
        for (int r = 0; r < 3; r++)
#pragma unroll
            for (int k = 0; k < 3; k++) dR[r][k] = dA[r][k] * s[k];
        const float qr = q[0], qx = q[1], qy = q[2], qz = q[3];
        const float dq0 = 2.f * (-qz * dR[0][1] + qy * dR[0][2] + qz * dR[1][0] - qx * dR[1][2] - qy * dR[2][0] + qx * dR[2][1]);
        const float dq1 = 2.f * (qy * dR[0][1] + qz * dR[0][2] + qy * dR[1][0] - 2.f * qx * dR[1][1] - qr * dR[1][2] +
                                    qz * dR[2][0] + qr * dR[2][1] - 2.f * qx * dR[2][2]);
        const float dq2 = 2.f * (-2.f * qy * dR[0][0] + qx * dR[0][1] + qr * dR[0][2] + qx * dR[1][0] + qz * dR[1][2] -
                                    qr * dR[2][0] + qz * dR[2][1] - 2.f * qy * dR[2][2]);
        const float dq3 = 2.f * (-2.f * qz * dR[0][0] - qr * dR[0][1] + qx * dR[0][2] + qr * dR[1][0] - 2.f * qz * dR[1][1] +
                                    qy * dR[1][2] + qx * dR[2][0] + qy * dR[2][1]);
        PUT(dL_drot, 4 * i, dq0, CSPLAT_ACC_ROT); PUT(dL_drot, 4 * i + 1, dq1, CSPLAT_ACC_ROT);
        PUT(dL_drot, 4 * i + 2, dq2, CSPLAT_ACC_ROT); PUT(dL_drot, 4 * i + 3, dq3, CSPLAT_ACC_ROT);
    }
    }   // visible
    }   // i < P
    if constexpr (CAM) cam_block_sum<NT>(s_cam, rows, s_cpart, cam_slab + (size_t)blockIdx.x * CAM_NC);
    if (STAGE) {   // coalesced 16-byte stores of the workgroup's SH gradients
        __syncthreads();
        float4 *dst4 = reinterpret_cast<float4 *>(dL_dsh + (size_t)blockIdx.x * NT * 48);
        for (int t = threadIdx.x; t < rows * 12; t += NT) {
            const int row = t / 12, c = (t - row * 12) * 4;
            const float *sp = s_out + row * SH_ROW + c;
            float4 o = make_float4(sp[0], sp[1], sp[2], sp[3]);
            if (accmask & CSPLAT_ACC_SH) { const float4 u = dst4[t]; o.x += u.x; o.y += u.y; o.z += u.z; o.w += u.w; }
            dst4[t] = o;
        }
    }
#undef PUT
}
#define CSPLAT_K8_ARGS                                                                                                                 \
    int P, int D, int M, const float *__restrict__ means3D, const float *__restrict__ shs, const float *__restrict__ scales,            \
        float scale_mod, const float *__restrict__ rotations, int use_precomp_cov, Cam cam, Geom g, const int32_t *__restrict__ radii,  \
        const float *__restrict__ acc, float *__restrict__ dL_dmean2D, float *__restrict__ dL_dconic, float *__restrict__ dL_dopacity,  \
        float *__restrict__ dL_dcolor, float *__restrict__ dL_dmean3D, float *__restrict__ dL_dcov3D, float *__restrict__ dL_dsh,      \
        float *__restrict__ dL_dscale, float *__restrict__ dL_drot, unsigned accmask
#define CSPLAT_K8_PASS P, D, M, means3D, shs, scales, scale_mod, rotations, use_precomp_cov, cam, g, radii, acc, dL_dmean2D, dL_dconic, \
                       dL_dopacity, dL_dcolor, dL_dmean3D, dL_dcov3D, dL_dsh, dL_dscale, dL_drot, accmask
template <bool STAGE, int NT>
__global__ __launch_bounds__(NT) void k_preprocess_bwd(CSPLAT_K8_ARGS) { preprocess_bwd_body<STAGE, NT, false>(CSPLAT_K8_PASS); }
template <bool STAGE, int NT>
__global__ __launch_bounds__(NT) void k_preprocess_bwd_depth(CSPLAT_K8_ARGS) { preprocess_bwd_body<STAGE, NT, true>(CSPLAT_K8_PASS); }
template <bool STAGE, int NT, bool DEPTH>
__global__ __launch_bounds__(NT) void k_preprocess_bwd_cam(CSPLAT_K8_ARGS, float *__restrict__ cam_slab) {
    preprocess_bwd_body<STAGE, NT, DEPTH, true>(CSPLAT_K8_PASS, cam_slab);
}
// the antialiased K8 (every combination of the DEPTH / CAM paths; cam_slab NULL without CAM), opacities = the raw o
template <bool STAGE, int NT, bool DEPTH, bool CAM>
__global__ __launch_bounds__(NT) void k_preprocess_bwd_aa(CSPLAT_K8_ARGS, float *__restrict__ cam_slab, const float *__restrict__ opacities) {
    preprocess_bwd_body<STAGE, NT, DEPTH, CAM, true>(CSPLAT_K8_PASS, cam_slab, opacities);
}
#undef CSPLAT_K8_ARGS
#undef CSPLAT_K8_PASS

// K8 for ALL views of a step in one launch (csplat_backward_views).  The per-view kernels above add into shared gradient
// buffers and therefore run one after the other behind the concurrent K7s (a tail of ~27 us per view).  Here a thread
// keeps its Gaussian and loops over the views: inputs and SH rows are read once, gradients of parameters that all views
// share are summed in registers (SH: across the quad, see the body) and written once, per-view outputs (mean2D, conic, and mean3D /
// rotation when every view has its own deformed copy) are written per view.  Same arithmetic per view as k_preprocess_bwd.
constexpr int K8_MAX_VIEWS = RASTER_MAX_VIEWS;      // (the name csplat_k8_views_body.h sizes its LDS rows with)
struct K8View {
    Cam cam;
    Geom g;
    const int32_t *radii;
    const float *acc, *means3D, *rotations;
    float *dL_dmean2D, *dL_dconic, *dL_dopacity, *dL_dcolor, *dL_dmean3D, *dL_dcov3D, *dL_dscale, *dL_drot;
    unsigned accmask;
};
struct K8Table {
    int n;
    unsigned sharedmask;   // CSPLAT_ACC_* bits of the outputs whose buffer is the same in every view
    unsigned unread;       // != 0: every view carries CSPLAT_K8_OUTPUTS_UNREAD -- dL_dconic, dL_dcolor and dL_dcov3D are not stored
    const uint32_t *valid; // (csplat_forward_views_faith) 0 there: the forward left the views untouched -- nothing to differentiate
    K8View v[RASTER_MAX_VIEWS];
};

// VL lanes per Gaussian, lane vl takes the views vl, vl + VL, ...: with one lane per Gaussian the launch has P / 64 = 1564 waves (1.5 per
// SIMD) that each walk V dependent load -> compute rounds; with VL = 4 it has four times the waves and (V <= 4) one round each.  The
// sums over the views of the shared-parameter gradients cross the VL lanes with quad DPP adds (fixed association); for the SH gradient
// the lanes exchange (direction, dRGB) by DPP and each forms and stores a quarter of the Gaussian's row.
// The batched K8's body lives in csplat_k8_views_body.h and is included into both kernels below, so that the default kernel is compiled
// exactly as before (a shared __device__ body changed its register allocation).  DEPTH: k_preprocess_bwd_views_depth, the depth-gradient
// path -- every view's record slot 9 (dL/dz, zero for a view without a depth gradient) adds dL/dz (view[2], view[6], view[10]) to dL/dmean3D.
// CAM: k_preprocess_bwd_views_cam<.., DEPTH>, the camera-gradient path -- per view, one slab row per workgroup (CamSlabs, see
// cam_partials_view): the lanes of a quad hold different views, so the partials go to LDS rows [view][Gaussian] and only rows of one view
// are summed together.
struct CamSlabs {
    float *p[RASTER_MAX_VIEWS];   // per view: the slab (rows of CAM_NC floats, one per workgroup)
};
template <int NT, int VL, bool UNREAD>
__global__ __launch_bounds__(NT, UNREAD ? 4 : 3) void k_preprocess_bwd_views(int P, int D, int M, const float *__restrict__ shs,
                                                               const float *__restrict__ scales, float scale_mod,
                                                               int use_precomp_cov, float *__restrict__ dL_dsh, K8Table tab, int block0) {
    constexpr bool DEPTH = false, CAM = false, AA = false, STAMP = false;
    unsigned long long *const stamp_buf = nullptr;
    (void)stamp_buf;
    const CamSlabs *const cam_slabs = nullptr;
    const float *const aa_opacities = nullptr;
    (void)aa_opacities;
#include "csplat_k8_views_body.h"
}
// (the flagship form, k_preprocess_bwd_views<NT, VL, true>, with s_memtime stamps: the measurement hook of csplat_debug_stamps)
template <int NT, int VL>
__global__ __launch_bounds__(NT, 4) void k_preprocess_bwd_views_stamps(int P, int D, int M, const float *__restrict__ shs,
                                                                        const float *__restrict__ scales, float scale_mod,
                                                                        int use_precomp_cov, float *__restrict__ dL_dsh, K8Table tab, int block0,
                                                                        unsigned long long *stamp_buf) {
    constexpr bool DEPTH = false, CAM = false, AA = false, UNREAD = true, STAMP = true;
    const CamSlabs *const cam_slabs = nullptr;
    const float *const aa_opacities = nullptr;
    (void)aa_opacities;
#include "csplat_k8_views_body.h"
}
template <int NT, int VL>
__global__ __launch_bounds__(NT) void k_preprocess_bwd_views_depth(int P, int D, int M, const float *__restrict__ shs,
                                                                     const float *__restrict__ scales, float scale_mod,
                                                                     int use_precomp_cov, float *__restrict__ dL_dsh, K8Table tab, int block0) {
    constexpr bool DEPTH = true, CAM = false, AA = false, UNREAD = false, STAMP = false;
    unsigned long long *const stamp_buf = nullptr;
    (void)stamp_buf;
    const CamSlabs *const cam_slabs = nullptr;
    const float *const aa_opacities = nullptr;
    (void)aa_opacities;
#include "csplat_k8_views_body.h"
}
template <int NT, int VL, bool DEPTH>
__global__ __launch_bounds__(NT) void k_preprocess_bwd_views_cam(int P, int D, int M, const float *__restrict__ shs,
                                                                   const float *__restrict__ scales, float scale_mod,
                                                                   int use_precomp_cov, float *__restrict__ dL_dsh, K8Table tab, int block0,
                                                                   CamSlabs slabs) {
    constexpr bool CAM = true, AA = false, UNREAD = false, STAMP = false;
    unsigned long long *const stamp_buf = nullptr;
    (void)stamp_buf;
    const CamSlabs *const cam_slabs = &slabs;
    const float *const aa_opacities = nullptr;
    (void)aa_opacities;
#include "csplat_k8_views_body.h"
}
// AA: the antialiased batched K8 on any of the paths above (slabs used with CAM only); opacities = the raw o every view shares
template <int NT, int VL, bool DEPTH, bool CAM>
__global__ __launch_bounds__(NT) void k_preprocess_bwd_views_aa(int P, int D, int M, const float *__restrict__ shs,
                                                                  const float *__restrict__ scales, float scale_mod,
                                                                  int use_precomp_cov, float *__restrict__ dL_dsh, K8Table tab, int block0,
                                                                  CamSlabs slabs, const float *__restrict__ opacities) {
    constexpr bool AA = true, UNREAD = false, STAMP = false;
    unsigned long long *const stamp_buf = nullptr;
    (void)stamp_buf;
    const CamSlabs *const cam_slabs = &slabs;
    const float *const aa_opacities = opacities;
    (void)cam_slabs;
#include "csplat_k8_views_body.h"
}

// ---- the fixed-order sums of the camera path.  dL/dbg_c = sum_pix dL/dC_c(pix) T_final(pix) (the depth image has no background term):
// k_bg_partials writes one row of 3 per (pixel block, view), BG_BLOCKS contiguous pixel ranges per view.  k_cam_sum then sums, per view,
// the K8 slab (rows of CAM_NC) and the background slab (rows of 3) in index order: thread t takes rows t, t + 256, ..., and the 256
// partial rows meet in a fixed LDS tree.
constexpr int BG_BLOCKS = 256;
struct BgView {
    const float *final_T, *dL_dpix;
    float *slab;           // NULL: the view takes no background gradient
    int npix;
};
struct BgTable {
    BgView v[RASTER_MAX_VIEWS];
};
__global__ __launch_bounds__(256) void k_bg_partials(BgTable tab) {
    const BgView w = tab.v[blockIdx.y];
    if (!w.slab) return;
    const int64_t n = w.npix, lo = n * blockIdx.x / BG_BLOCKS, hi = n * (blockIdx.x + 1) / BG_BLOCKS;
    float a[3] = {0.f, 0.f, 0.f};
    for (int64_t q = lo + threadIdx.x; q < hi; q += 256) {
        const float T = w.final_T ? w.final_T[q] : 1.f;      // (no image chunk: a view without Gaussians is all background)
        a[0] += w.dL_dpix[q] * T; a[1] += w.dL_dpix[n + q] * T; a[2] += w.dL_dpix[2 * n + q] * T;
    }
    __shared__ float s[3][256];
#pragma unroll
    for (int c = 0; c < 3; c++) s[c][threadIdx.x] = a[c];
    for (int st = 128; st > 0; st >>= 1) {
        __syncthreads();
        if ((int)threadIdx.x < st)
#pragma unroll
            for (int c = 0; c < 3; c++) s[c][threadIdx.x] += s[c][threadIdx.x + st];
    }
    if (threadIdx.x < 3) w.slab[blockIdx.x * 3 + threadIdx.x] = s[threadIdx.x][0];
}
struct CamSumView {
    const float *slab, *bg_slab;    // K8 slab (rows of CAM_NC), background slab (rows of 3; NULL: no background gradient)
    int rows, bg_rows;
    float *dL_dview, *dL_dproj, *dL_dcampos, *dL_dbg;   // each may be NULL
};
struct CamSumTable {
    CamSumView v[RASTER_MAX_VIEWS];
};
// columns [0, NC) of rows [0, rows) summed in a fixed order; the result is left in s[0 .. NC) (s: 256 x NC floats of LDS)
template <int NC>
__device__ __forceinline__ void slab_sum(const float *slab, int rows, float *s) {
    float a[NC];
#pragma unroll
    for (int c = 0; c < NC; c++) a[c] = 0.f;
    for (int r = threadIdx.x; r < rows; r += 256)
#pragma unroll
        for (int c = 0; c < NC; c++) a[c] += slab[(size_t)r * NC + c];
    __syncthreads();
#pragma unroll
    for (int c = 0; c < NC; c++) s[threadIdx.x * NC + c] = a[c];
    for (int st = 128; st > 0; st >>= 1) {
        __syncthreads();
        if ((int)threadIdx.x < st)
#pragma unroll
            for (int c = 0; c < NC; c++) s[threadIdx.x * NC + c] += s[(threadIdx.x + st) * NC + c];
    }
    __syncthreads();
}
__global__ __launch_bounds__(256) void k_cam_sum(CamSumTable tab) {
    const CamSumView w = tab.v[blockIdx.y];
    __shared__ float s[256 * CAM_NC];
    const int t = threadIdx.x;
    if (w.dL_dview || w.dL_dproj || w.dL_dcampos) {
        slab_sum<CAM_NC>(w.slab, w.rows, s);
        if (w.dL_dview && t < 16) w.dL_dview[t] = s[t];
        if (w.dL_dproj && t < 16) w.dL_dproj[t] = s[16 + t];
        if (w.dL_dcampos && t < 3) w.dL_dcampos[t] = s[32 + t];
    }
    if (w.dL_dbg) {
        slab_sum<3>(w.bg_slab, w.bg_rows, s);
        if (t < 3) w.dL_dbg[t] = s[t];
    }
}

}  // namespace
