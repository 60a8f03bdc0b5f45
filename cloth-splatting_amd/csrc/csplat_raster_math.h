// csplat_raster_math.h -- part of csplat_raster.hip, included there once, first of its parts (the inventory at the top of that file lists
// them in order); not a header of its own: it compiles only inside that translation unit, behind csplat_common.h.
// What every stage shares: the constants, Geom / Cam / ProjJac, the quaternion -> cov3D -> cov2D chain with its antialiasing helpers,
// tile_rect and the SH row staging.  Uses nothing of another part.
#pragma once

namespace {

constexpr float NEAR_Z = 0.2f;
// views per batched launch: every per-view table a kernel takes by value (K1Table, P2Table, B2Table, K8Table, ...) holds this many, and the
// host cuts larger calls into groups of at most this many (view_groups)
constexpr int RASTER_MAX_VIEWS = 8;

__device__ constexpr float SH_C0 = 0.28209479177387814f;
__device__ constexpr float SH_C1 = 0.4886025119029199f;
__device__ constexpr float SH_C2[5] = {1.0925484305920792f, -1.0925484305920792f, 0.31539156525252005f,
                                       -1.0925484305920792f, 0.5462742152960396f};
__device__ constexpr float SH_C3[7] = {-0.5900435899266435f, 2.890611442640554f, -0.4570457994644658f,
                                       0.3731763325901154f, -0.4570457994644658f, 1.445305721320277f,
                                       -0.5900435899266435f};

struct Geom {
    float *depth;           // [P]
    float2 *xy;             // [P]
    float4 *conic_opacity;  // [P]
    float *rgb;             // [P][3]
    float *cov3D;           // [P][6]
    uint32_t *clamped;      // [P] bit c
    uint32_t *tiles_touched;// [P]
    uint32_t *offsets;      // [P] inclusive scan
    float *cut2;            // [P] squared cut-off distance for wave-level culling (see box_hit)
    void *scan_tmp;
    float4 *pack;           // [P][3] (x, y, conic a, conic b | conic c, opacity, r, g | b, depth, cut2, 0): what k_block_masks needs of a
                            // Gaussian in ONE 48-byte record -- it visits the Gaussians in list order (a random gather per field otherwise)
};

struct Cam {
    const float *view;    // device, 16 floats (transposed world->view)
    const float *proj;    // device, 16 floats (transposed full projection)
    const float *campos;  // device, 3 floats
    float tanfovx, tanfovy, fx, fy;
    int W, H, gx, gy;
};

struct ProjJac {
    float t0[3], t1[3];
    float tx, ty, tz;
    bool x_in, y_in;
};

__device__ __forceinline__ void quat_to_rot(const float *q, float R[3][3]) {
#pragma clang fp contract(off)
    float r = q[0], x = q[1], y = q[2], z = q[3];
    R[0][0] = 1.f - 2.f * (y * y + z * z);
    R[0][1] = 2.f * (x * y - r * z);
    R[0][2] = 2.f * (x * z + r * y);
    R[1][0] = 2.f * (x * y + r * z);
    R[1][1] = 1.f - 2.f * (x * x + z * z);
    R[1][2] = 2.f * (y * z - r * x);
    R[2][0] = 2.f * (x * z - r * y);
    R[2][1] = 2.f * (y * z + r * x);
    R[2][2] = 1.f - 2.f * (x * x + y * y);
}

__device__ __forceinline__ void cov3d_from_scale_rot(const float *scale, float mod, const float *q, float *c6) {
#pragma clang fp contract(off)
    float R[3][3], m[3][3];
    quat_to_rot(q, R);
#pragma unroll
    for (int k = 0; k < 3; k++) {
        float s = mod * scale[k];
#pragma unroll
        for (int i = 0; i < 3; i++) m[k][i] = s * R[i][k];
    }
    c6[0] = m[0][0] * m[0][0] + m[1][0] * m[1][0] + m[2][0] * m[2][0];
    c6[1] = m[0][0] * m[0][1] + m[1][0] * m[1][1] + m[2][0] * m[2][1];
    c6[2] = m[0][0] * m[0][2] + m[1][0] * m[1][2] + m[2][0] * m[2][2];
    c6[3] = m[0][1] * m[0][1] + m[1][1] * m[1][1] + m[2][1] * m[2][1];
    c6[4] = m[0][1] * m[0][2] + m[1][1] * m[1][2] + m[2][1] * m[2][2];
    c6[5] = m[0][2] * m[0][2] + m[1][2] * m[1][2] + m[2][2] * m[2][2];
}

__device__ __forceinline__ void view_point(const float *p, const float *V, float *o) {
#pragma clang fp contract(off)
    o[0] = V[0] * p[0] + V[4] * p[1] + V[8] * p[2] + V[12];
    o[1] = V[1] * p[0] + V[5] * p[1] + V[9] * p[2] + V[13];
    o[2] = V[2] * p[0] + V[6] * p[1] + V[10] * p[2] + V[14];
}

__device__ __forceinline__ void proj_jacobian(const float *pv, const Cam &c, ProjJac &o) {
#pragma clang fp contract(off)
    const float limx = 1.3f * c.tanfovx, limy = 1.3f * c.tanfovy;
    const float tz = pv[2];
    const float txtz = pv[0] / tz, tytz = pv[1] / tz;
    o.x_in = !(txtz < -limx || txtz > limx);
    o.y_in = !(tytz < -limy || tytz > limy);
    const float tx = fminf(limx, fmaxf(-limx, txtz)) * tz;
    const float ty = fminf(limy, fmaxf(-limy, tytz)) * tz;
    const float J00 = c.fx / tz, J02 = -(c.fx * tx) / (tz * tz);
    const float J11 = c.fy / tz, J12 = -(c.fy * ty) / (tz * tz);
#pragma unroll
    for (int a = 0; a < 3; a++) {
        o.t0[a] = c.view[4 * a + 0] * J00 + c.view[4 * a + 2] * J02;
        o.t1[a] = c.view[4 * a + 1] * J11 + c.view[4 * a + 2] * J12;
    }
    o.tx = tx; o.ty = ty; o.tz = tz;
}

__device__ __forceinline__ void cov2d_from_cov3d(const float *c6, const ProjJac &pj, float &a, float &b, float &c) {
#pragma clang fp contract(off)
    const float *t0 = pj.t0, *t1 = pj.t1;
    const float Vm[3][3] = {{c6[0], c6[1], c6[2]}, {c6[1], c6[3], c6[4]}, {c6[2], c6[4], c6[5]}};
    float u0[3], u1[3];
#pragma unroll
    for (int j = 0; j < 3; j++) {
        u0[j] = t0[0] * Vm[0][j] + t0[1] * Vm[1][j] + t0[2] * Vm[2][j];
        u1[j] = t1[0] * Vm[0][j] + t1[1] * Vm[1][j] + t1[2] * Vm[2][j];
    }
    a = (u0[0] * t0[0] + u0[1] * t0[1] + u0[2] * t0[2]) + 0.3f;
    b = u0[0] * t1[0] + u0[1] * t1[1] + u0[2] * t1[2];
    c = (u1[0] * t1[0] + u1[1] * t1[1] + u1[2] * t1[2]) + 0.3f;
}

// ---- antialiasing (csplat_view.prefiltered & CSPLAT_ANTIALIAS): the opacity is scaled by the ratio of the footprint areas of the
// undilated and the dilated cov2D, o' = o h with h = sqrt(max(2.5e-5, det0 / det1)).  (a0, b, c0) = T Sigma T^T without the 0.3 px^2
// dilation: the same sums cov2d_from_cov3d forms before it adds 0.3, so a0 + 0.3f / c0 + 0.3f are its a / c bit for bit.  K1 and K8
// form h with these helpers (contraction off), so both see the same h.
__device__ __forceinline__ void cov2d_undilated(const float *c6, const ProjJac &pj, float &a0, float &b, float &c0) {
#pragma clang fp contract(off)
    const float *t0 = pj.t0, *t1 = pj.t1;
    const float Vm[3][3] = {{c6[0], c6[1], c6[2]}, {c6[1], c6[3], c6[4]}, {c6[2], c6[4], c6[5]}};
    float u0[3], u1[3];
#pragma unroll
    for (int j = 0; j < 3; j++) {
        u0[j] = t0[0] * Vm[0][j] + t0[1] * Vm[1][j] + t0[2] * Vm[2][j];
        u1[j] = t1[0] * Vm[0][j] + t1[1] * Vm[1][j] + t1[2] * Vm[2][j];
    }
    a0 = u0[0] * t0[0] + u0[1] * t0[1] + u0[2] * t0[2];
    b = u0[0] * t1[0] + u0[1] * t1[1] + u0[2] * t1[2];
    c0 = u1[0] * t1[0] + u1[1] * t1[1] + u1[2] * t1[2];
}
constexpr float AA_DILATE = 0.3f, AA_FLOOR = 2.5e-5f;
// h of (a0, b, c0); det1 = (a0 + 0.3)(c0 + 0.3) - b^2 is the determinant K1 inverts for the conic
__device__ __forceinline__ float aa_factor(float a0, float b, float c0) {
#pragma clang fp contract(off)
    const float det0 = a0 * c0 - b * b;
    const float det1 = (a0 + AA_DILATE) * (c0 + AA_DILATE) - b * b;
    return sqrtf(fmaxf(AA_FLOOR, det0 / det1));
}
// K8: g = o dL/do' (the raw opacity times the opacity moment M0); adds g dh/d(a0, b, c0) to (ga, gb, gc) -- b is the one scalar
// off-diagonal entry, as in dL_db.  With f = det0 / det1, w = 0.3: df/da0 = w (c0^2 + w c0 + b^2) / det1^2, df/dc0 = w (a0^2 + w a0 + b^2)
// / det1^2, df/db = -2 w b (a0 + c0 + w) / det1^2, dh = df / (2 h); nothing where the floor is active.  Returns h.
__device__ __forceinline__ float aa_backward(float a0, float b, float c0, float g, float &ga, float &gb, float &gc) {
#pragma clang fp contract(off)
    const float det0 = a0 * c0 - b * b;
    const float det1 = (a0 + AA_DILATE) * (c0 + AA_DILATE) - b * b;
    const float f = det0 / det1;
    const float h = sqrtf(fmaxf(AA_FLOOR, f));
    if (f > AA_FLOOR) {
        const float k = g * AA_DILATE / (2.f * h * det1 * det1);
        ga += k * (c0 * c0 + AA_DILATE * c0 + b * b);
        gc += k * (a0 * a0 + AA_DILATE * a0 + b * b);
        gb += k * (-2.f * b * (a0 + c0 + AA_DILATE));
    }
    return h;
}

__device__ __forceinline__ void tile_rect(float px, float py, int rad, const Cam &c, int &minx, int &miny, int &maxx,
                                          int &maxy) {
#pragma clang fp contract(off)
    minx = min(c.gx, max(0, (int)((px - (float)rad) / (float)CSPLAT_TILE)));
    miny = min(c.gy, max(0, (int)((py - (float)rad) / (float)CSPLAT_TILE)));
    maxx = min(c.gx, max(0, (int)((px + (float)rad + (float)(CSPLAT_TILE - 1)) / (float)CSPLAT_TILE)));
    maxy = min(c.gy, max(0, (int)((py + (float)rad + (float)(CSPLAT_TILE - 1)) / (float)CSPLAT_TILE)));
}

// SH coefficients are 48 floats (192 B) per Gaussian: read lane-per-Gaussian that is a 192-byte stride.  With STAGE the
// workgroup first copies its 256 x 48 contiguous floats into LDS with 16-byte coalesced loads (row stride 49 floats:
// conflict-free column reads) and the per-Gaussian code reads LDS instead.
constexpr int SH_ROW = 49;

template <int NT>
__device__ __forceinline__ void stage_sh_rows(const float *__restrict__ src, int rows, float *s_rows) {
    const float4 *src4 = reinterpret_cast<const float4 *>(src);
    for (int t = threadIdx.x; t < rows * 12; t += NT) {
        const float4 v = src4[t];
        const int row = t / 12, c = (t - row * 12) * 4;
        float *d = s_rows + row * SH_ROW + c;
        d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
    }
}

}  // namespace
