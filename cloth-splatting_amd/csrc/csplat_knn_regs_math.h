// csplat_knn_regs_math.h -- the per-pair arithmetic of the kNN-graph regularisers (include/csplat.h: csplat_knn_regs_fwd / _bwd).
// Plain float functions with FP contraction off, shared by the forward and the backward kernel so that both see the same bits.
// Quaternions are (w, x, y, z) in a float[4].
#pragma once
#include <math.h>

#ifndef KR_FN
#define KR_FN __host__ __device__ __forceinline__
#endif

KR_FN float kr_len(const float o[3]) {
#pragma clang fp contract(off)
    return sqrtf((o[0] * o[0] + o[1] * o[1]) + o[2] * o[2]);
}

KR_FN float kr_sign(float x) { return (float)((x > 0.f) - (x < 0.f)); }

// Hamilton product
KR_FN void kr_qmul(const float p[4], const float q[4], float r[4]) {
#pragma clang fp contract(off)
    r[0] = ((p[0] * q[0] - p[1] * q[1]) - p[2] * q[2]) - p[3] * q[3];
    r[1] = ((p[0] * q[1] + p[1] * q[0]) + p[2] * q[3]) - p[3] * q[2];
    r[2] = ((p[0] * q[2] - p[1] * q[3]) + p[2] * q[0]) + p[3] * q[1];
    r[3] = ((p[0] * q[3] + p[1] * q[2]) - p[2] * q[1]) + p[3] * q[0];
}

KR_FN void kr_conj(const float q[4], float c[4]) { c[0] = q[0]; c[1] = -q[1]; c[2] = -q[2]; c[3] = -q[3]; }

// r = a (x) conj(b), n = r / |r|, R = rotmat(n) (row-major)
struct KrRot { float n[4], nrm, R[9]; };

KR_FN void kr_rot(const float a[4], const float b[4], KrRot &k) {
#pragma clang fp contract(off)
    float c[4], r[4];
    kr_conj(b, c);
    kr_qmul(a, c, r);
    k.nrm = sqrtf(((r[0] * r[0] + r[1] * r[1]) + r[2] * r[2]) + r[3] * r[3]);
    for (int m = 0; m < 4; m++) k.n[m] = r[m] / k.nrm;
    const float w = k.n[0], x = k.n[1], y = k.n[2], z = k.n[3];
    k.R[0] = 1.f - 2.f * (y * y + z * z); k.R[1] = 2.f * (x * y - w * z);       k.R[2] = 2.f * (x * z + w * y);
    k.R[3] = 2.f * (x * y + w * z);       k.R[4] = 1.f - 2.f * (x * x + z * z); k.R[5] = 2.f * (y * z - w * x);
    k.R[6] = 2.f * (x * z - w * y);       k.R[7] = 2.f * (y * z + w * x);       k.R[8] = 1.f - 2.f * (x * x + y * y);
}

// e = R off - prev; returns sqrt(w |e|^2 + 1e-20)
KR_FN float kr_rigid_value(const float R[9], const float off[3], const float prev[3], float w, float e[3]) {
#pragma clang fp contract(off)
    for (int a = 0; a < 3; a++) e[a] = ((R[3 * a] * off[0] + R[3 * a + 1] * off[1]) + R[3 * a + 2] * off[2]) - prev[a];
    const float s = (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2];
    return sqrtf(s * w + 1e-20f);
}

// the adjoint of (a, b) -> R for a given dL/dR = u off^T: da, db are ADDED to
KR_FN void kr_rot_adjoint(const float a[4], const float b[4], const KrRot &k, const float u[3], const float off[3], float da[4], float db[4]) {
#pragma clang fp contract(off)
    float G[9];
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) G[3 * r + c] = u[r] * off[c];
    const float w = k.n[0], x = k.n[1], y = k.n[2], z = k.n[3];
    float dn[4];
    dn[0] = 2.f * (((z * (G[3] - G[1])) + (y * (G[2] - G[6]))) + (x * (G[7] - G[5])));
    dn[1] = 2.f * ((((y * (G[1] + G[3])) + (z * (G[2] + G[6]))) + (w * (G[7] - G[5]))) - 2.f * (x * (G[4] + G[8])));
    dn[2] = 2.f * ((((x * (G[1] + G[3])) + (z * (G[5] + G[7]))) + (w * (G[2] - G[6]))) - 2.f * (y * (G[0] + G[8])));
    dn[3] = 2.f * ((((x * (G[2] + G[6])) + (y * (G[5] + G[7]))) + (w * (G[3] - G[1]))) - 2.f * (z * (G[0] + G[4])));
    // through n = r / |r|
    const float dot = ((k.n[0] * dn[0] + k.n[1] * dn[1]) + k.n[2] * dn[2]) + k.n[3] * dn[3];
    float dr[4];
    for (int m = 0; m < 4; m++) dr[m] = (dn[m] - k.n[m] * dot) / k.nrm;
    // r = a (x) conj(b):  da = dr (x) b,   d conj(b) = conj(a) (x) dr
    float t[4], ca[4];
    kr_qmul(dr, b, t);
    for (int m = 0; m < 4; m++) da[m] += t[m];
    kr_conj(a, ca);
    kr_qmul(ca, dr, t);
    db[0] += t[0]; db[1] -= t[1]; db[2] -= t[2]; db[3] -= t[3];
}

struct KrCoef { float iso, spring, rigid; int iso_abs; };     // the three weights times the upstream gradient over the terms' counts

// dL/d off_t of ONE pair (node i, neighbour j, rest length d0, weight w) at time row t, into f[3]; with dq != nullptr the pair's
// share of dL/dQ[t][j] is ADDED to dq[4].  M [T,N,3]; Q [T,N,4] (read only when c.rigid != 0).
KR_FN void kr_pair_row_grad(int T, int t, int N, int i, int j, float d0, float w, const float *__restrict__ M, const float *__restrict__ Q,
                            const KrCoef &c, float f[3], float *dq) {
#pragma clang fp contract(off)
    const float *mi = M + ((size_t)t * N + i) * 3, *mj = M + ((size_t)t * N + j) * 3;
    const size_t row = (size_t)N * 3;
    float off[3], prev[3], next[3];
    for (int a = 0; a < 3; a++) off[a] = mj[a] - mi[a];
    const float d = kr_len(off);
    float s = c.iso * (c.iso_abs ? kr_sign(d - d0) : 1.f);
    const bool has_prev = t >= 1, has_next = t + 1 < T;
    if (has_prev) {
        for (int a = 0; a < 3; a++) prev[a] = (mj - row)[a] - (mi - row)[a];
        if (c.spring != 0.f) s += c.spring * kr_sign(d - kr_len(prev));
    }
    if (has_next) {
        for (int a = 0; a < 3; a++) next[a] = (mj + row)[a] - (mi + row)[a];
        if (c.spring != 0.f) s -= c.spring * kr_sign(kr_len(next) - d);
    }
    for (int a = 0; a < 3; a++) f[a] = d > 0.f ? s * (off[a] / d) : 0.f;
    if (c.rigid == 0.f) return;
    const float4 *q4 = reinterpret_cast<const float4 *>(Q);
    const float4 qt = q4[(size_t)t * N + j];
    const float b[4] = {qt.x, qt.y, qt.z, qt.w};
    KrRot k;
    float e[3], u[3];
    if (has_prev) {                              // the term of rows (t-1, t): off_t is rotated, Q[t][j] is the conjugated factor
        const float4 qp = q4[(size_t)(t - 1) * N + j];
        const float a_[4] = {qp.x, qp.y, qp.z, qp.w};
        kr_rot(a_, b, k);
        const float v = kr_rigid_value(k.R, off, prev, w, e);
        const float kk = c.rigid * w / v;
        for (int a = 0; a < 3; a++) u[a] = kk * e[a];
        for (int a = 0; a < 3; a++) f[a] += (k.R[a] * u[0] + k.R[3 + a] * u[1]) + k.R[6 + a] * u[2];
        if (dq) {
            float da[4] = {0.f, 0.f, 0.f, 0.f};
            kr_rot_adjoint(a_, b, k, u, off, da, dq);
        }
    }
    if (has_next) {                              // the term of rows (t, t+1): off_t is the subtracted one, Q[t][j] the left factor
        const float4 qn = q4[(size_t)(t + 1) * N + j];
        const float b_[4] = {qn.x, qn.y, qn.z, qn.w};
        kr_rot(b, b_, k);
        const float v = kr_rigid_value(k.R, next, off, w, e);
        const float kk = c.rigid * w / v;
        for (int a = 0; a < 3; a++) u[a] = kk * e[a];
        for (int a = 0; a < 3; a++) f[a] -= u[a];
        if (dq) {
            float db[4] = {0.f, 0.f, 0.f, 0.f};
            kr_rot_adjoint(b, b_, k, u, next, dq, db);
        }
    }
}
