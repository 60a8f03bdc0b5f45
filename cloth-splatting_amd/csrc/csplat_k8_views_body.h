// Body of the batched per-Gaussian backward (K8 of csplat_backward_views), included by csplat_raster.hip into k_preprocess_bwd_views
// (DEPTH = false), k_preprocess_bwd_views_depth (DEPTH = true), k_preprocess_bwd_views_cam (CAM = true) and k_preprocess_bwd_views_aa
// (AA = true: antialiasing, see preprocess_bwd_body).  Not a standalone header: it expects the kernels' parameters, constexpr bools DEPTH,
// CAM, AA, STAMP (with an `unsigned long long *stamp_buf`) and UNREAD (the caller reads no dL_dconic / dL_dcolor / dL_dcov3D, known at compile time: the default kernel's second
// instantiation, which then drops their nine running sums from the view loop), a `const CamSlabs *cam_slabs` and a `const float *aa_opacities` (the raw opacities when AA) in scope.
    constexpr bool STAGE = true;
    if (tab.valid && *tab.valid == 0u) return;
    // (block0: first workgroup of a Gaussian-range SLICE of the launch -- csplat_backward_views_parts: the gradient rows of a finished slice
    //  can leave for the other ranks while the next slice computes)
    const int bx = (int)blockIdx.x + block0;
    const unsigned smask = tab.sharedmask;
    // CSPLAT_K8_OUTPUTS_UNREAD on every view: dL_dconic, dL_dcolor and dL_dcov3D are not stored (wave-uniform, from the kernel argument)
    const bool put3 = !UNREAD && tab.unread == 0u;
    // shared output: add to the thread's running sum; per-view output: write (or add, by that view's accmask)
#define PUTL(local, ptr, idx, val, bit)                                                    \
    do {                                                                                   \
        if (smask & (bit)) (local) += (val);                                               \
        else { float *p_ = (ptr) + (idx); *p_ = (accmask & (bit)) ? *p_ + (val) : (val); } \
    } while (0)
    static_assert(VL == 4 && K8_MAX_VIEWS <= 2 * VL, "one quad per Gaussian, at most two views per lane");
    constexpr int NG = NT / VL;                   // Gaussians per workgroup
    __shared__ float s_in[STAGE ? NG * SH_ROW : 1];
    __shared__ float s_cam[CAM ? K8_MAX_VIEWS * NG * CAM_NC : 1];     // (CAM) [view][Gaussian of the workgroup][CAM_NC]
    __shared__ float s_cpart[CAM ? CAM_PARTS * CAM_NC : 1];
    const int gi = threadIdx.x / VL, vl = threadIdx.x % VL;
    const int i = bx * NG + gi;
    const int rows = min(NG, P - bx * NG);
    if (tab.n <= 0) return;
    // (STAMP: k_preprocess_bwd_views_stamps, see StampMark -- words 0..5 of the workgroup's 8 = entry, behind the staging barrier, the record
    //  arrived, the conic arrived, the last of the visible branch's inputs arrived, the last store issued; the last four where thread 0 got there)
    auto mark = [&](int k, float dep) {
        if constexpr (STAMP) StampMark{stamp_buf + (size_t)bx * 8}(k, dep);
    };
    mark(0, 0.f);
    // ---- Every global load of the lane's first view is issued here, unconditionally and in front of the SH staging loads: all of a wave's
    // loads travel in ONE memory round trip.  (Read where they are used -- the staging barrier, then the radius and the record, then the conic
    // behind the radius, then the visible branch's means3D / cov3D / clamped / rotations / scales -- they were four dependent round trips.)
    // Visibility only SELECTS among what arrived: a culled Gaussian's values are never used, so its gradients stay exactly 0 whatever was
    // loaded.  A lane past P requests the last Gaussian's values, a lane without a view (V < 4) the last view's: valid addresses, dropped.
    struct ViewIn {
        float4 co;      // g.conic_opacity[i]
        float c6[6];    // g.cov3D[6 i ..]
        float p[3];     // means3D[3 i ..]
        uint32_t cl;    // g.clamped[i]                 (read only when the SH gradient is wanted)
        float q[4];     // rotations[4 i ..]            (read only when the view's pointer is set and cov3D is not precomputed)
    };
    const bool want_sh = shs && dL_dsh;
    // (the view's pointers are read from the table first, all of them, and no load below is conditional: a pointer fetched or a branch taken
    //  between two of these loads would make the later one wait for the earlier.  Where the rotations are not read -- no pointer, or a
    //  precomputed cov3D -- the four words come from the start of the conic array, which is always there, and are never used.)
    auto load_view_inputs = [&](const K8View &w_, int i_, ViewIn &o) {
        const float4 *co_ = w_.g.conic_opacity;
        const float *c6_ = w_.g.cov3D, *m3_ = w_.means3D, *rot_ = w_.rotations;
        const uint32_t *cl_ = w_.g.clamped;
        const bool rot_ok = !use_precomp_cov && rot_;
        const float *rp_ = rot_ok ? rot_ : reinterpret_cast<const float *>(co_);
        const int ri_ = rot_ok ? 4 * i_ : 0;
        o.co = co_[i_];
#pragma unroll
        for (int k = 0; k < 6; k++) o.c6[k] = c6_[6 * i_ + k];
#pragma unroll
        for (int k = 0; k < 3; k++) o.p[k] = m3_[3 * i_ + k];
        o.cl = cl_[i_];
#pragma unroll
        for (int k = 0; k < 4; k++) o.q[k] = rp_[ri_ + k];
    };
    float L_op = 0.f, L_col[3] = {0.f, 0.f, 0.f}, L_m3[3] = {0.f, 0.f, 0.f}, L_c6[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    float L_sc[3] = {0.f, 0.f, 0.f}, L_rt[4] = {0.f, 0.f, 0.f, 0.f};
    // the per-view record (radius, the nine accumulated pixel-level gradients) of view vi+1 is requested while view vi is
    // processed: otherwise the thread walks V dependent load -> compute rounds
    bool vis_n = false;
    float a9_n[9];
    float dz_n = 0.f;                                    // (DEPTH) record slot 9
    // the 64-byte-aligned record as three 16-byte loads (slots 0-3, 4-7, 8-11): slot 9 rides along
    auto load_record = [](const float *acc_, int i_, float (&a)[9], float &dz_) {
        const float4 *r4 = reinterpret_cast<const float4 *>(acc_ + (size_t)i_ * ACC_STRIDE);
        const float4 q0 = r4[0], q1 = r4[1], q2 = r4[2];
        a[0] = q0.x; a[1] = q0.y; a[2] = q0.z; a[3] = q0.w; a[4] = q1.x; a[5] = q1.y; a[6] = q1.z; a[7] = q1.w; a[8] = q2.x;
        if constexpr (DEPTH) dz_ = q2.y;
    };
    // what the SH gradient of this lane's FIRST view (views 0..3) is formed from after the loop: direction, dRGB (0 where clamped); all
    // zero for a view that is culled or absent.  A second view's (4..7) six values go to the quad's own row of s_in: see below.
    float e0[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    ViewIn in;                                           // the other inputs of the view in hand
    const int il = min(i, P - 1);
    const int v0 = min(vl, tab.n - 1);
    const int32_t *radii0 = tab.v[v0].radii;
    const float *acc0 = tab.v[v0].acc;
    const unsigned accmask0 = tab.v[v0].accmask;
    load_view_inputs(tab.v[v0], il, in);
    vis_n = radii0[il] > 0;
    load_record(acc0, il, a9_n, dz_n);
    // the scales (and the raw opacity when AA) are the same in every view
    float sc3[3];
    {
        const bool sc_ok = !use_precomp_cov && scales;
        const float *sp = sc_ok ? scales : reinterpret_cast<const float *>(tab.v[v0].g.conic_opacity);
        const int si = sc_ok ? 3 * il : 0;
#pragma unroll
        for (int k = 0; k < 3; k++) sc3[k] = sp[si + k];
    }
    float aa_o = 0.f;
    if constexpr (AA) aa_o = aa_opacities[il];
    (void)aa_o;
    if (STAGE) {
        // (the barrier cannot sit inside the divergent visible branch where s_in is first read: it stands here, behind every request)
        stage_sh_rows_batched<NT, NG>(shs + (size_t)bx * NG * 48, rows, s_in);
        __syncthreads();
    }
    mark(1, 0.f);
    if (i < P) {
    vis_n = vis_n && vl < tab.n;
    if (vis_n && (accmask0 & CSPLAT_SCRATCH_ZEROED)) clear_record(acc0, i);
    for (int vi = vl; vi < tab.n; vi += VL) {
    const K8View &w = tab.v[vi];
    const Cam cam = w.cam;
    const int32_t *radii = w.radii;
    const float *acc = w.acc;
    float *dL_dmean2D = w.dL_dmean2D, *dL_dconic = w.dL_dconic, *dL_dopacity = w.dL_dopacity, *dL_dcolor = w.dL_dcolor;
    float *dL_dmean3D = w.dL_dmean3D, *dL_dcov3D = w.dL_dcov3D, *dL_dscale = w.dL_dscale, *dL_drot = w.dL_drot;
    const unsigned accmask = w.accmask;
    (void)radii; (void)acc;
    const bool vis = vis_n;
    float *const crow = s_cam + (CAM ? (vi * NG + gi) * CAM_NC : 0);   // (CAM) this (view, Gaussian)'s partials
    float a9[9];
#pragma unroll
    for (int k = 0; k < 9; k++) a9[k] = vis ? a9_n[k] : 0.f;
    const float dz = vis ? dz_n : 0.f;
    mark(2, a9_n[8]);
    mark(3, in.co.w);
    moments_to_gradients(a9, vis ? in.co : make_float4(0.f, 0.f, 0.f, 0.f));
    a9[0] *= (float)cam.W; a9[1] *= (float)cam.H;      // (see k_preprocess_bwd)
    if (vi + VL < tab.n) {
        const K8View &wn = tab.v[vi + VL];
        vis_n = wn.radii[i] > 0;
        load_record(wn.acc, i, a9_n, dz_n);
        if (vis_n && (wn.accmask & CSPLAT_SCRATCH_ZEROED)) clear_record(wn.acc, i);
    }
    dL_dmean2D[3 * i] = a9[0]; dL_dmean2D[3 * i + 1] = a9[1]; dL_dmean2D[3 * i + 2] = 0.f;
    if (put3) { dL_dconic[4 * i] = a9[2]; dL_dconic[4 * i + 1] = a9[3]; dL_dconic[4 * i + 2] = 0.f; dL_dconic[4 * i + 3] = a9[4]; }
    if constexpr (!AA) PUTL(L_op, dL_dopacity, i, a9[5], CSPLAT_ACC_OPACITY);     // (AA: h dL/do', below)
    if (put3) {
        PUTL(L_col[0], dL_dcolor, 3 * i, a9[6], CSPLAT_ACC_COLOR); PUTL(L_col[1], dL_dcolor, 3 * i + 1, a9[7], CSPLAT_ACC_COLOR);
        PUTL(L_col[2], dL_dcolor, 3 * i + 2, a9[8], CSPLAT_ACC_COLOR);
    }

    float e[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    float dmean[3] = {0.f, 0.f, 0.f};
    float g6[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (!vis) {
        if constexpr (AA) PUTL(L_op, dL_dopacity, i, 0.f, CSPLAT_ACC_OPACITY);
#pragma unroll
        for (int k = 0; k < 3; k++) PUTL(L_m3[k], dL_dmean3D, 3 * i + k, 0.f, CSPLAT_ACC_MEAN3D);
        if (put3)
#pragma unroll
            for (int k = 0; k < 6; k++) PUTL(L_c6[k], dL_dcov3D, 6 * i + k, 0.f, CSPLAT_ACC_COV3D);
        if (dL_dscale)
#pragma unroll
            for (int k = 0; k < 3; k++) PUTL(L_sc[k], dL_dscale, 3 * i + k, 0.f, CSPLAT_ACC_SCALE);
        if (dL_drot)
#pragma unroll
            for (int k = 0; k < 4; k++) PUTL(L_rt[k], dL_drot, 4 * i + k, 0.f, CSPLAT_ACC_ROT);
        if constexpr (CAM) cam_partials_zero(crow);
    } else {
    const float p[3] = {in.p[0], in.p[1], in.p[2]};
    const float *view = cam.view, *proj = cam.proj;

    // ---- conic -> cov2D -> cov3D and view-space mean
    {
        float pv[3];
        view_point(p, view, pv);
        ProjJac pj;
        proj_jacobian(pv, cam, pj);
        float c6[6];
#pragma unroll
        for (int k = 0; k < 6; k++) c6[k] = in.c6[k];
        float a, b, c;
        float aa_ga = 0.f, aa_gb = 0.f, aa_gc = 0.f;     // (AA) o dL/do' dh/d(a0, b, c0)
        if constexpr (AA) {
            float a0, c0;
            cov2d_undilated(c6, pj, a0, b, c0);
            a = a0 + AA_DILATE; c = c0 + AA_DILATE;
            const float h = aa_backward(a0, b, c0, aa_o * a9[5], aa_ga, aa_gb, aa_gc);
            PUTL(L_op, dL_dopacity, i, h * a9[5], CSPLAT_ACC_OPACITY);
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
    if (want_sh) {
        const float *sh = (const float *)(s_in + gi * SH_ROW);
        const uint32_t cl = in.cl;
        const float vx = p[0] - cam.campos[0], vy = p[1] - cam.campos[1], vz = p[2] - cam.campos[2];
        const float sum2 = vx * vx + vy * vy + vz * vz;
        const float len = sqrtf(sum2);
        const float x = vx / len, y = vy / len, z = vz / len;
        float ddx = 0.f, ddy = 0.f, ddz = 0.f;
        // (the SH gradient itself, basis_k(x, y, z) dRGB, is formed after the view loop: sh_quad_rows)
        e[0] = x; e[1] = y; e[2] = z;
#pragma unroll
        for (int ch = 0; ch < 3; ch++) {
            const float dRGB = ((cl >> ch) & 1u) ? 0.f : a9[6 + ch];
            e[3 + ch] = dRGB;
            float dx_ = 0.f, dy_ = 0.f, dz_ = 0.f;
#define S(k) sh[(k) * 3 + ch]
            if (D > 0) {
                dx_ = -SH_C1 * S(3); dy_ = -SH_C1 * S(1); dz_ = SH_C1 * S(2);
                if (D > 1) {
                    const float xx = x * x, yy = y * y, zz = z * z, xy = x * y, yz = y * z, xz = x * z;
                    dx_ += SH_C2[0] * y * S(4) + SH_C2[2] * 2.f * -x * S(6) + SH_C2[3] * z * S(7) + SH_C2[4] * 2.f * x * S(8);
                    dy_ += SH_C2[0] * x * S(4) + SH_C2[1] * z * S(5) + SH_C2[2] * 2.f * -y * S(6) + SH_C2[4] * 2.f * -y * S(8);
                    dz_ += SH_C2[1] * y * S(5) + SH_C2[2] * 4.f * z * S(6) + SH_C2[3] * x * S(7);
                    if (D > 2) {
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
    for (int k = 0; k < 3; k++) PUTL(L_m3[k], dL_dmean3D, 3 * i + k, dmean[k], CSPLAT_ACC_MEAN3D);
    if (put3)
#pragma unroll
        for (int k = 0; k < 6; k++) PUTL(L_c6[k], dL_dcov3D, 6 * i + k, g6[k], CSPLAT_ACC_COV3D);

    // ---- cov3D -> scale, quaternion
    if (!use_precomp_cov && dL_dscale && dL_drot) {
        const float q[4] = {in.q[0], in.q[1], in.q[2], in.q[3]};
        float R[3][3];
        quat_to_rot(q, R);
        const float s[3] = {scale_mod * sc3[0], scale_mod * sc3[1], scale_mod * sc3[2]};
        mark(4, s[2]);
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
        for (int k = 0; k < 3; k++) PUTL(L_sc[k], dL_dscale, 3 * i + k, dA[0][k] * R[0][k] + dA[1][k] * R[1][k] + dA[2][k] * R[2][k], CSPLAT_ACC_SCALE);
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
        PUTL(L_rt[0], dL_drot, 4 * i, dq0, CSPLAT_ACC_ROT); PUTL(L_rt[1], dL_drot, 4 * i + 1, dq1, CSPLAT_ACC_ROT);
        PUTL(L_rt[2], dL_drot, 4 * i + 2, dq2, CSPLAT_ACC_ROT); PUTL(L_rt[3], dL_drot, 4 * i + 3, dq3, CSPLAT_ACC_ROT);
    }
    }   // visible
    if (vi < VL) {
#pragma unroll
        for (int k = 0; k < 6; k++) e0[k] = e[k];
    } else {
        // the lane's second and last view: this view's reads were the quad's last of its SH row (no other quad reads it, and a wave's LDS
        // accesses keep their order), so the row now carries the four lanes' values to the exchange below -- no register held for V <= 4
#pragma unroll
        for (int k = 0; k < 6; k++) s_in[gi * SH_ROW + vl * 6 + k] = e[k];
    }
    // (V > 4) the lane's next view: its record was requested above; its other inputs go out here in one batch, behind this view's stores
    if (vi + VL < tab.n) load_view_inputs(tab.v[vi + VL], i, in);
    }   // views
    __builtin_amdgcn_wave_barrier();
    if (VL == 4) {   // the four lanes' sums over their views: ((v0 + v1) + (v2 + v3)) in every lane
        auto quad_sum = [](float v) {
            v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0xB1, 0xF, 0xF, false));   // quad_perm [1,0,3,2]
            v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x4E, 0xF, 0xF, false));   // quad_perm [2,3,0,1]
            return v;
        };
        L_op = quad_sum(L_op);
#pragma unroll
        for (int k = 0; k < 3; k++) { L_col[k] = quad_sum(L_col[k]); L_m3[k] = quad_sum(L_m3[k]); L_sc[k] = quad_sum(L_sc[k]); }
#pragma unroll
        for (int k = 0; k < 6; k++) L_c6[k] = quad_sum(L_c6[k]);
#pragma unroll
        for (int k = 0; k < 4; k++) L_rt[k] = quad_sum(L_rt[k]);
    }
    // ---- the SH gradient.  Every lane of the quad takes all four lanes' (direction, dRGB) by DPP and forms coefficients 12 vl .. 12 vl + 11
    // (basis functions 4 vl .. 4 vl + 3, three channels) of each: the quad stores the Gaussian's 192-byte row as 4 x 3 16-byte stores, no LDS.
    // Association as ever: lane order ((r0 + r1) + r2) + r3, r = the sum over that lane's views in order.
    if (VL == 4 && shs && dL_dsh) {
        float o[12];
        auto coeffs = [&](const float (&b)[6], float (&c)[12]) {
            const float x = b[0], y = b[1], z = b[2];
            const float xx = x * x, yy = y * y, zz = z * z, xy = x * y, yz = y * z, xz = x * z;
            const float b0[4] = {SH_C0, -SH_C1 * y, SH_C1 * z, -SH_C1 * x};
            const float b1[4] = {SH_C2[0] * xy, SH_C2[1] * yz, SH_C2[2] * (2.f * zz - xx - yy), SH_C2[3] * xz};
            const float b2[4] = {SH_C2[4] * (xx - yy), SH_C3[0] * y * (3.f * xx - yy), SH_C3[1] * xy * z, SH_C3[2] * y * (4.f * zz - xx - yy)};
            const float b3[4] = {SH_C3[3] * z * (2.f * zz - 3.f * xx - 3.f * yy), SH_C3[4] * x * (4.f * zz - xx - yy), SH_C3[5] * z * (xx - yy),
                                 SH_C3[6] * x * (xx - 3.f * yy)};
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const float lo = (vl & 1) ? b1[k] : b0[k], hi = (vl & 1) ? b3[k] : b2[k];
                const float f = (vl & 2) ? hi : lo;        // basis function 4 vl + k
#pragma unroll
                for (int ch = 0; ch < 3; ch++) c[k * 3 + ch] = f * b[3 + ch];
            }
        };
        auto lane_of_quad = [](float v, auto J) {      // lane J of the quad, in all four
            constexpr int j = decltype(J)::value;
            return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), j * 0x55, 0xF, 0xF, false));
        };
        auto add_lane = [&](auto J) {
            constexpr int j = decltype(J)::value;
            float b[6], c[12];
#pragma unroll
            for (int k = 0; k < 6; k++) b[k] = lane_of_quad(e0[k], J);
            coeffs(b, c);
            if (VL + j < tab.n) {      // lane j's second view: from the quad's row
                float c1[12];
#pragma unroll
                for (int k = 0; k < 6; k++) b[k] = s_in[gi * SH_ROW + j * 6 + k];
                coeffs(b, c1);
#pragma unroll
                for (int k = 0; k < 12; k++) c[k] += c1[k];
            }
#pragma unroll
            for (int k = 0; k < 12; k++) o[k] = j == 0 ? c[k] : o[k] + c[k];
        };
        add_lane(std::integral_constant<int, 0>{}); add_lane(std::integral_constant<int, 1>{});
        add_lane(std::integral_constant<int, 2>{}); add_lane(std::integral_constant<int, 3>{});
        // the basis functions above the active degree D take no gradient
        const int nbasis = (D + 1) * (D + 1);
#pragma unroll
        for (int k = 0; k < 4; k++)
            if (4 * vl + k >= nbasis) { o[3 * k] = 0.f; o[3 * k + 1] = 0.f; o[3 * k + 2] = 0.f; }
        float4 *dst4 = reinterpret_cast<float4 *>(dL_dsh + (size_t)i * 48 + 12 * vl);
        const bool add_in = (tab.v[0].accmask & CSPLAT_ACC_SH) != 0u;
#pragma unroll
        for (int k = 0; k < 3; k++) {
            float4 w4 = make_float4(o[4 * k], o[4 * k + 1], o[4 * k + 2], o[4 * k + 3]);
            if (add_in) { const float4 u = dst4[k]; w4.x += u.x; w4.y += u.y; w4.z += u.z; w4.w += u.w; }
            dst4[k] = w4;
        }
    }
    if (vl == 0) {   // gradients of the parameters every view shares: one write (added to the buffer only if the first view was asked to)
        const unsigned accmask = tab.v[0].accmask;
        const K8View &w = tab.v[0];
#define PUTS(ptr, idx, val, bit) do { if (smask & (bit)) { float *p_ = (ptr) + (idx); *p_ = (accmask & (bit)) ? *p_ + (val) : (val); } } while (0)
        PUTS(w.dL_dopacity, i, L_op, CSPLAT_ACC_OPACITY);
        if (put3)
#pragma unroll
            for (int k = 0; k < 3; k++) PUTS(w.dL_dcolor, 3 * i + k, L_col[k], CSPLAT_ACC_COLOR);
#pragma unroll
        for (int k = 0; k < 3; k++) PUTS(w.dL_dmean3D, 3 * i + k, L_m3[k], CSPLAT_ACC_MEAN3D);
        if (put3)
#pragma unroll
            for (int k = 0; k < 6; k++) PUTS(w.dL_dcov3D, 6 * i + k, L_c6[k], CSPLAT_ACC_COV3D);
        if (w.dL_dscale)
#pragma unroll
            for (int k = 0; k < 3; k++) PUTS(w.dL_dscale, 3 * i + k, L_sc[k], CSPLAT_ACC_SCALE);
        if (w.dL_drot)
#pragma unroll
            for (int k = 0; k < 4; k++) PUTS(w.dL_drot, 4 * i + k, L_rt[k], CSPLAT_ACC_ROT);
#undef PUTS
    }
    }   // i < P
    mark(5, 0.f);
    if constexpr (CAM)   // (every view of the call: each lane with i < P has written its rows of all the views it holds)
        for (int vi = 0; vi < tab.n; vi++) cam_block_sum<NT>(s_cam + vi * NG * CAM_NC, rows, s_cpart, cam_slabs->p[vi] + (size_t)bx * CAM_NC);
#undef PUTL
