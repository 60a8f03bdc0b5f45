"""The one-launch per-Gaussian backward of csplat_backward_views (K8 for all views: csrc/csplat_k8_views_body.h), with the compositing
backward in its bit-reproducible mode (csplat_debug_flags 256), so that what differs between two runs is K8's own arithmetic:

  - against the per-view K8 launches (flags 256 | 128), util.rel_err < 1e-6, and against fp64 autograd (tests/antialias_ref.py, which
    renders with and without antialiasing and carries the depth image and the camera leaves), util.rel_err < 1e-4 -- the two bars of
    tests/test_raster_gpu.py -- for V in {2, 3, 4, 5, 8} (one and two views per lane of a quad), P not a multiple of 32, shared and
    per-view means3D / rotations, one view close to the cloth (part of the Gaussians culled), and through the depth, camera and
    antialiased kernels;
  - cut into three Gaussian ranges (csplat_backward_views_parts) == the whole call, torch.equal;
  - CSPLAT_K8_OUTPUTS_UNREAD (include/csplat.h) by direct calls of csplat_backward_views on a csplat_view array: the bit changes no
    gradient the caller reads, and dL_dconic / dL_dcolor / dL_dcov3D are each written in full or left untouched;
  - a gradient buffer at a 4-byte-aligned address that is not 16-byte aligned: same result as the aligned buffer;
  - in the default mode, the csplat_view array of a real deferred backward against the plan tests/test_raster_grad_layout_cpu.py pins."""
import ctypes as C

import numpy as np
import pytest

import util
import antialias_ref
from util import make_case, oracle_forward, rel_err

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

TOL = 1e-4          # against fp64 (tests/test_raster_gpu.py: TOL)
TOL_K8 = 1e-6       # batched against per-view K8 (tests/test_raster_gpu.py: test_one_k8_for_all_views_equals_per_view_k8)
W, H = 128, 96
CAM_KEYS = ("view", "proj", "campos", "bg")
UNREAD = 512        # csplat.h: CSPLAT_K8_OUTPUTS_UNREAD
POISON = 12345.0


def _flags(f):
    from csplat import native
    native.lib.csplat_debug_flags(f)


def _views(V, P, own):
    """V views around one cloth; view 1 stands close to it (radius 1.2: the frustum culls part of the Gaussians).  own: every view has its
    own means3D / rotations (the train step's deformed copies)"""
    cases = []
    for i in range(V):
        c = make_case(P=P, W=W, H=H, seed=7, grid=20, theta=-40.0 + 25.0 * i, radius=1.2 if i == 1 else 4.0)
        if own:
            g = c["g"] = dict(c["g"])
            g["means3D"] = (g["means3D"] + 0.001 * i).astype(np.float32)
            g["rotations"] = (g["rotations"] * (1.0 + 0.01 * i)).astype(np.float32)
        cases.append(c)
    rng = np.random.default_rng(21)
    wts = [dict(color=rng.normal(size=(3, H, W)), depth=rng.normal(size=(1, H, W))) for _ in range(V)]
    return cases, wts


def _gpu(cases, wts, own, depth=False, cam=False, aa=False, flags=256):
    """one rasterize_views step under csplat_debug_flags(flags) -> ({name: float64 array}, radii of every view)"""
    import diff_gaussian_rasterization as dgr
    V, P = len(cases), cases[0]["P"]
    T = lambda a: torch.tensor(np.asarray(a, np.float32), device="cuda", requires_grad=True)  # noqa: E731
    t = lambda a: torch.tensor(np.asarray(a, np.float32), device="cuda")  # noqa: E731
    _flags(flags)
    try:
        inp = util.gpu_inputs(cases[0])
        means = [T(c["g"]["means3D"]) for c in cases] if own else [inp["means3D"]] * V
        rots = [T(c["g"]["rotations"]) for c in cases] if own else [inp["rotations"]] * V
        m2d = [torch.zeros(P, 3, device="cuda", requires_grad=True) for _ in range(V)]
        settings, leaves = [], []
        for c in cases:
            rs = util.gpu_settings(c)
            if cam:
                k = c["cam"]
                lv = dict(view=T(k["world_view_transform"]), proj=T(k["full_proj_transform"]), campos=T(k["camera_center"]), bg=T(c["bg"]))
                rs = rs._replace(viewmatrix=lv["view"], projmatrix=lv["proj"], campos=lv["campos"], bg=lv["bg"])
                leaves.append(lv)
            settings.append(rs)
        kws = [dict(means3D=means[i], means2D=m2d[i], opacities=inp["opacities"], shs=inp["shs"], scales=inp["scales"], rotations=rots[i],
                    antialiasing=aa) for i in range(V)]
        outs = dgr.rasterize_views(settings, kws)
        loss = sum((outs[i][0] * t(wts[i]["color"])).sum() for i in range(V))
        if depth:
            loss = loss + sum((outs[i][2] * t(wts[i]["depth"])).sum() for i in range(V) if i != 1)      # (view 1 has no depth gradient)
        loss.backward()
        torch.cuda.synchronize()
    finally:
        _flags(0)
    got = dict(opacity=inp["opacities"].grad.reshape(-1), sh=inp["shs"].grad, scale=inp["scales"].grad)
    for i in range(V):
        got["mean2D_%d" % i] = m2d[i].grad
        if own:
            got["mean3D_%d" % i], got["rot_%d" % i] = means[i].grad, rots[i].grad
        if cam:
            got.update({"%s_%d" % (k, i): leaves[i][k].grad for k in CAM_KEYS})
    if not own:
        got["mean3D"], got["rot"] = inp["means3D"].grad, inp["rotations"].grad
    return {k: v.detach().cpu().numpy().astype(np.float64) for k, v in got.items()}, [o[1].cpu().numpy() for o in outs]


def _ref(cases, wts, own, depth=False, cam=False, aa=False):
    """the same step in fp64 autograd"""
    V, P = len(cases), cases[0]["P"]
    T = lambda a: torch.tensor(np.asarray(a, np.float64), requires_grad=True)  # noqa: E731
    g0 = cases[0]["g"]
    op, sh, sc = T(g0["opacities"]), T(g0["shs"]), T(g0["scales"])
    means = [T(c["g"]["means3D"]) for c in cases] if own else [T(g0["means3D"])] * V
    rots = [T(c["g"]["rotations"]) for c in cases] if own else [T(g0["rotations"])] * V
    m2d = [T(np.zeros((P, 3))) for _ in range(V)]
    loss, cams = 0.0, []
    for i, c in enumerate(cases):
        o = oracle_forward(c, dtype=np.float64)
        lv = dict(zip(CAM_KEYS, antialias_ref.camera_tensors(o)))
        cams.append(lv)
        color, dimg = antialias_ref.render(o, means[i], m2d[i], op, lv["view"], lv["proj"], lv["campos"], lv["bg"], shs=sh, scales=sc,
                                           rotations=rots[i], antialiasing=aa)[:2]
        loss = loss + (color * torch.tensor(wts[i]["color"])).sum()
        if depth and i != 1:
            loss = loss + (dimg * torch.tensor(wts[i]["depth"])).sum()
    loss.backward()
    ref = dict(opacity=op.grad.reshape(-1), sh=sh.grad, scale=sc.grad)
    for i in range(V):
        ref["mean2D_%d" % i] = m2d[i].grad
        if own:
            ref["mean3D_%d" % i], ref["rot_%d" % i] = means[i].grad, rots[i].grad
        if cam:
            ref.update({"%s_%d" % (k, i): cams[i][k].grad for k in CAM_KEYS})
    if not own:
        ref["mean3D"], ref["rot"] = means[0].grad, rots[0].grad
    return {k: v.numpy() for k, v in ref.items()}


def _check(V, P, own, **variant):
    cases, wts = _views(V, P, own)
    one, radii = _gpu(cases, wts, own, flags=256, **variant)
    per_view, _ = _gpu(cases, wts, own, flags=256 | 128, **variant)
    n_vis = int((radii[1] > 0).sum())
    assert 0 < n_vis < P, n_vis                    # (the close view culls part of the cloth and keeps part of it)
    assert one.keys() == per_view.keys()
    for k in one:
        assert np.isfinite(one[k]).all(), k
        e = rel_err(one[k], per_view[k])
        print("K8 for all views against per-view K8: %-12s %.3e" % (k, e))
        assert e < TOL_K8, (k, e)
    ref = _ref(cases, wts, own, **variant)
    for k in one:
        e = rel_err(one[k], ref[k])
        print("K8 for all views against fp64:        %-12s %.3e" % (k, e))
        assert e < TOL, (k, e)


@pytest.mark.parametrize("own", [False, True], ids=["shared_means", "own_means"])
@pytest.mark.parametrize("V", [2, 3, 4, 5, 8])
def test_all_views_k8_against_per_view_k8_and_fp64(V, own):
    _check(V, 2013, own)          # 2013 = 62 * 32 + 29: the last workgroup holds 29 Gaussians


@pytest.mark.parametrize("variant", [dict(depth=True), dict(cam=True), dict(depth=True, cam=True), dict(aa=True),
                                     dict(aa=True, depth=True), dict(aa=True, cam=True), dict(aa=True, depth=True, cam=True)],
                         ids=["depth", "cam", "cam_depth", "aa", "aa_depth", "aa_cam", "aa_cam_depth"])
@pytest.mark.parametrize("V,own", [(4, False), (5, True)], ids=["V4_shared", "V5_own"])
def test_depth_camera_and_antialiased_kernels(V, own, variant):
    _check(V, 2013, own, **variant)


def _deferred_step(V, P, own=False):
    """a rasterize_views step whose backward has launched K7 only (deferred_k8) -> (handle, gradient tensors by name)"""
    import diff_gaussian_rasterization as dgr
    cases, wts = _views(V, P, own)
    T = lambda a: torch.tensor(np.asarray(a, np.float32), device="cuda", requires_grad=True)  # noqa: E731
    inp = util.gpu_inputs(cases[0])
    means = [T(c["g"]["means3D"]) for c in cases] if own else [inp["means3D"]] * V
    rots = [T(c["g"]["rotations"]) for c in cases] if own else [inp["rotations"]] * V
    m2d = [torch.zeros(P, 3, device="cuda", requires_grad=True) for _ in range(V)]
    kws = [dict(means3D=means[i], means2D=m2d[i], opacities=inp["opacities"], shs=inp["shs"], scales=inp["scales"], rotations=rots[i])
           for i in range(V)]
    outs = dgr.rasterize_views([util.gpu_settings(c) for c in cases], kws)
    loss = sum((outs[i][0] * torch.tensor(np.asarray(wts[i]["color"], np.float32), device="cuda")).sum() for i in range(V))
    with dgr.deferred_k8() as h:
        loss.backward()
    assert len(h.entries) == 1
    leaves = dict(opacity=inp["opacities"], sh=inp["shs"], scale=inp["scales"])
    leaves.update({"mean2D_%d" % i: m2d[i] for i in range(V)})
    if own:
        leaves.update({"mean3D_%d" % i: means[i] for i in range(V)})
        leaves.update({"rot_%d" % i: rots[i] for i in range(V)})
    else:
        leaves.update(mean3D=inp["means3D"], rot=inp["rotations"])
    return h, {k: v.grad for k, v in leaves.items()}


@pytest.mark.parametrize("V,own", [(4, False), (5, True)], ids=["V4_shared", "V5_own"])
def test_three_slices_equal_the_whole_call(V, own):
    _flags(256)
    try:
        res = []
        for G in (1, 3):
            h, grads = _deferred_step(V, 2013, own)
            for t in grads.values():
                t.fill_(float("nan"))
            for g_ in range(G):
                h.launch(g_, G)
            torch.cuda.synchronize()
            res.append({k: v.clone() for k, v in grads.items()})
    finally:
        _flags(0)
    for k in res[0]:
        assert torch.isfinite(res[0][k]).all(), k
        assert torch.equal(res[0][k], res[1][k]), k


def _call(h, flags):
    """csplat_backward_views on the handle's csplat_view array (K7 in its bit-reproducible mode writes every record anew: the call can be
    repeated on one array)"""
    from csplat import native
    sub, n, dev, _P, _keep = h.entries[0]
    _flags(flags)
    with native.on_device(dev):
        rc = native.lib.csplat_backward_views(n, C.cast(sub, C.c_void_p), torch.cuda.current_stream(dev).cuda_stream)
    native.check(rc, "csplat_backward_views")
    torch.cuda.synchronize()


@pytest.mark.parametrize("shared3", [False, True], ids=["three_per_view", "colour_cov3D_shared"])
@pytest.mark.parametrize("V", [4, 5])
def test_unread_outputs_bit(V, shared3):
    """shared3: dL_dcolor and dL_dcov3D are one buffer for all views (views after the first add into it), as a caller with shared
    parameters may lay them out; otherwise every view has its own, as the autograd wrapper lays them out."""
    from csplat import native
    P = 2013
    _flags(256)
    try:
        h, grads = _deferred_step(V, P)
        sub = h.entries[0][0]
        z = lambda n, w: [torch.empty(P, w, device="cuda") for _ in range(n)]  # noqa: E731
        conic, color, cov = z(V, 4), z(1 if shared3 else V, 3), z(1 if shared3 else V, 6)
        base_mask = []
        for a in range(V):
            sub[a].dL_dconic = conic[a].data_ptr()
            sub[a].dL_dcolor = color[0 if shared3 else a].data_ptr()
            sub[a].dL_dcov3D = cov[0 if shared3 else a].data_ptr()
            m = int(sub[a].accmask) & ~UNREAD
            if shared3 and a > 0:
                m |= native.ACC_COLOR | native.ACC_COV3D
            base_mask.append(m)
        three = dict(conic=conic, color=color, cov3D=cov)

        def run(flags, bit):
            for a in range(V):
                sub[a].accmask = base_mask[a] | (UNREAD if bit else 0)
            for ts in three.values():
                for t in ts:
                    t.fill_(POISON)
            for t in grads.values():
                t.fill_(float("nan"))
            _call(h, flags)
            return {k: v.clone() for k, v in grads.items()}, {k: [t.clone() for t in ts] for k, ts in three.items()}
        g_pv, t_pv = run(256 | 128, False)
        g_clear, t_clear = run(256, False)
        g_set, t_set = run(256, True)
        g_pv_set, t_pv_set = run(256 | 128, True)
    finally:
        _flags(0)
    for k in g_clear:
        assert torch.isfinite(g_clear[k]).all(), k
        assert torch.equal(g_clear[k], g_set[k]), k
        assert torch.equal(g_pv[k], g_pv_set[k]), k
    for k in t_clear:
        for a, (c, s, p, ps) in enumerate(zip(t_clear[k], t_set[k], t_pv[k], t_pv_set[k])):
            assert not (p == POISON).any() and torch.equal(p, ps), (k, a)      # the per-view launches write the three, bit or no bit
            e = rel_err(c.cpu().numpy(), p.cpu().numpy())
            print("bit clear, %s[%d] against the per-view K8: %.3e" % (k, a, e))
            assert e < TOL_K8, (k, a, e)
            assert torch.equal(s, c) or bool((s == POISON).all()), (k, a)      # with the bit: written in full or not at all


@pytest.mark.parametrize("V,own", [(4, False), (5, True)], ids=["V4_shared", "V5_own"])
def test_misaligned_gradient_buffers(V, own):
    """every gradient buffer but dL_dsh (whose 16-byte alignment the one-launch K8 requires: a call without it takes the per-view launches)
    moved to an address that is 4 bytes past a 16-byte boundary"""
    P = 2013
    fields = ("dL_dmean2D", "dL_dconic", "dL_dopacity", "dL_dcolor", "dL_dmean3D", "dL_dcov3D", "dL_dscale", "dL_drot")
    width = dict(dL_dmean2D=3, dL_dconic=4, dL_dopacity=1, dL_dcolor=3, dL_dmean3D=3, dL_dcov3D=6, dL_dscale=3, dL_drot=4)
    _flags(256)
    try:
        h, grads = _deferred_step(V, P, own)
        sub = h.entries[0][0]
        orig = {(a, f): int(getattr(sub[a], f)) for a in range(V) for f in fields}
        for a in range(V):
            sub[a].accmask = int(sub[a].accmask) & ~UNREAD
        res = []
        for shift in (0, 1):
            bufs = {}           # the call's buffer -> ours (a buffer that several views share stays shared)
            for a in range(V):
                for f in fields:
                    key = (f, orig[(a, f)])
                    if key not in bufs:
                        bufs[key] = torch.full((P * width[f] + 4,), float("nan"), device="cuda")
                        assert bufs[key].data_ptr() % 16 == 0
                    setattr(sub[a], f, bufs[key].data_ptr() + 4 * shift)
            grads["sh"].fill_(float("nan"))
            _call(h, 256)
            out = {k: v[shift:shift + P * width[k[0]]].clone() for k, v in bufs.items()}
            out[("dL_dsh", 0)] = grads["sh"].clone()
            res.append(out)
    finally:
        _flags(0)
    assert res[0].keys() == res[1].keys()
    for k in res[0]:
        assert torch.isfinite(res[0][k]).all(), k
        assert torch.equal(res[0][k], res[1][k]), k


def test_deferred_plan_lies_where_the_pinned_layout_says():
    """the csplat_view array a real backward hands the library -- default mode, persistent zeroed records -- against the default-mode entry
    of the table tests/test_raster_grad_layout_cpu.py pins without a GPU: every gradient pointer as an offset from the one allocation,
    and the accumulate masks.  V = 2, P = 33, a 16 x 16 image, every parameter shared -- but means2D: K8 turns a view's K7 moments into its dL_dmean2D
    (csrc/csplat_k8_views_body.h: `dL_dmean2D[3 * i] = a9[0]`), one buffer per view, and inside deferred_k8() a leaf must get its gradient from one buffer alone (a shared means2D would have autograd add two
    buffers K8 has not written yet); the layout never shares that row, so the pinned plan is the same."""
    import diff_gaussian_rasterization as dgr
    import test_raster_grad_layout_cpu as L
    case = make_case(P=33, W=16, H=16, seed=3, grid=4, scale_mul=3.0)
    inp = util.gpu_inputs(case)
    m2d = [inp["means2D"], torch.zeros(33, 3, device="cuda", requires_grad=True)]
    kws = [dict(means3D=inp["means3D"], means2D=m, opacities=inp["opacities"], shs=inp["shs"], scales=inp["scales"],
                rotations=inp["rotations"]) for m in m2d]
    assert inp["shs"].shape[1] == 16 and inp["shs"].data_ptr() % 16 == 0
    outs = dgr.rasterize_views([util.gpu_settings(case)] * 2, kws)
    with dgr.deferred_k8() as h:
        (outs[0][0].sum() + 2.0 * outs[1][0].sum()).backward()
    assert len(h.entries) == 1
    sub, n, _dev, P, keep = h.entries[0]
    want = L.expected()["0"]["V2_P33_M16_all"]
    assert (n, P) == (2, 33) and keep[0].numel() == want["total"]
    base = keep[0].data_ptr()
    for a in range(n):
        got = [int(sub[a].accmask)] + [None if not getattr(sub[a], f) else (getattr(sub[a], f) - base) // 4 for f in L.FIELDS]
        assert got == want["views"][a][:1] + want["views"][a][2:], (a, got)
        assert all((getattr(sub[a], f) - base) % 4 == 0 for f in L.FIELDS if getattr(sub[a], f))
        assert sub[a].scratch and not base <= sub[a].scratch < base + 4 * keep[0].numel()      # (the persistent records: outside)
    leaves = [t for k, t in kws[0].items() if k != "means2D"] + m2d
    for t in leaves:      # the gradients autograd adopted ARE the plan's buffers: K8 has yet to write them
        assert base <= t.grad.data_ptr() < base + 4 * keep[0].numel()
        t.grad.fill_(float("nan"))
    h.launch(0, 1)
    torch.cuda.synchronize()
    assert all(torch.isfinite(t.grad).all() for t in leaves)
