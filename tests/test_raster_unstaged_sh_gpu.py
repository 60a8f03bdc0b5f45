"""The per-Gaussian kernels that do NOT stage the SH rows through LDS.  The library stages only when M == 16 and the SH tensor (for K8
also dL_dsh) is 16-byte aligned (include/csplat.h, at `M`); a model of sh_degree 0..2 (M = 1, 4, 9), a tensor with spare coefficient
rows (M = 25) and a contiguous [P, 16, 3] view 4 bytes off a 16-byte boundary are served by
    K1  k_preprocess<false>, k_preprocess_aa<false>, k_preprocess_views<false>, k_preprocess_views_aa<false>
    K8  k_preprocess_bwd / _depth / _cam<DEPTH> / _aa<DEPTH, CAM>, each <STAGE = false, NT = 256>
and, around them, by begin_views_compatible (the batched K1 takes any M), k8_views_table (the one-launch K8 does not: per-view K8) and
_RasterizeGaussiansBatch._plan_backward (views share one dL_dsh only when the library can add into it).
Inputs: tests/unstaged_sh_ref.py (short / padded / off16).  Bars: against the staged twin (the same call with the 16-coefficient,
aligned tensor) K1 is equal BIT FOR BIT -- the body is one expression compiled with contraction off, only the source of the SH values
differs; against the fp32 oracle the bars of tests/test_raster_gpu.py:test_indices_bit_exact; gradients against fp64 within 1e-4
(BASELINE.json north_star), batched against per-view calls within the bars of tests/test_camera_grad_gpu.py (1e-6 in the bit-reproducible
mode, 1e-5 with atomics).  tests/test_raster_unstaged_sh_cpu.py holds, without a GPU, that the oracles treat short and padded alike.
(A dL_dsh buffer off a 16-byte boundary cannot arise through Python: the plan reserves every gradient at a 256-byte granule of one
allocation, and takes a gradient sink only when it is 16-byte aligned.  It is therefore not tested.)"""
import collections
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

import util
import unstaged_sh_ref as us
from unstaged_sh_ref import PAIRS, padded, short, with_sh
from util import image_err, make_case, oracle_forward, rel_err

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

TOL = 1e-4                      # against fp64
BIT_REPRODUCIBLE = 256          # csplat_debug_flags bit 8
PER_VIEW_LAUNCHES = 512         # csplat_debug_flags bit 9
SPECS = [(M, D, False) for M, D in PAIRS] + [(16, D, True) for D in us.OFF16_DEGREES]      # (M, D, off16)
FEW = [(4, 1, False), (25, 3, False), (16, 3, True)]
FORM_SPECS = [(4, 1, False), (16, 3, True)]
K1_FIELDS = ("depth", "xy", "conic_opacity", "cov3D", "rgb", "clamped", "tiles_touched")
EDGE_P = [1, 63, 64, 65, 255, 256, 257, 449]     # around the 64-Gaussian workgroup of the batched K1 and the 256 threads of K1 / unstaged K8
EW, EH = 33, 17                                   # partial tiles on both edges


def _id(spec):
    return "M%d_D%d%s" % (spec[0], spec[1], "_off16" if spec[2] else "")


def _T(a, grad=True):
    return torch.tensor(np.asarray(a, np.float32), device="cuda", requires_grad=grad)


def _flags(f):
    from csplat import native
    native.lib.csplat_debug_flags(f)


def _sh_numpy(shs, spec):
    """what the oracles are fed: the tensor the unstaged kernels see"""
    return np.ascontiguousarray(shs) if spec[2] else short(shs, spec[0])


def _sh_tensors(shs, spec):
    """(the tensor only the unstaged kernels serve, its staged twin), both leaves on the GPU"""
    M, _D, off = spec
    if off:
        a, b = us.off16(_T(shs, False)), _T(shs)
        assert a.data_ptr() % 16 == 4 and a.is_contiguous() and a.is_leaf
    else:
        a, b = _T(short(shs, M)), _T(padded(shs, M))
    assert tuple(a.shape[1:]) == (M, 3) and tuple(b.shape[1:]) == (16, 3) and b.data_ptr() % 16 == 0
    return a, b


def _spec_case(base, spec):
    return with_sh(base, _sh_numpy(base["g"]["shs"], spec), spec[1])


def _behind():
    """the axis the cameras of syn.make_camera circle around, pointing to their side of the cloth: a Gaussian moved far along it stands
    behind every camera"""
    a = util.syn.make_camera(0.0, EW, EH)["camera_center"].astype(np.float64) + util.syn.make_camera(180.0, EW, EH)["camera_center"]
    return a / np.linalg.norm(a)


def _edge_case(P):
    """the first P Gaussians of a cloth in a 33 x 17 image, every eighth behind the camera"""
    case = make_case(P=EDGE_P[-1], W=EW, H=EH, seed=7, grid=6, scale_mul=4.0, radius=1.5)
    g = dict(case["g"])
    m = np.array(g["means3D"], np.float64)
    m[5::8] += 50.0 * _behind()
    g["means3D"] = m.astype(np.float32)
    return dict(case, P=P, g={k: v[:P] for k, v in g.items()})


def _same_bits(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, what
    if a.tobytes() != b.tobytes():
        ua, ub = a.view(np.uint32).astype(np.int64).reshape(-1), b.view(np.uint32).astype(np.int64).reshape(-1)
        bad = np.nonzero(ua != ub)[0]
        raise AssertionError("%s: %d of %d words differ, first at %d, largest distance %d ulp" %
                             (what, bad.size, ua.size, bad[0], int(np.abs(ua - ub)[bad].max())))


def _all_same(got, twin, what):
    assert got.keys() == twin.keys()
    for k in got:
        _same_bits(got[k], twin[k], "%s: %s" % (what, k))


def _oracle_bars(got, o):
    """the per-Gaussian bars of tests/test_raster_gpu.py:test_indices_bit_exact, against the fp32 oracle fed the same SH tensor"""
    np.testing.assert_array_equal(got["radii"], o.radii)
    np.testing.assert_array_equal(got["tiles_touched"], o.tiles_touched)
    for k in ("depth", "xy", "conic_opacity", "cov3D"):
        np.testing.assert_array_equal(got[k].view(np.uint32), getattr(o, k).view(np.uint32), err_msg=k)
    clamped = np.stack([(got["clamped"] >> c) & 1 for c in range(3)], 1).astype(np.uint8)
    vis = o.radii > 0
    e = rel_err(got["rgb"], o.rgb)
    print("rgb against the fp32 oracle %.3e, clamp mismatches %d" % (e, int((clamped[vis] != o.clamped[vis]).sum())))
    assert (clamped[vis] != o.clamped[vis]).sum() <= 2
    assert e < 1e-5


# ------------------------------------------------------------------------------------------------ 1. K1, single view
def _forward_raw(case, sh):
    """the single-view Function's forward (csplat_forward_begin / _finish: k_preprocess) -> K1's fields, radii and the two images"""
    inp = util.gpu_inputs(case, requires_grad=False)
    inp["shs"] = sh.detach()
    color, radii, depth, st = util.gpu_forward_raw(case, inputs=inp)
    out = {k: st[k] for k in K1_FIELDS}
    out.update(radii=radii.cpu().numpy(), color=color.cpu().numpy(), depth_image=depth.cpu().numpy())
    return out


def _single_view_k1(base, spec):
    case = _spec_case(base, spec)
    a, b = _sh_tensors(base["g"]["shs"], spec)
    got, twin = _forward_raw(case, a), _forward_raw(case, b)
    _all_same(got, twin, "unstaged K1 against its staged twin")
    _oracle_bars(got, oracle_forward(case))
    return got


@pytest.mark.parametrize("spec", SPECS, ids=_id)
@pytest.mark.parametrize("ci", range(len(us.CASES)))
def test_k1_single_view(ci, spec):
    got = _single_view_k1(make_case(**us.CASES[ci]), spec)
    vis = got["radii"] > 0
    assert vis.any() and (ci != us.CULLING or not vis.all())


@pytest.mark.parametrize("spec", FEW, ids=_id)
@pytest.mark.parametrize("P", EDGE_P)
def test_k1_single_view_launch_edges(P, spec):
    _single_view_k1(_edge_case(P), spec)


def _geom_fields(view, P):
    """K1's fields out of a view's GEOM chunk (csplat_geom_layout), as util.gpu_chunks reads them"""
    from csplat import native as n
    o8 = (C.c_size_t * 8)(); n.lib.csplat_geom_layout(P, o8)
    geom = view.chunks[0].cpu().numpy().tobytes()
    f = lambda off, dt, count: np.frombuffer(geom, dtype=dt, count=count, offset=off).copy()  # noqa: E731
    return dict(depth=f(o8[0], np.float32, P), xy=f(o8[1], np.float32, 2 * P).reshape(P, 2),
                conic_opacity=f(o8[2], np.float32, 4 * P).reshape(P, 4), rgb=f(o8[3], np.float32, 3 * P).reshape(P, 3),
                cov3D=f(o8[4], np.float32, 6 * P).reshape(P, 6), clamped=f(o8[5], np.uint32, P), tiles_touched=f(o8[6], np.uint32, P))


def _views_forward(cases, sh, aa=False, flags=0, images=True):
    """one rasterize_views call under csplat_debug_flags(flags): every view has its own means3D / rotations (its case's), opacities,
    scales and the SH tensor are shared -> per view K1's fields and radii (and the two images)"""
    import diff_gaussian_rasterization as dgr
    from csplat import native
    P, g0 = cases[0]["P"], cases[0]["g"]
    op, sc = _T(g0["opacities"]), _T(g0["scales"])
    kws = [dict(means3D=_T(c["g"]["means3D"]), means2D=torch.zeros(P, 3, device="cuda", requires_grad=True), opacities=op, shs=sh, scales=sc,
                rotations=_T(c["g"]["rotations"]), antialiasing=aa) for c in cases]
    old = int(native.lib.csplat_debug_flags_query())
    _flags(flags)
    try:
        outs = dgr.rasterize_views([util.gpu_settings(c) for c in cases], kws)
        torch.cuda.synchronize()
        res = []
        for i, v in enumerate(outs[0][0].grad_fn.views):
            f = _geom_fields(v, P)
            f["radii"] = outs[i][1].cpu().numpy()
            if images:
                f.update(color=outs[i][0].detach().cpu().numpy(), depth_image=outs[i][2].detach().cpu().numpy())
            res.append(f)
    finally:
        _flags(old)
    return res


@pytest.mark.parametrize("spec", FEW, ids=_id)
@pytest.mark.parametrize("ci", range(len(us.CASES)))
def test_k1_single_view_antialiased(ci, spec):
    """k_preprocess_aa<false>: one antialiased view with the per-view launches (csplat_debug_flags bit 9)"""
    base = make_case(**us.CASES[ci])
    case = _spec_case(base, spec)
    a, b = _sh_tensors(base["g"]["shs"], spec)
    got, = _views_forward([case], a, aa=True, flags=PER_VIEW_LAUNCHES)
    twin, = _views_forward([case], b, aa=True, flags=PER_VIEW_LAUNCHES)
    _all_same(got, twin, "unstaged antialiased K1 against its staged twin")
    vis = got["radii"] > 0
    assert vis.any() and (got["conic_opacity"][vis, 3] < case["g"]["opacities"][vis, 0]).any(), "antialiasing left every opacity alone"
    o = oracle_forward(case)        # (no antialiasing there: what does not depend on the opacity)
    np.testing.assert_array_equal(got["radii"], o.radii)
    for k in ("depth", "xy", "cov3D"):
        np.testing.assert_array_equal(got[k].view(np.uint32), getattr(o, k).view(np.uint32), err_msg=k)
    assert rel_err(got["rgb"], o.rgb) < 1e-5


# ------------------------------------------------------------------------------------------------ 2. K1, batched
def _view_cases(V, spec, P=EDGE_P[-1], W=EW, H=EH, scale_mul=4.0, radius=1.5):
    """V views of one cloth with the SH tensor of `spec`: per-view means3D / rotations (slightly moved, as a deformed cloth's are), every
    eighth Gaussian behind all cameras, view 2 closer to the cloth -> (cases, the cloth's [P, 16, 3] coefficients)"""
    plain = make_case(P=P, W=W, H=H, seed=11, grid=6, scale_mul=scale_mul, radius=radius)
    base = _spec_case(plain, spec)
    up = _behind()
    cases = []
    for i in range(V):
        g = dict(base["g"])
        m = np.array(g["means3D"], np.float64) + 0.001 * i
        m[5::8] += 50.0 * up
        g["means3D"] = m.astype(np.float32)
        g["rotations"] = (g["rotations"] * (1.0 + 0.01 * i)).astype(np.float32)
        cam = util.syn.make_camera(-60.0 + 17.0 * i, W, H, radius=0.8 * radius if i == 2 else radius)
        cases.append(dict(base, g=g, cam=cam))
    return cases, plain["g"]["shs"]


BATCHED_K1 = [(V, spec, False) for V in (1, 2, 4, 5, 8) for spec in SPECS] + [(V, spec, True) for V in (1, 5) for spec in FEW]


@pytest.mark.parametrize("V,spec,aa", BATCHED_K1, ids=["V%d_%s%s" % (V, _id(s), "_aa" if aa else "") for V, s, aa in BATCHED_K1])
def test_k1_batched(V, spec, aa):
    """k_preprocess_views<false> / k_preprocess_views_aa<false> (V = 5, 8: a wave's second round of views; P = 449: a partly filled last
    workgroup) against the per-view launches (k_preprocess<false> / k_preprocess_aa<false>) and against the batched staged twin"""
    from csplat import native
    cases, shs = _view_cases(V, spec)
    a, b = _sh_tensors(shs, spec)
    batched = _views_forward(cases, a, aa)
    per_view = _views_forward(cases, a, aa, flags=native.DEBUG_UNBATCHED, images=False)
    twin = _views_forward(cases, b, aa)
    vis = np.stack([f["radii"] > 0 for f in batched])
    assert vis.all(0).any() and not vis[:, 5::8].any(), "not a mix of visible and culled"
    for i in range(V):
        _all_same(batched[i], twin[i], "view %d of %d, batched unstaged K1 against the batched staged twin" % (i, V))
        _all_same({k: batched[i][k] for k in per_view[i]}, per_view[i], "view %d of %d, batched against per-view launches" % (i, V))


# ------------------------------------------------------------------------------------------------ 3. K8, plain form
def _gpu_grads(case, sh, wts, terms=("color",), aa=False, feats=None, cam=False):
    """one GaussianRasterizer call with the SH tensor `sh`; loss = sum over `terms` of (image * wts[term]).sum()
    -> ({image: array}, {gradient (unstaged_sh_ref.GRADS, CAM_GRADS, "features"): float64 array}, radii)"""
    import diff_gaussian_rasterization as dgr
    inp = util.gpu_inputs(case)
    rs = util.gpu_settings(case)
    leaves = {}
    if cam:
        k = case["cam"]
        leaves = dict(view=_T(k["world_view_transform"]), proj=_T(k["full_proj_transform"]), campos=_T(k["camera_center"]), bg=_T(case["bg"]))
        rs = rs._replace(viewmatrix=leaves["view"], projmatrix=leaves["proj"], campos=leaves["campos"], bg=leaves["bg"])
    kw = dict(means3D=inp["means3D"], means2D=inp["means2D"], opacities=inp["opacities"], shs=sh, scales=inp["scales"],
              rotations=inp["rotations"])
    if aa:
        kw["antialiasing"] = True
    if feats is not None:
        leaves["features"] = _T(feats)
        kw.update(features=leaves["features"], return_alpha=True)
    out = dgr.GaussianRasterizer(rs)(**kw)
    img = dict(color=out[0], depth=out[2])
    if feats is not None:
        img.update(feat=out[3], alpha=out[4])
    sum((img[k] * _T(wts[k], False)).sum() for k in terms).backward()
    torch.cuda.synchronize()
    got = dict(mean3D=inp["means3D"].grad, mean2D=inp["means2D"].grad, opacity=inp["opacities"].grad, sh=sh.grad, scale=inp["scales"].grad,
               rot=inp["rotations"].grad)
    got.update({k: t.grad for k, t in leaves.items()})
    assert all(v is not None for v in got.values()), [k for k, v in got.items() if v is None]
    return ({k: v.detach().cpu().numpy() for k, v in img.items()}, {k: v.detach().cpu().numpy().astype(np.float64) for k, v in got.items()},
            out[1].cpu().numpy())


def _sh_rows(grad, spec, radii, P):
    """what every dL_dsh of the unstaged K8 must be: [P, M, 3], exact zeros past (D+1)^2 and for culled Gaussians"""
    M, D, _off = spec
    assert grad.shape == (P, M, 3), grad.shape
    assert not grad[:, (D + 1) ** 2:].any(), "a coefficient row past (D+1)^2 has a gradient"
    assert not grad[radii == 0].any(), "a culled Gaussian has an SH gradient"
    assert grad[:, :(D + 1) ** 2].any()


@pytest.mark.parametrize("spec", SPECS, ids=_id)
@pytest.mark.parametrize("ci", range(len(us.CASES)))
def test_k8_colour_gradients_match_fp64(ci, spec):
    """k_preprocess_bwd<false, 256>"""
    base = make_case(**us.CASES[ci])
    case = _spec_case(base, spec)
    P = case["P"]
    dpix = np.random.default_rng(3).normal(size=(3, case["H"], case["W"])).astype(np.float32)
    o64 = oracle_forward(case, dtype=np.float64)
    g64 = util.ro.backward(o64, dpix)
    img, got, radii = _gpu_grads(case, _sh_tensors(base["g"]["shs"], spec)[0], dict(color=dpix))
    np.testing.assert_array_equal(radii, o64.radii)
    assert ci != us.CULLING or (radii == 0).any()
    e = image_err(img["color"], o64.color)
    print("colour image %.3e" % e)
    assert e < TOL
    rowwise = ci == 0 and spec in ((4, 1, False), (16, 3, True))
    for k in us.GRADS:
        ref = getattr(g64, k).reshape(got[k].shape)
        e = rel_err(got[k], ref)
        print("%-8s %.3e" % (k, e))
        assert e < TOL, (k, e)
        if rowwise:     # (the per-Gaussian bars of tests/test_raster_gpu.py:_test_backward_grads)
            e10 = util.rowwise_rel_err(got[k], ref, P, floor=1e-1)
            e1 = util.rowwise_rel_err(got[k], ref, P, floor=1e-2)
            print("%-8s row-wise: floor 10 %% %.3e, floor 1 %% %.3e (%d rows above)" % (k, e10.max(), e1.max(), int((e1 > TOL).sum())))
            assert e10.max() < TOL, (k, "floor 10 %", float(e10.max()))
            assert (e1 > TOL).sum() <= max(4, 2e-3 * P) and e1.max() < 5e-4, (k, "floor 1 %", int((e1 > TOL).sum()), float(e1.max()))
    _sh_rows(got["sh"], spec, radii, P)


# ------------------------------------------------------------------------------------------------ 4. every K8 output is written
SENTINEL = -7.0e33
OUT_FIELDS = ("dL_dmean2D", "dL_dconic", "dL_dopacity", "dL_dcolor", "dL_dmean3D", "dL_dcov3D", "dL_dsh", "dL_dscale", "dL_drot")


@pytest.mark.parametrize("P", [257, 0])
def test_every_k8_output_is_written(P):
    """csplat_backward_views(1) through the C ABI (the harness of tests/test_raster_backward_dispatch_gpu.py) with M = 4, D = 0 on the
    culling case, every output filled with a sentinel first: the single-view K8 owes every element of all nine -- dL_dsh in full, for
    visible and culled Gaussians alike.  P = 0: the early return writes nothing (the buffers handed over have rows all the same)."""
    import diff_gaussian_rasterization as dgr
    from csplat import native as n
    M, D = 4, 0
    full = make_case(**us.CASES[us.CULLING])
    case = dict(full, P=P, g={k: v[:P] for k, v in full["g"].items()})
    case = with_sh(case, short(case["g"]["shs"], M), D)
    W, H = case["W"], case["H"]
    dev = torch.device("cuda")
    inp = util.gpu_inputs(case, requires_grad=False)
    rs = util.gpu_settings(case)

    class Ctx:
        def save_for_backward(self, *a): self.saved_tensors = a
        def mark_non_differentiable(self, *a): pass
    ctx = Ctx()
    with torch.no_grad():
        dgr._RasterizeGaussians.forward(ctx, inp["means3D"], inp["means2D"], inp["shs"], None, inp["opacities"], inp["scales"],
                                        inp["rotations"], None, rs)
    vs = ctx.view_state
    means3D, sh, colors_precomp, scales, rotations, cov3Ds_precomp, radii, color = ctx.saved_tensors
    assert vs.M == M and vs.P == P
    rows = max(P, 3)
    shapes = ((rows, 3), (rows, 4), (rows, 1), (rows, 3), (rows, 3), (rows, 6), (rows, M, 3), (rows, 3), (rows, 4))
    outs = [torch.full(s, SENTINEL, dtype=torch.float32, device=dev) for s in shapes]
    dpix = _T(np.random.default_rng(11).normal(size=(3, H, W)), False)
    scratch = torch.empty(max(int(n.lib.csplat_backward_scratch_bytes(P, vs.num_rendered)), 256), dtype=torch.uint8, device=dev)
    stream = n.stream_handle(dev)
    w = n.CsplatView()
    vs.fill(w, stream, (means3D, sh, colors_precomp, None, scales, rotations, cov3Ds_precomp, color, radii))
    w.dL_dpix, w.scratch = n.ptr(dpix), n.ptr(scratch)
    for f, o in zip(OUT_FIELDS, outs):
        setattr(w, f, n.ptr(o))
    with n.on_device(dev):
        rc = n.lib.csplat_backward_views(1, C.addressof(w), w.stream)
    n.check(rc, "csplat_backward_views")
    torch.cuda.synchronize()
    if P == 0:
        for f, o in zip(OUT_FIELDS, outs):
            assert bool((o == SENTINEL).all()), f
        return
    vis = radii.cpu().numpy() > 0
    assert vis.any() and not vis.all()
    for f, o in zip(OUT_FIELDS, outs):
        o = o.cpu().numpy()
        left = np.nonzero((o == np.float32(SENTINEL)).reshape(P, -1).any(1))[0]
        assert left.size == 0, "%s: the sentinel is left in rows %s" % (f, left[:8])
        assert np.isfinite(o).all(), f
    gsh = outs[OUT_FIELDS.index("dL_dsh")].cpu().numpy()
    _sh_rows(gsh, (M, D, False), radii.cpu().numpy(), P)
    g64 = util.ro.backward(oracle_forward(case, dtype=np.float64), dpix.cpu().numpy())
    assert rel_err(gsh, g64.sh) < TOL


# ------------------------------------------------------------------------------------------------ 5. the other K8 forms
# form -> (the fp64 reference of the form's own test file, the loss terms, antialiasing, camera leaves, feature channels)
FORMS = {
    "depth": ("raster_torch", ("color", "depth"), False, False, 0),              # k_preprocess_bwd_depth
    "cam": ("camera_ref", ("color",), False, True, 0),                           # k_preprocess_bwd_cam<.., false>
    "cam_depth": ("camera_ref", ("color", "depth"), False, True, 0),             # k_preprocess_bwd_cam<.., true>
    "aa": ("antialias_ref", ("color",), True, False, 0),                         # k_preprocess_bwd_aa<.., false, false>
    "aa_depth": ("antialias_ref", ("color", "depth"), True, False, 0),           # k_preprocess_bwd_aa<.., true, false>
    "aa_cam": ("antialias_ref", ("color",), True, True, 0),                      # k_preprocess_bwd_aa<.., false, true>
    "aa_cam_depth": ("antialias_ref", ("color", "depth"), True, True, 0),        # k_preprocess_bwd_aa<.., true, true>
    "features": ("feature_ref", ("color", "feat", "alpha"), False, False, 2),    # the feature path with short SH
}


@pytest.mark.parametrize("spec", FORM_SPECS, ids=_id)
@pytest.mark.parametrize("form", sorted(FORMS))
def test_k8_other_forms_match_their_fp64_reference(form, spec):
    kind, terms, aa, cam, F = FORMS[form]
    base = make_case(**us.CASES[us.CULLING])
    case = _spec_case(base, spec)
    wts = us.weights(case, F)
    feats = np.random.default_rng(5).normal(size=(case["P"], F)).astype(np.float32) if F else None
    img, got, radii = _gpu_grads(case, _sh_tensors(base["g"]["shs"], spec)[0], wts, terms, aa, feats, cam)
    rimg, ref = us.fp64(kind, case, wts, terms, antialiasing=aa, feats=feats)
    assert (radii == 0).any() and (radii > 0).any()
    for k in terms:
        e = image_err(img[k], rimg[k])
        print("%-8s image %.3e" % (k, e))
        assert e < TOL, (k, e)
    for k, v in got.items():
        e = rel_err(v, ref[k].reshape(v.shape))
        print("%-8s %.3e" % (k, e))
        assert e < TOL, (k, e)
    _sh_rows(got["sh"], spec, radii, case["P"])


# ------------------------------------------------------------------------------------------------ 6. batched backward
def _views_backward(cases, sh, dpix, batched):
    """the loss sum_i (colour_i * dpix_i).sum() through one rasterize_views call or one GaussianRasterizer call per view -> gradients:
    sh / opacity / scale of the shared tensors (summed over the views), mean3D_i / rot_i / mean2D_i per view"""
    import diff_gaussian_rasterization as dgr
    V, P, g0 = len(cases), cases[0]["P"], cases[0]["g"]
    sh.grad = None
    op, sc = _T(g0["opacities"]), _T(g0["scales"])
    kws = [dict(means3D=_T(c["g"]["means3D"]), means2D=torch.zeros(P, 3, device="cuda", requires_grad=True), opacities=op, shs=sh, scales=sc,
                rotations=_T(c["g"]["rotations"])) for c in cases]
    settings = [util.gpu_settings(c) for c in cases]
    outs = dgr.rasterize_views(settings, kws) if batched else [dgr.GaussianRasterizer(settings[i])(**kws[i]) for i in range(V)]
    sum((outs[i][0] * _T(dpix[i], False)).sum() for i in range(V)).backward()
    torch.cuda.synchronize()
    got = dict(sh=sh.grad, opacity=op.grad, scale=sc.grad)
    for i, kw in enumerate(kws):
        got.update({"mean3D_%d" % i: kw["means3D"].grad, "rot_%d" % i: kw["rotations"].grad, "mean2D_%d" % i: kw["means2D"].grad})
    return {k: v.detach().cpu().numpy().astype(np.float64) for k, v in got.items()}, [o[1].cpu().numpy() for o in outs]


@pytest.mark.parametrize("flags,tol", [(BIT_REPRODUCIBLE, 1e-6), (0, 1e-5)], ids=["bit_reproducible", "atomics"])
@pytest.mark.parametrize("spec", FORM_SPECS, ids=_id)
@pytest.mark.parametrize("V", [2, 4])
def test_batched_backward_with_a_shared_unstaged_sh_tensor(V, spec, flags, tol):
    """Views that share an SH tensor the library cannot stage: k8_views_table keeps the per-view K8, whose unstaged form cannot add into
    a shared dL_dsh -- the plan gives every view a dL_dsh of its own (autograd sums them).  With M = 16 off a 16-byte boundary the plan
    used to share the buffer on M == 16 alone, and the backward raised "accumulating dL_dsh needs M == 16 and 16-byte aligned buffers"."""
    cases, shs = _view_cases(V, spec, P=800, W=64, H=64)
    P = cases[0]["P"]
    sh = _sh_tensors(shs, spec)[0]
    dpix = [np.random.default_rng(40 + i).normal(size=(3, 64, 64)).astype(np.float32) for i in range(V)]
    _flags(flags)
    try:
        got, radii = _views_backward(cases, sh, dpix, True)
        single, _ = _views_backward(cases, sh, dpix, False)
    finally:
        _flags(0)
    ref = dict(sh=0.0, opacity=0.0, scale=0.0)
    for i, c in enumerate(cases):
        o64 = oracle_forward(c, dtype=np.float64)
        np.testing.assert_array_equal(radii[i], o64.radii)
        g = util.ro.backward(o64, dpix[i])
        ref["sh"], ref["opacity"], ref["scale"] = ref["sh"] + g.sh, ref["opacity"] + g.opacity.reshape(P, 1), ref["scale"] + g.scale
        ref.update({"mean3D_%d" % i: g.mean3D, "rot_%d" % i: g.rot, "mean2D_%d" % i: g.mean2D})
    assert got.keys() == single.keys() == ref.keys()
    for k in got:
        e64, e1 = rel_err(got[k], ref[k]), rel_err(got[k], single[k])
        print("%-10s against fp64 %.3e, against the per-view calls %.3e" % (k, e64, e1))
        assert e64 < TOL, (k, e64)
        assert e1 < tol, (k, e1)
    seen = np.any([r > 0 for r in radii], 0)
    _sh_rows(got["sh"], spec, seen.astype(np.int32), P)


# ------------------------------------------------------------------------------------------------ 7. through the model
def _model_scene(M):
    sc = util.syn.scene_1(P=1000, W=64, H=64, n_cams=3, grid=8, n_times=5, seed=31)
    sc["log_scales"] = sc["log_scales"] + np.log(2.5)
    sc["sh"] = np.ascontiguousarray(sc["sh"][:, :M])
    return sc


def _model(sc, deg, dev, dt):
    from csplat.gaussians import MeshGaussians
    from meshnet.meshnet_network import ResidualMeshSimulator
    T = lambda a, d=dt: torch.tensor(a, device=dev, dtype=d)  # noqa: E731
    pc = MeshGaussians(deg).from_arrays(T(sc["mesh_pos"][0]), T(sc["faces"].T.copy(), torch.long), T(sc["edge_index"], torch.long),
                                        T(sc["face_ids"], torch.long), T(sc["bary"]), T(sc["log_scales"]), T(sc["quats"]),
                                        T(sc["opacity_logits"]), T(sc["sh"]))
    pc.active_sh_degree = deg
    sim = ResidualMeshSimulator(T(sc["mesh_pos"]), device=dev)
    return pc, sim


def _cameras(sc, times, dt):
    t = lambda a: torch.tensor(a).to(dt)  # noqa: E731
    return [SimpleNamespace(image_height=c["image_height"], image_width=c["image_width"], FoVx=c["FoVx"], FoVy=c["FoVy"],
                            world_view_transform=t(c["world_view_transform"]), full_proj_transform=t(c["full_proj_transform"]),
                            camera_center=t(c["camera_center"]), time=time) for c, time in zip(sc["cameras"], times)]


@pytest.mark.allow_fallbacks("shape")
@pytest.mark.parametrize("deg", [0, 1, 2])
def test_render_views_of_a_low_degree_model_matches_fp64(deg):
    """gaussian_renderer.render_views on a MeshGaussians of sh_degree 0, 1, 2 (M = 1, 4, 9: the fused activations do not apply -- reported
    as the composed fallback of kind "shape", and nothing else is) against util.oracle_render_views on its fp64 CPU copy"""
    from csplat import native
    from gaussian_renderer import render_views
    M = (deg + 1) ** 2
    sc = _model_scene(M)
    times = (0.25, 0.5, 0.75)
    pipe = SimpleNamespace(compute_cov3D_python=False, convert_SHs_python=False, debug=False)
    wts = [np.random.default_rng(70 + i).normal(size=(3, 64, 64)) for i in range(len(times))]
    pc, sim = _model(sc, deg, "cuda", torch.float32)
    with torch.no_grad():
        torch.manual_seed(0)
        sim.output.weight.normal_(0, 1e-3)
    before = collections.Counter(native.FALLBACK_COUNTS)
    assert pc.activations() is None
    res = render_views(_cameras(sc, times, torch.float32), pc, sim, pipe, torch.ones(3, device="cuda"))
    reported = collections.Counter(native.FALLBACK_COUNTS) - before
    assert set(reported) == {("MeshGaussians.activations", "shape")}, reported
    sum((r.render * _T(w, False)).sum() for r, w in zip(res, wts)).backward()
    torch.cuda.synchronize()
    # the fp64 CPU copy: the same parameters, the torch formulation of the mesh transform, the oracle as the rasterizer
    pc64, sim64 = _model(sc, deg, "cpu", torch.float64)
    pc64.fused = False
    sim64 = sim64.double()
    with torch.no_grad():
        for p64, p in zip(sim64.parameters(), sim.parameters()):
            p64.copy_(p.detach().cpu().double())
    res64, _ = util.oracle_render_views(_cameras(sc, times, torch.float64), pc64, sim64, pipe, torch.ones(3, dtype=torch.float64))
    sum((r.render * torch.tensor(w)).sum() for r, w in zip(res64, wts)).backward()
    P = sc["face_ids"].shape[0]
    for i, (r, r64) in enumerate(zip(res, res64)):
        e = image_err(r.render.detach().cpu().numpy(), r64.render.detach().numpy())
        print("view %d image %.3e" % (i, e))
        assert e < TOL, (i, e)
    assert tuple(pc._features_rest.shape) == (P, M - 1, 3)
    for name in ("_features_dc", "_features_rest", "_opacity", "_scaling"):
        p, p64 = getattr(pc, name), getattr(pc64, name)
        if p.numel() == 0:      # (sh_degree 0: no coefficient beyond the first)
            assert p.grad is None or tuple(p.grad.shape) == (P, 0, 3)
            continue
        assert p.grad is not None and tuple(p.grad.shape) == tuple(p.shape), name
        e = rel_err(p.grad.cpu().numpy(), p64.grad.numpy())
        print("%-15s %.3e" % (name, e))
        assert e < TOL, (name, e)
