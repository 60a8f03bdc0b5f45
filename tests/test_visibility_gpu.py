"""Gaussian visibility and the top-contributor map (include/csplat.h, csplat_visibility_views; GaussianRasterizer.forward(return_visibility=
True)): the four outputs against tests/visibility_ref.py (fp64), identities with the feature / alpha path, occlusion by a folded-over layer
(the reason for the outputs: radii > 0 holds behind it too), bit-reproducibility in the default mode, batched against per-view calls, the
unchanged default path, render_visibility(), the errors and the flagship shape."""
import math
from types import SimpleNamespace

import numpy as np
import pytest

import util
import visibility_ref
from util import make_case, oracle_forward, rel_err

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

TOL = 1e-4
CASES = [
    dict(P=2000, W=128, H=96, seed=7, grid=20, scale_mul=1.0),
    dict(P=3000, W=200, H=136, seed=8, grid=16, scale_mul=2.5),     # ragged: W,H not multiples of 16
    dict(P=800, W=64, H=64, seed=9, grid=10, scale_mul=4.0, radius=1.2),  # close camera: frustum clamp + culling
]
PER_CALL_SPECULATION = [True, False]


def _flags(f):
    from csplat import native
    native.lib.csplat_debug_flags(f)


def _np(t):
    return t.detach().cpu().numpy()


def _precomp(case):
    o0 = oracle_forward(case, dtype=np.float64)
    rng = np.random.default_rng(5)
    return dict(colors=rng.uniform(0, 1, size=(case["P"], 3)).astype(np.float32), cov3D=o0.cov3D.astype(np.float32))


def _call(case, mode="sh", aa=False, extra=None, **kw):
    """GaussianRasterizer with return_visibility=True and return_alpha=True -> (radii, alpha [1,H,W], Visibility)"""
    import diff_gaussian_rasterization as dgr
    inp = util.gpu_inputs(case, requires_grad=False)
    T = lambda a: torch.tensor(np.asarray(a, np.float32), device="cuda")  # noqa: E731
    geo = dict(colors_precomp=T(extra["colors"]), cov3D_precomp=T(extra["cov3D"])) if mode == "precomp" else \
        dict(shs=inp["shs"], scales=inp["scales"], rotations=inp["rotations"])
    out = dgr.GaussianRasterizer(util.gpu_settings(case))(means3D=inp["means3D"], means2D=inp["means2D"], opacities=inp["opacities"],
                                                          return_alpha=True, return_visibility=True, antialiasing=aa, **geo, **kw)
    torch.cuda.synchronize()
    vis = out[-1]
    assert isinstance(vis, dgr.Visibility) and len(out) == 5
    return out[1], out[3], vis


def _ref(case, mode="sh", aa=False, extra=None, top_id=None):
    g = case["g"]
    f64 = lambda a: torch.tensor(np.asarray(a, np.float64))  # noqa: E731
    if mode == "precomp":
        o = oracle_forward(case, dtype=np.float64, shs=None, colors_precomp=extra["colors"], scales=None, rotations=None,
                           cov3D_precomp=extra["cov3D"])
        geo = dict(cov3D_precomp=f64(extra["cov3D"]))
    else:
        o = oracle_forward(case, dtype=np.float64)
        geo = dict(scales=f64(g["scales"]), rotations=f64(g["rotations"]))
    V, Pm, _campos, _bg = visibility_ref.antialias_ref.camera_tensors(o, False)
    return visibility_ref.visibility(o, f64(g["means3D"]), f64(g["opacities"]), V, Pm, antialiasing=aa, top_id=top_id, **geo)


def _check_consistent(radii, alpha, vis):
    """the identities that hold inside one GPU result"""
    wm, ws, pc, top = _np(vis.weight_max), _np(vis.weight_sum), _np(vis.pixel_count), _np(vis.top_id)
    assert vis.weight_max.dtype == torch.float32 and vis.weight_sum.dtype == torch.float32
    assert vis.pixel_count.dtype == torch.int32 and vis.top_id.dtype == torch.int32
    assert not vis.weight_max.requires_grad and not vis.weight_sum.requires_grad
    assert np.array_equal(wm > 0, pc > 0) and np.array_equal(ws > 0, pc > 0)
    assert np.all(_np(radii)[pc > 0] > 0)
    assert float(wm.max()) <= 0.99 and float(wm.min()) >= 0.0
    assert np.array_equal(top == -1, _np(alpha) == 0)
    ids = top[top >= 0]
    assert ids.max() < wm.shape[0]
    assert np.all(np.bincount(ids, minlength=wm.shape[0]) <= pc)
    a = _np(alpha).astype(np.float64)
    assert abs(ws.astype(np.float64).sum() - a.sum()) <= 1e-5 * a.sum()


@pytest.mark.parametrize("mode", ["sh", "precomp"])
@pytest.mark.parametrize("aa", [False, True])
@pytest.mark.parametrize("ci", range(len(CASES)))
def test_matches_restatement(ci, aa, mode):
    case = make_case(**CASES[ci])
    extra = _precomp(case) if mode == "precomp" else None
    radii, alpha, vis = _call(case, mode, aa, extra)
    _check_consistent(radii, alpha, vis)
    top = _np(vis.top_id)[0]
    ref = _ref(case, mode, aa, extra, top_id=top)
    assert rel_err(_np(vis.weight_max), ref["weight_max"]) < TOL
    assert rel_err(_np(vis.weight_sum), ref["weight_sum"]) < TOL
    # pixel counts: exact but for the pixels where an alpha sits on the 1/255 skip or a T on the 1e-4 stop within fp32 rounding (the ties
    # the oracle tests allow for): a handful of (Gaussian, pixel) pairs
    d = np.abs(_np(vis.pixel_count).astype(np.int64) - ref["pixel_count"])
    assert d.sum() <= max(4, 1e-3 * ref["pixel_count"].sum()), (int(d.sum()), int(ref["pixel_count"].sum()))
    # the chosen id's restated weight is within 1e-5 of the pixel's largest; -1 exactly where nothing blended
    hit = ref["top_w"] > 0
    assert np.all(ref["at_top"][hit] >= ref["top_w"][hit] - 1e-5)
    assert np.array_equal(top == -1, _np(alpha)[0] == 0)
    assert float(ref["top_w"].max()) > 0.2       # (case 0 antialiased: small footprints, o' < o)


@pytest.mark.parametrize("ci", range(len(CASES)))
def test_weight_sum_is_the_feature_gradient(ci):
    """weight_sum == features.grad for features = ones(P, 1) and loss = feat.sum() (the feature path's adjoint), at 1e-5"""
    import diff_gaussian_rasterization as dgr
    case = make_case(**CASES[ci])
    radii, alpha, vis = _call(case)
    inp = util.gpu_inputs(case, requires_grad=False)
    f = torch.ones(case["P"], 1, device="cuda", requires_grad=True)
    out = dgr.GaussianRasterizer(util.gpu_settings(case))(means3D=inp["means3D"], means2D=inp["means2D"], opacities=inp["opacities"],
                                                          shs=inp["shs"], scales=inp["scales"], rotations=inp["rotations"], features=f)
    out[3].sum().backward()
    torch.cuda.synchronize()
    assert rel_err(_np(vis.weight_sum), _np(f.grad)[:, 0]) < 1e-5
    assert torch.equal(out[1], radii)


def _sheets(W=128, H=128):
    """two parallel square sheets facing the camera: the front one dense and opaque enough to stop every pixel it covers, the back one
    smaller and entirely behind it.  -> (case-like dict, index of the first back-sheet Gaussian)"""
    from csplat import synthetic as syn
    cam = syn.make_camera(0.0, W, H)
    c = np.asarray(cam["camera_center"], np.float64)
    d = -c / np.linalg.norm(c)
    u = np.cross(d, [0.0, 0.0, 1.0])
    u /= np.linalg.norm(u)
    v = np.cross(u, d)

    def sheet(n, half, offset, sigma, opacity):
        s = np.linspace(-half, half, n)
        a, b = np.meshgrid(s, s, indexing="ij")
        pts = a.reshape(-1, 1) * u + b.reshape(-1, 1) * v + offset * d
        m = pts.shape[0]
        return pts, np.full((m, 3), sigma), np.full((m, 1), opacity)
    n_front = 60
    spacing = 1.6 / (n_front - 1)
    fp, fs, fo = sheet(n_front, 0.8, -0.2, 2 * spacing, 0.99)
    bp, bs, bo = sheet(20, 0.4, 0.2, 0.02, 0.9)
    g = dict(means3D=np.concatenate([fp, bp]).astype(np.float32), scales=np.concatenate([fs, bs]).astype(np.float32),
             opacities=np.concatenate([fo, bo]).astype(np.float32))
    P = g["means3D"].shape[0]
    g["rotations"] = np.tile(np.array([1.0, 0.0, 0.0, 0.0], np.float32), (P, 1))
    g["colors"] = np.random.default_rng(0).uniform(0, 1, size=(P, 3)).astype(np.float32)
    return dict(g=g, cam=cam, W=W, H=H, P=P, bg=np.zeros(3, np.float32), sh_degree=0), fp.shape[0]


def test_occluded_layer_is_not_visible():
    """a folded cloth in miniature: every Gaussian of the hidden sheet is inside the frustum (radii > 0, the visibility_filter of today) but
    blends into no pixel (pixel_count == 0, weight_max == 0) and dominates none (top_id never names it); the front sheet is seen"""
    import diff_gaussian_rasterization as dgr
    case, nf = _sheets()
    g = case["g"]
    T = lambda a: torch.tensor(a, device="cuda")  # noqa: E731
    color, radii, _depth, alpha, vis = dgr.GaussianRasterizer(util.gpu_settings(case))(
        means3D=T(g["means3D"]), means2D=torch.zeros(case["P"], 3, device="cuda"), opacities=T(g["opacities"]),
        colors_precomp=T(g["colors"]), scales=T(g["scales"]), rotations=T(g["rotations"]), return_alpha=True, return_visibility=True)
    torch.cuda.synchronize()
    r, pc, wm, top = _np(radii), _np(vis.pixel_count), _np(vis.weight_max), _np(vis.top_id)
    assert np.all(r[nf:] > 0)                                  # radii > 0 says "visible"
    assert np.all(pc[nf:] == 0) and np.all(wm[nf:] == 0)       # ... but nothing of the back sheet is seen
    assert not np.any(top >= nf)
    assert float((pc[:nf] > 0).mean()) > 0.9 and float(wm[:nf].max()) > 0.9
    _check_consistent(radii, alpha, vis)


def _vis_tuple(vis):
    return [t.clone() for t in vis]


def test_batched_equals_per_view_and_reproducible():
    """default mode (flags 0): rasterize_views over 3 views that differ in the flag gives the per-view calls' outputs bit for bit, and two
    runs are bit-identical in all four outputs"""
    import diff_gaussian_rasterization as dgr
    from csplat import synthetic as syn
    base = make_case(P=2000, W=128, H=96, seed=7)
    cases = [dict(base, cam=syn.make_camera(-40.0 + 35.0 * i, 128, 96)) for i in range(3)]
    inp = util.gpu_inputs(base, requires_grad=False)
    want = [True, False, True]
    kws = [dict(means3D=inp["means3D"], means2D=inp["means2D"], opacities=inp["opacities"], shs=inp["shs"], scales=inp["scales"],
                rotations=inp["rotations"], return_visibility=w) for w in want]

    def per_view():
        res = []
        for c, kw in zip(cases, kws):
            out = dgr.GaussianRasterizer(util.gpu_settings(c))(**kw)
            res.append([t.clone() for t in out[:3]] + (_vis_tuple(out[3]) if kw["return_visibility"] else []))
        torch.cuda.synchronize()
        return res

    def batched(stacked):
        outs = dgr.rasterize_views([util.gpu_settings(c) for c in cases], kws, stacked=stacked)
        if stacked:
            outs = outs[1]
        res = [[t.clone() for t in o[:3]] + (_vis_tuple(o[3]) if w else []) for o, w in zip(outs, want)]
        assert all(len(o) == (4 if w else 3) for o, w in zip(outs, want))
        torch.cuda.synchronize()
        return res

    a, b, c, d = per_view(), per_view(), batched(False), batched(True)
    for va, vb, vc, vd in zip(a, b, c, d):
        assert len(va) == len(vb) == len(vc) == len(vd)
        for x, y, z, w in zip(va, vb, vc, vd):
            assert torch.equal(x, y) and torch.equal(x, z) and torch.equal(x, w)
    assert float(a[0][3].max()) > 0


def _plain_call(case, dpix, vis=False):
    import diff_gaussian_rasterization as dgr
    inp = util.gpu_inputs(case)
    out = dgr.GaussianRasterizer(util.gpu_settings(case))(
        means3D=inp["means3D"], means2D=inp["means2D"], opacities=inp["opacities"], shs=inp["shs"], scales=inp["scales"],
        rotations=inp["rotations"], **(dict(return_visibility=True) if vis else {}))
    assert len(out) == (4 if vis else 3)
    (out[0] * torch.tensor(dpix, dtype=torch.float32, device="cuda")).sum().backward()
    torch.cuda.synchronize()
    grads = [inp[k].grad.clone() for k in ("means3D", "means2D", "opacities", "shs", "scales", "rotations")]
    return [t.detach().clone() for t in out[:3]], grads


class _CountingLib:
    """native.lib with a count of csplat_visibility_views calls"""

    def __init__(self, lib):
        self._lib, self.calls = lib, 0

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if name != "csplat_visibility_views":
            return fn

        def counted(*a):
            self.calls += 1
            return fn(*a)
        return counted


@pytest.mark.parametrize("spec", PER_CALL_SPECULATION)
def test_default_path_unchanged(spec, monkeypatch):
    """bit-reproducible mode: a call without the flag gives the same images and gradients before and after visibility calls, and with the
    flag the colour call's images and gradients are those of the call without it; without the flag the library's visibility entry point
    is never called"""
    import diff_gaussian_rasterization as dgr
    from csplat import native
    monkeypatch.setattr(dgr, "PER_CALL_SPECULATION", spec)
    counting = _CountingLib(native.lib)
    monkeypatch.setattr(native, "lib", counting)
    case = make_case(**CASES[1])
    dpix = np.random.default_rng(4).normal(size=(3, case["H"], case["W"]))
    _flags(256)
    try:
        o0, g0 = _plain_call(case, dpix)
        assert counting.calls == 0
        o1, g1 = _plain_call(case, dpix, vis=True)
        assert counting.calls == 1
        o2, g2 = _plain_call(case, dpix)
        assert counting.calls == 1
    finally:
        _flags(0)
    for a, b, c in zip(o0, o1, o2):
        assert torch.equal(a, b) and torch.equal(a, c)
    for a, b, c in zip(g0, g1, g2):
        assert torch.equal(a, b) and torch.equal(a, c)


def test_default_mode_unchanged_after_visibility_calls():
    """default mode: a plain call's outputs are bit-equal before and after visibility calls (its gradients meet float atomics: 1e-5)"""
    case = make_case(**CASES[0])
    dpix = np.random.default_rng(4).normal(size=(3, case["H"], case["W"]))
    o0, g0 = _plain_call(case, dpix)
    _plain_call(case, dpix, vis=True)
    o1, g1 = _plain_call(case, dpix)
    for a, b in zip(o0, o1):
        assert torch.equal(a, b)
    for a, b in zip(g0, g1):
        assert rel_err(b.cpu().numpy(), a.cpu().numpy()) < 1e-5


def test_render_visibility_equals_the_rasterizer_call():
    from gaussian_renderer import render_visibility, _prepare
    from diff_gaussian_rasterization import GaussianRasterizer, Visibility
    from csplat import synthetic as syn
    from csplat.gaussians import MeshGaussians
    from meshnet.meshnet_network import ResidualMeshSimulator
    sc = syn.scene_1(P=3000, W=160, H=120, n_cams=1, grid=14, n_times=5, seed=31)
    sc["log_scales"] = sc["log_scales"] + math.log(2.5)
    T = lambda a, dt=torch.float32: torch.tensor(a, device="cuda", dtype=dt)  # noqa: E731
    pc = MeshGaussians(3).from_arrays(T(sc["mesh_pos"][0]), T(sc["faces"].T.copy(), torch.long), T(sc["edge_index"], torch.long),
                                      T(sc["face_ids"], torch.long), T(sc["bary"]), T(sc["log_scales"]), T(sc["quats"]),
                                      T(sc["opacity_logits"]), T(sc["sh"]))
    pc.active_sh_degree = 3
    sim = ResidualMeshSimulator(T(sc["mesh_pos"]), device="cuda")
    c = sc["cameras"][0]
    cam = SimpleNamespace(image_height=c["image_height"], image_width=c["image_width"], FoVx=c["FoVx"], FoVy=c["FoVy"],
                          world_view_transform=torch.tensor(c["world_view_transform"]),
                          full_proj_transform=torch.tensor(c["full_proj_transform"]), camera_center=torch.tensor(c["camera_center"]),
                          time=0.5)
    bg = torch.ones(3, device="cuda")
    for aa in (False, True):
        pipe = SimpleNamespace(compute_cov3D_python=False, convert_SHs_python=False, debug=False, antialiasing=aa)
        got = render_visibility(cam, pc, sim, pipe, bg)
        assert isinstance(got, Visibility) and got.top_id.shape == (1, 120, 160)
        with torch.no_grad():
            settings, kwargs, _ = _prepare(cam, pc, sim, pipe, bg, 1.0, None, None, False)
            want = GaussianRasterizer(settings)(**kwargs, return_visibility=True)[-1]
        torch.cuda.synchronize()
        for x, y in zip(got, want):
            assert torch.equal(x, y)
        assert int((got.pixel_count > 0).sum()) > 100


def test_errors():
    """RuntimeError under forward_mode(faith=...) and in a captured / replayed step's recording scope; a pending or faith-launched view is
    refused by the library"""
    import diff_gaussian_rasterization as dgr
    from csplat import graphs
    from csplat import synthetic as syn
    case = make_case(**CASES[0])
    inp = util.gpu_inputs(case)
    rs = util.gpu_settings(case)
    kw = dict(means3D=inp["means3D"], means2D=inp["means2D"], opacities=inp["opacities"], shs=inp["shs"], scales=inp["scales"],
              rotations=inp["rotations"])
    P = case["P"]
    cases = [dict(case, cam=syn.make_camera(-40.0 + 35.0 * i, case["W"], case["H"])) for i in range(2)]
    kws = [dict(kw, means2D=torch.zeros(P, 3, device="cuda", requires_grad=True)) for _ in range(2)]
    settings = [util.gpu_settings(c) for c in cases]
    _out, counts = graphs.counts_of_eager(lambda: dgr.rasterize_views(settings, kws, stacked=True))
    faith = {"caps": graphs.caps_from_counts(counts), "valid": torch.zeros(1, dtype=torch.int32, device="cuda")}
    with dgr.forward_mode(faith=faith):
        with pytest.raises(RuntimeError, match="on faith"):
            dgr.rasterize_views(settings, [dict(k, return_visibility=True) for k in kws], stacked=True)
        with pytest.raises(RuntimeError, match="on faith"):
            dgr.GaussianRasterizer(rs)(**kw, return_visibility=True)
    with dgr.forward_mode(replay_device=torch.device("cuda", torch.cuda.current_device())):     # (the scope CapturedStep records in)
        with pytest.raises(RuntimeError, match="captured"):
            dgr.GaussianRasterizer(rs)(**kw, return_visibility=True)
    torch.cuda.synchronize()
    assert dgr.forward_mode_is_default()
    # the library itself: a pending view and a view launched on faith are refused, before any launch
    from csplat import native
    import ctypes as C
    arr = (native.CsplatView * 1)()
    outs = (native.CsplatVisibility * 1)()
    top = torch.empty(1, case["H"], case["W"], dtype=torch.int32, device="cuda")
    outs[0].top_id = top.data_ptr()
    arr[0].P, arr[0].W, arr[0].H, arr[0].num_rendered = P, case["W"], case["H"], -1
    stream = torch.cuda.current_stream().cuda_stream
    assert native.lib.csplat_visibility_views(1, C.cast(arr, C.c_void_p), C.cast(outs, C.c_void_p), stream) != 0
    assert b"pending" in native.lib.csplat_last_error()
    arr[0].num_rendered, arr[0].valid = 0, faith["valid"].data_ptr()
    assert native.lib.csplat_visibility_views(1, C.cast(arr, C.c_void_p), C.cast(outs, C.c_void_p), stream) != 0
    assert b"faith" in native.lib.csplat_last_error()
    assert native.lib.csplat_visibility_views(9, C.cast(arr, C.c_void_p), C.cast(outs, C.c_void_p), stream) != 0
    arr[0].valid, arr[0].num_rendered = None, 10
    assert native.lib.csplat_visibility_views(1, C.cast(arr, C.c_void_p), C.cast(outs, C.c_void_p), stream) != 0
    assert b"missing chunks" in native.lib.csplat_last_error()


def test_flagship_identities_and_reproducible():
    """P = 100 000, 4 views of 800 x 800: the identities above in every view, weight_sum against the all-ones feature gradient, and two runs
    bit-identical in all four outputs (default mode)"""
    import diff_gaussian_rasterization as dgr
    from csplat import synthetic as syn
    P, S, NV = 100_000, 800, 4
    sc = syn.scene_1(P=P, W=S, H=S, n_cams=NV, seed=0)
    g = syn.gaussians_at(sc)
    T = lambda x: torch.tensor(np.asarray(x, np.float32), device="cuda")  # noqa: E731
    inp = {k: T(g[k]) for k in ("means3D", "opacities", "shs", "scales", "rotations")}
    settings = [dgr.GaussianRasterizationSettings(
        image_height=S, image_width=S, tanfovx=cm["tanfovx"], tanfovy=cm["tanfovy"], bg=T(sc["bg"]), scale_modifier=1.0,
        viewmatrix=T(cm["world_view_transform"]), projmatrix=T(cm["full_proj_transform"]), sh_degree=3, campos=T(cm["camera_center"]),
        prefiltered=False, debug=False) for cm in sc["cameras"][:NV]]

    def run(feat=None):
        kws = [dict(means3D=inp["means3D"], means2D=torch.zeros(P, 3, device="cuda"), opacities=inp["opacities"], shs=inp["shs"],
                    scales=inp["scales"], rotations=inp["rotations"], return_alpha=True, return_visibility=True,
                    **({} if feat is None else dict(features=feat[i]))) for i in range(NV)]
        _colors, outs = dgr.rasterize_views(settings, kws, stacked=True)
        return outs

    a = run()
    b = run()
    torch.cuda.synchronize()
    for oa, ob in zip(a, b):
        for x, y in zip(oa[-1], ob[-1]):
            assert torch.equal(x, y)
        _check_consistent(oa[1], oa[3], oa[-1])
        assert int((oa[-1].pixel_count > 0).sum()) > 1000
    fs = [torch.ones(P, 1, device="cuda", requires_grad=True) for _ in range(NV)]
    c = run(fs)
    sum(o[3].sum() for o in c).backward()     # (o[3]: the feature image, o[4]: alpha)
    torch.cuda.synchronize()
    for i in range(NV):
        assert rel_err(_np(a[i][-1].weight_sum), _np(fs[i].grad)[:, 0]) < 1e-5
        for x, y in zip(a[i][-1], c[i][-1]):
            assert torch.equal(x, y)
