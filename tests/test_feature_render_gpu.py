"""Feature channels and the alpha image of the rasterizer (include/csplat.h, csplat_view.features .. dL_dfeat_in): forward images and every
input gradient against tests/feature_ref.py (fp64 autograd), identities with the colour path, the unchanged default path,
reproducibility, batched against per-view calls, the errors, and the flagship shape.  Bars: the colour image's (util.image_err 1e-4) for
the images, 1e-4 relative (util.rel_err) for gradients."""
import numpy as np
import pytest

import util
import feature_ref
from util import image_err, make_case, oracle_forward, rel_err

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

TOL = 1e-4
CASES = [
    dict(P=2000, W=128, H=96, seed=7, grid=20, scale_mul=1.0),
    dict(P=3000, W=200, H=136, seed=8, grid=16, scale_mul=2.5),     # ragged: W,H not multiples of 16
    dict(P=800, W=64, H=64, seed=9, grid=10, scale_mul=4.0, radius=1.2),  # close camera: frustum clamp + culling
]
FS = [1, 2, 5, 6]
LOSSES = ["feat", "alpha", "cfa", "cfad", "cfadc"]     # c colour, f features, a alpha, d depth, c camera (campos / viewmatrix)


def _flags(f):
    from csplat import native
    native.lib.csplat_debug_flags(f)


def _features(case, F, seed=5):
    return np.random.default_rng(seed).normal(size=(case["P"], F)).astype(np.float32)


def _weights(case, F, seed=11):
    rng = np.random.default_rng(seed)
    H, W = case["H"], case["W"]
    return dict(color=rng.normal(size=(3, H, W)), depth=rng.normal(size=(1, H, W)), feat=rng.normal(size=(F, H, W)),
                alpha=rng.normal(size=(1, H, W)))


def _precomp_extra(case):
    o0 = oracle_forward(case, dtype=np.float64)
    rng = np.random.default_rng(5)
    return dict(colors=rng.uniform(0, 1, size=(case["P"], 3)).astype(np.float32), cov3D=o0.cov3D.astype(np.float32))


def _loss(outs, wts, loss, lib):
    color, depth, feat, alpha = outs
    t = (lambda a: torch.tensor(a, dtype=torch.float32, device="cuda")) if lib == "gpu" else torch.tensor  # noqa: E731
    L = 0.0
    if loss != "alpha":
        L = L + (feat * t(wts["feat"])).sum()
    if loss != "feat":
        L = L + (alpha * t(wts["alpha"])).sum()
    if loss.startswith("cfa"):
        L = L + (color * t(wts["color"])).sum()
    if loss.startswith("cfad"):
        L = L + (depth * t(wts["depth"])).sum()
    return L


def _gpu(case, feats, wts, loss, mode="sh", extra=None):
    import diff_gaussian_rasterization as dgr
    inp = util.gpu_inputs(case)
    rs = util.gpu_settings(case)
    cam = {}
    if loss == "cfadc":
        c = case["cam"]
        cam = dict(campos=torch.tensor(np.asarray(c["camera_center"], np.float32), device="cuda", requires_grad=True),
                   view=torch.tensor(np.asarray(c["world_view_transform"], np.float32), device="cuda", requires_grad=True))
        rs = rs._replace(campos=cam["campos"], viewmatrix=cam["view"])
    T = lambda a: torch.tensor(np.asarray(a, np.float32), device="cuda", requires_grad=True)  # noqa: E731
    kw = dict(colors_precomp=T(extra["colors"]), cov3D_precomp=T(extra["cov3D"])) if mode == "precomp" else \
        dict(shs=inp["shs"], scales=inp["scales"], rotations=inp["rotations"])
    f = T(feats)
    color, _r, depth, feat, alpha = dgr.GaussianRasterizer(rs)(means3D=inp["means3D"], means2D=inp["means2D"], opacities=inp["opacities"],
                                                               features=f, return_alpha=True, **kw)
    _loss((color, depth, feat, alpha), wts, loss, "gpu").backward()
    torch.cuda.synchronize()
    got = dict(mean3D=inp["means3D"].grad, mean2D=inp["means2D"].grad, opacity=inp["opacities"].grad.reshape(-1), features=f.grad)
    if mode == "precomp":
        got.update(colors=kw["colors_precomp"].grad, cov3D=kw["cov3D_precomp"].grad)
    else:
        got.update(sh=inp["shs"].grad, scale=inp["scales"].grad, rot=inp["rotations"].grad)
    got.update({k: v.grad for k, v in cam.items()})
    return {k: (v.detach().cpu().numpy().astype(np.float64) if v is not None else None) for k, v in got.items()}


def _ref(case, feats, wts, loss, mode="sh", extra=None):
    g, P = case["g"], case["P"]
    T = lambda a: torch.tensor(np.asarray(a, np.float64), requires_grad=True)  # noqa: E731
    if mode == "precomp":
        o = oracle_forward(case, dtype=np.float64, shs=None, colors_precomp=extra["colors"], scales=None, rotations=None,
                           cov3D_precomp=extra["cov3D"])
        ins = dict(colors_precomp=T(extra["colors"]), cov3D_precomp=T(extra["cov3D"]))
    else:
        o = oracle_forward(case, dtype=np.float64)
        ins = dict(shs=T(g["shs"]), scales=T(g["scales"]), rotations=T(g["rotations"]))
    V, Pm, campos, bg = feature_ref.camera_tensors(o)
    m3, m2, op, f = T(g["means3D"]), T(np.zeros((P, 3))), T(g["opacities"]), T(feats)
    outs = feature_ref.render(o, m3, m2, op, V, Pm, campos, bg, f, **ins)
    _loss(outs, wts, loss, "ref").backward()
    ref = dict(mean3D=m3.grad, mean2D=m2.grad, opacity=op.grad.reshape(-1), features=f.grad, campos=campos.grad, view=V.grad)
    if mode == "precomp":
        ref.update(colors=ins["colors_precomp"].grad, cov3D=ins["cov3D_precomp"].grad)
    else:
        ref.update(sh=ins["shs"].grad, scale=ins["scales"].grad, rot=ins["rotations"].grad)
    return {k: (v.numpy() if v is not None else None) for k, v in ref.items()}, [t.detach().numpy() for t in outs]


@pytest.mark.parametrize("F", FS)
@pytest.mark.parametrize("ci", range(len(CASES)))
def test_forward_images_match_fp64(ci, F):
    import diff_gaussian_rasterization as dgr
    case = make_case(**CASES[ci])
    feats = _features(case, F)
    inp = util.gpu_inputs(case, requires_grad=False)
    color, _r, _d, feat, alpha = dgr.GaussianRasterizer(util.gpu_settings(case))(
        means3D=inp["means3D"], means2D=inp["means2D"], opacities=inp["opacities"], shs=inp["shs"], scales=inp["scales"],
        rotations=inp["rotations"], features=torch.tensor(feats, device="cuda"), return_alpha=True)
    torch.cuda.synchronize()
    assert tuple(feat.shape) == (F, case["H"], case["W"]) and tuple(alpha.shape) == (1, case["H"], case["W"])
    _g, (c64, _d64, f64, a64) = _ref(case, feats, _weights(case, F), "feat")
    assert image_err(color.cpu().numpy(), c64) < TOL
    assert image_err(feat.cpu().numpy(), f64) < TOL
    assert image_err(alpha.cpu().numpy(), a64) < TOL
    # color = sum T alpha c + (1 - alpha) bg holds with the returned alpha
    assert float(alpha.min()) >= 0.0 and float(alpha.max()) <= 1.0 and float(alpha.max()) > 0.5


@pytest.mark.parametrize("mode", ["sh", "precomp"])
@pytest.mark.parametrize("loss", LOSSES)
@pytest.mark.parametrize("ci", range(len(CASES)))
def test_gradients_match_fp64_autograd(ci, loss, mode):
    case = make_case(**CASES[ci])
    F = FS[(ci + LOSSES.index(loss)) % len(FS)]
    feats, wts = _features(case, F), _weights(case, F)
    extra = _precomp_extra(case) if mode == "precomp" else None
    got = _gpu(case, feats, wts, loss, mode, extra)
    ref, _outs = _ref(case, feats, wts, loss, mode, extra)
    for k, v in got.items():
        if k == "features" and loss == "alpha":
            assert np.all(v == 0.0)    # (the feature image takes no gradient: the feature path hands the features exact zeros)
            continue
        if ref[k] is None:         # (campos with colors_precomp: no path from the camera centre to the loss)
            assert np.all(v == 0.0), k
            continue
        e = rel_err(v, ref[k])
        assert e < TOL, (k, e)


def _identity_pair(case, c, cprime, dpix, flags=256):
    """(feature-loss call with features = c, colors_precomp = c'; colour-loss call with colors_precomp = c), bg = 0, the same weights"""
    import diff_gaussian_rasterization as dgr
    extra = _precomp_extra(case)
    rs = util.gpu_settings(case)
    rs = rs._replace(bg=torch.zeros(3, device="cuda"))
    res = []
    _flags(flags)
    try:
        for use_feat in (True, False):
            inp = util.gpu_inputs(case)
            T = lambda a: torch.tensor(np.asarray(a, np.float32), device="cuda", requires_grad=True)  # noqa: E731
            cov, f = T(extra["cov3D"]), T(c)
            cp = T(cprime if use_feat else c)
            out = dgr.GaussianRasterizer(rs)(means3D=inp["means3D"], means2D=inp["means2D"], opacities=inp["opacities"], colors_precomp=cp,
                                             cov3D_precomp=cov, **(dict(features=f) if use_feat else {}))
            img = out[3] if use_feat else out[0]
            (img * torch.tensor(dpix, dtype=torch.float32, device="cuda")).sum().backward()
            torch.cuda.synchronize()
            res.append(dict(img=img.detach(), c=(f if use_feat else cp).grad, mean3D=inp["means3D"].grad, mean2D=inp["means2D"].grad,
                            opacity=inp["opacities"].grad, cov3D=cov.grad))
    finally:
        _flags(0)
    return res


@pytest.mark.parametrize("ci", range(len(CASES)))
def test_feature_identity_with_colour(ci):
    """features = c (F = 3), colors_precomp = c', bg = 0: a loss on the feature image gives features.grad and every Gaussian gradient of a
    colour loss with colors_precomp = c.  Not bit-equal, in flag 256 either: the feature path forms each entry's 'behind' term as (this and
    later segments' partials) - (in-segment prefix), the colour path as (the finished pixel) - (prefix), and its per-entry sums associate
    differently.  Measured: the image and features.grad against colors_precomp.grad within 1e-6 relative; the Gaussian gradients
    (opacity, means2D, means3D, cov3D), which take the cancelling behind terms through dL/dalpha, up to 3.4e-6 -- hence 1e-5 for those."""
    case = make_case(**CASES[ci])
    rng = np.random.default_rng(2)
    c, cprime = rng.uniform(0, 1, size=(case["P"], 3)), rng.uniform(0, 1, size=(case["P"], 3))
    dpix = rng.normal(size=(3, case["H"], case["W"]))
    a, b = _identity_pair(case, c, cprime, dpix)
    assert rel_err(a["img"].cpu().numpy(), b["img"].cpu().numpy()) < 1e-6
    for k in ("c", "mean3D", "mean2D", "opacity", "cov3D"):
        e = rel_err(a[k].cpu().numpy(), b[k].cpu().numpy())
        assert e <= (1e-6 if k == "c" else 1e-5), (k, e)


def _plain_call(case, dpix, features=None, loss_feat=False):
    import diff_gaussian_rasterization as dgr
    inp = util.gpu_inputs(case)
    extra = {} if features is None else dict(features=torch.tensor(features, device="cuda", requires_grad=True), return_alpha=True)
    out = dgr.GaussianRasterizer(util.gpu_settings(case))(
        means3D=inp["means3D"], means2D=inp["means2D"], opacities=inp["opacities"], shs=inp["shs"], scales=inp["scales"],
        rotations=inp["rotations"], **extra)
    loss = (out[0] * torch.tensor(dpix, dtype=torch.float32, device="cuda")).sum()
    if loss_feat:
        loss = loss + out[3].sum() + out[4].sum()
    loss.backward()
    torch.cuda.synchronize()
    grads = [inp[k].grad.clone() for k in ("means3D", "means2D", "opacities", "shs", "scales", "rotations")]
    return [t.detach().clone() for t in out[:3]], grads, (extra["features"].grad if extra else None)


@pytest.mark.parametrize("spec", [True, False])
def test_default_path_unchanged(spec, monkeypatch):
    """bit-reproducible mode: calls without the new arguments give the same bits before and after feature calls; with features given
    but a colour-only loss the Gaussian gradients are bit-equal to the call without features and features.grad stays None"""
    import diff_gaussian_rasterization as dgr
    monkeypatch.setattr(dgr, "PER_CALL_SPECULATION", spec)
    case = make_case(**CASES[1])
    dpix = np.random.default_rng(4).normal(size=(3, case["H"], case["W"]))
    feats = _features(case, 4)
    _flags(256)
    try:
        o0, g0, _ = _plain_call(case, dpix)
        o1, g1, fg1 = _plain_call(case, dpix, feats)
        _o2, _g2, fg2 = _plain_call(case, dpix, feats, loss_feat=True)
        o3, g3, _ = _plain_call(case, dpix)
    finally:
        _flags(0)
    assert fg1 is None and fg2 is not None and float(fg2.abs().max()) > 0
    for a, b, c in zip(o0, o1, o3):
        assert torch.equal(a, b) and torch.equal(a, c)
    for a, b, c in zip(g0, g1, g3):
        assert torch.equal(a, b) and torch.equal(a, c)


def test_default_mode_unchanged_after_feature_calls():
    """default mode: a plain call's outputs are bit-equal before and after feature calls (its gradients meet float atomics: 1e-5)"""
    case = make_case(**CASES[0])
    dpix = np.random.default_rng(4).normal(size=(3, case["H"], case["W"]))
    o0, g0, _ = _plain_call(case, dpix)
    _plain_call(case, dpix, _features(case, 2), loss_feat=True)
    o1, g1, _ = _plain_call(case, dpix)
    for a, b in zip(o0, o1):
        assert torch.equal(a, b)
    for a, b in zip(g0, g1):
        assert rel_err(b.cpu().numpy(), a.cpu().numpy()) < 1e-5


def _views(V=3, P=2000, W=128, H=96, seed=7):
    from csplat import synthetic as syn
    base = make_case(P=P, W=W, H=H, seed=seed)
    return [dict(base, cam=syn.make_camera(-40.0 + 35.0 * i, W, H)) for i in range(V)]


def test_reproducible_and_batched_equals_per_view():
    """flag 256: two identical feature calls are bit-equal, and rasterize_views with features over 3 views gives the per-view calls'
    feature / alpha images and features gradients bit for bit (each view its own feature tensor)"""
    import diff_gaussian_rasterization as dgr
    cases = _views(3)
    P, H, W = cases[0]["P"], cases[0]["H"], cases[0]["W"]
    rng = np.random.default_rng(3)
    feats = [rng.normal(size=(P, 2)).astype(np.float32) for _ in range(3)]
    wf = [rng.normal(size=(2, H, W)).astype(np.float32) for _ in range(3)]
    wa = [rng.normal(size=(1, H, W)).astype(np.float32) for _ in range(3)]
    wc = [rng.normal(size=(3, H, W)).astype(np.float32) for _ in range(3)]
    t = lambda a: torch.tensor(a, device="cuda")  # noqa: E731

    def per_view():
        inp = util.gpu_inputs(cases[0])
        fs = [torch.tensor(f, device="cuda", requires_grad=True) for f in feats]
        imgs = []
        for i, c in enumerate(cases):
            col, _r, _d, feat, alpha = dgr.GaussianRasterizer(util.gpu_settings(c))(
                means3D=inp["means3D"], means2D=torch.zeros(P, 3, device="cuda"), opacities=inp["opacities"], shs=inp["shs"],
                scales=inp["scales"], rotations=inp["rotations"], features=fs[i], return_alpha=True)
            ((col * t(wc[i])).sum() + (feat * t(wf[i])).sum() + (alpha * t(wa[i])).sum()).backward()
            imgs += [feat.detach(), alpha.detach()]
        torch.cuda.synchronize()
        return imgs, [f.grad for f in fs]

    def batched():
        inp = util.gpu_inputs(cases[0])
        fs = [torch.tensor(f, device="cuda", requires_grad=True) for f in feats]
        kws = [dict(means3D=inp["means3D"], means2D=torch.zeros(P, 3, device="cuda"), opacities=inp["opacities"], shs=inp["shs"],
                    scales=inp["scales"], rotations=inp["rotations"], features=fs[i], return_alpha=True) for i in range(3)]
        outs = dgr.rasterize_views([util.gpu_settings(c) for c in cases], kws)
        sum((o[0] * t(wc[i])).sum() + (o[3] * t(wf[i])).sum() + (o[4] * t(wa[i])).sum() for i, o in enumerate(outs)).backward()
        torch.cuda.synchronize()
        return [x.detach() for o in outs for x in o[3:]], [f.grad for f in fs]

    _flags(256)
    try:
        a, b, c = per_view(), per_view(), batched()
    finally:
        _flags(0)
    for x, y, z in zip(a[0] + a[1], b[0] + b[1], c[0] + c[1]):
        assert torch.equal(x, y) and torch.equal(x, z)


def test_shared_features_sum_over_views():
    """one feature tensor passed to every view of rasterize_views: its gradient is the sum of the per-view calls' (stacked output)"""
    import diff_gaussian_rasterization as dgr
    cases = _views(3)
    P, H, W = cases[0]["P"], cases[0]["H"], cases[0]["W"]
    rng = np.random.default_rng(6)
    wf = torch.tensor(rng.normal(size=(3, 2, H, W)).astype(np.float32), device="cuda")
    inp = util.gpu_inputs(cases[0], requires_grad=False)
    f = torch.tensor(rng.normal(size=(P, 2)).astype(np.float32), device="cuda", requires_grad=True)
    kws = [dict(means3D=inp["means3D"], means2D=torch.zeros(P, 3, device="cuda"), opacities=inp["opacities"], shs=inp["shs"],
                scales=inp["scales"], rotations=inp["rotations"], features=f) for _ in range(3)]
    colors, outs = dgr.rasterize_views([util.gpu_settings(c) for c in cases], kws, stacked=True)
    assert tuple(colors.shape) == (3, 3, H, W) and all(len(o) == 4 for o in outs)
    sum((outs[i][3] * wf[i]).sum() for i in range(3)).backward()
    tot = torch.zeros(P, 2, device="cuda", dtype=torch.float64)
    for i in range(3):
        f1 = f.detach().clone().requires_grad_(True)
        out = dgr.GaussianRasterizer(util.gpu_settings(cases[i]))(**dict(kws[i], features=f1))
        (out[3] * wf[i]).sum().backward()
        tot += f1.grad.double()
    torch.cuda.synchronize()
    assert rel_err(f.grad.cpu().numpy(), tot.cpu().numpy()) < 1e-6


def test_errors():
    import diff_gaussian_rasterization as dgr
    from csplat import graphs
    case = make_case(**CASES[0])
    inp = util.gpu_inputs(case)
    rs = util.gpu_settings(case)
    kw = dict(means3D=inp["means3D"], means2D=inp["means2D"], opacities=inp["opacities"], shs=inp["shs"], scales=inp["scales"],
              rotations=inp["rotations"])
    P = case["P"]
    for bad in (torch.zeros(P, 2, device="cuda", dtype=torch.float64), torch.zeros(P - 1, 2, device="cuda"), torch.zeros(P, 7, device="cuda"),
                torch.zeros(P, 0, device="cuda"), torch.zeros(P, 2), torch.zeros(P, device="cuda")):
        with pytest.raises(ValueError):
            dgr.GaussianRasterizer(rs)(**kw, features=bad)
    cases = _views(2)
    kws = [dict(kw, means2D=torch.zeros(P, 3, device="cuda", requires_grad=True)) for _ in range(2)]
    settings = [util.gpu_settings(c) for c in cases]
    with pytest.raises(ValueError, match="same number of feature channels"):
        dgr.rasterize_views(settings, [dict(kws[0], features=torch.zeros(P, 2, device="cuda")),
                                       dict(kws[1], features=torch.zeros(P, 3, device="cuda"))])
    # a forward launched on faith renders no feature / alpha image
    _out, counts = graphs.counts_of_eager(lambda: dgr.rasterize_views(settings, kws, stacked=True))
    faith = {"caps": graphs.caps_from_counts(counts), "valid": torch.zeros(1, dtype=torch.int32, device="cuda")}
    with dgr.forward_mode(faith=faith):
        with pytest.raises(RuntimeError, match="on faith"):
            dgr.rasterize_views(settings, [dict(k, return_alpha=True) for k in kws], stacked=True)
        with pytest.raises(RuntimeError, match="on faith"):
            dgr.GaussianRasterizer(rs)(**kw, features=torch.zeros(P, 2, device="cuda"))
    torch.cuda.synchronize()
    assert dgr.forward_mode_is_default()
    # deferred_k8(): a feature or alpha gradient raises, a colour-only loss of the same call does not reach the feature path
    f = torch.zeros(P, 2, device="cuda", requires_grad=True)
    colors, outs = dgr.rasterize_views(settings, [dict(k, features=f, return_alpha=True) for k in kws], stacked=True)
    with pytest.raises(RuntimeError, match="deferred_k8"):
        with dgr.deferred_k8():
            (outs[0][3].sum() + outs[1][4].sum()).backward()
    torch.cuda.synchronize()


def test_flagship_identities():
    """P = 100 000, 4 views of 800 x 800: with features = colors_precomp (F = 3) and bg = 0 the feature image is the colour image and
    features.grad is the colour-loss call's colors_precomp.grad; the alpha image is the colour of an all-ones render with bg = 0"""
    import diff_gaussian_rasterization as dgr
    from csplat import synthetic as syn
    P, S, NV = 100_000, 800, 4
    sc = syn.scene_1(P=P, W=S, H=S, n_cams=NV, seed=0)
    g = syn.gaussians_at(sc)
    T = lambda x, rg=False: torch.tensor(np.asarray(x, np.float32), device="cuda", requires_grad=rg)  # noqa: E731
    inp = {k: T(g[k]) for k in ("means3D", "opacities", "scales", "rotations")}
    c = torch.rand(P, 3, device="cuda", generator=torch.Generator(device="cuda").manual_seed(0))
    settings = [dgr.GaussianRasterizationSettings(
        image_height=S, image_width=S, tanfovx=cm["tanfovx"], tanfovy=cm["tanfovy"], bg=torch.zeros(3, device="cuda"), scale_modifier=1.0,
        viewmatrix=T(cm["world_view_transform"]), projmatrix=T(cm["full_proj_transform"]), sh_degree=3, campos=T(cm["camera_center"]),
        prefiltered=False, debug=False) for cm in sc["cameras"][:NV]]
    w = torch.rand(NV, 3, S, S, device="cuda", generator=torch.Generator(device="cuda").manual_seed(1)) - 0.5

    def run(colors, features):
        cp = colors.clone().requires_grad_(True)
        f = features.clone().requires_grad_(True)
        kws = [dict(means3D=inp["means3D"], means2D=torch.zeros(P, 3, device="cuda"), opacities=inp["opacities"], colors_precomp=cp,
                    scales=inp["scales"], rotations=inp["rotations"], features=f, return_alpha=True) for _ in range(NV)]
        colors_img, outs = dgr.rasterize_views(settings, kws, stacked=True)
        return cp, f, colors_img, torch.stack([o[3] for o in outs]), torch.stack([o[4] for o in outs])

    cp, f, col, feat, alpha = run(c, c)
    assert rel_err(feat.detach().cpu().numpy(), col.detach().cpu().numpy()) < 1e-5
    _cp1, _f1, col1, _feat1, _alpha1 = run(torch.ones(P, 3, device="cuda"), c)
    for ch in range(3):
        assert rel_err(alpha[:, 0].detach().cpu().numpy(), col1[:, ch].detach().cpu().numpy()) < 1e-5
    (feat * w).sum().backward()
    cp2, _f2, col2, _feat2, _alpha2 = run(c, c)
    (col2 * w).sum().backward()
    torch.cuda.synchronize()
    assert float(f.grad.abs().max()) > 0
    assert rel_err(f.grad.cpu().numpy(), cp2.grad.cpu().numpy()) < 1e-5
