"""Antialiased rendering (include/csplat.h, CSPLAT_ANTIALIAS; GaussianRasterizer.forward(antialiasing=True)): colour, depth, feature and
alpha images and every input gradient -- camera and background included -- against tests/antialias_ref.py (fp64 autograd), the unchanged
default path, reproducibility, batched against per-view calls, launches on faith / replayed / captured steps / deferred_k8() slices
against the eager step, the renderer's pipeline flag, and the flagship shape.  Bars: util.image_err 1e-4 for images, util.rel_err 1e-4
for gradients."""
import math
from types import SimpleNamespace

import numpy as np
import pytest

import util
import antialias_ref
from util import image_err, make_case, oracle_forward, rel_err

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

TOL = 1e-4
CASES = [
    dict(P=2000, W=128, H=96, seed=7, grid=20, scale_mul=1.0),
    dict(P=3000, W=200, H=136, seed=8, grid=16, scale_mul=2.5),     # ragged: W,H not multiples of 16
    dict(P=800, W=64, H=64, seed=9, grid=10, scale_mul=4.0, radius=1.2),  # close camera: frustum clamp + culling
    dict(P=2000, W=128, H=96, seed=7, grid=20, scale_mul=1.0, thin=True),  # one scale axis at 1e-3 of the others: cloth seen edge-on
]
# The thin case.  Seen edge-on, a Gaussian with one axis at 1e-3 of the others projects to a nearly degenerate cov2D, and
# det0 = a0 c0 - b^2 cancels: its relative rounding is the entries' (fp32, ~6e-8) times kappa = (a0 c0 + b^2) / |det0|, and h and
# dh (which carries a 1 / h) inherit it.  Against fp64 that is no defect of the kernels, it is the fp32 input: a Gaussian with kappa =
# 1e6 has an fp32 h that is right only to a few per cent.  So the thin case renders the Gaussians with kappa <= KAPPA_MAX only (opacity 0
# for the others, in both runs: they are culled and take no gradient): 1.5 % of them at 1e3, about 5 % at 1e2.  With kappa <= 100 the
# expected relative error of h is <= 1e-5, an order below the bars, and h still spans the floor (0.005) to 0.7.
KAPPA_MAX = 100.0


def _flags(f):
    from csplat import native
    native.lib.csplat_debug_flags(f)


def _case(cfg):
    cfg = dict(cfg)
    thin = cfg.pop("thin", False)
    case = make_case(**cfg)
    if thin:
        g = case["g"] = dict(case["g"])
        g["scales"] = g["scales"].copy()
        g["scales"][:, 2] *= 1e-3
        o = oracle_forward(case, dtype=np.float64)
        V, Pm, campos, bg = antialias_ref.camera_tensors(o, False)
        T = lambda a: torch.tensor(np.asarray(a, np.float64))  # noqa: E731
        aux = antialias_ref.render(o, T(g["means3D"]), T(np.zeros((case["P"], 3))), T(g["opacities"]), V, Pm, campos, bg,
                                   shs=T(g["shs"]), scales=T(g["scales"]), rotations=T(g["rotations"]))[5]
        keep = (antialias_ref.conditioning(aux["cov2"]) <= KAPPA_MAX).numpy()
        g["opacities"] = np.where(keep[:, None], g["opacities"], 0.0).astype(np.float32)
    return case


def _weights(case, F=2, seed=11):
    rng = np.random.default_rng(seed)
    H, W = case["H"], case["W"]
    return dict(color=rng.normal(size=(3, H, W)), depth=rng.normal(size=(1, H, W)), feat=rng.normal(size=(F, H, W)),
                alpha=rng.normal(size=(1, H, W)))


def _features(case, F=2, seed=5):
    return np.random.default_rng(seed).normal(size=(case["P"], F)).astype(np.float32)


def _precomp_extra(case):
    o0 = oracle_forward(case, dtype=np.float64)
    rng = np.random.default_rng(5)
    return dict(colors=rng.uniform(0, 1, size=(case["P"], 3)).astype(np.float32), cov3D=o0.cov3D.astype(np.float32))


def _loss(outs, wts, t):
    color, depth, feat, alpha = outs
    return (color * t(wts["color"])).sum() + (depth * t(wts["depth"])).sum() + (feat * t(wts["feat"])).sum() + (alpha * t(wts["alpha"])).sum()


CAM_KEYS = ("view", "proj", "campos", "bg")


def _gpu(case, feats, wts, mode="sh", extra=None, aa=True):
    import diff_gaussian_rasterization as dgr
    inp = util.gpu_inputs(case)
    c = case["cam"]
    T = lambda a: torch.tensor(np.asarray(a, np.float32), device="cuda", requires_grad=True)  # noqa: E731
    cam = dict(view=T(c["world_view_transform"]), proj=T(c["full_proj_transform"]), campos=T(c["camera_center"]), bg=T(case["bg"]))
    rs = util.gpu_settings(case)._replace(viewmatrix=cam["view"], projmatrix=cam["proj"], campos=cam["campos"], bg=cam["bg"])
    kw = dict(colors_precomp=T(extra["colors"]), cov3D_precomp=T(extra["cov3D"])) if mode == "precomp" else \
        dict(shs=inp["shs"], scales=inp["scales"], rotations=inp["rotations"])
    f = T(feats)
    color, _r, depth, feat, alpha = dgr.GaussianRasterizer(rs)(means3D=inp["means3D"], means2D=inp["means2D"], opacities=inp["opacities"],
                                                               features=f, return_alpha=True, antialiasing=aa, **kw)
    _loss((color, depth, feat, alpha), wts, lambda a: torch.tensor(a, dtype=torch.float32, device="cuda")).backward()
    torch.cuda.synchronize()
    got = dict(mean3D=inp["means3D"].grad, mean2D=inp["means2D"].grad, opacity=inp["opacities"].grad.reshape(-1), features=f.grad)
    if mode == "precomp":
        got.update(colors=kw["colors_precomp"].grad, cov3D=kw["cov3D_precomp"].grad)
    else:
        got.update(sh=inp["shs"].grad, scale=inp["scales"].grad, rot=inp["rotations"].grad)
    got.update({k: cam[k].grad for k in CAM_KEYS})
    imgs = [t.detach().cpu().numpy().astype(np.float64) for t in (color, depth, feat, alpha)]
    return {k: v.detach().cpu().numpy().astype(np.float64) for k, v in got.items()}, imgs


def _ref(case, feats, wts, mode="sh", extra=None):
    g, P = case["g"], case["P"]
    T = lambda a: torch.tensor(np.asarray(a, np.float64), requires_grad=True)  # noqa: E731
    if mode == "precomp":
        o = oracle_forward(case, dtype=np.float64, shs=None, colors_precomp=extra["colors"], scales=None, rotations=None,
                           cov3D_precomp=extra["cov3D"])
        ins = dict(colors_precomp=T(extra["colors"]), cov3D_precomp=T(extra["cov3D"]))
    else:
        o = oracle_forward(case, dtype=np.float64)
        ins = dict(shs=T(g["shs"]), scales=T(g["scales"]), rotations=T(g["rotations"]))
    cam = dict(zip(CAM_KEYS, antialias_ref.camera_tensors(o)))
    m3, m2, op, f = T(g["means3D"]), T(np.zeros((P, 3))), T(g["opacities"]), T(feats)
    c, d, fi, a, _n, aux = antialias_ref.render(o, m3, m2, op, cam["view"], cam["proj"], cam["campos"], cam["bg"], f, **ins)
    _loss((c, d, fi, a), wts, torch.tensor).backward()
    ref = dict(mean3D=m3.grad, mean2D=m2.grad, opacity=op.grad.reshape(-1), features=f.grad)
    if mode == "precomp":
        ref.update(colors=ins["colors_precomp"].grad, cov3D=ins["cov3D_precomp"].grad)
    else:
        ref.update(sh=ins["shs"].grad, scale=ins["scales"].grad, rot=ins["rotations"].grad)
    ref.update({k: cam[k].grad for k in CAM_KEYS})
    # (None: no path from that input to the loss -- campos with colors_precomp)
    return ({k: (v.numpy() if v is not None else None) for k, v in ref.items()}, [t.detach().numpy() for t in (c, d, fi, a)],
            aux["h"].detach().numpy(), o)


@pytest.mark.parametrize("mode", ["sh", "precomp"])
@pytest.mark.parametrize("ci", range(len(CASES)))
def test_images_and_gradients_match_fp64(ci, mode):
    case = _case(CASES[ci])
    feats, wts = _features(case), _weights(case)
    extra = _precomp_extra(case) if mode == "precomp" else None
    got, imgs = _gpu(case, feats, wts, mode, extra)
    ref, rimgs, h, o = _ref(case, feats, wts, mode, extra)
    vis = o.radii > 0
    assert float(h[vis].min()) < 0.9        # (antialiasing matters in every case)
    for name, a, b in zip(("color", "depth", "feat", "alpha"), imgs, rimgs):
        e = image_err(a, b)
        assert e < TOL, (name, e)
    for k, v in got.items():
        if ref[k] is None:
            assert np.all(v == 0.0), k
            continue
        e = rel_err(v, ref[k])
        assert e < TOL, (k, e)


def test_thin_case_differs_from_the_plain_render():
    """antialiasing is no no-op: on the thin case the images move by far more than the bars"""
    case = _case(CASES[3])
    feats, wts = _features(case), _weights(case)
    _g1, on = _gpu(case, feats, wts, aa=True)
    _g0, off = _gpu(case, feats, wts, aa=False)
    for a, b in zip(on, off):
        assert rel_err(a, b) > 0.05
    assert float(on[3].mean()) < float(off[3].mean())       # less coverage


def _call(case, dpix, **kw):
    import diff_gaussian_rasterization as dgr
    inp = util.gpu_inputs(case)
    out = dgr.GaussianRasterizer(util.gpu_settings(case))(
        means3D=inp["means3D"], means2D=inp["means2D"], opacities=inp["opacities"], shs=inp["shs"], scales=inp["scales"],
        rotations=inp["rotations"], **kw)
    ((out[0] * torch.tensor(dpix, dtype=torch.float32, device="cuda")).sum() + out[2].sum()).backward()
    torch.cuda.synchronize()
    return [t.detach().clone() for t in out[:3]] + [inp[k].grad.clone() for k in ("means3D", "means2D", "opacities", "shs", "scales",
                                                                                    "rotations")]


@pytest.mark.parametrize("spec", [True, False])
def test_off_is_the_call_without_the_keyword(spec, monkeypatch):
    """bit-reproducible mode: antialiasing=False is the call without the keyword, bit for bit (images, radii, gradients), before and after
    antialiased calls; two antialiased calls are bit-equal"""
    import diff_gaussian_rasterization as dgr
    monkeypatch.setattr(dgr, "PER_CALL_SPECULATION", spec)
    case = make_case(**CASES[1])
    dpix = np.random.default_rng(4).normal(size=(3, case["H"], case["W"]))
    _flags(256)
    try:
        a = _call(case, dpix)
        b = _call(case, dpix, antialiasing=False)
        c1 = _call(case, dpix, antialiasing=True)
        c2 = _call(case, dpix, antialiasing=True)
        d = _call(case, dpix)
    finally:
        _flags(0)
    for x, y, z in zip(a, b, d):
        assert torch.equal(x, y) and torch.equal(x, z)
    for x, y in zip(c1, c2):
        assert torch.equal(x, y)
    assert not torch.equal(a[0], c1[0])


def _views(V=4, P=2000, W=128, H=96, seed=7):
    from csplat import synthetic as syn
    base = make_case(P=P, W=W, H=H, seed=seed)
    return [dict(base, cam=syn.make_camera(-40.0 + 25.0 * i, W, H)) for i in range(V)]


def test_batched_views_match_per_view_calls():
    """rasterize_views over 4 views with antialiasing (one K1 / K8 launch for all views) against 4 GaussianRasterizer calls: images
    bit-equal, per-view gradients and the shared parameters' summed gradients within 1e-5 (bit-reproducible mode)"""
    import diff_gaussian_rasterization as dgr
    cases = _views(4)
    P, H, W = cases[0]["P"], cases[0]["H"], cases[0]["W"]
    rng = np.random.default_rng(3)
    wc = [torch.tensor(rng.normal(size=(3, H, W)).astype(np.float32), device="cuda") for _ in range(4)]
    names = ("means3D", "opacities", "shs", "scales", "rotations")

    def per_view():
        inp = util.gpu_inputs(cases[0])
        m2 = [torch.zeros(P, 3, device="cuda", requires_grad=True) for _ in range(4)]
        imgs = []
        for i, c in enumerate(cases):
            col, _r, dep = dgr.GaussianRasterizer(util.gpu_settings(c))(
                means3D=inp["means3D"], means2D=m2[i], opacities=inp["opacities"], shs=inp["shs"], scales=inp["scales"],
                rotations=inp["rotations"], antialiasing=True)
            (col * wc[i]).sum().backward()
            imgs += [col.detach(), dep.detach()]
        torch.cuda.synchronize()
        return imgs, [inp[k].grad for k in names] + [m.grad for m in m2]

    def batched():
        inp = util.gpu_inputs(cases[0])
        m2 = [torch.zeros(P, 3, device="cuda", requires_grad=True) for _ in range(4)]
        kws = [dict(means3D=inp["means3D"], means2D=m2[i], opacities=inp["opacities"], shs=inp["shs"], scales=inp["scales"],
                    rotations=inp["rotations"], antialiasing=True) for i in range(4)]
        outs = dgr.rasterize_views([util.gpu_settings(c) for c in cases], kws)
        sum((o[0] * wc[i]).sum() for i, o in enumerate(outs)).backward()
        torch.cuda.synchronize()
        return [x.detach() for o in outs for x in (o[0], o[2])], [inp[k].grad for k in names] + [m.grad for m in m2]

    _flags(256)
    try:
        a, b = per_view(), batched()
    finally:
        _flags(0)
    for x, y in zip(a[0], b[0]):
        assert torch.equal(x, y)
    for x, y in zip(a[1], b[1]):
        assert rel_err(y.cpu().numpy(), x.cpu().numpy()) < 1e-5


NAMES = ("means3D", "opacities", "shs", "scales", "rotations")


def _step_fn(V=3, P=2901, W=144, H=112):
    """one batched antialiased step (rasterize_views, loss, backward) on fixed buffers: what ReplayedSteps records"""
    import diff_gaussian_rasterization as dgr
    base = make_case(P=P, W=W, H=H, seed=4, theta=-30.0, scale_mul=2.0)
    inp = util.gpu_inputs(base)
    cases = [make_case(P=P, W=W, H=H, seed=4, theta=-30.0 + 30.0 * i, scale_mul=2.0) for i in range(V)]
    settings = [util.gpu_settings(c) for c in cases]
    tgt = torch.rand(V, 3, H, W, device="cuda", generator=torch.Generator(device="cuda").manual_seed(3))
    zeros = torch.zeros(V, P, 3, device="cuda")

    def run():
        for k in NAMES:
            inp[k].grad = None
        m2d = [zeros[i].detach().requires_grad_() for i in range(V)]
        kws = [dict(means3D=inp["means3D"], means2D=m2d[i], opacities=inp["opacities"], shs=inp["shs"], scales=inp["scales"],
                    rotations=inp["rotations"], antialiasing=True) for i in range(V)]
        colors, _outs = dgr.rasterize_views(settings, kws, stacked=True)
        ((colors - tgt) ** 2).mean().backward()
        return colors.detach(), [inp[k].grad for k in NAMES] + [m.grad for m in m2d]
    return run


def test_faith_replay_and_deferred_k8_equal_the_eager_step():
    """bit-reproducible mode: the antialiased step launched on faith (forward_mode), recorded and replayed by csplat.graphs.ReplayedSteps,
    and with its K8 cut into deferred_k8() slices, equals the eager step bit for bit (images and every gradient)"""
    import diff_gaussian_rasterization as dgr
    from csplat import graphs
    _flags(256)
    try:
        run = _step_fn()
        col0, g0 = run()
        torch.cuda.synchronize()
        eager = [col0.clone()] + [t.clone() for t in g0]
        # on faith
        _out, counts = graphs.counts_of_eager(run)
        faith = {"caps": graphs.caps_from_counts(counts), "valid": torch.zeros(1, dtype=torch.int32, device="cuda")}
        with dgr.forward_mode(faith=faith):
            col1, g1 = run()
        torch.cuda.synchronize()
        assert dgr.forward_mode_is_default() and int(faith["valid"].item()) == 1
        for a, b in zip(eager, [col1] + g1):
            assert torch.equal(a, b)
        # recorded and replayed
        rs = graphs.ReplayedSteps(run, torch.device("cuda", torch.cuda.current_device()), G=2)
        rs.record()
        assert dgr.forward_mode_is_default()
        for _k in range(3):
            col, gr = rs.outs[rs.k % 2]
            with torch.no_grad():
                col.fill_(float("nan"))
                for t in gr:
                    t.fill_(float("nan"))
            rs.step()
        rs.check()
        col2, g2 = rs.outs[rs.last()]
        for a, b in zip(eager, [col2] + g2):
            assert torch.equal(a, b)
        # deferred K8 in three slices
        run3 = _step_fn()
        with dgr.deferred_k8() as h:
            col3, g3 = run3()
        for t in g3:
            t.fill_(float("nan"))
        for s in range(3):
            h.launch(s, 3)
        torch.cuda.synchronize()
        for a, b in zip(eager, [col3] + g3):
            assert torch.equal(a, b)
    finally:
        _flags(0)


def test_render_with_the_pipeline_flag_matches_a_direct_call():
    """gaussian_renderer.render with pipe.antialiasing = True is the antialiased GaussianRasterizer call on what render() handed over;
    without the attribute render() is the plain call"""
    import diff_gaussian_rasterization as dgr
    from csplat import synthetic as syn
    from gaussian_renderer import render
    from csplat.gaussians import MeshGaussians
    from meshnet.meshnet_network import ResidualMeshSimulator
    sc = syn.scene_1(P=3000, W=160, H=120, n_cams=1, grid=14, n_times=5, seed=31)
    T = lambda a, dt=torch.float32: torch.tensor(a, device="cuda", dtype=dt)  # noqa: E731
    pc = MeshGaussians(3).from_arrays(T(sc["mesh_pos"][0]), T(sc["faces"].T.copy(), torch.long), T(sc["edge_index"], torch.long),
                                      T(sc["face_ids"], torch.long), T(sc["bary"]), T(sc["log_scales"]), T(sc["quats"]),
                                      T(sc["opacity_logits"]), T(sc["sh"]))
    pc.active_sh_degree = 3
    sim = ResidualMeshSimulator(T(sc["mesh_pos"]), device="cuda")
    c = sc["cameras"][0]
    t = lambda a: torch.tensor(a)  # noqa: E731
    cam = SimpleNamespace(image_height=c["image_height"], image_width=c["image_width"], FoVx=c["FoVx"], FoVy=c["FoVy"],
                          world_view_transform=t(c["world_view_transform"]), full_proj_transform=t(c["full_proj_transform"]),
                          camera_center=t(c["camera_center"]), time=0.5)
    bg = torch.ones(3, device="cuda")
    dpix = torch.tensor(np.random.default_rng(2).normal(size=(3, 120, 160)).astype(np.float32), device="cuda")
    outs = {}
    for aa in (False, True):
        pipe = SimpleNamespace(compute_cov3D_python=False, convert_SHs_python=False, debug=False)
        if aa:
            pipe.antialiasing = True
        res = render(cam, pc, sim, pipe, bg)
        res.means3D_deform.retain_grad()
        (res.render * dpix).sum().backward()
        m3 = res.means3D_deform.detach().clone().requires_grad_(True)
        op = pc.get_opacity.detach().clone().requires_grad_(True)
        rs = dgr.GaussianRasterizationSettings(image_height=120, image_width=160, tanfovx=math.tan(c["FoVx"] * 0.5),
                                               tanfovy=math.tan(c["FoVy"] * 0.5), bg=bg, scale_modifier=1.0,
                                               viewmatrix=T(c["world_view_transform"]), projmatrix=T(c["full_proj_transform"]),
                                               sh_degree=3, campos=T(c["camera_center"]), prefiltered=False, debug=False)
        col, _r, _d = dgr.GaussianRasterizer(rs)(means3D=m3, means2D=torch.zeros_like(m3), opacities=op,
                                                 shs=pc.get_features.detach(), scales=pc.get_scaling.detach(),
                                                 rotations=res.rotations.detach(), antialiasing=aa)
        (col * dpix).sum().backward()
        torch.cuda.synchronize()
        assert torch.equal(col.detach(), res.render.detach())
        assert rel_err(res.means3D_deform.grad.cpu().numpy(), m3.grad.cpu().numpy()) < 1e-5
        outs[aa] = col.detach()
    assert not torch.equal(outs[False], outs[True])


def test_captured_train_step_equals_the_eager_step():
    """train_step(captured=True) with pipe.antialiasing: a few CapturedStep iterations (recorded once, replayed) equal the eager
    train_step iterations bit for bit in the bit-reproducible mode, and the flag is part of the graph key"""
    import test_train_gpu as ttg
    from csplat import train as tr
    pipe = SimpleNamespace(compute_cov3D_python=False, convert_SHs_python=False, debug=False, antialiasing=True)

    def run(mode):
        with ttg._reproducible_k7(True):
            pc, sim, mopt, cams, bg = ttg._captured_fixture(seed=3)
            log = []
            for it in range(1, 5):
                ps, loss, stats = tr.train_step(it, cams, pc, sim, mopt, pipe=pipe, background=bg, captured=(mode == "captured"))
                log.append((float(ps), float(loss), stats["radii"].clone(), stats["viewspace_grad"].clone(), stats["visibility_filter"].clone()))
            torch.cuda.synchronize()
            params = [p.detach().clone() for p in list(pc.parameters()) + list(sim.parameters())]
            moments = ttg._adam_state(pc.optimizer, pc.parameters()) + ttg._adam_state(mopt, sim.parameters())
            steps = [float(pc.optimizer.state[p]["step"]) for p in pc.parameters() if pc.optimizer.state.get(p)] + \
                [float(mopt.state[p]["step"]) for p in sim.parameters()]
        return {"log": log, "params": params, "moments": moments, "steps": steps, "cs": getattr(pc, "_captured_step", None)}

    eager = run("eager")
    cap = run("captured")
    cs = cap["cs"]
    assert cs is not None and cs.stats["recorded"] == 1 and cs.stats["replayed"] == 3 and cs.stats["missed"] == 0, cs.stats
    assert all(k[-1] is True for k in cs.graphs)
    ttg._assert_runs_bit_equal(eager, cap)


def test_flagship_shape_finite_and_reproducible():
    """P = 100 000, 4 views of 800 x 800, SH 3: the antialiased forward + backward is finite, reproducible bit for bit in the
    bit-reproducible mode, and renders less coverage than the plain call"""
    import diff_gaussian_rasterization as dgr
    from csplat import synthetic as syn
    P, S, NV = 100_000, 800, 4
    sc = syn.scene_1(P=P, W=S, H=S, n_cams=NV, seed=0)
    g = syn.gaussians_at(sc)
    T = lambda x, rg=False: torch.tensor(np.asarray(x, np.float32), device="cuda", requires_grad=rg)  # noqa: E731
    settings = [dgr.GaussianRasterizationSettings(
        image_height=S, image_width=S, tanfovx=cm["tanfovx"], tanfovy=cm["tanfovy"], bg=T(sc["bg"]), scale_modifier=1.0,
        viewmatrix=T(cm["world_view_transform"]), projmatrix=T(cm["full_proj_transform"]), sh_degree=3, campos=T(cm["camera_center"]),
        prefiltered=False, debug=False) for cm in sc["cameras"][:NV]]
    w = torch.rand(NV, 3, S, S, device="cuda", generator=torch.Generator(device="cuda").manual_seed(1)) - 0.5

    def run(aa):
        inp = {k: T(g[k], True) for k in ("means3D", "opacities", "shs", "scales", "rotations")}
        kws = [dict(means3D=inp["means3D"], means2D=torch.zeros(P, 3, device="cuda"), opacities=inp["opacities"], shs=inp["shs"],
                    scales=inp["scales"], rotations=inp["rotations"], antialiasing=aa) for _ in range(NV)]
        colors, outs = dgr.rasterize_views(settings, kws, stacked=True)
        (colors * w).sum().backward()
        torch.cuda.synchronize()
        return [colors.detach()] + [inp[k].grad for k in inp]

    _flags(256)
    try:
        a, b = run(True), run(True)
    finally:
        _flags(0)
    for x, y in zip(a, b):
        assert torch.isfinite(x).all() and torch.equal(x, y)
    assert float(a[2].abs().max()) > 0
    plain = run(False)
    assert rel_err(a[0].cpu().numpy(), plain[0].cpu().numpy()) > 1e-3
