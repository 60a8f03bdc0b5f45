"""Gradients through the rendered DEPTH image (the depth fork of the rasterizer the reference pins): D = sum_i T_i alpha_i z_i per
pixel, differentiated w.r.t. every Gaussian input (csplat_backward_depth / csplat_view.dL_ddepth).  Truth: autograd of the fp64 torch
oracle (oracle/raster_torch.render builds its depth image from differentiable torch ops).  Bar: 1e-4 relative, the repo's gradient bar."""
from types import SimpleNamespace

import numpy as np
import pytest

import util
from util import make_case, oracle_forward, rel_err

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
from oracle import raster_torch as rt  # noqa: E402

TOL = 1e-4

CASES = [
    dict(P=2000, W=128, H=96, seed=7, grid=20, scale_mul=1.0),
    dict(P=3000, W=200, H=136, seed=8, grid=16, scale_mul=2.5),     # ragged: W,H not multiples of 16
    dict(P=800, W=64, H=64, seed=9, grid=10, scale_mul=4.0, radius=1.2),  # close camera: frustum clamp + culling
]


def _images(case, seed=11):
    rng = np.random.default_rng(seed)
    return (rng.normal(size=(3, case["H"], case["W"])).astype(np.float32),
            rng.normal(size=(1, case["H"], case["W"])).astype(np.float32))


def _flags(f):
    from csplat import native
    native.lib.csplat_debug_flags(f)


def _gpu(case, dpix, ddepth, mode="sh_scale_rot", scale_mod=1.0, extra=None):
    """one GaussianRasterizer call; loss = sum dpix * color + sum ddepth * depth (either may be None).  -> {name: grad (numpy)}"""
    import diff_gaussian_rasterization as dgr
    inp = util.gpu_inputs(case)
    rs = util.gpu_settings(case, scale_mod=scale_mod)
    T = lambda a: torch.tensor(np.asarray(a, np.float32), device="cuda", requires_grad=True)  # noqa: E731
    if mode == "precomp":
        kw = dict(colors_precomp=T(extra["colors"]), cov3D_precomp=T(extra["cov3D"]))
    else:
        kw = dict(shs=inp["shs"], scales=inp["scales"], rotations=inp["rotations"])
    color, _radii, depth = dgr.GaussianRasterizer(rs)(means3D=inp["means3D"], means2D=inp["means2D"], opacities=inp["opacities"], **kw)
    loss = 0.0
    if dpix is not None:
        loss = loss + (color * torch.tensor(dpix, device="cuda")).sum()
    if ddepth is not None:
        loss = loss + (depth * torch.tensor(ddepth, device="cuda")).sum()
    loss.backward()
    torch.cuda.synchronize()
    got = dict(mean3D=inp["means3D"].grad, mean2D=inp["means2D"].grad, opacity=inp["opacities"].grad.reshape(-1))
    for k, t in kw.items():
        got[k] = t.grad
    return {k: (v.cpu().numpy() if v is not None else None) for k, v in got.items()}


def _oracle(case, dpix, ddepth, mode="sh_scale_rot", scale_mod=1.0, extra=None):
    """the same loss through rt.render on the fp64 oracle, autograd -> {name: grad} (dL/dscales as the rasterizer reports it: w.r.t.
    modifier * scale, the upstream convention)"""
    g, P = case["g"], case["P"]
    T = lambda a: torch.tensor(np.asarray(a, np.float64), requires_grad=True)  # noqa: E731
    m3, m2, op = T(g["means3D"]), T(np.zeros((P, 3))), T(g["opacities"])
    if mode == "precomp":
        o = oracle_forward(case, dtype=np.float64, shs=None, colors_precomp=extra["colors"], scales=None, rotations=None,
                           cov3D_precomp=extra["cov3D"])
        ins = dict(colors_precomp=T(extra["colors"]), cov3D_precomp=T(extra["cov3D"]))
    else:
        o = oracle_forward(case, dtype=np.float64, scale_mod=scale_mod)
        ins = dict(shs=T(g["shs"]), scales=T(g["scales"]), rotations=T(g["rotations"]))
    color, dimg, _ = rt.render(o, m3, m2, op, **ins)
    loss = 0.0
    if dpix is not None:
        loss = loss + (color * torch.tensor(dpix, dtype=torch.float64)).sum()
    if ddepth is not None:
        loss = loss + (dimg * torch.tensor(ddepth, dtype=torch.float64)).sum()
    loss.backward()
    out = dict(mean3D=m3.grad, mean2D=m2.grad, opacity=op.grad.reshape(-1))
    for k, t in ins.items():
        out[k] = t.grad
    out = {k: (v.numpy() if v is not None else np.zeros(tuple(ins.get(k, m3).shape))) for k, v in out.items()}
    if "scales" in out:
        out["scales"] = out["scales"] / scale_mod
    return out


def _precomp_extra(case):
    o0 = oracle_forward(case, dtype=np.float64)
    rng = np.random.default_rng(5)
    return dict(colors=rng.uniform(0, 1, size=(case["P"], 3)).astype(np.float32), cov3D=o0.cov3D.astype(np.float32))


@pytest.mark.parametrize("mode", ["sh_scale_rot", "precomp", "scale_mod"])
@pytest.mark.parametrize("cfg", CASES)
def test_depth_and_colour_loss_matches_fp64_autograd(cfg, mode):
    case = make_case(**cfg)
    dpix, ddepth = _images(case)
    mod = 1.6 if mode == "scale_mod" else 1.0
    extra = _precomp_extra(case) if mode == "precomp" else None
    m = "precomp" if mode == "precomp" else "sh_scale_rot"
    got = _gpu(case, dpix, ddepth, m, mod, extra)
    ref = _oracle(case, dpix, ddepth, m, mod, extra)
    for k in ref:
        e = rel_err(got[k], ref[k])
        assert e < TOL, (k, e)


@pytest.mark.parametrize("cfg", CASES[:2])
def test_depth_only_loss(cfg):
    """no colour term: grad_color never arrives (treated as zero); the colour / SH gradients are exactly zero"""
    case = make_case(**cfg)
    _dpix, ddepth = _images(case, seed=12)
    got = _gpu(case, None, ddepth)
    ref = _oracle(case, None, ddepth)
    for k in ("mean3D", "mean2D", "opacity", "scales", "rotations"):
        e = rel_err(got[k], ref[k])
        assert e < TOL, (k, e)
        assert np.abs(got[k]).max() > 0, k
    assert not np.any(got["shs"])


def _colour_vs_zero_depth(case, dpix):
    import diff_gaussian_rasterization as dgr
    res = []
    for with_depth in (False, True):
        inp = util.gpu_inputs(case)
        color, _r, depth = dgr.GaussianRasterizer(util.gpu_settings(case))(
            means3D=inp["means3D"], means2D=inp["means2D"], opacities=inp["opacities"], shs=inp["shs"], scales=inp["scales"],
            rotations=inp["rotations"])
        loss = (color * torch.tensor(dpix, device="cuda")).sum()
        if with_depth:
            loss = loss + 0.0 * depth.sum()
        loss.backward()
        torch.cuda.synchronize()
        res.append([inp[k].grad.clone() for k in ("means3D", "means2D", "opacities", "shs", "scales", "rotations")])
    return res


def test_zero_depth_gradient_changes_nothing():
    """a depth gradient of zeros takes the depth path and adds nothing: bit for bit in the bit-reproducible mode.  In the default mode the
    depth K7 is another launch whose float atomics meet in another order: the opacity gradient (a cancelling sum over every pixel a
    Gaussian blends) moved by 2.9e-6 of its largest value, the others by <= 8e-7 (two colour-only runs: <= 1.5e-7) -- held at 1e-5, the
    bar between the default and the bit-reproducible mode."""
    case = make_case(**CASES[0])
    dpix, _ = _images(case)
    _flags(256)
    try:
        a, b = _colour_vs_zero_depth(case, dpix)
    finally:
        _flags(0)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    c, d = _colour_vs_zero_depth(case, dpix)
    for x, y, z in zip(a, c, d):
        for u, v in ((y, x), (z, x), (z, y)):
            e = rel_err(u.cpu().numpy(), v.cpu().numpy())
            assert e < 1e-5, e


def test_depth_gradient_reproducible():
    case = make_case(**CASES[1])
    dpix, ddepth = _images(case)
    _flags(256)
    try:
        r1 = _gpu(case, dpix, ddepth)
        r2 = _gpu(case, dpix, ddepth)
    finally:
        _flags(0)
    r3 = _gpu(case, dpix, ddepth)
    for k in r1:
        assert np.array_equal(r1[k], r2[k]), k
        assert rel_err(r3[k], r1[k]) < 1e-5, k


def _views(V=4, P=2000):
    cases = [make_case(P=P, W=128, H=96, seed=7, grid=20, theta=-30.0 + 20.0 * i) for i in range(V)]
    rng = np.random.default_rng(21)
    dpix = [rng.normal(size=(3, 96, 128)).astype(np.float32) for _ in range(V)]
    ddepth = [rng.normal(size=(1, 96, 128)).astype(np.float32) if i in (0, 2) else None for i in range(V)]
    return cases, dpix, ddepth


NAMES = ("means3D", "opacities", "shs", "scales", "rotations")


@pytest.mark.parametrize("stacked", [False, True])
def test_batched_views_equal_single_view_calls(stacked):
    import diff_gaussian_rasterization as dgr
    cases, dpix, ddepth = _views()
    V = len(cases)
    # per-view calls, the parameter gradients summed by autograd
    inp = util.gpu_inputs(cases[0])
    m2d = [torch.zeros(cases[0]["P"], 3, device="cuda", requires_grad=True) for _ in range(V)]
    loss = 0.0
    for i, c in enumerate(cases):
        color, _r, depth = dgr.GaussianRasterizer(util.gpu_settings(c))(
            means3D=inp["means3D"], means2D=m2d[i], opacities=inp["opacities"], shs=inp["shs"], scales=inp["scales"],
            rotations=inp["rotations"])
        loss = loss + (color * torch.tensor(dpix[i], device="cuda")).sum()
        if ddepth[i] is not None:
            loss = loss + (depth * torch.tensor(ddepth[i], device="cuda")).sum()
    loss.backward()
    single = [inp[k].grad.clone() for k in NAMES] + [m.grad.clone() for m in m2d]
    # one batched call
    inp = util.gpu_inputs(cases[0])
    m2d = [torch.zeros(cases[0]["P"], 3, device="cuda", requires_grad=True) for _ in range(V)]
    kws = [dict(means3D=inp["means3D"], means2D=m2d[i], opacities=inp["opacities"], shs=inp["shs"], scales=inp["scales"],
                rotations=inp["rotations"]) for i in range(V)]
    settings = [util.gpu_settings(c) for c in cases]
    if stacked:
        colors, outs = dgr.rasterize_views(settings, kws, stacked=True)
        loss = (colors * torch.tensor(np.stack(dpix), device="cuda")).sum()
    else:
        outs = dgr.rasterize_views(settings, kws)
        loss = sum((outs[i][0] * torch.tensor(dpix[i], device="cuda")).sum() for i in range(V))
    for i in range(V):
        if ddepth[i] is not None:
            loss = loss + (outs[i][2] * torch.tensor(ddepth[i], device="cuda")).sum()
    loss.backward()
    torch.cuda.synchronize()
    batched = [inp[k].grad for k in NAMES] + [m.grad for m in m2d]
    for a, b in zip(single, batched):
        assert rel_err(b.cpu().numpy(), a.cpu().numpy()) < 1e-5


def test_depth_only_view_runs_and_unused_view_costs_nothing():
    """a view whose colour is unused but whose depth is in the loss still runs (its gradient arrives); a view with neither gets none"""
    import diff_gaussian_rasterization as dgr
    cases, _dpix, ddepth = _views(V=3)
    inp = util.gpu_inputs(cases[0])
    m2d = [torch.zeros(cases[0]["P"], 3, device="cuda", requires_grad=True) for _ in range(3)]
    kws = [dict(means3D=inp["means3D"], means2D=m2d[i], opacities=inp["opacities"], shs=inp["shs"], scales=inp["scales"],
                rotations=inp["rotations"]) for i in range(3)]
    outs = dgr.rasterize_views([util.gpu_settings(c) for c in cases], kws)
    (outs[0][2] * torch.tensor(ddepth[0], device="cuda")).sum().backward()
    torch.cuda.synchronize()
    assert float(m2d[0].grad.abs().max()) > 0 and float(inp["means3D"].grad.abs().max()) > 0
    assert m2d[1].grad is None and m2d[2].grad is None


def test_deferred_k8_slices_equal_whole_backward_with_depth():
    from csplat import native  # noqa: F401
    import diff_gaussian_rasterization as dgr
    V, P, G = 3, 2901, 3
    _flags(256)
    try:
        def run(parts):
            base = make_case(P=P, W=144, H=112, seed=4, theta=-30.0, scale_mul=2.0)
            inp = util.gpu_inputs(base)
            cases = [make_case(P=P, W=144, H=112, seed=4, theta=-30.0 + 30.0 * i, scale_mul=2.0) for i in range(V)]
            m2d = [torch.zeros(P, 3, device="cuda", requires_grad=True) for _ in range(V)]
            kws = [dict(means3D=inp["means3D"], means2D=m2d[i], opacities=inp["opacities"], shs=inp["shs"], scales=inp["scales"],
                        rotations=inp["rotations"]) for i in range(V)]
            colors, outs = dgr.rasterize_views([util.gpu_settings(c) for c in cases], kws, stacked=True)
            gen = torch.Generator(device="cuda").manual_seed(3)
            loss = ((colors - torch.rand(V, 3, 112, 144, device="cuda", generator=gen)) ** 2).mean()
            loss = loss + 0.05 * sum((outs[i][2] * torch.rand(1, 112, 144, device="cuda", generator=gen)).sum() for i in (0, 2))
            if parts:
                with dgr.deferred_k8() as h:
                    loss.backward()
                for t in [inp[k].grad for k in NAMES] + [m.grad for m in m2d]:
                    t.fill_(float("nan"))
                for g_ in range(G):
                    h.launch(g_, G)
            else:
                loss.backward()
            torch.cuda.synchronize()
            return [inp[k].grad.clone() for k in NAMES] + [m.grad.clone() for m in m2d]
        whole = run(False)
        cut = run(True)
    finally:
        _flags(0)
    for a, b in zip(whole, cut):
        assert torch.equal(a, b)


def test_depth_gradient_on_faith_raises():
    """a forward launched on faith (captured / replayed steps) takes no depth loss: a clear error, never a silently dropped term"""
    import diff_gaussian_rasterization as dgr
    from csplat import graphs
    cases, _dpix, ddepth = _views(V=2)
    inp = util.gpu_inputs(cases[0])
    m2d = [torch.zeros(cases[0]["P"], 3, device="cuda", requires_grad=True) for _ in range(2)]
    kws = [dict(means3D=inp["means3D"], means2D=m2d[i], opacities=inp["opacities"], shs=inp["shs"], scales=inp["scales"],
                rotations=inp["rotations"]) for i in range(2)]
    settings = [util.gpu_settings(c) for c in cases]
    _out, counts = graphs.counts_of_eager(lambda: dgr.rasterize_views(settings, kws, stacked=True))
    faith = {"caps": graphs.caps_from_counts(counts), "valid": torch.zeros(1, dtype=torch.int32, device="cuda")}
    with dgr.forward_mode(faith=faith):
        _colors, outs = dgr.rasterize_views(settings, kws, stacked=True)
    torch.cuda.synchronize()
    assert dgr.forward_mode_is_default() and int(faith["valid"].item()) == 1
    with pytest.raises(RuntimeError, match="depth gradient"):
        (outs[0][2] * torch.tensor(ddepth[0], device="cuda")).sum().backward()


def test_depth_loss_through_the_renderer():
    """gaussian_renderer.render: a depth loss reaches the Gaussian parameters and the simulator, and the rasterizer-level gradients
    it produces are those of a direct GaussianRasterizer call on the same inputs"""
    import math
    import diff_gaussian_rasterization as dgr
    from csplat import synthetic as syn
    from gaussian_renderer import render
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
    with torch.no_grad():
        torch.manual_seed(0)
        sim.output.weight.normal_(0, 1e-3)
    c = sc["cameras"][0]
    t = lambda a: torch.tensor(a)  # noqa: E731
    cam = SimpleNamespace(image_height=c["image_height"], image_width=c["image_width"], FoVx=c["FoVx"], FoVy=c["FoVy"],
                          world_view_transform=t(c["world_view_transform"]), full_proj_transform=t(c["full_proj_transform"]),
                          camera_center=t(c["camera_center"]), time=0.5)
    pipe = SimpleNamespace(compute_cov3D_python=False, convert_SHs_python=False, debug=False)
    bg = torch.ones(3, device="cuda")
    res = render(cam, pc, sim, pipe, bg)
    res.means3D_deform.retain_grad()
    ddepth = torch.tensor(np.random.default_rng(2).normal(size=(1, 120, 160)).astype(np.float32), device="cuda")
    (res.depth * ddepth).sum().backward()
    torch.cuda.synchronize()
    for p in (pc.face_bary, pc._opacity, pc._scaling, pc._rotation):
        assert p.grad is not None and torch.isfinite(p.grad).all() and float(p.grad.abs().max()) > 0
    assert sim.output.weight.grad is not None and float(sim.output.weight.grad.abs().max()) > 0
    assert float(res.viewspace_points.grad[:, :2].abs().max()) > 0
    # the same rasterizer call on detached copies of what render() handed it
    m3 = res.means3D_deform.detach().clone().requires_grad_(True)
    m2 = torch.zeros_like(m3, requires_grad=True)
    rs = dgr.GaussianRasterizationSettings(image_height=120, image_width=160, tanfovx=math.tan(c["FoVx"] * 0.5),
                                           tanfovy=math.tan(c["FoVy"] * 0.5), bg=bg, scale_modifier=1.0,
                                           viewmatrix=T(c["world_view_transform"]), projmatrix=T(c["full_proj_transform"]),
                                           sh_degree=3, campos=T(c["camera_center"]), prefiltered=False, debug=False)
    _col, _r, depth = dgr.GaussianRasterizer(rs)(means3D=m3, means2D=m2, opacities=pc.get_opacity.detach(),
                                                 shs=pc.get_features.detach(), scales=pc.get_scaling.detach(),
                                                 rotations=res.rotations.detach())
    (depth * ddepth).sum().backward()
    torch.cuda.synchronize()
    assert rel_err(res.means3D_deform.grad.cpu().numpy(), m3.grad.cpu().numpy()) < 1e-5
    assert rel_err(res.viewspace_points.grad.cpu().numpy(), m2.grad.cpu().numpy()) < 1e-5


def test_per_call_path_matches_fp64_autograd():
    """the single-view Function without the batched entry (PER_CALL_SPECULATION off: csplat_backward_depth)"""
    import diff_gaussian_rasterization as dgr
    case = make_case(**CASES[1])
    dpix, ddepth = _images(case)
    old = dgr.PER_CALL_SPECULATION
    dgr.PER_CALL_SPECULATION = False
    try:
        got = _gpu(case, dpix, ddepth)
        only = _gpu(case, None, ddepth)
    finally:
        dgr.PER_CALL_SPECULATION = old
    ref = _oracle(case, dpix, ddepth)
    for k in ref:
        assert rel_err(got[k], ref[k]) < TOL, k
    ref = _oracle(case, None, ddepth)
    for k in ("mean3D", "mean2D", "opacity", "scales", "rotations"):
        assert rel_err(only[k], ref[k]) < TOL, k
