"""Gradients of the CAMERA tensors of the rasterizer settings: viewmatrix, projmatrix, campos and bg (include/csplat.h,
csplat_view.dL_dview .. dL_dbg).  Truth: autograd of tests/camera_ref.py, the fp64 restatement of the forward with the camera tensors as
inputs.  Bar: 1e-4 relative (util.rel_err), the repo's gradient bar."""
import math
from types import SimpleNamespace

import numpy as np
import pytest

import util
import camera_ref
from util import make_case, oracle_forward, rel_err

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

TOL = 1e-4
CASES = [
    dict(P=2000, W=128, H=96, seed=7, grid=20, scale_mul=1.0),
    dict(P=3000, W=200, H=136, seed=8, grid=16, scale_mul=2.5),     # ragged: W,H not multiples of 16
    dict(P=800, W=64, H=64, seed=9, grid=10, scale_mul=4.0, radius=1.2),  # close camera: frustum clamp + culling
]
CAMS = ("view", "proj", "campos", "bg")


def _flags(f):
    from csplat import native
    native.lib.csplat_debug_flags(f)


def _images(case, seed=11):
    rng = np.random.default_rng(seed)
    return (rng.normal(size=(3, case["H"], case["W"])).astype(np.float32),
            rng.normal(size=(1, case["H"], case["W"])).astype(np.float32))


def _precomp_extra(case):
    o0 = oracle_forward(case, dtype=np.float64)
    rng = np.random.default_rng(5)
    return dict(colors=rng.uniform(0, 1, size=(case["P"], 3)).astype(np.float32), cov3D=o0.cov3D.astype(np.float32))


def _cam_leaves(case, dev="cuda"):
    """camera leaves; the viewmatrix is handed over as a .transpose(0, 1) view of its leaf, as the reference builds it"""
    cam = case["cam"]
    t = lambda a: torch.tensor(np.asarray(a, np.float32), device=dev, requires_grad=True)  # noqa: E731
    return dict(view_t=t(np.asarray(cam["world_view_transform"]).T), proj=t(cam["full_proj_transform"]), campos=t(cam["camera_center"]),
                bg=t(case["bg"]))


def _settings(case, leaves, scale_mod=1.0):
    from diff_gaussian_rasterization import GaussianRasterizationSettings
    cam = case["cam"]
    return GaussianRasterizationSettings(
        image_height=case["H"], image_width=case["W"], tanfovx=cam["tanfovx"], tanfovy=cam["tanfovy"], bg=leaves["bg"],
        scale_modifier=scale_mod, viewmatrix=leaves["view_t"].transpose(0, 1), projmatrix=leaves["proj"], sh_degree=case["sh_degree"],
        campos=leaves["campos"], prefiltered=False, debug=False)


def _cam_grads(leaves):
    return dict(view=leaves["view_t"].grad.T.contiguous(), proj=leaves["proj"].grad, campos=leaves["campos"].grad, bg=leaves["bg"].grad)


def _gpu(case, dpix, ddepth, mode="sh", scale_mod=1.0, extra=None):
    import diff_gaussian_rasterization as dgr
    inp = util.gpu_inputs(case)
    leaves = _cam_leaves(case)
    T = lambda a: torch.tensor(np.asarray(a, np.float32), device="cuda", requires_grad=True)  # noqa: E731
    kw = dict(colors_precomp=T(extra["colors"]), cov3D_precomp=T(extra["cov3D"])) if mode == "precomp" else \
        dict(shs=inp["shs"], scales=inp["scales"], rotations=inp["rotations"])
    color, _r, depth = dgr.GaussianRasterizer(_settings(case, leaves, scale_mod))(
        means3D=inp["means3D"], means2D=inp["means2D"], opacities=inp["opacities"], **kw)
    loss = (color * torch.tensor(dpix, device="cuda")).sum()
    if ddepth is not None:
        loss = loss + (depth * torch.tensor(ddepth, device="cuda")).sum()
    loss.backward()
    torch.cuda.synchronize()
    return {k: v.detach().cpu().numpy().astype(np.float64) for k, v in _cam_grads(leaves).items()}


_REF = {}


def _ref(ci, case, dpix, ddepth, mode, scale_mod, extra):
    key = (ci, mode, scale_mod, ddepth is not None)
    if key in _REF:
        return _REF[key]
    g, P = case["g"], case["P"]
    T = lambda a: torch.tensor(np.asarray(a, np.float64), requires_grad=True)  # noqa: E731
    if mode == "precomp":
        o = oracle_forward(case, dtype=np.float64, shs=None, colors_precomp=extra["colors"], scales=None, rotations=None,
                           cov3D_precomp=extra["cov3D"])
        ins = dict(colors_precomp=T(extra["colors"]), cov3D_precomp=T(extra["cov3D"]))
    else:
        o = oracle_forward(case, dtype=np.float64, scale_mod=scale_mod)
        ins = dict(shs=T(g["shs"]), scales=T(g["scales"]), rotations=T(g["rotations"]))
    V, Pm, campos, bg = camera_ref.camera_tensors(o)
    color, dimg = camera_ref.render(o, T(g["means3D"]), T(np.zeros((P, 3))), T(g["opacities"]), V, Pm, campos, bg, **ins)
    loss = (color * torch.tensor(dpix, dtype=torch.float64)).sum()
    if ddepth is not None:
        loss = loss + (dimg * torch.tensor(ddepth, dtype=torch.float64)).sum()
    loss.backward()
    z = lambda t, n: t.grad.numpy() if t.grad is not None else np.zeros(n)  # noqa: E731
    _REF[key] = dict(view=z(V, (4, 4)), proj=z(Pm, (4, 4)), campos=z(campos, 3), bg=z(bg, 3))
    return _REF[key]


@pytest.mark.parametrize("spec", [True, False])
@pytest.mark.parametrize("mode", ["sh", "sh_depth", "precomp", "scale_mod"])
@pytest.mark.parametrize("ci", range(len(CASES)))
def test_camera_gradients_match_fp64_autograd(ci, mode, spec, monkeypatch):
    import diff_gaussian_rasterization as dgr
    monkeypatch.setattr(dgr, "PER_CALL_SPECULATION", spec)
    case = make_case(**CASES[ci])
    dpix, ddepth = _images(case)
    ddepth = ddepth if mode == "sh_depth" else None
    mod = 1.6 if mode == "scale_mod" else 1.0
    extra = _precomp_extra(case) if mode == "precomp" else None
    m = "precomp" if mode == "precomp" else "sh"
    got = _gpu(case, dpix, ddepth, m, mod, extra)
    ref = _ref(ci, case, dpix, ddepth, m, mod, extra)
    assert np.all(got["view"][:, 3] == 0.0)
    for k in CAMS:
        if k == "campos" and mode == "precomp":
            assert np.all(got[k] == 0.0)
            continue
        e = rel_err(got[k], ref[k])
        assert e < TOL, (k, e)


def _views(V=3, P=2000, W=128, H=96, seed=7):
    from csplat import synthetic as syn
    base = make_case(P=P, W=W, H=H, seed=seed)
    cases = [dict(base, cam=syn.make_camera(-40.0 + 35.0 * i, W, H)) for i in range(V)]
    rng = np.random.default_rng(3)
    dpix = [rng.normal(size=(3, H, W)).astype(np.float32) for _ in range(V)]
    ddepth = [rng.normal(size=(1, H, W)).astype(np.float32) if i != 1 else None for i in range(V)]
    return cases, dpix, ddepth


def _batched_vs_single(stacked, V, flags):
    import diff_gaussian_rasterization as dgr
    cases, dpix, ddepth = _views(V)
    _flags(flags)
    try:
        inp = util.gpu_inputs(cases[0])
        leaves = [_cam_leaves(c) for c in cases]
        m2d = [torch.zeros(cases[0]["P"], 3, device="cuda", requires_grad=True) for _ in range(V)]
        loss = 0.0
        for i, c in enumerate(cases):
            color, _r, depth = dgr.GaussianRasterizer(_settings(c, leaves[i]))(
                means3D=inp["means3D"], means2D=m2d[i], opacities=inp["opacities"], shs=inp["shs"], scales=inp["scales"],
                rotations=inp["rotations"])
            loss = loss + (color * torch.tensor(dpix[i], device="cuda")).sum()
            if ddepth[i] is not None:
                loss = loss + (depth * torch.tensor(ddepth[i], device="cuda")).sum()
        loss.backward()
        single = [_cam_grads(lv) for lv in leaves]
        inp = util.gpu_inputs(cases[0])
        leaves = [_cam_leaves(c) for c in cases]
        m2d = [torch.zeros(cases[0]["P"], 3, device="cuda", requires_grad=True) for _ in range(V)]
        kws = [dict(means3D=inp["means3D"], means2D=m2d[i], opacities=inp["opacities"], shs=inp["shs"], scales=inp["scales"],
                    rotations=inp["rotations"]) for i in range(V)]
        settings = [_settings(c, lv) for c, lv in zip(cases, leaves)]
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
        batched = [_cam_grads(lv) for lv in leaves]
    finally:
        _flags(0)
    return single, batched


@pytest.mark.parametrize("flags,tol", [(256, 1e-6), (0, 1e-5)])
@pytest.mark.parametrize("stacked,V", [(False, 3), (True, 4)])
def test_batched_views_equal_per_view_calls(stacked, V, flags, tol):
    single, batched = _batched_vs_single(stacked, V, flags)
    for a, b in zip(single, batched):
        for k in CAMS:
            assert rel_err(b[k].cpu().numpy(), a[k].cpu().numpy()) < tol, k


def test_shared_camera_tensor_sums_over_views():
    """one background tensor passed to every view: autograd sums the views' gradients"""
    import diff_gaussian_rasterization as dgr
    cases, dpix, _dd = _views(3)
    inp = util.gpu_inputs(cases[0])
    bg = torch.tensor(cases[0]["bg"], dtype=torch.float32, device="cuda", requires_grad=True)
    leaves = [_cam_leaves(c) for c in cases]
    for lv in leaves:
        lv["bg"] = bg
    kws = [dict(means3D=inp["means3D"], means2D=torch.zeros(cases[0]["P"], 3, device="cuda"), opacities=inp["opacities"], shs=inp["shs"],
                scales=inp["scales"], rotations=inp["rotations"]) for _ in range(3)]
    outs = dgr.rasterize_views([_settings(c, lv) for c, lv in zip(cases, leaves)], kws)
    sum((outs[i][0] * torch.tensor(dpix[i], device="cuda")).sum() for i in range(3)).backward()
    # per view: dL/dbg_c = sum_pix dpix_c T_final, with T_final = (C - sum T alpha c) / bg ... checked through single-view calls instead
    tot = torch.zeros(3, device="cuda", dtype=torch.float64)
    for i in range(3):
        b1 = torch.tensor(cases[0]["bg"], dtype=torch.float32, device="cuda", requires_grad=True)
        lv = _cam_leaves(cases[i])
        lv["bg"] = b1
        color, _r, _d = dgr.GaussianRasterizer(_settings(cases[i], lv))(**kws[i])
        (color * torch.tensor(dpix[i], device="cuda")).sum().backward()
        tot += b1.grad.double()
    torch.cuda.synchronize()
    assert rel_err(bg.grad.cpu().numpy(), tot.cpu().numpy()) < 1e-5


def test_translation_identity_full_size():
    """the bench shape: moving the world by delta (means and campos + delta, V' = A V, Pm' = A Pm, A = [[I, 0], [-delta, 1]]) changes
    nothing, so sum_i dL/dm_i + sum_views (dL/dcampos - V[:3,:] dL/dV[3,:] - Pm[:3,:] dL/dPm[3,:]) = 0"""
    import diff_gaussian_rasterization as dgr
    from csplat import synthetic as syn
    P, S, NV = 100_000, 800, 4
    sc = syn.scene_1(P=P, W=S, H=S, n_cams=NV, seed=0)
    g = syn.gaussians_at(sc)
    T = lambda x, rg=True: torch.tensor(np.asarray(x, np.float32), device="cuda", requires_grad=rg)  # noqa: E731
    inp = {k: T(g[k]) for k in ("means3D", "opacities", "shs", "scales", "rotations")}
    settings = [dgr.GaussianRasterizationSettings(
        image_height=S, image_width=S, tanfovx=c["tanfovx"], tanfovy=c["tanfovy"], bg=T(sc["bg"]), scale_modifier=1.0,
        viewmatrix=T(c["world_view_transform"]), projmatrix=T(c["full_proj_transform"]), sh_degree=3, campos=T(c["camera_center"]),
        prefiltered=False, debug=False) for c in sc["cameras"][:NV]]
    kws = [dict(means3D=inp["means3D"], means2D=torch.zeros(P, 3, device="cuda", requires_grad=True),
                **{k: inp[k] for k in ("opacities", "shs", "scales", "rotations")}) for _ in range(NV)]
    gen = torch.Generator(device="cuda").manual_seed(0)
    target = torch.rand(NV, 3, S, S, device="cuda", generator=gen)
    dtarget = torch.rand(NV, 1, S, S, device="cuda", generator=gen) * 4.0
    colors, outs = dgr.rasterize_views(settings, kws, stacked=True)
    loss = (colors - target).abs().mean() + (torch.stack([o[2] for o in outs]) - dtarget).abs().mean()
    loss.backward()
    torch.cuda.synchronize()
    dm = inp["means3D"].grad.double()
    res = dm.sum(0)
    for rs in settings:
        Vm, Pm = rs.viewmatrix.detach().double(), rs.projmatrix.detach().double()
        res = res + rs.campos.grad.double() - Vm[:3, :] @ rs.viewmatrix.grad.double()[3, :] - Pm[:3, :] @ rs.projmatrix.grad.double()[3, :]
        assert float(rs.viewmatrix.grad.abs().max()) > 0 and float(rs.projmatrix.grad.abs().max()) > 0
    scale = float(dm.abs().sum())
    assert float(res.abs().max()) <= 1e-4 * scale, (res.cpu().numpy(), scale)


def _one_call(case, leaves_grad, dpix, ddepth):
    import diff_gaussian_rasterization as dgr
    inp = util.gpu_inputs(case)
    leaves = _cam_leaves(case)
    if not leaves_grad:
        for k in leaves:
            leaves[k].requires_grad_(False)
    color, _r, depth = dgr.GaussianRasterizer(_settings(case, leaves))(
        means3D=inp["means3D"], means2D=inp["means2D"], opacities=inp["opacities"], shs=inp["shs"], scales=inp["scales"],
        rotations=inp["rotations"])
    ((color * torch.tensor(dpix, device="cuda")).sum() + (depth * torch.tensor(ddepth, device="cuda")).sum()).backward()
    torch.cuda.synchronize()
    gauss = [inp[k].grad.clone() for k in ("means3D", "means2D", "opacities", "shs", "scales", "rotations")]
    return gauss, leaves


@pytest.mark.parametrize("spec", [True, False])
def test_rest_of_backward_untouched_and_reproducible(spec, monkeypatch):
    """bit-reproducible mode: asking for camera gradients changes no bit of a Gaussian gradient, and two identical calls give
    bit-identical camera gradients; without a settings tensor requiring grad, their .grad stays None"""
    import diff_gaussian_rasterization as dgr
    monkeypatch.setattr(dgr, "PER_CALL_SPECULATION", spec)
    case = make_case(**CASES[1])
    dpix, ddepth = _images(case)
    _flags(256)
    try:
        g0, lv0 = _one_call(case, False, dpix, ddepth)
        g1, lv1 = _one_call(case, True, dpix, ddepth)
        g2, lv2 = _one_call(case, True, dpix, ddepth)
    finally:
        _flags(0)
    assert all(lv0[k].grad is None for k in lv0)
    for a, b, c in zip(g0, g1, g2):
        assert torch.equal(a, b) and torch.equal(b, c)
    for k in lv1:
        assert torch.equal(lv1[k].grad, lv2[k].grad), k


def test_camera_gradient_on_faith_raises():
    import diff_gaussian_rasterization as dgr
    from csplat import graphs
    cases, dpix, _dd = _views(V=2)
    inp = util.gpu_inputs(cases[0])
    kws = [dict(means3D=inp["means3D"], means2D=torch.zeros(cases[0]["P"], 3, device="cuda", requires_grad=True), opacities=inp["opacities"],
                shs=inp["shs"], scales=inp["scales"], rotations=inp["rotations"]) for _ in range(2)]
    settings = [_settings(c, _cam_leaves(c)) for c in cases]
    _out, counts = graphs.counts_of_eager(lambda: dgr.rasterize_views(settings, kws, stacked=True))
    faith = {"caps": graphs.caps_from_counts(counts), "valid": torch.zeros(1, dtype=torch.int32, device="cuda")}
    with dgr.forward_mode(faith=faith):
        colors, _outs = dgr.rasterize_views(settings, kws, stacked=True)
    torch.cuda.synchronize()
    assert dgr.forward_mode_is_default()
    with pytest.raises(RuntimeError, match="camera / background gradient"):
        (colors * torch.tensor(np.stack(dpix), device="cuda")).sum().backward()


def test_camera_gradient_in_deferred_k8_raises():
    import diff_gaussian_rasterization as dgr
    cases, dpix, _dd = _views(V=2)
    inp = util.gpu_inputs(cases[0])
    kws = [dict(means3D=inp["means3D"], means2D=torch.zeros(cases[0]["P"], 3, device="cuda", requires_grad=True), opacities=inp["opacities"],
                shs=inp["shs"], scales=inp["scales"], rotations=inp["rotations"]) for _ in range(2)]
    settings = [_settings(c, _cam_leaves(c)) for c in cases]
    colors, _outs = dgr.rasterize_views(settings, kws, stacked=True)
    with pytest.raises(RuntimeError, match="deferred_k8"):
        with dgr.deferred_k8():
            (colors * torch.tensor(np.stack(dpix), device="cuda")).sum().backward()
    torch.cuda.synchronize()


def _pose_errors(wv_true, wv_est):
    rel = torch.linalg.inv(wv_true) @ wv_est          # [[R^T, 0], [t, 1]] of the remaining correction
    c = float(((torch.trace(rel[:3, :3]) - 1.0) / 2.0).clamp(-1.0, 1.0))
    return math.acos(c), float(rel[3, :3].norm())


def test_pose_recovery():
    """a 0.5 degree / 1 % pose error is refined by Adam on (omega, tau) through csplat.camera.perturbed and an L1 photometric loss.
    Learning rates 1e-3 (omega) and 1e-2 (tau), decayed by 0.995 per step, 200 steps (bar: both errors <= 1/4 of their start, <= 200
    steps).  Measured: both errors fall to 6-9 % of their start (12 / 9 % after 150 steps)."""
    import diff_gaussian_rasterization as dgr
    from csplat import camera as camlib
    from csplat import synthetic as syn
    P, S = 20_000, 256
    sc = syn.scene_1(P=P, W=S, H=S, n_cams=1, seed=0)
    g = syn.gaussians_at(sc)
    c = sc["cameras"][0]
    T = lambda x: torch.tensor(np.asarray(x, np.float32), device="cuda")  # noqa: E731
    inp = {k: T(g[k]) for k in ("means3D", "opacities", "shs", "scales", "rotations")}
    true = SimpleNamespace(world_view_transform=T(c["world_view_transform"]), full_proj_transform=T(c["full_proj_transform"]),
                           camera_center=T(c["camera_center"]), tanfovx=c["tanfovx"], tanfovy=c["tanfovy"])
    bg = T(sc["bg"])

    def render(cam):
        rs = dgr.GaussianRasterizationSettings(
            image_height=S, image_width=S, tanfovx=cam.tanfovx, tanfovy=cam.tanfovy, bg=bg, scale_modifier=1.0,
            viewmatrix=cam.world_view_transform, projmatrix=cam.full_proj_transform, sh_degree=3, campos=cam.camera_center,
            prefiltered=False, debug=False)
        return dgr.GaussianRasterizer(rs)(means3D=inp["means3D"], means2D=torch.zeros(P, 3, device="cuda"), **{
            k: inp[k] for k in ("opacities", "shs", "scales", "rotations")})[0]
    rng = np.random.default_rng(1)
    axis = rng.normal(size=3); axis /= np.linalg.norm(axis)
    tdir = rng.normal(size=3); tdir /= np.linalg.norm(tdir)
    dist = float(np.linalg.norm(c["camera_center"]))
    start = camlib.perturbed(true, T(axis * math.radians(0.5)), T(tdir * 0.01 * dist))
    start = SimpleNamespace(**{k: (v.detach() if torch.is_tensor(v) else v) for k, v in vars(start).items()})
    _flags(256)
    try:
        with torch.no_grad():
            target = render(true)
        omega = torch.zeros(3, device="cuda", requires_grad=True)
        tau = torch.zeros(3, device="cuda", requires_grad=True)
        opt = torch.optim.Adam([dict(params=[omega], lr=1e-3), dict(params=[tau], lr=1e-2)])
        sched = torch.optim.lr_scheduler.ExponentialLR(opt, 0.995)
        r0, t0 = _pose_errors(true.world_view_transform.double(), start.world_view_transform.double())
        for _ in range(200):
            opt.zero_grad()
            cam = camlib.perturbed(start, omega, tau)
            (render(cam) - target).abs().mean().backward()
            opt.step()
            sched.step()
        with torch.no_grad():
            r1, t1 = _pose_errors(true.world_view_transform.double(), camlib.perturbed(start, omega, tau).world_view_transform.double())
    finally:
        _flags(0)
    assert r1 <= 0.25 * r0 and t1 <= 0.25 * t0, (r0, r1, t0, t1)
