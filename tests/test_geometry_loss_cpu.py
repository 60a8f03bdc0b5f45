"""The geometry loss (depth and silhouette supervision, csplat.train.geometry_losses) without a GPU: the float64 restatement
(tests/geometry_loss_ref.py) against the known answer, against autograd of its own loss, and for its selection semantics; the CPU
composition of geometry_losses against the restatement; every argument error; the header, the library and the binding."""
import os
import re
from types import SimpleNamespace

import pytest

import util
import geometry_loss_ref as R

torch = pytest.importorskip("torch")
F64 = torch.float64


def _t(rows, dtype=F64):
    return [torch.tensor(rows, dtype=dtype).reshape(1, 1, -1)]


def _views(gen, V, H, W, lo=0.0, hi=1.0, dtype=F64):
    return [lo + (hi - lo) * torch.rand(1, H, W, generator=gen, dtype=dtype) for _ in range(V)]


def _grad_bound(g, lam_d, lam_s, Z, n):
    """four float64 roundings of the gradients' unit |g| max(lambda_depth max(1, max valid Z), lambda_silhouette) / n: the two sides
    multiply the same factors in another order"""
    zs = torch.stack(Z)
    zmax = float(zs[torch.isfinite(zs) & (zs > 0)].max()) if bool((torch.isfinite(zs) & (zs > 0)).any()) else 0.0
    return 4 * 2.0 ** -52 * abs(g) * max(lam_d * max(1.0, zmax), lam_s) / n


def test_known_answer():
    """V = 1, H = 1, W = 4, no mask: the worked example of include/csplat.h's semantics"""
    D, A = _t([1.0, 0.5, 0.0, 2.0]), _t([0.5, 0.5, 0.0, 1.0])
    Z, S = _t([1.0, 2.0, 3.0, 0.0]), _t([1.0, 0.0, 0.0, 1.0])
    lam_d, lam_s, g = 0.7, 0.3, 1.9
    total, ld, ls, gD, gA, codes = R.geometry_loss(D, A, Z, S, None, lam_d, lam_s, g=g)
    assert abs(float(ld) - 0.25) <= 1e-15 and abs(float(ls) - 0.25) <= 1e-15
    assert abs(float(total) - (lam_d * 0.25 + lam_s * 0.25)) <= 1e-15
    want_D = g * lam_d / 4 * torch.tensor([1.0, -1.0, 0.0, 0.0], dtype=F64)
    want_A = g * (lam_d / 4 * torch.tensor([-1.0, 2.0, 0.0, 0.0], dtype=F64) + lam_s / 4 * torch.tensor([-1.0, 1.0, 0.0, 0.0], dtype=F64))
    assert float((gD.reshape(-1) - want_D).abs().max()) <= 1e-15
    assert float((gA.reshape(-1) - want_A).abs().max()) <= 1e-15
    # the byte: depth signs (+, -, 0, invalid -> 0) in bits 0-1, silhouette signs (-, +, 0, 0) in bits 2-3
    assert codes.reshape(-1).tolist() == [2 | (0 << 2), 0 | (2 << 2), 1 | (1 << 2), 1 | (1 << 2)]


@pytest.mark.parametrize("with_mask", [False, True])
def test_closed_form_gradients_equal_autograd(with_mask):
    """random float64 inputs have no ties: the closed forms are autograd's gradient of the restated loss"""
    gen = torch.Generator().manual_seed(5)
    V, H, W = 3, 7, 9
    D, A = _views(gen, V, H, W, 0.0, 3.0), _views(gen, V, H, W)
    Z, S = _views(gen, V, H, W, -0.5, 4.0), _views(gen, V, H, W)     # (some Z <= 0: holes)
    M = _views(gen, V, H, W) if with_mask else None
    if with_mask:
        for m in M:
            m[0, :2] = 0.0
    lam_d, lam_s = 0.6, 1.7
    total, _ld, _ls, gD, gA, _c = R.geometry_loss(D, A, Z, S, M, lam_d, lam_s)
    Ds, As = torch.stack(D).requires_grad_(), torch.stack(A).requires_grad_()
    loss = R.differentiable_loss(Ds, As, torch.stack(Z), torch.stack(S), None if M is None else torch.stack(M), lam_d, lam_s)
    loss.backward()
    assert abs(float(loss.detach()) - float(total)) <= 1e-15
    bound = _grad_bound(1.0, lam_d, lam_s, Z, V * H * W)
    assert float((Ds.grad.reshape(gD.shape) - gD).abs().max()) <= bound
    assert float((As.grad.reshape(gA.shape) - gA).abs().max()) <= bound
    assert float(gD.abs().max()) > 0 and float(gA.abs().max()) > 0


def test_selection_not_multiplication():
    """NaN / Inf / 0 / negative Z are holes, M = 0 switches a pixel off: the loss stays finite and the gradients there are EXACTLY zero,
    whatever D and A hold there"""
    nan, inf = float("nan"), float("inf")
    Z = _t([nan, inf, 0.0, -1.0, 2.0, 2.0, -inf, 1.0])
    D = _t([1.0, 1.0, 1.0, 1.0, nan, 1.5, inf, 3.0])
    A = _t([0.5, 0.5, 0.5, 0.5, 0.5, nan, nan, 0.5])
    S = _t([1.0, 1.0, 0.0, 1.0, 1.0, 1.0, 1.0, 0.0])
    M = _t([1.0, 1.0, 1.0, 1.0, 0.0, 0.0, 0.0, 1.0])
    total, ld, ls, gD, gA, codes = R.geometry_loss(D, A, Z, S, M, 1.0, 1.0)
    assert all(bool(torch.isfinite(x)) for x in (total, ld, ls))
    assert abs(float(ld) - (3.0 - 0.5) / 8) <= 1e-15            # only the last pixel has a depth term
    assert abs(float(ls) - (4 * 0.5 + 0.5) / 8) <= 1e-15        # pixels 0-3 and 7
    assert gD.reshape(-1)[:7].tolist() == [0.0] * 7 and gA.reshape(-1)[4:7].tolist() == [0.0] * 3
    assert bool(torch.isfinite(gD).all()) and bool(torch.isfinite(gA).all())
    assert codes.reshape(-1)[4:7].tolist() == [1 | (1 << 2)] * 3
    # depth only, every Z a hole: exactly zero
    total, ld, _ls, gD, gA, _c = R.geometry_loss(D, A, _t([nan, inf, 0.0, -1.0, 0.0, 0.0, -inf, -2.0]), None, None, 1.0, 0.0)
    assert float(total) == 0.0 and float(ld) == 0.0 and not gD.any() and not gA.any()
    # a NaN where the weight is NOT zero makes the term NaN
    _tot, ld, ls, _gD, _gA, codes = R.geometry_loss(_t([nan, 1.0]), _t([0.5, 0.5]), _t([1.0, 1.0]), _t([1.0, 1.0]), None, 1.0, 1.0)
    assert bool(torch.isnan(ld)) and bool(torch.isfinite(ls)) and codes.reshape(-1).tolist() == [3 | (0 << 2), 2 | (0 << 2)]


@pytest.mark.parametrize("variant", ["both", "depth", "silhouette", "masked", "holes_and_nans", "add_weight"])
def test_cpu_composition_equals_restatement(variant):
    """csplat.train.geometry_losses on float64 CPU tensors composes the formulas from torch operations: loss values and autograd
    gradients equal the restatement's closed forms"""
    from csplat import train as tr
    gen = torch.Generator().manual_seed(11)
    V, H, W = 2, 5, 6
    D = [d.requires_grad_() for d in _views(gen, V, H, W, 0.0, 3.0)]
    A = [a.requires_grad_() for a in _views(gen, V, H, W)]
    Z, S = _views(gen, V, H, W, -0.5, 4.0), _views(gen, V, H, W)
    M = None
    lam_d, lam_s = {"depth": (0.8, 0.0), "silhouette": (0.0, 0.4)}.get(variant, (0.8, 0.4))
    add, kw = None, {}
    if variant in ("masked", "holes_and_nans"):
        M = _views(gen, V, H, W)
        M[0][0, 1] = 0.0
    if variant == "holes_and_nans":
        with torch.no_grad():
            Z[0][0, 0, :4] = torch.tensor([float("nan"), float("inf"), 0.0, -3.0], dtype=F64)
            D[0][0, 0, 0] = float("nan")              # under a hole
            D[0][0, 1, 2], A[0][0, 1, 3] = float("inf"), float("nan")      # under M = 0
    if variant == "add_weight":
        add = torch.tensor(0.37, dtype=F64, requires_grad=True)
        kw = dict(weight=0.5, add_weight=0.25)
    total, ld, ls = tr.geometry_losses(D, A, Z if lam_d else None, S if lam_s else None, lam_d, lam_s, masks=M, add=add, **kw)
    g = 1.3
    total.backward(torch.tensor(g, dtype=F64))
    r_total, r_ld, r_ls, r_gD, r_gA, _c = R.geometry_loss(D, A, Z, S, M, lam_d, lam_s, add=add, g=g, **kw)
    assert not ld.requires_grad and not ls.requires_grad
    assert abs(float(total.detach()) - float(r_total)) <= 1e-15 and abs(float(ld) - float(r_ld)) <= 1e-15 and abs(float(ls) - float(r_ls)) <= 1e-15
    bound = _grad_bound(g * kw.get("weight", 1.0), lam_d, lam_s, Z, V * H * W)
    for v in range(V):
        if lam_d:
            assert float((D[v].grad.reshape(H, W) - r_gD[v]).abs().max()) <= bound
        else:
            assert D[v].grad is None
        assert float((A[v].grad.reshape(H, W) - r_gA[v]).abs().max()) <= bound
    if add is not None:
        assert abs(float(add.grad) - g * 0.25) <= 1e-17
    if variant == "holes_and_nans":
        assert torch.isfinite(total) and D[0].grad[0, 0, 0] == 0.0 and D[0].grad[0, 1, 2] == 0.0 and A[0].grad[0, 1, 3] == 0.0


def test_argument_errors_are_value_errors():
    from csplat import train as tr
    gen = torch.Generator().manual_seed(2)
    V, H, W = 2, 4, 5
    D, A, Z, S = (_views(gen, V, H, W) for _ in range(4))
    ok = lambda **kw: tr.geometry_losses(**{**dict(depths=D, alphas=A, gt_depths=Z, silhouettes=S, lambda_depth=1.0,  # noqa: E731
                                                  lambda_silhouette=1.0), **kw})
    assert len(ok()) == 3
    bad = [dict(lambda_depth=0.0, lambda_silhouette=0.0),                    # no term on
           dict(lambda_depth=-1.0),
           dict(gt_depths=None),                                             # a weight > 0 without its data
           dict(silhouettes=None),
           dict(depths=None),
           dict(alphas=[]),
           dict(gt_depths=Z[:1]),                                            # view counts differ
           dict(silhouettes=[S[0], torch.rand(1, H, W + 1, dtype=F64)]),     # all views one size
           dict(alphas=[A[0], torch.rand(1, H + 1, W, dtype=F64)]),
           dict(depths=[D[0], torch.rand(3, H, W, dtype=F64)]),              # one plane per view
           dict(gt_depths=[z.float() for z in Z]),                           # dtypes differ
           dict(masks=[torch.ones(1, H, W, dtype=torch.bool)] * V),
           dict(masks=[torch.ones(1, H, W, dtype=F64)]),
           dict(silhouettes=[S[0], S[1].to("meta")]),                        # devices differ
           dict(add=torch.zeros(2, dtype=F64)),
           dict(gt_depths=[z.clone().requires_grad_() for z in Z])]
    for kw in bad:
        with pytest.raises(ValueError):
            ok(**kw)
    # a term that is off needs no data
    assert len(ok(lambda_depth=0.0, gt_depths=None, depths=None)) == 3 and len(ok(lambda_silhouette=0.0, silhouettes=None)) == 3


def test_train_step_checks_cameras_before_the_simulator():
    """a weight > 0 with a camera that lacks the field, or carries another shape or dtype, is a ValueError -- and the view-parallel and
    per-camera paths refuse the terms -- before the simulator or anything else of the step runs"""
    from csplat import train as tr

    class Untouchable:
        def __getattr__(self, name):
            raise AssertionError(f"the step touched .{name} before it checked its cameras")

    H, W = 6, 8
    cam = lambda **kw: SimpleNamespace(image_height=H, image_width=W, mask=None, **kw)  # noqa: E731
    step = lambda cams, opt, **kw: tr.train_step(1, cams, Untouchable(), Untouchable(), Untouchable(), opt=opt, **kw)  # noqa: E731
    both = SimpleNamespace(**vars(tr.DEFAULT_OPT), lambda_depth=0.5, lambda_silhouette=0.5)
    depth_only = SimpleNamespace(**vars(tr.DEFAULT_OPT), lambda_depth=0.5)
    good = dict(depth=torch.ones(1, H, W), silhouette=torch.ones(H, W))
    for cams, opt in [([cam(depth=good["depth"])], both),                                       # no silhouette
                      ([cam(**good), cam(silhouette=good["silhouette"])], both),                 # the second camera lacks depth
                      ([cam(depth=torch.ones(1, H, W + 1))], depth_only),                        # shape
                      ([cam(depth=torch.ones(3, H, W))], depth_only),
                      ([cam(depth=torch.ones(1, H, W, dtype=F64))], depth_only),                 # dtype
                      ([cam(depth=[[1.0]])], depth_only),                                        # not a tensor
                      ([cam(**good), SimpleNamespace(image_height=H + 1, image_width=W, mask=None, depth=torch.ones(1, H + 1, W))], depth_only),
                      ([cam(**good)], SimpleNamespace(**vars(tr.DEFAULT_OPT), lambda_depth=-0.5))]:
        with pytest.raises(ValueError):
            step(cams, opt)
    with pytest.raises(NotImplementedError):
        step([cam(**good)], both, batched_views=False)
    assert tr._geometry_weights(tr.DEFAULT_OPT) == (0.0, 0.0) and not hasattr(tr.DEFAULT_OPT, "lambda_depth")


def test_render_views_return_alpha_keeps_the_default_return():
    from gaussian_renderer import render_views
    assert render_views([], None, None, None, None) == [] and render_views([], None, None, None, None, return_stacked=True) == ([], None)
    assert render_views([], None, None, None, None, return_alpha=True) == ([], [])
    assert render_views([], None, None, None, None, return_stacked=True, return_alpha=True) == ([], None, [])


def test_header_and_exports():
    from csplat import native
    hdr = open(os.path.join(util.ROOT, "include", "csplat.h")).read()
    for name in ("csplat_geom_loss_scratch_bytes", "csplat_geom_loss_fwd", "csplat_geom_loss_bwd"):
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
        assert name in native.EXPORTS and hasattr(native.lib, name)
    assert native.PROF_TRAIN_CLASSES == ["geometry_loss_fwd", "geometry_loss_bwd"]
    # partials: two floats per workgroup, at most 1024 workgroups of 256 pixels per view; grows with the views, never 0
    sizes = [int(native.lib.csplat_geom_loss_scratch_bytes(V, hw)) for V, hw in ((1, 1), (1, 257), (3, 640_000), (17, 640_000))]
    assert sizes[0] >= 8 and sizes[1] >= 2 * 2 * 4 and sizes[2] >= 2 * 3 * 1024 * 4 and sizes[3] >= 2 * 17 * 1024 * 4
    assert sizes == sorted(sizes)
