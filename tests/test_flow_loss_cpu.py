"""The optical-flow term without a GPU: known answers of the restatement tests/flow_loss_ref.py (and of the CPU composition of
csplat.flow_loss.flow_losses, which must equal it), the selection semantics, every argument error of flow_losses and of the train
step's plan, and the library's surface (header, exports, bindings, ABI number, scratch size)."""
import os
import re
from types import SimpleNamespace

import pytest
import torch

import util  # noqa: F401
import flow_loss_ref as R

F64 = torch.float64
NAN, INF = float("nan"), float("inf")
W, H = 16, 8          # powers of two: the orthographic projection of a dyadic coordinate is exact


def ortho(T):
    return [R.ortho_full(W, H) for _ in range(T)]


def pts(*rows):
    """points [P,3] in float64 from (x, y) pairs: under the orthographic camera pixel = (x, y)"""
    return torch.tensor([[x, y, 0.0] for x, y in rows], dtype=F64)


def const_flow(dx, dy):
    return torch.stack([torch.full((H, W), float(dx), dtype=F64), torch.full((H, W), float(dy), dtype=F64)])


def both(points, fulls, flows, **kw):
    """(the restatement, flow_losses on CPU float64 tensors with its gradient) on the same inputs"""
    from csplat.flow_loss import flow_losses
    ref = R.flow_loss(points, fulls, flows, W, H, **kw)
    X = [p.clone().requires_grad_() for p in points]
    g = kw.pop("g", 1.0)
    lam = kw.pop("lam", 1.0)
    total, lf, nv = flow_losses(X, fulls, flows, (H, W), lambda_flow=lam, **kw)
    if total.requires_grad:
        total.backward(torch.tensor(g, dtype=F64))
    grad = torch.stack([torch.zeros_like(x) if x.grad is None else x.grad for x in X])
    return ref, SimpleNamespace(total=total.detach(), L=lf, count=int(nv), grad=grad, nv=nv)


def assert_same(ref, got, tol=1e-13):
    assert got.count == ref["count"]
    assert abs(float(got.L) - float(ref["L"])) <= tol and abs(float(got.total) - float(ref["total"])) <= tol
    assert float((got.grad - ref["grad"]).abs().max()) <= tol
    assert not got.L.requires_grad and got.nv.dtype == torch.int32


# ------------------------------------------------------------------------------------------------------------------ known answers
def test_exact_displacement_is_a_tie_with_zero_loss_and_zero_gradient():
    a, b = pts((1.5, 2.25), (3.0, 4.0), (6.75, 0.5)), pts((2.5, 2.0), (4.0, 3.75), (7.75, 0.25))
    ref, got = both([a, b], ortho(2), [const_flow(1.0, -0.25)])
    assert ref["count"] == 3 and float(ref["L"]) == 0.0 and not ref["grad"].any()       # sign(0) = 0
    assert_same(ref, got, 0.0)


def test_constant_offset_gives_the_hand_value_and_unit_gradients():
    a, b = pts((1.5, 2.25), (3.0, 4.0)), pts((3.0, 2.0), (3.5, 5.0))
    # flow (1, 0): r = (1.5 - 1, -0.25) and (0.5 - 1, 1.0): e = 0.75 and 1.5, n = 2
    ref, got = both([a, b], ortho(2), [const_flow(1.0, 0.0)])
    assert ref["count"] == 2 and abs(float(ref["L"]) - (0.75 + 1.5) / 2) < 1e-15
    want_b = torch.tensor([[1.0, -1.0, 0.0], [-1.0, 1.0, 0.0]], dtype=F64) / 2        # dL/dp_b = s / n; a constant flow has J_g = 0
    assert torch.equal(ref["grad"][1], want_b) and torch.equal(ref["grad"][0], -want_b)
    assert_same(ref, got, 1e-15)
    # a mask weighs value and gradient: m = 0.5 at the nearest pixel of point 0, 1 elsewhere
    M = torch.ones(H, W, dtype=F64)
    M[2, 2] = 0.5                                                                    # (floor(2.25 + 0.5), floor(1.5 + 0.5))
    ref, got = both([a, b], ortho(2), [const_flow(1.0, 0.0)], masks=[M])
    assert abs(float(ref["L"]) - (0.5 * 0.75 + 1.5) / 2) < 1e-15 and torch.equal(ref["grad"][1][0], torch.tensor([0.25, -0.25, 0.0], dtype=F64))
    assert_same(ref, got, 1e-15)


def test_linear_ramp_exercises_the_jacobian_of_the_sample():
    # F = (0.5 x + 0.25 y, -0.125 x): bilinear interpolation reproduces it exactly inside the image; J_g = [[0.5, 0.25], [-0.125, 0]]
    ys, xs = torch.meshgrid(torch.arange(H, dtype=F64), torch.arange(W, dtype=F64), indexing="ij")
    F = torch.stack([0.5 * xs + 0.25 * ys, -0.125 * xs])
    a, b = pts((2.5, 1.5)), pts((7.0, 3.0))
    # g = (1.625, -0.3125); r = (4.5 - 1.625, 1.5 + 0.3125) > 0: s = (1, 1); dL/dp_a = -(I + J^T) s = -(1 + 0.5 - 0.125, 1 + 0.25 + 0)
    ref, got = both([a, b], ortho(2), [F])
    assert abs(float(ref["L"]) - (2.875 + 1.8125)) < 1e-14
    assert torch.allclose(ref["grad"][0][0], torch.tensor([-1.375, -1.25, 0.0], dtype=F64), atol=1e-14)
    assert torch.allclose(ref["grad"][1][0], torch.tensor([1.0, 1.0, 0.0], dtype=F64), atol=1e-14)
    assert_same(ref, got, 1e-14)


def test_a_middle_frame_sums_both_roles_and_the_weights_scale():
    a, b, c = pts((1.5, 2.25), (3.0, 4.0)), pts((3.0, 2.0), (3.5, 5.0)), pts((3.25, 2.5), (2.0, 1.0))
    add = torch.tensor(0.4, dtype=F64)
    ref, got = both([a, b, c], ortho(3), [const_flow(1.0, 0.0), const_flow(0.0, 0.0)], lam=0.7, weight=0.5, add=add, add_weight=2.0, g=-3.0)
    # pair 1: r = (0.25, 0.5), (-1.5, -4): s = (1, 1), (-1, -1)
    scale = -3.0 * 0.5 * 0.7 / 4
    want_mid = scale * (torch.tensor([[1.0, -1.0, 0.0], [-1.0, 1.0, 0.0]], dtype=F64) - torch.tensor([[1.0, 1.0, 0.0], [-1.0, -1.0, 0.0]], dtype=F64))
    assert torch.allclose(ref["grad"][1], want_mid, atol=1e-15)
    assert abs(float(ref["total"]) - (0.5 * 0.7 * float(ref["L"]) + 0.8)) < 1e-15
    assert_same(ref, got, 1e-15)


def test_restatement_gradient_is_autograd_of_a_plain_composition():
    """on inputs without ties and without anything selected out, the `where`-based restatement equals the formulas written plainly"""
    gen = torch.Generator().manual_seed(5)
    P = 40
    X = [torch.cat([1.0 + 5.0 * torch.rand(P, 1, generator=gen, dtype=F64), 1.0 + 3.0 * torch.rand(P, 1, generator=gen, dtype=F64),
                    torch.rand(P, 1, generator=gen, dtype=F64)], 1) for _ in range(3)]
    fulls = [R.ortho_full(W, H) + 0.01 * torch.rand(4, 4, generator=gen, dtype=F64) * torch.tensor([1.0, 1.0, 0.0, 0.2]) for _ in range(3)]
    flows = [torch.randn(2, H, W, generator=gen, dtype=F64) for _ in range(2)]
    ref = R.flow_loss(X, fulls, flows, W, H)
    assert ref["count"] == 2 * P
    leaves = [x.clone().requires_grad_() for x in X]
    total = 0.0
    for t in range(2):
        xa, ya, _ = R.project(leaves[t], fulls[t], W, H)
        xb, yb, _ = R.project(leaves[t + 1], fulls[t + 1], W, H)
        x0, y0 = xa.detach().floor().long(), ya.detach().floor().long()
        fx, fy = xa - x0, ya - y0
        F = flows[t]
        g = (1 - fy) * ((1 - fx) * F[:, y0, x0] + fx * F[:, y0, x0 + 1]) + fy * ((1 - fx) * F[:, y0 + 1, x0] + fx * F[:, y0 + 1, x0 + 1])
        total = total + ((xb - xa - g[0]).abs() + (yb - ya - g[1]).abs()).sum()
    total = total / (2 * P)
    total.backward()
    assert abs(float(total.detach()) - float(ref["L"])) < 1e-14
    assert float((torch.stack([x.grad for x in leaves]) - ref["grad"]).abs().max()) < 1e-14


# ------------------------------------------------------------------------------------------------------------------ selection
def _selection_case(kind):
    a, b = pts((1.5, 2.25), (3.0, 4.0), (5.5, 1.0)), pts((3.0, 2.0), (3.5, 5.0), (6.0, 1.5))
    fulls, flows, kw = ortho(2), [const_flow(1.0, 0.0)], {}
    out = 0                  # the pair that is selected out
    if kind == "nan_point_a":
        a[0, 0] = NAN
    elif kind == "nan_point_b":
        b[0, 1] = NAN
    elif kind == "inf_point":
        a[0, 2] = INF
        fulls[0] = fulls[0].clone()
        fulls[0][2, 0] = 0.5
    elif kind == "nan_flow":
        flows[0][0, 2, 1] = NAN           # tap (y0, x0) of point 0
    elif kind == "inf_flow":
        flows[0][1, 3, 2] = INF           # tap (y1, x1) of point 0, the other channel
    elif kind == "w_zero":
        fulls[1] = fulls[1].clone()
        fulls[1][0, 3] = -1.0 / 3.0       # w_b = 1 - x / 3 = 0 at x = 3: point 0; point 1 (3.5) has w < 0; point 2 (6.0) too
        out = (0, 1, 2)
    elif kind == "invisible":
        kw["visible"] = [torch.tensor([0, 3, 1], dtype=torch.int32), None]
    elif kind == "mask_zero":
        M = torch.ones(H, W, dtype=F64)
        M[2, 2] = 0.0
        kw["masks"] = [M]
    elif kind == "mask_nan":
        M = torch.ones(H, W, dtype=F64)
        M[2, 2] = NAN
        kw["masks"] = [M]
    elif kind == "cap":
        kw["max_error"] = 0.74            # e = 0.75, 1.5, 1.0 -> all out
        out = (0, 1, 2)
    elif kind == "outside":
        a[0, 0] = -0.001
    return a, b, fulls, flows, kw, (out,) if isinstance(out, int) else out


@pytest.mark.parametrize("kind", ["nan_point_a", "nan_point_b", "inf_point", "nan_flow", "inf_flow", "w_zero", "invisible", "mask_zero",
                                  "mask_nan", "cap", "outside"])
def test_an_invalid_pair_adds_nothing_and_receives_nothing(kind):
    a, b, fulls, flows, kw, out = _selection_case(kind)
    ref, got = both([a, b], fulls, flows, **kw)
    assert ref["count"] == 3 - len(out) and [bool(v) for v in ref["valid"][0]] == [i not in out for i in range(3)]
    assert bool(torch.isfinite(ref["L"])) and bool(torch.isfinite(ref["grad"]).all())
    for i in out:
        assert not ref["grad"][:, i].any() and not got.grad[:, i].any()
    keep = [i for i in range(3) if i not in out]
    if keep and kind != "w_zero":
        base = R.flow_loss([a[keep], b[keep]], fulls, flows, W, H, **{k: v for k, v in kw.items() if k not in ("visible", "masks")})
        assert abs(float(ref["L"]) * 3 - float(base["L"]) * len(keep)) < 1e-14
    assert_same(ref, got, 1e-14)


def test_image_edges_are_inclusive_and_the_clamped_tap_weighs_nothing():
    ys, xs = torch.meshgrid(torch.arange(H, dtype=F64), torch.arange(W, dtype=F64), indexing="ij")
    F = torch.stack([0.5 * xs, 0.25 * ys])
    a = pts((0.0, 0.0), (W - 1.0, H - 1.0), (W - 1.0, 2.5), (W - 0.999, 1.0), (3.0, H - 0.999))
    b = a + 2.0
    ref, got = both([a, b], ortho(2), [F])
    assert [bool(v) for v in ref["valid"][0]] == [True, True, True, False, False]
    # point 1 at (W-1, H-1): r = (2 - 7.5, 2 - 1.75), s = (-1, 1), and both clamped taps weigh nothing: dL/dp_a = -s / n
    assert abs(float(ref["grad"][0][1][0]) - 1.0 / 5) < 1e-15 and abs(float(ref["grad"][0][1][1]) + 1.0 / 5) < 1e-15
    assert abs(float(ref["grad"][0][2][1]) + (1.0 + 0.25) / 5) < 1e-15
    assert_same(ref, got, 1e-14)
    cap = R.flow_loss([a, b], ortho(2), [F], W, H, max_error=float(2.0 + 2.0))          # e of point 0 is exactly 4: `<=` keeps it
    assert bool(cap["valid"][0][0])


def test_decision_margin_is_the_distance_to_the_nearest_decision():
    a, b = pts((1.5, 2.25), (3.0004, 4.3), (5.5, 1.25)), pts((3.0, 2.0), (3.5, 5.0), (6.5002, 1.75))
    r = R.flow_loss([a, b], ortho(2), [const_flow(1.0, 0.0)], W, H, max_error=0.76)
    m = r["margin"][0]
    assert abs(float(m[0]) - 0.01) < 1e-12          # |e - cap| = |0.75 - 0.76|
    assert abs(float(m[1]) - 0.0004) < 1e-12        # x_a next to an integer
    assert abs(float(m[2]) - 0.0002) < 1e-12        # |r_x|
    far = R.flow_loss([pts((-5.0, 1.0)), pts((1.0, 1.0))], ortho(2), [const_flow(1.0, 0.0)], W, H)
    assert float(far["margin"][0][0]) == INF and far["count"] == 0


def test_float32_inputs_take_the_composition_on_the_cpu_too():
    from csplat.flow_loss import flow_losses
    a, b = pts((1.5, 2.25), (3.0, 4.0)).float(), pts((3.0, 2.0), (3.5, 5.0)).float()
    total, lf, nv = flow_losses(torch.stack([a, b]).requires_grad_(), [f.float() for f in ortho(2)], [const_flow(1.0, 0.0).float().numpy()[None]] * 2,
                                (H, W), visible=[torch.tensor([True, True]), None], masks=[torch.ones(1, H, W)] * 2)
    assert abs(float(lf) - 1.125) < 1e-6 and int(nv) == 2 and total.requires_grad and total.dtype == torch.float32


# ------------------------------------------------------------------------------------------------------------------ argument errors
def test_flow_losses_refuses_every_malformed_argument():
    from csplat.flow_loss import flow_losses
    a, b = pts((1.5, 2.25), (3.0, 4.0)), pts((3.0, 2.0), (3.5, 5.0))
    good = dict(points=[a, b], full_projs=ortho(2), flows=[const_flow(1.0, 0.0)], image_size=(H, W))

    def bad(match, **kw):
        with pytest.raises(ValueError, match=match):
            flow_losses(**{**good, **kw})

    bad("lambda_flow", lambda_flow=-1.0)
    bad("lambda_flow", lambda_flow=NAN)
    bad("max_error", max_error=0.0)
    bad("max_error", max_error=-2.0)
    bad("max_error", max_error=INF)
    bad("frames", points=[a])
    bad("frames", points=[a] * 17, full_projs=ortho(17), flows=[const_flow(0, 0)] * 16)
    bad(r"\[T,P,3\]", points=torch.zeros(2, 3))
    bad("one size", points=[a, b[:1]])
    bad("one size", points=[a, b.float()])
    bad(r"\[P,3\]", points=[torch.zeros(0, 3, dtype=F64)] * 2)
    bad(r"\[P,3\]", points=[a.long(), b.long()])
    bad("image_size", image_size=5)
    bad("image_size", image_size=(0, W))
    bad("full_projs", full_projs=ortho(3))
    bad("full_projs", full_projs=[torch.zeros(3, 4)] * 2)
    bad("constants", full_projs=[f.clone().requires_grad_() for f in ortho(2)])
    bad("`flows`", flows=[])
    bad("`flows`", flows=[const_flow(0, 0)] * 3)
    bad("`flows` holds", flows=[[1.0]])
    bad("`flows` image of shape", flows=[torch.zeros(2, H, W + 1, dtype=F64)])
    bad("`flows` image of dtype", flows=[torch.zeros(2, H, W, dtype=torch.int32)])
    bad("constants", flows=[const_flow(0, 0).requires_grad_()])
    bad("`masks`", masks=[])
    bad("`masks` image of shape", masks=[torch.ones(H + 1, W, dtype=F64)])
    bad("`visible`", visible=[None])
    bad("`visible` holds", visible=[torch.ones(2), None])
    bad("`visible` holds", visible=[torch.ones(3, dtype=torch.int32), None])
    bad("`add`", add=torch.zeros(2, dtype=F64))
    bad("`add`", add=1.0)


def _opt(**kw):
    from csplat import train as tr
    return SimpleNamespace(**vars(tr.DEFAULT_OPT), **kw)


def _cam(**kw):
    return SimpleNamespace(image_height=H, image_width=W, mask=None, **kw)


class Untouchable:
    def __getattr__(self, name):
        raise AssertionError(f"the step touched .{name} before it checked its options and cameras")


def _step(cams, opt, **kw):
    from csplat import train as tr
    return tr.train_step(1, cams, Untouchable(), Untouchable(), Untouchable(), opt=opt, **kw)


def test_train_step_options_and_plan_refusals(monkeypatch):
    from csplat import flow_loss, native, train as tr
    assert tr.flow_losses is flow_loss.flow_losses and tr.FlowLoss is flow_loss.FlowLoss
    assert any(c is flow_loss._FLOW_SCRATCH for c in native.TICKET_CACHES)
    assert tr._flow_options(tr.DEFAULT_OPT) == (0.0, None) and not hasattr(tr.DEFAULT_OPT, "lambda_flow")
    assert tr._flow_options(_opt(lambda_flow=0.5, flow_max_error=3)) == (0.5, 3.0)
    assert tr._flow_options(_opt(lambda_flow=None, flow_max_error=None)) == (0.0, None)
    for kw in (dict(lambda_flow=-1.0), dict(lambda_flow=NAN), dict(lambda_flow=INF)):
        with pytest.raises(ValueError, match="lambda_flow"):
            tr._flow_options(_opt(**kw))
    for cap in (0.0, -1.0, NAN):
        with pytest.raises(ValueError, match="flow_max_error"):
            tr._flow_options(_opt(lambda_flow=1.0, flow_max_error=cap))
    assert tr._optional_terms_on(_opt(lambda_flow=0.5)) is True and tr._optional_terms_on(_opt(lambda_flow=0.0)) is False
    flow = torch.zeros(2, H, W)
    on = _opt(lambda_flow=0.5)
    with pytest.raises(ValueError, match="lambda_flow"):
        _step([_cam(flow=flow), _cam()], _opt(lambda_flow=-0.5), batched_views=False)
    with pytest.raises(NotImplementedError, match="optical-flow term needs batched_views"):
        _step([_cam()], on, batched_views=False)
    with pytest.raises(ValueError, match="at least 2 cameras"):
        _step([_cam(flow=flow)], on)
    with pytest.raises(ValueError, match="`flow`"):
        _step([_cam(), _cam(flow=flow)], on)
    with pytest.raises(ValueError, match="camera.flow is"):
        _step([_cam(flow=torch.zeros(2, H, W + 1)), _cam()], on)
    with pytest.raises(ValueError, match="camera.flow is"):
        _step([_cam(flow=flow.double()), _cam()], on)
    with pytest.raises(ValueError, match="one image size"):
        _step([_cam(flow=flow), SimpleNamespace(image_height=H + 1, image_width=W, mask=None)], on)
    with pytest.raises(ValueError, match="ONE view"):
        _step([_cam(flow=flow, view_id=0), _cam(view_id=1)], on)
    with pytest.raises(ValueError, match="camera.mask"):
        _step([SimpleNamespace(image_height=H, image_width=W, mask=torch.ones(3, H, W), flow=flow), _cam()], on)
    # in order (a numpy flow too, the last camera without one): the step goes on to its first use of the model
    import numpy as np
    with pytest.raises(AssertionError, match="touched"):
        _step([_cam(flow=flow, view_id=2), _cam(flow=np.zeros((1, 2, H, W), np.float32), view_id=2), _cam(view_id=2)], on)
    # the flow term comes LAST: the kNN regularisers' value, refusal and Gaussian count precede every flow refusal
    with pytest.raises(ValueError, match="lambda_spring"):
        _step([_cam()], _opt(lambda_spring=-1.0, lambda_flow=-1.0))
    with pytest.raises(NotImplementedError, match="kNN-graph regularisers need batched_views"):
        _step([_cam()], _opt(lambda_spring=1.0, lambda_flow=-1.0), batched_views=False)
    with pytest.raises(AssertionError, match="touched .num_gaussians"):
        _step([_cam()], _opt(lambda_spring=1.0, k_nearest=5, lambda_flow=-1.0))
    with pytest.raises(ValueError, match="`points`"):
        _step([_cam()], _opt(lambda_chamfer=0.5, lambda_flow=-1.0))
    monkeypatch.setattr(tr.cd, "is_dist", lambda: True)
    with pytest.raises(NotImplementedError, match="optical-flow term is not part of the view-parallel"):
        _step([_cam()], on, view_parallel=True, batched_views=False)


# ------------------------------------------------------------------------------------------------------------------ the library's surface
def test_header_exports_and_bindings():
    from csplat import native
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "csplat.h")).read()
    names = ("csplat_flow_loss_scratch_bytes", "csplat_flow_loss_fwd", "csplat_flow_loss_bwd")
    for name in names:
        assert re.search(r"\b" + name + r"\s*\(", header), name
        assert name in native.EXPORTS and hasattr(native.lib, name)
    assert len(native.EXPORTS["csplat_flow_loss_fwd"][1]) == 19 and len(native.EXPORTS["csplat_flow_loss_bwd"][1]) == 8
    assert "Added exports: CSPLAT_ABI_VERSION is unchanged" in header
    assert native.ABI_VERSION == 9 and native.lib.csplat_abi_version() == 9


def test_scratch_bytes_are_monotone_and_the_library_refuses_bad_arguments_before_any_launch():
    from csplat import native
    size = lambda T, P: int(native.lib.csplat_flow_loss_scratch_bytes(T, P))  # noqa: E731
    grid = [[size(T, P) for P in (1, 256, 257, 100_000, 10_000_000)] for T in (2, 3, 16)]
    for row in grid:
        assert all(x > 0 for x in row) and row == sorted(row)
    for lo, hi in zip(grid, grid[1:]):
        assert all(x <= y for x, y in zip(lo, hi))
    assert grid[0][-1] < grid[-1][-1] and grid[0][0] <= grid[0][-1]
    # argument errors need no device: rc 2 and a message, nothing launched
    import ctypes as C
    two, one = (C.c_void_p * 2)(16, 16), (C.c_void_p * 1)(16)
    fwd = lambda T=2, P=4, w=W, h=H, pts_=two, full=two, flow=one, lam=1.0, cap=0.0, scratch=16, out=16, cnt=16: native.lib.csplat_flow_loss_fwd(  # noqa: E731
        None, T, P, w, h, pts_, full, flow, None, None, cap, lam, 1.0, None, 1.0, None, scratch, out, cnt)
    for kw in (dict(T=1), dict(T=17), dict(P=0), dict(w=0), dict(h=0), dict(lam=-1.0), dict(cap=NAN), dict(pts_=None), dict(full=None),
               dict(flow=None), dict(out=None), dict(cnt=None), dict(scratch=None), dict(pts_=(C.c_void_p * 2)(16, 0)),
               dict(flow=(C.c_void_p * 1)(18)), dict(P=2 ** 31)):
        assert fwd(**kw) == 2, kw
        assert b"csplat_flow_loss_fwd" in native.lib.csplat_last_error()
    bwd = lambda T=2, P=4, unit=16, lam=1.0, g=16, d=16: native.lib.csplat_flow_loss_bwd(None, T, P, unit, lam, 1.0, g, d)  # noqa: E731
    for kw in (dict(T=1), dict(T=17), dict(P=0), dict(lam=-1.0), dict(unit=None), dict(g=None), dict(d=None), dict(d=18), dict(P=2 ** 31)):
        assert bwd(**kw) == 2, kw
