"""The optical-flow kernels (csplat_flow_loss_fwd / _bwd through csplat.train.flow_losses) and the train step's flow term on the GPU,
against the float64 restatement of tests/flow_loss_ref.py.

Bars, by the rule of tests/test_train_kernels_gpu.py (its check() and TABLE are used): the same restatement evaluated in float32 on the
CPU has an error e32 against float64 on the same inputs; the kernel must stay within 8 x e32, with a floor of 1e-6.  Errors are relative
to max |ref| or to a unit that does not vanish: lambda * weight for the values, max |ref gradient| for the gradients.

Ties.  The term takes decisions -- the signs of r_x and r_y, the cell and the mask pixel p_a falls into, inside / outside, the cap -- and a
float32 evaluation may take a decision the other way when the float64 quantity sits within rounding of it.  The restatement returns each
pair's decision margin in pixels; pairs whose float64 margin is below tau = 64 * 2^-24 * max(W, H) pixels (64 float32 ulps of a pixel
coordinate) are EXCLUDED from the gradient comparison, together with the rows of the two frames they touch.  The test asserts that the
excluded share is at most 1 % of a case's pairs and that among the kept pairs the float32 restatement takes the float64 decisions.
L_flow is compared over all pairs with the same bar plus excluded * tau * max m / n.  The count must be equal once the excluded pairs are
removed from both sides: without exclusions it is compared as it is, with exclusions kernel and restatement are run once more with the
Gaussians of the excluded pairs made invisible, and count and L_flow are compared there.

Inputs (make_case): a pinhole full_proj with tan(fov / 2) = 0.5 per axis, per frame a 0.02 rad yaw and a 0.01 shift; points uniform in
x, y in [-1.2, 1.2], z in [2, 4], every 11th behind the camera, per-frame Gaussian motion of sigma 0.06; flows 3 N(0, 1) pixels with a
lattice of NaN pixels; 15 % invisible per frame; masks 20 % zeros, otherwise in [0.1, 1].

Shapes.  The kernel's launch constants are the wave (64) and the workgroup (256), one thread per (frame, Gaussian), no grid cap and no
stride: P = 1, 63, 64, 65, 255, 256, 257, 1000, 4099; T = 2, 3, 16 (1 and 17 are refused); images 1x1, 5x1, 1x5, 37x23, 64x48, 128x96.

What the table showed on an MI355X when this file was written (largest e32 / bar / kernel error of a group): the values sit at e32
1e-7 .. 5e-7, bars 1.0e-6 .. 4.2e-6, kernel errors 6e-8 .. 6e-7 (plain: 5.3e-7 / 4.2e-6 / 6.0e-7, closest to its bar at bar / error 3.9;
mask_cap 3.9e-7 / 3.1e-6 / 5.7e-7; thin images 1.1e-7 / 1.0e-6 / 5.5e-8); the gradients at e32 5.6e-6 .. 9.1e-6 of their maximum, bars
4.5e-5 .. 7.3e-5, kernel errors 5.6e-6 .. 9.1e-6 (plain: 9.1e-6 / 7.3e-5 / 9.1e-6; thin images 1.2e-7 / 1.0e-6 / 8.0e-8): the float32
projection through 1 / w, not the kernel, sets them.  mask all zero and all invisible: e32, error 0.  The train step's term: 3.8e-8 /
1.0e-6 / 3.8e-8.  At most 31 of 8198 pairs (0.38 %) were excluded in a case.  Descent: flow_loss 1.76 -> 0.057 in 40 steps.  Wall time
of the 114 tests: 7 s."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

import util  # noqa: F401
import flow_loss_ref as R
from test_train_kernels_gpu import FLOOR, K, TABLE, check  # (the project's rule for a bar, and the table its comparisons are entered into)

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
F64, F32 = torch.float64, torch.float32
NAN = float("nan")


@pytest.fixture(scope="module", autouse=True)
def _threads_and_table():
    """torch gets at most 16 host threads for the restatement; afterwards the table of this module's bars (pytest -rP shows it)"""
    old = torch.get_num_threads()
    torch.set_num_threads(min(16, old))
    yield
    torch.set_num_threads(old)
    print("\ngroup | comparisons | largest e32 | largest bar | largest kernel error | smallest bar / error")
    for g in sorted(k for k in TABLE if k.startswith(("flow_loss", "train_step flow"))):
        n, e32, bar, err, margin = TABLE[g]
        print(f"{g} | {n} | {e32:.2e} | {bar:.2e} | {err:.2e} | {margin:.1f}")


PS = [1, 63, 64, 65, 255, 256, 257, 1000, 4099]
IMAGES = [(1, 1), (5, 1), (1, 5), (37, 23), (64, 48), (128, 96)]          # (W, H)
VARIANTS = ["plain", "no_vis", "null_entry", "mask", "mask_zero", "cap", "mask_cap", "scaled", "stacked", "offset_flow", "all_invalid"]


def pinhole(t, W, H):
    """full_proj of frame t in the transposed convention (hom = [X, 1] @ full), float64: yaw 0.02 t, shift 0.01 t, tan(fov / 2) = 0.5"""
    a = 0.02 * t
    view = torch.eye(4, dtype=F64)
    view[0, 0], view[0, 2], view[2, 0], view[2, 2] = np.cos(a), -np.sin(a), np.sin(a), np.cos(a)
    view[3, :3] = torch.tensor([0.01 * t, -0.01 * t, 0.0], dtype=F64)
    proj = torch.zeros(4, 4, dtype=F64)
    proj[0, 0] = proj[1, 1] = 2.0
    proj[2, 2], proj[2, 3], proj[3, 2] = 1.0001, 1.0, -0.010001
    return view @ proj


def make_case(P, T, size, variant, seed=0):
    """float32 CPU inputs of one call"""
    W, H = size
    gen = torch.Generator().manual_seed(100003 * seed + 31 * P + 7 * T + 13 * W + H)
    x0 = torch.cat([2.4 * torch.rand(P, 2, generator=gen) - 1.2, 2.0 + 2.0 * torch.rand(P, 1, generator=gen)], 1)
    x0[::11, 2] *= -1.0                                                  # every 11th behind the camera
    X = [x0]
    for _ in range(T - 1):
        X.append(X[-1] + 0.06 * torch.randn(P, 3, generator=gen))
    flows = []
    for _ in range(T - 1):
        f = 3.0 * torch.randn(2, H, W, generator=gen)
        f[:, 2::5, 3::7] = NAN                                           # "no flow here"
        flows.append(f)
    vis = [((torch.rand(P, generator=gen) >= 0.15) * torch.randint(1, 10, (P,), generator=gen)).to(torch.int32) for _ in range(T)]
    masks = [torch.where(torch.rand(H, W, generator=gen) < 0.2, torch.zeros(()), 0.1 + 0.9 * torch.rand(H, W, generator=gen)) for _ in range(T - 1)]
    c = dict(P=P, T=T, W=W, H=H, X=X, full=[pinhole(t, W, H).float() for t in range(T)], flows=flows, vis=vis, masks=None, cap=None,
             lam=1.0, add=None, weight=1.0, add_weight=1.0, g=1.0, layout="separate", flow_layout="plain")
    if variant == "no_vis":
        c["vis"] = None
    elif variant == "null_entry":
        c["vis"][T // 2] = None
    elif variant == "mask":
        c["masks"] = masks
    elif variant == "mask_zero":
        c["masks"] = [torch.zeros(H, W) for _ in range(T - 1)]
    elif variant == "cap":
        c["cap"] = 6.0
    elif variant == "mask_cap":
        c["masks"], c["cap"] = masks, 6.0
    elif variant == "scaled":
        c.update(lam=0.7, add=torch.tensor(-1.25), weight=0.37, add_weight=0.5, g=-2.75)
    elif variant == "stacked":
        c["layout"] = "stacked"                                          # the frames' points are slices of one [T,P,3] buffer
    elif variant == "offset_flow":
        c["flow_layout"] = "offset"                                      # every flow image starts one float behind a 16-byte boundary
    elif variant == "all_invalid":
        c["vis"] = [torch.zeros(P, dtype=torch.int32) for _ in range(T)]
    else:
        assert variant == "plain", variant
    return c


def _flows_to_gpu(flows, layout):
    if layout == "plain":
        return [f.cuda() for f in flows]
    n = flows[0].numel()
    pad = (n + 4 + 3) // 4 * 4
    buf = torch.zeros(len(flows) * pad + 4, device="cuda")
    out = [buf[k * pad + 1:k * pad + 1 + n].view(flows[0].shape).copy_(f) for k, f in enumerate(flows)]
    assert all(t.data_ptr() % 16 == 4 for t in out)
    return out


def run_kernel(c, grad=True, vis=False):
    """-> SimpleNamespace(total, L, count, grad [T,P,3] or None) from csplat.train.flow_losses on the GPU; vis: another visibility table"""
    from csplat import train as tr
    T, P = c["T"], c["P"]
    if c["layout"] == "stacked":
        leaf = torch.stack(c["X"]).cuda().requires_grad_(grad)
        X = list(leaf.unbind(0))
    else:
        X = [x.cuda().requires_grad_(grad) for x in c["X"]]
    table = c["vis"] if vis is False else vis
    total, lf, nv = tr.flow_losses(X, [f.cuda() for f in c["full"]], _flows_to_gpu(c["flows"], c["flow_layout"]), (c["H"], c["W"]),
                                   visible=None if table is None else [None if v is None else v.cuda() for v in table],
                                   masks=None if c["masks"] is None else [m.cuda() for m in c["masks"]], lambda_flow=c["lam"],
                                   max_error=c["cap"], add=None if c["add"] is None else c["add"].cuda(), weight=c["weight"],
                                   add_weight=c["add_weight"])
    assert total.requires_grad == grad and not lf.requires_grad and nv.dtype == torch.int32 and total.is_cuda and nv.is_cuda
    g = None
    if grad:
        total.backward(torch.tensor(c["g"], device="cuda"))
        g = leaf.grad if c["layout"] == "stacked" else torch.stack([x.grad for x in X])
        assert g.shape == (T, P, 3)
    return SimpleNamespace(total=total.detach(), L=lf, count=int(nv), grad=g)


def restate(c, dtype, vis=False, want_grad=True):
    return R.flow_loss(c["X"], c["full"], c["flows"], c["W"], c["H"], visible=c["vis"] if vis is False else vis, masks=c["masks"],
                       max_error=c["cap"], lam=c["lam"], add=c["add"], weight=c["weight"], add_weight=c["add_weight"], g=c["g"], dtype=dtype,
                       want_grad=want_grad)


def check_value(group, what, got, r64, r32, unit, slack):
    """check() for one value with an absolute allowance on top of the bar (the excluded pairs' share of L_flow)"""
    got, r64, r32 = float(got), float(r64), float(r32)
    scale = max(abs(r64), float(unit))
    e32 = abs(r32 - r64) / scale
    bar = max(K * e32, FLOOR)
    err = abs(got - r64) / scale
    print(f"{group} | {what}: e32 {e32:.3e} bar {bar:.3e} (+ {slack / scale:.3e} for excluded pairs) kernel {err:.3e}")
    n, a, b, c_, m = TABLE.get(group, (0, 0.0, 0.0, 0.0, float("inf")))
    TABLE[group] = (n + 1, max(a, e32), max(b, bar), max(c_, err), min(m, (bar + slack / scale) / max(err, 1e-30)))
    assert err <= bar + slack / scale, f"{group} {what}: kernel error {err:.3e} > bar {bar:.3e} + {slack / scale:.3e} (float32 restatement: {e32:.3e})"


def compare(group, c, got, ties=True):
    """ties=False: the case sits on decisions by construction and takes them exactly (no pair is excluded)"""
    T, P, W, H = c["T"], c["P"], c["W"], c["H"]
    what = f"P {P} T {T} {W}x{H}"
    r64, r32 = restate(c, F64), restate(c, F32)
    n = (T - 1) * P
    tau = 64.0 * 2.0 ** -24 * max(W, H) if ties else 0.0
    excl = r64["margin"] < tau                                          # [T-1,P]
    n_excl = int(excl.sum())
    assert n_excl <= 0.01 * n, f"{what}: {n_excl} of {n} pairs within {tau:.2e} px of a decision"
    assert torch.equal(r32["valid"][~excl], r64["valid"][~excl]), f"{what}: the float32 restatement decides a kept pair the other way"
    assert torch.equal(r32["m"][~excl].double(), r64["m"].float().double()[~excl]), f"{what}: the float32 restatement reads another mask pixel"
    unit = c["lam"] * c["weight"]
    m_max = float(r64["m"].max()) if r64["m"].numel() else 1.0
    slack_l = n_excl * tau * m_max / n
    check_value(group, what + " L_flow", got.L, r64["L"], r32["L"], 1.0, slack_l)
    check_value(group, what + " total", got.total, r64["total"], r32["total"], unit, unit * slack_l)
    if n_excl == 0:
        assert got.count == r64["count"], (what, got.count, r64["count"])
    else:
        # the Gaussians of the excluded pairs made invisible on both sides: the counts must be equal
        gone = excl.any(dim=0)
        table = [(torch.ones(P, dtype=torch.int32) if (c["vis"] is None or c["vis"][t] is None) else c["vis"][t].clone()) for t in range(T)]
        for v in table:
            v[gone] = 0
        k2, q64, q32 = run_kernel(c, grad=False, vis=table), restate(c, F64, vis=table, want_grad=False), restate(c, F32, vis=table, want_grad=False)
        assert q64["count"] == q32["count"] and k2.count == q64["count"], (what, k2.count, q64["count"], q32["count"])
        check(group, what + " L_flow without the excluded", k2.L, q64["L"], q32["L"], 1.0)
    if got.grad is not None:
        rows = torch.ones(T, P, dtype=torch.bool)                       # rows of frames no excluded pair touches
        rows[:-1] &= ~excl
        rows[1:] &= ~excl
        u_grad = float(r64["grad"].abs().max())
        g = got.grad.cpu()
        dead = torch.ones(T, P, dtype=torch.bool)                       # rows whose pairs are all invalid
        dead[:-1] &= ~r64["valid"]
        dead[1:] &= ~r64["valid"]
        assert not g[dead & rows].any(), f"{what}: an invalid pair received a gradient"
        if u_grad == 0.0:
            assert not g[rows].any(), what
        elif bool(rows.any()):
            check(group + " grad", what + " dL/dX", g[rows], r64["grad"][rows], r32["grad"][rows], u_grad)


# P at every launch constant with a middle-sized image; every image with two P; T = 16 and T = 2
SHAPES = [(P, 3, (64, 48)) for P in PS] + [(P, 3, size) for size in IMAGES for P in (65, 1000) if size != (64, 48)] + \
         [(P, 2, (37, 23)) for P in (1, 257)] + [(P, 16, (37, 23)) for P in (1, 65, 257)] + [(4099, 3, (128, 96)), (4099, 2, (128, 96))]


@pytest.mark.parametrize("variant", ["plain", "mask_cap"])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_kernels_against_restatement_every_shape(shape, variant):
    c = make_case(*shape, variant)
    compare("flow_loss " + variant, c, run_kernel(c))


# k_flow_loss_finish: 256 threads walk T * ceil(P / 256) partials.  One short of a full pass, a full pass, and a second pass of two
# (257 is prime and T >= 2: 258 = 6 * 43 is the first count beyond 256 that frames x workgroups reach)
FINISH_SHAPES = [(4099, 15, (37, 23)), (4096, 16, (37, 23)), (10753, 6, (37, 23))]


@pytest.mark.parametrize("shape", FINISH_SHAPES, ids=str)
def test_finish_kernel_at_255_256_and_258_partials(shape):
    P, T, _ = shape
    assert T * -(-P // 256) == {4099: 255, 4096: 256, 10753: 258}[P]
    c = make_case(*shape, "plain")
    compare("flow_loss plain", c, run_kernel(c))


@pytest.mark.parametrize("variant", [v for v in VARIANTS if v not in ("plain", "mask_cap")])
@pytest.mark.parametrize("shape", [(1, 2, (37, 23)), (257, 3, (37, 23)), (65, 16, (64, 48)), (4099, 3, (128, 96))], ids=str)
def test_kernels_against_restatement_every_variant(shape, variant):
    c = make_case(*shape, variant)
    got = run_kernel(c)
    compare("flow_loss " + variant, c, got)
    if variant in ("mask_zero", "all_invalid"):
        assert got.count == 0 and float(got.L) == 0.0 and float(got.total) == 0.0 and not got.grad.any()


@pytest.mark.parametrize("size", [(1, 1), (5, 1), (1, 5)], ids=str)
def test_thin_images_with_the_points_on_them(size):
    """the pinhole cases leave nothing valid on a 1-pixel-wide image; here an orthographic camera (pixel = (X, Y), exactly so where the
    size is 1) puts every point ON it: y = 0 exactly on a 5 x 1 image is inside (inclusive edges), both taps of that axis are the one
    pixel and J_g has no entry along it"""
    W, H = size
    P, T = 65, 3
    gen = torch.Generator().manual_seed(17 + W + 3 * H)
    X = [torch.cat([(W - 1) * torch.rand(P, 1, generator=gen), (H - 1) * torch.rand(P, 1, generator=gen), torch.zeros(P, 1)], 1) for _ in range(T)]
    c = make_case(P, T, size, "mask")
    c.update(X=X, full=[R.ortho_full(W, H).float() for _ in range(T)], vis=None)
    c["flows"] = [0.5 * torch.randn(2, H, W, generator=gen) for _ in range(T - 1)]
    c["masks"] = [0.1 + 0.9 * torch.rand(H, W, generator=gen) for _ in range(T - 1)]
    got = run_kernel(c)
    assert got.count == (T - 1) * P
    compare("flow_loss thin images", c, got, ties=False)


@pytest.mark.parametrize("variant", ["plain", "mask_cap", "scaled", "stacked"])
@pytest.mark.parametrize("shape", [(1, 2, (37, 23)), (257, 3, (37, 23)), (65, 16, (64, 48)), (4099, 3, (128, 96))], ids=str)
def test_forward_only_and_repeated_calls_return_the_same_bits(shape, variant):
    c = make_case(*shape, variant)
    a, b, f = run_kernel(c), run_kernel(c), run_kernel(c, grad=False)
    for x in (b, f):
        assert torch.equal(a.total, x.total) and torch.equal(a.L, x.L) and a.count == x.count
    assert torch.equal(a.grad, b.grad) and f.grad is None


def test_points_and_flows_that_are_not_numbers_under_invalid_pairs():
    """NaN / Inf points and flow pixels: their pairs are selected out, every other pair keeps its value and gradient bit for bit"""
    c = make_case(257, 3, (37, 23), "mask_cap")
    base = run_kernel(c)
    r64 = restate(c, F64)
    d = {**c, "X": [x.clone() for x in c["X"]], "flows": [f.clone() for f in c["flows"]]}
    dead = ~r64["valid"][0] & ~r64["valid"][1] & (r64["margin"] == float("inf")).all(dim=0)       # Gaussians no pair of which is valid
    assert int(dead.sum()) >= 20
    ids = dead.nonzero().flatten()
    d["X"][0][ids[0::3], 0] = NAN
    d["X"][1][ids[1::3], 2] = float("inf")
    d["X"][2][ids[2::3], 1] = -float("inf")
    got = run_kernel(d)
    assert got.count == base.count and torch.equal(got.L, base.L) and torch.equal(got.total, base.total)
    assert torch.equal(got.grad, base.grad) and not got.grad[:, ids].any()
    compare("flow_loss not numbers", d, got)


def _raw(c, **kw):
    """csplat_flow_loss_fwd through the C-ABI with overrides -> the return code"""
    from csplat import native as n
    T, P = c["T"], c["P"]
    X, full, F = [x.cuda() for x in c["X"]], [f.cuda() for f in c["full"]], [f.cuda() for f in c["flows"]]
    tab = lambda ts: (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])  # noqa: E731
    out, cnt = torch.zeros(2, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
    scratch = torch.empty(int(n.lib.csplat_flow_loss_scratch_bytes(T, P)), dtype=torch.uint8, device="cuda")
    a = dict(T=T, P=P, W=c["W"], H=c["H"], X=tab(X), full=tab(full), F=tab(F), lam=1.0)
    a.update(kw)
    rc = n.lib.csplat_flow_loss_fwd(n.stream_handle(torch.device("cuda:0")), a["T"], a["P"], a["W"], a["H"], a["X"], a["full"], a["F"], None, None,
                                    0.0, a["lam"], 1.0, None, 1.0, None, n.ptr(scratch), n.ptr(out), n.ptr(cnt))
    torch.cuda.synchronize()
    return rc, out, cnt, (X, full, F)


def test_library_refuses_bad_arguments_and_flow_losses_refuses_the_frame_counts():
    from csplat import train as tr
    c = make_case(65, 3, (37, 23), "plain")
    rc, out, cnt, _ = _raw(c)
    assert rc == 0 and int(cnt) == restate({**c, "vis": None}, F64, want_grad=False)["count"]
    for kw in (dict(T=1), dict(T=17), dict(P=0), dict(W=0), dict(H=0), dict(lam=-1.0), dict(X=None), dict(full=None), dict(F=None)):
        assert _raw(c, **kw)[0] == 2, kw
    X = [x.cuda() for x in c["X"]]
    for T in (1, 17):
        with pytest.raises(ValueError, match="frames"):
            tr.flow_losses([X[0]] * T, [c["full"][0].cuda()] * T, [c["flows"][0].cuda()] * max(T - 1, 0), (c["H"], c["W"]))


def test_other_forms_leave_the_hip_path_visibly():
    """float64 GPU tensors and a non-contiguous flow compose the formulas from torch operations: reported (raises under STRICT), same
    values when allowed"""
    from csplat import native as n
    from csplat import train as tr
    c = make_case(65, 3, (37, 23), "mask_cap")
    r64 = restate(c, F64)

    def call(dt, strided=False):
        X = [x.cuda().to(dt).requires_grad_() for x in c["X"]]
        flows = [f.cuda().to(dt) for f in c["flows"]]
        if strided:
            flows = [torch.stack([f, f], -1)[..., 0] for f in flows]
            assert not flows[0].is_contiguous()
        out = tr.flow_losses(X, [f.cuda().to(dt) for f in c["full"]], flows, (c["H"], c["W"]), visible=[v.cuda() for v in c["vis"]],
                             masks=[m.cuda().to(dt) for m in c["masks"]], max_error=c["cap"])
        return X, out

    strict, n.STRICT = n.STRICT, True
    try:
        with pytest.raises(n.CsplatError):
            call(F64)
        with pytest.raises(n.CsplatError):
            call(F32, strided=True)
        with n.allow_fallbacks("dtype"):
            X, (total, lf, nv) = call(F64)
            total.backward()
    finally:
        n.STRICT = strict
    assert int(nv) == r64["count"] and abs(float(lf) - float(r64["L"])) <= 1e-12
    assert float((torch.stack([x.grad for x in X]).cpu() - r64["grad"]).abs().max()) <= 1e-12


# ---------------------------------------------------------------------------------------------------------------- the train step
from test_geometry_loss_gpu import _assert_same_bits, _opt, _scene, _three_steps  # noqa: E402  (the small synthetic scene of that file)


def _flow_cams(s, flows=None, seed=11):
    """the scene's plain cameras, each carrying a flow image (kept on the scene: the same objects every step)"""
    if getattr(s, "flow_cams", None) is None:
        gen = torch.Generator().manual_seed(seed)
        H, W = int(s.plain[0].image_height), int(s.plain[0].image_width)
        s.flow_cams = []
        for k, cam in enumerate(s.plain):
            f = (1.5 * torch.randn(2, H, W, generator=gen)).cuda() if flows is None else flows[k]
            s.flow_cams.append(SimpleNamespace(**vars(cam), flow=f, view_id=0))
    return s.flow_cams


def test_train_step_loss_and_gradients_equal_flow_losses_on_the_same_records(monkeypatch):
    """(a) the term on: what the step hands to flow_losses, the gradients that reach the views' means3D_deform (hooks) and the two stats
    equal flow_losses called on clones of the same records, bit for bit, and the restatement within the bar"""
    from csplat import train as tr
    s = _scene()
    cams = _flow_cams(s)
    seen = {}
    inner = tr.flow_losses

    def spy(points, full_projs, flows, image_size, **kw):
        # the views' centres also feed the rasterizer: the term is handed aliases, so that the hooks see the term's gradient alone
        alias = [p.view(p.shape) for p in points]
        seen.update(X=[p.detach().clone() for p in points], full=[f.detach().clone() for f in full_projs], flows=list(flows), size=image_size,
                    vis=[v.clone() for v in kw["visible"]], kw=kw, add=kw["add"].detach().clone(), g=[None] * len(points))
        for t, p in enumerate(alias):
            p.register_hook(lambda g, t=t: seen["g"].__setitem__(t, g.detach().clone()))
        out = inner(alias, full_projs, flows, image_size, **kw)
        seen["out"] = [o.detach().clone() for o in out]
        return out

    monkeypatch.setattr(tr, "flow_losses", spy)
    lam = 0.05
    _ps, loss, stats = tr.train_step(1, cams, s.pc, s.sim, s.mopt, opt=_opt(lambda_flow=lam, flow_max_error=20.0), background=s.bg)
    assert seen and seen["kw"]["masks"] is None and seen["kw"]["lambda_flow"] == lam and seen["kw"]["max_error"] == 20.0
    assert seen["size"] == (64, 64) and len(seen["flows"]) == 2 and all(f.data_ptr() == c.flow.data_ptr() for f, c in zip(seen["flows"], cams))
    assert all(g is not None for g in seen["g"]) and bool(torch.isfinite(loss))
    assert torch.equal(stats["flow_loss"], seen["out"][1]) and torch.equal(stats["flow_valid"], seen["out"][2])
    assert not stats["flow_loss"].requires_grad and stats["flow_loss"].is_cuda and stats["flow_valid"].dtype == torch.int32
    assert int(stats["flow_valid"]) > 0 and float(stats["flow_loss"]) > 0
    monkeypatch.setattr(tr, "flow_losses", inner)
    X = [x.clone().requires_grad_() for x in seen["X"]]
    total, lf, nv = inner(X, seen["full"], seen["flows"], seen["size"], visible=seen["vis"], lambda_flow=lam, max_error=20.0, add=seen["add"])
    total.backward()
    assert torch.equal(total.detach(), seen["out"][0]) and torch.equal(lf, seen["out"][1]) and torch.equal(nv, seen["out"][2])
    assert all(torch.equal(g, x.grad) for g, x in zip(seen["g"], X))
    c = dict(P=X[0].shape[0], T=3, W=64, H=64, X=[x.cpu() for x in seen["X"]], full=[f.cpu() for f in seen["full"]],
             flows=[f.cpu() for f in seen["flows"]], vis=[v.cpu() for v in seen["vis"]], masks=None, cap=20.0, lam=lam, add=seen["add"].cpu(),
             weight=1.0, add_weight=1.0, g=1.0, layout="separate", flow_layout="plain")
    compare("train_step flow term", c, SimpleNamespace(total=total.detach(), L=lf, count=int(nv), grad=torch.stack([x.grad for x in X])))


def test_train_step_unchanged_when_the_term_is_off():
    """(b) cameras that carry `flow` but lambda_flow 0, or absent, in the bit-reproducible mode: three steps leave every parameter, Adam
    moment, loss, PSNR and statistic bit-equal to the same steps with plain cameras; the stats keys are today's"""
    plain = _three_steps(lambda s: s.plain, None)
    absent = _three_steps(_flow_cams, None)
    zero = _three_steps(_flow_cams, _opt(lambda_flow=0.0, flow_max_error=5.0))
    assert plain["log"][0][2] == ["allreduce_ms", "radii", "viewspace_grad", "visibility_filter"]
    _assert_same_bits(plain, absent)
    _assert_same_bits(plain, zero)


def test_captured_step_with_the_term_runs_eagerly():
    """(c) captured=True with the term on: CapturedStep does not cover it, the step runs eagerly and returns the eager step's values"""
    opt = _opt(lambda_flow=0.05)
    eager = _three_steps(_flow_cams, opt, steps=2)
    cap = _three_steps(_flow_cams, opt, captured=True, steps=2)
    assert cap["cs"] is not None and cap["cs"].stats["eager"] == 2 and cap["cs"].stats["recorded"] == 0 and cap["cs"].stats["replayed"] == 0
    assert "flow_loss" in eager["log"][0][2] and "flow_valid" in eager["log"][0][2]
    _assert_same_bits(eager, cap)


def _teacher_flows(s, teacher, cams):
    """flow images of the displaced model: per pair the Gaussians' projected displacement p_{t+1} - p_t composited with frame t's
    blending weights (feature channels, INTEGRATION.md's recipe) and divided by alpha; NaN where less than half blends"""
    from csplat import train as tr
    from gaussian_renderer import GaussianRasterizer, _prepare, render
    with torch.no_grad():
        proj = [render(cam, s.pc, teacher, tr.DEFAULT_PIPE, s.bg).projections for cam in cams]
        flows = []
        for t in range(len(cams) - 1):
            settings, kwargs, _ = _prepare(cams[t], s.pc, teacher, tr.DEFAULT_PIPE, s.bg, 1.0, None, None, False)
            out = GaussianRasterizer(raster_settings=settings)(**kwargs, features=(proj[t + 1] - proj[t]).float().contiguous(), return_alpha=True)
            feat, alpha = out[3], out[4]
            flows.append(torch.where(alpha > 0.5, feat / alpha.clamp_min(1e-6), torch.full_like(feat, NAN)).contiguous())
    return flows


def test_train_step_descends_on_the_flow_term():
    """(d) teacher: a copy of the model whose mesh trajectory is displaced by 0.03 per frame along x; its flow images and colours are
    the targets.  The student starts from the undisplaced simulator; 40 steps with the term on.  The condition: flow_loss smaller at the
    last step than at the first, every parameter finite."""
    from csplat import train as tr
    from meshnet.meshnet_network import ResidualMeshSimulator
    s = _scene(P=4000, W=160, H=128, grid=16, scaling=0.9)
    dev = torch.device("cuda:0")
    with torch.no_grad():
        table = s.sim.mesh_predictions.clone()
        table[..., 0] += 0.03 * torch.arange(table.shape[0], device=dev, dtype=table.dtype)[:, None]
        torch.manual_seed(3)
        teacher = ResidualMeshSimulator(table, device=dev)
        colour = [tr.render(cam, s.pc, teacher, tr.DEFAULT_PIPE, s.bg).render.clamp(0, 1).clone() for cam in s.plain]
    cams = [SimpleNamespace(**{**vars(cam), "original_image": img}) for cam, img in zip(s.plain, colour)]
    flows = _teacher_flows(s, teacher, cams)
    assert all(bool(torch.isfinite(f).any()) for f in flows)
    for cam, f in zip(cams, flows):
        cam.flow = f
    opt = _opt(lambda_flow=0.05)
    fl = []
    for it in range(1, 41):
        _ps, _loss, stats = tr.train_step(it, cams, s.pc, s.sim, s.mopt, opt=opt, background=s.bg)
        fl.append(stats["flow_loss"])
    fl = [float(x) for x in fl]
    print(f"flow_loss {fl[0]:.4e} -> {fl[-1]:.4e} (x {fl[-1] / fl[0]:.3f}); valid pairs at the last step {int(stats['flow_valid'])}")
    assert all(bool(torch.isfinite(q).all()) for q in list(s.pc.parameters()) + list(s.sim.parameters()))
    assert fl[0] > 0 and fl[-1] < fl[0], (fl[0], fl[-1])
