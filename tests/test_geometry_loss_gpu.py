"""The geometry-loss kernels (csplat_geom_loss_fwd / _bwd through csplat.train.geometry_losses) and the train step's depth and
silhouette terms on the GPU, against the float64 restatement of tests/geometry_loss_ref.py.

Bars, by the rule of tests/test_train_kernels_gpu.py (its check() is used): the same restatement evaluated in float32 on the CPU has an
error e32 against float64 on the same inputs; the kernel must stay within 8 x e32, with a floor of 1e-6.  Errors are relative to
max |ref| or to a unit that does not vanish: max(lambda_depth, lambda_silhouette) for the loss values,
|g weight| max(lambda_depth max(1, max valid Z), lambda_silhouette) / n for the gradient images.  Sign bytes, the gradients of pixels of
weight zero, the all-invalid case, the forward-only form and a repeated call are compared for EQUALITY.

Shapes (V, H, W): 1 pixel; H W not a multiple of 4, as separate tensors and as 4-byte-aligned views of one batch; one workgroup (256
pixels on the elementwise path, 1024 on the 16-byte path) and one element beyond; 17 views (one beyond the kernel's 16-entry pointer
table: a second launch); and one view that needs more than the 1024 workgroups a view gets on either path (1029 / 1025: the kernels then
stride).  The second launch walks ANY number of partials with its 256 threads -- there is no size at which it runs out of threads.

What the table showed on an MI355X when this file was written (largest e32 / bar / kernel error of a group): every group of loss values
sits at e32 0 .. 9e-8, i.e. at the floor of 1e-6, with kernel errors of 0 .. 1.7e-7 (closest to its bar: silhouette only, bar / error
6.0); the gradient images at e32 7e-8 .. 1.5e-7, bars 1.0e-6 .. 1.2e-6, kernel errors 6e-8 .. 1.6e-7 (closest: mask_frac at
1025 x 1024, 7.5).  M all zero: e32, error 0.  The train step's terms: values 6.3e-10 / 1.0e-6 / 6.3e-10, gradients 6.9e-8 / 1.0e-6 /
1.0e-7.  Wall time of the 228 tests: 6 s."""
import ctypes as C
from types import SimpleNamespace

import pytest

import util  # noqa: F401
import geometry_loss_ref as R
from test_train_kernels_gpu import TABLE, check  # (the project's rule for a bar, and the table its comparisons are entered into)

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
F64, F32 = torch.float64, torch.float32


@pytest.fixture(scope="module", autouse=True)
def _threads_and_table():
    """torch gets at most 16 host threads for the restatement; afterwards the table of this module's bars (pytest -rP shows it)"""
    old = torch.get_num_threads()
    torch.set_num_threads(min(16, old))
    yield
    torch.set_num_threads(old)
    print("\ngroup | comparisons | largest e32 | largest bar | largest kernel error | smallest bar / error")
    for g in sorted(k for k in TABLE if k.startswith(("geometry_loss", "train_step geometry"))):
        n, e32, bar, err, margin = TABLE[g]
        print(f"{g} | {n} | {e32:.2e} | {bar:.2e} | {err:.2e} | {margin:.1f}")


SMALL = [(1, 1, 1), (1, 1, 3), (2, 3, 5), (1, 1, 255), (1, 1, 256), (1, 1, 257), (1, 16, 65), (1, 32, 32), (1, 4, 257), (3, 64, 64), (17, 4, 4)]
LARGE = [(1, 513, 513), (1, 1025, 1024)]          # 1029 workgroups of 256 pixels / 1025 of 256 x 4 pixels: beyond the 1024 a view gets
VARIANTS = ["both", "depth", "silhouette", "mask", "mask_zero", "mask_frac", "z_holes", "ties", "a_eq_s", "add", "weight", "g", "batch_views",
            "offset_views"]


def make_case(shape, variant, seed=0):
    """float32 CPU inputs of one call: lists of V [1,H,W] images and the scalars"""
    V, H, W = shape
    gen = torch.Generator().manual_seed(1000 * seed + 7 * V + 13 * H + W)
    rnd = lambda lo=0.0, hi=1.0: [lo + (hi - lo) * torch.rand(1, H, W, generator=gen) for _ in range(V)]  # noqa: E731
    A = [a * (a > 0.2) for a in rnd()]                                  # (a fifth of the pixels: nothing blended)
    Z = rnd(0.5, 4.0)
    D = [a * (z + 0.3 * (n - 0.5)) for a, z, n in zip(A, Z, rnd())]
    S = [(s > 0.5).float() for s in rnd()]
    c = dict(shape=shape, D=D, A=A, Z=Z, S=S, M=None, lam_d=0.7, lam_s=0.3, add=None, weight=1.0, add_weight=1.0, g=1.0, layout="separate")
    if variant == "depth":
        c["lam_s"] = 0.0
    elif variant == "silhouette":
        c["lam_d"] = 0.0
    elif variant == "mask":
        c["M"] = [(m > 0.3).float() for m in rnd()]
    elif variant == "mask_zero":
        c["M"] = [torch.zeros(1, H, W) for _ in range(V)]
    elif variant == "mask_frac":
        c["M"] = [m * (m > 0.25) for m in rnd()]
    elif variant == "z_invalid":
        bad = torch.tensor([0.0, -1.0, float("nan"), float("inf"), -float("inf")])
        c["Z"] = [bad[torch.randint(0, 5, (1, H, W), generator=gen)] for _ in range(V)]
        c["lam_s"] = 0.0
    elif variant == "z_holes":
        bad = torch.tensor([0.0, -2.0, float("nan"), float("inf")])
        for v in range(V):
            hole = torch.rand(1, H, W, generator=gen) < 0.4
            c["Z"][v] = torch.where(hole, bad[torch.randint(0, 4, (1, H, W), generator=gen)], Z[v])
            # under a hole D may hold anything (A also feeds the silhouette term, so it stays finite here)
            c["D"][v] = torch.where(hole & (torch.rand(1, H, W, generator=gen) < 0.5), torch.tensor(float("nan")), D[v])
        c["M"] = [(m > 0.2).float() for m in rnd()]
        for v in range(V):      # under M = 0 both D and A may hold anything
            off = c["M"][v] == 0
            c["A"][v] = torch.where(off & (torch.rand(1, H, W, generator=gen) < 0.5), torch.tensor(float("inf")), A[v])
            c["D"][v] = torch.where(off & (torch.rand(1, H, W, generator=gen) < 0.5), torch.tensor(float("nan")), c["D"][v])
    elif variant == "ties":
        # D = A Z exactly, from small integers and quarters, on half of the pixels; D = A = 0 on a quarter of them
        qa = [torch.randint(0, 5, (1, H, W), generator=gen).float() / 4 for _ in range(V)]
        qz = [torch.randint(1, 4, (1, H, W), generator=gen).float() for _ in range(V)]
        tie = [torch.rand(1, H, W, generator=gen) < 0.5 for _ in range(V)]
        c["A"], c["Z"] = qa, qz
        c["D"] = [torch.where(t, a * z, d) for t, a, z, d in zip(tie, qa, qz, D)]
        c["D"] = [torch.where(a == 0, torch.zeros(()), d) for a, d in zip(qa, c["D"])]
    elif variant == "a_eq_s":
        c["S"] = [a.clone() for a in A]
    elif variant == "add":
        c["add"] = torch.tensor(0.4321)
        c["add_weight"] = 0.5
    elif variant == "weight":
        c["weight"] = 0.37
        c["add"] = torch.tensor(-1.25)
    elif variant == "g":
        c["g"] = -2.75
    elif variant == "batch_views":
        c["layout"] = "batch"          # every view a slice of one [V,1,H,W] batch: 4-byte aligned, 16-byte only when H W % 4 == 0
    elif variant == "offset_views":
        c["layout"] = "offset"         # every view starts one float behind a 16-byte boundary
    else:
        assert variant == "both", variant
    return c


def _to_gpu(views, layout, grad=False):
    if views is None:
        return None
    V = len(views)
    if layout == "batch":
        out = list(torch.stack(views).cuda().unbind(0))
    elif layout == "offset":
        n = views[0].numel()
        pad = (n + 4 + 3) // 4 * 4
        buf = torch.zeros(V * pad + 4, device="cuda")
        out = [buf[v * pad + 1:v * pad + 1 + n].view(views[0].shape).copy_(views[v]) for v in range(V)]
        assert all(t.data_ptr() % 16 == 4 for t in out)
    else:
        out = [t.cuda() for t in views]
    return [t.detach().requires_grad_(grad) for t in out]


def run_kernel(c, grad=True):
    """-> (total, L_depth, L_sil, dD [V,H,W] or None, dA [V,H,W] or None) from csplat.train.geometry_losses on the GPU"""
    from csplat import train as tr
    V, H, W = c["shape"]
    lay = c["layout"]
    D, A = _to_gpu(c["D"], lay, grad), _to_gpu(c["A"], lay, grad)
    add = None if c["add"] is None else c["add"].cuda()
    total, ld, ls = tr.geometry_losses(D if c["lam_d"] > 0 else None, A, _to_gpu(c["Z"], lay) if c["lam_d"] > 0 else None,
                                       _to_gpu(c["S"], lay) if c["lam_s"] > 0 else None, c["lam_d"], c["lam_s"],
                                       masks=_to_gpu(c["M"], lay), add=add, weight=c["weight"], add_weight=c["add_weight"])
    assert total.requires_grad == grad and not ld.requires_grad and not ls.requires_grad
    gD = gA = None
    if grad:
        total.backward(torch.tensor(c["g"], device="cuda"))
        gA = torch.stack([a.grad.reshape(H, W) for a in A])
        if c["lam_d"] > 0:
            gD = torch.stack([d.grad.reshape(H, W) for d in D])
        else:
            assert all(d.grad is None for d in D)
    return total.detach(), ld, ls, gD, gA


def restate(c, dtype):
    return R.geometry_loss(c["D"], c["A"], c["Z"], c["S"], c["M"], c["lam_d"], c["lam_s"], add=c["add"], weight=c["weight"],
                           add_weight=c["add_weight"], g=c["g"], dtype=dtype)


def units(c):
    V, H, W = c["shape"]
    z = torch.stack(c["Z"])
    ok = torch.isfinite(z) & (z > 0)
    zmax = float(z[ok].max()) if bool(ok.any()) else 0.0
    lam_d, lam_s = c["lam_d"], c["lam_s"]
    return max(lam_d, lam_s), abs(c["g"] * c["weight"]) * max(lam_d * max(1.0, zmax), lam_s) / (V * H * W)


def compare(group, c, got):
    """loss values and gradient images under the bar; zero-weight pixels exactly zero"""
    total, ld, ls, gD, gA = got
    r64, r32 = restate(c, F64), restate(c, F32)
    u_loss, u_grad = units(c)
    what = f"{c['shape']}"
    check(group, what + " total", total, r64[0], r32[0], u_loss)
    check(group, what + " L_depth", ld, r64[1], r32[1], u_loss)
    check(group, what + " L_sil", ls, r64[2], r32[2], u_loss)
    if gA is not None:
        check(group + " grad", what + " dL/dA", gA, r64[4], r32[4], u_grad)
        t = R.terms(c["D"] if c["lam_d"] > 0 else None, c["A"], c["Z"] if c["lam_d"] > 0 else None, c["S"] if c["lam_s"] > 0 else None, c["M"])
        off_d = torch.ones_like(t["A"], dtype=torch.bool) if t["w_d"] is None else t["w_d"] == 0
        off_s = torch.ones_like(t["A"], dtype=torch.bool) if t["w_s"] is None else t["w_s"] == 0
        assert not gA.cpu()[off_d & off_s].any(), "a pixel of weight zero received an alpha gradient"
        if gD is not None:
            check(group + " grad", what + " dL/dD", gD, r64[3], r32[3], u_grad)
            assert not gD.cpu()[off_d].any(), "a pixel of weight zero received a depth gradient"


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("shape", SMALL, ids=str)
def test_kernels_against_restatement(shape, variant):
    c = make_case(shape, variant)
    compare("geometry_loss " + variant, c, run_kernel(c))


@pytest.mark.parametrize("shape", [(1, 255, 255), (1, 255, 257), (1, 59, 1111)], ids=str)
def test_finish_kernel_at_255_256_and_257_partials(shape):
    """one view, a pixel count that is no multiple of 4 (the elementwise path: a workgroup per 256 pixels): k_geom_loss_finish's 256 threads
    walk one partial short of a pass, a full pass, and one partial of a second pass"""
    V, H, W = shape
    assert V == 1 and (H * W) % 4 != 0 and -(-(H * W) // 256) == {255: 255, 257: 256, 1111: 257}[W]
    c = make_case(shape, "both")
    compare("geometry_loss both", c, run_kernel(c))


@pytest.mark.parametrize("variant", ["both", "mask_frac", "z_holes"])
@pytest.mark.parametrize("shape", LARGE, ids=str)
def test_kernels_beyond_the_workgroup_cap(shape, variant):
    """more pixels in one view than 1024 workgroups cover in one pass, on the elementwise path (513 x 513) and the 16-byte path"""
    c = make_case(shape, variant)
    compare("geometry_loss large " + variant, c, run_kernel(c))


@pytest.mark.parametrize("shape", [(1, 1, 1), (2, 3, 5), (1, 1, 257), (3, 64, 64), (17, 4, 4)], ids=str)
def test_all_invalid_depth_is_exactly_zero(shape):
    """Z entirely invalid (0, negative, NaN, +-Inf): the loss and both gradient images are exactly 0"""
    c = make_case(shape, "z_invalid")
    total, ld, ls, gD, gA = run_kernel(c)
    assert float(total) == 0.0 and float(ld) == 0.0 and float(ls) == 0.0
    assert not gD.any() and not gA.any()


def _raw_forward(c, want_signs=True):
    """csplat_geom_loss_fwd through the C-ABI: (out[3], sign bytes [V,H,W])"""
    from csplat import native as n
    V, H, W = c["shape"]
    lay = c["layout"]
    tabs = [_to_gpu(c[k], lay) for k in ("D", "A", "Z", "S", "M")]
    table = lambda ts: None if ts is None else (C.c_void_p * V)(*[t.data_ptr() for t in ts])  # noqa: E731
    out = torch.empty(3, device="cuda")
    sign = torch.full((V, H, W), 255, dtype=torch.uint8, device="cuda")
    scratch = torch.empty(int(n.lib.csplat_geom_loss_scratch_bytes(V, H * W)), dtype=torch.uint8, device="cuda")
    n.check(n.lib.csplat_geom_loss_fwd(n.stream_handle(torch.device("cuda:0")), V, H * W, *[table(t) for t in tabs], c["lam_d"], c["lam_s"],
                                       c["weight"], None, 1.0, n.ptr(sign) if want_signs else None, n.ptr(scratch), n.ptr(out)),
            "csplat_geom_loss_fwd")
    torch.cuda.synchronize()
    return out, sign


@pytest.mark.parametrize("variant", ["both", "mask_frac", "z_holes", "ties", "a_eq_s", "offset_views"])
@pytest.mark.parametrize("shape", [(1, 1, 3), (2, 3, 5), (1, 1, 257), (1, 16, 65), (3, 64, 64), (17, 4, 4)], ids=str)
def test_sign_bytes_equal_the_restatement(shape, variant):
    """the byte per pixel: the exact signs of D - A Z (one fused multiply-add) and of A - S, 0 where the weight is 0; with no gradient
    wanted nothing is stored and the loss bits are the same"""
    c = make_case(shape, variant)
    out, sign = _raw_forward(c)
    codes = restate(c, F64)[5]
    assert torch.equal(sign.cpu(), codes)
    if variant == "ties":
        tie_d = (codes & 3) == 1
        assert int(tie_d.sum()) >= codes.numel() // 4 or codes.numel() < 8        # the ties are there
    out2, untouched = _raw_forward(c, want_signs=False)
    assert torch.equal(out, out2) and bool((untouched == 255).all())


def test_nan_where_the_weight_is_not_zero():
    """a NaN in D or A at a pixel with w != 0 makes that term, and that pixel's gradient, NaN; every other pixel keeps its gradient"""
    c = make_case((1, 4, 5), "both")
    c["D"][0][0, 1, 2] = float("nan")
    total, ld, ls, gD, gA = run_kernel(c)
    assert bool(torch.isnan(ld)) and bool(torch.isfinite(ls)) and bool(torch.isnan(total))
    r64 = restate(c, F64)
    assert bool(torch.isnan(r64[1])) and bool(torch.isnan(r64[3][0, 1, 2]))
    assert bool(torch.isnan(gD[0, 1, 2])) and int(torch.isnan(gD).sum()) == 1 and int(torch.isnan(gA).sum()) == 1
    c["D"][0][0, 1, 2] = 0.0
    fin = torch.isfinite(gD.cpu())
    assert torch.equal(gD.cpu()[fin], run_kernel(c)[3].cpu()[fin])


@pytest.mark.parametrize("variant", ["both", "mask_frac", "add", "depth", "silhouette"])
@pytest.mark.parametrize("shape", [(2, 3, 5), (1, 16, 65), (3, 64, 64), (17, 4, 4)], ids=str)
def test_forward_only_and_repeated_calls_return_the_same_bits(shape, variant):
    c = make_case(shape, variant)
    a, b, f = run_kernel(c), run_kernel(c), run_kernel(c, grad=False)
    for x, y, z in zip(a[:3], b[:3], f[:3]):
        assert torch.equal(x, y) and torch.equal(x, z)
    assert torch.equal(a[4], b[4]) and (a[3] is None or torch.equal(a[3], b[3])) and f[3] is None and f[4] is None


def test_library_refuses_a_call_without_a_term():
    """both tables NULL, or both weights 0: an argument error, nothing is launched"""
    from csplat import native as n
    c = make_case((1, 4, 4), "both")
    for kw in (dict(lam_d=0.0, lam_s=0.0), dict(Z=None, S=None), dict(Z=None, lam_s=0.0)):
        with pytest.raises(n.CsplatError):
            _raw_forward({**c, **kw})


def test_other_forms_leave_the_hip_path_visibly():
    """float64 GPU tensors compose the formulas from torch operations: reported (raises under STRICT), same values when allowed"""
    from csplat import native as n
    from csplat import train as tr
    c = make_case((2, 3, 5), "mask_frac")
    args = lambda dt: ([t.cuda().to(dt).requires_grad_() for t in c["D"]], [t.cuda().to(dt).requires_grad_() for t in c["A"]],  # noqa: E731
                       [t.cuda().to(dt) for t in c["Z"]], [t.cuda().to(dt) for t in c["S"]], c["lam_d"], c["lam_s"])
    strict, n.STRICT = n.STRICT, True
    try:
        with pytest.raises(n.CsplatError):
            tr.geometry_losses(*args(F64), masks=[t.cuda().double() for t in c["M"]])
        with n.allow_fallbacks("dtype"):
            D, A, Z, S, ld_, ls_ = args(F64)
            total, ld, ls = tr.geometry_losses(D, A, Z, S, ld_, ls_, masks=[t.cuda().double() for t in c["M"]])
            total.backward()
    finally:
        n.STRICT = strict
    r64 = restate(c, F64)
    assert abs(float(total) - float(r64[0])) <= 1e-14 and abs(float(ld) - float(r64[1])) <= 1e-14 and abs(float(ls) - float(r64[2])) <= 1e-14
    assert float((torch.stack([a.grad[0] for a in A]).cpu() - r64[4]).abs().max()) <= 1e-15


# ---------------------------------------------------------------------------------------------------------------- the train step
TIMES = [0.2, 0.4, 0.6]


def _scene(P=2000, W=64, H=64, grid=12, scaling=0.0, seed=3):
    """bench_train's scene with three cameras; targets from the model itself: colour, Z = D / A where A > 0.5 (else 0: a hole) and
    S = (A > 0.5)"""
    import bench_train as bt
    from csplat import train as tr
    from csplat.optim import GroupedAdam
    from gaussian_renderer import render_views
    dev = torch.device("cuda:0")
    torch.manual_seed(seed)
    sc, pc, sim = bt.build(P=P, W=W, H=H, grid=grid, n_times=6, dev=dev)
    bg = torch.ones(3, device=dev)
    with torch.no_grad():
        if scaling:
            pc._scaling.add_(scaling)
        res, alphas = render_views(bt.cameras(sc, TIMES, dev), pc, sim, tr.DEFAULT_PIPE, bg, return_alpha=True)
        colour = [r.render.clamp(0, 1).clone() for r in res]
        depth = [torch.where(a > 0.5, r.depth / a.clamp_min(1e-6), torch.zeros_like(a)) for r, a in zip(res, alphas)]
        sil = [(a > 0.5).float() for a in alphas]
    plain = bt.cameras(sc, TIMES, dev, colour)
    rich = bt.cameras(sc, TIMES, dev, colour)
    for cam, z, s in zip(rich, depth, sil):
        cam.depth, cam.silhouette = z, s
    pc.training_setup(feature_lr=0.01)
    mopt = GroupedAdam(sim.parameters(), lr=3e-4)
    return SimpleNamespace(pc=pc, sim=sim, mopt=mopt, bg=bg, plain=plain, rich=rich, depth=depth, sil=sil)


def _opt(**kw):
    from csplat import train as tr
    return SimpleNamespace(**vars(tr.DEFAULT_OPT), **kw)


def test_train_step_loss_inputs_and_gradients(monkeypatch):
    """(a) both terms on: the depth and alpha images that enter the loss, the gradients that leave it (hooks) and the two stats agree
    with the restatement evaluated on those images.  The chain behind them is the rasterizer's, which has its own tests."""
    from csplat import train as tr
    s = _scene()
    with torch.no_grad():
        s.pc._opacity.sub_(1.0)       # (off the targets, so that the residuals are not all ties)
    seen = {}
    inner = tr.geometry_losses

    def spy(depths, alphas, gt_depths, silhouettes, lam_d, lam_s, masks=None, add=None, **kw):
        seen.update(D=[d.detach().clone() for d in depths], A=[a.detach().clone() for a in alphas], add=add.detach().clone(), kw=kw,
                    gD=[None] * len(depths), gA=[None] * len(alphas), masks=masks)
        for v, (d, a) in enumerate(zip(depths, alphas)):
            d.register_hook(lambda g, v=v: seen["gD"].__setitem__(v, g.detach().clone()))
            a.register_hook(lambda g, v=v: seen["gA"].__setitem__(v, g.detach().clone()))
        out = inner(depths, alphas, gt_depths, silhouettes, lam_d, lam_s, masks=masks, add=add, **kw)
        seen["total"] = out[0].detach().clone()
        return out

    monkeypatch.setattr(tr, "geometry_losses", spy)
    lam_d, lam_s = 0.2, 0.5
    _ps, loss, stats = tr.train_step(1, s.rich, s.pc, s.sim, s.mopt, opt=_opt(lambda_depth=lam_d, lambda_silhouette=lam_s), background=s.bg)
    assert seen and seen["masks"] is None and seen["kw"] == {} and all(g is not None for g in seen["gD"] + seen["gA"])
    c = dict(shape=(3, 64, 64), D=[d.cpu() for d in seen["D"]], A=[a.cpu() for a in seen["A"]], Z=[z.cpu() for z in s.depth],
             S=[x.cpu() for x in s.sil], M=None, lam_d=lam_d, lam_s=lam_s, add=seen["add"].cpu(), weight=1.0, add_weight=1.0, g=1.0)
    H = W = 64
    got = (seen["total"], stats["depth_loss"], stats["silhouette_loss"], torch.stack([g.reshape(H, W) for g in seen["gD"]]),
           torch.stack([g.reshape(H, W) for g in seen["gA"]]))
    assert not stats["depth_loss"].requires_grad and stats["depth_loss"].is_cuda and stats["silhouette_loss"].is_cuda
    assert float(stats["depth_loss"]) > 0 and float(stats["silhouette_loss"]) > 0 and bool(torch.isfinite(loss))
    compare("train_step geometry terms", c, got)
    # one term on: only its key (without the spy: no gradient reaches the depth images then, and their hooks would be handed None)
    monkeypatch.setattr(tr, "geometry_losses", inner)
    _ps, _l, st = tr.train_step(2, s.rich, s.pc, s.sim, s.mopt, opt=_opt(lambda_silhouette=lam_s), background=s.bg)
    assert "silhouette_loss" in st and "depth_loss" not in st


def _three_steps(cams_of, opt, captured=False, steps=3):
    from csplat import native, train as tr
    native.lib.csplat_debug_flags(256)          # the bit-reproducible K7: every kernel of the step sums in a fixed order
    try:
        s = _scene()
        log = []
        for it in range(1, steps + 1):
            ps, loss, stats = tr.train_step(it, cams_of(s), s.pc, s.sim, s.mopt, background=s.bg, captured=captured,
                                            **({} if opt is None else dict(opt=opt)))
            log.append((float(ps), float(loss), sorted(stats), {k: v.clone() for k, v in stats.items() if torch.is_tensor(v)}))
        torch.cuda.synchronize()
        params = [p.detach().clone() for p in list(s.pc.parameters()) + list(s.sim.parameters())]
        moments = []
        for o, ps_ in ((s.pc.optimizer, s.pc.parameters()), (s.mopt, s.sim.parameters())):
            for p in ps_:
                st = o.state.get(p)
                if st:
                    moments += [st["exp_avg"].clone(), st["exp_avg_sq"].clone()]
        return dict(log=log, params=params, moments=moments, cs=getattr(s.pc, "_captured_step", None))
    finally:
        native.lib.csplat_debug_flags(0)


def _assert_same_bits(a, b):
    assert len(a["log"]) == len(b["log"])
    for (pa, la, ka, ta), (pb, lb, kb, tb) in zip(a["log"], b["log"]):
        assert pa == pb and la == lb and ka == kb
        assert all(torch.equal(ta[k], tb[k]) for k in ta)
    assert len(a["params"]) == len(b["params"]) and len(a["moments"]) == len(b["moments"]) > 0
    assert all(torch.equal(x, y) for x, y in zip(a["params"], b["params"]))
    assert all(torch.equal(x, y) for x, y in zip(a["moments"], b["moments"]))


def test_train_step_unchanged_when_the_terms_are_off():
    """(b) cameras that carry depth and silhouette but weights 0, or absent, in the bit-reproducible mode: three steps leave every
    parameter, Adam moment, loss, PSNR and statistic bit-equal to the same steps with plain cameras; the stats keys are today's"""
    plain = _three_steps(lambda s: s.plain, None)
    absent = _three_steps(lambda s: s.rich, None)
    zero = _three_steps(lambda s: s.rich, _opt(lambda_depth=0.0, lambda_silhouette=0.0))
    assert plain["log"][0][2] == ["allreduce_ms", "radii", "viewspace_grad", "visibility_filter"]
    _assert_same_bits(plain, absent)
    _assert_same_bits(plain, zero)


def test_captured_step_with_a_term_runs_eagerly():
    """(c) captured=True with a term on: CapturedStep does not cover it, the step runs eagerly and returns the eager step's values"""
    opt = _opt(lambda_depth=0.2, lambda_silhouette=0.5)
    eager = _three_steps(lambda s: s.rich, opt, steps=2)
    cap = _three_steps(lambda s: s.rich, opt, captured=True, steps=2)
    assert cap["cs"] is not None and cap["cs"].stats["eager"] == 2 and cap["cs"].stats["recorded"] == 0 and cap["cs"].stats["replayed"] == 0
    assert "depth_loss" in eager["log"][0][2] and "silhouette_loss" in eager["log"][0][2]
    _assert_same_bits(eager, cap)


def test_train_step_descends_on_both_terms():
    """(d) on the pattern of test_train_step_converges_small_scene (P = 4000, 160 x 128, scaling + 0.9): targets from the unperturbed
    model, opacity logits lowered by 1.5, 40 steps with both terms on.  The condition: depth_loss and silhouette_loss each smaller at the
    last step than at the first, every parameter finite.  Ratios last / first seen on an MI355X: depth_loss 1.64e-3 -> 2.11e-4 (x 0.129), silhouette_loss 9.12e-3 -> 6.53e-3 (x 0.716)."""
    from csplat import train as tr
    s = _scene(P=4000, W=160, H=128, grid=16, scaling=0.9)
    with torch.no_grad():
        s.pc._opacity.sub_(1.5)
    opt = _opt(lambda_depth=0.2, lambda_silhouette=0.5)
    dl, sl = [], []
    for it in range(1, 41):
        _ps, _loss, stats = tr.train_step(it, s.rich, s.pc, s.sim, s.mopt, opt=opt, background=s.bg)
        dl.append(stats["depth_loss"])
        sl.append(stats["silhouette_loss"])
    dl, sl = [float(x) for x in dl], [float(x) for x in sl]
    print(f"depth_loss {dl[0]:.4e} -> {dl[-1]:.4e} (x {dl[-1] / dl[0]:.3f}); silhouette_loss {sl[0]:.4e} -> {sl[-1]:.4e} (x {sl[-1] / sl[0]:.3f})")
    assert all(bool(torch.isfinite(q).all()) for q in list(s.pc.parameters()) + list(s.sim.parameters()))
    assert dl[-1] < dl[0] and sl[-1] < sl[0], (dl[0], dl[-1], sl[0], sl[-1])
