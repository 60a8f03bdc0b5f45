"""The kernels that run around the rasterizer in every training step -- the image losses of csrc/csplat_image.hip (k_l1, k_ssim_*,
k_image_loss_*, k_blur11, k_psnr) and the optimizer, store and bookkeeping kernels of csrc/csplat_optim.hip (k_adam, k_adam_dev,
csplat_mask_to_map, k_rows_scatter, k_gauss_act_*, k_step_stats, k_gather_words) -- against the float64 restatement
tests/train_kernels_ref.py, at the sizes a real scene has (each one beyond a launch cap: tests/test_train_kernels_cpu.py states which)
and at the launch edges (tile and window edges, 16-byte alignment, table lengths).

Bars, by the rule of tests/test_mesh_transform_gpu.py.  The same restatement evaluated in float32 on the CPU has an error e32 against
float64 on the same inputs; the kernel must stay within K = 8 x max(e32), with a floor of 1e-6.  An error is max |got - ref| over ALL
elements divided by the larger of max |ref| and a unit that does not vanish, stated at each call of check():
  gradient images   |upstream| / N, the size of one L1 gradient element (the float64 SSIM gradient of equal images is ~1e-20);
  the loss values   the weight of the term `lambda * 1` the SSIM loss 1 - mean(SSIM) is formed from (it cancels to ~0 on good images);
  SSIM means        1 (a mean of values bounded by 1: its error is the pixels' absolute error);
  Adam              per tensor: lr for the update, max |g| and max |g|^2 for the moments.
Integer outputs, bit copies and saturated activations are compared for equality.  check() prints e32, the bar and the kernel's error;
the module's last teardown prints the table of the largest of each per group (pytest -rP shows it).

What that table showed on an MI355X when this file was written (largest e32 / bar / kernel error of the group): most groups sit at
e32 1e-8 .. 6e-7, i.e. bars of 1e-6 .. 5e-6 and kernel errors of the size of e32.  Float32 itself loses digits on real-looking images:
  d/dx saturated 5.6e-5 / 4.5e-4 / 1.0e-4      d/dx quantised 2.2e-5 / 1.8e-4 / 2.3e-5      value quantised 1.6e-5 / 1.3e-4 / 1.6e-5
against d/dx uniform 6.3e-7 / 5.0e-6 / 6.4e-7 -- a fixed 1e-5 says nothing about such an image.  Closest to its bar: d/dx saturated at
[4,3,800,800] (bar / error 3.9).  Wall time 29 s for the 113 tests (tests/test_train_gpu.py: 8 s): the restatement is already two
in-place 11-tap passes with a self-adjoint backward, no test takes 2 s, and the rest is the number of cases."""
import ctypes as C

import numpy as np
import pytest

import util  # noqa: F401
import train_kernels_ref as R

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

K, FLOOR = 8.0, 1e-6
F64, F32 = torch.float64, torch.float32
TABLE = {}


@pytest.fixture(scope="module", autouse=True)
def _threads_and_table():
    """the restatement dominates the wall time: torch gets at most 16 host threads; afterwards the table of the bars"""
    old = torch.get_num_threads()
    torch.set_num_threads(min(16, old))
    yield
    torch.set_num_threads(old)
    print("\ngroup | comparisons | largest e32 | largest bar | largest kernel error | smallest bar / error")
    for g in sorted(TABLE):
        n, e32, bar, err, margin = TABLE[g]
        print(f"{g} | {n} | {e32:.2e} | {bar:.2e} | {err:.2e} | {margin:.1f}")


def _np(t):
    return t.detach().cpu().double().numpy() if torch.is_tensor(t) else np.asarray(t, np.float64)


def check(group, what, got, r64, r32, unit):
    """got (the kernel), r64, r32 (the restatement in float64 / float32): every element, relative to max(max |r64|, unit); where r64 is
    not finite (the PSNR of equal images) the three must be EQUAL there"""
    got, r64, r32 = _np(got), _np(r64), _np(r32)
    assert got.shape == r64.shape == r32.shape, (group, what, got.shape, r64.shape)
    fin = np.isfinite(r64)
    if not fin.all():
        np.testing.assert_array_equal(got[~fin], r64[~fin], err_msg=f"{group} {what}: non-finite reference values")
        got, r64, r32 = got[fin], r64[fin], r32[fin]
        if got.size == 0:
            return
    scale = max(float(np.abs(r64).max()), float(unit))
    e32 = float(np.abs(r32 - r64).max()) / scale
    bar = max(K * e32, FLOOR)
    err = float(np.abs(got - r64).max()) / scale
    print(f"{group} | {what}: e32 {e32:.3e} bar {bar:.3e} kernel {err:.3e}")
    n, a, b, c, m = TABLE.get(group, (0, 0.0, 0.0, 0.0, float("inf")))
    TABLE[group] = (n + 1, max(a, e32), max(b, bar), max(c, err), min(m, bar / max(err, 1e-30)))
    assert err <= bar, f"{group} {what}: kernel error {err:.3e} > bar {bar:.3e} (float32 restatement: {e32:.3e}; scale {scale:.3e})"


def cuda(t, grad=False):
    return None if t is None else t.detach().cuda().requires_grad_(grad)


def leaf(t, dtype):
    """a fresh leaf holding t's values in `dtype` (never t itself: .to() of the same dtype returns its argument)"""
    return t.detach().to(dtype).clone().requires_grad_()


# ================================================================================================ image losses
LAM, W_IMG, W_ADD, PS, UP, ADD = 0.2, 2.0 / 3.0, 0.5, 1.0 / 3.0, 1.7, 0.37


def _ref_image_loss(x, y, mask, with_add, dtype):
    a = leaf(x, dtype)
    add = torch.tensor(ADD, dtype=dtype, requires_grad=True) if with_add else None
    out0, ps, il, _ = R.image_loss(a, y, LAM, mask, add, W_IMG, W_ADD if with_add else 1.0, PS, dtype=dtype)
    (UP * out0).backward()
    return dict(loss=out0.detach(), psnr=ps, il=il, dx=a.grad, dadd=(add.grad if with_add else None))


def _gpu_image_loss(x, y, mask, with_add, grad=True):
    from csplat import train as tr
    a, yc, mc = cuda(x, grad), cuda(y), cuda(mask)
    add = torch.tensor(ADD, device="cuda", requires_grad=grad) if with_add else None
    loss, ps, il = tr.FusedImageLoss.apply(a, yc, LAM, mc, add, W_IMG, W_ADD if with_add else 1.0, PS)
    out = dict(loss=loss.detach().clone(), psnr=ps.clone(), il=il.clone(), dx=None, dadd=None)
    if grad:
        assert type(loss.grad_fn).__name__.startswith("FusedImageLoss")
        (UP * loss).backward()
        out.update(dx=a.grad, dadd=(add.grad if with_add else None))
    return out


def _same_bits(a, b, keys):
    for k in keys:
        if a[k] is not None:
            assert torch.equal(a[k].view(torch.int32) if a[k].dtype == F32 else a[k], b[k].view(torch.int32) if b[k].dtype == F32 else b[k]), k


def image_loss_case(group, kind, shape, mc, with_add, seed=0):
    x, y, mask = R.image_case(kind, shape, mc, seed)
    got = _gpu_image_loss(x, y, mask, with_add)
    _same_bits(got, _gpu_image_loss(x, y, mask, with_add, grad=False), ("loss", "psnr", "il"))       # the no-grad path (no partials written)
    _same_bits(got, _gpu_image_loss(x, y, mask, with_add), ("loss", "psnr", "il", "dx", "dadd"))     # a second call: fixed summation order
    r64, r32 = (_ref_image_loss(x, y, mask, with_add, dt) for dt in (F64, F32))
    where = f"{kind} {tuple(shape)} mask {mc} add {with_add}"
    check(group, f"{where} loss", got["loss"], r64["loss"], r32["loss"], W_IMG * LAM)
    check(group, f"{where} image_loss", got["il"], r64["il"], r32["il"], LAM)
    check(group + " psnr", f"{where} psnr", got["psnr"], r64["psnr"], r32["psnr"], 1.0)
    check(group + " d/dx", f"{where} d/dx", got["dx"], r64["dx"], r32["dx"], UP * W_IMG / x.numel())
    if with_add:
        check(group, f"{where} d/dadd", got["dadd"], r64["dadd"], r32["dadd"], 1e-30)


@pytest.mark.parametrize("kind,shape,mc,with_add", R.IMAGE_LOSS_CASES)
def test_fused_image_loss_every_kind_of_image(kind, shape, mc, with_add):
    """csplat_image_loss_fwd / _bwd on the five kinds of image, small and at production size: value, image loss, PSNR, d/dx, d/d add"""
    image_loss_case(f"image_loss {kind}", kind, shape, mc, with_add)


def _ref_ssim(x, y, dtype):
    a = leaf(x, dtype)
    s = R.ssim(a, y, dtype)
    (UP * s).backward()
    return s.detach(), a.grad


def ssim_case(group, x, y):
    from csplat import train as tr
    a, yc = cuda(x, True), cuda(y)
    s = tr.ssim(a, yc)
    assert type(s.grad_fn).__name__.startswith("FusedSSIM")
    (UP * s).backward()
    with torch.no_grad():
        assert torch.equal(tr.ssim(a.detach(), yc), s.detach())          # the no-grad path (no partials written)
    b = cuda(x, True)
    s2 = tr.ssim(b, yc)
    (UP * s2).backward()
    assert torch.equal(s2.detach(), s.detach()) and torch.equal(b.grad, a.grad)
    (v64, g64), (v32, g32) = _ref_ssim(x, y, F64), _ref_ssim(x, y, F32)
    check(group, f"{tuple(x.shape)} value", s, v64, v32, 1.0)
    check(group + " d/dx", f"{tuple(x.shape)} d/dx", a.grad, g64, g32, UP / x.numel())


def _ref_l1(x, y, mask, dtype):
    a = leaf(x, dtype)
    v = R.l1(a, y, mask, dtype)
    (2.5 * v).backward()
    return v.detach(), a.grad


def l1_case(group, x, y, mask, xc=None, yc=None):
    """tr.l1_loss on (x, y[, mask]); xc / yc: the GPU tensors to use instead of copies of x / y (views at an odd offset)"""
    from csplat import train as tr
    a = (cuda(x) if xc is None else xc).requires_grad_()
    yc, mc = cuda(y) if yc is None else yc, cuda(mask)
    v = tr.l1_loss(a, yc, mc)
    assert type(v.grad_fn).__name__.startswith("FusedL1")
    (2.5 * v).backward()
    assert torch.equal(tr.l1_loss(a.detach(), yc, mc), v.detach())
    b = a.detach().clone().requires_grad_() if xc is None else a.detach().requires_grad_()
    v2 = tr.l1_loss(b, yc, mc)
    (2.5 * v2).backward()
    assert torch.equal(v2.detach(), v.detach()) and torch.equal(b.grad, a.grad)
    (v64, g64), (v32, g32) = _ref_l1(x, y, mask, F64), _ref_l1(x, y, mask, F32)
    where = f"{tuple(x.shape)} mask {None if mask is None else tuple(mask.shape)}"
    check(group, f"{where} value", v, v64, v32, 1e-30)
    check(group, f"{where} d/dx", a.grad, g64, g32, 2.5 / x.numel())
    np.testing.assert_array_equal(np.sign(_np(a.grad)), np.sign(_np(g64)), err_msg="the sign bytes")


def blur_case(group, x, seed=0):
    from csplat import train as tr
    wgt = torch.rand(x.shape, generator=torch.Generator().manual_seed(seed))
    a = cuda(x, True)
    out = tr.GaussianBlur11.apply(a)
    assert type(out.grad_fn).__name__.startswith("GaussianBlur11")
    (out * wgt.cuda()).sum().backward()
    with torch.no_grad():
        assert torch.equal(tr.GaussianBlur11.apply(a), out.detach())
    res = []
    for dt in (F64, F32):
        b = leaf(x, dt)
        o = R.blur(b, dt)
        (o * wgt.to(dt)).sum().backward()
        res.append((o.detach(), b.grad))
    check(group, f"{tuple(x.shape)} value", out, res[0][0], res[1][0], 1e-30)
    check(group, f"{tuple(x.shape)} adjoint", a.grad, res[0][1], res[1][1], 1e-30)


def psnr_case(group, x, y):
    from csplat import train as tr
    xc, yc = cuda(x), cuda(y)
    got = tr.psnr(xc, yc)
    assert got.shape == (x.shape[0], 1) and torch.equal(got, tr.psnr(xc, yc))
    check(group, f"{tuple(x.shape)}", got, R.psnr(x, y, F64), R.psnr(x, y, F32), 1.0)


@pytest.mark.parametrize("shape", R.IMAGE_SMALL)
def test_every_image_entry_point_on_small_and_thin_images(shape):
    """ssim, l1_loss (plain, masked), FusedImageLoss (plain, masked with 1 and C planes, with and without add), GaussianBlur11, psnr on
    images narrower or shorter than the 11-tap window or than one 64 x 16 tile, and at the tile edges +- 1"""
    x, y, _ = R.image_case("uniform", shape, 0, seed=sum(shape))
    ssim_case("ssim small", x, y)
    l1_case("l1 small", x, y, None)
    blur_case("blur small", x)
    psnr_case("psnr small", x, y)
    image_loss_case("image_loss small", "uniform", shape, 0, False, seed=sum(shape))
    image_loss_case("image_loss small", "uniform", shape, 0, True, seed=sum(shape))
    if shape[2] * shape[3] > 1:
        for mc in sorted({1, shape[1]}):
            image_loss_case("image_loss small", "uniform", shape, mc, mc == 1, seed=sum(shape))
            l1_case("l1 small", x, y, R.make_mask(shape, mc, 3))


@pytest.mark.parametrize("kind,shape", [("saturated", R.IMAGE_PRODUCTION[0]), ("quantised", R.IMAGE_PRODUCTION[1]), ("uniform", R.IMAGE_PRODUCTION[2])])
def test_ssim_blur_and_psnr_at_production_size(kind, shape):
    x, y, _ = R.image_case(kind, shape, 0, seed=5)
    ssim_case(f"ssim {kind}", x, y)
    blur_case("blur production", x)
    psnr_case("psnr production", x, y)


def test_image_kernels_at_the_most_planes_one_launch_carries():
    """[21845,3,16,8]: 65 535 planes, blockIdx.z at its limit"""
    x, y, _ = R.image_case("uniform", R.IMAGE_MAX_PLANES, 0, seed=9)
    image_loss_case("image_loss 65535 planes", "uniform", R.IMAGE_MAX_PLANES, 1, True, seed=9)
    ssim_case("ssim 65535 planes", x, y)
    blur_case("blur 65535 planes", x)


def test_more_planes_than_one_launch_carries_are_split_not_refused():
    """65 536 planes through ssim() and GaussianBlur11, and 13 108 through ssim(return_map=True), whose five stacked windows make 65 540:
    the wrappers call the library in chunks of at most 65 535 planes (the sums are per plane), on the HIP path"""
    from csplat import train as tr
    x, y, _ = R.image_case("uniform", R.IMAGE_OVER_PLANES, 0, seed=10)
    ssim_case("ssim 65536 planes", x, y)
    blur_case("blur 65536 planes", x)
    x, y, _ = R.image_case("uniform", R.IMAGE_OVER_PLANES_MAP, 0, seed=11)
    wgt = torch.rand(x.shape, generator=torch.Generator().manual_seed(1))
    a = cuda(x, True)
    m = tr.ssim(a, cuda(y), return_map=True)
    (m * wgt.cuda()).sum().backward()
    res = []
    for dt in (F64, F32):
        b = leaf(x, dt)
        o = R.ssim_map(b, y, dt)
        (o * wgt.to(dt)).sum().backward()
        res.append((o.detach(), b.grad))
    check("ssim map 13108 planes", "map", m, res[0][0], res[1][0], 1.0)
    check("ssim map 13108 planes", "d/dx", a.grad, res[0][1], res[1][1], 1e-30)


@pytest.mark.allow_fallbacks("shape")
def test_image_losses_reports_too_many_planes_as_a_miss_on_shape():
    """image_losses at 65 536 planes leaves the one-launch kernel: the miss is of kind "shape" (not "dtype"), and the composed
    l1_loss + ssim it then runs are the HIP kernels, in chunks"""
    from types import SimpleNamespace
    from csplat import native, train as tr
    x, y, _ = R.image_case("uniform", R.IMAGE_OVER_PLANES, 0, seed=12)
    before = dict(native.FALLBACK_COUNTS)
    a = cuda(x, True)
    loss = tr.image_losses(a, cuda(y), SimpleNamespace(lambda_dssim=LAM))
    (UP * loss).backward()
    moved = {k: v - before.get(k, 0) for k, v in native.FALLBACK_COUNTS.items() if v != before.get(k, 0)}
    assert moved == {("train.image_losses", "shape"): 1}, moved
    res = []
    for dt in (F64, F32):
        b = leaf(x, dt)
        o = R.image_loss(b, y, LAM, dtype=dt)[0]
        (UP * o).backward()
        res.append((o.detach(), b.grad))
    check("image_losses 65536 planes", "loss", loss, res[0][0], res[1][0], LAM)
    check("image_losses 65536 planes", "d/dx", a.grad, res[0][1], res[1][1], UP / x.numel())


# ---- the SSIM's C-ABI surface that no Python wrapper reaches: csplat_ssim_fwd_masked, map_out of csplat_ssim_fwd, addend / add_scale
# of csplat_ssim_bwd (include/csplat.h states them), called through native.lib
def _taps11():
    return (C.c_float * 11)(*[float(v) for v in R.window(F32)])


def _ssim_fwd_abi(x, y, mask=None, want_p=True, want_map=False):
    """csplat_ssim_fwd (mask None) / csplat_ssim_fwd_masked -> (p [3,B,C,H,W] or None, map [B,C,H,W] or None, partial); every output
    starts as NaN, so an element the kernel leaves out fails whatever looks at it"""
    n_, dev = _lib()
    B, Cc, H, W = x.shape
    xc, yc, mk = cuda(x), cuda(y), cuda(mask)
    p = torch.full((3,) + tuple(x.shape), float("nan"), device=dev) if want_p else None
    mp = torch.full(tuple(x.shape), float("nan"), device=dev) if want_map else None
    partial = torch.full((int(n_.lib.csplat_ssim_partial_count(B * Cc, H, W)),), float("nan"), device=dev)
    pp = [n_.ptr(p[k]) if want_p else None for k in range(3)]
    if mask is None:
        n_.check(n_.lib.csplat_ssim_fwd(n_.stream_handle(dev), B * Cc, H, W, _taps11(), n_.ptr(xc), n_.ptr(yc), *pp, n_.ptr(mp),
                                        n_.ptr(partial)), "csplat_ssim_fwd")
    else:
        n_.check(n_.lib.csplat_ssim_fwd_masked(n_.stream_handle(dev), B, Cc, H, W, _taps11(), n_.ptr(xc), n_.ptr(yc), n_.ptr(mk),
                                               int(mask.shape[1]), *pp, n_.ptr(mp), n_.ptr(partial)), "csplat_ssim_fwd_masked")
    return p, mp, partial


def _ssim_bwd_abi(x, y, p, g, addend=None, add_scale=None):
    """csplat_ssim_bwd with inv_n = 1 / numel -> (rc, dx)"""
    n_, dev = _lib()
    B, Cc, H, W = x.shape
    xc, yc = cuda(x), cuda(y)
    gs = torch.tensor([g], dtype=F32, device=dev)
    dx = torch.full(tuple(x.shape), float("nan"), device=dev)
    rc = n_.lib.csplat_ssim_bwd(n_.stream_handle(dev), B * Cc, H, W, _taps11(), n_.ptr(xc), n_.ptr(yc), n_.ptr(p[0]), n_.ptr(p[1]),
                                n_.ptr(p[2]), n_.ptr(gs), 1.0 / x.numel(), n_.ptr(addend), n_.ptr(add_scale), n_.ptr(dx))
    torch.cuda.synchronize()
    return rc, dx


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("shape", R.SSIM_ABI_SHAPES)
def test_ssim_fwd_masked_with_one_mask_plane_and_with_one_per_channel(shape):
    """csplat_ssim_fwd_masked: sum(partial) / n is mean((1 - S) m); p1..p3 are the mask times the unmasked call's p1..p3 (one float32
    product, so equal); csplat_ssim_bwd on them with g = -1 writes the gradient of the masked term"""
    x, y, _ = R.image_case("uniform", shape, 0, seed=sum(shape))
    n = x.numel()
    p_plain, _, _ = _ssim_fwd_abi(x, y)
    for mc in sorted({1, shape[1]}):
        mask = R.make_mask(shape, mc, 3)
        if shape[2] * shape[3] == 1:
            mask.fill_(0.5)                      # (make_mask leaves the only pixel of a 1 x 1 image at 1)
        p, _, partial = _ssim_fwd_abi(x, y, mask)
        res = []
        for dt in (F64, F32):
            a = leaf(x, dt)
            v = ((1.0 - R.ssim_map(a, y, dt)) * mask.to(dt)).mean()
            v.backward()
            res.append((v.detach(), a.grad))
        where = f"{tuple(shape)} mask planes {mc}"
        check("ssim abi masked", f"{where} value", partial.double().sum() / n, res[0][0], res[1][0], 1.0)
        assert torch.equal(p, p_plain * cuda(mask).unsqueeze(0)), f"{where}: p1..p3 are not mask * the unmasked partials"
        rc, dx = _ssim_bwd_abi(x, y, p, -1.0)
        assert rc == 0
        check("ssim abi masked d/dx", f"{where} d/dx", dx, res[0][1], res[1][1], 1.0 / n)


@pytest.mark.parametrize("shape", R.SSIM_ABI_SHAPES)
def test_ssim_map_out_with_and_without_the_partial_derivatives(shape):
    """map_out of csplat_ssim_fwd is the SSIM map, the same bits whether p1..p3 are asked for or NULL; the masked entry writes the same
    (unweighted) map"""
    x, y, _ = R.image_case("uniform", shape, 0, seed=sum(shape))
    _, m_with, part_with = _ssim_fwd_abi(x, y, want_p=True, want_map=True)
    _, m_without, part_without = _ssim_fwd_abi(x, y, want_p=False, want_map=True)
    assert torch.equal(_bits(m_with), _bits(m_without)) and torch.equal(_bits(part_with), _bits(part_without))
    check("ssim abi map", f"{tuple(shape)} map", m_with, R.ssim_map(x, y, F64), R.ssim_map(x, y, F32), 1.0)
    check("ssim abi map", f"{tuple(shape)} mean", part_with.double().sum() / x.numel(), R.ssim(x, y, F64), R.ssim(x, y, F32), 1.0)
    if shape[2] * shape[3] > 1:
        _, m_masked, _ = _ssim_fwd_abi(x, y, R.make_mask(shape, 1, 3), want_p=False, want_map=True)
        assert torch.equal(_bits(m_masked), _bits(m_with))


@pytest.mark.parametrize("shape", R.SSIM_ABI_SHAPES)
def test_ssim_bwd_addend_and_add_scale_go_together(shape):
    """csplat_ssim_bwd with addend / add_scale: dx = dx_without + add_scale[0] * addend; one of the pair without the other is refused"""
    n_, dev = _lib()
    x, y, _ = R.image_case("uniform", shape, 0, seed=sum(shape))
    p, _, _ = _ssim_fwd_abi(x, y)
    rc, dx0 = _ssim_bwd_abi(x, y, p, UP)
    assert rc == 0
    addend = (torch.rand(x.shape, generator=torch.Generator().manual_seed(7)) - 0.5) * (4.0 / x.numel())
    ac, sc = cuda(addend), torch.tensor([-0.3], dtype=F32, device=dev)
    rc, dx = _ssim_bwd_abi(x, y, p, UP, ac, sc)
    assert rc == 0
    want = [dx0.cpu().to(dt) + sc.cpu().to(dt) * addend.to(dt) for dt in (F64, F32)]
    check("ssim abi addend", f"{tuple(shape)} d/dx", dx, want[0], want[1], 1e-30)
    for a_, s_ in ((ac, None), (None, sc)):
        rc, _ = _ssim_bwd_abi(x, y, p, UP, a_, s_)
        assert rc == 2 and b"addend and add_scale go together" in n_.lib.csplat_last_error()


@pytest.mark.parametrize("n", R.L1_SIZES)
def test_l1_sizes_around_the_four_in_flight_loop(n):
    x, y, _ = R.image_case("saturated" if n > 100 else "uniform", (1, 1, 1, n), 0, seed=n % 97)
    if n > 1:
        y[0, 0, 0, n // 2] = x[0, 0, 0, n // 2]              # an exact tie: sign 0
    l1_case("l1 sizes", x.reshape(n), y.reshape(n), None)


@pytest.mark.parametrize("shape,mc", R.L1_MASKED)
def test_l1_masked_with_planes_of_whole_and_broken_float4_groups(shape, mc):
    x, y, mask = R.image_case("saturated", shape, mc, seed=4)
    l1_case("l1 masked", x, y, mask)


def test_l1_of_a_slice_of_a_batch_with_odd_planes():
    """l1_loss(img[i], gt[i]) where an image is 3 * 37 * 53 floats: the views start 4, 8 or 12 bytes off a 16-byte boundary.  The kernel
    takes its scalar form (as k_psnr and adam_span do); plain, masked with a mask slice at an odd offset, and one operand only misaligned"""
    shape, i = R.L1_SLICE
    x, y, mask = R.image_case("uniform", shape, 1, seed=6)
    xb, yb, mb = x.cuda(), y.cuda(), mask.cuda()
    for j in range(shape[0]):
        assert xb[j].is_contiguous() and (j == 0 or xb[j].data_ptr() % 16 != 0)
        l1_case("l1 slice", x[j], y[j], None, xc=xb[j].detach(), yc=yb[j])
    l1_case("l1 slice", x[i], y[i], None, xc=xb[i].detach(), yc=y[i].cuda())              # only a misaligned
    l1_case("l1 slice", x[i], y[i], None, xc=x[i].cuda(), yc=yb[i])                       # only b misaligned
    from csplat import train as tr
    a = xb[i:i + 1].detach().requires_grad_()
    v = tr.l1_loss(a, yb[i:i + 1], mb[i:i + 1])                                           # a [1,C,H,W] view with its [1,1,H,W] mask view
    assert type(v.grad_fn).__name__.startswith("FusedL1") and mb[i:i + 1].data_ptr() % 16 != 0
    (2.5 * v).backward()
    (v64, g64), (v32, g32) = _ref_l1(x[i:i + 1], y[i:i + 1], mask[i:i + 1], F64), _ref_l1(x[i:i + 1], y[i:i + 1], mask[i:i + 1], F32)
    check("l1 slice", "masked value", v, v64, v32, 1e-30)
    check("l1 slice", "masked d/dx", a.grad, g64, g32, 2.5 / a.numel())


def test_psnr_of_equal_images_is_inf():
    """utils/image_utils.py:17-21 gives 20 log10(1 / sqrt(0)) = inf; a batch with one equal image has inf there and finite values elsewhere"""
    x, y, _ = R.image_case("uniform", (3, 3, 37, 53), 0, seed=8)
    y[1] = x[1]
    psnr_case("psnr equal", x, y)
    from csplat import train as tr
    got = tr.psnr(x.cuda(), y.cuda()).cpu()
    assert torch.isinf(got[1]) and got[1] > 0 and torch.isfinite(got[0]) and torch.isfinite(got[2])
    psnr_case("psnr equal", x, x.clone())


# ================================================================================================ Adam
LRS = [1.6e-4, 2.5e-3, 0.05, 1e-3, 5e-3]


def _adam_inputs(n, lr, seed, with_state):
    """(p, g, m, v) float32 CUDA: a share of p exactly 0, a share |p| <= lr, the rest ~1; g with exact zeros, 1e-20 and 1e+4 mixed in"""
    gen = torch.Generator(device="cuda").manual_seed(seed)
    u = torch.rand(n, device="cuda", generator=gen)
    p = torch.randn(n, device="cuda", generator=gen)
    p = torch.where(u < 0.3, torch.zeros_like(p), torch.where(u < 0.6, p.clamp(-1, 1) * lr, p))
    w = torch.rand(n, device="cuda", generator=gen)
    g = torch.randn(n, device="cuda", generator=gen) * 10.0 ** float(seed % 5 - 2)
    g = torch.where(w < 0.1, torch.zeros_like(g), torch.where(w < 0.2, torch.full_like(g, 1e-20), torch.where(w < 0.25, torch.full_like(g, 1e4), g)))
    if with_state:
        m = torch.randn(n, device="cuda", generator=gen) * g.abs().clamp(1e-3, 10.0)
        v = (m * (0.5 + 1.5 * torch.rand(n, device="cuda", generator=gen))) ** 2
    else:
        m, v = torch.zeros_like(p), torch.zeros_like(p)
    return p, g, m, v


def _offset_view(t, off_floats):
    """a contiguous view holding t's values that starts off_floats * 4 bytes past a 16-byte boundary (a slice of a larger buffer)"""
    buf = torch.zeros(t.numel() + 8, dtype=t.dtype, device=t.device)
    assert buf.data_ptr() % 16 == 0
    v = buf[off_floats:off_floats + t.numel()]
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == (4 * off_floats) % 16
    return v


def _make_optimizer(tensors, lrs, betas, eps, step):
    """GroupedAdam over `tensors` [(p, g, m, v)], one group each; step > 1: the state (step - 1, m, v) is injected"""
    from csplat.optim import GroupedAdam
    ps = [torch.nn.Parameter(p) for p, _, _, _ in tensors]
    for q, (p, g, _, _) in zip(ps, tensors):
        assert q.data_ptr() == p.data_ptr()
        q.grad = g
    opt = GroupedAdam([{"params": [q], "lr": lr} for q, lr in zip(ps, lrs)], lr=0.0, betas=betas, eps=eps)
    if step > 1:
        for q, (_, _, m, v) in zip(ps, tensors):
            opt.state[q] = {"step": torch.tensor(float(step - 1)), "exp_avg": m, "exp_avg_sq": v}
    return ps, opt


def _check_adam(group, where, tensors0, ps, opt, lrs, betas, eps, step):
    """parameters (all elements against max |p|, and the UPDATE of the elements that started at |p| <= lr against lr) and both moments
    after the step, against adam_step from the saved inputs"""
    for k, ((p0, g, m0, v0), q, lr) in enumerate(zip(tensors0, ps, lrs)):
        if p0.numel() == 0:
            continue
        st = opt.state[q]
        assert float(st["step"]) == float(step)
        r = [R.adam_step(p0, g, m0, v0, lr, betas[0], betas[1], eps, step, dt) for dt in (F64, F32)]
        tag = f"{where} tensor {k} n {p0.numel()}"
        check(group + " p", f"{tag} p", q.detach(), r[0][0], r[1][0], lr)
        small = (p0.abs() <= lr)
        if bool(small.any()):
            upd = lambda t: (t.detach().cpu().double() - p0.double())[small]  # noqa: E731
            check(group + " update", f"{tag} update", upd(q), upd(r[0][0]), upd(r[1][0]), lr)
        gmax = float(g.abs().max())
        check(group + " m", f"{tag} exp_avg", st["exp_avg"], r[0][1], r[1][1], max(gmax, 1e-30))
        check(group + " v", f"{tag} exp_avg_sq", st["exp_avg_sq"], r[0][2], r[1][2], max(gmax * gmax, 1e-30))


def adam_case(group, where, sizes, betas=(0.9, 0.999), eps=1e-15, step=10, misalign=None, dev_path=True):
    """one step of every tensor through GroupedAdam.step() (csplat_adam_step), and through captured_setup() / step_captured()
    (csplat_adam_step_dev), called eagerly: first with valid = 0 (nothing may change, bit for bit), then with valid = 1.
    misalign: {tensor index: (which of "pgmv", offset in floats)}"""
    lrs = [LRS[k % len(LRS)] for k in range(len(sizes))]
    for path in (("host", "dev") if dev_path else ("host",)):
        made = [_adam_inputs(n, lr, 31 * k + n % 1000, True) for k, (n, lr) in enumerate(zip(sizes, lrs))]
        if misalign:
            for k, (which, off) in misalign.items():
                made[k] = tuple(_offset_view(t, off) if c in which else t for c, t in zip("pgmv", made[k]))
        saved = [tuple(t.detach().cpu().clone() for t in ts) for ts in made]
        # (the host path at step 1 starts from no state: GroupedAdam creates the zero moments itself)
        if step == 1:
            saved = [(p, g, torch.zeros_like(p), torch.zeros_like(p)) for p, g, _, _ in saved]
        if path == "host":
            ps, opt = _make_optimizer(made, lrs, betas, eps, step)
            opt.step()
        else:
            if step == 1:
                continue                      # captured_setup() needs existing state: the device path starts at step 2
            ps, opt = _make_optimizer(made, lrs, betas, eps, step)
            cap = opt.captured_setup()
            assert int(cap["state"].item()) == step - 1
            before = [t.clone() for ts in made for t in ts]
            opt.step_captured(torch.zeros(1, dtype=torch.int32, device="cuda"))
            torch.cuda.synchronize()
            assert int(cap["state"].item()) == step - 1
            for a, b in zip(before, [t for ts in made for t in ts]):
                assert torch.equal(a.view(torch.int32), b.view(torch.int32)), "valid = 0 changed something"
            opt.step_captured(torch.ones(1, dtype=torch.int32, device="cuda"))
            assert int(cap["state"].item()) == step
            opt.captured_advance_host()
        _check_adam(f"{group} {path}", where, saved, ps, opt, lrs, betas, eps, step)


@pytest.mark.parametrize("eps", R.ADAM_EPS)
@pytest.mark.parametrize("betas", R.ADAM_BETAS)
@pytest.mark.parametrize("step", R.ADAM_STEPS)
def test_adam_one_step_from_an_injected_state(step, betas, eps):
    """bias corrections at step counts up to 30 000, two beta pairs, two eps; sizes around one float4, one workgroup, one grid row"""
    adam_case("adam injected", f"step {step} betas {betas} eps {eps}", [1, 3, 4, 5, 1023, 1025, 4097], betas, eps, step)


@pytest.mark.parametrize("sizes", [R.ADAM_SIZES[:7], R.ADAM_SIZES[7:8], R.ADAM_SIZES[8:9], R.ADAM_SIZES[9:], list(R.ADAM_LONG_SHORT)])
def test_adam_sizes_up_to_the_capped_grid(sizes):
    """n around and beyond 2048 workgroups x 4096 elements (the stride loop of adam_span repeats); 9 000 000 next to 7 in one launch (the
    short tensor's workgroups leave k_adam_dev early)"""
    adam_case("adam sizes", f"sizes {sizes}", sizes)


@pytest.mark.parametrize("n_tensors", R.ADAM_MANY)
def test_adam_more_tensors_than_one_table(n_tensors):
    sizes = [1 + (37 * k) % 301 for k in range(n_tensors)]
    sizes[5] = 0                                          # an empty tensor in the list
    adam_case("adam tables", f"{n_tensors} tensors", sizes)


def test_adam_operands_off_the_16_byte_boundary():
    """p, g, m, v each in turn a contiguous view 4, 8 or 12 bytes past a 16-byte boundary, and all four at once: adam_span's scalar path"""
    mis, sizes = {}, []
    for which in ("p", "g", "m", "v", "pgmv"):
        for off in (1, 2, 3):
            mis[len(sizes)] = (which, off)
            sizes.append([1025, 4097, 5, 1023, 260][len(sizes) % 5])
    sizes.append(4097)                                    # an aligned one in the same launch
    adam_case("adam misaligned", "views", sizes, misalign=mis)


def _grads_at(it, k, n):
    gen = torch.Generator(device="cuda").manual_seed(1000 * it + k)
    g = torch.randn(n, device="cuda", generator=gen) * 10.0 ** (k - 1)
    return torch.where(torch.rand(n, device="cuda", generator=gen) < 0.1, torch.zeros_like(g), g)


@pytest.mark.parametrize("path,n_steps", [("host", 200), ("dev", 20)])
def test_adam_many_steps_with_a_tensor_that_skips_every_second(path, n_steps):
    """200 steps of GroupedAdam.step() with tensor 1 receiving no gradient on every second step (its count lags: two launches per
    step); 20 steps of the device-side form (every tensor has a gradient there), after one ordinary step"""
    sizes, lrs, betas, eps = [4097, 1025, 7], [1.6e-4, 0.05, 1e-3], (0.9, 0.999), 1e-15
    init = [_adam_inputs(n, lr, k, False)[0] for k, (n, lr) in enumerate(zip(sizes, lrs))]
    saved = [p.cpu().clone() for p in init]
    skip = lambda it, k: path == "host" and k == 1 and it % 2 == 1  # noqa: E731
    ps, opt = _make_optimizer([(p, None, None, None) for p in init], lrs, betas, eps, 1)
    valid = torch.ones(1, dtype=torch.int32, device="cuda")
    for it in range(n_steps):
        for k, q in enumerate(ps):
            q.grad = None if skip(it, k) else _grads_at(it, k, sizes[k])
        if path == "host" or it == 0:
            opt.step()
            if path == "dev":
                opt.captured_setup()
        else:
            opt.captured_refresh_lr()
            opt.step_captured(valid)
            opt.captured_advance_host()
    grads_of = lambda it, k: None if skip(it, k) else _grads_at(it, k, sizes[k]).cpu()  # noqa: E731
    r64, s64 = R.adam_run(saved, grads_of, n_steps, lrs, betas[0], betas[1], eps, F64)
    r32, s32 = R.adam_run(saved, grads_of, n_steps, lrs, betas[0], betas[1], eps, F32)
    for k, q in enumerate(ps):
        st = opt.state[q]
        assert int(st["step"]) == s64[k][0]
        gmax = max(float(_grads_at(it, k, sizes[k]).abs().max()) for it in range(0, n_steps, 7))
        check(f"adam run {path}", f"tensor {k} p after {n_steps}", q.detach(), r64[k], r32[k], lrs[k])
        small = saved[k].abs() <= lrs[k]
        upd = lambda t: (t.detach().cpu().double() - saved[k].double())[small]  # noqa: E731
        check(f"adam run {path}", f"tensor {k} path of small p", upd(q), upd(r64[k]), upd(r32[k]), lrs[k])
        check(f"adam run {path}", f"tensor {k} exp_avg", st["exp_avg"], s64[k][1], s32[k][1], gmax)
        check(f"adam run {path}", f"tensor {k} exp_avg_sq", st["exp_avg_sq"], s64[k][2], s32[k][2], gmax * gmax)
    if path == "dev":
        assert int(opt._cap["state"].item()) == n_steps


# ================================================================================================ store and bookkeeping (C ABI)
def _lib():
    from csplat import native as n_
    return n_, torch.device("cuda")


def _mask_to_map(mask_u8, base):
    n_, dev = _lib()
    n = mask_u8.shape[0]
    m8 = torch.from_numpy(mask_u8).to(dev)
    mp = torch.full((n,), -7, dtype=torch.int32, device=dev)
    cnt = torch.full((1,), -7, dtype=torch.int32, device=dev)
    tmp = torch.empty(int(n_.lib.csplat_mask_to_map_temp_bytes(n)), dtype=torch.uint8, device=dev)
    n_.check(n_.lib.csplat_mask_to_map(n_.stream_handle(dev), n, n_.ptr(m8), base, n_.ptr(mp), n_.ptr(cnt), n_.ptr(tmp)), "csplat_mask_to_map")
    return mp, int(cnt.item())


def _masks(n, rng):
    first, last = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
    first[0], last[-1] = 1, 1
    return {"all 0": np.zeros(n, np.uint8), "all 1": np.ones(n, np.uint8), "first": first, "last": last,
            "0.5": (rng.random(n) < 0.5).astype(np.uint8), "0.001": (rng.random(n) < 0.001).astype(np.uint8),
            "bytes": rng.choice(np.array([0, 1, 2, 255], np.uint8), n)}


@pytest.mark.parametrize("n", R.MAP_SIZES)
def test_mask_to_map_at_the_scan_tile_edges_and_the_second_sweep(n):
    """csplat_mask_to_map == the stable compaction map, at multiples of SCAN_TILE +- 1, beyond 4096 block sums, on all-0 / all-1 /
    one-hot / sparse / dense masks and on mask bytes other than 0 and 1; three bases"""
    rng = np.random.default_rng(n % 1000)
    for j, (name, mask) in enumerate(_masks(n, rng).items()):
        for base in ([R.MAP_BASES[j % 3]] if n > 100_000 else R.MAP_BASES):
            mp, cnt = _mask_to_map(mask, base)
            want, want_cnt = R.mask_to_map(mask, base)
            assert cnt == want_cnt, (n, name, base, cnt, want_cnt)
            got = mp.cpu().numpy()
            if not np.array_equal(got, want):
                bad = np.flatnonzero(got != want)
                raise AssertionError(f"n {n} mask {name} base {base}: {bad.size} rows differ, first {bad[0]}: {got[bad[0]]} != {want[bad[0]]}")


def _scatter(srcs, dsts, n_rows, mp):
    n_, dev = _lib()
    k = len(dsts)
    sp = (C.c_void_p * k)(*[None if t is None else t.data_ptr() for t in srcs])
    dp = (C.c_void_p * k)(*[t.data_ptr() for t in dsts])
    rb = (C.c_int64 * k)(*[t[0].numel() * t.element_size() for t in dsts])
    return n_.lib.csplat_rows_scatter(n_.stream_handle(dev), k, C.cast(sp, C.c_void_p), C.cast(dp, C.c_void_p), C.cast(rb, C.c_void_p),
                                      n_rows, n_.ptr(mp))


SENTINEL = 0x7A7A7A7A


def _scatter_case(n, widths, mask, zero_fill=()):
    """srcs of the given widths (int32 words, every word distinct), dsts pre-filled with a sentinel, a map from `mask`; srcs listed in
    zero_fill are NULL.  Every word of every destination is compared: a stray write shows"""
    dev = torch.device("cuda")
    mp, cnt = _mask_to_map(mask, 0)
    srcs = [None if i in zero_fill else (torch.arange(n * w, dtype=torch.int32, device=dev).reshape(n, w) * 7 + i) for i, w in enumerate(widths)]
    dsts = [torch.full((n + 20, w), SENTINEL, dtype=torch.int32, device=dev) for w in widths]
    rc = _scatter(srcs, dsts, n, mp)
    want_map = mp.cpu().numpy()
    return rc, srcs, dsts, want_map


@pytest.mark.parametrize("n", R.SCATTER_ROWS)
def test_rows_scatter_beyond_the_capped_grid(n):
    """100 000 and 250 000 rows of widths {1, 3, 4, 45, 48} words in one launch (the grid is capped at 4096 x 1024 words: the stride loop
    repeats), one source zero-filled; a map that keeps nothing"""
    rng = np.random.default_rng(n)
    widths = R.SCATTER_WIDTHS + [45]
    rc, srcs, dsts, mp = _scatter_case(n, widths, (rng.random(n) < 0.5).astype(np.uint8), zero_fill=(5,))
    assert rc == 0
    for s, d in zip(srcs, dsts):
        ref = np.full(tuple(d.shape), SENTINEL, np.int32)
        R.rows_scatter([None if s is None else s.cpu().numpy()], [ref], mp)
        np.testing.assert_array_equal(d.cpu().numpy(), ref)
    rc, srcs, dsts, mp = _scatter_case(n, [3, 48], np.zeros(n, np.uint8))
    assert rc == 0 and (mp == -1).all()
    for d in dsts:
        assert bool((d == SENTINEL).all())


def test_rows_scatter_table_limit():
    """32 tensors in one launch; 33 are refused with an error code and nothing is written"""
    n = 20_000
    rng = np.random.default_rng(1)
    mask = (rng.random(n) < 0.5).astype(np.uint8)
    widths = [R.SCATTER_WIDTHS[i % 5] for i in range(32)]
    rc, srcs, dsts, mp = _scatter_case(n, widths, mask, zero_fill=(7, 31))
    assert rc == 0
    for s, d in zip(srcs, dsts):
        ref = np.full(tuple(d.shape), SENTINEL, np.int32)
        R.rows_scatter([None if s is None else s.cpu().numpy()], [ref], mp)
        np.testing.assert_array_equal(d.cpu().numpy(), ref)
    rc, srcs, dsts, mp = _scatter_case(n, widths + [4], mask)
    torch.cuda.synchronize()
    assert rc != 0
    for d in dsts:
        assert bool((d == SENTINEL).all())


def _act_inputs(P, seed):
    """raw parameters with saturating rows: opacities and scales of +-100 next to ordinary ones -> (raw, saturated-row mask)"""
    gen = torch.Generator().manual_seed(seed)
    raw = [torch.randn(P, 1, generator=gen) * 3, torch.randn(P, 3, generator=gen), torch.randn(P, 1, 3, generator=gen),
           torch.randn(P, 15, 3, generator=gen)]
    sat = torch.zeros(P, dtype=torch.bool)
    idx = torch.arange(0, P, 5)
    sat[idx] = True
    raw[0][idx, 0] = torch.tensor([100.0, -100.0, 30.0, -90.0])[torch.arange(idx.numel()) % 4]
    raw[1][idx] = torch.tensor([[100.0, -100.0, 89.0], [-100.0, 100.0, -110.0]])[torch.arange(idx.numel()) % 2]
    return raw, sat


@pytest.mark.parametrize("P", R.ACT_P)
def test_gaussian_activations_beyond_the_capped_grid_and_saturated(P):
    """_GaussianActivations (k_gauss_act_fwd / _bwd; the grid is capped at 8192 x 256 threads: from P = 43 691 the stride loop repeats).
    Ordinary rows against float64; rows whose raw opacity / scale saturates float32 (sigmoid -> 0 or 1, exp -> 0 or inf) against torch's
    float32 result for equality (they are disjoint from the ordinary rows by construction); the SH copy and its gradient bit for bit;
    each upstream gradient absent in turn"""
    from csplat.gaussians import _GaussianActivations
    raw, sat = _act_inputs(P, P % 1000)
    gen = torch.Generator().manual_seed(7)
    w = [torch.randn(P, 1, generator=gen) + 2.5, torch.randn(P, 3, generator=gen) + 2.5, torch.randn(P, 16, 3, generator=gen)]
    ok = ~sat
    for absent in (None, 0, 1, 2):
        a = [cuda(t, True) for t in raw]
        out = _GaussianActivations.apply(*a)
        assert type(out[0].grad_fn).__name__.startswith("_GaussianActivations")
        ws = [None if k == absent else w[k] for k in range(3)]
        sum((o * wk.cuda()).sum() for o, wk in zip(out, ws) if wk is not None).backward()
        t32 = [cuda(t, True) for t in raw]
        o32 = (torch.sigmoid(t32[0]), torch.exp(t32[1]), torch.cat((t32[2], t32[3]), dim=1))
        sum((o * wk.cuda()).sum() for o, wk in zip(o32, ws) if wk is not None).backward()
        grads = [t.grad if t.grad is not None else torch.zeros_like(t) for t in a]
        g32 = [t.grad if t.grad is not None else torch.zeros_like(t) for t in t32]
        # saturated rows and the copies: equality with torch's float32 result
        for name, x, y in (("opacity", out[0], o32[0]), ("scales", out[1], o32[1]), ("d_opacity", grads[0], g32[0]), ("d_scaling", grads[1], g32[1])):
            np.testing.assert_array_equal(x.detach().cpu().numpy()[sat.numpy()], y.detach().cpu().numpy()[sat.numpy()], err_msg=f"saturated {name}")
        assert torch.equal(out[2].detach().view(torch.int32), o32[2].detach().view(torch.int32))
        assert torch.equal(grads[2].view(torch.int32), g32[2].view(torch.int32)) and torch.equal(grads[3].view(torch.int32), g32[3].view(torch.int32))
        if absent is None and P > 1:
            assert bool(torch.isinf(out[1].detach()[sat.cuda()]).any()) and float(out[0].detach()[sat.cuda()].min()) == 0.0
        if not bool(ok.any()):
            continue
        # ordinary rows: the restatement
        r = []
        for dt in (F64, F32):
            o = R.gauss_act(*raw, dtype=dt)
            r.append((o, R.gauss_act_adjoint(raw, ws, dt)))
        tag = f"P {P} absent {absent}"
        check("gauss_act", f"{tag} opacity", out[0].detach().cpu()[ok], r[0][0][0][ok], r[1][0][0][ok], 1e-30)
        check("gauss_act", f"{tag} scales", out[1].detach().cpu()[ok], r[0][0][1][ok], r[1][0][1][ok], 1e-30)
        check("gauss_act", f"{tag} d_opacity", grads[0].cpu()[ok], r[0][1][0][ok], r[1][1][0][ok], 1e-30)
        check("gauss_act", f"{tag} d_scaling", grads[1].cpu()[ok], r[0][1][1][ok], r[1][1][1][ok], 1e-30)


def _stats_inputs(P, V, present, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    grads = [torch.randn(P, 3, device="cuda", generator=g) * 10.0 ** (v % 3 - 1) if present[v] else None for v in range(V)]
    radii = [torch.randint(0, 40, (P,), device="cuda", dtype=torch.int32, generator=g) *
             (torch.rand(P, device="cuda", generator=g) > 0.6).int() for _ in range(V)]
    return grads, radii


def _stats_check(group, P, V, present, seed):
    from csplat import train as tr
    grads, radii = _stats_inputs(P, V, present, seed)
    vsg, rmax, vis = tr.step_stats(grads, radii, P, torch.device("cuda"))
    gn = [None if t is None else t.cpu().numpy() for t in grads]
    rn = [t.cpu().numpy() for t in radii]
    s64, r, v = R.step_stats(gn, rn, np.float64)
    s32, _, _ = R.step_stats(gn, rn, np.float32)
    assert vis.dtype == torch.bool and rmax.dtype == torch.int32
    np.testing.assert_array_equal(rmax.cpu().numpy(), r)
    np.testing.assert_array_equal(vis.cpu().numpy(), v)
    gmax = max([float(np.abs(t).max()) for t in gn if t is not None] + [1e-30])
    check(group, f"P {P} V {V} present {''.join('x' if p else '-' for p in present)}", vsg, s64, s32, gmax)


@pytest.mark.parametrize("V", R.STATS_V)
@pytest.mark.parametrize("P", R.STATS_P)
def test_step_stats_views_missing_gradients_and_the_capped_grid(P, V):
    """csplat_step_stats with 1, 2 and 16 views, the gradient missing at view 0, at the last view, everywhere but one view, nowhere;
    from P = 349 526 the stride loop repeats"""
    patterns = {tuple([True] * V), tuple([False] + [True] * (V - 1)), tuple([True] * (V - 1) + [False]),
                tuple(v == V // 2 for v in range(V)), tuple([False] * V)}
    for j, present in enumerate(sorted(patterns)):
        _stats_check("step_stats", P, V, present, 100 * V + j)


@pytest.mark.allow_fallbacks("shape")
def test_step_stats_with_more_views_than_the_table_holds():
    from csplat import native
    before = native.FALLBACK_COUNTS[("train.step_stats", "shape")]
    _stats_check("step_stats 17 views", 1237, 17, tuple(v != 3 for v in range(17)), 5)
    assert native.FALLBACK_COUNTS[("train.step_stats", "shape")] == before + 1


def _gather(sources, kinds):
    n_, dev = _lib()
    n = len(sources)
    keep = [torch.from_numpy(s).to(dev) for s in sources]
    dst = torch.full((sum(s.size for s in sources) + 8,), -7, dtype=torch.int32, device=dev)
    pp = (C.c_void_p * n)(*[t.data_ptr() for t in keep])
    rc = n_.lib.csplat_gather_words(n_.stream_handle(dev), n, C.cast(pp, C.c_void_p), C.cast((C.c_int * n)(*kinds), C.c_void_p),
                                    C.cast((C.c_int * n)(*[s.size for s in sources]), C.c_void_p), n_.ptr(dst))
    torch.cuda.synchronize()
    return rc, dst.cpu().numpy()


def _words(kind, cnt, rng):
    if kind == 0:
        return rng.normal(size=cnt).astype(np.float32)
    if kind == 1:
        s = rng.integers(-(1 << 30), 1 << 30, cnt).astype(np.int32)
        edge = np.array([(1 << 24) - 1, (1 << 24) + 1, (1 << 24) + 3, -(1 << 24) - 1, (1 << 25) + 2, (1 << 25) + 6], np.int32)
        s[:min(cnt, 6)] = edge[:min(cnt, 6)]
        return s
    s = rng.integers(-(1 << 31), 1 << 31, cnt).astype(np.int32)
    nan = np.array([0x7FC00001, 0x7F800001, -1, 0x7FFFFFFF], np.int64).astype(np.int32)          # NaNs as floats
    s[:min(cnt, 4)] = nan[:min(cnt, 4)]
    return s


def test_gather_words_every_kind_bit_for_bit():
    """1 and 32 sources (33 are refused and nothing is written) of 1, 64, 65 and 200 words (one 64-thread workgroup strides over a
    source); kind 1 converts int32 to float32 with round-to-nearest-even (values 2^24 +- 1 and beyond), kind 2 copies bit patterns that
    are NaNs as floats; the line is compared as int32, and the words behind it stay"""
    rng = np.random.default_rng(0)
    lines = [([_words(kind, cnt, rng)], [kind]) for cnt in R.GATHER_COUNTS for kind in (0, 1, 2)]
    for n in (32, 33):
        kinds = [i % 3 for i in range(n)]
        lines.append(([_words(k, R.GATHER_COUNTS[(i // 3) % 4], rng) for i, k in enumerate(kinds)], kinds))
    for sources, kinds in lines:
        rc, got = _gather(sources, kinds)
        if len(sources) > 32:
            assert rc != 0 and (got == -7).all()
            continue
        assert rc == 0
        want = R.gather_words(sources, kinds)
        np.testing.assert_array_equal(got[:want.size], want, err_msg=f"{len(sources)} sources, kinds {kinds}")
        assert (got[want.size:] == -7).all()
