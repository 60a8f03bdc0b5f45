"""tests/train_kernels_ref.py is what tests/test_train_kernels_gpu.py holds the train-step kernels to, so it is checked here first,
without a GPU: against fixtures produced by RUNNING THE REFERENCE (tests/golden/losses.npz, float32 runs; the bars are the ones
tests/test_reference_goldens_cpu.py uses for the same quantities), against torch.optim.Adam on float64 tensors, and against F.conv2d with
the 11 x 11 window.  Then the preconditions of the GPU file's cases: they are conditions on the inputs, not measurements of any kernel."""
import numpy as np
import pytest

import util  # noqa: F401
import train_kernels_ref as R
from util import golden

torch = pytest.importorskip("torch")
F64 = torch.float64


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-30))


# ------------------------------------------------------------------------------------------------ against the reference's own run
def test_losses_match_the_reference_run():
    g = golden("losses.npz")
    img, gt, mask = (torch.tensor(g[k]) for k in ("img", "gt", "mask"))
    for tag, mk in (("plain", None), ("masked", mask)):
        x = img.double().requires_grad_(True)
        v = R.l1(x, gt, mk)
        v.backward()
        assert abs(float(v.detach()) - float(g[f"{tag}.l1"])) < 1e-7
        assert _rel(x.grad.numpy(), g[f"{tag}.l1_grad"]) < 1e-6
        x = img.double().requires_grad_(True)
        out0, ps, il, ll1 = R.image_loss(x, gt, 0.05, mk)
        out0.backward()
        assert abs(float(out0.detach()) - float(g[f"{tag}.loss"])) < 1e-6 and float(il) == float(out0.detach())
        assert abs(float(ll1) - float(g[f"{tag}.l1"])) < 1e-7
        assert abs((float(il) - float(ll1)) / 0.05 - float(g[f"{tag}.ssim_loss"])) < 1e-6
        assert _rel(x.grad.numpy(), g[f"{tag}.loss_grad"]) < 1e-4
    x = img.double().requires_grad_(True)
    s = R.ssim(x, gt)
    s.backward()
    assert abs(float(s.detach()) - float(g["ssim"])) < 1e-6
    assert _rel(x.grad.numpy(), g["ssim_grad"]) < 1e-4
    assert _rel(R.ssim_map(img, gt).numpy(), g["ssim_map"]) < 1e-4
    assert _rel(R.ssim_map(img, gt).mean((1, 2, 3)).numpy(), g["ssim_per_image"]) < 1e-5


def test_image_loss_weights_add_and_psnr():
    """the side outputs are what their definitions say: out0 = w_img * image_loss + w_add * add with the gradients w_img * d image_loss
    and w_add; the PSNR is the reference's expression per image, summed and scaled, and inf for an image that equals its target"""
    x, y, mask = R.image_case("uniform", (3, 3, 20, 30), 1, seed=2)
    y[1] = x[1]
    a = x.double().requires_grad_(True)
    add = torch.tensor(0.37, dtype=F64, requires_grad=True)
    out0, ps, il, ll1 = R.image_loss(a, y, 0.2, mask, add, 2.0 / 3.0, 0.5, 1.0 / 3.0)
    (1.7 * out0).backward()
    b = x.double().requires_grad_(True)
    plain = R.image_loss(b, y, 0.2, mask)[0]
    plain.backward()
    assert abs(float(out0.detach()) - (2.0 / 3.0 * float(plain.detach()) + 0.5 * 0.37)) < 1e-15
    assert _rel(a.grad.numpy(), 1.7 * 2.0 / 3.0 * b.grad.numpy()) < 1e-14 and abs(float(add.grad) - 1.7 * 0.5) < 1e-15
    p = R.psnr(x, y)
    assert p.shape == (3, 1) and torch.isinf(p[1]) and p[1] > 0 and torch.isfinite(p[0]) and torch.isfinite(p[2])
    want0 = 20 * np.log10(1.0 / np.sqrt(((x[0].double() - y[0].double()) ** 2).mean().item()))
    assert abs(float(p[0]) - want0) < 1e-12 and torch.isinf(ps)


# ------------------------------------------------------------------------------------------------ the window
@pytest.mark.parametrize("shape", [(2, 3, 37, 53), (1, 1, 1, 1), (1, 2, 5, 3), (2, 1, 10, 40), (1, 3, 40, 7), (1, 1, 11, 11), (3, 1, 1, 30)])
def test_separable_blur_is_the_grouped_conv2d(shape):
    """two 11-tap passes == F.conv2d with the 11 x 11 window built as utils/loss_utils.py:34-38 builds it (float32 outer product), zero
    padding 5, one group per channel -- values and the gradient (the adjoint), H or W below the window included.  The 2-D window is the
    float32-ROUNDED outer product, the passes use the exact one: they agree to float32 rounding of the window entries (1e-7), not to 1e-16."""
    import torch.nn.functional as F
    c = shape[1]
    w1 = R.window(torch.float32).unsqueeze(1)
    w2 = w1.mm(w1.t()).double().unsqueeze(0).unsqueeze(0).expand(c, 1, 11, 11).contiguous()
    w2_exact = (R.window(F64).unsqueeze(1) @ R.window(F64).unsqueeze(0)).unsqueeze(0).unsqueeze(0).expand(c, 1, 11, 11).contiguous()
    gen = torch.Generator().manual_seed(sum(shape))
    x = torch.rand(*shape, generator=gen, dtype=F64)
    wgt = torch.rand(*shape, generator=gen, dtype=F64)
    for w, bar in ((w2, 2e-7), (w2_exact, 1e-14)):
        a = x.clone().requires_grad_(True)
        ref = F.conv2d(a, w, padding=5, groups=c)
        (ref * wgt).sum().backward()
        b = x.clone().requires_grad_(True)
        got = R.blur(b)
        (got * wgt).sum().backward()
        assert float((got.detach() - ref.detach()).abs().max()) <= bar * float(ref.detach().abs().max())
        assert float((b.grad - a.grad).abs().max()) <= bar * float(a.grad.abs().max())
    assert R.blur(x.float(), torch.float32).dtype == torch.float32


# ------------------------------------------------------------------------------------------------ Adam
@pytest.mark.parametrize("n_steps", [1, 6, 1000])
@pytest.mark.parametrize("eps", R.ADAM_EPS)
@pytest.mark.parametrize("betas", R.ADAM_BETAS)
def test_adam_run_is_torch_adam_in_float64(n_steps, eps, betas):
    """the documented recurrence == torch.optim.Adam on float64 CPU tensors, to 1e-12 relative: parameters and both moments, with a
    tensor that gets no gradient on every second step (its own step count then lags)"""
    gen = torch.Generator().manual_seed(n_steps)
    shapes, lrs = [(40, 3), (7,), (5, 2)], [1.6e-4, 0.05, 1e-3]
    init = [torch.randn(*s, generator=gen, dtype=F64) for s in shapes]
    init[0][:10] = 0.0
    grads = [[torch.randn(*s, generator=gen, dtype=F64) * 10.0 ** (k - 1) for k, s in enumerate(shapes)] for _ in range(8)]
    grads_of = lambda it, k: None if (k == 1 and it % 2 == 0) else grads[it % 8][k]  # noqa: E731
    ps = [torch.nn.Parameter(t.clone()) for t in init]
    opt = torch.optim.Adam([{"params": [p], "lr": lr} for p, lr in zip(ps, lrs)], lr=0.0, betas=betas, eps=eps)
    for it in range(n_steps):
        for k, p in enumerate(ps):
            g = grads_of(it, k)
            p.grad = None if g is None else g.clone()
        opt.step()
    got, st = R.adam_run(init, grads_of, n_steps, lrs, betas[0], betas[1], eps)
    for k, (p, q) in enumerate(zip(ps, got)):
        assert _rel(q.numpy(), p.detach().numpy()) < 1e-12, k
        if p in opt.state and opt.state[p]:
            assert int(opt.state[p]["step"]) == st[k][0]
            assert _rel(st[k][1].numpy(), opt.state[p]["exp_avg"].numpy()) < 1e-12
            assert _rel(st[k][2].numpy(), opt.state[p]["exp_avg_sq"].numpy()) < 1e-12
        else:
            assert st[k][0] == 0


# ------------------------------------------------------------------------------------------------ store and bookkeeping
def test_bookkeeping_restatements_on_hand_made_inputs():
    mp, cnt = R.mask_to_map(np.array([0, 2, 0, 255, 1], np.uint8), 11)
    assert mp.tolist() == [-1, 11, -1, 12, 13] and cnt == 3 and mp.dtype == np.int32
    assert R.mask_to_map(np.zeros(4, np.uint8), 5)[0].tolist() == [-1] * 4
    src = np.arange(10, dtype=np.float32).reshape(5, 2)
    dst = np.full((4, 2), 7, np.float32)
    zf = np.full((4, 1), 7, np.float32)
    R.rows_scatter([src, None], [dst, zf], np.array([-1, 0, -1, 1, 2]))
    assert dst.tolist() == [[2, 3], [6, 7], [8, 9], [7, 7]] and zf[:, 0].tolist() == [0, 0, 0, 7]
    s, r, vis = R.step_stats([None, np.ones((2, 3)), 2 * np.ones((2, 3))], [np.array([0, 3]), np.array([0, 1]), np.array([0, 2])])
    assert s.tolist() == [[3.0] * 3] * 2 and r.tolist() == [0, 3] and vis.tolist() == [False, True]
    words = R.gather_words([np.array([1.5], np.float32), np.array([(1 << 24) + 1, (1 << 24) + 3], np.int32), np.array([-1, 0x7FC00001], np.int32)],
                           [0, 1, 2])
    assert words.view(np.float32)[0] == 1.5 and words.view(np.float32)[1:3].tolist() == [float(1 << 24), float((1 << 24) + 4)]
    assert words[3:].tolist() == [-1, 0x7FC00001]
    raw = [torch.tensor([[0.0]]), torch.tensor([[0.0, 1.0, -1.0]]), torch.ones(1, 1, 3), 2 * torch.ones(1, 15, 3)]
    o, s_, f = R.gauss_act(*raw)
    assert float(o) == 0.5 and f.shape == (1, 16, 3) and float(f[0, 0, 0]) == 1.0 and float(f[0, 1, 0]) == 2.0
    d = R.gauss_act_adjoint(raw, [torch.ones(1, 1), None, torch.ones(1, 16, 3)])
    assert float(d[0]) == 0.25 and float(d[1].abs().max()) == 0.0 and float(d[2].min()) == 1.0 and float(d[3].min()) == 1.0


# ------------------------------------------------------------------------------------------------ preconditions of the GPU file's cases
def test_image_cases_have_the_properties_they_are_there_for():
    shape = (3, 3, 40, 70)
    x, y, _ = R.image_case("saturated", shape)
    ties = (x == y)
    assert 0.2 < float(ties.float().mean()) < 0.95                       # exact ties, and not only ties
    assert float(((x == 1.0) & (y == 1.0)).float().mean()) > 0.2 and float(x.min()) >= 0.0 and float(x.max()) <= 1.0
    x, y, _ = R.image_case("equal", shape)
    assert torch.equal(x, y)
    x, y, _ = R.image_case("dark", shape)
    assert float(x.max()) <= 1e-3 and float(y.max()) <= 1e-3 and not torch.equal(x, y)
    x, y, _ = R.image_case("quantised", shape)
    assert torch.equal(torch.round(y * 255.0) / 255.0, y)                # a PNG's values
    bg = [float(y[b, :, 0, 0].max()) for b in range(3)]
    assert bg == [0.0, 1.0, 0.0] and float((y[0] == 0).float().mean()) > 0.3 and float((y[1] == 1).float().mean()) > 0.3
    assert 0 < float((x - y).abs().max()) <= 4.5 / 255.0 and float(x.min()) >= 0.0 and float(x.max()) <= 1.0
    assert 0.02 < float(((y > 0) & (y < 1)).float().mean())              # the shape itself


def _masked_cases():
    for kind, shape, mc, _ in R.IMAGE_LOSS_CASES:
        if mc:
            yield kind, shape, (shape[1] if mc == 3 else 1)
    for shape, mc in R.L1_MASKED:
        yield "uniform", shape, mc


def test_every_mask_has_zeros_and_non_zeros_in_every_image():
    seen = set()
    for kind, shape, mc in _masked_cases():
        if (shape, mc) in seen:
            continue
        seen.add((shape, mc))
        m = R.make_mask(shape, mc, seed=1)
        assert m.shape == (shape[0], mc, shape[2], shape[3]) and m.dtype == torch.float32
        for b in range(shape[0]):
            assert bool((m[b] == 0).any()) and bool((m[b] != 0).any()), (shape, mc, b)
        mid = (m > 0) & (m < 1)
        assert float(m.min()) == 0.0 and float(m.max()) == 1.0 and (not mid.any() or float(m[mid].min()) >= 0.25)
        assert shape[2] * shape[3] < 50 or bool(mid.any())
    assert {mc for _, mc in seen} >= {1, 3}                              # both layouts, [B,1,H,W] and [B,C,H,W]


def test_sizes_lie_on_the_intended_side_of_the_launch_constants():
    """The constants are restated here next to the .hip line they come from; if one is retuned, the assertion that names the moved case
    fails, and the size table in tests/train_kernels_ref.py follows the kernel."""
    # ---- csplat_image.hip, k_image_loss_finish::block_sum: `for (; i + 3 * SSIM_THREADS < n4; i += 4 * SSIM_THREADS)`, SSIM_THREADS = 512
    SSIM_THREADS = 512
    unrolled = lambda n_partials: (n_partials - 3) // 4 > 3 * SSIM_THREADS      # (<= 3 elements may sit in front of the float4 body)  # noqa: E731
    assert [unrolled(R.image_partials(s)) for s in R.IMAGE_PRODUCTION] == [True, True, True]
    assert R.image_partials((4, 3, 800, 800)) == 7800
    B, C, H, W = R.IMAGE_PRODUCTION[2]
    assert B == 1 and unrolled(R.image_partials((1, C, H, W)))                   # ... inside ONE image's PSNR range [b C per_plane, (b+1) C per_plane)
    assert not any(unrolled(R.image_partials(s)) for s in R.IMAGE_SMALL)
    for k, s in R.IMAGE_PARTIALS_MOD4.items():                                   # the 2nd / 3rd partial arrays start off a 16-byte boundary
        assert R.image_partials(s) == k
    assert sorted(k % 4 for k in R.IMAGE_PARTIALS_MOD4) == [1, 1, 2, 3]
    # ---- tiles: BW = 64, BH = 16, the 11-tap window (csplat_image.hip: `constexpr int BW = 64, BH = 16, R5 = 5`)
    hs, ws = {s[2] for s in R.IMAGE_SMALL}, {s[3] for s in R.IMAGE_SMALL}
    assert hs >= {1, 5, 15, 16, 17, 33} and ws >= {1, 3, 10, 11, 63, 64, 65, 129} and len(R.IMAGE_SMALL) >= 12
    assert {s[1] for s in R.IMAGE_SMALL} == {1, 3} and {s[0] for s in R.IMAGE_SMALL} == {1, 3}
    # ---- planes: `CSPLAT_REQUIRE(n_images < 65536, ...)` in csplat_blur11 / ssim_fwd_launch / csplat_image_loss_fwd (blockIdx.z)
    planes = lambda s: s[0] * s[1]  # noqa: E731
    assert planes(R.IMAGE_MAX_PLANES) == 65535 and planes(R.IMAGE_OVER_PLANES) == 65536
    assert 5 * planes(R.IMAGE_OVER_PLANES_MAP) >= 65536 > 5 * (planes(R.IMAGE_OVER_PLANES_MAP) - 1)
    # ---- k_l1: `constexpr int L1_BLOCKS = 256, L1_THREADS = 1024`, `for (; i + 3 * stride < n4; i += 4 * stride)`, stride = grid * L1_THREADS
    L1_BLOCKS, L1_THREADS = 256, 1024
    four_in_flight = lambda n: n // 4 > 3 * L1_BLOCKS * L1_THREADS  # noqa: E731
    assert [four_in_flight(n) for n in R.L1_SIZES] == [False] * 5 + [False, True, True, True]
    assert R.L1_SIZES[5] // 4 == 3 * L1_BLOCKS * L1_THREADS                      # the last size the loop does not take
    assert {n % 4 for n in R.L1_SIZES[5:]} == {0, 3}
    assert {(s[2] * s[3]) % 4 for s, _ in R.L1_MASKED} == {0, 1, 3}              # `n4 = (mask && (hw & 3)) ? 0 : n >> 2` (801 * 803 = 3 mod 4)
    s, i = R.L1_SLICE
    assert (i * s[1] * s[2] * s[3] * 4) % 16 != 0                                # the slice starts off a 16-byte boundary
    # ---- csplat_optim.hip, csplat_adam_step: `want = (longest + 4095) / 4096; grid = min(want, 2048)`, 256 threads x float4
    capped = lambda n: (n + 4095) // 4096 > 2048  # noqa: E731
    assert [capped(n) for n in R.ADAM_SIZES] == [False] * 7 + [False, True, True] and R.ADAM_SIZES[7] == 2048 * 4096
    assert capped(R.ADAM_LONG_SHORT[0]) and R.ADAM_LONG_SHORT[1] < 256           # k_adam_dev: `if (blockIdx.x * 256 >= units) return`
    ADAM_MAX_TENSORS = 48                                                        # include/csplat.h: CSPLAT_ADAM_MAX_TENSORS
    assert [(n - 1) // ADAM_MAX_TENSORS for n in R.ADAM_MANY] == [1, 2]          # a second and a third table
    assert {n % 4 for n in R.ADAM_SIZES} == {0, 1, 3} and {1023, 1025} <= set(R.ADAM_SIZES)     # the scalar tail of adam_span
    # ---- csplat_sort.hip: `SCAN_TILE = 2048`; k_scan_single: `for (base = 0; base < m; base += 4096)` over the m = ceil(n / SCAN_TILE) block sums
    SCAN_TILE, SWEEP = 2048, 4096
    second_sweep = lambda n: -(-n // SCAN_TILE) > SWEEP  # noqa: E731
    assert [second_sweep(n) for n in R.MAP_SIZES] == [False] * 7 + [False, True, True] and R.MAP_SIZES[7] == SCAN_TILE * SWEEP
    assert {2047, 2048, 2049, 4096, 4097} <= set(R.MAP_SIZES)
    # ---- k_rows_scatter: `want = (longest * n_rows + 1023) / 1024; grid = min(want, 4096)`
    assert all((max(R.SCATTER_WIDTHS) * n + 1023) // 1024 > 4096 for n in R.SCATTER_ROWS) and 45 * 100_000 > 4096 * 1024
    # ---- k_gauss_act_fwd / _bwd: `want = cdiv(P * 48, 256); grid = min(want, 8192)`
    strided = lambda P: -(-P * 48 // 256) > 8192  # noqa: E731
    assert [strided(P) for P in R.ACT_P] == [False, False, True, True, True]
    # ---- k_step_stats: `work = (3 * P + 255) / 256; grid = min(work, 4096)`, `STATS_MAX_VIEWS = 16`
    strided = lambda P: (3 * P + 255) // 256 > 4096  # noqa: E731
    assert [strided(P) for P in R.STATS_P] == [False, False, True, True] and max(R.STATS_V) == 16
    # ---- k_gather_words: `<<<1, 64>>>`, `struct WordsTable { const void *src[32]; ...`
    assert {c > 64 for c in R.GATHER_COUNTS} == {False, True} and {64, 65} <= set(R.GATHER_COUNTS)
