"""Plain torch / numpy restatement, on the CPU, of what the train-step kernels of csrc/csplat_image.hip and csrc/csplat_optim.hip
compute, for tests/test_train_kernels_cpu.py (which checks THIS file against the reference's goldens and against torch's float64 Adam)
and tests/test_train_kernels_gpu.py (which checks the kernels against this file in float64 and derives its bars from this file in
float32).  Written from the reference's formulas (utils/loss_utils.py, utils/image_utils.py, scene_reconstruction/train_utils.py,
scene_reconstruction/gaussian_model.py: cited per function) and from the Adam recurrence as torch.optim.Adam documents it; nothing is
imported from csplat.  Every function takes the dtype it computes in.

Also here, because both test files need them: the image case generators and the SIZE TABLES of the GPU file (a test without a GPU
checks that every size lies on the intended side of the launch constant it is meant to cross)."""
from math import exp

import numpy as np
import torch

F64, F32 = torch.float64, torch.float32


# ------------------------------------------------------------------------------------------------ the window and the SSIM
def window(dtype=F64):
    """utils/loss_utils.py:30-32 (`gaussian(11, 1.5)`): torch.Tensor([exp(.)]) / sum, both in FLOAT32; returned in `dtype`"""
    g = torch.Tensor([exp(-(x - 11 // 2) ** 2 / float(2 * 1.5 ** 2)) for x in range(11)])
    return (g / g.sum()).to(dtype)


def _pass(x, w, dim):
    """one zero-padded 11-tap pass along `dim` (-1 or -2): out[i] = sum_k w[k] x[i + k - 5]"""
    n = x.shape[dim]
    out = torch.zeros_like(x)
    for k in range(11):
        s = k - 5                                   # out[i] += w[k] * x[i + s] for 0 <= i + s < n
        lo, hi = max(0, -s), min(n, n - s)
        if hi > lo:
            out.narrow(dim, lo, hi - lo).add_(x.narrow(dim, lo + s, hi - lo), alpha=float(w[k]))
    return out


class _Blur(torch.autograd.Function):
    """utils/loss_utils.py:34-38, 47: conv2d with the 11 x 11 window (the outer product of window() with itself), padding 5, one group
    per plane -- as a horizontal and a vertical 11-tap pass, which is the same sum in exact arithmetic.  The window is symmetric and the
    padding zero, so the operator is its own adjoint: the backward is the same two passes (tests/test_train_kernels_cpu.py checks both
    statements against F.conv2d)."""

    @staticmethod
    def forward(ctx, x, w):
        ctx.w = w
        return _pass(_pass(x, w, -1), w, -2)

    @staticmethod
    def backward(ctx, g):
        return _pass(_pass(g.contiguous(), ctx.w, -2), ctx.w, -1), None


def blur(x, dtype=F64):
    return _Blur.apply(x.to(dtype), window(dtype))


def ssim_map(x, y, dtype=F64):
    """utils/loss_utils.py:46-62 (`_ssim`), every plane of x, y [..., H, W]"""
    x, y = x.to(dtype), y.to(dtype)
    mu1, mu2 = blur(x, dtype), blur(y, dtype)
    mu1_sq, mu2_sq, mu1_mu2 = mu1.pow(2), mu2.pow(2), mu1 * mu2
    sigma1_sq = blur(x * x, dtype) - mu1_sq
    sigma2_sq = blur(y * y, dtype) - mu2_sq
    sigma12 = blur(x * y, dtype) - mu1_mu2
    C1, C2 = 0.01 ** 2, 0.03 ** 2
    return ((2 * mu1_mu2 + C1) * (2 * sigma12 + C2)) / ((mu1_sq + mu2_sq + C1) * (sigma1_sq + sigma2_sq + C2))


def ssim(x, y, dtype=F64):
    """utils/loss_utils.py:66-67 (size_average)"""
    return ssim_map(x, y, dtype).mean()


def l1(x, y, mask=None, dtype=F64):
    """utils/loss_utils.py:20-23"""
    d = x.to(dtype) - y.to(dtype)
    return torch.abs(d if mask is None else d * mask.to(dtype)).mean()


def psnr(x, y, dtype=F64):
    """utils/image_utils.py:17-21: [B, 1], one value per image of the batch"""
    mse = ((x.to(dtype) - y.to(dtype)) ** 2).reshape(x.shape[0], -1).mean(1, keepdim=True)
    return 20 * torch.log10(1.0 / torch.sqrt(mse))


def image_loss(x, y, lam, mask=None, add=None, w_img=1.0, w_add=1.0, psnr_scale=1.0, dtype=F64):
    """scene_reconstruction/train_utils.py:50-74 (Ll1 + lambda_dssim * ssim_loss; masked: mean|(x - y) m| + lambda mean((1 - ssim_map) m))
    and :262-283 (the PSNR of the step's cameras, the sum with the regularisers) as the four outputs of csplat_image_loss_fwd:
        (w_img * image_loss + w_add * add, psnr_scale * sum_b PSNR_b, image_loss, Ll1)
    x [B,C,H,W] (or [C,H,W]) and `add` may require grad: the first output is differentiable towards both."""
    x4 = x if x.dim() == 4 else x.unsqueeze(0)
    y4 = y if y.dim() == 4 else y.unsqueeze(0)
    x4, y4 = x4.to(dtype), y4.to(dtype)
    ll1 = l1(x4, y4, mask, dtype)
    if mask is None:
        ssim_loss = 1.0 - ssim(x4, y4, dtype)
    else:
        ssim_loss = ((1.0 - ssim_map(x4, y4, dtype)) * mask.to(dtype)).mean()
    il = ll1 + lam * ssim_loss
    out0 = w_img * il if add is None else w_img * il + w_add * add.to(dtype)
    with torch.no_grad():
        ps = psnr_scale * psnr(x4, y4, dtype).sum()
    return out0, ps, il.detach(), ll1.detach()


# ------------------------------------------------------------------------------------------------ Adam
def adam_step(p, g, m, v, lr, beta1, beta2, eps, step, dtype=F64):
    """one update of torch.optim.Adam as its documentation states it (no weight decay, no amsgrad), t = `step` >= 1:
        m_t = beta1 m + (1 - beta1) g;  v_t = beta2 v + (1 - beta2) g^2;  mhat = m_t / (1 - beta1^t);  vhat = v_t / (1 - beta2^t)
        p_t = p - lr mhat / (sqrt(vhat) + eps)
    Tensors in `dtype`, the hyper-parameters (and their powers) are Python floats.  Returns (p_t, m_t, v_t)."""
    p, g, m, v = (t.to(dtype) for t in (p, g, m, v))
    m = beta1 * m + (1.0 - beta1) * g
    v = beta2 * v + (1.0 - beta2) * (g * g)
    mhat = m / (1.0 - beta1 ** step)
    vhat = v / (1.0 - beta2 ** step)
    return p - lr * mhat / (torch.sqrt(vhat) + eps), m, v


def adam_run(params, grads_of, n_steps, lrs, beta1, beta2, eps, dtype=F64, state=None):
    """n_steps updates of every tensor: grads_of(it, k) -> the gradient of tensor k at step `it` (0-based) or None = the tensor is
    skipped at that step (torch: no update, its own step count does not advance).  state: per tensor (step, m, v) to start from.
    Returns (params, state)."""
    ps = [p.to(dtype).clone() for p in params]
    st = [(0, torch.zeros_like(p), torch.zeros_like(p)) for p in ps] if state is None else \
        [(int(s), m.to(dtype).clone(), v.to(dtype).clone()) for s, m, v in state]
    for it in range(n_steps):
        for k in range(len(ps)):
            g = grads_of(it, k)
            if g is None:
                continue
            s, m, v = st[k]
            ps[k], m, v = adam_step(ps[k], g, m, v, lrs[k], beta1, beta2, eps, s + 1, dtype)
            st[k] = (s + 1, m, v)
    return ps, st


# ------------------------------------------------------------------------------------------------ store and bookkeeping (numpy)
def mask_to_map(mask, base):
    """the stable compaction map of csplat_mask_to_map (gaussian_model.py:266-341 keeps `tensor[mask]`, i.e. the kept rows in order):
    map[i] = base + (number of kept rows before i) for a kept row, -1 otherwise; any non-zero byte keeps.  -> (map int32, count)"""
    keep = np.asarray(mask) != 0
    rank = np.cumsum(keep, dtype=np.int64) - 1
    return np.where(keep, rank + base, -1).astype(np.int32), int(keep.sum())


def rows_scatter(srcs, dsts, row_map):
    """dst[map[i]] = src[i] for every row with map[i] >= 0 (src None: the row is zero-filled); other rows of dst stay.  In place."""
    row_map = np.asarray(row_map)
    keep = row_map >= 0
    for s, d in zip(srcs, dsts):
        d[row_map[keep]] = 0 if s is None else s[keep]
    return dsts


def gauss_act(op_raw, sc_raw, f_dc, f_rest, dtype=F64):
    """gaussian_model.py:96-121: get_opacity = sigmoid(_opacity), get_scaling = exp(_scaling), get_features = cat(dc, rest) along dim 1.
    The adjoint comes from autograd on these three expressions."""
    return torch.sigmoid(op_raw.to(dtype)), torch.exp(sc_raw.to(dtype)), torch.cat((f_dc.to(dtype), f_rest.to(dtype)), dim=1)


def gauss_act_adjoint(raw, weights, dtype=F64):
    """d/d raw of sum_k <out_k, w_k> over the outputs whose weight is not None -> four arrays (zeros where nothing flows)"""
    a = [t.detach().to(dtype).clone().requires_grad_() for t in raw]
    out = gauss_act(*a, dtype=dtype)
    terms = [(o * w.to(dtype)).sum() for o, w in zip(out, weights) if w is not None]
    if terms:
        sum(terms).backward()
    return [t.grad if t.grad is not None else torch.zeros_like(t) for t in a]


def step_stats(grads, radii, dtype=np.float64):
    """train_utils.py:276-285: the views' screen-space gradients summed in view order in `dtype`, radii = max over the views,
    visible = any radius > 0.  grads: list of [P,3] arrays or None (no gradient for that view: counts as zero)."""
    P = radii[0].shape[0]
    s = np.zeros((P, 3), dtype)
    for g in grads:
        if g is not None:
            s = (s + np.asarray(g, dtype)).astype(dtype)
    r = np.stack(radii).max(0).astype(np.int32)
    return s, r, r > 0


def gather_words(sources, kinds):
    """the packed log line of csplat_gather_words as int32 BIT PATTERNS: kind 0 float32 copied, kind 1 int32 converted to float32
    (round to nearest even, numpy's astype), kind 2 int32 copied bit for bit"""
    out = []
    for s, k in zip(sources, kinds):
        s = np.asarray(s)
        if k == 1:
            out.append(s.astype(np.int32).astype(np.float32).view(np.int32))
        else:
            out.append(s.view(np.int32))
    return np.concatenate(out)


# ------------------------------------------------------------------------------------------------ image cases
def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))


def _grid(H, W):
    return np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")


def make_mask(shape, mask_channels, seed):
    """ones and zeros in blocks, with values from [0.25, 1] mixed in; [B, mask_channels, H, W] (mask_channels 1 or C).  Every image
    gets at least one zero and one non-zero (images of one pixel cannot: the masked cases use none)."""
    B, C, H, W = shape
    rng = np.random.default_rng(seed)
    m = np.ones((B, mask_channels, H, W))
    yy, xx = _grid(H, W)
    for b in range(B):
        for c in range(mask_channels):
            cy, cx = rng.uniform(0, H), rng.uniform(0, W)
            m[b, c][((yy - cy) / max(H / 3.0, 1)) ** 2 + ((xx - cx) / max(W / 3.0, 1)) ** 2 < 1] = 0.0      # a hole
            soft = rng.random((H, W)) < 0.15
            m[b, c][soft] = rng.uniform(0.25, 1.0, size=int(soft.sum()))
        flat = m[b].reshape(-1)
        flat[rng.integers(0, flat.size // 2) if flat.size > 1 else 0] = 0.0
        flat[flat.size // 2 + rng.integers(0, flat.size - flat.size // 2)] = 1.0
    return _t(m)


def case_uniform(shape, seed=0):
    """what the existing tests use: x uniform, y = clamp(x + 0.15 noise)"""
    rng = np.random.default_rng(seed)
    x = rng.random(shape)
    y = np.clip(x + 0.15 * rng.normal(size=shape), 0, 1)
    return _t(x), _t(y)


def case_saturated(shape, seed=0):
    """x = y = 1 outside a disc; noisy inside; clamped to [0, 1] -- so there are exact ties x == y (outside, and where both clamp)"""
    B, C, H, W = shape
    rng = np.random.default_rng(seed)
    yy, xx = _grid(H, W)
    inside = (((yy - H / 2.0) / max(H / 3.0, 0.6)) ** 2 + ((xx - W / 2.0) / max(W / 3.0, 0.6)) ** 2 < 1)[None, None]
    y = np.where(inside, 0.6 + 0.5 * rng.normal(size=shape), 1.0)
    x = np.where(inside, y + 0.1 * rng.normal(size=shape), 1.0)
    return _t(np.clip(x, 0, 1)), _t(np.clip(y, 0, 1))


def case_equal(shape, seed=0):
    x = _t(np.random.default_rng(seed).random(shape))
    return x, x.clone()


def case_dark(shape, seed=0):
    rng = np.random.default_rng(seed)
    return _t(1e-3 * rng.random(shape)), _t(1e-3 * rng.random(shape))


def case_quantised(shape, seed=0):
    """what a training pair looks like: the target a smooth shaded, textured shape on a background of exactly 0 or exactly 1 (by image),
    rounded to k / 255 as a PNG delivers it; the rendered image = the target + a smooth error of a few 1/255, clamped"""
    B, C, H, W = shape
    rng = np.random.default_rng(seed)
    yy, xx = _grid(H, W)
    y = np.empty(shape)
    x = np.empty(shape)
    for b in range(B):
        bg = float(b % 2)
        cy, cx = H * rng.uniform(0.35, 0.65), W * rng.uniform(0.35, 0.65)
        shape_in = ((yy - cy) / max(0.33 * H, 0.6)) ** 2 + ((xx - cx) / max(0.28 * W, 0.6)) ** 2 < 1
        for c in range(C):
            shade = 0.55 + 0.3 * np.sin(yy / 37.0 + 0.7 * c + b) * np.cos(xx / 29.0 - 0.3 * c)
            texture = 0.06 * np.sin(yy * 1.3 + xx * 0.9 + c) + 0.03 * rng.normal(size=(H, W))
            y[b, c] = np.round(np.clip(np.where(shape_in, shade + texture, bg), 0, 1) * 255.0) / 255.0
            err = (3.0 / 255.0) * np.sin(yy / 11.0 + b + c) * np.cos(xx / 13.0 + 2 * c) + (1.0 / 255.0) * np.sin(xx / 3.0 + yy / 5.0)
            x[b, c] = np.clip(y[b, c] + err, 0, 1)
    return _t(x), _t(y)


CASES = {"uniform": case_uniform, "saturated": case_saturated, "equal": case_equal, "dark": case_dark, "quantised": case_quantised}


def image_case(kind, shape, mask_channels=0, seed=0):
    """(x, y, mask): float32 CPU tensors; mask None (mask_channels 0) or [B, mask_channels, H, W]"""
    x, y = CASES[kind](tuple(shape), seed)
    return x, y, (make_mask(shape, mask_channels, seed + 1) if mask_channels else None)


# ------------------------------------------------------------------------------------------------ the GPU file's size tables
# Every "production" entry is there to cross one launch constant of the .hip files; tests/test_train_kernels_cpu.py restates those
# constants and asserts the side each entry lies on.
IMAGE_SMALL = [(1, 1, 1, 1), (1, 3, 1, 11), (3, 1, 5, 3), (1, 3, 5, 64), (1, 1, 15, 10), (3, 3, 15, 65), (1, 3, 16, 63), (1, 1, 16, 64),
               (1, 1, 17, 1), (3, 3, 17, 129), (1, 3, 33, 10), (1, 1, 33, 65), (1, 1, 17, 64), (3, 3, 33, 129)]
IMAGE_PRODUCTION = [(4, 3, 800, 800), (4, 3, 801, 803), (1, 3, 1600, 1300)]
IMAGE_PARTIALS_MOD4 = {1: (1, 1, 16, 64), 2: (1, 1, 17, 64), 3: (1, 3, 16, 63), 81: (3, 3, 33, 129)}     # partial count -> shape
IMAGE_MAX_PLANES = (21845, 3, 16, 8)            # 65 535 planes: the most one launch carries
IMAGE_OVER_PLANES = (65536, 1, 16, 8)           # one more: the wrappers split it
IMAGE_OVER_PLANES_MAP = (13108, 1, 16, 8)       # the return_map form stacks 5 x the planes through the blur: 65 540
# (kind, shape, mask_channels, with_add): FusedImageLoss
IMAGE_LOSS_CASES = [("uniform", (3, 3, 33, 129), 0, False), ("uniform", (4, 3, 800, 800), 0, True), ("uniform", (1, 3, 16, 63), 3, True),
                    ("saturated", (3, 3, 17, 129), 1, False), ("saturated", (1, 3, 33, 10), 0, False), ("saturated", (4, 3, 800, 800), 1, True),
                    ("equal", (1, 3, 5, 64), 0, False), ("equal", (3, 3, 15, 65), 3, True), ("equal", (1, 3, 1600, 1300), 0, False),
                    ("dark", (1, 1, 33, 65), 1, False), ("dark", (3, 1, 5, 3), 0, True), ("dark", (4, 3, 801, 803), 3, False),
                    ("quantised", (3, 3, 33, 129), 1, True), ("quantised", (1, 3, 1600, 1300), 1, False), ("quantised", (4, 3, 801, 803), 0, False)]
# the C-ABI surface of the SSIM that no Python wrapper calls (csplat_ssim_fwd_masked, map_out, addend): a single pixel, narrower and shorter
# than the window, one tile minus a column, a second tile row of one line, 3 x 2 ragged tiles on 9 planes
SSIM_ABI_SHAPES = [(1, 1, 1, 1), (3, 1, 5, 3), (1, 3, 16, 63), (1, 1, 17, 64), (3, 3, 17, 129)]
L1_SIZES = [1, 3, 4, 5, 4097, 3_145_728, 3_145_732, 7_680_000, 7_680_003]
L1_MASKED = [((4, 3, 800, 800), 1), ((4, 3, 800, 800), 3), ((4, 3, 801, 803), 1), ((4, 3, 801, 803), 3), ((3, 3, 37, 53), 1)]
L1_SLICE = ((3, 3, 37, 53), 1)                  # l1_loss(img[i], gt[i]): 3 * 37 * 53 = 5883 floats per image, not a multiple of 4

ADAM_SIZES = [1, 3, 4, 5, 1023, 1025, 4097, 8_388_608, 8_388_613, 9_000_000]
ADAM_LONG_SHORT = (9_000_000, 7)
ADAM_MANY = [49, 97]
ADAM_STEPS = [1, 2, 10, 1000, 30_000]
ADAM_BETAS = [(0.9, 0.999), (0.5, 0.9)]
ADAM_EPS = [1e-15, 1e-8]

MAP_SIZES = [1, 2047, 2048, 2049, 4096, 4097, 1_000_001, 8_388_608, 8_388_609, 8_392_705]
MAP_BASES = [0, 11, 1 << 30]
SCATTER_ROWS = [100_000, 250_000]
SCATTER_WIDTHS = [1, 3, 4, 45, 48]
ACT_P = [1, 43_690, 43_691, 100_000, 500_000]
STATS_P = [1, 349_525, 349_526, 500_000]
STATS_V = [1, 2, 16]
GATHER_COUNTS = [1, 64, 65, 200]


def image_partials(shape):
    """workgroup partials of one of the three sums of csplat_image_loss_fwd: one per 64 x 16 tile and plane"""
    B, C, H, W = shape
    return B * C * ((H + 15) // 16) * ((W + 63) // 64)
