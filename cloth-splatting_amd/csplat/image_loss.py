"""The image loss of the train step (train_utils.py:50-74, utils/loss_utils.py:20-70, utils/image_utils.py:17-21): L1, SSIM and PSNR as
fused HIP launches with their autograd nodes, FusedImageLoss (L1 + lambda_dssim * (1 - SSIM) + PSNR + the sum with the regularisers as
one node) and the composed torch forms they fall back to.  The scratch caches here are registered in native.TICKET_CACHES.  Every
name is re-exported by csplat.train."""
from math import exp

import ctypes as C

import torch
import torch.nn.functional as F
from torch.autograd.function import once_differentiable

from . import native as _n


def _mask_layout(x, mask):
    """(n_batch, channels, H*W, mask_channels) when `mask` is a [B,1,H,W] / [B,C,H,W] fp32 GPU companion of the image batch
    x [B,C,H,W] (train_utils.py:256-285 stacks Camera.mask [1,H,W] per view), else None (composed torch ops are used)."""
    if mask is None or x.dim() != 4 or mask.dim() != 4 or not mask.is_cuda or mask.dtype != torch.float32 or mask.requires_grad:
        return None
    B, Cc, H, W = x.shape
    if tuple(mask.shape) not in ((B, 1, H, W), (B, Cc, H, W)):
        return None
    return B, Cc, H * W, int(mask.shape[1])


def l1_loss(network_output, gt, mask=None):
    """utils/loss_utils.py:20-23.  fp32 GPU images go through the fused HIP kernel (loss + gradient, one pass)."""
    ok = network_output.is_cuda and network_output.dtype == torch.float32 and gt.dtype == torch.float32 and \
        network_output.shape == gt.shape and network_output.numel() > 0
    if mask is not None:
        if ok and _mask_layout(network_output, mask) is not None:
            return FusedL1.apply(network_output, gt, mask)
        _n.composed_fallback("train.l1_loss", "dtype" if not ok and network_output.shape == gt.shape else "shape", network_output)
        return torch.abs((network_output - gt) * mask).mean()
    if ok:
        return FusedL1.apply(network_output, gt)
    _n.composed_fallback("train.l1_loss", "dtype" if network_output.shape == gt.shape and network_output.numel() else "shape", network_output)
    return torch.abs(network_output - gt).mean()

_TAPS = {}


def _taps(window_size=11, sigma=1.5):
    """the reference's float32 window (loss_utils.py:30-32): torch.Tensor([exp(.)]) / sum, both in float32"""
    if window_size not in _TAPS:
        g = torch.tensor([exp(-(x - window_size // 2) ** 2 / float(2 * sigma ** 2)) for x in range(window_size)])
        g = g / g.sum()
        _TAPS[window_size] = (C.c_float * window_size)(*[float(v) for v in g])
    return _TAPS[window_size]


# workgroup partial sums of csplat_l1 for the stream the work runs on (launches on one stream cannot overlap): one buffer per stream
# instead of an allocation per loss.  (Rounds 1-4 kept a ticket counter here too; since round 5 a second one-workgroup launch sums the
# partials -- the ticket's device-scope release cost ~10 us of L2 write-back per call, csrc/csplat_image.hip.)
_L1_SCRATCH = _n.ScratchCache()


class FusedL1(torch.autograd.Function):
    """mean |a - b| (mean |(a - b) * mask| with a mask).  Forward: csplat_l1_signs -- the loss and ONE BYTE per element
    (sign((a - b) m)); backward: csplat_l1_signs_bwd writes g * sign * m / n in one pass (g = the incoming gradient, read on the
    device).  The reference's l1_loss is three elementwise launches each way (utils/loss_utils.py:20-23)."""

    @staticmethod
    def forward(ctx, a, b, mask=None):
        _n.require_cuda(a)
        # (asked of the ARGUMENTS: grad mode is off in here, so the copy .contiguous() makes of a strided image requires no gradient)
        need = ctx.needs_input_grad[0] or ctx.needs_input_grad[1]
        a, b = a.contiguous(), b.contiguous()
        mask = None if mask is None else mask.contiguous()
        scratch = _L1_SCRATCH.buffer(a.device, (), _n.lib.csplat_l1_scratch_bytes)
        loss = torch.empty((), dtype=torch.float32, device=a.device)
        if mask is not None:
            B, Cc, hw, mc = _mask_layout(a, mask)
        else:
            B, Cc, hw, mc = 1, 1, a.numel(), 1
        if need:
            sign8 = torch.empty(a.numel(), dtype=torch.int8, device=a.device)
            _n.launch("csplat_l1_signs", a.device, B, Cc, hw, _n.ptr(a), _n.ptr(b), _n.ptr(mask), mc, _n.ptr(scratch), _n.ptr(loss), _n.ptr(sign8))
            ctx.save_for_backward(sign8, mask)
            ctx.layout = (B, Cc, hw, mc, tuple(a.shape))
        elif mask is None:
            _n.launch("csplat_l1", a.device, a.numel(), _n.ptr(a), _n.ptr(b), _n.ptr(scratch), _n.ptr(loss), None)
        else:
            _n.launch("csplat_l1_masked", a.device, B, Cc, hw, _n.ptr(a), _n.ptr(b), _n.ptr(mask), mc, _n.ptr(scratch), _n.ptr(loss), None)
        return loss

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        sign8, mask = ctx.saved_tensors
        B, Cc, hw, mc, shape = ctx.layout
        g = g.reshape(1).float().contiguous()
        out = torch.empty(shape, dtype=torch.float32, device=sign8.device)
        _n.launch("csplat_l1_signs_bwd", sign8.device, B, Cc, hw, _n.ptr(sign8), _n.ptr(mask), mc, _n.ptr(g), _n.ptr(out))
        ga = out if ctx.needs_input_grad[0] else None
        gb = -out if ctx.needs_input_grad[1] else None
        return ga, gb, None


_MAX_PLANES = 65535          # one launch of the tile kernels carries the plane in blockIdx.z


def _plane_chunks(n_planes):
    """[start, end) ranges of at most _MAX_PLANES planes: the tile kernels are called once per range (their sums are per plane, so
    the result is the same sum)"""
    return [(s, min(s + _MAX_PLANES, n_planes)) for s in range(0, n_planes, _MAX_PLANES)]


def _launch_per_chunk(name, device, n_planes, H, W, *args):
    """lib.<name>(stream, planes of the range, H, W, taps, *args) once per _plane_chunks range.  A tensor among `args` holds one row
    per plane and passes as the pointer of the range's rows; anything else (None, a number, a pointer) passes as it is."""
    for s, e in _plane_chunks(n_planes):
        _n.launch(name, device, e - s, H, W, _taps(), *[_n.ptr(a[s:e]) if torch.is_tensor(a) else a for a in args])


class GaussianBlur11(torch.autograd.Function):
    """zero-padded 11x11 Gaussian window (sigma 1.5) on every [H, W] plane, HIP kernel csplat_blur11; self-adjoint."""

    @staticmethod
    def forward(ctx, x):
        _n.require_cuda(x)
        x = x.contiguous().float()
        H, W = x.shape[-2:]
        out = torch.empty_like(x)
        if x.numel() == 0:
            return out
        xp = x.view(-1, H, W)
        _launch_per_chunk("csplat_blur11", x.device, xp.shape[0], H, W, xp, out.view(-1, H, W))
        return out

    @staticmethod
    def backward(ctx, g):
        return GaussianBlur11.apply(g)


_WINDOWS = {}


def _window1d(window_size, channel, like):
    key = (window_size, channel, like.device, like.dtype)
    if key not in _WINDOWS:
        g = torch.tensor([exp(-(x - window_size // 2) ** 2 / float(2 * 1.5 ** 2)) for x in range(window_size)])
        g = (g / g.sum()).to(like)
        _WINDOWS[key] = (g.view(1, 1, 1, -1).expand(channel, 1, 1, window_size).contiguous(),
                         g.view(1, 1, -1, 1).expand(channel, 1, window_size, 1).contiguous())
    return _WINDOWS[key]


def _blur(x, wh, wv, pad, channel):
    """the reference's 11x11 window is the outer product of a 1-D Gaussian with itself (loss_utils.py:30-38): the
    zero-padded 2-D grouped convolution equals a horizontal then a vertical 11-tap pass (22 instead of 121 MACs)."""
    return F.conv2d(F.conv2d(x, wh, padding=(0, pad), groups=channel), wv, padding=(pad, 0), groups=channel)


class FusedSSIM(torch.autograd.Function):
    """mean SSIM(img1, img2) through csplat_ssim_fwd / csplat_ssim_bwd: windows, map, mean and the three partial
    derivatives in one launch; the backward (w.r.t. img1) in one more.  img2 is treated as a constant (ground truth)."""

    @staticmethod
    def forward(ctx, img1, img2):
        _n.require_cuda(img1)
        x, y = img1.contiguous(), img2.contiguous()
        H, W = x.shape[-2:]
        n_img = x.numel() // (H * W)
        need = img1.requires_grad
        p = torch.empty((3,) + tuple(x.shape), dtype=torch.float32, device=x.device) if need else None
        per_plane = int(_n.lib.csplat_ssim_partial_count(1, H, W))
        partial = torch.empty(n_img * per_plane, dtype=torch.float32, device=x.device)
        pp = p.view(3, -1, H, W) if need else (None,) * 3
        _launch_per_chunk("csplat_ssim_fwd", x.device, n_img, H, W, x.view(-1, H, W), y.view(-1, H, W), pp[0], pp[1], pp[2], None,
                          partial.view(n_img, per_plane))
        ctx.save_for_backward(x, y, p)
        ctx.dims = (n_img, H, W)
        return partial.sum() / float(x.numel())

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        x, y, p = ctx.saved_tensors
        n_img, H, W = ctx.dims
        g = g.reshape(1).float().contiguous()
        dx = torch.empty_like(x)
        pp = p.view(3, -1, H, W)
        _launch_per_chunk("csplat_ssim_bwd", x.device, n_img, H, W, x.view(-1, H, W), y.view(-1, H, W), pp[0], pp[1], pp[2], _n.ptr(g),
                          1.0 / float(x.numel()), None, None, dx.view(-1, H, W))
        return dx, None


# workgroup partials of csplat_image_loss_fwd, one buffer per (device, stream, shape); csplat.cloth_regs keeps its own here, under a "regs" tag
_IMG_SCRATCH = _n.ScratchCache(cap=64)


class FusedImageLoss(torch.autograd.Function):
    """Ll1 + lambda_dssim * ssim_loss of the reference's train step (train_utils.py:50-74), the PSNR it logs (:262-283) and the sum with
    the regularisers as ONE node: csplat_image_loss_fwd (tile kernel + a one-workgroup sum) and csplat_image_loss_bwd (one launch).  gt is a constant.  With a mask (Camera.mask
    stacked to [B,1,H,W], :61-67) the two terms are mean |(x - y) m| and mean((1 - ssim_map) m).
    Returns (img_weight * image_loss + add_weight * add, psnr_scale * sum_b PSNR_b, image_loss); only the first is differentiable."""

    @staticmethod
    def forward(ctx, image, gt, lam, mask=None, add=None, img_weight=1.0, add_weight=1.0, psnr_scale=1.0):
        _n.require_cuda(image)
        x, y = image.contiguous(), gt.contiguous()
        mask = None if mask is None else mask.contiguous()
        if x.dim() == 3:
            x, y = x.unsqueeze(0), y.unsqueeze(0)
        H, W = x.shape[-2:]
        Cc = int(x.shape[-3])
        B = x.numel() // (Cc * H * W)
        need = image.requires_grad
        dev = x.device
        mc = 1 if mask is None else _mask_layout(x, mask)[3]
        out = torch.empty(4, dtype=torch.float32, device=dev)
        p = torch.empty((3,) + tuple(x.shape), dtype=torch.float32, device=dev) if need else None
        sign = torch.empty(x.shape, dtype=torch.int8, device=dev) if need else None
        addc = None if add is None else add.reshape(1).float()
        scratch = _IMG_SCRATCH.buffer(dev, (B, Cc, H, W), lambda: _n.lib.csplat_image_loss_scratch_bytes(B, Cc, H, W))
        _n.launch("csplat_image_loss_fwd", dev, B, Cc, H, W, _taps(), _n.ptr(x), _n.ptr(y), _n.ptr(mask), mc, float(lam), float(img_weight),
                  _n.ptr(addc), float(add_weight), float(psnr_scale), *([_n.ptr(p[k]) for k in range(3)] if need else [None] * 3),
                  _n.ptr(sign), _n.ptr(scratch), _n.ptr(out))
        ctx.save_for_backward(x, y, p, sign, mask)
        ctx.dims = (B, Cc, H, W, mc, float(lam), float(img_weight), float(add_weight), add is not None, image.shape)
        loss, ps, il = out[0], out[1], out[2]
        ctx.mark_non_differentiable(ps, il)
        ctx.set_materialize_grads(False)
        return loss, ps, il

    @staticmethod
    @once_differentiable
    def backward(ctx, g, _gp, _gi):
        x, y, p, sign, mask = ctx.saved_tensors
        B, Cc, H, W, mc, lam, w_img, w_add, has_add, shape = ctx.dims
        if g is None:
            return (None,) * 8
        g = g.reshape(1).float()
        dx = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty_like(x)
            _n.launch("csplat_image_loss_bwd", x.device, B, Cc, H, W, _taps(), _n.ptr(x), _n.ptr(y), _n.ptr(p[0]), _n.ptr(p[1]), _n.ptr(p[2]),
                      _n.ptr(sign), _n.ptr(mask), mc, lam, w_img, _n.ptr(g), _n.ptr(dx))
            dx = dx.reshape(shape)
        gadd = None
        if has_add and ctx.needs_input_grad[4]:
            gadd = g.reshape(()) if w_add == 1.0 else g.reshape(()) * w_add
        return dx, None, None, None, gadd, None, None, None


def _image_loss_fusable(image_tensor, gt_image_tensor, opt, mask_tensor):
    return bool(opt.lambda_dssim != 0 and image_tensor.is_cuda and image_tensor.dtype == torch.float32 and
                gt_image_tensor.dtype == torch.float32 and image_tensor.shape == gt_image_tensor.shape and image_tensor.dim() in (3, 4)
                and image_tensor.numel() > 0 and image_tensor.numel() // (image_tensor.shape[-1] * image_tensor.shape[-2]) <= _MAX_PLANES
                and not gt_image_tensor.requires_grad and
                (mask_tensor is None or (image_tensor.dim() == 4 and _mask_layout(image_tensor, mask_tensor) is not None)))


def ssim(img1, img2, window_size=11, size_average=True, return_map=False):
    """utils/loss_utils.py:40-70: Gaussian-window SSIM (window 11, sigma 1.5), separable form."""
    if window_size == 11 and size_average and not return_map and img1.is_cuda and img1.dtype == torch.float32 and \
            img2.dtype == torch.float32 and img1.shape == img2.shape and img1.numel() > 0 and not img2.requires_grad:
        return FusedSSIM.apply(img1, img2)
    if window_size == 11 and size_average and not return_map:     # the fused kernel's form, missed on dtype / shape
        _n.composed_fallback("train.ssim", "dtype" if img1.shape == img2.shape and img1.numel() else "shape", img1)
    channel = img1.size(-3)
    wh, wv = _window1d(window_size, channel, img1)
    pad = window_size // 2
    stacked = torch.cat([img1, img2, img1 * img1, img2 * img2, img1 * img2], dim=0)
    if window_size == 11 and stacked.is_cuda and stacked.dtype == torch.float32:
        both = GaussianBlur11.apply(stacked)                     # one HIP launch for all five windows (and one in backward)
    else:
        _n.composed_fallback("train.ssim.window", "mode" if window_size != 11 else "dtype", stacked)
        both = _blur(stacked, wh, wv, pad, channel)              # CPU tensors (tests) / other window sizes
    n = img1.shape[0]
    mu1, mu2 = both[:n], both[n:2 * n]
    mu1_sq, mu2_sq, mu1_mu2 = mu1.pow(2), mu2.pow(2), mu1 * mu2
    sigma1_sq = both[2 * n:3 * n] - mu1_sq
    sigma2_sq = both[3 * n:4 * n] - mu2_sq
    sigma12 = both[4 * n:] - mu1_mu2
    C1, C2 = 0.01 ** 2, 0.03 ** 2
    ssim_map = ((2 * mu1_mu2 + C1) * (2 * sigma12 + C2)) / ((mu1_sq + mu2_sq + C1) * (sigma1_sq + sigma2_sq + C2))
    if return_map:
        return ssim_map
    return ssim_map.mean() if size_average else ssim_map.mean(1).mean(1).mean(1)


@torch.no_grad()
def psnr(img1, img2):
    """utils/image_utils.py:17-21: [B, 1] PSNR per image.  On the GPU one launch (csplat_psnr); otherwise torch ops."""
    if img1.is_cuda and img1.dtype == torch.float32 and img2.dtype == torch.float32 and img1.shape == img2.shape \
            and img1.dim() >= 2 and img1.numel() > 0:
        a, b = img1.contiguous(), img2.contiguous()
        B = int(a.shape[0])
        out = torch.empty(B, 1, dtype=torch.float32, device=a.device)
        scratch = _n.temp(a.device, _n.lib.csplat_psnr_scratch_bytes(B))
        _n.launch("csplat_psnr", a.device, B, a.numel() // B, _n.ptr(a), _n.ptr(b), _n.ptr(scratch), _n.ptr(out))
        return out
    _n.composed_fallback("train.psnr", "dtype" if img1.shape == img2.shape and img1.numel() else "shape", img1)
    mse = ((img1 - img2) ** 2).view(img1.shape[0], -1).mean(1, keepdim=True)
    return 20 * torch.log10(1.0 / torch.sqrt(mse))


def image_losses(image_tensor, gt_image_tensor, opt, mask_tensor=None):
    """train_utils.py:50-74 (returns the loss; the reference's loss_dict of .item() host reads is not built)."""
    if _image_loss_fusable(image_tensor, gt_image_tensor, opt, mask_tensor):
        return FusedImageLoss.apply(image_tensor, gt_image_tensor, opt.lambda_dssim, mask_tensor)[0]
    if opt.lambda_dssim != 0:
        # (more planes than one launch of the fused kernel carries is a miss on SHAPE; l1_loss + ssim below take any plane count)
        planes = image_tensor.numel() // max(image_tensor.shape[-1] * image_tensor.shape[-2], 1) if image_tensor.dim() >= 2 else 0
        _n.composed_fallback("train.image_losses", "dtype" if image_tensor.shape == gt_image_tensor.shape and image_tensor.numel() and
                             planes <= _MAX_PLANES else "shape", image_tensor)
    loss = l1_loss(image_tensor, gt_image_tensor, mask_tensor)
    if opt.lambda_dssim != 0:
        if mask_tensor is None:
            ssim_loss = 1.0 - ssim(image_tensor, gt_image_tensor)
        else:
            ssim_loss = ((1.0 - ssim(image_tensor, gt_image_tensor, return_map=True)) * mask_tensor).mean()
        loss = loss + opt.lambda_dssim * ssim_loss
    return loss
