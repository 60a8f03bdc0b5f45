"""train_step analogue (BASELINE.json configs[2]): the call pattern of
/root/reference/scene_reconstruction/train_utils.py:240-321 around the hot path -- for each camera of the mini-batch
(3 consecutive timesteps of one view, scene_reconstruction/dataset.py:75-87) render() = simulator -> mesh->Gaussian
transform -> HIP rasterizer; stack; L1 + lambda_dssim*(1-SSIM) (train_utils.py:50-74, utils/loss_utils.py:20-70);
regularisation (train_utils.py:77-100: deformation magnitude, rigid edge length, momentum); ONE backward; the summed
screen-space gradient / radii / visibility that densification consumes (:276-292); two Adam steps (:310-319).
Densification / pruning itself (Adam-state surgery) is a "next" row and is not performed here.
Host-side torch only; the compute is in the drop-in modules."""
from math import exp
from types import SimpleNamespace

import ctypes as C

import torch
import torch.nn.functional as F

from gaussian_renderer import render, render_views
from . import dist as cd
from . import native as _n
from .densify import densification

# arguments/__init__.py:109-150 overlaid by arguments/cloth_splatting/default.py:1-43
DEFAULT_OPT = SimpleNamespace(lambda_dssim=0.05, lambda_rigid=0.3, lambda_deform_mag=0.01, lambda_momentum=0.1,
                              position_lr_init=0.00016, feature_lr=0.00025, opacity_lr=0.05, scaling_lr=0.005,
                              rotation_lr=0.001, meshnet_lr=3e-4)
DEFAULT_PIPE = SimpleNamespace(compute_cov3D_python=False, convert_SHs_python=False, debug=False)


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


import ctypes as _C
from math import exp as _exp

_TAPS = {}


def _taps(window_size=11, sigma=1.5):
    """the reference's float32 window (loss_utils.py:30-32): torch.Tensor([exp(.)]) / sum, both in float32"""
    if window_size not in _TAPS:
        g = torch.tensor([_exp(-(x - window_size // 2) ** 2 / float(2 * sigma ** 2)) for x in range(window_size)])
        g = g / g.sum()
        _TAPS[window_size] = (_C.c_float * window_size)(*[float(v) for v in g])
    return _TAPS[window_size]


_L1_SCRATCH = {}
_n.TICKET_CACHES.append(_L1_SCRATCH)


def _l1_scratch(device):
    """workgroup partial sums of csplat_l1 for the CURRENT stream of `device` (launches on one stream cannot overlap): one buffer per
    stream instead of an allocation per loss.  (Rounds 1-4 kept a ticket counter here too; since round 5 a second one-workgroup launch sums
    the partials -- the ticket's device-scope release cost ~10 us of L2 write-back per call, csrc/csplat_image.hip.)"""
    key = (str(device), _n.scratch_stream(device))
    buf = _L1_SCRATCH.get(key)
    if buf is None:
        buf = _L1_SCRATCH[key] = torch.zeros(int(_n.lib.csplat_l1_scratch_bytes()) // 4, dtype=torch.int32, device=device)
    return buf


def _launch_l1(x, y, mask, scratch, loss, grad):
    st = _n.stream_handle(x.device)
    if mask is None:
        _n.check(_n.lib.csplat_l1(st, x.numel(), _n.ptr(x), _n.ptr(y), _n.ptr(scratch), _n.ptr(loss), _n.ptr(grad)), "csplat_l1")
    else:
        B, Cc, hw, mc = _mask_layout(x, mask)
        _n.check(_n.lib.csplat_l1_masked(st, B, Cc, hw, _n.ptr(x), _n.ptr(y), _n.ptr(mask), mc, _n.ptr(scratch), _n.ptr(loss),
                                         _n.ptr(grad)), "csplat_l1_masked")


class FusedL1(torch.autograd.Function):
    """mean |a - b| (mean |(a - b) * mask| with a mask).  Forward: csplat_l1_signs -- the loss and ONE BYTE per element
    (sign((a - b) m)); backward: csplat_l1_signs_bwd writes g * sign * m / n in one pass (g = the incoming gradient, read on the
    device).  The reference's l1_loss is three elementwise launches each way (utils/loss_utils.py:20-23)."""

    @staticmethod
    def forward(ctx, a, b, mask=None):
        _n.require_cuda(a)
        a, b = a.contiguous(), b.contiguous()
        mask = None if mask is None else mask.contiguous()
        need = a.requires_grad or b.requires_grad
        scratch = _l1_scratch(a.device)
        loss = torch.empty((), dtype=torch.float32, device=a.device)
        if mask is not None:
            B, Cc, hw, mc = _mask_layout(a, mask)
        else:
            B, Cc, hw, mc = 1, 1, a.numel(), 1
        with _n.on_device(a.device):
            if need:
                sign8 = torch.empty(a.numel(), dtype=torch.int8, device=a.device)
                _n.check(_n.lib.csplat_l1_signs(_n.stream_handle(a.device), B, Cc, hw, _n.ptr(a), _n.ptr(b), _n.ptr(mask), mc, _n.ptr(scratch),
                                                _n.ptr(loss), _n.ptr(sign8)), "csplat_l1_signs")
                ctx.save_for_backward(sign8, mask)
                ctx.layout = (B, Cc, hw, mc, tuple(a.shape))
            else:
                _launch_l1(a, b, mask, scratch, loss, None)
        return loss

    @staticmethod
    def backward(ctx, g):
        sign8, mask = ctx.saved_tensors
        B, Cc, hw, mc, shape = ctx.layout
        g = g.reshape(1).float().contiguous()
        out = torch.empty(shape, dtype=torch.float32, device=sign8.device)
        with _n.on_device(sign8.device):
            _n.check(_n.lib.csplat_l1_signs_bwd(_n.stream_handle(sign8.device), B, Cc, hw, _n.ptr(sign8), _n.ptr(mask), mc, _n.ptr(g), _n.ptr(out)),
                     "csplat_l1_signs_bwd")
        ga = out if ctx.needs_input_grad[0] else None
        gb = -out if ctx.needs_input_grad[1] else None
        return ga, gb, None


_MAX_PLANES = 65535          # one launch of the tile kernels carries the plane in blockIdx.z


def _plane_chunks(n_planes):
    """[start, end) ranges of at most _MAX_PLANES planes: the tile kernels are called once per range (their sums are per plane, so
    the result is the same sum)"""
    return [(s, min(s + _MAX_PLANES, n_planes)) for s in range(0, n_planes, _MAX_PLANES)]


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
        xp, op = x.view(-1, H, W), out.view(-1, H, W)
        with _n.on_device(x.device):
            for s, e in _plane_chunks(xp.shape[0]):
                _n.check(_n.lib.csplat_blur11(_n.stream_handle(x.device), e - s, H, W, _taps(), _n.ptr(xp[s:e]), _n.ptr(op[s:e])),
                         "csplat_blur11")
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
        xp, yp, pp = x.view(-1, H, W), y.view(-1, H, W), (p.view(3, -1, H, W) if need else None)
        with _n.on_device(x.device):
            for s, e in _plane_chunks(n_img):
                _n.check(_n.lib.csplat_ssim_fwd(_n.stream_handle(x.device), e - s, H, W, _taps(), _n.ptr(xp[s:e]), _n.ptr(yp[s:e]),
                                                _n.ptr(pp[0, s:e]) if need else None, _n.ptr(pp[1, s:e]) if need else None,
                                                _n.ptr(pp[2, s:e]) if need else None, None, _n.ptr(partial[s * per_plane:e * per_plane])),
                         "csplat_ssim_fwd")
        ctx.save_for_backward(x, y, p)
        ctx.dims = (n_img, H, W)
        return partial.sum() / float(x.numel())

    @staticmethod
    def backward(ctx, g):
        x, y, p = ctx.saved_tensors
        n_img, H, W = ctx.dims
        g = g.reshape(1).float().contiguous()
        dx = torch.empty_like(x)
        xp, yp, pp, dp = x.view(-1, H, W), y.view(-1, H, W), p.view(3, -1, H, W), dx.view(-1, H, W)
        with _n.on_device(x.device):
            for s, e in _plane_chunks(n_img):
                _n.check(_n.lib.csplat_ssim_bwd(_n.stream_handle(x.device), e - s, H, W, _taps(), _n.ptr(xp[s:e]), _n.ptr(yp[s:e]),
                                                _n.ptr(pp[0, s:e]), _n.ptr(pp[1, s:e]), _n.ptr(pp[2, s:e]), _n.ptr(g), 1.0 / float(x.numel()),
                                                None, None, _n.ptr(dp[s:e])), "csplat_ssim_bwd")
        return dx, None


_IMG_SCRATCH = {}
_n.TICKET_CACHES.append(_IMG_SCRATCH)


def _image_loss_scratch(dev, shape):
    """workgroup partials of csplat_image_loss_fwd: one buffer per (device, stream, shape)"""
    B, Cc, H, W = shape
    key = (dev, _n.scratch_stream(dev), B, Cc, H, W)
    buf = _IMG_SCRATCH.get(key)
    if buf is None:
        if len(_IMG_SCRATCH) >= 64:
            _n.evict_scratch(_IMG_SCRATCH)
        buf = _IMG_SCRATCH[key] = torch.zeros(int(_n.lib.csplat_image_loss_scratch_bytes(B, Cc, H, W)), dtype=torch.uint8, device=dev)
    return buf


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
        with _n.on_device(dev):
            scratch = _image_loss_scratch(dev, (B, Cc, H, W))
            _n.check(_n.lib.csplat_image_loss_fwd(_n.stream_handle(dev), B, Cc, H, W, _taps(), _n.ptr(x), _n.ptr(y),
                                                  None if mask is None else _n.ptr(mask), mc, float(lam), float(img_weight),
                                                  None if addc is None else _n.ptr(addc), float(add_weight), float(psnr_scale),
                                                  *([_n.ptr(p[k]) for k in range(3)] if need else [None] * 3),
                                                  _n.ptr(sign) if need else None, _n.ptr(scratch), _n.ptr(out)), "csplat_image_loss_fwd")
        ctx.save_for_backward(x, y, p, sign, mask)
        ctx.dims = (B, Cc, H, W, mc, float(lam), float(img_weight), float(add_weight), add is not None, image.shape)
        loss, ps, il = out[0], out[1], out[2]
        ctx.mark_non_differentiable(ps, il)
        ctx.set_materialize_grads(False)
        return loss, ps, il

    @staticmethod
    def backward(ctx, g, _gp, _gi):
        x, y, p, sign, mask = ctx.saved_tensors
        B, Cc, H, W, mc, lam, w_img, w_add, has_add, shape = ctx.dims
        if g is None:
            return (None,) * 8
        g = g.reshape(1).float()
        dx = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty_like(x)
            with _n.on_device(x.device):
                _n.check(_n.lib.csplat_image_loss_bwd(_n.stream_handle(x.device), B, Cc, H, W, _taps(), _n.ptr(x), _n.ptr(y), _n.ptr(p[0]),
                                                      _n.ptr(p[1]), _n.ptr(p[2]), _n.ptr(sign), None if mask is None else _n.ptr(mask), mc,
                                                      lam, w_img, _n.ptr(g), _n.ptr(dx)), "csplat_image_loss_bwd")
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
        scratch = torch.empty(_n.lib.csplat_psnr_scratch_bytes(B), dtype=torch.uint8, device=a.device)
        with _n.on_device(a.device):
            _n.check(_n.lib.csplat_psnr(_n.stream_handle(a.device), B, a.numel() // B, _n.ptr(a), _n.ptr(b), _n.ptr(scratch),
                                        _n.ptr(out)), "csplat_psnr")
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


_GEOM_SCRATCH = {}
_n.TICKET_CACHES.append(_GEOM_SCRATCH)


def _geom_scratch(dev, V, hw):
    """workgroup partials of csplat_geom_loss_fwd: one buffer per (device, stream, views, pixels)"""
    key = (dev, _n.scratch_stream(dev), V, hw)
    buf = _GEOM_SCRATCH.get(key)
    if buf is None:
        if len(_GEOM_SCRATCH) >= 64:
            _n.evict_scratch(_GEOM_SCRATCH)
        buf = _GEOM_SCRATCH[key] = torch.zeros(int(_n.lib.csplat_geom_loss_scratch_bytes(V, hw)), dtype=torch.uint8, device=dev)
    return buf


def _ptr_table(tensors):
    return None if not tensors else (C.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


class GeometryLoss(torch.autograd.Function):
    """depth and silhouette supervision of a step's views as ONE node (include/csplat.h, csplat_geom_loss_fwd, states the semantics):
    csplat_geom_loss_fwd (one pass over the pixels of all views + a one-workgroup sum) keeps one byte per pixel, csplat_geom_loss_bwd
    (one launch) writes d(depth) and d(alpha) of every view from it.  The views are separate tensors (the rasterizer's outputs): they
    reach the library as pointer tables, nothing is stacked.  `views` = depths + alphas + gt_depths + silhouettes + masks, V tensors
    each, the last three groups present as `has` = (Z, S, M) says.  Returns (weight * (lambda_depth * L_depth + lambda_silhouette * L_sil)
    + add_weight * add, L_depth, L_sil); only the first is differentiable, in depths, alphas and add."""

    @staticmethod
    def forward(ctx, V, hw, lam_d, lam_s, weight, add_weight, has, add, *views):
        _n.require_cuda(*views)
        views = [t.contiguous() for t in views]
        groups, at = [], 0
        for present in (True, True) + tuple(has):
            groups.append(views[at:at + V] if present else [])
            at += V if present else 0
        D, A, Z, S, M = groups
        dev = A[0].device
        need = any(ctx.needs_input_grad[8 + i] for i in range(2 * V))
        out = torch.empty(3, dtype=torch.float32, device=dev)
        sign = torch.empty(V * hw, dtype=torch.uint8, device=dev) if need else None
        addc = None if add is None else add.reshape(1).float()
        with _n.on_device(dev):
            scratch = _geom_scratch(dev, V, hw)
            _n.check(_n.lib.csplat_geom_loss_fwd(_n.stream_handle(dev), V, hw, _ptr_table(D if Z else []), _ptr_table(A), _ptr_table(Z),
                                                 _ptr_table(S), _ptr_table(M), float(lam_d), float(lam_s), float(weight),
                                                 None if addc is None else _n.ptr(addc), float(add_weight), _n.ptr(sign), _n.ptr(scratch),
                                                 _n.ptr(out)), "csplat_geom_loss_fwd")
        ctx.save_for_backward(sign, *Z, *M)
        ctx.dims = (V, hw, float(lam_d) if Z else 0.0, float(lam_s) if S else 0.0, float(weight), float(add_weight), len(Z), len(M),
                    add is not None, [tuple(t.shape) for t in views[:2 * V]], len(views))
        loss, ld, ls = out[0], out[1], out[2]
        ctx.mark_non_differentiable(ld, ls)
        ctx.set_materialize_grads(False)
        return loss, ld, ls

    @staticmethod
    def backward(ctx, g, _gd, _gs):
        V, hw, lam_d, lam_s, weight, w_add, nz, nm, has_add, shapes, n_views_in = ctx.dims
        if g is None:
            return (None,) * (8 + n_views_in)
        sign, rest = ctx.saved_tensors[0], ctx.saved_tensors[1:]
        Z, M = list(rest[:nz]), list(rest[nz:nz + nm])
        g = g.reshape(1).float()
        want_d = lam_d > 0 and any(ctx.needs_input_grad[8:8 + V])
        want_a = any(ctx.needs_input_grad[8 + V:8 + 2 * V])
        gD = gA = None
        if sign is not None and (want_d or want_a):
            dev = sign.device
            gD = torch.empty(V, hw, dtype=torch.float32, device=dev) if want_d else None
            gA = torch.empty(V, hw, dtype=torch.float32, device=dev) if want_a else None
            with _n.on_device(dev):
                _n.check(_n.lib.csplat_geom_loss_bwd(_n.stream_handle(dev), V, hw, _n.ptr(sign), _ptr_table(Z), _ptr_table(M), lam_d, lam_s,
                                                     weight, _n.ptr(g), _n.ptr(gD), _n.ptr(gA)), "csplat_geom_loss_bwd")
        grads = []
        for k, buf in enumerate((gD, gA)):      # every view's gradient is a slice of the one buffer the launch wrote
            for v in range(V):
                i = k * V + v
                grads.append(buf[v].view(shapes[i]) if (buf is not None and ctx.needs_input_grad[8 + i]) else None)
        gadd = None
        if has_add and ctx.needs_input_grad[7]:
            gadd = g.reshape(()) if w_add == 1.0 else g.reshape(()) * w_add
        return (None,) * 7 + (gadd,) + tuple(grads) + (None,) * (n_views_in - 2 * V)


def _geometry_views(name, views, V, hw_shape, like, optional=False):
    """a list of V images [1,H,W] / [H,W] of one size, dtype and device -> ValueError otherwise (nothing touches the device)"""
    if views is None:
        if optional:
            return None
        raise ValueError(f"geometry_losses: `{name}` is needed")
    views = list(views)
    if len(views) != V:
        raise ValueError(f"geometry_losses: {len(views)} `{name}` images for {V} views")
    for t in views:
        if not torch.is_tensor(t):
            raise ValueError(f"geometry_losses: `{name}` holds a {type(t).__name__}, not a tensor")
        if t.dim() not in (2, 3) or (t.dim() == 3 and t.shape[0] != 1) or tuple(t.shape[-2:]) != tuple(hw_shape):
            raise ValueError(f"geometry_losses: a `{name}` image of shape {tuple(t.shape)}; all views are [1,H,W] or [H,W] of one size "
                             f"{tuple(hw_shape)}")
        if t.dtype != like.dtype:
            raise ValueError(f"geometry_losses: a `{name}` image of dtype {t.dtype}, the alpha images are {like.dtype}")
        if t.device != like.device:
            raise ValueError(f"geometry_losses: a `{name}` image on {t.device}, the alpha images are on {like.device}")
    return views


def _geometry_composed(D, A, Z, S, M, lam_d, lam_s, n):
    """the formulas of csplat_geom_loss_fwd from torch operations (float64, CPU tensors): selection by `where` on the INPUTS, so that an
    unselected NaN neither reaches the sum nor, through 0 * NaN, the gradient"""
    zero = A[0].new_zeros(())
    sum_d, sum_s = zero, zero
    for v in range(len(A)):
        a = A[v].reshape(A[v].shape[-2:])
        m = None if M is None else M[v].reshape(a.shape)
        if Z is not None:
            z, d = Z[v].reshape(a.shape), D[v].reshape(a.shape)
            valid = torch.isfinite(z) & (z > 0)
            w = torch.where(valid, torch.ones_like(z) if m is None else m, torch.zeros_like(z))
            on = w != 0
            r = torch.where(on, d, zero) - torch.where(on, a, zero) * torch.where(on, z, zero)
            sum_d = sum_d + torch.abs(r * w).sum()
        if S is not None:
            s = S[v].reshape(a.shape)
            if m is None:
                sum_s = sum_s + torch.abs(a - s).sum()
            else:
                on = m != 0
                sum_s = sum_s + torch.abs((torch.where(on, a, zero) - torch.where(on, s, zero)) * m).sum()
    ld, ls = sum_d / n, sum_s / n
    return lam_d * ld + lam_s * ls, ld, ls


def geometry_losses(depths, alphas, gt_depths, silhouettes, lambda_depth, lambda_silhouette, masks=None, add=None, weight=1.0,
                    add_weight=1.0):
    """Depth and silhouette supervision of the views of a step -> (total, depth_loss, silhouette_loss), device scalars:
        total = weight * (lambda_depth * L_depth + lambda_silhouette * L_sil) + add_weight * add
        L_depth = (1/n) sum |(D - A Z) w_d|,  w_d = mask where Z is finite and > 0, else 0;     L_sil = (1/n) sum |(A - S) mask|
    with D / A the rasterizer's depth (sum T alpha z) and alpha (1 - T_final) images, Z the measured z-depth, S the silhouette in [0, 1],
    n the pixels of ALL views (include/csplat.h, csplat_geom_loss_fwd: selection semantics, sign(0) = 0).  Every argument but the weights is
    a list of V images [1,H,W] or [H,W] of one size; gt_depths / silhouettes may be None when their weight is 0, masks may be None.  A term
    is on when its weight is > 0.  Only `total` is differentiable, in depths, alphas and add.
    ValueError before anything touches the device: no view, shapes / dtypes / devices that differ, a weight < 0, no term on, a term's
    weight > 0 without its data.  float32 GPU tensors take the HIP kernels (GeometryLoss); anything else composes the same formulas from
    torch operations (reported through csplat.native.composed_fallback for GPU tensors: raises under STRICT)."""
    lam_d, lam_s = float(lambda_depth), float(lambda_silhouette)
    if not (lam_d >= 0.0 and lam_s >= 0.0):
        raise ValueError(f"geometry_losses: the weights are >= 0, got lambda_depth={lam_d}, lambda_silhouette={lam_s}")
    if lam_d == 0.0 and lam_s == 0.0:
        raise ValueError("geometry_losses: no term is on (both weights are 0)")
    alphas = list(alphas) if alphas is not None else []
    V = len(alphas)
    if V == 0 or not torch.is_tensor(alphas[0]) or alphas[0].dim() not in (2, 3):
        raise ValueError("geometry_losses: `alphas` is a non-empty list of [1,H,W] or [H,W] images")
    like, hw_shape = alphas[0], tuple(alphas[0].shape[-2:])
    if not like.dtype.is_floating_point or hw_shape[0] * hw_shape[1] == 0:
        raise ValueError(f"geometry_losses: the alpha images are non-empty floating-point images, got {like.dtype} {tuple(like.shape)}")
    A = _geometry_views("alphas", alphas, V, hw_shape, like)
    if lam_d > 0.0 and gt_depths is None:
        raise ValueError("geometry_losses: lambda_depth > 0 needs `gt_depths`")
    if lam_s > 0.0 and silhouettes is None:
        raise ValueError("geometry_losses: lambda_silhouette > 0 needs `silhouettes`")
    Z = _geometry_views("gt_depths", gt_depths, V, hw_shape, like) if lam_d > 0.0 else None
    D = _geometry_views("depths", depths, V, hw_shape, like) if lam_d > 0.0 else None
    S = _geometry_views("silhouettes", silhouettes, V, hw_shape, like) if lam_s > 0.0 else None
    M = _geometry_views("masks", masks, V, hw_shape, like, optional=True)
    if add is not None and (not torch.is_tensor(add) or add.numel() != 1 or add.device != like.device):
        raise ValueError("geometry_losses: `add` is a scalar tensor on the images' device")
    const = [t for grp in (Z, S, M) if grp is not None for t in grp]
    if any(t.requires_grad for t in const):
        raise ValueError("geometry_losses: gt_depths, silhouettes and masks are constants (requires_grad is set on one)")
    hw = hw_shape[0] * hw_shape[1]
    if like.is_cuda and like.dtype == torch.float32 and (add is None or add.dtype == torch.float32):
        views = (D if D is not None else [a.detach() for a in A]) + A + (Z or []) + (S or []) + (M or [])
        return GeometryLoss.apply(V, hw, lam_d, lam_s, float(weight), float(add_weight), (Z is not None, S is not None, M is not None),
                                  add, *views)
    _n.composed_fallback("train.geometry_losses", "dtype", like)
    total, ld, ls = _geometry_composed(D, A, Z, S, M, lam_d, lam_s, float(V * hw))
    total = weight * total
    if add is not None:
        total = total + add_weight * add.reshape(())
    return total, ld.detach(), ls.detach()


class FusedClothRegs(torch.autograd.Function):
    """the three cloth regularisers and their gradient in one launch (csplat_cloth_regs); backward scales the stored gradient."""

    @staticmethod
    def forward(ctx, D, edge_index, rest_len, lam_deform, lam_rigid, lam_mom, csr=None, tap=False, defer=False):
        D = D.contiguous().float()
        ctx.set_materialize_grads(False)
        T, V = int(D.shape[0]), int(D.shape[1])
        E = int(edge_index.shape[1])
        loss = torch.empty((), dtype=torch.float32, device=D.device)
        grad = torch.empty_like(D)
        ei, rl = edge_index.contiguous(), rest_len.contiguous().float()
        dev, stream, skey = D.device, _n.stream_handle(D.device), _n.scratch_stream(D.device)

        def launch():
            with _n.on_device(dev):
                key = ("regs", dev, skey, T, V, E)
                scratch = _IMG_SCRATCH.get(key)          # zeroed once per (device, stream, sizes): the kernel leaves its ticket at zero
                if scratch is None:
                    if len(_IMG_SCRATCH) >= 64:
                        _n.evict_scratch(_IMG_SCRATCH)
                    scratch = _IMG_SCRATCH[key] = torch.zeros(_n.lib.csplat_cloth_regs_scratch_bytes(T, V, E), dtype=torch.uint8, device=dev)
                _n.check(_n.lib.csplat_cloth_regs(stream, T, V, E, _n.ptr(D), _n.ptr(ei), _n.ptr(rl), float(lam_deform), float(lam_rigid),
                                                           float(lam_mom), _n.ptr(loss), _n.ptr(grad), _n.ptr(scratch),
                                                           *([None] * 4 if csr is None else [_n.ptr(c) for c in csr])),
                         "csplat_cloth_regs")
        if defer:       # the kernel writes into `loss` / `grad`, which exist already: WHEN it is launched is the caller's choice
            ctx.pending = _defer(launch)                 # (launch_deferred(): e.g. behind the rasterizer's forward, off the step's critical path)
        else:
            ctx.pending = None
            launch()
        ctx.save_for_backward(grad)
        ctx.tap = bool(tap)
        if tap:     # D passes through: the gradient arriving for it and the regularisers' own leave as ONE tensor (one launch)
            return loss, D.view_as(D)
        return loss

    @staticmethod
    def backward(ctx, g, g_through=None):
        _issue(ctx.pending)
        (grad,) = ctx.saved_tensors
        if ctx.tap and g_through is not None:
            out = torch.addcmul(g_through, grad, g) if g is not None else g_through
        else:
            out = grad * g if g is not None else None
        return out, None, None, None, None, None, None, None, None


class SimulatorStep(torch.autograd.Function):
    """The head of a training step as ONE autograd node: the time-conditioned simulator for the step's T cameras
    (meshnet_network.py:361-373 per time: hidden layers, output layer, + the table rows) AND the cloth regularisers of its output
    (train_utils.py:83-102) -- graph_ops.SimResidual followed by FusedClothRegs(tap=True): the same three forward launches (the
    regularisers' queued for launch_deferred()) and three backward launches, two nodes less to record and to walk.
    Returns (vertices [T,V,3], regulariser loss)."""

    @staticmethod
    def forward(ctx, e, W1, b1, W2, b2, Wo, bo, base, edge_index, rest_len, lam_deform, lam_rigid, lam_mom, csr, defer=False):
        from meshnet import graph_ops as go
        ctx.sinks = tuple(_n.grad_sink(t) for t in (W1, b1, W2, b2, Wo, bo))       # (csplat.dist.FlatGrads: gradients written in place)
        e, W2s, h1, h2 = go._sim_hidden_fwd(e, W1, b1, W2, b2)
        y, Wo = go._rows_dot_fwd(h2, Wo, bo, base)
        T = int(e.shape[0])
        D = y.view(T, -1, 3)
        V, E = int(D.shape[1]), int(edge_index.shape[1])
        loss = torch.empty((), dtype=torch.float32, device=D.device)
        grad = torch.empty_like(D)
        ei, rl = edge_index.contiguous(), rest_len.contiguous().float()
        dev, stream, skey = D.device, _n.stream_handle(D.device), _n.scratch_stream(D.device)

        def launch():
            with _n.on_device(dev):
                key = ("regs", dev, skey, T, V, E)
                scratch = _IMG_SCRATCH.get(key)
                if scratch is None:
                    if len(_IMG_SCRATCH) >= 64:
                        _n.evict_scratch(_IMG_SCRATCH)
                    scratch = _IMG_SCRATCH[key] = torch.zeros(_n.lib.csplat_cloth_regs_scratch_bytes(T, V, E), dtype=torch.uint8, device=dev)
                _n.check(_n.lib.csplat_cloth_regs(stream, T, V, E, _n.ptr(D), _n.ptr(ei), _n.ptr(rl), float(lam_deform), float(lam_rigid),
                                                           float(lam_mom), _n.ptr(loss), _n.ptr(grad), _n.ptr(scratch), *[_n.ptr(c) for c in csr]),
                         "csplat_cloth_regs")
        if defer:      # (the caller issues it with launch_deferred(), e.g. behind the rasterizer's forward)
            ctx.pending = _defer(launch)
        else:
            ctx.pending = None
            launch()
        ctx.save_for_backward(e, W2s, h1, h2, Wo, grad)
        ctx.set_materialize_grads(False)
        return D, loss

    @staticmethod
    def backward(ctx, g_D, g_loss):
        from meshnet import graph_ops as go
        _issue(ctx.pending)
        e, W2s, h1, h2, Wo, grad = ctx.saved_tensors
        if g_D is None and g_loss is None:
            return (None,) * 15
        if g_D is None:
            g = grad * g_loss
        else:
            g = g_D.contiguous().float() if g_loss is None else torch.addcmul(g_D, grad, g_loss)
        dWo, dbo, dh = go._rows_dot_bwd(Wo, h2, g, sinks=ctx.sinks[4:6])
        dW1, db1, dW2, db2 = go._sim_hidden_bwd(e, W2s, h1, h2, dh, sinks=ctx.sinks[:4])
        return (None, dW1, db1, dW2, db2, dWo, dbo) + (None,) * 8


def simulator_step(simulator, times, gaussians, opt, defer=False, static=None):
    """(vertices [T,V,3], regulariser loss) through SimulatorStep when the simulator is the time-conditioned residual MLP on the GPU and
    the fused regularisers apply; None otherwise (the caller composes forward_times + regularization).  defer=True: the regularisers'
    kernel is queued, the caller MUST run launch_deferred() before the loss is consumed.  static = (code [T,K0], table rows [T,V,3]):
    the parameter-free inputs of the camera times in buffers of the caller's (CapturedStep refills them between replays)."""
    from meshnet import graph_ops as go
    need = ("times_on_device", "input", "hidden", "output")
    if not all(hasattr(simulator, a) for a in need) or len(times) > 8 or len(times) == 0:
        return None
    if static is not None:
        enc, base = static
    else:
        _tt, enc, base = simulator.times_on_device(times)
    if not go.sim_residual_applies(enc, simulator.input, simulator.hidden, simulator.output, base):
        return None
    ei = gaussians.mesh.edge_index
    nv = int(base.shape[1])
    key = (ei.data_ptr(), ei._version, tuple(ei.shape), nv)
    cache = getattr(gaussians, "_edge_csr", None)       # the cloth graph is static: its CSR is built once
    if cache is None or cache[0] != key:
        cache = (key, edge_csr(ei, nv))
        try:
            gaussians._edge_csr = cache
        except Exception:
            pass
    lam_d = opt.lambda_deform_mag if opt.lambda_deform_mag > 0. else 0.
    lam_r = opt.lambda_rigid if opt.lambda_rigid > 0 else 0.
    lam_m = opt.lambda_momentum if opt.lambda_momentum > 0 else 0.
    s = simulator
    return SimulatorStep.apply(enc, s.input.weight, s.input.bias, s.hidden.weight, s.hidden.bias, s.output.weight, s.output.bias, base,
                               ei, gaussians.edge_norm.reshape(-1), lam_d, lam_r, lam_m, cache[1], bool(defer))


_DEFERRED = []


def _defer(launch):
    """queue a launch for launch_deferred(); returns the queue entry [launch, issued] the node keeps: its backward issues a launch that
    nobody issued (regularization(..., defer=True) outside train_step -- ADVICE r3: the gradient would be read uninitialised; the LOSS
    value is only defined once the launch has been issued, which is the caller's contract with defer=True)"""
    ent = [launch, False]
    _DEFERRED.append(ent)
    return ent


def _issue(ent):
    if ent is None:
        return
    # the entry leaves the queue BEFORE its launch runs: a launch that raises must not stay at the head (launch_deferred would spin on an
    # entry already marked issued -- ADVICE r4)
    _DEFERRED[:] = [e for e in _DEFERRED if e is not ent]
    if not ent[1]:
        ent[1] = True
        fn, ent[0] = ent[0], None       # (the closure holds the node's tensors: drop it with the launch -- kept on the ctx it is a
        fn()                            #  reference cycle through the node's own output, and memory of a graph's private pool then
        #                                  outlives the capture: a segfault at capture_end, measured)


def launch_deferred():
    """launches what FusedClothRegs(defer=True) queued (same stream, in order); a no-op otherwise"""
    while _DEFERRED:
        _issue(_DEFERRED.pop(0))


def edge_csr(edge_index, n_nodes):
    """(dst_rowptr, dst_perm, src_rowptr, src_perm), int32: edge ids grouped by target / source vertex, ascending in a group."""
    out = []
    for row in (1, 0):
        out += list(_n.group_by_key(edge_index[row], n_nodes))
    return tuple(out)


def regularization(all_vertice_deform, gaussians, opt, static=False, fused=True, tap=False, defer=False):
    """train_utils.py:76-237 (the active terms).  On the GPU the terms and their gradient come from one kernel
    (FusedClothRegs); fused=False composes them from torch ops as upstream does (the parity reference of the tests).
    tap=True returns (loss, vertices): `vertices` is all_vertice_deform passed THROUGH the regulariser node -- render from it and the
    two gradients of the vertices (image path, regularisers) are combined in the node's backward instead of by autograd (one launch
    instead of a multiply and an add).  defer=True (with tap, on the fused path): the kernel is queued, not launched -- the caller runs
    launch_deferred() once the work that must not wait for it (the rasterizer's forward) has been issued."""
    n_cams = all_vertice_deform.shape[0]
    if fused and not static and all_vertice_deform.is_cuda and all_vertice_deform.dim() == 3:
        lam_d = opt.lambda_deform_mag if opt.lambda_deform_mag > 0. else 0.
        lam_r = opt.lambda_rigid if opt.lambda_rigid > 0 else 0.
        lam_m = opt.lambda_momentum if opt.lambda_momentum > 0 else 0.
        ei = gaussians.mesh.edge_index
        key = (ei.data_ptr(), ei._version, tuple(ei.shape), int(all_vertice_deform.shape[1]))
        cache = getattr(gaussians, "_edge_csr", None)       # the cloth graph is static: its CSR is built once
        if cache is None or cache[0] != key:
            cache = (key, edge_csr(ei, int(all_vertice_deform.shape[1])))
            try:
                gaussians._edge_csr = cache
            except Exception:
                pass
        if tap and all_vertice_deform.dtype == torch.float32 and all_vertice_deform.is_contiguous():
            return FusedClothRegs.apply(all_vertice_deform, ei, gaussians.edge_norm.reshape(-1), lam_d, lam_r, lam_m, cache[1], True,
                                        bool(defer))
        loss = FusedClothRegs.apply(all_vertice_deform, ei, gaussians.edge_norm.reshape(-1), lam_d, lam_r, lam_m, cache[1])
        return (loss, all_vertice_deform) if tap else loss
    if tap:
        return regularization(all_vertice_deform, gaussians, opt, static, fused), all_vertice_deform
    if fused and not static:
        _n.composed_fallback("train.regularization", "shape", all_vertice_deform)
    loss = torch.zeros([], device=all_vertice_deform.device)
    if not static and opt.lambda_deform_mag > 0. and n_cams >= 3:
        d0 = torch.linalg.norm(all_vertice_deform[1] - all_vertice_deform[0], dim=-1).mean()
        d1 = torch.linalg.norm(all_vertice_deform[2] - all_vertice_deform[1], dim=-1).mean()
        loss = loss + opt.lambda_deform_mag * 0.5 * (d0 + d1)
    if not static and opt.lambda_rigid > 0:
        ei = gaussians.mesh.edge_index
        # (index_select: its backward is an atomic index_add; advanced indexing would sort the 2E indices every step)
        disp = all_vertice_deform.index_select(1, ei[1]) - all_vertice_deform.index_select(1, ei[0])
        deformed_norm = torch.linalg.norm(disp, dim=-1, keepdim=True)
        static_norm = gaussians.edge_norm.unsqueeze(0).expand(n_cams, -1, -1)
        loss = loss + opt.lambda_rigid * F.l1_loss(static_norm, deformed_norm)
    if not static and opt.lambda_momentum > 0 and n_cams >= 3:
        m = all_vertice_deform[2] - 2 * all_vertice_deform[1] + all_vertice_deform[0]
        loss = loss + opt.lambda_momentum * torch.linalg.norm(m, dim=-1, ord=1).mean()
    return loss


_ONES = {}
_GT_STACKS = {}          # insertion-ordered: least recently used first
_GT_STACKS_MAX = 8


def _gt_stack(cams, device):
    """torch.cat of the cameras' ground-truth images (train_utils.py:262-270 builds it every step).  A caller that cycles through a few
    camera OBJECTS whose images never change (bench_train, the parity runs) gets the stack of a camera set built once: a small LRU
    (8 sets) keyed on the image tensors' identities and in-place versions.  The entry holds WEAK references to the source images -- an id
    recycled by a new tensor cannot alias (the dead reference no longer matches) and nothing of the caller's is pinned.  The
    reference's dataset builds a fresh Camera per item (scene_reconstruction/dataset.py:89-): such a caller never hits, and then the
    cache costs eight stale stacks at most (it used to hold up to 512 entries with strong references to the sources)."""
    import weakref
    imgs = [cam.original_image for cam in cams]
    key = tuple((id(t), t._version) for t in imgs) + (str(device),)
    hit = _GT_STACKS.get(key)
    if hit is not None and all(r() is t for r, t in zip(hit[0], imgs)):
        _GT_STACKS[key] = _GT_STACKS.pop(key)          # most recently used: to the back
        return hit[1]
    stack = torch.cat([t.to(device).unsqueeze(0) for t in imgs], 0)
    _GT_STACKS.pop(key, None)
    while len(_GT_STACKS) >= _GT_STACKS_MAX:
        _GT_STACKS.pop(next(iter(_GT_STACKS)))
    _GT_STACKS[key] = ([weakref.ref(t) for t in imgs], stack)
    return stack


@torch.no_grad()
def step_stats(grads, radii_list, P, dev, dtype=torch.float32, out_vsg=None):
    """train_utils.py:276-285 for the cameras of a step: (sum of the screen-space gradients [P,3], largest radii [P], visible [P] bool).
    On the GPU one launch (csplat_step_stats) for up to 16 cameras; a camera whose gradient is None counts as zero.  out_vsg: an fp32
    [P,3] tensor the sum is written into (the tail of the view-parallel step's flat buffer) instead of fresh memory."""
    if not radii_list:
        return (torch.zeros(P, 3, dtype=dtype, device=dev), torch.zeros(P, dtype=torch.int32, device=dev),
                torch.zeros(P, dtype=torch.bool, device=dev))
    V = len(radii_list)
    ok = V <= 16 and all(r.is_cuda and r.dtype == torch.int32 and r.is_contiguous() and r.numel() == P for r in radii_list) and \
        all(g is None or (g.is_cuda and g.dtype == torch.float32 and g.is_contiguous() and g.numel() == 3 * P) for g in grads)
    if ok:
        vsg = out_vsg if (out_vsg is not None and out_vsg.is_cuda and out_vsg.dtype == torch.float32 and out_vsg.is_contiguous() and
                          out_vsg.numel() == 3 * P) else torch.empty(P, 3, dtype=torch.float32, device=dev)
        radii = torch.empty(P, dtype=torch.int32, device=dev)
        vis = torch.empty(P, dtype=torch.bool, device=dev)
        gp = (C.c_void_p * V)(*[None if g is None else g.data_ptr() for g in grads])
        rp = (C.c_void_p * V)(*[r.data_ptr() for r in radii_list])
        with _n.on_device(dev):
            _n.check(_n.lib.csplat_step_stats(_n.stream_handle(dev), P, V, gp, rp, _n.ptr(vsg), _n.ptr(radii), _n.ptr(vis)), "csplat_step_stats")
        return vsg.to(dtype), radii, vis
    if radii_list[0].is_cuda:
        _n.composed_fallback("train.step_stats", "shape" if V > 16 else "dtype", radii_list[0])
    live = [g for g in grads if g is not None]
    vsg = torch.stack(live).sum(0) if live else torch.zeros(P, 3, dtype=dtype, device=dev)
    radii = torch.stack(list(radii_list), 0).max(dim=0).values
    return vsg, radii, radii > 0


def _root_one(loss):
    """a resident 1.0 as the root gradient of `loss.backward()` (autograd otherwise launches a fill for it every step)"""
    key = (loss.device, loss.dtype)
    if key not in _ONES:
        _ONES[key] = torch.ones((), dtype=loss.dtype, device=loss.device)
    return _ONES[key]


def _geometry_weights(opt):
    """(lambda_depth, lambda_silhouette) of an options namespace; absent = 0.  A term is on when its weight is > 0."""
    lam_d, lam_s = float(getattr(opt, "lambda_depth", 0.0) or 0.0), float(getattr(opt, "lambda_silhouette", 0.0) or 0.0)
    if lam_d < 0.0 or lam_s < 0.0:
        raise ValueError(f"train_step: lambda_depth and lambda_silhouette are >= 0, got {lam_d}, {lam_s}")
    return lam_d, lam_s


def _geometry_targets(cams, lam_d, lam_s):
    """the cameras' `depth` / `silhouette` images of the terms that are on (float32, [1,H,W] or [H,W]) -> (depths or None, silhouettes or
    None); ValueError for a camera that lacks a field or carries another shape or dtype, for cameras of different sizes and for a mask
    that is not one float32 plane -- all from the host-side attributes, before anything is launched"""
    sizes = {(int(c.image_height), int(c.image_width)) for c in cams}
    if len(sizes) > 1:
        raise ValueError(f"train_step: the depth and silhouette terms need cameras of one image size, got {sorted(sizes)}")

    def field(cam, name, what, needed=True):
        t = getattr(cam, name, None)
        if t is None and not needed:
            return None
        H, W = int(cam.image_height), int(cam.image_width)
        if not torch.is_tensor(t):
            raise ValueError(f"train_step: {what} needs every camera's `{name}` (a float32 [1,{H},{W}] or [{H},{W}] tensor), "
                             f"got {type(t).__name__}")
        if t.dtype != torch.float32 or tuple(t.shape) not in ((1, H, W), (H, W)):
            raise ValueError(f"train_step: camera.{name} is {t.dtype} {tuple(t.shape)}, expected float32 [1,{H},{W}] or [{H},{W}]")
        return t

    for cam in cams:
        field(cam, "mask", "a masked depth / silhouette term", needed=False)
    return ([field(c, "depth", "lambda_depth > 0") for c in cams] if lam_d > 0.0 else None,
            [field(c, "silhouette", "lambda_silhouette > 0") for c in cams] if lam_s > 0.0 else None)


def _chamfer_weight(opt):
    """(lambda_chamfer, squared cap or None) of an options namespace; absent = 0.  The term is on when the weight is > 0."""
    lam = float(getattr(opt, "lambda_chamfer", 0.0) or 0.0)
    if not lam >= 0.0:
        raise ValueError(f"train_step: lambda_chamfer is >= 0, got {lam}")
    cap = getattr(opt, "chamfer_max_dist", None)
    if cap is not None:
        cap = float(cap)
        if not cap >= 0.0:
            raise ValueError(f"train_step: chamfer_max_dist is a distance >= 0 (or None), got {cap}")
        cap = cap * cap
    return lam, cap


def _chamfer_targets(cams):
    """the cameras' observed point clouds (`points`, float32 [n,3], n >= 1, world coordinates); ValueError for a camera that lacks the
    field or carries another shape or dtype -- from the host-side attributes, before anything is launched"""
    out = []
    for cam in cams:
        t = getattr(cam, "points", None)
        if not torch.is_tensor(t):
            raise ValueError(f"train_step: lambda_chamfer > 0 needs every camera's `points` (a float32 [n,3] tensor), got {type(t).__name__}")
        if t.dtype != torch.float32 or t.dim() != 2 or t.shape[1] != 3 or t.shape[0] == 0:
            raise ValueError(f"train_step: camera.points is {t.dtype} {tuple(t.shape)}, expected float32 [n,3] with n >= 1")
        out.append(t)
    return out


def _neighbour_options(opt, iteration=None, static=False):
    """the kNN-graph regularisers' options of a namespace (absent = 0 / off): dict(lams=(isometric, spring, rigidity), lambda_w, k,
    update, reg_iter, iso_abs); ValueError for a bad value.  With `iteration` given: None unless the term is ON -- some weight > 0, the
    step is not static, iteration > reg_iter."""
    lams = []
    for name in ("lambda_isometric", "lambda_spring", "lambda_rigidity"):
        v = float(getattr(opt, name, 0.0) or 0.0)
        if not (v >= 0.0 and v <= 3.0e38):
            raise ValueError(f"train_step: {name} is a finite number >= 0, got {v}")
        lams.append(v)
    o = dict(lams=tuple(lams), on=max(lams) > 0.0)
    if not o["on"]:
        return None if iteration is not None else o
    lw = getattr(opt, "lambda_w", None)
    o["lambda_w"] = 2000.0 if lw is None else float(lw)
    if not (o["lambda_w"] >= 0.0 and o["lambda_w"] <= 3.0e38):
        raise ValueError(f"train_step: lambda_w is a finite number >= 0, got {o['lambda_w']}")
    for key, name, default, least in (("k", "k_nearest", 20, 1), ("update", "knn_update_iter", 1000, 1), ("reg_iter", "reg_iter", 0, 0)):
        v = getattr(opt, name, None)
        v = default if v is None else v
        if isinstance(v, bool) or not isinstance(v, int) or v < least:
            raise ValueError(f"train_step: {name} is an integer >= {least}, got {v!r}")
        o[key] = v
    if o["k"] > 32:
        raise ValueError(f"train_step: k_nearest is at most 32 (simple_knn.MAX_K), got {o['k']}")
    o["iso_abs"] = bool(getattr(opt, "isometric_abs", False))
    if iteration is not None and (static or iteration <= o["reg_iter"]):
        return None
    return o


def _neighbour_graph(gaussians, iteration, o):
    """the step's NeighbourGraph: the exact k-NN graph of the detached, UNDEFORMED centres, cached on the Gaussians object; rebuilt when
    absent, when the number of Gaussians (or k / lambda_w) has changed, and every knn_update_iter iterations"""
    from .knn_regs import NeighbourGraph
    key = (int(gaussians.num_gaussians), o["k"], o["lambda_w"])
    cached = gaussians.__dict__.get("_neighbour_graph")
    if cached is None or cached[0] != key or iteration % o["update"] == 0:
        with torch.no_grad():
            pts = gaussians.get_xyz().detach().float().contiguous()
        cached = gaussians._neighbour_graph = (key, NeighbourGraph.from_points(pts, o["k"], o["lambda_w"]), iteration)
    return cached[1]


def train_step(iteration, viewpoint_cams, gaussians, simulator, meshnet_optimizer, pipe=DEFAULT_PIPE, opt=DEFAULT_OPT,
               background=None, static=False, view_parallel=False, batched_views=True, densify_opt=None, time_allreduce=False, captured=False,
               _cap=None):
    """One optimisation step.  Returns (psnr, loss, stats) where stats holds what densification consumes.
    batched_views=True renders the step's cameras in one rasterizer call (gaussian_renderer.render_views).
    densify_opt: OptimizationParams-like namespace (+ cameras_extent, white_background) -> the reference's densification /
    pruning / opacity-reset schedule runs between backward and the optimizer step (csplat/densify.py).

    view_parallel=True with more than one rank in the default process group reproduces the SINGLE-GPU step on the full camera
    list (train_utils.py:240-321) with the cameras dealt round-robin over the ranks (csplat/dist.py):
      * the simulator and the cloth regularisers run on ALL cameras on every rank -- the regularisers couple the (t-1, t, t+1)
        triple, which a shard would break -- and enter the local loss with weight 1/world;
      * the image loss is a mean over all images: the local mean enters with weight n_local / n_total; a rank without a camera
        contributes zero but joins the collectives;
      * every parameter gradient, the screen-space gradient sum, the PSNR and the loss value travel in ONE all-reduce(sum) of
        the persistent flat buffer the `.grad` tensors are views of; the radii take one all-reduce(max).
    After the reduction every rank holds exactly the gradients and statistics of the one-rank step (up to summation order)
    and takes the same optimizer / densification decisions, so the replicas stay identical without exchanging parameters.

    Depth and silhouette supervision: `opt.lambda_depth` / `opt.lambda_silhouette` (absent = 0; a term is on when its weight is > 0) add
    lambda_depth * L_depth + lambda_silhouette * L_sil of geometry_losses() to the loss -- the views' RenderResults.depth and alpha images
    (render_views(..., return_alpha=True)) against `camera.depth` (measured z-depth, holes 0 / negative / NaN / Inf) and
    `camera.silhouette` (in [0, 1]), float32 [1,H,W] or [H,W], weighted by `camera.mask` when the cameras carry one.  stats then holds
    "depth_loss" / "silhouette_loss" (detached device scalars) for the terms that are on.  ValueError before the simulator runs: a camera
    without the field of a term that is on, or with another shape or dtype; cameras of different sizes.  NotImplementedError, also before
    anything runs: a view-parallel step (csplat.dist.is_dist()) and batched_views=False -- the terms are computed on the batched path only.
    captured=True runs such a step eagerly.  With both weights 0 or absent the step is exactly the one above.

    Point-cloud supervision: `opt.lambda_chamfer` (absent = 0; on when > 0) adds lambda_chamfer * the mean over the step's cameras of
    csplat.pointcloud.chamfer_distance(camera.points, the camera's deformed Gaussian centres, two_sided=False, max_sq_dist=
    opt.chamfer_max_dist ** 2 when that option is set) -- `camera.points`: the observed cloud, float32 [n,3] in world coordinates, n
    free per camera.  stats then holds "chamfer_loss" (the detached mean, a device scalar).  The rules are the geometry terms':
    ValueError before the simulator runs for a camera without `points` or with another shape or dtype; NotImplementedError before
    anything runs for a view-parallel step and for batched_views=False; captured=True runs such a step eagerly.  With the weight 0 or
    absent nothing is added to the step.

    kNN-graph regularisers (csplat.knn_regs): `opt.lambda_isometric`, `opt.lambda_spring`, `opt.lambda_rigidity` (absent = 0) add
    neighbour_regularization(the views' means3D_deform, the views' rotations, in camera order) on the k-NN graph of the undeformed
    centres -- `opt.k_nearest` (absent: 20), `opt.lambda_w` (absent: 2000; w = exp(-lambda_w d^2)), rebuilt every `opt.knn_update_iter`
    iterations (absent: 1000) and after the number of Gaussians changed; `opt.isometric_abs` (absent: the reference's signed isometry
    term).  The term is on when some weight is > 0, the step is not static and iteration > `opt.reg_iter` (absent: 0).  stats then
    holds "isometric_loss", "spring_loss", "rigidity_loss" (detached device scalars, unweighted; 0 for rigidity without its weight).  ValueError before the simulator
    runs: a bad option value, num_gaussians <= k_nearest; NotImplementedError before anything runs: a view-parallel step,
    batched_views=False; captured=True runs such a step eagerly.  With all three weights 0 or absent nothing is added to the step."""
    if captured and _cap is None:     # the step as a replayed hipGraph (CapturedStep below); falls back to this function when it must
        cs = gaussians.__dict__.get("_captured_step")
        if cs is None or not cs.matches(simulator, meshnet_optimizer, pipe, opt, background):
            cs = gaussians._captured_step = CapturedStep(gaussians, simulator, meshnet_optimizer, pipe, opt, background)
        if not (static or view_parallel or not batched_views or densify_opt is not None):
            return cs(iteration, viewpoint_cams)
    all_cams = list(viewpoint_cams)
    lam_depth, lam_sil = _geometry_weights(opt)
    geom = (lam_depth > 0.0 or lam_sil > 0.0) and bool(all_cams)
    geom_z = geom_s = None
    if geom:
        if view_parallel and cd.is_dist():
            raise NotImplementedError("train_step: the depth and silhouette terms are not part of the view-parallel step")
        if not batched_views:
            raise NotImplementedError("train_step: the depth and silhouette terms need batched_views=True")
        geom_z, geom_s = _geometry_targets(all_cams, lam_depth, lam_sil)
    lam_chamfer, chamfer_cap = _chamfer_weight(opt)
    chamfer_pts = None
    if lam_chamfer > 0.0 and all_cams:
        if view_parallel and cd.is_dist():
            raise NotImplementedError("train_step: the Chamfer term is not part of the view-parallel step")
        if not batched_views:
            raise NotImplementedError("train_step: the Chamfer term needs batched_views=True")
        chamfer_pts = _chamfer_targets(all_cams)
    nbr = _neighbour_options(opt, iteration, static) if all_cams else None
    if nbr is not None:
        if view_parallel and cd.is_dist():
            raise NotImplementedError("train_step: the kNN-graph regularisers are not part of the view-parallel step")
        if not batched_views:
            raise NotImplementedError("train_step: the kNN-graph regularisers need batched_views=True")
        if int(gaussians.num_gaussians) <= nbr["k"]:
            raise ValueError(f"train_step: {int(gaussians.num_gaussians)} Gaussians have no k_nearest = {nbr['k']} neighbours each")
    if iteration % 1000 == 0 and _cap is None:
        gaussians.oneupSHdegree()
    _DEFERRED.clear()                 # (a launch queued by a step that raised before issuing it)
    n_total = len(all_cams)
    world, rank = cd.world_rank() if view_parallel else (1, 0)
    dist_mode = view_parallel and cd.is_dist()          # (world > 1, or one rank under CSPLAT_FORCE_DIST: csplat/dist.py)
    idx = cd.shard_indices(n_total, rank, world) if dist_mode else list(range(n_total))
    cams = [all_cams[i] for i in idx]
    P = int(gaussians.num_gaussians)
    fg = None
    if dist_mode:
        # one flat buffer: [Gaussian parameters | simulator parameters | tail].  The Gaussian gradients -- ~95 % of the bytes -- are final
        # as soon as the rasterizer's backward and the mesh-transform adjoint have run: their slice is exchanged then (early bucket),
        # under the simulator's and the regularisers' backward.  Tail: the summed screen-space gradient [3P], PSNR, loss, and every
        # rank's largest radii in its own [P] slot (zeros elsewhere), so that the max over ranks rides in the SAME sum
        gparams = list(gaussians.parameters())
        fg = cd.flat_grads_for(gaussians, gparams + list(simulator.parameters()), extra=3 * P + 2 + world * P, early=len(gparams))
        fg.bind(key=(bool(static), n_total))
    images, gts, radii_l, vsp_l, verts = [], [], [], [], []
    masks = [] if all_cams and getattr(all_cams[0], "mask", None) is not None else None          # train_utils.py:256
    stacked = reg = deforms = None
    if not static and all_cams and (dist_mode or (batched_views and hasattr(simulator, "forward_times"))):
        # simulator for all cameras at once, and the regularisers recorded BEFORE the rasterizer: autograd runs
        # later-recorded nodes first, so the rasterizer's backward -- the long GPU work of the step -- is launched
        # first and the small launches of everything else are issued under it
        head = simulator_step(simulator, [cam.time for cam in all_cams], gaussians, opt, defer=True,
                              static=None if _cap is None else _cap["sim_in"]) if gaussians.mesh.pos.is_cuda else None
        if head is not None:      # simulator + regularisers: one autograd node (the regularisers' launch queued, see launch_deferred)
            deforms_all, reg = head
        else:
            if hasattr(simulator, "forward_times"):
                deforms_all = simulator.forward_times([cam.time for cam in all_cams])
            else:
                nv, dev0 = gaussians.mesh.pos.shape[0], gaussians.mesh.pos.device
                deforms_all = torch.stack([simulator(time_vector=torch.tensor(cam.time).to(dev0).repeat(nv, 1)) for cam in all_cams])
            # (defer: the regularisers feed nothing before the loss -- their launch waits until the rasterizer's forward has been issued)
            reg, deforms_all = regularization(deforms_all, gaussians, opt, static, tap=True, defer=True)
        deforms = deforms_all if not dist_mode else (deforms_all[idx] if idx else None)
    alphas = None
    if geom:
        pkgs, stacked, alphas = render_views(cams, gaussians, simulator, pipe, background, render_static=static, return_stacked=True,
                                             vertice_deforms=deforms, by_products=False, return_alpha=True)
    elif dist_mode or batched_views:
        pkgs, stacked = render_views(cams, gaussians, simulator, pipe, background, render_static=static, return_stacked=True,
                                     vertice_deforms=deforms, by_products=False) if cams else ([], None)
    else:
        pkgs = [render(cam, gaussians, simulator, pipe, background, render_static=static) for cam in cams]
    launch_deferred()
    for cam, pkg in zip(cams, pkgs):
        images.append(pkg.render.unsqueeze(0))
        radii_l.append(pkg.radii.unsqueeze(0))
        vsp_l.append(pkg.viewspace_points)
        if masks is not None:
            masks.append(cam.mask.to(pkg.render.device).unsqueeze(0))                      # train_utils.py:273-274
        verts.append(pkg.vertice_deform[None])
    dev = gaussians.face_bary.device
    if reg is None:
        reg = regularization(torch.cat(verts, 0), gaussians, opt, static) if verts else torch.zeros((), device=dev)
    psnr_ = None
    geom_stats = {}
    if geom:
        # the two terms and their sum with the regularisers: two launches (and one in backward); the sum then rides into the image loss
        # where the regularisers alone would
        gdev = alphas[0].device
        reg, gl_d, gl_s = geometry_losses([pkg.depth for pkg in pkgs], alphas,
                                          None if geom_z is None else [t.to(gdev) for t in geom_z],
                                          None if geom_s is None else [t.to(gdev) for t in geom_s], lam_depth, lam_sil,
                                          masks=None if masks is None else [m[0] for m in masks], add=reg)
        if lam_depth > 0.0:
            geom_stats["depth_loss"] = gl_d.detach()
        if lam_sil > 0.0:
            geom_stats["silhouette_loss"] = gl_s.detach()
    if chamfer_pts is not None:
        # observed cloud -> deformed Gaussian centres, per camera (the clouds differ in size); the mean rides into the image loss with the
        # regularisers
        from .pointcloud import chamfer_distance
        terms = [chamfer_distance(t.to(pkg.means3D_deform.device), pkg.means3D_deform, two_sided=False, max_sq_dist=chamfer_cap)
                 for t, pkg in zip(chamfer_pts, pkgs)]
        chamfer_mean = torch.stack(terms).mean()
        reg = reg + lam_chamfer * chamfer_mean
        geom_stats["chamfer_loss"] = chamfer_mean.detach()
    if nbr is not None:
        # isometry, spring and rigidity of the deformed centres / rotations over the step's time rows: one launch (and one in backward);
        # the sum rides into the image loss with the regularisers
        from .knn_regs import neighbour_regularization
        graph = _neighbour_graph(gaussians, iteration, nbr)
        # (without a rigidity weight the rotations are not handed over: nothing of them is read, rigidity_loss reports 0)
        nb_loss, nb_parts = neighbour_regularization(torch.stack([pkg.means3D_deform for pkg in pkgs]),
                                                     torch.stack([pkg.rotations for pkg in pkgs]) if nbr["lams"][2] > 0.0 else None,
                                                     graph, *nbr["lams"], isometric_abs=nbr["iso_abs"])
        reg = reg + nb_loss
        geom_stats["isometric_loss"], geom_stats["spring_loss"], geom_stats["rigidity_loss"] = nb_parts.unbind(0)
    if cams:
        image_tensor = stacked if stacked is not None else torch.cat(images, 0)
        gt_image_tensor = _gt_stack(cams, image_tensor.device) if _cap is None else _cap["gt"]
        mask_tensor = torch.cat(masks, 0) if masks is not None else None
        w_img = 1.0 if len(cams) == n_total else len(cams) / n_total
        if _image_loss_fusable(image_tensor, gt_image_tensor, opt, mask_tensor) and reg.dtype == torch.float32:
            # image loss + PSNR + the sum with the regularisers: one launch (and one in backward)
            loss, psnr_, _ = FusedImageLoss.apply(image_tensor, gt_image_tensor, opt.lambda_dssim, mask_tensor, reg, w_img,
                                                  1.0 / world if dist_mode else 1.0, 1.0 / max(n_total, 1))
            if _cap is not None:      # a recorded step: its log line (go word, PSNR, loss, counts) leaves for the host HERE, half a step early
                _cap["log"](psnr_, loss)
        else:
            psnr_sum = psnr(image_tensor, gt_image_tensor).sum().double()
            image_loss = image_losses(image_tensor, gt_image_tensor, opt, mask_tensor)
            if len(cams) != n_total:
                image_loss = image_loss * (len(cams) / n_total)
    else:   # a rank without a camera of this step
        psnr_sum = torch.zeros((), dtype=torch.float64, device=dev)
        image_loss = torch.zeros((), dtype=gaussians.face_bary.dtype, device=dev)
    if psnr_ is None:
        loss = image_loss + (reg / world if dist_mode else reg)
        psnr_ = psnr_sum / max(n_total, 1)
    if loss.requires_grad:
        try:
            loss.backward(gradient=_root_one(loss))
        finally:
            if fg is not None:
                fg.unbind()           # (the gradient sinks are for this backward only)
    viewspace_grad, radii, visibility_filter = step_stats([v.grad for v in vsp_l], [r.reshape(-1) for r in radii_l], P, dev,
                                                          gaussians.face_bary.dtype,
                                                          out_vsg=fg.tail[:3 * P].view(P, 3) if (fg is not None and radii_l) else None)
    loss_value = loss.detach()
    with torch.no_grad():
        if dist_mode:
            if viewspace_grad.data_ptr() != fg.tail.data_ptr():       # (csplat_step_stats wrote the sum into the tail already otherwise)
                fg.tail[:3 * P].copy_(viewspace_grad.reshape(-1))
            fg.tail[3 * P] = psnr_.to(fg.tail.dtype)
            fg.tail[3 * P + 1] = loss_value.to(fg.tail.dtype)
            slots = fg.tail[3 * P + 2:].view(world, P)
            slots[rank].copy_(radii)                          # (radii < 2^24: exact in fp32; the other ranks' slots stay zero)
            fg.all_reduce(timed=time_allreduce)
            fg.drop_untouched(key=(bool(static), n_total))
            viewspace_grad = fg.tail[:3 * P].view(P, 3).clone()
            psnr_, loss_value = fg.tail[3 * P].double(), fg.tail[3 * P + 1].clone()
            radii = slots.max(dim=0).values.to(radii.dtype)   # train_utils.py:276-277 over all ranks' cameras
            visibility_filter = radii > 0        # == torch.cat(vis_l).any(dim=0): some camera sees it <=> its largest radius > 0
        if densify_opt is not None and iteration < densify_opt.densify_until_iter:      # train_utils.py:295-304
            densification(gaussians, iteration, visibility_filter, radii, viewspace_grad, densify_opt,
                          getattr(densify_opt, "cameras_extent", 1.0))
            if iteration % densify_opt.opacity_reset_interval == 0 or (
                    getattr(densify_opt, "white_background", False) and iteration == densify_opt.densify_from_iter):
                gaussians.reset_opacity()
        if densify_opt is not None and getattr(densify_opt, "bary_cleanup", 0) and iteration % densify_opt.bary_cleanup == 0:
            gaussians.cleanup_barycentric_coordinates()                                  # train_utils.py:306-307
        # (GroupedAdam.step_now / zero_grad_now: the same step without torch.optim's per-call wrapper; any other optimizer: its own)
        if _cap is not None:          # recorded under stream capture: step count, learning rates and the go / no-go word live on the device
            gaussians.optimizer.step_captured(_cap["valid"])
            meshnet_optimizer.step_captured(_cap["valid"])
        else:
            getattr(gaussians.optimizer, "step_now", gaussians.optimizer.step)()
            if not static:
                getattr(meshnet_optimizer, "step_now", meshnet_optimizer.step)()
        zg = getattr(gaussians.optimizer, "zero_grad_now", None)
        zg() if zg is not None else gaussians.optimizer.zero_grad(set_to_none=True)
        zg = getattr(meshnet_optimizer, "zero_grad_now", None)
        zg() if zg is not None else meshnet_optimizer.zero_grad()
    return psnr_, loss_value, dict(viewspace_grad=viewspace_grad, radii=radii, visibility_filter=visibility_filter,
                                   allreduce_ms=fg.last_allreduce_ms if fg is not None else 0.0, **geom_stats)


class CapturedStep:
    """train_step recorded ONCE into a hipGraph and replayed (the reference times its step with an event pair around
    the loop body, train.py:146,178 -- the GPU work of a step, which is what a replayed graph costs).

    The eager step is bound by the host: ~33 launches of 5-300 us, ~25 us of Python and launch overhead each, and one read of the
    forward's counts in the middle.  Recorded, the launches cost the host nothing -- which needs a step without a single per-step host
    value in its launches:
      * the rasterizer's forward is launched ON FAITH (csplat_forward_views_faith): both phases with capacities from the last eager
        step's counts + 1/8, nothing read back; a device word `valid` says whether the counts fitted, every kernel of the second phase
        and of the backward leaves an unfitting step alone, and BOTH Adam steps honour the same word (csplat_adam_step_dev: step count
        and learning rates on the device too) -- a miss changes no parameter, no moment, no count;
      * camera matrices, the simulator's time inputs and the ground-truth images live in buffers of this object that are refilled
        between replays (only when the cameras changed);
      * ONE host read per step, at its end: [valid, PSNR, loss, the views' counts] arrive in pinned memory through a copy node of the
        graph.  valid == 0 -> the step is repeated eagerly (exact sizes) and the graph is re-recorded with new capacities at the next
        call; counts within 3 % of a capacity re-record too, before a miss happens.
    One graph per step SHAPE: (number of cameras, image size, field of view, number of Gaussians, active SH degree, parameter storage,
    pipe.antialiasing).
    Falls back to the eager train_step for what it does not cover: masks, a static stage, view-parallel runs, densification steps, the
    depth and silhouette terms (opt.lambda_depth / opt.lambda_silhouette > 0), the Chamfer term (opt.lambda_chamfer > 0), the kNN-graph
    regularisers (opt.lambda_isometric / opt.lambda_spring / opt.lambda_rigidity > 0)."""

    MARGIN = 8          # capacities = counts + counts / MARGIN (+ a constant)

    def __init__(self, gaussians, simulator, meshnet_optimizer, pipe=DEFAULT_PIPE, opt=DEFAULT_OPT, background=None):
        self.g, self.sim, self.mopt, self.pipe, self.opt, self.bg = gaussians, simulator, meshnet_optimizer, pipe, opt, background
        self.graphs = {}
        self.stats = {"eager": 0, "recorded": 0, "replayed": 0, "missed": 0, "rerecorded_early": 0}

    def matches(self, simulator, meshnet_optimizer, pipe, opt, background):
        return simulator is self.sim and meshnet_optimizer is self.mopt and pipe is self.pipe and opt is self.opt and background is self.bg

    # ---- shape of a step
    def _key(self, cams):
        c0 = cams[0]
        g = self.g
        return (len(cams), int(c0.image_height), int(c0.image_width), float(c0.FoVx), float(c0.FoVy), int(g.num_gaussians),
                int(g.active_sh_degree), tuple(int(p.data_ptr()) for p in g.parameters()),
                tuple(int(p.data_ptr()) for p in self.sim.parameters()), bool(getattr(self.pipe, "antialiasing", False)))

    def _coverable(self, cams):
        from .optim import GroupedAdam
        return (len(cams) >= 2 and len(cams) <= 8 and all(getattr(c, "mask", None) is None for c in cams) and
                max(_geometry_weights(self.opt)) == 0.0 and       # (a depth / silhouette term: the rasterizer refuses its gradients on a forward launched on faith)
                _chamfer_weight(self.opt)[0] == 0.0 and           # (the Chamfer term: the observed clouds' sizes are per camera, not part of a step's shape)
                not _neighbour_options(self.opt)["on"] and          # (the kNN-graph regularisers: the graph is refreshed on the host's schedule)
                len({(int(c.image_height), int(c.image_width), float(c.FoVx), float(c.FoVy)) for c in cams}) == 1 and
                self.g.mesh.pos.is_cuda and isinstance(self.g.optimizer, GroupedAdam) and isinstance(self.mopt, GroupedAdam) and
                not (int(_n.lib.csplat_debug_flags_query()) & _n.DEBUG_UNBATCHED) and      # (global sort, per-view launches; the bit-reproducible K7, bit 8, is served by the batched path since round 6)
                all(hasattr(self.sim, a) for a in ("times_on_device", "input", "hidden", "output")))

    def _eager(self, iteration, cams):
        import diff_gaussian_rasterization as dgr
        self.stats["eager"] += 1
        with dgr.forward_mode(keep_info=True):      # (the step's counts stay readable on the device: the next recording's capacities)
            return train_step(iteration, cams, self.g, self.sim, self.mopt, self.pipe, self.opt, self.bg)

    # ---- static inputs
    def _fill(self, st, cams):
        """the cameras of this call -> the graph's input buffers (skipped when they are the objects of the previous call)"""
        if st["cams_seen"] is not None and len(st["cams_seen"]) == len(cams) and all(a is b for a, b in zip(st["cams_seen"], cams)) and \
                st["times_seen"] == tuple(float(c.time) for c in cams):
            return
        dev = st["gt"].device
        for i, c in enumerate(cams):
            st["view"][i].copy_(c.world_view_transform.to(dev).reshape(16), non_blocking=True)
            st["proj"][i].copy_(c.full_proj_transform.to(dev).reshape(16), non_blocking=True)
            st["campos"][i].copy_(c.camera_center.to(dev).reshape(3), non_blocking=True)
            st["gt"][i].copy_(c.original_image.to(dev), non_blocking=True)
        _tt, enc, base = self.sim.times_on_device([c.time for c in cams])
        st["enc"].copy_(enc)
        st["base"].copy_(base.reshape(st["base"].shape))
        st["cams_seen"], st["times_seen"] = list(cams), tuple(float(c.time) for c in cams)

    def _record(self, key, cams, caps):
        import diff_gaussian_rasterization as dgr
        g = self.g
        dev = g.face_bary.device
        T = len(cams)
        c0 = cams[0]
        H, W = int(c0.image_height), int(c0.image_width)
        _tt, enc, base = self.sim.times_on_device([c.time for c in cams])
        st = {"view": torch.zeros(T, 16, device=dev), "proj": torch.zeros(T, 16, device=dev), "campos": torch.zeros(T, 3, device=dev),
              "gt": torch.zeros(T, 3, H, W, device=dev), "enc": torch.zeros_like(enc), "base": torch.zeros_like(base),
              "valid": torch.zeros(1, dtype=torch.int32, device=dev), "cams_seen": None, "times_seen": None, "caps": tuple(int(c) for c in caps)}
        scams = [SimpleNamespace(image_height=H, image_width=W, FoVx=c0.FoVx, FoVy=c0.FoVy, world_view_transform=st["view"][i].view(4, 4),
                                 full_proj_transform=st["proj"][i].view(4, 4), camera_center=st["campos"][i], time=float(cams[i].time),
                                 original_image=st["gt"][i], mask=None) for i in range(T)]
        self._fill(st, cams)
        g.optimizer.captured_setup()
        self.mopt.captured_setup()
        for p in list(g.parameters()) + list(self.sim.parameters()):
            p.grad = None
        torch.cuda.synchronize(dev)
        graph = torch.cuda.CUDAGraph()
        faith = {"caps": st["caps"], "valid": st["valid"]}
        n_log = 4 + 3 * T
        st["host"] = torch.zeros(n_log, dtype=torch.float32).pin_memory()
        st["host_seq"] = torch.full((1,), -1.0, dtype=torch.float32).pin_memory()
        st["packed"] = torch.zeros(n_log, dtype=torch.float32, device=dev)
        seq_src = g.optimizer._cap["state"]        # steps taken BEFORE this one: the host knows the value it waits for

        def log(psnr_t, loss_t):
            srcs = [seq_src, st["valid"], psnr_t.reshape(1), loss_t.reshape(1)] + list(faith["info"])
            kinds = [1, 1, 0, 0] + [2] * T          # (the views' counts travel as raw int32 bits: exact at any size)
            counts = [1, 1, 1, 1] + [3] * T
            n = len(srcs)
            keep = [t if t.dtype in (torch.float32, torch.int32) else t.float() for t in srcs]
            pp = (C.c_void_p * n)(*[t.data_ptr() for t in keep])
            with _n.on_device(dev):
                _n.check(_n.lib.csplat_gather_words(_n.stream_handle(dev), n, C.cast(pp, C.c_void_p), C.cast((C.c_int * n)(*kinds), C.c_void_p),
                                                    C.cast((C.c_int * n)(*counts), C.c_void_p), _n.ptr(st["packed"])), "csplat_gather_words")
            # two copy nodes: the line, then the word the host spins on -- when the second has landed the first has
            st["host"].copy_(st["packed"], non_blocking=True)
            st["host_seq"].copy_(st["packed"][0:1], non_blocking=True)
            st["_keep"] = keep
        from .graphs import capture
        with dgr.forward_mode(faith=faith, replay_device=dev):
            with capture(graph):          # (the cyclic collector is held off during the capture: csplat/graphs.py)
                ps, loss, stats = train_step(0, scams, g, self.sim, self.mopt, self.pipe, self.opt, self.bg,
                                             _cap={"sim_in": (st["enc"], st["base"]), "gt": st["gt"], "valid": st["valid"], "log": log})
        # what the recording's raw pointers depend on: the ticketed scratch caches and both optimizers' device words
        st.update(graph=graph, psnr=ps, loss=loss, stats=stats, epochs=self._epochs())
        self.graphs[key] = st
        self.stats["recorded"] += 1
        return st

    def _caps_from_counts(self, counts):
        from .graphs import caps_from_counts
        return caps_from_counts(counts, self.MARGIN)

    def _epochs(self):
        return (_n.SCRATCH_EPOCH[0], self.g.optimizer.__dict__.get("_cap", {}).get("epoch"), self.mopt.__dict__.get("_cap", {}).get("epoch"))

    def _counts_of_last_eager(self):
        import diff_gaussian_rasterization as dgr
        return torch.stack(list(dgr.LAST_INFO)).cpu().tolist() if dgr.LAST_INFO else None

    def __call__(self, iteration, cams):
        cams = list(cams)
        # (a step that raises the SH degree, and whatever the graph does not cover, is an ordinary train_step)
        if iteration % 1000 == 0 or not self._coverable(cams):
            return self._eager(iteration, cams)
        key = self._key(cams)
        st = self.graphs.get(key)
        if st is None:
            # first step of a shape: eager -- it creates the optimizer state and leaves the exact counts the capacities are taken from
            out = self._eager(iteration, cams)
            counts = self._counts_of_last_eager()
            if counts is not None:
                if len(self.graphs) >= 8:
                    self.graphs.clear()
                self.graphs[key] = {"graph": None, "pending_caps": self._caps_from_counts(counts)}
            return out
        if st.get("graph") is not None and st["epochs"] != self._epochs():
            # a scratch cache was evicted (an entry point failed, a cache overflowed) or an optimizer's device words were re-allocated since
            # this graph was recorded: its raw pointers may be dangling -- never replay it; record again with the same capacities
            self.stats["rerecorded_stale"] = self.stats.get("rerecorded_stale", 0) + 1
            st = self.graphs[key] = {"graph": None, "pending_caps": st["caps"]}
        if st.get("graph") is None:
            st = self._record(key, cams, st["pending_caps"])
        else:
            self._fill(st, cams)
        self.g.optimizer.captured_refresh_lr()
        self.mopt.captured_refresh_lr()
        expect = float(int(self.g.optimizer._cap["items"][0][1]["step"].item()))      # (a CPU tensor: the host-side step counter)
        st["host_seq"][0] = -1.0            # (the previous replay's copies have landed: its line was read)
        st["graph"].replay()
        # the step's log line leaves the GPU right behind the image loss -- half a step before the step ends -- and the host only waits for
        # THAT: it returns to the caller (and issues the next replay) while the backward and the optimizer steps still run
        host, seq = st["host"], st["host_seq"]
        spins = 0
        while float(seq[0]) != expect:
            spins += 1
            if spins > 200000:          # (seconds: something is wrong -- fall back to the stream)
                torch.cuda.current_stream(st["gt"].device).synchronize()
                if float(seq[0]) != expect:
                    raise RuntimeError(f"CapturedStep: the recorded step reported step count {float(seq[0])}, expected {expect}")
                break
        if float(host[1]) != 1.0:           # the counts outgrew the capacities: nothing was applied -- repeat eagerly, re-record next time
            self.stats["missed"] += 1
            self.graphs.pop(key, None)
            out = self._eager(iteration, cams)
            counts = self._counts_of_last_eager()
            if counts is not None:
                self.graphs[key] = {"graph": None, "pending_caps": self._caps_from_counts(counts)}
            return out
        self.stats["replayed"] += 1
        self.g.optimizer.captured_advance_host()
        self.mopt.captured_advance_host()
        T = len(cams)
        counts = host[4:4 + 3 * T].view(torch.int32).view(T, 3)
        caps = st["caps"]
        psnr_v, loss_v = host[2].clone(), host[3].clone()        # (the pinned line is overwritten by the next replay)
        if int(counts[:, 0].max()) > 0.97 * caps[0] or int(counts[:, 1].max()) > 0.97 * caps[1] or int(counts[:, 2].max()) > 0.97 * caps[2]:
            # close to a capacity: re-record with room before a step is lost (the results of this replay are final -- copies are returned)
            self.graphs[key] = {"graph": None, "pending_caps": self._caps_from_counts(counts.tolist())}
            self.stats["rerecorded_early"] += 1
            return psnr_v, loss_v, {k: (v.clone() if torch.is_tensor(v) else v) for k, v in st["stats"].items()}
        return psnr_v, loss_v, dict(st["stats"])
