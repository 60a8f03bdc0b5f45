"""Depth and silhouette supervision of a step's views (csplat_geom_loss_fwd / _bwd, include/csplat.h): the GeometryLoss node, the
float64 composition of the same formulas, and geometry_losses(), which validates the views and chooses between them.  Re-exported by
csplat.train, whose train_step adds the term when opt.lambda_depth / opt.lambda_silhouette are > 0."""
import torch
from torch.autograd.function import once_differentiable

from . import native as _n


# workgroup partials of csplat_geom_loss_fwd: one buffer per (device, stream, views, pixels)
_GEOM_SCRATCH = _n.ScratchCache(cap=64)


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
        scratch = _GEOM_SCRATCH.buffer(dev, (V, hw), lambda: _n.lib.csplat_geom_loss_scratch_bytes(V, hw))
        _n.launch("csplat_geom_loss_fwd", dev, V, hw, _n.ptr_table(D if Z else []), _n.ptr_table(A), _n.ptr_table(Z), _n.ptr_table(S), _n.ptr_table(M),
                  float(lam_d), float(lam_s), float(weight), _n.ptr(addc), float(add_weight), _n.ptr(sign), _n.ptr(scratch), _n.ptr(out))
        ctx.save_for_backward(sign, *Z, *M)
        ctx.dims = (V, hw, float(lam_d) if Z else 0.0, float(lam_s) if S else 0.0, float(weight), float(add_weight), len(Z), len(M),
                    add is not None, [tuple(t.shape) for t in views[:2 * V]], len(views))
        loss, ld, ls = out[0], out[1], out[2]
        ctx.mark_non_differentiable(ld, ls)
        ctx.set_materialize_grads(False)
        return loss, ld, ls

    @staticmethod
    @once_differentiable
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
            _n.launch("csplat_geom_loss_bwd", dev, V, hw, _n.ptr(sign), _n.ptr_table(Z), _n.ptr_table(M), lam_d, lam_s, weight, _n.ptr(g),
                      _n.ptr(gD), _n.ptr(gA))
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
