"""Optical-flow supervision of the Gaussians' motion between the frames of a step (csplat_flow_loss_fwd / _bwd, include/csplat.h): the
FlowLoss node, the `where`-based torch composition of the same formulas, and flow_losses(), which validates the arguments and chooses
between them.  Re-exported by csplat.train, whose train_step adds the term when opt.lambda_flow is > 0."""
import torch
from torch.autograd.function import once_differentiable

from . import native as _n


MAX_FRAMES = 16          # csplat_flow_loss.hip: FL_FRAMES
# workgroup partials of csplat_flow_loss_fwd: one buffer per (device, stream, frames, Gaussians)
_FLOW_SCRATCH = _n.ScratchCache(cap=64)


class FlowLoss(torch.autograd.Function):
    """the flow term of a step's T frames as ONE node (include/csplat.h, csplat_flow_loss_fwd, states the semantics): forward is two
    launches (one gather pass over the T P rows, which also writes the unit gradient [T,P,3] when one is wanted, + a one-workgroup
    sum), backward one (g weight lambda unit).  The frames' centres are separate tensors (the renderer's means3D_deform): they reach
    the library as a pointer table, nothing is stacked, and their gradients are slices of the one buffer the backward launch wrote.
    dims = (T, P, W, H, lambda, max_error or 0, weight, add_weight, visible present per frame, masks given); tensors = T points + T
    full_proj + (T-1) flows + the present visibilities + the (T-1) masks.  Returns (weight lambda L_flow + add_weight add, L_flow,
    valid pairs); only the first is differentiable, in the points and add."""

    @staticmethod
    def forward(ctx, dims, add, *tensors):
        T, P, W, H, lam, cap, weight, add_weight, vis_on, has_m = dims
        _n.require_cuda(*tensors)
        X, full, F = list(tensors[:T]), list(tensors[T:2 * T]), list(tensors[2 * T:3 * T - 1])
        rest = list(tensors[3 * T - 1:])
        vis = None
        if any(vis_on):
            vis = [rest.pop(0) if on else None for on in vis_on]
        M = rest if has_m else None
        dev = X[0].device
        need = any(ctx.needs_input_grad[2:2 + T])
        out = torch.empty(2, dtype=torch.float32, device=dev)
        count = torch.empty(1, dtype=torch.int32, device=dev)
        unit = torch.empty(T, P, 3, dtype=torch.float32, device=dev) if need else None
        addc = None if add is None else add.reshape(1).float()
        scratch = _FLOW_SCRATCH.buffer(dev, (T, P), lambda: _n.lib.csplat_flow_loss_scratch_bytes(T, P))
        _n.launch("csplat_flow_loss_fwd", dev, T, P, W, H, _n.ptr_table(X), _n.ptr_table(full), _n.ptr_table(F), _n.ptr_table(vis), _n.ptr_table(M),
                  float(cap), float(lam), float(weight), _n.ptr(addc), float(add_weight), _n.ptr(unit), _n.ptr(scratch), _n.ptr(out),
                  _n.ptr(count))
        ctx.save_for_backward(unit)
        ctx.dims = (T, P, float(lam), float(weight), float(add_weight), add is not None, len(tensors))
        loss, lf, nv = out[0], out[1], count[0]
        ctx.mark_non_differentiable(lf, nv)
        ctx.set_materialize_grads(False)
        return loss, lf, nv

    @staticmethod
    @once_differentiable
    def backward(ctx, g, _gl, _gn):
        T, P, lam, weight, w_add, has_add, n_in = ctx.dims
        if g is None:
            return (None,) * (2 + n_in)
        unit, = ctx.saved_tensors
        g = g.reshape(1).float()
        grads = [None] * T
        if unit is not None:
            dev = unit.device
            d = torch.empty(T, P, 3, dtype=torch.float32, device=dev)
            _n.launch("csplat_flow_loss_bwd", dev, T, P, _n.ptr(unit), lam, weight, _n.ptr(g), _n.ptr(d))
            grads = [d[t] if ctx.needs_input_grad[2 + t] else None for t in range(T)]      # slices of the one buffer the launch wrote
        gadd = None
        if has_add and ctx.needs_input_grad[1]:
            gadd = g.reshape(()) if w_add == 1.0 else g.reshape(()) * w_add
        return (None, gadd) + tuple(grads) + (None,) * (n_in - T)


def _project(X, full, W, H):
    """gaussian_renderer._project -> (x, y, w), each [P]"""
    hom = X[:, 0:1] * full[0] + X[:, 1:2] * full[1] + X[:, 2:3] * full[2] + full[3]
    w = hom[:, 3]
    return ((hom[:, 0] / w + 1.0) * W - 1.0) * 0.5, ((hom[:, 1] / w + 1.0) * H - 1.0) * 0.5, w


def _flow_composed(X, full, F, W, H, vis, M, cap):
    """the formulas of csplat_flow_loss_fwd from torch operations, in the dtype of the points: selection by `where` on the INPUTS, so that
    an unselected NaN neither reaches the sum nor, through 0 * NaN, the gradient -> (L_flow, valid pairs)"""
    T, P = len(X), X[0].shape[0]
    dt = X[0].dtype
    zero = X[0].new_zeros(())
    total, count = zero, torch.zeros((), dtype=torch.int64, device=X[0].device)
    proj = []
    for t in range(T):
        with torch.no_grad():
            x_, y_, w_ = _project(X[t], full[t].to(dt), W, H)
            row = torch.isfinite(x_) & torch.isfinite(y_) & torch.isfinite(w_)
        # (a row that does not project to numbers is replaced BEFORE the differentiable projection: 0 * NaN in its backward otherwise)
        proj.append(_project(torch.where(row[:, None], X[t], zero), full[t].to(dt), W, H) + (row,))
    for t in range(T - 1):
        (xa, ya, wa, ra), (xb, yb, wb, rb) = proj[t], proj[t + 1]
        flow = F[t].to(dt)
        ok = (wa > 0) & (wb > 0) & ra & rb
        ok = ok & (xa >= 0) & (xa <= W - 1) & (ya >= 0) & (ya <= H - 1)
        for v in (None if vis is None else vis[t], None if vis is None else vis[t + 1]):
            if v is not None:
                ok = ok & (v > 0)
        xs, ys = torch.where(ok, xa, zero), torch.where(ok, ya, zero)          # (a point that is out keeps no path to the sum)
        x0f, y0f = torch.floor(xs.detach()), torch.floor(ys.detach())
        x0, y0 = x0f.long().clamp(0, W - 1), y0f.long().clamp(0, H - 1)
        x1, y1 = (x0 + 1).clamp(max=W - 1), (y0 + 1).clamp(max=H - 1)
        fx, fy = xs - x0f, ys - y0f
        taps = [flow[:, yy, xx] for yy, xx in ((y0, x0), (y0, x1), (y1, x0), (y1, x1))]          # each [2,P]
        for tap in taps:
            ok = ok & torch.isfinite(tap).all(dim=0)
        f00, f01, f10, f11 = [torch.where(ok, tap, zero) for tap in taps]
        g = (1.0 - fy) * ((1.0 - fx) * f00 + fx * f01) + fy * ((1.0 - fx) * f10 + fx * f11)
        if M is not None:
            xm = torch.floor(xs.detach() + 0.5).long().clamp(0, W - 1)
            ym = torch.floor(ys.detach() + 0.5).long().clamp(0, H - 1)
            m = M[t].to(dt)[ym, xm]
            ok = ok & torch.isfinite(m) & (m > 0)
            m = torch.where(ok, m, zero)
        else:
            m = torch.ones_like(xs)
        rx = torch.where(ok, xb, zero) - xs - g[0]
        ry = torch.where(ok, yb, zero) - ys - g[1]
        e = rx.abs() + ry.abs()
        if cap is not None:
            ok = ok & (e.detach() <= cap)
        total = total + torch.where(ok, m * e, zero).sum()
        count = count + ok.sum()
    return total / float((T - 1) * P), count


def _image(name, t, like, shapes, what):
    """one flow image or mask as a tensor on the points' device -> ValueError for another type or shape (nothing touches the device)"""
    if not torch.is_tensor(t):
        try:
            import numpy as np
            if isinstance(t, np.ndarray):
                t = torch.from_numpy(t)
        except ImportError:
            pass
    if not torch.is_tensor(t):
        raise ValueError(f"flow_losses: `{name}` holds a {type(t).__name__}, not a tensor or numpy array")
    if tuple(t.shape) not in shapes:
        raise ValueError(f"flow_losses: a `{name}` image of shape {tuple(t.shape)}; {what}")
    if not t.dtype.is_floating_point:
        raise ValueError(f"flow_losses: a `{name}` image of dtype {t.dtype}, expected a floating-point image")
    if t.requires_grad:
        raise ValueError(f"flow_losses: `{name}` are constants (requires_grad is set on one)")
    return t.reshape(shapes[0]).to(like.device)


def flow_losses(points, full_projs, flows, image_size, visible=None, masks=None, lambda_flow=1.0, max_error=None, add=None, weight=1.0,
                add_weight=1.0):
    """Optical-flow supervision of the motion of P Gaussians over T consecutive frames -> (total, L_flow, n_valid), device scalars:
        total  = weight * lambda_flow * L_flow + add_weight * add
        L_flow = (1/n) sum over the VALID pairs of m (|r_x| + |r_y|),  r = (p_b - p_a) - bilinear(F_t, p_a),  n = (T - 1) P
    with p_a / p_b the projections of Gaussian i in frames t / t+1, F_t the flow image of frame t and m the mask weight at the pixel
    nearest to p_a (include/csplat.h, csplat_flow_loss_fwd: validity, selection semantics, sign(0) = 0, the full gradient).
      points       a list of T [P,3] tensors or one [T,P,3] tensor, 2 <= T <= 16
      full_projs   T [4,4] tensors, camera.full_proj_transform (hom = [X, 1] @ full)
      flows        T-1 (or T, the last ignored) [2,H,W] or [1,2,H,W] float tensors or numpy arrays: dx, dy in pixels at frame t's pixels;
                   a NaN / Inf pixel means "no flow here"
      image_size   (H, W), one size for all frames
      visible      None, or T int32 / bool [P] tensors (entries may be None): the rasterizer's radii; `Visibility.weight_max > thr` from
                   gaussian_renderer.render_visibility is the occlusion-aware choice
      masks        None, or T-1 (or T) [H,W] / [1,H,W] float images: the cameras' masks
      max_error    None, or a cap > 0 in pixels: a pair whose |r_x| + |r_y| exceeds it is dropped (occlusions, wrong flow)
    Only `total` is differentiable, in the points and add.  ValueError before anything touches the device for every malformed argument.
    float32 contiguous GPU tensors take the HIP kernels (FlowLoss); anything else composes the same formulas from torch operations
    (reported through csplat.native.composed_fallback for GPU tensors: raises under STRICT; it is the CPU path)."""
    lam = float(lambda_flow)
    if not (lam >= 0.0 and lam <= 3.0e38):
        raise ValueError(f"flow_losses: lambda_flow is a finite number >= 0, got {lam}")
    cap = None if max_error is None else float(max_error)
    if cap is not None and not (cap > 0.0 and cap <= 3.0e38):
        raise ValueError(f"flow_losses: max_error is a finite number > 0 (or None), got {cap}")
    if torch.is_tensor(points):
        if points.dim() != 3:
            raise ValueError(f"flow_losses: `points` as one tensor is [T,P,3], got {tuple(points.shape)}")
        points = list(points.unbind(0))
    points = list(points) if points is not None else []
    T = len(points)
    if T < 2 or T > MAX_FRAMES:
        raise ValueError(f"flow_losses: {T} frames; the term takes 2 to {MAX_FRAMES}")
    like = points[0]
    if not torch.is_tensor(like) or like.dim() != 2 or like.shape[1] != 3 or like.shape[0] < 1 or not like.dtype.is_floating_point:
        raise ValueError("flow_losses: `points` holds floating-point [P,3] tensors with P >= 1")
    P = int(like.shape[0])
    for t in points:
        if not torch.is_tensor(t) or tuple(t.shape) != (P, 3) or t.dtype != like.dtype or t.device != like.device:
            raise ValueError(f"flow_losses: the frames' points are [P,3] tensors of one size, dtype and device; got "
                             f"{tuple(t.shape) if torch.is_tensor(t) else type(t).__name__} next to {(P, 3)}")
    if (T - 1) * P >= 2 ** 31:
        raise ValueError(f"flow_losses: {(T - 1) * P} pairs; the term takes fewer than 2^31")
    try:
        H, W = int(image_size[0]), int(image_size[1])
    except (TypeError, IndexError, ValueError):
        raise ValueError(f"flow_losses: `image_size` is (H, W), got {image_size!r}") from None
    if H < 1 or W < 1:
        raise ValueError(f"flow_losses: `image_size` is (H, W) with both >= 1, got {(H, W)}")
    full_projs = list(full_projs) if full_projs is not None else []
    if len(full_projs) != T:
        raise ValueError(f"flow_losses: {len(full_projs)} `full_projs` for {T} frames")
    for f in full_projs:
        if not torch.is_tensor(f) or tuple(f.shape) != (4, 4) or not f.dtype.is_floating_point:
            raise ValueError("flow_losses: `full_projs` holds floating-point [4,4] tensors (camera.full_proj_transform)")
        if f.requires_grad:
            raise ValueError("flow_losses: the cameras are constants of this term (requires_grad is set on a `full_projs` entry)")
    flows = list(flows) if flows is not None else []
    if len(flows) not in (T - 1, T):
        raise ValueError(f"flow_losses: {len(flows)} `flows` for {T} frames; one per pair ({T - 1}), or one per frame with the last ignored")
    F = [_image("flows", f, like, ((2, H, W), (1, 2, H, W)), f"a flow image is [2,H,W] or [1,2,H,W] of the one size {(H, W)}")
         for f in flows[:T - 1]]
    M = None
    if masks is not None:
        masks = list(masks)
        if len(masks) not in (T - 1, T):
            raise ValueError(f"flow_losses: {len(masks)} `masks` for {T} frames; one per pair ({T - 1}), or one per frame with the last ignored")
        M = [_image("masks", m, like, ((H, W), (1, H, W)), f"a mask is [H,W] or [1,H,W] of the one size {(H, W)}") for m in masks[:T - 1]]
    vis = None
    if visible is not None:
        visible = list(visible)
        if len(visible) != T:
            raise ValueError(f"flow_losses: {len(visible)} `visible` entries for {T} frames")
        vis = []
        for v in visible:
            if v is not None:
                if not torch.is_tensor(v) or v.numel() != P or v.dtype not in (torch.int32, torch.bool) or v.device != like.device:
                    raise ValueError(f"flow_losses: `visible` holds int32 or bool [P] tensors on the points' device (or None), got "
                                     f"{(v.dtype, tuple(v.shape), str(v.device)) if torch.is_tensor(v) else type(v).__name__}")
                v = v.reshape(P)
                v = v.to(torch.int32) if v.dtype == torch.bool else v
            vis.append(v)
        if all(v is None for v in vis):
            vis = None
    if add is not None and (not torch.is_tensor(add) or add.numel() != 1 or add.device != like.device):
        raise ValueError("flow_losses: `add` is a scalar tensor on the points' device")
    full = [f.to(like.device) for f in full_projs]
    if like.is_cuda:
        why = _n.why_not_f32c(*points, *full, *F, *(M or []), *([] if add is None else [add]))
        if why is None and vis is not None and not all(v is None or v.is_contiguous() for v in vis):
            why = "layout"
        if why is None:
            dims = (T, P, W, H, lam, 0.0 if cap is None else cap, float(weight), float(add_weight),
                    tuple(v is not None for v in vis) if vis is not None else (False,) * T, M is not None)
            tensors = points + full + F + ([v for v in vis if v is not None] if vis is not None else []) + (M or [])
            return FlowLoss.apply(dims, add, *tensors)
        _n.composed_fallback("train.flow_losses", why, like)
    lf, count = _flow_composed(points, full, F, W, H, vis, M, cap)
    total = (float(weight) * lam) * lf
    if add is not None:
        total = total + add_weight * add.reshape(())
    return total, lf.detach(), count.to(torch.int32)
