"""Restatement of the geometry loss (include/csplat.h, csplat_geom_loss_fwd) in torch, float64 or float32, `where`-based.  The loss AND
both gradient images come from the closed forms below, not from autograd, so that ties (sign(0) = 0) are exact.

Per step the views v = 0..V-1 are all H x W, n = V H W.  Per view: D the rasterizer's depth image (sum T alpha z), A its alpha image,
Z measured z-depth (optional), S silhouette in [0, 1] (optional), M mask (optional):
    valid   = isfinite(Z) and Z > 0
    w_d     = valid ? (M given ? M : 1) : 0            w_s = M given ? M : 1
    r_d     = D - A Z                                  r_s = A - S
    L_depth = (1/n) sum_{w_d != 0} |r_d w_d|           L_sil = (1/n) sum_{w_s != 0} |r_s w_s|
    total   = weight (lambda_depth L_depth + lambda_silhouette L_sil) + add_weight add
    dL/dD   = g weight lambda_depth w_d sign(r_d w_d) / n
    dL/dA   = g weight (-lambda_depth w_d Z sign(r_d w_d) + lambda_silhouette w_s sign(r_s w_s)) / n
A pixel with w == 0 contributes exactly 0 and receives exactly 0, whatever D, A, Z hold there (selection, not multiplication); a NaN in
D or A where w != 0 makes that term NaN."""
import torch


def _stack(views, dtype):
    return None if views is None else torch.stack([t.detach().cpu().reshape(t.shape[-2:]).to(dtype) for t in views])


def terms(D, A, Z, S, M, dtype=torch.float64):
    """-> dict of the stacked [V,H,W] quantities: w_d, w_s, r_d, r_s (None for a term whose data are absent), Z"""
    A = _stack(A, dtype)
    D, Z, S, M = _stack(D, dtype), _stack(Z, dtype), _stack(S, dtype), _stack(M, dtype)
    one, zero = torch.ones_like(A), torch.zeros_like(A)
    out = dict(A=A, Z=Z, w_d=None, r_d=None, w_s=None, r_s=None)
    if Z is not None:
        valid = torch.isfinite(Z) & (Z > 0)
        out["w_d"] = torch.where(valid, one if M is None else M, zero)
        # ONE rounding, as the kernel's fmaf(-A, Z, D): the product of two float32 is exact in float64, so float64 holds the exact sign
        out["r_d"] = (D.double() - A.double() * Z.double()).to(dtype)
    if S is not None:
        out["w_s"] = one if M is None else M
        out["r_s"] = A - S
    return out


def _sign_product(r, w):
    """sign(r w) from the two signs (the product itself may underflow); NaN where either is NaN"""
    s = torch.sign(r) * torch.sign(w)        # (torch.sign(NaN) is 0)
    return torch.where(torch.isnan(r) | torch.isnan(w), torch.full_like(s, float("nan")), s)


def geometry_loss(D, A, Z, S, M, lambda_depth, lambda_silhouette, add=None, weight=1.0, add_weight=1.0, g=1.0, dtype=torch.float64):
    """-> (total, L_depth, L_sil, dL/dD [V,H,W], dL/dA [V,H,W], sign codes [V,H,W] uint8) in `dtype`.  A term is on when its data are given
    and its weight is > 0.  The codes are the kernel's byte: bits 0-1 sign(r_d w_d), bits 2-3 sign(r_s w_s), as 0: -1, 1: 0, 2: +1, 3: NaN."""
    if not lambda_depth > 0:
        Z = None
    if not lambda_silhouette > 0:
        S = None
    t = terms(D if Z is not None else None, A, Z, S, M, dtype)
    A_ = t["A"]
    n = float(A_.numel())
    zero = torch.zeros_like(A_)
    L_d = L_s = torch.zeros((), dtype=dtype)
    gD, gA = zero.clone(), zero.clone()
    code_d = torch.ones_like(A_, dtype=torch.uint8)
    code_s = torch.ones_like(A_, dtype=torch.uint8)

    def code(s):
        return torch.where(torch.isnan(s), torch.full_like(s, 3.0), s + 1.0).to(torch.uint8)

    gg = torch.tensor(float(g) * float(weight), dtype=dtype)
    if Z is not None:
        on = t["w_d"] != 0
        L_d = torch.where(on, (t["r_d"] * t["w_d"]).abs(), zero).sum() / n
        s = torch.where(on, _sign_product(t["r_d"], t["w_d"]), zero)
        gD = torch.where(on, gg * lambda_depth * t["w_d"] * s / n, zero)
        gA = torch.where(on, -gg * lambda_depth * t["w_d"] * t["Z"] * s / n, zero)
        code_d = code(s)
    if S is not None:
        on = t["w_s"] != 0
        L_s = torch.where(on, (t["r_s"] * t["w_s"]).abs(), zero).sum() / n
        s = torch.where(on, _sign_product(t["r_s"], t["w_s"]), zero)
        gA = gA + torch.where(on, gg * lambda_silhouette * t["w_s"] * s / n, zero)
        code_s = code(s)
    total = weight * ((lambda_depth * L_d if Z is not None else 0.0) + (lambda_silhouette * L_s if S is not None else 0.0))
    total = torch.as_tensor(total, dtype=dtype)
    if add is not None:
        total = total + add_weight * add.detach().cpu().reshape(()).to(dtype)
    return total, L_d, L_s, gD, gA, code_d | (code_s << 2)


def differentiable_loss(D, A, Z, S, M, lambda_depth, lambda_silhouette):
    """the same total from differentiable torch operations on stacked [V,H,W] leaves D, A (for autograd checks of the closed forms on
    inputs without ties and without unselected NaNs)"""
    n = float(A.numel())
    one, zero = torch.ones_like(A), torch.zeros_like(A)
    total = torch.zeros((), dtype=A.dtype)
    if Z is not None and lambda_depth > 0:
        valid = torch.isfinite(Z) & (Z > 0)
        w = torch.where(valid, one if M is None else M, zero)
        Zs = torch.where(valid, Z, zero)
        total = total + lambda_depth * torch.where(w != 0, ((D - A * Zs) * w).abs(), zero).sum() / n
    if S is not None and lambda_silhouette > 0:
        w = one if M is None else M
        total = total + lambda_silhouette * torch.where(w != 0, ((A - S) * w).abs(), zero).sum() / n
    return total
