"""Restatement of the optical-flow term (include/csplat.h, csplat_flow_loss_fwd) in torch, float64 or float32, `where`-based; autograd
supplies the gradient (abs'(0) = 0 in torch, which is the term's sign(0) = 0).

T frames of P Gaussians, pair t = (frame t -> frame t+1), n = (T - 1) P.  Per pair and Gaussian:
    p_a, p_b   projections of X_t[i] / X_{t+1}[i]:  hom = [X, 1] @ full,  x = ((hom_x / w + 1) W - 1) / 2,  y likewise with H
    g          bilinear(F_t, p_a): x0 = floor(x), x1 = min(x0 + 1, W - 1), fx = x - x0 (the same in y)
    m          M_t[floor(y + 0.5)][floor(x + 0.5)] clamped to the image (1 without masks)
    r          (p_b - p_a) - g,   e = |r_x| + |r_y|
    valid      visible_t > 0, visible_{t+1} > 0, w_a > 0, w_b > 0, p_a and p_b finite, p_a inside [0, W-1] x [0, H-1], the eight taps
               finite, m finite and > 0, e <= max_error when a cap is given
    L_flow     (1/n) sum_valid m e          total = weight lambda L_flow + add_weight add
Non-finite flow taps are replaced BEFORE they are sampled and finiteness is decided on the originals: a NaN that only `where` keeps out
of the forward value still reaches the gradient as 0 * NaN.

flow_loss() also returns, per pair, the DECISION MARGIN in pixels: the smallest of |r_x|, |r_y| (the signs), the distances of x_a, y_a
to the nearest integer (cell and image edges), of x_a + 0.5, y_a + 0.5 to the nearest integer when masks are given (the mask pixel) and
|e - max_error| when a cap is given.  A pair whose margin is below a few float32 ulps of a pixel coordinate may be decided the other
way by a float32 evaluation; pairs that are invalid for a reason no rounding can change (visibility, w <= 0, far outside) have margin
+inf."""
import torch


def project(X, full, W, H):
    hom = X[:, 0:1] * full[0] + X[:, 1:2] * full[1] + X[:, 2:3] * full[2] + full[3]
    w = hom[:, 3]
    return ((hom[:, 0] / w + 1.0) * W - 1.0) * 0.5, ((hom[:, 1] / w + 1.0) * H - 1.0) * 0.5, w


def _frac_dist(v):
    """distance to the nearest integer"""
    return (v - torch.round(v)).abs()


def flow_loss(points, fulls, flows, W, H, visible=None, masks=None, max_error=None, lam=1.0, add=None, weight=1.0, add_weight=1.0,
              g=1.0, dtype=torch.float64, want_grad=True):
    """points: T tensors [P,3]; fulls: T [4,4]; flows: T-1 [2,H,W]; visible: None or T entries (None or [P] ints); masks: None or T-1
    [H,W] -> dict(total, L, count, grad [T,P,3] (d(g total)/d points), valid [T-1,P] bool, margin [T-1,P], m [T-1,P]) in `dtype`"""
    T = len(points)
    X = [p.detach().cpu().to(dtype).clone().requires_grad_(want_grad) for p in points]
    P = X[0].shape[0]
    zero = torch.zeros((), dtype=dtype)
    inf = torch.full((P,), float("inf"), dtype=dtype)
    proj = []
    for t in range(T):
        full = fulls[t].detach().cpu().to(dtype)
        with torch.no_grad():
            x_, y_, w_ = project(X[t], full, W, H)
            row_ok = torch.isfinite(x_) & torch.isfinite(y_) & torch.isfinite(w_)
        # a row that does not project to numbers is replaced BEFORE the differentiable projection (0 * NaN in its backward otherwise)
        proj.append(project(torch.where(row_ok[:, None], X[t], zero), full, W, H) + (row_ok,))
    total = zero
    valids, margins, ms = [], [], []
    for t in range(T - 1):
        (xa, ya, wa, oka), (xb, yb, wb, okb) = proj[t], proj[t + 1]
        F = flows[t].detach().cpu().reshape(2, H, W).to(dtype)
        hard = (wa > 0) & (wb > 0) & oka & okb
        if visible is not None:
            for v in (visible[t], visible[t + 1]):
                if v is not None:
                    hard = hard & (v.detach().cpu().reshape(P) > 0)
        inside = (xa >= 0) & (xa <= W - 1) & (ya >= 0) & (ya <= H - 1)
        ok = hard & inside
        xs, ys = torch.where(ok, xa, zero), torch.where(ok, ya, zero)
        x0f, y0f = torch.floor(xs.detach()), torch.floor(ys.detach())
        x0, y0 = x0f.long().clamp(0, W - 1), y0f.long().clamp(0, H - 1)
        x1, y1 = (x0 + 1).clamp(max=W - 1), (y0 + 1).clamp(max=H - 1)
        fx, fy = xs - x0f, ys - y0f
        fin = torch.isfinite(F)
        Fs = torch.where(fin, F, zero)          # sanitised BEFORE sampling; finiteness from the originals
        taps_ok = fin[:, y0, x0] & fin[:, y0, x1] & fin[:, y1, x0] & fin[:, y1, x1]
        ok = ok & taps_ok.all(dim=0)
        f00, f01, f10, f11 = Fs[:, y0, x0], Fs[:, y0, x1], Fs[:, y1, x0], Fs[:, y1, x1]
        gs = (1.0 - fy) * ((1.0 - fx) * f00 + fx * f01) + fy * ((1.0 - fx) * f10 + fx * f11)
        if masks is not None:
            Mt = masks[t].detach().cpu().reshape(H, W).to(dtype)
            xm = torch.floor(xs.detach() + 0.5).long().clamp(0, W - 1)
            ym = torch.floor(ys.detach() + 0.5).long().clamp(0, H - 1)
            m = Mt[ym, xm]
            ok = ok & torch.isfinite(m) & (m > 0)
            m = torch.where(ok, m, zero)
        else:
            m = torch.ones(P, dtype=dtype)
        rx = torch.where(ok, xb, zero) - xs - gs[0]
        ry = torch.where(ok, yb, zero) - ys - gs[1]
        e = rx.abs() + ry.abs()
        before_cap = ok
        if max_error is not None:
            ok = ok & (e.detach() <= max_error)
        total = total + torch.where(ok, m * e, zero).sum()
        # the decision margin: only where a rounding could change something -- the hard conditions hold and the point is inside or within
        # a pixel of the image
        with torch.no_grad():
            near = hard & (xa > -1) & (xa < W) & (ya > -1) & (ya < H)
            mg = torch.minimum(_frac_dist(xa), _frac_dist(ya))
            if masks is not None:
                mg = torch.minimum(mg, torch.minimum(_frac_dist(xa + 0.5), _frac_dist(ya + 0.5)))
            live = before_cap
            mg = torch.where(live, torch.minimum(mg, torch.minimum(rx.abs(), ry.abs())), mg)
            if max_error is not None:
                mg = torch.where(live, torch.minimum(mg, (e - max_error).abs()), mg)
            margins.append(torch.where(near, mg, inf))
        valids.append(ok)
        ms.append(m.detach())
    L = total / float((T - 1) * P)
    out_total = (float(weight) * float(lam)) * L
    if add is not None:
        out_total = out_total + float(add_weight) * add.detach().cpu().reshape(()).to(dtype)
    grad = None
    if want_grad:
        if L.requires_grad:
            grads = torch.autograd.grad(float(g) * out_total, X, allow_unused=True)
            grad = torch.stack([torch.zeros(P, 3, dtype=dtype) if gr is None else gr for gr in grads])
        else:
            grad = torch.zeros(T, P, 3, dtype=dtype)
    valid = torch.stack(valids)
    return dict(total=out_total.detach(), L=L.detach(), count=int(valid.sum()), grad=grad, valid=valid, margin=torch.stack(margins),
                m=torch.stack(ms))


def ortho_full(W, H):
    """a full_proj under which pixel = (X, Y) and w = 1"""
    full = torch.zeros(4, 4, dtype=torch.float64)
    full[0, 0], full[1, 1] = 2.0 / W, 2.0 / H
    full[3] = torch.tensor([1.0 / W - 1.0, 1.0 / H - 1.0, 0.0, 1.0], dtype=torch.float64)
    return full
