"""fp64 torch restatement of the antialiased rasterizer forward (helper of the antialiasing tests, not collected).

tests/feature_ref.py's forward (camera tensors as inputs, colour, depth, feature and alpha images) with the opacity compensation of
include/csplat.h, CSPLAT_ANTIALIAS:
    (a0, b, c0) = T Sigma T^T (the cov2D before its 0.3 px^2 dilation)
    det0 = a0 c0 - b^2,  det1 = (a0 + 0.3)(c0 + 0.3) - b^2,  h = sqrt(max(2.5e-5, det0 / det1)),  o' = o h
and every use of the opacity takes o'.  The tile lists and sorted ids come from the C oracle's namespace `o` (the tile rectangle is that of
the dilated cov2D, which antialiasing leaves alone), but the termination is computed here, from o' (raster_torch.render's
own_termination rule): the oracle's n_contrib was found with the raw opacity.  With antialiasing=False the result is that of
camera_ref.render / feature_ref.render (tests/test_antialias_cpu.py holds that bit for bit)."""
import numpy as np
import torch

from oracle import raster_torch as rt
from camera_ref import camera_tensors  # noqa: F401  (re-exported: the camera leaves of the oracle's inputs)

DILATE, FLOOR = 0.3, 2.5e-5


def aa_factor(a0, b, c0):
    """h of the undilated cov2D entries (tensors); the floor stops the gradient where it is active"""
    det0 = a0 * c0 - b * b
    det1 = (a0 + DILATE) * (c0 + DILATE) - b * b
    return torch.sqrt(torch.clamp_min(det0 / det1, FLOOR))


def render(o, means3D, means2D, opacities, V, Pm, campos, bg, features=None, shs=None, colors_precomp=None, scales=None, rotations=None,
           cov3D_precomp=None, antialiasing=True, own_termination=True):
    """-> (color [3,H,W], depth [1,H,W], feat [F,H,W] or None, alpha [1,H,W], n_contrib [H,W] int64, aux); tensors float64,
    features [P, F]; aux = {"h": h [P], "cov2": the undilated cov2D [P, 2, 2] (detached)}.  own_termination=False takes the oracle's
    n_contrib (valid with antialiasing=False only)."""
    i = o._inputs
    W, H = o.W, o.H
    f64 = torch.float64
    tanx, tany, mod = float(i.tanfovx), float(i.tanfovy), float(i.scale_mod)
    fx, fy = W / (2 * tanx), H / (2 * tany)
    P = means3D.shape[0]
    ph = torch.cat([means3D, torch.ones(P, 1, dtype=f64)], 1)
    pv = ph @ V
    hom = ph @ Pm
    pw = 1.0 / (hom[:, 3] + 1e-7)
    ndc = hom[:, :2] * pw[:, None] + means2D[:, :2]
    px = ((ndc[:, 0] + 1.0) * W - 1.0) * 0.5
    py = ((ndc[:, 1] + 1.0) * H - 1.0) * 0.5
    if cov3D_precomp is None:
        R = rt._rot(rotations)
        A = R * (mod * scales)[:, None, :]
        Sig = A @ A.transpose(1, 2)
    else:
        c = cov3D_precomp
        Sig = torch.stack([c[:, 0], c[:, 1], c[:, 2], c[:, 1], c[:, 3], c[:, 4], c[:, 2], c[:, 4], c[:, 5]], 1).reshape(-1, 3, 3)
    tz = pv[:, 2]
    tz = torch.where(tz > 0.2, tz, torch.ones_like(tz))
    limx, limy = 1.3 * tanx, 1.3 * tany
    txtz, tytz = pv[:, 0] / tz, pv[:, 1] / tz
    inx = (txtz >= -limx) & (txtz <= limx)
    iny = (tytz >= -limy) & (tytz <= limy)
    tx = torch.where(inx, pv[:, 0], (txtz.clamp(-limx, limx) * tz).detach())     # the clamp stops the gradient of a clamped axis
    ty = torch.where(iny, pv[:, 1], (tytz.clamp(-limy, limy) * tz).detach())
    zero = torch.zeros_like(tz)
    J = torch.stack([fx / tz, zero, -fx * tx / (tz * tz), zero, fy / tz, -fy * ty / (tz * tz)], 1).reshape(-1, 2, 3)
    T = J @ V[:3, :3].T
    cov2 = T @ Sig @ T.transpose(1, 2)
    a = cov2[:, 0, 0] + 0.3
    b = cov2[:, 0, 1]
    c = cov2[:, 1, 1] + 0.3
    det = a * c - b * b
    det = torch.where(det == 0, torch.ones_like(det), det)
    conic = torch.stack([c / det, -b / det, a / det], 1)
    if shs is not None:
        d = means3D - campos[None]
        d = d / d.norm(dim=1, keepdim=True)
        rgb = torch.clamp_min(rt._eval_sh(o.D, shs, d) + 0.5, 0.0)
    else:
        rgb = colors_precomp
    depth = pv[:, 2]
    h = aa_factor(cov2[:, 0, 0], b, cov2[:, 1, 1])
    op = opacities.reshape(-1) * h if antialiasing else opacities.reshape(-1)
    F = features.shape[1] if features is not None else 0
    # every non-empty tile's pixels (flat indices) and values are collected and written into the images ONCE behind the loop: a slice assignment per
    # tile costs autograd a copy of the whole image per tile in the backward (hours at 30 000 tiles); the values are the same
    where, cparts, dparts, fparts, aparts = [], [], [], [], []
    gx = (W + 15) // 16
    ids_all = torch.from_numpy(o.ids.astype(np.int64))
    ncon = torch.from_numpy(o.n_contrib.astype(np.int64))
    ncon_out = torch.zeros(H, W, dtype=torch.int64)
    for t in range(o.ranges.shape[0]):
        s, e = int(o.ranges[t, 0]), int(o.ranges[t, 1])
        x0, y0 = (t % gx) * 16, (t // gx) * 16
        x1, y1 = min(x0 + 16, W), min(y0 + 16, H)
        if x1 <= x0 or y1 <= y0:
            continue
        if e <= s:          # (an empty tile keeps the background the colour image starts from)
            continue
        ys, xs = torch.meshgrid(torch.arange(y0, y1), torch.arange(x0, x1), indexing="ij")
        xs = xs.reshape(-1); ys = ys.reshape(-1)
        npx = xs.shape[0]
        where.append(ys * W + xs)
        xs = xs.to(f64); ys = ys.to(f64)
        g = ids_all[s:e]
        dx = px[g][None, :] - xs[:, None]
        dy = py[g][None, :] - ys[:, None]
        cn = conic[g]
        power = -0.5 * (cn[None, :, 0] * dx * dx + cn[None, :, 2] * dy * dy) - cn[None, :, 1] * dx * dy
        G = torch.exp(torch.clamp_max(power, 0.0))
        araw = op[g][None, :] * G
        alpha = araw + (torch.clamp_max(araw, 0.99) - araw).detach()      # straight-through at the cap
        idx = torch.arange(e - s)[None, :].expand(npx, -1)
        live = (power <= 0) & (alpha.detach() >= 1.0 / 255.0)
        if own_termination:        # (raster_torch.render's rule: the entry that would take T below 1e-4 and all behind it are not blended)
            with torch.no_grad():
                a0 = torch.where(live, alpha, torch.zeros_like(alpha))
                T0 = torch.cumprod(1.0 - a0, dim=1)
                stop = live & (T0 < 1e-4)
                dead = torch.cumsum(stop.to(torch.int64), dim=1) > 0
                live = live & ~dead
                last = torch.where(live, idx + 1, torch.zeros_like(idx)).max(dim=1).values
        else:
            last = ncon[y0:y1, x0:x1].reshape(-1)
            live = live & (idx < last[:, None])
        ncon_out[y0:y1, x0:x1] = last.reshape(y1 - y0, x1 - x0)
        alpha = torch.where(live, alpha, torch.zeros_like(alpha))
        Tincl = torch.cumprod(1.0 - alpha, dim=1)
        Tbefore = torch.cat([torch.ones(npx, 1, dtype=f64), Tincl[:, :-1]], 1)
        w = alpha * Tbefore
        Cpix = w @ rgb[g] + Tincl[:, -1][:, None] * bg[None, :]
        cparts.append(Cpix.T)
        dparts.append(w @ depth[g])
        fparts.append((w @ features[g]).T if F else torch.zeros(0, npx, dtype=f64))
        aparts.append(1.0 - Tincl[:, -1])
    at = torch.cat(where) if where else None

    def image(parts, C, base=None):      # [C, H, W] from the tiles' [C, pixels] pieces, over `base` (zeros) where no tile has a list
        base = torch.zeros(C, H * W, dtype=f64) if base is None else base
        return (base.index_copy(1, at, torch.cat(parts, 1)) if where else base.clone()).reshape(C, H, W)
    color, fimg = image(cparts, 3, bg[:, None].expand(3, H * W)), image(fparts, F)
    dimg, aimg = image([p_[None] for p_ in dparts], 1), image([p_[None] for p_ in aparts], 1)
    return color, dimg, (fimg if F else None), aimg, ncon_out, dict(h=h, cov2=cov2.detach())


def conditioning(cov2):
    """(a0 c0 + b^2) / |det0| of undilated cov2D entries [P, 2, 2]: the factor by which the cancellation in det0 = a0 c0 - b^2 amplifies
    the relative rounding of the entries in h (and in dh, which has a 1 / h)"""
    a0, b, c0 = cov2[:, 0, 0], cov2[:, 0, 1], cov2[:, 1, 1]
    return (a0 * c0 + b * b) / (a0 * c0 - b * b).abs().clamp_min(1e-300)
