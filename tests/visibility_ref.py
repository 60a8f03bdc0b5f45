"""fp64 restatement of the rasterizer's visibility outputs (helper of the visibility tests, not collected).

With w_i(pix) = T_i alpha_i, the weight with which the colour blends Gaussian i at pix (include/csplat.h, csplat_visibility_views):
    weight_max[i] = max_pix w_i(pix),  weight_sum[i] = sum_pix w_i(pix),  pixel_count[i] = #{pix : i blended at pix},
    top_id[pix] = argmax_i w_i(pix)  (-1 where nothing blended).
The walk is feature_ref.render's: geometry from the camera tensors, the tile lists and sorted ids of the C oracle's namespace `o`, the
oracle's n_contrib as the termination.  With antialiasing=True the opacity is antialias_ref's o' = o h and the termination is its own rule
(the oracle's n_contrib was found with the raw opacity)."""
import numpy as np
import torch

from oracle import raster_torch as rt
import antialias_ref

TIE = 1e-9      # top_id: any id whose weight is within TIE of the pixel's largest


def _geometry(o, means3D, opacities, V, Pm, scales=None, rotations=None, cov3D_precomp=None, antialiasing=False):
    """-> pixel centres px, py [P], conic [P, 3], opacity [P] (o' with antialiasing), the lines of feature_ref / antialias_ref.render"""
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
    ndc = hom[:, :2] * pw[:, None]
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
    tx = torch.where((txtz >= -limx) & (txtz <= limx), pv[:, 0], txtz.clamp(-limx, limx) * tz)
    ty = torch.where((tytz >= -limy) & (tytz <= limy), pv[:, 1], tytz.clamp(-limy, limy) * tz)
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
    op = opacities.reshape(-1)
    if antialiasing:
        op = op * antialias_ref.aa_factor(cov2[:, 0, 0], b, cov2[:, 1, 1])
    return px, py, conic, op


def visibility(o, means3D, opacities, V, Pm, scales=None, rotations=None, cov3D_precomp=None, antialiasing=False, top_id=None):
    """-> dict(weight_max [P], weight_sum [P], pixel_count [P] int64, top_w [H, W] (the largest weight, 0 where nothing blended),
    top_ids [H, W] (one argmax, -1 where nothing blended), at_top [H, W] (the weight of `top_id` [H, W] at its pixel, when given; 0 for
    -1), alpha [H, W] = sum_i w_i); tensor arguments float64"""
    W, H = o.W, o.H
    f64 = torch.float64
    with torch.no_grad():
        px, py, conic, op = _geometry(o, means3D, opacities, V, Pm, scales, rotations, cov3D_precomp, antialiasing)
        P = means3D.shape[0]
        wmax = torch.zeros(P, dtype=f64)
        wsum = torch.zeros(P, dtype=f64)
        cnt = torch.zeros(P, dtype=torch.int64)
        top_w = torch.zeros(H, W, dtype=f64)
        top_ids = torch.full((H, W), -1, dtype=torch.int64)
        at_top = torch.zeros(H, W, dtype=f64)
        alpha_img = torch.zeros(H, W, dtype=f64)
        tid = None if top_id is None else torch.as_tensor(np.asarray(top_id), dtype=torch.int64).reshape(H, W)
        gx = (W + 15) // 16
        ids_all = torch.from_numpy(o.ids.astype(np.int64))
        ncon = torch.from_numpy(o.n_contrib.astype(np.int64))
        for t in range(o.ranges.shape[0]):
            s, e = int(o.ranges[t, 0]), int(o.ranges[t, 1])
            x0, y0 = (t % gx) * 16, (t // gx) * 16
            x1, y1 = min(x0 + 16, W), min(y0 + 16, H)
            if x1 <= x0 or y1 <= y0 or e <= s:
                continue
            ys, xs = torch.meshgrid(torch.arange(y0, y1), torch.arange(x0, x1), indexing="ij")
            xs = xs.reshape(-1).to(f64); ys = ys.reshape(-1).to(f64)
            g = ids_all[s:e]
            dx = px[g][None, :] - xs[:, None]
            dy = py[g][None, :] - ys[:, None]
            cn = conic[g]
            power = -0.5 * (cn[None, :, 0] * dx * dx + cn[None, :, 2] * dy * dy) - cn[None, :, 1] * dx * dy
            alpha = torch.clamp_max(op[g][None, :] * torch.exp(torch.clamp_max(power, 0.0)), 0.99)
            idx = torch.arange(e - s)[None, :].expand(xs.shape[0], -1)
            live = (power <= 0) & (alpha >= 1.0 / 255.0)
            if antialiasing:       # (antialias_ref's own termination: the entry that would take T below 1e-4 and all behind it)
                T0 = torch.cumprod(1.0 - torch.where(live, alpha, torch.zeros_like(alpha)), dim=1)
                live = live & ~(torch.cumsum((live & (T0 < 1e-4)).to(torch.int64), dim=1) > 0)
            else:
                live = live & (idx < ncon[y0:y1, x0:x1].reshape(-1)[:, None])
            alpha = torch.where(live, alpha, torch.zeros_like(alpha))
            Tincl = torch.cumprod(1.0 - alpha, dim=1)
            Tbefore = torch.cat([torch.ones(xs.shape[0], 1, dtype=f64), Tincl[:, :-1]], 1)
            w = alpha * Tbefore                                   # [pixels, entries]
            wmax[g] = torch.maximum(wmax[g], w.max(dim=0).values)      # (a Gaussian is in a tile's list once)
            wsum.index_add_(0, g, w.sum(dim=0))
            cnt.index_add_(0, g, live.sum(dim=0))
            best, arg = w.max(dim=1)
            shape = (y1 - y0, x1 - x0)
            top_w[y0:y1, x0:x1] = best.reshape(shape)
            top_ids[y0:y1, x0:x1] = torch.where(best > 0, g[arg], torch.full_like(arg, -1)).reshape(shape)
            alpha_img[y0:y1, x0:x1] = (1.0 - Tincl[:, -1]).reshape(shape)
            if tid is not None:
                want = tid[y0:y1, x0:x1].reshape(-1)
                hit = (g[None, :] == want[:, None]) & (want[:, None] >= 0)
                at_top[y0:y1, x0:x1] = (w * hit).sum(dim=1).reshape(shape)
    return dict(weight_max=wmax.numpy(), weight_sum=wsum.numpy(), pixel_count=cnt.numpy(), top_w=top_w.numpy(),
                top_ids=top_ids.numpy(), at_top=at_top.numpy(), alpha=alpha_img.numpy())


def top_ties(ref, top_id):
    """bool [H, W]: `top_id` is an argmax of the restatement at the pixel (its weight within TIE of the largest), or -1 where nothing
    blended -- needs ref computed with this top_id"""
    top_id = np.asarray(top_id).reshape(ref["top_w"].shape)
    none = ref["top_w"] == 0
    return np.where(none, top_id == -1, (top_id >= 0) & (ref["at_top"] >= ref["top_w"] - TIE))
