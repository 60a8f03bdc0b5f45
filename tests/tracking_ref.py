"""Restatement of the tracking kernels (csplat_track_visibility, csplat_track_mte; include/csplat.h states the semantics) in torch on the
CPU, in float64 or float32, written from those semantics.  Besides the results it returns each decision's MARGIN, the distance of the
float64 quantity from the point where the decision changes:
  margin_border   distance of x, y to the four image borders x = 0, x = W, y = 0, y = H, in pixels (inf for a point that does not
                  project to numbers, or -- when projecting -- has w <= 0: no rounding moves those)
  margin_cell     for a point in the image, distance of x and y to the nearest integer (where the depth tap changes), in pixels; else inf
  margin_depth    |(|X - c| - thr) - d| for a point in the image with a depth that is a number; else inf
  margin_min      |d_raw - min_depth| for a point in the image while the min_depth rule is on; else inf
  scale_depth     max(|X - c|, |d|): what the two depth margins are measured against
ties() applies the bar of tests/test_tracking_gpu.py to them."""
import torch

F64, F32 = torch.float64, torch.float32
INF = float("inf")
TIE_ULPS = 64.0 * 2.0 ** -24


def project(X, full, W, H):
    """[F,N,3] points, [F,4,4] full_proj (hom = [X, 1] @ full) -> x, y, w, each [F,N]"""
    col = lambda c: X[..., 0] * full[:, None, 0, c] + X[..., 1] * full[:, None, 1, c] + X[..., 2] * full[:, None, 2, c] + full[:, None, 3, c]  # noqa: E731
    hx, hy, w = col(0), col(1), col(3)
    return ((hx / w + 1.0) * W - 1.0) * 0.5, ((hy / w + 1.0) * H - 1.0) * 0.5, w


def visibility(points, full, cam, depth, W, H, pixels=None, thr=0.2, min_depth=1.0, far=1e4, dtype=F64):
    """-> dict(pixels [F,N,2], in_image, visible [F,N] bool, counts [F,2] int64, the margins [F,N] in `dtype`)"""
    X = points.to(dtype)
    Fr, N = X.shape[0], X.shape[1]
    if pixels is None:
        x, y, w = project(X, full.to(dtype), W, H)
        front = w > 0
    else:
        x, y = pixels[..., 0].to(dtype), pixels[..., 1].to(dtype)
        front = torch.ones(Fr, N, dtype=torch.bool)
    number = torch.isfinite(x) & torch.isfinite(y)
    inside = front & number & (x >= 0) & (x < W) & (y >= 0) & (y < H)
    inf = torch.full((Fr, N), INF, dtype=dtype)
    border = torch.minimum(torch.minimum(x.abs(), (x - W).abs()), torch.minimum(y.abs(), (y - H).abs()))
    out = dict(pixels=torch.stack([x, y], -1), in_image=inside, margin_border=torch.where(front & number, border, inf))
    near = lambda v: torch.minimum(v - torch.floor(v), torch.ceil(v) - v)  # noqa: E731
    # (a coordinate that IS an integer sits exactly on the edge of its cell: margin 0)
    out["margin_cell"] = torch.where(inside, torch.minimum(near(x), near(y)), inf) if depth is not None else inf
    out["margin_depth"], out["margin_min"], out["scale_depth"] = inf, inf, torch.ones(Fr, N, dtype=dtype)
    vis = inside
    if depth is not None:
        zero = torch.zeros((), dtype=dtype)
        xi = torch.trunc(torch.where(inside, x, zero)).long().clamp(0, W - 1)
        yi = torch.trunc(torch.where(inside, y, zero)).long().clamp(0, H - 1)
        raw = depth.to(dtype).reshape(Fr, H * W).gather(1, yi * W + xi)
        d = raw
        if min_depth > 0:
            d = torch.where(raw < min_depth, torch.full_like(raw, far), raw)
            out["margin_min"] = torch.where(inside & ~torch.isnan(raw), (raw - min_depth).abs(), inf)
        diff = X - cam.to(dtype)[:, None, :]
        dist = torch.sqrt(diff[..., 0] * diff[..., 0] + diff[..., 1] * diff[..., 1] + diff[..., 2] * diff[..., 2])
        vis = inside & ((dist - thr) <= d)
        ok = inside & ~torch.isnan(d) & ~torch.isnan(dist)
        out["margin_depth"] = torch.where(ok, ((dist - thr) - d).abs(), inf)
        out["scale_depth"] = torch.where(ok, torch.maximum(dist, d.abs()), torch.ones_like(dist))
    out["visible"] = vis
    out["counts"] = torch.stack([inside.sum(1), vis.sum(1)], 1)
    return out


def ties(r, W, H):
    """[F,N] bool: the points of a float64 result `r` a float32 evaluation may decide the other way -- a pixel margin below
    tau = 64 * 2^-24 * max(W, H), or one of the two depth margins below 64 * 2^-24 * max(|X - c|, d)"""
    tau = TIE_ULPS * max(W, H)
    return (r["margin_border"] < tau) | (r["margin_cell"] < tau) | (r["margin_depth"] < TIE_ULPS * r["scale_depth"]) | \
        (r["margin_min"] < TIE_ULPS * r["scale_depth"])


def rotation(q):
    """[...,4] quaternions, r first, normalised here -> [...,3,3]; a zero quaternion gives NaN"""
    n = torch.sqrt((q * q).sum(-1, keepdim=True))
    r, x, y, z = (q / n).unbind(-1)
    m = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y),
                     2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x),
                     2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], -1)
    return m.reshape(q.shape[:-1] + (3, 3))


def mte(gt, traj, rotations, assoc, dtype=F64):
    """gt [T,G,3], traj [T,N,3], rotations [T,N,4] or None, assoc [G] -> dict(aligned [T,G,3], err [T,G], mte [G], mean [])"""
    gt, sel = gt.to(dtype), traj.to(dtype)[:, assoc.long()]
    T, G = gt.shape[0], gt.shape[1]
    aligned = sel.clone()
    if rotations is not None:
        R = rotation(rotations.to(dtype)[:, assoc.long()])          # [T,G,3,3]
        t0 = gt[0] - sel[0]
        aligned[0] = sel[0] + t0
        for k in range(1, T):
            rel = R[k] @ R[0].transpose(1, 2)
            aligned[k] = sel[k] + (rel @ t0[:, :, None])[:, :, 0]
    e = gt - aligned
    err = torch.sqrt(e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1] + e[..., 2] * e[..., 2])
    per = torch.zeros(G, dtype=dtype)
    for k in range(T):
        per = per + err[k]
    per = per / T
    return dict(aligned=aligned, err=err, mte=per, mean=per.sum() / G)
