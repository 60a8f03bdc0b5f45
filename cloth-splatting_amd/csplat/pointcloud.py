"""Point-cloud losses on the exact two-cloud neighbour search (simple_knn.knn_query): the Chamfer distance between two clouds, and
its one-sided form, the 3-D companion of the depth / silhouette terms -- a loss that pulls the deformed Gaussian centres onto an
observed point cloud."""
import torch
from torch.autograd.function import once_differentiable

import simple_knn

from . import native as _n

CPU_CHUNK = 1024      # queries per [chunk, N] distance matrix of the CPU composition


class ChamferDirection(torch.autograd.Function):
    """L(a -> b) = (1/|a|) sum_i w_i min_j |b_j - a_i|^2 on float32 GPU clouds (include/csplat.h: csplat_chamfer_fwd / _bwd).
    forward: csplat_knn_query (K = 1) + csplat_chamfer_fwd; backward: one csplat_chamfer_bwd, the gradient flowing through the
    stored nearest index to both clouds.  cap < 0: no cap."""

    @staticmethod
    def forward(ctx, a, b, cap):
        _n.require_cuda(a, b)
        qa, pb = a.detach().contiguous(), b.detach().contiguous()
        dev = qa.device
        d2, idx = simple_knn._knn_query_i32(qa, pb, 1)
        d2, idx = d2.view(-1), idx.view(-1)
        loss = torch.empty(1, dtype=torch.float32, device=dev)
        _n.launch("csplat_chamfer_fwd", dev, int(qa.shape[0]), _n.ptr(d2), float(cap), _n.ptr(loss))
        ctx.save_for_backward(qa, pb, d2, idx)
        ctx.cap = float(cap)
        ctx.set_materialize_grads(False)
        return loss.view(())

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        if g is None or not (ctx.needs_input_grad[0] or ctx.needs_input_grad[1]):
            return None, None, None
        qa, pb, d2, idx = ctx.saved_tensors
        Q, N, dev = int(qa.shape[0]), int(pb.shape[0]), qa.device
        g = g.reshape(1).float().contiguous()
        ga = torch.empty(Q, 3, dtype=torch.float32, device=dev) if ctx.needs_input_grad[0] else None
        gb = torch.empty(N, 3, dtype=torch.float32, device=dev) if ctx.needs_input_grad[1] else None
        temp = _n.temp(dev, _n.lib.csplat_chamfer_bwd_temp_bytes(Q, N)) if gb is not None else None
        _n.launch("csplat_chamfer_bwd", dev, Q, N, _n.ptr(qa), _n.ptr(pb), _n.ptr(d2), _n.ptr(idx), ctx.cap, _n.ptr(g), _n.ptr(ga), _n.ptr(gb),
                  _n.ptr(temp))
        return ga, gb, None


def _nearest_cpu(a, b):
    """int64 [|a|]: the index of the nearest b to every a on float32 squared distances, ties to the smaller index (no gradient)"""
    out = []
    N = b.shape[0]
    ar = torch.arange(N, device=b.device)
    with torch.no_grad():
        for s in range(0, a.shape[0], CPU_CHUNK):
            d = b[None, :, :] - a[s:s + CPU_CHUNK, None, :]
            d2 = d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]
            best = d2.min(dim=1, keepdim=True).values
            out.append(torch.where(d2 == best, ar[None, :], N).min(dim=1).values.clamp_(max=N - 1))
    return torch.cat(out)


def _direction_composed(a, b, cap):
    idx = _nearest_cpu(a.detach(), b.detach())
    d = b[idx] - a
    d2 = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]
    if cap >= 0.0:
        d2 = torch.where(d2.detach() <= cap, d2, torch.zeros_like(d2))
    return d2.sum() / a.shape[0]


def _checked_cloud(t, name):
    if not torch.is_tensor(t) or t.dim() != 2 or t.shape[1] != 3:
        raise ValueError(f"chamfer_distance: `{name}` must be a [n, 3] tensor, got {tuple(getattr(t, 'shape', ()))}")
    if t.shape[0] == 0:
        raise ValueError(f"chamfer_distance: `{name}` is empty")
    if t.dtype != torch.float32:
        raise ValueError(f"chamfer_distance: `{name}` must be float32, got {t.dtype}")


def chamfer_distance(x, y, *, two_sided=True, max_sq_dist=None):
    """x [n,3], y [m,3], float32 on one device -> float32 scalar
        L = L(x -> y) [+ L(y -> x) when two_sided],     L(a -> b) = (1/|a|) sum_i w_i min_j |b_j - a_i|^2
    with w_i = 1 when max_sq_dist is None or the squared distance is <= max_sq_dist, else 0 (the divisor stays |a|).  The nearest
    point is the one simple_knn.knn_query returns (float32 squared distances, ties to the smaller index); the gradient flows through
    that index to both clouds, to whichever of them requires it.
    ValueError before anything touches the device: a cloud that is not a non-empty float32 [n,3] tensor, clouds on different devices,
    a max_sq_dist that is negative or NaN.  GPU tensors always take the HIP kernels (ChamferDirection); CPU tensors take a chunked
    torch composition of the same definition."""
    _checked_cloud(x, "x")
    _checked_cloud(y, "y")
    if x.device != y.device:
        raise ValueError(f"chamfer_distance: x is on {x.device}, y on {y.device}")
    cap = -1.0
    if max_sq_dist is not None:
        cap = float(max_sq_dist)
        if not cap >= 0.0:
            raise ValueError(f"chamfer_distance: max_sq_dist is None or >= 0, got {max_sq_dist!r}")
    one = ChamferDirection.apply if x.is_cuda else _direction_composed
    loss = one(x, y, cap)
    if two_sided:
        loss = loss + one(y, x, cap)
    return loss
