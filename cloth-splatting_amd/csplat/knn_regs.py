"""Neighbourhood regularisers on the Gaussians' k-nearest-neighbour graph: isometry, spring and local rigidity of the deformed centres
and rotations over the time rows of a step (the reference's --lambda_isometric / --lambda_spring / --lambda_rigidity with --k_nearest and
--lambda_w), fused: one forward launch, one gather-only backward launch (include/csplat.h: csplat_knn_regs_graph / _fwd / _bwd).  The
terms are stated in include/csplat.h; they are written from that definition -- the reference's own block is commented out and cannot
be run, so there is no reference-run fixture and parity is against tests/knn_regs_ref.py."""
import math

import torch
from torch.autograd.function import once_differentiable

import simple_knn

from . import native as _n


def _reverse_lists_cpu(idx, N):
    flat = idx.reshape(-1)
    entries = torch.sort(flat, stable=True).indices.to(torch.int32)
    offsets = torch.zeros(N + 1, dtype=torch.int64)
    offsets[1:] = torch.cumsum(torch.bincount(flat, minlength=N), 0)
    return offsets.to(torch.int32), entries


class NeighbourGraph:
    """A K-neighbour graph of N nodes with its rest state.  Fields: idx int64 [N,K] (neighbour j of pair (i,k)), d0 float32 [N,K] (rest
    distance), w float32 [N,K] (weight), rev_offsets int32 [N+1] / rev_entries int32 [N*K] (for every node the pair numbers i*K + k
    that name it, ascending), N, K.  Built once per graph refresh, not per step."""

    def __init__(self, idx, d0, w, rev_offsets, rev_entries):
        self.idx, self.d0, self.w, self.rev_offsets, self.rev_entries = idx, d0, w, rev_offsets, rev_entries
        self.N, self.K = int(idx.shape[0]), int(idx.shape[1])
        self.idx32 = idx.to(torch.int32).contiguous()
        self.device = idx.device

    @staticmethod
    def _build(idx32, d2, lambda_w):
        """(d0, w, rev_offsets, rev_entries) on the GPU; d2 None: only the reverse lists"""
        N, K, dev = int(idx32.shape[0]), int(idx32.shape[1]), idx32.device
        d0 = w = None
        if d2 is not None:
            d0, w = torch.empty_like(d2), torch.empty_like(d2)
        off = torch.empty(N + 1, dtype=torch.int32, device=dev)
        ent = torch.empty(N * K, dtype=torch.int32, device=dev)
        temp = _n.temp(dev, _n.lib.csplat_knn_regs_graph_temp_bytes(N, K))
        _n.launch("csplat_knn_regs_graph", dev, N, K, _n.ptr(idx32), _n.ptr(d2), float(lambda_w), _n.ptr(d0), _n.ptr(w), _n.ptr(off), _n.ptr(ent),
                  _n.ptr(temp))
        return d0, w, off, ent

    @classmethod
    def from_points(cls, points, k, lambda_w):
        """the exact k-NN graph of a float32 [N,3] GPU cloud (simple_knn.knn: ties to the smaller index), N > k:
        d0 = sqrt(d2), w = exp(-lambda_w * d2)"""
        simple_knn._checked_points(points, k, "NeighbourGraph.from_points")
        lambda_w = float(lambda_w)
        if not (lambda_w >= 0.0 and math.isfinite(lambda_w)):
            raise ValueError(f"NeighbourGraph.from_points: lambda_w is a finite number >= 0, got {lambda_w}")
        if int(points.shape[0]) <= k:
            raise ValueError(f"NeighbourGraph.from_points: {int(points.shape[0])} points have no {k} neighbours each (N > k is needed)")
        d2, idx = simple_knn.knn(points, k)
        idx32 = idx.to(torch.int32)
        d0, w, off, ent = cls._build(idx32, d2.contiguous(), lambda_w)
        return cls(idx, d0, w, off, ent)

    @classmethod
    def from_indices(cls, idx, d0, w):
        """any in-range graph (mesh-edge neighbourhoods, tests): idx integer [N,K], d0 / w float32 [N,K] on idx's device"""
        if not torch.is_tensor(idx) or idx.dim() != 2 or idx.dtype not in (torch.int32, torch.int64) or idx.shape[0] < 1 or \
                not 1 <= idx.shape[1] <= simple_knn.MAX_K:
            raise ValueError(f"NeighbourGraph.from_indices: idx must be an int32 / int64 [N, K] tensor, N >= 1, 1 <= K <= {simple_knn.MAX_K}")
        for name, t in (("d0", d0), ("w", w)):
            if not torch.is_tensor(t) or t.dtype != torch.float32 or t.shape != idx.shape or t.device != idx.device:
                raise ValueError(f"NeighbourGraph.from_indices: {name} must be a float32 tensor of idx's shape on idx's device")
        N = int(idx.shape[0])
        if N * int(idx.shape[1]) >= 2 ** 31:
            raise ValueError("NeighbourGraph.from_indices: N * K must stay below 2^31")
        lo, hi = int(idx.min()), int(idx.max())
        if lo < 0 or hi >= N:
            raise ValueError(f"NeighbourGraph.from_indices: indices must lie in 0 .. {N - 1}, found {lo} .. {hi}")
        idx = idx.detach().to(torch.int64).contiguous()
        d0, w = d0.detach().contiguous(), w.detach().contiguous()
        if idx.is_cuda:
            _, _, off, ent = cls._build(idx.to(torch.int32), None, 0.0)
        else:
            off, ent = _reverse_lists_cpu(idx, N)
        return cls(idx, d0, w, off, ent)


class _FusedRegs(torch.autograd.Function):
    """(loss, parts [3]) of csplat_knn_regs_fwd on float32 GPU tensors; backward: one csplat_knn_regs_bwd for whichever of means /
    rotations requires a gradient."""

    @staticmethod
    def forward(ctx, means, rotations, graph, lam_i, lam_s, lam_r, iso_abs):
        M = means.detach().contiguous()
        Q = None if rotations is None else rotations.detach().contiguous()
        dev = M.device
        T, N, K = int(M.shape[0]), graph.N, graph.K
        out = torch.empty(4, dtype=torch.float32, device=dev)
        scratch = _n.temp(dev, _n.lib.csplat_knn_regs_fwd_scratch_bytes())
        _n.launch("csplat_knn_regs_fwd", dev, T, N, K, _n.ptr(M), _n.ptr(Q), _n.ptr(graph.idx32), _n.ptr(graph.d0), _n.ptr(graph.w), lam_i, lam_s,
                  lam_r, int(iso_abs), _n.ptr(out), _n.ptr(scratch))
        ctx.save_for_backward(M, Q)
        ctx.graph, ctx.lams, ctx.iso_abs = graph, (lam_i, lam_s, lam_r), int(iso_abs)
        ctx.set_materialize_grads(False)
        loss, parts = out[3], out[:3]
        ctx.mark_non_differentiable(parts)
        return loss, parts

    @staticmethod
    @once_differentiable
    def backward(ctx, g, _g_parts):
        want_m, want_q = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if g is None or not (want_m or want_q):
            return (None,) * 7
        M, Q = ctx.saved_tensors
        graph, dev = ctx.graph, M.device
        T = int(M.shape[0])
        g = g.reshape(1).float().contiguous()
        dM = torch.empty_like(M) if want_m else None
        dQ = torch.empty_like(Q) if (want_q and Q is not None) else None
        _n.launch("csplat_knn_regs_bwd", dev, T, graph.N, graph.K, _n.ptr(M), _n.ptr(Q), _n.ptr(graph.idx32), _n.ptr(graph.d0), _n.ptr(graph.w),
                  _n.ptr(graph.rev_offsets), _n.ptr(graph.rev_entries), ctx.lams[0], ctx.lams[1], ctx.lams[2], ctx.iso_abs, _n.ptr(g), _n.ptr(dM),
                  _n.ptr(dQ))
        return dM, dQ, None, None, None, None, None


class _Length(torch.autograd.Function):
    """|off|; its derivative is off / |off|, and 0 where |off| == 0"""

    @staticmethod
    def forward(ctx, off):
        x, y, z = off.unbind(-1)
        d = torch.sqrt((x * x + y * y) + z * z)
        ctx.save_for_backward(off, d)
        return d

    @staticmethod
    def backward(ctx, g):
        off, d = ctx.saved_tensors
        unit = torch.where((d > 0).unsqueeze(-1), off / torch.where(d > 0, d, torch.ones_like(d)).unsqueeze(-1), torch.zeros_like(off))
        return g.unsqueeze(-1) * unit


def _qmul(p, q):
    p0, p1, p2, p3 = p.unbind(-1)
    q0, q1, q2, q3 = q.unbind(-1)
    return torch.stack((((p0 * q0 - p1 * q1) - p2 * q2) - p3 * q3, ((p0 * q1 + p1 * q0) + p2 * q3) - p3 * q2,
                        ((p0 * q2 - p1 * q3) + p2 * q0) + p3 * q1, ((p0 * q3 + p1 * q2) - p2 * q1) + p3 * q0), -1)


def _composed(means, rotations, graph, lam_i, lam_s, lam_r, iso_abs):
    """the definition as torch ops (CPU tensors): the same operations in the same order as the kernels, summed by torch"""
    idx, T = graph.idx, means.shape[0]
    off = means[:, idx] - means.unsqueeze(2)
    d = _Length.apply(off)
    x = d - graph.d0
    zero = means.new_zeros(())
    iso = (x.abs() if iso_abs else x).mean()
    spring = rigid = zero
    if T > 1:
        spring = (d[1:] - d[:-1]).abs().mean()
        if rotations is not None:
            qn = rotations[:, idx]
            r = _qmul(qn[:-1], qn[1:] * qn.new_tensor([1.0, -1.0, -1.0, -1.0]))
            n = r / torch.sqrt(((r[..., 0] * r[..., 0] + r[..., 1] * r[..., 1]) + r[..., 2] * r[..., 2]) + r[..., 3] * r[..., 3]).unsqueeze(-1)
            qw, qx, qy, qz = n.unbind(-1)
            rows = ((1 - 2 * (qy * qy + qz * qz), 2 * (qx * qy - qw * qz), 2 * (qx * qz + qw * qy)),
                    (2 * (qx * qy + qw * qz), 1 - 2 * (qx * qx + qz * qz), 2 * (qy * qz - qw * qx)),
                    (2 * (qx * qz - qw * qy), 2 * (qy * qz + qw * qx), 1 - 2 * (qx * qx + qy * qy)))
            o0, o1, o2 = off[1:].unbind(-1)
            e = [((row[0] * o0 + row[1] * o1) + row[2] * o2) - off[:-1][..., a] for a, row in enumerate(rows)]
            rigid = torch.sqrt(((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]) * graph.w + 1e-20).mean()
    loss = (lam_i * iso + lam_s * spring) + lam_r * rigid
    return loss, torch.stack((iso, spring, rigid)).detach()


def neighbour_regularization(means, rotations, graph, lambda_isometric, lambda_spring, lambda_rigidity, *, isometric_abs=False):
    """means float32 [T,N,3] (the Gaussian centres at the step's T time rows, in the order given), rotations float32 [T,N,4] ((w,x,y,z),
    not assumed normalised) or None, graph a NeighbourGraph of the same N on the same device -> (loss, parts):
        loss = lambda_isometric L_iso + lambda_spring L_spring + lambda_rigidity L_rigid      (include/csplat.h states the terms)
        parts = the detached float32 [3] (L_iso, L_spring, L_rigid), unweighted; L_rigid is 0 without rotations.
    L_iso is SIGNED, mean (d_t - d0), as the reference wrote it; isometric_abs=True takes |d_t - d0|.  T = 1: L_spring = L_rigid = 0.
    Gradients go to means and rotations (one autograd node; only rows that are someone's neighbour get a non-zero rotation gradient).
    ValueError before anything touches the device: wrong shape, dtype or device, N != graph.N, T < 1, a negative or NaN weight,
    rotations None with lambda_rigidity > 0.  GPU tensors always take the HIP kernels; CPU tensors take a torch composition of the
    same definition."""
    if not isinstance(graph, NeighbourGraph):
        raise ValueError(f"neighbour_regularization: graph must be a NeighbourGraph, got {type(graph).__name__}")
    if not torch.is_tensor(means) or means.dim() != 3 or means.shape[2] != 3 or means.dtype != torch.float32:
        raise ValueError(f"neighbour_regularization: means must be a float32 [T, N, 3] tensor, got {getattr(means, 'dtype', None)} "
                         f"{tuple(getattr(means, 'shape', ()))}")
    T, N = int(means.shape[0]), int(means.shape[1])
    if T < 1:
        raise ValueError("neighbour_regularization: at least one time row is needed (T >= 1)")
    if N != graph.N:
        raise ValueError(f"neighbour_regularization: means has {N} nodes, the graph {graph.N}")
    if T >= 65536 or T * N >= 2 ** 31:
        raise ValueError("neighbour_regularization: T < 65536 and T * N < 2^31 are needed")
    if means.device != graph.device:
        raise ValueError(f"neighbour_regularization: means is on {means.device}, the graph on {graph.device}")
    lams = []
    for name, v in (("lambda_isometric", lambda_isometric), ("lambda_spring", lambda_spring), ("lambda_rigidity", lambda_rigidity)):
        v = float(v)
        if not (v >= 0.0 and v <= 3.0e38):
            raise ValueError(f"neighbour_regularization: {name} is a finite number >= 0, got {v}")
        lams.append(v)
    if rotations is None:
        if lams[2] > 0.0:
            raise ValueError("neighbour_regularization: lambda_rigidity > 0 needs the rotations")
    elif not torch.is_tensor(rotations) or rotations.dtype != torch.float32 or tuple(rotations.shape) != (T, N, 4) or \
            rotations.device != means.device:
        raise ValueError(f"neighbour_regularization: rotations must be a float32 [{T}, {N}, 4] tensor on {means.device}, got "
                         f"{getattr(rotations, 'dtype', None)} {tuple(getattr(rotations, 'shape', ()))}")
    if means.is_cuda:
        return _FusedRegs.apply(means, rotations, graph, lams[0], lams[1], lams[2], bool(isometric_abs))
    return _composed(means, rotations, graph, lams[0], lams[1], lams[2], bool(isometric_abs))
