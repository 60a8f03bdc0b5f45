"""Restatement in torch of the kNN-graph regularisers (include/csplat.h: csplat_knn_regs_fwd / csplat_knn_regs_bwd), runnable in
float64 and in float32; gradients come from autograd, with the two conventions of the definition: d|off|/d off = 0 where |off| == 0
(Length below) and sign(0) = 0 (torch.abs).  Shares no code with the library."""
import numpy as np
import torch

U = 2.0 ** -24      # unit roundoff of float32


class Length(torch.autograd.Function):
    """|off| over the last axis; the derivative is off / |off|, and 0 where |off| == 0"""

    @staticmethod
    def forward(ctx, off):
        d = torch.sqrt((off[..., 0] * off[..., 0] + off[..., 1] * off[..., 1]) + off[..., 2] * off[..., 2])
        ctx.save_for_backward(off, d)
        return d

    @staticmethod
    def backward(ctx, g):
        off, d = ctx.saved_tensors
        safe = torch.where(d > 0, d, torch.ones_like(d))
        return torch.where((d > 0)[..., None], g[..., None] * off / safe[..., None], torch.zeros_like(off))


def hamilton(p, q):
    pw, px, py, pz = p.unbind(-1)
    qw, qx, qy, qz = q.unbind(-1)
    return torch.stack([((pw * qw - px * qx) - py * qy) - pz * qz,
                        ((pw * qx + px * qw) + py * qz) - pz * qy,
                        ((pw * qy - px * qz) + py * qw) + pz * qx,
                        ((pw * qz + px * qy) - py * qx) + pz * qw], -1)


def conj(q):
    return torch.cat([q[..., :1], -q[..., 1:]], -1)


def rotmat_rows(q):
    """the nine entries (row-major list) of the rotation matrix of q / |q|, q = (w, x, y, z)"""
    n = torch.sqrt(((q[..., 0] * q[..., 0] + q[..., 1] * q[..., 1]) + q[..., 2] * q[..., 2]) + q[..., 3] * q[..., 3])
    w, x, y, z = (q / n[..., None]).unbind(-1)
    return [1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
            2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
            2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]


def terms(M, Q, idx, d0, w, isometric_abs=False):
    """M [T,N,3], Q [T,N,4] or None, idx int64 [N,K], d0 / w [N,K] (the dtype of M) -> (L_iso, L_spring, L_rigid) scalars"""
    T = M.shape[0]
    off = M[:, idx] - M[:, :, None, :]                       # [T,N,K,3]: off_t = M[t][j] - M[t][i]
    d = Length.apply(off)                                    # [T,N,K]
    x = d - d0[None]
    iso = (x.abs() if isometric_abs else x).mean()
    zero = M.new_zeros(())
    if T < 2:
        return iso, zero, zero
    spring = (d[1:] - d[:-1]).abs().mean()
    if Q is None:
        return iso, spring, zero
    R = rotmat_rows(hamilton(Q[:-1][:, idx], conj(Q[1:][:, idx])))          # r = Q[t-1][j] (x) conj(Q[t][j]),  [T-1,N,K]
    o, p = off[1:], off[:-1]
    e = [((R[3 * a] * o[..., 0] + R[3 * a + 1] * o[..., 1]) + R[3 * a + 2] * o[..., 2]) - p[..., a] for a in range(3)]
    s = (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]
    rigid = torch.sqrt(s * w[None] + 1e-20).mean()
    return iso, spring, rigid


def evaluate(M, Q, idx, d0, w, lams, isometric_abs=False, up=1.0, dtype=torch.float64):
    """one evaluation in `dtype` on the CPU: dict(parts [3], loss, dM [T,N,3], dQ [T,N,4] or None) as float64 numpy; `up` the upstream
    gradient of the loss"""
    Mt = torch.as_tensor(np.asarray(M)).to(dtype).requires_grad_()
    Qt = None if Q is None else torch.as_tensor(np.asarray(Q)).to(dtype).requires_grad_()
    it = torch.as_tensor(np.asarray(idx)).long()
    dt, wt = torch.as_tensor(np.asarray(d0)).to(dtype), torch.as_tensor(np.asarray(w)).to(dtype)
    parts = terms(Mt, Qt, it, dt, wt, isometric_abs)
    loss = (lams[0] * parts[0] + lams[1] * parts[1]) + lams[2] * parts[2]
    (loss * up).backward()
    dQ = None
    if Qt is not None:
        dQ = (Qt.grad if Qt.grad is not None else torch.zeros_like(Qt)).double().numpy()
    return dict(parts=np.array([float(p.detach()) for p in parts]), loss=float(loss.detach()), dM=Mt.grad.double().numpy(), dQ=dQ)


def reverse_lists(idx, N):
    """(offsets int64 [N+1], entries int64 [N*K]) of an in-range idx [N,K]: entries[offsets[j] : offsets[j+1]] are the pair numbers
    i*K + k with idx[i,k] == j, ascending -- a stable argsort"""
    flat = np.asarray(idx).reshape(-1)
    entries = np.argsort(flat, kind="stable")
    offsets = np.concatenate([[0], np.cumsum(np.bincount(flat, minlength=N))])
    return offsets.astype(np.int64), entries.astype(np.int64)


def scale_err(got, want):
    """max |got - want| / max |want| (the error scaled by the tensor's largest component); 0 for two all-zero tensors"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    top = float(np.abs(want).max()) if want.size else 0.0
    err = float(np.abs(got - want).max()) if want.size else 0.0
    return err / top if top > 0 else (0.0 if err == 0 else float("inf"))
