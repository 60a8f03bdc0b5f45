"""float64 restatement of one direction of the Chamfer distance (include/csplat.h: csplat_chamfer_fwd / csplat_chamfer_bwd) for GIVEN
nearest indices, with the per-component rounding bound of a float32 evaluation.  numpy only; shares no code with the kernels."""
import numpy as np

U = 2.0 ** -24      # unit roundoff of float32


def direction(a, b, idx, d2_f32, cap=None, g=1.0):
    """a [Q,3] queries, b [N,3] points, idx [Q] the nearest point of every query, d2_f32 [Q] the float32 squared distances the
    weights are decided on (w_i = 1 when cap is None or d2_f32[i] <= cap), g the upstream gradient.
    -> dict(loss, dq [Q,3], dp [N,3], bound_q, bound_p, count [N]):
        loss = (1/Q) sum w_i |b_idx[i] - a_i|^2,    t_i = g (2/Q) w_i (a_i - b_idx[i]),    dq[i] = t_i,    dp[j] = - sum_{idx[i] = j} t_i
        bound = (n + 8) U sum |t_i| per component, n the number of terms of the sum (1 for dq): at most four roundings per term
        (2/Q, times g, the difference, the product) plus n - 1 in the sum, whatever its order, with slack for another factoring of
        the coefficient"""
    a64, b64 = np.asarray(a, np.float64), np.asarray(b, np.float64)
    idx = np.asarray(idx, np.int64).reshape(-1)
    Q, N = a64.shape[0], b64.shape[0]
    w = np.ones(Q) if cap is None else (np.asarray(d2_f32, np.float32).reshape(-1) <= np.float32(cap)).astype(np.float64)
    diff = a64 - b64[idx]
    loss = float((w * (diff * diff).sum(1)).sum() / Q)
    t = float(g) * (2.0 / Q) * w[:, None] * diff
    dp, absum = np.zeros((N, 3)), np.zeros((N, 3))
    np.add.at(dp, idx, -t)
    np.add.at(absum, idx, np.abs(t))
    count = np.bincount(idx, minlength=N)
    return dict(loss=loss, dq=t, dp=dp, bound_q=9 * U * np.abs(t), bound_p=(count[:, None] + 8) * U * absum, count=count, w=w)
