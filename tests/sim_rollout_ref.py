"""Plain torch restatement, on the CPU, of what the kernels of csrc/csplat_sim.hip (the simulator's output layer and hidden layers, the
cloth regularisers) and the rollout-step kernels of csrc/csplat_gnn.hip (head, decode, integrate, edge features, edge-length refinement)
compute, for tests/test_sim_rollout_kernels_cpu.py (which checks THIS file against what the project already trusts: F.linear, autograd
over the composed MLP, train.regularization(fused=False), rollout.refine_edge_lengths' CPU branch, tests/golden/simulator.npz and
refine.npz) and tests/test_sim_rollout_kernels_gpu.py (which checks the kernels against this file in float64 and derives its bars from
this file in float32).  Written from the formulas the kernels' headers cite; nothing is imported from csplat or meshnet.  Every function
takes the dtype it computes in.

Also here, because both test files need them: the SIZE TABLES and the case builders of the GPU file (a test without a GPU checks that
every size lies beyond the launch constant it is meant to cross, and that the inputs are conditioned so that the restatement itself is
stable: tests/test_sim_rollout_kernels_cpu.py)."""
import torch

F64, F32 = torch.float64, torch.float32


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# ------------------------------------------------------------------------------------------------ the simulator's output layer
def rows_dot(h, W, b, add=None, dtype=F64):
    """y[t][r] = b[r] + sum_k W[r][k] h[t][k] (+ add[t][r]): Linear(256, R) on the T time rows"""
    y = h.to(dtype) @ W.to(dtype).t() + b.to(dtype)
    return y if add is None else add.to(dtype).reshape(y.shape) + y


def rows_dot_grads(h, W, dy, dtype=F64):
    """(dW, db, dh) of rows_dot for the cotangent dy [T, R]"""
    h, W, dy = h.to(dtype), W.to(dtype), dy.to(dtype)
    return dy.t() @ h, dy.sum(0), dy @ W


# ------------------------------------------------------------------------------------------------ the simulator's hidden layers
def sim_hidden(e, W1, b1, W2, b2, dtype=F64):
    """(h1, h2): h1 = relu(e W1^T + b1), h2 = relu(h1 W2^T + b2); torch.relu keeps a NaN"""
    e, W1, b1, W2, b2 = (t.to(dtype) for t in (e, W1, b1, W2, b2))
    h1 = torch.relu(e @ W1.t() + b1)
    return h1, torch.relu(h1 @ W2.t() + b2)


def sim_hidden_grads(e, W1, b1, W2, b2, dh2, dtype=F64):
    """(dW1, db1, dW2, db2) for the cotangent dh2 [T, 256] of h2; the ReLU's derivative at 0 is 0"""
    h1, h2 = sim_hidden(e, W1, b1, W2, b2, dtype)
    dz2 = dh2.to(dtype) * (h2 > 0).to(dtype)
    dz1 = (dz2 @ W2.to(dtype)) * (h1 > 0).to(dtype)
    return dz1.t() @ e.to(dtype), dz1.sum(0), dz2.t() @ h1, dz2.sum(0)


# ------------------------------------------------------------------------------------------------ the cloth regularisers
def _norm3(x):
    return (x[..., 0] * x[..., 0] + x[..., 1] * x[..., 1] + x[..., 2] * x[..., 2]).sqrt()


def _unit(x, n):
    """x / |x| with 0 at |x| = 0 (the gradient of a norm at 0 is 0)"""
    safe = torch.where(n > 0, n, torch.ones_like(n))
    return torch.where((n > 0)[..., None], x / safe[..., None], torch.zeros_like(x))


def cloth_regs(D, ei, rest, lam_d, lam_r, lam_m, dtype=F64):
    """(loss, dLoss/dD) of the three terms as the header of k_cloth_regs states them, D [T][V][3], ei [2][E] int64, rest [E]:
         deform-magnitude  lam_d * 0.5 * (mean_v |D1 - D0|_2 + mean_v |D2 - D1|_2)                    (T >= 3; time rows 0..2 only)
         rigidity          lam_r * mean_{t,e} | rest[e] - |D[t][ei[1][e]] - D[t][ei[0][e]]|_2 |       (every time row)
         momentum          lam_m * mean_v |D2 - 2 D1 + D0|_1                                           (T >= 3; time rows 0..2 only)
    sign(0) = 0 and the gradient of a norm at 0 is 0."""
    D, rest = D.to(dtype), rest.to(dtype)
    T, V = int(D.shape[0]), int(D.shape[1])
    E = int(ei.shape[1])
    g = torch.zeros_like(D)
    loss = torch.zeros((), dtype=dtype)
    if T >= 3 and V > 0:
        if lam_d != 0:
            a, b = D[1] - D[0], D[2] - D[1]
            na, nb = _norm3(a), _norm3(b)
            loss = loss + lam_d * 0.5 * (na.mean() + nb.mean())
            w = 0.5 * lam_d / V
            ua, ub = _unit(a, na), _unit(b, nb)
            g[0] -= w * ua
            g[1] += w * (ua - ub)
            g[2] += w * ub
        if lam_m != 0:
            m = D[2] - 2 * D[1] + D[0]
            loss = loss + lam_m * m.abs().sum(1).mean()
            s = torch.sign(m) * (lam_m / V)
            g[0] += s
            g[1] -= 2 * s
            g[2] += s
    if T > 0 and E > 0 and V > 0 and lam_r != 0:
        disp = D[:, ei[1]] - D[:, ei[0]]                      # [T, E, 3]
        ln = _norm3(disp)
        diff = rest[None] - ln
        loss = loss + lam_r * diff.abs().mean()
        ge = (-torch.sign(diff) * (lam_r / (T * E)))[..., None] * _unit(disp, ln)       # d|rest - len| / d disp
        g.index_add_(1, ei[1], ge)
        g.index_add_(1, ei[0], -ge)
    return loss, g


# ------------------------------------------------------------------------------------------------ the rollout step's head and tail
def rollout_head(hist, node_type, mean, std, T, dtype=F64):
    """(feats [N][3H + T], max |feats|): cat(hist[0] .. hist[H-1], one_hot(node_type, T)), then (x - mean) / std when given.
    hist [H][N][3]; a node type outside 0..T-1 has an all-zero one-hot."""
    H, N = int(hist.shape[0]), int(hist.shape[1])
    onehot = (node_type.reshape(N, 1).long() == torch.arange(T).reshape(1, T)).to(dtype)
    x = torch.cat([hist[h].to(dtype) for h in range(H)] + [onehot], 1)
    if mean is not None:
        x = (x - mean.to(dtype)) / std.to(dtype)
    return x, (x.abs().max() if x.numel() else torch.zeros((), dtype=dtype))


def rollout_decode(h, W, b, omean, ostd, last_v, dtype=F64):
    """(v [N][D], fine): v = last_v + (h W^T + b) [* ostd + omean]; fine = 1 when every v is finite, else 0"""
    acc = h.to(dtype) @ W.to(dtype).t() + b.to(dtype)
    if omean is not None:
        acc = acc * ostd.to(dtype) + omean.to(dtype)
    v = last_v.to(dtype) + acc
    return v, int(bool(torch.isfinite(v).all()))


def rollout_integrate(v, actions, k, grasped, pos, hist, preds, dtype=F64):
    """step k (1-based, as the head's counter leaves it): (v, pos, hist, preds) after pinning v[grasped] = actions[k-1] (nothing is pinned
    for an index outside [0, N)), preds[k-1] = v, pos += v, hist <- (hist[1:], v)"""
    v, pos, hist, preds = (t.to(dtype).clone() for t in (v, pos, hist, preds))
    if 0 <= grasped < v.shape[0]:
        v[grasped] = actions[k - 1].to(dtype)
    preds[k - 1] = v
    return v, pos + v, torch.cat([hist[1:], v[None]], 0), preds


def edge_features(pos, ei, order=None, dtype=F64):
    """(rows [E][4], max |rows|): (pos[ei[0]] - pos[ei[1]], its norm); row r = edge order[r] when an order is given"""
    pos = pos.to(dtype)
    d = pos[ei[0]] - pos[ei[1]]
    rows = torch.cat([d, _norm3(d)[:, None]], 1)
    if order is not None:
        rows = rows[order]
    return rows, (rows.abs().max() if rows.numel() else torch.zeros((), dtype=dtype))


def edge_length_refine(pos, v, ei, rest, edge_w, iters, lr, dtype=F64, beta1=0.9, beta2=0.999, eps=1e-8, return_grads=False):
    """`iters` iterations of a fresh Adam(lr) on v [N][3] against sum_e w_e (|x[ei[0][e]] - x[ei[1][e]]| - rest[e])^2, x = pos + v:
    the gradient written out (the norm's gradient is 0 at length 0), then torch.optim.Adam's recurrence:
        m <- m + (g - m)(1 - beta1);  s <- s beta2 + (1 - beta2) g^2;  v <- v - (lr / (1 - beta1^t)) m / (sqrt(s) / sqrt(1 - beta2^t) + eps)"""
    pos, v, rest = pos.to(dtype), v.to(dtype).clone(), rest.to(dtype)
    w = torch.ones_like(rest) if edge_w is None else edge_w.to(dtype)
    m, s = torch.zeros_like(v), torch.zeros_like(v)
    grads = []
    for t in range(1, iters + 1):
        x = pos + v
        d = x[ei[0]] - x[ei[1]]
        ln = _norm3(d)
        ge = (2 * w * (ln - rest))[:, None] * _unit(d, ln)
        g = torch.zeros_like(v)
        g.index_add_(0, ei[0], ge)
        g.index_add_(0, ei[1], -ge)
        grads.append(g)
        m = m + (g - m) * (1 - beta1)
        s = s * beta2 + (1 - beta2) * g * g
        denom = s.sqrt() / (1 - beta2 ** t) ** 0.5 + eps
        v = v - (lr / (1 - beta1 ** t)) * (m / denom)
    return (v, grads) if return_grads else v


# ================================================================================================ size tables and case builders
# (the constants are asserted against the sources' literals in tests/test_sim_rollout_kernels_cpu.py)
ROWS_DOT_T = (1, 2, 3, 4, 5, 6, 7, 8)
ROWS_DOT_FWD_R = (1, 3, 5, 8191, 8193, 32768, 32769, 32771)
ROWS_DOT_BWD_R = (1, 5, 8193, 32769)
SIM_HIDDEN_T = (1, 2, 3, 4, 5, 6, 7, 8)
SIM_HIDDEN_K0 = (1, 12, 13, 16)
REGS_CASES = ((3, 1, 0), (3, 255, 1), (3, 256, 255), (3, 257, 300), (1, 300, 2000), (2, 300, 2000), (4, 300, 2000), (8, 300, 2000),
              (3, 22001, 22003), (3, 300, 70001))
REGS_LAMBDAS = ((0.01, 0.3, 0.1), (0.01, 0.0, 0.0), (0.0, 0.3, 0.0), (0.0, 0.0, 0.1), (0.0, 0.0, 0.0))
HEAD_N = (0, 1, 255, 256, 257, 10007)
HEAD_HT = ((1, 0), (1, 1), (2, 2), (5, 9), (16, 16))
DECODE_N = (1, 2, 7, 8, 9, 10007)
DECODE_D = (1, 2, 3, 4)
INTEGRATE_N = (1, 257, 10007)
INTEGRATE_H = (1, 2, 3, 5)
INTEGRATE_D = (1, 3, 4)
EDGE_FEATURES_E = (0, 1, 255, 257, 131073)
GATHER_CASES = ((128, 1), (128, 257), (128, 32801), (4, 7))          # (L, E)
REFINE_CASES = ((1, 0), (1, 300), (1, 3000), (257, 0), (257, 300), (257, 3000))           # (N, E): the cross product; N = 1: self-loops only
REFINE_ITERS = (0, 1, 2, 10)
REFINE_LR = 1e-3


def rows_dot_case(R, seed=0):
    """(h8 [8][256], W [R][256], b [R], add [8][R], dy [8][R]): W's row 0 at 1e4 and its last row, with its bias and table entries, at 1e-4
    (R = 1: row 0 at 1e4)"""
    g = _gen(1000 + R + seed)
    h8 = torch.randn(8, 256, generator=g)
    W = torch.randn(R, 256, generator=g)
    W[0] *= 1e4
    if R > 1:
        W[R - 1] *= 1e-4
    b, add, dy = torch.randn(R, generator=g), torch.randn(8, R, generator=g), torch.randn(8, R, generator=g)
    if R > 1:
        b[R - 1] *= 1e-4
        add[:, R - 1] *= 1e-4
    return h8, W, b, add, dy


SIM_ZERO_UNIT_1, SIM_ZERO_UNIT_2 = 17, 201         # hidden units whose preactivation is exactly 0 (zero weight row, zero bias)


def sim_hidden_case(K0, seed=0):
    """(e8 [8][K0], W1, b1, W2, b2, dh2 [8][256]): biases of the size of the products, so that either ReLU has dead and live units in
    every row; units SIM_ZERO_UNIT_1 (layer 1) and SIM_ZERO_UNIT_2 (layer 2) have a preactivation of exactly 0; every other
    preactivation is at least 1e-4 of its layer's largest (the offending units' biases are nudged)"""
    g = _gen(2000 + K0 + seed)
    e8 = torch.randn(8, K0, generator=g)
    W1 = torch.randn(256, K0, generator=g) / K0 ** 0.5
    b1 = torch.randn(256, generator=g)
    W2 = torch.randn(256, 256, generator=g) / 16.0
    b2 = torch.randn(256, generator=g)
    dh2 = torch.randn(8, 256, generator=g)
    W1[SIM_ZERO_UNIT_1] = 0.0
    b1[SIM_ZERO_UNIT_1] = 0.0
    W2[SIM_ZERO_UNIT_2] = 0.0
    b2[SIM_ZERO_UNIT_2] = 0.0
    for _ in range(50):
        z1 = e8.double() @ W1.double().t() + b1.double()
        bad = ((z1.abs() < 1e-4 * z1.abs().max()) & (z1 != 0)).any(0)
        bad[SIM_ZERO_UNIT_1] = False
        if not bool(bad.any()):
            break
        b1[bad] += 1e-2
    for _ in range(50):
        z2 = torch.relu(z1) @ W2.double().t() + b2.double()
        bad = ((z2.abs() < 1e-4 * z2.abs().max()) & (z2 != 0)).any(0)
        bad[SIM_ZERO_UNIT_2] = False
        if not bool(bad.any()):
            break
        b2[bad] += 1e-2
    return e8, W1, b1, W2, b2, dh2


REGS_GRID = 2.0 ** -8          # the vertices of a regulariser case lie on this grid: every difference of them is exact in float32


def regs_case(T, V, E, seed=0):
    """(D [T][V][3], ei [2][E], rest [E], info): a random graph on grid vertices with, where the sizes allow it,
         isolated vertices (the last 5, V >= 257), a self-loop, 20 copies of one edge, a vertex of in-degree 300 and one of out-degree 300
         (E >= 2000), and the exact zeros: vertices with D0 = D1 = D2 (momentum and both deform norms exactly 0), an edge whose ends
         differ by (3, 4, 0) with rest length 5 (|rest - len| exactly 0 in float32 in any evaluation order), an edge with coincident ends
         and the self-loop (length exactly 0).
    Conditioning: every momentum component is a multiple of the grid (0 or >= 2^-8 exactly); the rest length of an edge with
    0 < |rest - len| < 2e-4 of the largest at any time row is moved until none is left.  info: what was built, for the tests."""
    g = _gen(3000 + 7 * T + 3 * V + E + seed)
    D = torch.round(torch.randn(T, V, 3, generator=g) / REGS_GRID) * REGS_GRID
    ei = torch.randint(0, V, (2, E), generator=g, dtype=torch.int64)
    rest = 0.25 + 3.0 * torch.rand(E, generator=g)
    info = dict(isolated=[], self_loop=None, copies=None, hub_in=None, hub_out=None, still=[], exact_rest=None, coincident=None, moved=0)
    nv = V
    if V >= 257:
        nv = V - 5
        ei %= nv
        info["isolated"] = list(range(nv, V))
    if E >= 2000 and nv >= 12:
        ei[0, 10:30], ei[1, 10:30] = 8, 9
        ei[0, 100:400], ei[1, 100:400] = torch.arange(300) % nv, 10
        ei[0, 400:700], ei[1, 400:700] = 11, torch.arange(300) % nv
        info.update(copies=(10, 30), hub_in=10, hub_out=11)
    if E >= 8 and nv >= 8:
        ei[:, 0] = 2
        ei[0, 1], ei[1, 1] = 3, 4
        D[:, 4] = D[:, 3]
        ei[0, 2], ei[1, 2] = 5, 6
        D[:, 6] = D[:, 5] + torch.tensor([3.0, 4.0, 0.0])
        rest[2] = 5.0
        info.update(self_loop=0, coincident=1, exact_rest=2)
    if T >= 3 and nv >= 16:
        D[1, 12:16] = D[0, 12:16]
        D[2, 12:16] = D[0, 12:16]
        info["still"] = [12, 13, 14, 15]
    if E > 0:
        for _ in range(100):
            diff = (rest.double()[None] - _norm3(D.double()[:, ei[1]] - D.double()[:, ei[0]])).abs()
            bad = ((diff < 2e-4 * diff.max()) & (diff != 0)).any(0)
            if not bool(bad.any()):
                break
            rest[bad] += 1.0 / 64
            info["moved"] += int(bad.sum())
    return D, ei, rest, info


def head_case(N, H, T, seed=0):
    """(hist [H][N][3], node_type [N] int32 in 0..max(T,1)-1 mixed, mean [3H+T], std [3H+T])"""
    g = _gen(4000 + N + 31 * H + T + seed)
    hist = torch.randn(H, N, 3, generator=g)
    nt = torch.randint(0, max(T, 1), (N,), generator=g, dtype=torch.int32)
    F = 3 * H + T
    return hist, nt, 0.3 * torch.randn(F, generator=g), 0.5 + torch.rand(F, generator=g)


def decode_case(N, D, seed=0):
    """(h [N][128], W [D][128], b [D], omean [D], ostd [D], last_v [N][D])"""
    g = _gen(5000 + N + 17 * D + seed)
    return (torch.randn(N, 128, generator=g), torch.randn(D, 128, generator=g) / 128 ** 0.5, torch.randn(D, generator=g),
            0.1 * torch.randn(D, generator=g), 0.5 + torch.rand(D, generator=g), torch.randn(N, D, generator=g))


def integrate_case(N, H, D, steps=3, seed=0):
    """(v [N][D], actions [steps][D], pos [N][D], hist [H][N][D])"""
    g = _gen(6000 + N + 13 * H + D + seed)
    return torch.randn(N, D, generator=g), torch.randn(steps, D, generator=g), torch.randn(N, D, generator=g), torch.randn(H, N, D, generator=g)


def edge_case(E, seed=0):
    """(pos [N][3], ei [2][E], order [E]): N = 1000 nodes; edge 0 a self-loop and edge 1 between coincident nodes where E allows"""
    g = _gen(7000 + E + seed)
    N = 1000
    pos = torch.randn(N, 3, generator=g)
    pos[6] = pos[5]
    ei = torch.randint(0, N, (2, E), generator=g, dtype=torch.int64)
    if E >= 2:
        ei[:, 0] = 3
        ei[0, 1], ei[1, 1] = 5, 6
    return pos, ei, torch.randperm(E, generator=g)


def refine_case(N, E, seed=0):
    """(pos [N][3], v [N][3], ei [2][E], rest [E], edge_w [E]) at a length scale of 30 (so that ten steps of lr = 1e-3 move every gradient
    by far less than the 1e-3 of the largest that the conditioning keeps clear) with velocities of 0.01 (an update of lr is then far
    above the spacing of the float32 numbers it is added to).  Every seventh edge weight is 0.  Where the node count allows it
    (N > 8): the last 5 nodes isolated, edge 0 a self-loop, edge 1 between coincident nodes (pos and v equal, no other edge: one step
    apart the edge's direction would be decided by rounding), node 10 the row end of 300 edges (E >= 3000).  At N = 1 every edge is a
    self-loop on the only node: both CSR lists of that node hold all E edges, every length is 0, there is no gradient at all.
    Conditioning: a node whose first gradient has a component below 2e-3 of the largest gets another position (at most 200 rounds);
    tests/test_sim_rollout_kernels_cpu.py asserts 1e-3 at EVERY iteration."""
    g = _gen(8000 + N + E + seed)
    pos, v = 30.0 * torch.randn(N, 3, generator=g), 0.01 * torch.randn(N, 3, generator=g)
    nv = N - 5 if N > 8 else N
    ei = torch.randint(0, nv, (2, E), generator=g, dtype=torch.int64)
    rest = 30.0 * (0.5 + torch.rand(E, generator=g))
    w = torch.ones(E)
    w[::7] = 0.0
    if E >= 3000 and nv >= 12:
        ei[0, 100:400], ei[1, 100:400] = 10, torch.arange(300) % nv
    if E >= 8 and nv >= 8:
        ei[(ei == 5) | (ei == 6)] = 7      # the coincident pair has no other edge: it stays coincident at every iteration
        ei[:, 0] = 3
        ei[0, 1], ei[1, 1] = 5, 6
        pos[6], v[6] = pos[5], v[5]
        w[0] = w[1] = 1.0
    for _ in range(200):
        if E == 0:
            break
        g0 = edge_length_refine(pos, v, ei, rest, w, 1, REFINE_LR, F64, return_grads=True)[1][0]
        bad = ((g0.abs() < 2e-3 * g0.abs().max()) & (g0 != 0)).any(1)
        if not bool(bad.any()):
            break
        pos[bad] += torch.randn(int(bad.sum()), 3, generator=g)
        if E >= 8 and nv >= 8:
            pos[6] = pos[5]                # (kept coincident)
    return pos, v, ei, rest, w
