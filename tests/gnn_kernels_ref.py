"""Plain torch restatement, on the CPU, of what the 128-wide Linear kernels of csrc/csplat_gemm.hip (k_linear128 with every epilogue
option, k_linear128_rows32, k_linear_narrow, k_node_update, k_dw128) and the message-passing half of csrc/csplat_gnn.hip (the CSR build,
k_segment_sum, k_edge_combine_fwd, k_relu_mask, k_gather_rows, k_ln128_fwd / _bwd, k_colsum128, k_relu_mask_bias128) compute, for
tests/test_gnn_kernels_cpu.py (which checks THIS file against what the project already trusts: F.linear, F.layer_norm, autograd,
index_add_ and numpy's stable argsort) and tests/test_gnn_kernels_gpu.py (which checks the kernels against this file in float64 and
derives its bars from this file in float32).  Written from the formulas the kernels' headers and include/csplat.h state; nothing is
imported from csplat or meshnet.  Every function takes the dtype it computes in.

Also here, because both test files need them: the SIZE LISTS and the input builders of the GPU file."""
import numpy as np
import torch

F64, F32 = torch.float64, torch.float32
EPS = 1e-5                    # nn.LayerNorm's default, what every LayerNorm of the network uses


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _c(t, dtype):
    return None if t is None else t.to(dtype)


# ------------------------------------------------------------------------------------------------ LayerNorm over 128-wide rows
def layer_norm(v, gamma, beta, eps=EPS, dtype=F64):
    """(y, stats [M][2] = (mean, rstd)): two passes -- the mean, then the biased variance of the centred row"""
    v, gamma, beta = v.to(dtype), gamma.to(dtype), beta.to(dtype)
    mean = v.mean(1, keepdim=True)
    d = v - mean
    rstd = 1.0 / ((d * d).mean(1, keepdim=True) + eps).sqrt()
    return d * rstd * gamma + beta, torch.cat([mean, rstd], 1)


def layer_norm_one_pass(v, gamma, beta, eps=EPS, dtype=F64):
    """the form no kernel may take: var = E[x^2] - mean^2 (tests/test_gnn_kernels_cpu.py shows that the LayerNorm rows tell it apart)"""
    v, gamma, beta = v.to(dtype), gamma.to(dtype), beta.to(dtype)
    mean = v.mean(1, keepdim=True)
    var = ((v * v).mean(1, keepdim=True) - mean * mean).clamp_min(0)
    return (v - mean) / (var + eps).sqrt() * gamma + beta


def layer_norm_bwd(g, x, stats, gamma, g_rows=None, x_normalized=False, dtype=F64):
    """(dx, dgamma, dbeta, column sums of dx): row r's incoming gradient is g[g_rows[r]] when g_rows is given; x_normalized: x is xhat
    itself and stats only supplies rstd.   dx = rstd (w - mean_c(w) - xhat mean_c(w xhat)),  w = g gamma"""
    g, x, stats, gamma = g.to(dtype), x.to(dtype), stats.to(dtype), gamma.to(dtype)
    if g_rows is not None:
        g = g[g_rows]
    rstd = stats[:, 1:2]
    xhat = x if x_normalized else (x - stats[:, 0:1]) * rstd
    w = g * gamma
    dx = rstd * (w - w.mean(1, keepdim=True) - xhat * (w * xhat).mean(1, keepdim=True))
    return dx, (g * xhat).sum(0), g.sum(0), dx.sum(0)


def relu_mask_bias(g, out, dtype=F64):
    """(g where out > 0 else 0, its column sums); out None: no mask"""
    g = g.to(dtype)
    gm = g if out is None else torch.where(out > 0, g, torch.zeros_like(g))
    return gm, gm.sum(0)


# ------------------------------------------------------------------------------------------------ the Linear layers
def linear128(A, W, bias=None, alpha=1.0, relu=False, gather=None, ln=None, add_pre=None, add_post=None, mask=None, eps=EPS, dtype=F64,
              prod=None):
    """(out, stats or None) in the order include/csplat.h documents:
         alpha (A W^T) -> + bias -> + ga[ia] + gb[ib] -> + add_pre -> ReLU (keeps a NaN) -> LayerNorm (gamma, beta) -> + add_post -> mask > 0
    W [128][128] is the matrix as torch's Linear.weight holds it, whatever storage the kernel reads it from; prod: A W^T of this dtype,
    when the caller has it already"""
    v = (A.to(dtype) @ W.to(dtype).t()) if prod is None else prod
    v = alpha * v
    if bias is not None:
        v = v + bias.to(dtype)
    if gather is not None:
        ga, ia, gb, ib = gather
        v = v + (ga.to(dtype)[ia] + gb.to(dtype)[ib])
    if add_pre is not None:
        v = v + add_pre.to(dtype)
    if relu:
        v = torch.relu(v)
    stats = None
    if ln is not None:
        v, stats = layer_norm(v, ln[0], ln[1], eps, dtype)
    if add_post is not None:
        v = v + add_post.to(dtype)
    if mask is not None:
        v = torch.where(mask > 0, v, torch.zeros_like(v))
    return v, stats


def linear128_row_scale(A, W, bias=None, alpha=1.0, gather=None, add_pre=None, add_post=None):
    """[M] float64: max_j sum_k |alpha a_ik w_jk| plus the magnitudes of the addends -- what a row's rounding errors are proportional to"""
    s = abs(alpha) * (A.double().abs() @ W.double().abs().t())
    if bias is not None:
        s = s + bias.double().abs()
    if gather is not None:
        ga, ia, gb, ib = gather
        s = s + ga.double().abs()[ia] + gb.double().abs()[ib]
    for t in (add_pre, add_post):
        if t is not None:
            s = s + t.double().abs()
    return s.amax(1)


def weight_storage(W, layout):
    """(storage tensor, ldw, w_transposed, element offset) for the four ways csplat_linear128_ex reads a weight:
    'plain' [128][128]; 'slice' columns 128..255 of a [128][384] matrix; 'transpose' the transpose of a [128][128] one; 'transposed slice'"""
    if layout == "plain":
        return W.contiguous(), 128, 0, 0
    if layout == "slice":
        wide = torch.full((128, 384), 77.0)
        wide[:, 128:256] = W
        return wide, 384, 0, 128
    if layout == "transpose":
        return W.t().contiguous(), 128, 1, 0
    if layout == "transposed slice":
        wide = torch.full((128, 384), 77.0)
        wide[:, 256:] = W.t()
        return wide, 384, 1, 256
    raise ValueError(layout)


def linear_narrow(x, W, bias, relu, dtype=F64):
    y = x.to(dtype) @ W.to(dtype).t()
    if bias is not None:
        y = y + bias.to(dtype)
    return torch.relu(y) if relu else y


def node_update(agg, x, p, dtype=F64):
    """(x', xa', xb'): h = relu(agg Wa^T + x Wx^T + b0); h = relu(h W2^T + b2); x' = LN(h W3^T + b3) + x; xa' = x' Wi^T, xb' = x' Wj^T"""
    q = {k: v.to(dtype) for k, v in p.items()}
    agg, x = agg.to(dtype), x.to(dtype)
    h = torch.relu(agg @ q["Wa"].t() + x @ q["Wx"].t() + q["b0"])
    h = torch.relu(h @ q["W2"].t() + q["b2"])
    xn = layer_norm(h @ q["W3"].t() + q["b3"], q["gamma"], q["beta"], EPS, dtype)[0] + x
    return xn, xn @ q["Wi"].t(), xn @ q["Wj"].t()


def dw128(g, x, x_relu=False, dtype=F64):
    """(dW [128][128] = g^T x', dbias = column sums of g), x' = relu(x) with x_relu"""
    g, x = g.to(dtype), x.to(dtype)
    if x_relu:
        x = torch.relu(x)
    return g.t() @ x, g.sum(0)


# ------------------------------------------------------------------------------------------------ graph structure and row movers
def csr(keys, N):
    """(rowptr [N + 1] int32, perm [E] int32): edge ids grouped by key, ascending edge id inside a row -- written as a counting sort"""
    keys = np.asarray(keys, np.int64)
    cnt = np.zeros(N + 1, np.int64)
    for k in keys:
        cnt[k + 1] += 1
    rowptr = np.cumsum(cnt)
    cur = rowptr[:-1].copy()
    perm = np.zeros(len(keys), np.int64)
    for e, k in enumerate(keys):
        perm[cur[k]] = e
        cur[k] += 1
    return rowptr.astype(np.int32), perm.astype(np.int32)


def csr_fast(keys, N):
    """the same by numpy (tests/test_gnn_kernels_cpu.py checks it against csr() on every graph shape)"""
    keys = np.asarray(keys, np.int64)
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(keys, minlength=N))]).astype(np.int32)
    return rowptr, np.argsort(keys, kind="stable").astype(np.int32)


def segment_sum(msg, keys, N, dtype=F64):
    """agg[n] = sum of msg[e] over the edges with keys[e] = n"""
    out = torch.zeros(N, msg.shape[1], dtype=dtype)
    return out.index_add_(0, keys, msg.to(dtype)) if msg.shape[0] else out


def segment_abs_sum(msg, keys, N):
    return segment_sum(msg.double().abs(), keys, N, F64)


def edge_combine(xa, xb, ec, ei, relu, dtype=F64):
    """relu?((xa[dst] + xb[src]) + ec), dst = ei[1], src = ei[0]"""
    v = (xa.to(dtype)[ei[1]] + xb.to(dtype)[ei[0]]) + ec.to(dtype)
    return torch.relu(v) if relu else v


def edge_combine_bwd(g, out, ei, N, relu, dtype=F64):
    """(g masked by out > 0, dxa = its sums per destination, dxb = per source)"""
    gm = relu_mask_bias(g, out if relu else None, dtype)[0]
    return gm, segment_sum(gm, ei[1], N, dtype), segment_sum(gm, ei[0], N, dtype)


# ================================================================================================ size lists and input builders
# (each size is stated against the launch constant it crosses in tests/test_gnn_kernels_cpu.py)
ROWS32_M = (1, 31, 32, 33, 65536)
PERSIST_M = (65537, 65568, 131073)
GATHER_M = (1, 33, 128, 129, 255, 257, 65537)
LN_BWD_M = (1, 8, 9, 64, 65, 511, 513, 65536, 65537)
CSR_N = (1, 2047, 2048, 2049, 4097, 70001)
WIDTHS = (128, 32, 20, 6)
NARROW_K = (1, 5, 32)
NARROW_M = (64, 65, 131073)
DW_M = (1, 63, 65, 16385)
HUB_DEGREE = 3000          # k_sort_rows is an insertion sort: <= 3000^2 / 2 moves by ONE thread when k_fill left the row reversed
LAYOUTS = ("plain", "slice", "transpose", "transposed slice")
ROW_CLASSES = ("ordinary", "1e-3", "1e+3", "1e-6..1e+4 inside the row", "1e-30", "1e+20", "one-hot", "zero")
LN_CLASSES = ("mean 16 std 1/16", "mean 64 std 1/16", "constant", "var << eps", "1e-3", "1", "1e+3", "3 randn + 0.5")
LN_CONSTANTS = (3.0, -0.5, 16.0, 0.0)


def row_classes(M, seed=0):
    """A [M][128]: row i is of class ROW_CLASSES[i % 8]"""
    g = _gen(100 + M + seed)
    A = torch.randn(M, 128, generator=g)
    mag = 10.0 ** (torch.rand(M, 128, generator=g) * 10.0 - 6.0)
    i = torch.arange(M)
    A[i % 8 == 1] *= 1e-3
    A[i % 8 == 2] *= 1e+3
    A[i % 8 == 3] *= mag[i % 8 == 3]
    A[i % 8 == 4] *= 1e-30
    A[i % 8 == 5] *= 1e+20
    hot = i[i % 8 == 6]
    A[hot] = 0.0
    A[hot, (hot // 8) % 128] = 1e-3
    A[i % 8 == 7] = 0.0
    return A


def ln_rows(M, seed=0):
    """x [M][128]: row i is of class LN_CLASSES[i % 8]; a constant row holds LN_CONSTANTS[(i // 8) % 4] (its sum and mean are exact in
    float32 in any order, so the centred row is exactly 0)"""
    g = _gen(200 + M + seed)
    x = torch.randn(M, 128, generator=g)
    i = torch.arange(M)
    x[i % 8 == 0] = 16.0 + x[i % 8 == 0] / 16.0
    x[i % 8 == 1] = 64.0 + x[i % 8 == 1] / 16.0
    for c, v in enumerate(LN_CONSTANTS):
        x[(i % 8 == 2) & ((i // 8) % 4 == c)] = v
    x[i % 8 == 3] = 1.0 + 1e-4 * x[i % 8 == 3]
    x[i % 8 == 4] *= 1e-3
    x[i % 8 == 6] *= 1e+3
    x[i % 8 == 7] = 3.0 * x[i % 8 == 7] + 0.5
    return x


def small_variance_row(seed=0):
    """a row with var << eps: 1 + 1e-4 randn (LN_CLASSES[3])"""
    return 1.0 + 1e-4 * torch.randn(128, generator=_gen(350 + seed))


def hard_bias(mean=16.0, seed=0):
    """a bias row of the given mean and std 1/16"""
    return mean + torch.randn(128, generator=_gen(300 + int(mean) + seed)) / 16.0


def linear_params(seed=0):
    """(W [128][128] of O(0.1), bias, gamma, beta)"""
    g = _gen(400 + seed)
    return (0.1 * torch.randn(128, 128, generator=g), torch.randn(128, generator=g), 1.0 + 0.3 * torch.randn(128, generator=g),
            torch.randn(128, generator=g))


def addends(M, seed=0):
    """(add_pre, add_post, mask) [M][128]; the mask holds negative entries, exact +0 and -0 (all three: 'not positive')"""
    g = _gen(500 + M + seed)
    pre, post, mask = (torch.randn(M, 128, generator=g) for _ in range(3))
    mask[:, 5] = 0.0
    mask[:, 9] = -0.0
    return pre, post, mask


def gather_case(M, pattern, seed=0):
    """(ga [N][128], ia [M], gb, ib), N = max(M, 2): 'equal' every index the same, 'last' every index N - 1, 'perm' a permutation"""
    g = _gen(600 + M + seed)
    N = max(M, 2)
    ga, gb = torch.randn(N, 128, generator=g), torch.randn(N, 128, generator=g)
    if pattern == "equal":
        ia, ib = torch.full((M,), 1 % N, dtype=torch.int64), torch.zeros(M, dtype=torch.int64)
    elif pattern == "last":
        ia = ib = torch.full((M,), N - 1, dtype=torch.int64)
    else:
        ia, ib = torch.randperm(N, generator=g)[:M], torch.randperm(N, generator=g)[:M]
    return ga, ia.contiguous(), gb, ib.contiguous()


def node_update_params(seed=0, hard=None):
    """weights of O(1 / sqrt(128)) so that every layer keeps O(1) rows; hard = a mean, or the row itself [128]: W3 = 0 and b3 =
    hard_bias(mean) / that row, so that every row in front of the LayerNorm is that bias row"""
    g = _gen(700 + seed)
    p = {k: torch.randn(128, 128, generator=g) / 128 ** 0.5 for k in ("Wa", "Wx", "W2", "W3", "Wi", "Wj")}
    p.update({k: 0.5 * torch.randn(128, generator=g) for k in ("b0", "b2", "b3")})
    p["gamma"], p["beta"] = 1.0 + 0.3 * torch.randn(128, generator=g), torch.randn(128, generator=g)
    if hard is not None:
        p["W3"] = torch.zeros(128, 128)
        p["b3"] = hard.clone() if torch.is_tensor(hard) else hard_bias(hard)
    return p


GRAPHS = ("hub", "last", "duplicates", "self loops", "degrees 0..9")


def graph(N, kind, seed=0):
    """ei [2][E] int64 on N nodes.  'hub': node N // 2 is the destination of HUB_DEGREE edges (every edge of the graph) whose sources
    run over all nodes; 'last': every edge ends at node N - 1; 'duplicates': 40 edges, each present 5 times; 'self loops': one per node
    (at most 3000); 'degrees 0..9': node n has in-degree n % 10 (the first 3000 nodes), sources random -- every residue mod 4 of the
    four-at-a-time loop, and rows of length 0"""
    g = _gen(800 + N + seed)
    if kind == "hub":
        E = HUB_DEGREE
        src, dst = torch.arange(E) % N, torch.full((E,), N // 2)
    elif kind == "last":
        E = 257
        src, dst = torch.randint(0, N, (E,), generator=g), torch.full((E,), N - 1)
    elif kind == "duplicates":
        s, d = torch.randint(0, N, (40,), generator=g), torch.randint(0, N, (40,), generator=g)
        src, dst = s.repeat(5), d.repeat(5)
    elif kind == "self loops":
        src = dst = torch.arange(min(N, 3000))
    elif kind == "degrees 0..9":
        n = torch.arange(min(N, 3000))
        dst = torch.repeat_interleave(n, n % 10)
        dst = dst[torch.randperm(dst.numel(), generator=g)]          # (edge ids of a row are not consecutive)
        src = torch.randint(0, N, (dst.numel(),), generator=g)
    else:
        raise ValueError(kind)
    return torch.stack([src.long(), dst.long()]).contiguous()


MESSAGES = ("ordinary", "cancelling", "zeros")


def messages(ei, L, kind, seed=0):
    """msg [E][L].  'cancelling': the first edge of every destination row of three or more edges carries +1e6 and its last one -1e6 (a
    plain running sum loses 1e6 * eps = 0.06 of the O(1) remainder there); 'zeros': exact +0 and -0 rows mixed into ordinary ones"""
    E = int(ei.shape[1])
    g = _gen(900 + E + L + seed)
    msg = torch.randn(E, L, generator=g)
    if kind == "cancelling" and E:
        rowptr, perm = csr_fast(ei[1].numpy(), int(ei.max()) + 1)
        deg = rowptr[1:] - rowptr[:-1]
        rows = np.nonzero(deg >= 3)[0]
        msg[torch.from_numpy(perm[rowptr[rows]].astype(np.int64))] = 1e6
        msg[torch.from_numpy(perm[rowptr[rows + 1] - 1].astype(np.int64))] = -1e6
    if kind == "zeros":
        msg[0::3] = 0.0
        msg[1::3] = -0.0
    return msg
