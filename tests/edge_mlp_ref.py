"""Plain torch restatement, on the CPU, of what the one-launch kernels of csrc/csplat_edge_mlp.hip compute (k_edge_mlp3r<F16, MODE 0 / 1 / 2>,
k_node_update_b3, k_rows_chain, k_absmax and the two pack kernels), for tests/test_edge_mlp_cpu.py (which checks THIS file against itself
and against the constants of the .hip file) and tests/test_edge_mlp_gpu.py (which checks the kernels against this file).  Nothing is
imported from csplat or meshnet.  Two restatements of every operation:

  exact(op, ..., dtype)        the operation itself, in float64 or float32
  model(op, ..., kind, acc)    the operation as the kernel's ARITHMETIC states it: every operand of every product cut into 16-bit pieces
                               by round-to-nearest-even casts (two fp16 pieces for kind "f16", three bf16 pieces for "bf16"), only the
                               products of piece indices i + j <= NP - 1 kept, everything multiplied by the power of two the kernel runs
                               under (edge kernel: s = cs / alpha with cs = 2^(4 - ex) from max |e0| in mode "f16", 1 in "bf16"; node
                               kernels: 2^-4 / 1), biases and node terms as accumulator starts, ReLU as x < 0 ? 0 : x (keeps a NaN),
                               LayerNorm with s^2 eps.  acc = float64 accumulates the kept products exactly; acc = float32 rounds what
                               the kernel rounds: the node-term sum, each layer's accumulators -- after every matrix instruction of the kernels'
                               accumulation chain (accumulate()) -- before they are cut into pieces again, the LayerNorm (and the
                               residual addition, and the sum of a node's pieces).

op is "edge" (messages; the narrow-row form when xa is None), "node" (the node update) or "chain" (rows_chain modes 0 and 1).
Also here, because both test files need them: the SIZE LISTS, the row classes and the input builders."""
import math

import numpy as np
import torch

F64, F32 = torch.float64, torch.float32
EPS = 1e-5                    # nn.LayerNorm's default
# ---- what the kernels' constants are taken to be (tests/test_edge_mlp_cpu.py parses each from csrc/csplat_edge_mlp.hip)
TILE = 32                     # rows per tile
STEP_ROWS = 64                # two tiles per workgroup step
EM_STRIDE = 136
GRID_CAP = 256                # persistent grid: min(ceil(rows / 64), 256) workgroups
NO_LOOP_ROWS = GRID_CAP * STEP_ROWS          # 16 384: the last size at which no workgroup loops
CHUNK_ROWS = 1 << 22
GROUP = 8                     # rows of one piece group
NP = {"f16": 2, "bf16": 3}
NPROD = {"f16": 3, "bf16": 6}
NODE_SC = {"f16": 2.0 ** -4, "bf16": 1.0}
EX_CLAMP = (-96, 100)
ABSMAX_GRID_CAP, ABSMAX_LANES = 2048, 256
PIECE_DTYPE = {"f16": torch.float16, "bf16": torch.bfloat16}
F16_MAX = 65504.0

EDGE_E = (1, 31, 32, 33, 63, 64, 65, 16384, 16385, 16417, 32769)
NODE_N = (1, 31, 32, 33, 1031)
NARROW_K = (4, 12, 20, 124, 128)
NARROW_M = (1, 33, 65, 16385)
ABSMAX_N = (0, 4, 1020, 1024, 1028, 2_097_152, 2_097_156)
ALPHAS = (0.5, 1.0, 64.0, 16384.0)
ROW_CLASSES = ("ordinary", "2^0 .. 2^-20 of the largest", "zero row", "one-hot")
WEIGHT_KINDS = ("0.1 randn", "down to 1e-3")
LAUNCHES = ("mixed", "outlier 2^6", "outlier 2^12", "no node terms 2^-6", "no node terms 2^-12", "understated absmax 2^-6",
            "overstated absmax 2^6")
NODE_CLASSES = ("1e-3", "1", "30 / 5", "1e+3", "1e+5", "zero row")
NODE_SCALES = ((1e-3, 1e-3), (1.0, 1.0), (30.0, 5.0), (1e3, 1e3), (1e5, 1e5), (0.0, 0.0))       # (aggregate, latent)
INDEX_PATTERNS = ("ia == ib", "one node", "last node", "random")


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def edge_in_domain(kind, launch, wkind, alpha):
    """the launches whose zero, small, one-hot and ordinary rows the piece arithmetic serves to fp32's own accuracy (held by
    tests/test_edge_mlp_cpu.py): bf16 pieces always; fp16 pieces with 0.1 randn weights as long as alpha x (the launch's own 2^6) <= 2^6"""
    if kind == "bf16":
        return True
    if wkind != "0.1 randn":
        return False
    spread = {"mixed": 1.0, "outlier 2^6": 64.0, "overstated absmax 2^6": 64.0}.get(launch)
    return spread is not None and alpha * spread <= 64.0


def edge_comparable(kind, alpha, name):
    """fp16 pieces at alpha > 64: a row whose edge features are zero or tiny holds its node terms at s = cs / alpha, a few fp16 quanta.  One
    fp32 rounding more or less moves a piece by a whole quantum there: model(acc = float32) is up to 1.6e-4 from model(acc = float64) on
    these rows at 16 384 of them -- a bar of 1.3e-3, which the rule of the GPU file (a bar above 1e-3 = ill-conditioned inputs) does not
    admit; with few rows the largest of a handful of such flips is a lottery.  These rows are held to be finite, not compared"""
    return not (kind == "f16" and alpha > 64.0 and name in ROW_CLASSES[1:3])


def chain_in_domain(kind, name, mode):
    """rows_chain mode 0 has neither a LayerNorm nor a bias: nothing of O(1) is under its row scale, and rows of 1e-3 x 2^-4 are fp16
    denormals (tests/test_edge_mlp_cpu.py)"""
    return kind == "bf16" or name != "1e-3" or mode == 1


def er_src_col(layer, pos):
    """the contraction order of layers 2 and 3: position pos of an activation row <-> feature (the .hip file's er_src_col)"""
    if layer == 0:
        return pos
    j, h, r = pos >> 5, (pos >> 4) & 1, pos & 15
    return 32 * j + 8 * (r >> 2) + 4 * h + (r & 3)


def scale_exponent(m):
    """ex of the edge kernel's cs = 2^(4 - ex): frexp of max |e0|, clamped; 0 for 0, NaN, Inf and anything not below 3e38"""
    m = float(np.float32(m))
    ex = 0
    if m > 0.0 and m < 3.0e38:
        ex = math.frexp(m)[1]
    return max(EX_CLAMP[0], min(EX_CLAMP[1], ex))


# ------------------------------------------------------------------------------------------------ pieces
def split(v, kind, npieces=None):
    """v (float64 holding what the kernel holds in fp32) -> its pieces as float64: p_q = cast(r_q), r_(q+1) = r_q - p_q.  An element beyond
    the piece format's range gives (Inf, -Inf, ...) or (Inf, NaN, ...): the products then hold NaN, as the kernel's do."""
    dt = PIECE_DTYPE[kind]
    r, out = v.to(F64), []
    for _ in range(npieces or NP[kind]):
        p = r.to(F32).to(dt).to(F64)
        out.append(p)
        r = r - p
    return out


def piece_product(ap, wp, keep=None):
    """sum over the kept (i, j), i + j <= keep, of ap_j wp_i^T, accumulated in float64: sum_i (sum_(j <= keep - i) ap_j) wp_i^T"""
    keep = len(ap) - 1 if keep is None else keep
    acc = None
    for i, w in enumerate(wp):
        js = [a for j, a in enumerate(ap) if i + j <= keep]
        if not js:
            continue
        if any(not bool(torch.isfinite(a).all()) for a in js):       # (Inf - Inf inside a partial sum of pieces: multiply piece by piece)
            t = sum(a @ w.t() for a in js)
        else:
            t = sum(js) @ w.t()
        acc = t if acc is None else acc + t
    return acc


def _rnd(v, acc):
    return v.to(F32).to(F64) if acc == F32 else v


# (weight piece, activation piece) of a contraction step's products in the order the kernels issue them: small terms first
CHAIN = {"f16": ((0, 1), (1, 0), (0, 0)), "bf16": ((0, 2), (2, 0), (1, 1), (0, 1), (1, 0), (0, 0))}


def accumulate(start, ap, wp, layer, kind, acc, keep=None):
    """start + the kept piece products.  acc = float64: exactly.  acc = float32: as the kernels' accumulation chain rounds -- eight contraction
    steps of 16 positions (8 st + i and 64 + 8 st + i; for layer > 0 a position is feature er_src_col(layer, position)), NPROD matrix
    instructions per step in the order CHAIN, each taken as its exact 16-term sum added to the fp32 accumulator with one rounding"""
    if acc != F32 or keep is not None or len(ap) != NP[kind]:
        return _rnd(start + piece_product(ap, wp, keep), acc)
    a = start.to(F32).to(F64) + torch.zeros(ap[0].shape[0], wp[0].shape[0], dtype=F64)
    for st in range(8):
        cols = torch.tensor([er_src_col(layer, 64 * h + 8 * st + i) for h in (0, 1) for i in range(8)])
        As, Ws = [p[:, cols] for p in ap], [w[:, cols].t().contiguous() for w in wp]
        for wi, xj in CHAIN[kind]:
            a = (a + As[xj] @ Ws[wi]).to(F32).to(F64)
    return a


def relu_nan(v):
    return torch.where(v < 0, torch.zeros_like(v), v)


def layer_norm(v, gamma, beta, eps, dtype):
    """two passes, in `dtype`; eps a python float or a 0-d tensor of that dtype"""
    v, gamma, beta = v.to(dtype), gamma.to(dtype), beta.to(dtype)
    mean = v.mean(1, keepdim=True)
    d = v - mean
    return d / ((d * d).mean(1, keepdim=True) + eps).sqrt() * gamma + beta


def _scaled_eps(eps, s, acc):
    if acc == F32:      # eps *= s * s in fp32, as the kernel forms it (2^200 is Inf there)
        s32 = torch.tensor(s, dtype=F32)
        return torch.tensor(eps, dtype=F32) * (s32 * s32)
    return eps * s * s


# ------------------------------------------------------------------------------------------------ the edge message MLP
def exact_edge(c, alpha=1.0, dtype=F64):
    """LN(W2 relu(W1 relu(alpha W0 e0 + b0 + xa[ia] + xb[ib]) + b1) + b2); narrow rows (xa None): e0 is [M][K] and meets the first K
    columns of W0"""
    q = {k: (v.to(dtype) if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in c.items()}
    e0 = q["e0"]
    v = alpha * (e0 @ q["W0"][:, :e0.shape[1]].t()) + q["b0"]
    if q.get("xa") is not None:
        v = v + (q["xa"][q["ia"]] + q["xb"][q["ib"]])
    h = torch.relu(v)
    h = torch.relu(h @ q["W1"].t() + q["b1"])
    return layer_norm(h @ q["W2"].t() + q["b2"], q["gamma"], q["beta"], EPS, dtype)


def model_edge(c, alpha=1.0, kind="f16", acc=F64, e0_absmax=None, npieces=None, keep=None):
    e0 = c["e0"].to(F32)
    if e0.shape[1] < 128:
        e0 = torch.cat([e0, torch.zeros(e0.shape[0], 128 - e0.shape[1])], 1)
    cs = 1.0
    if kind == "f16":
        m = float(e0.abs().max()) if (e0_absmax is None and e0.numel()) else float(e0_absmax or 0.0)
        cs = 2.0 ** (4 - scale_exponent(m))
    s = cs / alpha
    s32 = torch.tensor(s, dtype=F32)
    e = (e0 * torch.tensor(cs, dtype=F32)).to(F64) if kind == "f16" else e0.to(F64)       # (an fp32 product: exact, or Inf / 0 as fp32 has it)
    if c.get("xa") is not None:
        if acc == F32:      # (xa + xb) rounded, then one fma with s and s b0
            t = (c["xa"].to(F32)[c["ia"]] + c["xb"].to(F32)[c["ib"]]).to(F64)
            G = (t * s32.to(F64) + (c["b0"].to(F32) * s32).to(F64)).to(F32).to(F64)
        else:
            G = (c["xa"].to(F64)[c["ia"]] + c["xb"].to(F64)[c["ib"]] + c["b0"].to(F64)) * s
    else:
        G = (c["b0"].to(F32) * s32).to(F64).expand(e0.shape[0], 128)
    sp = lambda t: split(t, kind, npieces)  # noqa: E731
    bias = lambda b: (b.to(F32) * s32).to(F64)  # noqa: E731
    a1 = accumulate(G, sp(e), sp(c["W0"].to(F64)), 0, kind, acc, keep)
    a2 = accumulate(bias(c["b1"]), sp(relu_nan(a1)), sp(c["W1"].to(F64)), 1, kind, acc, keep)
    a3 = accumulate(bias(c["b2"]), sp(relu_nan(a2)), sp(c["W2"].to(F64)), 1, kind, acc, keep)
    return layer_norm(a3, c["gamma"], c["beta"], _scaled_eps(EPS, s, acc), acc).to(F64)


# ------------------------------------------------------------------------------------------------ the node update
def sum_pieces(pieces, piece_ptr, dtype=F64):
    """agg[v] = pieces[pp[v]] + pieces[pp[v] + 1] + ..., added in that order from 0, in `dtype`"""
    pp = np.asarray(piece_ptr, np.int64)
    cnt = torch.from_numpy(pp[1:] - pp[:-1])
    p0 = torch.from_numpy(pp[:-1])
    pieces = pieces.to(dtype)
    out = torch.zeros(len(pp) - 1, pieces.shape[1], dtype=dtype)
    for k in range(int(cnt.max()) if cnt.numel() else 0):
        on = (cnt > k).nonzero()[:, 0]
        out[on] = out[on] + pieces[p0[on] + k]
    return out


def exact_node(agg, x, p, dtype=F64, piece_ptr=None):
    """(x', xa', xb', the hidden activations of the three layers)"""
    q = {k: v.to(dtype) for k, v in p.items()}
    agg = sum_pieces(agg, piece_ptr, dtype) if piece_ptr is not None else agg.to(dtype)
    x = x.to(dtype)
    h = torch.relu(agg @ q["Wa"].t() + x @ q["Wx"].t() + q["b0"])
    h = torch.relu(h @ q["W2"].t() + q["b2"])
    xn = layer_norm(h @ q["W3"].t() + q["b3"], q["gamma"], q["beta"], EPS, dtype) + x
    return xn, xn @ q["Wi"].t(), xn @ q["Wj"].t()


def model_node(agg, x, p, kind="f16", acc=F64, piece_ptr=None, npieces=None, keep=None):
    sc = NODE_SC[kind]
    agg = sum_pieces(agg, piece_ptr, acc).to(F64) if piece_ptr is not None else agg.to(F32).to(F64)
    x = x.to(F32).to(F64)
    sp = lambda t: split(t, kind, npieces)  # noqa: E731
    W = {k: sp(p[k].to(F64)) for k in ("Wa", "Wx", "W2", "W3", "Wi", "Wj")}
    a = accumulate(p["b0"].to(F64) * sc, sp(agg * sc), W["Wa"], 0, kind, acc, keep)
    a = accumulate(a, sp(x * sc), W["Wx"], 0, kind, acc, keep)
    a = accumulate(p["b2"].to(F64) * sc, sp(relu_nan(a)), W["W2"], 1, kind, acc, keep)
    a = accumulate(p["b3"].to(F64) * sc, sp(relu_nan(a)), W["W3"], 1, kind, acc, keep)
    y = layer_norm(a, p["gamma"], p["beta"], _scaled_eps(EPS, sc, acc), acc)
    xn = (y + x.to(acc)).to(F64)
    xs = sp(xn * sc)
    z = torch.zeros(128, dtype=F64)
    xa = accumulate(z, xs, W["Wi"], 1, kind, acc, keep) / sc
    xb = accumulate(z, xs, W["Wj"], 1, kind, acc, keep) / sc
    return xn, xa, xb


# ------------------------------------------------------------------------------------------------ rows_chain
def exact_chain(x, mode, Wf, Ws, b0=None, b1=None, dtype=F64):
    """mode 0: (x Wf^T, x Ws^T); mode 1: relu(Ws relu(Wf x + b0) + b1), missing biases zero.  Also returns the hidden layer (mode 1)"""
    x, Wf, Ws = x.to(dtype), Wf.to(dtype), Ws.to(dtype)
    if mode == 0:
        return x @ Wf.t(), x @ Ws.t()
    z = torch.zeros(128, dtype=dtype)
    h = torch.relu(x @ Wf.t() + (z if b0 is None else b0.to(dtype)))
    return torch.relu(h @ Ws.t() + (z if b1 is None else b1.to(dtype))), h


def model_chain(x, mode, Wf, Ws, b0=None, b1=None, kind="f16", acc=F64, npieces=None, keep=None):
    sc = NODE_SC[kind]
    sp = lambda t: split(t, kind, npieces)  # noqa: E731
    xs, wf, ws = sp(x.to(F32).to(F64) * sc), sp(Wf.to(F64)), sp(Ws.to(F64))
    z = torch.zeros(128, dtype=F64)
    if mode == 0:
        return accumulate(z, xs, wf, 0, kind, acc, keep) / sc, accumulate(z, xs, ws, 0, kind, acc, keep) / sc
    a = accumulate((z if b0 is None else b0.to(F64)) * sc, xs, wf, 0, kind, acc, keep)
    a = accumulate((z if b1 is None else b1.to(F64)) * sc, sp(relu_nan(a)), ws, 1, kind, acc, keep)
    return relu_nan(a) / sc


def exact(op, *a, **kw):
    return {"edge": exact_edge, "node": exact_node, "chain": exact_chain}[op](*a, **kw)


def model(op, *a, **kw):
    return {"edge": model_edge, "node": model_node, "chain": model_chain}[op](*a, **kw)


# ------------------------------------------------------------------------------------------------ row scales and row errors
def ln_scale(r64):
    return r64.abs().amax(1).clamp_min(1.0)


def product_scale(a, W, bias=None):
    """max_j sum_k |a_ik w_jk| plus the bias magnitude"""
    s = a.double().abs() @ W.double().abs().t()
    if bias is not None:
        s = s + bias.double().abs()
    return s.amax(1)


def row_err(got, ref, scale):
    """[rows]: max_j |got - ref| / scale; a row that is non-finite on either side: Inf"""
    got, ref = got.to(F64), ref.to(F64)
    scale = torch.broadcast_to(torch.as_tensor(scale, dtype=F64).reshape(-1), (got.shape[0],)).clamp_min(1e-300)
    e = (got - ref).abs().amax(1) / scale
    return torch.where(torch.isfinite(e), e, torch.full_like(e, float("inf")))


# ------------------------------------------------------------------------------------------------ pieces of the fused aggregation
def runs(dst_sorted, group=GROUP):
    """(start [P], end [P], gp0 [ceil(E / group)], pp [N + 1] is left to the caller): the runs of equal destination, cut additionally at
    every multiple of `group` rows, in row order"""
    d = np.asarray(dst_sorted, np.int64)
    E = len(d)
    if E == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.int32)
    new = (np.arange(E) % group == 0)
    new[1:] |= d[1:] != d[:-1]
    start = np.nonzero(new)[0]
    end = np.concatenate([start[1:], [E]])
    pidx = np.cumsum(new) - 1
    return start, end, pidx[0::group].astype(np.int32)


def piece_ptr(dst_sorted, N, group=GROUP):
    """pp [N + 1] int32: node v owns pieces pp[v] .. pp[v + 1] - 1"""
    start, _end, _ = runs(dst_sorted, group)
    d = np.asarray(dst_sorted, np.int64)
    owner = d[start] if len(start) else np.zeros(0, np.int64)
    return np.concatenate([[0], np.cumsum(np.bincount(owner, minlength=N))]).astype(np.int32)


def run_sums(msg, start, end, dtype=F64):
    """[P][128]: the rows of each run added in row order from 0, in `dtype` (a run has at most GROUP rows)"""
    msg = msg.to(dtype)
    out = torch.zeros(len(start), msg.shape[1], dtype=dtype)
    s, e = torch.from_numpy(np.asarray(start)), torch.from_numpy(np.asarray(end))
    for k in range(GROUP):
        on = (s + k < e).nonzero()[:, 0]
        if on.numel():
            out[on] = out[on] + msg[s[on] + k]
    return out


# ================================================================================================ input builders
def weights(kind, seed=0, n=3):
    """n [128][128] matrices: '0.1 randn', or the same with element magnitudes spread log-uniformly down to 1e-3 of the largest"""
    g = _gen(1000 + seed)
    Ws = [0.1 * torch.randn(128, 128, generator=g) for _ in range(n)]
    if kind == "down to 1e-3":
        Ws = [W * 10.0 ** (-3.0 * torch.rand(128, 128, generator=g)) for W in Ws]
        for W in Ws:
            W[5, 7] = W.abs().max() * 1e-3
    else:
        assert kind == "0.1 randn"
    return Ws


def edge_params(kind="0.1 randn", seed=0):
    g = _gen(1100 + seed)
    W0, W1, W2 = weights(kind, seed)
    return dict(W0=W0, W1=W1, W2=W2, b0=0.3 * torch.randn(128, generator=g), b1=0.3 * torch.randn(128, generator=g),
                b2=0.3 * torch.randn(128, generator=g), gamma=1.0 + 0.3 * torch.randn(128, generator=g), beta=torch.randn(128, generator=g))


def edge_rows(E, seed=0):
    """e0 [E][128]: row i is of class ROW_CLASSES[i % 4]; the scaled rows cycle through 2^0 .. 2^-20"""
    g = _gen(1200 + E + seed)
    e0 = torch.randn(E, 128, generator=g)
    i = torch.arange(E)
    e0[i % 4 == 1] *= (2.0 ** -((i[i % 4 == 1] // 4) % 21).double()).float()[:, None]
    e0[i % 4 == 2] = 0.0
    hot = i[i % 4 == 3]
    e0[hot] = 0.0
    e0[hot, (hot // 4) % 128] = 1.0
    return e0


def indices(E, N, pattern, seed=0):
    g = _gen(1300 + E + seed)
    if pattern == "ia == ib":
        ia = torch.randint(0, N, (E,), generator=g)
        return ia, ia.clone()
    if pattern == "one node":
        return torch.full((E,), N // 2, dtype=torch.int64), torch.full((E,), N // 2, dtype=torch.int64)
    if pattern == "last node":
        return torch.full((E,), N - 1, dtype=torch.int64), torch.randint(0, N, (E,), generator=g)
    assert pattern == "random"
    return torch.randint(0, N, (E,), generator=g), torch.randint(0, N, (E,), generator=g)


def outlier_row(E):
    return (E // 2) & ~3          # (an 'ordinary' row)


def edge_case(E, launch="mixed", wkind="0.1 randn", pattern="random", seed=0):
    """One launch: the dict exact_edge / model_edge take, plus 'absmax' (what is handed in as e0_absmax), 'classes' (row -> index into
    'names') and 'names'.  Launch kinds (LAUNCHES): 'mixed' the four row classes cycling; 'outlier 2^k' the same with ONE ordinary row 2^k
    above (a class of its own); 'no node terms 2^-k' xa, xb, b0 zero and every row but row 0 scaled by 2^-k; 'understated / overstated
    absmax' the mixed launch with the true maximum times 2^-6 / 2^6 handed in"""
    N = max(2, min(E, 300))
    g = _gen(1400 + E + seed)
    c = edge_params(wkind, seed)
    c["e0"] = edge_rows(E, seed)
    c["xa"], c["xb"] = torch.randn(N, 128, generator=g), torch.randn(N, 128, generator=g)
    c["ia"], c["ib"] = indices(E, N, pattern, seed)
    classes = torch.arange(E) % 4
    names = list(ROW_CLASSES)
    factor = 1.0
    if launch.startswith("outlier"):
        k = int(launch.split("^")[1])
        r = outlier_row(E)
        c["e0"][r] *= 2.0 ** k
        classes[r] = 4
        names.append("the outlier")
    elif launch.startswith("no node terms"):
        k = int(launch.split("^-")[1])
        c["xa"], c["xb"], c["b0"] = torch.zeros(N, 128), torch.zeros(N, 128), torch.zeros(128)
        c["e0"][1:] *= 2.0 ** -k
        classes[0] = 4
        names.append("the largest row")
    elif launch.startswith("understated"):
        factor = 2.0 ** -6
    elif launch.startswith("overstated"):
        factor = 2.0 ** 6
    else:
        assert launch == "mixed", launch
    c["absmax"] = float(c["e0"].abs().max()) * factor if E else 0.0
    c["classes"], c["names"] = classes, names
    return c


def narrow_case(M, K, seed=0):
    """x [M][K] at three scales cycling, W0 [128][128] with zero columns from K on"""
    g = _gen(1500 + M + K + seed)
    c = edge_params("0.1 randn", seed + 1)
    c["W0"] = torch.zeros(128, 128)
    c["W0"][:, :K] = torch.randn(128, K, generator=g) / K ** 0.5
    c["e0"] = torch.randn(M, K, generator=g) * torch.tensor([1.0, 2.0 ** -10, 2.0 ** -3])[torch.arange(M) % 3][:, None]
    c["absmax"] = float(c["e0"].abs().max())
    return c


def node_params(seed=0):
    g = _gen(1600 + seed)
    p = {k: torch.randn(128, 128, generator=g) / 128 ** 0.5 for k in ("Wa", "Wx", "W2", "W3", "Wi", "Wj")}
    p.update({k: 0.5 * torch.randn(128, generator=g) for k in ("b0", "b2", "b3")})
    p["gamma"], p["beta"] = 1.0 + 0.3 * torch.randn(128, generator=g), torch.randn(128, generator=g)
    return p


def node_rows(N, seed=0):
    """(agg, x) [N][128]: row i of class NODE_CLASSES[i % 6]"""
    g = _gen(1700 + N + seed)
    sc = torch.tensor(NODE_SCALES)[torch.arange(N) % len(NODE_SCALES)]
    return torch.randn(N, 128, generator=g) * sc[:, 0:1], torch.randn(N, 128, generator=g) * sc[:, 1:2]


AGG_GRAPHS = ("hub", "runs on boundaries", "many empty nodes", "random")


def agg_graph(E, kind, seed=0):
    """(dst sorted ascending [E] int64, src [E], N).  'hub': one node owns the middle half of the rows (at the sizes beyond one step its run
    crosses 8-row groups, both tiles of a step and, from 16 385 rows, the rows of two workgroups), the rest have runs of 1-3; 'runs on
    boundaries': runs of 4, 12, 16 and 32 rows repeating, which end on rows 4, 16, 32 and 64 of every 64 (a group, a tile and a step boundary,
    from a start that is on none); 'many empty
    nodes': destinations 50 apart (2 apart from 1000 rows on: the node tables stay small); 'random': random destinations on E // 3 + 1 nodes (E % 8 != 0 at every odd E of EDGE_E)"""
    g = _gen(1800 + E + seed)
    if kind == "hub":
        lo, hi = E // 4, E - E // 4
        left = torch.arange(lo) // 2
        right = torch.arange(E - hi) // 3 + (lo // 2 + 2)
        dst = torch.cat([left, torch.full((hi - lo,), lo // 2 + 1), right])
    elif kind == "runs on boundaries":
        lens = torch.tensor([4, 12, 16, 32]).repeat(E // 64 + 1)
        dst = torch.repeat_interleave(torch.arange(lens.numel()), lens)[:E]
    elif kind == "many empty nodes":
        dst = (50 if E < 1000 else 2) * (torch.arange(E) // 3) + 7
    else:
        dst, _ = torch.sort(torch.randint(0, E // 3 + 1, (E,), generator=g))
    dst = dst.long().contiguous()
    N = int(dst.max()) + 3 if E else 3
    return dst, torch.randint(0, N, (E,), generator=g), N
