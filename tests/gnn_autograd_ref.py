"""Plain torch restatement, on the CPU, of the autograd nodes of cloth-splatting_amd/meshnet/graph_ops.py that a MeshNet training step
runs -- EdgeCombine, SegmentSum, LayerNorm128, SplitKLinear, EdgeLatentLinear, EdgeFirstLayer, EdgeTailAggregate (+ the caller's affine
part) -- and of one InteractionNetwork.message_update, with the gradients left to torch's own autograd: index_select / index_add_ for
the gathers and sums, F.linear, the LayerNorm written out (biased variance, eps inside the root), ReLU as z * (z > 0) (gradient 0 at
z = 0).  Written from the formulas in graph_ops.py's docstrings and oracle/gnn_ref.py; nothing is imported from csplat or meshnet.
Every function computes in the dtype of the tensors it is given: tests/test_gnn_autograd_nodes_gpu.py runs it in float64 (the
reference) and in float32 (the yardstick e32), tests/test_gnn_autograd_nodes_cpu.py checks it against the module composition.

A Tape records every Linear, LayerNorm and affine step on the way forward; run() asks autograd for the gradient of every recorded
pre-activation as well, and Tape.scales() turns them into the row and column scales of tests/test_gnn_kernels_gpu.py's table:
  a Linear's output               max_j sum_k |alpha x_ik w_jk| + |bias| (+ what the caller adds: gathered rows)
  a Linear's input gradient       max_j sum_k |alpha dz_ik w_kj| per row (+ what the caller adds: the running sum g_next, a residual)
  db, dbeta                       per column, sum_i |term_ij|
  dW                              per element, sum_i |dz_ij| |x_ik| -- tests/test_gnn_kernels_gpu.py's scale -- where both factors are
                                  EXACT: x an input and dz a cotangent or a cotangent under an exact mask (SplitKLinear, EdgeFirstLayer and
                                  EdgeLatentLinear on their own); an element whose scale is 0 must then be exactly 0.
                                  A COMPUTED factor (an activation, a back-propagated gradient) carries an error relative to ITS
                                  row's scale, not to the entry's own value, so it counts with its row's largest entry:
                                    x an input, dz computed     sum_i max_j' |dz_ij'| |x_ik|      (tail dW1, a chain's first dW, message_update's first blocks)
                                    both computed               sum_i (max_j' |dz_ij'| |x_ik| + |dz_ij| max_k' |x_ik'|)      (hidden layers)
                                  With |dz_ij| |x_ik| alone, a hidden unit that is switched on in two rows of 257 at 3e-4 makes the float32
                                  restatement itself miss float64 by 4.5e-4 of that scale (the activation carries 1e-6 of its row's
                                  scale), and the bar calls the inputs ill-conditioned
  dgamma                          per column, sum_i |dy_ij| max(max_j' |xhat_ij'|, 1): xhat is behind a normalisation
Also here, because both test files need them: the SIZE TUPLES, the graphs, and the input draws WITHOUT ReLU TIES."""
import torch
import torch.nn.functional as F

import gnn_kernels_ref as R

F64, F32 = torch.float64, torch.float32
EPS = R.EPS

# ================================================================================================ sizes (each is stated against the
# constant it crosses in tests/test_gnn_autograd_nodes_cpu.py)
NODE_E = (1, 33, 257, 16383, 16384, 16385, 65537)   # rows32 row edges, SplitKLinear.BIG_ROWS, the rows32 -> persistent switch
NODE_N = (1, 2049, 2500)
LAYER_N = 16384                                     # the whole-layer (message_update) cases only: see layer_case()
SCALES = (1.0, 2.0, 16384.0)                        # 2^l: the first, the second and the last of 15 processor layers
TAIL_K = (1, 2, 3)                                  # Linear layers behind the first edge Linear
CHUNK_M = (1, 3071, 3072, 3073, 6145, 16384)        # the generic SplitKLinear path: around multiples of CHUNK = 3072
SPLITK_M = (511, 512, 16383, 16384, 16385)          # linear_rows' 512-row threshold, BIG_ROWS
LN_M = (1, 513, 65537)
TAIL_E = (257, 16385, 65537)
MARGIN = 2.0 ** -14       # four times 128 * 2^-23: the classical bound of a 128-term fp32 dot product, relative to sum |terms|
ROUNDS = 8


def nodes_for(E):
    """the node count a family of E edges runs on: one node for the two smallest (every edge a self loop of node 0), NODE_N[1] up to
    BIG_ROWS - 1, NODE_N[2] from BIG_ROWS on.  (k_sort_rows sorts a CSR row by insertion, one thread per row: no row may be much
    longer than R.HUB_DEGREE, so one node takes at most that many edges)"""
    N = NODE_N[0] if E <= 33 else (NODE_N[1] if E < 16384 else NODE_N[2])
    assert N > 1 or E <= R.HUB_DEGREE
    return N


def graph(E, N, kind, seed=0):
    """ei [2][E] int64: the first E edges of gnn_kernels_ref.graph(N, kind); when that graph has fewer, its edges that do not end in a
    node n with n % 7 == 3, followed by random edges that do not either (nodes of in-degree 0 remain; the random part stays far below
    the hub's degree)"""
    base = R.graph(N, kind, seed)
    E0 = int(base.shape[1])
    if E <= E0:
        return base[:, :E].contiguous()
    if N == 1:                      # (one node: every edge is its self loop)
        return torch.zeros(2, E, dtype=torch.int64)
    base = base[:, base[1] % 7 != 3]
    E0 = int(base.shape[1])
    g = R._gen(1300 + E + N + seed)
    ok = torch.arange(N)[torch.arange(N) % 7 != 3]
    dst = ok[torch.randint(0, ok.numel(), (E - E0,), generator=g)]
    src = torch.randint(0, N, (E - E0,), generator=g)
    return torch.cat([base, torch.stack([src, dst])], 1).contiguous()


# ================================================================================================ the tape
class Tape:
    """what a restatement did, for the scales: Linear (x, W, z, alpha, which leaf / columns the weight and bias are), LayerNorm and
    affine steps.  *key arguments name the entry of run()'s inputs a gradient belongs to."""

    def __init__(self):
        self.lin, self.ln, self.aff = [], [], []

    def linear(self, x, W, b=None, alpha=1.0, wkey=None, cols=None, bkey=None, xkey=None, dz_exact=False):
        """xkey: x is the input of that name (an exact factor of dW); dz_exact: the gradient of z is a cotangent, or one under an exact mask"""
        z = F.linear(x, W)
        if alpha != 1.0:
            z = alpha * z
        if b is not None:
            z = z + b
        self.lin.append(dict(x=x, W=W, b=b, z=z, alpha=float(alpha), wkey=wkey, cols=cols, bkey=bkey, xkey=xkey, dz_exact=dz_exact))
        return z

    def normalise(self, v, eps=EPS):
        mean = v.mean(1, keepdim=True)
        d = v - mean
        return d / ((d * d).mean(1, keepdim=True) + eps).sqrt()

    def layer_norm(self, v, gamma, beta, eps=EPS, gkey=None, bkey=None):
        xhat = self.normalise(v, eps)
        y = xhat * gamma + beta
        self.ln.append(dict(v=v, xhat=xhat, y=y, gamma=gamma, gkey=gkey, bkey=bkey))
        return y

    def affine(self, S, deg, gamma, beta, gkey=None, bkey=None, s_scale=None):
        """sum_e (gamma xhat_e + beta) = gamma S + deg beta: the LayerNorm's affine part on the per-node sums; s_scale [N]: the scale of
        a row of S, max_j sum_e |xhat_ej|"""
        y = S * gamma + deg.to(S.dtype)[:, None] * beta
        self.aff.append(dict(S=S, deg=deg, y=y, gkey=gkey, bkey=bkey, s_scale=s_scale))
        return y

    def tensors(self):
        return [r["z"] for r in self.lin] + [r["y"] for r in self.ln] + [r["v"] for r in self.ln] + [r["y"] for r in self.aff]

    def take(self, grads):
        """the gradients of tensors(), in that order (None: that step is not on the way to the loss -- zeros)"""
        grads = list(grads)
        for rs, of, key in ((self.lin, "z", "dz"), (self.ln, "y", "dy"), (self.ln, "v", "dv"), (self.aff, "y", "dy")):
            for r in rs:
                g = grads.pop(0)
                r[key] = torch.zeros_like(r[of]) if g is None else g.detach()

    def scales(self, shapes):
        """{key: scale} for the keys of `shapes` ({key: shape of the leaf}): element-wise for 2-d weights and vectors recorded as wkey /
        bkey / gkey, per ROW for the leaves recorded as xkey"""
        out = {}

        def acc(key, val, shape, cols=None):
            if key is None or key not in shapes:
                return
            if key not in out:
                out[key] = torch.zeros(shape, dtype=F64)
            if cols is None:
                out[key] += val
            else:
                out[key][:, cols[0]:cols[1]] += val
        for r in self.lin:
            dz, x, W = r["dz"].double().abs(), r["x"].detach().double().abs(), r["W"].detach().double().abs()
            a = abs(r["alpha"])
            if r["wkey"] in shapes:
                x_exact = r["xkey"] is not None
                if x_exact and r["dz_exact"]:
                    val = dz.t() @ x                                        # sum_i |dz_ij| |x_ik|
                else:
                    val = (dz.amax(1, keepdim=True) * x).sum(0)[None, :].expand(dz.shape[1], -1)        # sum_i max_j' |dz_ij'| |x_ik|
                    if not x_exact:
                        val = val + (dz * x.amax(1, keepdim=True)).sum(0)[:, None]                    # + sum_i |dz_ij| max_k' |x_ik'|
                acc(r["wkey"], a * val, shapes[r["wkey"]], r["cols"])
            acc(r["bkey"], dz.sum(0), shapes.get(r["bkey"]))
            if r["xkey"] in shapes:
                acc(r["xkey"], a * (dz @ W).amax(1), (x.shape[0],))
        for r in self.ln:
            dy = r["dy"].double().abs()
            acc(r["gkey"], (dy * r["xhat"].detach().double().abs().amax(1, keepdim=True).clamp_min(1.0)).sum(0), shapes.get(r["gkey"]))
            acc(r["bkey"], dy.sum(0), shapes.get(r["bkey"]))
        for r in self.aff:
            dy = r["dy"].double().abs()
            s_row = r["S"].detach().double().abs().amax(1) if r["s_scale"] is None else r["s_scale"].double()
            acc(r["gkey"], (dy * s_row[:, None]).sum(0), shapes.get(r["gkey"]))
            acc(r["bkey"], (dy * r["deg"].double()[:, None]).sum(0), shapes.get(r["bkey"]))
        return out


def out_scale_full(rec):
    """[M][out] float64: sum_k |alpha x_ik w_jk| + |bias_j| of a recorded Linear, per unit"""
    s = abs(rec["alpha"]) * (rec["x"].detach().double().abs() @ rec["W"].detach().double().abs().t())
    return s if rec["b"] is None else s + rec["b"].detach().double().abs()


def out_scale(rec):
    """[M] float64: the largest of a row's units"""
    return out_scale_full(rec).amax(1)


class Run:
    pass


def run(fn, inputs, cots, dtype, wrt=None):
    """fn(tape, v) -> {name: tensor}, v = the float tensors of `inputs` as leaves of `dtype` (everything else passed through).
    Loss = sum over the cotangents that are not None of (output * cotangent).sum().  Returns a Run with .out (detached outputs),
    .grad ({key: gradient or None} for the float inputs, or for `wrt`), .tape (with dz / dy of every recorded step)."""
    t = Tape()
    v = {k: (a.detach().to(dtype).clone().requires_grad_() if torch.is_tensor(a) and a.is_floating_point() else a) for k, a in inputs.items()}
    out = fn(t, v)
    keys = [k for k, a in v.items() if torch.is_tensor(a) and a.is_floating_point()] if wrt is None else list(wrt)
    r = Run()
    r.out = {k: a.detach() for k, a in out.items()}
    r.tape, r.grad = t, {k: None for k in keys}
    terms = [(out[k] * c.to(dtype)).sum() for k, c in cots.items() if c is not None]
    if terms:
        targets = [v[k] for k in keys] + t.tensors()
        grads = torch.autograd.grad(sum(terms), targets, allow_unused=True)
        r.grad = {k: (None if g is None else g.detach()) for k, g in zip(keys, grads[:len(keys)])}
        t.take(grads[len(keys):])
    return r


# ================================================================================================ the nodes
def relu(z):
    return z * (z > 0).to(z.dtype)


def segment_sum(msg, keys, N):
    out = torch.zeros(N, msg.shape[1], dtype=msg.dtype)
    return out.index_add(0, keys, msg) if msg.shape[0] else out


def edge_combine(t, v):
    """EdgeCombine: v = xa, xb, ec, ei, relu -> z (the pre-activation), out"""
    ei = v["ei"]
    z = v["xa"].index_select(0, ei[1]) + v["xb"].index_select(0, ei[0]) + v["ec"]
    return dict(z=z, out=relu(z) if v["relu"] else z)


def segment_sum_node(t, v):
    """SegmentSum: v = msg, ei, N"""
    return dict(agg=segment_sum(v["msg"], v["ei"][1], v["N"]))


def layer_norm128(t, v):
    """LayerNorm128: v = x, gamma, beta"""
    return dict(y=t.layer_norm(v["x"], v["gamma"], v["beta"], EPS, "gamma", "beta"))


def splitk_linear(t, v):
    """SplitKLinear: v = x, W, b (or None), relu -> z, y"""
    z = t.linear(v["x"], v["W"], v.get("b"), wkey="W", bkey="b", xkey="x", dz_exact=True)
    return dict(z=z, y=relu(z) if v["relu"] else z)


def edge_latent_linear(t, v):
    """EdgeLatentLinear: v = e, Wfull [128][384] (the e block = columns 256..), scale -> ec, e_next"""
    ec = t.linear(v["e"], v["Wfull"][:, 256:], None, v["scale"], wkey="Wfull", cols=(256, 384), xkey="e", dz_exact=True)
    return dict(ec=ec, e_next=v["e"] * 1.0)


def edge_first_layer(t, v):
    """EdgeFirstLayer: v = e, Wfull, scale, xa, xb, ei -> z (pre-activation: what the node's backward takes the gradient OF), a0, e_next"""
    ei = v["ei"]
    ec = t.linear(v["e"], v["Wfull"][:, 256:], None, v["scale"], wkey="Wfull", cols=(256, 384), xkey="e", dz_exact=True)
    z = ec + v["xa"].index_select(0, ei[1]) + v["xb"].index_select(0, ei[0])
    return dict(z=z, a0=relu(z), e_next=v["e"] * 1.0)


def tail_layers(t, h, v, k, prefix="", a0_key=None):
    """Linear_1 .. Linear_k behind the first edge Linear (ReLU between them, none behind the last): the input of the normalisation.
    a0_key: h is the input of that name (or its ReLU), not something computed"""
    for i in range(1, k + 1):
        h = t.linear(h, v[f"{prefix}W{i}"], v[f"{prefix}b{i}"], wkey=f"{prefix}W{i}", bkey=f"{prefix}b{i}", xkey=a0_key if i == 1 else None)
        if i < k:
            h = relu(h)
    return h


def edge_tail_aggregate(t, v, prefix=""):
    """EdgeTailAggregate + the caller's affine part: v = a0, a0_relu, ei, N, k, W1, b1, ..., gamma, beta -> S, agg"""
    a0 = relu(v[prefix + "a0"]) if v["a0_relu"] else v[prefix + "a0"]
    xhat = t.normalise(tail_layers(t, a0, v, v["k"], prefix, prefix + "a0"))
    S = segment_sum(xhat, v["ei"][1], v["N"])
    deg = torch.bincount(v["ei"][1], minlength=v["N"])
    return dict(xhat=xhat, S=S, agg=t.affine(S, deg, v[prefix + "gamma"], v[prefix + "beta"], prefix + "gamma", prefix + "beta",
                                            segment_sum(xhat.detach().abs(), v["ei"][1], v["N"]).amax(1)))


def mlp_ln_sum(t, v):
    """the same as the reference network states it: LayerNorm(MLP(a0)) summed per destination"""
    a0 = relu(v["a0"]) if v["a0_relu"] else v["a0"]
    msg = t.layer_norm(tail_layers(t, a0, v, v["k"], "", "a0"), v["gamma"], v["beta"], EPS, "gamma", "beta")
    return dict(agg=segment_sum(msg, v["ei"][1], v["N"]))


def chain(t, v):
    """three message paths sharing one e: layer l = first edge Linear at scale v['scales'][l] on its own xa / xb, then the tail and the sum
    -> agg0, agg1, agg2, e_next.  v['affine_on_sums'] (default): the LayerNorm's affine part on the per-node sums, as EdgeTailAggregate's
    caller applies it; False: per edge, before the sum, as the per-layer nodes do -- one function, two orders of rounding"""
    out = {}
    for l, s in enumerate(v["scales"]):
        p = f"l{l}."
        ei = v["ei"]
        ec = t.linear(v["e"], v[p + "Wfull"][:, 256:], None, s, wkey=p + "Wfull", cols=(256, 384), xkey="e")
        z = ec + v[p + "xa"].index_select(0, ei[1]) + v[p + "xb"].index_select(0, ei[0])
        h = tail_layers(t, relu(z), v, v["k"], p)
        out[f"z{l}"], out[f"xhat{l}"] = z, t.normalise(h)
        if v.get("affine_on_sums", True):
            S = segment_sum(out[f"xhat{l}"], ei[1], v["N"])
            out[f"agg{l}"] = t.affine(S, torch.bincount(ei[1], minlength=v["N"]), v[p + "gamma"], v[p + "beta"], p + "gamma", p + "beta",
                                      segment_sum(out[f"xhat{l}"].detach().abs(), ei[1], v["N"]).amax(1))
        else:
            out[f"agg{l}"] = segment_sum(t.layer_norm(h, v[p + "gamma"], v[p + "beta"], EPS, p + "gamma", p + "beta"), ei[1], v["N"])
    out["e_next"] = v["e"] * 1.0
    return out


def mlp_names(prefix, nlin):
    return [(f"{prefix}.0.NN-{i}.weight", f"{prefix}.0.NN-{i}.bias") for i in range(nlin)]


def interaction_layer(t, v):
    """InteractionNetwork.message_update on state_dict-named parameters: v = x, e, ei, scale, nlin + the parameters -> x_new, e_next.
    The first Linear of either MLP is applied as column blocks, like the module does (and like cat[...] @ W^T is, exactly, in real
    arithmetic)."""
    x, e, ei, N, nlin = v["x"], v["e"], v["ei"], v["x"].shape[0], v["nlin"]
    n = x.shape[1]
    (w0, b0), *rest = mlp_names("edge_fn", nlin)
    xa = t.linear(x, v[w0][:, :n], v[b0], wkey=w0, cols=(0, n), bkey=b0, xkey="x")
    xb = t.linear(x, v[w0][:, n:2 * n], None, wkey=w0, cols=(n, 2 * n), xkey="x")
    ec = t.linear(e, v[w0][:, 2 * n:], None, v["scale"], wkey=w0, cols=(2 * n, v[w0].shape[1]), xkey="e")
    z0 = ec + xa.index_select(0, ei[1]) + xb.index_select(0, ei[0])
    h, pre = relu(z0), [z0]
    for i, (w, b) in enumerate(rest):
        h = t.linear(h, v[w], v[b], wkey=w, bkey=b)
        if i < len(rest) - 1:
            pre.append(h)
            h = relu(h)
    msg = t.layer_norm(h, v["edge_fn.1.weight"], v["edge_fn.1.bias"], EPS, "edge_fn.1.weight", "edge_fn.1.bias")
    agg = segment_sum(msg, ei[1], N)
    (w0, b0), *rest = mlp_names("node_fn", nlin)
    a = agg.shape[1]
    zn = t.linear(agg, v[w0][:, :a], v[b0], wkey=w0, cols=(0, a), bkey=b0) + t.linear(x, v[w0][:, a:], None, wkey=w0, cols=(a, v[w0].shape[1]), xkey="x")
    hn, npre = relu(zn), [zn]
    for i, (w, b) in enumerate(rest):
        hn = t.linear(hn, v[w], v[b], wkey=w, bkey=b)
        if i < len(rest) - 1:
            npre.append(hn)
            hn = relu(hn)
    y = t.layer_norm(hn, v["node_fn.1.weight"], v["node_fn.1.bias"], EPS, "node_fn.1.weight", "node_fn.1.bias")
    out = dict(x_new=y + x, e_next=e * 1.0)
    out.update({f"edge_pre{i}": p for i, p in enumerate(pre)})
    out.update({f"node_pre{i}": p for i, p in enumerate(npre)})
    return out


# ================================================================================================ inputs without ReLU ties
def draw_without_ties(E, draw, preacts, seed, rounds=ROUNDS):
    """rows [E][.] = draw(E, generator) such that no ReLU'd pre-activation of any row lies within MARGIN * s of zero, s = the sum of the
    magnitudes of its terms, both evaluated in float64: preacts(rows, ids) yields (z, s) pairs for the given rows (ids = their row
    numbers).  Rows that hold such a unit are drawn again, at most `rounds` times; the MLPs are row-wise and everything gathered stays
    fixed, so a redraw touches that row only.  Returns (rows, [number of rows drawn again per round])."""
    g = R._gen(seed)
    rows = draw(E, g)
    bad, hist = torch.arange(E), []
    for r in range(rounds + 1):
        tie = torch.zeros(bad.numel(), dtype=torch.bool)
        for z, s in preacts(rows[bad], bad):
            tie |= (z.abs() < MARGIN * s).any(1)
        bad = bad[tie]
        if bad.numel() == 0 or r == rounds:
            break
        hist.append(int(bad.numel()))
        rows[bad] = draw(bad.numel(), g)
    assert bad.numel() == 0, f"{bad.numel()} rows still hold a ReLU tie after {rounds} rounds"
    return rows, hist


def randn_rows(n, g):
    return torch.randn(n, 128, generator=g)


def relu_rows(n, g):
    """rows that are themselves the output of a ReLU: about half the entries exactly 0"""
    return torch.relu(torch.randn(n, 128, generator=g))


def linear_preacts(W, b=None, alpha=1.0, gathered=None):
    """(z, s) of alpha x W^T + b + gathered[ids] (gathered = (value rows, magnitude rows) per row id)"""
    W64 = W.double()
    Wabs = W64.abs()

    def f(rows, ids):
        x = rows.double()
        z, s = alpha * (x @ W64.t()), abs(alpha) * (x.abs() @ Wabs.t())
        if b is not None:
            z, s = z + b.double(), s + b.double().abs()
        if gathered is not None:
            z, s = z + gathered[0][ids], s + gathered[1][ids]
        return z, s
    return f


def gathered_rows(xa, xb, ei):
    """(xa[dst] + xb[src], |xa[dst]| + |xb[src]|) in float64, per edge"""
    a, b = xa.double()[ei[1]], xb.double()[ei[0]]
    return a + b, a.abs() + b.abs()


def mlp_preacts(first, hidden, first_relu=True):
    """preacts() of a row-wise MLP: `first` = linear_preacts of the first layer (None: the rows are activations already, ReLU'd when
    first_relu), hidden = [(W, b)] of the ReLU'd layers behind it"""
    def f(rows, ids):
        if first is not None:
            z, s = first(rows, ids)
            yield z, s
            h = torch.relu(z)
        else:
            h = torch.relu(rows.double()) if first_relu else rows.double()
        for W, b in hidden:
            z, s = linear_preacts(W, b)(h, ids)
            yield z, s
            h = torch.relu(z)
    return f


# ------------------------------------------------------------------------------------------------ parameter draws
def weight(g, out=128, inp=128):
    """O(1 / sqrt(inp)) entries: every layer keeps O(1) rows"""
    return torch.randn(out, inp, generator=g) / inp ** 0.5


def tail_params(k, seed, prefix=""):
    g = R._gen(1500 + seed)
    p = {}
    for i in range(1, k + 1):
        p[f"{prefix}W{i}"], p[f"{prefix}b{i}"] = weight(g), 0.5 * torch.randn(128, generator=g)
    p[prefix + "gamma"], p[prefix + "beta"] = 1.0 + 0.3 * torch.randn(128, generator=g), torch.randn(128, generator=g)
    return p


def tail_hidden(p, k, prefix=""):
    return [(p[f"{prefix}W{i}"], p[f"{prefix}b{i}"]) for i in range(1, k)]


def combine_case(E, kind, relu, seed=0):
    """inputs of EdgeCombine: ec without ties in relu(xa[dst] + xb[src] + ec)"""
    N = nodes_for(E)
    ei = graph(E, N, kind, seed)
    g = R._gen(1400 + E + seed)
    xa, xb = torch.randn(N, 128, generator=g), torch.randn(N, 128, generator=g)
    ga, gs = gathered_rows(xa, xb, ei)
    ec, hist = draw_without_ties(E, randn_rows, lambda rows, ids: [(rows.double() + ga[ids], rows.double().abs() + gs[ids])], 1450 + E + seed)
    return dict(xa=xa, xb=xb, ec=ec, ei=ei, N=N, relu=relu), hist


def splitk_case(M, K=128, O=128, relu=True, bias=True, seed=0):
    """inputs of SplitKLinear [M][K] -> [M][O]: x without ties in relu(x W^T + b)"""
    g = R._gen(1480 + M + K + O + seed)
    W, b = weight(g, O, K), (0.5 * torch.randn(O, generator=g) if bias else None)
    draw = lambda n, gen: torch.randn(n, K, generator=gen)  # noqa: E731
    x, hist = draw_without_ties(M, draw, mlp_preacts(linear_preacts(W, b), []) if relu else (lambda rows, ids: []), 1490 + M + K + seed)
    v = dict(x=x, W=W, relu=relu)
    if bias:
        v["b"] = b
    return v, hist


def first_layer_case(E, kind, scale, seed=0):
    """inputs of EdgeLatentLinear / EdgeFirstLayer: e without ties in relu(scale e We^T + xa[dst] + xb[src])"""
    N = nodes_for(E)
    ei = graph(E, N, kind, seed)
    g = R._gen(1600 + E + seed)
    Wfull = torch.cat([torch.full((128, 256), 77.0), weight(g)], 1)
    xa, xb = torch.randn(N, 128, generator=g), torch.randn(N, 128, generator=g)
    e, hist = draw_without_ties(E, randn_rows, mlp_preacts(linear_preacts(Wfull[:, 256:], None, scale, gathered_rows(xa, xb, ei)), []), 1700 + E + seed)
    return dict(e=e, Wfull=Wfull, scale=scale, xa=xa, xb=xb, ei=ei, N=N), hist


def tail_case(E, k, a0_relu, kind="hub", seed=0):
    """inputs of EdgeTailAggregate: a0 without ties in its hidden layers"""
    N = nodes_for(E)
    ei = graph(E, N, kind, seed)
    p = tail_params(k, seed)
    a0, hist = draw_without_ties(E, relu_rows if a0_relu else randn_rows, mlp_preacts(None, tail_hidden(p, k), a0_relu), 1800 + E + k + seed)
    return dict(a0=a0, a0_relu=a0_relu, ei=ei, N=N, k=k, **p), hist


def chain_case(E, scales, k=2, kind="hub", seed=0):
    """inputs of chain(): one e without ties in any of the three layers' first and hidden pre-activations"""
    N = nodes_for(E)
    ei = graph(E, N, kind, seed)
    g = R._gen(1900 + E + seed)
    v = dict(ei=ei, N=N, k=k, scales=tuple(scales))
    pre = []
    for l, s in enumerate(scales):
        p = f"l{l}."
        v[p + "Wfull"] = torch.cat([torch.zeros(128, 256), weight(g)], 1)
        v[p + "xa"], v[p + "xb"] = torch.randn(N, 128, generator=g), torch.randn(N, 128, generator=g)
        v.update(tail_params(k, seed + 10 * (l + 1), p))
        pre.append(mlp_preacts(linear_preacts(v[p + "Wfull"][:, 256:], None, s, gathered_rows(v[p + "xa"], v[p + "xb"], ei)), tail_hidden(v, k, p)))

    def all_layers(rows, ids):
        for f in pre:
            yield from f(rows, ids)
    v["e"], hist = draw_without_ties(E, randn_rows, all_layers, 2000 + E + seed)
    return v, hist


def layer_params(nlin, seed):
    """state_dict-named parameters of one InteractionNetwork(128, 128, 128, 128, nlin - 1, 128)"""
    g = R._gen(2100 + seed)
    p = {}
    for prefix, k0 in (("edge_fn", 384), ("node_fn", 256)):
        for i, (w, b) in enumerate(mlp_names(prefix, nlin)):
            p[w], p[b] = weight(g, 128, k0 if i == 0 else 128), 0.5 * torch.randn(128, generator=g)
        p[prefix + ".1.weight"], p[prefix + ".1.bias"] = 1.0 + 0.3 * torch.randn(128, generator=g), torch.randn(128, generator=g)
    return p


LAYER_ROUNDS = 24


def layer_case(N, ei, scale, nlin=3, seed=0):
    """inputs of interaction_layer() without ties in ANY ReLU, the node MLP's included.  A node's pre-activations depend on every edge
    that arrives at it, so no redraw is local: every round evaluates the whole layer in float64 and draws again the rows of e whose edge
    MLP holds a tie and the rows of x whose node MLP does; a redrawn x row disturbs its few neighbours only, so the number of ties falls
    geometrically on a sparse graph (LAYER_ROUNDS rounds at most, then an assertion)."""
    E = int(ei.shape[1])
    g = R._gen(2200 + E + seed)
    p = layer_params(nlin, seed)
    x, e = torch.randn(N, 128, generator=g), torch.randn(E, 128, generator=g)
    v = dict(x=x, e=e, ei=ei, scale=scale, nlin=nlin, **p)
    hist = []
    for r in range(LAYER_ROUNDS + 1):
        t = Tape()
        with torch.no_grad():
            out = interaction_layer(t, {k: (a.double() if torch.is_tensor(a) and a.is_floating_point() else a) for k, a in v.items()})
        recs = t.lin
        # the ReLU'd Linear records: edge level = record 2 (the e block; its z lacks the gathered rows) and the hidden ones; node level likewise
        s_first = out_scale_full(recs[2]) + (out_scale_full(recs[0]).index_select(0, ei[1]) + out_scale_full(recs[1]).index_select(0, ei[0]))
        bad_e = (out["edge_pre0"].abs() < MARGIN * s_first).any(1)
        for i in range(1, nlin - 1):
            bad_e |= (out[f"edge_pre{i}"].abs() < MARGIN * out_scale_full(recs[2 + i])).any(1)
        nrec = recs[nlin + 2:]           # behind the three blocks of the first edge Linear and the nlin - 1 layers after it: the node MLP's
        s_first = out_scale_full(nrec[0]) + out_scale_full(nrec[1])
        bad_x = (out["node_pre0"].abs() < MARGIN * s_first).any(1)
        for i in range(1, nlin - 1):
            bad_x |= (out[f"node_pre{i}"].abs() < MARGIN * out_scale_full(nrec[1 + i])).any(1)
        ne, nx = int(bad_e.sum()), int(bad_x.sum())
        if ne + nx == 0 or r == LAYER_ROUNDS:
            break
        hist.append((ne, nx))
        e[bad_e] = torch.randn(ne, 128, generator=g)
        x[bad_x] = torch.randn(nx, 128, generator=g)
    assert ne + nx == 0, f"{ne} edge rows and {nx} node rows still hold a ReLU tie after {LAYER_ROUNDS} rounds"
    return v, hist

