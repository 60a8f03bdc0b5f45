"""The autograd nodes of meshnet/graph_ops.py that a config-4 train step runs -- EdgeCombine, SegmentSum, LayerNorm128, SplitKLinear,
EdgeLatentLinear, EdgeFirstLayer, EdgeTailAggregate -- each called through .apply on its own, and the dispatchers that choose between
them (linear_rows, edge_tail_aggregate, InteractionNetwork.message_update, GraphCSR.get), against the float64 restatement
tests/gnn_autograd_ref.py with torch's own autograd behind it: every forward output and every returned gradient, at the sizes where a
node or the kernels under it take another path (tests/test_gnn_autograd_nodes_cpu.py states which constant every size crosses), on
the graphs of tests/gnn_kernels_ref.py (a hub of 3000 edges, nodes without edges, duplicates, self loops), at the scales 1, 2 and 2^14
of the first, second and last processor layer, with every needs_input_grad subset and every (g, g_next) combination of the chained
edge-latent gradient.

What a whole-network comparison cannot see and these do: the PRE-ACTIVATION gradient contract (EdgeFirstLayer.backward and
EdgeCombine(grad_premasked=True) take the gradient of z, EdgeTailAggregate(a0_relu=True) applies the mask -- the restatement
differentiates z for the former and relu(a0) for the latter, so masking twice or not at all fails on exactly the rows where it
matters); `scale` once in de and once in dW; the three sources of EdgeTailAggregate's bias gradients; k = 1; the column slice
W[:, 256:] whose gradient must land in W.grad[:, 256:] and nowhere else; gradient 0 at z = 0 in every element.

Inputs hold NO ReLU TIES (gnn_autograd_ref.draw_without_ties: every ReLU'd pre-activation is at least 2^-14 of the sum of its terms'
magnitudes away from zero in float64, rows that are not are drawn again), so a mask is the same in float32 and float64 and is compared
for equality; nothing is excluded from any comparison.

Bars, by the rule of tests/test_gnn_kernels_gpu.py: e32 = the restatement's own float32-on-the-CPU error against float64 on the same
inputs; the largest row (or column) error of a comparison must stay within 8 x the largest e32 of that comparison, floor 1e-6; a bar
above 1e-3 means ill-conditioned inputs and fails by itself.  Row and column scales (gnn_autograd_ref.Tape.scales):
  a Linear's output or input gradient   max_j sum_k |alpha g_ik w_kj| plus the magnitudes of the addends (gathered rows, g_next, a residual)
  column sums (db, dbeta)               per column, sum_i |term_ij|
  dW of SplitKLinear, EdgeFirstLayer, EdgeLatentLinear      per element, sum_i |dz_ij| |x_ik|: both factors are inputs (or a cotangent
                                        under an exact mask); an element whose scale is 0 must be exactly 0
  dW where a factor is COMPUTED         (EdgeTailAggregate, chain, message_update: dz is back-propagated, x behind the first layer an
                                        activation) the computed factor counts with its row's largest entry, the scale its own error is
                                        relative to; an input still counts with its own value (gnn_autograd_ref.py's header gives the
                                        formulas and what |dz_ij| |x_ik| alone does there: the float32 restatement itself is 4.5e-4 off)
  dgamma                                per column, sum_i |dy_ij| max(max_j |xhat_ij|, 1)
  per-node sums (S, agg, dxa, dxb)      per node, max_j sum_e |row_ej|
  anything behind a LayerNorm           max(max_j |r64_ij|, 1);  LayerNorm dx: rstd_i max_j |g_ij gamma_j|
Masks, masked zeros, copies (e_next, the gradient that is g_next alone, SegmentSum's backward), the zero columns of a sliced weight's
gradient and the rows of nodes without edges are compared for EQUALITY.

check_rows() prints e32, the bar and the node's error; the module's teardown prints the table of the largest of each per group
(pytest -rP shows it).

What that table showed on an MI355X when this file was written (group | comparisons | largest e32 | largest bar | largest error |
smallest bar / error; "chain": three layers sharing one e through the fused / the per-layer nodes; "message_update": one
InteractionNetwork layer at BIG_ROWS edges (fused) and at BIG_ROWS - 1 (layers), its 16 parameter gradients grouped by kind):
  EdgeCombine dxa              |  80 | 1.62e-07 | 1.29e-06 | 5.91e-08 |  17.0
  EdgeCombine dxb              |  80 | 1.55e-07 | 1.24e-06 | 5.86e-08 |  17.2
  EdgeCombine out              |  80 | 1.02e-07 | 1.00e-06 | 1.02e-07 |   9.8
  EdgeFirstLayer dW            |  99 | 2.55e-07 | 2.04e-06 | 1.23e-07 |  16.1
  EdgeFirstLayer de            |  99 | 3.51e-07 | 2.81e-06 | 3.68e-07 |   6.1
  EdgeFirstLayer dxa           | 165 | 2.11e-07 | 1.69e-06 | 5.92e-08 |  16.9
  EdgeFirstLayer dxb           | 165 | 1.85e-07 | 1.48e-06 | 5.90e-08 |  16.9
  EdgeFirstLayer out           | 165 | 5.01e-07 | 4.01e-06 | 2.37e-07 |   5.6
  EdgeLatentLinear dW          |  99 | 2.55e-07 | 2.04e-06 | 1.23e-07 |  16.1
  EdgeLatentLinear de          |  99 | 3.51e-07 | 2.81e-06 | 3.68e-07 |   6.1
  EdgeLatentLinear out         | 132 | 4.95e-07 | 3.96e-06 | 2.86e-07 |   5.5
  EdgeTailAggregate S          |  36 | 1.34e-06 | 1.07e-05 | 5.44e-07 |  10.9
  EdgeTailAggregate agg        |  36 | 9.91e-07 | 7.93e-06 | 2.94e-07 |   8.5
  EdgeTailAggregate dW1        |  36 | 2.47e-07 | 1.98e-06 | 1.43e-07 |  10.8
  EdgeTailAggregate dW2        |  24 | 1.48e-07 | 1.18e-06 | 4.56e-08 |  24.5
  EdgeTailAggregate dW3        |  12 | 1.09e-07 | 1.00e-06 | 6.02e-08 |  16.6
  EdgeTailAggregate da0        |  18 | 4.11e-07 | 3.29e-06 | 3.89e-07 |   6.1
  EdgeTailAggregate db1        |  36 | 1.05e-06 | 8.44e-06 | 1.68e-06 |   2.5
  EdgeTailAggregate db2        |  24 | 8.06e-07 | 6.45e-06 | 2.49e-06 |   2.1
  EdgeTailAggregate db3        |  12 | 2.71e-07 | 2.17e-06 | 5.31e-07 |   4.1
  EdgeTailAggregate dbeta      |  36 | 9.73e-08 | 1.00e-06 | 6.78e-08 |  14.7
  EdgeTailAggregate dgamma     |  36 | 4.59e-07 | 3.67e-06 | 8.08e-08 |  33.4
  LayerNorm128 dbeta           |   3 | 2.35e-08 | 1.00e-06 | 1.49e-08 |  67.3
  LayerNorm128 dgamma          |   3 | 2.51e-06 | 2.01e-05 | 2.51e-06 |   8.0
  LayerNorm128 dx              |  17 | 3.64e-05 | 2.91e-04 | 2.95e-05 |   4.0
  LayerNorm128 y               |  17 | 1.07e-04 | 8.54e-04 | 1.02e-04 |   7.2
  SegmentSum                   |  20 | 1.41e-06 | 1.13e-05 | 5.94e-08 |  16.8
  SplitKLinear 128 dW          | 120 | 1.18e-07 | 1.00e-06 | 2.57e-07 |   3.9
  SplitKLinear 128 db          |  20 | 2.54e-08 | 1.00e-06 | 4.21e-08 |  23.7
  SplitKLinear 128 dx          | 120 | 2.97e-07 | 2.37e-06 | 3.08e-07 |   7.3
  SplitKLinear 128 y           | 160 | 3.05e-07 | 2.44e-06 | 3.14e-07 |   6.7
  SplitKLinear generic dW      | 144 | 2.32e-07 | 1.86e-06 | 3.18e-07 |   3.1
  SplitKLinear generic db      |  24 | 1.31e-08 | 1.00e-06 | 1.46e-08 |  68.4
  SplitKLinear generic dx      | 144 | 2.90e-07 | 2.32e-06 | 2.75e-07 |   6.4
  SplitKLinear generic y       | 192 | 3.10e-07 | 2.48e-06 | 3.38e-07 |   6.9
  chain fused agg              |   6 | 1.07e-06 | 8.54e-06 | 3.66e-07 |  15.6
  chain fused dW first         |   6 | 8.94e-09 | 1.00e-06 | 4.69e-09 | 213.2
  chain fused dW1              |   6 | 5.26e-08 | 1.00e-06 | 2.04e-08 |  49.1
  chain fused dW2              |   6 | 8.12e-08 | 1.00e-06 | 1.90e-08 |  52.7
  chain fused db1              |   6 | 1.05e-07 | 1.00e-06 | 7.18e-08 |  13.9
  chain fused db2              |   6 | 1.20e-07 | 1.00e-06 | 7.29e-08 |  13.7
  chain fused dbeta            |   6 | 1.98e-07 | 1.58e-06 | 6.60e-08 |  15.9
  chain fused de               |   2 | 2.25e-07 | 1.80e-06 | 1.68e-07 |  10.7
  chain fused dgamma           |   6 | 4.36e-07 | 3.49e-06 | 4.64e-08 |  39.2
  chain fused dxa              |   6 | 1.54e-06 | 1.23e-05 | 7.24e-07 |  10.8
  chain fused dxb              |   6 | 5.64e-07 | 4.51e-06 | 5.71e-07 |   6.7
  chain layers agg             |   6 | 1.76e-06 | 1.41e-05 | 3.92e-07 |  17.7
  chain layers dW first        |   6 | 8.94e-09 | 1.00e-06 | 4.83e-09 | 207.0
  chain layers dW1             |   6 | 5.26e-08 | 1.00e-06 | 2.04e-08 |  49.1
  chain layers dW2             |   6 | 8.12e-08 | 1.00e-06 | 2.09e-08 |  47.8
  chain layers db1             |   6 | 1.05e-07 | 1.00e-06 | 8.29e-08 |  12.1
  chain layers db2             |   6 | 1.20e-07 | 1.00e-06 | 7.29e-08 |  13.7
  chain layers dbeta           |   6 | 1.71e-07 | 1.37e-06 | 5.30e-08 |  24.5
  chain layers de              |   2 | 2.25e-07 | 1.80e-06 | 1.72e-07 |  10.2
  chain layers dgamma          |   6 | 3.22e-08 | 1.00e-06 | 2.17e-08 |  46.2
  chain layers dxa             |   6 | 1.54e-06 | 1.23e-05 | 6.86e-07 |   9.9
  chain layers dxb             |   6 | 5.64e-07 | 4.51e-06 | 5.81e-07 |   7.1
  message_update fused dW      |   6 | 9.97e-09 | 1.00e-06 | 8.07e-09 | 123.9
  message_update fused db      |   6 | 3.58e-07 | 2.87e-06 | 2.10e-07 |  13.7
  message_update fused dbeta   |   2 | 1.32e-08 | 1.00e-06 | 1.20e-08 |  83.3
  message_update fused de      |   1 | 2.04e-07 | 1.63e-06 | 1.83e-07 |   8.9
  message_update fused dgamma  |   2 | 4.95e-09 | 1.00e-06 | 4.74e-09 | 211.0
  message_update fused dx      |   1 | 1.73e-07 | 1.38e-06 | 1.59e-07 |   8.7
  message_update fused x_new   |   1 | 4.65e-07 | 3.72e-06 | 5.14e-07 |   7.2
  message_update layers dW     |   6 | 8.77e-09 | 1.00e-06 | 7.20e-09 | 138.8
  message_update layers db     |   6 | 2.00e-07 | 1.60e-06 | 2.00e-07 |   8.0
  message_update layers dbeta  |   2 | 1.31e-08 | 1.00e-06 | 1.28e-08 |  78.0
  message_update layers de     |   1 | 1.86e-07 | 1.49e-06 | 2.11e-07 |   7.1
  message_update layers dgamma |   2 | 6.12e-09 | 1.00e-06 | 6.40e-09 | 156.2
  message_update layers dx     |   1 | 2.06e-07 | 1.65e-06 | 1.65e-07 |  10.0
  message_update layers x_new  |   1 | 4.84e-07 | 3.87e-06 | 5.06e-07 |   7.7
No bar is above 8.6e-4 (LayerNorm128's rows of mean 64, std 1/16; 2.9e-4 for their dx); every other bar is below 2.1e-5.  The closest
calls are EdgeTailAggregate's hidden-layer bias gradients (csplat_dw128_bias's column sums: 2.1 and 2.5 times inside their bar) and
db3 from csplat_ln128_bwd's dxsum (4.1), then SplitKLinear's dW on the per-element scale sum_i |dz_ij| |x_ik| (3.1 through the chunked
batched GEMM, 3.9 through csplat_dw128).  Every mask equals the float64 mask, every copy is a copy, and a repeated backward gives the
same bits.  Wall time 25 to 36 s for the 108 tests (tests/test_gnn_kernels_gpu.py's docstring: 30 s for its 66); the slowest,
test_edge_first_layer_and_edge_latent_linear[65537-hub-2.0] at 2.7 to 4.5 s, spends it in the float64 / float32 restatements on the CPU.

Two deviations from the sizes and caps the other cases use, both in the message_update cases and for one reason: a node's
pre-activations depend on every edge that arrives at it, so a draw without ties in the NODE MLP's ReLUs cannot redraw one row at a
time.  gnn_autograd_ref.layer_case evaluates the whole layer per round and redraws the tied rows of e AND of x; the number of ties
falls geometrically only on a sparse graph, so these cases run on LAYER_N = 16384 nodes instead of a NODE_N value (the node-level
Linear layers then take the kernels too), and the cap is LAYER_ROUNDS = 24 rounds instead of draw_without_ties' 8 (6 were needed).

One finding, fixed with this file: GraphCSR kept the caller's edge_index tensor itself (contiguous() of a contiguous tensor), so an
in-place edit between forward and backward changed the edge list under a CSR whose rowptr / perm described the old one --
test_graph_csr_cache_follows_the_tensor_its_version_and_the_node_count saw SegmentSum's backward gather the edited destination's
row -- and the cache entry held its own key alive, so no entry was ever dropped.  The CSR now owns a copy.
"""
import gc
import weakref

import pytest

torch = pytest.importorskip("torch")       # (before the restatements, which import it)

import util  # noqa: E402,F401
import gnn_kernels_ref as R  # noqa: E402
import gnn_autograd_ref as A  # noqa: E402

pytestmark = pytest.mark.gpu

K, FLOOR, BAR_MAX = 8.0, 1e-6, 1e-3
F64, F32 = torch.float64, torch.float32
EPS32 = 2.0 ** -23
TABLE = {}


@pytest.fixture(scope="module", autouse=True)
def _threads_and_table():
    old = torch.get_num_threads()
    torch.set_num_threads(min(16, old))
    yield
    torch.set_num_threads(old)
    print("\ngroup | comparisons | largest e32 | largest bar | largest error | smallest bar / error")
    for g in sorted(TABLE):
        n, e32, bar, err, margin = TABLE[g]
        print(f"{g} | {n} | {e32:.2e} | {bar:.2e} | {err:.2e} | {margin:.1f}")


def _t(x):
    return x.detach().cpu().to(F64)


def check_rows(group, what, got, r64, r32, scale):
    """got (the node), r64, r32 (the restatement in float64 / float32) as [rows][columns]; scale: one number per row (or one for all)"""
    assert got is not None, f"{group} {what}: no gradient came back"
    got, r64, r32 = _t(got), _t(r64), _t(r32)
    assert got.shape == r64.shape == r32.shape, (group, what, got.shape, r64.shape, r32.shape)
    got, r64, r32 = (a.reshape(a.shape[0], -1) if a.dim() > 1 else a.reshape(-1, 1) for a in (got, r64, r32))
    assert bool(torch.isfinite(r64).all()) and bool(torch.isfinite(got).all()), f"{group} {what}: non-finite values"
    scale = torch.broadcast_to(_t(torch.as_tensor(scale)).reshape(-1), (got.shape[0],)).clamp_min(1e-300)
    e32 = float(((r32 - r64).abs().amax(1) / scale).max())
    rows = (got - r64).abs().amax(1) / scale
    worst = int(rows.argmax())
    err = float(rows[worst])
    bar = max(K * e32, FLOOR)
    print(f"{group} | {what}: e32 {e32:.3e} bar {bar:.3e} node {err:.3e} (row {worst})")
    n, a, b, c, m = TABLE.get(group, (0, 0.0, 0.0, 0.0, float("inf")))
    TABLE[group] = (n + 1, max(a, e32), max(b, bar), max(c, err), min(m, bar / max(err, 1e-30)))
    assert bar <= BAR_MAX, f"{group} {what}: bar {bar:.3e} > {BAR_MAX}: the inputs are ill-conditioned"
    assert err <= bar, f"{group} {what}: row {worst}: error {err:.3e} > bar {bar:.3e} (float32 restatement: {e32:.3e})"


def check_classes(group, what, got, r64, r32, scale, names):
    k = len(names)
    scale = torch.broadcast_to(_t(scale).reshape(-1), (got.shape[0],))
    for c in range(min(k, got.shape[0])):
        check_rows(group, f"{what} [{names[c]}]", got[c::k], r64[c::k], r32[c::k], scale[c::k])


def check_columns(group, what, got, r64, r32, scale):
    """one comparison per tensor, every element (column sum) on its own scale"""
    assert got is not None, f"{group} {what}: no gradient came back"
    dead = _t(scale).reshape(-1) == 0
    assert not bool(_t(got).reshape(-1)[dead].any()), f"{group} {what}: an element without any term (a unit the ReLU switches off in every row) is not exactly 0"
    check_rows(group, what, _t(got).reshape(-1, 1), _t(r64).reshape(-1, 1), _t(r32).reshape(-1, 1), _t(scale).reshape(-1))


def same(a, b):
    """equal values (float32 values are exact in float64)"""
    return a is not None and a.shape == b.shape and torch.equal(a.detach().cpu().double(), b.detach().cpu().double())


def dev(t):
    return t.detach().clone().contiguous().cuda()


def leaf(t, requires_grad=True):
    return dev(t).requires_grad_(requires_grad)


def refs(fn, v, cots, wrt=None):
    return A.run(fn, v, cots, F64, wrt), A.run(fn, v, cots, F32, wrt)


def shapes(r, *keys):
    return {k: tuple(r.grad[k].shape) for k in keys if r.grad.get(k) is not None}


def randn(seed, *shape):
    return torch.randn(*shape, generator=R._gen(3000 + seed))


def csr_of(ei, N):
    from meshnet.graph_ops import GraphCSR
    return GraphCSR(ei.cuda(), N)


def node_names(t):
    """type names of every node of the autograd graph behind t"""
    names, stack, seen, keep = set(), [t.grad_fn], set(), []
    while stack:
        f = stack.pop()
        if f is None or id(f) in seen:
            continue
        keep.append(f)                       # (the wrappers of graph nodes are created on demand: hold them, or ids get recycled)
        seen.add(id(f))
        names.add(type(f).__name__)
        stack += [nf for nf, _ in f.next_functions]
    return names


def has(names, prefix):
    return any(n.startswith(prefix) for n in names)


class _Drop(torch.autograd.Function):
    """identity whose backward hands NO gradient on: the producer's backward runs with None for this output"""

    @staticmethod
    def forward(ctx, x):
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        return None


def degrees(ei, N):
    return torch.bincount(ei[1], minlength=N), torch.bincount(ei[0], minlength=N)


def node_sum_scale(rows, keys, N):
    return R.segment_abs_sum(rows, keys, N).amax(1)


# ================================================================================================ EdgeCombine
@pytest.mark.parametrize("kind", R.GRAPHS)
@pytest.mark.parametrize("E", A.NODE_E[:4])
def test_edge_combine(E, kind):
    """out, dxa, dxb per row / node; gm (the gradient of ec) is the cotangent masked by the float64 mask, bit for bit -- and the cotangent's
    own values where the consumer has masked already (grad_premasked) or there is no ReLU"""
    from meshnet.graph_ops import EdgeCombine
    g = randn(E, E, 128)
    for relu in (False, True):
        v, _ = A.combine_case(E, kind, relu)
        ei, N = v["ei"], v["N"]
        csr = csr_of(ei, N)
        din, dout = degrees(ei, N)
        by = {False: refs(A.edge_combine, v, dict(out=g)), True: refs(A.edge_combine, v, dict(z=g))}
        s_out = (v["xa"].double().abs()[ei[1]] + v["xb"].double().abs()[ei[0]] + v["ec"].double().abs()).amax(1)
        for premasked in (False, True):
            r64, r32 = by[premasked]
            where = f"E {E} {kind} relu {relu} premasked {premasked}"
            xa, xb, ec, gd = leaf(v["xa"]), leaf(v["xb"]), leaf(v["ec"]), dev(g)
            out = EdgeCombine.apply(xa, xb, ec, csr, relu, premasked)
            out.backward(gd)
            check_rows("EdgeCombine out", where, out, r64.out["out"], r32.out["out"], s_out)
            assert same(out > 0, r64.out["out"] > 0), where
            gm64 = r64.grad["ec"]
            assert same(ec.grad, gm64), f"{where}: gm is not the cotangent under the float64 mask"
            if premasked or not relu:
                assert same(ec.grad, g), where
            check_rows("EdgeCombine dxa", where, xa.grad, r64.grad["xa"], r32.grad["xa"], node_sum_scale(gm64, ei[1], N))
            check_rows("EdgeCombine dxb", where, xb.grad, r64.grad["xb"], r32.grad["xb"], node_sum_scale(gm64, ei[0], N))
            assert bool((xa.grad[(din == 0).cuda()] == 0).all()) and bool((xb.grad[(dout == 0).cuda()] == 0).all()), where


# ================================================================================================ SegmentSum
@pytest.mark.parametrize("kind", R.GRAPHS)
@pytest.mark.parametrize("E", (257, 16385))
def test_segment_sum(E, kind):
    """forward under the segment-sum rule of tests/test_gnn_kernels_gpu.py (per node, and element by element inside the bound of
    compensated summation); backward = g[dst], a copy"""
    from meshnet.graph_ops import SegmentSum
    N = A.nodes_for(E)
    ei = A.graph(E, N, kind)
    csr = csr_of(ei, N)
    g = randn(E + 1, N, 128)
    for mk in ("ordinary", "cancelling"):
        msg = R.messages(ei, 128, mk)
        r64, r32 = refs(A.segment_sum_node, dict(msg=msg, ei=ei, N=N), dict(agg=g))
        m = leaf(msg)
        agg = SegmentSum.apply(m, csr)
        agg.backward(dev(g))
        sabs = R.segment_abs_sum(msg, ei[1], N)
        check_rows("SegmentSum", f"E {E} {kind} {mk}", agg, r64.out["agg"], r32.out["agg"], sabs.amax(1))
        deg = torch.bincount(ei[1], minlength=N).double()[:, None]
        excess = (_t(agg) - r64.out["agg"]).abs() - (EPS32 * r64.out["agg"].abs() + deg * EPS32 ** 2 * sabs)
        assert float(excess.max()) <= 0.0, f"E {E} {kind} {mk}: {float(excess.max()):.3e} beyond eps |sum| + n eps^2 sum |x|"
        assert same(m.grad, g[ei[1]]) and same(m.grad, r64.grad["msg"])
        assert bool((agg[(deg[:, 0] == 0).cuda()] == 0).all())


# ================================================================================================ LayerNorm128
@pytest.mark.parametrize("M", A.LN_M)
def test_layer_norm128(M):
    """y and dx per row class of gnn_kernels_ref.LN_CLASSES, dgamma / dbeta per column"""
    from meshnet.graph_ops import LayerNorm128
    x = R.ln_rows(M)
    _, _, gamma, beta = R.linear_params(M)
    g = randn(M, M, 128)
    r64, r32 = refs(A.layer_norm128, dict(x=x, gamma=gamma, beta=beta), dict(y=g))
    xd, gad, bed = leaf(x), leaf(gamma), leaf(beta)
    y = LayerNorm128.apply(xd, gad, bed, R.EPS)
    y.backward(dev(g))
    check_classes("LayerNorm128 y", f"M {M}", y, r64.out["y"], r32.out["y"], r64.out["y"].abs().amax(1).clamp_min(1.0), R.LN_CLASSES)
    v64 = x.double()
    rstd = 1.0 / ((v64 - v64.mean(1, keepdim=True)).pow(2).mean(1) + R.EPS).sqrt()
    check_classes("LayerNorm128 dx", f"M {M}", xd.grad, r64.grad["x"], r32.grad["x"], rstd * (g.double() * gamma.double()).abs().amax(1), R.LN_CLASSES)
    sc = r64.tape.scales(shapes(r64, "gamma", "beta"))
    check_columns("LayerNorm128 dgamma", f"M {M}", gad.grad, r64.grad["gamma"], r32.grad["gamma"], sc["gamma"])
    check_columns("LayerNorm128 dbeta", f"M {M}", bed.grad, r64.grad["beta"], r32.grad["beta"], sc["beta"])


# ================================================================================================ SplitKLinear
NIG = {"all": (True, True, True), "x only": (True, False, False), "weight only": (False, True, False), "bias frozen": (True, True, False)}


def _splitk(M, Kin, Out, dispatcher, odd_cotangent_at=None):
    from meshnet.graph_ops import SplitKLinear, linear_rows
    g = randn(M + Kin, M, Out)
    for relu in (False, True):
        for bias in (False, True):
            v, _ = A.splitk_case(M, Kin, Out, relu, bias)
            r64, r32 = refs(A.splitk_linear, v, dict(y=g))
            rec = r64.tape.lin[0]
            sc = r64.tape.scales(shapes(r64, "x", "W", "b"))
            for nig, (x_rg, w_rg, b_rg) in NIG.items():
                routes = ("apply", "linear_rows") if dispatcher else ("apply",)
                for route in routes:
                    where = f"M {M} {Kin}->{Out} relu {relu} bias {bias} grads {nig} via {route}"
                    x, W = leaf(v["x"], x_rg), leaf(v["W"], w_rg)
                    b = leaf(v["b"], b_rg) if bias else None
                    if route == "apply":
                        y = SplitKLinear.apply(x, W, b, relu)
                        assert has(node_names(y), "SplitKLinear")
                    else:
                        y = linear_rows(x, W, b, relu=relu)
                        meant = M >= SplitKLinear.BIG_ROWS or (M >= SplitKLinear.MIN_ROWS and w_rg)
                        assert has(node_names(y), "SplitKLinear") == meant, (where, sorted(node_names(y)))
                    gd = dev(g)
                    if odd_cotangent_at == (relu, bias, nig):
                        gd = gd.t().contiguous().t()
                        assert M == 1 or not gd.is_contiguous()
                    y.backward(gd)
                    grp = "SplitKLinear 128" if Kin == Out == 128 else "SplitKLinear generic"
                    check_rows(f"{grp} y", where, y, r64.out["y"], r32.out["y"], A.out_scale(rec))
                    if relu:
                        assert same(y > 0, r64.out["z"] > 0), f"{where}: the ReLU mask differs from float64's on tie-free inputs"
                    for key, t_, on in (("x", x, x_rg), ("W", W, w_rg), ("b", b, b_rg and bias)):
                        if t_ is None:
                            continue
                        if not on:
                            assert t_.grad is None, (where, key)
                        elif key == "x":
                            check_rows(f"{grp} dx", where, t_.grad, r64.grad[key], r32.grad[key], sc[key])
                        else:
                            check_columns(f"{grp} d{key}", where, t_.grad, r64.grad[key], r32.grad[key], sc[key])


@pytest.mark.parametrize("M", A.SPLITK_M)
def test_splitk_linear_128(M):
    """128 -> 128: kernels both ways from BIG_ROWS on, the library's GEMM with csplat_dw128 / csplat_relu_mask_bias128 below; through
    .apply and through linear_rows, which must pick the node from 512 rows on when the weight wants a gradient and from 16384 anyway"""
    _splitk(M, 128, 128, True, odd_cotangent_at=(True, True, "all"))


@pytest.mark.parametrize("Kin,Out", ((128, 64), (20, 128)))
@pytest.mark.parametrize("M", A.CHUNK_M)
def test_splitk_linear_generic_shapes(M, Kin, Out):
    """other widths: plain torch with the weight gradient as a chunked batched GEMM (C == 0, whole chunks only, chunks and a remainder).
    SplitKLinear reports no fallback of its own -- the callers that send a 128-wide network here do -- so STRICT asks for no mark"""
    _splitk(M, Kin, Out, False, odd_cotangent_at=(True, True, "all"))


# ================================================================================================ EdgeLatentLinear, EdgeFirstLayer
FIRST_CASES = [(E, "hub") for E in A.NODE_E] + [(257, kind) for kind in R.GRAPHS[1:]]


@pytest.mark.parametrize("scale", A.SCALES)
@pytest.mark.parametrize("E,kind", FIRST_CASES)
def test_edge_first_layer_and_edge_latent_linear(E, kind, scale):
    """the weight is the column slice W[:, 256:] of a [128, 384] parameter; (g, g_next) given / None by using one output only; e and the
    weight with and without requires_grad; a0 > 0 is the float64 mask; dxa / dxb are exactly 0 on nodes without edges"""
    from meshnet.graph_ops import EdgeFirstLayer, EdgeLatentLinear
    v, _ = A.first_layer_case(E, kind, scale)
    ei, N = v["ei"], v["N"]
    csr = csr_of(ei, N)
    din, dout = degrees(ei, N)
    g, gn = randn(E + 7, E, 128), randn(E + 8, E, 128)
    wrt = ("e", "Wfull", "xa", "xb")
    repeat = {}
    for node in ("EdgeFirstLayer", "EdgeLatentLinear"):
        first = node == "EdgeFirstLayer"
        fn, main = (A.edge_first_layer, "z") if first else (A.edge_latent_linear, "ec")
        for use_g, use_gn in ((True, True), (True, False), (False, True), (False, False)):
            if use_g:
                r64, r32 = refs(fn, v, {main: g, "e_next": gn if use_gn else None}, wrt if first else wrt[:2])
                rec = r64.tape.lin[0]
                sc = r64.tape.scales(shapes(r64, "e", "Wfull"))
                s_e = sc["e"] + (gn.double().abs().amax(1) if use_gn else 0.0)
                s_out = A.out_scale_full(rec)
                if first:
                    s_out = s_out + v["xa"].double().abs()[ei[1]] + v["xb"].double().abs()[ei[0]]
            for e_rg, w_rg in (((True, True), (False, True), (True, False), (False, False)) if use_g and use_gn else ((True, True),)):
                if not first and not (e_rg or w_rg):
                    continue
                where = f"{node} E {E} {kind} scale {scale} g {use_g} g_next {use_gn} e.rg {e_rg} W.rg {w_rg}"
                e, W, xa, xb = leaf(v["e"], e_rg), leaf(v["Wfull"], w_rg), leaf(v["xa"]), leaf(v["xb"])
                if first:
                    out, e_next = EdgeFirstLayer.apply(e, W[:, 256:], scale, xa, xb, csr)
                else:
                    out, e_next = EdgeLatentLinear.apply(e, W[:, 256:], scale)
                assert same(e_next, v["e"]), where
                loss = ((out * dev(g)).sum() if use_g else _Drop.apply(out).sum()) + ((e_next * dev(gn)).sum() if use_gn else 0.0)
                loss.backward()
                if use_g:
                    check_rows(f"{node} out", where, out, r64.out["a0" if first else "ec"], r32.out["a0" if first else "ec"], s_out.amax(1))
                    if first:
                        assert same(out > 0, r64.out["z"] > 0), f"{where}: a0 > 0 differs from the float64 mask on tie-free inputs"
                if not e_rg:
                    assert e.grad is None, where
                elif use_g:
                    check_rows(f"{node} de", where, e.grad, r64.grad["e"], r32.grad["e"], s_e)
                elif use_gn:
                    assert same(e.grad, gn), f"{where}: with g = None the gradient of e is g_next itself"
                else:
                    assert e.grad is None or not bool(e.grad.any()), where
                if not w_rg:
                    assert W.grad is None, where
                elif use_g:
                    check_columns(f"{node} dW", where, W.grad, r64.grad["Wfull"], r32.grad["Wfull"], sc["Wfull"])
                    if node in repeat:          # dW does not depend on g_next or on what else wants a gradient: bit for bit
                        assert same(W.grad, repeat[node]), f"{where}: dW differs from an earlier run's"
                    repeat[node] = W.grad.clone()
                    assert not bool(W.grad[:, :256].any()), f"{where}: the gradient of a column slice left its columns"
                else:
                    assert W.grad is None or not bool(W.grad.any()), where
                if first and use_g:
                    check_rows(f"{node} dxa", where, xa.grad, r64.grad["xa"], r32.grad["xa"], node_sum_scale(g, ei[1], N))
                    check_rows(f"{node} dxb", where, xb.grad, r64.grad["xb"], r32.grad["xb"], node_sum_scale(g, ei[0], N))
                    assert bool((xa.grad[(din == 0).cuda()] == 0).all()) and bool((xb.grad[(dout == 0).cuda()] == 0).all()), where
                elif first:
                    assert (xa.grad is None or not bool(xa.grad.any())) and (xb.grad is None or not bool(xb.grad.any())), where


# ================================================================================================ EdgeTailAggregate
def tail_module(v, k, prefix=""):
    """[build_mlp(384 -> 128 x k -> 128), LayerNorm(128)] on the GPU holding the case's tail parameters (its first Linear is not used)"""
    from meshnet.graph_network import build_mlp
    seq = torch.nn.Sequential(build_mlp(384, [128] * k, 128), torch.nn.LayerNorm(128)).cuda()
    with torch.no_grad():
        for i in range(1, k + 1):
            seq[0][2 * i].weight.copy_(v[f"{prefix}W{i}"])
            seq[0][2 * i].bias.copy_(v[f"{prefix}b{i}"])
        seq[1].weight.copy_(v[prefix + "gamma"])
        seq[1].bias.copy_(v[prefix + "beta"])
    return seq


def tail_grads(seq, k, prefix=""):
    out = {prefix + "gamma": seq[1].weight.grad, prefix + "beta": seq[1].bias.grad}
    for i in range(1, k + 1):
        out[f"{prefix}W{i}"], out[f"{prefix}b{i}"] = seq[0][2 * i].weight.grad, seq[0][2 * i].bias.grad
    return out


def check_tail_grads(group, where, got, r64, r32, sc):
    for key, val in got.items():
        check_columns(f"{group} d{key.split('.')[-1]}", where, val, r64.grad[key], r32.grad[key], sc[key])


@pytest.mark.parametrize("a0_relu", (True, False))
@pytest.mark.parametrize("k", A.TAIL_K)
@pytest.mark.parametrize("E", A.TAIL_E)
def test_edge_tail_aggregate(E, k, a0_relu):
    """S from the raw node, everything else through edge_tail_aggregate on a [build_mlp, LayerNorm] module: agg, d a0, every dW_i and
    db_i (csplat_dw128_bias for hidden layers, csplat_ln128_bwd's dxsum for the last), dgamma and dbeta (autograd on the caller's
    affine part)"""
    from meshnet.graph_ops import EdgeTailAggregate, edge_tail_aggregate
    v, _ = A.tail_case(E, k, a0_relu)
    ei, N = v["ei"], v["N"]
    csr = csr_of(ei, N)
    din, _ = degrees(ei, N)
    c = randn(E + k, N, 128)
    keys = ["a0", "gamma", "beta"] + [f"{n}{i}" for i in range(1, k + 1) for n in "Wb"]
    r64, r32 = refs(A.edge_tail_aggregate, v, dict(agg=c), keys)
    sc = r64.tape.scales(shapes(r64, *keys))
    s_S = node_sum_scale(r64.out["xhat"], ei[1], N)
    s_agg = (v["gamma"].double().abs() * R.segment_abs_sum(r64.out["xhat"], ei[1], N) + din.double()[:, None] * v["beta"].double().abs()).amax(1)
    seq = tail_module(v, k)
    wb = [t for i in range(1, k + 1) for t in (seq[0][2 * i].weight, seq[0][2 * i].bias)]
    for a0_rg in (True, False):
        where = f"E {E} k {k} a0_relu {a0_relu} a0.rg {a0_rg}"
        seq.zero_grad(set_to_none=True)
        a0 = leaf(v["a0"], a0_rg)
        with torch.no_grad():
            S = EdgeTailAggregate.apply(a0, csr, R.EPS, a0_relu, *wb)
        check_rows("EdgeTailAggregate S", where, S, r64.out["S"], r32.out["S"], s_S)
        assert bool((S[(din == 0).cuda()] == 0).all()), f"{where}: S of a node without edges is not 0"
        agg = edge_tail_aggregate(a0, csr, seq, a0_relu=a0_relu)
        assert has(node_names(agg), "EdgeTailAggregate")
        (agg * dev(c)).sum().backward()
        check_rows("EdgeTailAggregate agg", where, agg, r64.out["agg"], r32.out["agg"], s_agg)
        if a0_rg:
            check_rows("EdgeTailAggregate da0", where, a0.grad, r64.grad["a0"], r32.grad["a0"], sc["a0"])
            if a0_relu:
                zero = (v["a0"] == 0).cuda()
                assert bool(zero.any()) and bool((a0.grad[zero] == 0).all()), f"{where}: a0 = 0 must get gradient 0"
        else:
            assert a0.grad is None
        assert seq[0][0].weight.grad is None
        check_tail_grads("EdgeTailAggregate", where, tail_grads(seq, k), r64, r32, sc)
        if a0_rg:
            first = {key: val.clone() for key, val in tail_grads(seq, k).items()}
            first["S"], first["agg"] = S, agg.detach()
        else:       # a repeat, but for the last input-gradient GEMM: every parameter gradient, S and agg bit for bit
            assert all(same(val, first[key]) for key, val in tail_grads(seq, k).items()) and same(S, first["S"]) and same(agg, first["agg"]), where


def test_edge_tail_aggregate_unused_sum_returns_none_and_launches_nothing(monkeypatch):
    from meshnet import graph_ops
    v, _ = A.tail_case(257, 2, True)
    csr = csr_of(v["ei"], v["N"])
    seq = tail_module(v, 2)
    wb = [t for i in (1, 2) for t in (seq[0][2 * i].weight, seq[0][2 * i].bias)]
    a0 = leaf(v["a0"])
    S = graph_ops.EdgeTailAggregate.apply(a0, csr, R.EPS, True, *wb)
    calls, entered = [], []
    for name in ("linear128", "dw128", "ln128_bwd"):
        monkeypatch.setattr(graph_ops, name, lambda *a, _n=name, **k: calls.append(_n))
    backward = graph_ops.EdgeTailAggregate.backward

    def recording(ctx, g_S):
        out = backward(ctx, g_S)
        entered.append((g_S, out))
        return out
    monkeypatch.setattr(graph_ops.EdgeTailAggregate, "backward", staticmethod(recording))
    _Drop.apply(S).sum().backward()
    assert len(entered) == 1 and entered[0][0] is None, "EdgeTailAggregate.backward did not run with g_S = None"
    assert len(entered[0][1]) == 4 + len(wb) and all(o is None for o in entered[0][1])
    assert calls == [] and a0.grad is None and all(t.grad is None for t in wb)


# ================================================================================================ exact zeros
def test_gradient_is_zero_where_the_pre_activation_is_exactly_zero():
    """whole pre-activation rows exactly 0 in every ReLU'd node: e row 0 with xa[dst] = -xb[src]; a hidden layer with zero weights and
    bias.  torch's convention, relu'(0) = 0, in every element"""
    from meshnet.graph_ops import EdgeCombine, EdgeFirstLayer, SplitKLinear, edge_tail_aggregate
    E, N = 16385, 2500
    ei = A.graph(E, N, "hub")
    csr = csr_of(ei, N)
    row = randn(1, 1, 128)
    xa, xb = row.repeat(N, 1), -row.repeat(N, 1)
    zero_rows = torch.arange(E) % 3 == 0
    g = randn(2, E, 128)
    # EdgeCombine: z = ec exactly
    ec = randn(3, E, 128)
    ec[zero_rows] = 0.0
    ec[1::6] = -0.0
    a, b, c = leaf(xa), leaf(xb), leaf(ec)
    out = EdgeCombine.apply(a, b, c, csr, True)
    out.backward(dev(g))
    assert same(out, torch.relu(ec)) and same(c.grad, g * (ec > 0)) and not bool(c.grad[zero_rows.cuda()].any())
    # EdgeFirstLayer + EdgeTailAggregate: e row 0 -> a0 row 0 -> the mask of the tail's last input-gradient GEMM -> de row 0
    v = A.tail_params(3, 5)
    seq = tail_module(v, 3)
    e = randn(4, E, 128)
    e[zero_rows] = 0.0
    W = leaf(torch.cat([torch.zeros(128, 256), A.weight(R._gen(9))], 1))
    el, a, b = leaf(e), leaf(xa), leaf(xb)
    for scale in (1.0, 16384.0):
        el.grad = None
        a0, _ = EdgeFirstLayer.apply(el, W[:, 256:], scale, a, b, csr)
        assert not bool(a0[zero_rows.cuda()].any())
        agg = edge_tail_aggregate(a0, csr, seq, a0_relu=True)
        (agg * dev(randn(5, N, 128))).sum().backward()
        assert not bool(el.grad[zero_rows.cuda()].any()) and bool(el.grad[~zero_rows.cuda()].any())
    # EdgeTailAggregate: hidden layer 1 with zero weights and bias -> nothing flows below it
    with torch.no_grad():
        seq[0][2].weight.zero_()
        seq[0][2].bias.zero_()
    seq.zero_grad(set_to_none=True)
    a0 = leaf(torch.relu(randn(6, E, 128)))
    agg = edge_tail_aggregate(a0, csr, seq, a0_relu=True)
    (agg * dev(randn(5, N, 128))).sum().backward()
    assert not bool(a0.grad.any()) and not bool(seq[0][2].weight.grad.any()) and not bool(seq[0][2].bias.grad.any())
    assert not bool(seq[0][4].weight.grad.any()) and bool(seq[0][6].bias.grad.isfinite().all())
    # SplitKLinear with a ReLU: zero weight and bias, in both regimes
    for M in (512, 16385):
        x, Wz, bz = leaf(randn(7, M, 128)), leaf(torch.zeros(128, 128)), leaf(torch.zeros(128))
        y = SplitKLinear.apply(x, Wz, bz, True)
        y.backward(dev(randn(8, M, 128)))
        assert not bool(y.any()) and not bool(x.grad.any()) and not bool(Wz.grad.any()) and not bool(bz.grad.any())


# ================================================================================================ chains
def _chain_route(v, csr, route, use_e_next):
    """(aggs, e leaf, [W leaves], [xa], [xb], [seq]) of the three layers through the fused nodes ('fused': EdgeFirstLayer +
    edge_tail_aggregate) or through the per-layer ones ('layers': EdgeLatentLinear + EdgeCombine + the Linear / LayerNorm / SegmentSum
    nodes message_update composes below BIG_ROWS)"""
    from meshnet.graph_network import _tail
    from meshnet.graph_ops import EdgeCombine, EdgeFirstLayer, EdgeLatentLinear, SegmentSum, edge_tail_aggregate, layer_norm_rows
    k = v["k"]
    e = leaf(v["e"])
    cur, aggs, Ws, xas, xbs, seqs = e, [], [], [], [], []
    for l, s in enumerate(v["scales"]):
        p = f"l{l}."
        W, xa, xb, seq = leaf(v[p + "Wfull"]), leaf(v[p + "xa"]), leaf(v[p + "xb"]), tail_module(v, k, p)
        if route == "fused":
            a0, cur = EdgeFirstLayer.apply(cur, W[:, 256:], s, xa, xb, csr)
            aggs.append(edge_tail_aggregate(a0, csr, seq, a0_relu=True))
        else:
            ec, cur = EdgeLatentLinear.apply(cur, W[:, 256:], s)
            h = _tail(seq[0], EdgeCombine.apply(xa, xb, ec, csr, True), True)
            aggs.append(SegmentSum.apply(layer_norm_rows(h, seq[1]), csr))
        Ws.append(W), xas.append(xa), xbs.append(xb), seqs.append(seq)
    return aggs, e, cur, Ws, xas, xbs, seqs


@pytest.mark.parametrize("scales", ((1.0, 2.0, 4.0), (4096.0, 8192.0, 16384.0)))
def test_three_layers_share_one_edge_latent(scales):
    """e.grad is the sum of three layers' contributions, built as a running sum inside their input-gradient GEMMs; each layer's weight
    gradient carries its own scale once.  The same chain through the per-layer nodes, against the same float64 numbers (its float32
    yardstick is the restatement in ITS order: LayerNorm with the affine part per edge, then the sum)"""
    E, k = 16385, 2
    v, _ = A.chain_case(E, scales, k)
    ei, N = v["ei"], v["N"]
    csr = csr_of(ei, N)
    cs = {f"agg{l}": randn(20 + l, N, 128) for l in range(3)}
    keys = ["e"] + [f"l{l}.{n}" for l in range(3) for n in ["Wfull", "xa", "xb", "gamma", "beta"] + [f"{m}{i}" for i in range(1, k + 1) for m in "Wb"]]
    for route in ("fused", "layers"):
        vv = dict(v, affine_on_sums=route == "fused")
        r64, r32 = refs(A.chain, vv, cs, keys)
        if route == "fused":
            first64 = r64
        else:
            for key in keys:        # the two orders are one function
                assert float((r64.grad[key] - first64.grad[key]).abs().max()) <= 1e-10 * float(first64.grad[key].abs().max()), key
        sc = r64.tape.scales(shapes(r64, *keys))
        aggs, e, _, Ws, xas, xbs, seqs = _chain_route(v, csr, route, False)
        names = set().union(*[node_names(a) for a in aggs])
        assert has(names, "EdgeFirstLayer") == (route == "fused") and has(names, "EdgeLatentLinear") == (route == "layers")
        sum((a * dev(cs[f"agg{l}"])).sum() for l, a in enumerate(aggs)).backward()
        grp = f"chain {route}"
        where = f"scales {scales}"
        check_rows(f"{grp} de", where, e.grad, r64.grad["e"], r32.grad["e"], sc["e"])
        nlin = len(r64.tape.lin) // 3
        for l in range(3):
            p = f"l{l}."
            xhat_abs = R.segment_abs_sum(r64.out[f"xhat{l}"], ei[1], N)
            s_agg = (v[p + "gamma"].double().abs() * xhat_abs + torch.bincount(ei[1], minlength=N).double()[:, None] * v[p + "beta"].double().abs()).amax(1)
            check_rows(f"{grp} agg", f"{where} layer {l}", aggs[l], r64.out[f"agg{l}"], r32.out[f"agg{l}"], s_agg)
            check_columns(f"{grp} dW first", f"{where} layer {l}", Ws[l].grad, r64.grad[p + "Wfull"], r32.grad[p + "Wfull"], sc[p + "Wfull"])
            assert not bool(Ws[l].grad[:, :256].any())
            dz = r64.tape.lin[l * nlin]["dz"]
            check_rows(f"{grp} dxa", f"{where} layer {l}", xas[l].grad, r64.grad[p + "xa"], r32.grad[p + "xa"], node_sum_scale(dz, ei[1], N))
            check_rows(f"{grp} dxb", f"{where} layer {l}", xbs[l].grad, r64.grad[p + "xb"], r32.grad[p + "xb"], node_sum_scale(dz, ei[0], N))
            check_tail_grads(grp, f"{where} layer {l}", tail_grads(seqs[l], k, p), r64, r32, sc)


# ================================================================================================ InteractionNetwork.message_update
@pytest.mark.parametrize("big", (False, True))
def test_message_update_below_and_at_big_rows(big):
    """one InteractionNetwork layer at E = BIG_ROWS - 1 (the per-layer nodes) and on the same graph plus one edge (the fused ones): the
    branch from the grad_fn names, x_new, x.grad, e.grad and every parameter's gradient per tensor.  16384 nodes: a draw without ties in
    the NODE MLP's ReLUs needs a sparse graph (gnn_autograd_ref.layer_case), and the node-level Linear layers take the kernels too"""
    from meshnet.graph_network import InteractionNetwork
    from meshnet.graph_ops import SplitKLinear
    BIG = SplitKLinear.BIG_ROWS
    N, E, scale = A.LAYER_N, BIG if big else BIG - 1, 2.0
    ei = A.graph(BIG, N, "hub")[:, :E].contiguous()
    v, _ = A.layer_case(N, ei, scale)
    cx, ce = randn(30, N, 128), randn(31, E, 128)
    params = [k for k in v if k.startswith(("edge_fn", "node_fn"))]
    r64, r32 = refs(A.interaction_layer, v, dict(x_new=cx, e_next=ce), ["x", "e"] + params)
    sc = r64.tape.scales(shapes(r64, "x", "e", *params))
    net = InteractionNetwork(128, 128, 128, 128, v["nlin"] - 1, 128).cuda()
    net.load_state_dict({k: v[k] for k in params})
    x, e = leaf(v["x"]), leaf(v["e"])
    x_new, e_next = net.message_update(x, ei.cuda(), e, scale)
    names = node_names(x_new)
    assert has(names, "EdgeFirstLayer") == has(names, "EdgeTailAggregate") == big, sorted(names)
    assert has(names, "EdgeCombine") == has(names, "SegmentSum") == (not big), sorted(names)
    assert same(e_next, v["e"])
    ((x_new * dev(cx)).sum() + (e_next * dev(ce)).sum()).backward()
    grp = "message_update fused" if big else "message_update layers"
    check_rows(f"{grp} x_new", f"E {E}", x_new, r64.out["x_new"], r32.out["x_new"], r64.out["x_new"].abs().amax(1).clamp_min(1.0))
    check_rows(f"{grp} dx", f"E {E}", x.grad, r64.grad["x"], r32.grad["x"], sc["x"] + cx.double().abs().amax(1))
    check_rows(f"{grp} de", f"E {E}", e.grad, r64.grad["e"], r32.grad["e"], sc["e"] + ce.double().abs().amax(1))
    for name, q in net.named_parameters():
        kind = ("dgamma" if name.endswith("weight") else "dbeta") if ".1." in name else ("dW" if q.dim() == 2 else "db")
        check_columns(f"{grp} {kind}", f"E {E} {name}", q.grad, r64.grad[name], r32.grad[name], sc[name])


# ================================================================================================ GraphCSR.get
def test_graph_csr_cache_follows_the_tensor_its_version_and_the_node_count():
    from meshnet.graph_ops import GraphCSR, SegmentSum
    N, E = 2049, 257
    ei_cpu = A.graph(E, N, "degrees 0..9")
    ei = ei_cpu.clone().cuda()
    csr = GraphCSR.get(ei, N)
    assert GraphCSR.get(ei, N) is csr
    other_n = GraphCSR.get(ei, N + 1)
    assert other_n is not csr and other_n.N == N + 1
    csr = GraphCSR.get(ei, N)
    # a backward that runs after an in-place edit uses the CSR -- the edge list included -- that its forward saw
    msg, g = leaf(randn(40, E, 128)), randn(41, N, 128)
    agg = SegmentSum.apply(msg, csr)
    old_dst = int(ei_cpu[1, 0])
    new_dst = (old_dst + 7) % N
    ei[1, 0] = new_dst
    edited = GraphCSR.get(ei, N)
    assert edited is not csr and GraphCSR.get(ei, N) is edited
    agg.backward(dev(g))
    assert same(msg.grad, g[ei_cpu[1]]), "the backward read the edited edge list"
    rp = edited.rowptr["dst"].cpu()
    want = ei_cpu.clone()
    want[1, 0] = new_dst
    assert torch.equal((rp[1:] - rp[:-1]).long(), torch.bincount(want[1], minlength=N))
    # a freed tensor leaves the cache: it is held weakly, and its entry goes with the next miss
    w = weakref.ref(ei)
    del ei, csr, edited, agg, other_n
    gc.collect()
    assert w() is None, "the cache keeps its edge_index tensors alive"
    ei2 = ei_cpu.flip(0).contiguous().cuda()
    fresh = GraphCSR.get(ei2, N)
    assert all(ref() is not None for ref, *_ in GraphCSR._cache.values())
    rp = fresh.rowptr["dst"].cpu()
    assert torch.equal((rp[1:] - rp[:-1]).long(), torch.bincount(ei_cpu[0], minlength=N))
