"""tests/gnn_autograd_ref.py is what tests/test_gnn_autograd_nodes_gpu.py holds the autograd nodes of meshnet/graph_ops.py to, so it is
checked here first, without a GPU: one InteractionNetwork layer of the restatement against the module composition that
tests/test_knn_gnn_gpu.py's composed() wires from the network's own pieces (edge_fn on cat[x_i, x_j, e], index_add_, node_fn on
cat[agg, x], + x), forward and every gradient, in float64; the EdgeTailAggregate restatement with the caller's affine part against
LayerNorm(MLP(a0)) summed per destination.  Then the preconditions of the GPU file: every draw without ReLU ties ends within its cap,
and every size of the tuples lies beyond the constant it is meant to cross (SplitKLinear.CHUNK / BIG_ROWS / MIN_ROWS read from graph_ops;
the kernels' row constants through the size lists that tests/test_gnn_kernels_cpu.py already holds against the kernel source)."""
import pytest

torch = pytest.importorskip("torch")       # (before the restatements, which import it)

import gnn_kernels_ref as R  # noqa: E402
import gnn_autograd_ref as A  # noqa: E402

F64, F32 = torch.float64, torch.float32


def _rel(a, b):
    return float((a.double() - b.double()).abs().max() / (b.double().abs().max() + 1e-300))


# ------------------------------------------------------------------------------------------------ the restatement against the modules
@pytest.mark.parametrize("scale", (1.0, 4.0))
def test_interaction_layer_is_the_module_composition(scale):
    from meshnet.graph_network import InteractionNetwork
    N, nlin = 50, 3
    ei = A.graph(400, N, "degrees 0..9")
    assert ei.shape[1] == 400 and bool((torch.bincount(ei[1], minlength=N) == 0).any())
    p = A.layer_params(nlin, 3)
    g = R._gen(5)
    x, e = torch.randn(N, 128, generator=g), torch.randn(400, 128, generator=g)
    cx, ce = torch.randn(N, 128, generator=g), torch.randn(400, 128, generator=g)
    r = A.run(A.interaction_layer, dict(x=x, e=e, ei=ei, scale=scale, nlin=nlin, **p), dict(x_new=cx, e_next=ce), F64)
    net = InteractionNetwork(128, 128, 128, 128, nlin - 1, 128).double()
    net.load_state_dict({k: v.double() for k, v in p.items()})
    x64, e64 = x.double().requires_grad_(), e.double().requires_grad_()
    ee = scale * e64
    m = net.edge_fn(torch.cat([x64.index_select(0, ei[1]), x64.index_select(0, ei[0]), ee], -1))
    agg = torch.zeros_like(x64).index_add_(0, ei[1], m)
    y = net.node_fn(torch.cat([agg, x64], -1)) + x64
    ((y * cx.double()).sum() + (e64 * ce.double()).sum()).backward()
    assert _rel(r.out["x_new"], y.detach()) < 1e-12
    assert _rel(r.grad["x"], x64.grad) < 1e-12 and _rel(r.grad["e"], e64.grad) < 1e-12
    for k, q in net.named_parameters():
        assert _rel(r.grad[k], q.grad) < 1e-12, k
    # the scales of every gradient exist, have the gradient's shape (rows for x and e) and bound it
    sc = r.tape.scales({k: tuple(v.shape) for k, v in r.grad.items()})
    for k, q in net.named_parameters():
        assert sc[k].shape == q.shape and bool((q.grad.abs() <= sc[k] * (1 + 1e-9) + 1e-300).all()), k
    assert sc["x"].shape == (N,) and sc["e"].shape == (400,)


@pytest.mark.parametrize("k", A.TAIL_K)
@pytest.mark.parametrize("a0_relu", (True, False))
def test_tail_with_the_affine_part_is_layer_norm_of_the_mlp_summed_per_destination(k, a0_relu):
    v, _ = A.tail_case(257, k, a0_relu)
    c = torch.randn(v["N"], 128, generator=R._gen(6))
    a, b = A.run(A.edge_tail_aggregate, v, dict(agg=c), F64), A.run(A.mlp_ln_sum, v, dict(agg=c), F64)
    assert _rel(a.out["agg"], b.out["agg"]) < 1e-12
    for key in a.grad:
        assert _rel(a.grad[key], b.grad[key]) < 1e-12, key
    # against torch's own LayerNorm and ReLU
    h = torch.relu(v["a0"].double()) if a0_relu else v["a0"].double()
    for i in range(1, k + 1):
        h = torch.nn.functional.linear(h, v[f"W{i}"].double(), v[f"b{i}"].double())
        h = torch.relu(h) if i < k else h
    msg = torch.nn.functional.layer_norm(h, (128,), v["gamma"].double(), v["beta"].double(), R.EPS)
    assert _rel(a.out["agg"], torch.zeros(v["N"], 128, dtype=F64).index_add_(0, v["ei"][1], msg)) < 1e-12
    if a0_relu:
        assert bool((v["a0"] == 0).any()) and bool((a.grad["a0"][v["a0"] == 0] == 0).all())


def test_relu_has_gradient_zero_at_zero_like_torch():
    z = torch.tensor([-1.0, -0.0, 0.0, 2.0], dtype=F64, requires_grad=True)
    A.relu(z).sum().backward()
    z2 = z.detach().clone().requires_grad_()
    torch.relu(z2).sum().backward()
    assert torch.equal(z.grad, z2.grad) and z.grad.tolist() == [0.0, 0.0, 0.0, 1.0]


# ------------------------------------------------------------------------------------------------ the draws end within their cap
def _within_cap(hist, E):
    assert len(hist) <= A.ROUNDS and (not hist or hist[0] <= 0.5 * E + 8), hist


@pytest.mark.parametrize("E", A.NODE_E)
def test_first_layer_and_combine_draws_end(E):
    for scale in A.SCALES:
        v, hist = A.first_layer_case(E, "hub", scale)
        _within_cap(hist, E)
        assert v["e"].shape == (E, 128) and v["ei"].shape == (2, E)
    if E in A.NODE_E[:4]:
        for kind in R.GRAPHS:
            _within_cap(A.combine_case(E, kind, True)[1], E)


@pytest.mark.parametrize("E", A.TAIL_E)
def test_tail_draws_end(E):
    for k in A.TAIL_K:
        for a0_relu in (True, False):
            v, hist = A.tail_case(E, k, a0_relu)
            _within_cap(hist, E)
            assert k > 1 or not hist                # (no hidden layer: nothing to tie)


def test_splitk_chain_and_layer_draws_end():
    for M in A.SPLITK_M:
        _within_cap(A.splitk_case(M)[1], M)
    for K, O in ((128, 64), (20, 128)):
        for M in A.CHUNK_M:
            _within_cap(A.splitk_case(M, K, O)[1], M)
    for scales in ((1.0, 2.0, 4.0), (4096.0, 8192.0, 16384.0)):
        _within_cap(A.chain_case(16385, scales)[1], 16385)


@pytest.mark.parametrize("E", (16383, 16384))
def test_whole_layer_draw_ends(E):
    from meshnet.graph_ops import SplitKLinear
    assert E in (SplitKLinear.BIG_ROWS - 1, SplitKLinear.BIG_ROWS)
    N = A.LAYER_N
    ei = A.graph(16384, N, "hub")[:, :E]
    v, hist = A.layer_case(N, ei, 2.0)
    assert len(hist) <= A.LAYER_ROUNDS, hist


# ------------------------------------------------------------------------------------------------ graphs
def test_graphs_hold_a_hub_and_nodes_without_edges_at_every_size():
    for E in A.NODE_E:
        N = A.nodes_for(E)
        for kind in R.GRAPHS:
            ei = A.graph(E, N, kind)
            assert ei.shape == (2, E) and int(ei.min()) >= 0 and int(ei.max()) < N
            din, dout = torch.bincount(ei[1], minlength=N), torch.bincount(ei[0], minlength=N)
            assert int(din.max()) <= R.HUB_DEGREE + 200 and int(dout.max()) <= R.HUB_DEGREE + 200       # (k_sort_rows: one thread per row)
            if N > 1:
                assert bool((din == 0).any()), (E, kind)
        if E >= R.HUB_DEGREE:
            assert int(torch.bincount(A.graph(E, N, "hub")[1], minlength=N)[N // 2]) >= R.HUB_DEGREE
    # the second whole-layer graph is the first plus one edge
    a, b = A.graph(16384, 16384, "hub")[:, :16383], A.graph(16384, 16384, "hub")
    assert torch.equal(a, b[:, :16383]) and b.shape[1] == a.shape[1] + 1


# ------------------------------------------------------------------------------------------------ sizes against the constants
def test_sizes_lie_beyond_the_constants_they_name():
    """the node-level constants are READ from graph_ops (SplitKLinear.BIG_ROWS / CHUNK / MIN_ROWS, linear_rows' default min_rows); the
    kernels' row constants are not spelled again here: each size is one that tests/gnn_kernels_ref.py already lists and
    tests/test_gnn_kernels_cpu.py already holds against the kernel source"""
    import inspect
    from meshnet import graph_ops
    BIG, CHUNK, MIN = graph_ops.SplitKLinear.BIG_ROWS, graph_ops.SplitKLinear.CHUNK, graph_ops.SplitKLinear.MIN_ROWS
    assert inspect.signature(graph_ops.linear_rows).parameters["min_rows"].default == BIG
    # NODE_E: one row; a 32-row tile and one; 8 tiles and one (the sizes of the rows32 / gather lists); BIG_ROWS - 1, BIG_ROWS,
    # BIG_ROWS + 1 (edge_tail_ok, edge_latent_linear, SplitKLinear.forward switch there; BIG_ROWS + 1 is no multiple of a tile); the
    # first size of the persistent kernel
    assert A.NODE_E == (1, 33, 257, BIG - 1, BIG, BIG + 1, min(R.PERSIST_M))
    assert {1, 33} <= set(R.ROWS32_M) and {1, 33, 257} <= set(R.GATHER_M) and max(R.ROWS32_M) + 1 == min(R.PERSIST_M) and (BIG + 1) % 32
    # NODE_N: one node; one more than the count scan's tile (a size of the CSR list); a cloth mesh's count, a multiple of no tile
    assert A.NODE_N == (1, 2049, 2500) and {1, 2049} <= set(R.CSR_N) and 2048 in R.CSR_N and 2500 % 32 != 0
    # LAYER_N: the whole-layer cases need a sparse graph (layer_case); BIG_ROWS nodes also send the node-level Linear layers to the kernels
    assert A.LAYER_N == BIG and A.LAYER_N not in A.NODE_N
    # SCALES: 2^l of the first, the second and the last of the 15 processor layers of config 4
    assert A.SCALES == (2.0 ** 0, 2.0 ** 1, 2.0 ** 14)
    # TAIL_K: no hidden layer (other indices everywhere), one, the network's two
    assert A.TAIL_K == (1, 2, 3)
    # CHUNK_M: C == 0 with a remainder only (1, CHUNK - 1); one chunk and no remainder; one chunk and one row; two and one; BIG_ROWS =
    # 5 chunks and a remainder
    assert A.CHUNK_M == (1, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1, BIG)
    assert [(M // CHUNK, M % CHUNK) for M in A.CHUNK_M] == [(0, 1), (0, CHUNK - 1), (1, 0), (1, 1), (2, 1), (5, BIG - 5 * CHUNK)] and BIG % CHUNK
    # SPLITK_M: linear_rows' threshold for 128 -> 128 layers, and BIG_ROWS
    assert A.SPLITK_M == (MIN - 1, MIN, BIG - 1, BIG, BIG + 1)
    # LN_M: sizes of the LayerNorm-backward list: one row; 9 workgroups (k_colsum128's slices 5 .. 7 empty); beyond every sweep
    assert set(A.LN_M) <= set(R.LN_BWD_M) and A.LN_M == (1, 513, max(R.LN_BWD_M))
    # TAIL_E: NODE_E's 9 tiles; BIG_ROWS + 1, the size at which csplat_dw128 runs all its parts (the largest of DW_M); the persistent kernel
    assert A.TAIL_E == (A.NODE_E[2], BIG + 1, A.NODE_E[-1]) and BIG + 1 == max(R.DW_M)
    # the margin of the draws: four times the classical bound of a 128-term fp32 dot product
    assert A.MARGIN == 4 * 128 * 2.0 ** -23
