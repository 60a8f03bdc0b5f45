"""tests/gnn_kernels_ref.py is what tests/test_gnn_kernels_gpu.py holds the 128-wide Linear, LayerNorm and CSR kernels to, so it is checked
here first, without a GPU: against F.linear, F.layer_norm, autograd over both, index_add_ and numpy's stable argsort, on the GPU file's
own inputs.  Then the preconditions of the GPU file's cases: every size lies beyond the launch constant it is meant to cross (the
constants as literals, each with the source expression that holds it), and the inputs are conditioned so that the restatement itself is
stable -- every bar the restatement alone produces (8 x its own float32 error, per row class) is below the 1e-3 ceiling -- and sharp:
the LayerNorm rows tell E[x^2] - mean^2 from the two-pass variance, the cancelling messages tell a plain running sum from a compensated
one, and the compensated update is what turned an Inf into a NaN.  Conditions on the inputs, not measurements of any kernel."""
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")       # (before gnn_kernels_ref, which imports it)

import gnn_kernels_ref as R  # noqa: E402  (tests/ is on sys.path: conftest.py; nothing here needs the built library)

F64, F32 = torch.float64, torch.float32
K, FLOOR, BAR_MAX = 8.0, 1e-6, 1e-3
EPS32 = 2.0 ** -23
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "cloth-splatting_amd", "csrc")


def _rel(a, b):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30)) if b.numel() else 0.0


def _row_e32(r64, r32, scale):
    return float(((r32.double() - r64).abs().amax(1) / scale.clamp_min(1e-300)).max())


# ------------------------------------------------------------------------------------------------ the restatement against trusted forms
def test_linear128_is_F_linear_with_the_epilogue_in_the_documented_order():
    M = 67
    A = R.row_classes(M)
    A[5::8] *= 1e-12                    # (LayerNorm variants: see _run_variant of the GPU file)
    W, bias, gamma, beta = R.linear_params()
    pre, post, mask = R.addends(M)
    ga, ia, gb, ib = R.gather_case(M, "perm")
    lin = torch.nn.functional.linear
    a, w, b = A.double(), W.double(), bias.double()
    # alpha scales the product, not the bias; add_pre sits in front of the ReLU, add_post behind the LayerNorm, the mask comes last
    v = torch.relu(0.5 * lin(a, w) + b + pre.double())
    full = torch.nn.functional.layer_norm(v, (128,), gamma.double(), beta.double(), R.EPS) + post.double()
    full = full * (mask > 0)
    got, stats = R.linear128(A, W, bias, 0.5, True, None, (gamma, beta), pre, post, mask)
    assert _rel(got, full) < 1e-13
    assert _rel(stats[:, 0], v.mean(1)) < 1e-13 and _rel(stats[:, 1], 1 / (v.var(1, unbiased=False) + R.EPS).sqrt()) < 1e-12
    assert _rel(R.linear128(A, W, bias, 4.0, True, (ga, ia, gb, ib))[0], torch.relu(4.0 * lin(a, w) + b + ga.double()[ia] + gb.double()[ib])) < 1e-14
    assert _rel(R.linear128(A, W, None, 1.0, False, mask=mask)[0], lin(a, w) * (mask > 0)) < 1e-14
    assert R.linear128(A, W)[1] is None
    # the orders matter on these inputs: the misplaced forms are far away
    wrong_alpha = torch.relu(0.5 * (lin(a, w) + b))
    wrong_post = torch.nn.functional.layer_norm(torch.relu(0.5 * lin(a, w) + b) + post.double(), (128,), gamma.double(), beta.double(), R.EPS)
    right = R.linear128(A, W, bias, 0.5, True, None, (gamma, beta), None, post)[0]
    o = slice(0, None, 8)            # (the ordinary rows: a whole-tensor error would be owned by the huge ones)
    assert _rel(wrong_alpha[o], R.linear128(A, W, bias, 0.5, True)[0][o]) > 1e-2 and _rel(wrong_post[o], right[o]) > 1e-2
    # a mask entry of +0 or -0 is "not positive": `>=` would let those columns through
    assert bool((mask[:, 5] == 0).all()) and bool((mask[:, 9] == 0).all()) and not bool(got[:, [5, 9]].any())
    assert bool(R.linear128(A, W, bias, mask=torch.ones(M, 128))[0][:, [5, 9]].any())
    # torch.relu keeps a NaN
    A2 = A.clone()
    A2[3, 7] = float("nan")
    assert bool(torch.isnan(R.linear128(A2, W, bias, relu=True)[0][3]).all())
    # the four storages hold the same matrix
    for layout in R.LAYOUTS:
        st, ldw, wt, off = R.weight_storage(W, layout)
        flat = st.reshape(-1)
        j, k = torch.meshgrid(torch.arange(128), torch.arange(128), indexing="ij")
        read = flat[off + (k * ldw + j if wt else j * ldw + k)]
        assert torch.equal(read, W) and ldw >= 128 and (4 * off) % 16 == 0, layout
    assert {ldw for ldw in (R.weight_storage(W, lay)[1] for lay in R.LAYOUTS)} == {128, 384}


def test_layer_norm_forward_and_backward_are_F_layer_norm_and_its_autograd():
    for M in (1, 67):
        x = R.ln_rows(M)
        _W, _b, gamma, beta = R.linear_params(1)
        g = torch.randn(M, 128, generator=torch.Generator().manual_seed(M))
        xd, gd, bd = (t.double().requires_grad_() for t in (x, gamma, beta))
        y = torch.nn.functional.layer_norm(xd, (128,), gd, bd, R.EPS)
        y.backward(g.double())
        got, stats = R.layer_norm(x, gamma, beta)
        assert _rel(got, y.detach()) < 1e-12
        dx, dgamma, dbeta, dxsum = R.layer_norm_bwd(g, x, stats, gamma)
        assert _rel(dx, xd.grad) < 1e-9 and _rel(dgamma, gd.grad) < 1e-12 and _rel(dbeta, bd.grad) < 1e-13 and _rel(dxsum, xd.grad.sum(0)) < 1e-9
        # x_normalized: xhat in place of x
        xhat = R.layer_norm(x, torch.ones(128), torch.zeros(128))[0]
        for a, b in zip(R.layer_norm_bwd(g, xhat, stats, gamma, x_normalized=True), (dx, dgamma, dbeta, dxsum)):
            assert _rel(a, b) < 1e-12
        # g_rows: the gathered copy
        rows = torch.randint(0, max(M // 3, 1), (M,), generator=torch.Generator().manual_seed(1))
        small = g[:max(M // 3, 1)]
        for a, b in zip(R.layer_norm_bwd(small, x, stats, gamma, g_rows=rows), R.layer_norm_bwd(small[rows], x, stats, gamma)):
            assert torch.equal(a, b)
        # a constant row: exactly beta, in float32 too
        if M > 2:
            assert torch.equal(R.layer_norm(x, gamma, beta, dtype=F32)[0][2], beta) and torch.equal(got[2], beta.double())
    out = torch.randn(9, 128, generator=torch.Generator().manual_seed(2))
    out[:, 3], out[:, 70] = 0.0, -0.0
    g = torch.randn(9, 128, generator=torch.Generator().manual_seed(3))
    gm, db = R.relu_mask_bias(g, out, F32)
    assert torch.equal(gm, torch.ops.aten.threshold_backward(g, out, 0)) and torch.equal(db, gm.sum(0)) and not bool(gm[:, [3, 70]].any())
    assert torch.equal(R.relu_mask_bias(g, None, F32)[0], g)


def test_node_update_narrow_linear_and_dw_are_their_torch_expressions():
    N = 33
    g = torch.Generator().manual_seed(0)
    agg, x = torch.randn(N, 128, generator=g), torch.randn(N, 128, generator=g)
    p = R.node_update_params()
    d = {k: v.double() for k, v in p.items()}
    lin = torch.nn.functional.linear
    h = torch.relu(lin(torch.cat([agg, x], 1).double(), torch.cat([d["Wa"], d["Wx"]], 1), d["b0"]))      # the first Linear on cat(agg, x)
    h = torch.relu(lin(h, d["W2"], d["b2"]))
    xn = torch.nn.functional.layer_norm(lin(h, d["W3"], d["b3"]), (128,), d["gamma"], d["beta"], R.EPS) + x.double()
    got = R.node_update(agg, x, p)
    assert _rel(got[0], xn) < 1e-13 and _rel(got[1], lin(xn, d["Wi"])) < 1e-13 and _rel(got[2], lin(xn, d["Wj"])) < 1e-13
    hard = R.node_update_params(hard=64.0)
    ln = R.layer_norm(hard["b3"][None], hard["gamma"], hard["beta"])[0]
    assert _rel(R.node_update(agg, x, hard)[0] - x.double(), ln.expand(N, 128)) < 1e-13
    assert abs(float(hard["b3"].mean()) - 64.0) < 0.05 and abs(float(hard["b3"].std()) - 1 / 16) < 0.02
    xs, W, b = torch.randn(65, 5, generator=g), torch.randn(128, 5, generator=g), torch.randn(128, generator=g)
    assert _rel(R.linear_narrow(xs, W, b, True), torch.relu(lin(xs.double(), W.double(), b.double()))) < 1e-14
    assert _rel(R.linear_narrow(xs, W, None, False), lin(xs.double(), W.double())) < 1e-14
    gr, xr = torch.randn(65, 128, generator=g), torch.randn(65, 128, generator=g)
    for x_relu in (False, True):
        Wd = torch.zeros(128, 128, dtype=F64, requires_grad=True)
        bd = torch.zeros(128, dtype=F64, requires_grad=True)
        inp = torch.relu(xr.double()) if x_relu else xr.double()
        lin(inp, Wd, bd).backward(gr.double())
        dW, db = R.dw128(gr, xr, x_relu)
        assert _rel(dW, Wd.grad) < 1e-13 and _rel(db, bd.grad) < 1e-13


@pytest.mark.parametrize("N", R.CSR_N)
def test_csr_is_the_stable_argsort_and_segment_sum_is_index_add(N):
    for kind in R.GRAPHS:
        ei = R.graph(N, kind)
        E = int(ei.shape[1])
        assert ei.dtype == torch.int64 and (E == 0 or (int(ei.min()) >= 0 and int(ei.max()) < N))
        for row in (0, 1):
            keys = ei[row].numpy()
            rowptr, perm = R.csr_fast(keys, N)
            np.testing.assert_array_equal(perm, np.argsort(keys, kind="stable"))
            np.testing.assert_array_equal(rowptr, np.searchsorted(np.sort(keys), np.arange(N + 1)))
            if N <= 2049:            # the counting sort written out
                a, b = R.csr(keys, N)
                np.testing.assert_array_equal(a, rowptr)
                np.testing.assert_array_equal(b, perm)
            for n_ in (0, N // 2, N - 1):        # ascending edge ids inside a row
                seg = perm[rowptr[n_]:rowptr[n_ + 1]]
                assert (np.diff(seg) > 0).all() and (keys[seg] == n_).all()
        if N > 2049:
            continue
        for L in (128, 6):
            msg = R.messages(ei, L, "cancelling")
            ref = torch.zeros(N, L, dtype=F64)
            for e in range(E):
                ref[ei[1, e]] += msg[e].double()
            assert _rel(R.segment_sum(msg, ei[1], N), ref) < 1e-12
            xa, xb = torch.randn(N, L), torch.randn(N, L)
            out = R.edge_combine(xa, xb, msg, ei, True, F32)
            assert torch.equal(out, torch.relu((xa[ei[1]] + xb[ei[0]]) + msg))
            gm, dxa, dxb = R.edge_combine_bwd(msg, out, ei, N, True)
            assert torch.equal(gm, torch.where(out > 0, msg, torch.zeros_like(msg)).double())
            assert _rel(dxa, torch.zeros(N, L, dtype=F64).index_add_(0, ei[1], gm)) < 1e-15
            assert _rel(dxb, torch.zeros(N, L, dtype=F64).index_add_(0, ei[0], gm)) < 1e-15
    assert R.segment_sum(torch.zeros(0, 6), torch.zeros(0, dtype=torch.int64), N).shape == (N, 6)


def test_graph_shapes_hold_what_they_are_to_contain():
    N = 2049
    deg = {k: torch.bincount(R.graph(N, k)[1], minlength=N) for k in R.GRAPHS}
    assert int(deg["hub"][N // 2]) == R.HUB_DEGREE == int(deg["hub"].sum()) and 2000 <= R.HUB_DEGREE <= 4000
    assert int(deg["last"][N - 1]) == int(deg["last"].sum()) > 0
    ei = R.graph(N, "duplicates")
    assert ei.shape[1] == 200 and torch.equal(ei[:, :40], ei[:, 40:80])
    ei = R.graph(N, "self loops")
    assert torch.equal(ei[0], ei[1]) and ei.shape[1] == N
    d = deg["degrees 0..9"]
    assert torch.equal(d[:3000 if N > 3000 else N], torch.arange(N) % 10) and {int(v) % 4 for v in d.unique()} == {0, 1, 2, 3} and bool((d == 0).any())
    ei = R.graph(N, "degrees 0..9")
    seg = (ei[1] == 19).nonzero().reshape(-1)
    assert seg.numel() == 9 and int((seg[1:] - seg[:-1]).max()) > 1            # (the edge ids of a row are scattered)
    assert R.graph(1, "hub").shape[1] == R.HUB_DEGREE and not bool(R.graph(1, "hub").any())


# ------------------------------------------------------------------------------------------------ sizes against the launch constants
def _source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _has(source, literal):
    """the launch constant as the source spells it.  A tripwire on the TEXT: if only the spelling changed (a reformat, a renamed variable),
    update the literal here; if the constant changed, the size lists of tests/gnn_kernels_ref.py must follow it"""
    assert literal in source, (f"`{literal}` is no longer in the kernel source: if the launch constant it holds changed, move the sizes of "
                               "tests/gnn_kernels_ref.py across the new value; if only its spelling changed, update this literal, not the kernel")
    return True


def test_sizes_lie_beyond_the_launch_constants():
    """the constants as literals; each comment gives the source expression that holds it, and the expression is looked up in the source
    so that a changed constant fails here and not silently in the GPU file"""
    cdiv = lambda a, b: -(-a // b)  # noqa: E731
    gemm, gnn, sort = _source("csplat_gemm.hip"), _source("csplat_gnn.hip"), _source("csplat_sort.hip")
    # csplat_gemm.hip, csplat_linear128_ex: `if (!gather && ntile <= 2048)` with `ntile = (M + 31) / 32`: rows32 up to 65 536 rows
    assert _has(gemm, "if (!gather && ntile <= 2048)") and _has(gemm, "const int64_t ntile = (M + 31) / 32;")
    assert cdiv(65536, 32) == 2048 and cdiv(65537, 32) == 2049 and max(R.ROWS32_M) == 65536 and min(R.PERSIST_M) == 65537
    assert {1, 31, 32, 33} <= set(R.ROWS32_M)                                   # one row, a tile less one, a tile, a tile and one
    # `int grid = b3 ? (int)((ntile + 7) / 8) : (int)((ntile + 3) / 4);` `const int cap = b3 ? 256 : 512;` and `NW = B3 ? 8 : 4`:
    # either mode holds 2048 tiles in one sweep of the capped grid
    assert _has(gemm, "const int cap = b3 ? 256 : 512;") and _has(gemm, "constexpr int NW = B3 ? 8 : 4;")
    assert _has(gemm, "int grid = b3 ? (int)((ntile + 7) / 8) : (int)((ntile + 3) / 4);")
    assert 256 * 8 == 512 * 4 == 2048
    for M, tiles, ragged in ((65537, 2049, True), (65568, 2049, False), (131073, 4097, True)):
        assert M in R.PERSIST_M and cdiv(M, 32) == tiles and (M % 32 != 0) == ragged
    assert 2049 - 2048 == 1                 # 65 537 / 65 568: the last tile is the only one of the second sweep, ragged and full
    assert 4097 - 2 * 2048 == 1             # 131 073: every wave a second tile, one ragged tile in a third sweep
    # gathers never take rows32: M below the 4 (fp32) and 8 (bf16) waves of ONE workgroup (1 tile, 2 tiles), around 4 and 8 tiles
    assert {1, 33} <= set(R.GATHER_M) and cdiv(33, 32) == 2 < 4
    assert [cdiv(m, 32) for m in (128, 129, 255, 257)] == [4, 5, 8, 9] and {128, 129, 255, 257, 65537} <= set(R.GATHER_M)
    # csplat_sort.hip `SCAN_THREADS = 256`, `SCAN_ITEMS = 8`, `SCAN_TILE = SCAN_THREADS * SCAN_ITEMS`: the count scan of
    # csplat_gnn_build_csr runs over N counts in tiles of 2048
    assert _has(sort, "constexpr int SCAN_THREADS = 256;") and _has(sort, "constexpr int SCAN_ITEMS = 8;")
    assert _has(sort, "constexpr int SCAN_TILE = SCAN_THREADS * SCAN_ITEMS;") and 256 * 8 == 2048
    assert {2047, 2048, 2049} <= set(R.CSR_N) and cdiv(4097, 2048) == 3 and 4097 in R.CSR_N and max(R.CSR_N) > 32 * 2048 and 1 in R.CSR_N
    # csplat_gnn.hip `int ln_blocks(int64_t M) { const int64_t want = (M + 63) / 64; ... want > 1024 ? 1024 : want`,
    # `LN_ROWS_PER_BLOCK_ITER = LN_THREADS / 32` = 8 row slots per workgroup
    assert _has(gnn, "const int64_t want = (M + 63) / 64;") and _has(gnn, "want > 1024 ? 1024 : want") and _has(gnn, "LN_THREADS = 256, LN_ROWS_PER_BLOCK_ITER = LN_THREADS / 32")
    blocks = lambda M: min(max(cdiv(M, 64), 1), 1024)  # noqa: E731
    assert {1, 8, 9} <= set(R.LN_BWD_M)                                          # below, at and beyond the 8 slots of one workgroup
    assert blocks(64) == 1 and blocks(65) == 2 and {64, 65} <= set(R.LN_BWD_M)
    # k_colsum128 `const int per = (nblocks + 7) / 8`: 8 slices of the partials -- 7.98 and 8.02 blocks per slice, and empty slices below
    assert _has(gnn, "const int per = (nblocks + 7) / 8")
    assert blocks(511) == 8 and blocks(513) == 9 and {511, 513} <= set(R.LN_BWD_M) and cdiv(9, 8) * 5 > 9        # (9 blocks: slices 5 .. 7 empty)
    assert blocks(65536) == 1024 and 65536 // (1024 * 8) == 8 and 65537 - 1024 * 8 * 8 == 1 and {65536, 65537} <= set(R.LN_BWD_M)
    # csplat_gemm.hip `constexpr int SK_ROWS = 64;` `const int grid = (int)(nb < 2048 ? nb : 2048);` K <= 32
    assert _has(gemm, "constexpr int SK_ROWS = 64;") and _has(gemm, "const int grid = (int)(nb < 2048 ? nb : 2048);") and _has(gemm, "K >= 1 && K <= 32")
    assert set(R.NARROW_M) == {64, 65, 2048 * 64 + 1} and {1, 32} <= set(R.NARROW_K) and any(k % 4 for k in R.NARROW_K if k > 1)
    # `int dw128_parts(int64_t M) { const int64_t want = (M + 4 * 4 * DW_GROUP - 1) / (4 * 4 * DW_GROUP);` DW_GROUP = 4, DW_WG_MAX = 256
    assert _has(gemm, "constexpr int DW_GROUP = 4;") and _has(gemm, "constexpr int DW_WG_MAX = 256;") and _has(gemm, "(M + 4 * 4 * DW_GROUP - 1) / (4 * 4 * DW_GROUP)")
    parts = lambda M: min(max(cdiv(M, 64), 1), 256)  # noqa: E731
    assert [parts(m) for m in R.DW_M] == [1, 1, 2, 256] and 16385 > 256 * 64 and 16385 % 2 == 1
    # k_segment_sum `for (; i + 4 <= e; i += 4)`: degrees of every residue mod 4; widths with L % 4 == 0 (float4) and not
    assert _has(gnn, "for (; i + 4 <= e; i += 4)") and {w % 4 == 0 for w in R.WIDTHS} == {True, False} and 128 in R.WIDTHS


# ------------------------------------------------------------------------------------------------ input conditions
def _bars(r64, r32, scale, names):
    k = len(names)
    out = {}
    for c in range(min(k, r64.shape[0])):
        e32 = _row_e32(r64[c::k], r32[c::k], scale[c::k])
        out[names[c]] = max(K * e32, FLOOR)
    return out


@pytest.mark.parametrize("M", (33, 4099))
def test_linear_inputs_are_conditioned(M):
    """every bar the restatement alone produces on the Linear cases is below the ceiling, class by class; tiny and zero rows stay
    representable; the classes are what they say"""
    A = R.row_classes(M)
    W, bias, gamma, beta = R.linear_params()
    pre, post, mask = R.addends(M)
    assert A.dtype == F32 and not bool(A[7::8].any()) and bool(((A[6::8] != 0).sum(1) == 1).all())
    assert 1e-32 < float(A[4::8].abs().max()) < 1e-28 and 1e19 < float(A[5::8].abs().max()) < 1e22
    wide = A[3::8].abs()
    assert float((wide.amax(1) / wide.clamp_min(1e-30).amin(1)).median()) > 1e6
    assert bool(torch.isfinite(A @ W.t()).all()) and float((A[4::8] @ W.t()).abs().max()) > 1e-33      # (far above the denormals)
    p64 = A.double() @ W.double().t()
    absprod = A.double().abs() @ W.double().abs().t()
    for alpha, b, pr, po, mk in ((1.0, None, None, None, None), (0.5, bias, None, None, None), (0.5, bias, pre, post, mask), (1.0, None, None, None, mask)):
        r64 = R.linear128(A, W, b, alpha, b is not None, None, None, pr, po, mk)[0]
        r32 = R.linear128(A, W, b, alpha, b is not None, None, None, pr, po, mk, dtype=F32)[0]
        scale = alpha * absprod + sum(t.double().abs() for t in (b, pr, po) if t is not None)
        bars = _bars(r64, r32, scale.amax(1), R.ROW_CLASSES)
        assert max(bars.values()) <= 1e-5, bars
    A2 = A.clone()
    A2[5::8] *= 1e-12
    for pr, po, mk in ((None, None, None), (pre, post, mask)):
        r64, s64 = R.linear128(A2, W, bias, 2.0, True, None, (gamma, beta), pr, po, mk)
        r32, s32 = R.linear128(A2, W, bias, 2.0, True, None, (gamma, beta), pr, po, mk, dtype=F32)
        bars = _bars(r64, r32, r64.abs().amax(1).clamp_min(1.0), R.ROW_CLASSES)
        assert max(bars.values()) <= 1e-4, bars
        assert bool(torch.isfinite(s32).all())
    # the squares of a 1e20 row are Inf in a float32 LayerNorm (rstd = 0: the row comes out as beta; torch's own float32 layer_norm gives NaN), which is why the
    # LayerNorm variants hold their huge rows at 1e8
    huge = A[5:6] @ W.t()
    assert torch.equal(R.layer_norm(huge, gamma, beta, dtype=F32)[0][0], beta) and bool(torch.isnan(torch.nn.functional.layer_norm(huge, (128,), gamma, beta, R.EPS)).all())
    assert _rel(R.layer_norm(huge, gamma, beta)[0][0], beta) > 0.1
    assert p64.shape == (M, 128)


@pytest.mark.parametrize("M", (67, 65537))
def test_layernorm_rows_are_conditioned_and_tell_the_one_pass_variance_apart(M):
    x = R.ln_rows(M)
    _W, _b, gamma, beta = R.linear_params(1)
    r64, s64 = R.layer_norm(x, gamma, beta)
    r32, s32 = R.layer_norm(x, gamma, beta, dtype=F32)
    scale = r64.abs().amax(1).clamp_min(1.0)
    bars = _bars(r64, r32, scale, R.LN_CLASSES)
    assert max(bars.values()) <= BAR_MAX, bars
    one = R.layer_norm_one_pass(x, gamma, beta, dtype=F32)
    for c, name in ((0, "mean 16 std 1/16"), (1, "mean 64 std 1/16")):
        miss = _row_e32(r64[c::8], one[c::8], scale[c::8])
        assert miss > 10 * bars[name], (name, miss, bars[name])           # E[x^2] - mean^2 in float32 is far outside the bar
    # ... and on the rows the old test used it is not: 3 randn + 0.5
    assert _row_e32(r64[7::8], one[7::8], scale[7::8]) < bars["3 randn + 0.5"]
    # the classes are what they say
    assert abs(float(x[0].mean()) - 16) < 0.05 and abs(float(x[1].mean()) - 64) < 0.05 and abs(float(x[1].std()) - 1 / 16) < 0.02
    assert float(x[2].var(unbiased=False)) == 0.0 and 0 < float(x[3].var(unbiased=False)) < 1e-2 * R.EPS
    if M > 32:
        assert {float(x[2 + 8 * k, 0]) for k in range(4)} == set(R.LN_CONSTANTS)
    # the backward on these rows
    g = torch.randn(M, 128, generator=torch.Generator().manual_seed(M)) * torch.tensor([1.0, 1e-3, 1e3])[(torch.arange(M) // 8) % 3][:, None]
    d64, d32 = R.layer_norm_bwd(g, x, s32, gamma), R.layer_norm_bwd(g, x, s32, gamma, dtype=F32)
    bars = _bars(d64[0], d32[0], s32[:, 1].double() * (g.double() * gamma.double()).abs().amax(1), R.LN_CLASSES)
    assert max(bars.values()) <= 1e-5, bars


def _neumaier32(values, finish):
    """k_segment_sum's update in float32, value by value; finish: acc alone when acc is not finite"""
    f = np.float32
    acc, comp = f(0), f(0)
    with np.errstate(all="ignore"):
        for v in values:
            v = f(v)
            t = f(acc + v)
            comp = f(comp + (f(f(acc - t) + v) if abs(acc) >= abs(v) else f(f(v - t) + acc)))
            acc = t
        return acc if (finish and not np.isfinite(acc)) else f(acc + comp)


def test_messages_tell_compensated_from_plain_sums_and_the_inf_rule():
    inf = float("inf")
    for vals, want in (([1, inf, 2], inf), ([1, -inf, 2], -inf), ([3e38, 3e38, 1], inf), ([-3e38, -3e38, -3e38, 1], -inf)):
        ref = float(torch.zeros(1).index_add_(0, torch.zeros(len(vals), dtype=torch.int64), torch.tensor(vals, dtype=F32)))
        assert ref == want and np.isnan(_neumaier32(vals, False)) and float(_neumaier32(vals, True)) == want
    assert np.isnan(_neumaier32([inf, 1, -inf], True)) and np.isnan(_neumaier32([1, float("nan"), 2], True))
    g = np.random.default_rng(0)
    finite = g.normal(size=50).astype(np.float32)
    assert _neumaier32(finite, True) == _neumaier32(finite, False)                 # finite sums: the same bits
    # a cancelling row: the plain running sum breaks the bound the GPU file holds the kernel to, the compensated one keeps it
    ei = R.graph(300, "degrees 0..9")
    msg = R.messages(ei, 6, "cancelling")
    node = 9                                                                        # (degree 9)
    col = msg[ei[1] == node][:, 0].numpy()
    assert col[0] == 1e6 and col[-1] == -1e6 and len(col) == 9
    exact = float(col.astype(np.float64).sum())
    bound = EPS32 * abs(exact) + len(col) * EPS32 ** 2 * float(np.abs(col.astype(np.float64)).sum())
    plain = np.float32(0)
    for v in col:
        plain = np.float32(plain + v)
    assert abs(float(plain) - exact) > 100 * bound and abs(float(_neumaier32(col, True)) - exact) <= bound
    z = R.messages(ei, 6, "zeros")
    assert bool((z[0::3] == 0).all()) and bool(torch.signbit(z[1::3]).all()) and not bool(torch.signbit(z[0::3]).any())
