"""The scratch / temp / workspace buffers of include/csplat.h under hostile contents, at their exact sizes, between guard bytes.

Every other GPU test hands these buffers over as production does: torch.empty, often max(bytes, 256), from an allocator that mostly
returns zeros.  Two kinds of bug pass that way: a kernel that reads a scratch word before this call wrote it (a partial behind a
grid-stride edge, a digit table, a counter, a ticket) where the header says "any contents", and a size query that is short of what the host
carves out of the buffer.  Here every entry behind a size query (TABLE below; tests/test_scratch_contracts_cpu.py holds it against the
header) is called through native.lib with

  * a scratch of EXACTLY the queried bytes (tests/scratch_guard.py: no minimum size, 256-byte aligned inside a larger allocation), filled
    with 0x00, 0xFF (float NaN, int32 -1) and 0x7F (float 3.39e38, a huge integer) in turn -- but for the words the header wants zero;
  * 4096 guard bytes in front of and behind the scratch AND every output, which must survive;
  * outputs that are equal BIT FOR BIT across the three fills wherever the header calls the entry deterministic, reproducible or
    bit-exact, and held to the owning test file's bar in each run where it does not (the float-atomic form of the rasterizer backward);
  * the 0xFF run compared with the reference its owning test file uses (the brute-force entry, the numpy restatement, float64 under that
    file's bar): "independent of the fill, but wrong" cannot pass;
  * the ticket words the header promises to leave at zero read back after the call.

The sizes are the smallest that cross the launch constants (stated at each parametrize), not workload sizes; no tolerance is invented
here: every bar is imported from, or restated with a reference to, the file that owns the kernel.  Where an owning file has an importable
helper for the direct call it is used (_sim_fwd, _ssim_fwd_abi, flat_call of tests/test_raster_backward_dispatch_gpu.py); the other calls
are made here because their outputs lie between guards.

On an MI355X when this file was written: 150 tests in 7.5 s, the slowest test_rows_dot[32769] at 0.9 s, every other below 0.5 s; no guard
byte written, no output dependent on the fill.  With the hipMemsetAsync of csplat_psnr's tickets removed in a scratch build, the 0xFF and
0x7F runs of csplat_psnr fail (the last-arrival branch never fires, `out` keeps its initial bytes) and the 0x00 run passes."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

import util
from scratch_guard import FILLS, guarded, guarded_out

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
F64, F32, I32, U8 = torch.float64, torch.float32, torch.int32, torch.uint8

# size query -> the tests of this file that run the entry behind it.  tests/test_scratch_contracts_cpu.py: every `size_t csplat_*_bytes(`
# of the header is a key here or in EXCLUDED, and every name here is a test of this file.
TABLE = {
    "csplat_dist2_temp_bytes": ["test_dist2_ws"],
    "csplat_knn_temp_bytes": ["test_knn_ws"],
    "csplat_knn_query_temp_bytes": ["test_knn_query_ws"],
    "csplat_chamfer_bwd_temp_bytes": ["test_chamfer_bwd"],
    "csplat_knn_regs_graph_temp_bytes": ["test_knn_regs_graph"],
    "csplat_knn_regs_fwd_scratch_bytes": ["test_knn_regs_fwd"],
    "csplat_mask_to_map_temp_bytes": ["test_mask_to_map"],
    "csplat_rows_dot_scratch_bytes": ["test_rows_dot"],
    "csplat_sim_hidden_scratch_bytes": ["test_sim_hidden_one_buffer_for_every_T"],
    "csplat_cloth_regs_scratch_bytes": ["test_cloth_regs_exact_size"],
    "csplat_psnr_scratch_bytes": ["test_psnr", "test_psnr_off_the_16_byte_boundary"],
    "csplat_image_loss_scratch_bytes": ["test_image_loss", "test_ssim_fwd_masked_outputs"],
    "csplat_l1_scratch_bytes": ["test_l1", "test_l1_masked_and_signs"],
    "csplat_geom_loss_scratch_bytes": ["test_geom_loss"],
    "csplat_flow_loss_scratch_bytes": ["test_flow_loss"],
    "csplat_obs_unproject_temp_bytes": ["test_obs_unproject"],
    "csplat_obs_voxel_temp_bytes": ["test_obs_voxel"],
    "csplat_gnn_csr_temp_bytes": ["test_gnn_build_csr"],
    "csplat_dw128_workspace_bytes": ["test_dw128"],
    "csplat_backward_scratch_bytes": ["test_raster_backward"],
    "csplat_backward_depth_scratch_bytes": ["test_raster_backward"],
    "csplat_visibility_scratch_bytes": ["test_visibility_views"],
}
# the two scratch buffers the header sizes in words, not through a query (csplat/gaussians.py: corner_scratch_floats,
# meshnet/rollout.py: refine_scratch_floats)
SIZED_IN_PYTHON = {"corner_scratch_floats": ["test_vertex_gather_scratch"], "refine_scratch_floats": ["test_edge_length_refine_scratch"]}
EXCLUDED = {
    "csplat_geom_bytes": "forward chunk: allocated through the speculative two-phase forward, layout pinned by test_indices_bit_exact",
    "csplat_image_bytes": "forward chunk: allocated through the speculative two-phase forward, layout pinned by test_indices_bit_exact",
    "csplat_binning_bytes": "forward chunk: allocated through the speculative two-phase forward, layout pinned by test_indices_bit_exact",
    "csplat_temp_bytes": "forward chunk: allocated through the speculative two-phase forward, layout pinned by test_indices_bit_exact",
    "csplat_backward_camera_scratch_bytes": "reached through the batched view records only; layout pinned by test_raster_scratch_layout_cpu.py",
    "csplat_backward_feature_scratch_bytes": "reached through the batched view records only; layout pinned by test_raster_scratch_layout_cpu.py",
    "csplat_mesh_rest_bytes": "persistent data (the rest-pose records), not scratch",
    "csplat_gnn_node_update_image_bytes": "persistent data (a packed weight image), not scratch",
    "csplat_gnn_edge_mlp3_image_bytes": "persistent data (a packed weight image), not scratch",
    "csplat_sort_pairs_temp_bytes": "exact size and guard bytes in tests/test_sort_scan_gpu.py",
    "csplat_scan_u32_temp_bytes": "exact size and guard bytes in tests/test_sort_scan_gpu.py",
}


# ================================================================================================ the harness
def _n():
    from csplat import native
    return native


def call(name, *args):
    n = _n()
    n.check(getattr(n.lib, name)(n.stream_handle(torch.device("cuda")), *args), name)


def P(t):
    """device pointer: None -> NULL; a guarded output -> its address (valid for an empty one too); any other tensor, empty -> NULL"""
    if t is None:
        return None
    g = getattr(t, "guard_ptr", None)
    if g is not None:
        return g
    assert t.is_cuda and t.is_contiguous()
    return t.data_ptr() or None


def cu(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)) if isinstance(a, np.ndarray) else a
    t = t.detach().contiguous().cuda()
    return t if dtype is None else t.to(dtype)


def table(ts):
    """a host array of device pointers (None -> NULL table; a None entry -> NULL)"""
    return None if ts is None else (C.c_void_p * len(ts))(*[None if t is None else t.data_ptr() for t in ts])


def bits(t):
    t = t.detach().contiguous()
    return t.view(I32) if t.dtype == F32 else t


class Bufs:
    """the guarded buffers of one call under one fill"""

    def __init__(self, fill):
        self.fill, self.dev, self.checks = fill, torch.device("cuda"), []

    def scratch(self, nbytes, zero_words=(), align=256):
        """-> the address of a guarded scratch of exactly nbytes bytes"""
        _view, chk = guarded(int(nbytes), self.fill, self.dev, align=align, zero_words=zero_words)
        self.checks.append((f"scratch of {int(nbytes)} bytes", chk))
        return chk.ptr

    def out(self, shape, dtype=F32):
        t, chk = guarded_out(shape, dtype, self.dev)
        t.guard_ptr = chk.ptr
        self.checks.append((f"output {tuple(t.shape)} {dtype}", chk))
        return t

    def done(self, what):
        torch.cuda.synchronize()
        for name, chk in self.checks:
            chk(f"{what}, fill {self.fill:#04x}, {name}")
            chk.restored(f"{what}, fill {self.fill:#04x}, {name}")


def across_fills(what, run, exact=True, each=None, fills=FILLS):
    """run(B) -> {name: output tensor} once per fill; the guards of every buffer of B; exact: the outputs of all fills equal bit for bit
    (whole tensors, the bytes a call leaves unwritten included); each: called on every fill's outputs (the bar of a non-deterministic
    entry).  -> the outputs of the 0xFF fill"""
    res = {}
    for fill in fills:
        B = Bufs(fill)
        outs = run(B)
        B.done(what)
        res[fill] = outs
        if each is not None:
            each(outs, fill)
    first = res[fills[0]]
    if exact:
        for fill in fills[1:]:
            for k, t in first.items():
                assert torch.equal(bits(t), bits(res[fill][k])), \
                    f"{what}: output {k} under fill {fill:#04x} differs from fill {fills[0]:#04x}: the scratch contents reached the result"
    return res[0xFF] if 0xFF in res else first


def _cloud(n, seed, span=1.0):
    return np.random.default_rng(seed).uniform(-span, span, (n, 3)).astype(np.float32)


# ================================================================================================ nearest neighbours (csplat_knn.hip)
@pytest.mark.parametrize("n", [4, 1023, 1024, 1025, 4097])          # KNN_BOX = 1024: one box, its edges, five boxes
def test_dist2_ws(n):
    """csplat_dist2_ws == csplat_dist2 (the brute-force entry) bit for bit, whatever the temp held"""
    nat, pts = _n(), cu(_cloud(n, n))
    want = torch.full((n,), -1.0, device="cuda")
    call("csplat_dist2", n, P(pts), P(want))

    def run(B):
        out = B.out(n)
        call("csplat_dist2_ws", n, P(pts), P(out), B.scratch(nat.lib.csplat_dist2_temp_bytes(n)))
        return dict(out=out)
    got = across_fills(f"csplat_dist2_ws P {n}", run)
    assert torch.equal(bits(got["out"]), bits(want))


@pytest.mark.parametrize("K", [1, 32])
@pytest.mark.parametrize("n", [1, 2, 65, 1024, 1025, 4097])
def test_knn_ws(n, K):
    """csplat_knn_ws == csplat_knn in distances and indices (P = 1, 2: slots without a neighbour hold +inf / -1)"""
    nat, pts = _n(), cu(_cloud(n, 10 * n + K))
    want_d, want_i = torch.full((n, K), -1.0, device="cuda"), torch.full((n, K), -7, dtype=I32, device="cuda")
    call("csplat_knn", n, K, P(pts), P(want_d), P(want_i))

    def run(B):
        d2, idx = B.out((n, K)), B.out((n, K), I32)
        call("csplat_knn_ws", n, K, P(pts), P(d2), P(idx), B.scratch(nat.lib.csplat_knn_temp_bytes(n, K)))
        return dict(d2=d2, idx=idx)
    got = across_fills(f"csplat_knn_ws P {n} K {K}", run)
    assert torch.equal(bits(got["d2"]), bits(want_d)) and torch.equal(got["idx"], want_i)
    if n <= K:
        assert bool(torch.isinf(got["d2"][:, n - 1:]).all()) and bool((got["idx"][:, n - 1:] == -1).all())


@pytest.mark.parametrize("Q,N,K", [(1, 1, 1), (257, 1025, 8), (4097, 1024, 32), (300, 5, 32)])
def test_knn_query_ws(Q, N, K):
    """csplat_knn_query_ws == csplat_knn_query in distances and indices"""
    nat = _n()
    q, p = cu(_cloud(Q, Q + N)), cu(_cloud(N, Q + N + 1, 0.8))
    want_d, want_i = torch.full((Q, K), -1.0, device="cuda"), torch.full((Q, K), -7, dtype=I32, device="cuda")
    call("csplat_knn_query", Q, N, K, P(q), P(p), P(want_d), P(want_i))

    def run(B):
        d2, idx = B.out((Q, K)), B.out((Q, K), I32)
        call("csplat_knn_query_ws", Q, N, K, P(q), P(p), P(d2), P(idx), B.scratch(nat.lib.csplat_knn_query_temp_bytes(Q, N, K)))
        return dict(d2=d2, idx=idx)
    got = across_fills(f"csplat_knn_query_ws Q {Q} N {N} K {K}", run)
    assert torch.equal(bits(got["d2"]), bits(want_d)) and torch.equal(got["idx"], want_i)


@pytest.mark.parametrize("only_points", [False, True], ids=["both_outputs", "dL_dpoints_only"])
@pytest.mark.parametrize("Q,N", [(1, 1), (257, 300), (4097, 7)])
def test_chamfer_bwd(Q, N, only_points):
    """csplat_chamfer_bwd (a stable sort of (idx, i) in the temp, one lane per run): reproducible bit for bit, so equal across fills;
    values under the per-component bound of tests/chamfer_ref.py, as tests/test_chamfer_gpu.py holds them"""
    import chamfer_ref
    from test_chamfer_gpu import _check_direction
    nat = _n()
    a, b = _cloud(Q, 3 * Q + N), _cloud(N, 3 * Q + N + 1)
    q, p = cu(a), cu(b)
    d2, idx = torch.empty(Q, device="cuda"), torch.empty(Q, dtype=I32, device="cuda")
    call("csplat_knn_query", Q, N, 1, P(q), P(p), P(d2), P(idx))
    d2_h = d2.cpu().numpy()
    cap = float(np.sort(d2_h)[Q // 2])                      # one of the float32 distances: the <= edge
    g = torch.tensor([0.37], device="cuda")

    def run(B):
        dq = None if only_points else B.out((Q, 3))
        dp = B.out((N, 3))
        call("csplat_chamfer_bwd", Q, N, P(q), P(p), P(d2), P(idx), cap, P(g), P(dq), P(dp),
             B.scratch(nat.lib.csplat_chamfer_bwd_temp_bytes(Q, N)))
        return dict(dp=dp) if only_points else dict(dq=dq, dp=dp)
    got = across_fills(f"csplat_chamfer_bwd Q {Q} N {N}", run)
    r = chamfer_ref.direction(a, b, idx.cpu().numpy(), d2_h, cap, g=float(np.float32(0.37)))
    _check_direction(f"Q {Q} N {N}", None if only_points else got["dq"].cpu().numpy(), got["dp"].cpu().numpy(), r)


# ================================================================================================ kNN-graph regularisers
@pytest.mark.parametrize("N,K", [(1, 1), (257, 5), (4097, 32)])
def test_knn_regs_graph(N, K):
    """csplat_knn_regs_graph (integer counts, csplat_scan, a stable csplat_sort_pairs in the temp): the reverse lists equal the stable
    argsort of tests/knn_regs_ref.py; d0 / w within the 2 ulp of tests/test_knn_regs_gpu.py (from_points)"""
    import knn_regs_ref
    nat = _n()
    rng = np.random.default_rng(N + K)
    idx_h = rng.integers(0, N, (N, K)).astype(np.int32)
    idx_h[: N // 3] = 0                                       # a hub: one long reverse run
    d2_h = rng.uniform(1e-3, 0.5, (N, K)).astype(np.float32)
    idx, d2, lam = cu(idx_h), cu(d2_h), 20.0

    def run(B):
        d0, w, off, ent = B.out((N, K)), B.out((N, K)), B.out(N + 1, I32), B.out(N * K, I32)
        call("csplat_knn_regs_graph", N, K, P(idx), P(d2), lam, P(d0), P(w), P(off), P(ent),
             B.scratch(nat.lib.csplat_knn_regs_graph_temp_bytes(N, K)))
        return dict(d0=d0, w=w, off=off, ent=ent)
    got = across_fills(f"csplat_knn_regs_graph N {N} K {K}", run)
    off, ent = knn_regs_ref.reverse_lists(idx_h, N)
    assert np.array_equal(got["off"].cpu().numpy(), off) and np.array_equal(got["ent"].cpu().numpy(), ent)
    d64 = d2_h.astype(np.float64)
    for name, ref in (("d0", np.sqrt(d64)), ("w", np.exp(-lam * d64))):
        ulps = np.abs(got[name].cpu().numpy().astype(np.float64) - ref) / np.spacing(ref.astype(np.float32)).astype(np.float64)
        assert ulps.max() <= 2.0, (name, float(ulps.max()))


@pytest.mark.parametrize("T", [1, 3])
def test_knn_regs_fwd(T):
    """csplat_knn_regs_fwd at (N, K) = (257, 5) (two workgroups; T = 1: no spring, no rigidity), scratch "any contents": the four loss
    words equal across fills, each within 4 e32 + 4 u of float64 (the bar of tests/test_knn_regs_gpu.py:compare)"""
    import knn_regs_ref as R
    import test_knn_regs_gpu as TK
    nat = _n()
    N, K, lams = 257, 5, TK.ALL
    pts, M, Q = TK.rows(N, T, "near", seed=N + 7 * K + T)
    graph = TK.knn_graph(pts, K)
    Mc, Qc = cu(M), cu(Q)

    def run(B):
        out4 = B.out(4)
        call("csplat_knn_regs_fwd", T, N, K, P(Mc), P(Qc), P(graph.idx32), P(graph.d0), P(graph.w), lams[0], lams[1], lams[2], 0, P(out4),
             B.scratch(nat.lib.csplat_knn_regs_fwd_scratch_bytes(), align=16))
        return dict(out4=out4)
    got = across_fills(f"csplat_knn_regs_fwd T {T}", run)["out4"].cpu().numpy().astype(np.float64)
    idx, d0, w = graph.idx.cpu().numpy(), graph.d0.cpu().numpy(), graph.w.cpu().numpy()
    r64, r32 = R.evaluate(M, Q, idx, d0, w, lams), R.evaluate(M, Q, idx, d0, w, lams, dtype=F32)
    for word, g, x32, x64 in [(f"part {m}", got[m], r32["parts"][m], r64["parts"][m]) for m in range(3)] + [("L", got[3], r32["loss"], r64["loss"])]:
        e32, ek = R.scale_err(x32, x64), R.scale_err(g, x64)
        assert ek <= 4 * e32 + 4 * R.U, f"T {T} {word}: kernel error {ek:.3e} beyond 4 e32 + 4 u = {4 * e32 + 4 * R.U:.3e}"


# ================================================================================================ compaction map
@pytest.mark.parametrize("kind", ["zeros", "ones", "alternating"])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 4097, 70_001])
def test_mask_to_map(n, kind):
    """csplat_mask_to_map == the stable compaction map (integers: equality), base 11"""
    nat = _n()
    m = {"zeros": np.zeros(n, np.uint8), "ones": np.full(n, 255, np.uint8), "alternating": (np.arange(n) % 2).astype(np.uint8)}[kind]
    mask, base = cu(m), 11

    def run(B):
        mp, cnt = B.out(n, I32), B.out(1, I32)
        call("csplat_mask_to_map", n, P(mask), base, P(mp), P(cnt), B.scratch(nat.lib.csplat_mask_to_map_temp_bytes(n)))
        return dict(map=mp, count=cnt)
    got = across_fills(f"csplat_mask_to_map n {n} {kind}", run)
    sel = m != 0
    want = np.where(sel, base + np.cumsum(sel) - sel, -1).astype(np.int32)
    assert np.array_equal(got["map"].cpu().numpy(), want) and int(got["count"]) == int(sel.sum())


# ================================================================================================ simulator kernels (csplat_sim.hip)
def _SR():
    import sim_rollout_ref as R
    import test_sim_rollout_kernels_gpu as SR
    return SR, R


@pytest.mark.parametrize("Rr", [1, 5, 8193, 32769])                  # sim_rollout_ref.ROWS_DOT_BWD_R
def test_rows_dot(Rr):
    """csplat_rows_dot_bwd, scratch "contents irrelevant": dW, db, dh for every T of tests/test_sim_rollout_kernels_gpu.py equal across
    fills; the 0xFF run under that file's check(); csplat_rows_dot_fwd (no scratch) into a guarded output"""
    SR, R = _SR()
    assert (Rr in R.ROWS_DOT_BWD_R) and tuple(R.ROWS_DOT_T) == tuple(range(1, 9))
    nat = _n()
    h8, W, b, add, dy = R.rows_dot_case(Rr)
    Wc, bc, W64 = cu(W), cu(b), W.double()
    for T in R.ROWS_DOT_T:
        hc, dyc, ac = cu(h8[:T]), cu(dy[:T]), cu(add[:T])

        def run(B):
            y = B.out((T, Rr))
            call("csplat_rows_dot_fwd", T, Rr, 256, P(Wc), P(bc), P(hc), P(y), P(ac))
            dW, db, dh = B.out((Rr, 256)), B.out(Rr), B.out((T, 256))
            call("csplat_rows_dot_bwd", T, Rr, 256, P(Wc), P(hc), P(dyc), P(dW), P(db), P(dh),
                 B.scratch(nat.lib.csplat_rows_dot_scratch_bytes(T), align=16))
            return dict(y=y, dW=dW, db=db, dh=dh)
        got = across_fills(f"csplat_rows_dot T {T} R {Rr}", run)
        SR.check("rows_dot fwd", f"contracts T {T} R {Rr}", got["y"], R.rows_dot(h8[:T], W64, b, add[:T], F64),
                 R.rows_dot(h8[:T], W, b, add[:T], F32), 1e-30)
        r64, r32 = R.rows_dot_grads(h8[:T], W64, dy[:T], F64), R.rows_dot_grads(h8[:T], W, dy[:T], F32)
        dmax, hmax = float(dy[:T].abs().max()), float(h8[:T].abs().max())           # (the units of test_rows_dot_backward_every_T)
        for name, a, c, unit in zip(("dW", "db", "dh"), r64, r32, (dmax * hmax, dmax, 1e-30)):
            SR.check(f"rows_dot bwd {name}", f"contracts T {T} R {Rr}", got[name], a, c, unit)


def test_sim_hidden_one_buffer_for_every_T():
    """csplat_sim_hidden_bwd: first word (the ticket) zero on entry and left at zero, everything else hostile; ONE buffer of the T = 8
    size serves T = 1, 3, 8 in a row"""
    SR, R = _SR()
    nat, K0 = _n(), 13
    e8, W1, b1, W2, b2, dh2 = R.sim_hidden_case(K0)
    W1c, b1c, W2c, b2c = cu(W1), cu(b1), cu(W2), cu(b2)
    nbytes = int(nat.lib.csplat_sim_hidden_scratch_bytes(8))
    assert all(int(nat.lib.csplat_sim_hidden_scratch_bytes(T)) <= nbytes for T in (1, 3, 8))
    res = {}
    for fill in FILLS:
        B = Bufs(fill)
        sp = B.scratch(nbytes, zero_words=[0], align=16)
        res[fill] = {}
        for T in (1, 3, 8):
            ec = cu(e8[:T])
            h1, h2 = SR._sim_fwd(T, K0, ec, W1c, b1c, W2c, b2c)
            outs = [B.out((256, K0)), B.out(256), B.out((256, 256)), B.out(256)]
            call("csplat_sim_hidden_bwd", T, K0, P(ec), P(W2c), P(h1), P(h2), P(cu(dh2[:T])), *[P(o) for o in outs], sp)
            B.done(f"csplat_sim_hidden_bwd T {T}")             # (guards, and the ticket back at zero, after EVERY call)
            res[fill][T] = outs
    for T in (1, 3, 8):
        for fill in FILLS[1:]:
            for a, c in zip(res[FILLS[0]][T], res[fill][T]):
                assert torch.equal(bits(a), bits(c)), f"T {T} fill {fill:#04x}: the scratch contents reached the result"
        g64, g32 = R.sim_hidden_grads(e8[:T], W1, b1, W2, b2, dh2[:T], F64), R.sim_hidden_grads(e8[:T], W1, b1, W2, b2, dh2[:T], F32)
        for name, a, c, d in zip(("dW1", "db1", "dW2", "db2"), res[0xFF][T], g64, g32):
            SR.check(f"sim_hidden bwd {name}", f"contracts T {T}", a, c, d, 1e-30)


@pytest.mark.parametrize("T,V,E", [(3, 22001, 22003), (4, 300, 2000)])   # test_cloth_regs_ticket_and_scratch_across_sizes
def test_cloth_regs_exact_size(T, V, E):
    """csplat_cloth_regs, both forms: the header wants the scratch ZERO before the first call, so the fill is 0x00 only -- what is
    checked is the exact size (guards in front and behind), the ticket back at zero, and the values under the owning file's check()"""
    from csplat import train as tr
    SR, R = _SR()
    nat = _n()
    D, ei, rest, _info = R.regs_case(T, V, E)
    Dc, eic, restc = cu(D), cu(ei), cu(rest)
    csr = tr.edge_csr(eic, V)
    lams = R.REGS_LAMBDAS[0]
    nbytes = int(nat.lib.csplat_cloth_regs_scratch_bytes(T, V, E))
    (l64, g64), (l32, g32) = R.cloth_regs(D, ei, rest, *lams, dtype=F64), R.cloth_regs(D, ei, rest, *lams, dtype=F32)
    B = Bufs(0x00)
    sp = B.scratch(nbytes, zero_words=[-64])                   # the ticket word opens the last 256 bytes
    for form, c in (("scatter", None), ("csr", csr), ("scatter", None), ("csr", csr)):
        loss, grad = B.out(1), B.out((T, V, 3))
        call("csplat_cloth_regs", T, V, E, P(Dc), P(eic), P(restc), *[float(v) for v in lams], P(loss), P(grad), sp,
             *([None] * 4 if c is None else [t.data_ptr() for t in c]))
        B.done(f"csplat_cloth_regs ({T}, {V}, {E}) {form}")
        SR.check(f"cloth_regs {form} loss", f"contracts ({T}, {V}, {E})", loss[0], l64, l32, 1e-30)
        SR.check(f"cloth_regs {form} grad", f"contracts ({T}, {V}, {E})", grad, g64, g32, 1e-30)


# ================================================================================================ image kernels (csplat_image.hip)
def _TK():
    import test_train_kernels_gpu as TK
    import train_kernels_ref as R
    return TK, R


def _psnr_case(n_images, n_per_image, offset_floats=0):
    TK, R = _TK()
    nat = _n()
    gen = torch.Generator(device="cuda").manual_seed(n_images * 7 + n_per_image)
    store = [torch.rand(n_images * n_per_image + 4, device="cuda", generator=gen) for _ in range(2)]
    a, b = (s[offset_floats:offset_floats + n_images * n_per_image].view(n_images, n_per_image) for s in store)
    assert a.data_ptr() % 16 == 4 * offset_floats

    def run(B):
        out = B.out(n_images)
        call("csplat_psnr", n_images, n_per_image, P(a), P(b), B.scratch(nat.lib.csplat_psnr_scratch_bytes(n_images)), P(out))
        return dict(out=out)
    got = across_fills(f"csplat_psnr {n_images} x {n_per_image}", run)
    # (the restatement of tests/train_kernels_ref.py evaluated where the data lie: 67 M values at the largest case)
    TK.check("psnr contracts", f"{n_images} x {n_per_image}", got["out"].reshape(-1, 1), R.psnr(a, b, F64).cpu(), R.psnr(a, b, F32).cpu(), 1.0)


@pytest.mark.parametrize("n_per_image", [1, 5, 4099, 64 * 4096 + 3])
@pytest.mark.parametrize("n_images", [1, 3, 257])
def test_psnr(n_images, n_per_image):
    """csplat_psnr clears its tickets itself: a scratch of any contents gives the same bits (fixed summation order), and the last
    workgroup to arrive at an image does fire (a ticket that starts at 0xFFFFFFFF or 0x7F7F7F7F would never reach its count)"""
    _psnr_case(n_images, n_per_image)


def test_psnr_off_the_16_byte_boundary():
    """both images start 4 bytes behind a 16-byte boundary"""
    _psnr_case(3, 4099, offset_floats=1)


def _image_inputs(shape, mc):
    TK, R = _TK()
    x, y, _ = R.image_case("uniform", shape, 0, seed=sum(shape))
    mask = None
    if mc:
        mask = R.make_mask(shape, mc, 3)
        if shape[2] * shape[3] == 1:
            mask.fill_(0.5)                                      # (make_mask leaves the only pixel of a 1 x 1 image at 1)
    return x, y, mask


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("shape", [(1, 1, 1, 1), (3, 1, 5, 3), (1, 3, 16, 63), (1, 1, 17, 64), (3, 3, 17, 129)])   # R.SSIM_ABI_SHAPES
def test_image_loss(shape, masked):
    """csplat_image_loss_fwd / _bwd, scratch "no initial state", bit-reproducible: the four output words, the partial-derivative images,
    the sign bytes and d/dx equal across fills; the 0xFF run under the bars of test_fused_image_loss_every_kind_of_image"""
    TK, R = _TK()
    assert list(R.SSIM_ABI_SHAPES) == [(1, 1, 1, 1), (3, 1, 5, 3), (1, 3, 16, 63), (1, 1, 17, 64), (3, 3, 17, 129)]
    nat = _n()
    Bn, Cc, H, W = shape
    mc = 1 if masked else 0
    x, y, mask = _image_inputs(shape, mc)
    xc, yc, mk = cu(x), cu(y), (None if mask is None else cu(mask))
    add, g = torch.tensor([TK.ADD], device="cuda"), torch.tensor([TK.UP], device="cuda")
    taps = TK._taps11()

    def run(B):
        p = [B.out(shape) for _ in range(3)]
        sign8, out, dx = B.out(shape, torch.int8), B.out(4), B.out(shape)
        call("csplat_image_loss_fwd", Bn, Cc, H, W, taps, P(xc), P(yc), P(mk), mc, TK.LAM, TK.W_IMG, P(add), TK.W_ADD, TK.PS, *[P(t) for t in p],
             P(sign8), B.scratch(nat.lib.csplat_image_loss_scratch_bytes(Bn, Cc, H, W)), P(out))
        call("csplat_image_loss_bwd", Bn, Cc, H, W, taps, P(xc), P(yc), *[P(t) for t in p], P(sign8), P(mk), mc, TK.LAM, TK.W_IMG, P(g), P(dx))
        return dict(p1=p[0], p2=p[1], p3=p[2], sign8=sign8, out=out, dx=dx)
    got = across_fills(f"csplat_image_loss {shape} masked {masked}", run)
    r64, r32 = (TK._ref_image_loss(x, y, mask, True, dt) for dt in (F64, F32))
    where = f"contracts {shape} mask {mc}"
    TK.check("image_loss contracts", f"{where} loss", got["out"][0], r64["loss"], r32["loss"], TK.W_IMG * TK.LAM)
    TK.check("image_loss contracts", f"{where} image_loss", got["out"][2], r64["il"], r32["il"], TK.LAM)
    TK.check("image_loss contracts psnr", f"{where} psnr", got["out"][1], r64["psnr"], r32["psnr"], 1.0)
    TK.check("image_loss contracts d/dx", f"{where} d/dx", got["dx"], r64["dx"], r32["dx"], TK.UP * TK.W_IMG / x.numel())


@pytest.mark.parametrize("shape", [(1, 1, 1, 1), (3, 1, 5, 3), (1, 3, 16, 63), (1, 1, 17, 64), (3, 3, 17, 129)])   # R.SSIM_ABI_SHAPES
def test_ssim_fwd_masked_outputs(shape):
    """csplat_ssim_fwd_masked takes no scratch: its five outputs (csplat_ssim_partial_count floats of partial sums among them) between
    guards, equal to the call of tests/test_train_kernels_gpu.py bit for bit, the value under that test's bar"""
    TK, R = _TK()
    nat = _n()
    Bn, Cc, H, W = shape
    x, y, _ = _image_inputs(shape, 0)
    xc, yc = cu(x), cu(y)
    for mc in sorted({1, Cc}):
        mask = _image_inputs(shape, mc)[2]
        mk = cu(mask)
        B = Bufs(0xFF)
        p, mp = [B.out(shape) for _ in range(3)], B.out(shape)
        partial = B.out(int(nat.lib.csplat_ssim_partial_count(Bn * Cc, H, W)))
        call("csplat_ssim_fwd_masked", Bn, Cc, H, W, TK._taps11(), P(xc), P(yc), P(mk), mc, *[P(t) for t in p], P(mp), P(partial))
        B.done(f"csplat_ssim_fwd_masked {shape} mask planes {mc}")
        p_ref, _, partial_ref = TK._ssim_fwd_abi(x, y, mask)
        assert torch.equal(bits(torch.stack(p)), bits(p_ref)) and torch.equal(bits(partial), bits(partial_ref))
        v = [((1.0 - R.ssim_map(x.to(dt), y, dt)) * mask.to(dt)).mean() for dt in (F64, F32)]
        TK.check("ssim abi masked contracts", f"{shape} mask planes {mc}", partial.double().sum() / x.numel(), v[0], v[1], 1.0)


def _l1_scratch(B):
    return B.scratch(_n().lib.csplat_l1_scratch_bytes(), zero_words=[-1])      # "last word zero on entry (the kernel restores it)"


@pytest.mark.parametrize("n", [1, 3, 4, 5, 4097, 3_145_728, 3_145_732, 7_680_000, 7_680_003])      # R.L1_SIZES
def test_l1(n):
    """csplat_l1: scratch hostile but for its last word, which is zero on entry and zero again after the call; loss and gradient equal
    across fills (fixed summation order), the 0xFF run under the bars of l1_case"""
    TK, R = _TK()
    assert n in R.L1_SIZES
    gen = torch.Generator().manual_seed(n)
    x, y = torch.rand(n, generator=gen), torch.rand(n, generator=gen)
    xc, yc = cu(x), cu(y)

    def run(B):
        loss, grad = B.out(1), B.out(n)
        call("csplat_l1", n, P(xc), P(yc), _l1_scratch(B), P(loss), P(grad))
        return dict(loss=loss, grad=grad)
    got = across_fills(f"csplat_l1 n {n}", run)
    (v64, g64), (v32, g32) = TK._ref_l1(x, y, None, F64), TK._ref_l1(x, y, None, F32)      # (the gradient of 2.5 * loss)
    TK.check("l1 contracts", f"n {n} value", got["loss"][0], v64, v32, 1e-30)
    TK.check("l1 contracts", f"n {n} d/dx", 2.5 * got["grad"].double(), g64, g32, 2.5 / n)


@pytest.mark.parametrize("shape,mc", [((4, 3, 800, 800), 1), ((4, 3, 800, 800), 3), ((4, 3, 801, 803), 1), ((4, 3, 801, 803), 3), ((3, 3, 37, 53), 1)])
def test_l1_masked_and_signs(shape, mc):
    """csplat_l1_masked and csplat_l1_signs (+ csplat_l1_signs_bwd, which takes no scratch) at R.L1_MASKED: as test_l1; the two forms
    give the same loss bits, and sign8 * mask / n is the float gradient"""
    TK, R = _TK()
    assert (shape, mc) in [tuple(c) for c in R.L1_MASKED]
    Bn, Cc, H, W = shape
    hw, n = H * W, Bn * Cc * H * W
    x, y, mask = R.image_case("uniform", shape, mc, seed=sum(shape))
    xc, yc, mk = cu(x), cu(y), cu(mask)
    g = torch.tensor([2.5], device="cuda")

    def run(B):
        loss, grad = B.out(1), B.out(shape)
        call("csplat_l1_masked", Bn, Cc, hw, P(xc), P(yc), P(mk), mc, _l1_scratch(B), P(loss), P(grad))
        loss2, sign8, back = B.out(1), B.out(shape, torch.int8), B.out(shape)
        call("csplat_l1_signs", Bn, Cc, hw, P(xc), P(yc), P(mk), mc, _l1_scratch(B), P(loss2), P(sign8))
        call("csplat_l1_signs_bwd", Bn, Cc, hw, P(sign8), P(mk), mc, P(g), P(back))
        return dict(loss=loss, grad=grad, loss2=loss2, sign8=sign8, back=back)
    got = across_fills(f"csplat_l1_masked / _signs {shape} mask planes {mc}", run)
    assert torch.equal(bits(got["loss"]), bits(got["loss2"]))
    (v64, g64), (v32, g32) = TK._ref_l1(x, y, mask, F64), TK._ref_l1(x, y, mask, F32)
    TK.check("l1 contracts", f"{shape} mask {mc} value", got["loss"][0], v64, v32, 1e-30)
    TK.check("l1 contracts", f"{shape} mask {mc} d/dx", 2.5 * got["grad"].double(), g64, g32, 2.5 / n)
    TK.check("l1 contracts", f"{shape} mask {mc} signs d/dx", got["back"], g64, g32, 2.5 / n)


# ================================================================================================ geometry and flow losses
@pytest.mark.parametrize("variant", ["both", "z_holes"])
@pytest.mark.parametrize("shape", [(1, 1, 1), (1, 1, 3), (2, 3, 5), (1, 1, 255), (1, 1, 256), (1, 1, 257), (1, 16, 65), (1, 32, 32), (1, 4, 257),
                                   (3, 64, 64), (17, 4, 4)], ids=str)                               # test_geometry_loss_gpu.SMALL
def test_geom_loss(shape, variant):
    """csplat_geom_loss_fwd / _bwd, scratch "no initial state", bit-reproducible (17 views: two launches of 16 and 1 on one scratch):
    the three loss words, the sign bytes and both gradient images equal across fills; the 0xFF run through compare() of
    tests/test_geometry_loss_gpu.py"""
    import test_geometry_loss_gpu as TG
    assert shape in TG.SMALL
    nat = _n()
    c = TG.make_case(shape, variant)
    V, H, W = shape
    tabs = {k: TG._to_gpu(c[k], c["layout"]) for k in ("D", "A", "Z", "S", "M")}
    g = torch.tensor([c["g"]], dtype=F32, device="cuda")

    def run(B):
        out, sign = B.out(3), B.out((V, H, W), U8)
        call("csplat_geom_loss_fwd", V, H * W, *[table(tabs[k]) for k in ("D", "A", "Z", "S", "M")], c["lam_d"], c["lam_s"], c["weight"], None,
             1.0, P(sign), B.scratch(nat.lib.csplat_geom_loss_scratch_bytes(V, H * W)), P(out))
        dD, dA = B.out((V, H, W)), B.out((V, H, W))
        call("csplat_geom_loss_bwd", V, H * W, P(sign), table(tabs["Z"]), table(tabs["M"]), c["lam_d"], c["lam_s"], c["weight"], P(g), P(dD), P(dA))
        return dict(out=out, sign=sign, dD=dD, dA=dA)
    got = across_fills(f"csplat_geom_loss {shape} {variant}", run)
    assert torch.equal(got["sign"].cpu(), TG.restate(c, F64)[5])
    TG.compare("geometry_loss contracts " + variant, c, (got["out"][0], got["out"][1], got["out"][2], got["dD"], got["dA"]))


@pytest.mark.parametrize("Pn,T", [(1, 2), (257, 3)])
def test_flow_loss(Pn, T):
    """csplat_flow_loss_fwd / _bwd on a 37 x 23 image, scratch "no initial state", bit-reproducible: the two loss words, the count, the
    unit gradient and d_points equal across fills; the 0xFF run through compare() of tests/test_flow_loss_gpu.py"""
    import test_flow_loss_gpu as TF
    nat = _n()
    c = TF.make_case(Pn, T, (37, 23), "mask_cap")
    X, full, flows = [x.cuda() for x in c["X"]], [f.cuda() for f in c["full"]], [f.cuda() for f in c["flows"]]
    vis, masks = [v.cuda() for v in c["vis"]], [m.cuda() for m in c["masks"]]
    g = torch.tensor([c["g"]], dtype=F32, device="cuda")

    def run(B):
        unit, out, cnt = B.out((T, Pn, 3)), B.out(2), B.out(1, I32)
        call("csplat_flow_loss_fwd", T, Pn, c["W"], c["H"], table(X), table(full), table(flows), table(vis), table(masks), c["cap"], c["lam"],
             c["weight"], None, 1.0, P(unit), B.scratch(nat.lib.csplat_flow_loss_scratch_bytes(T, Pn)), P(out), P(cnt))
        d = B.out((T, Pn, 3))
        call("csplat_flow_loss_bwd", T, Pn, P(unit), c["lam"], c["weight"], P(g), P(d))
        return dict(unit=unit, out=out, count=cnt, d=d)
    got = across_fills(f"csplat_flow_loss P {Pn} T {T}", run)
    TF.compare("flow_loss contracts", c, SimpleNamespace(total=got["out"][0], L=got["out"][1], count=int(got["count"]), grad=got["d"]))


# ================================================================================================ observation clouds
@pytest.mark.parametrize("which", ["3 views of 37x29", "one 1x1 view"])
def test_obs_unproject(which):
    """csplat_obs_unproject (selection bytes, csplat_mask_to_map and its scan inside the temp): points, source and the count equal across
    fills -- rows beyond the count keep their initial bytes; source and count equal the restatement, points under the owning file's bar"""
    import observation_ref as R
    import test_observation_gpu as TO
    nat = _n()
    if which == "one 1x1 view":
        d, mask = np.full((1, 1, 1), 2.0, np.float32), None
        intr, c2w = np.array([[1.0, 1.0, 0.0, 0.0]], np.float32), np.array([[[1.0, 0, 0, 0], [0, 1.0, 0, 0], [0, 0, 1.0, 0]]], np.float32)
    else:
        d, mask, intr, c2w = TO.depth_case(3, 29, 37, "mixed")
    V, H, W = d.shape
    cap = V * H * W
    dg, mg, kg, cg = cu(d), (None if mask is None else cu(mask)), cu(intr), cu(c2w)

    def run(B):
        pts, source, count = B.out((cap, 3)), B.out(cap, I32), B.out(1, I32)
        call("csplat_obs_unproject", V, H, W, P(dg), P(mg), P(kg), P(cg), 1, 0.0, 0, cap, P(pts), P(source), P(count),
             B.scratch(nat.lib.csplat_obs_unproject_temp_bytes(V, H, W)))
        return dict(points=pts, source=source, count=count)
    got = across_fills(f"csplat_obs_unproject {which}", run)
    r32, src, _view = R.unproject(d, intr, c2w, mask, 1, 0.0, 0, np.float32)
    r64 = R.unproject(d, intr, c2w, mask, 1, 0.0, 0, np.float64)[0]
    k = len(src)
    assert int(got["count"]) == k > 0 and np.array_equal(got["source"][:k].cpu().numpy(), src)
    TO.check("observation unproject contracts", which, got["points"][:k], r64, r32, 1.0)


@pytest.mark.parametrize("M", [1, 257, 4097])
def test_obs_voxel(M):
    """csplat_obs_voxel (a u64 sort, a head-flag scan and a segment reduction inside the temp; origin found on the device): every output
    equal across fills; counts, inverse and the voxel count equal the restatement, centroids under the owning file's bar"""
    import observation_ref as R
    import test_observation_gpu as TO
    nat = _n()
    pts = _cloud(M, M)
    pg = cu(pts)

    def run(B):
        cen, cnt, inv, nv, no = B.out((M, 3)), B.out(M, I32), B.out(M, I32), B.out(1, I32), B.out(1, I32)
        call("csplat_obs_voxel", M, P(pg), 0.4, None, P(cen), P(cnt), P(inv), P(nv), P(no), B.scratch(nat.lib.csplat_obs_voxel_temp_bytes(M)))
        return dict(centroids=cen, counts=cnt, inverse=inv, n_voxels=nv, n_outside=no)
    got = across_fills(f"csplat_obs_voxel M {M}", run)
    r32, r64 = R.voxel(pts, 0.4, None, np.float32), R.voxel(pts, 0.4, None, np.float64)
    k = len(r32["counts"])
    assert int(got["n_voxels"]) == k and int(got["n_outside"]) == 0
    assert np.array_equal(got["counts"][:k].cpu().numpy(), r32["counts"]) and np.array_equal(got["inverse"].cpu().numpy(), r32["inverse"])
    TO.check("observation voxel contracts", f"M {M}", got["centroids"][:k], r64["centroids"], r32["centroids"], 1.0)


# ================================================================================================ MeshNet kernels
@pytest.mark.parametrize("N,E", [(1, 0), (3, 5), (900, 20_011)])
def test_gnn_build_csr(N, E):
    """csplat_gnn_build_csr, the entry behind csplat_gnn_csr_temp_bytes: rowptr and perm equal the stable counting sort of
    tests/gnn_kernels_ref.py (integers: equality), whatever the temp held"""
    import gnn_kernels_ref as R
    nat = _n()
    rng = np.random.default_rng(N + E)
    keys_h = rng.integers(0, N, E).astype(np.int64)
    keys_h[: E // 40] = N - 1                                  # a hub of 500 edges (its row is sorted by ONE thread: kept short)
    keys = cu(keys_h)

    def run(B):
        rowptr, perm = B.out(N + 1, I32), B.out(E, I32)
        call("csplat_gnn_build_csr", N, E, P(keys), P(rowptr), P(perm), B.scratch(nat.lib.csplat_gnn_csr_temp_bytes(N, E)))
        return dict(rowptr=rowptr, perm=perm)
    got = across_fills(f"csplat_gnn_build_csr N {N} E {E}", run)
    want_rp, want_pm = R.csr_fast(keys_h, N)
    assert np.array_equal(got["rowptr"].cpu().numpy(), want_rp) and np.array_equal(got["perm"].cpu().numpy(), want_pm)


@pytest.mark.parametrize("M", [1, 63, 64, 65, 16_385, 70_001])
def test_dw128(M):
    """csplat_dw128 and csplat_dw128_bias (deterministic split-K through the workspace): dW and dbias equal across fills; against float64
    relative to sum |g||x| per output <= 2e-6, the bar of tests/test_knn_gnn_gpu.py:test_dw128_vs_fp64"""
    nat = _n()
    gen = torch.Generator().manual_seed(M)
    g, x = torch.randn(M, 128, generator=gen).cuda(), (torch.randn(M, 128, generator=gen) * 2 + 0.3).cuda()
    nbytes = nat.lib.csplat_dw128_workspace_bytes(M)

    def run(B):
        dW, dW2, db = B.out((128, 128)), B.out((128, 128)), B.out(128)
        call("csplat_dw128", M, P(g), P(x), P(dW), B.scratch(nbytes))
        call("csplat_dw128_bias", M, P(g), P(x), 0, P(dW2), P(db), B.scratch(nbytes))
        return dict(dW=dW, dW2=dW2, db=db)
    got = across_fills(f"csplat_dw128 M {M}", run)
    assert torch.equal(bits(got["dW"]), bits(got["dW2"]))
    ref, bound = g.double().t() @ x.double(), (g.double().abs().t() @ x.double().abs()).clamp_min(1e-30)
    assert float(((got["dW"].double() - ref).abs() / bound).max()) < 2e-6
    assert float(((got["db"].double() - g.double().sum(0)).abs() / g.double().abs().sum(0).clamp_min(1e-30)).max()) < 2e-6


@pytest.mark.parametrize("Pn,T", [(1, 1), (257, 3)])
def test_vertex_gather_scratch(Pn, T):
    """the corner scratch of csplat_mesh_transform_bwd_views (csplat/gaussians.py: corner_scratch_floats = T * P * 9 floats, sized in
    Python): the gathered vertex gradients are deterministic, so equal across fills; under the bars of tests/test_mesh_transform_gpu.py"""
    import mesh_transform_ref as M
    import test_mesh_transform_gpu as TM
    from csplat.gaussians import corner_scratch_floats
    nat = _n()
    case = M.branch_case(Pn, T=T, seed=100 * T + Pn)
    pc = TM._model(case)
    r = pc._rest()
    dv = torch.tensor(case["deformed"], device="cuda")
    V = int(dv.shape[1])
    gx, gq = torch.tensor(case["w_xyz"], device="cuda"), torch.tensor(case["w_quat"], device="cuda")
    assert corner_scratch_floats(T, Pn) == T * Pn * 9

    def run(B):
        d_v, d_b, d_r = B.out(tuple(dv.shape)), B.out((Pn, 3)), B.out((Pn, 4))
        call("csplat_mesh_transform_bwd_views", T, Pn, V, P(r[1]), P(dv), P(pc.face_bary.data), P(pc._rotation.data), P(r[2]), P(gx), P(gq),
             P(d_v), P(d_b), P(d_r), P(r[3]), P(r[4]), B.scratch(4 * corner_scratch_floats(T, Pn), align=16))
        return dict(d_vertices=d_v, d_bary=d_b, d_rotation=d_r)
    got = across_fills(f"csplat_mesh_transform_bwd_views P {Pn} T {T}", run)
    r64, r32 = TM.reference(case, q_gpu=TM.run_gather(case, False, False)["quat"])
    for k in ("d_vertices", "d_bary", "d_rotation"):
        TM.check(k, got[k].cpu().numpy(), r64, r32, f"contracts P {Pn} T {T}")


@pytest.mark.parametrize("N,E", [(1, 0), (257, 300)])
def test_edge_length_refine_scratch(N, E):
    """the scratch of csplat_gnn_edge_length_refine (meshnet/rollout.py: refine_scratch_floats = 9 N floats, "contents irrelevant"): an
    odd and an even number of iterations (the double buffer ends in the scratch or in v) equal across fills; under the owning file's bar"""
    from meshnet.graph_ops import GraphCSR
    from meshnet.rollout import refine_scratch_floats
    SR, R = _SR()
    pos, v0, ei, rest, w = R.refine_case(N, E)
    pc, eic, rc, wc = cu(pos), cu(ei), cu(rest), cu(w)
    csr = GraphCSR(eic, N)
    assert refine_scratch_floats(N) == 9 * N
    for iters in (1, 2):
        def run(B):
            v = B.out((N, 3))
            v.copy_(cu(v0))
            call("csplat_gnn_edge_length_refine", N, E, P(pc), P(v), P(eic), P(rc), P(wc), P(csr.rowptr["dst"]), P(csr.perm["dst"]),
                 P(csr.rowptr["src"]), P(csr.perm["src"]), iters, R.REFINE_LR, 0.9, 0.999, 1e-8, B.scratch(4 * refine_scratch_floats(N), align=16))
            return dict(v=v)
        got = across_fills(f"csplat_gnn_edge_length_refine N {N} E {E} iters {iters}", run)
        if E == 0:
            assert torch.equal(bits(got["v"]), bits(cu(v0)))
            continue
        r64, r32 = (R.edge_length_refine(pos, v0, ei, rest, w, iters, R.REFINE_LR, dt) for dt in (F64, F32))
        SR.check("edge_length_refine v", f"contracts N {N} E {E} iters {iters}", got["v"], r64, r32, 1e-30)


# ================================================================================================ the rasterizer
BIT_REPRODUCIBLE = 256
_RASTER = {}


def _raster_case(which):
    """(case, dpix, ddepth, float64 colour gradients, float64 colour + depth gradients), formed once and shared, never changed"""
    if which not in _RASTER:
        import image_sizes_ref
        import test_depth_grad_gpu as TDG
        import test_raster_gpu as TR
        case = util.make_case(**TR.CASES[0]) if which == "first case" else image_sizes_ref.sparse_case("1x1")
        rng = np.random.default_rng(3)
        dpix = rng.normal(size=(3, case["H"], case["W"])).astype(np.float32)
        ddepth = rng.normal(size=(1, case["H"], case["W"])).astype(np.float32)
        o64 = util.oracle_forward(case, dtype=np.float64)
        _RASTER[which] = (case, dpix, ddepth, util.ro.backward(o64, dpix), TDG._oracle(case, dpix, ddepth))
    return _RASTER[which]


OUT_SHAPES = lambda P_, M_: ((P_, 3), (P_, 4), (P_, 1), (P_, 3), (P_, 3), (P_, 6), (P_, M_, 3), (P_, 3), (P_, 4))  # noqa: E731


def _hold_colour_bar(got, g64, Pn, where):
    """the bar of tests/test_raster_gpu.py:_test_backward_grads, restated: 1e-4 of the tensor's largest entry, every Gaussian within 1e-4
    of its own gradient above a floor of 10 %, all but a handful above a floor of 1 %"""
    from test_raster_gpu import TOL
    for k, v in got.items():
        v, ref = v.cpu().numpy(), getattr(g64, k)
        e = util.rel_err(v, ref)
        assert e < TOL, (where, k, e)
        e10, e1 = util.rowwise_rel_err(v, ref, Pn, floor=1e-1), util.rowwise_rel_err(v, ref, Pn, floor=1e-2)
        assert e10.max() < TOL, (where, k, "floor 10 %", float(e10.max()))
        assert (e1 > TOL).sum() <= max(4, 2e-3 * Pn) and e1.max() < 5e-4, (where, k, "floor 1 %", int((e1 > TOL).sum()), float(e1.max()))


@pytest.mark.parametrize("mode", [0, BIT_REPRODUCIBLE], ids=["atomics", "bit_reproducible"])
@pytest.mark.parametrize("entry", ["csplat_backward", "csplat_backward_depth"])
@pytest.mark.parametrize("which", ["first case", "1x1"])
def test_raster_backward(which, entry, mode):
    """csplat_backward / csplat_backward_depth through the direct-call helper of tests/test_raster_backward_dispatch_gpu.py: the flat
    entries do not take CSPLAT_SCRATCH_ZEROED, so their accumulation records may hold anything.  Bit-reproducible mode (the flag is set
    before sizing): all nine outputs equal across fills.  Default mode (float atomics): EVERY fill's run is held to the bar of
    test_backward_grads (colour) / test_depth_and_colour_loss_matches_fp64_autograd (depth)."""
    import test_raster_backward_dispatch_gpu as TD
    from test_depth_grad_gpu import TOL as DEPTH_TOL
    nat = _n()
    case, dpix_h, ddepth_h, g64, g64_depth = _raster_case(which)
    Pn, W, H = case["P"], case["W"], case["H"]
    depth = entry == "csplat_backward_depth"
    old = int(nat.lib.csplat_debug_flags_query())
    try:
        nat.lib.csplat_debug_flags(mode)
        st = TD.forward_state(case, W, H)
        R_, M_ = st.vs.num_rendered, st.vs.M
        nbytes = int(nat.lib.csplat_backward_depth_scratch_bytes(Pn, R_, W, H) if depth else nat.lib.csplat_backward_scratch_bytes(Pn, R_))
        dpix, ddepth = cu(dpix_h), cu(ddepth_h)

        def run(B):
            outs = [B.out(s) for s in OUT_SHAPES(Pn, M_)]
            TD.flat_call(st, entry, dpix, [nat.ptr(ddepth)] if depth else [], B.scratch(nbytes), [P(o) for o in outs])
            return dict(zip(TD.OUT_FIELDS, outs))

        def bar(outs, fill):
            got = dict(mean3D=outs["dL_dmean3D"], mean2D=outs["dL_dmean2D"], opacity=outs["dL_dopacity"].reshape(-1), sh=outs["dL_dsh"],
                       scale=outs["dL_dscale"], rot=outs["dL_drot"])
            where = f"{entry} {which} mode {mode} fill {fill:#04x}"
            if not depth:
                _hold_colour_bar(got, g64, Pn, where)
            else:
                for k, name in (("mean3D", "mean3D"), ("mean2D", "mean2D"), ("opacity", "opacity"), ("sh", "shs"), ("scale", "scales"), ("rot", "rotations")):
                    e = util.rel_err(got[k].cpu().numpy(), g64_depth[name])
                    assert e < DEPTH_TOL, (where, k, e)
        got = across_fills(f"{entry} {which} mode {mode}", run, exact=(mode == BIT_REPRODUCIBLE), each=bar if mode == 0 else None)
        if mode == BIT_REPRODUCIBLE:
            bar(got, 0xFF)
    finally:
        nat.lib.csplat_debug_flags(old)


def test_visibility_views():
    """csplat_visibility_views on one view of the first case of tests/test_raster_gpu.py, scratch "no initial state", bit-reproducible in
    the default mode: the four outputs equal across fills; the 0xFF run against the restatement under the bars of
    tests/test_visibility_gpu.py:test_matches_restatement"""
    import test_raster_backward_dispatch_gpu as TD
    import test_visibility_gpu as TV
    nat = _n()
    case = _raster_case("first case")[0]
    Pn, W, H = case["P"], case["W"], case["H"]
    st = TD.forward_state(case, W, H)
    means3D, sh, colors_precomp, scales, rotations, cov3Ds_precomp, radii, color = st.saved
    stream = nat.stream_handle(torch.device("cuda"))
    w = nat.CsplatView()
    st.vs.fill(w, stream, (means3D, sh, colors_precomp, None, scales, rotations, cov3Ds_precomp, color, radii))
    nbytes = int(nat.lib.csplat_visibility_scratch_bytes(Pn, max(w.layout_rendered, w.num_rendered, 0), W, H))

    def run(B):
        wm, ws, pc, top = B.out(Pn), B.out(Pn), B.out(Pn, I32), B.out((H, W), I32)
        o = (nat.CsplatVisibility * 1)()
        o[0].weight_max, o[0].weight_sum, o[0].pixel_count, o[0].top_id, o[0].scratch = P(wm), P(ws), P(pc), P(top), B.scratch(nbytes)
        nat.check(nat.lib.csplat_visibility_views(1, C.addressof(w), C.cast(o, C.c_void_p), stream), "csplat_visibility_views")
        return dict(weight_max=wm, weight_sum=ws, pixel_count=pc, top_id=top)
    got = {k: v.cpu().numpy() for k, v in across_fills("csplat_visibility_views", run).items()}
    ref = TV._ref(case, top_id=got["top_id"])
    assert util.rel_err(got["weight_max"], ref["weight_max"]) < TV.TOL and util.rel_err(got["weight_sum"], ref["weight_sum"]) < TV.TOL
    d = np.abs(got["pixel_count"].astype(np.int64) - ref["pixel_count"])
    assert d.sum() <= max(4, 1e-3 * ref["pixel_count"].sum()), (int(d.sum()), int(ref["pixel_count"].sum()))
    hit = ref["top_w"] > 0
    assert np.all(ref["at_top"][hit] >= ref["top_w"][hit] - 1e-5)
