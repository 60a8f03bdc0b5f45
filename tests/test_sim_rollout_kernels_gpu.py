"""The small kernels that open every training step and close every rollout step -- csrc/csplat_sim.hip (k_rows_dot_fwd/_bwd/_dh,
k_sim_hidden_fwd/_bwd, k_cloth_regs, k_cloth_regs_csr) and the rollout-step kernels of csrc/csplat_gnn.hip (k_rollout_head/_decode/
_integrate, k_edge_features, k_edge_features_ordered, k_gather_rows_absmax, k_edge_len_adam) -- through the raw C ABI against the float64
restatement tests/sim_rollout_ref.py, at the sizes where each launch takes another path (tests/test_sim_rollout_kernels_cpu.py states
which constant every size crosses) and on the degenerate inputs (zero lengths, exact zeros, hubs, NaN and Inf DATA; no index, size or
pointer is ever garbled).

Bars, by the rule of tests/test_mesh_transform_gpu.py and tests/test_train_kernels_gpu.py.  The same restatement evaluated in float32 on
the CPU has an error e32 against float64 on the same inputs; the kernel must stay within K = 8 x e32, with a floor of 1e-6.  An error is
max |got - ref| over ALL elements divided by the larger of max |ref| and a unit stated at each call of check() (1e-30 = "exactly 0 where
the reference is all 0"; the Adam update: lr).  A bar above 1e-3 means ill-conditioned inputs and fails by itself.  Integer outputs,
copies, single additions, pinned rows, the absmax words (the maximum of values the kernel itself stored) and run-to-run repeats of the
deterministic kernels are compared for EQUALITY.  check() prints e32, the bar and the kernel's error; the module's teardown prints the
table of the largest of each per group (pytest -rP shows it).

What that table showed on an MI355X when this file was written (group | comparisons | largest e32 | largest bar | largest kernel error |
smallest bar / error):
  rows_dot fwd                  | 128 | 6.80e-07 | 5.44e-06 | 4.15e-07 |  8.0      rows_dot bwd dW   | 32 | 1.27e-07 | 1.02e-06 | 1.16e-07 |  8.6
  rows_dot fwd ordinary rows    | 112 | 4.30e-07 | 3.44e-06 | 1.47e-06 |  2.3      rows_dot bwd db   | 32 | 9.42e-08 | 1.00e-06 | 9.42e-08 | 10.6
  rows_dot fwd 1e-4 row         | 112 | 6.20e-06 | 4.96e-05 | 8.77e-06 |  5.7      rows_dot bwd dh   | 32 | 7.24e-06 | 5.79e-05 | 4.24e-07 |  8.0
  rows_dot bwd dW ordinary rows |  24 | 1.16e-07 | 1.00e-06 | 1.16e-07 |  8.6      sim_hidden fwd    | 64 | 2.85e-07 | 2.28e-06 | 1.95e-07 |  5.1
  sim_hidden bwd dW1            |  35 | 4.24e-07 | 3.39e-06 | 1.89e-07 |  7.5      sim_hidden bwd db1 | 35 | 4.01e-07 | 3.21e-06 | 1.81e-07 |  8.9
  sim_hidden bwd dW2            |  35 | 1.73e-07 | 1.38e-06 | 1.70e-07 |  6.1      sim_hidden bwd db2 | 35 | 1.14e-07 | 1.00e-06 | 1.14e-07 |  8.7
  cloth_regs scatter loss       |  54 | 1.48e-07 | 1.18e-06 | 1.29e-07 |  7.8      cloth_regs csr loss | 54 | 1.48e-07 | 1.18e-06 | 1.03e-07 |  9.7
  cloth_regs scatter grad       | 104 | 1.58e-06 | 1.26e-05 | 1.87e-06 |  2.4      cloth_regs csr grad | 104 | 1.58e-06 | 1.26e-05 | 9.01e-07 |  6.8
  SimulatorStep                 |   8 | 8.51e-07 | 6.81e-06 | 1.84e-07 | 10.8      FusedClothRegs tap | 2 | 3.70e-08 | 1.00e-06 | 3.16e-08 | 31.7
  rollout_head                  |  50 | 7.78e-08 | 1.00e-06 | 7.78e-08 | 12.9      rollout_decode    | 50 | 1.77e-07 | 1.42e-06 | 1.34e-07 |  8.8
  edge_features (and ordered)   |   4 | 9.45e-08 | 1.00e-06 | 9.84e-08 | 10.2      edge_length_refine v / update | 6 | 1.39e-07 / 1.70e-06 | 1.11e-06 / 1.36e-05 | = e32 | 8.0
(the scatter form's margin moves with the order of its atomics: 3.3 and 2.4 in two runs.)  No bar is above 6e-5; the CSR regulariser's plain running sum at the vertex of 300 in-edges stays 6.8 times inside its bar.  Wall time 7 s
for the 67 tests (tests/test_knn_gnn_gpu.py in the same session: 60 s); the slowest, test_rows_dot_backward_every_T[32769] at 1.5 s, spends
it converting eight [32 769, 256] gradients to float64 for the comparison."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")       # (before sim_rollout_ref, which imports it)

import util  # noqa: E402,F401
import sim_rollout_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

K, FLOOR, BAR_MAX = 8.0, 1e-6, 1e-3
F64, F32 = torch.float64, torch.float32
SENT = -7.25            # what output buffers hold before a launch
TABLE = {}


@pytest.fixture(scope="module", autouse=True)
def _threads_and_table():
    old = torch.get_num_threads()
    torch.set_num_threads(min(16, old))
    yield
    torch.set_num_threads(old)
    print("\ngroup | comparisons | largest e32 | largest bar | largest kernel error | smallest bar / error")
    for g in sorted(TABLE):
        n, e32, bar, err, margin = TABLE[g]
        print(f"{g} | {n} | {e32:.2e} | {bar:.2e} | {err:.2e} | {margin:.1f}")


def _np(t):
    return t.detach().cpu().double().numpy() if torch.is_tensor(t) else np.asarray(t, np.float64)


def check(group, what, got, r64, r32, unit):
    """got (the kernel), r64, r32 (the restatement in float64 / float32): every element, relative to max(max |r64|, unit)"""
    got, r64, r32 = _np(got), _np(r64), _np(r32)
    assert got.shape == r64.shape == r32.shape, (group, what, got.shape, r64.shape)
    if got.size == 0:
        return
    assert np.isfinite(r64).all() and np.isfinite(got).all(), f"{group} {what}: non-finite values"
    scale = max(float(np.abs(r64).max()), float(unit))
    e32 = float(np.abs(r32 - r64).max()) / scale
    bar = max(K * e32, FLOOR)
    err = float(np.abs(got - r64).max()) / scale
    print(f"{group} | {what}: e32 {e32:.3e} bar {bar:.3e} kernel {err:.3e}")
    n, a, b, c, m = TABLE.get(group, (0, 0.0, 0.0, 0.0, float("inf")))
    TABLE[group] = (n + 1, max(a, e32), max(b, bar), max(c, err), min(m, bar / max(err, 1e-30)))
    assert bar <= BAR_MAX, f"{group} {what}: bar {bar:.3e} > {BAR_MAX}: the inputs are ill-conditioned"
    assert err <= bar, f"{group} {what}: kernel error {err:.3e} > bar {bar:.3e} (float32 restatement: {e32:.3e}; scale {scale:.3e})"


def cuda(t):
    return None if t is None else t.detach().contiguous().cuda()


def P(t):
    """device pointer (None, and an empty tensor: NULL)"""
    if t is None:
        return None
    assert t.is_cuda and t.is_contiguous()
    return t.data_ptr() or None


def call(name, *args):
    from csplat import native as n
    n.check(getattr(n.lib, name)(n.stream_handle(torch.device("cuda")), *args), name)


def bits(t):
    t = t.detach().contiguous()
    return t.view(torch.int32) if t.dtype == F32 else t


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def filled(*shape, value=SENT, dtype=F32):
    return torch.full(shape, value, dtype=dtype, device="cuda")


# ================================================================================================ rows_dot
def _rows_dot_fwd(T, Rr, W, b, h, add):
    y = filled(T, Rr)
    call("csplat_rows_dot_fwd", T, Rr, 256, P(W), P(b), P(h), P(y), P(add))
    return y


@pytest.mark.parametrize("Rr", R.ROWS_DOT_FWD_R)
def test_rows_dot_forward_every_T_and_both_passes(Rr):
    """csplat_rows_dot_fwd: the eight instantiations, with and without the table rows, on either side of the 512 x 16 and 2048 x 16 row
    limits of the grid; row 0 of W at 1e4 and the last at 1e-4, so the ordinary rows and the small row are also measured on their own"""
    h8, W, b, add, _dy = R.rows_dot_case(Rr)
    Wc, bc, W64 = cuda(W), cuda(b), W.double()
    for T in R.ROWS_DOT_T:
        hc = cuda(h8[:T])
        for use_add in (False, True):
            a = add[:T] if use_add else None
            y = _rows_dot_fwd(T, Rr, Wc, bc, hc, cuda(a))
            r64, r32 = R.rows_dot(h8[:T], W64, b, a, F64), R.rows_dot(h8[:T], W, b, a, F32)
            where = f"T {T} R {Rr} add {use_add}"
            check("rows_dot fwd", where, y, r64, r32, 1e-30)                         # unit: none needed, max |y| ~ 1e5 (the 1e4 row)
            if Rr > 2:
                check("rows_dot fwd ordinary rows", where, y[:, 1:Rr - 1], r64[:, 1:Rr - 1], r32[:, 1:Rr - 1], 1e-30)
            if Rr > 1:
                check("rows_dot fwd 1e-4 row", where, y[:, Rr - 1], r64[:, Rr - 1], r32[:, Rr - 1], 1e-30)
            assert same_bits(y, _rows_dot_fwd(T, Rr, Wc, bc, hc, cuda(a)))


def test_rows_dot_forward_empty_calls_write_nothing():
    h8, W, b, _add, _dy = R.rows_dot_case(5)
    Wc, bc, hc = cuda(W), cuda(b), cuda(h8[:3])
    y = filled(3, 5)
    call("csplat_rows_dot_fwd", 0, 5, 256, P(Wc), P(bc), P(hc), P(y), None)
    call("csplat_rows_dot_fwd", 3, 0, 256, P(Wc), P(bc), P(hc), P(y), None)
    assert bool((y == SENT).all())


@pytest.mark.parametrize("Rr", R.ROWS_DOT_BWD_R)
def test_rows_dot_backward_every_T(Rr):
    """csplat_rows_dot_bwd: dW, db and dh for the eight instantiations, below and beyond one 512 x 16-row pass; dh (a fixed-order sum of
    per-workgroup partials) has the same bits on a second call"""
    from csplat import native as n
    h8, W, _b, _add, dy = R.rows_dot_case(Rr)
    Wc, W64 = cuda(W), W.double()
    for T in R.ROWS_DOT_T:
        hc, dyc = cuda(h8[:T]), cuda(dy[:T])
        outs = []
        for _ in range(2):
            dW, db, dh = filled(Rr, 256), filled(Rr), filled(T, 256)
            scratch = torch.empty(int(n.lib.csplat_rows_dot_scratch_bytes(T)), dtype=torch.uint8, device="cuda")
            call("csplat_rows_dot_bwd", T, Rr, 256, P(Wc), P(hc), P(dyc), P(dW), P(db), P(dh), P(scratch))
            outs.append((dW, db, dh))
        for a, c in zip(*outs):
            assert same_bits(a, c)
        r64, r32 = R.rows_dot_grads(h8[:T], W64, dy[:T], F64), R.rows_dot_grads(h8[:T], W, dy[:T], F32)
        # units: one term of the sum over the T time rows (at R = 1 the five cotangents of db cancel to 2 % of one of them); dh is
        # carried by the 1e4 row and needs none
        dmax, hmax = float(dy[:T].abs().max()), float(h8[:T].abs().max())
        for name, got, a, c, unit in zip(("dW", "db", "dh"), outs[0], r64, r32, (dmax * hmax, dmax, 1e-30)):
            check(f"rows_dot bwd {name}", f"T {T} R {Rr}", got, a, c, unit)
        if Rr > 2:      # dh without the 1e4 row's share is not observable; dW row by row is
            check("rows_dot bwd dW ordinary rows", f"T {T} R {Rr}", outs[0][0][1:Rr - 1], r64[0][1:Rr - 1], r32[0][1:Rr - 1], dmax * hmax)


def test_rows_dot_nan_and_inf_poison_exactly_what_reads_them():
    Rr, T = 8193, 3
    h8, W, b, _add, _dy = R.rows_dot_case(Rr)
    Wc, bc = cuda(W), cuda(b)
    clean = _rows_dot_fwd(T, Rr, Wc, bc, cuda(h8[:T]), None)
    h = h8[:T].clone()
    h[1, 77] = float("nan")
    y = _rows_dot_fwd(T, Rr, Wc, bc, cuda(h), None)
    assert bool(torch.isnan(y[1]).all()) and same_bits(y[[0, 2]], clean[[0, 2]])
    r0 = 4097
    W2 = W.clone()
    W2[r0, 5] = float("inf")
    y = _rows_dot_fwd(T, Rr, cuda(W2), bc, cuda(h8[:T]), None)
    keep = torch.arange(Rr, device="cuda") != r0
    assert not bool(torch.isfinite(y[:, r0]).any()) and same_bits(y[:, keep], clean[:, keep])


def test_rows_dot_misaligned_operands_are_copied_by_the_wrappers_and_refused_by_the_entry():
    """W, h, dW and the scratch are read as float4: the entry refuses a pointer off a 16-byte boundary; RowsDot and SimResidual copy such
    an operand (a view one float into a larger buffer) and give the bits of the aligned call"""
    from csplat import native as n
    from meshnet import graph_ops as go
    Rr, T = 771, 3
    h8, W, b, add, dy = R.rows_dot_case(Rr)
    e8, W1, b1, W2, b2, _ = R.sim_hidden_case(13)

    def off_by_one(t):
        buf = torch.zeros(t.numel() + 1, device="cuda")
        v = buf[1:].view(t.shape)
        v.copy_(t)
        assert v.is_contiguous() and v.data_ptr() % 16 == 4
        return v
    hc, Wc, bc, dyc = cuda(h8[:T]), cuda(W), cuda(b), cuda(dy[:T])
    y = filled(T, Rr)
    for hh, WW in ((off_by_one(hc), Wc), (hc, off_by_one(Wc))):
        with pytest.raises(n.CsplatError):
            n.check(n.lib.csplat_rows_dot_fwd(n.stream_handle(torch.device("cuda")), T, Rr, 256, P(WW), P(bc), P(hh), P(y), None), "csplat_rows_dot_fwd")
    assert bool((y == SENT).all())

    def run(h, Wt, W2t):
        h, Wt = h.detach().requires_grad_(), Wt.detach().requires_grad_()
        out = go.rows_dot(h, Wt, bc, cuda(add[:T]))
        assert type(out.grad_fn).__name__.startswith("RowsDot")
        out.backward(dyc)
        prm = [t.detach().requires_grad_() for t in (cuda(W1), cuda(b1), W2t, cuda(b2), Wt.detach(), bc)]
        res = go.SimResidual.apply(cuda(e8[:T]), *prm, cuda(add[:T]))
        res.backward(dyc)
        return [out.detach(), h.grad, Wt.grad, res.detach()] + [q.grad for q in prm]
    aligned = run(hc, Wc, cuda(W2))
    for moved in (run(off_by_one(hc), Wc, cuda(W2)), run(hc, off_by_one(Wc), cuda(W2)), run(hc, Wc, off_by_one(cuda(W2)))):
        for a, c in zip(aligned, moved):
            assert same_bits(a, c)


def test_native_launch_takes_the_failure_path_of_check_and_the_next_launch_succeeds():
    """csplat.native.launch(name, device, *args) on an entry that refuses its arguments BEFORE launching anything (csplat_rows_dot_fwd
    with h off a 16-byte boundary): CsplatError naming the entry, every registered ticket cache emptied, SCRATCH_EPOCH moved by one,
    nothing written; the same call with the aligned operand then succeeds and gives the bits of the plain check() call"""
    from csplat import native as n
    Rr, T = 771, 3
    h8, W, b, _add, _dy = R.rows_dot_case(Rr)
    hc, Wc, bc = cuda(h8[:T]), cuda(W), cuda(b)
    buf = torch.zeros(hc.numel() + 1, device="cuda")
    moved = buf[1:].view(hc.shape)
    moved.copy_(hc)
    assert moved.data_ptr() % 16 == 4
    dev = torch.device("cuda", torch.cuda.current_device())
    y = filled(T, Rr)
    cache = {"ticket": object()}
    n.TICKET_CACHES.append(cache)
    try:
        epoch = n.SCRATCH_EPOCH[0]
        with pytest.raises(n.CsplatError, match="csplat_rows_dot_fwd"):
            n.launch("csplat_rows_dot_fwd", dev, T, Rr, 256, P(Wc), P(bc), P(moved), P(y), None)
        assert not cache and n.SCRATCH_EPOCH[0] == epoch + 1
        assert bool((y == SENT).all())
        cache["ticket"] = object()
        assert n.launch("csplat_rows_dot_fwd", dev, T, Rr, 256, P(Wc), P(bc), P(hc), P(y), None) is None
        assert cache and n.SCRATCH_EPOCH[0] == epoch + 1
    finally:
        n.TICKET_CACHES[:] = [c for c in n.TICKET_CACHES if c is not cache]
    assert same_bits(y, _rows_dot_fwd(T, Rr, Wc, bc, hc, None))
    # device None: the current device
    y2 = filled(T, Rr)
    n.launch("csplat_rows_dot_fwd", None, T, Rr, 256, P(Wc), P(bc), P(hc), P(y2), None)
    assert same_bits(y2, y)


def test_scratch_cache_keys_on_device_index_and_run_stream_and_evicts_through_the_epoch():
    """csplat.native.ScratchCache, a private one with cap=2 and 256-byte buffers: a miss asks the size function once and returns zeros; a
    hit returns the identical tensor and asks nothing; other sizes are another buffer; the third distinct key empties the cache and moves
    SCRATCH_EPOCH by exactly one; `cuda` and `cuda:0`-style devices share a buffer; with REPLAY_STREAM set the key carries that handle,
    not the current stream's; an explicit stream key wins over both; a failing entry (csplat_rows_dot_fwd refusing an operand off a
    16-byte boundary: it returns on the host, nothing is launched) empties it."""
    from csplat import native as n
    idx = torch.cuda.current_device()
    dev = torch.device("cuda", idx)
    asked = []

    def size():
        asked.append(1)
        return 256
    cache = n.ScratchCache(cap=2)
    assert cache.cap == 2 and any(c is cache for c in n.TICKET_CACHES)
    had_alias = idx in n.REPLAY_STREAM
    alias = n.REPLAY_STREAM.get(idx)
    n.REPLAY_STREAM.pop(idx, None)
    try:
        cur = n.stream_handle(idx)
        a = cache.buffer(dev, (3, 5), size)
        assert len(asked) == 1 and a.dtype == torch.uint8 and a.numel() == 256 and a.device == dev and not bool(a.any())
        assert list(cache) == [(idx, cur, 3, 5)]
        assert cache.buffer(dev, (3, 5), size) is a and len(asked) == 1                      # a hit: no size query
        assert cache.buffer(torch.device("cuda"), (3, 5), size) is a and cache.buffer(None, (3, 5), size) is a and len(asked) == 1
        b = cache.buffer(dev, (3, 6), size)
        assert b is not a and b.data_ptr() != a.data_ptr() and len(asked) == 2 and len(cache) == 2
        epoch = n.SCRATCH_EPOCH[0]
        c = cache.buffer(dev, (4, 6), size)                                                  # the third key: at the cap, so the cache is emptied first
        assert n.SCRATCH_EPOCH[0] == epoch + 1 and list(cache) == [(idx, cur, 4, 6)] and cache[(idx, cur, 4, 6)] is c and len(asked) == 3
        made_up = cur + 0x1000 if cur else 0x1000                                            # (never dereferenced: it is only a key)
        n.REPLAY_STREAM[idx] = made_up
        d = cache.buffer(dev, (4, 6), size)
        assert d is not c and (idx, made_up, 4, 6) in cache and cache[(idx, made_up, 4, 6)] is d and len(cache) == 2
        assert cache.buffer(dev, (4, 6), size, stream=cur) is c                              # an explicit stream key wins over the alias ...
        n.REPLAY_STREAM.pop(idx)
        assert cache.buffer(dev, (4, 6), size, stream=made_up) is d and len(asked) == 4      # ... and over the current stream
        # a failing entry empties it
        h8, W, b_, _add, _dy = R.rows_dot_case(771)
        hc, Wc, bc = cuda(h8[:3]), cuda(W), cuda(b_)
        moved = torch.zeros(hc.numel() + 1, device="cuda")[1:].view(hc.shape)
        assert moved.data_ptr() % 16 == 4
        epoch = n.SCRATCH_EPOCH[0]
        with pytest.raises(n.CsplatError, match="csplat_rows_dot_fwd"):
            n.launch("csplat_rows_dot_fwd", dev, 3, 771, 256, P(Wc), P(bc), P(moved), P(filled(3, 771)), None)
        assert not cache and n.SCRATCH_EPOCH[0] == epoch + 1
        e = cache.buffer(dev, (4, 6), size)
        assert len(asked) == 5 and not bool(e.any())
    finally:
        n.REPLAY_STREAM.pop(idx, None)
        if had_alias:
            n.REPLAY_STREAM[idx] = alias
        n.TICKET_CACHES[:] = [x for x in n.TICKET_CACHES if x is not cache]


# ================================================================================================ sim_hidden
def _sim_fwd(T, K0, e, W1, b1, W2, b2):
    h1, h2 = filled(T, 256), filled(T, 256)
    call("csplat_sim_hidden_fwd", T, K0, P(e), P(W1), P(b1), P(W2), P(b2), P(h1), P(h2))
    return h1, h2


def _sim_bwd(T, K0, e, W2, h1, h2, dh2, scratch):
    dW1, db1, dW2, db2 = filled(256, K0), filled(256), filled(256, 256), filled(256)
    call("csplat_sim_hidden_bwd", T, K0, P(e), P(W2), P(h1), P(h2), P(dh2), P(dW1), P(db1), P(dW2), P(db2), P(scratch))
    return dW1, db1, dW2, db2


def _sim_scratch():
    from csplat import native as n
    return torch.zeros(int(n.lib.csplat_sim_hidden_scratch_bytes(8)) // 4, dtype=torch.int32, device="cuda")


@pytest.mark.parametrize("K0", R.SIM_HIDDEN_K0)
def test_sim_hidden_every_T_forward_and_backward(K0):
    """csplat_sim_hidden_fwd / _bwd: the eight instantiations of either switch at the K0 limits and the reference's 13; both ReLUs have
    dead and live units in every row; the two units with a preactivation of exactly 0 give 0 and take no gradient; the order of every
    sum is the same for every T (the rows of a T-row forward have the bits of the 8-row one), and the 8-row one has the bits dumped
    from the build before the ReLU change; one scratch serves every call"""
    e8, W1, b1, W2, b2, dh2 = R.sim_hidden_case(K0)
    W1c, b1c, W2c, b2c = cuda(W1), cuda(b1), cuda(W2), cuda(b2)
    scratch = _sim_scratch()
    full = _sim_fwd(8, K0, cuda(e8), W1c, b1c, W2c, b2c)
    # the bits the build before relu_keep_nan gave on the same inputs (tests/golden/make_sim_hidden_bits.py): on finite data the change of
    # the ReLU is invisible.  (The zero units are +0 here.  A preactivation of exactly -0.0, which these cases do not hold, stays -0.0
    # under relu_keep_nan, as under every other ReLU of the library; fmaxf was free to give either zero.)
    parent = util.golden("sim_hidden_parent_bits.npz")
    for name, got in (("h1", full[0]), ("h2", full[1])):
        np.testing.assert_array_equal(bits(got).cpu().numpy(), parent[f"{name}_{K0}_8"], err_msg=f"{name} K0 {K0}")
    for T in R.SIM_HIDDEN_T:
        ec, dc = cuda(e8[:T]), cuda(dh2[:T])
        h1, h2 = _sim_fwd(T, K0, ec, W1c, b1c, W2c, b2c)
        assert same_bits(h1, full[0][:T]) and same_bits(h2, full[1][:T])
        r64, r32 = R.sim_hidden(e8[:T], W1, b1, W2, b2, F64), R.sim_hidden(e8[:T], W1, b1, W2, b2, F32)
        check("sim_hidden fwd", f"T {T} K0 {K0} h1", h1, r64[0], r32[0], 1e-30)       # unit: none needed (live units in every row)
        check("sim_hidden fwd", f"T {T} K0 {K0} h2", h2, r64[1], r32[1], 1e-30)
        assert not bool(h1[:, R.SIM_ZERO_UNIT_1].any()) and not bool(h2[:, R.SIM_ZERO_UNIT_2].any())
        assert bool(((h1 > 0) == cuda(r64[0] > 0)).all()) and bool(((h2 > 0) == cuda(r64[1] > 0)).all())
        got = _sim_bwd(T, K0, ec, W2c, h1, h2, dc, scratch)
        assert int(scratch[0]) == 0
        for a, c in zip(got, _sim_bwd(T, K0, ec, W2c, h1, h2, dc, scratch)):
            assert same_bits(a, c)
        g64, g32 = R.sim_hidden_grads(e8[:T], W1, b1, W2, b2, dh2[:T], F64), R.sim_hidden_grads(e8[:T], W1, b1, W2, b2, dh2[:T], F32)
        for name, a, c, d in zip(("dW1", "db1", "dW2", "db2"), got, g64, g32):
            check(f"sim_hidden bwd {name}", f"T {T} K0 {K0}", a, c, d, 1e-30)          # unit: none needed, no gradient tensor vanishes
        assert not bool(got[0][R.SIM_ZERO_UNIT_1].any()) and float(got[1][R.SIM_ZERO_UNIT_1]) == 0.0
        assert not bool(got[2][R.SIM_ZERO_UNIT_2].any()) and float(got[3][R.SIM_ZERO_UNIT_2]) == 0.0


def test_sim_hidden_backward_ticket_is_reusable_across_T():
    K0 = 13
    e8, W1, b1, W2, b2, dh2 = R.sim_hidden_case(K0)
    W1c, b1c, W2c, b2c = cuda(W1), cuda(b1), cuda(W2), cuda(b2)
    scratch = _sim_scratch()
    runs = []
    for T in (3, 8, 1):          # three calls in a row on one scratch, nothing read in between
        ec = cuda(e8[:T])
        h1, h2 = _sim_fwd(T, K0, ec, W1c, b1c, W2c, b2c)
        runs.append((T, _sim_bwd(T, K0, ec, W2c, h1, h2, cuda(dh2[:T]), scratch)))
    assert int(scratch[0]) == 0
    for T, got in runs:
        g64, g32 = R.sim_hidden_grads(e8[:T], W1, b1, W2, b2, dh2[:T], F64), R.sim_hidden_grads(e8[:T], W1, b1, W2, b2, dh2[:T], F32)
        for name, a, c, d in zip(("dW1", "db1", "dW2", "db2"), got, g64, g32):
            check(f"sim_hidden bwd {name}", f"T {T} in a row", a, c, d, 1e-30)


def test_sim_hidden_relu_keeps_a_nan():
    """a diverged simulator must show: a NaN time code poisons its own row of h1 and h2 only, a NaN weight row poisons its unit of h1 in
    every row and from there all of h2 -- as torch.relu does (fmaxf(x, 0) returned 0 for a NaN)"""
    K0, T = 13, 3
    e8, W1, b1, W2, b2, _ = R.sim_hidden_case(K0)
    W1c, b1c, W2c, b2c = cuda(W1), cuda(b1), cuda(W2), cuda(b2)
    clean = _sim_fwd(T, K0, cuda(e8[:T]), W1c, b1c, W2c, b2c)
    e = e8[:T].clone()
    e[1, 4] = float("nan")
    h1, h2 = _sim_fwd(T, K0, cuda(e), W1c, b1c, W2c, b2c)
    r1, r2 = R.sim_hidden(e, W1, b1, W2, b2, F64)
    for got, ref, cl in ((h1, r1, clean[0]), (h2, r2, clean[1])):
        assert torch.equal(torch.isnan(got).cpu(), torch.isnan(ref)) and bool(torch.isnan(got[1]).all())
        assert same_bits(got[[0, 2]], cl[[0, 2]])
    Wn = W1.clone()
    Wn[40, 2] = float("nan")
    h1, h2 = _sim_fwd(T, K0, cuda(e8[:T]), cuda(Wn), b1c, W2c, b2c)
    r1, r2 = R.sim_hidden(e8[:T], Wn, b1, W2, b2, F64)
    assert torch.equal(torch.isnan(h1).cpu(), torch.isnan(r1)) and bool(torch.isnan(h1[:, 40]).all())
    keep = torch.arange(256, device="cuda") != 40
    assert same_bits(h1[:, keep], clean[0][:, keep])
    assert torch.equal(torch.isnan(h2).cpu(), torch.isnan(r2)) and bool(torch.isnan(h2).all())


def _step_inputs(T=3, V=257, E=300):
    D, ei, rest, _info = R.regs_case(T, V, E)
    e8, W1, b1, W2, b2, _ = R.sim_hidden_case(13)
    g = torch.Generator().manual_seed(99)
    Wo, bo = torch.randn(3 * V, 256, generator=g) / 16.0, 0.1 * torch.randn(3 * V, generator=g)
    wD = torch.randn(T, V, 3, generator=g)
    return dict(e=e8[:T], W1=W1, b1=b1, W2=W2, b2=b2, Wo=Wo, bo=bo, base=D, ei=ei, rest=rest, wD=wD, T=T, V=V)


def test_a_nan_reaches_the_vertices_and_the_loss_through_both_nodes():
    from csplat import train as tr
    from meshnet import graph_ops as go
    s = _step_inputs()
    csr = tr.edge_csr(cuda(s["ei"]), s["V"])
    for where in ("time code", "weight row"):
        e, W1 = s["e"].clone(), s["W1"].clone()
        if where == "time code":
            e[1, 0] = float("nan")
        else:
            W1[7, 3] = float("nan")
        prm = [cuda(t) for t in (W1, s["b1"], s["W2"], s["b2"], s["Wo"], s["bo"])]
        y = go.SimResidual.apply(cuda(e), *prm, cuda(s["base"])).view(s["T"], s["V"], 3)
        D, loss = tr.SimulatorStep.apply(cuda(e), *prm, cuda(s["base"]), cuda(s["ei"]), cuda(s["rest"]), 0.01, 0.3, 0.1, csr, False)
        for verts in (y, D):
            if where == "time code":
                assert bool(torch.isnan(verts[1]).all()) and bool(torch.isfinite(verts[[0, 2]]).all())
            else:
                assert bool(torch.isnan(verts).all())
        assert bool(torch.isnan(loss))


# ================================================================================================ cloth regularisers
def _regs_blocks(T, V, E):
    cdiv = lambda a, b: -(-a // b)  # noqa: E731
    return cdiv(V + T * E, 256), T * cdiv(V, 256)


def _regs_scratch(T, V, E):
    from csplat import native as n
    nbytes = int(n.lib.csplat_cloth_regs_scratch_bytes(T, V, E))
    assert nbytes - 256 >= 4 * max(_regs_blocks(T, V, E)) and nbytes % 4 == 0      # the ticket word sits behind either form's partials
    return torch.zeros(nbytes, dtype=torch.uint8, device="cuda")


def _ticket(scratch):
    return int(scratch[scratch.numel() - 256:].view(torch.int32)[0])


def _regs_gpu(D, ei, rest, lams, csr, scratch):
    T, V, E = int(D.shape[0]), int(D.shape[1]), int(ei.shape[1])
    loss, grad = filled(1), filled(T, V, 3)
    call("csplat_cloth_regs", T, V, E, P(D), P(ei), P(rest), float(lams[0]), float(lams[1]), float(lams[2]), P(loss), P(grad), P(scratch),
         *([None] * 4 if csr is None else [c.data_ptr() for c in csr]))
    return loss, grad


@pytest.mark.parametrize("T,V,E", R.REGS_CASES)
def test_cloth_regs_both_forms_every_lambda_set(T, V, E):
    """csplat_cloth_regs, atomic scatter form and CSR form, on graphs with isolated vertices, self-loops, 20 copies of an edge, hubs of
    degree 300 and the exact zeros (tests/sim_rollout_ref.py:regs_case); all lambdas, each alone, none.  The loss has the same bits on a
    repeat in both forms, the CSR gradient too; with no active term a sentinel-filled gradient is zeroed; the ticket is left at 0"""
    from csplat import train as tr
    D, ei, rest, _info = R.regs_case(T, V, E)
    Dc, eic, restc = cuda(D), cuda(ei), cuda(rest)
    csr = tr.edge_csr(eic, V)
    scratch = _regs_scratch(T, V, E)
    for lams in R.REGS_LAMBDAS:
        (l64, g64), (l32, g32) = R.cloth_regs(D, ei, rest, *lams, dtype=F64), R.cloth_regs(D, ei, rest, *lams, dtype=F32)
        for form, c in (("scatter", None), ("csr", csr)):
            loss, grad = _regs_gpu(Dc, eic, restc, lams, c, scratch)
            loss2, grad2 = _regs_gpu(Dc, eic, restc, lams, c, scratch)
            assert same_bits(loss, loss2) and (form == "scatter" or same_bits(grad, grad2))
            where = f"({T}, {V}, {E}) lambdas {lams}"
            if not any(lams):
                assert float(loss) == 0.0 and not bool(grad.any())
            # unit 1e-30: a term that is switched off (or has T < 3) must give exactly 0, everything else is measured by its own largest
            check(f"cloth_regs {form} loss", where, loss[0], l64, l32, 1e-30)
            check(f"cloth_regs {form} grad", where, grad, g64, g32, 1e-30)
            check(f"cloth_regs {form} grad", where + " (repeat)", grad2, g64, g32, 1e-30)
    assert _ticket(scratch) == 0


def test_cloth_regs_ticket_and_scratch_across_sizes():
    """two calls of either form on one scratch, then another (T, V, E) on its own: every result right, every ticket back at 0"""
    from csplat import train as tr
    for (T, V, E) in ((3, 22001, 22003), (4, 300, 2000)):
        D, ei, rest, _info = R.regs_case(T, V, E)
        Dc, eic, restc = cuda(D), cuda(ei), cuda(rest)
        csr = tr.edge_csr(eic, V)
        scratch = _regs_scratch(T, V, E)
        lams = R.REGS_LAMBDAS[0]
        runs = [(_regs_gpu(Dc, eic, restc, lams, c, scratch), f) for c, f in ((None, "scatter"), (csr, "csr"), (None, "scatter"), (csr, "csr"))]
        assert _ticket(scratch) == 0
        (l64, g64), (l32, g32) = R.cloth_regs(D, ei, rest, *lams, dtype=F64), R.cloth_regs(D, ei, rest, *lams, dtype=F32)
        for (loss, grad), form in runs:
            check(f"cloth_regs {form} loss", f"({T}, {V}, {E}) in a row", loss[0], l64, l32, 1e-30)
            check(f"cloth_regs {form} grad", f"({T}, {V}, {E}) in a row", grad, g64, g32, 1e-30)


def _step_reference(s, gl, dtype):
    h1, h2 = R.sim_hidden(s["e"], s["W1"], s["b1"], s["W2"], s["b2"], dtype)
    T, V = s["T"], s["V"]
    D = R.rows_dot(h2, s["Wo"], s["bo"], s["base"].reshape(T, -1), dtype).view(T, V, 3)
    loss, gD = R.cloth_regs(D, s["ei"], s["rest"], 0.01, 0.3, 0.1, dtype)
    g = s["wD"].to(dtype) + gl * gD
    dWo, dbo, dh = R.rows_dot_grads(h2, s["Wo"], g.reshape(T, -1), dtype)
    dW1, db1, dW2, db2 = R.sim_hidden_grads(s["e"], s["W1"], s["b1"], s["W2"], s["b2"], dh, dtype)
    return dict(D=D, loss=loss, W1=dW1, b1=db1, W2=dW2, b2=db2, Wo=dWo, bo=dbo)


def test_simulator_step_and_tapped_regs_against_the_chained_restatement():
    """train.SimulatorStep (hidden layers, output layer + table rows, regularisers; backward through all three) and FusedClothRegs(tap=True)
    at (3, 257, 300): vertices, loss and all six parameter gradients against sim_hidden -> rows_dot -> cloth_regs of the restatement"""
    from csplat import train as tr
    s, gl = _step_inputs(), 1.7
    csr = tr.edge_csr(cuda(s["ei"]), s["V"])
    r64, r32 = _step_reference(s, gl, F64), _step_reference(s, gl, F32)
    names = ("W1", "b1", "W2", "b2", "Wo", "bo")
    prm = [cuda(s[k]).requires_grad_() for k in names]
    D, loss = tr.SimulatorStep.apply(cuda(s["e"]), *prm, cuda(s["base"]), cuda(s["ei"]), cuda(s["rest"]), 0.01, 0.3, 0.1, csr, False)
    ((D * cuda(s["wD"])).sum() + gl * loss).backward()
    check("SimulatorStep", "vertices", D, r64["D"], r32["D"], 1e-30)               # unit: none needed
    check("SimulatorStep", "loss", loss, r64["loss"], r32["loss"], 1e-30)
    for k, q in zip(names, prm):
        check("SimulatorStep", f"d/d{k}", q.grad, r64[k], r32[k], 1e-30)
    # the tapped node alone, on the grid vertices of the case
    Dl = cuda(s["base"]).requires_grad_()
    loss, thru = tr.FusedClothRegs.apply(Dl, cuda(s["ei"]), cuda(s["rest"]), 0.01, 0.3, 0.1, csr, True)
    assert same_bits(thru, Dl)
    ((thru * cuda(s["wD"])).sum() + gl * loss).backward()
    ref = []
    for dt in (F64, F32):
        l, g = R.cloth_regs(s["base"], s["ei"], s["rest"], 0.01, 0.3, 0.1, dt)
        ref.append((l, s["wD"].to(dt) + gl * g))
    check("FusedClothRegs tap", "loss", loss, ref[0][0], ref[1][0], 1e-30)
    check("FusedClothRegs tap", "d/dD", Dl.grad, ref[0][1], ref[1][1], 1e-30)


# ================================================================================================ rollout head / decode / integrate
def _head(N, H, T, hist, nt, mean, std, counter, am):
    feats = filled(N, 3 * H + T)
    call("csplat_rollout_head", N, H, T, P(hist), P(nt), P(mean), P(std), P(feats), P(counter), P(am))
    return feats


@pytest.mark.parametrize("N", R.HEAD_N)
def test_rollout_head(N):
    """csplat_rollout_head: node counts around one workgroup and N = 0; (H, T) from (1, 0) to the limits (16, 16), node types mixed over
    all T; with and without statistics; the counter goes up by exactly one per call (N = 0 included, NULL accepted); the absmax word is
    the maximum of the stored features bit for bit, and keeps a larger value it held before"""
    for H, T in R.HEAD_HT:
        hist, nt, mean, std = R.head_case(N, H, T)
        hc, ntc = cuda(hist), cuda(nt)
        counter = torch.zeros(1, dtype=torch.int32, device="cuda")
        calls = 0
        for norm in (False, True):
            m, s = (cuda(mean), cuda(std)) if norm else (None, None)
            am = torch.zeros(1, device="cuda")
            feats = _head(N, H, T, hc, ntc, m, s, counter, am)
            calls += 1
            r64 = R.rollout_head(hist, nt, mean if norm else None, std if norm else None, T, F64)[0]
            r32 = R.rollout_head(hist, nt, mean if norm else None, std if norm else None, T, F32)[0]
            check("rollout_head", f"N {N} H {H} T {T} norm {norm}", feats, r64, r32, 1e-30)     # unit: none needed (velocities of O(1))
            if not norm:
                assert same_bits(feats, cuda(r32))                                             # copies and 0 / 1
            assert same_bits(am, feats.abs().max().reshape(1) if N else torch.zeros(1, device="cuda"))
            big = torch.full((1,), 1e9, device="cuda")
            assert same_bits(_head(N, H, T, hc, ntc, m, s, counter, big), feats) and float(big) == 1e9
            calls += 1
            assert same_bits(_head(N, H, T, hc, ntc, m, s, None, None), feats)
            assert int(counter) == calls


@pytest.mark.parametrize("N", R.DECODE_N)
def test_rollout_decode(N):
    """csplat_rollout_decode: eight rows per workgroup and odd counts, every output width, with and without the output statistics"""
    for D in R.DECODE_D:
        h, W, b, om, os_, last = R.decode_case(N, D)
        hc, Wc, bc, lc = cuda(h), cuda(W), cuda(b), cuda(last)
        for norm in (False, True):
            m, s = (om, os_) if norm else (None, None)
            mc, sc = cuda(m), cuda(s)
            fine = torch.ones(1, dtype=torch.int32, device="cuda")
            v = filled(N, D)
            call("csplat_rollout_decode", N, D, P(hc), P(Wc), P(bc), P(mc), P(sc), P(lc), P(v), P(fine))
            v2 = filled(N, D)
            call("csplat_rollout_decode", N, D, P(hc), P(Wc), P(bc), P(mc), P(sc), P(lc), P(v2), P(fine))
            assert int(fine) == 1 and same_bits(v, v2)
            r64, r32 = R.rollout_decode(h, W, b, m, s, last, F64), R.rollout_decode(h, W, b, m, s, last, F32)
            assert r64[1] == 1
            check("rollout_decode", f"N {N} D {D} norm {norm}", v, r64[0], r32[0], 1e-30)       # unit: none needed (last_v of O(1))


def test_rollout_decode_fine_word_sees_a_nan_and_an_overflow():
    N, D = 10007, 3
    h, W, b, om, os_, last = R.decode_case(N, D)
    Wc, bc, lc, omc, osc = cuda(W), cuda(b), cuda(last), cuda(om), cuda(os_)

    def run(hh):
        fine, v, hc = torch.ones(1, dtype=torch.int32, device="cuda"), filled(N, D), cuda(hh)
        call("csplat_rollout_decode", N, D, P(hc), P(Wc), P(bc), P(omc), P(osc), P(lc), P(v), P(fine))
        return v, int(fine)
    clean, fine = run(h)
    assert fine == 1
    r64, r32 = R.rollout_decode(h, W, b, om, os_, last, F64)[0], R.rollout_decode(h, W, b, om, os_, last, F32)[0]
    for row, value in ((5001, float("nan")), (4098, 3e38)):
        hh = h.clone()
        if value != value:
            hh[row, 17] = value
        else:
            hh[row] = value * torch.sign(W[0])                # output 0 of the row sums 128 products of one sign: Inf
        v, fine = run(hh)
        keep = torch.arange(N, device="cuda") != row
        assert fine == 0 and not bool(torch.isfinite(v[row]).all()) and R.rollout_decode(hh, W, b, om, os_, last, F32)[1] == 0
        assert value == value or bool(torch.isnan(v[row]).all())
        assert same_bits(v[keep], clean[keep])
        check("rollout_decode", f"non-finite row {row}: every other row", v[keep], r64[keep.cpu()], r32[keep.cpu()], 1e-30)


def _bump(counter):
    """one call of the head (the step counter's only writer) on a one-node graph"""
    hist, nt = torch.zeros(1, 1, 3, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
    _head(1, 1, 0, hist, nt, None, None, counter, None)


@pytest.mark.parametrize("N", R.INTEGRATE_N)
def test_rollout_integrate_three_steps(N):
    """csplat_rollout_integrate behind 1, 2 and 3 calls of the head on one set of buffers: history depths where the in-place shift is
    empty, runs once, and has an order; every width; the pinned index at both ends and outside [0, N) (nothing pinned).  Every output is
    a copy or one float32 addition: equality with the float32 restatement, step after step; at D = 3 the counter is moved by the step's
    own head, whose features of the shifted history are compared as well"""
    for H in R.INTEGRATE_H:
        for D in R.INTEGRATE_D:
            v0, act, pos0, hist0 = R.integrate_case(N, H, D)
            for grasped in sorted({0, N - 1, N, -1}):
                pos, hist, preds, actc = cuda(pos0), cuda(hist0), filled(3, N, D), cuda(act)
                counter = torch.zeros(1, dtype=torch.int32, device="cuda")
                r_pos, r_hist, r_preds = pos0.clone(), hist0.clone(), torch.full((3, N, D), SENT)
                nt = torch.arange(N, dtype=torch.int32) % 2
                for k in (1, 2, 3):
                    if D == 3:      # the step's own head on the history the last integrate left
                        feats = _head(N, H, 2, hist, cuda(nt), None, None, counter, None)
                        assert same_bits(feats, cuda(R.rollout_head(r_hist, nt, None, None, 2, F32)[0])), (N, H, grasped, k)
                    else:
                        _bump(counter)
                    v_in = v0 * float(k)
                    v, am2 = cuda(v_in), torch.tensor([5.0, 7.0], device="cuda")
                    call("csplat_rollout_integrate", N, H, D, P(v), P(actc), P(counter), grasped, P(pos), P(hist), P(preds), P(am2))
                    r_v, r_pos, r_hist, r_preds = R.rollout_integrate(v_in, act, k, grasped, r_pos, r_hist, r_preds, F32)
                    where = (N, H, D, grasped, k)
                    assert same_bits(v, cuda(r_v)) and same_bits(pos, cuda(r_pos)), where
                    assert same_bits(hist, cuda(r_hist)) and same_bits(preds, cuda(r_preds)), where
                    assert bool((preds[k:] == SENT).all()) and not bool(am2.any()) and int(counter) == k, where
                    if 0 <= grasped < N:
                        assert same_bits(preds[k - 1, grasped], actc[k - 1]), where


def test_rollout_with_an_index_outside_the_graph_takes_the_generic_step():
    """_FusedClothStep.applicable refuses a grasped index outside [0, N): the generic step gives -1 Python's meaning (the last node is
    pinned), k_rollout_integrate would pin nothing"""
    from meshnet import rollout as ro
    from meshnet.cloth_network import ClothMeshSimulator
    dev = "cuda"
    g = torch.Generator().manual_seed(43)
    N, E = 300, 3000
    pos = torch.randn(N, 3, generator=g).to(dev)
    ei = torch.stack([torch.randint(0, N, (E,), generator=g), torch.randint(0, N, (E,), generator=g)]).to(dev)
    torch.manual_seed(9)
    sim = ClothMeshSimulator(3, 8, 4, 128, 3, 2, 128, 2, 2, normalize=False, device=dev).eval()
    hist = (torch.randn(2, N, 3, generator=g) * 0.01).to(dev)
    ntype = torch.randint(0, 2, (N, 1), generator=g).to(dev)
    actions = (torch.randn(3, 3, generator=g) * 0.01).to(dev)
    assert ro._FusedClothStep.applicable(sim, pos, hist, ntype, ei, actions, N - 1)
    for outside in (-1, N, -N - 1):
        assert not ro._FusedClothStep.applicable(sim, pos, hist, ntype, ei, actions, outside)
    a_pred, a_pos = ro.rollout(sim, pos, hist, ntype, ei, actions, -1, 3, graph=False)
    was = ro.FUSED_STEP
    ro.FUSED_STEP = False
    try:
        b_pred, b_pos = ro.rollout(sim, pos, hist, ntype, ei, actions, -1, 3, graph=False)
    finally:
        ro.FUSED_STEP = was
    assert torch.equal(a_pred, b_pred) and torch.equal(a_pos, b_pos) and torch.equal(a_pred[:, N - 1], actions)
    assert bool(torch.isfinite(a_pred).all())


# ================================================================================================ edge features, row gather, refinement
@pytest.mark.parametrize("E", R.EDGE_FEATURES_E)
def test_edge_features_plain_and_ordered(E):
    """csplat_gnn_edge_features and _ordered (a random permutation; past the 512-workgroup cap at E = 131 073): a self-loop and an edge
    between coincident nodes have length exactly 0; the absmax word as for the head"""
    pos, ei, order = R.edge_case(E)
    pc, eic, oc = cuda(pos), cuda(ei), cuda(order)
    out = filled(E, 4)
    call("csplat_gnn_edge_features", E, P(pc), P(eic), P(out))
    r64, r32 = R.edge_features(pos, ei, None, F64)[0], R.edge_features(pos, ei, None, F32)[0]
    check("edge_features", f"E {E}", out, r64, r32, 1e-30)              # unit: none needed (positions of O(1))
    if E >= 2:
        assert float(out[0, 3]) == 0.0 and float(out[1, 3]) == 0.0 and not bool(out[:2].any())
    am = torch.zeros(1, device="cuda")
    ordered = filled(E, 4)
    call("csplat_gnn_edge_features_ordered", E, P(pc), P(eic), P(oc), P(ordered), P(am))
    assert same_bits(ordered, out[oc]) and same_bits(am, ordered.abs().max().reshape(1) if E else torch.zeros(1, device="cuda"))
    check("edge_features ordered", f"E {E}", ordered, r64[order], r32[order], 1e-30)
    big, again = torch.full((1,), 1e9, device="cuda"), filled(E, 4)
    call("csplat_gnn_edge_features_ordered", E, P(pc), P(eic), P(oc), P(again), P(big))
    assert same_bits(again, ordered) and float(big) == 1e9
    call("csplat_gnn_edge_features_ordered", E, P(pc), P(eic), P(oc), P(again), None)
    assert same_bits(again, ordered)


@pytest.mark.parametrize("L,E", tuple(R.GATHER_CASES) + ((128, 0),))
def test_gather_rows_absmax(L, E):
    """csplat_gnn_gather_rows_absmax: copies, so equality; the absmax word (zeroed by the entry itself) is exact; past the 4096-workgroup
    cap at (128, 32 801)"""
    g = torch.Generator().manual_seed(E + L)
    rows = torch.randn(500, L, generator=g).cuda()
    keys = torch.randint(0, 500, (E,), generator=g, dtype=torch.int64).cuda()
    out, am = filled(E, L), filled(1, value=3.0)
    call("csplat_gnn_gather_rows_absmax", E, L, P(rows), P(keys), P(out), P(am))
    assert same_bits(out, rows[keys])
    assert same_bits(am, out.abs().max().reshape(1) if E else torch.zeros(1, device="cuda"))


@pytest.mark.parametrize("N,E", R.REFINE_CASES)
def test_edge_length_refine(N, E):
    """csplat_gnn_edge_length_refine: an even and an odd number of iterations (the double buffer ends in the scratch or in v), none at
    all; weights with zeros, a self-loop, coincident nodes, a node of degree 300; isolated nodes, a graph without edges and the one-node
    graph whose 300 or 3000 edges are all self-loops keep their v bit for bit; NaN-filled scratch on entry (its contents are irrelevant)"""
    from meshnet.graph_ops import GraphCSR
    pos, v0, ei, rest, w = R.refine_case(N, E)
    pc, eic, rc, wc = cuda(pos), cuda(ei), cuda(rest), cuda(w)
    csr = GraphCSR(eic, N)
    for iters in R.REFINE_ITERS:
        outs = []
        for _ in range(2):
            v, scratch = cuda(v0), filled(9 * N, value=float("nan"))
            call("csplat_gnn_edge_length_refine", N, E, P(pc), P(v), P(eic), P(rc), P(wc), P(csr.rowptr["dst"]), P(csr.perm["dst"]),
                 P(csr.rowptr["src"]), P(csr.perm["src"]), iters, R.REFINE_LR, 0.9, 0.999, 1e-8, P(scratch))
            outs.append(v)
        v = outs[0]
        assert same_bits(v, outs[1])
        if E == 0 or iters == 0 or N == 1:          # (N = 1: every edge a self-loop of length exactly 0, walked in both CSR lists)
            assert same_bits(v, cuda(v0))
            continue
        assert same_bits(v[N - 5:], cuda(v0)[N - 5:])                      # isolated nodes
        r64, r32 = (R.edge_length_refine(pos, v0, ei, rest, w, iters, R.REFINE_LR, dt) for dt in (F64, F32))
        check("edge_length_refine v", f"N {N} E {E} iters {iters}", v, r64, r32, 1e-30)          # unit: none needed (v of O(0.01))
        # the update itself, unit lr: Adam's first steps have the size lr whatever the gradient
        check("edge_length_refine update", f"N {N} E {E} iters {iters}", v.cpu().double() - v0.double(), r64 - v0.double(),
              r32.double() - v0.double(), R.REFINE_LR)
