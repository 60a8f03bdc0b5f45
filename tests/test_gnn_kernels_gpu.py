"""The kernels a MeshNet rollout and training step spend most of their time in -- csrc/csplat_gemm.hip (k_linear128<GATHER, LN, ADD, B3>
with its transposed-accumulator branch, k_linear128_rows32<LN>, k_linear_narrow, k_node_update, k_dw128) and the message-passing half of
csrc/csplat_gnn.hip (the CSR build, k_segment_sum, k_edge_combine_fwd, k_relu_mask, k_gather_rows, k_ln128_fwd / _bwd, k_colsum128,
k_relu_mask_bias128) -- through the raw C ABI against the float64 restatement tests/gnn_kernels_ref.py, at the sizes where each launch
takes another path (tests/test_gnn_kernels_cpu.py states which constant every size crosses), on rows of very different scale inside one
launch, on the LayerNorm rows that tell a two-pass variance from E[x^2] - mean^2, on hubs, duplicates, self loops and cancelling
messages, and on NaN and Inf DATA (no index, size or pointer is ever garbled).  Output buffers hold a sentinel before every launch.

Bars, by the rule of tests/test_sim_rollout_kernels_gpu.py, applied PER ROW.  The same restatement evaluated in float32 on the CPU has
an error e32 against float64 on the same inputs.  The error of row i is max_j |got - r64| divided by that row's scale; the largest row
error of a comparison must stay within K = 8 x the largest row e32 of the same comparison, floor 1e-6; a bar above 1e-3 means
ill-conditioned inputs and fails by itself.  Rows of different classes (tests/gnn_kernels_ref.py: ROW_CLASSES, LN_CLASSES) are separate
comparisons, so a hard class does not lend its bar to an easy one.  Row scales:
  a Linear without LayerNorm      max_j sum_k |alpha a_ik w_jk| plus the magnitudes of bias, gathered rows, add_pre and add_post
  anything behind a LayerNorm     max(max_j |r64_ij|, 1): normalised rows are O(1) by construction (gamma, beta of O(1))
  LayerNorm statistics            the mean in units of max(|mean|, the row's std); rstd relative to itself
  LayerNorm backward dx           rstd_i max_j |g_ij gamma_j|, the size of the terms dx is the difference of
  column sums (dgamma, dbeta, dxsum, dbias, dW)   per column, sum_i |term_ij|
  segment sums                    per node, max_j sum_e |msg_ej|; and element by element the bound of compensated summation,
                                  |got - r64| <= eps |r64| + n eps^2 sum |x|  (eps = 2^-23, n = the row's degree)
Integer outputs, copies, single additions, the masked zeros, the ReLU-masked gradients, run-to-run repeats and in-place against
out-of-place runs are compared for EQUALITY.

One deviation from "where torch gives Inf the kernel gives Inf", derived from the arithmetic and held as stated: the bf16-split product
(csplat_linear128_mode 1, persistent kernels only) forms x - bf16(x) for every operand, which is Inf - Inf = NaN for x = +-Inf, and
multiplies the leading piece by low-order pieces of either sign; a row that reads an Inf is therefore held to be NON-FINITE in every
column (NaN or Inf), nothing more.  The fp32-MFMA kernels (rows32, mode 0, node update, narrow, dw128) are held to torch's own +-Inf.

check_rows() prints e32, the bar and the kernel's error; the module's teardown prints the table of the largest of each per group
(pytest -rP shows it).

What that table showed on an MI355X when this file was written (group | comparisons | largest e32 | largest bar | largest kernel error |
smallest bar / error; "LN rows": the five LayerNorm implementations on the LayerNorm row classes, "stats": the (mean, rstd) outputs,
"TR": the transposed-accumulator branch):
  LN rows persistent mode 0       |  16 | 9.87e-05 | 7.90e-04 | 9.48e-05 |   7.8
  LN rows persistent mode 0 stats |  32 | 1.87e-07 | 1.50e-06 | 1.68e-07 |   7.7
  LN rows persistent mode 1       |  16 | 9.87e-05 | 7.90e-04 | 9.48e-05 |   7.8
  LN rows persistent mode 1 stats |  32 | 1.87e-07 | 1.50e-06 | 1.68e-07 |   7.7
  LN rows rows32                  |  16 | 3.54e-05 | 2.83e-04 | 3.45e-05 |   6.3
  LN rows rows32 stats            |  32 | 1.21e-07 | 1.00e-06 | 1.08e-07 |   9.2
  dw128 dW                        |   8 | 2.49e-07 | 1.99e-06 | 1.83e-07 |  10.2
  dw128 dbias                     |   8 | 8.71e-08 | 1.00e-06 | 1.08e-07 |   9.3
  fused chains LN(bias)           |   3 | 9.11e-06 | 7.29e-05 | 5.04e-06 |  14.4
  gather mode 0                   | 147 | 5.97e-07 | 4.78e-06 | 5.89e-07 |   5.1
  gather mode 1                   | 147 | 5.97e-07 | 4.78e-06 | 4.99e-07 |   6.7
  linear_narrow                   | 108 | 2.86e-07 | 2.29e-06 | 6.06e-07 |   1.7
  ln128_bwd dbeta                 |   9 | 1.23e-07 | 1.00e-06 | 1.07e-07 |   9.4
  ln128_bwd dgamma                |   9 | 1.31e-07 | 1.05e-06 | 1.28e-07 |   8.2
  ln128_bwd dx                    |  65 | 1.98e-07 | 1.59e-06 | 1.89e-07 |   8.0
  ln128_bwd dxsum                 |   9 | 2.67e-06 | 2.14e-05 | 2.58e-06 |   5.3
  ln128_bwd g_rows dbeta          |   9 | 5.20e-07 | 4.16e-06 | 1.95e-06 |   2.0
  ln128_bwd g_rows dgamma         |   9 | 1.02e-07 | 1.00e-06 | 1.02e-07 |   9.8
  ln128_bwd g_rows dx             |  65 | 1.42e-07 | 1.14e-06 | 1.30e-07 |   8.0
  ln128_bwd g_rows dxsum          |   9 | 4.71e-06 | 3.77e-05 | 4.29e-06 |   1.9
  ln128_bwd x_normalized dbeta    |   9 | 1.23e-07 | 1.00e-06 | 1.07e-07 |   9.4
  ln128_bwd x_normalized dgamma   |   9 | 1.27e-07 | 1.01e-06 | 1.09e-07 |   9.2
  ln128_bwd x_normalized dx       |  65 | 1.98e-07 | 1.58e-06 | 1.90e-07 |   8.0
  ln128_bwd x_normalized dxsum    |   9 | 2.19e-06 | 1.75e-05 | 2.10e-06 |   5.3
  ln128_fwd                       |  25 | 9.87e-05 | 7.90e-04 | 9.58e-05 |   7.3
  ln128_fwd stats                 |  50 | 1.87e-07 | 1.50e-06 | 1.81e-07 |   7.2
  node_update LN(b3)              |   9 | 7.59e-06 | 6.07e-05 | 1.78e-05 |   2.6
  node_update x'                  |   7 | 3.55e-07 | 2.84e-06 | 4.67e-07 |   5.9
  node_update xa' xb'             |  14 | 2.13e-07 | 1.71e-06 | 2.45e-07 |   5.5
  persistent mode 0 LN            |  48 | 1.18e-06 | 9.44e-06 | 1.31e-06 |   5.9
  persistent mode 0 LN stats      |  96 | 2.97e-07 | 2.38e-06 | 2.61e-07 |   7.5
  persistent mode 0 linear        |  96 | 6.38e-07 | 5.10e-06 | 6.49e-07 |   5.7
  persistent mode 1 LN            |  48 | 1.18e-06 | 9.44e-06 | 1.17e-06 |   5.9
  persistent mode 1 LN stats      |  96 | 2.97e-07 | 2.38e-06 | 2.65e-07 |   7.0
  persistent mode 1 TR            |  48 | 6.38e-07 | 5.10e-06 | 5.32e-07 |   4.9
  persistent mode 1 linear        |  48 | 6.38e-07 | 5.10e-06 | 5.46e-07 |   5.8
  relu_mask_bias128 dbias         |  18 | 1.74e-07 | 1.39e-06 | 1.74e-07 |   8.0
  rows32 LN                       |  66 | 1.17e-06 | 9.38e-06 | 1.04e-06 |   5.1
  rows32 LN stats                 | 132 | 2.65e-07 | 2.12e-06 | 2.40e-07 |   7.9
  rows32 linear                   | 132 | 6.28e-07 | 5.03e-06 | 5.62e-07 |   4.7
  segment_sum                     | 732 | 1.78e-06 | 1.42e-05 | 5.96e-08 |  16.8
No bar is above 7.9e-4 (the rows of mean 64, std 1/16 at 8192 rows of that class; 2.8e-4 at 8 of them).  The segment sum stays 17 times
inside the bar a plain float32 index_add_ sets and, element by element, inside eps |sum| + n eps^2 sum |x| on every graph, the hub of 3000
edges and the cancelling rows included.  The fused 16-bit-piece chains give LN(bias) 14 times inside their bar and csplat_gnn_rows_chain the
bias row bit for bit.  Wall time 30 s for the 66 tests (31 s with interpreter start-up; tests/test_knn_gnn_gpu.py in the same session: 63 s for
its 212, 65 s with start-up); the slowest, test_linear_narrow_strided_inputs[131073] at 3.6 s, spends it in the float64 / float32 references
of twelve [131 073, 128] products on the CPU."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")       # (before gnn_kernels_ref, which imports it)

import util  # noqa: E402,F401
import gnn_kernels_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

K, FLOOR, BAR_MAX = 8.0, 1e-6, 1e-3
F64, F32 = torch.float64, torch.float32
EPS32 = 2.0 ** -23
SENT = -7.25            # what output buffers hold before a launch
TABLE = {}
_CACHE = {}


@pytest.fixture(scope="module", autouse=True)
def _threads_and_table():
    old = torch.get_num_threads()
    torch.set_num_threads(min(16, old))
    yield
    torch.set_num_threads(old)
    _CACHE.clear()
    print("\ngroup | comparisons | largest e32 | largest bar | largest kernel error | smallest bar / error")
    for g in sorted(TABLE):
        n, e32, bar, err, margin = TABLE[g]
        print(f"{g} | {n} | {e32:.2e} | {bar:.2e} | {err:.2e} | {margin:.1f}")


@pytest.fixture(autouse=True)
def _default_mode():
    yield
    from csplat import native as n
    n.lib.csplat_linear128_mode(1)


def _t(x):
    return x.detach().cpu().to(F64) if torch.is_tensor(x) else torch.as_tensor(np.asarray(x), dtype=F64)


def check_rows(group, what, got, r64, r32, scale):
    """got (the kernel), r64, r32 (the restatement in float64 / float32) as [rows][columns]; scale: one number per row (or one for all)"""
    got, r64, r32 = _t(got), _t(r64), _t(r32)
    assert got.shape == r64.shape == r32.shape, (group, what, got.shape, r64.shape, r32.shape)
    if got.numel() == 0:
        return
    got, r64, r32 = (a.reshape(a.shape[0], -1) if a.dim() > 1 else a.reshape(-1, 1) for a in (got, r64, r32))
    assert bool(torch.isfinite(r64).all()) and bool(torch.isfinite(got).all()), f"{group} {what}: non-finite values"
    scale = torch.broadcast_to(_t(scale).reshape(-1), (got.shape[0],)).clamp_min(1e-300)
    e32 = float(((r32 - r64).abs().amax(1) / scale).max())
    rows = (got - r64).abs().amax(1) / scale
    worst = int(rows.argmax())
    err = float(rows[worst])
    bar = max(K * e32, FLOOR)
    print(f"{group} | {what}: e32 {e32:.3e} bar {bar:.3e} kernel {err:.3e} (row {worst})")
    n, a, b, c, m = TABLE.get(group, (0, 0.0, 0.0, 0.0, float("inf")))
    TABLE[group] = (n + 1, max(a, e32), max(b, bar), max(c, err), min(m, bar / max(err, 1e-30)))
    assert bar <= BAR_MAX, f"{group} {what}: bar {bar:.3e} > {BAR_MAX}: the inputs are ill-conditioned"
    assert err <= bar, f"{group} {what}: row {worst}: kernel error {err:.3e} > bar {bar:.3e} (float32 restatement: {e32:.3e})"


def check_classes(group, what, got, r64, r32, scale, names):
    """one comparison per row class (row i is of class i % len(names))"""
    k = len(names)
    scale = torch.broadcast_to(_t(scale).reshape(-1), (got.shape[0],))
    for c in range(min(k, got.shape[0])):
        check_rows(group, f"{what} [{names[c]}]", got[c::k], r64[c::k], r32[c::k], scale[c::k])


def check_columns(group, what, got, r64, r32, scale):
    check_rows(group, what, _t(got).reshape(-1, 1), _t(r64).reshape(-1, 1), _t(r32).reshape(-1, 1), scale)


def ln_scale(r64):
    return r64.abs().amax(1).clamp_min(1.0)


def check_stats(group, what, got, s64, s32, names):
    std = 1.0 / s64[:, 1]
    check_classes(group, what + " mean", got[:, 0:1], s64[:, 0:1], s32[:, 0:1], torch.maximum(s64[:, 0].abs(), std), names)
    check_classes(group, what + " rstd", got[:, 1:2], s64[:, 1:2], s32[:, 1:2], s64[:, 1], names)


def cuda(t):
    return None if t is None else t.detach().contiguous().cuda()


def P(t):
    """device pointer (None, and an empty tensor: NULL)"""
    if t is None:
        return None
    assert t.is_cuda and t.is_contiguous()
    return t.data_ptr() or None


def raw(name, *args):
    from csplat import native as n
    return int(getattr(n.lib, name)(n.stream_handle(torch.device("cuda")), *args))


def call(name, *args):
    from csplat import native as n
    n.check(raw(name, *args), name)


def refused(name, *args, match="16-byte"):
    """the entry returns an error and says why; nothing was launched (the caller checks its sentinels)"""
    from csplat import native as n
    assert raw(name, *args) != 0, name
    msg = n.lib.csplat_last_error().decode(errors="replace")
    assert match in msg, (name, msg)


def bits(t):
    t = t.detach().contiguous()
    return t.view(torch.int32) if t.dtype == F32 else t


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def same_values_and_nans(a, b):
    """equal where neither is a NaN, NaN in the same places (a NaN's payload is not part of any contract)"""
    a, b = a.detach().cpu(), b.detach().cpu()
    return a.shape == b.shape and torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(torch.nan_to_num(a, nan=0.0), torch.nan_to_num(b, nan=0.0))


def filled(*shape, value=SENT, dtype=F32):
    return torch.full(shape, value, dtype=dtype, device="cuda")


def off_by_one(t):
    """a contiguous view of the same values that starts one float into a larger buffer"""
    buf = torch.zeros(t.numel() + 1, device="cuda", dtype=t.dtype)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v


def set_mode(mode):
    call_plain("csplat_linear128_mode", mode)


def call_plain(name, *args):
    from csplat import native as n
    n.check(getattr(n.lib, name)(*args), name)


# ================================================================================================ csplat_linear128_ex
def linear_ex(A, W, layout="plain", bias=None, alpha=1.0, relu=False, gather=None, ln=None, add_pre=None, add_post=None, mask=None,
              want_stats=False, out=None):
    """A [M][128] on the GPU, W the logical [128][128] matrix on the CPU (stored as `layout` says); the rest GPU tensors or None.
    Returns (out with ONE EXTRA sentinel row behind the M rows unless `out` is given, stats or None)"""
    M = int(A.shape[0])
    st, ldw, wt, off = R.weight_storage(W, layout)
    st = st.cuda()
    buf = filled(M + 1, 128) if out is None else out
    stats = filled(M + 1, 2) if want_stats else None
    ga, ia, gb, ib = gather if gather is not None else (None,) * 4
    g, b = ln if ln is not None else (None, None)
    call("csplat_linear128_ex", M, P(A), st.data_ptr() + 4 * off, ldw, wt, P(bias), float(alpha), int(relu), P(ga), P(ia), P(gb), P(ib),
         P(g), P(b), R.EPS, P(add_pre), P(add_post), P(mask), P(stats), P(buf))
    if out is None:
        assert bool((buf[M] == SENT).all()), "a row behind the last one was written"
        buf = buf[:M]
    if stats is not None:
        assert bool((stats[M] == SENT).all())
        stats = stats[:M]
    return buf, stats


def _linear_case(M, huge):
    """the inputs of one size, on both sides, and A W^T in both precisions (shared by every variant and mode of that size)"""
    key = ("linear", M, huge)
    if key not in _CACHE:
        for k in [k for k in _CACHE if k[0] == "linear" and k[1] != M]:
            del _CACHE[k]
        A = R.row_classes(M)
        if huge != 1e20:
            A[5::8] *= huge / 1e20
        W, bias, gamma, beta = R.linear_params()
        pre, post, mask = R.addends(M)
        c = dict(A=A, W=W, bias=bias, gamma=gamma, beta=beta, pre=pre, post=post, mask=mask, p64=A.double() @ W.double().t(), p32=A @ W.t())
        c["absprod"] = A.double().abs() @ W.double().abs().t()
        c["g"] = {k: cuda(c[k]) for k in ("A", "bias", "gamma", "beta", "pre", "post", "mask")}
        _CACHE[key] = c
    return _CACHE[key]


VARIANTS = {   # name: (layout, alpha, bias, relu, ln, add_pre, add_post, mask)
    "bare": ("plain", 1.0, False, False, False, False, False, False),
    "plain": ("slice", 0.5, True, True, False, False, False, False),
    "LN": ("transpose", 2.0, True, True, True, False, False, False),
    "ADD": ("transposed slice", 0.5, True, True, False, True, True, True),
    "ADD+LN": ("plain", 0.5, True, True, True, True, True, True),
    "mask alone": ("transpose", 1.0, False, False, False, False, False, True),
}


def _run_variant(M, name, group, in_place=False):
    layout, alpha, use_bias, relu, use_ln, use_pre, use_post, use_mask = VARIANTS[name]
    c = _linear_case(M, 1e8 if use_ln else 1e20)       # (a row of 1e20 squares to Inf in a float32 LayerNorm, in torch's too)
    g = c["g"]
    kw = dict(bias="bias" if use_bias else None, add_pre="pre" if use_pre else None, add_post="post" if use_post else None,
              mask="mask" if use_mask else None)
    cpu = {k: (c[v] if v else None) for k, v in kw.items()}
    gpu = {k: (g[v] if v else None) for k, v in kw.items()}
    ln_c, ln_g = ((c["gamma"], c["beta"]), (g["gamma"], g["beta"])) if use_ln else (None, None)
    out, stats = linear_ex(g["A"], c["W"], layout, alpha=alpha, relu=relu, ln=ln_g, want_stats=use_ln, **gpu)
    r64, s64 = R.linear128(c["A"], c["W"], alpha=alpha, relu=relu, ln=ln_c, dtype=F64, prod=c["p64"], **cpu)
    r32, s32 = R.linear128(c["A"], c["W"], alpha=alpha, relu=relu, ln=ln_c, dtype=F32, prod=c["p32"], **cpu)
    where = f"M {M} {name}"
    if use_ln:
        check_classes(group, where, out, r64, r32, ln_scale(r64), R.ROW_CLASSES)
        check_stats(group + " stats", where, stats, s64, s32, R.ROW_CLASSES)
    else:
        scale = abs(alpha) * c["absprod"]
        for t in (cpu["bias"], cpu["add_pre"], cpu["add_post"]):
            if t is not None:
                scale = scale + t.double().abs()
        check_classes(group, where, out, r64, r32, scale.amax(1), R.ROW_CLASSES)
    if use_mask:       # the masked zeros: exactly 0 wherever the mask is not positive (negative, +0, -0), and only there by the mask
        off = ~(g["mask"] > 0)
        assert not bool(out[off].any()), where
    again, stats2 = linear_ex(g["A"], c["W"], layout, alpha=alpha, relu=relu, ln=ln_g, want_stats=use_ln, **gpu)
    assert same_bits(out, again) and (stats is None or same_bits(stats, stats2)), where
    if in_place:
        A2 = g["A"].clone()
        o2, _ = linear_ex(A2, c["W"], layout, alpha=alpha, relu=relu, ln=ln_g, out=A2, **gpu)
        assert same_bits(o2, out), where + " in place"
    return out


@pytest.mark.parametrize("M", R.ROWS32_M)
def test_linear128_rows32_row_classes_every_epilogue(M):
    """k_linear128_rows32<false / true> (every call without a gather up to 65 536 rows): one row, one short of a tile, a tile, one more,
    and the last size of this kernel; every epilogue option and weight layout; rows of every class in one launch; out aliasing A"""
    for name in VARIANTS:
        _run_variant(M, name, "rows32 " + ("LN" if VARIANTS[name][4] else "linear"), in_place=True)


@pytest.mark.parametrize("M,mode", [(M, mode) for M in R.PERSIST_M for mode in (0, 1)])
def test_linear128_persistent_row_classes_every_epilogue(M, mode):
    """k_linear128<false, LN, ADD, B3> from its first size: 65 537 (one ragged tile, the only one of the second sweep of the capped grid),
    65 568 (that tile full), 131 073 (every wave a second tile, one ragged tile in a third sweep of mode 0); mode 1 takes the bf16 split
    and, for ADD and the mask alone, its transposed-accumulator branch.  The hard rows the split was never given are all here."""
    set_mode(mode)
    for name in VARIANTS:
        tr = mode == 1 and name in ("ADD", "mask alone")
        group = f"persistent mode {mode} " + ("LN" if VARIANTS[name][4] else ("TR" if tr else "linear"))
        _run_variant(M, name, group, in_place=(M == 65537 and name in ("plain", "ADD", "LN")))


@pytest.mark.parametrize("M", R.GATHER_M)
def test_linear128_gather_every_size_and_index_pattern(M):
    """k_linear128<true, ...> (a gather never takes rows32): fewer rows than one workgroup has waves, around 4 and 8 tiles, and the
    persistent size; every index the same, every index N - 1, a permutation; both modes"""
    c = _linear_case(M, 1e20)
    g = c["g"]
    for pattern in ("equal", "last", "perm"):
        ga, ia, gb, ib = R.gather_case(M, pattern)
        gg = (cuda(ga), cuda(ia), cuda(gb), cuda(ib))
        r64 = R.linear128(c["A"], c["W"], c["bias"], 4.0, True, (ga, ia, gb, ib), dtype=F64, prod=c["p64"])[0]
        r32 = R.linear128(c["A"], c["W"], c["bias"], 4.0, True, (ga, ia, gb, ib), dtype=F32, prod=c["p32"])[0]
        scale = (4.0 * c["absprod"] + c["bias"].double().abs() + ga.double().abs()[ia] + gb.double().abs()[ib]).amax(1)
        for mode in (0, 1):
            set_mode(mode)
            out, _ = linear_ex(g["A"], c["W"], "slice", bias=g["bias"], alpha=4.0, relu=True, gather=gg)
            check_classes(f"gather mode {mode}", f"M {M} {pattern}", out, r64, r32, scale, R.ROW_CLASSES)
            assert same_bits(out, linear_ex(g["A"], c["W"], "slice", bias=g["bias"], alpha=4.0, relu=True, gather=gg)[0])
            A2 = g["A"].clone()
            assert same_bits(linear_ex(A2, c["W"], "slice", bias=g["bias"], alpha=4.0, relu=True, gather=gg, out=A2)[0], out)


def test_linear128_refused_combinations_stay_refused():
    M = 70
    A, W, out = filled(M, 128, value=1.0), filled(128, 128, value=0.5), filled(M, 128)
    rows, idx, vec = filled(M, 128, value=2.0), torch.zeros(M, dtype=torch.int64, device="cuda"), filled(128, value=1.0)

    def ex(ldw=128, ga=None, ia=None, gb=None, ib=None, gam=None, bet=None, pre=None, post=None, mask=None):
        return ("csplat_linear128_ex", M, P(A), P(W), ldw, 0, None, 1.0, 0, P(ga), P(ia), P(gb), P(ib), P(gam), P(bet), R.EPS, P(pre),
                P(post), P(mask), None, P(out))
    refused(*ex(ga=rows, ia=idx, gb=rows, ib=idx, gam=vec, bet=vec), match="not combined")
    refused(*ex(ga=rows, ia=idx, gb=rows, ib=idx, pre=rows), match="not combined")
    refused(*ex(ga=rows, ia=idx, gb=rows, ib=idx, mask=rows), match="not combined")
    refused(*ex(ga=rows, ia=idx), match="gather needs both")
    refused(*ex(gam=vec), match="gamma and beta")
    refused(*ex(ldw=127), match="bad arguments")
    assert bool((out == SENT).all())


# ================================================================================================ LayerNorm rows, every implementation
def _ln_case(M):
    x = R.ln_rows(M)
    _W, _b, gamma, beta = R.linear_params(1)
    r64, s64 = R.layer_norm(x, gamma, beta, dtype=F64)
    r32, s32 = R.layer_norm(x, gamma, beta, dtype=F32)
    return x, gamma, beta, r64, s64, r32, s32


def _check_ln(group, where, y, stats, case, add=None):
    x, gamma, beta, r64, s64, r32, s32 = case
    if add is not None:
        r64, r32 = r64 + add.double(), r32 + add
    check_classes(group, where, y, r64, r32, ln_scale(r64), R.LN_CLASSES)
    if stats is not None:
        check_stats(group + " stats", where, stats, s64, s32, R.LN_CLASSES)
    if add is None:       # a constant row: the centred row is exactly 0, the output exactly beta
        const = y[2::8]
        assert same_bits(const, cuda(beta).expand_as(const).contiguous()), where


@pytest.mark.parametrize("M", (1, 8, 67, 65537))
def test_layernorm_rows_ln128_fwd(M):
    """csplat_ln128_fwd on rows of mean 16 and 64 with std 1/16 (where E[x^2] - mean^2 is off by 1e-2 and 0.25), constant rows, var << eps
    and three scales side by side; below one workgroup, below and beyond ln_blocks' cap"""
    case = _ln_case(M)
    xc, gc, bc = cuda(case[0]), cuda(case[1]), cuda(case[2])
    outs = []
    for _ in range(2):
        y, stats = filled(M + 1, 128), filled(M + 1, 2)
        call("csplat_ln128_fwd", M, P(xc), P(gc), P(bc), R.EPS, P(y), P(stats))
        assert bool((y[M] == SENT).all()) and bool((stats[M] == SENT).all())
        outs.append((y[:M], stats[:M]))
    assert same_bits(outs[0][0], outs[1][0]) and same_bits(outs[0][1], outs[1][1])
    _check_ln("ln128_fwd", f"M {M}", outs[0][0], outs[0][1], case)


def test_layernorm_rows_rows32_and_persistent_epilogues():
    """the same rows through the LayerNorm epilogues of the Linear kernels, with W = the identity (every product is exact in both
    product modes: the row in front of the LayerNorm is the input row): rows32<true>, k_linear128<false, true, false, B3> and
    k_linear128<false, true, true, B3> (add_post behind the LayerNorm) in both modes"""
    eye = torch.eye(128)
    for M, modes in ((67, (1,)), (65537, (0, 1))):
        case = _ln_case(M)
        xc, ln_g = cuda(case[0]), (cuda(case[1]), cuda(case[2]))
        post = R.addends(M)[1]
        for mode in modes:
            set_mode(mode)
            kind = "rows32" if M == 67 else f"persistent mode {mode}"
            y, stats = linear_ex(xc, eye, "plain", ln=ln_g, want_stats=True)
            _check_ln(f"LN rows {kind}", f"M {M}", y, stats, case)
            y, stats = linear_ex(xc, eye, "transpose", ln=ln_g, add_post=cuda(post), want_stats=True)
            _check_ln(f"LN rows {kind}", f"M {M} + add_post", y, stats, case, add=post)


def _node_update(N, agg, x, p, with_next=True):
    g = {k: cuda(v) for k, v in p.items()}
    xn, xa, xb = filled(N + 1, 128), filled(N + 1, 128), filled(N + 1, 128)
    call("csplat_gnn_node_update", N, P(agg), P(x), P(g["Wa"]), P(g["Wx"]), P(g["b0"]), P(g["W2"]), P(g["b2"]), P(g["W3"]), P(g["b3"]),
         P(g["gamma"]), P(g["beta"]), R.EPS, P(g["Wi"]) if with_next else None, P(g["Wj"]) if with_next else None, P(xn),
         P(xa) if with_next else None, P(xb) if with_next else None)
    for t in (xn, xa, xb):
        assert bool((t[N] == SENT).all())
    if not with_next:
        assert bool((xa == SENT).all()) and bool((xb == SENT).all())
    return xn[:N], xa[:N], xb[:N]


@pytest.mark.parametrize("N", (1, 33, 1031))
def test_node_update_rows_and_layernorm(N):
    """csplat_gnn_node_update: (a) aggregates and node rows of scale 1e-3 / 1 / 1e+3 side by side, x', xa', xb' held per row; (b) W3 = 0
    and a chosen bias row in front of its LayerNorm, so that every x' row is LN(b3) + x: mean 16 and 64 with std 1/16, var << eps
    (1 + 1e-4 randn), and the constant rows (var = 0: the centred row is exactly 0, LN(b3) is exactly beta, and x' is the ONE float32
    addition beta + x bit for bit -- x' - x itself is not beta's bits, the addition rounds)"""
    g = torch.Generator().manual_seed(N)
    sc = torch.tensor([1e-3, 1.0, 1e3])[torch.arange(N) % 3][:, None]
    agg, x = torch.randn(N, 128, generator=g) * sc, torch.randn(N, 128, generator=g) * sc
    names = ("1e-3", "1", "1e+3")
    p = R.node_update_params()
    got = _node_update(N, cuda(agg), cuda(x), p)
    r64, r32 = R.node_update(agg, x, p, F64), R.node_update(agg, x, p, F32)
    # x' = LN(.) + x: a normalised row of O(1) plus the residual.  xa', xb' = x' W^T: the scale of a product's terms
    check_classes("node_update x'", f"N {N}", got[0], r64[0], r32[0], torch.maximum(ln_scale(r64[0]), x.double().abs().amax(1)), names)
    for k, w in ((1, "Wi"), (2, "Wj")):
        check_classes("node_update xa' xb'", f"N {N} {w}", got[k], r64[k], r32[k], (r64[0].abs() @ p[w].double().abs().t()).amax(1), names)
    for a, b in zip(got, _node_update(N, cuda(agg), cuda(x), p)):
        assert same_bits(a, b)
    assert same_bits(_node_update(N, cuda(agg), cuda(x), p, with_next=False)[0], got[0])
    x1 = torch.randn(N, 128, generator=g)
    aggc, x1c = cuda(agg), cuda(x1)
    for what, row in (("mean 16", 16.0), ("mean 64", 64.0), ("var << eps", R.small_variance_row())):
        p = R.node_update_params(hard=row)
        got = _node_update(N, aggc, x1c, p)[0]
        ln64, ln32 = (R.layer_norm(p["b3"][None], p["gamma"], p["beta"], dtype=dt)[0] for dt in (F64, F32))
        check_rows("node_update LN(b3)", f"N {N} {what}", got.cpu().double() - x1.double(), ln64.expand(N, 128),
                   (ln32 + x1).double() - x1.double(), ln_scale(ln64))
    for const in R.LN_CONSTANTS:
        p = R.node_update_params(hard=torch.full((128,), const))
        got = _node_update(N, aggc, x1c, p)
        assert same_bits(got[0], cuda(p["beta"] + x1)), (N, const)
        assert torch.equal(R.layer_norm(p["b3"][None], p["gamma"], p["beta"], dtype=F32)[0][0], p["beta"])


def test_fused_piece_chains_layernorm_of_a_hard_bias_row():
    """csplat_gnn_edge_mlp3, csplat_gnn_mlp3_rows, csplat_gnn_node_update_packed: the last layer has zero weights and a bias row of mean
    16, std 1/16, so every row in front of the LayerNorm is that bias row whatever the 16-bit pieces do.  csplat_gnn_rows_chain has no
    LayerNorm: its last layer's output is relu(bias) = the bias row itself, bit for bit.  Nothing else about these kernels is held here."""
    from meshnet import graph_ops as go
    E, N = 257, 61
    g = torch.Generator().manual_seed(5)
    W0, W1 = (torch.randn(128, 128, generator=g) / 128 ** 0.5 for _ in range(2))
    zero = torch.zeros(128, 128)
    b0, b1 = 0.1 * torch.randn(128, generator=g), 0.1 * torch.randn(128, generator=g)
    hard = R.hard_bias(16.0)
    _W, _b, gamma, beta = R.linear_params(2)
    ln = torch.nn.LayerNorm(128, eps=R.EPS).cuda()
    with torch.no_grad():
        ln.weight.copy_(gamma)
        ln.bias.copy_(beta)
    ln64, ln32 = (R.layer_norm(hard[None], gamma, beta, dtype=dt)[0] for dt in (F64, F32))
    e0, xa, xb = torch.randn(E, 128, generator=g), torch.randn(N, 128, generator=g), torch.randn(N, 128, generator=g)
    ia, ib = torch.randint(0, N, (E,), generator=g), torch.randint(0, N, (E,), generator=g)
    assert go.edge_mlp3_mode() == 0
    with torch.no_grad():
        img = go.edge_mlp3_pack(cuda(W0), cuda(W1), cuda(zero))
        out = go.edge_mlp3(cuda(e0), 2.0, cuda(xa), cuda(ia), cuda(xb), cuda(ib), img, cuda(b0), cuda(b1), cuda(hard), ln)
        check_rows("fused chains LN(bias)", "edge_mlp3", out, ln64.expand(E, 128), ln32.expand(E, 128), ln_scale(ln64))
        x8 = torch.randn(E, 8, generator=g)
        W0n = torch.zeros(128, 128)
        W0n[:, :8] = torch.randn(128, 8, generator=g) / 8 ** 0.5
        img = go.edge_mlp3_pack(cuda(W0n), cuda(W1), cuda(zero))
        out = go.mlp3_rows(cuda(x8), img, cuda(b0), cuda(b1), cuda(hard), ln)
        check_rows("fused chains LN(bias)", "mlp3_rows", out, ln64.expand(E, 128), ln32.expand(E, 128), ln_scale(ln64))
        agg, x = torch.randn(N, 128, generator=g), torch.randn(N, 128, generator=g)
        img = go.node_update_pack(cuda(W0), cuda(W1), cuda(W0), cuda(zero))
        xn, _, _ = go.node_update_packed(cuda(agg), cuda(x), img, cuda(b0), cuda(b1), cuda(hard), ln, False)
        check_rows("fused chains LN(bias)", "node_update_packed", xn.cpu().double() - x.double(), ln64.expand(N, 128),
                   (ln32 + x).double() - x.double(), ln_scale(ln64))
        img = go.rows_chain_pack(1, cuda(W0), cuda(zero))
        out = go.rows_chain(cuda(x), img, 1, cuda(b0), cuda(hard))
        assert same_bits(out, cuda(hard).expand(N, 128).contiguous())


# ================================================================================================ csplat_ln128_bwd, csplat_relu_mask_bias128
def _ln_bwd(M, g, x, stats, gamma, g_rows=None, x_normalized=False, want_dxsum=True):
    from csplat import native as n
    dx, dg, db, dxs = filled(M + 1, 128), filled(128), filled(128), filled(128)
    part = torch.empty(3 * int(n.lib.csplat_ln128_partial_floats(M)), device="cuda")
    call("csplat_ln128_bwd", M, P(g), P(x), P(stats), P(gamma), P(dx), P(dg), P(db), P(dxs) if want_dxsum else None, P(g_rows),
         int(x_normalized), P(part))
    assert bool((dx[M] == SENT).all()) and (want_dxsum or bool((dxs == SENT).all()))
    return dx[:M], dg, db, dxs


@pytest.mark.parametrize("M", R.LN_BWD_M)
def test_ln128_bwd_row_classes_g_rows_and_x_normalized(M):
    """csplat_ln128_bwd on the LayerNorm rows, the incoming gradient at scales 1e-3 / 1 / 1e+3: dx per row, dgamma / dbeta / dxsum per
    column; the gradient read through g_rows (repeated rows, every row the same one) has the bits of the gathered copy;
    x_normalized = 1 on xhat (the call the fused message path makes) against the plain form"""
    x, gamma, _beta, _r64, _s64, _r32, s32 = _ln_case(M)
    gen = torch.Generator().manual_seed(M)
    g = torch.randn(M, 128, generator=gen) * torch.tensor([1.0, 1e-3, 1e3])[(torch.arange(M) // 8) % 3][:, None]
    xc, gc, sc, gac = cuda(x), cuda(g), cuda(s32), cuda(gamma)
    got = _ln_bwd(M, gc, xc, sc, gac)
    for a, b in zip(got, _ln_bwd(M, gc, xc, sc, gac)):
        assert same_bits(a, b)

    def hold(group, where, got, args, kw):
        r64, r32 = R.layer_norm_bwd(*args, dtype=F64, **kw), R.layer_norm_bwd(*args, dtype=F32, **kw)
        gg = args[0].double() if kw.get("g_rows") is None else args[0].double()[kw["g_rows"]]
        xhat = args[1].double() if kw.get("x_normalized") else (args[1].double() - args[2][:, 0:1].double()) * args[2][:, 1:2].double()
        check_classes(f"{group} dx", where, got[0], r64[0], r32[0], args[2][:, 1].double() * (gg * gamma.double()).abs().amax(1), R.LN_CLASSES)
        check_columns(f"{group} dgamma", where, got[1], r64[1], r32[1], (gg * xhat).abs().sum(0))
        check_columns(f"{group} dbeta", where, got[2], r64[2], r32[2], gg.abs().sum(0))
        check_columns(f"{group} dxsum", where, got[3], r64[3], r32[3], r64[0].abs().sum(0))
    hold("ln128_bwd", f"M {M}", got, (g, x, s32, gamma), {})
    assert same_bits(_ln_bwd(M, gc, xc, sc, gac, want_dxsum=False)[0], got[0])
    # through a row index
    Rr = max(M // 3, 1)
    small = torch.randn(Rr, 128, generator=gen)
    for rows in (torch.randint(0, Rr, (M,), generator=gen), torch.full((M,), Rr - 1, dtype=torch.int64)):
        via = _ln_bwd(M, cuda(small), xc, sc, gac, g_rows=cuda(rows))
        for a, b in zip(via, _ln_bwd(M, cuda(small[rows]), xc, sc, gac)):
            assert same_bits(a, b)
    hold("ln128_bwd g_rows", f"M {M}", via, (small, x, s32, gamma), dict(g_rows=rows))
    # x_normalized: xhat as the LayerNorm epilogue of the Linear leaves it (float32)
    xhat = R.layer_norm(x, torch.ones(128), torch.zeros(128), dtype=F32)[0]
    got_n = _ln_bwd(M, gc, cuda(xhat), sc, gac, x_normalized=True)
    hold("ln128_bwd x_normalized", f"M {M}", got_n, (g, xhat, s32, gamma), dict(x_normalized=True))
    # and ignoring the flag is not the same thing: the plain form on xhat would centre and scale it again
    plain64 = R.layer_norm_bwd(g, xhat, s32, gamma, dtype=F64)[0]
    norm64 = R.layer_norm_bwd(g, xhat, s32, gamma, x_normalized=True, dtype=F64)[0]
    assert M == 1 or float((plain64 - norm64).abs().max()) > 1e-2 * float(norm64.abs().max())


@pytest.mark.parametrize("M", R.LN_BWD_M)
def test_relu_mask_bias128(M):
    """csplat_relu_mask_bias128: the masked gradient is a copy or an exact 0 (out negative, +0, -0: not positive), its column sums per column;
    without a mask; sums only"""
    from csplat import native as n
    gen = torch.Generator().manual_seed(M + 1)
    g = torch.randn(M, 128, generator=gen) * torch.tensor([1.0, 1e-3, 1e3])[torch.arange(M) % 3][:, None]
    out = torch.randn(M, 128, generator=gen)
    out[:, 3], out[:, 70] = 0.0, -0.0
    gc, oc = cuda(g), cuda(out)
    part = torch.empty(int(n.lib.csplat_ln128_partial_floats(M)), device="cuda")
    for use_out in (True, False):
        gm, db = filled(M + 1, 128), filled(128)
        call("csplat_relu_mask_bias128", M, P(gc), P(oc) if use_out else None, P(gm), P(db), P(part))
        assert bool((gm[M] == SENT).all())
        r64, r32 = R.relu_mask_bias(g, out if use_out else None, F64), R.relu_mask_bias(g, out if use_out else None, F32)
        assert same_bits(gm[:M], cuda(r32[0]))
        check_columns("relu_mask_bias128 dbias", f"M {M} mask {use_out}", db, r64[1], r32[1], r64[0].abs().sum(0))
        db2 = filled(128)
        call("csplat_relu_mask_bias128", M, P(gc), P(oc) if use_out else None, None, P(db2), P(part))
        assert same_bits(db, db2)


# ================================================================================================ CSR, segment sum, edge combine, row gather
def _build_csr(keys, N):
    from csplat import native as n
    E = int(keys.numel())
    rowptr = torch.full((N + 2,), -7, dtype=torch.int32, device="cuda")
    perm = torch.full((E + 1,), -7, dtype=torch.int32, device="cuda")
    tmp = torch.empty(max(int(n.lib.csplat_gnn_csr_temp_bytes(N, E)), 256), dtype=torch.uint8, device="cuda")
    call("csplat_gnn_build_csr", N, E, P(keys), P(rowptr), P(perm), P(tmp))
    assert int(rowptr[N + 1]) == -7 and int(perm[E]) == -7
    return rowptr[:N + 1].contiguous(), perm[:E].contiguous()


def _segment_sum(N, L, msg, rowptr, perm):
    agg = filled(N + 1, L)
    call("csplat_gnn_segment_sum", N, int(msg.shape[0]), L, P(msg), P(rowptr), P(perm), P(agg))
    assert bool((agg[N] == SENT).all())
    return agg[:N]


def _hold_segment_sum(where, got, msg, keys, N):
    """the table's comparison against the float32 index_add_, and element by element the bound of compensated summation -- on the nodes
    that have edges (the references are formed for those rows only); every other row of the N is exactly 0"""
    nodes, inv = torch.unique(keys, return_inverse=True)
    n = int(nodes.numel())
    empty = torch.ones(N, dtype=torch.bool, device="cuda")
    empty[nodes.cuda()] = False
    assert not bool(got[empty].any()), f"{where}: a node without edges has a sum"
    if n == 0:
        return
    got = got[nodes.cuda()]
    r64, r32 = R.segment_sum(msg, inv, n, F64), R.segment_sum(msg, inv, n, F32)
    sabs = R.segment_abs_sum(msg, inv, n)
    check_rows("segment_sum", where, got, r64, r32, sabs.amax(1))
    deg = torch.bincount(inv, minlength=n).double()[:, None]
    bound = EPS32 * r64.abs() + deg * EPS32 ** 2 * sabs
    excess = (got.cpu().double() - r64).abs() - bound
    assert float(excess.max()) <= 0.0, f"{where}: {float(excess.max()):.3e} beyond eps |sum| + n eps^2 sum |x|"


@pytest.mark.parametrize("N", R.CSR_N)
def test_csr_segment_sum_edge_combine_gather(N):
    """csplat_gnn_build_csr (node counts around the scan's tile of 2048, two and many tiles; no edges; a hub of 3000 edges for k_sort_rows,
    which k_fill's atomics leave nearly sorted: its worst case, a reversed row, is 4.5e6 moves by one thread), csplat_gnn_segment_sum
    (degrees 0..9: every residue of the four-at-a-time loop; widths on the float4 and the scalar path; cancelling messages; exact zeros),
    edge combine forward / backward and the row gather on the same graphs.  At N = 70 001 (many workgroups of every kernel) only the widths
    128 and 6 -- one float4 and one scalar width; 32 and 20 take the same two kernels with another LV -- and no 'zeros' messages are run:
    neither changes a launch there"""
    big = N > 4097
    for kind in (None,) + R.GRAPHS:
        ei = torch.zeros(2, 0, dtype=torch.int64) if kind is None else R.graph(N, kind)
        E = int(ei.shape[1])
        eic = cuda(ei)
        csr = {}
        for name, row in (("src", 0), ("dst", 1)):
            rp, pm = _build_csr(eic[row].contiguous(), N)
            ref_rp, ref_pm = R.csr_fast(ei[row].numpy(), N)
            np.testing.assert_array_equal(rp.cpu().numpy(), ref_rp, err_msg=f"N {N} {kind} {name} rowptr")
            np.testing.assert_array_equal(pm.cpu().numpy(), ref_pm, err_msg=f"N {N} {kind} {name} perm")
            csr[name] = (rp, pm)
        for L in ((128, 6) if big else R.WIDTHS):
            for mk in (R.MESSAGES[:2] if big else R.MESSAGES):
                if E == 0 and mk != "ordinary":
                    continue
                where = f"N {N} {kind} L {L} {mk}"
                msg = R.messages(ei, L, mk)
                mc = cuda(msg)
                agg = _segment_sum(N, L, mc, *csr["dst"])
                assert same_bits(agg, _segment_sum(N, L, mc, *csr["dst"])), where
                _hold_segment_sum(where, agg, msg, ei[1], N)
            if E == 0:
                continue
            # edge combine forward: two float32 additions in a fixed order -- equality; backward: the masked gradient is a copy or 0
            g = torch.Generator().manual_seed(N + L)
            xa, xb, ec, gh = (torch.randn(n_, L, generator=g) for n_ in (N, N, E, E))
            ec[0::5] = -ec[0::5].abs() - 3.0          # (rows the ReLU switches off almost entirely)
            xac, xbc, ecc, ghc, dst_c = cuda(xa), cuda(xb), cuda(ec), cuda(gh), eic[1].contiguous()
            for relu in (0, 1):
                out = filled(E + 1, L)
                call("csplat_gnn_edge_combine_fwd", N, E, L, P(eic), P(xac), P(xbc), P(ecc), relu, P(out))
                ref = R.edge_combine(xa, xb, ec, ei, relu, F32)
                assert bool((out[E] == SENT).all()) and same_bits(out[:E], cuda(ref)), f"N {N} {kind} L {L} relu {relu}"
                gm, dxa, dxb = filled(E + 1, L), filled(N + 1, L), filled(N + 1, L)
                fwd_out = out[:E].contiguous()
                call("csplat_gnn_edge_combine_bwd", N, E, L, P(ghc), P(fwd_out), relu, P(csr["dst"][0]), P(csr["dst"][1]),
                     P(csr["src"][0]), P(csr["src"][1]), P(gm), P(dxa), P(dxb))
                m64 = R.edge_combine_bwd(gh, ref, ei, N, relu, F32)[0]
                assert bool((gm[E] == SENT).all()) and bool((dxa[N] == SENT).all()) and bool((dxb[N] == SENT).all())
                assert same_bits(gm[:E], cuda(m64)) if relu else bool((gm == SENT).all())
                _hold_segment_sum(f"N {N} {kind} L {L} dxa relu {relu}", dxa[:N], m64, ei[1], N)
                _hold_segment_sum(f"N {N} {kind} L {L} dxb relu {relu}", dxb[:N], m64, ei[0], N)
            rows = filled(E + 1, L)
            call("csplat_gnn_gather_rows", E, L, P(xac), P(dst_c), P(rows))
            assert bool((rows[E] == SENT).all()) and same_bits(rows[:E], cuda(xa[ei[1]]))


def _parent_cases():
    for kind in R.GRAPHS:
        ei = R.graph(300, kind)
        for L in (32, 6):
            for mk in R.MESSAGES:
                yield f"{kind}_{L}_{mk}".replace(" ", "_").replace("..", "to"), ei, L, R.messages(ei, L, mk)


def test_segment_sum_finite_sums_keep_the_bits_of_the_build_before_the_inf_rule():
    """every finite sum has the bits k_segment_sum gave before an unbounded running sum was returned on its own
    (tests/golden/make_segment_sum_bits.py: a build of the parent commit on these inputs)"""
    parent = util.golden("segment_sum_parent_bits.npz")
    for name, ei, L, msg in _parent_cases():
        rp, pm = _build_csr(cuda(ei[1]), 300)
        agg = _segment_sum(300, L, cuda(msg), rp, pm)
        np.testing.assert_array_equal(bits(agg).cpu().numpy(), parent[name], err_msg=name)


# ================================================================================================ narrow Linear, dw128
@pytest.mark.parametrize("M", R.NARROW_M)
def test_linear_narrow_strided_inputs(M):
    """csplat_linear_narrow128 with ldx > K and ldw > K (column slices of wider arrays), K = 1, odd, the limit; one pass of 64 rows, one
    more row, and one row beyond the 2048 x 64 rows of the capped grid's first sweep; rows at three scales"""
    for Kk in R.NARROW_K:
        g = torch.Generator().manual_seed(M + Kk)
        ldx, ldw = Kk + 3, Kk + 5
        xw = torch.randn(M, ldx, generator=g) * torch.tensor([1.0, 1e-3, 1e3])[torch.arange(M) % 3][:, None]
        Ww, b = torch.randn(128, ldw, generator=g), torch.randn(128, generator=g)
        xw[:, Kk:], Ww[:, Kk:] = 1e30, 1e30           # (what lies beside the slices must not be read)
        x, W = xw[:, :Kk], Ww[:, :Kk]
        xwc, Wwc, bcu = cuda(xw), cuda(Ww), cuda(b)
        for relu in (0, 1):
            for bias in (b, None):
                out = filled(M + 1, 128)
                call("csplat_linear_narrow128", M, Kk, P(xwc), ldx, P(Wwc), ldw, P(bcu) if bias is not None else None, relu, P(out))
                assert bool((out[M] == SENT).all())
                r64, r32 = R.linear_narrow(x, W, bias, relu, F64), R.linear_narrow(x, W, bias, relu, F32)
                scale = x.double().abs() @ W.double().abs().t() + (0 if bias is None else bias.double().abs())
                check_classes("linear_narrow", f"M {M} K {Kk} relu {relu} bias {bias is not None}", out[:M], r64, r32, scale.amax(1),
                              ("1", "1e-3", "1e+3"))


@pytest.mark.parametrize("M", R.DW_M)
def test_dw128_row_classes_and_x_relu(M):
    """csplat_dw128_bias: what tests/test_knn_gnn_gpu.py's sweep over M lacks -- gradient rows of every class against activations of every
    LayerNorm class, element by element relative to sum_e |g||x|; x_relu on activations with negative, +0 and -0 entries"""
    from csplat import native as n
    g, x = R.row_classes(M, seed=1), R.ln_rows(M, seed=1)
    g[4::8] *= 1e20          # (rows of 1e-30 would vanish from every sum: 1e-10 here)
    g[5::8] *= 1e-10         # (and 1e+20 rows would own every column: 1e+10)
    x[:, 7], x[:, 90] = 0.0, -0.0
    x[1::2, 11] = -x[1::2, 11].abs() - 1.0
    gc, xc = cuda(g), cuda(x)
    ws = torch.empty(max(int(n.lib.csplat_dw128_workspace_bytes(M)), 256), dtype=torch.uint8, device="cuda")
    for x_relu in (0, 1):
        dW, db = filled(129, 128), filled(128)
        call("csplat_dw128_bias", M, P(gc), P(xc), x_relu, P(dW), P(db), P(ws))
        assert bool((dW[128] == SENT).all())
        r64, r32 = R.dw128(g, x, bool(x_relu), F64), R.dw128(g, x, bool(x_relu), F32)
        xs = torch.relu(x.double()) if x_relu else x.double()
        scale = g.double().abs().t() @ xs.abs()
        got, a, b = dW[:128].cpu().double(), r64[0], r32[0].double()
        live = scale > 0
        assert not bool(got[~live].any())              # a column of activations the ReLU switches off entirely: exactly 0
        check_rows("dw128 dW", f"M {M} x_relu {x_relu}", (got / scale.clamp_min(1e-300)), (a / scale.clamp_min(1e-300)),
                   (b / scale.clamp_min(1e-300)), 1.0)
        check_columns("dw128 dbias", f"M {M} x_relu {x_relu}", db, r64[1], r32[1], g.double().abs().sum(0))
        dW2, db2 = filled(128, 128), filled(128)
        call("csplat_dw128_bias", M, P(gc), P(xc), x_relu, P(dW2), P(db2), P(ws))
        assert same_bits(dW[:128], dW2) and same_bits(db, db2)


# ================================================================================================ NaN and Inf data
@pytest.mark.parametrize("M,mode", [(33, 1), (65537, 0), (65537, 1)])
def test_linear128_nan_and_inf_poison_exactly_what_reads_them(M, mode):
    """one NaN, one +Inf and one -Inf in a row of A: that row and no other; one NaN / Inf in W: that output column and no other.  The fp32
    products give torch's own values there (+-Inf where F.linear gives +-Inf); the bf16 split is held to non-finite (module docstring)"""
    set_mode(mode)
    split = mode == 1 and M > 65536
    g = torch.Generator().manual_seed(3)
    A, (W, bias, gamma, beta) = torch.randn(M, 128, generator=g), R.linear_params()
    bc = cuda(bias)
    clean, _ = linear_ex(cuda(A), W, bias=bc, alpha=0.5, relu=False)
    row = M - 2 if M > 2 else 0
    for value in (float("nan"), float("inf"), float("-inf")):
        A2 = A.clone()
        A2[row, 77] = value
        out, _ = linear_ex(cuda(A2), W, bias=bc, alpha=0.5, relu=False)
        keep = torch.arange(M, device="cuda") != row
        assert same_bits(out[keep], clean[keep]) and not bool(torch.isfinite(out[row]).any()), (M, mode, value)
        ref = torch.nn.functional.linear(A2[row:row + 1], W) * 0.5 + bias
        assert split or same_values_and_nans(out[row:row + 1], ref), (M, mode, value)
        out, _ = linear_ex(cuda(A2), W, bias=bc, alpha=0.5, relu=True, ln=(cuda(gamma), cuda(beta)))     # ReLU keeps the NaN; LN(Inf) is NaN
        assert bool(torch.isnan(out[row]).all()) and bool(torch.isfinite(out[keep]).all()), (M, mode, value)
    col = 45
    for value in (float("nan"), float("inf")):
        W2 = W.clone()
        W2[col, 9] = value
        out, _ = linear_ex(cuda(A), W2, bias=bc, alpha=0.5, relu=False)
        keep = torch.arange(128, device="cuda") != col
        assert same_bits(out[:, keep], clean[:, keep]) and not bool(torch.isfinite(out[:, col]).any()), (M, mode, value)
        ref = torch.nn.functional.linear(A, W2[col:col + 1]) * 0.5 + bias[col]
        assert split or same_values_and_nans(out[:, col:col + 1], ref), (M, mode, value)


def test_segment_sum_an_inf_stays_an_inf():
    """a message of +-Inf, and a sum that overflows, give what index_add_ gives (Inf; NaN only for Inf - Inf and for a NaN), on the float4
    and on the scalar path, in the four-at-a-time loop and in its tail; every other row keeps the bits of the clean run"""
    N = 40
    inf, nan = float("inf"), float("nan")
    rows = {3: [1.0, inf, 2.0], 5: [1.0, -inf, 2.0], 7: [3e38, 3e38, 1.0], 9: [inf, 1.0, -inf], 11: [1.0, nan, 2.0],
            13: [1.0, 2.0, 3.0, 4.0, inf, 5.0], 15: [-3e38, -3e38, -3e38, -3e38, 1.0], 17: [inf], 19: [1.0, 2.0, 3.0, inf]}
    dst = torch.tensor([n_ for n_, v in rows.items() for _ in v] + list(range(20, 40)) * 3)
    for L in (8, 6):
        g = torch.Generator().manual_seed(L)
        msg = torch.randn(dst.numel(), L, generator=g)
        clean_msg = msg.clone()
        at = 0
        for n_, v in rows.items():
            msg[at:at + len(v), 1] = torch.tensor(v)
            at += len(v)
        rp, pm = _build_csr(cuda(dst), N)
        got, clean = _segment_sum(N, L, cuda(msg), rp, pm), _segment_sum(N, L, cuda(clean_msg), rp, pm)
        ref = R.segment_sum(msg, dst, N, F32)
        touched = torch.zeros(N, L, dtype=torch.bool)
        touched[list(rows), 1] = True
        assert same_values_and_nans(got.cpu()[touched], ref[touched]), (L, got.cpu()[touched], ref[touched])
        assert [float(x) for x in got.cpu()[[3, 5, 7, 13, 15, 17, 19], 1]] == [inf, -inf, inf, inf, -inf, inf, inf]
        assert bool(torch.isnan(got[[9, 11], 1]).all())
        assert same_bits(got[cuda(~touched)], clean[cuda(~touched)])


def test_layernorm_dw_combine_and_gather_nan_and_inf():
    """csplat_ln128_fwd / _bwd, csplat_gnn_node_update, csplat_dw128_bias, csplat_linear_narrow128, csplat_relu_mask_bias128,
    csplat_gnn_edge_combine_fwd / _bwd, csplat_gnn_gather_rows: one NaN / Inf
    in an input reaches exactly the outputs that read it, as torch's own ops have it"""
    from csplat import native as n
    M = 67
    x, gamma, beta, _r64, _s64, _r32, s32 = _ln_case(M)
    gc, bc = cuda(gamma), cuda(beta)

    def fwd(xx):
        y, stats, xxc = filled(M, 128), filled(M, 2), cuda(xx)
        call("csplat_ln128_fwd", M, P(xxc), P(gc), P(bc), R.EPS, P(y), P(stats))
        return y
    clean = fwd(x)
    keep = torch.arange(M, device="cuda") != 40
    for value in (float("nan"), float("inf")):
        x2 = x.clone()
        x2[40, 3] = value
        y = fwd(x2)
        assert bool(torch.isnan(y[40]).all()) and same_bits(y[keep], clean[keep])          # (torch: LN of a row with an Inf is NaN)
        assert bool(torch.isnan(torch.nn.functional.layer_norm(x2, (128,), gamma, beta, R.EPS)[40]).all())
    g = torch.randn(M, 128, generator=torch.Generator().manual_seed(1))
    dclean = _ln_bwd(M, cuda(g), cuda(x), cuda(s32), gc)
    g2 = g.clone()
    g2[40, 3] = float("nan")
    d = _ln_bwd(M, cuda(g2), cuda(x), cuda(s32), gc)
    assert bool(torch.isnan(d[0][40]).all()) and same_bits(d[0][keep], dclean[0][keep])
    kc = torch.arange(128, device="cuda") != 3
    for k in (1, 2):
        assert bool(torch.isnan(d[k][3])) and same_bits(d[k][kc], dclean[k][kc])
    assert bool(torch.isnan(d[3]).all())               # (every column of dx row 40 is NaN)
    # node update: a NaN in a node row
    p = R.node_update_params()
    agg = torch.randn(M, 128, generator=torch.Generator().manual_seed(2))
    nclean = _node_update(M, cuda(agg), cuda(x), p)
    x2 = x.clone()
    x2[40, 3] = float("nan")
    ngot = _node_update(M, cuda(agg), cuda(x2), p)
    for a, b in zip(ngot, nclean):
        assert bool(torch.isnan(a[40]).all()) and same_bits(a[keep], b[keep])
    # dw128: a NaN / Inf in gradient row 5, column 9: row 9 of dW and dbias[9]
    ws = torch.empty(max(int(n.lib.csplat_dw128_workspace_bytes(M)), 256), dtype=torch.uint8, device="cuda")

    def dw(gg):
        dW, db, ggc, xc_ = filled(128, 128), filled(128), cuda(gg), cuda(x)
        call("csplat_dw128_bias", M, P(ggc), P(xc_), 0, P(dW), P(db), P(ws))
        return dW, db
    wclean = dw(g)
    kr = torch.arange(128, device="cuda") != 9
    for value in (float("nan"), float("inf")):
        g2 = g.clone()
        g2[5, 9] = value
        dW, db = dw(g2)
        assert same_bits(dW[kr], wclean[0][kr]) and same_bits(db[kr], wclean[1][kr])
        ref = R.dw128(g2, x, False, F32)
        assert same_values_and_nans(dW[9], ref[0][9]) and same_values_and_nans(db[9:10], ref[1][9:10])
        assert not bool(torch.isfinite(dW[9]).any())
    # narrow Linear: row 5 reads the value, no other row does
    Kk, ldx = 5, 8
    gen = torch.Generator().manual_seed(7)
    xw, Wn, bn = torch.randn(M, ldx, generator=gen), torch.randn(128, Kk, generator=gen), torch.randn(128, generator=gen)
    Wnc, bnc = cuda(Wn), cuda(bn)

    def narrow(xx):
        out, xxc = filled(M, 128), cuda(xx)
        call("csplat_linear_narrow128", M, Kk, P(xxc), ldx, P(Wnc), Kk, P(bnc), 0, P(out))
        return out
    nclean = narrow(xw)
    k5 = torch.arange(M, device="cuda") != 5
    for value in (float("nan"), float("inf"), float("-inf")):
        x2 = xw.clone()
        x2[5, 2] = value
        out = narrow(x2)
        assert same_bits(out[k5], nclean[k5]) and same_values_and_nans(out[5:6], R.linear_narrow(x2[5:6, :Kk], Wn, bn, False, F32))
        assert not bool(torch.isfinite(out[5]).any())
    # relu_mask_bias128: a NaN / Inf gradient under a live unit reaches gm there and its column's sum; under a dead unit (and under
    # a NaN activation, which is not > 0) it is masked to 0, as torch.where has it
    part = torch.empty(int(n.lib.csplat_ln128_partial_floats(M)), device="cuda")
    act = torch.randn(M, 128, generator=gen)
    act[5, 9], act[6, 9], act[7, 20], act[8, 30] = 1.0, -1.0, 1.0, float("nan")

    def rmb(gg, oo):
        gm, db, ggc, ooc = filled(M, 128), filled(128), cuda(gg), cuda(oo)
        call("csplat_relu_mask_bias128", M, P(ggc), P(ooc), P(gm), P(db), P(part))
        return gm, db
    rclean = rmb(g, act)
    g2 = g.clone()
    g2[5, 9], g2[6, 9], g2[7, 20] = float("nan"), float("inf"), float("-inf")
    gm, db = rmb(g2, act)
    ref = R.relu_mask_bias(g2, act, F32)
    assert same_values_and_nans(gm, ref[0]) and bool(torch.isnan(gm[5, 9])) and float(gm[6, 9]) == 0.0 and float(gm[8, 30]) == 0.0
    assert bool(torch.isnan(db[9])) and float(db[20]) == float("-inf")
    kc2 = torch.ones(128, dtype=torch.bool, device="cuda")
    kc2[[9, 20]] = False
    assert same_bits(db[kc2], rclean[1][kc2])
    # edge combine and gather: bits of torch's own additions / of the source rows
    ei = R.graph(M, "degrees 0..9")
    E = int(ei.shape[1])
    for L in (128, 6):
        gen = torch.Generator().manual_seed(L)
        xa, xb, ec = torch.randn(M, L, generator=gen), torch.randn(M, L, generator=gen), torch.randn(E, L, generator=gen)
        xa[9, 1], xb[8, 2], ec[4, 3] = float("nan"), float("inf"), float("-inf")
        eic, xac, xbc, ecc, dst_c = cuda(ei), cuda(xa), cuda(xb), cuda(ec), cuda(ei[1])
        for relu in (0, 1):
            out = filled(E, L)
            call("csplat_gnn_edge_combine_fwd", M, E, L, P(eic), P(xac), P(xbc), P(ecc), relu, P(out))
            assert same_values_and_nans(out, R.edge_combine(xa, xb, ec, ei, relu, F32))
        rows = filled(E, L)
        call("csplat_gnn_gather_rows", E, L, P(xac), P(dst_c), P(rows))
        assert same_bits(rows, cuda(xa[ei[1]]))
        # backward: the masked gradient is a copy or 0; the sums of the two nodes an edge joins take its NaN / Inf in that column
        # (what index_add_ gives there), every other sum keeps the bits of the clean run
        rp_d, pm_d = _build_csr(dst_c, M)
        rp_s, pm_s = _build_csr(eic[0].contiguous(), M)
        live = torch.randn(E, L, generator=gen)
        live[[4, 7], :] = 1.0
        gh = torch.randn(E, L, generator=gen)

        def bwd(gg):
            gm, dxa, dxb, ggc, lc = filled(E, L), filled(M, L), filled(M, L), cuda(gg), cuda(live)
            call("csplat_gnn_edge_combine_bwd", M, E, L, P(ggc), P(lc), 1, P(rp_d), P(pm_d), P(rp_s), P(pm_s), P(gm), P(dxa), P(dxb))
            return gm, dxa, dxb
        bclean = bwd(gh)
        gh2 = gh.clone()
        gh2[4, 3], gh2[7, 1] = float("nan"), float("inf")
        got = bwd(gh2)
        ref = R.edge_combine_bwd(gh2, live, ei, M, True, F32)
        assert same_values_and_nans(got[0], ref[0])
        for k, row in ((1, 1), (2, 0)):
            touched = torch.zeros(M, L, dtype=torch.bool)
            touched[ei[row, 4], 3] = touched[ei[row, 7], 1] = True
            assert same_values_and_nans(got[k].cpu()[touched], ref[k][touched]) and not bool(torch.isfinite(got[k].cpu()[touched]).any())
            assert same_bits(got[k][cuda(~touched)], bclean[k][cuda(~touched)])


# ================================================================================================ 16-byte operands
def test_misaligned_operands_are_refused_by_the_entries_and_copied_by_the_wrappers():
    """every operand a kernel reads or writes with 16-byte accesses: the entry refuses a pointer off a 16-byte boundary on the host
    (error return, csplat_last_error says so) before anything is launched -- every output keeps its sentinel --, and the wrappers of
    meshnet/graph_ops.py copy such a view (a contiguous view one float into a larger buffer) and give the bits of the aligned call"""
    from csplat import native as n
    from meshnet import graph_ops as go
    M = 70000            # (the persistent kernels)
    gen = torch.Generator().manual_seed(0)
    A, g, out_prev = (torch.randn(M, 128, generator=gen).cuda() for _ in range(3))
    W, bias, gamma, beta = (cuda(t) for t in R.linear_params())
    out = filled(M, 128)
    sent = [out]

    def ex(bias=None, pre=None, post=None, mask=None, stats=None):
        return ("csplat_linear128_ex", M, P(A), P(W), 128, 0, P(bias), 1.0, 0, None, None, None, None, P(gamma) if stats is not None else None,
                P(beta) if stats is not None else None, R.EPS, P(pre), P(post), P(mask), P(stats), P(out))
    refused(*ex(bias=off_by_one(bias)))
    refused(*ex(pre=off_by_one(g)))
    refused(*ex(post=off_by_one(g)))
    refused(*ex(mask=off_by_one(g)))
    refused(*ex(stats=torch.empty(2 * M + 1, device="cuda")[1:]), match="8-byte")
    stats = cuda(R.layer_norm(A.cpu(), gamma.cpu(), beta.cpu(), dtype=F32)[1])
    dx, dg, db = filled(M, 128), filled(128), filled(128)
    part = torch.empty(3 * int(n.lib.csplat_ln128_partial_floats(M)) + 4, device="cuda")
    sent += [dx, dg, db]

    def lnb(g_=g, x_=A, gamma_=gamma, dx_=dx, part_=part, stats_=stats):
        return ("csplat_ln128_bwd", M, P(g_), P(x_), P(stats_), P(gamma_), P(dx_), P(dg), P(db), None, None, 0, P(part_))
    refused(*lnb(g_=off_by_one(g)))
    refused(*lnb(x_=off_by_one(A)))
    refused(*lnb(gamma_=off_by_one(gamma)))
    refused(*lnb(dx_=off_by_one(dx)))
    refused(*lnb(part_=part[1:]))
    refused(*lnb(stats_=torch.empty(2 * M + 1, device="cuda")[1:]))
    gm = filled(M, 128)
    sent.append(gm)
    refused("csplat_relu_mask_bias128", M, P(off_by_one(g)), P(out_prev), P(gm), P(db), P(part))
    refused("csplat_relu_mask_bias128", M, P(g), P(off_by_one(out_prev)), P(gm), P(db), P(part))
    refused("csplat_relu_mask_bias128", M, P(g), P(out_prev), P(off_by_one(gm)), P(db), P(part))
    refused("csplat_relu_mask_bias128", M, P(g), P(out_prev), P(gm), P(db), P(part[1:]))
    # the row movers: L = 128 moves float4, L = 6 moves floats (any 4-byte boundary will do)
    N = 300
    ei = cuda(R.graph(N, "degrees 0..9"))
    E = int(ei.shape[1])
    csr = go.GraphCSR(ei, N)
    for L in (128, 6):
        xa, xb, ec, gh = (torch.randn(n_, L, generator=gen).cuda() for n_ in (N, N, E, E))
        o_e, o_n, o_n2, o_g = filled(E, L), filled(N, L), filled(N, L), filled(E, L)

        def combine(xa_=xa, xb_=xb, ec_=ec, o_=o_e):
            return ("csplat_gnn_edge_combine_fwd", N, E, L, P(ei), P(xa_), P(xb_), P(ec_), 1, P(o_))

        def combine_bwd(g_=gh, out_=ec, gm_=o_g, dxa_=o_n, dxb_=o_n2):
            return ("csplat_gnn_edge_combine_bwd", N, E, L, P(g_), P(out_), 1, P(csr.rowptr["dst"]), P(csr.perm["dst"]), P(csr.rowptr["src"]),
                    P(csr.perm["src"]), P(gm_), P(dxa_), P(dxb_))
        tries = [combine(xa_=off_by_one(xa)), combine(xb_=off_by_one(xb)), combine(ec_=off_by_one(ec)), combine(o_=off_by_one(o_e)),
                 combine_bwd(g_=off_by_one(gh)), combine_bwd(out_=off_by_one(ec)), combine_bwd(gm_=off_by_one(o_g)),
                 combine_bwd(dxa_=off_by_one(o_n)), combine_bwd(dxb_=off_by_one(o_n2)),
                 ("csplat_gnn_segment_sum", N, E, L, P(off_by_one(ec)), P(csr.rowptr["dst"]), P(csr.perm["dst"]), P(o_n)),
                 ("csplat_gnn_segment_sum", N, E, L, P(ec), P(csr.rowptr["dst"]), P(csr.perm["dst"]), P(off_by_one(o_n))),
                 ("csplat_gnn_gather_rows", E, L, P(off_by_one(xa)), P(ei[1].contiguous()), P(o_e)),
                 ("csplat_gnn_gather_rows", E, L, P(xa), P(ei[1].contiguous()), P(off_by_one(o_e)))]
        if L == 128:
            for t in tries:
                refused(*t)
            for o in (o_e, o_n, o_n2, o_g):
                assert bool((o == SENT).all())
        else:          # scalar rows: accepted wherever they start, same result
            call(*combine())
            want = o_e.clone()
            mxa, mxb, mec = off_by_one(xa), off_by_one(xb), off_by_one(ec)
            call(*combine(xa_=mxa, xb_=mxb, ec_=mec))
            assert same_bits(o_e, want)
            call("csplat_gnn_segment_sum", N, E, L, P(ec), P(csr.rowptr["dst"]), P(csr.perm["dst"]), P(o_n))
            call("csplat_gnn_segment_sum", N, E, L, P(mec), P(csr.rowptr["dst"]), P(csr.perm["dst"]), P(o_n2))
            assert same_bits(o_n, o_n2)
    for o in sent:
        assert bool((o == SENT).all())
    # the wrappers
    unit = torch.nn.LayerNorm(128).cuda()
    with torch.no_grad():
        for mode in (0, 1):
            set_mode(mode)
            want = go.linear128(A, W, bias, alpha=0.5, add_pre=g, add_post=out_prev, mask=g)
            assert same_bits(go.linear128(A, W, off_by_one(bias), alpha=0.5, add_pre=off_by_one(g), add_post=off_by_one(out_prev),
                                          mask=off_by_one(g)), want)
        st = torch.empty(M, 2, device="cuda")
        xhat = go.linear128(A, W, bias, layer_norm=unit, ln_stats=st)
        want = go.ln128_bwd(g, xhat, st, unit.weight, want_dxsum=True, x_normalized=True)
        moved = go.ln128_bwd(off_by_one(g), off_by_one(xhat), st, off_by_one(unit.weight.detach()), want_dxsum=True, x_normalized=True)
        for a, b in zip(want, moved):
            assert same_bits(a, b)
        st4 = torch.empty(2 * M + 1, device="cuda")[1:].view(M, 2)          # (a stats view on a 4-byte boundary: read and written as float2)
        assert st4.data_ptr() % 8 == 4
        assert same_bits(go.linear128(A, W, bias, layer_norm=unit, ln_stats=st4), xhat) and same_bits(st4, st)
        for a, b in zip(want, go.ln128_bwd(g, xhat, st4, unit.weight, want_dxsum=True, x_normalized=True)):
            assert same_bits(a, b)
        for a, b in zip(go.relu_mask_bias128(g, out_prev), go.relu_mask_bias128(off_by_one(g), off_by_one(out_prev))):
            assert same_bits(a, b)
        xa, xb, ec = (torch.randn(n_, 128, generator=gen).cuda() for n_ in (N, N, E))
        assert same_bits(go.gather_rows(off_by_one(xa), ei[1].contiguous()), go.gather_rows(xa, ei[1].contiguous()))
        assert same_bits(go.segment_sum_rows(off_by_one(ec), csr.rowptr["dst"], csr.perm["dst"], N),
                         go.segment_sum_rows(ec, csr.rowptr["dst"], csr.perm["dst"], N))
    leaves = [t.clone().requires_grad_() for t in (xa, xb, ec)]
    moved = [off_by_one(t).requires_grad_() for t in (xa, xb, ec)]
    cot = torch.randn(N, 128, generator=gen).cuda()
    for ts, gr in ((leaves, cot), (moved, off_by_one(cot))):
        go.SegmentSum.apply(go.EdgeCombine.apply(ts[0], ts[1], ts[2], csr, True), csr).backward(gr)
    for a, b in zip(leaves, moved):
        assert same_bits(a.grad, b.grad)
