"""The one-launch kernels of csrc/csplat_edge_mlp.hip -- k_edge_mlp3r<F16, MODE 0 / 1 / 2> (messages, fused aggregation, narrow rows),
k_node_update_b3, k_rows_chain, k_absmax and the two pack kernels -- through meshnet.graph_ops, against tests/edge_mlp_ref.py: the float64
restatement of each operation and the model of the kernels' piece arithmetic, at the sizes where a launch takes another path
(tests/test_edge_mlp_cpu.py states which constant every size crosses), on rows of very different scale inside one launch, at every alpha,
on both weight kinds, on hubs and runs that end on group, tile and step boundaries, on NaN and Inf DATA and on overflows of single rows
(no index, size or pointer is ever garbled, no misaligned operand is ever launched).  Output buffers hold a sentinel before every launch.

Bars, per row and per row class, by the rule of tests/test_gnn_kernels_gpu.py (K = 8, floor 1e-6, a bar above 1e-3 fails by itself):
  every class               kernel against model(acc = float64), e32 = model(acc = float32) against model(acc = float64)
  in-domain classes, also   kernel against exact(float64), e32 = exact(float32) against exact(float64)
(in-domain: tests/edge_mlp_ref.py edge_in_domain / chain_in_domain, held by tests/test_edge_mlp_cpu.py).  A row the model gives as non-finite
in every column must be non-finite in every column; such rows are left out of the comparison.  Row scales: behind a LayerNorm
max(max_j |r64_ij|, 1) (for x' also max_j |x_ij|); without one max_j sum_k |a_ik w_jk| plus the bias magnitude; for a piece of the
aggregation max_j of the sum of |msg| over the rows of its run.

check_rows() prints e32, the bar and the kernel's error; the module's teardown prints the table of the largest of each per group
(pytest -rP shows it).

What the table showed on an MI355X when this file was written (group | comparisons | largest e32 | largest bar | largest kernel error |
smallest bar / error; "vs fp64": the second bar, in-domain classes only; "pieces": the aggregate handed in as pieces):
  Inf in e0 bf16                   |   1 | 5.60e-07 | 4.48e-06 | 4.93e-07 |   9.1
  Inf in e0 f16                    |   1 | 2.90e-07 | 2.32e-06 | 3.81e-07 |   6.1
  fused aggregation                |  44 | 4.79e-07 | 3.83e-06 | 6.33e-07 |   4.3
  launch scale bf16                |  84 | 5.26e-07 | 4.21e-06 | 7.41e-07 |   4.1
  launch scale bf16 vs fp64        |  84 | 5.58e-07 | 4.46e-06 | 7.44e-07 |   2.5
  launch scale f16                 |  84 | 3.68e-05 | 2.95e-04 | 3.69e-05 |   2.6
  launch scale f16 vs fp64         |  18 | 5.58e-07 | 4.46e-06 | 1.79e-06 |   2.5
  messages bf16                    | 382 | 7.09e-07 | 5.67e-06 | 8.64e-07 |   3.7
  messages bf16 vs fp64            | 382 | 9.15e-07 | 7.32e-06 | 8.59e-07 |   1.8
  messages f16                     | 354 | 4.79e-06 | 3.83e-05 | 5.84e-06 |   3.6
  messages f16 vs fp64             | 162 | 7.41e-07 | 5.93e-06 | 2.15e-06 |   2.4
  mlp3_rows                        |  50 | 3.74e-07 | 2.99e-06 | 4.53e-07 |   3.8
  mlp3_rows vs fp64                |  50 | 6.04e-07 | 4.83e-06 | 5.77e-07 |   3.2
  node_update bf16 pieces x'       |  25 | 4.28e-07 | 3.43e-06 | 6.69e-07 |   4.8
  node_update bf16 pieces xa'      |  25 | 1.22e-07 | 1.00e-06 | 1.72e-07 |   5.8
  node_update bf16 pieces xb'      |  25 | 1.19e-07 | 1.00e-06 | 1.58e-07 |   6.3
  node_update bf16 x'              |  50 | 5.35e-07 | 4.28e-06 | 5.61e-07 |   5.1
  node_update bf16 x' vs fp64      |  50 | 3.38e-07 | 2.70e-06 | 5.62e-07 |   3.4
  node_update bf16 xa'             |  25 | 1.50e-07 | 1.20e-06 | 2.00e-07 |   5.0
  node_update bf16 xa' vs fp64     |  25 | 2.70e-07 | 2.16e-06 | 2.00e-07 |   6.8
  node_update bf16 xb'             |  25 | 1.45e-07 | 1.16e-06 | 1.64e-07 |   6.3
  node_update bf16 xb' vs fp64     |  25 | 2.44e-07 | 1.95e-06 | 1.64e-07 |   6.6
  node_update f16 pieces x'        |  25 | 8.55e-07 | 6.84e-06 | 8.51e-07 |   5.7
  node_update f16 pieces xa'       |  25 | 2.10e-07 | 1.68e-06 | 2.64e-07 |   6.4
  node_update f16 pieces xb'       |  25 | 1.90e-07 | 1.52e-06 | 2.01e-07 |   6.8
  node_update f16 x'               |  50 | 8.10e-07 | 6.48e-06 | 7.48e-07 |   6.0
  node_update f16 x' vs fp64       |  50 | 3.38e-07 | 2.70e-06 | 1.03e-06 |   1.8
  node_update f16 xa'              |  25 | 1.89e-07 | 1.51e-06 | 1.99e-07 |   6.0
  node_update f16 xa' vs fp64      |  25 | 2.70e-07 | 2.16e-06 | 2.21e-07 |   5.5
  node_update f16 xb'              |  25 | 1.77e-07 | 1.42e-06 | 2.32e-07 |   6.1
  node_update f16 xb' vs fp64      |  25 | 2.44e-07 | 1.95e-06 | 2.18e-07 |   4.8
  overflow bf16                    |  12 | 2.24e-06 | 1.79e-05 | 4.44e-06 |   4.0
  overflow chain bf16              |   1 | 1.89e-07 | 1.51e-06 | 2.49e-07 |   6.1
  overflow chain f16               |   1 | 1.78e-07 | 1.43e-06 | 2.19e-07 |   6.5
  overflow f16                     |  12 | 2.26e-06 | 1.81e-05 | 3.00e-06 |   3.4
  overflow node bf16 x'            |   6 | 3.87e-07 | 3.10e-06 | 5.60e-07 |   5.5
  overflow node bf16 xa'           |   6 | 1.16e-07 | 1.00e-06 | 1.63e-07 |   6.1
  overflow node bf16 xb'           |   6 | 1.22e-07 | 1.00e-06 | 1.34e-07 |   7.5
  overflow node f16 x'             |   6 | 5.39e-07 | 4.32e-06 | 6.41e-07 |   6.7
  overflow node f16 xa'            |   6 | 1.63e-07 | 1.30e-06 | 1.84e-07 |   7.1
  overflow node f16 xb'            |   6 | 1.51e-07 | 1.21e-06 | 1.44e-07 |   7.8
  overflow rows vs fp64            |   3 | 1.82e-07 | 1.46e-06 | 2.23e-07 |   5.9
  range ends bf16 vs fp64          |  12 | 3.60e-07 | 2.88e-06 | 5.20e-07 |   5.5
  range ends f16                   |   5 | 3.09e-07 | 2.48e-06 | 4.31e-07 |   3.7
  range ends f16 vs fp64           |   4 | 3.60e-07 | 2.88e-06 | 4.01e-07 |   7.0
  rows_chain 0 bf16                |  50 | 1.40e-07 | 1.12e-06 | 1.97e-07 |   5.1
  rows_chain 0 bf16 vs fp64        |  50 | 2.27e-07 | 1.82e-06 | 1.98e-07 |   6.0
  rows_chain 0 f16                 |  50 | 1.01e-07 | 1.00e-06 | 1.54e-07 |   6.5
  rows_chain 0 f16 vs fp64         |  40 | 2.27e-07 | 1.82e-06 | 2.49e-07 |   6.9
  rows_chain 1 bf16                |  50 | 2.52e-07 | 2.02e-06 | 3.04e-07 |   4.0
  rows_chain 1 bf16 vs fp64        |  25 | 2.12e-07 | 1.70e-06 | 3.04e-07 |   3.3
  rows_chain 1 f16                 |  50 | 2.41e-07 | 1.92e-06 | 2.94e-07 |   4.9
  rows_chain 1 f16 vs fp64         |  25 | 2.12e-07 | 1.70e-06 | 4.09e-07 |   2.4
The fp16 launches out of their domain ("launch scale f16": the other rows of a launch with one edge row 2^12 above them) sit 3.7e-5 from the
model, exactly where the model's own float32 form sits, and 2.6 times inside the bar; inside the domain the kernels are 1.8 to 7 times inside
the float64 bar.  Wall time of the file: 31 s for its 62 tests; the slowest, test_edge_mlp3_messages_row_classes_every_size[32769] at 12 s,
spends it on the CPU in the float32 accumulation-chain form of the model (48 rounded partial products per layer for two weight kinds and
two piece modes at 32 769 rows), the next, test_fused_aggregation_piece_by_piece[32769], 3.7 s; every other test stays below 2.5 s.
Mutants (each built once in a scratch copy, none committed; "old" = the tests of these kernels that existed before):
  (a) h1 h2 product dropped in layer 2 of the fp16 edge kernel   new: messages, launch scale, fused aggregation, mlp3_rows, overflow rows (37 tests); old: 27
  (b) LayerNorm given eps instead of s^2 eps                      new: messages, launch scale, mlp3_rows, fused aggregation (33); old: 21
  (c) relu_nan replaced by fmaxf(x, 0)                            new: NaN data, overflow of single rows, overflow in the node kernels, mlp3_rows' NaN row (10); old: 2
  (d) ex taken from 1.0 instead of e0_absmax                      new: launch_wide_scale[understated / overstated], ends of the range (3); old: 5
  (e) SC not applied to the node kernel's bias start              new: node_update_packed (5), overflow in the node kernels (6); old: 15
  (f) k_absmax skips its last float4                              new: test_absmax (6 of 7 sizes), mlp3_rows' own absmax (7); old: NONE
  (g) two neighbouring entries of the pack permutation swapped    new: 51 tests of every kernel; old: 85"""
import contextlib
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import util  # noqa: E402,F401
import edge_mlp_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

K, FLOOR, BAR_MAX = 8.0, 1e-6, 1e-3
F64, F32 = torch.float64, torch.float32
SENT = -7.25
TABLE = {}
KIND = {0: "f16", 1: "bf16"}


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


def go():
    from meshnet import graph_ops
    return graph_ops


@contextlib.contextmanager
def piece_mode(mode):
    was = go().edge_mlp3_mode(mode)
    try:
        yield KIND[mode]
    finally:
        go().edge_mlp3_mode(was)


def _t(x):
    return x.detach().cpu().to(F64)


def check_rows(group, what, got, r64, r32, scale):
    """got (the kernel), r64, r32 (the reference in both precisions) as [rows][columns]; scale: one number per row.  All finite."""
    got, r64, r32 = _t(got), _t(r64), _t(r32)
    assert got.shape == r64.shape == r32.shape, (group, what, got.shape, r64.shape, r32.shape)
    if got.numel() == 0:
        return
    assert bool(torch.isfinite(r64).all()) and bool(torch.isfinite(r32).all()), f"{group} {what}: non-finite reference"
    assert bool(torch.isfinite(got).all()), f"{group} {what}: non-finite values in rows {(~torch.isfinite(got).all(1)).nonzero()[:8, 0].tolist()}"
    scale = torch.broadcast_to(torch.as_tensor(scale, dtype=F64).reshape(-1), (got.shape[0],)).clamp_min(1e-300)
    e32 = float(((r32 - r64).abs().amax(1) / scale).max())
    rows = (got - r64).abs().amax(1) / scale
    worst = int(rows.argmax())
    err = float(rows[worst])
    bar = max(K * e32, FLOOR)
    print(f"{group} | {what}: e32 {e32:.3e} bar {bar:.3e} kernel {err:.3e} (row {worst})")
    n, a, b, c, m = TABLE.get(group, (0, 0.0, 0.0, 0.0, float("inf")))
    TABLE[group] = (n + 1, max(a, e32), max(b, bar), max(c, err), min(m, bar / max(err, 1e-30)))
    assert bar <= BAR_MAX, f"{group} {what}: bar {bar:.3e} > {BAR_MAX}: the inputs are ill-conditioned"
    assert err <= bar, f"{group} {what}: row {worst}: kernel error {err:.3e} > bar {bar:.3e} (float32 reference: {e32:.3e})"


def hold(group, what, got, m64, m32, scale, classes=None, names=("all",), exact=None, skip=None):
    """per class: kernel against the model (rows the model loses entirely must be lost entirely), and against exact = (r64, r32) if given"""
    got_c = got.detach().cpu()
    scale = torch.broadcast_to(torch.as_tensor(scale, dtype=F64).reshape(-1), (got_c.shape[0],))
    classes = torch.zeros(got_c.shape[0], dtype=torch.int64) if classes is None else classes
    lost = ~torch.isfinite(m32).any(1) | ~torch.isfinite(m64).any(1)
    if bool(lost.any()):
        assert not bool(torch.isfinite(got_c[lost]).any()), f"{group} {what}: a row the arithmetic loses came out with finite columns"
    unsure = ~lost & ~(torch.isfinite(m32).all(1) & torch.isfinite(m64).all(1))       # (lost in part: not compared)
    for k, name in enumerate(names):
        on = (classes == k) & ~lost & ~unsure
        if not bool(on.any()):
            continue
        if skip is not None and skip(name):       # (tests/edge_mlp_ref.py edge_comparable: finite, nothing more)
            assert bool(torch.isfinite(got_c[on]).all()), f"{group} {what} [{name}]: non-finite rows"
            continue
        check_rows(group, f"{what} [{name}]", got_c[on], m64[on], m32[on], scale[on])
        if exact is not None:
            check_rows(group + " vs fp64", f"{what} [{name}]", got_c[on], exact[0][on], exact[1][on], scale[on])


def cuda(t):
    return None if t is None else t.detach().contiguous().cuda()


def bits(t):
    t = t.detach().contiguous()
    return t.view(torch.int32) if t.dtype == F32 else t


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def filled(*shape, value=SENT, dtype=F32):
    return torch.full(shape, value, dtype=dtype, device="cuda")


def off_by_one(t):
    """a contiguous view of the same values that starts one element into a larger buffer"""
    buf = torch.zeros(t.numel() + 1, device="cuda", dtype=t.dtype)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v


def ln_module(gamma, beta):
    ln = torch.nn.LayerNorm(128, eps=R.EPS).cuda()
    with torch.no_grad():
        ln.weight.copy_(gamma)
        ln.bias.copy_(beta)
    return ln


def edge_gpu(c, slice_w0=False):
    """the case's tensors on the GPU and its image under the CURRENT piece mode; slice_w0: W0 as a column slice (ld = 384)"""
    g = {k: cuda(c[k]) for k in ("e0", "xa", "xb", "ia", "ib", "b0", "b1", "b2") if c.get(k) is not None}
    w0 = cuda(c["W0"])
    if slice_w0:
        wide = filled(128, 384, value=77.0)
        wide[:, 128:256] = w0
        w0 = wide[:, 128:256]
    g["img"] = go().edge_mlp3_pack(w0, cuda(c["W1"]), cuda(c["W2"]))
    g["ln"] = ln_module(c["gamma"], c["beta"])
    g["absmax"] = torch.tensor([c["absmax"]], dtype=F32, device="cuda")
    return g


def run_edge(g, alpha, E, agg=None, e0=None, absmax=None, **over):
    """messages into a sentinel buffer with one row to spare (or pieces, with agg)"""
    a = dict(g, **over)
    am = a["absmax"] if absmax is None else absmax
    with torch.no_grad():
        if agg is not None:
            return go().edge_mlp3(a["e0"] if e0 is None else e0, alpha, a["xa"], a["ia"], a["xb"], a["ib"], a["img"], a["b0"], a["b1"], a["b2"],
                                  a["ln"], e0_absmax=am, agg=agg)
        buf = filled(E + 1, 128)
        out = go().edge_mlp3(a["e0"] if e0 is None else e0, alpha, a["xa"], a["ia"], a["xb"], a["ib"], a["img"], a["b0"], a["b1"], a["b2"],
                             a["ln"], out=buf[:E], e0_absmax=am)
        assert out.data_ptr() == buf.data_ptr() and bool((buf[E] == SENT).all()), "a row behind the last one was written"
    return buf[:E]


def edge_refs(c, alpha, kind):
    return R.model("edge", c, alpha, kind, F64, c["absmax"]), R.model("edge", c, alpha, kind, F32, c["absmax"])


def hold_edge(group, what, got, c, alpha, kind, launch, wkind, exact):
    m64, m32 = edge_refs(c, alpha, kind)
    dom = R.edge_in_domain(kind, launch, wkind, alpha)
    hold(group, what, got, m64, m32, R.ln_scale(exact[0]), c["classes"], c["names"], exact if dom else None,
         skip=lambda name: not R.edge_comparable(kind, alpha, name))


# ================================================================================================ csplat_gnn_edge_mlp3: messages
@pytest.mark.parametrize("E", R.EDGE_E)
def test_edge_mlp3_messages_row_classes_every_size(E):
    """every size of EDGE_E, the four row classes in one launch, both weight kinds, both piece modes.  Up to 65 rows: every alpha and
    every index pattern; from 16 384 rows: one alpha (cycling through the sizes) and the random pattern.  Twice and into out=: the same
    bits.  W0 as a column slice (ld = 384) at the sizes that are a multiple of 32 + 1"""
    small = E <= 65
    for wi, wkind in enumerate(R.WEIGHT_KINDS):
        patterns = R.INDEX_PATTERNS if small else ("random",)
        alphas = R.ALPHAS if small else (R.ALPHAS[(R.EDGE_E.index(E) + wi) % 4],)
        for pi, pattern in enumerate(patterns):
            c = R.edge_case(E, "mixed", wkind, pattern)
            for alpha in (alphas if pi == len(patterns) - 1 else (alphas[pi % len(alphas)],)):
                exact = (R.exact("edge", c, alpha, F64), R.exact("edge", c, alpha, F32))
                for mode in (0, 1):
                    with piece_mode(mode) as kind:
                        g = edge_gpu(c, slice_w0=(E % 32 == 1))
                        out = run_edge(g, alpha, E)
                        hold_edge(f"messages {kind}", f"E {E} {wkind} {pattern} alpha {alpha:g}", out, c, alpha, kind, "mixed", wkind, exact)
                        assert same_bits(out, run_edge(g, alpha, E))
                        with torch.no_grad():      # (no out=: the wrapper's own buffer; no e0_absmax: the wrapper's own csplat_absmax)
                            own = go().edge_mlp3(g["e0"], alpha, g["xa"], g["ia"], g["xb"], g["ib"], g["img"], g["b0"], g["b1"], g["b2"], g["ln"])
                        assert same_bits(out, own)


@pytest.mark.parametrize("launch", R.LAUNCHES[1:])
def test_edge_mlp3_launch_wide_scale(launch):
    """the launch-wide scale of mode 0 with rows of different size in one launch: an outlier 2^6 / 2^12 above the rest, no node terms, an
    understated / overstated e0_absmax; both weight kinds; alpha 1, and 0.5 with the 0.1 randn weights.  4161 rows (66 workgroups, the last with one
    row), 1040 of every class: out of its domain the arithmetic's error is that of a few fp16 quanta flipping, and the largest of a
    thousand rows is a steadier statistic -- for the model's own float32 form (the bar) and for the kernel -- than that of sixteen"""
    for E, wkinds in ((4161, R.WEIGHT_KINDS),):
        for wkind in wkinds:
            c = R.edge_case(E, launch, wkind)
            for alpha in ((1.0, 0.5) if wkind == R.WEIGHT_KINDS[0] else (1.0,)):
                exact = (R.exact("edge", c, alpha, F64), R.exact("edge", c, alpha, F32))
                for mode in (0, 1):
                    with piece_mode(mode) as kind:
                        out = run_edge(edge_gpu(c), alpha, E)
                        hold_edge(f"launch scale {kind}", f"E {E} {launch} {wkind} alpha {alpha:g}", out, c, alpha, kind, launch, wkind, exact)


@pytest.mark.parametrize("top", (0.0, 2.0 ** -100, 2.0 ** -130, 1e38))
def test_edge_mlp3_ends_of_the_range(top):
    """max |e0| = 0 (cs = 16: an ordinary launch), 2^-100 and a denormal (ex clamped to -96: s = 2^100 takes the ordinary node terms out of
    fp16's range -- mode 0 loses every row, visibly), 1e38 (ex clamped to 100: the rows that hold such values are lost in mode 0, visibly;
    mode 1 gives what fp32 gives).  The kernel's own csplat_absmax supplies the scale"""
    E = 65
    c = R.edge_case(E, "mixed")
    c["e0"] = c["e0"] * (top / float(c["e0"].abs().max()))
    c["absmax"] = float(c["e0"].abs().max())
    exact = (R.exact("edge", c, 1.0, F64), R.exact("edge", c, 1.0, F32))
    for mode in (0, 1):
        with piece_mode(mode) as kind:
            g = edge_gpu(c)
            out = run_edge(g, 1.0, E)
            m64, m32 = edge_refs(c, 1.0, kind)
            if top < 1.0:
                assert bool(torch.isfinite(m32).all()) == (mode == 1 or top == 0.0)
                hold(f"range ends {kind}", f"max |e0| {top:g}", out, m64, m32, R.ln_scale(exact[0]), c["classes"], c["names"],
                     exact if (mode == 1 or top == 0.0) else None)
            elif mode == 1:       # fp32 itself is at the end of its range: the rows the model loses are lost, nothing more is held
                gone = ~torch.isfinite(m32).any(1)
                assert not bool(torch.isfinite(out.cpu()[gone]).any())
            else:       # what the model says: the rows it loses are lost, the others within the bar
                assert bool((~torch.isfinite(m32).any(1)).any())
                hold(f"range ends {kind}", f"max |e0| {top:g}", out, m64, m32, R.ln_scale(torch.nan_to_num(m64)), c["classes"], c["names"])
            with torch.no_grad():
                own = go().edge_mlp3(g["e0"], 1.0, g["xa"], g["ia"], g["xb"], g["ib"], g["img"], g["b0"], g["b1"], g["b2"], g["ln"])
            assert torch.equal(torch.isnan(out), torch.isnan(own)) and same_bits(torch.nan_to_num(out), torch.nan_to_num(own))


# ================================================================================================ csplat_gnn_mlp3_rows
@pytest.mark.parametrize("M", R.NARROW_M)
def test_mlp3_rows_narrow_inputs(M):
    """NARROW_K x M: x is the leading part of a larger allocation whose remainder is NaN; with a NaN in row i + 1, row i keeps its bits (the
    columns >= K of a row are never read as data) and row i + 1 is lost"""
    for Kk in R.NARROW_K:
        c = R.narrow_case(M, Kk)
        exact = (R.exact("edge", c, 1.0, F64), R.exact("edge", c, 1.0, F32))
        m64, m32 = edge_refs(c, 1.0, "f16")
        with piece_mode(0):
            g = edge_gpu(c)
            buf = filled(M * Kk + 1024, value=float("nan"))
            x = buf[:M * Kk].view(M, Kk)
            x.copy_(g["e0"])
            with torch.no_grad():
                out = go().mlp3_rows(x, g["img"], g["b0"], g["b1"], g["b2"], g["ln"], x_absmax=g["absmax"])
                assert tuple(out.shape) == (M, 128)
                hold("mlp3_rows", f"M {M} K {Kk}", out, m64, m32, R.ln_scale(exact[0]), torch.arange(M) % 3, ("1", "2^-10", "2^-3"), exact)
                assert same_bits(out, go().mlp3_rows(x, g["img"], g["b0"], g["b1"], g["b2"], g["ln"]))       # (its own csplat_absmax)
                i = M // 2
                if i + 1 < M:
                    x[i + 1, 0] = float("nan")
                    again = go().mlp3_rows(x, g["img"], g["b0"], g["b1"], g["b2"], g["ln"], x_absmax=g["absmax"])
                    assert not bool(torch.isfinite(again[i + 1]).any())
                    keep = torch.arange(M, device="cuda") != i + 1
                    assert same_bits(again[keep], out[keep])


# ================================================================================================ the fused aggregation
def _agg_case(E, kind):
    dst, src, N = R.agg_graph(E, kind)
    c = R.edge_case(E, "mixed")
    g = torch.Generator().manual_seed(E)
    c["xa"], c["xb"] = torch.randn(N, 128, generator=g), torch.randn(N, 128, generator=g)
    c["ia"], c["ib"] = dst, src
    return c, dst, N


@pytest.mark.parametrize("E", R.EDGE_E)
def test_fused_aggregation_piece_by_piece(E):
    """every graph of AGG_GRAPHS: the plan (gp0, pp) equals the runs derived in numpy from the sorted destinations and the 8-row cuts; each
    piece against the float64 sum of the model's messages over its run; every piece written, nothing behind the last; nodes without
    edges own no piece; twice the same bits"""
    with piece_mode(0):
        for kind in R.AGG_GRAPHS:
            c, dst, N = _agg_case(E, kind)
            start, end, gp0_ref = R.runs(dst.numpy())
            pp_ref = R.piece_ptr(dst.numpy(), N)
            rowptr = torch.from_numpy(np.concatenate([[0], np.cumsum(np.bincount(dst.numpy(), minlength=N))]).astype(np.int32)).cuda()
            gp0, pp, npieces = go().piece_numbering(cuda(dst), rowptr)
            assert npieces == len(start)
            np.testing.assert_array_equal(gp0.cpu().numpy(), gp0_ref)
            np.testing.assert_array_equal(pp.cpu().numpy(), pp_ref)
            deg = np.bincount(dst.numpy(), minlength=N)
            assert np.array_equal(np.diff(pp_ref) == 0, deg == 0)
            g = edge_gpu(c)
            got = []
            for _ in range(2):
                pieces = filled(npieces + 1, 128, value=float("nan"))
                run_edge(g, 2.0, E, agg=(gp0, pieces))
                assert bool(torch.isnan(pieces[npieces]).all()), "a piece behind the last one was written"
                assert not bool(torch.isnan(pieces[:npieces]).any()), "a piece was not written"
                got.append(pieces[:npieces])
            assert same_bits(got[0], got[1])
            m64, m32 = edge_refs(c, 2.0, "f16")
            p64, p32 = R.run_sums(m64, start, end, F64), R.run_sums(m32.to(F32), start, end, F32)
            hold("fused aggregation", f"E {E} {kind}", got[0], p64, p32.to(F64), R.run_sums(m64.abs(), start, end, F64).amax(1))
            msg = run_edge(g, 2.0, E)      # and the pieces ARE the sums of the message rows the other form writes, added in row order
            assert same_bits(got[0], cuda(R.run_sums(msg.cpu(), start, end, F32)))


CHILD = r"""
import os, sys, torch
sys.path.insert(0, os.path.join(os.getcwd(), "cloth-splatting_amd"))
sys.path.insert(0, os.path.join(os.getcwd(), "tests"))
import edge_mlp_ref as R
from meshnet import graph_ops as go
E = 203
dst, src, N = R.agg_graph(E, "random")
c = R.edge_case(E, "mixed")
g = torch.Generator().manual_seed(E)
xa, xb = torch.randn(N, 128, generator=g).cuda(), torch.randn(N, 128, generator=g).cuda()
ln = torch.nn.LayerNorm(128).cuda()
rowptr = torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(torch.bincount(dst, minlength=N), 0)]).to(torch.int32).cuda()
with torch.no_grad():
    gp0, pp, npieces = go.piece_numbering(dst.cuda(), rowptr)
    img = go.edge_mlp3_pack(c["W0"].cuda(), c["W1"].cuda(), c["W2"].cuda())
    a = (xa, dst.cuda(), xb, src.cuda(), img, c["b0"].cuda(), c["b1"].cuda(), c["b2"].cuda(), ln)
    msg = go.edge_mlp3(c["e0"].cuda(), 4.0, *a)
    pieces = torch.full((npieces, 128), float("nan"), device="cuda")
    go.edge_mlp3(c["e0"].cuda(), 4.0, *a, agg=(gp0, pieces))
torch.save({"msg": msg.cpu(), "pieces": pieces.cpu(), "gp0": gp0.cpu()}, sys.argv[1])
"""


def test_row_chunks_of_64_in_a_fresh_process():
    """CSPLAT_EM_CHUNK_ROWS=64 in ONE fresh child process: E = 203 takes four launches, the last one partial (11 rows), the piece numbering
    entered at r0 / 8: messages and pieces bit-equal to the one-launch results of this process"""
    E = 203
    dst, src, N = R.agg_graph(E, "random")
    c = R.edge_case(E, "mixed")
    g = torch.Generator().manual_seed(E)
    c["xa"], c["xb"] = torch.randn(N, 128, generator=g), torch.randn(N, 128, generator=g)
    c["ia"], c["ib"] = dst, src
    start, _end, gp0_ref = R.runs(dst.numpy())
    assert -(-E // 64) == 4 and E % 64 == 11 and len(gp0_ref) == 26
    with piece_mode(0):
        gg = edge_gpu(c)
        gg["ln"] = torch.nn.LayerNorm(128).cuda()
        msg = run_edge(gg, 4.0, E, absmax=go().absmax(gg["e0"]))
        pieces = filled(len(start), 128, value=float("nan"))
        run_edge(gg, 4.0, E, agg=(cuda(torch.from_numpy(gp0_ref)), pieces), absmax=go().absmax(gg["e0"]))
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "chunks.pt")
        env = dict(os.environ, CSPLAT_EM_CHUNK_ROWS="64")
        subprocess.run([sys.executable, "-c", CHILD, path], check=True, env=env, cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
        child = torch.load(path)
    np.testing.assert_array_equal(child["gp0"].numpy(), gp0_ref)
    assert same_bits(child["msg"], msg.cpu()) and same_bits(child["pieces"], pieces.cpu())
    assert not bool(torch.isnan(child["pieces"]).any())


# ================================================================================================ csplat_gnn_node_update_packed
def node_gpu(p, has_next):
    g = {k: cuda(v) for k, v in p.items()}
    g["img"] = go().node_update_pack(g["Wa"], g["Wx"], g["W2"], g["W3"], g["Wi"] if has_next else None, g["Wj"] if has_next else None)
    g["ln"] = ln_module(p["gamma"], p["beta"])
    return g


def run_node(g, agg, x, has_next, piece_ptr=None):
    with torch.no_grad():
        return go().node_update_packed(agg, x, g["img"], g["b0"], g["b2"], g["b3"], g["ln"], has_next, piece_ptr)


def hold_node(group, what, got, agg, x, p, kind, has_next, piece_ptr=None, exact_too=True):
    e64, e32 = R.exact("node", agg, x, p, F64, piece_ptr), R.exact("node", agg, x, p, F32, piece_ptr)
    m64, m32 = R.model("node", agg, x, p, kind, F64, piece_ptr), R.model("node", agg, x, p, kind, F32, piece_ptr)
    N = x.shape[0]
    cls = torch.arange(N) % len(R.NODE_CLASSES)
    ref = torch.nan_to_num(e64[0])
    scales = (torch.maximum(R.ln_scale(ref), x.double().abs().amax(1)), R.product_scale(ref, p["Wi"]), R.product_scale(ref, p["Wj"]))
    for k, name in enumerate(("x'", "xa'", "xb'")[:3 if has_next else 1]):
        hold(f"{group} {name}", what, got[k], m64[k], m32[k], scales[k], cls, R.NODE_CLASSES, (e64[k], e32[k]) if exact_too else None)


@pytest.mark.parametrize("N", R.NODE_N)
def test_node_update_packed_magnitude_classes_and_pieces(N):
    """NODE_N x has_next x both piece modes, aggregates and latents of 1e-3, 1, 30 / 5, 1e+3, 1e+5 and a zero row inside one launch.  The
    aggregate as pieces: 0, 1, 9 and 2 pieces per node cycling, one node with 300 -- the same bits as the launch on the sums added in
    that order"""
    p = R.node_params()
    agg, x = R.node_rows(N)
    cnt = np.array([0, 1, 9, 2])[np.arange(N) % 4]
    cnt[min(3, N - 1)] = 300
    pp = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int32)
    gen = torch.Generator().manual_seed(N)
    scale = torch.tensor(R.NODE_SCALES)[:, 0][torch.repeat_interleave(torch.arange(N), torch.from_numpy(cnt)) % len(R.NODE_SCALES)]
    pieces = torch.randn(int(pp[-1]), 128, generator=gen) * scale[:, None]
    summed = R.sum_pieces(pieces, pp, F32)
    for mode in (0, 1):
        with piece_mode(mode) as kind:
            for has_next in (True, False):
                g = node_gpu(p, has_next)
                xn_buf = run_node(g, cuda(agg), cuda(x), has_next)
                assert (xn_buf[1] is None) == (not has_next) and (xn_buf[2] is None) == (not has_next)
                hold_node(f"node_update {kind}", f"N {N} next {has_next}", xn_buf, agg, x, p, kind, has_next)
                for a, b in zip(xn_buf[:3 if has_next else 1], run_node(g, cuda(agg), cuda(x), has_next)):
                    assert same_bits(a, b)
                via = run_node(g, cuda(pieces), cuda(x), has_next, cuda(torch.from_numpy(pp)))
                for a, b in zip(via[:3 if has_next else 1], run_node(g, cuda(summed), cuda(x), has_next)):
                    assert same_bits(a, b)
                if has_next:
                    hold_node(f"node_update {kind} pieces", f"N {N}", via, pieces, x, p, kind, True, pp, exact_too=False)


# ================================================================================================ csplat_gnn_rows_chain
@pytest.mark.parametrize("N", R.NODE_N)
def test_rows_chain_magnitude_classes(N):
    """NODE_N x mode 0 / 1 x both piece modes; mode 1 with biases, and without: null biases are zero biases, bit for bit"""
    p = R.node_params(1)
    _agg, x = R.node_rows(N, 1)
    cls = torch.arange(N) % len(R.NODE_CLASSES)
    zero = torch.zeros(128)
    for mode in (0, 1):
        with piece_mode(mode) as kind:
            xc = cuda(x)
            with torch.no_grad():
                img0, img1 = go().rows_chain_pack(0, cuda(p["Wa"]), cuda(p["W2"])), go().rows_chain_pack(1, cuda(p["Wa"]), cuda(p["W2"]))
                oa, ob = go().rows_chain(xc, img0, 0)
                e64, e32 = (R.exact("chain", x, 0, p["Wa"], p["W2"], dtype=dt) for dt in (F64, F32))
                m64, m32 = (R.model("chain", x, 0, p["Wa"], p["W2"], kind=kind, acc=a) for a in (F64, F32))
                for k, (o, w) in enumerate(((oa, "Wa"), (ob, "W2"))):
                    sc = R.product_scale(x, p[w])
                    for ci, name in enumerate(R.NODE_CLASSES):
                        on = cls == ci
                        if bool(on.any()):
                            hold(f"rows_chain 0 {kind}", f"N {N} {w}", o[on.cuda()], m64[k][on], m32[k][on], sc[on], None, (name,),
                                 (e64[k][on], e32[k][on]) if R.chain_in_domain(kind, name, 0) else None)
                for b0, b1 in ((p["b0"], p["b2"]), (None, None)):
                    out = go().rows_chain(xc, img1, 1, cuda(b0), cuda(b1))
                    e64, e32 = (R.exact("chain", x, 1, p["Wa"], p["W2"], b0, b1, dtype=dt) for dt in (F64, F32))
                    m64, m32 = (R.model("chain", x, 1, p["Wa"], p["W2"], b0, b1, kind=kind, acc=a) for a in (F64, F32))
                    sc = R.product_scale(e64[1], p["W2"], b1)
                    if b0 is None:
                        assert same_bits(out, go().rows_chain(xc, img1, 1, cuda(zero), cuda(zero)))
                        sc = sc.clamp_min(1e-30)
                    hold(f"rows_chain 1 {kind}", f"N {N} biases {b0 is not None}", out, m64, m32, sc, cls, R.NODE_CLASSES,
                         (e64[0], e32[0]) if b0 is not None else None)
                    assert same_bits(out, go().rows_chain(xc, img1, 1, cuda(b0), cuda(b1)))


# ================================================================================================ csplat_absmax
@pytest.mark.parametrize("n", R.ABSMAX_N)
def test_absmax_is_numpys_maximum_over_what_is_not_nan(n):
    """the maximum in the first float4, in the last one and in the grid-stride tail; -0.0, denormals, Inf; a NaN beside larger and smaller
    values (fmaxf ignores it: graph_ops.absmax's docstring); n = 0 gives 0"""
    def want(a):
        a = np.abs(a[~np.isnan(a)])
        return np.float32(a.max() if a.size else 0.0)

    def got(a):
        t = torch.from_numpy(a).cuda()
        r = go().absmax(t)
        assert tuple(r.shape) == (1,) and r.dtype == F32
        return r.cpu().numpy()[0]

    rng = np.random.default_rng(n)
    base = rng.standard_normal(n).astype(np.float32)
    assert got(base).tobytes() == want(base).tobytes()
    if n == 0:
        assert got(base) == 0.0 and not np.signbit(got(base))
        return
    for pos in sorted({0, 3, n - 4, n - 1, n // 2, max(n - 1028, 0)}):
        for v in (-9.5, np.float32("inf"), -np.float32("inf")):
            a = base.copy()
            a[pos] = v
            assert got(a).tobytes() == want(a).tobytes(), (n, pos, v)
        a = base.copy()
        a[pos] = np.nan       # a NaN beside larger and smaller values
        assert got(a).tobytes() == want(a).tobytes(), (n, pos)
        a[(pos + 1) % n] = 77.0
        assert got(a) == 77.0
    tiny = np.full(n, -0.0, np.float32)
    assert got(tiny).tobytes() == np.float32(0.0).tobytes()
    tiny[n - 1] = -1e-45      # a denormal
    assert got(tiny).tobytes() == np.float32(1e-45).tobytes()
    assert got(np.full(n, np.nan, np.float32)).tobytes() == np.float32(0.0).tobytes()


# ================================================================================================ NaN and Inf data
def _lost(t):
    return ~torch.isfinite(t).any(-1)


@pytest.mark.parametrize("mode", (0, 1))
def test_nan_and_inf_data_reach_exactly_the_rows_that_read_them(mode):
    """one NaN in turn in one e0 element, one xa row, b1[j], gamma[j]: exactly the rows (columns) that read it are non-finite, every other
    one keeps the bits of the clean launch (the clean data's e0_absmax handed in: the same scale); an Inf in e0 likewise.  The fused
    aggregation (mode 0): exactly the pieces whose run holds the poisoned row"""
    E = 203
    c, dst, N = _agg_case(E, "random")
    nan, inf = float("nan"), float("inf")
    with piece_mode(mode) as kind:
        g = edge_gpu(c)
        clean = run_edge(g, 2.0, E)
        assert bool(torch.isfinite(clean).all())
        r, v, j = 77, int(dst[100]), 45
        for bad in (nan, inf, -inf):
            e0 = g["e0"].clone()
            e0[r, 9] = bad
            out = run_edge(g, 2.0, E, e0=e0)
            keep = torch.arange(E, device="cuda") != r
            assert bool(_lost(out)[r]) and same_bits(out[keep], clean[keep]), bad
        xa = g["xa"].clone()
        xa[v, 3] = nan
        out = run_edge(g, 2.0, E, xa=xa)
        reads = cuda(dst == v)
        assert int(reads.sum()) >= 1 and bool(_lost(out)[reads].all()) and same_bits(out[~reads], clean[~reads])
        b1 = g["b1"].clone()
        b1[j] = nan
        assert bool(_lost(run_edge(g, 2.0, E, b1=b1)).all())          # (every row's third layer reads column j of the second)
        ln = ln_module(c["gamma"], c["beta"])
        with torch.no_grad():
            ln.weight[j] = nan
        out = run_edge(g, 2.0, E, ln=ln)
        cols = torch.arange(128, device="cuda") != j
        assert bool(torch.isnan(out[:, j]).all()) and same_bits(out[:, cols], clean[:, cols])
        # an Inf with the scale taken from the data (max |e0| = Inf: ex = 0): the other rows are what the model says for that scale
        e0 = g["e0"].clone()
        e0[r, 9] = inf
        c2 = dict(c, e0=c["e0"].clone(), absmax=inf)
        c2["e0"][r, 9] = inf
        out = run_edge(g, 2.0, E, e0=e0, absmax=go().absmax(e0))
        m64, m32 = edge_refs(c2, 2.0, kind)
        assert bool(_lost(out)[r]) and not bool(torch.isfinite(m32[r]).any())
        hold(f"Inf in e0 {kind}", "the other rows", out, m64, m32, R.ln_scale(torch.nan_to_num(m64)))
        if mode == 0:
            start, end, gp0 = R.runs(dst.numpy())
            gp0c = cuda(torch.from_numpy(gp0))
            pc = filled(len(start), 128, value=nan)
            run_edge(g, 2.0, E, agg=(gp0c, pc))
            e0 = g["e0"].clone()
            e0[r, 9] = nan
            pb = filled(len(start), 128, value=nan)
            run_edge(g, 2.0, E, agg=(gp0c, pb), e0=e0)
            hit = cuda(torch.from_numpy((start <= r) & (r < end)))
            assert int(hit.sum()) == 1 and bool(_lost(pb)[hit].all()) and same_bits(pb[~hit], pc[~hit])
        # the node update and rows_chain: one poisoned aggregate / latent row
        p = R.node_params()
        agg, x = R.node_rows(67)
        gn = node_gpu(p, True)
        want = run_node(gn, cuda(agg), cuda(x), True)
        agg2 = agg.clone()
        agg2[40, 100] = nan
        got = run_node(gn, cuda(agg2), cuda(x), True)
        keep = torch.arange(67, device="cuda") != 40
        for a, b in zip(got, want):
            assert bool(_lost(a)[40]) and same_bits(a[keep], b[keep])
        with torch.no_grad():
            img = go().rows_chain_pack(0, cuda(p["Wa"]), cuda(p["W2"]))
            x2 = x.clone()
            x2[40, 100] = inf
            for a, b in zip(go().rows_chain(cuda(x2), img, 0), go().rows_chain(cuda(x), img, 0)):
                assert bool(_lost(a)[40]) and same_bits(a[keep], b[keep])


# ================================================================================================ overflow is visible, per row
OVER_E = 16417
OVER_ROWS = (5, 16387, 16416)        # the first tile; a tile of a workgroup's second trip; the last, partial tile (its only row)


def _overflow_case(layer):
    """layer 1: the three rows read a node row of xa at 1e7.  Layer 2 / 3: they read a node row that puts 2^15 (in the scaled units) into
    column 7 of the first inner activation, and column 7 of W1 is 40 times what it was, elements of about 4 (layer 2: the second inner
    activation reaches 2^17, beyond fp16) -- or column 7 of W1 is 1 in row 7 alone and column 7 of W2 is 40 times what it was (layer 3:
    the 2^17 arises in the last layer's fp32 accumulators, which are never cut into pieces: the row stays finite and right).  (A larger
    factor would only make the OTHER rows, which meet the same column, ill-conditioned.)"""
    c = R.edge_case(OVER_E, "mixed")
    N = c["xa"].shape[0]
    v = N - 1
    c["ia"][c["ia"] == v] = 0
    c["ib"][c["ib"] == v] = 0
    rows = torch.tensor(OVER_ROWS)
    c["ia"][rows] = v
    c["e0"][rows] = 0.0
    s = 2.0 ** (4 - R.scale_exponent(c["absmax"]))
    if layer == 1:
        c["xa"][v] = 1e7
    else:
        c["xa"][v] = 0.0
        c["xa"][v, 7] = 2.0 ** 15 / s
        c["W1"] = c["W1"].clone()
        if layer == 2:
            c["W1"][:, 7] *= 40.0
        else:
            c["W1"][:, 7] = 0.0
            c["W1"][7, 7] = 1.0
            c["W2"] = c["W2"].clone()
            c["W2"][:, 7] *= 40.0
    return c, rows


@pytest.mark.parametrize("layer", (1, 2, 3))
def test_overflow_of_single_rows_is_visible(layer):
    """mode 0: every affected row is non-finite in EVERY column or within the in-domain bar of exact(float64) -- never finite and wrong;
    every other row is within its bar.  Mode 1 on the same launch: finite and within its bar everywhere"""
    c, rows = _overflow_case(layer)
    exact = (R.exact("edge", c, 1.0, F64), R.exact("edge", c, 1.0, F32))
    affected = torch.zeros(OVER_E, dtype=torch.bool)
    affected[rows] = True
    for mode in (0, 1):
        with piece_mode(mode) as kind:
            out = run_edge(edge_gpu(c), 1.0, OVER_E)
            m64, m32 = edge_refs(c, 1.0, kind)
            oc = out.cpu()
            if mode == 1:
                assert bool(torch.isfinite(oc).all())
            else:
                assert bool(_lost(m64)[rows].all()) == (layer < 3)
                for r in rows.tolist():
                    if bool(torch.isfinite(oc[r]).any()):
                        check_rows("overflow rows vs fp64", f"layer {layer} row {r}", oc[r:r + 1], exact[0][r:r + 1], exact[1][r:r + 1],
                                   R.ln_scale(exact[0][r:r + 1]))
            others = ~affected if mode == 0 else torch.ones(OVER_E, dtype=torch.bool)
            hold(f"overflow {kind}", f"layer {layer} the other rows", out[others.cuda()], m64[others], m32[others],
                 R.ln_scale(exact[0])[others], c["classes"][others], c["names"])


def test_overflow_in_the_node_kernels_is_visible():
    """one aggregate row at 3e6 (x 2^-4: beyond fp16): x', xa', xb' of that node non-finite in every column, every other row within its
    bar; rows_chain with one latent row at 3e6 likewise; mode 1 finite and within its bar everywhere"""
    N = 67
    p = R.node_params()
    agg, x = R.node_rows(N)
    agg[40] = 3e6
    x2 = x.clone()
    x2[40] = 3e6
    for mode in (0, 1):
        with piece_mode(mode) as kind:
            got = run_node(node_gpu(p, True), cuda(agg), cuda(x), True)
            if mode == 0:
                assert all(bool(_lost(t)[40]) for t in got)
            else:
                assert all(bool(torch.isfinite(t).all()) for t in got)
            hold_node(f"overflow node {kind}", "agg row 3e6", got, agg, x, p, kind, True, exact_too=False)
            with torch.no_grad():
                img = go().rows_chain_pack(1, cuda(p["Wa"]), cuda(p["W2"]))
                out = go().rows_chain(cuda(x2), img, 1, cuda(p["b0"]), cuda(p["b2"]))
            assert bool(_lost(out)[40]) == (mode == 0)
            e64 = R.exact("chain", x2, 1, p["Wa"], p["W2"], p["b0"], p["b2"], dtype=F64)
            m64, m32 = (R.model("chain", x2, 1, p["Wa"], p["W2"], p["b0"], p["b2"], kind=kind, acc=a) for a in (F64, F32))
            hold(f"overflow chain {kind}", "x row 3e6", out, m64, m32, R.product_scale(e64[1], p["W2"], p["b2"]))


# ================================================================================================ refusals and alignment
def test_refusals_on_the_host_before_any_launch():
    from csplat.native import CsplatError
    E, N = 40, 9
    c = R.edge_case(E, "mixed")
    with piece_mode(0):
        g = edge_gpu(c)
        a = lambda **o: dict(g, **o)  # noqa: E731

        def edge(alpha=1.0, out=None, agg=None, **o):
            q = a(**o)
            with torch.no_grad():
                return go().edge_mlp3(q["e0"], alpha, q["xa"], q["ia"], q["xb"], q["ib"], q["img"], q["b0"], q["b1"], q["b2"], q["ln"], out=out,
                                      e0_absmax=q["absmax"], agg=agg)
        for alpha in (3.0, 0.0, -2.0, 0.75):
            with pytest.raises(CsplatError, match="power of two"):
                edge(alpha=alpha)
        with pytest.raises(CsplatError, match="alias"):
            edge(out=g["e0"])
        buf = filled(E, 256)
        for bad in (buf[:, :128], filled(E, 128, dtype=torch.float64), filled(E + 1, 128), torch.zeros(E, 128), off_by_one(filled(E, 128))):
            with pytest.raises(ValueError, match="out must be"):
                edge(out=bad)
        assert bool((buf == SENT).all())
        start, _end, gp0 = R.runs(np.sort(c["ia"].numpy()))
        pieces = filled(len(start), 128)
        with pytest.raises(AssertionError):
            edge(agg=(cuda(torch.from_numpy(gp0)).long(), pieces))
        with pytest.raises(AssertionError):
            edge(agg=(cuda(torch.from_numpy(gp0)), filled(len(start), 256)[:, :128]))
        p = R.node_params()
        gn = node_gpu(p, False)
        x = filled(N, 128, value=1.0)
        with pytest.raises(CsplatError, match="alias"):
            from csplat import native as n
            n.check(n.lib.csplat_gnn_node_update_packed(n.stream_handle(torch.device("cuda")), N, x.data_ptr(), x.data_ptr(), gn["img"].data_ptr(),
                                                        gn["b0"].data_ptr(), gn["b2"].data_ptr(), gn["b3"].data_ptr(), gn["ln"].weight.data_ptr(),
                                                        gn["ln"].bias.data_ptr(), R.EPS, 0, x.data_ptr(), None, None, None), "node_update_packed")
        with pytest.raises(AssertionError):
            run_node(gn, x, x, False, torch.zeros(N + 1, dtype=torch.int64, device="cuda"))
        for Kk in (6, 0, 132):
            with pytest.raises(AssertionError):
                go().mlp3_rows(filled(E, Kk, value=1.0), g["img"], g["b0"], g["b1"], g["b2"], g["ln"])
    with piece_mode(1):
        g1 = edge_gpu(c)
        start, _end, gp0 = R.runs(np.sort(c["ia"].numpy()))
        pieces = filled(len(start), 128)
        with pytest.raises(CsplatError, match="mode 0"), torch.no_grad():
            go().edge_mlp3(g1["e0"], 1.0, g1["xa"], g1["ia"], g1["xb"], g1["ib"], g1["img"], g1["b0"], g1["b1"], g1["b2"], g1["ln"],
                           e0_absmax=g1["absmax"], agg=(cuda(torch.from_numpy(gp0)), pieces))
        assert bool((pieces == SENT).all())
        with pytest.raises(AssertionError):
            go().mlp3_rows(filled(E, 8, value=1.0), g1["img"], g1["b0"], g1["b1"], g1["b2"], g1["ln"])
        from csplat import native as n
        rc = n.lib.csplat_gnn_mlp3_rows(n.stream_handle(torch.device("cuda")), E, filled(E, 8).data_ptr(), 8, None, g1["img"].data_ptr(),
                                        g1["b0"].data_ptr(), g1["b1"].data_ptr(), g1["b2"].data_ptr(), g1["ln"].weight.data_ptr(),
                                        g1["ln"].bias.data_ptr(), R.EPS, filled(E, 128).data_ptr())
        assert rc != 0 and b"mode 0" in n.lib.csplat_last_error()


def test_misaligned_operands_are_refused_by_the_entries_and_copied_by_the_wrappers():
    """a view one float into a buffer: the five raw entries refuse it (nothing is launched: the sentinels stay), the five wrappers copy it"""
    from csplat import native as n
    E, N = 70, 33
    c = R.edge_case(E, "mixed")
    p = R.node_params()
    agg, x = R.node_rows(N)
    st = n.stream_handle(torch.device("cuda"))

    def refused(name, *args):
        assert int(getattr(n.lib, name)(st, *args)) != 0, name
        assert b"16-byte" in n.lib.csplat_last_error(), (name, n.lib.csplat_last_error())

    with piece_mode(0):
        g = edge_gpu(c)
        out = filled(E, 128)
        ga, be = g["ln"].weight.detach(), g["ln"].bias.detach()

        def edge_args(**o):
            q = {k: (v.data_ptr() if torch.is_tensor(v) else v) for k, v in dict(dict(g, ga=ga, be=be, out=out), **o).items() if k != "ln"}
            return (E, q["e0"], 1.0, q["absmax"], q["xa"], q["ia"], q["xb"], q["ib"], q["img"], q["b0"], q["b1"], q["b2"], q["ga"], q["be"], R.EPS,
                    q["out"], None, None)
        for k in ("e0", "xa", "xb", "b0", "b1", "b2", "ga", "be", "out"):
            refused("csplat_gnn_edge_mlp3", *edge_args(**{k: off_by_one(dict(g, ga=ga, be=be, out=out)[k])}))
        assert bool((out == SENT).all())
        xn = g["e0"][:, :8].contiguous()
        for k in ("x", "b0", "ga", "out"):
            q = dict(x=xn, b0=g["b0"], ga=ga, out=out)
            q[k] = off_by_one(q[k])
            refused("csplat_gnn_mlp3_rows", E, q["x"].data_ptr(), 8, g["absmax"].data_ptr(), g["img"].data_ptr(), q["b0"].data_ptr(),
                    g["b1"].data_ptr(), g["b2"].data_ptr(), q["ga"].data_ptr(), be.data_ptr(), R.EPS, q["out"].data_ptr())
        assert bool((out == SENT).all())
        gn = node_gpu(p, True)
        aggc, xc, o1, o2, o3 = cuda(agg), cuda(x), filled(N, 128), filled(N, 128), filled(N, 128)
        gna, gnb = gn["ln"].weight.detach(), gn["ln"].bias.detach()
        for k in ("agg", "x", "b0", "ga", "o1", "o3"):
            q = dict(agg=aggc, x=xc, b0=gn["b0"], ga=gna, o1=o1, o3=o3)
            q[k] = off_by_one(q[k])
            refused("csplat_gnn_node_update_packed", N, q["agg"].data_ptr(), q["x"].data_ptr(), gn["img"].data_ptr(), q["b0"].data_ptr(),
                    gn["b2"].data_ptr(), gn["b3"].data_ptr(), q["ga"].data_ptr(), gnb.data_ptr(), R.EPS, 1, q["o1"].data_ptr(), o2.data_ptr(),
                    q["o3"].data_ptr(), None)
        with torch.no_grad():
            img1 = go().rows_chain_pack(1, gn["Wa"], gn["W2"])
        for k in ("x", "b0", "b1", "o1"):
            q = dict(x=xc, b0=gn["b0"], b1=gn["b2"], o1=o1)
            q[k] = off_by_one(q[k])
            refused("csplat_gnn_rows_chain", N, 1, q["x"].data_ptr(), img1.data_ptr(), q["b0"].data_ptr(), q["b1"].data_ptr(), q["o1"].data_ptr(), None)
        assert all(bool((t == SENT).all()) for t in (o1, o2, o3))
        one = filled(1)
        assert int(n.lib.csplat_absmax(st, 64, off_by_one(xc[0, :64]).data_ptr(), one.data_ptr())) != 0 and float(one) == SENT
        # ---- the wrappers copy
        m = off_by_one
        with torch.no_grad():
            want = run_edge(g, 1.0, E)
            ln_m = torch.nn.LayerNorm(128, eps=R.EPS).cuda()
            ln_m.weight.data, ln_m.bias.data = m(ga), m(be)
            got = go().edge_mlp3(m(g["e0"]), 1.0, m(g["xa"]), g["ia"], m(g["xb"]), g["ib"], g["img"], m(g["b0"]), m(g["b1"]), m(g["b2"]), ln_m,
                                 e0_absmax=g["absmax"])
            assert same_bits(got, want)
            assert same_bits(go().mlp3_rows(m(xn), g["img"], m(g["b0"]), m(g["b1"]), m(g["b2"]), ln_m),
                             go().mlp3_rows(xn, g["img"], g["b0"], g["b1"], g["b2"], g["ln"]))
            ln_n = torch.nn.LayerNorm(128, eps=R.EPS).cuda()
            ln_n.weight.data, ln_n.bias.data = m(gna), m(gnb)
            for a, b in zip(go().node_update_packed(m(aggc), m(xc), gn["img"], m(gn["b0"]), m(gn["b2"]), m(gn["b3"]), ln_n, True),
                            run_node(gn, aggc, xc, True)):
                assert same_bits(a, b)
            assert same_bits(go().rows_chain(m(xc), img1, 1, m(gn["b0"]), m(gn["b2"])), go().rows_chain(xc, img1, 1, gn["b0"], gn["b2"]))
            assert same_bits(go().absmax(m(xc)), go().absmax(xc))
