"""What tests/test_edge_mlp_gpu.py rests on, without a GPU and without the built library: the launch constants tests/edge_mlp_ref.py assumes
are the ones csrc/csplat_edge_mlp.hip holds, every size of its lists crosses one of them, the pack permutation is a permutation, the piece
model of edge_mlp_ref.py IS the operation once no product is dropped and no piece is lost, its float32-accumulating form stays beside its
float64-accumulating one, and -- the condition that makes the GPU file's second bar fair -- the arithmetic's own loss (model(acc = float64)
against exact(float64), per row, scale max(max_j |ref|, 1)) is within 8 x fp32's own error e32 (exact(float32) against exact(float64),
floor 1e-6) on every IN-DOMAIN class.

In-domain, fp16 pieces (mode 0): the launches 'mixed', 'outlier 2^6' (its other rows) and 'overstated absmax 2^6' with 0.1 randn weights,
as long as alpha x (the launch's 2^6) <= 2^6 -- alpha multiplies the edge term only, so the rows whose edge features are small or zero sit
alpha times further below the launch's scale (s = cs / alpha multiplies their node terms).  bf16 pieces (mode 1): every class.  Everything
else is OUT of the domain the kernel's header states, and what the model loses there is recorded, not held to e32.  Printed by
test_arithmetic_loss_table (pytest -s), E = 257, worst class of each launch; "loss" = model(float64) against exact(float64), e32 beside it:

  fp16 pieces, 0.1 randn weights               alpha 0.5          alpha 1            alpha 64           alpha 16384
  launch                                       loss     e32       loss     e32       loss     e32       loss     e32
  mixed                                        3.8e-07  4.6e-07   4.7e-07  4.8e-07   6.6e-07  4.8e-07   1.3e-04  5.0e-07
  outlier 2^6 (the other rows)                 5.6e-07  4.6e-07   8.4e-07  4.8e-07   3.3e-05  4.8e-07   8.6e-03  5.0e-07
  outlier 2^12 (the other rows)                1.9e-05  4.6e-07   4.2e-05  4.8e-07   2.2e-03  4.8e-07   5.7e-01  5.0e-07
  no node terms 2^-6                           1.8e-07  2.8e-07   1.5e-07  2.3e-07   1.7e-06  4.6e-07   3.5e-04  5.4e-07
  no node terms 2^-12                          1.8e-07  2.8e-07   1.5e-07  2.5e-07   1.6e-06  2.5e-07   4.8e-04  7.6e-07
  understated absmax 2^-6                      3.8e-07  4.6e-07   4.6e-07  4.8e-07   5.1e-07  4.8e-07   2.0e-06  5.0e-07
  overstated absmax 2^6                        5.6e-07  4.6e-07   8.4e-07  4.8e-07   3.3e-05  4.8e-07   8.6e-03  5.0e-07
  fp16 pieces, weights down to 1e-3 of the largest
  mixed                                        4.1e-07  2.3e-07   4.1e-07  2.0e-07   1.7e-06  4.9e-07   1.1e-04  5.2e-07
  outlier 2^12 (the other rows)                1.2e-05  2.3e-07   2.5e-05  2.0e-07   1.6e-03  4.9e-07   3.8e-01  5.2e-07
  bf16 pieces: every launch, weight kind and alpha   loss <= 3.0e-08, e32 up to 7.6e-07
(the outlier row itself: 2e-7 with 0.1 randn weights, 1.1e-6 with the small ones, at every alpha).  The loss is that of the rows furthest
below the launch's scale -- the zero rows and the rows 2^-20 of the largest, which hold the node terms only: an element below 2^-3 of fp16's
normal range keeps an absolute error of 2^-25 in the scaled units, and the LayerNorm divides it by the row's own size.  5e-5 on the other
rows of a launch that holds one edge row 2^12 above them at alpha 1; the same 2^12 reached as alpha 64 x 2^6 gives 3e-5; 2^14 and beyond
(alpha 16384 on a zero edge row) 1e-4 to O(1).  With b1, b2 in place the 'no node terms' launches keep fp32's accuracy up to alpha 64.
An understated absmax costs no accuracy (the rows sit higher in fp16's range) until an activation leaves that range: an overflow, visible
as NaN rows (test_overflow_is_visible_through_the_model)."""
import os
import re

import pytest

torch = pytest.importorskip("torch")

import edge_mlp_ref as R  # noqa: E402

F64, F32 = torch.float64, torch.float32
K, FLOOR = 8.0, 1e-6
HIP = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "cloth-splatting_amd", "csrc", "csplat_edge_mlp.hip")


@pytest.fixture(scope="module")
def src():
    with open(HIP) as f:
        return f.read()


def _one(src, pattern):
    m = re.findall(pattern, src)
    assert m, pattern
    assert len(set(m)) == 1, (pattern, m)
    return m[0]


def test_constants_of_the_hip_file_are_the_ones_the_reference_assumes(src):
    assert int(_one(src, r"constexpr int EM_STRIDE = (\d+);")) == R.EM_STRIDE
    assert int(_one(src, r"ntiles = \(int\)\(\(M \+ 31\) / (\d+)\)")) == R.TILE
    assert int(_one(src, r"constexpr int ER_TILE_P = (\d+) \* EM_STRIDE;")) == R.TILE
    assert int(_one(src, r"nst = \(rows \+ 63\) / (\d+);")) == R.STEP_ROWS == 2 * R.TILE
    assert {int(v) for v in re.findall(r"nst < (\d+) \? nst : (\d+)", src)[0]} == {R.GRID_CAP}
    # one chunked launcher, em_launch_chunks, for the edge entry and the narrow-row entry: one grid rule, one chunk size, and both reach it
    assert len(re.findall(r"nst < 256 \? nst : 256", src)) == 1 and len(re.findall(r"\bCHUNK = ", src)) == 1
    assert len(re.findall(r"return em_launch_chunks<", src)) == 2 and "return em_launch_chunks<true, 2>(" in src
    assert R.NO_LOOP_ROWS == 16384
    assert int(_one(src, r"\? v : \(int64_t\)1 << (\d+);")) == 22 and int(_one(src, r"v <= \(\(int64_t\)1 << (\d+)\)")) == 22
    assert 1 << 22 == R.CHUNK_ROWS
    assert _one(src, r"static constexpr int NP = F16 \? (\d) : (\d);") == (str(R.NP["f16"]), str(R.NP["bf16"]))
    assert _one(src, r"static constexpr int NPROD = F16 \? (\d) : (\d);") == (str(R.NPROD["f16"]), str(R.NPROD["bf16"]))
    # those two lines are Piece<F16>'s, the only place that says them: the edge kernel's ErCfg and the node kernels' PieceChain take them from it
    assert len(re.findall(r"NP = F16 \?", src)) == 1 and len(re.findall(r"NPROD = F16 \?", src)) == 1
    assert "static constexpr int NP = Piece<F16>::NP, NPROD = Piece<F16>::NPROD;" in src      # (ErCfg)
    assert "typedef Piece<F16> P;\n    static constexpr int NP = P::NP, NPROD = P::NPROD;" in src      # (PieceChain)
    for kind in ("f16", "bf16"):       # NPROD = the number of (i, j) with i + j <= NP - 1
        n = R.NP[kind]
        assert sum(1 for i in range(n) for j in range(n) if i + j <= n - 1) == R.NPROD[kind]
    wp, xp = _one(src, r"WP\[6\] = \{([^}]*)\}, XP\[6\] = \{([^}]*)\}")
    for f16 in (True, False):          # the (weight piece, activation piece) lists ARE those pairs
        ev = lambda s: [int(eval(t.replace("F16 ?", "(").replace(":", ") if F16 else (") + ")" if "F16" in t else t, {"F16": f16}))  # noqa: E731
                        for t in s.split(",")]
        n, k = (2, 3) if f16 else (3, 6)
        order = tuple(zip(ev(wp)[:k], ev(xp)[:k]))
        assert order == R.CHAIN["f16" if f16 else "bf16"], order
        assert sorted(order) == sorted((i, j) for i in range(n) for j in range(n) if i + j <= n - 1), order
    assert _one(src, r"constexpr float SC = F16 \? ([0-9.]+)f : 1\.f, ISC = F16 \? ([0-9.]+)f : 1\.f;") == ("0.0625", "16.")
    assert R.NODE_SC == {"f16": 0.0625, "bf16": 1.0}
    assert tuple(int(v) for v in _one(src, r"ex = ex < (-?\d+) \? -?\d+ : \(ex > (\d+) \? \d+ : ex\);")) == R.EX_CLAMP
    assert _one(src, r"cs = ldexpf\(1\.f, (\d+) - ex\);") == "4"
    assert _one(src, r"if \(m > 0\.f && m < ([0-9.e]+)f\)") == "3.0e38"
    assert int(_one(src, r"nb < (\d+) \? nb : \d+\), (\d+), 0, s>>>")[0]) == R.ABSMAX_GRID_CAP
    assert int(_one(src, r"nb < (\d+) \? nb : \d+\), (\d+), 0, s>>>")[1]) == R.ABSMAX_LANES
    common = open(os.path.join(os.path.dirname(HIP), "csplat_common.h")).read()
    assert "float relu_keep_nan(float x) { return x < 0.f ? 0.f : x; }" in common      # a NaN passes; the one ReLU of this file:
    assert src.count("relu_keep_nan(acc[") == 6 and "float relu" not in src and "fmaxf(acc[" not in src
    assert R.GROUP == 8 and "((M + 7) / 8)" in src and "r0 / 8" in src


def test_every_size_crosses_a_constant():
    T, S, G = R.TILE, R.STEP_ROWS, R.NO_LOOP_ROWS
    assert R.EDGE_E == (1, T - 1, T, T + 1, S - 1, S, S + 1, G, G + 1, G + T + 1, 2 * G + 1)
    # 16 385: the first size at which a workgroup loops (257 steps on 256 workgroups); 16 417: that second trip's step has a whole tile and one
    # row of the next; 32 769: every workgroup loops twice and one takes a third trip.  E % 8 != 0 at every odd size
    assert -(-G // S) == R.GRID_CAP and -(-(G + 1) // S) == R.GRID_CAP + 1
    assert (G + T + 1) - G == T + 1 and -(-(2 * G + 1) // S) == 2 * R.GRID_CAP + 1
    assert R.NODE_N == (1, T - 1, T, T + 1, 1031) and -(-1031 // T) == 33 and 1031 % T == 7         # one tile per workgroup: 33 workgroups, 7 rows in the last
    assert all(k % 4 == 0 and 4 <= k <= 128 for k in R.NARROW_K) and R.NARROW_K[0] == 4 and R.NARROW_K[-1] == 128
    assert 12 % 16 != 0 and 20 > 16 and 124 == 128 - 4       # one float4 and a bit, more than one, one short of full
    cap = R.ABSMAX_GRID_CAP * R.ABSMAX_LANES * 4
    assert R.ABSMAX_N == (0, 4, 4 * R.ABSMAX_LANES - 4, 4 * R.ABSMAX_LANES, 4 * R.ABSMAX_LANES + 4, cap, cap + 4)
    assert all(a > 0 and abs(torch.frexp(torch.tensor(a))[0].item()) == 0.5 for a in R.ALPHAS)


def test_er_src_col_is_a_permutation():
    assert [R.er_src_col(0, p) for p in range(128)] == list(range(128))
    for layer in (1, 2):
        cols = [R.er_src_col(layer, p) for p in range(128)]
        assert sorted(cols) == list(range(128)) and cols != list(range(128))
        # what the producing wave leaves: lane-half h' of wave j' holds register r <-> feature 32j' + 8(r >> 2) + 4h' + (r & 3)
        for p in range(128):
            j, h, r = p // 32, (p // 16) % 2, p % 16
            assert cols[p] == 32 * j + 8 * (r // 4) + 4 * h + r % 4


def test_er_src_col_in_the_hip_file_is_the_same_expression(src):
    assert "return 32 * j + 8 * (r >> 2) + 4 * h + (r & 3);" in src and "const int j = pos >> 5, h = (pos >> 4) & 1, r = pos & 15;" in src


def _worst(a, b, scale, on=None):
    e = R.row_err(a, b, scale)
    return float((e if on is None else e[on]).max())


def test_model_with_no_product_dropped_and_no_piece_lost_is_the_operation():
    """seven bf16 pieces hold 56 bits of any float64 activation; keep = 12 keeps every product"""
    kw = dict(kind="bf16", acc=F64, npieces=7, keep=12)
    for launch in ("mixed", "outlier 2^12", "no node terms 2^-12"):
        for alpha in (0.5, 64.0):
            c = R.edge_case(67, launch)
            r = R.exact("edge", c, alpha, F64)
            assert _worst(R.model("edge", c, alpha, e0_absmax=c["absmax"], **kw), r, R.ln_scale(r)) < 1e-12
    c = R.narrow_case(33, 20)
    r = R.exact("edge", c, 1.0, F64)
    assert _worst(R.model("edge", c, 1.0, e0_absmax=c["absmax"], **kw), r, R.ln_scale(r)) < 1e-12
    p = R.node_params()
    agg, x = R.node_rows(37)
    for got, ref in zip(R.model("node", agg, x, p, **kw), R.exact("node", agg, x, p, F64)):
        assert _worst(got, ref, ref.abs().amax(1).clamp_min(1.0)) < 1e-12
    for mode in (0, 1):
        got = R.model("chain", x, mode, p["Wa"], p["W2"], p["b0"], p["b2"], **kw)
        ref = R.exact("chain", x, mode, p["Wa"], p["W2"], p["b0"], p["b2"], dtype=F64)
        for a, b in zip(got if mode == 0 else (got,), ref[:2] if mode == 0 else (ref[0],)):
            assert _worst(a, b, b.abs().amax(1).clamp_min(1.0)) < 1e-12
    # the pieces the kernel does keep are NOT the operation: the same comparison with its own NP is seven orders of magnitude away
    c = R.edge_case(67, "mixed")
    r = R.exact("edge", c, 1.0, F64)
    assert _worst(R.model("edge", c, 1.0, "f16", F64, c["absmax"]), r, R.ln_scale(r)) > 1e-8


def _cases():
    for wkind in R.WEIGHT_KINDS:
        for launch in R.LAUNCHES:
            for alpha in R.ALPHAS:
                c = R.edge_case(257, launch, wkind)
                r64, r32 = R.exact("edge", c, alpha, F64), R.exact("edge", c, alpha, F32)
                yield wkind, launch, alpha, c, r64, r32


def test_arithmetic_loss_table():
    """per launch, weight kind, alpha, mode and row class: model(acc = float64) against exact(float64) beside e32; held within 8 x e32 (floor
    1e-6) on the in-domain classes (module docstring).  Also: the float32-accumulating model against the float64-accumulating one, held
    within 8 x e32 where the class is in-domain and within 8 x max(e32, the arithmetic's own loss) elsewhere -- one fp32 rounding of an
    accumulator moves the pieces cut from it by no more than cutting them does, and both are amplified by the same LayerNorm"""
    bad = []
    for wkind, launch, alpha, c, r64, r32 in _cases():
        sc = R.ln_scale(r64)
        for kind in ("f16", "bf16"):
            m64 = R.model("edge", c, alpha, kind, F64, c["absmax"])
            m32 = R.model("edge", c, alpha, kind, F32, c["absmax"])
            for k, name in enumerate(c["names"]):
                on = c["classes"] == k
                e32, loss, m3264 = _worst(r32, r64, sc, on), _worst(m64, r64, sc, on), _worst(m32, m64, sc, on)
                dom = R.edge_in_domain(kind, launch, wkind, alpha) or name in ("the outlier", "the largest row") and wkind == "0.1 randn"
                print(f"{kind:4s} | {wkind:12s} | {launch:24s} | alpha {alpha:7g} | {name:28s} | loss {loss:.1e} | e32 {e32:.1e} | "
                      f"model32 - model64 {m3264:.1e} | {'in' if dom else 'out of'} domain")
                bar = max(K * e32, FLOOR)
                if dom and loss > bar:
                    bad.append(("loss", kind, wkind, launch, alpha, name, loss, bar))
                bar2 = bar if dom else max(bar, K * loss)
                if m3264 > bar2:
                    bad.append(("model32", kind, wkind, launch, alpha, name, m3264, bar2))
    assert not bad, bad


def test_node_and_chain_models_stay_beside_the_operation():
    """the node kernels' fixed 2^-4: aggregates and latents from 1e-3 to 1e+5 and a zero row inside one launch, per class"""
    p = R.node_params()
    agg, x = R.node_rows(61)
    e64, e32 = R.exact("node", agg, x, p, F64), R.exact("node", agg, x, p, F32)
    scales = (torch.maximum(R.ln_scale(e64[0]), x.double().abs().amax(1)), R.product_scale(e64[0], p["Wi"]), R.product_scale(e64[0], p["Wj"]))
    for kind in ("f16", "bf16"):
        m64, m32 = R.model("node", agg, x, p, kind, F64), R.model("node", agg, x, p, kind, F32)
        for what, a64, a32, r64, r32, sc in zip(("x'", "xa'", "xb'"), m64, m32, e64, e32, scales):
            for k, name in enumerate(R.NODE_CLASSES):
                on = torch.arange(61) % len(R.NODE_CLASSES) == k
                e, loss, mm = _worst(r32, r64, sc, on), _worst(a64, r64, sc, on), _worst(a32, a64, sc, on)
                print(f"node {kind} {what} [{name}]: loss {loss:.1e} e32 {e:.1e} model32 - model64 {mm:.1e}")
                assert loss <= max(K * e, FLOOR) and mm <= max(K * e, FLOOR), (kind, what, name, loss, mm, e)
    for mode in (0, 1):
        r64 = R.exact("chain", x, mode, p["Wa"], p["W2"], p["b0"], p["b2"], dtype=F64)
        r32 = R.exact("chain", x, mode, p["Wa"], p["W2"], p["b0"], p["b2"], dtype=F32)
        if mode == 0:
            outs = [(r64[0], r32[0], R.product_scale(x, p["Wa"])), (r64[1], r32[1], R.product_scale(x, p["W2"]))]
        else:
            outs = [(r64[0], r32[0], R.product_scale(r64[1], p["W2"], p["b2"]))]
        for kind in ("f16", "bf16"):
            got = R.model("chain", x, mode, p["Wa"], p["W2"], p["b0"], p["b2"], kind=kind, acc=F64)
            for g, (a, b, sc) in zip(got if mode == 0 else (got,), outs):
                for k, name in enumerate(R.NODE_CLASSES):
                    on = torch.arange(61) % len(R.NODE_CLASSES) == k
                    loss, e = _worst(g, a, sc, on), _worst(b, a, sc, on)
                    print(f"chain mode {mode} {kind} [{name}]: loss {loss:.1e} e32 {e:.1e}")
                    # rows of 1e-3 times 2^-4 are fp16 denormals: an absolute 2^-25 x 16 = 5e-7 of the original units beside a row scale
                    # of 1e-2 (the header: "an element below 2 of the original units keeps an absolute error of 5e-7"): out of domain
                    if R.chain_in_domain(kind, name, mode):
                        assert loss <= max(K * e, FLOOR), (mode, kind, name, loss, e)
                    else:       # every element of x within 2^-25 x 16 of its two pieces: the row's error within that times max_j sum_k |w_jk|
                        wsum = float(torch.maximum(p["Wa"].double().abs().sum(1).max(), p["W2"].double().abs().sum(1).max()))
                        assert loss <= 2.0 ** -21 * wsum / float(sc[on].min()), (mode, kind, name, loss)


def _overflow_case(v):
    """s = 1 (alpha 1, e0_absmax 8 handed in with e0 = 0): row 1's first inner activation is v in column 0, the other rows' are O(1)"""
    c = R.edge_case(5, "mixed")
    c["e0"] = torch.zeros(5, 128)
    c["b0"] = torch.zeros(128)
    c["xa"], c["xb"] = torch.rand(5, 128, generator=torch.Generator().manual_seed(1)), torch.zeros(5, 128)
    c["xa"][1, 0] = v
    c["ia"], c["ib"] = torch.arange(5), torch.arange(5)
    return c


def test_overflow_is_visible_through_the_model():
    """a row whose scaled inner activation is beyond fp16's largest finite value comes out non-finite in EVERY column (pieces Inf and -Inf:
    every product of the next layer is NaN, and relu_nan keeps it); 65504 (1 - 2^-11) = 65472 and 65519 (which still rounds to 65504) come
    out finite, and in every case so do the other rows.  The bf16 pieces hold all of them"""
    assert R.F16_MAX == float(torch.finfo(torch.float16).max)
    for v, finite in ((65536.0, False), (65520.0, False), (1e7, False), (65519.0, True), (65504.0 * (1.0 - 2.0 ** -11), True)):
        c = _overflow_case(v)
        for acc in (F64, F32):
            y = R.model("edge", c, 1.0, "f16", acc, 8.0)
            assert bool(torch.isfinite(y[[0, 2, 3, 4]]).all()), v
            assert bool(torch.isfinite(y[1]).all()) if finite else not bool(torch.isfinite(y[1]).any()), (v, acc)
            assert bool(torch.isfinite(R.model("edge", c, 1.0, "bf16", acc)).all())
    # layer 2: an activation of 4096 meeting a weight column of 32 (the product 131 072 is the next layer's input); and the node kernels
    c = _overflow_case(4096.0)
    c["W0"], c["W1"] = c["W0"].clone(), c["W1"].clone()
    c["W1"][:, 0] = 32.0
    y = R.model("edge", c, 1.0, "f16", F64, 8.0)
    assert not bool(torch.isfinite(y[1]).any()) and bool(torch.isfinite(y[[0, 2, 3, 4]]).all())
    p = R.node_params()
    agg, x = R.node_rows(7)
    agg[3] = 3e6        # (x 2^-4 = 187 500: beyond fp16)
    xn, xa, xb = R.model("node", agg, x, p, "f16", F64)
    keep = [0, 1, 2, 4, 5, 6]
    for t in (xn, xa, xb):
        assert not bool(torch.isfinite(t[3]).any()) and bool(torch.isfinite(t[keep]).all())
    assert all(bool(torch.isfinite(t).all()) for t in R.model("node", agg, x, p, "bf16", F64))


def test_scale_exponent_and_the_launches_at_the_ends_of_the_range():
    """cs = 2^(4 - ex) brings max |e0| to [8, 16); the clamp, 0, a denormal, 1e38, Inf and NaN"""
    for m in (1.0, 3.7, 2.0 ** -20, 1e30):
        assert 8.0 <= m * 2.0 ** (4 - R.scale_exponent(m)) < 16.0
    assert R.scale_exponent(0.0) == 0 and R.scale_exponent(float("inf")) == 0 and R.scale_exponent(float("nan")) == 0
    assert R.scale_exponent(3.1e38) == 0 and R.scale_exponent(1e38) == 100 and R.scale_exponent(2.0 ** 99) == 100
    assert R.scale_exponent(2.0 ** -100) == -96 and R.scale_exponent(2.0 ** -130) == -96 and R.scale_exponent(2.0 ** 120) == 100
    # all-zero e0: cs = 16, an ordinary launch.  Ordinary node terms beside edge rows of 2^-100 or of a denormal: s = 2^100 takes the node
    # terms out of fp16's range -- every row non-finite, visibly (the header's domain: inner activations within 2^12 of the edge rows'
    # scale).  1e38: ex is clamped to 100, the rows that hold such values leave fp16's range and are non-finite in every column.  The bf16
    # pieces serve what fp32 serves
    c = R.edge_case(9, "mixed")
    base = R.edge_rows(9)
    for top in (0.0, 2.0 ** -100, 2.0 ** -130, 1e38):
        c["e0"] = base * (top / float(base.abs().max()))
        y = R.model("edge", c, 1.0, "f16", F32, float(c["e0"].abs().max()))
        r = R.exact("edge", c, 1.0, F64)
        if top == 0.0:
            assert _worst(y, r, R.ln_scale(r)) < 8e-6
        elif top < 1.0:
            assert not bool(torch.isfinite(y).any()), top
        else:
            assert not bool(torch.isfinite(y[0::4]).any()), top
        yb = R.model("edge", c, 1.0, "bf16", F32)
        if top < 1.0:
            assert _worst(yb, r, R.ln_scale(r)) < 8e-6, top
        else:       # (1e38 times a weight row overflows fp32 itself: the rows the float32 restatement loses, and no others)
            assert torch.equal(torch.isfinite(yb).all(1), torch.isfinite(R.exact("edge", c, 1.0, F32)).all(1))


def test_run_numbering_and_piece_sums():
    """runs(): cut where the destination changes and every 8 rows; piece_ptr(): a node's pieces are consecutive; the pieces add up to the
    per-node sums"""
    import numpy as np
    for E in (1, 33, 65, 203):
        for kind in R.AGG_GRAPHS:
            dst, _src, N = R.agg_graph(E, kind)
            assert bool((dst[1:] >= dst[:-1]).all()) and int(dst.max()) < N
            start, end, gp0 = R.runs(dst.numpy())
            assert start[0] == 0 and end[-1] == E and (start[1:] == end[:-1]).all() and (end - start).max() <= 8
            for s, e in zip(start, end):
                assert len(set(dst[s:e].tolist())) == 1 and s // 8 == (e - 1) // 8
            assert len(gp0) == (E + 7) // 8 and all(start[gp0[g]] == 8 * g for g in range(len(gp0)))
            pp = R.piece_ptr(dst.numpy(), N)
            assert pp[-1] == len(start) and np.all(np.diff(pp) >= 0)
            msg = torch.randn(E, 128, generator=torch.Generator().manual_seed(E))
            node_sums = R.sum_pieces(R.run_sums(msg, start, end), pp)
            ref = torch.zeros(N, 128, dtype=F64).index_add_(0, dst, msg.double())
            assert float((node_sums - ref).abs().max()) < 1e-12
            if kind == "many empty nodes":
                assert int((np.diff(pp) == 0).sum()) > N // 2
    dst, _src, N = R.agg_graph(16385, "hub")
    start, end, _ = R.runs(dst.numpy())
    hub = int(torch.bincount(dst).argmax())
    rows = (dst == hub).nonzero()[:, 0]
    assert int(rows[0]) // 64 < 64 * 0 + int(rows[-1]) // 64 and int(rows.numel()) > 8192        # many steps: two workgroups' ranges and more
