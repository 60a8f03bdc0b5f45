"""The calling contract of the MeshNet autograd nodes -- the ten of meshnet/graph_ops.py (EdgeCombine, SegmentSum, RowsDot, SimHidden,
SimResidual, LayerNorm128, SplitKLinear, EdgeTailAggregate, EdgeFirstLayer, EdgeLatentLinear), UpdatePrediction of meshnet/train_sim.py
and _Length of csplat/knn_regs.py -- through tests/autograd_contract.py, with the helpers, the strict dispatch and the fallback counter
of tests/test_autograd_contract_gpu.py: one case per form of a node, each through C1 strided inputs, C2 second backward, C3 accumulation,
C4 needs_input_grad subsets, C5 upstream gradient forms, C6 in-place edit before backward, C7 create_graph.  tests/test_gnn_autograd_
nodes_gpu.py varies the VALUES these nodes see, at the kernels' size edges; this file varies how autograd reaches them, at the smallest
shapes at which the Python of a node takes each of its branches.  C1 hands every input in three forms: a column slice, a transpose, and
("offset") a contiguous view that starts one float past a 16-byte boundary.

Every clause is equality of bits with the case's PLAIN form; test_plain_form_meets_the_fp64_bar anchors that form to the node's float64
restatement under the rule of the file that owns the node (imported, not restated): check_rows / check_columns of test_gnn_autograd_
nodes_gpu.py with its scales, check() of test_sim_rollout_kernels_gpu.py, the rule of test_train_sim_gpu.py (check() of test_train_
kernels_gpu.py relative to the incoming gradients), 4 e32 + 4 u of test_knn_regs_gpu.py.  ReLU'd inputs are drawn without ties
(gnn_autograd_ref.draw_without_ties; tests/test_autograd_contract_meshnet_cpu.py runs every draw and every bar on the CPU).

What the table showed on an MI355X when this file was written ("equal bits" = eq; wall time of the 161 tests: 6 s; the slowest 1.3 s,
the first case with the library's first-call set-up, then 0.4 s, C1 of update_prediction through the composed branch):

  case                               | C1                     | C2 | C3 | C4 | C5 | C6          | C7
  EdgeCombine (its three forms)      | eq                     | eq | eq | eq | eq | eq          | raises
  SegmentSum                         | eq                     | eq | eq | eq | eq | eq          | raises
  LayerNorm128                       | eq                     | eq | eq | eq | eq | eq / raises | raises
  SplitKLinear M=512                 | eq / within bar (0.15) | eq | eq | eq | eq | eq / raises | raises
  SplitKLinear M=512 relu no bias    | eq / within bar (0.14) | eq | eq | eq | eq | raises      | raises
  SplitKLinear M=16384 relu          | eq                     | eq | eq | eq | eq | eq / raises | raises
  SplitKLinear 7->5 M=3073           | eq                     | eq | eq | eq | eq | eq / raises | raises
  EdgeLatentLinear                   | eq                     | eq | eq | eq | eq | raises      | raises
  EdgeFirstLayer                     | eq                     | eq | eq | eq | eq | eq / raises | raises
  EdgeTailAggregate (both)           | eq                     | eq | eq | eq | eq | eq / raises | raises
  RowsDot, SimHidden, SimResidual    | eq                     | eq | eq | eq | eq | eq / raises | raises
  update_prediction                  | eq / within bar (0.12) | eq | eq | eq | eq | eq          | raises
  update_prediction folded           | eq / within bar (0.17) | eq | eq | eq | eq | eq          | raises
  update_prediction E=0              | eq / within bar (0.05) | eq | eq | eq | eq | eq          | raises
  _Length                            | eq                     | eq | eq | eq | eq | raises      | within bar (0.17)

An entry with two words: the inputs of the case differ.  Why an entry is not "equal bits":
  C1 within bar   update_prediction: a strided pred_acc or init_position leaves the HIP path as a counted "layout" fallback (the composed
                  definitions), compared with the float64 restatement; the "offset" form stays on the kernels, which read with 4-byte
                  accesses: equal bits.  SplitKLinear below BIG_ROWS: y and dx are the LIBRARY's GEMM, which meets a strided x or weight
                  in another layout (another leading dimension, a transposed operand) and sums in another order (Case.reorder): held
                  to the node's own float64 bar; the "offset" form is contiguous and equal bits there too (the harness applies reorder
                  to strided views only, and test_contract runs the "offset" form of every case on its own).  From BIG_ROWS on csplat_linear128 reads a
                  column slice or a transpose of the weight in place, in one order: equal bits.
  C6 raises       the input is saved (x, the weights, a0, e), or, for e of the two edge-latent nodes, an output is a view of it; "equal
                  bits": the node kept a copy or its own outputs (EdgeCombine's out, the biases, xa / xb, the added rows).
  C7 raises       once_differentiable; _Length's backward is torch operations: a true second derivative, within the bar of
                  torch.linalg.vector_norm in float64 (exactly 0 on the zero rows).
No pair is n.a.  Plain forms against fp64, error / bar: 0.01 .. 0.73 (EdgeTailAggregate 0.73 and 0.70: db of the hidden layer and of the
last one, the closest calls of test_gnn_autograd_nodes_gpu.py as well; every other case below 0.19).

Two calls go through .apply although a public callable exists: LayerNorm128 (layer_norm_rows takes the node only while a graph is
recorded, and C4 calls under torch.no_grad() too) and SplitKLinear / the edge nodes (linear_rows, edge_latent_linear and message_update
keep rows below their thresholds, and inputs that require no gradient, away from the node).  LayerNorm128 is weighted with
test_layer_norm128's own zero-mean upstream gradient: see _layer_norm.

What the table showed BEFORE the fixes that came with this file (the same cases on the parent's modules: 27 of the 161 tests failed):
  C7, every case but _Length (19)   no node of graph_ops.py and not UpdatePrediction carried once_differentiable; their backward passes
                  write kernel results into fresh buffers, so under create_graph=True the gradients "came back as a constant" -- no
                  error, no graph: a Hessian-vector product or a gradient penalty through the GNN got zeros.  SplitKLinear's generic
                  branch, torch operations, returned a second derivative: one node, two behaviours.  All eleven now raise.
  C1 "offset" (8)   a contiguous input 4 bytes past a 16-byte boundary was refused by CSPLAT_REQUIRE (no launch, no fault) -- in FORWARD
                  by csplat_ln128_fwd (LayerNorm128: x, gamma, beta through _f32) and by csplat_linear128_ex (its A through
                  .contiguous(); a misaligned contiguous weight through _weight_layout's .contiguous(), which returns the tensor itself:
                  SplitKLinear from BIG_ROWS on, EdgeLatentLinear, EdgeFirstLayer, EdgeTailAggregate), and in BACKWARD by
                  csplat_dw128_bias (dw128's g and x through _f32: SplitKLinear below BIG_ROWS, whose forward is the library's GEMM and
                  takes any pointer) -- a CsplatError out of loss.backward() for an input the forward had accepted.  linear128's A,
                  _weight_layout's copy, the LayerNorm epilogue's gamma / beta, dw128's operands, LayerNorm128.forward and
                  EdgeTailAggregate's a0 now go through _f32a, which copies a misaligned tensor only: the aligned path and its bits
                  are unchanged.  linear128's gathered rows (EdgeFirstLayer's xa / xb) stay on _f32: k_linear128 reads them with
                  4-byte loads and csplat_linear128_ex asks no alignment of them.
Nothing else showed: C2 .. C6 held on the parent's modules, EdgeCombine's gm = g alias at L = 6 included.
"""
import dataclasses
from types import SimpleNamespace

import pytest

import util  # noqa: F401
import autograd_contract as ac
import gnn_kernels_ref as GR
import gnn_autograd_ref as A
import sim_rollout_ref as SR
import train_sim_ref as TSR
import knn_regs_ref as KR
import test_autograd_contract_gpu as TC
import test_gnn_autograd_nodes_gpu as TGN
import test_sim_rollout_kernels_gpu as TS
import test_train_kernels_gpu as TK
import test_knn_regs_gpu as TN

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
F64, F32 = torch.float64, torch.float32
KINDS = ("columns", "transposed", "offset")
ROWS = {}
RATIOS = {}
E, SCALE = 257, 2.0
cpu, _ratio = TC.cpu, TC._ratio


def _graph():
    N = A.nodes_for(E)
    return A.graph(E, N, "hub"), N


def _v(r, consts):
    """the restatement's inputs: the case's constants and the leaves' values, on the CPU"""
    return {**consts, **{k: cpu(t) for k, t in r.leaves.items()}}


def _groups(table, prefix):
    """the groups of one case: `prefix` itself or `prefix` + " " + what (a case's prefix ends with its bracketed name or is no other's start)"""
    return [g for g in table if g == prefix or g.startswith(prefix + " ")]


class Build:
    """what a case is built on: dev "cuda" = the nodes themselves; "cpu" = the float32 restatement stands in for the node (every draw and
    every bar of this file can then run without a GPU: tests/test_autograd_contract_meshnet_cpu.py)"""

    def __init__(self, dev):
        self.dev, self.hip = dev, dev != "cpu"

    def to(self, t):
        return None if t is None else t.detach().to(self.dev).contiguous()

    def csr(self, ei, N):
        return TGN.csr_of(ei, N) if self.hip else None

    def case(self, name, call, stand_in, diff, **kw):
        """stand_in(tensors) -> the outputs from the float32 restatement under torch's own autograd (dev "cpu")"""
        return ac.Case(name=name, call=call if self.hip else stand_in, diff={k: self.to(t) for k, t in diff.items()}, kinds=KINDS,
                       fallbacks=TC._fallbacks if self.hip else None, **kw)


def _through(value, grad_of):
    """`value`, with the gradient of `grad_of` (a node whose backward takes the gradient of its pre-activation, on the CPU stand-in)"""
    return value.detach() + (grad_of - grad_of.detach())


# ================================================================================================ EdgeCombine, SegmentSum
def _edge_combine(b, L, relu, premasked):
    ei, N = _graph()
    if L == 128:
        v, _hist = A.combine_case(E, "hub", relu)
    else:               # (no ReLU: nothing to draw again.  L % 4 != 0: the scalar kernels, and gm is the incoming gradient itself)
        g = GR._gen(5100 + L)
        v = dict(xa=torch.randn(N, L, generator=g), xb=torch.randn(N, L, generator=g), ec=torch.randn(E, L, generator=g), ei=ei, N=N, relu=relu)
    consts = dict(ei=ei, N=N, relu=relu)
    csr = b.csr(ei, N)
    name = f"EdgeCombine L={L}" + (" relu" if relu else "") + (" premasked" if premasked else "")
    group = f"contract [{name}]"

    def call(t):
        from meshnet.graph_ops import EdgeCombine
        return EdgeCombine.apply(t["xa"], t["xb"], t["ec"], csr, relu, premasked)

    def stand_in(t):
        o = A.edge_combine(None, {**consts, **t})
        return _through(o["out"], o["z"]) if premasked else o["out"]

    def bar(r):
        vv = _v(r, consts)
        r64, r32 = TGN.refs(A.edge_combine, vv, {"z" if premasked else "out": cpu(r.ups[0])})
        s_out = (vv["xa"].double().abs()[ei[1]] + vv["xb"].double().abs()[ei[0]] + vv["ec"].double().abs()).amax(1)
        TGN.check_rows(f"{group} out", name, r.outs[0], r64.out["out"], r32.out["out"], s_out)
        assert TGN.same(r.outs[0] > 0, r64.out["out"] > 0) or not relu, name
        gm64 = r64.grad["ec"]
        assert TGN.same(r.grads["ec"], gm64), f"{name}: gm is not the cotangent under the float64 mask"
        if premasked or not relu:
            assert TGN.same(r.grads["ec"], r.ups[0]), name
        TGN.check_rows(f"{group} dxa", name, r.grads["xa"], r64.grad["xa"], r32.grad["xa"], TGN.node_sum_scale(gm64, ei[1], N))
        TGN.check_rows(f"{group} dxb", name, r.grads["xb"], r64.grad["xb"], r32.grad["xb"], TGN.node_sum_scale(gm64, ei[0], N))
        return _ratio(TGN.TABLE, *_groups(TGN.TABLE, group))
    return b.case(name, call, stand_in, dict(xa=v["xa"], xb=v["xb"], ec=v["ec"]), bar=bar)


def _segment_sum(b):
    ei, N = _graph()
    msg = GR.messages(ei, 128, "ordinary")
    consts = dict(ei=ei, N=N)
    csr = b.csr(ei, N)
    group = "contract SegmentSum"

    def call(t):
        from meshnet.graph_ops import SegmentSum
        return SegmentSum.apply(t["msg"], csr)

    def bar(r):
        vv = _v(r, consts)
        r64, r32 = TGN.refs(A.segment_sum_node, vv, dict(agg=cpu(r.ups[0])))
        TGN.check_rows(group, "agg", r.outs[0], r64.out["agg"], r32.out["agg"], GR.segment_abs_sum(vv["msg"], ei[1], N).amax(1))
        assert TGN.same(r.grads["msg"], cpu(r.ups[0])[ei[1]]) and TGN.same(r.grads["msg"], r64.grad["msg"])      # (a copy)
        return _ratio(TGN.TABLE, group)
    return b.case("SegmentSum", call, lambda t: A.segment_sum_node(None, {**consts, **t})["agg"], dict(msg=msg), bar=bar)


# ================================================================================================ LayerNorm128
def _layer_norm(b, M=513):
    x = GR.ln_rows(M)
    _, _, gamma, beta = GR.linear_params(M)
    group = "contract LayerNorm128"

    def call(t):         # (.apply: layer_norm_rows takes the node only while a graph is recorded, and C4 also calls under torch.no_grad())
        from meshnet.graph_ops import LayerNorm128
        return LayerNorm128.apply(t["x"], t["gamma"], t["beta"], GR.EPS)

    def bar(r):
        vv = _v(r, {})
        g = cpu(r.ups[0])
        r64, r32 = TGN.refs(A.layer_norm128, vv, dict(y=g))
        TGN.check_classes(f"{group} y", f"M {M}", r.outs[0], r64.out["y"], r32.out["y"], r64.out["y"].abs().amax(1).clamp_min(1.0), GR.LN_CLASSES)
        v64 = vv["x"].double()
        rstd = 1.0 / ((v64 - v64.mean(1, keepdim=True)).pow(2).mean(1) + GR.EPS).sqrt()
        TGN.check_classes(f"{group} dx", f"M {M}", r.grads["x"], r64.grad["x"], r32.grad["x"],
                          rstd * (g.double() * vv["gamma"].double()).abs().amax(1), GR.LN_CLASSES)
        sc = r64.tape.scales(TGN.shapes(r64, "gamma", "beta"))
        TGN.check_columns(f"{group} dgamma", f"M {M}", r.grads["gamma"], r64.grad["gamma"], r32.grad["gamma"], sc["gamma"])
        TGN.check_columns(f"{group} dbeta", f"M {M}", r.grads["beta"], r64.grad["beta"], r32.grad["beta"], sc["beta"])
        return _ratio(TGN.TABLE, *_groups(TGN.TABLE, group))
    # the upstream gradient of test_gnn_autograd_nodes_gpu.test_layer_norm128 (zero mean): under the harness's all-positive weights the
    # rows of mean 64 and deviation 1/16 put the float32 restatement's own dx beyond BAR_MAX (1.4e-3 of rstd max |g gamma|)
    return b.case("LayerNorm128", call, lambda t: A.layer_norm128(A.Tape(), t)["y"], dict(x=x, gamma=gamma, beta=beta), bar=bar,
                  weights=lambda i, o: TGN.randn(M, M, 128))


# ================================================================================================ SplitKLinear
def _splitk(b, M, Kin, Out, relu, bias, name):
    """M = 512: csplat_dw128 (+ csplat_relu_mask_bias128) for dW / db, the library's GEMM for y and dx; M = 16384: csplat_linear128 both
    ways; 7 -> 5: torch operations, dW as a chunked batched GEMM plus a remainder row"""
    v, _hist = A.splitk_case(M, Kin, Out, relu, bias)
    consts = dict(relu=relu)
    group = f"contract [{name}]"

    def call(t):
        from meshnet.graph_ops import SplitKLinear
        return SplitKLinear.apply(t["x"], t["W"], t.get("b"), relu)

    def bar(r):
        vv = _v(r, consts)
        r64, r32 = TGN.refs(A.splitk_linear, vv, dict(y=cpu(r.ups[0])))
        sc = r64.tape.scales(TGN.shapes(r64, "x", "W", "b"))
        TGN.check_rows(f"{group} y", name, r.outs[0], r64.out["y"], r32.out["y"], A.out_scale(r64.tape.lin[0]))
        if relu:
            assert TGN.same(r.outs[0] > 0, r64.out["z"] > 0), f"{name}: the ReLU mask differs from float64's on tie-free inputs"
        TGN.check_rows(f"{group} dx", name, r.grads["x"], r64.grad["x"], r32.grad["x"], sc["x"])
        for key in ("W", "b") if bias else ("W",):
            TGN.check_columns(f"{group} d{key}", name, r.grads[key], r64.grad[key], r32.grad[key], sc[key])
        return _ratio(TGN.TABLE, *_groups(TGN.TABLE, group))

    def another_gemm(got, ref):
        """a strided x or weight reaches the LIBRARY's GEMM in another layout (another leading dimension, a transposed operand): the
        library may then pick another kernel, whose sums run in another order.  Held to the node's own float64 bar"""
        return bar(got)
    diff = dict(x=v["x"], W=v["W"], **(dict(b=v["b"]) if bias else {}))
    library = M < 16384 or (Kin, Out) != (128, 128)
    return b.case(name, call, lambda t: A.splitk_linear(A.Tape(), {**consts, **t})["y"], diff, bar=bar, reorder=another_gemm if library else None)


# ================================================================================================ EdgeLatentLinear, EdgeFirstLayer
def _edge_first(b, first):
    """the e block of the first edge Linear at scale 2 (the second processor layer); e_next is a view of e"""
    v, _hist = A.first_layer_case(E, "hub", SCALE)
    ei, N = v["ei"], v["N"]
    csr = b.csr(ei, N)
    name = "EdgeFirstLayer" if first else "EdgeLatentLinear"
    group = f"contract [{name}]"
    fn, main = (A.edge_first_layer, "z") if first else (A.edge_latent_linear, "ec")
    pad = torch.full((128, 256), 77.0)

    def restate_inputs(t, like=None):
        w = t["W"]
        return dict(e=t["e"], Wfull=torch.cat([pad.to(w.dtype), w], 1), scale=SCALE, xa=t.get("xa"), xb=t.get("xb"), ei=ei, N=N)

    def call(t):
        from meshnet.graph_ops import EdgeFirstLayer, EdgeLatentLinear
        if first:
            return EdgeFirstLayer.apply(t["e"], t["W"], SCALE, t["xa"], t["xb"], csr)
        return EdgeLatentLinear.apply(t["e"], t["W"], SCALE)

    def stand_in(t):
        o = fn(A.Tape(), restate_inputs(t))
        return (_through(o["a0"], o["z"]) if first else o["ec"]), o["e_next"]

    def bar(r):
        vv = restate_inputs({k: cpu(t) for k, t in r.leaves.items()})
        g, gn = cpu(r.ups[0]), cpu(r.ups[1])
        wrt = ("e", "Wfull", "xa", "xb") if first else ("e", "Wfull")
        r64, r32 = TGN.refs(fn, {k: t for k, t in vv.items() if t is not None}, {main: g, "e_next": gn}, wrt)
        sc = r64.tape.scales(TGN.shapes(r64, "e", "Wfull"))
        s_out = A.out_scale_full(r64.tape.lin[0])
        if first:
            s_out = s_out + vv["xa"].double().abs()[ei[1]] + vv["xb"].double().abs()[ei[0]]
        key = "a0" if first else "ec"
        TGN.check_rows(f"{group} out", name, r.outs[0], r64.out[key], r32.out[key], s_out.amax(1))
        if first:
            assert TGN.same(r.outs[0] > 0, r64.out["z"] > 0), f"{name}: a0 > 0 differs from the float64 mask on tie-free inputs"
        assert TGN.same(r.outs[1], vv["e"]), name
        TGN.check_rows(f"{group} de", name, r.grads["e"], r64.grad["e"], r32.grad["e"], sc["e"] + gn.double().abs().amax(1))
        TGN.check_columns(f"{group} dW", name, r.grads["W"], r64.grad["Wfull"][:, 256:], r32.grad["Wfull"][:, 256:], sc["Wfull"][:, 256:])
        if first:
            TGN.check_rows(f"{group} dxa", name, r.grads["xa"], r64.grad["xa"], r32.grad["xa"], TGN.node_sum_scale(g, ei[1], N))
            TGN.check_rows(f"{group} dxb", name, r.grads["xb"], r64.grad["xb"], r32.grad["xb"], TGN.node_sum_scale(g, ei[0], N))
        return _ratio(TGN.TABLE, *_groups(TGN.TABLE, group))
    diff = dict(e=v["e"], W=v["Wfull"][:, 256:].contiguous(), **(dict(xa=v["xa"], xb=v["xb"]) if first else {}))
    return b.case(name, call, stand_in, diff, outputs=(0, 1), bar=bar)


# ================================================================================================ EdgeTailAggregate
def _edge_tail(b, k, a0_relu):
    """the node itself (S, the sums of the normalised rows): the LayerNorm's affine part behind it is the caller's torch operations"""
    v, _hist = A.tail_case(E, k, a0_relu)
    ei, N = v["ei"], v["N"]
    csr = b.csr(ei, N)
    name = f"EdgeTailAggregate k={k}" + (" a0_relu" if a0_relu else "")
    group = f"contract [{name}]"
    keys = ["a0"] + [f"{n}{i}" for i in range(1, k + 1) for n in "Wb"]
    consts = dict(a0_relu=a0_relu, ei=ei, N=N, k=k, gamma=v["gamma"], beta=v["beta"])

    def call(t):
        from meshnet.graph_ops import EdgeTailAggregate
        return EdgeTailAggregate.apply(t["a0"], csr, GR.EPS, a0_relu, *[t[key] for key in keys[1:]])

    def bar(r):
        vv = _v(r, consts)
        r64, r32 = TGN.refs(A.edge_tail_aggregate, vv, dict(S=cpu(r.ups[0])), keys)
        sc = r64.tape.scales(TGN.shapes(r64, *keys))
        TGN.check_rows(f"{group} S", name, r.outs[0], r64.out["S"], r32.out["S"], TGN.node_sum_scale(r64.out["xhat"], ei[1], N))
        TGN.check_rows(f"{group} da0", name, r.grads["a0"], r64.grad["a0"], r32.grad["a0"], sc["a0"])
        if a0_relu:
            zero = vv["a0"] == 0
            assert bool(zero.any()) and not bool(cpu(r.grads["a0"])[zero].any()), f"{name}: a0 = 0 must get gradient 0"
        for key in keys[1:]:
            TGN.check_columns(f"{group} d{key}", name, r.grads[key], r64.grad[key], r32.grad[key], sc[key])
        return _ratio(TGN.TABLE, *_groups(TGN.TABLE, group))
    return b.case(name, call, lambda t: A.edge_tail_aggregate(A.Tape(), {**consts, **t})["S"], {key: v[key] for key in keys}, bar=bar)


# ================================================================================================ the simulator's residual MLP, T = 3, V = 37
SIM_T, SIM_V = 3, 37


def _sim_inputs():
    e8, W1, b1, W2, b2, _ = SR.sim_hidden_case(13)
    h8, Wo, bo, add8, _dy = SR.rows_dot_case(3 * SIM_V)
    return dict(e=e8[:SIM_T], W1=W1, b1=b1, W2=W2, b2=b2, h=h8[:SIM_T], Wo=Wo, bo=bo, base=add8[:SIM_T].contiguous())


def _lin(t, w, bias):
    return SimpleNamespace(weight=t[w], bias=t[bias])


def _rows_dot(b):
    s = _sim_inputs()
    group = "contract RowsDot"

    def call(t):
        from meshnet.graph_ops import rows_dot
        y = rows_dot(t["h"], t["Wo"], t["bo"], t["base"])
        assert type(y.grad_fn).__name__.startswith("RowsDot") or not y.requires_grad
        return y

    def bar(r):
        L = {k: cpu(t) for k, t in r.leaves.items()}
        g = cpu(r.ups[0])
        res = [(SR.rows_dot(L["h"], L["Wo"], L["bo"], L["base"], dt),) + SR.rows_dot_grads(L["h"], L["Wo"], g, dt) for dt in (F64, F32)]
        TS.check(group, "y", r.outs[0], res[0][0], res[1][0], 1e-30)
        for n, key in enumerate(("Wo", "bo", "h")):
            TS.check(group, f"d/d{key}", r.grads[key], res[0][1 + n], res[1][1 + n], 1e-30)
        assert TGN.same(r.grads["base"], g), "the gradient of the added rows is the incoming gradient itself"
        return _ratio(TS.TABLE, group)
    return b.case("RowsDot", call, lambda t: SR.rows_dot(t["h"], t["Wo"], t["bo"], t["base"], F32), {k: s[k] for k in ("h", "Wo", "bo", "base")},
                  bar=bar)


def _sim_hidden(b):
    s = _sim_inputs()
    e = b.to(s["e"])
    group = "contract SimHidden"
    names = ("W1", "b1", "W2", "b2")

    def call(t):
        from meshnet.graph_ops import sim_hidden
        h2 = sim_hidden(e, _lin(t, "W1", "b1"), _lin(t, "W2", "b2"))
        assert type(h2.grad_fn).__name__.startswith("SimHidden") or not h2.requires_grad
        return h2

    def bar(r):
        L = [cpu(r.leaves[k]) for k in names]
        res = [(SR.sim_hidden(s["e"], *L, dt)[1],) + SR.sim_hidden_grads(s["e"], *L, cpu(r.ups[0]), dt) for dt in (F64, F32)]
        TS.check(group, "h2", r.outs[0], res[0][0], res[1][0], 1e-30)
        for n, key in enumerate(names):
            TS.check(group, f"d/d{key}", r.grads[key], res[0][1 + n], res[1][1 + n], 1e-30)
        return _ratio(TS.TABLE, group)
    return b.case("SimHidden", call, lambda t: SR.sim_hidden(e, *[t[k] for k in names], F32)[1], {k: s[k] for k in names}, bar=bar)


def _sim_residual(b):
    s = _sim_inputs()
    e = b.to(s["e"])
    group = "contract SimResidual"
    names = ("W1", "b1", "W2", "b2", "Wo", "bo")

    def call(t):
        from meshnet.graph_ops import sim_residual
        y = sim_residual(e, _lin(t, "W1", "b1"), _lin(t, "W2", "b2"), _lin(t, "Wo", "bo"), t["base"])
        assert type(y.grad_fn).__name__.startswith("SimResidual") or not y.requires_grad
        return y

    def stand_in(t):
        return SR.rows_dot(SR.sim_hidden(e, *[t[k] for k in names[:4]], F32)[1], t["Wo"], t["bo"], t["base"], F32)

    def bar(r):
        L = {k: cpu(t) for k, t in r.leaves.items()}
        g = cpu(r.ups[0])
        res = []
        for dt in (F64, F32):
            h2 = SR.sim_hidden(s["e"], *[L[k] for k in names[:4]], dt)[1]
            dWo, dbo, dh = SR.rows_dot_grads(h2, L["Wo"], g, dt)
            res.append(dict(zip(("y",) + names, (SR.rows_dot(h2, L["Wo"], L["bo"], L["base"], dt),) +
                                SR.sim_hidden_grads(s["e"], *[L[k] for k in names[:4]], dh, dt) + (dWo, dbo))))
        TS.check(group, "y", r.outs[0], res[0]["y"], res[1]["y"], 1e-30)
        for key in names:
            TS.check(group, f"d/d{key}", r.grads[key], res[0][key], res[1][key], 1e-30)
        assert TGN.same(r.grads["base"], g), "the gradient of the added rows is the incoming gradient itself"
        return _ratio(TS.TABLE, group)
    return b.case("SimResidual", call, stand_in, {k: s[k] for k in names + ("base",)}, bar=bar)


# ================================================================================================ UpdatePrediction, N = 65, H = 2
UP_N, UP_H = 65, 2


def _update_prediction(b, fold, edges):
    """through update_prediction (fold: the internal transition, with the output normaliser's statistics); a strided pred_acc or
    init_position leaves the HIP path as a counted "layout" fallback (the composed definitions), held to the bar below"""
    ei = A.graph(E, UP_N, "hub") if edges else torch.zeros(2, 0, dtype=torch.int64)
    d = TSR.inputs(UP_N, UP_H, "grasped, one component exactly 0", with_noise=True, fold=fold, seed=3)
    name = "update_prediction" + (" folded" if fold else "") + ("" if edges else " E=0")
    group = f"contract [{name}]"
    ei_d = b.to(ei)
    c = {k: b.to(d[k]) for k in ("noise", "velocity", "old_actions", "actions", "omean", "ostd")}

    def call(t):
        from meshnet import train_sim as ts
        if fold:
            return ts._transition(c["noise"], c["velocity"], t["pred_acc"], t["init_position"], ei_d, c["old_actions"], c["actions"], UP_H,
                                  c["omean"], c["ostd"], "update_prediction")
        return ts.update_prediction(c["noise"], c["velocity"], t["pred_acc"], t["init_position"], ei_d, c["old_actions"], c["actions"], None, UP_H)

    def restate(pa, p0, dt):
        return TSR.forward(d["velocity"], d["noise"], pa, p0, d["old_actions"], d["actions"], ei, UP_H, dt, d["omean"], d["ostd"])

    def bar(r):
        pa, p0 = cpu(r.leaves["pred_acc"]), cpu(r.leaves["init_position"])
        g_ef, g_pos = cpu(r.ups[1]), cpu(r.ups[2])
        f64, f32 = restate(pa, p0, F64), restate(pa, p0, F32)
        unit = float(max(g_ef.abs().max() if g_ef.numel() else 0.0, g_pos.abs().max()))
        assert torch.equal(cpu(r.outs[0]), f32[0]) and not r.raw[0].requires_grad, f"{name}: hist"
        TK.check(group, "new_pos", r.outs[2], f64[2], f32[2], 1e-30)
        if edges:
            TK.check(group, "edge_feat", r.outs[1], f64[1], f32[1], 1e-30)
        b64 = TSR.backward(f64[1], g_ef, g_pos, d["old_actions"], d["actions"], ei, F64, d["ostd"])
        b32 = TSR.backward(f32[1], g_ef, g_pos, d["old_actions"], d["actions"], ei, F32, d["ostd"])
        for n, key in enumerate(("pred_acc", "init_position")):
            TK.check(group, f"g_{key}", r.grads[key], b64[n], b32[n], unit)
        free = (d["actions"] == 0) & (d["old_actions"] == 0)
        assert bool((~free).any()) and not bool(cpu(r.grads["pred_acc"])[~free].any()), f"{name}: a masked component's gradient is not 0"
        return _ratio(TK.TABLE, group)
    class StandIn(torch.autograd.Function):
        """the float32 restatement's forward with ITS stated backward (torch's own has no gradient for an edge of length 0: a self loop)"""

        @staticmethod
        def forward(ctx, pa, p0):
            ctx.set_materialize_grads(False)
            hist, ef, pos = restate(pa.detach(), p0.detach(), F32)
            ctx.ef = ef
            ctx.mark_non_differentiable(hist)
            return hist, ef, pos

        @staticmethod
        def backward(ctx, _g_hist, g_ef, g_pos):
            return TSR.backward(ctx.ef, g_ef, g_pos, d["old_actions"], d["actions"], ei, F32, d["ostd"])
    return b.case(name, call, lambda t: StandIn.apply(t["pred_acc"], t["init_position"]), dict(pred_acc=d["pred_acc"], init_position=d["init_position"]),
                  outputs=(1, 2), bar=bar)


# ================================================================================================ _Length
def _length(b):
    """the composed branch's node on GPU tensors: its backward is torch operations, so create_graph yields a true second derivative"""
    off = torch.randn(3, 40, 5, 3, generator=GR._gen(5200))
    zero = torch.zeros(3, 40, 5, dtype=torch.bool)
    zero[:, ::7, 1] = True
    zero[1, 3] = True
    off[zero] = 0.0
    group = "contract _Length"

    def call(t):
        from csplat.knn_regs import _Length
        return _Length.apply(t["off"])

    def rule(what, got, x32, x64):
        """test_knn_regs_gpu.compare's: the error, relative to the tensor's largest component, within 4 e32 + 4 u"""
        e32, ek = KR.scale_err(cpu(x32).numpy(), cpu(x64).numpy()), KR.scale_err(cpu(got).numpy(), cpu(x64).numpy())
        bound = 4 * e32 + 4 * KR.U
        print(f"{group} {what}: e32 {e32 / KR.U:.2f} u, node {ek / KR.U:.2f} u, error / bound {ek / bound:.3f}")
        assert ek <= bound, f"{group} {what}: error {ek:.3e} beyond 4 e32 + 4 u = {bound:.3e}"
        if ek / bound > TN.WORST["ratio"]:          # (that file's record of the closest call)
            TN.WORST.update(ratio=ek / bound, where=f"{group} {what}")
        return ek / bound

    def norm(x):
        """torch.linalg.vector_norm on the rows that are not zero, exact 0 (and no gradient) on the zero rows"""
        out = torch.zeros(x.shape[:-1], dtype=x.dtype)
        keep = ~zero
        return out.masked_scatter(keep, torch.linalg.vector_norm(x[keep], dim=-1))

    def bar(r):
        res = []
        for dt in (F64, F32):
            x = TC._leaf(r.leaves["off"], dt)
            dlen = norm(x)
            dlen.backward(cpu(r.ups[0]).to(dt))
            res.append((dlen.detach(), x.grad))
        assert not bool(cpu(r.outs[0])[zero].any()) and not bool(cpu(r.grads["off"])[zero].any()), "a zero row: |off| = 0 and gradient 0"
        return max(rule("d", r.outs[0], res[1][0], res[0][0]), rule("d/d off", r.grads["off"], res[1][1], res[0][1]))

    def second(r):
        """d/d off and d/d upstream of <u off / |off|, probe>"""
        res = []
        for dt in (F64, F32):
            x, u = TC._leaf(r["leaves"]["off"], dt), TC._leaf(r["ups"][0], dt)
            first, = torch.autograd.grad(norm(x), x, u, create_graph=True)
            first.backward(cpu(r["probe"]["off"]).to(dt))
            res.append((x.grad, u.grad))
        got = (r["d_leaves"]["off"], r["d_ups"][0])
        for gt in got:
            assert gt is not None and not bool(cpu(gt)[zero].any()), "a zero row: second derivative exactly 0"
        return max(rule("second d/d off", got[0], res[1][0], res[0][0]), rule("second d/d upstream", got[1], res[1][1], res[0][1]))
    return b.case("_Length", call, lambda t: norm(t["off"]), dict(off=off), bar=bar, second=second)


# ================================================================================================ the table
CASES = {
    "EdgeCombine L=128 relu": lambda b: _edge_combine(b, 128, True, False),
    "EdgeCombine L=128 relu premasked": lambda b: _edge_combine(b, 128, True, True),
    "EdgeCombine L=6": lambda b: _edge_combine(b, 6, False, False),
    "SegmentSum": _segment_sum,
    "LayerNorm128": _layer_norm,
    "SplitKLinear M=512": lambda b: _splitk(b, 512, 128, 128, False, True, "SplitKLinear M=512"),
    "SplitKLinear M=16384 relu": lambda b: _splitk(b, 16384, 128, 128, True, True, "SplitKLinear M=16384 relu"),
    "SplitKLinear 7->5 M=3073": lambda b: _splitk(b, 3073, 7, 5, True, True, "SplitKLinear 7->5 M=3073"),
    "SplitKLinear M=512 relu no bias": lambda b: _splitk(b, 512, 128, 128, True, False, "SplitKLinear M=512 relu no bias"),
    "EdgeLatentLinear": lambda b: _edge_first(b, False),
    "EdgeFirstLayer": lambda b: _edge_first(b, True),
    "EdgeTailAggregate k=2 a0_relu": lambda b: _edge_tail(b, 2, True),
    "EdgeTailAggregate k=1": lambda b: _edge_tail(b, 1, False),
    "RowsDot": _rows_dot, "SimHidden": _sim_hidden, "SimResidual": _sim_residual,
    "update_prediction": lambda b: _update_prediction(b, False, True),
    "update_prediction folded": lambda b: _update_prediction(b, True, True),
    "update_prediction E=0": lambda b: _update_prediction(b, False, False),
    "_Length": _length,
}
RAISES_C7 = [name for name in CASES if name != "_Length"]          # every node whose backward launches a kernel (SplitKLinear: in any branch)
_BUILT = {}


def built(name, dev="cuda"):
    """the case and its plain form, evaluated once and left unchanged"""
    if (name, dev) not in _BUILT:
        case = CASES[name](Build(dev))
        assert case.name == name, (case.name, name)
        _BUILT[(name, dev)] = (case, ac.plain(case))
    return _BUILT[(name, dev)]


@pytest.fixture(scope="module", autouse=True)
def _threads_and_table():
    old = torch.get_num_threads()
    torch.set_num_threads(min(16, old))
    yield
    torch.set_num_threads(old)
    rows = dict(ROWS)
    print("\n" + ac.table(rows, list(CASES)))
    print("plain form, error / bar against fp64: " + ", ".join(f"{k} {v:.2f}" for k, v in RATIOS.items()))
    for (name, clause), entry in rows.items():
        if entry == ac.NA:
            print(f"n.a. {name} {clause}: {_BUILT[(name, 'cuda')][0].na[clause]}")
    _BUILT.clear()


@pytest.mark.parametrize("name", list(CASES))
def test_plain_form_meets_the_fp64_bar(name):
    case, ref = built(name)
    RATIOS[name] = case.bar(ref)
    assert RATIOS[name] <= 1.0, RATIOS[name]


@pytest.mark.parametrize("clause", ac.CLAUSES)
@pytest.mark.parametrize("name", list(CASES))
def test_contract(name, clause):
    case, ref = built(name)
    ROWS[(name, clause)] = "FAILED"
    entry = ROWS[(name, clause)] = ac.run_clause(case, clause, ref)
    if clause == "C7" and name in RAISES_C7:
        assert entry == ac.RAISES, entry
    elif clause == "C7":
        assert entry.startswith("within bar"), entry        # (a true second derivative, against float64)
    if clause == "C1" and not name.startswith(("update_prediction", "SplitKLinear")):
        assert entry == ac.EQUAL, entry
    if clause == "C1":      # the "offset" kind alone, no bar of any kind: copied, or read with 4-byte accesses -- equal bits (no case refuses)
        alone = ac.c1(dataclasses.replace(case, kinds=("offset",), reorder=None, bar=None), ref)
        assert alone == ac.EQUAL, alone
    if clause == "C6" and name in ("EdgeLatentLinear", "EdgeFirstLayer"):
        assert ac.RAISES in entry.split(" / "), entry
        # e alone (the other inputs constants): e_next is a view of e, so autograd refuses the backward after an edit of e
        rest = {k: t for k, t in case.diff.items() if k != "e"}
        alone = ac.c6(dataclasses.replace(case, diff=dict(e=case.diff["e"]), const={**case.const, **rest}), ref)
        assert alone == ac.RAISES, alone


def test_at_most_one_pair_in_five_does_not_apply():
    na = sum(len(built(name)[0].na) for name in CASES)
    assert 5 * na <= len(CASES) * len(ac.CLAUSES), na
