"""The MeshNet training transition on the GPU (csplat_train_update_fwd / _bwd in csrc/csplat_train_sim.hip, behind meshnet.train_sim) against
the restatement tests/train_sim_ref.py, and the unrolled loss around a small ClothMeshSimulator, under strict dispatch.

Forward: hist and new_pos are compared with torch.equal against the float32 restatement (one rounded operation per element on both
sides), edge_feat with torch.equal against meshnet.rollout.edge_features on new_pos.  Backward: g_pred_acc and g_init_position follow the
rule of tests/test_train_kernels_gpu.py (its check() and TABLE are used): within 8 x the float32 restatement's own error against float64,
floor 1e-6, relative to the larger of the largest reference magnitude and the size of the incoming gradients.  Masked components are
compared for equality with 0, nodes without edges with g_new_pos, two runs with each other.

Sizes (tests/test_train_sim_cpu.py states which launch constant each crosses): N = 1, 2, 255, 256, 257, 1000 with 3 N + 1 random edges;
the graphs of tests/gnn_kernels_ref.py at N = 1000 (the 3000-edge hub, every edge ending at the last node, duplicates, self loops,
in-degrees 0..9) and E = 0; H = 1, 2, 3; the five action cases, with and without noise, the normaliser folded and not.

End to end: ClothMeshSimulator (latent 128, 2 message-passing steps, 300 nodes, 2100 edges, H = 2, trained normalisers), unrolled_loss at
F = 1, 2, 3 against the same loop with the transition composed in float64 torch operations around the same float32 network.  The loss and
every parameter gradient, grouped by kind, follow the bar rule of tests/test_gnn_autograd_nodes_gpu.py (its check_rows: 8 x e32, floor
1e-6, a bar above 1e-3 fails by itself), e32 being the same loop with the transition composed in float32; a gradient tensor is one row,
relative to its largest float64 magnitude.

What the table showed on an MI355X when this file was written (group | comparisons | largest e32 | largest bar | largest kernel error |
smallest bar / error):
  train_sim g_init_position | 150 | 1.27e-06 | 1.01e-05 | 1.29e-06 | 6.9
  train_sim g_pred_acc      | 150 | 7.48e-07 | 5.98e-06 | 5.10e-07 | 7.1
  train_sim dW              |  63 | 3.12e-05 | 2.49e-04 | 3.37e-07 | 5.5
  train_sim db              |  63 | 3.43e-05 | 2.75e-04 | 2.25e-07 | 5.3
  train_sim dbeta           |  18 | 1.07e-05 | 8.60e-05 | 1.97e-07 | 5.7
  train_sim dgamma          |  18 | 8.51e-06 | 6.81e-05 | 2.14e-07 | 4.9
  train_sim loss            |   3 | 0        | 1.00e-06 | 0        | -
  train_sim step loss       |   6 | 0        | 1.00e-06 | 0        | -
The transition's gradients sit at the float32 restatement's own error (the largest e32, 1.3e-6, is the 3000-edge hub: one node's sum of
3000 terms).  End to end the losses of the three loops are the same float32 numbers (a last-bit difference of the edge features moves a
mean over 900 squared errors by less than its rounding), the gradients differ: the largest e32 (3e-5) are F = 3, where two transitions
carry the float32 positions' rounding into edge lengths of 0.02; the kernels stay at 2e-7 .. 3.4e-7 of the float64 loop there, i.e. they
round like the float32 loop's forward and better than its scatter-add backward.  The path through the edge features (F = 2): the float64
loop with the prediction detached in front of the transition differs from the whole one by 2.3e-4 of the edge encoder's first weight
gradient (8.0e-5 .. 3e-4 over all weights) at a bar of 2.1e-6; the kernels are 2.0e-7 from the whole loop and 2.3e-4 from the cut one.
No training-mode node of graph_ops.py / graph_network.py dropped the gradient of the raw edge-feature input: nothing had to be fixed.
Wall time 3 s for the 24 tests of this file (the slowest, N = 1 with its first-call set-up, 1.2 s)."""
import copy

import pytest

import util  # noqa: F401
import gnn_kernels_ref as G
import train_sim_ref as R
from test_train_kernels_gpu import FLOOR, K, TABLE, check  # noqa: F401  (the project's rule for a bar, and the table of its comparisons)
from test_gnn_autograd_nodes_gpu import TABLE as ROWS_TABLE, check_rows  # (the bar rule of the autograd nodes, and its table)

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
from meshnet import rollout, train_sim as ts  # noqa: E402  (absent: every test of this file fails)
from meshnet.train_sim import collate, train_step, unrolled_loss, update_prediction  # noqa: E402

F64, F32 = torch.float64, torch.float32
W = R.WORKGROUP


@pytest.fixture(scope="module", autouse=True)
def _table():
    yield
    print("\ngroup | comparisons | largest e32 | largest bar | largest kernel error | smallest bar / error")
    for table in (TABLE, ROWS_TABLE):
        for g in sorted(g for g in table if g.startswith("train_sim")):
            n, e32, bar, err, margin = table[g]
            print(f"{g} | {n} | {e32:.2e} | {bar:.2e} | {err:.2e} | {margin:.1f}")


def cu(t, grad=False):
    return None if t is None else t.detach().cuda().requires_grad_(grad)


def transition_case(N, ei, H, kind, with_noise, fold, seed=0, what=""):
    """one transition forward and backward on the kernels, every output and gradient against the restatement"""
    E = int(ei.shape[1])
    d = R.inputs(N, H, kind, with_noise=with_noise, fold=fold, seed=seed)
    g_ef, g_pos = R.incoming(N, E, seed)
    args = (d["velocity"], d["noise"], d["pred_acc"], d["init_position"], d["old_actions"], d["actions"], ei, H)
    h32, e32_, p32 = R.forward(*args, F32, d["omean"], d["ostd"])
    e64 = R.forward(*args, F64, d["omean"], d["ostd"])[1]
    ei_g = ei.cuda()

    def run():
        pa, p0 = cu(d["pred_acc"], True), cu(d["init_position"], True)
        if fold:
            out = ts._transition(cu(d["noise"]), cu(d["velocity"]), pa, p0, ei_g, cu(d["old_actions"]), cu(d["actions"]), H, cu(d["omean"]), cu(d["ostd"]),
                                 "update_prediction")
        else:
            out = update_prediction(cu(d["noise"]), cu(d["velocity"]), pa, p0, ei_g, cu(d["old_actions"]), cu(d["actions"]), "cuda", H)
        return out, pa, p0
    (hist, ef, pos), pa, p0 = run()
    tag = f"{what} N{N} E{E} H{H} {kind}{' noise' if with_noise else ''}{' folded' if fold else ''}"
    assert hist.dtype == F32 and hist.shape == (N, 3 * H) and ef.shape == (E, 4) and pos.shape == (N, 3) and not hist.requires_grad
    assert torch.equal(hist.cpu(), h32) and torch.equal(pos.detach().cpu(), p32), tag
    assert torch.equal(ef.detach(), rollout.edge_features(pos.detach(), ei_g)), tag
    assert torch.equal(ef.detach().cpu()[:, :3], e32_[:, :3]), tag
    # backward: both incoming gradients, then each alone
    unit = float(max(g_ef.abs().max() if E else 0.0, g_pos.abs().max()))
    free = ((d["actions"] == 0) & (d["old_actions"] == 0))
    deg = torch.bincount(ei.reshape(-1), minlength=N)
    for name, ge, gp in (("both", g_ef, g_pos), ("edges only", g_ef, None), ("positions only", None, g_pos)):
        outs, gos = zip(*[(o, cu(g)) for o, g in ((ef, ge), (pos, gp)) if g is not None])
        got = torch.autograd.grad(outs, (pa, p0), gos, retain_graph=True)
        r64 = R.backward(e64, ge, gp, d["old_actions"], d["actions"], ei, F64, d["ostd"])
        r32 = R.backward(e32_, ge, gp, d["old_actions"], d["actions"], ei, F32, d["ostd"])
        for k, which in enumerate(("g_pred_acc", "g_init_position")):
            check(f"train_sim {which}", f"{tag} [{name}]", got[k], r64[k], r32[k], unit)
        assert not got[0].cpu()[~free].any(), tag                                        # masked components: exactly 0
        lone = deg == 0
        want = torch.zeros(N, 3) if gp is None else gp
        assert torch.equal(got[1].cpu()[lone], want[lone]), tag                          # nodes without edges: g_new_pos itself
        if name == "positions only":
            assert torch.equal(got[1].cpu(), gp), tag
        again = torch.autograd.grad(outs, (pa, p0), gos, retain_graph=True)
        assert torch.equal(again[0], got[0]) and torch.equal(again[1], got[1]), tag      # two runs: equal bits
    (hist2, ef2, pos2), _pa, _p0 = run()
    assert torch.equal(hist2, hist) and torch.equal(ef2, ef) and torch.equal(pos2, pos), tag


@pytest.mark.parametrize("N", [1, 2, W - 1, W, W + 1, 1000])
def test_sizes_around_the_workgroup(N):
    for H in (1, 2, 3):
        transition_case(N, R.random_graph(N, 3 * N + 1, seed=H), H, "grasped, one component exactly 0", with_noise=H != 2, fold=H != 1, seed=H,
                        what="size")


@pytest.mark.parametrize("graph", G.GRAPHS + ("no edges",))
def test_graphs_with_a_hub_lonely_nodes_duplicates_and_self_loops(graph):
    N = 1000
    ei = torch.zeros(2, 0, dtype=torch.int64) if graph == "no edges" else G.graph(N, graph)
    if graph == "hub":
        assert int(torch.bincount(ei[1], minlength=N).max()) == G.HUB_DEGREE
    transition_case(N, ei, 2, "grasped, three components", with_noise=True, fold=True, what=graph)
    transition_case(N, ei, 2, "all zero", with_noise=False, fold=False, what=graph)


@pytest.mark.parametrize("kind", R.ACTION_CASES)
def test_action_cases_with_and_without_noise_folded_and_not(kind):
    N = W + 1
    ei = R.random_graph(N, 1500, seed=9)
    for with_noise in (True, False):
        for fold in (True, False):
            transition_case(N, ei, 3, kind, with_noise, fold, what="actions")


def test_a_form_the_kernels_do_not_cover_is_reported_not_composed_silently():
    from csplat import native
    d = R.inputs(10, 2)
    ei = R.random_graph(10, 20).cuda()
    args = [cu(d[k]) for k in ("noise", "velocity", "pred_acc", "init_position")] + [ei, cu(d["old_actions"]), cu(d["actions"])]
    for i, bad in ((1, args[1].double()), (5, torch.zeros(10, 2, 3, device="cuda")[:, 0])):
        a = list(args)
        a[i] = bad
        if i == 1:
            a[0] = a[0].double()
        with pytest.raises(native.CsplatError, match="update_prediction"):
            update_prediction(*a)
    with native.allow_fallbacks("dtype", "layout"):
        a = list(args)
        a[5] = torch.zeros(10, 2, 3, device="cuda")[:, 0]
        a[5].copy_(args[5])
        got = update_prediction(*a)
    want = update_prediction(*args)
    assert torch.equal(got[0], want[0]) and torch.equal(got[2], want[2]) and torch.equal(got[1][:, :3], want[1][:, :3])


# ================================================================================================ end to end
def cloth(N=300, k=7, H=2, S=3, seed=0):
    """a 15 x 20 jittered grid of spacing 0.02, every node receiving an edge from each of its 7 nearest: 2100 edges; one grasped node;
    velocities of a quarter of the spacing per step"""
    g = torch.Generator().manual_seed(700 + seed)
    xs, ys = torch.meshgrid(torch.arange(15.0), torch.arange(20.0), indexing="ij")
    pos = torch.stack([xs.reshape(-1), ys.reshape(-1), torch.zeros(N)], 1) * 0.02 + (torch.rand(N, 3, generator=g) - 0.5) * 0.004
    near = torch.cdist(pos.double(), pos.double()).topk(k + 1, largest=False).indices[:, 1:]
    ei = torch.stack([near.reshape(-1), torch.arange(N).repeat_interleave(k)]).contiguous()
    node_types = torch.zeros(N, 1)
    grasped = N // 2 + 3 + seed
    node_types[grasped] = 1
    act = torch.zeros(N, S, 3)
    act[grasped] = torch.randn(S, 3, generator=g) * 5e-3
    act[grasped, 1, 2] = 0.0
    d = pos[ei[0]] - pos[ei[1]]
    ef = torch.cat([d, torch.sqrt((d * d).sum(1, keepdim=True))], 1)
    return (torch.randn(N, 3 * H, generator=g) * 5e-3, node_types, ei, ef, torch.randn(N, S, 3, generator=g) * 5e-3, act, pos)


@pytest.fixture(scope="module")
def simulator():
    from meshnet.cloth_network import ClothMeshSimulator
    torch.manual_seed(5)
    sim = ClothMeshSimulator(3, 8, 4, 128, 2, 2, 128, 2, 2, normalize=True, device="cuda")
    b = [t.cuda() for t in cloth()]
    with torch.no_grad():            # statistics for both normalisers, then no more accumulation
        sim.train()
        sim._encoder_preprocessor(b[0], b[1])
        sim._output_normalizer(b[4][:, 0] - b[0][:, -3:], True)
    return sim.eval()


def composed_loop(sim, b, F, dtype, cut=False):
    """the reference's loop with the transition from the restatement's torch operations in `dtype` on the GPU, torch's autograd behind
    them; the float32 network sees float32 inputs.  cut: the prediction is detached before the transition"""
    vel, nt, ei, ef, tgt, act, pos = b
    vel, pos, tgt = vel.to(dtype), pos.to(dtype), tgt.to(dtype)
    on = sim._output_normalizer
    omean, ostd = on._mean().reshape(-1), on._std_with_epsilon().reshape(-1)
    loss, steps = None, []
    for f in range(F):
        pred, target = sim.predict_acceleration(vel.float(), nt, ei, ef.float(), tgt[:, f].float())
        steps.append(((pred - target) ** 2).mean())
        loss = steps[-1] if loss is None else loss + steps[-1]
        if f < F - 1:
            vel, ef, pos = R.forward(vel, None, pred.detach() if cut else pred, pos, act[:, f], act[:, f + 1], ei, vel.shape[1] // 3, dtype, omean, ostd)
    return loss, steps


def kinds(sim):
    for name, q in sim.named_parameters():
        layer_norm = name.rsplit(".", 2)[-2] == "1"          # (`..._fn.1.weight`: the LayerNorm behind a build_mlp; Linears are `NN-i`)
        yield name, q, ("dgamma" if name.endswith("weight") else "dbeta") if layer_norm else ("dW" if q.dim() == 2 else "db")


def grads_of(sim, loss):
    params = [q for _n, q in sim.named_parameters()]
    return dict(zip([n for n, _q in sim.named_parameters()], torch.autograd.grad(loss, params, allow_unused=True)))


LOOPS = {}


def loops(sim, b, F):
    """(loss, per-step losses, gradients) of the kernels' loop, the float64 and the float32 composed loops and the cut float64 loop,
    computed once per F and shared"""
    if F not in LOOPS:
        res = {}
        for key, fn in (("got", lambda: unrolled_loss(sim, *b, F)), ("r64", lambda: composed_loop(sim, b, F, F64)),
                        ("r32", lambda: composed_loop(sim, b, F, F32)), ("cut", lambda: composed_loop(sim, b, F, F64, cut=True))):
            loss, steps = fn()
            res[key] = (loss.detach(), [s.detach() for s in steps], grads_of(sim, loss))
        LOOPS[F] = res
    return LOOPS[F]


@pytest.mark.parametrize("F", [1, 2, 3])
def test_unrolled_loss_against_the_float64_transition_around_the_same_network(simulator, F):
    b = [t.cuda() for t in cloth()]
    res = loops(simulator, b, F)
    got, r64, r32 = res["got"], res["r64"], res["r32"]
    assert len(got[1]) == F
    check_rows("train_sim loss", f"F{F}", got[0].reshape(1, 1), r64[0].reshape(1, 1), r32[0].reshape(1, 1), float(r64[0].abs()))
    for f in range(F):
        check_rows("train_sim step loss", f"F{F} f{f}", got[1][f].reshape(1, 1), r64[1][f].reshape(1, 1), r32[1][f].reshape(1, 1), float(r64[1][f].abs()))
    for name, q, kind in kinds(simulator):
        assert got[2][name] is not None, name
        check_rows(f"train_sim {kind}", f"F{F} {name}", got[2][name].reshape(1, -1), r64[2][name].reshape(1, -1), r32[2][name].reshape(1, -1),
                   float(r64[2][name].abs().max()))


def test_one_step_is_the_single_step_loss_bit_for_bit(simulator):
    b = [t.cuda() for t in cloth()]
    loss, steps = unrolled_loss(simulator, *b, 1)
    pred, target = simulator.predict_acceleration(b[0], b[1], b[2], b[3], b[4][:, 0])
    single = torch.mean((pred - target) ** 2)
    assert torch.equal(loss, single) and torch.equal(steps[0], single)
    g1, g2 = grads_of(simulator, loss), grads_of(simulator, single)
    assert all(torch.equal(g1[n], g2[n]) for n in g1)


def test_the_second_step_reaches_the_first_through_the_edge_features(simulator):
    """hist carries no gradient and the positions enter the network through the edge features alone: with the prediction detached in
    front of the transition ("cut") the second step's loss stops at the second network pass.  The float64 loop with and without the cut
    differ by the path's contribution.  Every weight's gradient from the kernels is within its bar of the uncut one; where the
    contribution is above 10 bars -- an order of magnitude over the largest rounding error the bar admits -- it is therefore at least 9
    bars away from the cut one.  That must be the case for the edge encoder's first weight, the one that multiplies the edge features
    themselves.  (Both figures come from the two float64 loops and the float32 one, none from the kernels.)"""
    b = [t.cuda() for t in cloth()]
    two, one = loops(simulator, b, 2), loops(simulator, b, 1)
    seen = []
    for name, q, kind in kinds(simulator):
        if kind != "dW":
            continue
        full, cut, got, first = two["r64"][2][name].double(), two["cut"][2][name].double(), two["got"][2][name].double(), one["got"][2][name].double()
        scale = float(full.abs().max())
        path = float((full - cut).abs().max()) / scale
        e32 = float((two["r32"][2][name].double() - full).abs().max()) / scale
        bar = max(K * e32, FLOOR)
        err_full, err_cut = float((got - full).abs().max()) / scale, float((got - cut).abs().max()) / scale
        print(f"train_sim path | {name}: path {path:.3e} bar {bar:.3e} kernels-to-uncut {err_full:.3e} kernels-to-cut {err_cut:.3e}")
        assert err_full <= bar, name
        assert not torch.equal(got, first), name                                      # F = 2 is not F = 1
        if path > 10 * bar:
            assert err_cut >= 9 * bar, name
            seen.append(name)
    assert any(name.endswith("_encoder.edge_fn.0.NN-0.weight") for name in seen), seen


def test_train_step_on_a_collated_batch_is_the_hand_built_block_diagonal_graph(simulator):
    samples = [tuple(t.cuda() for t in cloth(seed=s)) for s in range(3)]
    N = 300
    by_hand = tuple(torch.cat([s[i] for s in samples], 0) for i in (0, 1)) + \
        (torch.cat([samples[0][2], samples[1][2] + N, samples[2][2] + 2 * N], 1),) + \
        tuple(torch.cat([s[i] for s in samples], 0) for i in (3, 4, 5, 6))
    one = collate(samples)
    assert all(torch.equal(a, c) for a, c in zip(one, by_hand)) and one[2].shape == (2, 6300) and int(one[2].max()) == 3 * N - 1
    sims = [copy.deepcopy(simulator).train() for _ in range(2)]
    results = []
    for sim, batch in zip(sims, (one, by_hand)):
        opt = torch.optim.Adam(sim.parameters(), lr=1e-3)
        results.append(train_step(sim, opt, batch, future_sequence_length=3, noise_std=0.0))
    assert torch.equal(results[0][0], results[1][0]) and len(results[0][1]) == 3 and bool(torch.isfinite(results[0][0]))
    moved = 0
    for (name, p), q, p0 in zip(sims[0].named_parameters(), sims[1].parameters(), simulator.parameters()):
        assert torch.equal(p, q), name
        moved += int(not torch.equal(p, p0))
    assert moved > 0
    # the normalisers accumulated once per prediction, as in the reference
    assert float(sims[0]._output_normalizer._num_accumulations) == float(simulator._output_normalizer._num_accumulations) + 3
