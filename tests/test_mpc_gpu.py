"""The planning kernels (csplat_plan_integrate, csplat_plan_cost, csplat_plan_select, csplat_plan_refit_sample) on the GPU against the
float64 restatement of tests/mpc_ref.py, the batched candidate rollout of meshnet.mpc against meshnet.rollout.rollout of each candidate
alone, and MPC end to end.

Exact outputs.  v, pos, hist and preds of csplat_plan_integrate are one float32 add per element (or a copy): compared with torch.equal
against the float32 restatement.  order of csplat_plan_select equals torch.sort(cost.cpu(), stable=True) exactly -- the order is total, no
tie needs excluding -- and best is compared bit for bit.  Row 0 of the refitted candidates equals the clamped mean exactly.  The cost
contract is checked bit for bit: permuting the candidates permutes the costs, a candidate alone costs what it costs inside a batch of 65,
and csplat_plan_cost on the stored final positions equals the cost accumulated under the default step weights.

Values (cost, mu, sigma, actions) by the rule of tests/test_train_kernels_gpu.py (its check() and TABLE are used): within 8 x the float32
restatement's own error against float64, floor 1e-6, relative to max(max |ref|, unit).  Units: 1 for a cost (positions and goal are
N(0, 1): a mean squared distance is of size 2; a candidate whose weighted nodes all have weight 0 costs exactly 0), 0.01 for mu, sigma and
actions (the size of an action).

Shapes (tests/mpc_ref.py, checked against the source's launch constants by tests/test_mpc_cpu.py): a candidate's 3N elements are walked
256 at a time by one workgroup -- 3N = 3, 255, 258, 765 .. 771, 3000; B = 1, 2, 65 workgroups; H = 1 (nothing shifts), 2, 3.  select: B
around the wave, the workgroup and the 1024-key LDS tile.  refit: 3T = 3, 18, 99 threads; K = 1, 10, B elites in batches of 8.

End to end: B = 5 candidates of a 300-node, 2100-edge graph, 5 steps, against rollout(graph=False) of each candidate alone.  The two differ
only by the batch-wide absmax that scales the 16-bit pieces of the fused inference kernels (a batch's largest |feature| is at least each
candidate's own); the bar is the project's 1e-5 between two arithmetic paths of one rollout (tests/test_knn_gnn_gpu.py).

What an MI355X showed when this file was written.  End to end, the largest rel_err over the 5 candidates: predictions 1.40e-06 and final
positions 5.64e-07 without normalisers, 6.31e-07 and 1.23e-07 with them (bar 1e-5).  refine: best cost 2.97e-07 after iteration 0,
8.58e-08 after three iterations.  The table (largest e32 / bar / kernel error of a group; smallest bar / error):
  mpc cost           1.74e-07 / 1.39e-06 / 1.56e-07   6.4        mpc integrate   1.85e-07 / 1.48e-06 / 1.41e-07   7.9
  mpc refit_sample   4.19e-07 / 3.35e-06 / 4.19e-07   5.8
The kernels' errors are those of the float32 restatement; every exact comparison was equal.  Wall time of the 39 tests: 4 to 5 s.
"""
import pytest

import util
import mpc_ref as R
from test_train_kernels_gpu import FLOOR, K, TABLE, check  # noqa: F401  (the project's rule for a bar, and the table of its comparisons)

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
F64, F32 = torch.float64, torch.float32


@pytest.fixture(scope="module", autouse=True)
def _threads_and_table():
    """torch gets at most 16 host threads for the restatement; afterwards the table of this module's bars (pytest -rP shows it)"""
    old = torch.get_num_threads()
    torch.set_num_threads(min(16, old))
    yield
    torch.set_num_threads(old)
    print("\ngroup | comparisons | largest e32 | largest bar | largest kernel error | smallest bar / error")
    for g in sorted(k for k in TABLE if k.startswith("mpc")):
        n, e32, bar, err, margin = TABLE[g]
        print(f"{g} | {n} | {e32:.2e} | {bar:.2e} | {err:.2e} | {margin:.1f}")


def _lib():
    from csplat import native
    return native


def cu(t):
    return None if t is None else t.detach().cuda().contiguous()


def k_integrate(B, N, H, T, k, v, actions, grasped, pos, hist, preds=None, goal=None, node_w=None, step_w=None, cost=None):
    """csplat_plan_integrate on GPU tensors (v, pos, hist, preds, cost are updated in place)"""
    n = _lib()
    n.check(n.lib.csplat_plan_integrate(n.stream_handle(v.device), B, N, H, T, k, n.ptr(v), n.ptr(actions), grasped, n.ptr(pos), n.ptr(hist),
                                        n.ptr(preds), n.ptr(goal), n.ptr(node_w), n.ptr(step_w), n.ptr(cost)), "csplat_plan_integrate")


def k_cost(pos_b, goal, node_w=None, w=1.0, out=None):
    n = _lib()
    B, N = int(pos_b.shape[0]), int(pos_b.shape[1])
    cost = torch.full((B,), 7.0, device=pos_b.device) if out is None else out
    n.check(n.lib.csplat_plan_cost(n.stream_handle(pos_b.device), B, N, n.ptr(pos_b), n.ptr(goal), n.ptr(node_w), w, 0 if out is None else 1,
                                   n.ptr(cost)), "csplat_plan_cost")
    return cost


def run_chain(c, grasped, with_preds, goal_mode):
    """T consecutive steps of one case on the GPU and in the restatement (float64 and float32), each step fed the float32 state the kernel
    left; every exact output is compared at every step -> (kernel cost, r64 cost, r32 cost) or None without a goal"""
    B, N, H, T = c["B"], c["N"], c["H"], c["T"]
    goal = None if goal_mode == "none" else c["goal"]
    node_w, step_w = (c["node_w"], c["step_w"]) if goal_mode == "weights" else (None, None)
    pos, hist = c["pos"].clone(), c["hist"].clone()
    preds = torch.full((T, B * N, 3), -5.0) if with_preds else None
    g_pos, g_hist, g_preds = cu(pos), cu(hist), cu(preds)
    g_act, g_goal, g_nw, g_sw = cu(c["actions"]), cu(goal), cu(node_w), cu(step_w)
    g_cost = None if goal is None else torch.zeros(B, device="cuda")
    c64 = None if goal is None else torch.zeros(B, dtype=F64)
    c32 = None if goal is None else torch.zeros(B, dtype=F32)
    for k in range(T):
        g_v = cu(c["v"][k])
        k_integrate(B, N, H, T, k, g_v, g_act, grasped, g_pos, g_hist, g_preds, g_goal, g_nw, g_sw, g_cost)
        r32 = R.integrate(B, N, k, c["v"][k], c["actions"], grasped, pos, hist, preds, goal, node_w, step_w, c32, dtype=F32)
        r64 = R.integrate(B, N, k, c["v"][k], c["actions"], grasped, pos, hist, preds, goal, node_w, step_w, c64, dtype=F64)
        assert torch.equal(g_v.cpu(), r32["v"]) and torch.equal(g_pos.cpu(), r32["pos"]) and torch.equal(g_hist.cpu(), r32["hist"]), (k, B, N, H)
        if with_preds:
            assert torch.equal(g_preds.cpu(), r32["preds"]), (k, B, N, H)
        if 0 <= grasped < N:
            assert torch.equal(g_v.view(B, N, 3)[:, grasped].cpu(), c["actions"][:, k])
        pos, hist, preds, c32, c64 = r32["pos"], r32["hist"], r32["preds"], r32["cost"], r64["cost"]
    return None if goal is None else (g_cost.cpu(), c64, c32)


@pytest.mark.parametrize("B,N,H", R.INTEGRATE_SIZES)
def test_integrate_exact_outputs_and_cost_at_every_launch_edge(B, N, H):
    c = R.integrate_case(B, N, H)
    group = "mpc integrate"
    got = run_chain(c, 0, True, "weights")                    # grasped 0, predictions stored, node weights with zeros, step weights
    check(group, f"cost weights B{B} N{N} H{H}", *got, 1.0)
    got = run_chain(c, N - 1, False, "default")               # grasped N-1, no predictions, the default cost (the final state)
    check(group, f"cost default B{B} N{N} H{H}", *got, 1.0)
    assert run_chain(c, -1, True, "none") is None             # grasped -1 pins nothing, no goal: no cost word is touched
    assert run_chain(c, N, False, "none") is None             # N is outside too


def test_integrate_default_cost_is_the_mean_squared_distance_of_the_final_state():
    B, N, H = 2, 300, 2
    c = R.integrate_case(B, N, H, seed=3)
    kernel, _r64, _r32 = run_chain(c, 5, False, "default")
    pos = c["pos"].clone()
    for k in range(c["T"]):          # the float32 positions the kernel holds after its last step
        v = c["v"][k].clone().view(B, N, 3)
        v[:, 5] = c["actions"][:, k]
        pos = pos + v.view(-1, 3)
    want = torch.stack([(pos.double().view(B, N, 3)[b] - c["goal"].double()).pow(2).mean() for b in range(B)])          # planning.py:425
    assert util.rel_err(kernel.numpy(), want.numpy()) < 1e-6          # (3N = 900 float32 terms: a few 1e-7 at most)


def _final_state_costs(c, rows=None):
    """the T-step chain on the GPU under the default step weights for the candidates `rows` (default: all) -> (cost [B'], final pos [B',N,3])"""
    B, N, H, T = c["B"], c["N"], c["H"], c["T"]
    rows = torch.arange(B) if rows is None else rows
    Bp = len(rows)
    take = lambda t, lead=0: t.reshape(*t.shape[:lead], B, N, 3)[(slice(None),) * lead + (rows,)].reshape(*t.shape[:lead], Bp * N, 3)  # noqa: E731
    g_pos, g_hist, g_act, g_goal = cu(take(c["pos"])), cu(take(c["hist"], 1)), cu(c["actions"][rows]), cu(c["goal"])
    g_cost = torch.zeros(Bp, device="cuda")
    for k in range(T):
        k_integrate(Bp, N, H, T, k, cu(take(c["v"][k])), g_act, 3, g_pos, g_hist, None, g_goal, None, None, g_cost)
    return g_cost, g_pos.view(Bp, N, 3)


@pytest.mark.parametrize("N", [257, 1000])
def test_a_candidates_cost_depends_on_its_own_positions_only_bit_for_bit(N):
    B = 65
    c = R.integrate_case(B, N, 2, seed=1)
    cost, pos = _final_state_costs(c)
    assert bool(torch.isfinite(cost).all()) and len(set(cost.tolist())) == B
    perm = torch.randperm(B, generator=torch.Generator().manual_seed(2))
    cost_p, pos_p = _final_state_costs(c, perm)
    assert torch.equal(pos_p.cpu(), pos.cpu()[perm]) and torch.equal(cost_p.cpu(), cost.cpu()[perm])          # permuted candidates, permuted costs
    for b in (0, 37, 64):
        alone, _ = _final_state_costs(c, torch.tensor([b]))
        assert torch.equal(alone.cpu(), cost.cpu()[b:b + 1])                                                  # B = 1 against inside B = 65
    # csplat_plan_cost on the stored final positions: the same bits; accumulate adds w * the same term
    after = k_cost(pos, cu(c["goal"]))
    assert torch.equal(after, cost)
    acc = k_cost(pos, cu(c["goal"]), w=0.5, out=torch.ones(B, device="cuda"))
    assert torch.equal(acc, 1.0 + 0.5 * cost)
    nw = cu(c["node_w"])
    r64, r32 = R.cost(pos.cpu(), c["goal"], c["node_w"], F64), R.cost(pos.cpu(), c["goal"], c["node_w"], F32)
    check("mpc cost", f"node weights N{N}", k_cost(pos, cu(c["goal"]), nw), r64, r32, 1.0)


@pytest.mark.parametrize("B", R.SELECT_B)
def test_select_is_the_stable_sort_truncated(B):
    from meshnet import mpc
    cost = R.select_case(B)
    val, idx = torch.sort(cost, stable=True)
    for Kk in R.select_ks(B):
        order, best = mpc.select_candidates(cost.cuda(), Kk)
        assert order.dtype == torch.int32 and order.shape == (Kk,) and best.shape == (Kk,)
        assert torch.equal(order.cpu().long(), idx[:Kk]), (B, Kk)
        assert torch.equal(best.cpu().view(torch.int32), val[:Kk].view(torch.int32)), (B, Kk)          # the costs as stored: NaN, -0.0 included
        ro, rb = R.select(cost, Kk)
        assert torch.equal(ro, idx[:Kk]) and torch.equal(rb.view(torch.int32), val[:Kk].view(torch.int32))
    # all equal, all NaN: by ascending index
    for fill in (1.5, float("nan")):
        order, _ = mpc.select_candidates(torch.full((B,), fill).cuda(), B)
        assert order.tolist() == list(range(B))


@pytest.mark.parametrize("T,B", R.REFIT_SIZES)
def test_refit_sample_against_the_restatement(T, B):
    from meshnet import mpc
    group = "mpc refit_sample"
    for Kk in sorted({1, min(10, B), B}):
        c = R.refit_case(T, B, Kk)
        assert (B - 1) in c["order"].tolist() and (Kk < 2 or 0 in c["order"].tolist())          # rows the same call overwrites are elites
        for alpha in R.REFIT_ALPHAS:
            for a_max in (0.0, 0.04):
                a, mu, sg = cu(c["actions"]), cu(c["mu"]), cu(c["sigma"])
                mpc.refit_sample(a, cu(c["order"]), mu, sg, cu(c["noise"]), alpha, 1e-4 if Kk > 1 else 0.015, a_max)
                smin = 1e-4 if Kk > 1 else 0.015
                r64 = R.refit_sample(c["actions"], c["order"], c["mu"], c["sigma"], c["noise"], alpha, smin, a_max, F64)
                r32 = R.refit_sample(c["actions"], c["order"], c["mu"], c["sigma"], c["noise"], alpha, smin, a_max, F32)
                tag = f"T{T} B{B} K{Kk} alpha{alpha} a_max{a_max}"
                check(group, "mu " + tag, mu, r64[1], r32[1], 0.01)
                check(group, "sigma " + tag, sg, r64[2], r32[2], 0.01)
                check(group, "actions " + tag, a, r64[0], r32[0], 0.01)
                clamped = torch.clamp(mu, -a_max, a_max) if a_max > 0 else mu
                assert torch.equal(a[0], clamped), tag                                           # the incumbent, exactly
                if a_max > 0:
                    assert float(a.abs().max()) <= a_max
                    assert B * T < 100 or bool((a.abs() == a_max).any())                         # the clamp is in play
                if alpha == 1.0:
                    assert torch.equal(mu.cpu(), c["mu"])                                        # an identity refit
                if Kk == 1 and alpha == 0.0:
                    assert torch.equal(sg.cpu(), torch.full((T, 3), 0.015))                      # one elite: s = 0, sigma_min applies
    # K = 0: no refit, sampling only
    c = R.refit_case(T, B, 1)
    a, mu, sg = cu(c["actions"]), cu(c["mu"]), cu(c["sigma"])
    mpc.refit_sample(a, torch.zeros(0, dtype=torch.int32, device="cuda"), mu, sg, cu(c["noise"]), 0.0, 1e-4, 0.0)
    r32 = R.refit_sample(c["actions"], c["order"][:0], c["mu"], c["sigma"], c["noise"], 0.0, 1e-4, 0.0, F32)
    assert torch.equal(mu.cpu(), c["mu"]) and torch.equal(sg.cpu(), c["sigma"]) and torch.equal(a.cpu(), r32[0])


# ------------------------------------------------------------------------------------------------------------------ end to end
def _world(normalize, B=5, T=6, seed=41):
    from meshnet.cloth_network import ClothMeshSimulator
    dev = "cuda"
    g = torch.Generator().manual_seed(seed)
    N, E = 300, 2100
    pos = torch.randn(N, 3, generator=g).to(dev)
    ei = torch.stack([torch.randint(0, N, (E,), generator=g), torch.randint(0, N, (E,), generator=g)]).to(dev)
    torch.manual_seed(9)
    sim = ClothMeshSimulator(3, 8, 4, 128, 3, 2, 128, 2, 2, normalize=normalize, device=dev)
    if normalize:            # statistics as a few training batches would leave them
        sim.train()
        with torch.no_grad():
            for _ in range(3):
                sim._node_normalizer(torch.randn(N, 8, generator=g).to(dev) * 0.3 + 0.1, True)
                sim._output_normalizer(torch.randn(N, 3, generator=g).to(dev) * 0.02, True)
    sim.eval()
    hist = (torch.randn(2, N, 3, generator=g) * 0.01).to(dev)
    ntype = torch.randint(0, 2, (N, 1), generator=g).to(dev)
    actions = (torch.randn(B, T, 3, generator=g) * 0.01).to(dev)
    return dict(sim=sim, N=N, E=E, B=B, T=T, pos=pos, ei=ei, hist=hist, ntype=ntype, actions=actions)


@pytest.mark.parametrize("normalize", [False, True])
def test_batched_candidates_equal_the_rollout_of_each_candidate_alone(normalize):
    from csplat import native
    from meshnet import mpc, rollout as ro
    w = _world(normalize)
    steps, grasped = 5, 11
    before = sum(native.FALLBACK_COUNTS.values())
    r = mpc.rollout_candidates(w["sim"], w["pos"], w["hist"], w["ntype"], w["ei"], w["actions"], grasped, steps, return_trajectories=True)
    assert sum(native.FALLBACK_COUNTS.values()) == before
    assert r.predictions.shape == (steps, w["B"], w["N"], 3) and r.final_positions.shape == (w["B"], w["N"], 3) and r.costs is None
    assert bool(torch.isfinite(r.predictions).all()) and bool(torch.isfinite(r.final_positions).all())
    worst_pred = worst_pos = 0.0
    for b in range(w["B"]):
        pred, pos_end = ro.rollout(w["sim"], w["pos"], w["hist"], w["ntype"], w["ei"], w["actions"][b], grasped, steps, graph=False)
        worst_pred = max(worst_pred, util.rel_err(r.predictions[:, b].cpu().numpy(), pred.cpu().numpy()))
        worst_pos = max(worst_pos, util.rel_err(r.final_positions[b].cpu().numpy(), pos_end.cpu().numpy()))
        assert torch.equal(r.predictions[:, b, grasped], w["actions"][b, :steps])          # the grasped rows are the actions, exactly
    print(f"mpc end to end normalize={normalize}: largest rel_err predictions {worst_pred:.3e} final positions {worst_pos:.3e}")
    assert worst_pred < 1e-5 and worst_pos < 1e-5


def test_mpc_picks_the_candidate_whose_rollout_is_the_goal_and_refine_does_not_lose_ground():
    from csplat import native
    from meshnet import mpc
    w = _world(False, B=8)
    m = mpc.MPC(w["sim"], A=8, H=4, input_sequence_length=2)
    before = sum(native.FALLBACK_COUNTS.values())
    r = m.model_rollout(w["pos"], w["hist"], w["ntype"], w["ei"], w["actions"], 11)
    assert r.costs is None and r.actions.shape == (8, 4, 3)
    goal = r.final_positions[3].clone()
    idx, best_actions, cost = m.compute_cost(r, goal)
    assert idx.is_cuda and best_actions.is_cuda and cost.is_cuda                          # device tensors: the caller decides when to read
    costs = mpc.candidate_costs(r.final_positions, goal)
    assert int(idx) == 3 and float(cost) == 0.0 and torch.equal(best_actions, w["actions"][3, :4])
    assert bool((costs[torch.arange(8, device="cuda") != 3] > 0).all())
    # the fused path carries the same costs, bit for bit
    rc = m.model_rollout(w["pos"], w["hist"], w["ntype"], w["ei"], w["actions"], 11, goal=goal)
    assert torch.equal(rc.final_positions, r.final_positions) and torch.equal(rc.costs, costs)
    # CEM: three iterations under strict dispatch, no fallback; the best cost does not rise; mu stays inside the clamp
    a_max, mu0, sg0 = 0.03, torch.zeros(4, 3, device="cuda"), torch.full((4, 3), 0.01, device="cuda")
    g = lambda: torch.Generator(device="cuda").manual_seed(5)  # noqa: E731
    first = m.refine(w["pos"], w["hist"], w["ntype"], w["ei"], 11, goal, mu0, sg0, iterations=1, elites=3, a_max=a_max, generator=g())
    best_actions, best_cost, mu, sigma = m.refine(w["pos"], w["hist"], w["ntype"], w["ei"], 11, goal, mu0, sg0, iterations=3, elites=3,
                                                  a_max=a_max, generator=g())
    assert sum(native.FALLBACK_COUNTS.values()) == before
    assert best_actions.shape == (4, 3) and bool(torch.isfinite(best_cost)) and bool(torch.isfinite(mu).all())
    print(f"mpc refine: best cost after iteration 0 {float(first[1]):.6e}, after 3 iterations {float(best_cost):.6e}")
    assert float(best_cost) <= float(first[1]) * (1.0 + 1e-5)
    assert float(mu.abs().max()) <= a_max and float(best_actions.abs().max()) <= a_max and float(sigma.min()) >= 1e-4
