"""Planning without a GPU: the library's surface (header, exports, bindings, ABI number, argument checks before any launch), the Python
surface of meshnet.mpc on CPU tensors (its composed branch) against a loop of meshnet.rollout.rollout per candidate and against closed
forms, and self-checks of the restatement tests/mpc_ref.py that tests/test_mpc_gpu.py holds the kernels to."""
import os
import re

import numpy as np
import pytest
import torch

import util
import mpc_ref as R

F64, F32 = torch.float64, torch.float32
NAN, INF = float("nan"), float("inf")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------------------------ the library's surface
def test_header_exports_and_bindings():
    from csplat import native
    header = open(os.path.join(ROOT, "include", "csplat.h")).read()
    for name, n_args in (("csplat_plan_integrate", 16), ("csplat_plan_cost", 9), ("csplat_plan_select", 6), ("csplat_plan_refit_sample", 12)):
        assert re.search(r"\bint " + name + r"\s*\(", header), name
        assert name in native.EXPORTS and hasattr(native.lib, name) and len(native.EXPORTS[name][1]) == n_args
        decl = header[header.index("int " + name + "("):]
        decl = re.sub(r"/\*.*?\*/", "", decl[:decl.index(";")], flags=re.S)
        assert decl.count(",") + 1 == n_args, (name, decl)
    block = header[header.index("/* Planning"):header.index("int csplat_plan_integrate(")]
    assert "Added exports: CSPLAT_ABI_VERSION is unchanged" in block
    for word in ("b * N + n", "NO atomics", "order fixed by N alone", "bit-equal", "stable=True", "+inf before every NaN",
                 "r = 0 .. K-1", "incumbent", "read before any row is overwritten"):
        assert word.lower() in block.lower(), word
    assert native.ABI_VERSION == 9 and native.lib.csplat_abi_version() == 9


def test_the_library_refuses_bad_arguments_before_any_launch():
    from csplat import native
    L = native.lib
    integ = lambda B=2, N=4, H=2, T=3, k=0, v=16, act=16, g=1, pos=16, hist=16, preds=16, goal=16, nw=16, sw=16, cost=16: \
        L.csplat_plan_integrate(None, B, N, H, T, k, v, act, g, pos, hist, preds, goal, nw, sw, cost)  # noqa: E731
    for kw in (dict(B=-1), dict(N=-1), dict(B=65536, N=8192), dict(H=0), dict(T=0), dict(k=-1), dict(k=3), dict(v=None), dict(act=None),
               dict(pos=None), dict(hist=None), dict(cost=None), dict(v=18), dict(preds=17), dict(goal=18), dict(nw=2), dict(sw=1)):
        assert integ(**kw) == 2, kw
        assert b"csplat_plan_integrate" in L.csplat_last_error()
    assert integ(B=0) == 0 and integ(N=0) == 0          # nothing to do: no launch, no error
    cost = lambda B=2, N=4, pos=16, goal=16, nw=16, w=1.0, acc=0, c=16: L.csplat_plan_cost(None, B, N, pos, goal, nw, w, acc, c)  # noqa: E731
    for kw in (dict(B=-1), dict(N=-1), dict(B=65536, N=8192), dict(pos=None), dict(goal=None), dict(c=None), dict(w=NAN), dict(nw=18)):
        assert cost(**kw) == 2, kw
        assert b"csplat_plan_cost" in L.csplat_last_error()
    assert cost(B=0) == 0 and cost(N=0) == 0
    sel = lambda B=4, K=2, c=16, o=16, b=16: L.csplat_plan_select(None, B, K, c, o, b)  # noqa: E731
    for kw in (dict(B=-1), dict(B=65537), dict(K=5), dict(K=-1), dict(c=None), dict(o=None), dict(b=None), dict(c=18)):
        assert sel(**kw) == 2, kw
        assert b"csplat_plan_select" in L.csplat_last_error()
    assert sel(B=0, K=0) == 0 and sel(K=0) == 0
    refit = lambda B=4, T=3, K=2, a=16, o=16, mu=16, sg=16, nz=16, alpha=0.1, smin=1e-4, amax=0.0: \
        L.csplat_plan_refit_sample(None, B, T, K, a, o, mu, sg, nz, alpha, smin, amax)  # noqa: E731
    for kw in (dict(B=-1), dict(T=-1), dict(K=5), dict(K=-1), dict(a=None), dict(o=None), dict(mu=None), dict(sg=None), dict(nz=None),
               dict(alpha=-0.1), dict(alpha=1.5), dict(alpha=NAN), dict(smin=-1.0), dict(smin=NAN), dict(amax=NAN), dict(mu=18)):
        assert refit(**kw) == 2, kw
        assert b"csplat_plan_refit_sample" in L.csplat_last_error()
    assert refit(B=0, K=0) == 0 and refit(T=0) == 0


def test_the_size_tables_cross_the_launch_constants_of_the_source():
    src = open(os.path.join(ROOT, "cloth-splatting_amd", "csrc", "csplat_plan.hip")).read()
    m = re.search(r"constexpr int PL_THREADS = (\d+), PL_SEL_TILE = (\d+), PL_BATCH = (\d+);", src)
    assert m and tuple(int(x) for x in m.groups()) == (R.PL_THREADS, R.PL_SEL_TILE, R.PL_BATCH) == (256, 1024, 8)
    device = open(os.path.join(ROOT, "cloth-splatting_amd", "csrc", "csplat_device.h")).read()
    assert '#include "csplat_device.h"' in src
    assert "atomic" not in re.sub(r"//.*", "", src + device).lower()          # no atomics anywhere in the file, nor in the helpers it calls
    Bs, Ns, Hs = ({s[i] for s in R.INTEGRATE_SIZES} for i in range(3))
    assert {1, 2, 65} <= Bs and {1, 255, 256, 257, 1000} <= Ns and Hs == {1, 2, 3}
    # each value of one axis with the extremes of the two others
    for B in (1, 2, 65):
        assert any(s[0] == B and s[1] in (1, 1000) for s in R.INTEGRATE_SIZES) and any(s[0] == B and s[2] in (1, 3) for s in R.INTEGRATE_SIZES)
    for N in (1, 255, 256, 257, 1000):
        assert any(s[1] == N and s[0] in (1, 65) for s in R.INTEGRATE_SIZES) and any(s[1] == N and s[2] in (1, 3) for s in R.INTEGRATE_SIZES)
    for H in (1, 2, 3):
        assert any(s[2] == H and s[0] in (1, 65) for s in R.INTEGRATE_SIZES) and any(s[2] == H and s[1] in (1, 1000) for s in R.INTEGRATE_SIZES)
    n3 = sorted(3 * n for n in Ns)
    assert min(n3) < 64 and any(x == R.PL_THREADS - 1 for x in n3) and any(R.PL_THREADS < x <= R.PL_THREADS + 2 for x in n3) and \
        max(n3) > 8 * R.PL_THREADS                                    # one partial wave, just below / above one round, many rounds
    assert max(Bs) > 64
    assert R.SELECT_B == [1, 2, 63, 64, 65, 255, 256, 257, 1000, 4099]
    assert any(b > R.PL_SEL_TILE and b % R.PL_SEL_TILE % 4 for b in R.SELECT_B) and any(R.PL_THREADS < b < R.PL_SEL_TILE for b in R.SELECT_B)
    assert R.select_ks(1) == [1] and R.select_ks(4099) == [1, 10, 4099] and R.select_ks(2) == [1, 2]
    Ts, Bs2 = {s[0] for s in R.REFIT_SIZES}, {s[1] for s in R.REFIT_SIZES}
    assert Ts == {1, 6, 33} and Bs2 == {2, 100, 257} and R.REFIT_ALPHAS == [0.0, 0.1, 1.0]
    assert 3 * 33 < R.PL_THREADS < 257 * 3 * 1 and 257 > R.PL_BATCH and 257 % R.PL_BATCH and 10 % R.PL_BATCH          # a ragged elite batch
    assert 257 * 33 * 3 > 64 * R.PL_THREADS


# ------------------------------------------------------------------------------------------------------------------ the restatement
def test_ref_select_is_the_lexicographic_order_of_value_then_index():
    c = torch.tensor([1.0, NAN, -0.0, INF, 0.0, -INF, 1.0, NAN, -1.0, 0.0, INF, 1.0], dtype=F32)
    order, best = R.select(c, len(c))
    x = c.numpy().astype(np.float64)
    isnan = np.isnan(x)
    want = np.lexsort((np.arange(len(x)), np.where(isnan, 0.0, x) + 0.0, isnan))          # NaN last, then the value (-0 == 0), then the index
    assert order.tolist() == want.tolist() == [5, 8, 2, 4, 9, 0, 6, 11, 3, 10, 1, 7]
    assert torch.equal(best.isnan(), torch.tensor([False] * 10 + [True] * 2)) and best[:10].tolist() == x[want[:10]].tolist()
    assert R.select(c, 3)[0].tolist() == [5, 8, 2]
    for B in R.SELECT_B:
        c = R.select_case(B)
        x = c.numpy().astype(np.float64)
        want = np.lexsort((np.arange(B), np.where(np.isnan(x), 0.0, x) + 0.0, np.isnan(x)))
        assert R.select(c, B)[0].tolist() == want.tolist()
        if B >= 63:
            assert bool(c.isnan().any()) and bool((c == INF).any()) and bool((c == -INF).any()) and bool((c == 0).sum() >= 2)
            assert bool(torch.signbit(c[c == 0]).any()) and not bool(torch.signbit(c[c == 0]).all()) and len(set(x[np.isfinite(x)])) <= 8


def test_ref_refit_sample_known_answers():
    T, B = 2, 4
    a = torch.arange(B * T * 3, dtype=F64).reshape(B, T, 3)
    mu, sigma, noise = torch.ones(T, 3, dtype=F64), torch.full((T, 3), 0.5, dtype=F64), torch.ones(B, T, 3, dtype=F64)
    # K = 1: the deviation of one elite is 0 -- sigma_min applies at alpha = 0
    new, m, s = R.refit_sample(a, torch.tensor([2]), mu, sigma, noise, 0.0, 0.25, 0.0)
    assert torch.equal(m, a[2]) and torch.equal(s, torch.full((T, 3), 0.25, dtype=F64))
    assert torch.equal(new[0], a[2]) and torch.equal(new[1:], (a[2] + 0.25)[None].expand(3, T, 3))
    # alpha = 1: an identity refit; the clamp; row 0 is the clamped mean
    new, m, s = R.refit_sample(a, torch.tensor([3, 0]), mu, sigma, 4.0 * noise, 1.0, 1e-4, 2.0)
    assert torch.equal(m, mu) and torch.equal(s, sigma) and torch.equal(new[0], mu) and torch.equal(new[1:], torch.full((3, T, 3), 2.0, dtype=F64))
    # two elites: mean and population deviation; smoothing
    new, m, s = R.refit_sample(a, torch.tensor([3, 1]), mu, sigma, noise, 0.5, 1e-4, 0.0)
    assert torch.allclose(m, 0.5 * mu + 0.5 * (a[3] + a[1]) / 2, atol=1e-15) and torch.allclose(s, 0.5 * sigma + 0.5 * 6.0, atol=1e-15)
    # K = 0: no refit
    new, m, s = R.refit_sample(a, torch.zeros(0, dtype=torch.int64), mu, sigma, noise, 0.0, 1e-4, 0.0)
    assert torch.equal(m, mu) and torch.equal(s, sigma) and torch.equal(new[1], mu + sigma)
    for T_, B_ in R.REFIT_SIZES:
        for K in sorted({1, min(10, B_), B_}):
            o = R.refit_case(T_, B_, K)["order"].tolist()
            assert len(o) == K and len(set(o)) == K and B_ - 1 in o and (K < 2 or 0 in o)


def test_ref_cost_and_integrate_known_answers():
    g = torch.Generator().manual_seed(0)
    B, N, H, T = 3, 5, 2, 3
    pos, goal = torch.randn(B, N, 3, generator=g, dtype=F64), torch.randn(N, 3, generator=g, dtype=F64)
    want = torch.stack([(pos[b] - goal).pow(2).mean() for b in range(B)])          # planning.py:425 per candidate
    assert torch.allclose(R.cost(pos, goal), want, atol=1e-15)
    w = torch.tensor([0.0, 1.0, 2.0, 0.0, 0.5], dtype=F64)
    assert torch.allclose(R.cost(pos, goal, w), ((pos - goal) ** 2 * w[None, :, None]).sum((1, 2)) / 15, atol=1e-15)
    c = R.integrate_case(B, N, H)
    out = R.integrate(B, N, 1, c["v"][1], c["actions"], 4, c["pos"], c["hist"], preds=torch.zeros(T, B * N, 3), goal=c["goal"],
                      cost_in=torch.ones(B))
    v = c["v"][1].double().reshape(B, N, 3).clone()
    v[:, 4] = c["actions"][:, 1].double()
    assert torch.equal(out["v"], v.reshape(-1, 3)) and torch.equal(out["pos"], c["pos"].double() + v.reshape(-1, 3))
    assert torch.equal(out["hist"][0], c["hist"][1].double()) and torch.equal(out["hist"][1], out["v"])
    assert torch.equal(out["preds"][1], out["v"]) and not out["preds"][[0, 2]].any()
    assert torch.equal(out["cost"], torch.ones(B, dtype=F64))                      # default step weights: only the last step adds
    last = R.integrate(B, N, 2, c["v"][2], c["actions"], -1, c["pos"], c["hist"], goal=c["goal"], cost_in=torch.zeros(B))
    assert torch.equal(last["v"], c["v"][2].double())                              # -1 pins nothing
    assert torch.allclose(last["cost"], R.cost(last["pos"].reshape(B, N, 3), c["goal"]), atol=0)
    sw = R.integrate(B, N, 0, c["v"][0], c["actions"], 0, c["pos"], c["hist"], goal=c["goal"], node_w=c["node_w"], step_w=c["step_w"],
                     cost_in=torch.zeros(B))
    assert torch.allclose(sw["cost"], 0.25 * R.cost(sw["pos"].reshape(B, N, 3), c["goal"], c["node_w"]), atol=1e-16)
    assert bool((c["node_w"] == 0).any()) and c["step_w"].tolist() == [0.25, 0.0, 1.5]


# ------------------------------------------------------------------------------------------------------------------ the Python surface
def _hand_batch(pos, hist, ntype, ei, B):
    N = pos.shape[0]
    P = torch.cat([pos for _ in range(B)], 0)
    Hh = torch.cat([hist for _ in range(B)], 1)
    nt = torch.cat([ntype.reshape(N, 1) for _ in range(B)], 0)
    E = torch.cat([ei + b * N for b in range(B)], 1)
    batch = torch.cat([torch.full((N,), b, dtype=torch.int64) for b in range(B)])
    return P, Hh, nt, E, batch


@pytest.mark.parametrize("B,E", [(1, 9), (3, 9), (3, 0)])
def test_batch_candidates_is_the_block_diagonal_graph(B, E):
    from meshnet import mpc
    g = torch.Generator().manual_seed(B + E)
    N, H = 5, 2
    pos, hist = torch.randn(N, 3, generator=g), torch.randn(H, N, 3, generator=g)
    ntype, ei = torch.randint(0, 2, (N, 1), generator=g), torch.randint(0, N, (2, E), generator=g)
    b = mpc.batch_candidates(pos, hist, ntype, ei, B)
    P, Hh, nt, EI, batch = _hand_batch(pos, hist, ntype, ei, B)
    assert isinstance(b, mpc.CandidateBatch) and (b.B, b.N) == (B, N)
    assert torch.equal(b.pos, P) and torch.equal(b.hist, Hh) and torch.equal(b.node_type, nt) and torch.equal(b.batch, batch)
    assert b.edge_index.shape == (2, B * E) and b.edge_index.dtype == torch.int64 and torch.equal(b.edge_index, EI) and b.edge_index.is_contiguous()
    assert b.pos.shape == (B * N, 3) and b.hist.shape == (H, B * N, 3) and b.node_type.shape == (B * N, 1)
    with pytest.raises(ValueError):
        mpc.batch_candidates(pos, hist, ntype, ei, 0)
    with pytest.raises(ValueError):
        mpc.batch_candidates(pos, hist[:, :4], ntype, ei, B)


class _HostSimulator:
    """predict_velocity of a ClothMeshSimulator on CPU tensors: the module's own feature assembly and de-normalisation around the message
    passing of oracle/gnn_ref.py on the module's weights (the module's message passing builds its CSR orderings on the device and has
    no CPU path).  meshnet.rollout.rollout and meshnet.mpc.rollout_candidates ask a simulator for nothing but predict_velocity."""

    def __init__(self, sim):
        self.sim = sim
        self.weights = {k: v.detach().numpy() for k, v in sim._encode_process_decode.state_dict().items()}

    def predict_velocity(self, velocities, node_type, edge_index, edge_features):
        from oracle import gnn_ref
        feats = self.sim._encoder_preprocessor(velocities, node_type, velocity_noise=None)
        y = gnn_ref.encode_process_decode(self.weights, feats.numpy(), edge_index.numpy(), edge_features.numpy())
        return velocities[:, -3:] + self.sim._output_normalizer.inverse(torch.from_numpy(y).to(velocities.dtype))


@pytest.fixture(scope="module")
def small_world():
    from meshnet.cloth_network import ClothMeshSimulator
    g = torch.Generator().manual_seed(5)
    N, E, B, T = 20, 90, 3, 6
    torch.manual_seed(3)
    sim = _HostSimulator(ClothMeshSimulator(3, 8, 4, 32, 3, 2, 32, 2, 2, normalize=False, device="cpu").eval())
    w = dict(sim=sim, N=N, B=B, T=T, pos=torch.randn(N, 3, generator=g), hist=0.01 * torch.randn(2, N, 3, generator=g),
             ntype=torch.randint(0, 2, (N, 1), generator=g),
             ei=torch.stack([torch.randint(0, N, (E,), generator=g), torch.randint(0, N, (E,), generator=g)]),
             actions=0.01 * torch.randn(B, T, 3, generator=g), goal=torch.randn(N, 3, generator=g))
    return w


def test_rollout_candidates_on_cpu_tensors_equals_a_loop_of_rollout(small_world):
    from meshnet import mpc, rollout as ro
    w = small_world
    steps, grasped = 4, 7
    r = mpc.rollout_candidates(w["sim"], w["pos"], w["hist"], w["ntype"], w["ei"], w["actions"], grasped, steps, goal=w["goal"],
                               return_trajectories=True)
    assert isinstance(r, mpc.CandidateRollouts) and r._fields[:3] == ("final_positions", "costs", "predictions")
    assert r.final_positions.shape == (w["B"], w["N"], 3) and r.costs.shape == (w["B"],) and r.predictions.shape == (steps, w["B"], w["N"], 3)
    assert r.actions.shape == (w["B"], steps, 3) and torch.equal(r.actions, w["actions"][:, :steps])
    for b in range(w["B"]):
        pred, pos_end = ro.rollout(w["sim"], w["pos"], w["hist"], w["ntype"], w["ei"], w["actions"][b], grasped, steps)
        assert util.rel_err(r.predictions[:, b].numpy(), pred.numpy()) < 1e-5
        assert util.rel_err(r.final_positions[b].numpy(), pos_end.numpy()) < 1e-5
        assert torch.equal(r.predictions[:, b, grasped], w["actions"][b, :steps])          # the grasped rows are the actions, exactly
    # the cost with default weights is (pos - goal).pow(2).mean() of the final state, per candidate
    want = torch.stack([(r.final_positions[b].double() - w["goal"].double()).pow(2).mean() for b in range(w["B"])])
    assert util.rel_err(r.costs.numpy(), want.numpy()) < 1e-6
    # no goal: no costs; no trajectories unless asked for; the inputs are untouched
    pos0 = w["pos"].clone()
    q = mpc.rollout_candidates(w["sim"], w["pos"], w["hist"], w["ntype"], w["ei"], w["actions"], grasped, steps)
    assert q.costs is None and q.predictions is None and torch.equal(q.final_positions, r.final_positions) and torch.equal(w["pos"], pos0)
    # weights: the restatement on the trajectory
    nw, sw = torch.rand(w["N"]), torch.tensor([0.5, 0.0, 2.0, 1.0, 9.0])
    k = mpc.rollout_candidates(w["sim"], w["pos"], w["hist"], w["ntype"], w["ei"], w["actions"], grasped, steps, goal=w["goal"],
                               node_weights=nw, step_weights=sw)
    traj = w["pos"][None, None].double() + r.predictions.double().cumsum(0)
    want = sum(float(sw[s]) * R.cost(traj[s], w["goal"], nw) for s in range(steps))
    assert util.rel_err(k.costs.numpy(), want.numpy()) < 1e-5
    # an int outside [0, N) pins nothing (the kernel's rule)
    free = mpc.rollout_candidates(w["sim"], w["pos"], w["hist"], w["ntype"], w["ei"], w["actions"], -1, 2, return_trajectories=True)
    assert util.rel_err(free.predictions[:, 0].numpy(), free.predictions[:, 1].numpy()) < 1e-6


def test_rollout_candidates_argument_errors(small_world):
    from meshnet import mpc
    w = small_world
    args = (w["sim"], w["pos"], w["hist"], w["ntype"], w["ei"])
    with pytest.raises(ValueError, match="at least nsteps"):
        mpc.rollout_candidates(*args, w["actions"], 3, w["T"] + 1)
    with pytest.raises(ValueError, match=r"\[B,T,3\]"):
        mpc.rollout_candidates(*args, w["actions"][0], 3, 2)
    with pytest.raises(ValueError, match="goal"):
        mpc.rollout_candidates(*args, w["actions"], 3, 2, goal=w["goal"][:5])
    with pytest.raises(NotImplementedError):
        mpc.rollout_candidates(*args, w["actions"], 3, 2, real_world=True)
    # more actions than steps are accepted and only [:, :nsteps] is used
    long_ = torch.cat([w["actions"], torch.full((w["B"], 100, 3), NAN)], 1)
    a = mpc.rollout_candidates(*args, long_, 3, 2)
    b = mpc.rollout_candidates(*args, w["actions"], 3, 2)
    assert torch.equal(a.final_positions, b.final_positions) and a.actions.shape == (w["B"], 2, 3)
    zero = mpc.rollout_candidates(*args, w["actions"], 3, 0, goal=w["goal"], return_trajectories=True)
    assert torch.equal(zero.final_positions, w["pos"][None].expand(w["B"], -1, -1)) and zero.predictions.shape[0] == 0


def test_select_and_compute_cost_return_the_argmin_with_the_lowest_index_on_a_tie(small_world):
    from meshnet import mpc
    order, best = mpc.select_candidates(torch.tensor([3.0, 1.0, NAN, 1.0, -0.0, 0.0]), 4)
    assert order.dtype == torch.int32 and order.tolist() == [4, 5, 1, 3] and best.tolist() == [-0.0, 0.0, 1.0, 1.0]
    w = small_world
    m = mpc.MPC(w["sim"], A=w["B"], H=4, input_sequence_length=2)
    assert (m.A, m.H, m.input_sequence_length) == (3, 4, 2)
    r = m.model_rollout(w["pos"], w["hist"], w["ntype"], w["ei"], w["actions"], 7)
    assert r.costs is None and r.actions.shape == (3, 4, 3)                          # min(H, T) steps
    goal = r.final_positions[1].clone()
    idx, best_actions, cost = m.compute_cost(r, goal)
    assert int(idx) == 1 and float(cost) == 0.0 and torch.equal(best_actions, w["actions"][1, :4])
    # a tie: candidates 0 and 2 share their final state
    tied = mpc.CandidateRollouts(torch.stack([r.final_positions[2], r.final_positions[1], r.final_positions[2]]), None, None, r.actions)
    idx, best_actions, cost = m.compute_cost(tied, r.final_positions[2])
    assert int(idx) == 0 and float(cost) == 0.0 and torch.equal(best_actions, r.actions[0])
    # costs the rollout carried are used as they are
    carried = mpc.CandidateRollouts(r.final_positions, torch.tensor([2.0, 3.0, 1.0]), None, r.actions)
    idx, _a, cost = m.compute_cost(carried, goal)
    assert int(idx) == 2 and float(cost) == 1.0
    with pytest.raises(ValueError, match="A is 3"):
        m.model_rollout(w["pos"], w["hist"], w["ntype"], w["ei"], w["actions"][:2], 7)
    with pytest.raises(ValueError, match="input_sequence_length"):
        m.model_rollout(w["pos"], w["hist"][:1], w["ntype"], w["ei"], w["actions"], 7)


def test_refine_on_cpu_tensors_keeps_the_incumbent_and_the_clamp(small_world):
    from meshnet import mpc
    w = small_world
    m = mpc.MPC(w["sim"], A=8, H=3, input_sequence_length=2)
    mu0, sg0 = torch.zeros(3, 3), torch.full((3, 3), 0.02)
    gen = torch.Generator().manual_seed(11)
    one = m.refine(w["pos"], w["hist"], w["ntype"], w["ei"], 7, w["goal"], mu0, sg0, iterations=1, elites=3, a_max=0.03,
                   generator=torch.Generator().manual_seed(11))
    best_actions, best_cost, mu, sigma = m.refine(w["pos"], w["hist"], w["ntype"], w["ei"], 7, w["goal"], mu0, sg0, iterations=3, elites=3,
                                                  a_max=0.03, generator=gen)
    assert best_actions.shape == (3, 3) and best_cost.shape == () and mu.shape == (3, 3) and sigma.shape == (3, 3)
    assert float(best_actions.abs().max()) <= 0.03 and float(mu.abs().max()) <= 0.03 + 1e-9 and float(sigma.min()) >= 1e-4
    assert torch.equal(mu0, torch.zeros(3, 3)) and torch.equal(one[2], mu0) and torch.equal(one[3], sg0)          # the inputs are not written
    assert torch.isfinite(best_cost) and float(best_cost) <= float(one[1]) * (1 + 1e-5)


def test_shift_drops_the_executed_actions_and_pads_the_tail():
    from meshnet import mpc
    mu = torch.arange(12, dtype=F32).reshape(4, 3)
    sigma = torch.full((4, 3), 0.5)
    m2, s2 = mpc.MPC.shift(mu, sigma, 2, 0.125)
    assert torch.equal(m2, torch.stack([mu[2], mu[3], mu[3], mu[3]])) and torch.equal(s2, torch.tensor([[0.5] * 3] * 2 + [[0.125] * 3] * 2))
    m0, s0 = mpc.MPC.shift(mu, sigma, 0, 0.125)
    assert torch.equal(m0, mu) and torch.equal(s0, sigma) and m0 is not mu
    m9, s9 = mpc.MPC.shift(mu, sigma, 9, 0.125)
    assert torch.equal(m9, mu[3:].expand(4, 3)) and torch.equal(s9, torch.full((4, 3), 0.125))
