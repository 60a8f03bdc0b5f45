"""tests/sim_rollout_ref.py is what tests/test_sim_rollout_kernels_gpu.py holds the simulator and rollout-step kernels to, so it is
checked here first, without a GPU: against F.linear and autograd over the composed two-layer MLP, against train.regularization(fused=False)
in float64, against rollout.refine_edge_lengths' CPU branch (torch.optim.Adam on autograd's gradient), and against the runs of the
reference kept in tests/golden/simulator.npz and refine.npz.  Then the preconditions of the GPU file's cases: every size lies beyond the
launch constant it is meant to cross, and the inputs are conditioned so that the restatement itself is stable -- conditions on the
inputs, not measurements of any kernel.  No element of any case is excluded from any comparison."""
from types import SimpleNamespace

import pytest

torch = pytest.importorskip("torch")       # (before sim_rollout_ref, which imports it)

import util  # noqa: E402,F401
import sim_rollout_ref as R  # noqa: E402
from util import golden  # noqa: E402

F64, F32 = torch.float64, torch.float32


def _rel(a, b):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30)) if b.numel() else 0.0


# ------------------------------------------------------------------------------------------------ the restatement against trusted forms
def test_rows_dot_is_F_linear_and_its_autograd():
    h8, W, b, add, dy = R.rows_dot_case(5)
    for T in (1, 3, 8):
        h, Wd, bd = (t.double().requires_grad_() for t in (h8[:T], W, b))
        y = torch.nn.functional.linear(h, Wd, bd) + add[:T].double()
        y.backward(dy[:T].double())
        assert _rel(R.rows_dot(h8[:T], W, b, add[:T]), y.detach()) < 1e-14
        assert _rel(R.rows_dot(h8[:T], W, b), y.detach() - add[:T].double()) < 1e-14
        for got, ref in zip(R.rows_dot_grads(h8[:T], W, dy[:T]), (Wd.grad, bd.grad, h.grad)):
            assert _rel(got, ref) < 1e-14


@pytest.mark.parametrize("K0", R.SIM_HIDDEN_K0)
def test_sim_hidden_is_the_composed_mlp_and_its_autograd(K0):
    e8, W1, b1, W2, b2, dh2 = R.sim_hidden_case(K0)
    for T in (1, 3, 8):
        p = [t.double().requires_grad_() for t in (W1, b1, W2, b2)]
        h1 = torch.relu(torch.nn.functional.linear(e8[:T].double(), p[0], p[1]))
        h2 = torch.relu(torch.nn.functional.linear(h1, p[2], p[3]))
        h2.backward(dh2[:T].double())
        r1, r2 = R.sim_hidden(e8[:T], W1, b1, W2, b2)
        assert _rel(r1, h1.detach()) < 1e-14 and _rel(r2, h2.detach()) < 1e-14
        for got, q in zip(R.sim_hidden_grads(e8[:T], W1, b1, W2, b2, dh2[:T]), p):
            assert _rel(got, q.grad) < 1e-13
    # torch.relu keeps a NaN: what the GPU file's NaN cases expect of the kernel
    e = e8[:3].clone()
    e[1, 0] = float("nan")
    r1, r2 = R.sim_hidden(e, W1, b1, W2, b2)
    assert bool(torch.isnan(r1[1]).all()) and bool(torch.isnan(r2[1]).all()) and bool(torch.isfinite(r1[[0, 2]]).all())


def test_simulator_chain_matches_the_reference_run():
    """tests/golden/simulator.npz: the reference module's outputs for five times and its six parameter gradients for a fixed cotangent
    (float32 runs: 1e-5 absolute forward, 1e-4 of each gradient's scale, the bars of tests/test_reference_goldens_gpu.py)"""
    from meshnet.meshnet_network import ResidualMeshSimulator
    g = golden("simulator.npz")
    mesh = torch.tensor(g["res_mesh"])
    sim = ResidualMeshSimulator(mesh, device="cpu")
    sim.load_state_dict({k[4:]: torch.tensor(g[k]) for k in g.files if k.startswith("res.")})
    _tt, enc, base = sim.times_on_device([float(t) for t in g["res_times"]])
    P = {k: torch.tensor(g["res." + k]) for k in ("input.weight", "input.bias", "hidden.weight", "hidden.bias", "output.weight", "output.bias")}
    h1, h2 = R.sim_hidden(enc, P["input.weight"], P["input.bias"], P["hidden.weight"], P["hidden.bias"])
    y = R.rows_dot(h2, P["output.weight"], P["output.bias"], base)
    assert float((y.reshape(g["res_out"].shape) - torch.tensor(g["res_out"]).double()).abs().max()) < 1e-5
    dy = torch.tensor(g["res_grad_w"]).reshape(y.shape)
    dWo, dbo, dh = R.rows_dot_grads(h2, P["output.weight"], dy)
    dW1, db1, dW2, db2 = R.sim_hidden_grads(enc, P["input.weight"], P["input.bias"], P["hidden.weight"], P["hidden.bias"], dh)
    for k, got in (("input.weight", dW1), ("input.bias", db1), ("hidden.weight", dW2), ("hidden.bias", db2), ("output.weight", dWo),
                   ("output.bias", dbo)):
        assert _rel(got, g["res_grad." + k]) < 1e-4, k


def _composed_regs(D, ei, rest, lams):
    from csplat import train as tr
    gs = SimpleNamespace(mesh=SimpleNamespace(edge_index=ei), edge_norm=rest.double().reshape(-1, 1))
    opt = SimpleNamespace(lambda_deform_mag=lams[0], lambda_rigid=lams[1], lambda_momentum=lams[2])
    x = D.double().requires_grad_()
    loss = tr.regularization(x, gs, opt, fused=False)
    if loss.requires_grad:
        loss.backward()
    return loss.detach().double(), (x.grad if x.grad is not None else torch.zeros_like(x))


@pytest.mark.parametrize("T,V,E", R.REGS_CASES)
def test_cloth_regs_is_the_composed_regularisation(T, V, E):
    """every case and lambda set, float64, on the GPU file's own inputs (zero-length edges, exact zeros, hubs): torch's norm and abs have
    the subgradient 0 at 0 the kernel's header states.  One exception, stated: without edges (E = 0) the composed form's
    F.l1_loss is the mean of an empty set, NaN, where the kernel and the restatement define the rigidity term as 0 -- there the sets with
    lambda_rigid = 0 are compared and the restatement's rigidity term is checked to be exactly 0"""
    D, ei, rest, _info = R.regs_case(T, V, E)
    for lams in R.REGS_LAMBDAS:
        loss, grad = R.cloth_regs(D, ei, rest, *lams)
        if E == 0 and lams[1] != 0:
            assert bool(torch.isnan(_composed_regs(D, ei, rest, lams)[0]))
            l0, g0 = R.cloth_regs(D, ei, rest, lams[0], 0.0, lams[2])
            assert torch.equal(loss, l0) and torch.equal(grad, g0)
            continue
        ref_loss, ref_grad = _composed_regs(D, ei, rest, lams)
        assert abs(float(loss) - float(ref_loss)) <= 1e-13 * max(float(ref_loss), 1e-30), lams
        assert _rel(grad, ref_grad) < 1e-12, lams
        if T > 3:       # time rows 3 .. carry the rigidity gradient only, in the composed form too
            g_r = R.cloth_regs(D, ei, rest, 0.0, lams[1], 0.0)[1]
            assert torch.equal(grad[3:], g_r[3:]) and (lams[1] == 0) == (not bool(ref_grad[3:].any()))


def test_refine_is_torch_adam_on_autograds_gradient_and_the_reference_run():
    from meshnet.rollout import refine_edge_lengths
    d = golden("refine.npz")
    for name in ("a", "b"):
        t = lambda k: torch.from_numpy(d[f"{name}.{k}"])  # noqa: E731
        grasped = int(d[f"{name}.grasped"])
        E = t("edge_index").shape[1]
        w = torch.ones(E)
        w[grasped] = 0.0
        v = R.edge_length_refine(t("pos"), t("v"), t("edge_index"), t("rest_len"), w, 10, 1e-3)
        v64 = refine_edge_lengths(t("pos").double(), t("v").double(), t("edge_index"), t("rest_len").double(), grasped)
        assert _rel(v, v64) < 1e-12, name
        v[grasped] = t("action").double()
        assert _rel(v, t("v_refined")) < 2e-6, name                    # (a float32 run of the reference)
    # weights of 0 / 1 (a list of zeroed entries instead of one grasped index) through the same formulation: torch.optim.Adam on autograd
    for N, E in R.REFINE_CASES:
        pos, v0, ei, rest, w = R.refine_case(N, E)
        for iters in R.REFINE_ITERS:
            got = R.edge_length_refine(pos, v0, ei, rest, w, iters, R.REFINE_LR)
            if E == 0 or iters == 0:
                assert torch.equal(got, v0.double())
                continue
            with torch.enable_grad():
                vo = v0.double().clone().requires_grad_()
                opt = torch.optim.Adam([vo], lr=R.REFINE_LR)
                for _ in range(iters):
                    opt.zero_grad()
                    x = pos.double() + vo
                    dv = (torch.norm(x[ei[0]] - x[ei[1]], dim=1) - rest.double()) * w.double()
                    torch.sum(dv ** 2).backward()
                    opt.step()
            assert _rel(got - v0.double(), vo.detach() - v0.double()) < 1e-9, (N, E, iters)


def test_head_decode_integrate_and_edge_features_are_their_torch_expressions():
    hist, nt, mean, std = R.head_case(257, 5, 9)
    x = torch.cat([hist[h] for h in range(5)] + [torch.nn.functional.one_hot(nt.long(), 9).float()], 1).double()
    feats, am = R.rollout_head(hist, nt, mean, std, 9)
    assert _rel(feats, (x - mean.double()) / std.double()) < 1e-15 and float(am) == float(feats.abs().max())
    assert torch.equal(R.rollout_head(hist, nt, None, None, 9)[0], x)
    assert R.rollout_head(hist[:, :0], nt[:0], None, None, 9)[0].shape == (0, 24)
    h, W, b, om, os_, last = R.decode_case(9, 3)
    v, fine = R.rollout_decode(h, W, b, om, os_, last)
    assert fine == 1 and _rel(v, last.double() + (torch.nn.functional.linear(h.double(), W.double(), b.double()) * os_.double() + om.double())) < 1e-15
    h[4, 7] = float("nan")
    assert R.rollout_decode(h, W, b, None, None, last)[1] == 0
    v, act, pos, hs = R.integrate_case(257, 3, 3)
    preds = torch.full((3, 257, 3), -7.0)
    v2, p2, h2, pr2 = R.rollout_integrate(v, act, 2, 256, pos, hs, preds)
    assert torch.equal(v2[256], act[1].double()) and torch.equal(v2[:256], v[:256].double()) and torch.equal(p2, pos.double() + v2)
    assert torch.equal(h2[:2], hs[1:].double()) and torch.equal(h2[2], v2) and torch.equal(pr2[1], v2) and bool((pr2[[0, 2]] == -7).all())
    for grasped in (257, -1):
        assert torch.equal(R.rollout_integrate(v, act, 1, grasped, pos, hs, preds)[0], v.double())
    pos, ei, order = R.edge_case(257)
    rows, am = R.edge_features(pos, ei, order)
    d = pos.double()[ei[0]] - pos.double()[ei[1]]
    assert _rel(rows, torch.cat([d, d.norm(dim=1, keepdim=True)], 1)[order]) < 1e-15 and float(am) == float(rows.abs().max())
    assert float(R.edge_features(pos, ei)[0][1, 3]) == 0.0 and float(R.edge_features(pos, ei)[0][0, 3]) == 0.0


# ------------------------------------------------------------------------------------------------ sizes against the launch constants
def test_sizes_lie_beyond_the_launch_constants():
    """the constants as literals; each comment names the source line that holds it (line numbers of csrc/csplat_sim.hip and
    csrc/csplat_gnn.hip as of this test's commit, with the expression, which is what to look for once the lines have moved)"""
    cdiv = lambda a, b: -(-a // b)  # noqa: E731
    # csplat_sim.hip:321 `fwd_blocks = std::max(SIM_BLOCKS, std::min(2048, (R + 15) / 16))`, :32 / :36 four waves x four rows per workgroup:
    # the grid-stride loop of k_rows_dot_fwd (:36) takes a second pass only above 2048 * 16 rows
    one_pass = 2048 * 16
    assert one_pass == 32768 and max(R.ROWS_DOT_FWD_R) > one_pass and 32769 in R.ROWS_DOT_FWD_R and 32768 in R.ROWS_DOT_FWD_R
    assert any(r % 16 not in (0, 1) for r in R.ROWS_DOT_FWD_R if r > one_pass)          # (a partial wave behind the second pass)
    assert any(512 * 16 < r <= one_pass for r in R.ROWS_DOT_FWD_R) and any(r < 4 for r in R.ROWS_DOT_FWD_R)
    # csplat_sim.hip:18 `SIM_BLOCKS = 512`, :328 `k_rows_dot_bwd<T><<<SIM_BLOCKS, 256`, :67 the loop: 512 workgroups of 16 rows per pass
    assert max(R.ROWS_DOT_BWD_R) > 512 * 16 * 4 and any(512 * 16 < r <= 512 * 16 * 2 for r in R.ROWS_DOT_BWD_R)
    # csplat_sim.hip:17 `SIM_TMAX = 8`, :342 `SIM_K0MAX = 16`, :477-484 / :498-505 / :564 / :578 the four switches: every instantiation,
    # the K0 limits and the reference's 13
    assert tuple(R.ROWS_DOT_T) == tuple(range(1, 9)) == tuple(R.SIM_HIDDEN_T) and {1, 13, 16} <= set(R.SIM_HIDDEN_K0)
    # csplat_sim.hip:214 (k_cloth_regs) `for (unsigned j = threadIdx.x; j < gridDim.x; j += 256)`, :307 (k_cloth_regs_csr) `j < nblocks`:
    # a second sweep above 256 workgroups; :536 `blocks = cdiv(items, 256)`, :541 `dim3(cdiv(V, 256), T)`
    scatter = {c: cdiv(c[1] + c[0] * c[2], 256) for c in R.REGS_CASES}
    csr = {c: c[0] * cdiv(c[1], 256) for c in R.REGS_CASES}
    assert scatter[(3, 22001, 22003)] > 256 and csr[(3, 22001, 22003)] > 256 and scatter[(3, 300, 70001)] > 256 and csr[(3, 300, 70001)] <= 256
    assert scatter[(3, 1, 0)] == 1 and csr[(3, 255, 1)] == 3 and csr[(3, 256, 255)] == 3 and csr[(3, 257, 300)] == 6
    assert 257 % 256 != 0 and cdiv(257, 256) == cdiv(257 + 1, 256)            # node and edge items share the scatter form's workgroup 1
    assert {c[0] for c in R.REGS_CASES} >= {1, 2, 3, 4, 8}                    # :148 / :265 `T >= 3`, the node terms' threshold
    # csplat_gnn.hip:346 `k_rollout_head<<<cdiv(N > 0 ? N : 1, 256), 256`; :344 `H <= 16 && T >= 0 && T <= 16`
    assert {255, 256, 257} <= set(R.HEAD_N) and max(R.HEAD_N) > 256 * 32 and 0 in R.HEAD_N
    assert max(h for h, _ in R.HEAD_HT) == 16 and max(t for _, t in R.HEAD_HT) == 16 and min(t for _, t in R.HEAD_HT) == 0
    # csplat_gnn.hip:134 `n = (blockIdx.x * 256 + threadIdx.x) >> 5`, :356 `cdiv((int64_t)N * 32, 256)`: half a wave per row, 8 rows per workgroup
    assert 256 // 32 == 8 and {7, 8, 9} <= set(R.DECODE_N) and any(n % 2 for n in R.DECODE_N if n > 8) and tuple(R.DECODE_D) == (1, 2, 3, 4)
    # csplat_gnn.hip:364 `k_rollout_integrate<<<cdiv(N, 256), 256`: below one workgroup, one node into the second, many workgroups;
    # :170 `for (int h = 0; h + 1 < H; h++)` the shift loop: empty, once, order matters; :352 / :362 `D <= 4`
    assert min(R.INTEGRATE_N) < 256 and 257 in R.INTEGRATE_N and max(R.INTEGRATE_N) > 256 * 32 and max(R.INTEGRATE_N) % 256 != 0
    assert {1, 2, 3} <= set(R.INTEGRATE_H) and max(R.INTEGRATE_H) > 3 and {1, 4} <= set(R.INTEGRATE_D)
    # csplat_gnn.hip:338 `nb < 512 ? nb : 512` workgroups of 256 edges; :500 `nb < 4096 ? nb : 4096` of 256 float4 items
    assert max(R.EDGE_FEATURES_E) > 512 * 256 and {0, 1, 255, 257} <= set(R.EDGE_FEATURES_E)
    assert max(E * (L // 4) for L, E in R.GATHER_CASES) > 4096 * 256 and any(E * (L // 4) < 64 for L, E in R.GATHER_CASES)
    # csplat_gnn.hip:388 `k_edge_len_adam<<<cdiv(N, 256), 256`: one node, and one node into a second workgroup; :385 / :394 the double
    # buffer ends in the scratch after an odd number of iterations (copied back) and in v after an even one; :378 iters = 0 returns
    assert set(R.REFINE_CASES) == {(n, e) for n in (1, 257) for e in (0, 300, 3000)} and cdiv(257, 256) == 2
    assert 0 in R.REFINE_ITERS and any(i % 2 for i in R.REFINE_ITERS) and any(i and not i % 2 for i in R.REFINE_ITERS)
    assert max(R.REFINE_ITERS) == 10                                            # (the rollout's own count)


# ------------------------------------------------------------------------------------------------ input conditions
@pytest.mark.parametrize("T,V,E", R.REGS_CASES)
def test_regulariser_cases_are_conditioned(T, V, E):
    """every momentum component and every |rest - len| is exactly 0 by construction or at least 1e-4 of the case's largest; the exact
    zeros are exact in float32 too; what the case was to contain is there"""
    D, ei, rest, info = R.regs_case(T, V, E)
    assert D.dtype == F32 and rest.dtype == F32 and ei.dtype == torch.int64 and (E == 0 or (int(ei.min()) >= 0 and int(ei.max()) < V))
    assert torch.equal(torch.round(D / R.REGS_GRID) * R.REGS_GRID, D) and float(D.abs().max()) < 8            # on the grid: differences are exact
    if T >= 3:
        m = D[2].double() - 2 * D[1].double() + D[0].double()
        m32 = D[2] - 2 * D[1] + D[0]
        assert torch.equal(m32.double(), m)                                          # exact in float32: the same zeros, the same signs
        nz = m[m != 0].abs()
        assert nz.numel() == 0 or float(nz.min()) >= 1e-4 * float(m.abs().max())
        for v in info["still"]:
            assert not bool(m[v].any()) and torch.equal(D[0, v], D[1, v]) and torch.equal(D[1, v], D[2, v])
        assert len(info["still"]) == (4 if V >= 16 else 0)
    if E > 0:
        ln = R._norm3(D.double()[:, ei[1]] - D.double()[:, ei[0]])
        diff = (rest.double()[None] - ln).abs()
        nz = diff[diff != 0]
        assert float(nz.min()) >= 1e-4 * float(diff.max()), (float(nz.min()), float(diff.max()))
        assert info["moved"] <= max(4, (T * E) // 500)                               # the nudging touched few edges
        zero = (diff == 0).all(0).nonzero().reshape(-1).tolist()
        assert zero == ([] if info["exact_rest"] is None else [info["exact_rest"]])
        if info["exact_rest"] is not None:
            e = info["exact_rest"]
            d32 = D[:, ei[1, e]] - D[:, ei[0, e]]
            assert torch.equal(d32, torch.tensor([3.0, 4.0, 0.0]).expand(T, 3)) and float(rest[e]) == 5.0
            assert int(ei[0, info["self_loop"]]) == int(ei[1, info["self_loop"]])
            c = info["coincident"]
            assert int(ei[0, c]) != int(ei[1, c]) and torch.equal(D[:, ei[0, c]], D[:, ei[1, c]])
    deg_in, deg_out = (torch.bincount(ei[r], minlength=V) for r in (1, 0))
    for v in info["isolated"]:
        assert int(deg_in[v]) == 0 and int(deg_out[v]) == 0
    assert (len(info["isolated"]) == 5) == (V >= 257)
    if E >= 2000:
        assert int(deg_in[info["hub_in"]]) >= 300 and int(deg_out[info["hub_out"]]) >= 300
        a, b = info["copies"]
        assert b - a == 20 and bool((ei[:, a:b] == ei[:, a:a + 1]).all())


@pytest.mark.parametrize("K0", R.SIM_HIDDEN_K0)
def test_sim_hidden_cases_are_conditioned(K0):
    """either ReLU has dead and live units in every row; the two zero units are exactly 0; no other preactivation is within 1e-4 of 0"""
    e8, W1, b1, W2, b2, _ = R.sim_hidden_case(K0)
    z1 = e8.double() @ W1.double().t() + b1.double()
    z2 = torch.relu(z1) @ W2.double().t() + b2.double()
    for z, unit in ((z1, R.SIM_ZERO_UNIT_1), (z2, R.SIM_ZERO_UNIT_2)):
        assert bool((z > 0).any(1).all()) and bool((z < 0).any(1).all())
        assert not bool(z[:, unit].any())
        rest = torch.cat([z[:, :unit], z[:, unit + 1:]], 1).abs()
        assert float(rest.min()) >= 1e-4 * float(z.abs().max())
    z32 = e8 @ W1.t() + b1
    assert not bool(z32[:, R.SIM_ZERO_UNIT_1].any())


@pytest.mark.parametrize("N,E", [c for c in R.REFINE_CASES if c[1] > 0])
def test_refine_cases_are_conditioned(N, E):
    """every per-node gradient component at every iteration is 0 or at least 1e-3 of that iteration's largest (Adam's first steps are
    sign-like); the degenerate edges and the hub are there; isolated nodes have no gradient at all.  N = 1: nothing but self-loops, every
    gradient exactly 0 at every iteration in float64 and in float32, v unchanged"""
    pos, v, ei, rest, w = R.refine_case(N, E)
    assert int(ei.min()) >= 0 and int(ei.max()) < N and bool((w == 0).any()) and bool((w == 1).any())
    if N == 1:
        assert not bool(ei.any())
        for dt in (F64, F32):
            out, grads = R.edge_length_refine(pos, v, ei, rest, w, max(R.REFINE_ITERS), R.REFINE_LR, dt, return_grads=True)
            assert len(grads) == max(R.REFINE_ITERS) and not any(bool(g.any()) for g in grads) and torch.equal(out, v.to(dt))
        return
    _, grads = R.edge_length_refine(pos, v, ei, rest, w, max(R.REFINE_ITERS), R.REFINE_LR, return_grads=True)
    for t, g in enumerate(grads):
        nz = g[g != 0].abs()
        assert float(nz.min()) >= 1e-3 * float(g.abs().max()), (t, float(nz.min()), float(g.abs().max()))
        assert not bool(g[N - 5:].any())
    deg = torch.bincount(ei.reshape(-1), minlength=N)
    assert not bool(deg[N - 5:].any()) and int(ei[0, 0]) == int(ei[1, 0]) and torch.equal(pos[5] + v[5], pos[6] + v[6])
    if E >= 3000:
        assert int(torch.bincount(ei[0], minlength=N)[10]) >= 300
