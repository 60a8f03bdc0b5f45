"""The kNN-graph regularisers on the GPU (csplat.knn_regs: csplat_knn_regs_graph / _fwd / _bwd) against tests/knn_regs_ref.py.

Tolerance.  Float32 rounding of this function depends on the input (R off_t - off_{t-1} cancels when the motion is nearly rigid), so
no constant is fixed: every comparison runs the float32 restatement on the CPU on the same inputs, measures its scale-relative error
e32 = max |x32 - x64| / max |x64| per tensor (dM, dQ and each of the four loss words), and the kernel must stay within
4 e32 + 4 * 2^-24 -- the same arithmetic in another summation order.  A dropped or mis-signed pair moves a node's gradient by about
the scale itself.  Every case prints e32, the kernel's error and error / bound.
Largest error / bound seen on an MI355X: 0.501 (N = 300, K = 8, T = 3, near-rigid, isometric_abs, L_spring: e32 0.55 u, kernel 3.11 u,
u = 2^-24); the largest of a gradient is 0.41 (a dQ), the near-rigid gradients sit at 0.23 .. 0.26 (the kernel's error is the
restatement's own there).
"""
from types import SimpleNamespace

import numpy as np
import pytest

import util  # noqa: F401
import knn_regs_ref as R

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

ALL = (0.7, 1.3, 2.1)
WORST = {"ratio": 0.0, "where": ""}


@pytest.fixture(scope="module", autouse=True)
def _worst():
    yield
    print(f"\nlargest kernel error / bound of this run: {WORST['ratio']:.3f} ({WORST['where']})")


def gpu(a, grad=False):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda().requires_grad_(grad)


def rows(N, T, motion, seed, pts=None):
    """(pts [N,3], M [T,N,3], Q [T,N,4]) float32: 'large' = unrelated random rows and random unnormalised quaternions; 'near' = the
    cloud and one rotation field moved by 1e-3 per row (the training regime)"""
    rng = np.random.default_rng(seed)
    if pts is None:
        pts = rng.uniform(-1, 1, (N, 3))
    pts = np.asarray(pts, np.float32)
    if motion == "large":
        M = rng.normal(size=(T, N, 3))
        Q = rng.normal(size=(T, N, 4)) * rng.uniform(0.3, 3.0, (T, N, 1))
    else:
        M = pts[None] + 1e-3 * rng.normal(size=(T, N, 3))
        Q = rng.normal(size=(1, N, 4)) * rng.uniform(0.3, 3.0, (1, N, 1)) + 1e-3 * rng.normal(size=(T, N, 4))
    return pts, M.astype(np.float32), Q.astype(np.float32)


def run_kernel(graph, M, Q, lams, iso_abs, up):
    from csplat.knn_regs import neighbour_regularization
    tM, tQ = gpu(M, True), (None if Q is None else gpu(Q, True))
    loss, parts = neighbour_regularization(tM, tQ, graph, *lams, isometric_abs=iso_abs)
    assert loss.is_cuda and loss.dtype == torch.float32 and loss.shape == () and parts.shape == (3,) and not parts.requires_grad
    (loss * up).backward()
    dQ = None if tQ is None else (tQ.grad if tQ.grad is not None else torch.zeros_like(tQ)).cpu().numpy()
    return dict(loss=float(loss.detach()), parts=parts.cpu().numpy().astype(np.float64), dM=tM.grad.cpu().numpy(), dQ=dQ)


def compare(name, graph, M, Q, lams, iso_abs=False, up=1.0):
    idx, d0, w = graph.idx.cpu().numpy(), graph.d0.cpu().numpy(), graph.w.cpu().numpy()
    got = run_kernel(graph, M, Q, lams, iso_abs, up)
    u = float(np.float32(up))
    r64 = R.evaluate(M, Q, idx, d0, w, lams, iso_abs, up=u)
    r32 = R.evaluate(M, Q, idx, d0, w, lams, iso_abs, up=u, dtype=torch.float32)
    items = [("dM", got["dM"], r32["dM"], r64["dM"])]
    if Q is not None:
        items.append(("dQ", got["dQ"], r32["dQ"], r64["dQ"]))
    for m, word in enumerate(("L_iso", "L_spring", "L_rigid")):
        items.append((word, got["parts"][m], r32["parts"][m], r64["parts"][m]))
    items.append(("L", got["loss"], r32["loss"], r64["loss"]))
    failed = []
    for what, g, x32, x64 in items:
        e32, ek = R.scale_err(x32, x64), R.scale_err(g, x64)
        bound = 4 * e32 + 4 * R.U
        ratio = ek / bound
        print(f"{name} {what}: e32 {e32 / R.U:.2f} u, kernel {ek / R.U:.2f} u, error / bound {ratio:.3f} (scale {float(np.abs(x64).max()):.3e})")
        if ratio > WORST["ratio"]:
            WORST.update(ratio=ratio, where=f"{name} {what}")
        if not ek <= bound:
            failed.append(f"{what}: kernel error {ek:.3e} beyond 4 e32 + 4 u = {bound:.3e}")
    assert not failed, f"{name}: " + "; ".join(failed)
    return got, r64


def knn_graph(pts, K, lambda_w=20.0):
    from csplat.knn_regs import NeighbourGraph
    return NeighbourGraph.from_points(gpu(pts), K, lambda_w)


# ---------------------------------------------------------------------------------------------------------------- against the restatement
# N: K + 1 (every other node is a neighbour), 255 / 256 / 257 (one workgroup of the forward and its edges), 4097 (the boxed k-NN, many
# workgroups); K: 1, 5, 8 | 9 (the backward's group of 4 lanes ends at 8, 16 lanes from 9), 20, 32; T: 1, 2, 3, 5.
CASES = [
    (6, 5, 3, "large", False, ALL, 1.0),
    (33, 32, 2, "near", True, ALL, 0.37),
    (255, 5, 3, "large", True, ALL, 0.37),
    (256, 20, 5, "near", False, ALL, 1.0),
    (257, 1, 2, "large", False, ALL, 1.0),
    (257, 5, 1, "large", True, ALL, 0.37),
    (300, 8, 3, "near", True, ALL, 1.0),
    (300, 9, 3, "large", False, ALL, 0.37),
    (4097, 5, 3, "near", False, ALL, 1.0),
    (4097, 20, 3, "large", True, ALL, 0.37),
    (4097, 32, 2, "near", True, ALL, 1.0),
    (2000, 5, 3, "large", False, ALL, 1.0),
    (2000, 5, 3, "near", False, ALL, 0.37),
    (2000, 5, 3, "near", False, (0.7, 0.0, 0.0), 1.0),
    (2000, 5, 3, "near", True, (0.7, 0.0, 0.0), 1.0),
    (2000, 5, 3, "near", False, (0.0, 1.3, 0.0), 0.37),
    (2000, 5, 3, "near", False, (0.0, 0.0, 2.1), 1.0),
    (2000, 5, 5, "large", False, (0.0, 0.0, 2.1), 0.37),
]


@pytest.mark.parametrize("N,K,T,motion,iso_abs,lams,up", CASES)
def test_loss_and_gradients_against_the_restatement(N, K, T, motion, iso_abs, lams, up):
    pts, M, Q = rows(N, T, motion, seed=N + 7 * K + T)
    graph = knn_graph(pts, K)
    assert (graph.N, graph.K) == (N, K)
    got, r64 = compare(f"N={N} K={K} T={T} {motion} abs={iso_abs} lams={lams} g={up}", graph, M, Q, lams, iso_abs, up)
    assert np.abs(r64["dM"]).max() > 0
    if T == 1:
        assert got["parts"][1] == 0.0 and got["parts"][2] == 0.0 and not got["dQ"].any()
    if lams[2] == 0.0:
        assert not got["dQ"].view(np.uint32).any()


def test_long_reverse_runs_of_a_coincident_cloud():
    """all points coincide: ties go to the smaller index, so nodes 0 .. K are named by every other node"""
    N, K, T = 1500, 5, 3
    pts = np.tile(np.array([[0.3, -0.2, 0.5]], np.float32), (N, 1))
    graph = knn_graph(pts, K)
    off = graph.rev_offsets.cpu().numpy()
    assert int(np.diff(off).max()) > 1000 and int(graph.idx.max()) == K
    assert not graph.d0.any() and bool((graph.w == 1).all())
    _, M, Q = rows(N, T, "large", seed=5)
    compare("coincident cloud", graph, M, Q, ALL, False, 0.37)
    compare("coincident cloud abs", graph, M, Q, ALL, True, 1.0)


def test_long_reverse_runs_of_a_hub_graph():
    from csplat.knn_regs import NeighbourGraph
    N, K, T = 1200, 3, 3
    rng = np.random.default_rng(8)
    i = np.arange(N)
    idx = np.stack([np.zeros(N, np.int64), (i + 1) % N, (i + 7) % N], 1)
    idx[0] = [1, 2, 3]
    graph = NeighbourGraph.from_indices(torch.from_numpy(idx).cuda(), gpu(rng.uniform(0.1, 1.0, (N, K))), gpu(rng.uniform(0.0, 1.0, (N, K))))
    off, ent = R.reverse_lists(idx, N)
    assert np.array_equal(graph.rev_offsets.cpu().numpy(), off) and np.array_equal(graph.rev_entries.cpu().numpy(), ent)
    assert int(np.diff(off).max()) > 1000
    _, M, Q = rows(N, T, "large", seed=6)
    compare("hub graph", graph, M, Q, ALL, True, 0.37)
    _, M, Q = rows(N, T, "near", seed=6, pts=rng.uniform(-1, 1, (N, 3)))
    compare("hub graph near", graph, M, Q, ALL, False, 1.0)


# ---------------------------------------------------------------------------------------------------------------- exact facts
def _half_named(N=600, K=4, seed=2):
    """a graph whose neighbours all lie in the first half: nobody names a node of the second half"""
    from csplat.knn_regs import NeighbourGraph
    rng = np.random.default_rng(seed)
    idx = rng.integers(0, N // 2, (N, K))
    return NeighbourGraph.from_indices(torch.from_numpy(idx).cuda(), gpu(rng.uniform(0.1, 1.0, (N, K))), gpu(rng.uniform(0.1, 1.0, (N, K))))


def test_rotation_gradient_of_unnamed_nodes_is_bitwise_zero():
    graph = _half_named()
    _, M, Q = rows(graph.N, 3, "large", seed=3)
    got = run_kernel(graph, M, Q, ALL, False, 1.0)
    assert not got["dQ"][:, graph.N // 2:].view(np.uint32).any()
    named = np.diff(graph.rev_offsets.cpu().numpy()) > 0
    assert named[:graph.N // 2].any() and not named[graph.N // 2:].any()
    assert (np.abs(got["dQ"][1][named]).max(axis=1) > 0).all()
    compare("half-named graph", graph, M, Q, ALL, True, 0.37)


def test_no_rotations_without_rigidity_is_the_same_bits():
    pts, M, Q = rows(700, 3, "near", seed=4)
    graph = knn_graph(pts, 5)
    a = run_kernel(graph, M, Q, (0.7, 1.3, 0.0), False, 0.37)
    b = run_kernel(graph, M, None, (0.7, 1.3, 0.0), False, 0.37)
    assert np.float32(a["loss"]).view(np.uint32) == np.float32(b["loss"]).view(np.uint32)
    assert np.array_equal(a["dM"].view(np.uint32), b["dM"].view(np.uint32))
    assert np.array_equal(a["parts"][:2], b["parts"][:2]) and b["parts"][2] == 0.0 and a["parts"][2] > 0.0
    assert not a["dQ"].view(np.uint32).any()


def test_a_duplicated_time_row_has_no_spring():
    pts, M, Q = rows(500, 2, "large", seed=9)
    M[1] = M[0]
    graph = knn_graph(pts, 5)
    got = run_kernel(graph, M, Q, ALL, False, 1.0)
    assert got["parts"][1] == 0.0 and got["parts"][0] != 0.0 and got["parts"][2] > 0.0
    _, M3, Q3 = rows(500, 3, "large", seed=9)
    M3[2] = M3[1]
    r64 = R.evaluate(M3, Q3, graph.idx.cpu().numpy(), graph.d0.cpu().numpy(), graph.w.cpu().numpy(), (0.0, 1.0, 0.0))
    r64_first = R.evaluate(M3[:2], Q3[:2], graph.idx.cpu().numpy(), graph.d0.cpu().numpy(), graph.w.cpu().numpy(), (0.0, 1.0, 0.0))
    got3 = run_kernel(graph, M3, Q3, (0.0, 1.0, 0.0), False, 1.0)
    # rows (1, 2) add exactly nothing: the spring term of three rows is half that of the first two
    assert abs(got3["parts"][1] - 0.5 * r64_first["parts"][1]) <= 4 * R.U * r64["parts"][1]


def test_forward_bits_do_not_depend_on_who_requires_a_gradient():
    from csplat.knn_regs import neighbour_regularization
    pts, M, Q = rows(900, 3, "near", seed=12)
    graph = knn_graph(pts, 5)
    out, grads = [], []
    for gm, gq in ((True, True), (True, False), (False, True), (False, False)):
        tM, tQ = gpu(M, gm), gpu(Q, gq)
        loss, parts = neighbour_regularization(tM, tQ, graph, *ALL)
        assert loss.requires_grad == (gm or gq)
        if gm or gq:
            loss.backward()
        out.append(torch.cat([loss.detach().reshape(1), parts]).view(torch.int32))
        grads.append((tM.grad, tQ.grad))
    assert all(torch.equal(out[0], o) for o in out[1:])
    assert grads[1][1] is None and grads[2][0] is None and grads[3] == (None, None)
    assert torch.equal(grads[0][0].view(torch.int32), grads[1][0].view(torch.int32))
    assert torch.equal(grads[0][1].view(torch.int32), grads[2][1].view(torch.int32))


# ---------------------------------------------------------------------------------------------------------------- reproducibility, capture
def _run(graph, tM, tQ):
    from csplat.knn_regs import neighbour_regularization
    loss, parts = neighbour_regularization(tM, tQ, graph, *ALL, isometric_abs=True)
    gM, gQ = torch.autograd.grad(loss * 0.37, (tM, tQ))
    return loss.detach().clone(), parts.clone(), gM, gQ


def _repro_case():
    pts, M, Q = rows(4097, 3, "near", seed=21)
    return knn_graph(pts, 20), gpu(M, True), gpu(Q, True)


def test_two_runs_are_bit_equal():
    graph, tM, tQ = _repro_case()
    first, second = _run(graph, tM, tQ), _run(graph, tM, tQ)
    for x, y in zip(first, second):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))


def test_forward_and_backward_replayed_from_a_graph_equal_eager():
    from csplat import graphs
    graph, tM, tQ = _repro_case()
    eager = _run(graph, tM, tQ)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with graphs.capture(g):
        recorded = _run(graph, tM, tQ)
    for r in recorded:
        r.zero_()
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    for e, r in zip(eager, recorded):
        assert torch.equal(e.view(torch.int32), r.view(torch.int32))
    # on a side stream: the same bits
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        on_side = _run(graph, tM, tQ)
    side.synchronize()
    for e, s in zip(eager, on_side):
        assert torch.equal(e.view(torch.int32), s.view(torch.int32))


# ---------------------------------------------------------------------------------------------------------------- from_points
@pytest.mark.parametrize("N,K,lambda_w", [(300, 5, 20.0), (4097, 20, 200.0), (4096, 32, 100.0)])
def test_from_points_is_the_knn_graph_with_its_rest_state(N, K, lambda_w):
    import simple_knn
    from csplat.knn_regs import NeighbourGraph
    pts = gpu(np.random.default_rng(N).uniform(-1, 1, (N, 3)))
    graph = NeighbourGraph.from_points(pts, K, lambda_w)
    d2, idx = simple_knn.knn(pts, K)
    assert graph.idx.dtype == torch.int64 and torch.equal(graph.idx, idx)
    d2 = d2.cpu().numpy().astype(np.float64)
    for name, got, ref in (("d0", graph.d0, np.sqrt(d2)), ("w", graph.w, np.exp(-lambda_w * d2))):
        got = got.cpu().numpy()
        assert got.dtype == np.float32 and got.shape == (N, K)
        assert ref.min() > 1e-37, "the case is meant to stay in float32's normal range"
        ulps = np.abs(got.astype(np.float64) - ref) / np.spacing(ref.astype(np.float32)).astype(np.float64)
        print(f"N={N} K={K} lambda_w={lambda_w} {name}: largest error {ulps.max():.3f} ulp")
        assert ulps.max() <= 2.0
    off, ent = R.reverse_lists(idx.cpu().numpy(), N)
    assert np.array_equal(graph.rev_offsets.cpu().numpy(), off) and np.array_equal(graph.rev_entries.cpu().numpy(), ent)


# ---------------------------------------------------------------------------------------------------------------- the train step
LAMS = dict(lambda_isometric=0.3, lambda_spring=2.0, lambda_rigidity=5.0)
GRAPH = dict(k_nearest=5, lambda_w=20.0)
_CACHE = {}


def _plain_steps():
    from test_geometry_loss_gpu import _three_steps
    if "plain" not in _CACHE:
        _CACHE["plain"] = _three_steps(lambda s: s.plain, None)
    return _CACHE["plain"]


def test_train_step_unchanged_when_the_weights_are_zero_or_absent():
    from test_geometry_loss_gpu import _assert_same_bits, _opt, _three_steps
    plain = _plain_steps()
    zero = _three_steps(lambda s: s.plain, _opt(lambda_isometric=0.0, lambda_spring=0.0, lambda_rigidity=0.0, **GRAPH))
    assert plain["log"][0][2] == ["allreduce_ms", "radii", "viewspace_grad", "visibility_filter"]
    _assert_same_bits(plain, zero)


def test_train_step_untouched_up_to_reg_iter():
    from test_geometry_loss_gpu import _assert_same_bits, _opt, _three_steps
    waiting = _three_steps(lambda s: s.plain, _opt(reg_iter=3, **LAMS, **GRAPH))          # iterations 1 .. 3
    _assert_same_bits(_plain_steps(), waiting)


def test_captured_step_with_the_term_runs_eagerly():
    from test_geometry_loss_gpu import _assert_same_bits, _opt, _three_steps
    opt = _opt(**LAMS, **GRAPH)
    eager = _three_steps(lambda s: s.plain, opt, steps=2)
    cap = _three_steps(lambda s: s.plain, opt, captured=True, steps=2)
    assert cap["cs"] is not None and cap["cs"].stats["eager"] == 2 and cap["cs"].stats["recorded"] == 0 and cap["cs"].stats["replayed"] == 0
    assert all(k in eager["log"][0][2] for k in ("isometric_loss", "spring_loss", "rigidity_loss"))
    _assert_same_bits(eager, cap)


def _one_step(opt, monkeypatch, iteration=1):
    """step `iteration` on a fresh scene in the bit-reproducible mode -> loss, stats, the views' centres and rotations, the graph a
    caller would build by hand from the centres before the step"""
    from csplat import native, train as tr
    from csplat.knn_regs import NeighbourGraph
    from test_geometry_loss_gpu import _scene
    native.lib.csplat_debug_flags(256)
    try:
        s = _scene()
        with torch.no_grad():
            by_hand = NeighbourGraph.from_points(s.pc.get_xyz().detach().float().contiguous(), GRAPH["k_nearest"], GRAPH["lambda_w"])
        seen = {}
        inner = tr.render_views

        def spy(*a, **kw):
            out = inner(*a, **kw)
            seen["means"] = [r.means3D_deform.detach().clone() for r in out[0]]
            seen["rots"] = [r.rotations.detach().clone() for r in out[0]]
            return out

        monkeypatch.setattr(tr, "render_views", spy)
        _ps, loss, stats = tr.train_step(iteration, s.plain, s.pc, s.sim, s.mopt, opt=opt, background=s.bg)
        torch.cuda.synchronize()
        monkeypatch.setattr(tr, "render_views", inner)
        return SimpleNamespace(s=s, loss=loss, stats=stats, means=seen["means"], rots=seen["rots"], by_hand=by_hand)
    finally:
        native.lib.csplat_debug_flags(0)


@pytest.mark.parametrize("iso_abs", [False, True])
def test_train_step_loss_and_stats_with_the_weights_on(monkeypatch, iso_abs):
    from csplat.knn_regs import neighbour_regularization
    from test_geometry_loss_gpu import _opt
    off = _one_step(_opt(), monkeypatch)
    on = _one_step(_opt(isometric_abs=iso_abs, **LAMS, **GRAPH), monkeypatch)
    keys = ["isometric_loss", "rigidity_loss", "spring_loss"]
    assert not set(keys) & set(off.stats) and sorted(set(on.stats) - set(off.stats)) == keys
    for k in keys:
        v = on.stats[k]
        assert v.is_cuda and not v.requires_grad and v.shape == () and v.dtype == torch.float32
    # the same scene, the same forward: the two steps rendered the same centres
    assert all(torch.equal(a, b) for a, b in zip(on.means, off.means))
    # the graph is the k-NN graph of the undeformed centres before the step
    cached = on.s.pc._neighbour_graph[1]
    assert torch.equal(cached.idx, on.by_hand.idx) and torch.equal(cached.d0, on.by_hand.d0) and torch.equal(cached.w, on.by_hand.w)
    # the three stats are neighbour_regularization by hand on the views' centres and rotations, in camera order
    loss, parts = neighbour_regularization(torch.stack(on.means), torch.stack(on.rots), on.by_hand, LAMS["lambda_isometric"],
                                           LAMS["lambda_spring"], LAMS["lambda_rigidity"], isometric_abs=iso_abs)
    got = torch.stack([on.stats["isometric_loss"], on.stats["spring_loss"], on.stats["rigidity_loss"]])
    assert torch.equal(got.view(torch.int32), parts.view(torch.int32))
    # loss - loss_off is the weighted sum of the parts
    p = [float(x) for x in parts.double().cpu()]
    term = LAMS["lambda_isometric"] * p[0] + LAMS["lambda_spring"] * p[1] + LAMS["lambda_rigidity"] * p[2]
    diff = float(on.loss) - float(off.loss)
    print(f"abs={iso_abs}: parts {p}, weighted {term:.9g}, loss off {float(off.loss):.9g} on {float(on.loss):.9g}, difference {diff:.9g}")
    assert abs(diff - term) <= 2.0 ** -22 * (abs(float(off.loss)) + abs(term))
    assert abs(term) > 100 * 2.0 ** -22 * abs(float(off.loss)), "the term would not be seen in the loss"
    assert abs(float(loss) - term) <= 4 * R.U * sum(abs(x) for x in (LAMS["lambda_isometric"] * p[0], LAMS["lambda_spring"] * p[1],
                                                                       LAMS["lambda_rigidity"] * p[2]))


def test_train_step_rebuilds_the_graph_on_schedule_and_after_a_change_of_size():
    from csplat import train as tr
    from test_geometry_loss_gpu import _opt, _scene
    s = _scene()
    opt = _opt(knn_update_iter=3, **LAMS, **GRAPH)
    built = []
    for it in (1, 2, 3, 4):
        tr.train_step(it, s.plain, s.pc, s.sim, s.mopt, opt=opt, background=s.bg)
        built.append(s.pc._neighbour_graph[2])
    assert built == [1, 1, 3, 3]
    # the cache remembers the number of Gaussians it was built for: another number (as after densification) rebuilds it
    key, graph, _it = s.pc._neighbour_graph
    assert key[0] == int(s.pc.num_gaussians)
    s.pc._neighbour_graph = ((key[0] - 1,) + key[1:], graph, _it)
    tr.train_step(5, s.plain, s.pc, s.sim, s.mopt, opt=opt, background=s.bg)
    assert s.pc._neighbour_graph[2] == 5 and s.pc._neighbour_graph[0] == key and s.pc._neighbour_graph[1] is not graph
