"""The two-cloud k-NN kernels on the GPU: both forms (csplat_knn_query, csplat_knn_query_ws), called directly, bit for bit
against the numpy restatement tests/knn_query_ref.py; the pruned form against the brute-force form at a size the restatement
is too slow for; simple_knn.knn_query at full size against SciPy's KD-tree; csplat.external.find_closest_gauss against the
reference's formulation restated in numpy; side stream and graph replay."""
import numpy as np
import pytest
import torch

import util  # noqa: F401
import knn_query_ref as R

pytestmark = pytest.mark.gpu

TOL = 8 * 2.0 ** -24   # five float32 roundings (2^-24 each) in dx*dx + dy*dy + dz*dz, rounded up to a power of two

QS = [1, 63, 64, 65, 255, 256, 257, 1025]
NS = [1, 2, "K-1", "K", "K+1", 1023, 1024, 1025, 4097]          # 1023 .. 1025: the slab and box edge; K-1 with K = 1: no point at all
KS = [1, 3, 4, 5, 8, 9, 16, 17, 32]                             # the CAP boundaries
KINDS = ["uniform", "planar", "clustered", "duplicates", "self", "coincident", "far", "lattice16", "lattice4"]


def clouds(kind, Q, N, seed):
    """(queries [Q,3], points [N,3]) float32"""
    rng = np.random.default_rng(seed)
    f = lambda a: np.ascontiguousarray(a, np.float32).reshape(-1, 3)  # noqa: E731
    if kind == "lattice16":
        return R.lattice(rng, Q, 64, 16), R.lattice(rng, N, 64, 16)
    if kind == "lattice4":
        return R.lattice(rng, Q, 8, 4), R.lattice(rng, N, 8, 4)
    q = rng.uniform(-1, 1, (Q, 3))
    p = rng.uniform(-1, 1, (N, 3))
    if kind == "planar":
        p[:, 2] = 0.25
        q[:, 2] = 0.25 + 0.01 * rng.normal(size=Q)
    elif kind == "clustered":
        c = rng.uniform(-1, 1, (5, 3))
        p = c[rng.integers(0, 5, N)] + 0.01 * rng.normal(size=(N, 3))
        q = c[rng.integers(0, 5, Q)] + 0.02 * rng.normal(size=(Q, 3))
    elif kind == "duplicates":                 # every point about three times: index ties
        p = p[rng.integers(0, N // 3 + 1, N)] if N else p
    elif kind == "self":                       # queries ARE points (which repeat): distance 0 goes to the smallest index
        p = p[rng.integers(0, N // 2 + 1, N)] if N else p
        q = p[rng.integers(0, N, Q)] if N else q
    elif kind == "coincident":                 # a bounding box of zero extent
        p[:] = (0.3, -0.2, 0.5)
    elif kind == "far":                        # queries outside the points' box: their Morton codes clamp
        q = q * 100.0 + rng.choice([-50.0, 50.0], (Q, 3))
    return f(q), f(p)


def sparse_cross():
    """72 cases: every (Q, N) pair once (8 and 9 are coprime), K and the kind of cloud walking along"""
    out = []
    for i in range(72):
        K = KS[(i + i // 9) % 9]
        N = NS[i % 9]
        N = {"K-1": K - 1, "K": K, "K+1": K + 1}.get(N, N)
        out.append((QS[i % 8], N, K, KINDS[(2 * i + i // 8) % 9]))
    return out


def gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def call(form, q, p, K):
    """one of the two C entry points, directly -> (d2 [Q,K] float32, idx [Q,K] int32) on the GPU"""
    from csplat import native as n
    Q, N, dev = int(q.shape[0]), int(p.shape[0]), q.device
    d2 = torch.full((Q, K), -7.0, dtype=torch.float32, device=dev)
    idx = torch.full((Q, K), -7, dtype=torch.int32, device=dev)
    if form == "brute":
        n.check(n.lib.csplat_knn_query(n.stream_handle(dev), Q, N, K, n.ptr(q), n.ptr(p), n.ptr(d2), n.ptr(idx)), "csplat_knn_query")
    else:
        temp = torch.empty(int(n.lib.csplat_knn_query_temp_bytes(Q, N, K)), dtype=torch.uint8, device=dev)
        n.check(n.lib.csplat_knn_query_ws(n.stream_handle(dev), Q, N, K, n.ptr(q), n.ptr(p), n.ptr(d2), n.ptr(idx), n.ptr(temp)),
                "csplat_knn_query_ws")
    return d2, idx


def test_the_cross_covers_what_it_claims():
    cases = sparse_cross()
    assert {c[0] for c in cases} == set(QS) and {c[2] for c in cases} == set(KS) and {c[3] for c in cases} == set(KINDS)
    ns = {c[1] for c in cases}
    assert {0, 1, 2, 1023, 1024, 1025, 4097} <= ns
    assert any(c[1] == c[2] - 1 for c in cases) and any(c[1] == c[2] for c in cases) and any(c[1] == c[2] + 1 for c in cases)
    assert len({(c[0], NS[i % 9]) for i, c in enumerate(cases)}) == 72


@pytest.mark.parametrize("Q,N,K,kind", sparse_cross(), ids=lambda v: str(v))
def test_both_forms_are_bit_exact_against_the_restatement(Q, N, K, kind):
    q, p = clouds(kind, Q, N, seed=Q * 7 + N * 3 + K)
    rd, ri = R.knn_query(q, p, K)
    tq, tp = gpu(q), gpu(p)
    for form in ("brute", "pruned"):
        d2, idx = call(form, tq, tp, K)
        d2, idx = d2.cpu().numpy(), idx.cpu().numpy()
        assert np.array_equal(idx, ri), f"{form}: indices differ in {(idx != ri).any(1).sum()} rows"
        assert np.array_equal(d2.view(np.uint32), rd.view(np.uint32)), f"{form}: distances differ"


@pytest.mark.parametrize("kind", ["lattice16", "lattice4"])
def test_exact_lattice_equals_float64_brute_force(kind):
    q, p = clouds(kind, 700, 1500, seed=1)
    d64, i64 = R.brute64(q, p, 4)
    for form in ("brute", "pruned"):
        d2, idx = call(form, gpu(q), gpu(p), 4)
        assert np.array_equal(idx.cpu().numpy(), i64)
        assert np.array_equal(d2.cpu().numpy().astype(np.float64), d64)


@pytest.mark.parametrize("K", [1, 8])
@pytest.mark.parametrize("kind", ["uniform", "clustered", "planar", "duplicates", "far", "lattice16"])
def test_pruned_form_equals_brute_form_bit_for_bit(kind, K):
    q, p = clouds(kind, 5000, 20_000, seed=11)
    tq, tp = gpu(q), gpu(p)
    bd, bi = call("brute", tq, tp, K)
    wd, wi = call("pruned", tq, tp, K)
    assert torch.equal(bi, wi)
    assert torch.equal(bd.view(torch.int32), wd.view(torch.int32))
    assert int(bi.min()) >= 0 and int(bi.max()) < 20_000


@pytest.mark.parametrize("K", [1, 8])
@pytest.mark.parametrize("Q", [4095, 8191, 8192, 16_384, 40_000, 70_000, 140_000, 262_143, 262_144, 270_000])
def test_pruned_form_at_every_number_of_queries_a_wave_takes(Q, K):
    """the pruned search gives a wave 1, 2, 4 .. 64 of the queries, the more the more there are (the steps are at Q = 8192 x 2^n);
    whatever the grouping, the bits are the brute-force form's"""
    q, p = clouds("clustered" if K == 1 else "uniform", Q, 3000, seed=Q)
    tq, tp = gpu(q), gpu(p)
    bd, bi = call("brute", tq, tp, K)
    wd, wi = call("pruned", tq, tp, K)
    assert torch.equal(bi, wi)
    assert torch.equal(bd.view(torch.int32), wd.view(torch.int32))


def test_full_size_against_the_kdtree():
    import simple_knn
    from scipy.spatial import cKDTree
    rng = np.random.default_rng(0)
    q, p = rng.uniform(-1, 1, (100_000, 3)).astype(np.float32), rng.uniform(-1, 1, (100_000, 3)).astype(np.float32)
    assert len(p) >= simple_knn.QUERY_BOXED_FROM
    d2, idx = simple_knn.knn_query(gpu(q), gpu(p), 1)
    assert d2.shape == (100_000, 1) and d2.dtype == torch.float32 and idx.dtype == torch.int64 and idx.shape == (100_000, 1)
    dd, ii = cKDTree(p.astype(np.float64)).query(q.astype(np.float64), k=2, workers=16)
    r2 = dd ** 2
    rel = np.abs(d2.cpu().numpy()[:, 0].astype(np.float64) - r2[:, 0]) / r2[:, 0]
    clear = (r2[:, 1] - r2[:, 0]) > 2 * TOL * r2[:, 1]          # float32 cannot reorder those
    wrong = int((idx.cpu().numpy()[clear, 0] != ii[clear, 0]).sum())
    print(f"Q=N=100k K=1 vs cKDTree float64: max rel d2 error {rel.max():.3e} (bound {TOL:.3e}), other indices {wrong}, "
          f"rows left out by the gap rule {1.0 - clear.mean():.5%}")
    assert rel.max() <= TOL
    assert wrong == 0 and clear.mean() >= 1 - 1e-3


def test_find_closest_gauss_equals_the_reference_formulation():
    from csplat.external import find_closest_gauss
    rng = np.random.default_rng(7)
    gt, gauss = rng.normal(size=(600, 3)), rng.normal(size=(5000, 3))
    # float64 argmin
    full = ((gauss[None].astype(np.float32).astype(np.float64) - gt[:, None].astype(np.float32).astype(np.float64)) ** 2).sum(-1)
    two = np.partition(full, 1, axis=1)[:, :2]
    gap = float(((two[:, 1] - two[:, 0]) / two[:, 1]).min())
    print(f"smallest relative gap between a query's two nearest squared distances: {gap:.2e}")
    assert gap > 100 * TOL
    # the reference: gt [N,3] repeated over M, gauss [M,3] repeated over N, argmin over M of the float32 norms
    g32, p32 = gt.astype(np.float32), gauss.astype(np.float32)
    diff = p32[:, None, :].repeat(len(g32), 1) - g32[None, :, :].repeat(len(p32), 0)        # [M, N, 3]
    norms = np.sqrt((diff * diff).sum(-1, dtype=np.float32), dtype=np.float32)
    ref = norms.argmin(0)
    for a, b in ((gt, gauss), (g32, p32), (torch.from_numpy(gt), torch.from_numpy(gauss).cuda()), (torch.from_numpy(g32).cuda(), p32)):
        got = find_closest_gauss(a, b)
        assert isinstance(got, np.ndarray) and got.dtype == np.int64 and got.shape == (600,)
        assert np.array_equal(got, full.argmin(1))
        assert np.array_equal(got, ref)
    assert find_closest_gauss(gt.astype(np.float16), gauss.astype(np.float16)).shape == (600,)


def test_other_stream_and_graph_replay_give_the_eager_bits():
    from csplat import graphs
    q, p = clouds("clustered", 3000, 9000, seed=5)
    tq, tp = gpu(q), gpu(p)

    def run():
        return (*call("brute", tq, tp, 10), *call("pruned", tq, tp, 10), *call("pruned", tq, tp, 1))

    eager = run()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        on_side = run()
    side.synchronize()
    for e, s in zip(eager, on_side):
        assert torch.equal(e, s)
    graph = torch.cuda.CUDAGraph()
    with graphs.capture(graph):
        recorded = run()
    for r in recorded:
        r.zero_()
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    for e, r in zip(eager, recorded):
        assert torch.equal(e, r)
