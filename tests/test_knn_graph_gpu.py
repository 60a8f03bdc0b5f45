"""k-NN with indices (csplat_knn / csplat_knn_ws), the kNN cloth graph and farthest-point sampling (csplat_fps) on the GPU,
against the numpy restatement tests/knn_ref.py (bit-exact), SciPy's KD-tree in float64 and the reference fixtures."""
import numpy as np
import pytest
import torch

from util import golden
import knn_ref

pytestmark = pytest.mark.gpu

TOL = 8 * 2.0 ** -24   # five float32 roundings (2^-24 each) in dx*dx + dy*dy + dz*dz, rounded up to a power of two


def lattice(P):
    n = int(np.ceil(P ** (1 / 3) - 1e-9))
    while n ** 3 < P:
        n += 1
    g = np.arange(n, dtype=np.float32)
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)[:P].copy()


def cloud(kind, P, seed=5):
    rng = np.random.default_rng(seed)
    if kind == "uniform":
        p = rng.uniform(-1, 1, (P, 3))
    elif kind == "planar":
        p = np.c_[rng.uniform(-1, 1, (P, 2)), np.zeros(P)]
    elif kind == "duplicated":          # every point of the first half appears again in the second, shuffled
        h = rng.uniform(-1, 1, ((P + 1) // 2, 3))
        p = np.concatenate([h, h[:P - len(h)]])[rng.permutation(P)]
    elif kind == "clustered":
        c = rng.uniform(-1, 1, (7, 3))
        p = c[rng.integers(0, 7, P)] + rng.normal(0, 0.01, (P, 3))
    elif kind == "lattice":
        p = lattice(P)
    else:
        raise KeyError(kind)
    return np.ascontiguousarray(p, np.float32).reshape(P, 3)


def gpu(a):
    return torch.tensor(np.asarray(a, np.float32), device="cuda")


class forced:
    """simple_knn.knn (and distCUDA2) made to take one form: brute force or Morton order + boxes"""

    def __init__(self, boxed):
        self.value = 1 if boxed else 1 << 30

    def __enter__(self):
        import simple_knn
        import simple_knn._C as c
        self.old = simple_knn.BOXED_FROM, c.BOXED_FROM
        simple_knn.BOXED_FROM = c.BOXED_FROM = self.value

    def __exit__(self, *exc):
        import simple_knn
        import simple_knn._C as c
        simple_knn.BOXED_FROM, c.BOXED_FROM = self.old


def test_brute_form_is_bit_exact_against_the_restatement():
    import simple_knn
    with forced(boxed=False):
        for kind in ("uniform", "planar", "duplicated", "lattice"):
            for P in (1, 2, 5, 63, 64, 65, 1000, 4095):
                pts = cloud(kind, P)
                t = gpu(pts)
                for K in (1, 3, 10, 16, 32):
                    d2, idx = simple_knn.knn(t, K)
                    assert d2.shape == (P, K) and d2.dtype == torch.float32 and idx.shape == (P, K) and idx.dtype == torch.int64
                    rd, ri = knn_ref.knn(pts, K)
                    assert np.array_equal(idx.cpu().numpy(), ri), (kind, P, K)
                    assert np.array_equal(d2.cpu().numpy().view(np.uint32), rd.view(np.uint32)), (kind, P, K)
                    if P - 1 < K:       # the padding rule
                        assert torch.isinf(d2[:, max(P - 1, 0):]).all() and (idx[:, max(P - 1, 0):] == -1).all()
                        assert (idx[:, :max(P - 1, 0)] >= 0).all()
        for K in (1, 32):               # P = 0
            d2, idx = simple_knn.knn(torch.zeros(0, 3, device="cuda"), K)
            assert d2.shape == (0, K) and idx.shape == (0, K)


def test_small_clouds_agree_in_the_pruned_form_too():
    """the Morton-ordered form at the sizes where a wave's own stretch of the curve, the padding rule and the last ragged box
    matter, against the restatement directly"""
    import simple_knn
    with forced(boxed=True):
        for kind in ("uniform", "duplicated", "lattice"):
            for P in (1, 2, 5, 63, 64, 65, 1000, 1025, 4095):
                pts = cloud(kind, P)
                for K in (1, 3, 10, 32):
                    d2, idx = simple_knn.knn(gpu(pts), K)
                    rd, ri = knn_ref.knn(pts, K)
                    assert np.array_equal(idx.cpu().numpy(), ri), (kind, P, K)
                    assert np.array_equal(d2.cpu().numpy().view(np.uint32), rd.view(np.uint32)), (kind, P, K)


@pytest.mark.parametrize("K", [5, 8])
def test_the_eight_slot_list_in_both_forms_through_the_c_interface(K):
    """K in 5 .. 8 takes KBest<8>, which no K of the two tests above reaches.  Called directly, so that the form does not depend on
    the Python threshold: the brute-force form at P = 1025 and 2051 (two and three slabs, the last one ragged, a tail the four-wide
    loop leaves), the pruned form at P = 1025 and 4099 (two and five boxes, the same tails).  Every row is compared, so the query
    whose own point is the first or the last candidate of a slab or a box is among them."""
    from csplat import native as n
    for P in (1025, 2051, 4099):
        pts = cloud("duplicated" if P == 2051 else "uniform", P, seed=P + K)
        rd, ri = knn_ref.knn(pts, K)
        t = gpu(pts)
        for form in (("brute", "pruned") if P == 1025 else ("brute",) if P == 2051 else ("pruned",)):
            d2 = torch.full((P, K), -7.0, dtype=torch.float32, device="cuda")
            idx = torch.full((P, K), -7, dtype=torch.int32, device="cuda")
            if form == "brute":
                n.check(n.lib.csplat_knn(n.stream_handle(t.device), P, K, n.ptr(t), n.ptr(d2), n.ptr(idx)), "csplat_knn")
            else:
                temp = torch.empty(int(n.lib.csplat_knn_temp_bytes(P, K)), dtype=torch.uint8, device="cuda")
                n.check(n.lib.csplat_knn_ws(n.stream_handle(t.device), P, K, n.ptr(t), n.ptr(d2), n.ptr(idx), n.ptr(temp)), "csplat_knn_ws")
            assert np.array_equal(idx.cpu().numpy(), ri), (form, P, K)
            assert np.array_equal(d2.cpu().numpy().view(np.uint32), rd.view(np.uint32)), (form, P, K)


def test_pruned_form_equals_brute_form_bit_for_bit():
    import simple_knn
    for P in (4096, 20_000, 200_000):
        for kind in ("uniform", "clustered", "planar", "lattice", "duplicated"):
            t = gpu(cloud(kind, P, seed=P))
            for K in (3, 10, 32):
                with forced(boxed=False):
                    bd, bi = simple_knn.knn(t, K)
                with forced(boxed=True):
                    wd, wi = simple_knn.knn(t, K)
                assert torch.equal(wi, bi), (kind, P, K)
                assert torch.equal(wd.view(torch.int32), bd.view(torch.int32)), (kind, P, K)
                assert int(bi.min()) >= 0 and int(bi.max()) < P


def test_k3_row_mean_is_distcuda2_in_both_forms():
    """(d2[0] + d2[1] + d2[2]) / 3.0f, evaluated in IEEE float32 on the host: torch's division of a GPU tensor by a Python
    scalar multiplies by the rounded reciprocal instead, which is not the kernel's expression"""
    import simple_knn
    from simple_knn._C import distCUDA2
    for kind, P in (("uniform", 3000), ("duplicated", 3000), ("lattice", 4096), ("clustered", 50_000)):
        t = gpu(cloud(kind, P))
        for boxed in (False, True):
            with forced(boxed=boxed):
                d2, _ = simple_knn.knn(t, 3)
                ref = distCUDA2(t)
            d = d2.cpu().numpy()
            mean = ((d[:, 0] + d[:, 1]) + d[:, 2]) / np.float32(3.0)
            assert mean.dtype == np.float32 and torch.equal(torch.from_numpy(mean), ref.cpu()), (kind, boxed)


def compare_with_kdtree(points, d2, idx, K, workers=8):
    """float32 k-NN result against SciPy's KD-tree on the same points in float64.  Returns (largest relative d2 error, number
    of rows compared whose indices differ, fraction of rows left out by the gap rule).  A row is compared when every gap
    between consecutive float64 d2 of ranks 1 .. K+1 exceeds 2 TOL (relative to the larger): float32 cannot reorder those."""
    from scipy.spatial import cKDTree
    p64 = np.asarray(points, np.float64)
    dd, ii = cKDTree(p64).query(p64, k=K + 2, workers=workers)
    assert np.array_equal(ii[:, 0], np.arange(len(p64))), "the KD-tree's first column is not the point itself"
    r2 = dd[:, 1:] ** 2                                    # ranks 1 .. K+1
    clear = ((r2[:, 1:] - r2[:, :-1]) > 2 * TOL * r2[:, 1:]).all(1)
    rel = np.abs(np.asarray(d2, np.float64) - r2[:, :K]) / r2[:, :K]
    wrong = int((np.asarray(idx)[clear] != ii[clear, 1:K + 1]).any(1).sum())
    return float(rel.max()), wrong, float(1.0 - clear.mean())


def test_full_size_against_the_kdtree():
    import simple_knn
    pts = np.random.default_rng(0).uniform(-1, 1, (100_000, 3)).astype(np.float32)
    d2, idx = simple_knn.knn(gpu(pts), 10)
    rel, wrong, left_out = compare_with_kdtree(pts, d2.cpu().numpy(), idx.cpu().numpy(), 10)
    print(f"P=100k K=10 vs cKDTree float64: max rel d2 error {rel:.3e} (bound {TOL:.3e}), rows with other indices {wrong}, "
          f"rows left out by the gap rule {left_out:.5%}")
    assert left_out <= 1e-3
    assert rel <= TOL
    assert wrong == 0


def test_o3d_knn_and_the_knn_graph():
    import simple_knn
    from csplat.external import o3d_knn
    from meshnet.data_utils import compute_edges_index
    g = golden("knn_graph.npz")
    a = g["a_points"]
    d2, idx = simple_knn.knn(gpu(a), 7)
    for arg in (a, a.astype(np.float64), torch.from_numpy(a), gpu(a)):
        sq, ii = o3d_knn(arg, 7)
        assert isinstance(sq, np.ndarray) and isinstance(ii, np.ndarray) and sq.shape == (2000, 7) and ii.shape == (2000, 7)
        assert np.array_equal(sq, d2.cpu().numpy()) and np.array_equal(ii, idx.cpu().numpy())
        assert not (ii == np.arange(2000)[:, None]).any()
    for k in (3, 10):
        want = g[f"a_edges_k{k}"].T.astype(np.int64)
        for arg in (a, gpu(a)):
            e = compute_edges_index(arg, k=k)
            assert e.dtype == torch.long and e.shape == want.shape and e.is_cuda and e.is_contiguous()
            assert np.array_equal(e.cpu().numpy(), want)
        assert compute_edges_index(gpu(a), k).device == gpu(a).device


def test_farthest_point_sampling():
    import simple_knn
    from meshnet.data_utils import farthest_point_sampling
    g = golden("knn_graph.npz")
    b = g["b_points"]
    sel = farthest_point_sampling(b, 300, start=0)          # N = 4000: points in registers
    assert isinstance(sel, np.ndarray) and sel.dtype == np.int64 and np.array_equal(sel, g["b_fps"])
    sel = farthest_point_sampling(gpu(b), 300, start=0)
    assert torch.is_tensor(sel) and sel.is_cuda and sel.dtype == torch.long and np.array_equal(sel.cpu().numpy(), g["b_fps"])
    big = cloud("uniform", 20_000, seed=3)                  # N > 8192: points streamed from memory
    assert np.array_equal(farthest_point_sampling(big, 200, start=17), knn_ref.fps(big, 200, 17))
    lat = lattice(1000)                                     # exact ties at every round
    assert np.array_equal(farthest_point_sampling(lat, 64, start=0), knn_ref.fps(lat, 64, 0))
    lat = lattice(9261)
    assert np.array_equal(farthest_point_sampling(lat, 64, start=5), knn_ref.fps(lat, 64, 5))
    small = cloud("uniform", 300, seed=4)                   # S > N: repeats index 0 once every distance is 0
    sel = farthest_point_sampling(small, 500, start=3)
    assert np.array_equal(sel, knn_ref.fps(small, 500, 3)) and (sel[300:] == 0).all() and len(set(sel[:300])) == 300
    np.random.seed(7)
    first = np.random.randint(len(b))
    np.random.seed(7)
    sel = farthest_point_sampling(b, 5)
    assert sel[0] == first and np.array_equal(sel, knn_ref.fps(b, 5, first))
    assert farthest_point_sampling(b[:1], 1, start=0).tolist() == [0]
    assert farthest_point_sampling(b[:1], 3, start=0).tolist() == [0, 0, 0]
    assert farthest_point_sampling(b, 0, start=0).shape == (0,)
    # the work array on return: every point's squared distance to the selected set
    from csplat import native
    t = gpu(b)
    out = torch.empty(300, dtype=torch.int32, device="cuda")
    md = torch.empty(4000, dtype=torch.float32, device="cuda")
    native.check(native.lib.csplat_fps(native.stream_handle(t.device), 4000, 300, native.ptr(t), 0, native.ptr(md), native.ptr(out)), "csplat_fps")
    want = knn_ref.sq_dists(b, g["b_fps"].astype(np.int64)).min(0)
    assert np.array_equal(md.cpu().numpy(), want)
    with pytest.raises(ValueError):
        simple_knn.fps(t, 5, 4000)


def test_other_stream_and_graph_replay_give_the_eager_bits():
    import simple_knn
    from csplat import graphs
    pts = gpu(cloud("clustered", 6000))
    big = gpu(cloud("uniform", 9000))

    def run():
        with forced(boxed=False):
            a = simple_knn.knn(pts, 10)
        with forced(boxed=True):
            b = simple_knn.knn(pts, 10)
        return (*a, *b, simple_knn.fps(pts, 50, 2), simple_knn.fps(big, 50, 2))

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
