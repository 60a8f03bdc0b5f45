"""k-NN with indices, the kNN cloth graph and farthest-point sampling: everything that can be checked without a GPU -- the C-ABI
surface, argument errors, and the numpy restatement (tests/knn_ref.py) against SciPy's KD-tree and the reference fixtures."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import util
from util import golden
import knn_ref


def cloud_a(P=2000):
    return np.random.default_rng(0).uniform(-1, 1, (P, 3)).astype(np.float32)


def lattice(n=6):
    g = np.arange(n, dtype=np.float32)
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)


def test_knn_and_fps_are_exported_declared_and_bound():
    from csplat import native
    names = ("csplat_knn", "csplat_knn_ws", "csplat_knn_temp_bytes", "csplat_fps")
    hdr = open(os.path.join(util.ROOT, "include", "csplat.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = C.CDLL(native.LIB_PATH)
    for name in names:
        assert re.search(r"\b%s\s*\(" % name, code), f"include/csplat.h does not declare {name}"
        assert hasattr(lib, name), f"libcsplat.so does not export {name}"
        assert name in native.EXPORTS, f"csplat.native does not bind {name}"
    assert re.search(r"#define\s+CSPLAT_KNN_MAX_K\s+32\b", code)
    assert re.search(r"#define\s+CSPLAT_ABI_VERSION\s+9\b", code)
    assert native.ABI_VERSION == 9 and native.lib.csplat_abi_version() == 9
    # host-side parts of the entry points: the workspace size, and argument errors that never reach a launch
    assert native.lib.csplat_knn_temp_bytes(100_000, 10) >= 100_000 * 16
    assert native.lib.csplat_knn(None, 0, 3, None, None, None) == 0          # P = 0 is a no-op
    for bad_k in (0, 33):
        assert native.lib.csplat_knn(None, 10, bad_k, None, None, None) != 0
        assert b"csplat_knn" in native.lib.csplat_last_error()
        assert native.lib.csplat_knn_ws(None, 10, bad_k, None, None, None, None) != 0
    assert native.lib.csplat_knn(None, -1, 3, None, None, None) != 0
    assert native.lib.csplat_fps(None, 10, 0, None, 0, None, None) == 0      # S = 0 is a no-op
    assert native.lib.csplat_fps(None, 10, 5, None, 10, None, None) != 0     # start outside 0 .. N-1
    assert native.lib.csplat_fps(None, 0, 5, None, 0, None, None) != 0


def test_python_entry_points_exist_and_reject_bad_arguments_without_a_device():
    import simple_knn
    from csplat import external, native
    from meshnet import data_utils
    assert simple_knn.MAX_K == 32
    for f in (simple_knn.knn, external.o3d_knn, data_utils.compute_edges_index, data_utils.edges_from_knn,
              data_utils.farthest_point_sampling):
        assert callable(f)
    pts = torch.zeros(10, 3)
    for k in (0, 33):
        with pytest.raises(ValueError):
            simple_knn.knn(pts, k)
        with pytest.raises(ValueError):
            external.o3d_knn(pts.numpy(), k)
        with pytest.raises(ValueError):
            data_utils.compute_edges_index(pts, k=k)
    with pytest.raises(ValueError):
        simple_knn.knn(torch.zeros(10, 2), 3)
    with pytest.raises(ValueError):
        simple_knn.knn(torch.zeros(10, 3, dtype=torch.float64), 3)
    with pytest.raises(ValueError):
        data_utils.compute_edges_index(torch.zeros(10, 2), k=3)
    with pytest.raises(ValueError):
        data_utils.farthest_point_sampling(np.zeros((10, 2), np.float32), 4, start=0)
    with pytest.raises(NotImplementedError, match="SciPy"):
        data_utils.compute_edges_index(pts, k=3, delaunay=True)
    with pytest.raises(native.CsplatError):       # a valid request on a CPU tensor: the error distCUDA2 gives
        simple_knn.knn(pts, 3)


def test_knn_ref_equals_ckdtree_and_a_float64_sort():
    from scipy.spatial import cKDTree
    a = cloud_a()
    d2, idx = knn_ref.knn(a, 16)
    dd, ii = cKDTree(a.astype(np.float64)).query(a.astype(np.float64), k=17)
    assert np.array_equal(ii[:, 0], np.arange(len(a)))
    assert np.array_equal(idx, ii[:, 1:])
    assert np.abs(d2 - dd[:, 1:] ** 2).max() <= 8 * 2.0 ** -24 * (dd[:, 1:] ** 2).max()
    # integer lattice: many exact ties, every distance exact in float32 and in float64
    p = lattice()
    for k in (1, 6, 7, 26, 32):
        d2, idx = knn_ref.knn(p, k)
        p64 = p.astype(np.float64)
        full = ((p64[None] - p64[:, None]) ** 2).sum(-1)
        for i in range(len(p)):
            others = np.delete(np.arange(len(p)), i)
            order = others[np.lexsort((others, full[i, others]))][:k]
            assert np.array_equal(idx[i], order)
            assert np.array_equal(d2[i].astype(np.float64), full[i, order])
    # fewer than k other points: (+inf, -1) from slot P-1 on
    d2, idx = knn_ref.knn(p[:3], 5)
    assert np.isinf(d2[:, 2:]).all() and (idx[:, 2:] == -1).all() and (idx[:, :2] >= 0).all()


@pytest.mark.parametrize("k", [3, 10])
def test_edges_from_knn_equals_the_reference_graph(k):
    from meshnet import data_utils
    g = golden("knn_graph.npz")
    _, idx = knn_ref.knn(g["a_points"], k)
    e = data_utils.edges_from_knn(torch.from_numpy(idx))
    assert e.dtype == torch.long and e.shape[0] == 2 and e.is_contiguous()
    assert np.array_equal(e.numpy(), g[f"a_edges_k{k}"].T.astype(np.int64))
    assert np.array_equal(knn_ref.edges(idx), e.numpy())
    # padded rows (-1) and repeated pairs contribute nothing
    e = data_utils.edges_from_knn(torch.tensor([[1, 2, -1], [0, 2, -1], [0, 1, -1]]))
    assert e.tolist() == [[0, 0, 1], [1, 2, 2]]
    assert data_utils.edges_from_knn(torch.full((1, 3), -1)).shape == (2, 0)


def test_knn_ref_fps_equals_the_reference_selection():
    g = golden("knn_graph.npz")
    assert float(g["b_fps_min_rel_gap"]) > 60 * 8 * 2.0 ** -24
    assert np.array_equal(knn_ref.fps(g["b_points"], 300, 0), g["b_fps"].astype(np.int64))
