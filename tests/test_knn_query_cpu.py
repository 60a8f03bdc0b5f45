"""The two-cloud k-NN (csplat_knn_query / simple_knn.knn_query / csplat.external.find_closest_gauss): everything that can be checked
without a GPU -- the C-ABI surface, argument errors, and the numpy restatement (tests/knn_query_ref.py) against SciPy's KD-tree
and a float64 brute force."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import util
import knn_query_ref as R

NAMES = ("csplat_knn_query", "csplat_knn_query_ws", "csplat_knn_query_temp_bytes", "csplat_chamfer_fwd", "csplat_chamfer_bwd",
         "csplat_chamfer_bwd_temp_bytes")


def test_new_names_are_exported_declared_and_bound():
    from csplat import native
    hdr = open(os.path.join(util.ROOT, "include", "csplat.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = C.CDLL(native.LIB_PATH)
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, code), f"include/csplat.h does not declare {name}"
        assert hasattr(lib, name), f"libcsplat.so does not export {name}"
        assert name in native.EXPORTS, f"csplat.native does not bind {name}"
    assert re.search(r"#define\s+CSPLAT_ABI_VERSION\s+9\b", code)
    assert native.ABI_VERSION == 9 and native.lib.csplat_abi_version() == 9


def test_empty_sizes_and_argument_errors_of_the_entry_points():
    from csplat.native import lib
    err = lambda: lib.csplat_last_error().decode()  # noqa: E731
    # Q = 0 is a no-op, whatever N, with NULL pointers
    for n in (0, 5):
        assert lib.csplat_knn_query(None, 0, n, 3, None, None, None, None) == 0
        assert lib.csplat_knn_query_ws(None, 0, n, 3, None, None, None, None, None) == 0
    # N = 0 with Q > 0 writes (+inf, -1): the outputs are needed, and said so before any launch
    assert lib.csplat_knn_query(None, 4, 0, 3, None, None, None, None) != 0 and "csplat_knn_query: NULL" in err()
    assert lib.csplat_knn_query_ws(None, 4, 0, 3, None, None, None, None, None) != 0 and "csplat_knn_query_ws: NULL" in err()
    assert lib.csplat_knn_query(None, 4, 7, 3, None, None, None, None) != 0 and "csplat_knn_query: NULL" in err()
    for bad_k in (0, 33, -1):
        assert lib.csplat_knn_query(None, 10, 10, bad_k, None, None, None, None) != 0 and "csplat_knn_query: K" in err()
        assert lib.csplat_knn_query_ws(None, 10, 10, bad_k, None, None, None, None, None) != 0 and "csplat_knn_query_ws: K" in err()
    for q, n in ((-1, 10), (10, -1)):
        assert lib.csplat_knn_query(None, q, n, 3, None, None, None, None) != 0 and "csplat_knn_query: bad" in err()
        assert lib.csplat_knn_query_ws(None, q, n, 3, None, None, None, None, None) != 0 and "csplat_knn_query_ws: bad" in err()
    assert lib.csplat_knn_query_temp_bytes(1000, 100_000, 1) >= lib.csplat_knn_temp_bytes(100_000, 1) + 1000 * 12
    # the Chamfer entry points
    assert lib.csplat_chamfer_fwd(None, 0, None, -1.0, None) != 0 and "csplat_chamfer_fwd" in err()
    assert lib.csplat_chamfer_fwd(None, 5, None, -1.0, None) != 0 and "csplat_chamfer_fwd: NULL" in err()
    assert lib.csplat_chamfer_bwd(None, 0, 5, None, None, None, None, -1.0, None, None, None, None) != 0 and "csplat_chamfer_bwd" in err()
    assert lib.csplat_chamfer_bwd(None, 5, 5, None, None, None, None, -1.0, None, None, None, None) != 0 and "csplat_chamfer_bwd: NULL" in err()
    assert lib.csplat_chamfer_bwd_temp_bytes(1000, 10) >= 1000 * 12


def test_python_entry_points_reject_bad_arguments_without_a_device():
    import simple_knn
    from csplat import external, native
    q, p = torch.zeros(5, 3), torch.zeros(10, 3)
    assert isinstance(simple_knn.QUERY_BOXED_FROM, int) and simple_knn.QUERY_BOXED_FROM > 0
    for k in (0, 33, 2.0, True):
        with pytest.raises(ValueError):
            simple_knn.knn_query(q, p, k)
    for bad_q, bad_p in ((torch.zeros(5, 2), p), (q, torch.zeros(10, 4)), (torch.zeros(5, 3, dtype=torch.float64), p),
                         (q, torch.zeros(10, 3, dtype=torch.float64)), (q.numpy(), p), (q, p.numpy()), (torch.zeros(5, 3, device="meta"), p)):
        with pytest.raises(ValueError):
            simple_knn.knn_query(bad_q, bad_p, 3)
    with pytest.raises(native.CsplatError):       # a valid request on CPU tensors: the error simple_knn.knn gives
        simple_knn.knn_query(q, p, 3)
    for gt, gauss in ((np.zeros((5, 2)), np.zeros((10, 3))), (np.zeros((5, 3)), np.zeros((10, 2))), (np.zeros((5, 3)), np.zeros((0, 3))),
                      (np.zeros((5, 3), np.int64), np.zeros((10, 3)))):
        with pytest.raises(ValueError):
            external.find_closest_gauss(gt, gauss)


def test_restatement_equals_ckdtree_in_float64():
    from scipy.spatial import cKDTree
    rng = np.random.default_rng(0)
    q, p = rng.uniform(-1, 1, (700, 3)).astype(np.float32), rng.uniform(-1, 1, (1500, 3)).astype(np.float32)
    d2, idx = R.knn_query(q, p, 8)
    dd, ii = cKDTree(p.astype(np.float64)).query(q.astype(np.float64), k=9)
    r2 = dd ** 2
    assert ((r2[:, 1:] - r2[:, :-1]) > 2 * 8 * 2.0 ** -24 * r2[:, 1:]).all(), "the cloud has near-ties: choose another seed"
    assert np.array_equal(idx, ii[:, :8])
    assert (np.abs(d2 - r2[:, :8]) <= 8 * 2.0 ** -24 * r2[:, :8]).all()
    # fewer than k points: (+inf, -1) from slot N on; no point at all
    d2, idx = R.knn_query(q[:4], p[:3], 5)
    assert np.isinf(d2[:, 3:]).all() and (idx[:, 3:] == -1).all() and (np.sort(idx[:, :3], 1) == np.arange(3)).all()
    d2, idx = R.knn_query(q[:4], p[:0], 2)
    assert np.isinf(d2).all() and (idx == -1).all() and d2.shape == (4, 2)


@pytest.mark.parametrize("span,step", [(64, 16), (8, 4)])
def test_restatement_on_the_exact_lattice_equals_float64_brute_force(span, step):
    rng = np.random.default_rng(1)
    q, p = R.lattice(rng, 700, span, step), R.lattice(rng, 1500, span, step)
    d2, idx = R.knn_query(q, p, 4)
    d64, i64 = R.brute64(q, p, 4)
    assert np.array_equal(idx, i64)
    assert np.array_equal(d2.astype(np.float64), d64)
    tied = float((d2[:, 0] == d2[:, 1]).mean())
    print(f"lattice [-{span}, {span}] / {step}: {tied:.1%} of the queries have a tied first and second neighbour")
    assert tied > (0.005 if step == 16 else 0.5)
