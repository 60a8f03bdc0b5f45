"""Generator of tests/golden/knn_graph.npz: what the reference computes for a kNN graph and for farthest-point sampling.

Run from the repository root, with the reference checkout next to it (REF below or $CSPLAT_REFERENCE):
    python tests/golden/make_knn_golden.py

cloud A (2000 uniform points): the kNN graph of the reference's `compute_edges_index` (meshnet/data_utils.py:406-411) for
k = 3 and 10, recorded as sorted [E,2] int32 pairs.  Its two lines are restated here -- `cKDTree(points).query(points, k=k+1)`,
first column dropped, `{tuple(sorted((i, j)))}` -- instead of calling the function, because under the installed numpy 2.2.6 the
function's own `np.vstack({...})` of a set raises TypeError, and its module imports torch_geometric, h5py and matplotlib,
none of which the graph needs.

cloud B (4000 uniform points): the selection of the reference's `farthest_point_sampling` (meshnet/data_utils.py:134-160),
S = 300, in float64.  The function's source is read from the reference at run time and exec'd (nothing of it is stored), with
np.random.randint pinned to 0 so that the first point is index 0.  Along the run the generator tracks the smallest relative gap
between the best and the second-best distance-to-set (squared): it must stay far above float32 rounding (8 * 2**-24 = 4.8e-7)
for exact index equality to be a fair demand on a float32 implementation; it asserts that and stores the gap."""
import os
import re
import sys

import numpy as np
from scipy.spatial import cKDTree

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("CSPLAT_REFERENCE", os.path.join(os.path.dirname(os.path.dirname(os.path.dirname(HERE))), "reference"))


def knn_graph(points, k):
    _, indices = cKDTree(points).query(points, k=k + 1)
    assert np.array_equal(indices[:, 0], np.arange(len(points))), "first column is not the point itself"
    pairs = {tuple(sorted((i, int(j)))) for i, row in enumerate(indices) for j in row[1:]}
    return np.asarray(sorted(pairs), np.int32)


def reference_fps():
    src = open(os.path.join(REF, "meshnet", "data_utils.py")).read()
    m = re.search(r"^def farthest_point_sampling\(.*?(?=^\S)", src, re.S | re.M)
    ns = {"np": np}
    exec(compile(m.group(0), "data_utils.py:farthest_point_sampling", "exec"), ns)
    return ns["farthest_point_sampling"]


def fps_min_gap(points, sel):
    """smallest relative gap between the largest and second-largest squared distance-to-set over the selections of `sel`"""
    p = points.astype(np.float64)
    dist = np.full(len(p), np.inf)
    gap = np.inf
    for s in range(1, len(sel)):
        dist = np.minimum(dist, ((p - p[sel[s - 1]]) ** 2).sum(1))
        top = np.partition(dist, -2)[-2:]
        assert np.argmax(dist) == sel[s]
        gap = min(gap, (top[1] - top[0]) / top[1])
    return gap


def main():
    out = {}
    a = np.random.default_rng(0).uniform(-1, 1, (2000, 3)).astype(np.float32)
    out["a_points"] = a
    for k in (3, 10):
        out[f"a_edges_k{k}"] = knn_graph(a, k)
    b = np.random.default_rng(0).uniform(-1, 1, (4000, 3)).astype(np.float32)
    fps = reference_fps()
    randint = np.random.randint
    np.random.randint = lambda *args, **kw: 0
    try:
        sel = fps(b.astype(np.float64), 300)
    finally:
        np.random.randint = randint
    gap = fps_min_gap(b, sel)
    assert gap > 60 * 8 * 2.0 ** -24, gap
    out["b_points"] = b
    out["b_fps"] = np.asarray(sel, np.int32)
    out["b_fps_min_rel_gap"] = np.float64(gap)
    path = os.path.join(HERE, "knn_graph.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes; fps gap", gap, {k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    sys.exit(main())
