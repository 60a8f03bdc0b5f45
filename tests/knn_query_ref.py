"""numpy restatement of the two-cloud k-NN semantics of include/csplat.h (csplat_knn_query).  Shares no code with the kernels:
all-pairs float32 distances, formed as knn_ref.sq_dists forms them, and a lexsort by (d2, index)."""
import numpy as np


def sq_dists(queries, points):
    """float32 d2[i, j] = dx*dx + dy*dy + dz*dz with d = points[j] - queries[i], every operation rounded to float32, summed
    left to right"""
    q = np.asarray(queries, np.float32).reshape(-1, 3)
    p = np.asarray(points, np.float32).reshape(-1, 3)
    dx = p[None, :, 0] - q[:, None, 0]
    dy = p[None, :, 1] - q[:, None, 1]
    dz = p[None, :, 2] - q[:, None, 2]
    return (dx * dx + dy * dy) + dz * dz


def knn_query(queries, points, k, chunk=512):
    """(d2 float32 [Q,k], idx int64 [Q,k]): the k nearest points of every query, ascending in (d2, index); nothing is excluded;
    slots r >= N hold (+inf, -1)"""
    q = np.asarray(queries, np.float32).reshape(-1, 3)
    p = np.asarray(points, np.float32).reshape(-1, 3)
    Q, N = q.shape[0], p.shape[0]
    out_d = np.full((Q, k), np.inf, np.float32)
    out_i = np.full((Q, k), -1, np.int64)
    m = min(k, N)
    if m == 0:
        return out_d, out_i
    for lo in range(0, Q, chunk):
        d2 = sq_dists(q[lo:lo + chunk], p)
        kth = np.partition(d2, m - 1, axis=1)[:, m - 1]
        for r in range(d2.shape[0]):
            c = np.flatnonzero(d2[r] <= kth[r])
            c = c[np.lexsort((c, d2[r, c]))][:m]     # last key first: by d2, then by index
            out_d[lo + r, :m] = d2[r, c]
            out_i[lo + r, :m] = c
    return out_d, out_i


def lattice(rng, n, span=64, step=16):
    """n points with coordinates drawn from the integers in [-span, span] divided by `step`: every difference, square and sum of
    the distance is exact in float32 (and in float64), so both arithmetics give the same bits"""
    return (rng.integers(-span, span + 1, (n, 3)) / float(step)).astype(np.float32)


def brute64(queries, points, k):
    """float64 brute force with the (d2, index) rule"""
    q = np.asarray(queries, np.float64).reshape(-1, 3)
    p = np.asarray(points, np.float64).reshape(-1, 3)
    full = ((p[None] - q[:, None]) ** 2).sum(-1)
    ar = np.arange(p.shape[0])
    idx = np.stack([ar[np.lexsort((ar, full[i]))][:k] for i in range(q.shape[0])])
    return np.take_along_axis(full, idx, 1), idx
