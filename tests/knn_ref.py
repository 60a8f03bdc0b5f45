"""numpy restatement of the k-NN / kNN-graph / farthest-point-sampling semantics of include/csplat.h (csplat_knn, csplat_fps).
Shares no code with the kernels: all-pairs float32 distances and a sort."""
import numpy as np


def sq_dists(points, rows):
    """float32 d2[r, j] = dx*dx + dy*dy + dz*dz with d = points[j] - points[rows[r]], every operation rounded to float32,
    summed left to right"""
    p = np.asarray(points, np.float32)
    q = p[rows]
    dx = p[None, :, 0] - q[:, None, 0]
    dy = p[None, :, 1] - q[:, None, 1]
    dz = p[None, :, 2] - q[:, None, 2]
    return (dx * dx + dy * dy) + dz * dz


def knn(points, k, chunk=512):
    """(d2 float32 [P,k], idx int64 [P,k]): the k nearest other points of every point, ascending in (d2, index); the point
    itself is excluded by index; slots r >= P-1 hold (+inf, -1)"""
    p = np.asarray(points, np.float32).reshape(-1, 3)
    P = p.shape[0]
    out_d = np.full((P, k), np.inf, np.float32)
    out_i = np.full((P, k), -1, np.int64)
    m = min(k, P - 1)
    if m <= 0:
        return out_d, out_i
    for lo in range(0, P, chunk):
        rows = np.arange(lo, min(P, lo + chunk))
        d2 = sq_dists(p, rows)
        others = d2.copy()
        others[np.arange(len(rows)), rows] = np.inf
        kth = np.partition(others, m - 1, axis=1)[:, m - 1]
        for r, i in enumerate(rows):
            c = np.flatnonzero(others[r] <= kth[r])
            c = c[c != i]
            c = c[np.lexsort((c, d2[r, c]))][:m]     # last key first: by d2, then by index
            out_d[i, :m] = d2[r, c]
            out_i[i, :m] = c
    return out_d, out_i


def edges(indices):
    """[P,k] neighbour indices (negative = none) -> int64 [2,E]: the unique undirected pairs (i, j), i < j, sorted by (i, j)"""
    pairs = sorted({(min(i, int(j)), max(i, int(j))) for i, row in enumerate(np.asarray(indices)) for j in row if j >= 0 and j != i})
    return np.asarray(pairs, np.int64).reshape(-1, 2).T


def fps(points, num_samples, start):
    """farthest-point sampling in float32 squared distances; argmax takes the first of equal maxima"""
    p = np.asarray(points, np.float32).reshape(-1, 3)
    sel = np.zeros(num_samples, np.int64)
    if num_samples == 0:
        return sel
    sel[0] = start
    dist = np.full(len(p), np.inf, np.float32)
    for s in range(1, num_samples):
        dist = np.minimum(dist, sq_dists(p, [sel[s - 1]])[0])
        sel[s] = np.argmax(dist)
    return sel
