"""Drop-in for the `simple_knn` package (reference import: scene_reconstruction/gaussian_mesh.py:26)."""
import torch

from csplat import native as _n

MAX_K = 32          # include/csplat.h: CSPLAT_KNN_MAX_K
BOXED_FROM = 4096   # below this the single brute-force kernel is faster than sort + boxes (the threshold of distCUDA2)


def _checked_points(points, k, what):
    """argument errors are raised before anything touches the device"""
    if not isinstance(k, int) or isinstance(k, bool) or not 1 <= k <= MAX_K:
        raise ValueError(f"{what}: k must be an integer in 1 .. {MAX_K}, got {k!r}")
    if not torch.is_tensor(points) or points.dim() != 2 or points.shape[1] != 3:
        raise ValueError(f"{what}: points must be a [P, 3] tensor, got {tuple(getattr(points, 'shape', ()))}")
    if points.dtype != torch.float32:
        raise ValueError(f"{what}: points must be float32, got {points.dtype}")


def knn(points: torch.Tensor, k: int):
    """points [P,3] float32 on the GPU -> (sq_dists float32 [P,k], indices int64 [P,k]): the k nearest OTHER points of every
    point (self excluded by index, so coincident points are neighbours at distance 0), ascending in (sq_dist, index).  Exact:
    ties go to the smaller index; rows with fewer than k other points end in (+inf, -1).  For k = 3 the row mean is
    bit-identical to `simple_knn._C.distCUDA2`."""
    _checked_points(points, k, "simple_knn.knn")
    _n.require_cuda(points)
    pts = points.detach().contiguous()
    P, dev = int(pts.shape[0]), pts.device
    d2 = torch.empty(P, k, dtype=torch.float32, device=dev)
    idx = torch.empty(P, k, dtype=torch.int32, device=dev)
    if P >= BOXED_FROM:   # Morton order + box pruning; the same bits and indices
        temp = _n.temp(dev, _n.lib.csplat_knn_temp_bytes(P, k))
        _n.launch("csplat_knn_ws", dev, P, k, _n.ptr(pts), _n.ptr(d2), _n.ptr(idx), _n.ptr(temp))
    else:
        _n.launch("csplat_knn", dev, P, k, _n.ptr(pts), _n.ptr(d2), _n.ptr(idx))
    return d2, idx.to(torch.int64)


def fps(points: torch.Tensor, num_samples: int, start: int):
    """points [N,3] float32 on the GPU -> int64 [num_samples] farthest-point-sampling indices beginning at `start`: every
    further index is the point farthest (squared distance, float32) from those already chosen, the smallest index among
    equal maxima.  num_samples > N repeats indices as the reference's loop does."""
    if not torch.is_tensor(points) or points.dim() != 2 or points.shape[1] != 3 or points.dtype != torch.float32:
        raise ValueError(f"simple_knn.fps: points must be a float32 [N, 3] tensor, got {getattr(points, 'dtype', None)} "
                         f"{tuple(getattr(points, 'shape', ()))}")
    N, S = int(points.shape[0]), int(num_samples)
    if S < 0 or (S > 0 and not 0 <= int(start) < N):
        raise ValueError(f"simple_knn.fps: need num_samples >= 0 and 0 <= start < N, got num_samples={S}, start={start}, N={N}")
    _n.require_cuda(points)
    pts = points.detach().contiguous()
    dev = pts.device
    out = torch.empty(S, dtype=torch.int32, device=dev)
    min_d2 = torch.empty(max(N, 1), dtype=torch.float32, device=dev)
    _n.launch("csplat_fps", dev, N, S, _n.ptr(pts), int(start) if S else 0, _n.ptr(min_d2), _n.ptr(out))
    return out.to(torch.int64)


# knn_query: from this many POINTS on the Morton-ordered form (csplat_knn_query_ws) is taken.  Measured: profiles/knn_query_cost.txt
# (tools/knn_query_cost.py; N in {1k, 4k, 16k, 100k} x Q in {1k, 16k, 100k} x K in {1, 8}) -- the smallest N of the table from which the
# pruned form wins at every Q and K of the table.  At N = 16k it wins for K = 8 (x 1.5 .. 1.8) but loses for K = 1 at Q >= 16k
# (0.95 against 0.82 ms at Q = 16k, 1.05 against 0.83 at Q = 100k); at N = 100k it wins everywhere, x 2.4 .. 3.7.  No condition on Q: at N = 100k the order is the same at every Q.
QUERY_BOXED_FROM = 100_000


def _checked_query(queries, points, k, what):
    """argument errors of a two-cloud search, raised before anything touches the device"""
    _checked_points(points, k, what)
    if not torch.is_tensor(queries) or queries.dim() != 2 or queries.shape[1] != 3:
        raise ValueError(f"{what}: queries must be a [Q, 3] tensor, got {tuple(getattr(queries, 'shape', ()))}")
    if queries.dtype != torch.float32:
        raise ValueError(f"{what}: queries must be float32, got {queries.dtype}")
    if queries.device != points.device:
        raise ValueError(f"{what}: queries are on {queries.device}, points on {points.device}")


def _knn_query_i32(qry, pts, k, boxed=None):
    """(d2 float32 [Q,k], idx int32 [Q,k]) of checked, detached, contiguous GPU clouds; boxed: None = by QUERY_BOXED_FROM"""
    Q, N, dev = int(qry.shape[0]), int(pts.shape[0]), pts.device
    d2 = torch.empty(Q, k, dtype=torch.float32, device=dev)
    idx = torch.empty(Q, k, dtype=torch.int32, device=dev)
    if boxed is None:
        boxed = N >= QUERY_BOXED_FROM
    if boxed:   # Morton order + box pruning; the same bits and indices
        temp = _n.temp(dev, _n.lib.csplat_knn_query_temp_bytes(Q, N, k))
        _n.launch("csplat_knn_query_ws", dev, Q, N, k, _n.ptr(qry), _n.ptr(pts), _n.ptr(d2), _n.ptr(idx), _n.ptr(temp))
    else:
        _n.launch("csplat_knn_query", dev, Q, N, k, _n.ptr(qry), _n.ptr(pts), _n.ptr(d2), _n.ptr(idx))
    return d2, idx


def knn_query(queries: torch.Tensor, points: torch.Tensor, k: int):
    """queries [Q,3], points [N,3], float32 on one GPU -> (sq_dists float32 [Q,k], indices int64 [Q,k]): the k nearest of `points`
    to every query, ascending in (sq_dist, index).  Nothing is excluded: a query that coincides with a point finds it at distance
    0.  Exact: ties go to the smaller index; rows with fewer than k points end in (+inf, -1)."""
    _checked_query(queries, points, k, "simple_knn.knn_query")
    _n.require_cuda(queries, points)
    d2, idx = _knn_query_i32(queries.detach().contiguous(), points.detach().contiguous(), k)
    return d2, idx.to(torch.int64)
