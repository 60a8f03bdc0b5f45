"""Drop-in for the graph-building part of the reference's `meshnet/data_utils.py`: the kNN graph of `compute_edges_index`
(:371-414) and `farthest_point_sampling` (:134-160), on the GPU kernels of `simple_knn`.  The Delaunay branch, the PyG
`Data` builders and the trajectory loaders of that file are host-side plumbing and stay out of scope."""
import numpy as np
import torch

import simple_knn


def _gpu_points(points, what):
    """numpy array or tensor [N,3] -> float32 tensor on the GPU (shape errors before the device is touched)"""
    t = points.detach() if torch.is_tensor(points) else torch.from_numpy(np.ascontiguousarray(points))
    if t.dim() != 2 or t.shape[1] != 3:
        raise ValueError(f"{what}: points must be [N, 3], got {tuple(t.shape)}")
    return t.to(torch.float32).cuda() if not t.is_cuda else t.to(torch.float32)


def edges_from_knn(indices):
    """indices [P,k] (row i: the neighbours of point i; negative entries = no neighbour) -> the unique undirected pairs
    (i, j), i < j, as a torch.long [2,E] tensor sorted by (i, j), on the device of `indices`.  (The reference collects the same
    pairs in a Python set, whose order is arbitrary.)"""
    idx = torch.as_tensor(indices).to(torch.long)
    if idx.dim() != 2:
        raise ValueError(f"edges_from_knn: indices must be [P, k], got {tuple(idx.shape)}")
    P = int(idx.shape[0])
    own = torch.arange(P, dtype=torch.long, device=idx.device).unsqueeze(1).expand_as(idx)
    keep = (idx >= 0) & (idx != own)
    lo, hi = torch.minimum(own, idx)[keep], torch.maximum(own, idx)[keep]
    key = torch.unique(lo * P + hi)   # sorted
    return torch.stack((torch.div(key, max(P, 1), rounding_mode="floor"), key % max(P, 1))).contiguous()


def compute_edges_index(points, k=3, delaunay=False, sim_data=False, norm_threshold=0.01):
    """the kNN graph of the reference's function: every point joined to its k nearest other points, each undirected edge
    once.  points: numpy array or tensor [N,3].  Returns torch.long [2,E], sorted by (i, j), on the GPU (on the input's
    device for a GPU tensor).  `sim_data` and `norm_threshold` belong to the Delaunay branch."""
    if delaunay:
        raise NotImplementedError("compute_edges_index(delaunay=True) is host geometry (scipy.spatial.Delaunay in the reference) "
                                  "and is not provided here; build those edges with SciPy")
    if isinstance(k, np.integer):
        k = int(k)
    if not isinstance(k, int) or isinstance(k, bool) or not 1 <= k <= simple_knn.MAX_K:
        raise ValueError(f"compute_edges_index: k must be an integer in 1 .. {simple_knn.MAX_K}, got {k!r}")
    _d2, idx = simple_knn.knn(_gpu_points(points, "compute_edges_index"), k)
    return edges_from_knn(idx)


def farthest_point_sampling(points, num_samples, start=None):
    """the reference's farthest-point sampling on the GPU: indices of `num_samples` points, each the farthest from those
    already chosen.  points: numpy array or tensor [N,3]; the indices come back in the same kind (numpy int64 array, or
    torch.long tensor on the GPU).  start=None draws the first point with np.random.randint(len(points)) exactly as the
    reference does, so a seeded script selects the same first point."""
    if start is None:
        start = np.random.randint(len(points))
    sel = simple_knn.fps(_gpu_points(points, "farthest_point_sampling"), int(num_samples), int(start))
    return sel if torch.is_tensor(points) else sel.cpu().numpy()
