"""Drop-in for the neighbour search of the reference's `utils/external.py` (`o3d_knn`, :5-16), which feeds the isometry /
rigidity / spring regularisers: the Open3D KD-tree queried point by point is replaced by the exact k-NN kernels."""
import numpy as np
import torch

import simple_knn


def o3d_knn(pts, num_knn):
    """pts [P,3] (numpy array or tensor, any float type, any device) -> (sq_dists float32 [P,num_knn], indices int64
    [P,num_knn]) as numpy arrays: every point's num_knn nearest other points, nearest first, the point itself left out."""
    if torch.is_tensor(pts):
        t = pts.detach()
    else:
        t = torch.from_numpy(np.ascontiguousarray(pts, np.float32))
    if isinstance(num_knn, (np.integer,)):
        num_knn = int(num_knn)
    t = t.to(torch.float32)
    simple_knn._checked_points(t, num_knn, "o3d_knn")
    d2, idx = simple_knn.knn(t.cuda(), num_knn)
    return d2.cpu().numpy(), idx.cpu().numpy()


def find_closest_gauss(gt, gauss):
    """Drop-in for the reference's `find_closest_gauss` (render.py:123-134): gt [N,3], gauss [M,3] (numpy arrays or tensors, any
    float type, any device) -> int64 numpy array [N], for each `gt` point the index of the nearest `gauss` point.  The reference
    repeats both clouds to [M,N,3] and takes argmin of float32 norms; here the exact two-cloud search runs on squared float32
    distances and a tie goes to the smaller index (argmin's first minimum, but decided before the square root, which can merge
    two different squared distances into one norm)."""
    def as_f32(a, name):
        t = a.detach() if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))
        if not t.is_floating_point():
            raise ValueError(f"find_closest_gauss: `{name}` must be floating point, got {t.dtype}")
        return t.to(torch.float32)
    g, p = as_f32(gt, "gt"), as_f32(gauss, "gauss")
    if p.dim() == 2 and p.shape[0] == 0:
        raise ValueError("find_closest_gauss: `gauss` is empty")
    simple_knn._checked_query(g, p.to(g.device), 1, "find_closest_gauss")
    _d2, idx = simple_knn.knn_query(g.cuda(), p.cuda(), 1)
    return idx[:, 0].cpu().numpy()
