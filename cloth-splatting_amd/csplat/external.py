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
