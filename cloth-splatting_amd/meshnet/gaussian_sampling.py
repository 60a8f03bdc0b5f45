"""Drop-in for the reference's `meshnet/gaussian_sampling.py`: the mesh of a cloud and points sampled on its triangles.

  get_mesh(points)          the reference's (:22-47): the Delaunay triangulation of the x and y coordinates on the device
                            (csplat.triangulate.delaunay; the reference runs SciPy and a Python loop over simplices) -> (edges [E,2], each
                            once as i < j and sorted by (i, j) -- the reference's come out of a Python set in arbitrary order --,
                            triangle_vertices [M,3,3] = points[faces]); its `plot` option is not provided
  sample_gaussian_means     the reference's (:6-19): plain tensor arithmetic, no kernel

points: a GPU tensor or a numpy array [N,3] (numpy: the results come back as numpy, the edges int64, the vertices in the input's dtype).
There is no CPU Delaunay: a CPU tensor raises NotImplementedError, as meshnet.data_utils.compute_edges_index(delaunay=True) does."""
import numpy as np
import torch

from csplat import triangulate
from meshnet import data_utils as _du


def get_mesh(points):
    pts = _du._delaunay_points(points, "get_mesh")
    tri = triangulate.delaunay(pts[:, :2].contiguous())
    edges = tri.edge_index.t().contiguous()
    if torch.is_tensor(points):
        return edges, points.detach()[tri.faces.t()]
    return edges.cpu().numpy(), np.asarray(points)[tri.faces.t().cpu().numpy()]


def sample_gaussian_means(triangle_vertices, barycentric_coords, num_samples_per_triangle):
    """triangle_vertices [M,3,3], barycentric_coords [S,M,3] with S = num_samples_per_triangle -> the sampled points [S,M,3]:
    sum over a triangle's vertices of coordinate * vertex.  Tensors or numpy arrays; the result is of the vertices' kind."""
    as_numpy = not torch.is_tensor(triangle_vertices)
    tv = torch.as_tensor(triangle_vertices)
    bc = torch.as_tensor(barycentric_coords).to(device=tv.device, dtype=tv.dtype)
    if tv.dim() != 3 or tuple(tv.shape[1:]) != (3, 3):
        raise ValueError(f"sample_gaussian_means: triangle_vertices is [M,3,3], got {tuple(tv.shape)}")
    if tuple(bc.shape) != (int(num_samples_per_triangle), int(tv.shape[0]), 3):
        raise ValueError(f"sample_gaussian_means: barycentric_coords is [{int(num_samples_per_triangle)},{int(tv.shape[0])},3], got {tuple(bc.shape)}")
    out = (bc[..., None] * tv[None]).sum(dim=-2)
    return out.numpy() if as_numpy else out
