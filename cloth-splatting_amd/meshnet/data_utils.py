"""Drop-in for the reference's `meshnet/data_utils.py`, on the GPU kernels of this library.

Graph builders: the kNN graph of `compute_edges_index` (:371-414) and `farthest_point_sampling` (:134-160), on `simple_knn`; its
`delaunay=True` branch (:372-405, the default of every MeshNet script) and `compute_mesh` (:419-440) on csplat.triangulate, the Delaunay
triangulation on the device (include/csplat.h, "Delaunay triangulation": cocircular points are resolved by its tie rule, not by Qhull).

Trajectory preprocessing, the step between an observed / tracked cloud and the planner (include/csplat.h, "Trajectory preprocessing"):
  smooth_clouds / gaussian_smoothing   the reference's gaussian_smoothing (:267-278) for one cloud [N,3] or all frames [T,N,3] of a tracked
                        cloud in ONE launch of csplat_traj_smooth -- the reference loops over frames and points in Python, one KD-tree
                        query each.  Brute force per frame, O(T N^2): made for tracked clouds of hundreds to a few thousand points; the
                        Morton-pruned search per frame is not built (profiles/trajectory_cost.txt shows from which N that hurts)
  compute_edge_features, trajectory_features   velocities and per-frame edge features of all frames in one launch of csplat_traj_features.
                        displacement = points[edge_index[1]] - points[edge_index[0]]: the sign of the reference's compute_edge_features
                        (:443-448), the OPPOSITE of meshnet.rollout.edge_features
  process_traj          the reference's dictionary (:282-367) with the reference's shapes, as tensors
  get_data_traj         its `observations=` path (:165-236): gripper point, smoothing, z = 0, actions, grasped node
  expand_init_data, flip_trajectory    as the reference's

Dispatch as in csplat.observation: float32 contiguous GPU tensors take the HIP kernels; anything else composes the same definitions from
torch operations in the input's dtype (reported through csplat.native.composed_fallback for GPU tensors: raises under STRICT; it is the
CPU path).  A numpy array goes to the GPU as float32 when there is one, else the composed CPU path runs in its own dtype; the result comes
back as numpy in the input's dtype, like farthest_point_sampling.  Everything here is an observation: detached, no gradients.

The samples a training step reads are assembled from these dictionaries by meshnet.dataloader_sim (SamplesClothSimDataset), which stands
in for the PyG `Data` builders.  The file loaders of that module are host-side plumbing and stay out of scope.  There is no CPU Delaunay:
a CPU tensor with delaunay=True raises NotImplementedError (use SciPy there); a numpy array goes to the GPU when there is one."""
import math

import numpy as np
import torch

import simple_knn
from csplat import native as _n

CPU_CHUNK = 1024      # points per [chunk, N] distance matrix of the composed smoothing
FLT_MAX = 3.4028234663852886e38


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


def _delaunay_points(points, what):
    """numpy array or tensor [N,3] for the Delaunay branch -> float32 tensor on the GPU.  Shape errors come first; a CPU tensor, and a
    numpy array on a machine without a GPU, raise NotImplementedError: there is no CPU Delaunay here"""
    t = points.detach() if torch.is_tensor(points) else torch.from_numpy(np.ascontiguousarray(points))
    if t.dim() != 2 or t.shape[1] != 3:
        raise ValueError(f"{what}: points must be [N, 3], got {tuple(t.shape)}")
    if not t.is_cuda and (torch.is_tensor(points) or not torch.cuda.is_available()):
        raise NotImplementedError(f"{what}(delaunay=True) triangulates on the GPU (csplat.triangulate.delaunay) and has no CPU form; for "
                                  "points that live on the host build the edges and faces with SciPy (scipy.spatial.Delaunay, as the "
                                  "reference does) and pass them in")
    return t.to(torch.float32).cuda() if not t.is_cuda else t.to(torch.float32)


def compute_edges_index(points, k=3, delaunay=False, sim_data=False, norm_threshold=0.01):
    """delaunay=False: the kNN graph of the reference's function: every point joined to its k nearest other points, each undirected edge
    once.  points: numpy array or tensor [N,3].  Returns torch.long [2,E], sorted by (i, j), on the GPU (on the input's device for a GPU
    tensor).
    delaunay=True: (edge_index, faces) as the reference's -- the Delaunay triangulation of the points projected on [:, [0, 2]] with
    sim_data, else on [:, :2]; an edge of a face longer than norm_threshold (None: no limit) is left out and spoils its face.  edge_index
    [2,E] each edge once, i < j, sorted by (i, j); faces [3,M], lowest index first, counter-clockwise in the projection, sorted.  Both
    torch.long on the GPU, straight from csplat.triangulate.delaunay (which states the rule for cocircular points).  A GPU tensor that is
    not float32 is converted; a numpy array goes to the GPU; a CPU tensor raises NotImplementedError."""
    if delaunay:
        from csplat import triangulate
        what = "compute_edges_index"
        thr = triangulate.checked_threshold(norm_threshold, what)
        pts = _delaunay_points(points, what)
        tri = triangulate.delaunay(pts[:, [0, 2]] if sim_data else pts[:, :2].contiguous(), thr)
        return tri.edge_index, tri.faces
    if isinstance(k, np.integer):
        k = int(k)
    if not isinstance(k, int) or isinstance(k, bool) or not 1 <= k <= simple_knn.MAX_K:
        raise ValueError(f"compute_edges_index: k must be an integer in 1 .. {simple_knn.MAX_K}, got {k!r}")
    _d2, idx = simple_knn.knn(_gpu_points(points, "compute_edges_index"), k)
    return edges_from_knn(idx)


def compute_mesh(points):
    """the reference's compute_mesh (:419-440): the Delaunay triangulation of the x and y coordinates of points [N,3] as a
    SimpleNamespace(pos, face [3,M], edge_index, norm) -- edge_index = face_to_edge(face, N) (PyG's FaceToEdge), norm the unit vertex
    normals of GenerateMeshNormals as csplat.gaussians.mesh_vertex_normals forms them.  The reference joggles the input (Qhull's QJ) so
    that cocircular points give some triangulation; here the tie rule of csplat_delaunay gives one, the same on every run.  pos is the
    input as given when it is a float32 GPU tensor."""
    import types
    from csplat import triangulate
    from csplat.gaussians import mesh_vertex_normals
    from meshnet.dataloader_sim import face_to_edge
    pts = _delaunay_points(points, "compute_mesh")
    face = triangulate.delaunay(pts[:, :2].contiguous()).faces
    return types.SimpleNamespace(pos=pts, face=face, edge_index=face_to_edge(face, int(pts.shape[0])), norm=mesh_vertex_normals(pts, face))


def farthest_point_sampling(points, num_samples, start=None):
    """the reference's farthest-point sampling on the GPU: indices of `num_samples` points, each the farthest from those
    already chosen.  points: numpy array or tensor [N,3]; the indices come back in the same kind (numpy int64 array, or
    torch.long tensor on the GPU).  start=None draws the first point with np.random.randint(len(points)) exactly as the
    reference does, so a seeded script selects the same first point."""
    if start is None:
        start = np.random.randint(len(points))
    sel = simple_knn.fps(_gpu_points(points, "farthest_point_sampling"), int(num_samples), int(start))
    return sel if torch.is_tensor(points) else sel.cpu().numpy()


# ------------------------------------------------------------------------------------------------------------ trajectory preprocessing
class _Kind:
    """how an argument came in, and how results go back: a tensor stays a tensor on its device; a numpy array is worked on as float32 on
    the GPU when there is one (else on the CPU in its own dtype) and comes back as numpy (`tensors`: as a CPU tensor) in its own dtype"""

    def __init__(self, a, name, what):
        self.numpy = isinstance(a, np.ndarray)
        if self.numpy:
            a = torch.from_numpy(np.ascontiguousarray(a))
        if not torch.is_tensor(a):
            raise ValueError(f"{what}: `{name}` is a tensor or numpy array, got {type(a).__name__}")
        if not a.dtype.is_floating_point:
            raise ValueError(f"{what}: `{name}` must be floating point, got {a.dtype}")
        self.dtype, self.raw = a.dtype, a.detach()

    def work(self):
        """the tensor to compute on -- the first thing that may touch the device: call it after every check of the arguments"""
        if self.numpy and torch.cuda.is_available():
            return self.raw.to(torch.float32).cuda()
        return self.raw

    def back(self, t, tensors=False):
        if t is None or not self.numpy:
            return t
        t = t.cpu()
        if t.dtype.is_floating_point:
            t = t.to(self.dtype)
        return t if tensors else t.numpy()


def _checked_k(k, what):
    if isinstance(k, np.integer):
        k = int(k)
    if not isinstance(k, int) or isinstance(k, bool) or not 1 <= k <= simple_knn.MAX_K:
        raise ValueError(f"{what}: k must be an integer in 1 .. {simple_knn.MAX_K}, got {k!r}")
    return k


def _clouds(kind, name, what):
    """[N,3] or [T,N,3] -> (T, N, single)"""
    shape = tuple(kind.raw.shape)
    if len(shape) not in (2, 3) or shape[-1] != 3:
        raise ValueError(f"{what}: `{name}` is [N,3] or [T,N,3], got {shape}")
    return (1 if len(shape) == 2 else shape[0]), shape[-2], len(shape) == 2


def weight_scale(sigma, dtype):
    """c of w = exp(-(d2 * c)) as csplat_traj_smooth states it: 1 / (2 sigma^2) in double -- for float32 from the float32 sigma, rounded
    once to float32 and limited to FLT_MAX"""
    if dtype == torch.float32:
        s = float(np.float32(sigma))
        return float(np.float32(min(1.0 / (2.0 * s * s), FLT_MAX)))
    return 1.0 / (2.0 * float(sigma) * float(sigma))


def _smooth_composed(P, k, sigma):
    """the definitions of csplat_traj_smooth from torch operations, in the dtype of the points -> (out, d2 [T,N,k], idx int64 [T,N,k])"""
    T, N, _ = P.shape
    dt, dev = P.dtype, P.device
    c = weight_scale(sigma, dt)
    inf = torch.tensor(math.inf, dtype=dt, device=dev)
    out = P.clone()
    d2o = torch.full((T, N, k), math.inf, dtype=dt, device=dev)
    idxo = torch.full((T, N, k), -1, dtype=torch.int64, device=dev)
    kk = min(k, N)
    for t in range(T):
        X = P[t]
        for lo in range(0, N, CPU_CHUNK):
            Q = X[lo:lo + CPU_CHUNK]
            d = X[None, :, :] - Q[:, None, :]
            d2 = d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]
            d2 = torch.where(torch.isfinite(d2), d2, inf)          # a non-finite distance: nobody's neighbour
            near, idx = torch.sort(d2, dim=1, stable=True)         # ascending (d2, index)
            near, idx = near[:, :kk], idx[:, :kk]
            filled = torch.isfinite(near)
            w = torch.exp(-(near * c))
            nb = X[idx]                                            # [chunk, kk, 3]
            acc, sw = w[:, 0, None] * nb[:, 0], w[:, 0]            # the sum begins with its first term
            for j in range(1, kk):
                acc = torch.where(filled[:, j, None], acc + w[:, j, None] * nb[:, j], acc)
                sw = torch.where(filled[:, j], sw + w[:, j], sw)
            whole = torch.isfinite(Q).all(1)                       # a point with a non-finite coordinate goes through unchanged
            out[t, lo:lo + CPU_CHUNK] = torch.where(whole[:, None], acc / sw[:, None], Q)
            d2o[t, lo:lo + CPU_CHUNK, :kk] = near
            idxo[t, lo:lo + CPU_CHUNK, :kk] = torch.where(filled, idx, torch.full_like(idx, -1))
    return out, d2o, idxo


def smooth_clouds(points, k=20, sigma=0.1, return_neighbours=False):
    """Gaussian-weighted mean of every point's k nearest points of its own frame, the point itself included (include/csplat.h,
    csplat_traj_smooth, states the semantics: ascending (squared float32 distance, index), w = exp(-d2 / (2 sigma^2)), summed in that order;
    a point with a non-finite coordinate is nobody's neighbour and comes back unchanged).  points: [N,3] or [T,N,3], tensor or numpy; the
    smoothed cloud comes back in the same shape and kind, with `return_neighbours` also (d2 [..,N,k], idx int64 [..,N,k]; rows with fewer
    than k neighbours end in (+inf, -1)).  On the GPU all T frames are ONE launch, bit-reproducible.  Brute force per frame: for tracked
    clouds of hundreds to a few thousand points.  1 <= k <= simple_knn.MAX_K, sigma finite and > 0, T * N * k < 2^31."""
    what = "smooth_clouds"
    kind = _Kind(points, "points", what)
    T, N, single = _clouds(kind, "points", what)
    k = _checked_k(k, what)
    try:
        sg = float(sigma)
    except (TypeError, ValueError):
        raise ValueError(f"{what}: sigma is a finite number > 0, got {sigma!r}") from None
    if not (sg > 0.0 and sg < math.inf):
        raise ValueError(f"{what}: sigma is a finite number > 0, got {sigma!r}")
    if T * N * k >= 2 ** 31:
        raise ValueError(f"{what}: T * N * k must stay below 2^31, got {T} * {N} * {k}")
    if kind.dtype == torch.float32 or (kind.numpy and torch.cuda.is_available()):       # the float32 forms take sigma as a float32 number
        with np.errstate(over="ignore"):
            s32 = float(np.float32(sg))
        if not (s32 > 0.0 and s32 < math.inf):
            raise ValueError(f"{what}: sigma must be a finite float32 number > 0, got {sigma!r}")
    P = kind.work().reshape(T, N, 3)
    res = None
    if P.is_cuda and T * N > 0:
        why = _n.why_not_f32c(P)
        if why is None:
            dev = P.device
            out = torch.empty_like(P)
            d2 = torch.empty(T, N, k, dtype=torch.float32, device=dev) if return_neighbours else None
            idx = torch.empty(T, N, k, dtype=torch.int32, device=dev) if return_neighbours else None
            _n.launch("csplat_traj_smooth", dev, T, N, k, _n.ptr(P), sg, _n.ptr(out), _n.ptr(d2), _n.ptr(idx))
            res = (out, d2, None if idx is None else idx.to(torch.int64))
        else:
            _n.composed_fallback("data_utils.smooth_clouds", why, P)
    if res is None:
        res = _smooth_composed(P, k, sg)
    shape = (N,) if single else (T, N)
    out = kind.back(res[0].reshape(*shape, 3))
    if not return_neighbours:
        return out
    return out, kind.back(res[1].reshape(*shape, k)), kind.back(res[2].reshape(*shape, k))


def gaussian_smoothing(point_cloud, k=20, sigma=0.1):
    """the reference's name and signature for one cloud [N,3]; [T,N,3] is accepted too and replaces its Python loop over frames"""
    return smooth_clouds(point_cloud, k=k, sigma=sigma)


def _edges_form(edge_index, what):
    """[2,E] integers, tensor or numpy -> a detached tensor (type and shape errors: nothing touches the device)"""
    if isinstance(edge_index, np.ndarray):
        edge_index = torch.from_numpy(np.ascontiguousarray(edge_index))
    if not torch.is_tensor(edge_index) or edge_index.dtype.is_floating_point or edge_index.dtype in (torch.bool, torch.complex64, torch.complex128):
        raise ValueError(f"{what}: `edge_index` is an integer tensor or numpy array [2,E], got {getattr(edge_index, 'dtype', type(edge_index).__name__)}")
    if edge_index.dim() != 2 or edge_index.shape[0] != 2:
        raise ValueError(f"{what}: `edge_index` is [2,E], got {tuple(edge_index.shape)}")
    return edge_index.detach()


def _checked_edges(edge_index, N, device, what):
    """[2,E] integers -> contiguous int64 on `device`, entries inside 0 .. N-1 (one blocking read)"""
    ei = _edges_form(edge_index, what).to(device=device, dtype=torch.int64).contiguous()
    if ei.shape[1]:
        lo, hi = torch.stack((ei.min(), ei.max())).tolist()          # the one blocking read
        if lo < 0 or hi >= N:
            raise ValueError(f"{what}: `edge_index` entries must lie in 0 .. N-1 = {N - 1}, got {lo} .. {hi}")
    return ei


def _features(P, ei, inv_dt, want_vel, want_edges):
    """P [T,N,3], ei int64 [2,E] on one device -> (vel [T,N,3] | None, disp [T,E,3] | None, norm [T,E,1] | None)"""
    T, N, _ = P.shape
    E, dev, dt = int(ei.shape[1]), P.device, P.dtype
    if P.is_cuda:
        why = _n.why_not_f32c(P)
        if why is None:
            vel = torch.zeros(T, N, 3, dtype=dt, device=dev) if want_vel else None
            disp = torch.empty(T, E, 3, dtype=dt, device=dev) if want_edges else None
            norm = torch.empty(T, E, 1, dtype=dt, device=dev) if want_edges else None
            _n.launch("csplat_traj_features", dev, T, N, E, _n.ptr(P), _n.ptr(ei), inv_dt, _n.ptr(vel), _n.ptr(disp), _n.ptr(norm))
            return vel, disp, norm
        _n.composed_fallback("data_utils.trajectory_features", why, P)
    vel = disp = norm = None
    if want_vel:
        scale = float(np.float32(inv_dt)) if dt == torch.float32 else inv_dt
        vel = torch.zeros_like(P)
        vel[1:] = (P[1:] - P[:-1]) * scale
    if want_edges:
        disp = P[:, ei[1]] - P[:, ei[0]]
        norm = torch.sqrt(disp[..., 0] * disp[..., 0] + disp[..., 1] * disp[..., 1] + disp[..., 2] * disp[..., 2])[..., None]
    return vel, disp, norm


def _inv_dt(dt, what):
    try:
        v = float(dt)
    except (TypeError, ValueError):
        raise ValueError(f"{what}: dt is a finite number other than 0, got {dt!r}") from None
    with np.errstate(over="ignore"):
        ok = math.isfinite(v) and v != 0.0 and math.isfinite(float(np.float32(1.0 / v)))
    if not ok:
        raise ValueError(f"{what}: dt is a finite number other than 0 (and 1 / dt a float32 number), got {dt!r}")
    return 1.0 / v


def compute_edge_features(points, edge_index):
    """(displacement, norm) of every edge: displacement = points[edge_index[1]] - points[edge_index[0]] -- the reference's sign (receiver
    minus sender), the OPPOSITE of meshnet.rollout.edge_features -- and norm its Euclidean length.  [N,3] -> ([E,3], [E,1]), the
    reference's signature; [T,N,3] -> ([T,E,3], [T,E,1]), every frame in one launch.  edge_index [2,E] integers in 0 .. N-1."""
    what = "compute_edge_features"
    kind = _Kind(points, "points", what)
    T, N, single = _clouds(kind, "points", what)
    edge_index = _edges_form(edge_index, what)
    if T * N >= 2 ** 31 or T * int(edge_index.shape[1]) >= 2 ** 31:
        raise ValueError(f"{what}: T * N and T * E must stay below 2^31")
    P = kind.work().reshape(T, N, 3)
    ei = _checked_edges(edge_index, N, P.device, what)
    _v, disp, norm = _features(P, ei, 1.0, False, True)
    if single:
        disp, norm = disp[0], norm[0]
    return kind.back(disp), kind.back(norm)


def trajectory_features(traj, edge_index, dt):
    """traj [T,N,3], edge_index [2,E], dt -> (velocity [T,N,3], displacement [T,E,3], norm [T,E,1]), straight from csplat_traj_features:
    velocity[0] = 0, velocity[t] = (traj[t] - traj[t-1]) * (1 / dt); displacement and norm as compute_edge_features (the reference's sign,
    the opposite of meshnet.rollout.edge_features).  One launch for all frames; edge_index entries are range-checked (one blocking read)."""
    what = "trajectory_features"
    kind = _Kind(traj, "traj", what)
    if kind.raw.dim() != 3 or kind.raw.shape[2] != 3:
        raise ValueError(f"{what}: `traj` is [T,N,3], got {tuple(kind.raw.shape)}")
    T, N = int(kind.raw.shape[0]), int(kind.raw.shape[1])
    inv = _inv_dt(dt, what)
    edge_index = _edges_form(edge_index, what)
    if T * N >= 2 ** 31 or T * int(edge_index.shape[1]) >= 2 ** 31:
        raise ValueError(f"{what}: T * N and T * E must stay below 2^31")
    P = kind.work()
    ei = _checked_edges(edge_index, N, P.device, what)
    vel, disp, norm = _features(P, ei, inv, True, True)
    return kind.back(vel), kind.back(disp), kind.back(norm)


def process_traj(traj, dt, k=3, delaunay=False, subsample=False, num_samples=300, sim_data=False, norm_threshold=0.01,
                 sampled_points_indeces=None, edge_index=None, faces=None):
    """The reference's process_traj: traj [T,N,3] -> its dictionary with its shapes (S = the sampled points), every value a tensor on the
    input's device (a numpy input: CPU tensors in its dtype):
      pos [T,S,3]  velocity [T,S,3]  node_type [T,S,1] (zeros)  edge_index [T,2,E] (an expanded view of one [2,E])
      edge_displacement [T,E,3]  edge_norm [T,E,1]  edge_faces (None without `faces`, else `faces` expanded over T)  sampled_point_indeces [S]
    Kept from the reference: T = 1 gives one frame with zero velocity; for T > 1 frame 0's edge features are a COPY OF FRAME 1's (it inserts
    element 0 of a list that starts at frame 1); with sim_data the edges whose frame-1 norm is >= norm_threshold are pruned, in stable
    order.  Deliberately different: that prune mask is applied ONCE (the reference applies it twice and raises IndexError whenever an
    edge is actually pruned; once is the same result whenever it does not crash), and faces=None gives edge_faces None (the reference
    cannot stack None).  Subsampling is farthest_point_sampling, a missing edge_index comes from compute_edges_index (both need the GPU);
    with delaunay=True a missing edge_index comes with its faces from the triangulation of frame 0's sampled nodes
    (compute_edges_index(delaunay=True, sim_data, norm_threshold)), and edge_faces is those faces [T,3,M]; an explicit edge_index wins,
    as in the reference.  There is no CPU Delaunay: a CPU tensor that needs one raises NotImplementedError.  The displacement's sign is
    the reference's: see compute_edge_features."""
    what = "process_traj"
    kind = _Kind(traj, "traj", what)
    if kind.raw.dim() != 3 or kind.raw.shape[2] != 3 or kind.raw.shape[0] < 1:
        raise ValueError(f"{what}: `traj` is [T,N,3] with T >= 1, got {tuple(kind.raw.shape)}")
    T, N = int(kind.raw.shape[0]), int(kind.raw.shape[1])
    inv = _inv_dt(dt, what)
    try:
        thr = float(norm_threshold)
    except (TypeError, ValueError):
        raise ValueError(f"{what}: norm_threshold is a number, got {norm_threshold!r}") from None
    if thr != thr:
        raise ValueError(f"{what}: norm_threshold is a number, got {norm_threshold!r}")
    if edge_index is None:
        _checked_k(k, what)
    else:
        edge_index = _edges_form(edge_index, what)
    sel = None
    if sampled_points_indeces is not None:
        sel = torch.as_tensor(sampled_points_indeces)
        if sel.dim() != 1 or sel.dtype.is_floating_point or sel.dtype == torch.bool:
            raise ValueError(f"{what}: `sampled_points_indeces` is a 1-D integer array, got {sel.dtype} {tuple(sel.shape)}")
        if sel.numel() and (int(sel.min()) < 0 or int(sel.max()) >= N):
            raise ValueError(f"{what}: `sampled_points_indeces` entries must lie in 0 .. N-1 = {N - 1}")
    elif subsample and (not isinstance(num_samples, (int, np.integer)) or isinstance(num_samples, bool) or int(num_samples) < 1):
        raise ValueError(f"{what}: num_samples is an integer >= 1, got {num_samples!r}")
    if delaunay and edge_index is None and not kind.raw.is_cuda and not (kind.numpy and torch.cuda.is_available()):
        raise NotImplementedError("process_traj(delaunay=True) triangulates on the GPU and has no CPU form; for a trajectory that lives on "
                                  "the host pass `edge_index` (and `faces`) built with SciPy (scipy.spatial.Delaunay, as the reference does)")
    P = kind.work()
    dev = P.device
    if sel is None:
        sel = farthest_point_sampling(P[0], int(num_samples)) if subsample else torch.arange(N, device=dev)
    sel = sel.to(device=dev, dtype=torch.int64)
    pos = P[:, sel].contiguous()
    S = int(sel.shape[0])
    if edge_index is None:
        if delaunay:
            edge_index, faces = compute_edges_index(pos[0], k=k, delaunay=True, sim_data=sim_data, norm_threshold=thr)
        else:
            edge_index = compute_edges_index(pos[0], k=k)
    ei = _checked_edges(edge_index, S, dev, what)
    vel, disp, norm = _features(pos, ei, inv, True, True)
    first = min(1, T - 1)                                   # the frame whose edge features stand for frame 0 as well
    if sim_data:
        keep = norm[first, :, 0] < thr                      # applied once
        ei, disp, norm = ei[:, keep].contiguous(), disp[:, keep].contiguous(), norm[:, keep].contiguous()
    if T > 1:
        disp[0].copy_(disp[1])
        norm[0].copy_(norm[1])
    E = int(ei.shape[1])
    edge_faces = None
    if faces is not None:
        f = torch.as_tensor(faces).detach().to(dev)
        edge_faces = f[None].expand(T, *f.shape)
    b = lambda t: kind.back(t, tensors=True)  # noqa: E731
    return {"pos": b(pos), "velocity": b(vel), "node_type": b(torch.zeros(T, S, 1, dtype=pos.dtype, device=dev)),
            "edge_index": b(ei)[None].expand(T, 2, E), "edge_displacement": b(disp), "edge_norm": b(norm),
            "edge_faces": b(edge_faces), "sampled_point_indeces": b(sel)}


def expand_init_data(data, input_length_sequence):
    """the reference's: the first element of `data` (tensor or numpy) repeated in front, input_length_sequence - 1 times"""
    n = int(input_length_sequence) - 1
    if n <= 0:
        return data
    if isinstance(data, torch.Tensor):
        return torch.cat([data[0:1]] * n + [data], 0)
    return np.concatenate([data[0:1]] * n + [data], 0)


def flip_trajectory(traj, load_keys):
    """the reference's: swaps the y and z columns of the positional entries of `traj` that are in `load_keys` (in place; returns traj)"""
    for key in ("pos", "vel", "actions", "gripper_pos", "pick", "place"):
        if key in load_keys:
            v = traj[key]
            traj[key] = v[:, [0, 2, 1]] if v.ndim == 2 else (v[:, :, [0, 2, 1]] if v.ndim == 3 else v[[0, 2, 1]])
    return traj


GRIPPER_OFFSET = (0.0, -0.03, 0.02)     # the gripper point the reference appends to every frame: gripper_pos + this


def get_data_traj(data_path, load_keys, params, observations=None, sim_data=False, sampled_points_indices=None, rw_processing=True):
    """The reference's get_data_traj for `observations=` (a dict with pos [T,N,3], gripper_pos [T,3], pick [3], place [3], and actions
    [T,3] unless rw_processing makes them); loading `data_path` from a file is out of scope and raises NotImplementedError.
    params = (dt, k, delaunay, subsample, num_samples, input_length_sequence, action_steps).  Without sim_data and with rw_processing, as
    the reference: the gripper point gripper_pos + (0, -0.03, 0.02) is appended to every frame, the actions are ones in frame 0 and
    gripper differences from then on, all frames are smoothed (k = 20, sigma = 0.1) in ONE launch, and z is set to zero.  With sim_data the
    y and z columns are swapped first (flip_trajectory).  Then process_traj(..., sim_data=False, norm_threshold=0.1), the reference's action
    shift (actions[0] = 0), gripper_pos / gripper_vel / pick / place, the grasped node -- the node nearest to `pick` in frame 0
    (simple_knn.knn_query, k = 1, on the GPU; ties to the smaller index like np.argmin), its node_type set to 1 -- and expand_init_data
    for input_length_sequence > 1.  Every value is a tensor on the device of `pos` (numpy observations: CPU tensors in the dtype of `pos`);
    grasped_particle is an int."""
    what = "get_data_traj"
    if observations is None:
        raise NotImplementedError("get_data_traj: only the `observations=` path is provided; loading a trajectory file (`data_path`) is "
                                  "host-side plumbing and out of scope")
    try:
        dt, k, delaunay, subsample, num_samples, input_length_sequence, _action_steps = params
    except (TypeError, ValueError):
        raise ValueError(f"{what}: params is (dt, k, delaunay, subsample, num_samples, input_length_sequence, action_steps)") from None
    inv = _inv_dt(dt, what)
    need = ["pos", "gripper_pos", "pick", "place"] + ([] if (rw_processing and not sim_data) else ["actions"])
    for key in need:
        if key not in observations:
            raise ValueError(f"{what}: observations lack `{key}`")
    kind = _Kind(observations["pos"], "pos", what)
    if kind.raw.dim() != 3 or kind.raw.shape[2] != 3 or kind.raw.shape[0] < 1 or kind.raw.shape[1] < 1:
        raise ValueError(f"{what}: observations['pos'] is [T,N,3] with T, N >= 1, got {tuple(kind.raw.shape)}")
    T = int(kind.raw.shape[0])
    shapes = {"gripper_pos": (T, 3), "pick": (3,), "place": (3,), "actions": (T, 3)}
    raw = {}
    for key in need[1:]:
        v = _Kind(observations[key], key, what).raw
        if tuple(v.shape) != shapes[key]:
            raise ValueError(f"{what}: observations['{key}'] is {list(shapes[key])} next to this pos, got {list(v.shape)}")
        raw[key] = v
    traj = kind.work()
    dev, dtp = traj.device, traj.dtype
    data = {key: v.to(device=dev, dtype=dtp) for key, v in raw.items()}
    if sim_data:
        data["pos"] = traj
        data = flip_trajectory(data, list(data.keys()))
        traj = data.pop("pos")
    elif rw_processing:
        grip = data["gripper_pos"] + torch.tensor(GRIPPER_OFFSET, dtype=dtp, device=dev)
        traj = torch.cat([traj, grip[:, None, :]], 1).contiguous()
        actions = torch.ones_like(data["gripper_pos"])
        actions[1:] = data["gripper_pos"][1:] - data["gripper_pos"][:-1]
        data["actions"] = actions
        traj = smooth_clouds(traj, k=min(20, simple_knn.MAX_K), sigma=0.1)
        traj[:, :, 2] = 0
    out = process_traj(traj.contiguous(), dt, k, delaunay, subsample=subsample, num_samples=num_samples, sim_data=False, norm_threshold=0.1,
                       sampled_points_indeces=sampled_points_indices)
    out["actions"] = torch.cat([torch.zeros_like(data["actions"][:1]), data["actions"][1:]], 0)
    out["gripper_pos"] = data["gripper_pos"]
    gv = torch.zeros_like(data["gripper_pos"])
    gv[1:] = (data["gripper_pos"][1:] - data["gripper_pos"][:-1]) * (float(np.float32(inv)) if dtp == torch.float32 else inv)
    out["gripper_vel"] = gv
    out["pick"], out["place"] = data["pick"], data["place"]
    nodes0 = out["pos"][0]
    if nodes0.is_cuda and _n.why_not_f32c(nodes0) is None:
        _d2, near = simple_knn.knn_query(data["pick"][None].contiguous(), nodes0.contiguous(), 1)
        grasped = int(near[0, 0])
    else:
        if nodes0.is_cuda:
            _n.composed_fallback("data_utils.get_data_traj", _n.why_not_f32c(nodes0), nodes0)
        d = nodes0 - data["pick"][None]
        grasped = int(torch.argmin(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]))   # (the first of equal minima)
    out["node_type"][:, grasped] = 1
    out["grasped_particle"] = grasped
    if int(input_length_sequence) > 1:
        for key in ("actions", "pos", "velocity", "gripper_pos", "gripper_vel", "node_type", "edge_index", "edge_displacement", "edge_norm"):
            out[key] = expand_init_data(out[key], input_length_sequence)
    if kind.numpy:
        out = {key: (kind.back(v, tensors=True) if torch.is_tensor(v) else v) for key, v in out.items()}
    return out
