"""Observation clouds, the sensing end of the pipeline (csplat_obs_unproject / csplat_obs_voxel / csplat_obs_mark, include/csplat.h): from
what a user has -- depth images, silhouettes and cameras -- to the 3-D data the rest of the library reads.

  unproject_depth    depth images of V views -> Cloud(points, source, view), one launch for all views (the reference's get_world_coords,
                     manipulation/envs/camera_utils.py:106-133, manipulation/deform_mesh.py:168-195)
  voxel_downsample   a cloud -> Voxels(centroids, counts, inverse) on a grid of cubic cells, voxels in ascending (cz, cy, cx)
  observable_nodes   which nodes an observed cloud covers: the k nearest nodes of every cloud point (the reference's
                     get_observable_particle_index, k = 2, and _old, k = 1; camera_utils.py:136-162) -> bool [N]
  camera_points      the cameras' `depth` (and `silhouette` / `mask`) -> the cloud `camera.points` of the Chamfer term expects

Float32 contiguous GPU tensors take the HIP kernels; anything else (CPU tensors, float64) composes the same definitions from torch
operations (reported through csplat.native.composed_fallback for GPU tensors: raises under STRICT; it is the CPU path).  Everything here is
an observation: detached, no gradients.

Two pixel conventions.  This library's renderer puts pixel centres at the integers with the principal point at ((W-1)/2, (H-1)/2); that
is what `cameras=` gives, so tracking.project(unproject_depth(...).points, camera) returns the pixel centres again.  The reference's
get_world_coords puts the principal point at (W/2, H/2) (intrinsic_from_fov): pass explicit `intrinsics` (fx, fy, W/2, H/2) for that."""
import math
from typing import NamedTuple

import numpy as np
import torch

import simple_knn

from . import native as _n

CPU_CHUNK = 1024      # cloud points per [chunk, N] distance matrix of the composed observable_nodes
CELL_BITS = 21        # include/csplat.h: cells lie in [0, 2^21) per axis


class Cloud(NamedTuple):
    points: torch.Tensor        # [M,3] world coordinates, in ascending `source`
    source: torch.Tensor        # [M] int64: the flat pixel index (v * H + y) * W + x -- gather colours or labels with it
    view: torch.Tensor          # [M] int64: v


class Voxels(NamedTuple):
    centroids: torch.Tensor     # [K,3] the mean of each voxel's points, voxels in ascending (cz, cy, cx)
    counts: torch.Tensor        # [K] int32
    inverse: torch.Tensor       # [M] int64: the voxel of each point, -1 for a point with a non-finite coordinate


def _float(a, name, what):
    if isinstance(a, np.ndarray):
        a = torch.from_numpy(np.ascontiguousarray(a))
    if not torch.is_tensor(a):
        raise ValueError(f"{what}: `{name}` is a tensor or numpy array, got {type(a).__name__}")
    if not a.dtype.is_floating_point:
        raise ValueError(f"{what}: `{name}` must be floating point, got {a.dtype}")
    return a.detach()


def _images(images, name, what):
    """[V,H,W], [H,W] or a list of [1,H,W] / [H,W] -> [V,H,W]"""
    if isinstance(images, (list, tuple)):
        if not images:
            raise ValueError(f"{what}: `{name}` is an empty list")
        planes = []
        for im in images:
            t = _float(im, name, what)
            if t.dim() == 3 and t.shape[0] == 1:
                t = t[0]
            if t.dim() != 2:
                raise ValueError(f"{what}: a list `{name}` holds [1,H,W] or [H,W] images, got {tuple(im.shape)}")
            planes.append(t)
        if len({(tuple(t.shape), t.dtype, t.device) for t in planes}) != 1:
            raise ValueError(f"{what}: the images of `{name}` must share one size, dtype and device")
        return torch.stack(planes)
    t = _float(images, name, what)
    if t.dim() == 2:
        t = t[None]
    if t.dim() != 3:
        raise ValueError(f"{what}: `{name}` is [V,H,W], [H,W] or a list of [1,H,W], got {tuple(t.shape)}")
    return t


def camera_intrinsics(camera, H, W):
    """(fx, fy, cx, cy) of a reference-style camera as this library's renderer projects: fx = W / (2 tan(FoVx / 2)), cx = (W - 1) / 2"""
    return (W / (2.0 * math.tan(float(camera.FoVx) * 0.5)), H / (2.0 * math.tan(float(camera.FoVy) * 0.5)), (W - 1) * 0.5, (H - 1) * 0.5)


def camera_to_world(camera):
    """float64 numpy [3,4]: the inverse of the camera's world_view_transform (stored transposed: p_view = [X, 1] @ wvt), on the host"""
    wvt = camera.world_view_transform
    wvt = wvt.detach().cpu().numpy() if torch.is_tensor(wvt) else np.asarray(wvt)
    if wvt.shape != (4, 4):
        raise ValueError(f"unproject_depth: camera.world_view_transform is [4,4], got {wvt.shape}")
    return np.linalg.inv(wvt.astype(np.float64).T)[:3, :4]


def _unproject_composed(D, Mk, K4, C2W, stride, max_depth, kind):
    """the definitions of csplat_obs_unproject from torch operations, in the dtype of the depth"""
    V, H, W = D.shape
    dt, dev = D.dtype, D.device
    sel = torch.isfinite(D) & (D > 0)
    if max_depth > 0.0:
        sel &= D <= torch.tensor(max_depth, dtype=dt, device=dev)
    if Mk is not None:
        sel &= Mk > 0.5
    if stride > 1:
        on_y = (torch.arange(H, device=dev) % stride == 0)[None, :, None]
        on_x = (torch.arange(W, device=dev) % stride == 0)[None, None, :]
        sel &= on_y & on_x
    source = sel.reshape(-1).nonzero()[:, 0]
    view = torch.div(source, H * W, rounding_mode="floor")
    pix = source - view * (H * W)
    y = torch.div(pix, W, rounding_mode="floor")
    x = pix - y * W
    d = D.reshape(-1)[source]
    k, c = K4[view], C2W[view]
    a, b = x.to(dt) - k[:, 2], y.to(dt) - k[:, 3]
    if kind == 0:
        pc = (a * d / k[:, 0], b * d / k[:, 1], d)
    else:
        u, w = a / k[:, 0], b / k[:, 1]
        s = d / torch.sqrt(u * u + w * w + 1.0)
        pc = (u * s, w * s, s)
    points = torch.stack([c[:, r, 0] * pc[0] + c[:, r, 1] * pc[1] + c[:, r, 2] * pc[2] + c[:, r, 3] for r in range(3)], 1)
    return Cloud(points, source, view)


def unproject_depth(depth, *, intrinsics=None, cam_to_world=None, cameras=None, masks=None, stride=1, max_depth=None, kind="z"):
    """Depth images of V views -> Cloud(points [M,3], source [M] int64, view [M] int64), the selected pixels in ascending flat index
    (include/csplat.h, csplat_obs_unproject, states the semantics).
      depth         [V,H,W], [H,W] or a list of [1,H,W]; a hole is 0, negative, NaN or Inf and gives no point
      intrinsics    [V,4] = (fx, fy, cx, cy) in pixel units, pixel centres at the integers   } either these two
      cam_to_world  [V,3,4] or [V,4,4], column-vector form: p_world = R p_cam + t             } ([4] and [3,4] / [4,4]: one for all views)
      cameras       or reference-style cameras (world_view_transform in the transposed convention, FoVx, FoVy), one per view: the matrix
                    is inverted on the host in float64 and the intrinsics are the renderer's, fx = W / (2 tan(FoVx / 2)), cx = (W - 1) / 2
                    -- tracking.project(points, camera) then returns the pixel centres.  The reference's get_world_coords has its
                    principal point at (W / 2, H / 2): pass explicit `intrinsics` for that behaviour
      masks         None, or images like `depth`: a pixel is used where its mask value is > 0.5
      stride        use every stride-th row and column (x % stride == 0 and y % stride == 0)
      max_depth     None (or <= 0): no maximum; else pixels with depth > max_depth give no point
      kind          "z": depth is the view-space z;  "ray": depth is the distance from the camera centre along the pixel's ray
    One blocking read of the count per call.  ValueError before anything touches the device for every malformed argument."""
    what = "unproject_depth"
    D = _images(depth, "depth", what)
    V, H, W = (int(s) for s in D.shape)
    if V < 1 or V > 65535 or H < 1 or W < 1 or V * H * W >= 2 ** 31:
        raise ValueError(f"{what}: `depth` holds 1 to 65535 views of H x W >= 1 x 1 with V * H * W < 2^31, got {(V, H, W)}")
    if kind not in ("z", "ray"):
        raise ValueError(f"{what}: `kind` is \"z\" or \"ray\", got {kind!r}")
    if not isinstance(stride, int) or isinstance(stride, bool) or stride < 1:
        raise ValueError(f"{what}: `stride` is an integer >= 1, got {stride!r}")
    far = 0.0 if max_depth is None else float(max_depth)
    if far != far:
        raise ValueError(f"{what}: `max_depth` is None or a number, got {max_depth!r}")
    dev, dt = D.device, D.dtype
    if cameras is not None:
        if intrinsics is not None or cam_to_world is not None:
            raise ValueError(f"{what}: pass either `cameras` or `intrinsics` and `cam_to_world`, not both")
        cameras = list(cameras)
        if len(cameras) != V:
            raise ValueError(f"{what}: {len(cameras)} cameras for {V} views")
        K4 = torch.tensor([camera_intrinsics(c, H, W) for c in cameras], dtype=torch.float64)
        C2W = torch.from_numpy(np.stack([camera_to_world(c) for c in cameras]))
    else:
        if intrinsics is None or cam_to_world is None:
            raise ValueError(f"{what}: pass `cameras`, or both `intrinsics` [V,4] and `cam_to_world` [V,3,4]")
        K4, C2W = _float(intrinsics, "intrinsics", what), _float(cam_to_world, "cam_to_world", what)
        if K4.dim() == 1:
            K4 = K4[None].expand(V, -1)
        if C2W.dim() == 2:
            C2W = C2W[None].expand(V, -1, -1)
        if tuple(K4.shape) != (V, 4):
            raise ValueError(f"{what}: `intrinsics` is {[V, 4]} (or [4]: one for all views), got {list(intrinsics.shape)}")
        if tuple(C2W.shape) not in ((V, 3, 4), (V, 4, 4)):
            raise ValueError(f"{what}: `cam_to_world` is {[V, 3, 4]} or {[V, 4, 4]} (or one matrix for all views), got {list(cam_to_world.shape)}")
        C2W = C2W[:, :3, :]
    Mk = None
    if masks is not None:
        Mk = _images(masks, "masks", what).to(dev)
        if tuple(Mk.shape) != (V, H, W):
            raise ValueError(f"{what}: `masks` is {[V, H, W]} next to this depth, got {list(Mk.shape)}")
    K4, C2W = K4.to(device=dev, dtype=dt).contiguous(), C2W.to(device=dev, dtype=dt).contiguous()
    if D.is_cuda:
        why = "dtype" if (Mk is not None and Mk.dtype != dt) else _n.why_not_f32c(D, Mk)
        if why is None:
            cap = V * ((H + stride - 1) // stride) * ((W + stride - 1) // stride)
            points = torch.empty(cap, 3, dtype=torch.float32, device=dev)
            source = torch.empty(cap, dtype=torch.int32, device=dev)
            count = torch.empty(1, dtype=torch.int32, device=dev)
            temp = _n.temp(dev, _n.lib.csplat_obs_unproject_temp_bytes(V, H, W))
            _n.launch("csplat_obs_unproject", dev, V, H, W, _n.ptr(D), _n.ptr(Mk), _n.ptr(K4), _n.ptr(C2W), stride, far, 0 if kind == "z" else 1,
                      cap, _n.ptr(points), _n.ptr(source), _n.ptr(count), _n.ptr(temp))
            M = int(count.item())          # the call's one blocking read
            src = source[:M].to(torch.int64)
            return Cloud(points[:M], src, torch.div(src, H * W, rounding_mode="floor"))
        _n.composed_fallback("observation.unproject_depth", why, D)
    return _unproject_composed(D, None if Mk is None else Mk.to(dt), K4, C2W, stride, far, 0 if kind == "z" else 1)


def _points(points, name, what):
    if isinstance(points, Cloud):
        points = points.points
    elif isinstance(points, Voxels):
        points = points.centroids
    P = _float(points, name, what)
    if P.dim() != 2 or P.shape[1] != 3:
        raise ValueError(f"{what}: `{name}` is [n,3], got {tuple(P.shape)}")
    return P


def _voxel_composed(P, voxel, origin):
    """the definitions of csplat_obs_voxel from torch operations, in the dtype of the points -> (Voxels, points outside the cell range)"""
    M, dt, dev = P.shape[0], P.dtype, P.device
    finite = torch.isfinite(P).all(1)
    if origin is None:
        origin = P[finite].min(0).values if bool(finite.any()) else torch.zeros(3, dtype=dt, device=dev)
    size = torch.tensor(voxel, dtype=dt, device=dev)
    cell = torch.floor((P - origin[None]) / size)
    inside = finite & ((cell >= 0) & (cell < float(1 << CELL_BITS))).all(1)
    rows = inside.nonzero()[:, 0]
    c = cell[rows].to(torch.int64)
    key = (c[:, 2] << (2 * CELL_BITS)) | (c[:, 1] << CELL_BITS) | c[:, 0]
    keys, inv, counts = torch.unique(key, return_inverse=True, return_counts=True)
    cells = torch.stack([keys & ((1 << CELL_BITS) - 1), (keys >> CELL_BITS) & ((1 << CELL_BITS) - 1), keys >> (2 * CELL_BITS)], 1)
    corner = origin[None] + cells.to(dt) * size
    sums = torch.zeros(keys.shape[0], 3, dtype=dt, device=dev).index_add_(0, inv, P[rows] - corner[inv])
    inverse = torch.full((M,), -1, dtype=torch.int64, device=dev)
    inverse[rows] = inv
    return Voxels(corner + sums / counts.to(dt)[:, None], counts.to(torch.int32), inverse), int((finite & ~inside).sum())


def voxel_downsample(points, voxel_size, *, origin=None):
    """A cloud [M,3] (or a Cloud) on a grid of cubic cells of edge `voxel_size` -> Voxels(centroids [K,3], counts [K] int32, inverse [M]
    int64) (include/csplat.h, csplat_obs_voxel).  Per axis the cell is floor((p - origin) / voxel_size) in float32; `origin` [3] is None for
    the per-axis minimum over the finite points.  Voxels come in ascending (cz, cy, cx); a centroid is the mean of its voxel's points; a
    point with a non-finite coordinate belongs to no voxel (inverse -1).  Bit-reproducible on the GPU.  One blocking read, of K and the
    number of points outside the grid's 2^21 cells per axis: any such finite point raises ValueError (choose a larger voxel_size or an
    origin nearer the cloud)."""
    what = "voxel_downsample"
    P = _points(points, "points", what)
    size = float(voxel_size)
    if not (size > 0.0 and size < math.inf):
        raise ValueError(f"{what}: `voxel_size` is a finite number > 0, got {voxel_size!r}")
    M, dev, dt = int(P.shape[0]), P.device, P.dtype
    if M >= 2 ** 31:
        raise ValueError(f"{what}: at most 2^31 - 1 points, got {M}")
    O = None
    if origin is not None:
        O = torch.as_tensor(origin).detach().to(torch.float64).reshape(-1)
        if O.shape[0] != 3 or not bool(torch.isfinite(O).all()):
            raise ValueError(f"{what}: `origin` is None or three finite numbers, got {origin!r}")
        O = O.to(device=dev, dtype=dt)
    if M == 0:
        return Voxels(P.new_zeros(0, 3), torch.zeros(0, dtype=torch.int32, device=dev), torch.zeros(0, dtype=torch.int64, device=dev))
    vox = None
    if P.is_cuda:
        why = _n.why_not_f32c(P)
        if why is None:
            centroid = torch.empty(M, 3, dtype=torch.float32, device=dev)
            count = torch.empty(M, dtype=torch.int32, device=dev)
            inverse = torch.empty(M, dtype=torch.int32, device=dev)
            counters = torch.empty(2, dtype=torch.int32, device=dev)
            temp = _n.temp(dev, _n.lib.csplat_obs_voxel_temp_bytes(M))
            _n.launch("csplat_obs_voxel", dev, M, _n.ptr(P), size, _n.ptr(O), _n.ptr(centroid), _n.ptr(count), _n.ptr(inverse),
                      counters[0:].data_ptr(), counters[1:].data_ptr(), _n.ptr(temp))
            K, outside = counters.tolist()          # the call's one blocking read
            vox = Voxels(centroid[:K].clone(), count[:K].clone(), inverse.to(torch.int64))
        else:
            _n.composed_fallback("observation.voxel_downsample", why, P)
    if vox is None:
        vox, outside = _voxel_composed(P, size, O)
    if outside:
        raise ValueError(f"{what}: {outside} finite points lie outside the grid's 2^{CELL_BITS} cells per axis from the origin; choose a larger "
                         "`voxel_size` or an `origin` nearer the cloud (no coordinate may lie below the origin)")
    return vox


def _observable_composed(C, X, k, cap):
    """the k nearest nodes of every cloud point on squared distances in the clouds' dtype (the arithmetic of csplat_knn_query: d = node -
    point, dx dx + dy dy + dz dz), ties to the smaller index"""
    flags = torch.zeros(X.shape[0], dtype=torch.bool, device=X.device)
    for lo in range(0, C.shape[0], CPU_CHUNK):
        d = X[None, :, :] - C[lo:lo + CPU_CHUNK, None, :]
        d2 = d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]
        near, idx = torch.sort(d2, dim=1, stable=True)
        near, idx = near[:, :k], idx[:, :k]
        flags[idx[near <= cap] if cap >= 0.0 else idx.reshape(-1)] = True
    return flags


def observable_nodes(cloud, nodes, *, k=2, max_dist=None):
    """Which of the N `nodes` [N,3] an observed `cloud` [Q,3] (or a Cloud / Voxels) covers -> bool [N]: node n is observable iff it is
    among the k nearest nodes of some cloud point (exact; squared float32 distances, ties to the smaller index) and, with `max_dist`, within
    that distance of it.  k = 2 is the reference's get_observable_particle_index ("each point in the point cloud will cover at most two
    particles"), k = 1 its _old form; both return np.unique of the indices, this returns the flags (flags.nonzero() is that index list).
    On the GPU: simple_knn's two-cloud search and one csplat_obs_mark launch, no host read.  1 <= k <= min(N, simple_knn.MAX_K).
    The result suits `node_weights` of meshnet.mpc.candidate_costs after .float()."""
    what = "observable_nodes"
    C, X = _points(cloud, "cloud", what), _points(nodes, "nodes", what)
    N, Q = int(X.shape[0]), int(C.shape[0])
    if not isinstance(k, int) or isinstance(k, bool) or not 1 <= k <= min(N, simple_knn.MAX_K):
        raise ValueError(f"{what}: k is an integer in 1 .. min(N, {simple_knn.MAX_K}) = {min(N, simple_knn.MAX_K)}, got {k!r}")
    cap = -1.0
    if max_dist is not None:
        cap = float(max_dist)
        if not cap >= 0.0:
            raise ValueError(f"{what}: max_dist is None or >= 0, got {max_dist!r}")
        cap = cap * cap
    if C.device != X.device:
        raise ValueError(f"{what}: the cloud is on {C.device}, the nodes on {X.device}")
    if Q * k >= 2 ** 31:
        raise ValueError(f"{what}: Q * k must stay below 2^31, got {Q} * {k}")
    if X.is_cuda:
        why = "dtype" if C.dtype != X.dtype else _n.why_not_f32c(C, X)
        if why is None:
            dev = X.device
            d2, idx = simple_knn._knn_query_i32(C, X, k)
            flags = torch.empty(N, dtype=torch.uint8, device=dev)
            _n.launch("csplat_obs_mark", dev, Q, k, N, _n.ptr(idx), _n.ptr(d2), cap, _n.ptr(flags))
            return flags.view(torch.bool)
        _n.composed_fallback("observation.observable_nodes", why, X)
    return _observable_composed(C.to(X.dtype), X, k, cap)


def camera_points(cameras, *, voxel_size=None, stride=1, max_depth=None, kind="z"):
    """The observed cloud of reference-style cameras -> [M,3]: every camera's `depth` image ([1,H,W] or [H,W], one size) unprojected with
    the camera's own pose and field of view, all views in one launch; where a camera has a `silhouette`, and otherwise where it has a
    `mask`, that image is the mask (> 0.5) -- a camera with neither uses every valid pixel.  With `voxel_size` the merged cloud is thinned
    to its voxels' centroids.  The result is what the Chamfer term of csplat.train.train_step reads as `camera.points`."""
    what = "camera_points"
    cameras = list(cameras)
    if not cameras:
        raise ValueError(f"{what}: `cameras` is empty")
    for c in cameras:
        if getattr(c, "depth", None) is None:
            raise ValueError(f"{what}: every camera needs a `depth` image")
    depth = _images([c.depth for c in cameras], "camera.depth", what)
    fields = [getattr(c, "silhouette", None) if getattr(c, "silhouette", None) is not None else getattr(c, "mask", None) for c in cameras]
    masks = None
    if any(f is not None for f in fields):
        ones = torch.ones_like(depth[0])
        masks = _images([ones if f is None else f.to(device=depth.device, dtype=depth.dtype) for f in fields], "camera.silhouette", what)
    cloud = unproject_depth(depth, cameras=cameras, masks=masks, stride=stride, max_depth=max_depth, kind=kind)
    if voxel_size is None:
        return cloud.points
    return voxel_downsample(cloud.points, voxel_size).centroids
