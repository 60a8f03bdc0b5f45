"""numpy restatement of csplat.observation (include/csplat.h: csplat_obs_unproject, csplat_obs_voxel, csplat_obs_mark), in float64 and
in float32.  The float32 form restates the pixel SELECTION and the CELL of every point exactly (each operation one float32 rounding, in
the kernels' order); its centroid sum is sequential in sorted order, the kernel's a fixed tree -- values are compared by the rule of
tests/test_train_kernels_gpu.py:check().  The float64 form takes selection and cells from the float32 arithmetic (they are decisions of
the float32 data) and evaluates every value in float64."""
import numpy as np

CELL_BITS = 21
F32, F64 = np.float32, np.float64


def select(depth, mask=None, stride=1, max_depth=0.0):
    """bool [V,H,W]: the selected pixels of float32 depth images"""
    d = np.asarray(depth, F32)
    V, H, W = d.shape
    with np.errstate(invalid="ignore"):
        sel = np.isfinite(d) & (d > 0)
        if max_depth > 0.0:
            sel &= d <= F32(max_depth)
        if mask is not None:
            sel &= np.asarray(mask, F32) > F32(0.5)
    if stride > 1:
        sel &= (np.arange(H) % stride == 0)[None, :, None] & (np.arange(W) % stride == 0)[None, None, :]
    return sel


def unproject(depth, intrinsics, cam_to_world, mask=None, stride=1, max_depth=0.0, kind=0, dtype=F32):
    """-> (points [M,3] dtype, source [M] int64, view [M] int64); the inputs are float32 data, widened for dtype = float64"""
    d32 = np.asarray(depth, F32)
    V, H, W = d32.shape
    source = np.flatnonzero(select(d32, mask, stride, max_depth).reshape(-1)).astype(np.int64)
    view = source // (H * W)
    y, x = (source % (H * W)) // W, source % W
    d = d32.reshape(-1)[source].astype(dtype)
    k = np.asarray(intrinsics, F32).astype(dtype)[view]
    c = np.asarray(cam_to_world, F32).astype(dtype)[:, :3, :][view]
    a, b = x.astype(dtype) - k[:, 2], y.astype(dtype) - k[:, 3]
    if kind == 0:
        pc = (a * d / k[:, 0], b * d / k[:, 1], d)
    else:
        u, w = a / k[:, 0], b / k[:, 1]
        s = d / np.sqrt(u * u + w * w + dtype(1.0))
        pc = (u * s, w * s, s)
    points = np.stack([((c[:, r, 0] * pc[0] + c[:, r, 1] * pc[1]) + c[:, r, 2] * pc[2]) + c[:, r, 3] for r in range(3)], 1)
    assert points.dtype == dtype
    return points, source, view


def cells(points, voxel, origin=None):
    """the float32 cell arithmetic -> (cell [M,3] int64, has_cell [M] bool, finite [M] bool, origin float32 [3])"""
    p = np.asarray(points, F32)
    finite = np.isfinite(p).all(1)
    if origin is None:
        origin = p[finite].min(0) if finite.any() else np.zeros(3, F32)
    o = np.asarray(origin, F32)
    with np.errstate(invalid="ignore", over="ignore"):
        c = np.floor((p - o[None]) / F32(voxel))
        assert c.dtype == F32
        inside = finite & ((c >= 0) & (c < F32(1 << CELL_BITS))).all(1)
    return np.where(inside[:, None], c, 0).astype(np.int64), inside, finite, o


def voxel(points, voxel_size, origin=None, dtype=F32):
    """-> dict(centroids [K,3] dtype, counts [K] int32, inverse [M] int64, outside int, keys [K] int64)"""
    p32 = np.asarray(points, F32)
    M = p32.shape[0]
    c, inside, finite, o = cells(p32, voxel_size, origin)
    key = (c[:, 2] << (2 * CELL_BITS)) | (c[:, 1] << CELL_BITS) | c[:, 0]
    rows = np.flatnonzero(inside)
    order = rows[np.argsort(key[rows], kind="stable")]                       # by (key, index)
    skey = key[order]
    head = np.ones(len(order), bool)
    head[1:] = skey[1:] != skey[:-1]
    seg = np.cumsum(head) - 1
    K = int(seg[-1]) + 1 if len(order) else 0
    inverse = np.full(M, -1, np.int64)
    inverse[order] = seg
    start = np.flatnonzero(head)
    counts = np.diff(np.append(start, len(order))).astype(np.int32)
    keys = skey[head]
    mask = (1 << CELL_BITS) - 1
    cell = np.stack([keys & mask, (keys >> CELL_BITS) & mask, keys >> (2 * CELL_BITS)], 1)
    if dtype == F32:
        corner = o[None] + cell.astype(F32) * F32(voxel_size)
    else:
        corner = o.astype(F64)[None] + cell.astype(F64) * F64(F32(voxel_size))
    p = p32.astype(dtype)
    sums = np.zeros((K, 3), dtype)
    for r in range(int(counts.max()) if K else 0):                          # the r-th point of every voxel that has one: sequential sums
        live = np.flatnonzero(counts > r)
        sums[live] = sums[live] + (p[order[start[live] + r]] - corner[live])
    centroids = corner + sums / counts.astype(dtype)[:, None]
    assert centroids.dtype == dtype
    return dict(centroids=centroids, counts=counts, inverse=inverse, outside=int((finite & ~inside).sum()), keys=keys)


def sq_dists(cloud, nodes, dtype=F32):
    """[Q,N]: d = node - point, dx dx + dy dy + dz dz summed left to right (the arithmetic of csplat_knn_query)"""
    d = np.asarray(nodes, F32).astype(dtype)[None, :, :] - np.asarray(cloud, F32).astype(dtype)[:, None, :]
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def observable(cloud, nodes, k=2, max_dist=None):
    """bool [N]: the nodes among the k nearest (float32 squared distance, ties to the smaller index) of some cloud point"""
    N = np.asarray(nodes).shape[0]
    flags = np.zeros(N, bool)
    cloud = np.asarray(cloud, F32)
    for lo in range(0, cloud.shape[0], 4096):
        d2 = sq_dists(cloud[lo:lo + 4096], nodes)
        idx = np.argsort(d2, axis=1, kind="stable")[:, :k]
        near = np.take_along_axis(d2, idx, 1)
        keep = np.ones_like(idx, bool) if max_dist is None else near <= F32(F64(max_dist) * F64(max_dist))
        flags[idx[keep]] = True
    return flags


def tie_margins(cloud, nodes, k):
    """per cloud point: the gap between its k-th and (k+1)-th smallest float64 squared distance (inf when N == k)"""
    d2 = np.sort(sq_dists(cloud, nodes, F64), axis=1)
    return d2[:, k] - d2[:, k - 1] if d2.shape[1] > k else np.full(d2.shape[0], np.inf)


def camera_intrinsics(fovx, fovy, H, W):
    """the renderer's intrinsics: fx = W / (2 tan(FoVx / 2)), cx = (W - 1) / 2"""
    return np.array([W / (2 * np.tan(fovx * 0.5)), H / (2 * np.tan(fovy * 0.5)), (W - 1) * 0.5, (H - 1) * 0.5], F64)


def chamfer_one_sided(a, b):
    """(1/|a|) sum_i min_j |b_j - a_i|^2 in float64"""
    a, b = np.asarray(a, F64), np.asarray(b, F64)
    total = 0.0
    for lo in range(0, a.shape[0], 2048):
        d = b[None] - a[lo:lo + 2048, None]
        total += float((d * d).sum(-1).min(1).sum())
    return total / a.shape[0]
