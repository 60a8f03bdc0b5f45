"""Mesh z-buffer, the arrow mesh -> image (csplat_zb_mesh / csplat_zb_points / csplat_zb_mark, include/csplat.h): what a depth camera would
see of the cloth mesh.

  rasterize_mesh    a triangle mesh in V views -> MeshImages(depth, silhouette, face_id, bary, screen) (the reference renders its meshes with
                    Blender, manipulation/fold_rendering/)
  splat_points      a point cloud as one-pixel primitives -> PointImages(depth, point_id) (the reference's build_depth_from_pointcloud,
                    manipulation/envs/camera_utils.py:7-41, a Python double loop)
  mesh_visibility   face_id images -> which faces and which nodes each view sees (the reference guesses this from a cloud:
                    get_observable_particle_index)

Coverage is exact integer arithmetic on coordinates snapped to 1/256 pixel with the top-left rule, the depth interpolates 1 / z (perspective-
correct), the nearest face wins and equal depths go to the lower face index: every output is a pure function of the inputs and bit-
reproducible.  There is NO CLIPPING: a face with a corner behind `near` (or more than 16384 pixels from the origin) is dropped whole -- the
cloth is in front of the camera.

Float32 contiguous GPU tensors take the HIP kernels; anything else (CPU tensors, float64, strided) is converted to float32 and composes the
same definitions from torch operations, in chunks of faces with int64 edge functions (reported through csplat.native.composed_fallback for
GPU tensors: raises under STRICT; it is the CPU path).  Everything here is an observation: detached, no gradients.

The three uses:
    images = rasterize_mesh(vertices, faces, (H, W), cameras=cams)
    for v, camera in enumerate(cams):                                   # csplat.geometry_loss / observation.camera_points read these
        camera.depth, camera.silhouette = images.depth[v], images.silhouette[v]
    ray = rasterize_mesh(vertices, faces, (H, W), cameras=cams, kind="ray").depth[:, 0]      # the depth tracking.track_visibility compares
    _faces_seen, node_visible = mesh_visibility(images.face_id, faces, len(vertices))         # against |X - camera centre|
    weights = node_visible.any(0).float()                               # `node_weights` of meshnet.mpc.candidate_costs"""
from typing import NamedTuple, Optional

import numpy as np
import torch

from . import native as _n
from .observation import _float, camera_intrinsics

SUB = 256                 # include/csplat.h: snapped units per pixel
GUARD = 16384.0           # |px|, |py| of a valid vertex
CPU_CHUNK = 1 << 20       # (faces x pixels) per [chunk, H, W] block of the composed raster
_EMPTY = (1 << 63) - 1    # the composed key of the background (the kernels' is all-ones)


def temp_bytes(V, n, H, W):
    """the temp of csplat_zb_mesh / csplat_zb_points as include/csplat.h words it: the per-pixel keys and the screen records of n vertices
    (or points), each rounded up to a multiple of 256 bytes"""
    return ((8 * V * H * W + 255) & ~255) + ((16 * V * n + 255) & ~255)


class MeshImages(NamedTuple):
    depth: torch.Tensor                 # [V,1,H,W] float32, 0 where no face covers the pixel
    silhouette: torch.Tensor            # [V,1,H,W] float32, 0 or 1
    face_id: torch.Tensor               # [V,H,W] int32, -1 on the background
    bary: Optional[torch.Tensor]        # [V,3,H,W] float32 perspective-correct weights in the face's corner order (with_bary), else None
    screen: Optional[torch.Tensor]      # [V,N,4] int32 (sx, sy, float bits of 1 / z, valid) (return_screen), else None


class PointImages(NamedTuple):
    depth: torch.Tensor                 # [V,1,H,W] float32, 0 where no point lands
    point_id: torch.Tensor              # [V,H,W] int32, -1: none


def _size(size, what):
    try:
        H, W = int(size[0]), int(size[1])
    except (TypeError, IndexError, ValueError):
        raise ValueError(f"{what}: `size` is (H, W), got {size!r}") from None
    if H < 1 or W < 1 or H * W >= 2 ** 31:
        raise ValueError(f"{what}: `size` is (H, W) with both >= 1 and H * W < 2^31, got {(H, W)}")
    return H, W


def _scene(what, X, name, size, intrinsics, world_to_cam, cameras, near, kind):
    """the checks the two renderers share -> (X [V,n,3] or [n,3], per_view, V, H, W, K4 [V,4], W2C [V,3,4] on the host, near)"""
    X = _float(X, name, what)
    if X.dim() not in (2, 3) or X.shape[-1] != 3:
        raise ValueError(f"{what}: `{name}` is [n,3] or [V,n,3], got {tuple(X.shape)}")
    H, W = _size(size, what)
    if kind not in ("z", "ray"):
        raise ValueError(f"{what}: `kind` is \"z\" or \"ray\", got {kind!r}")
    near = float(near)
    if not (near >= 0.0 and near < float("inf")):
        raise ValueError(f"{what}: `near` is a finite number >= 0, got {near!r}")
    if cameras is not None:
        if intrinsics is not None or world_to_cam is not None:
            raise ValueError(f"{what}: pass either `cameras` or `intrinsics` and `world_to_cam`, not both")
        cameras = list(cameras)
        if not cameras:
            raise ValueError(f"{what}: `cameras` is empty")
        mats = []
        for c in cameras:
            wvt = c.world_view_transform
            wvt = wvt.detach().cpu().numpy() if torch.is_tensor(wvt) else np.asarray(wvt)
            if wvt.shape != (4, 4):
                raise ValueError(f"{what}: camera.world_view_transform is [4,4], got {wvt.shape}")
            mats.append(wvt.astype(np.float64).T[:3])
        K4 = torch.tensor([camera_intrinsics(c, H, W) for c in cameras], dtype=torch.float64)
        W2C = torch.from_numpy(np.stack(mats))
    else:
        if intrinsics is None or world_to_cam is None:
            raise ValueError(f"{what}: pass `cameras`, or both `intrinsics` [V,4] and `world_to_cam` [V,3,4]")
        K4, W2C = _float(intrinsics, "intrinsics", what).cpu(), _float(world_to_cam, "world_to_cam", what).cpu()
        if K4.dim() not in (1, 2) or K4.shape[-1] != 4:
            raise ValueError(f"{what}: `intrinsics` is [V,4] (or [4]: one for all views), got {list(K4.shape)}")
        if W2C.dim() not in (2, 3) or tuple(W2C.shape[-2:]) not in ((3, 4), (4, 4)):
            raise ValueError(f"{what}: `world_to_cam` is [V,3,4] or [V,4,4] (or one matrix for all views), got {list(W2C.shape)}")
    per_view = X.dim() == 3
    counts = {int(t.shape[0]) for t, full in ((X, 3), (K4, 2), (W2C, 3)) if t.dim() == full}
    if len(counts) > 1:
        raise ValueError(f"{what}: `{name}`, the intrinsics and the matrices disagree on the number of views: {sorted(counts)}")
    V = counts.pop() if counts else 1
    if V < 1 or V > 65535 or V * H * W >= 2 ** 31 or V * int(X.shape[-2]) >= 2 ** 31:
        raise ValueError(f"{what}: 1 to 65535 views with V * H * W < 2^31 and V * n < 2^31, got V = {V}, size {(H, W)}, n = {int(X.shape[-2])}")
    K4 = (K4[None].expand(V, -1) if K4.dim() == 1 else K4)
    W2C = (W2C[None].expand(V, -1, -1) if W2C.dim() == 2 else W2C)[:, :3, :]
    return X, per_view, V, H, W, K4, W2C, near


def _faces(faces, N, what):
    if isinstance(faces, np.ndarray):
        faces = torch.from_numpy(np.ascontiguousarray(faces))
    if not torch.is_tensor(faces) or faces.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"{what}: `faces` is an int32 / int64 tensor or array [F,3] (or the reference's [3,F])")
    if faces.dim() != 2 or 3 not in tuple(faces.shape):
        raise ValueError(f"{what}: `faces` is [F,3] or [3,F], got {tuple(faces.shape)}")
    if faces.shape[1] != 3:
        faces = faces.t()
    F = int(faces.shape[0])
    if F >= 2 ** 31:
        raise ValueError(f"{what}: at most 2^31 - 1 faces, got {F}")
    if F:
        lo, hi = int(faces.min()), int(faces.max())
        if lo < 0 or hi >= N:
            raise ValueError(f"{what}: face indices must lie in 0 .. {N - 1}, found {lo} .. {hi}")
    return faces.detach()


# ---------------------------------------------------------------------------------------------- the definitions from torch operations
def _project_composed(P, K4, W2C, near):
    """stage P in float32: P [V,n,3] -> (screen [V,n,4] int32, px, py, z, valid)"""
    X, Y, Z = P.unbind(-1)
    r = lambda i, j: W2C[:, i, j, None]  # noqa: E731
    x = r(0, 0) * X + r(0, 1) * Y + r(0, 2) * Z + r(0, 3)
    y = r(1, 0) * X + r(1, 1) * Y + r(1, 2) * Z + r(1, 3)
    z = r(2, 0) * X + r(2, 1) * Y + r(2, 2) * Z + r(2, 3)
    px = (K4[:, 0, None] * x) / z + K4[:, 2, None]
    py = (K4[:, 1, None] * y) / z + K4[:, 3, None]
    iz = 1.0 / z
    valid = torch.isfinite(x) & torch.isfinite(y) & torch.isfinite(z) & torch.isfinite(px) & torch.isfinite(py) & torch.isfinite(iz)
    valid &= (z > torch.tensor(near, dtype=z.dtype, device=z.device)) & (px.abs() <= GUARD) & (py.abs() <= GUARD)
    zero = torch.zeros_like(px)
    sx = torch.round(float(SUB) * torch.where(valid, px, zero)).to(torch.int32)
    sy = torch.round(float(SUB) * torch.where(valid, py, zero)).to(torch.int32)
    bits = torch.where(valid, iz, zero).contiguous().view(torch.int32)
    return torch.stack([sx, sy, bits, valid.to(torch.int32)], -1), px, py, z, valid


def _owns(E, dx, dy):
    return (E > 0) | ((E == 0) & ((dy < 0) | ((dy == 0) & (dx > 0))))


def _stage_d(c, Px, Py):
    """corner records c [...,3,4] int64 at the snapped points (Px, Py), which broadcast against c[..., 0, 0] -> (covered, b [3], iz [3], q)"""
    x0, y0, x1, y1, x2, y2 = c[..., 0, 0], c[..., 0, 1], c[..., 1, 0], c[..., 1, 1], c[..., 2, 0], c[..., 2, 1]
    A = (x1 - x0) * (y2 - y0) - (y1 - y0) * (x2 - x0)
    live = (c[..., 0, 3] != 0) & (c[..., 1, 3] != 0) & (c[..., 2, 3] != 0) & (A != 0)
    sw = A < 0
    x1, x2, y1, y2 = torch.where(sw, x2, x1), torch.where(sw, x1, x2), torch.where(sw, y2, y1), torch.where(sw, y1, y2)
    A = A.abs()

    def edge(xa, ya, xb, yb):
        dx, dy = xb - xa, yb - ya
        E = dx * (Py - ya) - dy * (Px - xa)
        return E, _owns(E, dx, dy)
    (E01, o01), (E12, o12), (E20, o20) = edge(x0, y0, x1, y1), edge(x1, y1, x2, y2), edge(x2, y2, x0, y0)
    fA = A.to(torch.float32)
    w0, w1, w2 = E12.to(torch.float32) / fA, E20.to(torch.float32) / fA, E01.to(torch.float32) / fA
    b = (w0, torch.where(sw, w2, w1), torch.where(sw, w1, w2))
    iz = tuple(c[..., k, 2].to(torch.int32).contiguous().view(torch.float32) for k in range(3))
    q = b[0] * iz[0] + b[1] * iz[1] + b[2] * iz[2]
    return live & o01 & o12 & o20, b, iz, q


def _keys(z, ids):
    return (z.contiguous().view(torch.int32).to(torch.int64) << 32) | ids


def _raster_composed(screen, faces, H, W):
    """stage D and the depth test: screen [V,N,4] int32, faces [F,3] int64 -> keys [V,H,W] int64 = (float bits of z) << 32 | face"""
    V, dev = screen.shape[0], screen.device
    F = int(faces.shape[0])
    keys = torch.full((V, H, W), _EMPTY, dtype=torch.int64, device=dev)
    Px = (SUB * torch.arange(W, dtype=torch.int64, device=dev))[None, None, :]
    Py = (SUB * torch.arange(H, dtype=torch.int64, device=dev))[None, :, None]
    chunk = max(1, CPU_CHUNK // (H * W))
    empty = torch.tensor(_EMPTY, dtype=torch.int64, device=dev)
    for v in range(V):
        s = screen[v].to(torch.int64)
        for lo in range(0, F, chunk):
            c = s[faces[lo:lo + chunk]][:, None, None]                 # [C,1,1,3,4]
            cov, b, iz, q = _stage_d(c, Px, Py)
            ids = torch.arange(lo, lo + c.shape[0], dtype=torch.int64, device=dev)[:, None, None]
            key = torch.where(cov, _keys(1.0 / q, ids), empty)
            keys[v] = torch.minimum(keys[v], key.min(0).values)
    return keys


def _points_composed(P, K4, W2C, near, H, W):
    """points as one-pixel primitives: P [V,M,3] -> keys [V,H,W] int64"""
    V, M, dev = P.shape[0], P.shape[1], P.device
    _screen, px, py, z, valid = _project_composed(P, K4, W2C, near)
    rx, ry = torch.round(px), torch.round(py)
    on = valid & (rx >= 0) & (rx <= W - 1) & (ry >= 0) & (ry <= H - 1)
    keys = torch.full((V, H * W), _EMPTY, dtype=torch.int64, device=dev)
    for v in range(V):
        m = on[v].nonzero()[:, 0]
        key = _keys(z[v][m], m)
        pix = ry[v][m].to(torch.int64) * W + rx[v][m].to(torch.int64)
        key, order = torch.sort(key)                                   # ascending key, then stable by pixel: a pixel's first entry is its minimum
        pix, second = torch.sort(pix[order], stable=True)
        key = key[second]
        first = torch.ones_like(pix, dtype=torch.bool)
        first[1:] = pix[1:] != pix[:-1]
        keys[v][pix[first]] = key[first]
    return keys.view(V, H, W)


def _resolve_composed(keys, K4, kind):
    """keys -> (depth [V,H,W] float32, hit [V,H,W] bool, ids [V,H,W] int32)"""
    V, H, W = keys.shape
    dev = keys.device
    hit = keys != _EMPTY
    z = (keys >> 32).to(torch.int32).contiguous().view(torch.float32)
    if kind == "ray":
        u = (torch.arange(W, dtype=torch.float32, device=dev)[None, None, :] - K4[:, 2, None, None]) / K4[:, 0, None, None]
        w = (torch.arange(H, dtype=torch.float32, device=dev)[None, :, None] - K4[:, 3, None, None]) / K4[:, 1, None, None]
        z = z * torch.sqrt(u * u + w * w + 1.0)
    ids = torch.where(hit, keys & 0xFFFFFFFF, torch.tensor(-1, dtype=torch.int64, device=dev)).to(torch.int32)
    return torch.where(hit, z, torch.zeros_like(z)), hit, ids


def _bary_composed(screen, faces, ids, hit):
    V, H, W = ids.shape
    dev = ids.device
    Px = (SUB * torch.arange(W, dtype=torch.int64, device=dev))[None, :]
    Py = (SUB * torch.arange(H, dtype=torch.int64, device=dev))[:, None]
    out = torch.zeros(V, 3, H, W, dtype=torch.float32, device=dev)
    if faces.shape[0] == 0:
        return out
    for v in range(V):
        c = screen[v].to(torch.int64)[faces[ids[v].clamp(min=0).to(torch.int64)]]          # [H,W,3,4]
        _cov, b, iz, q = _stage_d(c, Px, Py)
        for i in range(3):
            out[v, i] = torch.where(hit[v], (b[i] * iz[i]) / q, out[v, i])
    return out


# ---------------------------------------------------------------------------------------------- the public functions
def rasterize_mesh(vertices, faces, size, *, intrinsics=None, world_to_cam=None, cameras=None, near=0.01, kind="z", with_bary=False,
                   return_screen=False):
    """A triangle mesh in V views -> MeshImages(depth [V,1,H,W], silhouette [V,1,H,W], face_id [V,H,W] int32, bary, screen)
    (include/csplat.h, csplat_zb_mesh, states the semantics).
      vertices      [N,3] (one mesh for all views) or [V,N,3] (a mesh per view, e.g. per time), float
      faces         [F,3] or the reference's [3,F], int32 / int64, indices in [0, N) (a [3,3] tensor reads as [F,3])
      size          (H, W)
      intrinsics    [V,4] = (fx, fy, cx, cy) in pixel units, pixel centres at the integers   } either these two, exactly as
      world_to_cam  [V,3,4] or [V,4,4], column-vector form: p_cam = R p_world + t             } unproject_depth takes them, mirrored
      cameras       or reference-style cameras, one per view: world_to_cam = world_view_transform.T[:3] and the intrinsics are
                    observation.camera_intrinsics -- tracking.project of an unprojected pixel then returns its centre
      near          a vertex is valid when its view-space z > near (default: the reference's znear) and it lands within 16384 pixels
      kind          "z": the view-space z;  "ray": the distance along the pixel's ray, the exact inverse of unproject_depth's "ray"
      with_bary     also the perspective-correct weights [V,3,H,W] of the winning face's corners
      return_screen also the projected vertices [V,N,4] int32 = (sx, sy, float bits of 1 / z, valid) in 1/256 pixel
    A pixel is covered when its centre lies inside the face's snapped triangle (top-left rule, exact integers); the depth interpolates
    1 / z; the nearest face wins, equal depths go to the lower face index; a hole is 0 (the convention of unproject_depth).  NO CLIPPING: a
    face with an invalid corner is dropped whole -- the cloth is in front of the camera.  Both windings are drawn: the cloth is two-sided.
    ValueError before anything touches the device for every malformed argument (one blocking read: the range of the face indices)."""
    what = "rasterize_mesh"
    X, per_view, V, H, W, K4, W2C, near = _scene(what, vertices, "vertices", size, intrinsics, world_to_cam, cameras, near, kind)
    N, dev = int(X.shape[-2]), X.device
    Fc = _faces(faces, N, what).to(dev)
    F = int(Fc.shape[0])
    K4, W2C = K4.to(device=dev, dtype=torch.float32).contiguous(), W2C.to(device=dev, dtype=torch.float32).contiguous()
    if X.is_cuda:
        why = _n.why_not_f32c(X)
        if why is None:
            Fi = Fc.to(torch.int32).contiguous()
            depth = torch.empty(V, 1, H, W, dtype=torch.float32, device=dev)
            sil = torch.empty(V, 1, H, W, dtype=torch.float32, device=dev)
            ids = torch.empty(V, H, W, dtype=torch.int32, device=dev)
            bary = torch.empty(V, 3, H, W, dtype=torch.float32, device=dev) if with_bary else None
            screen = torch.empty(V, N, 4, dtype=torch.int32, device=dev) if return_screen else None
            temp = _n.temp(dev, temp_bytes(V, N, H, W))
            _n.launch("csplat_zb_mesh", dev, V, N, F, H, W, _n.ptr(X), int(per_view), _n.ptr(Fi), _n.ptr(K4), _n.ptr(W2C), near,
                      0 if kind == "z" else 1, _n.ptr(depth), _n.ptr(sil), _n.ptr(ids), _n.ptr(bary), _n.ptr(screen), _n.ptr(temp), temp.numel())
            return MeshImages(depth, sil, ids, bary, screen)
        _n.composed_fallback("zbuffer.rasterize_mesh", why, X)
    P = X.to(torch.float32)
    screen = _project_composed(P if per_view else P[None].expand(V, -1, -1), K4, W2C, near)[0]
    Fl = Fc.to(torch.int64)
    keys = _raster_composed(screen, Fl, H, W)
    depth, hit, ids = _resolve_composed(keys, K4, kind)
    bary = _bary_composed(screen, Fl, ids, hit) if with_bary else None
    return MeshImages(depth[:, None], hit.to(torch.float32)[:, None], ids, bary, screen if return_screen else None)


def splat_points(points, size, *, intrinsics=None, world_to_cam=None, cameras=None, near=0.01, kind="z"):
    """A point cloud as one-pixel primitives -> PointImages(depth [V,1,H,W], point_id [V,H,W] int32) (include/csplat.h, csplat_zb_points;
    the reference's build_depth_from_pointcloud).  `points` is [M,3] or [V,M,3]; cameras, `near` and `kind` as rasterize_mesh.  A valid
    point lands in the pixel (rint(px), rint(py)), round-half-even; points outside the image are dropped; the nearest point of a pixel
    wins and a tie goes to the lower index; a pixel without a point has depth 0 and id -1."""
    what = "splat_points"
    X, per_view, V, H, W, K4, W2C, near = _scene(what, points, "points", size, intrinsics, world_to_cam, cameras, near, kind)
    M, dev = int(X.shape[-2]), X.device
    K4, W2C = K4.to(device=dev, dtype=torch.float32).contiguous(), W2C.to(device=dev, dtype=torch.float32).contiguous()
    if X.is_cuda:
        why = _n.why_not_f32c(X)
        if why is None:
            depth = torch.empty(V, 1, H, W, dtype=torch.float32, device=dev)
            ids = torch.empty(V, H, W, dtype=torch.int32, device=dev)
            temp = _n.temp(dev, temp_bytes(V, M, H, W))
            _n.launch("csplat_zb_points", dev, V, M, H, W, _n.ptr(X), int(per_view), _n.ptr(K4), _n.ptr(W2C), near, 0 if kind == "z" else 1,
                      _n.ptr(depth), _n.ptr(ids), _n.ptr(temp), temp.numel())
            return PointImages(depth, ids)
        _n.composed_fallback("zbuffer.splat_points", why, X)
    P = X.to(torch.float32)
    keys = _points_composed(P if per_view else P[None].expand(V, -1, -1), K4, W2C, near, H, W)
    depth, _hit, ids = _resolve_composed(keys, K4, kind)
    return PointImages(depth[:, None], ids)


def mesh_visibility(face_id, faces, num_nodes):
    """face_id [V,H,W] (or [H,W]: one view) as rasterize_mesh returns it, faces [F,3] / [3,F], the number of nodes N -> (face_visible
    [V,F] bool, node_visible [V,N] bool): the faces that own a pixel of the view, and their corners (include/csplat.h, csplat_zb_mark).
    The exact counterpart of the reference's get_observable_particle_index for a mesh that was rendered; node_visible (.any(0) over the
    views, .float()) suits `node_weights` of meshnet.mpc.candidate_costs."""
    what = "mesh_visibility"
    if not torch.is_tensor(face_id) or face_id.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"{what}: `face_id` is an int32 / int64 tensor [V,H,W]")
    ids = face_id.detach()
    if ids.dim() == 2:
        ids = ids[None]
    if ids.dim() != 3:
        raise ValueError(f"{what}: `face_id` is [V,H,W] or [H,W], got {tuple(face_id.shape)}")
    if not isinstance(num_nodes, int) or isinstance(num_nodes, bool) or not 0 <= num_nodes < 2 ** 31:
        raise ValueError(f"{what}: `num_nodes` is an integer in 0 .. 2^31 - 1, got {num_nodes!r}")
    V, H, W = (int(s) for s in ids.shape)
    N, dev = num_nodes, ids.device
    Fc = _faces(faces, N, what).to(dev)
    F = int(Fc.shape[0])
    if V > 65535 or V * H * W >= 2 ** 31 or V * max(N, F) >= 2 ** 31:
        raise ValueError(f"{what}: at most 65535 views with V * H * W, V * N and V * F below 2^31, got {(V, H, W)}, N = {N}, F = {F}")
    if ids.numel() and int(ids.max()) >= F:
        raise ValueError(f"{what}: `face_id` holds {int(ids.max())}, the mesh has {F} faces")
    if ids.is_cuda:
        why = "dtype" if ids.dtype != torch.int32 else (None if ids.is_contiguous() else "layout")
        if why is None:
            Fi = Fc.to(torch.int32).contiguous()
            flags = torch.empty(V * (F + N), dtype=torch.uint8, device=dev)
            face_visible, node_visible = flags[:V * F].view(V, F), flags[V * F:].view(V, N)
            _n.launch("csplat_zb_mark", dev, V, N, F, H, W, _n.ptr(ids), _n.ptr(Fi), face_visible.data_ptr() if V * F else None,
                      node_visible.data_ptr() if V * N else None)
            return face_visible.view(torch.bool), node_visible.view(torch.bool)
        _n.composed_fallback("zbuffer.mesh_visibility", why, ids)
    face_visible = torch.zeros(V, F, dtype=torch.bool, device=dev)
    node_visible = torch.zeros(V, N, dtype=torch.bool, device=dev)
    Fl = Fc.to(torch.int64)
    for v in range(V):
        seen = ids[v][ids[v] >= 0].to(torch.int64)
        face_visible[v, seen] = True
        node_visible[v, Fl[seen].reshape(-1)] = True
    return face_visible, node_visible
