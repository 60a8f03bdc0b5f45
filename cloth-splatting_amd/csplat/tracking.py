"""Point tracking, the evaluation end of the pipeline (csplat_track_visibility / csplat_track_mte, include/csplat.h): occlusion-aware
tracks of the Gaussians or the mesh vertices over views and frames, and the mean trajectory error (MTE) against ground-truth tracks.

  track_visibility       pixel, in-image and visible decisions of N points in F view-frames, one launch
  get_mask, project      the reference's functions of the same names (render.py:77-121), thin wrappers
  mean_trajectory_error  the reference's align_traj + compute_mte (scripts/align_eval_trajs.py) for all ground-truth tracks, one launch
  track                  render.py's --log_deform / --show_flow / --track_vertices collection: a Tracks record, everything on the device

Float32 contiguous GPU tensors take the HIP kernels; anything else (CPU tensors, float64) composes the same decisions from torch
operations (reported through csplat.native.composed_fallback for GPU tensors: raises under STRICT; it is the CPU path).

Two behaviours to know.  When track_visibility PROJECTS, a point behind the camera (w <= 0) is never in the image; the reference has no
such test and mirrors it into the image.  get_mask receives projections and, like the reference's, has no such test.  A ZERO quaternion
makes its track's aligned positions and the MTE NaN, as build_rotation of the reference does; it is not guarded.  The quaternions are
read as the reference's evaluation reads them, first component r, whichever convention wrote them (get_vertice_rotation writes NaN for a
vertex whose normal did not move: such a track's MTE is NaN there and here)."""
from typing import NamedTuple, Optional

import numpy as np
import torch

from . import native as _n


class Visibility(NamedTuple):
    pixels: torch.Tensor        # [F,N,2] (or [N,2]) float: x, y in pixels, pixel centres at the integers
    in_image: torch.Tensor      # [F,N] bool
    visible: torch.Tensor       # [F,N] bool: in the image and not behind the rendered depth
    counts: torch.Tensor        # [F,2] int32: (in the image, visible)


class TrajectoryError(NamedTuple):
    mean: torch.Tensor          # [] the MTE: mean over the tracks of per_track
    per_track: torch.Tensor     # [G] mean over the frames of |gt - aligned|
    aligned: torch.Tensor       # [T,G,3] the associated trajectories after the alignment
    assoc: torch.Tensor         # [G] int64: the tracked point of each ground-truth track


def _tensor(a, name, what):
    if isinstance(a, np.ndarray):
        a = torch.from_numpy(np.ascontiguousarray(a))
    if not torch.is_tensor(a):
        raise ValueError(f"{what}: `{name}` is a tensor or numpy array, got {type(a).__name__}")
    return a.detach()


def _float(a, name, what):
    t = _tensor(a, name, what)
    if not t.dtype.is_floating_point:
        raise ValueError(f"{what}: `{name}` must be floating point, got {t.dtype}")
    return t


def _visibility_composed(X, pix, full, cam, depth, W, H, thr, min_depth, far):
    """the decisions of csplat_track_visibility from torch operations, in the dtype of the points"""
    if pix is None:
        hom = X[..., 0:1] * full[:, None, 0] + X[..., 1:2] * full[:, None, 1] + X[..., 2:3] * full[:, None, 2] + full[:, None, 3]
        w = hom[..., 3]
        x, y = ((hom[..., 0] / w + 1.0) * W - 1.0) * 0.5, ((hom[..., 1] / w + 1.0) * H - 1.0) * 0.5
        front = w > 0
    else:
        x, y = pix[..., 0], pix[..., 1]
        front = torch.ones_like(x, dtype=torch.bool)
    inside = front & torch.isfinite(x) & torch.isfinite(y) & (x >= 0) & (x < W) & (y >= 0) & (y < H)
    vis = inside
    if depth is not None:
        zero = torch.zeros((), dtype=x.dtype, device=x.device)
        xi = torch.where(inside, x, zero).long().clamp(0, W - 1)          # (.long() truncates, as C and astype(int))
        yi = torch.where(inside, y, zero).long().clamp(0, H - 1)
        d = depth.reshape(depth.shape[0], H * W).gather(1, yi * W + xi)
        if min_depth > 0.0:
            d = torch.where(d < min_depth, torch.full_like(d, far), d)
        dx, dy, dz = X[..., 0] - cam[:, None, 0], X[..., 1] - cam[:, None, 1], X[..., 2] - cam[:, None, 2]
        dist = torch.sqrt(dx * dx + dy * dy + dz * dz)
        vis = inside & ((dist - thr) <= d)
    counts = torch.stack([inside.sum(1), vis.sum(1)], 1).to(torch.int32)
    return torch.stack([x, y], -1), inside, vis, counts


def track_visibility(points, full_proj, cam_center, depth, size, *, pixels=None, depth_threshold=0.2, min_depth=1.0, far_value=1e4):
    """Where N points land in F view-frames and whether the rendered depth hides them -> Visibility(pixels, in_image, visible, counts)
    (include/csplat.h, csplat_track_visibility, states the semantics; the reference's `project` + `get_mask`, render.py:77-121).
      points       [F,N,3] or [N,3] (one frame: every result loses its leading axis), float
      full_proj    [F,4,4], or [4,4] for all frames: camera.full_proj_transform (hom = [X, 1] @ full); may be None when `pixels` is given
      cam_center   [F,3], or [3] for all frames: camera.camera_center; may be None without a depth image
      depth        None (visible = in_image), or the rendered depth images [F,H,W] / [F,1,H,W] ([H,W] for one frame)
      size         (H, W), one size for all frames
      pixels       None: the points are projected (and a point with w <= 0 is never in the image); [F,N,2] / [N,2]: these pixel
                   coordinates are used instead (the get_mask form, no test of w)
      depth_threshold   a point is visible when |X - cam_center| - depth_threshold <= depth at its pixel (C truncation)
      min_depth, far_value   a depth below min_depth reads as far_value (render.py:171, 206: `depth[depth < 1.0] = 10e3`); <= 0: off
    ValueError before anything touches the device for every malformed argument."""
    what = "track_visibility"
    X = _float(points, "points", what)
    single = X.dim() == 2
    if single:
        X = X[None]
    if X.dim() != 3 or X.shape[2] != 3:
        raise ValueError(f"{what}: `points` is [F,N,3] or [N,3], got {tuple(points.shape)}")
    F, N = int(X.shape[0]), int(X.shape[1])
    if F < 1 or F > 65535:
        raise ValueError(f"{what}: {F} frames; one call takes 1 to 65535")
    try:
        H, W = int(size[0]), int(size[1])
    except (TypeError, IndexError, ValueError):
        raise ValueError(f"{what}: `size` is (H, W), got {size!r}") from None
    if H < 1 or W < 1 or H * W >= 2 ** 31:
        raise ValueError(f"{what}: `size` is (H, W) with both >= 1 and H * W < 2^31, got {(H, W)}")
    thr, lo, far = float(depth_threshold), float(min_depth), float(far_value)
    if thr != thr or far != far or lo != lo:
        raise ValueError(f"{what}: depth_threshold, min_depth and far_value are numbers, got {(thr, lo, far)}")
    dev, dt = X.device, X.dtype

    def frames(t, name, shape):
        t = _float(t, name, what).to(dev)
        if t.dim() == len(shape):          # one camera for every frame
            t = t[None].expand(F, *t.shape)
        if tuple(t.shape) != (F,) + shape:
            raise ValueError(f"{what}: `{name}` is {list((F,) + shape)} (or {list(shape)}: one for all frames), got {list(t.shape)}")
        return t

    pix = None
    if pixels is not None:
        pix = _float(pixels, "pixels", what).to(dev)
        pix = pix[None] if pix.dim() == 2 else pix
        if tuple(pix.shape) != (F, N, 2):
            raise ValueError(f"{what}: `pixels` is {[F, N, 2]} next to these points, got {list(pix.shape)}")
    if full_proj is None:
        if pix is None:
            raise ValueError(f"{what}: `full_proj` may be None only when `pixels` is given")
        full = torch.zeros(F, 4, 4, dtype=dt, device=dev)
    else:
        full = frames(full_proj, "full_proj", (4, 4))
    D = None
    if depth is not None:
        D = _float(depth, "depth", what).to(dev)
        if D.dim() == 4 and D.shape[1] == 1:
            D = D[:, 0]
        if D.dim() == 2:
            D = D[None]
        if tuple(D.shape) != (F, H, W):
            raise ValueError(f"{what}: `depth` is {[F, H, W]} or {[F, 1, H, W]} (or [H,W] / [1,H,W] for one frame), got {list(depth.shape)}")
    if cam_center is None:
        if D is not None:
            raise ValueError(f"{what}: `cam_center` may be None only without a depth image")
        cam = torch.zeros(F, 3, dtype=dt, device=dev)
    else:
        cam = frames(cam_center, "cam_center", (3,))
    if X.is_cuda:
        if any(t is not None and t.dtype != dt for t in (pix, full, D, cam)):
            why = "dtype"
        else:
            full, cam = full.contiguous(), cam.contiguous()          # (19 floats a frame: one camera for all frames arrives expanded)
            why = _n.why_not_f32c(X, pix, full, D, cam)
        if why is None:
            pix_out = torch.empty(F, N, 2, dtype=torch.float32, device=dev)
            flags = torch.empty(2, F, N, dtype=torch.uint8, device=dev)
            counts = torch.empty(F, 2, dtype=torch.int32, device=dev)
            _n.launch("csplat_track_visibility", dev, F, N, W, H, _n.ptr(X), _n.ptr(pix), _n.ptr(full), _n.ptr(cam), _n.ptr(D), thr, lo, far,
                      _n.ptr(pix_out), flags[0].data_ptr(), flags[1].data_ptr(), _n.ptr(counts))
            out = (pix_out, flags[0].view(torch.bool), flags[1].view(torch.bool), counts)
            return Visibility(*(t[0] for t in out)) if single else Visibility(*out)
        _n.composed_fallback("tracking.track_visibility", why, X)
    others = [None if t is None else t.to(dt) for t in (pix, full, D, cam)]
    out = _visibility_composed(X, others[0], others[1], others[3], others[2], W, H, thr, lo, far)
    return Visibility(*(t[0] for t in out)) if single else Visibility(*out)


def get_mask(projections=None, gaussian_positions=None, depth=None, cam_center=None, height=800, width=800, depth_threshold=0.2):
    """Drop-in for the reference's `get_mask` (render.py:95-121) -> numpy (depth_mask & mask_in_image, mask_in_image), bool [N].
    projections [N,2], gaussian_positions [N,3], depth [H,W] or [1,H,W], cam_center [3]: numpy arrays or tensors.  As the reference's,
    it does NOT replace small depths (its caller does, render.py:206) and has no test of w: it receives projections."""
    for name, v in (("projections", projections), ("gaussian_positions", gaussian_positions), ("depth", depth), ("cam_center", cam_center)):
        if v is None:
            raise ValueError(f"get_mask: `{name}` is required")
    D = _float(depth, "depth", "get_mask")
    if D.dim() == 3:
        D = D[0]
    X = _float(gaussian_positions, "gaussian_positions", "get_mask")
    like = dict(dtype=X.dtype, device=X.device)
    r = track_visibility(X, None, _float(cam_center, "cam_center", "get_mask").to(**like), D.to(**like), (int(height), int(width)),
                         pixels=_float(projections, "projections", "get_mask").to(**like), depth_threshold=depth_threshold, min_depth=0.0)
    return r.visible.cpu().numpy(), r.in_image.cpu().numpy()


def project(means3D_deform, viewpoint_camera):
    """Drop-in for the reference's `project` (render.py:77-92): [N,3] positions (numpy or tensor) -> float32 tensor [N,2] of pixel
    coordinates in the camera, on the positions' device (a numpy array goes to the GPU when there is one, as the reference's)."""
    from gaussian_renderer import _project
    X = _float(means3D_deform, "means3D_deform", "project")
    if not torch.is_tensor(means3D_deform) and torch.cuda.is_available():
        X = X.cuda()
    if X.dim() != 2 or X.shape[1] != 3:
        raise ValueError(f"project: `means3D_deform` is [N,3], got {tuple(X.shape)}")
    return _project(viewpoint_camera, X.to(torch.float32).contiguous())


def _rotation_matrices(q):
    """build_rotation of scripts/align_eval_trajs.py:9-27 for [...,4] quaternions, r first, normalised inside -> [...,3,3]"""
    q = q / torch.sqrt(q[..., 0] * q[..., 0] + q[..., 1] * q[..., 1] + q[..., 2] * q[..., 2] + q[..., 3] * q[..., 3])[..., None]
    r, x, y, z = q.unbind(-1)
    rows = [1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y),
            2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x),
            2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)]
    return torch.stack(rows, -1).reshape(q.shape[:-1] + (3, 3))


def _mte_composed(gt, traj, rot, assoc):
    """the formulas of csplat_track_mte from torch operations -> (aligned [T,G,3], err [T,G], mte [G], mean [])"""
    T = gt.shape[0]
    sel = traj[:, assoc]
    if rot is None:
        aligned = sel
    else:
        t0 = gt[0] - sel[0]
        R = _rotation_matrices(rot[:, assoc])
        rel = R @ R[0].transpose(-1, -2)[None]
        shift = (rel @ t0[None, :, :, None])[..., 0]
        shift = torch.cat([t0[None], shift[1:]], 0)
        aligned = sel + shift
    e = gt - aligned
    err = torch.sqrt(e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1] + e[..., 2] * e[..., 2])
    total = err[0]
    for k in range(1, T):
        total = total + err[k]
    mte = total / T
    return aligned, err, mte, mte.sum() / mte.shape[0]


def _mte_kernel(gt, traj, rot, assoc):
    """csplat_track_mte on float32 contiguous GPU tensors (rot may be None), assoc [G] integers in [0, N) -> (aligned, err, mte, mean)"""
    _n.require_cuda(gt, traj, rot, assoc)
    (T, G), N, dev = gt.shape[:2], traj.shape[1], traj.device
    a32 = assoc.to(torch.int32).contiguous()
    aligned = torch.empty(T, G, 3, dtype=torch.float32, device=dev)
    err = torch.empty(T, G, dtype=torch.float32, device=dev)
    mte = torch.empty(G + 1, dtype=torch.float32, device=dev)          # (the mean behind the per-track values: one allocation)
    _n.launch("csplat_track_mte", dev, T, N, G, _n.ptr(traj), _n.ptr(rot), _n.ptr(gt), _n.ptr(a32), _n.ptr(aligned), _n.ptr(err), mte.data_ptr(),
              mte[G:].data_ptr())
    return aligned, err, mte[:G], mte[G]


def _closest(gt0, p0):
    """find_closest_gauss for CPU tensors: the nearest point on squared distances, a tie to the smaller index"""
    out = []
    for lo in range(0, gt0.shape[0], 1024):
        d = gt0[lo:lo + 1024, None, :] - p0[None]
        d2 = (d * d).sum(-1)
        best = d2.min(1, keepdim=True).values
        idx = torch.arange(p0.shape[0])[None].expand_as(d2)
        out.append(torch.where(d2 == best, idx, torch.full_like(idx, p0.shape[0])).min(1).values)
    return torch.cat(out)


def mean_trajectory_error(gt_traj, traj, rotations=None, *, align=True, assoc=None):
    """The reference's trajectory evaluation (scripts/align_eval_trajs.py) -> TrajectoryError(mean, per_track, aligned, assoc).
      gt_traj    [T,G,3] ground-truth tracks          traj   [T,N,3] tracked points (Tracks.traj, all_trajs.npz `traj`)
      rotations  [T,N,4] the points' quaternions, r first, any norm but zero (`rotations` of the same file); needed when align
      align      True: the reference's align_traj -- the offset t0 = gt[0] - traj[0] of a track is carried along by the relative rotation
                 R_k R_0^T of its point; False: no alignment, traj[:, assoc] is compared as it is (render.py's `deform[gt_idxs]`)
      assoc      [G] integers in [0, N): the tracked point of each ground-truth track; None: the nearest point to gt_traj[0] in traj[0]
                 (csplat.external.find_closest_gauss: exact, a tie to the smaller index)
    per_track[g] = mean_k |gt[k,g] - aligned[k,g]|, mean = mean_g per_track[g].  A zero quaternion gives NaN, as in the reference."""
    what = "mean_trajectory_error"
    gt, tr = _float(gt_traj, "gt_traj", what), _float(traj, "traj", what)
    if gt.dim() != 3 or gt.shape[2] != 3 or tr.dim() != 3 or tr.shape[2] != 3:
        raise ValueError(f"{what}: `gt_traj` is [T,G,3] and `traj` [T,N,3], got {tuple(gt.shape)} and {tuple(tr.shape)}")
    T, G, N = int(gt.shape[0]), int(gt.shape[1]), int(tr.shape[1])
    if tr.shape[0] != T or T < 1 or G < 1 or N < 1:
        raise ValueError(f"{what}: `gt_traj` {tuple(gt.shape)} and `traj` {tuple(tr.shape)} share T >= 1 frames; G and N are >= 1")
    if align and rotations is None:
        raise ValueError(f"{what}: align=True needs `rotations` [T,N,4]; pass align=False to compare without alignment")
    dev, dt = tr.device, tr.dtype
    gt = gt.to(dev)
    rot = None
    if align:
        rot = _float(rotations, "rotations", what).to(dev)
        if tuple(rot.shape) != (T, N, 4):
            raise ValueError(f"{what}: `rotations` is {[T, N, 4]} next to this `traj`, got {list(rot.shape)}")
    if assoc is None:
        if tr.is_cuda:
            from .external import find_closest_gauss
            idx = torch.from_numpy(find_closest_gauss(gt[0], tr[0]))
        else:
            idx = _closest(gt[0].to(torch.float32), tr[0].to(torch.float32))
    else:
        idx = _tensor(assoc, "assoc", what)
        if idx.dtype.is_floating_point or idx.dtype == torch.bool or tuple(idx.shape) != (G,):
            raise ValueError(f"{what}: `assoc` holds {G} integers, got {idx.dtype} {list(idx.shape)}")
        idx = idx.to(torch.int64)
        if int(idx.min()) < 0 or int(idx.max()) >= N:
            raise ValueError(f"{what}: `assoc` must lie in [0, {N}), got {int(idx.min())} .. {int(idx.max())}")
    idx = idx.to(dev)
    if tr.is_cuda:
        why = "dtype" if (gt.dtype != dt or (rot is not None and rot.dtype != dt)) else None
        if why is None:
            tr, gt = tr.contiguous(), gt.contiguous()
            rot = None if rot is None else rot.contiguous()
            why = _n.why_not_f32c(tr, gt, rot)
        if why is None:
            aligned, _err, mte, mean = _mte_kernel(gt, tr, rot, idx)
            return TrajectoryError(mean, mte, aligned, idx)
        _n.composed_fallback("tracking.mean_trajectory_error", why, tr)
    aligned, _err, mte, mean = _mte_composed(gt.to(dt), tr, None if rot is None else rot.to(dt), idx)
    return TrajectoryError(mean, mte, aligned, idx)


class Tracks(NamedTuple):
    """what track() collected: T distinct times, N tracked points, F view-frames"""
    times: torch.Tensor             # [T] float64, ascending (host)
    traj: torch.Tensor              # [T,N,3] positions per time
    rotations: torch.Tensor         # [T,N,4] quaternions per time, r first
    view_ids: torch.Tensor          # [F] int64 (host): view.view_id, or the view's place in `views` without one
    time_ids: torch.Tensor          # [F] int64 (host): the row of `times` / `traj` of each view-frame
    pixels: torch.Tensor            # [F,N,2]
    in_image: torch.Tensor          # [F,N] bool
    visible: torch.Tensor           # [F,N] bool
    gt_idxs: torch.Tensor           # [G] int64: the tracked point nearest to each ground-truth point at the first time; arange(N) without gt
    counts: Optional[torch.Tensor] = None      # [F,2] int32: (in the image, visible) per view-frame

    def save_npz(self, path):
        """the reference's all_trajs.npz (render.py:34-58): `traj` [T,N,3] and `rotations` [T,N,4]"""
        np.savez(path, traj=self.traj.detach().cpu().numpy(), rotations=self.rotations.detach().cpu().numpy())

    def mte(self, gt_traj, align=True):
        """mean_trajectory_error of these tracks against gt_traj [T,G,3]"""
        return mean_trajectory_error(gt_traj, self.traj, self.rotations if align else None, align=align)


def track(views, gaussians, simulator, pipe, bg_color, *, track_vertices=False, gt=None, depth_threshold=0.2, min_depth=1.0):
    """The tracking collection of the reference's render.py (--log_deform, --show_flow, --track_vertices) -> Tracks.  Every view is
    rendered once under no_grad; positions (means3D_deform, or vertice_deform when track_vertices), their rotations (render's, or
    get_vertice_rotation) and the depth image stay on the device; positions and rotations are kept once per distinct time; then ONE
    csplat_track_visibility launch judges all view-frames -- no host read per frame.  gt [T,G,3] or its first frame [G,3] (optional):
    gt_idxs are the tracked points nearest to gt at the first time."""
    from gaussian_renderer import render
    views = list(views)
    if not views:
        raise ValueError("track: `views` is empty")
    sizes = {(int(v.image_height), int(v.image_width)) for v in views}
    if len(sizes) != 1:
        raise ValueError(f"track: the views must share one image size, got {sorted(sizes)}")
    H, W = next(iter(sizes))
    times = sorted({float(v.time) for v in views})
    row = {t: k for k, t in enumerate(times)}
    traj, rots = [None] * len(times), [None] * len(times)
    depths, fulls, centres = [], [], []
    with torch.no_grad():
        for v in views:
            res = render(v, gaussians, simulator, pipe, bg_color, project_vertices=track_vertices)
            k = row[float(v.time)]
            if traj[k] is None:
                traj[k] = res.vertice_deform if track_vertices else res.means3D_deform
                rots[k] = gaussians.get_vertice_rotation(res.vertice_deform) if track_vertices else res.rotations
            dev = traj[k].device
            depths.append(res.depth.reshape(H, W))
            fulls.append(v.full_proj_transform.to(dev))
            centres.append(v.camera_center.to(dev))
        traj, rots = torch.stack(traj).float(), torch.stack(rots).float()
        time_ids = torch.tensor([row[float(v.time)] for v in views], dtype=torch.int64)
        vis = track_visibility(traj[time_ids.to(traj.device)], torch.stack(fulls).float(), torch.stack(centres).float(),
                               torch.stack(depths).float(), (H, W), depth_threshold=depth_threshold, min_depth=min_depth)
        N = traj.shape[1]
        if gt is None:
            gt_idxs = torch.arange(N, device=traj.device)
        else:
            from .external import find_closest_gauss
            g0 = _float(gt, "gt", "track")
            g0 = g0[0] if g0.dim() == 3 else g0
            gt_idxs = torch.from_numpy(find_closest_gauss(g0, traj[0])).to(traj.device)
    view_ids = torch.tensor([int(getattr(v, "view_id", i)) for i, v in enumerate(views)], dtype=torch.int64)
    return Tracks(torch.tensor(times, dtype=torch.float64), traj, rots, view_ids, time_ids, vis.pixels, vis.in_image, vis.visible, gt_idxs,
                  vis.counts)
