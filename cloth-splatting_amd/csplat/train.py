"""train_step analogue (BASELINE.json configs[2]): the call pattern of
/root/reference/scene_reconstruction/train_utils.py:240-321 around the hot path -- for the cameras of the mini-batch
(3 consecutive timesteps of one view, scene_reconstruction/dataset.py:75-87) simulator -> mesh->Gaussian transform -> HIP rasterizer,
all cameras in one call; L1 + lambda_dssim*(1-SSIM) (train_utils.py:50-74); regularisation (train_utils.py:77-100); the optional
depth / silhouette, Chamfer, kNN-graph and optical-flow terms; ONE backward; the summed screen-space gradient / radii / visibility (:276-292); with
`densify_opt` the reference's densification / pruning / opacity-reset schedule (:295-307, csplat/densify.py); two Adam steps
(:310-319).  The step also runs view-parallel (csplat/dist.py) and recorded into a hipGraph (captured_step.py).  Host-side torch only.
This module is the way in: image_loss.py, geometry_loss.py, flow_loss.py, cloth_regs.py and captured_step.py are re-exported here; train_step and
its stages stay here because tests replace `render_views`, `render`, `geometry_losses` and `cd` as globals of THIS module."""
from types import SimpleNamespace

import torch

from gaussian_renderer import render, render_views
from . import dist as cd
from . import native as _n
from .densify import densification
from .image_loss import (_mask_layout, l1_loss, _taps, _L1_SCRATCH, _IMG_SCRATCH, FusedL1, GaussianBlur11, FusedSSIM,  # noqa: F401
                         FusedImageLoss, _image_loss_fusable, ssim, psnr, image_losses)
from .geometry_loss import _GEOM_SCRATCH, GeometryLoss, geometry_losses  # noqa: F401
from .flow_loss import _FLOW_SCRATCH, FlowLoss, flow_losses  # noqa: F401
from .cloth_regs import (FusedClothRegs, SimulatorStep, simulator_step, _DEFERRED, launch_deferred, edge_csr,  # noqa: F401
                         regularization)
from .captured_step import CapturedStep

# arguments/__init__.py:109-150 overlaid by arguments/cloth_splatting/default.py:1-43
DEFAULT_OPT = SimpleNamespace(lambda_dssim=0.05, lambda_rigid=0.3, lambda_deform_mag=0.01, lambda_momentum=0.1,
                              position_lr_init=0.00016, feature_lr=0.00025, opacity_lr=0.05, scaling_lr=0.005,
                              rotation_lr=0.001, meshnet_lr=3e-4)
DEFAULT_PIPE = SimpleNamespace(compute_cov3D_python=False, convert_SHs_python=False, debug=False)


_ONES = {}
_GT_STACKS = {}          # insertion-ordered: least recently used first
_GT_STACKS_MAX = 8


def _batch_stack(cams, name, field, device):
    """the tensor `name` ("gt_stack" / "mask_stack") that ALL cameras carry and whose rows their `field` ("original_image" / "mask") still
    are, in order (camera i: gt_index == i; the batches of csplat.camera_dataset), when it lies on `device`; None for any other camera list"""
    stack = getattr(cams[0], name, None) if cams else None
    if not torch.is_tensor(stack) or stack.shape[0] != len(cams) or stack.device != device or not stack.is_contiguous():
        return None
    row = stack.stride(0) * stack.element_size()
    for i, cam in enumerate(cams):
        t = getattr(cam, field, None)
        if getattr(cam, name, None) is not stack or getattr(cam, "gt_index", None) != i or not torch.is_tensor(t) or \
                t.data_ptr() != stack.data_ptr() + i * row or t.shape != stack.shape[1:] or not t.is_contiguous():
            return None
    return stack


def _gt_stack(cams, device):
    """torch.cat of the cameras' ground-truth images (train_utils.py:262-270 builds it every step).  A caller that cycles through a few
    camera OBJECTS whose images never change (bench_train, the parity runs) gets the stack of a camera set built once: a small LRU
    (8 sets) keyed on the image tensors' identities and in-place versions.  The entry holds WEAK references to the source images -- an id
    recycled by a new tensor cannot alias (the dead reference no longer matches) and nothing of the caller's is pinned.  The
    reference's dataset builds a fresh Camera per item (scene_reconstruction/dataset.py:89-): such a caller never hits, and then the
    cache costs eight stale stacks at most (it used to hold up to 512 entries with strong references to the sources).
    The cameras of a csplat.camera_dataset step ARE slices of one stack: it is handed through (_batch_stack)."""
    stack = _batch_stack(cams, "gt_stack", "original_image", device)
    if stack is not None:
        return stack
    import weakref
    imgs = [cam.original_image for cam in cams]
    key = tuple((id(t), t._version) for t in imgs) + (str(device),)
    hit = _GT_STACKS.get(key)
    if hit is not None and all(r() is t for r, t in zip(hit[0], imgs)):
        _GT_STACKS[key] = _GT_STACKS.pop(key)          # most recently used: to the back
        return hit[1]
    stack = torch.cat([t.to(device).unsqueeze(0) for t in imgs], 0)
    _GT_STACKS.pop(key, None)
    while len(_GT_STACKS) >= _GT_STACKS_MAX:
        _GT_STACKS.pop(next(iter(_GT_STACKS)))
    _GT_STACKS[key] = ([weakref.ref(t) for t in imgs], stack)
    return stack


@torch.no_grad()
def step_stats(grads, radii_list, P, dev, dtype=torch.float32, out_vsg=None):
    """train_utils.py:276-285 for the cameras of a step: (sum of the screen-space gradients [P,3], largest radii [P], visible [P] bool).
    On the GPU one launch (csplat_step_stats) for up to 16 cameras; a camera whose gradient is None counts as zero.  out_vsg: an fp32
    [P,3] tensor the sum is written into (the tail of the view-parallel step's flat buffer) instead of fresh memory."""
    if not radii_list:
        return (torch.zeros(P, 3, dtype=dtype, device=dev), torch.zeros(P, dtype=torch.int32, device=dev),
                torch.zeros(P, dtype=torch.bool, device=dev))
    V = len(radii_list)
    ok = V <= 16 and all(r.is_cuda and r.dtype == torch.int32 and r.is_contiguous() and r.numel() == P for r in radii_list) and \
        all(g is None or (g.is_cuda and g.dtype == torch.float32 and g.is_contiguous() and g.numel() == 3 * P) for g in grads)
    if ok:
        vsg = out_vsg if (out_vsg is not None and out_vsg.is_cuda and out_vsg.dtype == torch.float32 and out_vsg.is_contiguous() and
                          out_vsg.numel() == 3 * P) else torch.empty(P, 3, dtype=torch.float32, device=dev)
        radii = torch.empty(P, dtype=torch.int32, device=dev)
        vis = torch.empty(P, dtype=torch.bool, device=dev)
        _n.launch("csplat_step_stats", dev, P, V, _n.ptr_table(grads), _n.ptr_table(radii_list), _n.ptr(vsg), _n.ptr(radii), _n.ptr(vis))
        return vsg.to(dtype), radii, vis
    if radii_list[0].is_cuda:
        _n.composed_fallback("train.step_stats", "shape" if V > 16 else "dtype", radii_list[0])
    live = [g for g in grads if g is not None]
    vsg = torch.stack(live).sum(0) if live else torch.zeros(P, 3, dtype=dtype, device=dev)
    radii = torch.stack(list(radii_list), 0).max(dim=0).values
    return vsg, radii, radii > 0


def _root_one(loss):
    """a resident 1.0 as the root gradient of `loss.backward()` (autograd otherwise launches a fill for it every step)"""
    key = (loss.device, loss.dtype)
    if key not in _ONES:
        _ONES[key] = torch.ones((), dtype=loss.dtype, device=loss.device)
    return _ONES[key]


def _geometry_weights(opt):
    """(lambda_depth, lambda_silhouette) of an options namespace; absent = 0.  A term is on when its weight is > 0."""
    lam_d, lam_s = float(getattr(opt, "lambda_depth", 0.0) or 0.0), float(getattr(opt, "lambda_silhouette", 0.0) or 0.0)
    if lam_d < 0.0 or lam_s < 0.0:
        raise ValueError(f"train_step: lambda_depth and lambda_silhouette are >= 0, got {lam_d}, {lam_s}")
    return lam_d, lam_s


def _geometry_targets(cams, lam_d, lam_s):
    """the cameras' `depth` / `silhouette` images of the terms that are on (float32, [1,H,W] or [H,W]) -> (depths or None, silhouettes or
    None); ValueError for a camera that lacks a field or carries another shape or dtype, for cameras of different sizes and for a mask
    that is not one float32 plane -- all from the host-side attributes, before anything is launched"""
    sizes = {(int(c.image_height), int(c.image_width)) for c in cams}
    if len(sizes) > 1:
        raise ValueError(f"train_step: the depth and silhouette terms need cameras of one image size, got {sorted(sizes)}")

    def field(cam, name, what, needed=True):
        t = getattr(cam, name, None)
        if t is None and not needed:
            return None
        H, W = int(cam.image_height), int(cam.image_width)
        if not torch.is_tensor(t):
            raise ValueError(f"train_step: {what} needs every camera's `{name}` (a float32 [1,{H},{W}] or [{H},{W}] tensor), "
                             f"got {type(t).__name__}")
        if t.dtype != torch.float32 or tuple(t.shape) not in ((1, H, W), (H, W)):
            raise ValueError(f"train_step: camera.{name} is {t.dtype} {tuple(t.shape)}, expected float32 [1,{H},{W}] or [{H},{W}]")
        return t

    for cam in cams:
        field(cam, "mask", "a masked depth / silhouette term", needed=False)
    return ([field(c, "depth", "lambda_depth > 0") for c in cams] if lam_d > 0.0 else None,
            [field(c, "silhouette", "lambda_silhouette > 0") for c in cams] if lam_s > 0.0 else None)


def _chamfer_weight(opt):
    """(lambda_chamfer, squared cap or None) of an options namespace; absent = 0.  The term is on when the weight is > 0."""
    lam = float(getattr(opt, "lambda_chamfer", 0.0) or 0.0)
    if not lam >= 0.0:
        raise ValueError(f"train_step: lambda_chamfer is >= 0, got {lam}")
    cap = getattr(opt, "chamfer_max_dist", None)
    if cap is not None:
        cap = float(cap)
        if not cap >= 0.0:
            raise ValueError(f"train_step: chamfer_max_dist is a distance >= 0 (or None), got {cap}")
        cap = cap * cap
    return lam, cap


def _chamfer_targets(cams):
    """the cameras' observed point clouds (`points`, float32 [n,3], n >= 1, world coordinates); ValueError for a camera that lacks the
    field or carries another shape or dtype -- from the host-side attributes, before anything is launched"""
    out = []
    for cam in cams:
        t = getattr(cam, "points", None)
        if not torch.is_tensor(t):
            raise ValueError(f"train_step: lambda_chamfer > 0 needs every camera's `points` (a float32 [n,3] tensor), got {type(t).__name__}")
        if t.dtype != torch.float32 or t.dim() != 2 or t.shape[1] != 3 or t.shape[0] == 0:
            raise ValueError(f"train_step: camera.points is {t.dtype} {tuple(t.shape)}, expected float32 [n,3] with n >= 1")
        out.append(t)
    return out


def _neighbour_options(opt, iteration=None, static=False):
    """the kNN-graph regularisers' options of a namespace (absent = 0 / off): dict(lams=(isometric, spring, rigidity), lambda_w, k,
    update, reg_iter, iso_abs); ValueError for a bad value.  With `iteration` given: None unless the term is ON -- some weight > 0, the
    step is not static, iteration > reg_iter."""
    lams = []
    for name in ("lambda_isometric", "lambda_spring", "lambda_rigidity"):
        v = float(getattr(opt, name, 0.0) or 0.0)
        if not (v >= 0.0 and v <= 3.0e38):
            raise ValueError(f"train_step: {name} is a finite number >= 0, got {v}")
        lams.append(v)
    o = dict(lams=tuple(lams), on=max(lams) > 0.0)
    if not o["on"]:
        return None if iteration is not None else o
    lw = getattr(opt, "lambda_w", None)
    o["lambda_w"] = 2000.0 if lw is None else float(lw)
    if not (o["lambda_w"] >= 0.0 and o["lambda_w"] <= 3.0e38):
        raise ValueError(f"train_step: lambda_w is a finite number >= 0, got {o['lambda_w']}")
    for key, name, default, least in (("k", "k_nearest", 20, 1), ("update", "knn_update_iter", 1000, 1), ("reg_iter", "reg_iter", 0, 0)):
        v = getattr(opt, name, None)
        v = default if v is None else v
        if isinstance(v, bool) or not isinstance(v, int) or v < least:
            raise ValueError(f"train_step: {name} is an integer >= {least}, got {v!r}")
        o[key] = v
    if o["k"] > 32:
        raise ValueError(f"train_step: k_nearest is at most 32 (simple_knn.MAX_K), got {o['k']}")
    o["iso_abs"] = bool(getattr(opt, "isometric_abs", False))
    if iteration is not None and (static or iteration <= o["reg_iter"]):
        return None
    return o


def _neighbour_graph(gaussians, iteration, o):
    """the step's NeighbourGraph: the exact k-NN graph of the detached, UNDEFORMED centres, cached on the Gaussians object; rebuilt when
    absent, when the number of Gaussians (or k / lambda_w) has changed, and every knn_update_iter iterations"""
    from .knn_regs import NeighbourGraph
    key = (int(gaussians.num_gaussians), o["k"], o["lambda_w"])
    cached = gaussians.__dict__.get("_neighbour_graph")
    if cached is None or cached[0] != key or iteration % o["update"] == 0:
        with torch.no_grad():
            pts = gaussians.get_xyz().detach().float().contiguous()
        cached = gaussians._neighbour_graph = (key, NeighbourGraph.from_points(pts, o["k"], o["lambda_w"]), iteration)
    return cached[1]


def _flow_options(opt):
    """(lambda_flow, flow_max_error or None) of an options namespace; absent or 0 = off, no cap.  The term is on when the weight is > 0."""
    lam = float(getattr(opt, "lambda_flow", 0.0) or 0.0)
    if not (lam >= 0.0 and lam <= 3.0e38):
        raise ValueError(f"train_step: lambda_flow is a finite number >= 0, got {lam}")
    cap = getattr(opt, "flow_max_error", None)
    if cap is not None:
        cap = float(cap)
        if not (cap > 0.0 and cap <= 3.0e38):
            raise ValueError(f"train_step: flow_max_error is a finite number of pixels > 0 (or None), got {cap}")
    return lam, cap


def _flow_targets(cams):
    """the flow images of the step's pairs: `camera.flow` of every camera but the last (float32 [2,H,W] or [1,2,H,W], tensor or numpy
    array; pair t is camera t -> camera t+1, the flow defined at camera t's pixels); ValueError for fewer than 2 cameras, a camera that
    lacks the field or carries another shape or dtype, cameras of different image sizes and cameras of different views (where they carry
    a `view_id`) -- all from the host-side attributes, before anything is launched"""
    if len(cams) < 2:
        raise ValueError(f"train_step: the optical-flow term needs at least 2 cameras (consecutive frames of one view), got {len(cams)}")
    sizes = {(int(c.image_height), int(c.image_width)) for c in cams}
    if len(sizes) > 1:
        raise ValueError(f"train_step: the optical-flow term needs cameras of one image size, got {sorted(sizes)}")
    views = {getattr(c, "view_id", None) for c in cams} - {None}
    if len(views) > 1:
        raise ValueError(f"train_step: the optical-flow term needs the frames of ONE view, got view_id {sorted(views)}")
    (H, W), out = next(iter(sizes)), []
    for cam in cams[:-1]:
        f = getattr(cam, "flow", None)
        if f is None or not hasattr(f, "shape") or not hasattr(f, "dtype"):
            raise ValueError(f"train_step: lambda_flow > 0 needs `flow` (float32 [2,{H},{W}] or [1,2,{H},{W}]) on every camera but the last, "
                             f"got {type(f).__name__}")
        if str(f.dtype).split(".")[-1] != "float32" or tuple(f.shape) not in ((2, H, W), (1, 2, H, W)):
            raise ValueError(f"train_step: camera.flow is {f.dtype} {tuple(f.shape)}, expected float32 [2,{H},{W}] or [1,2,{H},{W}]")
        out.append(f)
        m = getattr(cam, "mask", None)
        if m is not None and (not torch.is_tensor(m) or m.dtype != torch.float32 or tuple(m.shape) not in ((1, H, W), (H, W))):
            raise ValueError(f"train_step: a masked optical-flow term needs camera.mask as float32 [1,{H},{W}] or [{H},{W}], got "
                             f"{(m.dtype, tuple(m.shape)) if torch.is_tensor(m) else type(m).__name__}")
    return out


def _refuse_view_parallel(term, plural, view_parallel):
    """an optional term on the view-parallel step (csplat.dist.is_dist()): NotImplementedError"""
    if view_parallel and cd.is_dist():
        raise NotImplementedError(f"train_step: {term} {'are' if plural else 'is'} not part of the view-parallel step")


def _refuse_camera_by_camera(term, plural, batched_views):
    """an optional term with batched_views=False: NotImplementedError"""
    if not batched_views:
        raise NotImplementedError(f"train_step: {term} need{'' if plural else 's'} batched_views=True")


def _optional_terms_on(opt):
    """whether some optional term's weight is > 0 (ValueError for a bad value) -- from the options alone, nothing of the model is read"""
    return (max(_geometry_weights(opt)) > 0.0 or _chamfer_weight(opt)[0] > 0.0 or _neighbour_options(opt)["on"] or
            _flow_options(opt)[0] > 0.0)


def _plan_optional_terms(opt, cams, gaussians, iteration, static, view_parallel, batched_views):
    """What each optional term needs, None when it is off: geometry = (lambda_depth, lambda_silhouette, depths | None, silhouettes | None),
    chamfer = (lambda_chamfer, squared cap | None, clouds), neighbours = the _neighbour_options dict, flow = (lambda_flow, cap | None,
    the pairs' flow images).  Every refusal is raised here, in this order: geometry, Chamfer, kNN, flow; within a term the option value,
    view-parallel, batched_views=False, the cameras / Gaussian count.  Nothing of the model but num_gaussians is read."""
    def carried(term, plural):
        _refuse_view_parallel(term, plural, view_parallel)
        _refuse_camera_by_camera(term, plural, batched_views)
    plan = SimpleNamespace(geometry=None, chamfer=None, neighbours=None, flow=None)
    lam_d, lam_s = _geometry_weights(opt)
    if (lam_d > 0.0 or lam_s > 0.0) and cams:
        carried("the depth and silhouette terms", True)
        plan.geometry = (lam_d, lam_s) + _geometry_targets(cams, lam_d, lam_s)
    lam_c, cap = _chamfer_weight(opt)
    if lam_c > 0.0 and cams:
        carried("the Chamfer term", False)
        plan.chamfer = (lam_c, cap, _chamfer_targets(cams))
    nbr = _neighbour_options(opt, iteration, static) if cams else None
    if nbr is not None:
        carried("the kNN-graph regularisers", True)
        if int(gaussians.num_gaussians) <= nbr["k"]:
            raise ValueError(f"train_step: {int(gaussians.num_gaussians)} Gaussians have no k_nearest = {nbr['k']} neighbours each")
        plan.neighbours = nbr
    lam_f, cap_f = _flow_options(opt)
    if lam_f > 0.0 and cams:
        carried("the optical-flow term", False)
        plan.flow = (lam_f, cap_f, _flow_targets(cams))
    return plan


def _add_optional_terms(plan, reg, pkgs, alphas, masks, gaussians, iteration, cams=()):
    """(reg + the terms of `plan` that are on, their stats): geometry, then Chamfer, then the kNN regularisers, then the optical flow
    (which reads the cameras' full_proj_transform and image size from `cams`) -- the sum rides into the image loss where the
    regularisers alone would"""
    stats = {}
    if plan.geometry is not None:
        # the two terms and their sum with the regularisers: two launches (and one in backward)
        lam_d, lam_s, geom_z, geom_s = plan.geometry
        gdev = alphas[0].device
        reg, gl_d, gl_s = geometry_losses([pkg.depth for pkg in pkgs], alphas,
                                          None if geom_z is None else [t.to(gdev) for t in geom_z],
                                          None if geom_s is None else [t.to(gdev) for t in geom_s], lam_d, lam_s,
                                          masks=None if masks is None else [m[0] for m in masks], add=reg)
        if lam_d > 0.0:
            stats["depth_loss"] = gl_d.detach()
        if lam_s > 0.0:
            stats["silhouette_loss"] = gl_s.detach()
    if plan.chamfer is not None:
        # observed cloud -> deformed Gaussian centres, per camera (the clouds differ in size)
        from .pointcloud import chamfer_distance
        lam_c, cap, clouds = plan.chamfer
        terms = [chamfer_distance(t.to(pkg.means3D_deform.device), pkg.means3D_deform, two_sided=False, max_sq_dist=cap)
                 for t, pkg in zip(clouds, pkgs)]
        chamfer_mean = torch.stack(terms).mean()
        reg = reg + lam_c * chamfer_mean
        stats["chamfer_loss"] = chamfer_mean.detach()
    if plan.neighbours is not None:
        # isometry, spring and rigidity of the deformed centres / rotations over the step's time rows: one launch (and one in backward)
        from .knn_regs import neighbour_regularization
        nbr = plan.neighbours
        graph = _neighbour_graph(gaussians, iteration, nbr)
        # (without a rigidity weight the rotations are not handed over: nothing of them is read, rigidity_loss reports 0)
        nb_loss, nb_parts = neighbour_regularization(torch.stack([pkg.means3D_deform for pkg in pkgs]),
                                                     torch.stack([pkg.rotations for pkg in pkgs]) if nbr["lams"][2] > 0.0 else None,
                                                     graph, *nbr["lams"], isometric_abs=nbr["iso_abs"])
        reg = reg + nb_loss
        stats["isometric_loss"], stats["spring_loss"], stats["rigidity_loss"] = nb_parts.unbind(0)
    if plan.flow is not None:
        # the motion of every Gaussian between consecutive frames against the flow images, and the sum with what came before: two
        # launches (and one in backward); nothing is read back
        lam_f, cap_f, flows = plan.flow
        fdev = pkgs[0].means3D_deform.device
        reg, fl, fn = flow_losses([pkg.means3D_deform for pkg in pkgs], [cam.full_proj_transform.to(fdev).contiguous() for cam in cams],
                                  [_flow_image(f, fdev) for f in flows], (int(cams[0].image_height), int(cams[0].image_width)),
                                  visible=[pkg.radii.reshape(-1) for pkg in pkgs], masks=None if masks is None else [m[0] for m in masks[:-1]],
                                  lambda_flow=lam_f, max_error=cap_f, add=reg)
        stats["flow_loss"], stats["flow_valid"] = fl.detach(), fn.detach()
    return reg, stats


def _flow_image(f, dev):
    """a camera's flow (tensor or numpy array, [2,H,W] or [1,2,H,W]) as a contiguous [2,H,W] tensor on `dev`: the camera's own tensor
    when it is there already"""
    if not torch.is_tensor(f):
        f = torch.from_numpy(f)
    return f.reshape(f.shape[-3:]).to(dev).contiguous()


def _bind_flat_grads(gaussians, simulator, P, world, static, n_total):
    """the view-parallel step's flat gradient buffer, bound as the sink of this step's backward"""
    # one flat buffer: [Gaussian parameters | simulator parameters | tail].  The Gaussian gradients -- ~95 % of the bytes -- are final
    # as soon as the rasterizer's backward and the mesh-transform adjoint have run: their slice is exchanged then (early bucket),
    # under the simulator's and the regularisers' backward.  Tail: the summed screen-space gradient [3P], PSNR, loss, and every
    # rank's largest radii in its own [P] slot (zeros elsewhere), so that the max over ranks rides in the SAME sum
    gparams = list(gaussians.parameters())
    fg = cd.flat_grads_for(gaussians, gparams + list(simulator.parameters()), extra=3 * P + 2 + world * P, early=len(gparams))
    fg.bind(key=(bool(static), n_total))
    return fg


def _deform_all_cameras(all_cams, gaussians, simulator, opt, static, _cap):
    """(vertices [T,V,3] of all cameras, their cloth regularisers with the launch queued for launch_deferred())"""
    # simulator for all cameras at once, and the regularisers recorded BEFORE the rasterizer: autograd runs
    # later-recorded nodes first, so the rasterizer's backward -- the long GPU work of the step -- is launched
    # first and the small launches of everything else are issued under it
    head = simulator_step(simulator, [cam.time for cam in all_cams], gaussians, opt, defer=True,
                          static=None if _cap is None else _cap["sim_in"]) if gaussians.mesh.pos.is_cuda else None
    if head is not None:      # simulator + regularisers: one autograd node (the regularisers' launch queued, see launch_deferred)
        return head
    if hasattr(simulator, "forward_times"):
        deforms_all = simulator.forward_times([cam.time for cam in all_cams])
    else:
        nv, dev0 = gaussians.mesh.pos.shape[0], gaussians.mesh.pos.device
        deforms_all = torch.stack([simulator(time_vector=torch.tensor(cam.time).to(dev0).repeat(nv, 1)) for cam in all_cams])
    # (defer: the regularisers feed nothing before the loss -- their launch waits until the rasterizer's forward has been issued)
    reg, deforms_all = regularization(deforms_all, gaussians, opt, static, tap=True, defer=True)
    return deforms_all, reg


def _render_cameras(cams, gaussians, simulator, pipe, background, static, deforms, want_alpha, batched):
    """(per-camera records, the stacked images or None, the alpha images or None), then the queued regularisers' launch"""
    stacked = alphas = None
    if want_alpha:
        pkgs, stacked, alphas = render_views(cams, gaussians, simulator, pipe, background, render_static=static, return_stacked=True,
                                             vertice_deforms=deforms, by_products=False, return_alpha=True)
    elif batched:
        pkgs, stacked = render_views(cams, gaussians, simulator, pipe, background, render_static=static, return_stacked=True,
                                     vertice_deforms=deforms, by_products=False) if cams else ([], None)
    else:
        pkgs = [render(cam, gaussians, simulator, pipe, background, render_static=static) for cam in cams]
    launch_deferred()
    return pkgs, stacked, alphas


def _image_term(cams, n_total, world, dist_mode, stacked, pkgs, masks, reg, opt, gaussians, _cap):
    """(image loss of this rank's cameras + reg, PSNR mean): one fused launch, or composed; zeros on a rank without a camera"""
    dev = gaussians.face_bary.device
    if cams:
        image_tensor = stacked if stacked is not None else torch.cat([pkg.render.unsqueeze(0) for pkg in pkgs], 0)
        gt_image_tensor = _gt_stack(cams, image_tensor.device) if _cap is None else _cap["gt"]
        mask_tensor = None
        if masks is not None:         # (the masks of a csplat.camera_dataset step are the rows of one tensor already)
            mask_tensor = _batch_stack(cams, "mask_stack", "mask", image_tensor.device)
            mask_tensor = torch.cat(masks, 0) if mask_tensor is None else mask_tensor
        w_img = 1.0 if len(cams) == n_total else len(cams) / n_total
        if _image_loss_fusable(image_tensor, gt_image_tensor, opt, mask_tensor) and reg.dtype == torch.float32:
            # image loss + PSNR + the sum with the regularisers: one launch (and one in backward)
            loss, psnr_, _ = FusedImageLoss.apply(image_tensor, gt_image_tensor, opt.lambda_dssim, mask_tensor, reg, w_img,
                                                  1.0 / world if dist_mode else 1.0, 1.0 / max(n_total, 1))
            if _cap is not None:      # a recorded step: its log line (go word, PSNR, loss, counts) leaves for the host HERE, half a step early
                _cap["log"](psnr_, loss)
            return loss, psnr_
        psnr_sum = psnr(image_tensor, gt_image_tensor).sum().double()
        image_loss = image_losses(image_tensor, gt_image_tensor, opt, mask_tensor)
        if len(cams) != n_total:
            image_loss = image_loss * (len(cams) / n_total)
    else:   # a rank without a camera of this step
        psnr_sum = torch.zeros((), dtype=torch.float64, device=dev)
        image_loss = torch.zeros((), dtype=gaussians.face_bary.dtype, device=dev)
    return image_loss + (reg / world if dist_mode else reg), psnr_sum / max(n_total, 1)


@torch.no_grad()
def _exchange_step_results(fg, P, world, rank, static, n_total, viewspace_grad, radii, psnr_, loss_value, time_allreduce):
    """the view-parallel step's one all-reduce -> (viewspace_grad, radii, visibility_filter, psnr, loss) of ALL ranks' cameras"""
    if viewspace_grad.data_ptr() != fg.tail.data_ptr():       # (csplat_step_stats wrote the sum into the tail already otherwise)
        fg.tail[:3 * P].copy_(viewspace_grad.reshape(-1))
    fg.tail[3 * P] = psnr_.to(fg.tail.dtype)
    fg.tail[3 * P + 1] = loss_value.to(fg.tail.dtype)
    slots = fg.tail[3 * P + 2:].view(world, P)
    slots[rank].copy_(radii)                          # (radii < 2^24: exact in fp32; the other ranks' slots stay zero)
    fg.all_reduce(timed=time_allreduce)
    fg.drop_untouched(key=(bool(static), n_total))
    viewspace_grad = fg.tail[:3 * P].view(P, 3).clone()
    psnr_, loss_value = fg.tail[3 * P].double(), fg.tail[3 * P + 1].clone()
    radii = slots.max(dim=0).values.to(radii.dtype)   # train_utils.py:276-277 over all ranks' cameras
    # (radii > 0 == torch.cat(vis_l).any(dim=0): some camera sees it <=> its largest radius > 0)
    return viewspace_grad, radii, radii > 0, psnr_, loss_value


@torch.no_grad()
def _densify_and_step(iteration, gaussians, meshnet_optimizer, densify_opt, static, visibility_filter, radii, viewspace_grad, _cap):
    """the reference's densification schedule (train_utils.py:295-307), the two optimizer steps, the gradients zeroed"""
    if densify_opt is not None and iteration < densify_opt.densify_until_iter:      # train_utils.py:295-304
        densification(gaussians, iteration, visibility_filter, radii, viewspace_grad, densify_opt,
                      getattr(densify_opt, "cameras_extent", 1.0))
        if iteration % densify_opt.opacity_reset_interval == 0 or (
                getattr(densify_opt, "white_background", False) and iteration == densify_opt.densify_from_iter):
            gaussians.reset_opacity()
    if densify_opt is not None and getattr(densify_opt, "bary_cleanup", 0) and iteration % densify_opt.bary_cleanup == 0:
        gaussians.cleanup_barycentric_coordinates()                                  # train_utils.py:306-307
    # (GroupedAdam.step_now / zero_grad_now: the same step without torch.optim's per-call wrapper; any other optimizer: its own)
    if _cap is not None:          # recorded under stream capture: step count, learning rates and the go / no-go word live on the device
        gaussians.optimizer.step_captured(_cap["valid"])
        meshnet_optimizer.step_captured(_cap["valid"])
    else:
        getattr(gaussians.optimizer, "step_now", gaussians.optimizer.step)()
        if not static:
            getattr(meshnet_optimizer, "step_now", meshnet_optimizer.step)()
    zg = getattr(gaussians.optimizer, "zero_grad_now", None)
    zg() if zg is not None else gaussians.optimizer.zero_grad(set_to_none=True)
    zg = getattr(meshnet_optimizer, "zero_grad_now", None)
    zg() if zg is not None else meshnet_optimizer.zero_grad()


def train_step(iteration, viewpoint_cams, gaussians, simulator, meshnet_optimizer, pipe=DEFAULT_PIPE, opt=DEFAULT_OPT,
               background=None, static=False, view_parallel=False, batched_views=True, densify_opt=None, time_allreduce=False, captured=False,
               _cap=None):
    """One optimisation step.  Returns (psnr, loss, stats) where stats holds what densification consumes.
    batched_views=True renders the step's cameras in one rasterizer call (gaussian_renderer.render_views).
    densify_opt: OptimizationParams-like namespace (+ cameras_extent, white_background) -> the reference's densification /
    pruning / opacity-reset schedule runs between backward and the optimizer step (csplat/densify.py).

    view_parallel=True with more than one rank in the default process group reproduces the SINGLE-GPU step on the full camera
    list (train_utils.py:240-321) with the cameras dealt round-robin over the ranks (csplat/dist.py):
      * the simulator and the cloth regularisers run on ALL cameras on every rank -- the regularisers couple the (t-1, t, t+1)
        triple, which a shard would break -- and enter the local loss with weight 1/world;
      * the image loss is a mean over all images: the local mean enters with weight n_local / n_total; a rank without a camera
        contributes zero but joins the collectives;
      * every parameter gradient, the screen-space gradient sum, the PSNR and the loss value travel in ONE all-reduce(sum) of
        the persistent flat buffer the `.grad` tensors are views of; the radii take one all-reduce(max).
    After the reduction every rank holds exactly the gradients and statistics of the one-rank step (up to summation order)
    and takes the same optimizer / densification decisions, so the replicas stay identical without exchanging parameters.

    Optional terms, the same rules for each: off when its weights are 0 or absent (the step is then exactly the one above); a bad
    option value is a ValueError; a view-parallel step (csplat.dist.is_dist()) and batched_views=False refuse a term that is on with
    NotImplementedError before anything runs (the terms are computed on the batched path only); what it needs of the cameras or the model
    is checked before the simulator runs (ValueError); captured=True runs such a step eagerly; stats holds detached device scalars.
      * `opt.lambda_depth` / `opt.lambda_silhouette` add lambda_depth * L_depth + lambda_silhouette * L_sil of geometry_losses(): the
        views' RenderResults.depth and alpha images (render_views(..., return_alpha=True)) against `camera.depth` (measured z-depth,
        holes 0 / negative / NaN / Inf) and `camera.silhouette` (in [0, 1]), float32 [1,H,W] or [H,W] on every camera, one image size,
        weighted by `camera.mask` when the cameras carry one.  stats: "depth_loss" / "silhouette_loss" for the terms that are on.
      * `opt.lambda_chamfer` adds lambda_chamfer * the mean over the cameras of csplat.pointcloud.chamfer_distance(camera.points, the
        camera's deformed Gaussian centres, two_sided=False, max_sq_dist=opt.chamfer_max_dist ** 2 when that is set); `camera.points`:
        the observed cloud, float32 [n,3] in world coordinates, n >= 1 free per camera.  stats: "chamfer_loss" (the mean).
      * `opt.lambda_isometric`, `opt.lambda_spring`, `opt.lambda_rigidity` add csplat.knn_regs.neighbour_regularization(the views'
        means3D_deform, the views' rotations, in camera order) on the k-NN graph of the undeformed centres: `opt.k_nearest` (absent: 20;
        num_gaussians must exceed it), `opt.lambda_w` (absent: 2000; w = exp(-lambda_w d^2)), rebuilt every `opt.knn_update_iter`
        iterations (absent: 1000) and after the number of Gaussians changed; `opt.isometric_abs` (absent: the reference's signed term).
        On when some weight is > 0, the step is not static and iteration > `opt.reg_iter` (absent: 0).  stats: "isometric_loss",
        "spring_loss", "rigidity_loss" (unweighted; 0 for rigidity without its weight).
      * `opt.lambda_flow` adds lambda_flow * L_flow of csplat.flow_loss.flow_losses(): the motion of every Gaussian's projection between
        consecutive cameras of the step (the views' means3D_deform and full_proj_transform, in camera order) against `camera.flow` of
        every camera but the last -- float32 [2,H,W] or [1,2,H,W], tensor or numpy array, dx / dy in pixels defined at that camera's
        pixels towards the NEXT camera of the step, NaN = no flow there; the last camera's flow is not read.  Needs >= 2 cameras of one
        image size and (where they carry `view_id`) of one view; visibility is the views' radii > 0, weighted by `camera.mask` when
        the cameras carry one; `opt.flow_max_error` (absent / None: no cap; <= 0 is a ValueError) drops pairs whose error in pixels
        exceeds it.  stats: "flow_loss" (L_flow, unweighted), "flow_valid" (the number of valid pairs, int32)."""
    if captured and _cap is None:     # the step as a replayed hipGraph (CapturedStep); falls back to this function when it must
        cs = gaussians.__dict__.get("_captured_step")
        if cs is None or not cs.matches(simulator, meshnet_optimizer, pipe, opt, background):
            cs = gaussians._captured_step = CapturedStep(gaussians, simulator, meshnet_optimizer, pipe, opt, background)
        if not (static or view_parallel or not batched_views or densify_opt is not None):
            return cs(iteration, viewpoint_cams)
    all_cams = list(viewpoint_cams)
    plan = _plan_optional_terms(opt, all_cams, gaussians, iteration, static, view_parallel, batched_views)
    if iteration % 1000 == 0 and _cap is None:
        gaussians.oneupSHdegree()
    _DEFERRED.clear()                 # (a launch queued by a step that raised before issuing it)
    n_total = len(all_cams)
    world, rank = cd.world_rank() if view_parallel else (1, 0)
    dist_mode = view_parallel and cd.is_dist()          # (world > 1, or one rank under CSPLAT_FORCE_DIST: csplat/dist.py)
    idx = cd.shard_indices(n_total, rank, world) if dist_mode else list(range(n_total))
    cams = [all_cams[i] for i in idx]
    P = int(gaussians.num_gaussians)
    fg = _bind_flat_grads(gaussians, simulator, P, world, static, n_total) if dist_mode else None
    masked = bool(all_cams) and getattr(all_cams[0], "mask", None) is not None          # train_utils.py:256
    deforms = reg = None
    if not static and all_cams and (dist_mode or (batched_views and hasattr(simulator, "forward_times"))):
        deforms, reg = _deform_all_cameras(all_cams, gaussians, simulator, opt, static, _cap)
        if dist_mode:
            deforms = deforms[idx] if idx else None
    pkgs, stacked, alphas = _render_cameras(cams, gaussians, simulator, pipe, background, static, deforms,
                                            want_alpha=plan.geometry is not None, batched=dist_mode or batched_views)
    masks = [cam.mask.to(pkg.render.device).unsqueeze(0) for cam, pkg in zip(cams, pkgs)] if masked else None      # train_utils.py:273-274
    dev = gaussians.face_bary.device
    if reg is None:
        verts = [pkg.vertice_deform[None] for pkg in pkgs]
        reg = regularization(torch.cat(verts, 0), gaussians, opt, static) if verts else torch.zeros((), device=dev)
    reg, term_stats = _add_optional_terms(plan, reg, pkgs, alphas, masks, gaussians, iteration, cams)
    loss, psnr_ = _image_term(cams, n_total, world, dist_mode, stacked, pkgs, masks, reg, opt, gaussians, _cap)
    if loss.requires_grad:
        try:
            loss.backward(gradient=_root_one(loss))
        finally:
            if fg is not None:
                fg.unbind()           # (the gradient sinks are for this backward only)
    viewspace_grad, radii, visibility_filter = step_stats([pkg.viewspace_points.grad for pkg in pkgs], [pkg.radii.reshape(-1) for pkg in pkgs],
                                                          P, dev, gaussians.face_bary.dtype,
                                                          out_vsg=fg.tail[:3 * P].view(P, 3) if (fg is not None and pkgs) else None)
    loss_value = loss.detach()
    if dist_mode:
        viewspace_grad, radii, visibility_filter, psnr_, loss_value = _exchange_step_results(
            fg, P, world, rank, static, n_total, viewspace_grad, radii, psnr_, loss_value, time_allreduce)
    _densify_and_step(iteration, gaussians, meshnet_optimizer, densify_opt, static, visibility_filter, radii, viewspace_grad, _cap)
    return psnr_, loss_value, dict(viewspace_grad=viewspace_grad, radii=radii, visibility_filter=visibility_filter,
                                   allreduce_ms=fg.last_allreduce_ms if fg is not None else 0.0, **term_stats)
