"""Drop-in for `diff_gaussian_rasterization` (the depth fork), MI355X-native.

Mirrors the interface the reference binds at gaussian_renderer/__init__.py:16 and calls at :61-76,156-164:
    GaussianRasterizationSettings(image_height, image_width, tanfovx, tanfovy, bg, scale_modifier, viewmatrix,
                                  projmatrix, sh_degree, campos, prefiltered, debug)
    GaussianRasterizer(raster_settings)(means3D, means2D, opacities, shs=None, colors_precomp=None,
                                        scales=None, rotations=None, cov3D_precomp=None) -> (color, radii, depth)
Gradients are delivered for means3D, means2D (NDC-space screen gradient used by densification,
scene_reconstruction/train_utils.py:290-292), shs, colors_precomp, opacities, scales, rotations, cov3D_precomp.
The depth image D = sum_i T_i alpha_i z_i (view-space z, no background term) is differentiable, as in the depth fork of the rasterizer
the reference pins: a loss on it reaches means3D, means2D, opacities, scales / rotations / cov3D_precomp (csplat_backward_depth; without
a depth gradient the backward is exactly the colour-only one).  The camera tensors of the settings (viewmatrix, projmatrix, campos, bg)
receive gradients when they require grad (camera refinement, a learnable background; include/csplat.h csplat_view.dL_dview .. dL_dbg):
only then are they inputs of the autograd Functions, so without them the call is exactly the one without camera gradients.  All compute
is in libcsplat.so: csplat_forward_views_deferred / _settle / _faith and csplat_backward_views, which take their arguments as csplat_view
records; the flat csplat_forward_begin / _finish serve the single-view Function when PER_CALL_SPECULATION is off.
`rasterize_views` renders several independent views in one call, one HIP stream per view.
Beyond upstream, `features=` ([P, F] float32, 1 <= F <= 6) composites per-Gaussian feature channels with the colour's weights and
`return_alpha=True` returns the alpha image 1 - T_final, both differentiable (include/csplat.h, csplat_view.features .. dL_dfeat_in);
without them the call is exactly the upstream one.
`antialiasing=True` (upstream's option of that name; gsplat's rasterize_mode="antialiased") scales every opacity by the ratio of the
footprint areas of the undilated and the 0.3 px^2-dilated 2-D covariance, o' = o sqrt(max(2.5e-5, det0 / det1)), and renders and
differentiates with o' (include/csplat.h, CSPLAT_ANTIALIAS); it composes with everything above.  Without it the call is unchanged.
`return_visibility=True` appends a `Visibility(weight_max, weight_sum, pixel_count, top_id)`: per Gaussian the peak and the summed blending
weight T alpha and the number of pixels it blended into, per pixel the id of the Gaussian with the largest weight (include/csplat.h,
csplat_visibility_views) -- forward only, bit-reproducible.  Without it the call is unchanged.
Which tensor argument, output and returned gradient of the batched Function belongs to which view is the business of one object,
`_CallLayout`, built once per call by `rasterize_gaussians` / `rasterize_views`; what a per-Gaussian input is called, where it is saved
and which gradient field and shape it has is one table, `_INPUTS`; the layout also knows the order of the saved tensors
(tests/test_raster_call_layout_cpu.py needs no GPU).  Where a backward's gradients land -- shared buffers, accumulate bits, every offset in
the step's one allocation -- is decided by a second pure object, `_GradLayout` (tests/test_raster_grad_layout_cpu.py, no GPU), from
which `_plan_backward` fills the csplat_view array.  What one view's forward leaves and its backward needs is one record, `_View`.
"""
import contextlib as _contextlib
import ctypes as C
from math import prod as _prod
from operator import attrgetter as _attrgetter
from typing import NamedTuple

import torch
from torch.autograd.function import once_differentiable
import torch.nn as nn

from csplat import native as _n


class GaussianRasterizationSettings(NamedTuple):
    image_height: int
    image_width: int
    tanfovx: float
    tanfovy: float
    bg: torch.Tensor
    scale_modifier: float
    viewmatrix: torch.Tensor
    projmatrix: torch.Tensor
    sh_degree: int
    campos: torch.Tensor
    prefiltered: bool
    debug: bool


def _f32c(t, device, what="input", per_gaussian=True):
    """fp32, contiguous, on `device`.  The upstream binding takes `.contiguous().data<float>()` of every argument: a non-fp32 tensor
    is REJECTED there and a strided one silently copied.  Here a tensor of another dtype or on another device is converted -- which
    is a torch launch outside the HIP path, so it is reported (csplat.native.composed_fallback: counted, and an error under STRICT,
    kind "dtype"); a strided per-Gaussian tensor is copied like upstream does and reported as kind "layout"; the camera constants
    (4x4 matrices: the reference builds them as `.transpose(0, 1)` views, scene_reconstruction/cameras.py:63-67) are copied
    without a report, exactly upstream's behaviour."""
    if t is None:
        return None
    if t.device != device or t.dtype != torch.float32:
        _n.composed_fallback("diff_gaussian_rasterization." + what, "dtype", t if t.is_cuda else torch.empty(0, device=device))
        t = t.to(device=device, dtype=torch.float32)
    if not t.is_contiguous():
        if per_gaussian:
            _n.composed_fallback("diff_gaussian_rasterization." + what, "layout", t)
        t = t.contiguous()
    return t


def _f32c_grad(t, device):
    """the incoming image gradient: whatever autograd hands over (an expanded scalar, a slice) is made dense -- not the caller's input"""
    if t is None:
        return None
    if t.device != device or t.dtype != torch.float32:
        t = t.to(device=device, dtype=torch.float32)
    return t.contiguous()


def _cam_tensors(rs):
    """the settings tensors that can take a gradient, in the order of a view's trailing argument group"""
    return (rs.viewmatrix, rs.projmatrix, rs.campos, rs.bg)


def _cam_group(rs):
    """the view's trailing argument group when a settings tensor wants a gradient, else () -- the Functions then see exactly the
    inputs they saw before camera gradients existed"""
    cam = _cam_tensors(rs)
    if torch.is_grad_enabled() and any(torch.is_tensor(t) and t.requires_grad for t in cam):
        return cam
    return ()


_CAM_FIELDS = ("dL_dview", "dL_dproj", "dL_dcampos", "dL_dbg")
_CAM_NUMEL = (16, 16, 3, 3)


def _cam_outputs(need, dev):
    """the gradient buffers of one view's camera group (None where no gradient is wanted)"""
    return [torch.empty(n, dtype=torch.float32, device=dev) if w else None for w, n in zip(need, _CAM_NUMEL)]


def _cam_returns(outs, cam_inputs):
    """the buffers in the shape, dtype and device of the tensors the caller passed (autograd routes them on to the leaves, through a
    `.transpose(0, 1)` view too)"""
    return tuple(None if g is None else g.view(t.shape).to(device=t.device, dtype=t.dtype) for g, t in zip(outs, cam_inputs))


def _check_features(features, means3D):
    """-> F of a `features` argument; ValueError unless it is a float32 [P, F] tensor on the device of means3D with 1 <= F <= 6"""
    if not torch.is_tensor(features):
        raise ValueError("features must be a torch.Tensor")
    if features.dtype != torch.float32:
        raise ValueError(f"features must be float32, got {features.dtype}")
    if features.dim() != 2 or features.shape[0] != means3D.shape[0]:
        raise ValueError(f"features must be [P, F] with P = {int(means3D.shape[0])}, got {tuple(features.shape)}")
    if not 1 <= int(features.shape[1]) <= _n.MAX_FEATURES:
        raise ValueError(f"features must have 1 to {_n.MAX_FEATURES} channels, got {int(features.shape[1])}")
    if features.device != means3D.device:
        raise ValueError(f"features must be on {means3D.device}, got {features.device}")
    return int(features.shape[1])


CSPLAT_ANTIALIAS = 2      # csplat.h: csplat_view.prefiltered |= CSPLAT_ANTIALIAS in every view of an antialiased call


class Visibility(NamedTuple):
    """what a view's `return_visibility=True` adds (non-differentiable).  With w_i(pix) = T_i alpha_i, the weight with which the colour
    blended Gaussian i at pix: weight_max [P] float32 = max over pixels (0 where i blends nowhere), weight_sum [P] float32 = the sum,
    pixel_count [P] int32 = the pixels where i blended, top_id [1, H, W] int32 = argmax_i w_i(pix), the front-most on a tie, -1 where
    nothing blended.  `weight_max > thr` is an occlusion-aware replacement of `radii > 0`."""
    weight_max: torch.Tensor
    weight_sum: torch.Tensor
    pixel_count: torch.Tensor
    top_id: torch.Tensor


NVIS = len(Visibility._fields)      # outputs a view's visibility adds to the Function's outputs


def _check_visibility_flag(flag):
    """-> the flag; TypeError unless it is a bool"""
    if not isinstance(flag, bool):
        raise TypeError(f"return_visibility must be a bool, got {type(flag).__name__}")
    return flag


_EAGER_ONLY = "diff_gaussian_rasterization: %s by a forward launched on faith or a captured / replayed step -- %s in an eager step"
_EAGER_ONLY_VIS = _EAGER_ONLY % ("visibility is not computed", "compute it")
_EAGER_ONLY_FEAT = _EAGER_ONLY % ("feature / alpha images are not rendered", "render them")


def _eager_mode_check(message):
    """visibility, feature and alpha images are computed by eager steps only: RuntimeError(message) anywhere else"""
    if _FAITH is not None or _n.REPLAY_STREAM or (torch.cuda.is_available() and torch.cuda.is_current_stream_capturing()):
        raise RuntimeError(message)


class _Input(NamedTuple):
    """one per-Gaussian input of a view"""
    name: str           # the _View attribute (rasterize_gaussians' parameter)
    slot: int           # position among a view's NIN tensor arguments
    saved: object       # position among the saved tensors; None: not saved for the backward
    field: str          # the csplat_view gradient field
    acc: object         # the accumulate bit of a gradient buffer shared between views; None: formed from one view's K7 records, one buffer per view
    shape: object       # (P, M) -> shape of the gradient
    optional: bool      # may be None: present when its saved tensor is; else always present
    temp: bool = False  # K8 writes the buffer even when the input is absent (it is never handed back then)


_INPUTS = (
    _Input("means3D", 0, 0, "dL_dmean3D", _n.ACC_MEAN3D, lambda P, M: (P, 3), False),
    _Input("means2D", 1, None, "dL_dmean2D", None, lambda P, M: (P, 3), False),      # (from this view's K7 moments: one per view)
    _Input("sh", 2, 1, "dL_dsh", _n.ACC_SH, lambda P, M: (P, M, 3), True),
    _Input("colors_precomp", 3, 2, "dL_dcolor", _n.ACC_COLOR, lambda P, M: (P, 3), True, True),
    _Input("opacities", 4, None, "dL_dopacity", _n.ACC_OPACITY, lambda P, M: (P, 1), False),
    _Input("scales", 5, 3, "dL_dscale", _n.ACC_SCALE, lambda P, M: (P, 3), True),
    _Input("rotations", 6, 4, "dL_drot", _n.ACC_ROT, lambda P, M: (P, 4), True),
    _Input("cov3Ds_precomp", 7, 5, "dL_dcov3D", _n.ACC_COV3D, lambda P, M: (P, 6), True, True),
)
NIN = len(_INPUTS)
_IN = {r.name: r for r in _INPUTS}
_SAVED = sorted((r for r in _INPUTS if r.saved is not None), key=lambda r: r.saved)
_SAVED_NAMES = tuple(r.name for r in _SAVED) + ("radii", "color")          # what _View.take_saved() returns, in that order
_SAVED_OF = _attrgetter(*_SAVED_NAMES)
_GRAD_FIELDS = ("dL_dconic",) + tuple(r.field for r in _INPUTS)     # every gradient pointer of a csplat_view the plan sets
_K7_OUT = tuple(r for r in _INPUTS if r.acc is None)        # gradients of one view's K7 records, never shared
_K8_OUT = tuple(r for r in _INPUTS if r.acc is not None)    # gradients K8 writes, into a buffer of their view or a shared one
_BACK_TO_BACK = (_IN["means3D"], _IN["rotations"])          # per-view gradients csplat.gaussians.UnbindViews stacks as a view
SCRATCH_ZEROED, K8_OUTPUTS_UNREAD = 256, 512      # csplat.h: CSPLAT_SCRATCH_ZEROED, CSPLAT_K8_OUTPUTS_UNREAD


def _sh_staged(M, sh):
    """does the library stage this SH tensor's rows through LDS (include/csplat.h, at `M`)?  Only then may views share one dL_dsh
    (CSPLAT_ACC_SH) -- a [P, 16, 3] tensor that is a view into a flat buffer may start off a 16-byte boundary"""
    return M == 16 and sh.data_ptr() % 16 == 0


class _GradLayout:
    """Where every gradient of one batched backward lands, in one pass over the `active` views.  It holds no tensor and calls nothing but
    `sunk` (tests/test_raster_grad_layout_cpu.py needs no GPU); _RasterizeGaussiansBatch._plan_backward fills the csplat_view array from it.
    specs[i] = (P, M, present[slot], first_of[slot]: the first view that got the same tensor object, staged: _sh_staged, scratch: floats of
    per-call scratch or None for the persistent zeroed records).  sunk(view, slot, numel) -> does this owner's gradient go to a gradient
    sink?  Asked in the order the sinks must be claimed (grad_out claims on asking); None: no sinks.
    Per position a in `active`: owner[a][slot] = the view whose buffer the field points at -- itself, or an earlier active view that got the
    same tensor object: mask[a] then carries the row's CSPLAT_ACC_* bit (a dL_dsh only when staged: the unstaged K8 cannot add) -- or None:
    the input is absent, the field NULL.  The `temp` rows own a buffer even when absent (K8 writes it) unless CSPLAT_K8_OUTPUTS_UNREAD says
    that neither is present.  scratch[a] and fields[a] (in the order of _GRAD_FIELDS) are float offsets into the step's ONE allocation of
    `total` floats, None, or the (view, slot) of a sink; ret[a] = the returned (slot, offset or sink, shape).  Buffers lie in 256-byte granules,
    but the _BACK_TO_BACK gradients of DISTINCT, equally sized inputs (the rows of one [T, P, .] tensor upstream) back to back: their stack is a view."""
    __slots__ = ("active", "owner", "mask", "scratch", "fields", "ret", "total")

    def __init__(self, specs, active, sunk=None):
        total, block, at = 0, {}, {}

        def reserve(numel):
            nonlocal total
            off = total
            total += (int(numel) + 63) & ~63          # 256-byte granules
            return off
        equal = len(active) > 1 and len({specs[i][0] for i in active}) == 1
        for row in _BACK_TO_BACK:
            if equal and all(specs[i][3][row.slot] == i and specs[i][2][row.slot] for i in active):
                size = _prod(row.shape(specs[active[0]][0], 0))
                block[row.slot] = (reserve(len(active) * size), size)
        self.active, self.owner, self.mask, self.scratch, self.fields, self.ret = active, [], [], [], [], []
        for a, i in enumerate(active):
            P, M, present, first_of, staged, scratch = specs[i]
            mask = (SCRATCH_ZEROED if scratch is None else 0) | K8_OUTPUTS_UNREAD
            self.scratch.append(None if scratch is None else reserve(scratch))
            own, loc, ret = [None] * NIN, [None] * (1 + NIN), []
            for row in _K7_OUT:
                shape = row.shape(P, M)
                own[row.slot], loc[1 + row.slot] = i, reserve(_prod(shape))
                ret.append((row.slot, loc[1 + row.slot], shape))
            loc[0] = reserve(4 * P)                     # dL_dconic, never handed back
            for row in _K8_OUT:
                slot, there = row.slot, present[row.slot]
                if not there and not row.temp:
                    continue
                if there and row.temp:
                    mask &= ~K8_OUTPUTS_UNREAD
                j = first_of[slot]
                if there and j != i and j in at and (staged or row.name != "sh"):
                    own[slot], loc[1 + slot] = j, self.fields[at[j]][1 + slot]
                    mask |= row.acc
                    continue
                own[slot], shape = i, row.shape(P, M)
                if slot in block:
                    loc[1 + slot] = block[slot][0] + a * block[slot][1]
                else:
                    sink = there and sunk is not None and sunk(i, slot, _prod(shape))
                    loc[1 + slot] = (i, slot) if sink else reserve(_prod(shape))
                if there:
                    ret.append((slot, loc[1 + slot], shape))
            at[i] = a
            self.owner.append(own); self.mask.append(mask); self.fields.append(loc); self.ret.append(ret)
        self.total = total


class _CallLayout:
    """How one call of _RasterizeGaussiansBatch is laid out: the order of its tensor arguments, the order of its outputs and the tuple
    its backward returns.  Beside the settings it holds no tensor, and it calls nothing; `_call_layout` builds it once per call and it
    travels as the Function's first argument.  Index arithmetic on either sequence lives here and nowhere else.
    Tensor arguments: V groups of the NIN per-Gaussian inputs (the slots of _INPUTS); then, when `cam`, V groups of (viewmatrix,
    projmatrix, campos, bg); then, when a view asks for features or alpha (`has_feat`), V feature tensors (None where a view has none).
    An optional group is absent otherwise: the node then has exactly the inputs it had before the option existed.
    Outputs: the stacked colours [V, 3, H, W] when `stacked`; then per view colour (unless stacked), radii, depth, feat (F > 0), alpha
    (when asked for), the NVIS tensors of a Visibility (when asked for)."""

    OUTPUTS = ("color", "radii", "depth", "feat", "alpha") + Visibility._fields

    def __init__(self, settings, stacked, cam, antialias, feat, vis):
        V = self.V = len(settings)
        self.settings, self.stacked, self.cam, self.aa = tuple(settings), bool(stacked), bool(cam), bool(antialias)
        self.feat = [(int(f), bool(a)) for f, a in feat]       # per view (F, return_alpha); F = 0: no features
        self.vis = [bool(x) for x in vis]                      # per view: return_visibility
        self.has_feat = any(f or a for f, a in self.feat)
        self.has_vis = any(self.vis)
        self._cam0 = V * NIN
        self._feat0 = self._cam0 + (4 * V if self.cam else 0)
        self.n_tensors = self._feat0 + (V if self.has_feat else 0)
        self.stacked_output = 0 if self.stacked else None
        self._nsaved = len(_SAVED_NAMES) - (1 if self.stacked else 0)      # per view
        self.n_saved = V * self._nsaved + (1 if self.stacked else 0) + (V if self.has_feat else 0)
        self.outputs, at = [], 1 if self.stacked else 0       # per view {output name: index}, in output order
        for (F, alpha), v in zip(self.feat, self.vis):
            names = [n for n, w in zip(self.OUTPUTS, (not self.stacked, True, True, F > 0, alpha) + (v,) * NVIS) if w]
            self.outputs.append(dict(zip(names, range(at, at + len(names)))))
            at += len(names)
        self.n_outputs = at

    # ---- the tensor arguments.  An index counts from the first tensor: argument 1 + index of apply(), ctx.needs_input_grad[1:][index]
    def index(self, i, slot):
        return i * NIN + slot

    def cam_index(self, i, k):
        return self._cam0 + 4 * i + k if self.cam else None

    def feat_index(self, i):
        return self._feat0 + i if self.has_feat else None

    def pack(self, inputs, feats):
        """per view the NIN inputs and the feature tensor (or None) -> the tensor arguments (the camera groups come from the settings)"""
        tensors = [t for group in inputs for t in group]
        if self.cam:
            tensors += [t for rs in self.settings for t in _cam_tensors(rs)]
        return tensors + list(feats) if self.has_feat else tensors

    # (the accessors take any sequence laid out like the tensor arguments: the arguments themselves, ctx.needs_input_grad[1:])
    def view_inputs(self, tensors, i):
        return tensors[self.index(i, 0):self.index(i, NIN)]

    def cam_group(self, tensors, i):
        return tensors[self.cam_index(i, 0):self.cam_index(i, 4)] if self.cam else ()

    def features(self, tensors, i):
        return tensors[self.feat_index(i)] if self.has_feat else None

    # ---- the outputs
    def output(self, res, i, name):
        """view i's output `name` out of a sequence laid out like the outputs (the outputs, backward's gradients); None: it has none"""
        j = self.outputs[i].get(name)
        return None if j is None else res[j]

    def split(self, res):
        """the Function's outputs -> what rasterize_views returns: per view (color, radii, depth[, feat][, alpha][, Visibility]); with
        `stacked` (colors, [those tuples, color = colors[i]])"""
        colors = res[0] if self.stacked else None
        views = []
        for i, o in enumerate(self.outputs):
            t = [colors[i]] if self.stacked else []
            t += [res[j] for j in o.values()]
            if self.vis[i]:
                t[-NVIS:] = [Visibility(*t[-NVIS:])]
            views.append(tuple(t))
        return (colors, views) if self.stacked else views

    # ---- what is saved for the backward
    def pack_saved(self, per_view, colors=None, feats=()):
        """per view what _View.take_saved() returns, the stacked colours, per view the feature tensor (or None) -> the saved list: per view
        the _SAVED_NAMES (its colour only unless `stacked`); the stacked colours when `stacked`; the feature tensors when `has_feat`"""
        saved = [t for s in per_view for t in s[:self._nsaved]]
        if self.stacked:
            saved.append(colors)
        return saved + list(feats) if self.has_feat else saved

    def saved_input(self, saved, i, name):
        """view i's `name` of _SAVED_NAMES (its colour in a `stacked` call: the stacked colours, view i = row i)"""
        at = _SAVED_NAMES.index(name)
        return saved[i * self._nsaved + at if at < self._nsaved else self.V * self._nsaved]

    def saved_features(self, saved):
        """per view its feature tensor (None where it has none); () without `has_feat`"""
        return saved[self.n_saved - self.V:self.n_saved] if self.has_feat else ()

    # ---- what backward returns
    def grads(self, per_gaussian=None, cam=None, feat=None):
        """backward's return value: per_gaussian[i] = view i's NIN gradients, cam[i] = the 4 of its camera group, feat[i] = its feature
        tensor's -- each, and each entry, may be None; None for the layout and for every other input"""
        out = [None] * (1 + self.n_tensors)
        for seq, index, n in ((per_gaussian, self.index, NIN), (cam, self.cam_index, 4)):
            for i, g in enumerate(seq or ()):
                if g is not None:
                    out[1 + index(i, 0):1 + index(i, n)] = g
        for i, g in enumerate(feat or ()):
            out[1 + self.feat_index(i)] = g
        return tuple(out)


def _call_layout(settings, stacked, antialias, feat, vis):
    """the layout of one call (feat / vis: per view (F, return_alpha) / return_visibility, already checked).  The camera groups are
    passed only when a settings tensor wants a gradient.  Raises, before any launch, what a call with features or visibility may raise."""
    layout = _CallLayout(settings, stacked, any(_cam_group(rs) for rs in settings), antialias, feat, vis)
    if layout.has_feat:
        if len({f for f, _a in layout.feat}) > 1:
            raise ValueError("rasterize_views: every view must have the same number of feature channels, got "
                             f"{[f for f, _a in layout.feat]}")
        _eager_mode_check(_EAGER_ONLY_FEAT)
    if layout.has_vis:
        _eager_mode_check(_EAGER_ONLY_VIS)
    return layout


def _check_one_of_each(shs, colors_precomp, scales, rotations, cov3D_precomp):
    """upstream's checks of a view's arguments, with upstream's messages"""
    if (shs is None) == (colors_precomp is None):
        raise Exception('Please provide excatly one of either SHs or precomputed colors!')
    if ((scales is None or rotations is None) and cov3D_precomp is None) or \
            ((scales is not None or rotations is not None) and cov3D_precomp is not None):
        raise Exception('Please provide exactly one of either scale/rotation pair or precomputed 3D covariance!')


def rasterize_gaussians(means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp,
                        raster_settings, features=None, return_alpha=False, antialiasing=False, return_visibility=False):
    """One camera (what GaussianRasterizer.forward calls, gaussian_renderer/__init__.py:156-164).  Since round 5 a single view goes
    through the same library entry as a batch of views (csplat_forward_views_deferred with V = 1): from the second call of an image size
    on, the second forward phase is launched on the previous call's capacities and the counts are read AFTER the host has prepared the
    backward -- a camera-by-camera loop (the reference's train_utils.py:259-272) no longer leaves the GPU idle for a host round trip per
    camera.  Images, radii, depth and gradients are those of _RasterizeGaussians (tests: test_batched_views_equal_single_view_calls)."""
    vis = _check_visibility_flag(return_visibility)
    F = _check_features(features, means3D) if features is not None else 0
    # features, alpha, antialiasing and visibility exist in the batched Function only: csplat_forward_views_* render the extra images and
    # carry the antialiasing bit to K1 and K8, csplat_backward_views takes the gradients, csplat_visibility_views reads what they leave
    extended = bool(F or return_alpha or antialiasing or vis)
    if not extended and not (PER_CALL_SPECULATION and means3D.is_cuda):
        return _RasterizeGaussians.apply(means3D, means2D, sh, colors_precomp, opacities, scales, rotations,
                                         cov3Ds_precomp, raster_settings, *_cam_group(raster_settings))
    layout = _call_layout((raster_settings,), False, antialiasing, [(F, return_alpha)], [vis])
    if extended:
        _n.require_cuda(means3D)
    tensors = layout.pack([(means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp)], [features])
    return layout.split(_RasterizeGaussiansBatch.apply(layout, *tensors))[0]


PER_CALL_SPECULATION = True      # False: every call waits for its own counts (csplat_forward_begin / _finish, the path of rounds 1-4)


class _View:
    """Everything one view's forward produces and its backward needs.  `fill` writes it into a csplat_view, the record every library entry
    keeps a view's arguments in; `begin` / `finish` are the flat two-phase entries (csplat_forward_begin / _finish), which pack the same
    record themselves."""

    def __init__(self, means3D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, rs, features=None):
        _n.require_cuda(means3D)
        dev = self.dev = means3D.device
        self.rs, self.P = rs, int(means3D.shape[0])
        self.H, self.W = int(rs.image_height), int(rs.image_width)
        self.means3D = _f32c(means3D, dev, "means3D"); self.opacities = _f32c(opacities, dev, "opacities")
        self.sh = _f32c(sh, dev, "shs"); self.colors_precomp = _f32c(colors_precomp, dev, "colors_precomp")
        self.scales = _f32c(scales, dev, "scales"); self.rotations = _f32c(rotations, dev, "rotations")
        self.cov3Ds_precomp = _f32c(cov3Ds_precomp, dev, "cov3D_precomp")
        self.bg = _f32c(rs.bg, dev, "bg", False); self.view = _f32c(rs.viewmatrix, dev, "viewmatrix", False)
        self.proj = _f32c(rs.projmatrix, dev, "projmatrix", False); self.campos = _f32c(rs.campos, dev, "campos", False)
        self.M = int(self.sh.shape[1]) if self.sh is not None else 0
        self.present = [not r.optional or getattr(self, r.name) is not None for r in _INPUTS]      # per slot: the input is there
        self.staged = self.sh is not None and _sh_staged(self.M, self.sh)
        self.features = features                                # [P, F], contiguous: the feature channels the batched forward renders
        self.color = self.radii = self.depth = self.feat = self.alpha = self.vis = None      # the outputs: outputs()
        self.ticket = self.chunks = self.num_rendered = self.layout_rendered = None          # what a forward leaves: adopt()

    def outputs(self, F=0, alpha=False, vis=False, color=None):
        """allocates the view's outputs -- the feature image for F > 0 channels, the alpha image, the tensors of a Visibility; `color`: a
        slice to render into instead of a tensor of its own -> {their names in _CallLayout.OUTPUTS: tensor}"""
        P, H, W = self.P, self.H, self.W
        new = lambda dtype, *shape: torch.empty(*shape, dtype=dtype, device=self.dev)  # noqa: E731
        f32, i32 = torch.float32, torch.int32
        self.color, self.depth, self.radii = new(f32, 3, H, W) if color is None else color, new(f32, 1, H, W), new(i32, P)
        self.feat, self.alpha = new(f32, F, H, W) if F else None, new(f32, 1, H, W) if alpha else None
        made = {"color": self.color, "radii": self.radii, "depth": self.depth, "feat": self.feat, "alpha": self.alpha}
        if vis:
            self.vis = [new(f32, P), new(f32, P), new(i32, P), new(i32, 1, H, W)]
            made.update(zip(Visibility._fields, self.vis))
        return made

    def adopt(self, chunks, num_rendered, layout_rendered):
        """what a forward leaves for the backward: its GEOM, BINNING and IMAGE chunks out of {chunk: buffer} and its counts (num_rendered
        -1: the call is still pending; layout_rendered >= num_rendered: what the binning chunk was laid out for)"""
        self.chunks = (chunks[_n.GEOM], chunks[_n.BINNING], chunks[_n.IMAGE])
        self.num_rendered, self.layout_rendered = int(num_rendered), int(layout_rendered)

    def info_words(self):
        """the int32 [3] view of the device words (tile instances, longest tile list, non-empty tiles) in the IMAGE chunk"""
        off = int(_n.lib.csplat_image_info_offset(self.W, self.H))
        return self.chunks[_n.IMAGE][off:off + 12].view(torch.int32)

    def fill(self, w, stream, tensors=None):
        """the csplat_view fields a forward and a backward call share: sizes, scalars, the input and camera pointers, the output pointers
        and, once a forward has left them, the chunks and their counts.  tensors: (means3D, sh, colors_precomp, opacities, scales, rotations,
        cov3Ds_precomp, color, radii) where the view no longer holds them (a backward: they come out of ctx.saved_tensors)"""
        rs = self.rs
        means3D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, color, radii = tensors or (
            self.means3D, self.sh, self.colors_precomp, self.opacities, self.scales, self.rotations, self.cov3Ds_precomp, self.color, self.radii)
        w.stream = stream
        w.P, w.D, w.M, w.W, w.H = self.P, int(rs.sh_degree), self.M, self.W, self.H
        w.scale_modifier, w.tanfovx, w.tanfovy = float(rs.scale_modifier), float(rs.tanfovx), float(rs.tanfovy)
        w.bg, w.means3D, w.shs, w.colors_precomp = _n.ptr(self.bg), _n.ptr(means3D), _n.ptr(sh), _n.ptr(colors_precomp)
        w.opacities, w.scales, w.rotations = _n.ptr(opacities), _n.ptr(scales), _n.ptr(rotations)
        w.cov3D_precomp, w.view, w.proj, w.campos = _n.ptr(cov3Ds_precomp), _n.ptr(self.view), _n.ptr(self.proj), _n.ptr(self.campos)
        w.out_color, w.radii, w.out_depth = _n.ptr(color), _n.ptr(radii), _n.ptr(self.depth)
        if self.features is not None:
            w.features, w.n_features = _n.ptr(self.features), int(self.features.shape[1])
        w.out_features, w.out_alpha = _n.ptr(self.feat), _n.ptr(self.alpha)
        if self.chunks is not None:
            w.num_rendered, w.layout_rendered = self.num_rendered, self.layout_rendered
            w.geom, w.binning, w.image = (_n.ptr(c) for c in self.chunks)

    def begin(self):
        """K1 + the counting half of the binning on the CURRENT stream; nothing here waits for the GPU."""
        dev, rs = self.dev, self.rs
        self.outputs()
        self.alloc, tk = _n.ChunkAllocator(dev), C.c_int(-1)
        # (in this module: csplat_forward_finish takes a ticket and the entries on csplat_view tables the stream they join LAST -- not
        # native.launch's stream-first form, so they, and csplat_forward_begin beside them, stay on check())
        with _n.on_device(dev):
            rc = _n.lib.csplat_forward_begin(
                _n.stream_handle(dev), self.P, int(rs.sh_degree), self.M, _n.ptr(self.bg), self.W, self.H,
                _n.ptr(self.means3D), _n.ptr(self.sh), _n.ptr(self.colors_precomp), _n.ptr(self.opacities),
                _n.ptr(self.scales), float(rs.scale_modifier), _n.ptr(self.rotations), _n.ptr(self.cov3Ds_precomp),
                _n.ptr(self.view), _n.ptr(self.proj), _n.ptr(self.campos), float(rs.tanfovx), float(rs.tanfovy),
                int(bool(rs.prefiltered)), self.alloc.cb, None, _n.ptr(self.radii), C.byref(tk))
        _n.check(rc, "csplat_forward_begin")
        self.ticket = int(tk.value)

    def finish(self):
        """reads num_rendered (the one host round trip), allocates the R-sized chunks, K3..K6 on the begin() stream"""
        R = C.c_int(0)
        geom, binning, image = C.c_void_p(), C.c_void_p(), C.c_void_p()
        with _n.on_device(self.dev):
            rc = _n.lib.csplat_forward_finish(self.ticket, _n.ptr(self.color), _n.ptr(self.depth), C.byref(R),
                                              C.byref(geom), C.byref(binning), C.byref(image))
        self.ticket = None
        _n.check(rc, "csplat_forward_finish")
        self.adopt(self.alloc.chunks, R.value, R.value)
        self.alloc.cb = self.alloc = None  # break the allocator <-> callback cycle: TEMP / TABLE die here, not at the next cyclic GC

    def backward(self, grad_color, saved, grad_depth=None, cam_need=None):
        """K7 + K8 on the CURRENT stream: csplat_backward_views with this one view (it takes the chunks csplat_forward_finish leaves).
        Returns the per-input gradients in the Function's argument order.  grad_depth None: the colour path; else the depth path, where
        a missing grad_color counts as zero.  cam_need: which of (viewmatrix, projmatrix, campos, bg) want a gradient -- any does: the
        camera path, and a second tuple of the four camera gradients is returned."""
        t = dict(zip(_SAVED_NAMES, saved))
        dev, P, M = self.dev, self.P, self.M
        if grad_color is None:
            grad_color = torch.zeros(3, self.H, self.W, dtype=torch.float32, device=dev)
        grad_color, grad_depth = _f32c_grad(grad_color, dev), _f32c_grad(grad_depth, dev)
        # a buffer per gradient field: the `temp` rows and dL_dconic always (K8 writes them), an optional input's only when it is there
        rows = list(zip(_INPUTS, self.present))
        bufs = {r.field: torch.empty(r.shape(P, M), dtype=torch.float32, device=dev) for r, there in rows if there or r.temp}
        bufs["dL_dconic"] = torch.empty(P, 4, dtype=torch.float32, device=dev)
        grads = tuple(bufs[r.field] if there else None for r, there in rows)
        cam = cam_need is not None and any(cam_need)
        sized = _n.lib.csplat_backward_camera_scratch_bytes if cam else _n.lib.csplat_backward_depth_scratch_bytes
        nbytes = sized(P, self.num_rendered, self.W, self.H) if cam or grad_depth is not None else _n.lib.csplat_backward_scratch_bytes(P, self.num_rendered)
        scratch = _n.temp(dev, nbytes)
        w = _n.CsplatView()
        self.fill(w, _n.stream_handle(dev), (t["means3D"], t["sh"], t["colors_precomp"], None, t["scales"], t["rotations"], t["cov3Ds_precomp"],
                                            t["color"], t["radii"]))
        w.dL_dpix, w.dL_ddepth, w.scratch = _n.ptr(grad_color), _n.ptr(grad_depth), _n.ptr(scratch)
        for f in _GRAD_FIELDS:
            setattr(w, f, _n.ptr(bufs.get(f)))
        cam_out = _cam_outputs(cam_need, dev) if cam else ()
        for f, g in zip(_CAM_FIELDS, cam_out):
            setattr(w, f, _n.ptr(g))
        with _n.on_device(dev):
            rc = _n.lib.csplat_backward_views(1, C.addressof(w), w.stream)
        _n.check(rc, "csplat_backward_views")
        return (grads, cam_out) if cam else grads

    def take_saved(self):
        """-> the tensors of _SAVED_NAMES: they travel through ctx.save_for_backward, only constants and chunks are kept here"""
        saved = _SAVED_OF(self)
        self.means3D = self.sh = self.colors_precomp = self.opacities = self.scales = self.rotations = None
        self.cov3Ds_precomp = self.radii = self.color = self.depth = self.features = self.feat = self.alpha = None
        return saved


class _RasterizeGaussians(torch.autograd.Function):
    @staticmethod
    def forward(ctx, means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, rs, *cam):
        # cam: (viewmatrix, projmatrix, campos, bg) when one of them wants a gradient (_cam_group), else nothing
        ctx.ncam = len(cam)
        v = _View(means3D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, rs)
        v.begin()
        v.finish()
        color, radii, depth = v.color, v.radii, v.depth
        ctx.save_for_backward(*v.take_saved())
        ctx.view_state = v
        ctx.mark_non_differentiable(radii)
        if hasattr(ctx, "set_materialize_grads"):      # (an unused depth image arrives as None: the colour-only call)
            ctx.set_materialize_grads(False)
        return color, radii, depth

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_color, _grad_radii, grad_depth):
        if grad_color is None and grad_depth is None:
            return (None,) * (9 + ctx.ncam)
        if ctx.ncam and any(ctx.needs_input_grad[9:]):
            v = ctx.view_state
            g, cam_out = v.backward(grad_color, ctx.saved_tensors, grad_depth, ctx.needs_input_grad[9:])
            return g + (None,) + _cam_returns(cam_out, _cam_tensors(v.rs))
        return ctx.view_state.backward(grad_color, ctx.saved_tensors, grad_depth) + (None,) * (1 + ctx.ncam)


_side_streams = {}
# K7's per-Gaussian accumulation records, kept from step to step (round 5): zeroed ONCE per (device, stream the work runs on, P, view slot);
# K8 clears every record it consumes (csplat.h: CSPLAT_SCRATCH_ZEROED), so the next step finds them zero again -- no clearing launch and
# no 25.6 MB of zero fill per step.  Launches on one stream cannot overlap, so two backward passes that share a slot are ordered.  A failed
# entry point may leave records behind: the cache is a ticket cache (csplat.native.check drops it, recordings are invalidated).
_ACC_SCRATCH = _n.ScratchCache(cap=32)


def _acc_scratch(dev, P, slot):
    """(tensor, True) = the persistent zeroed records of `slot`; (None, False) in the bit-reproducible mode (its scratch is laid out per call)"""
    if int(_n.lib.csplat_debug_flags_query()) & _n.DEBUG_BIT_REPRODUCIBLE:
        return None, False
    # the hit, once per view and backward pass, stays written out: 0.56 us a call on the host this way, 0.72 us through buffer() alone
    buf = _ACC_SCRATCH.get((dev.index, _n.scratch_stream(dev), int(P), int(slot)))
    if buf is None:
        buf = _ACC_SCRATCH.buffer(dev, (int(P), int(slot)), lambda: max(_n.lib.csplat_backward_scratch_bytes(int(P), 0), 256))
    return buf, True
# how the batched forward's second phase went, per call (bench.py's `speculation` field, tests): "hit" = launched on the previous call's
# capacities before the counts were read and the counts fitted; "miss" = they did not fit and the phase was repeated with exact sizes;
# "wait" = no history for this (image size, P) yet (or speculation off): the counts were read first
SPEC_STATS = {"hit": 0, "miss": 0, "wait": 0}
# the device words (int32 [3] views into the IMAGE chunks: tile instances, longest tile list, non-empty tiles) of the last batched
# forward, per view -- what a caller sizes a launch on faith from (one .cpu() read at a moment of its choosing)
LAST_INFO = []
# ---- launch mode of the batched forward.  Two switches, both PRIVATE and both set only through `forward_mode(...)` below, which restores
# them on exit whatever happens inside (module globals toggled around a capture leak silently -- one leaked flag and the
# oracle-tested path and the timed path diverge):
#   keep_info  the call leaves LAST_INFO (the views cost ~10 us of host time per call)
#   faith      launch ON FAITH (csplat.train.CapturedStep, csplat.graphs.ReplayedSteps): a dict {"caps": (R, L, B), "valid": uint32 tensor
#              [1]} -- the batched forward launches both phases with those capacities and reads NOTHING back
#              (csplat_forward_views_faith): the form a hipGraph capture can record.  The forward leaves in the dict: "info" = per view an
#              int32 [3] VIEW of the device words holding (tile instances, longest tile list, non-empty tiles), to be read whenever the
#              caller syncs anyway.
_KEEP_INFO = False
_FAITH = None


@_contextlib.contextmanager
def forward_mode(faith=None, keep_info=False, replay_device=None):
    """Scope in which the batched forward runs in another launch mode: `faith` / `keep_info` as above; `replay_device` = a device whose
    CURRENT stream is the one the recording made inside this scope will be replayed on (scratch buffers that are "zeroed once per
    stream" are keyed on it instead of on the capture stream, csplat.native.scratch_stream).  Not re-entrant for `faith` /
    `replay_device`: nesting two recordings is a bug and raises."""
    global _FAITH, _KEEP_INFO
    if faith is not None and _FAITH is not None:
        raise RuntimeError("diff_gaussian_rasterization.forward_mode: a launch on faith is already in progress")
    prev = (_FAITH, _KEEP_INFO)
    idx = None
    if replay_device is not None:
        idx = replay_device.index if isinstance(replay_device, torch.device) else int(replay_device)
        idx = torch.cuda.current_device() if idx is None else idx
        if idx in _n.REPLAY_STREAM:
            raise RuntimeError("diff_gaussian_rasterization.forward_mode: a recording for this device is already in progress")
        _n.REPLAY_STREAM[idx] = _n.stream_handle(idx)
    _FAITH = faith if faith is not None else prev[0]
    _KEEP_INFO = bool(keep_info) or prev[1]
    try:
        yield faith
    finally:
        _FAITH, _KEEP_INFO = prev
        if idx is not None:
            _n.REPLAY_STREAM.pop(idx, None)


class DeferredK8:
    """Filled by `deferred_k8()`: the batched backward passes inside the scope launched their K7 only; `launch(slice, nslices)` launches
    the per-Gaussian backward (K8) of one Gaussian range for all of them, `rows(slice, nslices)` says which gradient rows that finishes
    (csplat_backward_views_parts / csplat_backward_slice_rows).  A view-parallel step hands the finished rows to its collective while
    the next slice computes (csplat.dist.FlatGrads.start_ranges).  The entries hold raw pointers of the pass that made them: valid as
    long as its gradient tensors are (for a recorded step: as long as the recording)."""

    def __init__(self):
        self.entries = []           # (csplat_view array, number of views, device, P, keep-alive)

    def launch(self, slice_, nslices):
        for sub, n, dev, _P, _keep in self.entries:
            with _n.on_device(dev):
                rc = _n.lib.csplat_backward_views_parts(n, C.cast(sub, C.c_void_p), torch.cuda.current_stream(dev).cuda_stream, 2, int(slice_),
                                                        int(nslices))
            _n.check(rc, "csplat_backward_views_parts")

    def rows(self, slice_, nslices):
        P = self.entries[0][3]
        lo, hi = C.c_int64(0), C.c_int64(0)
        # (host arithmetic, takes no stream: check(), not native.launch)
        _n.check(_n.lib.csplat_backward_slice_rows(int(P), int(slice_), int(nslices), C.byref(lo), C.byref(hi)), "csplat_backward_slice_rows")
        return int(lo.value), int(hi.value)


_K8_DEFER = None


@_contextlib.contextmanager
def deferred_k8(holder=None):
    """Scope in which `_RasterizeGaussiansBatch.backward` launches the compositing backward (K7) only and leaves the per-Gaussian backward
    (K8) to the caller: `with deferred_k8() as h: loss.backward()`, then `h.launch(g, G)` for g = 0 .. G-1.  The gradient tensors autograd
    has been handed are filled by those launches -- nothing may read them in between: every input of the node must be a LEAF (or feed
    leaves through nodes that do not read values, like views), each receiving its gradient from this node alone."""
    global _K8_DEFER
    if _K8_DEFER is not None:
        raise RuntimeError("diff_gaussian_rasterization.deferred_k8: already inside a deferred_k8 scope")
    _K8_DEFER = holder if holder is not None else DeferredK8()
    try:
        yield _K8_DEFER
    finally:
        _K8_DEFER = None


def forward_mode_is_default():
    """True when no forward_mode scope is open (tests assert it after every recording)"""
    return _FAITH is None and not _KEEP_INFO and not _n.REPLAY_STREAM


def _view_streams(dev, n, main):
    """the caller's stream + n-1 side streams: ROCm maps streams onto 4 hardware queues per device by default, and a
    fifth stream shares a queue with (= is serialised behind) another one"""
    pool = _side_streams.setdefault((dev.type, dev.index), [])
    while len(pool) < n - 1:
        pool.append(torch.cuda.Stream(device=dev))
    return [main] + pool[:n - 1]


# what _RasterizeGaussiansBatch.backward refuses, the first match is raised: (the gradient that arrived, where, the message)
_REFUSALS = (
    ("depth", "faith", "diff_gaussian_rasterization: a depth gradient reached a forward launched on faith (a captured / replayed step); "
                       "those steps take no depth loss -- render the depth term in an eager step"),
    ("feat", "faith", "diff_gaussian_rasterization: a feature / alpha gradient reached a forward launched on faith (a captured / "
                      "replayed step); render feature and alpha images in an eager step"),
    ("feat", "deferred_k8", "diff_gaussian_rasterization: a feature / alpha gradient reached a backward inside deferred_k8(); the sliced "
                            "per-Gaussian backward takes no feature or alpha gradient"),
    ("cam", "faith", "diff_gaussian_rasterization: a camera / background gradient reached a forward launched on faith (a captured / "
                     "replayed step); those steps take no camera gradient -- refine the camera in an eager step"),
    ("cam", "deferred_k8", "diff_gaussian_rasterization: a camera / background gradient reached a backward inside deferred_k8(); the sliced "
                           "per-Gaussian backward takes no camera gradient"),
)


class _Plan:
    """what _plan_backward leaves: the active views, the one allocation, their csplat_view array, per view the NIN gradients to return, the
    gradient sinks it claimed, per view its persistent records or None; `keep`: what backward() attaches (alive as long as the plan)"""
    __slots__ = ("active", "big", "sub", "out", "sinks", "acc", "keep")

    def __init__(self, active, big, sub, out, sinks, acc):
        self.active, self.big, self.sub, self.out, self.sinks, self.acc, self.keep = active, big, sub, out, sinks, acc, []

    def attach_camera(self, cam_need):
        """the camera path (csplat_view.dL_dview .. dL_dbg): the gradient buffers of the views that want them -> {view: its four}"""
        cam_out = {}
        for a, i in enumerate(self.active):
            cam_out[i] = _cam_outputs(cam_need[i], self.big.device)
            for f, g in zip(_CAM_FIELDS, cam_out[i]):
                setattr(self.sub[a], f, _n.ptr(g))
            self.keep += [g for g in cam_out[i] if g is not None]
        return cam_out

    def attach_features(self, ctx, gfeat, galpha, fsaved, need):
        """the feature path (csplat_view.dL_dfeatures / dL_dalpha): one dL_dfeat_in buffer per feature tensor OBJECT that wants a
        gradient, shared by the views it was passed to (the library adds their sums in view order) -> per view its buffer or None"""
        layout, dev = ctx.layout, self.big.device
        fout, owner = [None] * layout.V, {}
        for a, i in enumerate(self.active):
            w, F = self.sub[a], layout.feat[i][0]
            gf, ga = _f32c_grad(gfeat[i], dev), _f32c_grad(galpha[i], dev)
            w.features, w.n_features = _n.ptr(fsaved[i]), F
            w.dL_dfeatures, w.dL_dalpha = _n.ptr(gf), _n.ptr(ga)
            buf = None
            if F and layout.features(need, i):
                key = ctx.feat_first[i]
                if key not in owner:
                    owner[key] = fout[i] = torch.empty(ctx.views[i].P, F, dtype=torch.float32, device=dev)
                buf = owner[key]
            w.dL_dfeat_in = _n.ptr(buf)
            self.keep += [gf, ga]
        return fout

    def attach_depth_scratch(self, views, gdep, scratch_bytes):
        """the depth path (csplat_view.dL_ddepth): every view of the call gets scratch of the depth (camera, feature) layout, allocated
        here (never on the colour-only path) and cleared by the library -- the persistent zeroed records are not used by this call"""
        for a, i in enumerate(self.active):
            v, w = views[i], self.sub[a]
            gd = _f32c_grad(gdep[i], v.dev)
            buf = _n.temp(v.dev, scratch_bytes(v.P, v.layout_rendered, v.W, v.H))
            w.dL_ddepth, w.scratch, w.accmask = _n.ptr(gd), buf.data_ptr(), w.accmask & ~SCRATCH_ZEROED
            self.keep += [gd, buf]


class _RasterizeGaussiansBatch(torch.autograd.Function):
    """V independent views in one autograd node and ONE library call each way (csplat_forward_views /
    csplat_backward_views).  Every view runs on its own HIP stream (the caller's + V-1 side streams, fenced inside the
    library): all K1/K2 are issued before the first num_rendered read, the under-filled compositing kernels of the views
    overlap, and a parameter tensor passed to several views gets ONE gradient buffer that the views' K8 add into.
    Images / radii / depth are bit-identical to V calls of _RasterizeGaussians.
    apply(layout, *tensors): `layout` is the call's _CallLayout, `tensors` what its pack() returns.  forward() reads its inputs through
    the layout's accessors and places its outputs by the layout's names, backward() finds each view's gradients by those names and
    returns layout.grads(...) -- neither counts arguments itself."""

    @staticmethod
    def forward(ctx, layout, *tensors):
        V, stacked = layout.V, layout.stacked
        assert len(tensors) == layout.n_tensors
        ctx.layout = layout
        if layout.has_vis:
            _eager_mode_check(_EAGER_ONLY_VIS)
        if layout.has_feat:
            _eager_mode_check(_EAGER_ONLY_FEAT)
        groups = [layout.view_inputs(tensors, i) for i in range(V)]
        feats = [layout.features(tensors, i) for i in range(V)]
        ctx.feat_first = [next(j for j in range(i + 1) if feats[j] is feats[i]) for i in range(V)]     # (one gradient per tensor object)
        views = [_View(g[0], *g[2:], rs, f.contiguous() if F else None)      # (means2D only receives a gradient)
                 for g, rs, f, (F, _alpha) in zip(groups, layout.settings, feats, layout.feat)]
        dev = views[0].dev
        main, arr = torch.cuda.current_stream(dev), (_n.CsplatView * V)()
        # stacked: the V images land in ONE [V, 3, H, W] tensor (what the reference builds with torch.cat before the loss,
        # scene_reconstruction/train_utils.py:262-270) and that tensor is the node's first output
        colors = None
        if stacked:
            assert all((v.H, v.W) == (views[0].H, views[0].W) for v in views), "stacked output needs equal image sizes"
            colors = torch.empty(V, 3, views[0].H, views[0].W, dtype=torch.float32, device=dev)
        alloc = _n.ChunkAllocator(dev, V)     # (all on the caller's stream: the library fences the view streams around it)
        made = []
        for i, (v, st) in enumerate(zip(views, _view_streams(dev, V, main))):
            made.append(v.outputs(layout.feat[i][0], layout.feat[i][1], layout.vis[i], colors[i] if stacked else None))
            v.fill(arr[i], st.cuda_stream)
            arr[i].prefiltered = int(bool(v.rs.prefiltered)) | (CSPLAT_ANTIALIAS if layout.aa else 0)
            arr[i].alloc_ctx = i
        # the one host read of the call (its counts) is DEFERRED when the library can launch the second phase on the previous call's
        # capacities: everything below that does not need the counts -- the output lists, the backward plan -- is host work done
        # while the GPU runs K1..K6, instead of after a ~45 us wait for K1 / K2
        pending = C.c_int(0)
        try:
            faith = _FAITH
            if faith is not None:
                caps = (C.c_uint32 * 3)(*[int(c) for c in faith["caps"]])
                with _n.on_device(dev):
                    rc = _n.lib.csplat_forward_views_faith(V, C.cast(arr, C.c_void_p), alloc.cb, main.cuda_stream, C.cast(caps, C.c_void_p),
                                                           _n.ptr(faith["valid"]))
                _n.check(rc, "csplat_forward_views_faith")
            else:
                with _n.on_device(dev):
                    rc = _n.lib.csplat_forward_views_deferred(V, C.cast(arr, C.c_void_p), alloc.cb, main.cuda_stream, C.byref(pending))
                _n.check(rc, "csplat_forward_views_deferred")
            outs = [None] * layout.n_outputs
            for i, v in enumerate(views):
                v.adopt(alloc.views[i], arr[i].num_rendered, arr[i].layout_rendered)
                for name, j in layout.outputs[i].items():
                    outs[j] = made[i][name]
            if _FAITH is not None:
                _FAITH["info"] = [v.info_words() for v in views]
            # (mark_non_differentiable keeps its last call's tensors only: all of them in one call)
            ctx.mark_non_differentiable(*[v.radii for v in views], *[t for v in views if v.vis is not None for t in v.vis])
            if stacked:
                outs[layout.stacked_output] = colors
            # (antialiasing: K8 reads the raw opacities through the views' `opacities` pointers -- those tensors live as long as the node)
            ctx.aa_opacities = [v.opacities for v in views] if layout.aa else None
            features = [v.features for v in views]
            ctx.save_for_backward(*layout.pack_saved([v.take_saved() for v in views], colors, features))
            # which view first received each input tensor OBJECT (shared parameters get one gradient buffer)
            ctx.first_of = [[next(j for j in range(i + 1) if groups[j][k] is groups[i][k]) for k in range(NIN)] for i in range(V)]
            ctx.views, ctx.arr, ctx.on_faith = views, arr, _FAITH is not None
            ctx.set_materialize_grads(False)     # an unused view arrives as None in backward() and costs nothing

            def plan():
                return _RasterizeGaussiansBatch._plan_backward(views, arr, ctx.first_of, list(range(V)), groups if _n.GRAD_SINK else None)
            # the GPU is busy with K1..K6 of the views right now: prepare the backward call in its shadow
            ctx.plan = plan() if any(ctx.needs_input_grad) else None
            if not pending.value and _FAITH is None:
                SPEC_STATS["wait"] += 1
            if pending.value:
                relaunched = C.c_int(0)
                with _n.on_device(dev):
                    rc = _n.lib.csplat_forward_views_settle(V, C.cast(arr, C.c_void_p), main.cuda_stream, C.byref(relaunched))
                _n.check(rc, "csplat_forward_views_settle")
                for i, v in enumerate(views):       # the counts; after a miss, new binning chunks and a new layout
                    v.adopt(alloc.views[i], arr[i].num_rendered, arr[i].layout_rendered)
                pending.value = 0
                SPEC_STATS["miss" if relaunched.value else "hit"] += 1
                if relaunched.value and ctx.plan is not None:     # the speculation missed: the plan is rebuilt (rare)
                    _n.grad_release(ctx.plan.sinks)
                    ctx.plan = plan()
                elif ctx.plan is not None:
                    for a, i in enumerate(ctx.plan.active):
                        ctx.plan.sub[a].num_rendered = arr[i].num_rendered
                        ctx.plan.sub[a].busy_tiles = arr[i].busy_tiles
            if layout.has_vis:
                _RasterizeGaussiansBatch._visibility(views, arr, dev, main)
            if _KEEP_INFO and _FAITH is None and len({(v.W, v.H) for v in views}) == 1:
                LAST_INFO[:] = [v.info_words() for v in views]
            return tuple(outs)
        except BaseException:
            if pending.value:        # never leave a call pending in the library (its tickets stay reserved otherwise)
                dummy = C.c_int(0)
                try:
                    with _n.on_device(dev):
                        _n.lib.csplat_forward_views_settle(V, C.cast(arr, C.c_void_p), main.cuda_stream, C.byref(dummy))
                except Exception:
                    pass
            raise
        finally:
            alloc.cb = None          # (the allocator <-> callback cycle: the temporaries die here, not at the next cyclic GC)

    @staticmethod
    def _visibility(views, arr, dev, main):
        """csplat_visibility_views on the views that asked for it (the forward is settled: counts and chunks are final); the scratch is
        freed on the caller's stream, behind the launch"""
        outs, keep = (_n.CsplatVisibility * len(views))(), []
        for o, v in zip(outs, views):
            if v.vis is not None:
                keep.append(_n.temp(dev, _n.lib.csplat_visibility_scratch_bytes(v.P, max(v.layout_rendered, v.num_rendered, 0), v.W, v.H)))
                o.weight_max, o.weight_sum, o.pixel_count, o.top_id = (_n.ptr(t) for t in v.vis)
                o.scratch = keep[-1].data_ptr()
        with _n.on_device(dev):
            rc = _n.lib.csplat_visibility_views(len(views), C.cast(arr, C.c_void_p), C.cast(outs, C.c_void_p), main.cuda_stream)
        _n.check(rc, "csplat_visibility_views")
        for v in views:
            v.vis = None

    @staticmethod
    def _plan_backward(views, arr, first_of, active, inputs=None):
        """Everything of the backward call that does not depend on the incoming gradient values: ONE allocation for every gradient,
        temporary and K7 record of the step and the csplat_view array with all pointers but dL_dpix, as a _GradLayout says.  Built at the
        end of forward(), while the compositing kernels run: backward() is left with pointer patching and one library call.  inputs: the
        call's input tensors -- one with a registered gradient SINK (csplat.native.GRAD_SINK: a view-parallel step's flat buffer) gets its
        gradient written there by K8 and handed to autograd as a fresh view of the sink."""
        dev = views[0].dev
        specs, acc = [None] * len(views), []        # acc: per active view its persistent zeroed records, None in the bit-reproducible mode
        for a, i in enumerate(active):
            v = views[i]
            acc.append(_acc_scratch(dev, v.P, a)[0])
            specs[i] = (v.P, v.M, v.present, first_of[i], v.staged,
                        int(_n.lib.csplat_backward_scratch_bytes(v.P, v.layout_rendered)) // 4 + 64 if acc[a] is None else None)
        sink_of, claimed = {}, []        # (view, slot) -> a fresh view of the input's gradient sink; the sinks this plan claimed

        def sunk(i, slot, numel):
            t = inputs[i][slot]
            sk = _n.grad_sink(t)
            sv = _n.grad_out(sk, t.shape, dev) if sk is not None else None
            if sv is None or sv.numel() != numel or sv.data_ptr() % 16:
                return False
            sink_of[(i, slot)] = sv
            # (only a sink this plan really CLAIMED is given back when the plan is rebuilt: grad_out() hands out fresh memory
            # when another node holds the slice, and releasing that node's claim would let a third writer alias it -- ADVICE r5)
            if sv.data_ptr() == sk[0].data_ptr() + 4 * int(sk[1]):
                claimed.append(sk)
            return True
        lay = _GradLayout(specs, active, sunk if inputs is not None else None)
        big = torch.empty(max(lay.total, 64), dtype=torch.float32, device=dev)
        base, sub = big.data_ptr(), (_n.CsplatView * len(active))()
        out = [None] * len(views)       # per active view its NIN gradients, in slot order
        for a, i in enumerate(active):
            w = sub[a]
            C.memmove(C.byref(w), C.byref(arr[i]), C.sizeof(_n.CsplatView))
            w.scratch = acc[a].data_ptr() if lay.scratch[a] is None else base + 4 * lay.scratch[a]
            w.accmask = lay.mask[a]
            for field, loc in zip(_GRAD_FIELDS, lay.fields[a]):
                setattr(w, field, None if loc is None else sink_of[loc].data_ptr() if loc.__class__ is tuple else base + 4 * loc)
            out[i] = [None] * NIN
            for slot, loc, shape in lay.ret[a]:
                out[i][slot] = sink_of[loc] if loc.__class__ is tuple else big[loc:loc + _prod(shape)].view(shape)
        return _Plan(list(active), big, sub, out, claimed, acc)

    @staticmethod
    @once_differentiable
    def backward(ctx, *grads):
        layout, views, arr = ctx.layout, ctx.views, ctx.arr
        # unpacked on EVERY path: the plan made in forward() holds raw pointers into the inputs, so the usual pass would never touch the saved
        # tensors -- and autograd's version check, which refuses an input edited in place since the forward, runs when they are unpacked
        saved = ctx.saved_tensors
        V, dev = layout.V, views[0].dev
        main = torch.cuda.current_stream(dev)
        need = ctx.needs_input_grad[1:]
        cam_need = [tuple(layout.cam_group(need, i)) for i in range(V)]
        if layout.stacked:
            gstack = grads[layout.stacked_output]
            gcol = [None] * V if gstack is None else [gstack[i] for i in range(V)]
        else:
            gcol = [layout.output(grads, i, "color") for i in range(V)]
        gdep, gfeat, galpha = ([layout.output(grads, i, name) for i in range(V)] for name in ("depth", "feat", "alpha"))
        active = [i for i in range(V) if gcol[i] is not None or gdep[i] is not None or gfeat[i] is not None or galpha[i] is not None]
        if not active:
            return layout.grads()
        want_feat = any(gfeat[i] is not None or galpha[i] is not None for i in active)
        want_cam = any(any(cam_need[i]) for i in active)
        want_depth = any(gdep[i] is not None for i in active)
        arrived = {"depth": want_depth, "feat": want_feat, "cam": want_cam}
        where = {"faith": ctx.on_faith, "deferred_k8": _K8_DEFER is not None}
        for what, place, message in _REFUSALS:
            if arrived[what] and where[place]:
                raise RuntimeError(message)
        plan, ctx.plan = ctx.plan, None                         # (one use: the buffers are handed to autograd)
        # plan again: a view's image went unused, a second backward pass, or the bit-reproducible mode was switched on after the forward
        # (its scratch has another layout)
        if plan is not None and (plan.active != active or (plan.acc[0] is not None and int(_n.lib.csplat_debug_flags_query()) & _n.DEBUG_BIT_REPRODUCIBLE)):
            _n.grad_release(plan.sinks)
            plan = None
        if plan is None:
            plan = _RasterizeGaussiansBatch._plan_backward(views, arr, ctx.first_of, active)
        sub = plan.sub
        plan.keep += [_f32c_grad(gcol[i], dev) if gcol[i] is not None else torch.zeros(3, views[i].H, views[i].W, dtype=torch.float32, device=dev)
                      for i in active]
        for a, g in enumerate(plan.keep):
            sub[a].dL_dpix = _n.ptr(g)
        cam_out = plan.attach_camera(cam_need) if want_cam else {}
        fout = plan.attach_features(ctx, gfeat, galpha, layout.saved_features(saved), need) if want_feat else None
        if want_feat or want_cam or want_depth:
            plan.attach_depth_scratch(views, gdep, _n.lib.csplat_backward_feature_scratch_bytes if want_feat else
                                      _n.lib.csplat_backward_camera_scratch_bytes if want_cam else _n.lib.csplat_backward_depth_scratch_bytes)
        if _K8_DEFER is not None:
            # K7 now, K8 in slices later (DeferredK8.launch): the plan -- the view array and every buffer it points into -- stays alive
            with _n.on_device(dev):
                rc = _n.lib.csplat_backward_views_parts(len(active), C.cast(sub, C.c_void_p), main.cuda_stream, 1, 0, 1)
            _n.check(rc, "csplat_backward_views_parts")
            # (kept alive: the MEMORY the K8 slices write -- never the gradient tensor objects themselves: AccumulateGrad adopts a
            #  gradient only when nobody else holds it, and would otherwise snapshot the still unwritten buffer into a copy)
            outs, plan.out = plan.out, None
            _K8_DEFER.entries.append((sub, len(active), dev, views[active[0]].P, (plan.big, plan.acc, plan.keep, saved, ctx.aa_opacities)))
            return layout.grads(outs)
        with _n.on_device(dev):
            rc = _n.lib.csplat_backward_views(len(active), C.cast(sub, C.c_void_p), main.cuda_stream)
        _n.check(rc, "csplat_backward_views")
        cam = [_cam_returns(cam_out[i], _cam_tensors(views[i].rs)) if i in cam_out else None for i in range(V)]
        return layout.grads(plan.out, cam, fout)


def rasterize_views(settings, inputs, stacked=False):
    """Batched entry (no counterpart upstream, where cameras are rendered one by one in a Python loop --
    scene_reconstruction/train_utils.py:204-260): `settings` a list of GaussianRasterizationSettings, `inputs` a list of
    dicts with the keyword names of GaussianRasterizer.forward.  Returns a list of (color, radii, depth); with
    stacked=True (equal image sizes) returns (colors [V,3,H,W], [(colors[i], radii, depth), ...]) where `colors` is the
    differentiable output -- the batch the reference assembles with torch.cat before its losses -- and colors[i] are
    plain slices of it.  A dict may also carry `features` ([P, F], the same F in every view) and `return_alpha`: that view's tuple
    then grows by feat [F,H,W] and / or alpha [1,H,W] (GaussianRasterizer.forward).  `antialiasing` (GaussianRasterizer.forward) must be
    the same in every dict of a call (ValueError otherwise).  `return_visibility=True` in a dict appends that view's Visibility (last, a
    NamedTuple; GaussianRasterizer.forward); the views of a call may differ in it.  Every output and gradient -- features, alpha,
    visibility, the depth, camera and background gradients, antialiasing -- is taken for up to 64 views per call; the library runs a
    call of more than 8 views in groups of at most 8 (include/csplat.h, "More than 8 views"), adding every group into the same gradients."""
    groups, fspec, feats = [], [], []
    vis = [_check_visibility_flag(kw.get("return_visibility", False)) for kw in inputs]
    aa = [bool(kw.get("antialiasing", False)) for kw in inputs]
    if len(set(aa)) > 1:
        raise ValueError(f"rasterize_views: antialiasing must be the same in every view of a call, got {aa}")
    for kw in inputs:
        f, want_alpha = kw.get("features"), bool(kw.get("return_alpha", False))
        fspec.append((_check_features(f, kw["means3D"]) if f is not None else 0, want_alpha))
        feats.append(f)
        shs, cp, sc, ro, cov = (kw.get(k) for k in ("shs", "colors_precomp", "scales", "rotations", "cov3D_precomp"))
        _check_one_of_each(shs, cp, sc, ro, cov)
        groups.append((kw["means3D"], kw["means2D"], shs, cp, kw["opacities"], sc, ro, cov))
    layout = _call_layout(settings, stacked, True in aa, fspec, vis)
    return layout.split(_RasterizeGaussiansBatch.apply(layout, *layout.pack(groups, feats)))


class GaussianRasterizer(nn.Module):
    def __init__(self, raster_settings):
        super().__init__()
        self.raster_settings = raster_settings

    def markVisible(self, positions):
        """Frustum test of the upstream extension: visible iff view-space z > 0.2."""
        with torch.no_grad():
            V = self.raster_settings.viewmatrix.to(positions.device, torch.float32)
            z = positions @ V[:3, 2] + V[3, 2]
            return z > 0.2

    def forward(self, means3D, means2D, opacities, shs=None, colors_precomp=None, scales=None, rotations=None,
                cov3D_precomp=None, features=None, return_alpha=False, antialiasing=False, return_visibility=False):
        """-> (color [3,H,W], radii [P], depth [1,H,W]), then feat [F,H,W] when `features` ([P, F] float32, 1 <= F <= 6, on the device of
        means3D) is given -- feat[c] = sum_i T_i alpha_i features[i, c] over exactly the Gaussians the colour blends, no background term --
        then alpha [1,H,W] = 1 - T_final when `return_alpha` (color = sum T alpha c + (1 - alpha) bg).  Both are differentiable; neither
        is rendered by a forward launched on faith or a captured step (RuntimeError), nor differentiated inside deferred_k8().
        antialiasing=True: every opacity o becomes o' = o h, h = sqrt(max(2.5e-5, det0 / det1)) with det0 / det1 the determinants of
        the 2-D covariance before / after its 0.3 px^2 dilation -- a footprint below pixel size keeps the coverage of its true size.
        Images and gradients (opacities.grad = h dL/do', the covariance and camera terms through h) all use o'; it works eagerly, on
        faith, in captured / replayed steps and under deferred_k8().
        return_visibility=True: one more element at the very end, a Visibility(weight_max, weight_sum, pixel_count, top_id) of this view
        (non-differentiable, bit-reproducible; not for a forward launched on faith or a captured step: RuntimeError).  It composes with
        everything above."""
        _check_one_of_each(shs, colors_precomp, scales, rotations, cov3D_precomp)
        return rasterize_gaussians(means3D, means2D, shs, colors_precomp, opacities, scales, rotations, cov3D_precomp,
                                   self.raster_settings, features, bool(return_alpha), bool(antialiasing),
                                   _check_visibility_flag(return_visibility))
