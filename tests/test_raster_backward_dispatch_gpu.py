"""One way into the rasterizer backward (csplat_raster.hip: backward_views_impl): whichever door a single view comes through, the same
launches run, so in the bit-reproducible mode (csplat_debug_flags bit 8: ordered sums instead of float atomics) the gradients are equal
BIT FOR BIT.  Doors: the single-view Function (_RasterizeGaussians, PER_CALL_SPECULATION off), the batched Function with one view, and the
flat C entries csplat_backward / csplat_backward_depth, which nothing else in the tree calls.
Shape: P = 70 (no multiple of 32 or 128: more than one K8 workgroup in the single-view and the batched kernels, each with a ragged tail),
a 33 x 17 image (partial tiles on both edges), SH degree 3; and P = 0, a view without Gaussians."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

import util
from util import make_case

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

BIT_REPRODUCIBLE = 256
W, H = 33, 17
NAMES = ("means3D", "means2D", "opacities", "shs", "scales", "rotations")
CAM_NAMES = ("view_t", "proj", "campos", "bg")


def _case(P):
    case = make_case(P=70, W=W, H=H, seed=7, grid=6, scale_mul=4.0, radius=1.5)
    return dict(case, P=P, g={k: v[:P] for k, v in case["g"].items()})


def _images():
    rng = np.random.default_rng(11)
    return (torch.tensor(rng.normal(size=(3, H, W)).astype(np.float32), device="cuda"),
            torch.tensor(rng.normal(size=(1, H, W)).astype(np.float32), device="cuda"))


def _cam_leaves(case):
    cam = case["cam"]
    t = lambda a: torch.tensor(np.asarray(a, np.float32), device="cuda", requires_grad=True)  # noqa: E731
    return dict(view_t=t(np.asarray(cam["world_view_transform"]).T), proj=t(cam["full_proj_transform"]), campos=t(cam["camera_center"]),
                bg=t(case["bg"]))


def _settings(case, leaves):
    rs = util.gpu_settings(case)
    if leaves is None:
        return rs
    return rs._replace(bg=leaves["bg"], viewmatrix=leaves["view_t"].transpose(0, 1), projmatrix=leaves["proj"], campos=leaves["campos"])


def _grads(case, kind, batched):
    """every gradient one view returns for the loss of `kind`, through the single-view Function or the batched one"""
    import diff_gaussian_rasterization as dgr
    inp = util.gpu_inputs(case)
    leaves = _cam_leaves(case) if kind == "camera" else None
    rs = _settings(case, leaves)
    kw = dict(means3D=inp["means3D"], means2D=inp["means2D"], opacities=inp["opacities"], shs=inp["shs"], scales=inp["scales"],
              rotations=inp["rotations"])
    if batched:
        color, _radii, depth = dgr.rasterize_views([rs], [kw])[0]
    else:
        color, _radii, depth = dgr.GaussianRasterizer(rs)(**kw)
    dpix, ddepth = _images()
    loss = (color * dpix).sum()
    if kind == "depth":
        loss = loss + (depth * ddepth).sum()
    loss.backward()
    torch.cuda.synchronize()
    out = {k: inp[k].grad for k in NAMES}
    if leaves is not None:
        out.update({k: leaves[k].grad for k in CAM_NAMES})
    return out


@pytest.mark.parametrize("P", [70, 0])
@pytest.mark.parametrize("kind", ["colour", "depth", "camera"])
def test_single_view_function_equals_batched_function_bit_for_bit(kind, P):
    import diff_gaussian_rasterization as dgr
    from csplat import native
    case = _case(P)
    old_flags, old_spec = int(native.lib.csplat_debug_flags_query()), dgr.PER_CALL_SPECULATION
    try:
        native.lib.csplat_debug_flags(BIT_REPRODUCIBLE)
        dgr.PER_CALL_SPECULATION = False
        single = _grads(case, kind, batched=False)
        batch = _grads(case, kind, batched=True)
    finally:
        native.lib.csplat_debug_flags(old_flags)
        dgr.PER_CALL_SPECULATION = old_spec
    assert set(single) == set(batch)
    for k in single:
        assert single[k] is not None and batch[k] is not None, k
        assert single[k].shape == batch[k].shape and torch.equal(single[k], batch[k]), k
    if P:       # (the comparison is of gradients that exist)
        assert all(float(v.abs().max()) > 0 for v in single.values()), {k: float(v.abs().max()) for k, v in single.items()}


def _outputs(P, M, dev):
    """the nine gradient outputs of the C entries, in their argument order, filled with a sentinel"""
    shapes = ((P, 3), (P, 4), (P, 1), (P, 3), (P, 3), (P, 6), (P, M, 3), (P, 3), (P, 4))
    return [torch.full(s, 7.0, dtype=torch.float32, device=dev) for s in shapes]


OUT_FIELDS = ("dL_dmean2D", "dL_dconic", "dL_dopacity", "dL_dcolor", "dL_dmean3D", "dL_dcov3D", "dL_dsh", "dL_dscale", "dL_drot")


def forward_state(case, W=W, H=H):
    """ONE forward of the single-view path on `case` (a W x H image) -> what the flat C entries read: the view state with its chunks, the
    saved tensors, the settings"""
    import diff_gaussian_rasterization as dgr
    inp = util.gpu_inputs(case, requires_grad=False)
    rs = util.gpu_settings(case)

    class Ctx:
        def save_for_backward(self, *a): self.saved_tensors = a
        def mark_non_differentiable(self, *a): pass
    ctx = Ctx()
    with torch.no_grad():
        dgr._RasterizeGaussians.forward(ctx, inp["means3D"], inp["means2D"], inp["shs"], None, inp["opacities"], inp["scales"],
                                        inp["rotations"], None, rs)
    return SimpleNamespace(vs=ctx.view_state, saved=ctx.saved_tensors, rs=rs, P=case["P"], W=W, H=H)


def flat_call(st, entry, dpix, depth_arg, scratch_ptr, out_ptrs):
    """csplat_backward (depth_arg = []) or csplat_backward_depth (depth_arg = [pointer or None]) on the chunks of forward_state(), with
    the caller's scratch and the addresses of its nine outputs (the order of OUT_FIELDS); synchronised on return"""
    from csplat import native as n
    vs, rs = st.vs, st.rs
    means3D, sh, colors_precomp, scales, rotations, cov3Ds_precomp, radii, color = st.saved
    dev = means3D.device
    head = [n.stream_handle(dev), st.P, int(rs.sh_degree), vs.M, vs.num_rendered, n.ptr(vs.bg), st.W, st.H, n.ptr(means3D), n.ptr(sh),
            n.ptr(colors_precomp), n.ptr(scales), float(rs.scale_modifier), n.ptr(rotations), n.ptr(cov3Ds_precomp), n.ptr(vs.view),
            n.ptr(vs.proj), n.ptr(vs.campos), float(rs.tanfovx), float(rs.tanfovy), n.ptr(radii), *(n.ptr(c) for c in vs.chunks),
            n.ptr(color), n.ptr(dpix)]
    with n.on_device(dev):
        rc = getattr(n.lib, entry)(*head, *depth_arg, scratch_ptr, *out_ptrs)
    n.check(rc, entry)
    torch.cuda.synchronize()


@pytest.mark.parametrize("P", [70, 0])
@pytest.mark.parametrize("with_depth", [False, True])
def test_flat_entries_equal_the_views_entry_bit_for_bit(with_depth, P):
    """csplat_backward and csplat_backward_depth (with and without a depth gradient) against csplat_backward_views(1, ...), all on the
    chunks of ONE forward of the single-view path"""
    from csplat import native as n
    case = _case(P)
    dev = torch.device("cuda")
    old_flags = int(n.lib.csplat_debug_flags_query())
    try:
        n.lib.csplat_debug_flags(BIT_REPRODUCIBLE)
        st = forward_state(case)
        vs = st.vs
        means3D, sh, colors_precomp, scales, rotations, cov3Ds_precomp, radii, color = st.saved
        R, M = vs.num_rendered, vs.M
        dpix, ddepth = _images()
        if not with_depth:
            ddepth = None
        size_of = n.lib.csplat_backward_depth_scratch_bytes if with_depth else n.lib.csplat_backward_scratch_bytes
        nbytes = int(size_of(P, R, W, H) if with_depth else size_of(P, R))
        scratch = lambda: torch.empty(max(nbytes, 256), dtype=torch.uint8, device=dev)  # noqa: E731
        stream = n.stream_handle(dev)

        def flat(entry, depth_arg):
            outs, buf = _outputs(P, M, dev), scratch()
            flat_call(st, entry, dpix, depth_arg, n.ptr(buf), [n.ptr(o) for o in outs])
            return outs

        def views():
            outs, buf = _outputs(P, M, dev), scratch()
            w = n.CsplatView()
            vs.fill(w, stream, (means3D, sh, colors_precomp, None, scales, rotations, cov3Ds_precomp, color, radii))
            w.dL_dpix, w.dL_ddepth, w.scratch = n.ptr(dpix), n.ptr(ddepth), n.ptr(buf)
            for f, o in zip(OUT_FIELDS, outs):
                setattr(w, f, n.ptr(o))
            with n.on_device(dev):
                rc = n.lib.csplat_backward_views(1, C.addressof(w), w.stream)
            n.check(rc, "csplat_backward_views")
            torch.cuda.synchronize()
            return outs

        want = views()
        got = [flat("csplat_backward_depth", [n.ptr(ddepth)])]
        if not with_depth:
            got.append(flat("csplat_backward", []))
    finally:
        n.lib.csplat_debug_flags(old_flags)
    for outs in got:
        for f, a, b in zip(OUT_FIELDS, outs, want):
            assert torch.equal(a, b), f
    if P:       # (every output the call owes was written: dL_dcolor and dL_dcov3D belong to the precomputed inputs, absent here)
        for f, b in zip(OUT_FIELDS, want):
            assert f in ("dL_dcolor", "dL_dcov3D") or not bool((b == 7.0).all()), f
