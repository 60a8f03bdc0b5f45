#!/usr/bin/env python3
"""tools/backward_dispatch_trace.py -- every way into the rasterizer backward once, for a kernel trace.

  rocprofv3 --kernel-trace --output-format csv -d DIR -o t -- python3 tools/backward_dispatch_trace.py      (on the GPU)
  python3 tools/backward_dispatch_trace.py --list DIR/.../t_kernel_trace.csv                                  (anywhere)

The run: P = 70 Gaussians, a 33 x 17 image, SH degree 3; with csplat_debug_flags 0 and then 256 (the bit-reproducible backward), in this order
  colour1   one view, colour loss, the single-view Function (PER_CALL_SPECULATION off)
  colour3   three views sharing every parameter, one rasterize_views call
  depth     one view, colour + depth loss, the single-view Function
  camera    one view, colour loss, gradients of viewmatrix / projmatrix / campos / bg, the single-view Function
  feature   one view with two feature channels and the alpha image (the batched Function)
  parts     three views: the backward launches K7 only (deferred_k8), then K8 in two slices
A flip kernel (nothing else here launches one) separates the cases.  --list prints the kernel names in dispatch order, parameter
lists cut off, the flip as a `----` line: two commits whose host side issues the same launches print the same text
(profiles/backward_dispatch_before_after.txt)."""
import csv
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "cloth-splatting_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

P, W, H = 70, 33, 17
CASES = ("colour1", "colour3", "depth", "camera", "feature", "parts")


def listing(path):
    rows = list(csv.DictReader(open(path)))
    key = "Dispatch_Id" if "Dispatch_Id" in rows[0] else "Start_Timestamp"
    rows.sort(key=lambda r: int(r[key]))
    for r in rows:
        if "arange" not in r["Kernel_Name"]:      # (the separator's operand)
            print(short(r["Kernel_Name"]))


def short(name):
    """the kernel's name with its template arguments (they select the variant), without the parameter list; torch's kernels by name only"""
    name = re.sub(r"^void ", "", name).replace("(anonymous namespace)::", "")
    if "flip_kernel" in name:
        return "----"
    if name.startswith("at::"):
        return name.split("<", 1)[0]
    depth = 0
    for i, c in enumerate(name):
        depth += (c == "<") - (c == ">")
        if c == "(" and depth == 0:
            return name[:i]
    return name


def run():
    import numpy as np
    import torch
    import diff_gaussian_rasterization as dgr
    from csplat import native, synthetic as syn

    dev = torch.device("cuda")
    sc = syn.scene_1(P=P, W=W, H=H, n_cams=1, grid=6, seed=7)
    g = syn.gaussians_at(sc)
    g["scales"] = (g["scales"] * 4.0).astype(np.float32)
    T = lambda a, rg=False: torch.tensor(np.asarray(a, np.float32), device=dev, requires_grad=rg)  # noqa: E731
    rng = np.random.default_rng(11)
    dpix, ddepth = T(rng.normal(size=(3, H, W))), T(rng.normal(size=(1, H, W)))

    def settings(theta, leaves=False):
        cam = syn.make_camera(theta, W, H, radius=1.5)
        return dgr.GaussianRasterizationSettings(
            image_height=H, image_width=W, tanfovx=cam["tanfovx"], tanfovy=cam["tanfovy"], bg=T(sc["bg"], leaves), scale_modifier=1.0,
            viewmatrix=T(cam["world_view_transform"], leaves), projmatrix=T(cam["full_proj_transform"], leaves), sh_degree=3,
            campos=T(cam["camera_center"], leaves), prefiltered=False, debug=False)

    def inputs(V=1):
        shared = {k: T(g[k], True) for k in ("means3D", "opacities", "shs", "scales", "rotations")}
        return [dict(shared, means2D=torch.zeros(P, 3, device=dev, requires_grad=True)) for _ in range(V)]

    def case(name):
        if name in ("colour1", "depth", "camera"):
            color, _radii, depth = dgr.GaussianRasterizer(settings(0.0, name == "camera"))(**inputs()[0])
            loss = (color * dpix).sum() + ((depth * ddepth).sum() if name == "depth" else 0.0)
            loss.backward()
        elif name == "feature":
            kw = inputs()[0]
            color, _radii, _depth, feat, alpha = dgr.rasterize_gaussians(
                kw["means3D"], kw["means2D"], kw["shs"], None, kw["opacities"], kw["scales"], kw["rotations"], None, settings(0.0),
                features=T(rng.normal(size=(P, 2)), True), return_alpha=True)
            ((color * dpix).sum() + (feat * dpix[:2]).sum() + (alpha * ddepth).sum()).backward()
        else:
            outs = dgr.rasterize_views([settings(-30.0 + 30.0 * i) for i in range(3)], inputs(3))
            loss = sum((o[0] * dpix).sum() for o in outs)
            if name == "colour3":
                loss.backward()
            else:
                with dgr.deferred_k8() as h:
                    loss.backward()
                for s in range(2):
                    h.launch(s, 2)
        torch.cuda.synchronize()
        torch.arange(8, device=dev).flip(0)
        torch.cuda.synchronize()

    old = dgr.PER_CALL_SPECULATION
    dgr.PER_CALL_SPECULATION = False
    try:
        for flags in (0, 256):
            native.lib.csplat_debug_flags(flags)
            for name in CASES:
                case(name)
    finally:
        native.lib.csplat_debug_flags(0)
        dgr.PER_CALL_SPECULATION = old
    print("ran", CASES, "with flags 0 and 256")


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--list":
        listing(sys.argv[2])
    elif len(sys.argv) == 1:
        run()
    else:
        sys.exit(__doc__)
