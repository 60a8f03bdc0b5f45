#!/usr/bin/env python3
"""tools/forward_dispatch_trace.py -- every way into the rasterizer forward once, for a kernel trace.

  rocprofv3 --kernel-trace --output-format csv -d DIR -o t -- python3 tools/forward_dispatch_trace.py      (on the GPU)
  python3 tools/forward_dispatch_trace.py --list DIR/.../t_kernel_trace.csv                                  (anywhere)

The run: P = 70 Gaussians, a 33 x 17 image, SH degree 3, forwards only, in this order
  single    one view, the single-view Function with PER_CALL_SPECULATION off (csplat_forward_begin / _finish)
  percall   one view through the per-call path, twice: the first call waits for its counts, the second defers and settles
  shared3   three views sharing every parameter, one rasterize_views call, twice
  grown     three views after the scales grew fourfold: the counts no longer fit, settle launches the second phase again.  (At 70
            Gaussians no count can outgrow a capacity -- the longest list gets 64 entries of slack: this case alone is 300 Gaussians on
            64 x 48, as tests/test_raster_forward_dispatch_gpu.py::test_settle_that_must_relaunch)
  mixed     three views of different image sizes: every view on its own stream, first and second phase view by view
  global    three views under CSPLAT_DEBUG_GLOBAL_SORT (the global radix sort, view by view)
  nospec    three views under CSPLAT_DEBUG_NO_SPECULATION (the batched second phase behind the host read)
  faith     three views under forward_mode(faith=...): both phases on the caller's capacities, nothing read
  feature   one view with two feature channels and the alpha image
A flip kernel (nothing else here launches one) separates the cases.  --list prints the kernel names in dispatch order, parameter
lists cut off, the flip as a `----` line: two commits whose host side issues the same launches print the same text
(profiles/forward_dispatch_before_after.txt)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "cloth-splatting_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

from backward_dispatch_trace import listing  # noqa: E402  (tools/: the same listing for both traces)

CASES = ("single", "percall", "shared3", "grown", "mixed", "global", "nospec", "faith", "feature")
GLOBAL_SORT, NO_SPECULATION = 2, 1024


def run():
    import numpy as np
    import torch
    import diff_gaussian_rasterization as dgr
    from csplat import native, synthetic as syn

    dev = torch.device("cuda")
    T = lambda a: torch.tensor(np.asarray(a, np.float32), device=dev)  # noqa: E731

    class Scene:
        def __init__(self, P, W, H, grid, scale_mul, radius=1.5):
            self.P, self.W, self.H, self.radius = P, W, H, radius
            self.sc = syn.scene_1(P=P, W=W, H=H, n_cams=1, grid=grid, seed=7)
            g = syn.gaussians_at(self.sc)
            g["scales"] = (g["scales"] * scale_mul).astype(np.float32)
            self.g = {k: T(g[k]) for k in ("means3D", "opacities", "shs", "scales", "rotations")}

        def settings(self, theta=0.0, W=None, H=None):
            W, H = W or self.W, H or self.H
            cam = syn.make_camera(theta, W, H, radius=self.radius)
            return dgr.GaussianRasterizationSettings(
                image_height=H, image_width=W, tanfovx=cam["tanfovx"], tanfovy=cam["tanfovy"], bg=T(self.sc["bg"]), scale_modifier=1.0,
                viewmatrix=T(cam["world_view_transform"]), projmatrix=T(cam["full_proj_transform"]), sh_degree=3,
                campos=T(cam["camera_center"]), prefiltered=False, debug=False)

        def inputs(self, V=1):
            return [dict(self.g, means2D=torch.zeros(self.P, 3, device=dev)) for _ in range(V)]

        def three(self, sizes=None):
            sizes = sizes or [(self.W, self.H)] * 3
            return dgr.rasterize_views([self.settings(-30.0 + 30.0 * i, W, H) for i, (W, H) in enumerate(sizes)], self.inputs(3))

    tiny = Scene(70, 33, 17, grid=6, scale_mul=4.0)
    small, big = Scene(300, 64, 48, grid=20, scale_mul=2.0), Scene(300, 64, 48, grid=20, scale_mul=8.0)

    def case(name):
        if name == "single":
            dgr.PER_CALL_SPECULATION = False
            dgr.GaussianRasterizer(tiny.settings())(**tiny.inputs()[0])
            dgr.PER_CALL_SPECULATION = True
        elif name == "percall":
            for _ in range(2):
                dgr.GaussianRasterizer(tiny.settings())(**tiny.inputs()[0])
        elif name == "shared3":
            for _ in range(2):
                tiny.three()
        elif name == "grown":
            small.three()
            before = dgr.SPEC_STATS["miss"]
            big.three()
            assert dgr.SPEC_STATS["miss"] == before + 1, dgr.SPEC_STATS
        elif name == "mixed":
            tiny.three([(33, 17), (40, 24), (17, 33)])
        elif name in ("global", "nospec"):
            native.lib.csplat_debug_flags(GLOBAL_SORT if name == "global" else NO_SPECULATION)
            tiny.three()
            native.lib.csplat_debug_flags(0)
        elif name == "faith":
            faith = dict(caps=(4096, 128, 6), valid=torch.zeros(1, dtype=torch.int32, device=dev))
            with dgr.forward_mode(faith=faith):
                tiny.three()
            torch.cuda.synchronize()
            assert int(faith["valid"].cpu()[0]) == 1
        else:
            kw = tiny.inputs()[0]
            dgr.rasterize_gaussians(kw["means3D"], kw["means2D"], kw["shs"], None, kw["opacities"], kw["scales"], kw["rotations"], None,
                                    tiny.settings(), features=T(np.random.default_rng(11).normal(size=(tiny.P, 2))), return_alpha=True)
        torch.cuda.synchronize()
        torch.arange(8, device=dev).flip(0)
        torch.cuda.synchronize()

    old = dgr.PER_CALL_SPECULATION
    try:
        for name in CASES:
            case(name)
    finally:
        native.lib.csplat_debug_flags(0)
        dgr.PER_CALL_SPECULATION = old
    print("ran", CASES)


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--list":
        listing(sys.argv[2])
    elif len(sys.argv) == 1:
        run()
    else:
        sys.exit(__doc__)
