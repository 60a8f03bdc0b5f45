"""Cost of the visibility pass (csplat_visibility_views) on the flagship shape (P = 100 000, 4 views at 800 x 800, synthetic scene_1),
eager forward calls (rasterize_views, stacked, no_grad), timed with the library's event brackets per kernel class, two ways:
  default      the forward of today's step
  visibility   the same call with return_visibility=True in every view (the walk and the per-Gaussian reduce behind K6)
Prints the call time of each, the "visibility" class's time per call and the extra us per call.
Run it under `rocprofv3 --kernel-trace --stats -- python tools/visibility_cost.py` (a separate run) for the per-kernel table."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "cloth-splatting_amd"), ROOT):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from csplat import native, synthetic as syn  # noqa: E402
import diff_gaussian_rasterization as dgr  # noqa: E402

CLASSES = ["K6_render_fwd", "visibility"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--P", type=int, default=100_000)
    ap.add_argument("--views", type=int, default=4)
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--steps", type=int, default=20)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    sc = syn.scene_1(P=a.P, W=a.size, H=a.size, n_cams=a.views, seed=0)
    g = syn.gaussians_at(sc)
    T = lambda x: torch.tensor(np.asarray(x, np.float32), device=dev)  # noqa: E731
    inp = {k: T(g[k]) for k in ("means3D", "opacities", "shs", "scales", "rotations")}
    st = [dgr.GaussianRasterizationSettings(
        image_height=a.size, image_width=a.size, tanfovx=cam["tanfovx"], tanfovy=cam["tanfovy"], bg=T(sc["bg"]), scale_modifier=1.0,
        viewmatrix=T(cam["world_view_transform"]), projmatrix=T(cam["full_proj_transform"]), sh_degree=3,
        campos=T(cam["camera_center"]), prefiltered=False, debug=False) for cam in sc["cameras"][:a.views]]
    m2d = torch.zeros(a.P, 3, device=dev)

    def call(form):
        kws = [dict(means3D=inp["means3D"], means2D=m2d, opacities=inp["opacities"], shs=inp["shs"], scales=inp["scales"],
                    rotations=inp["rotations"], **(dict(return_visibility=True) if form == "visibility" else {})) for _ in range(a.views)]
        with torch.no_grad():
            dgr.rasterize_views(st, kws, stacked=True)

    res = {}
    forms = ("default", "visibility")
    for form in forms + forms:
        for _ in range(3):
            call(form)
        torch.cuda.synchronize()
        native.prof_enable(CLASSES)
        for c in CLASSES:
            native.prof_read(c)
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record()
        for _ in range(a.steps):
            call(form)
        ev1.record()
        torch.cuda.synchronize()
        per = {c: native.prof_read(c)[0] / a.steps for c in CLASSES}
        native.prof_enable([])
        res.setdefault(form, []).append(dict(call_ms=ev0.elapsed_time(ev1) / a.steps, **{k: round(v, 4) for k, v in per.items() if v}))
    for k, v in res.items():
        for r in v:
            print(k, {kk: round(vv, 4) for kk, vv in r.items()})
    best = {k: min(r["call_ms"] for r in v) for k, v in res.items()}
    vis_ms = min(r.get("visibility", 0.0) for r in res["visibility"])
    print("call_ms", {k: round(v, 4) for k, v in best.items()})
    print("visibility_kernels_us_per_call", round(1000.0 * vis_ms, 1))
    print("extra_us_per_call", round(1000.0 * (best["visibility"] - best["default"]), 1))


if __name__ == "__main__":
    main()
