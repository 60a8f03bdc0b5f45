"""Extra backward cost of camera and background gradients on the flagship shape (P = 100 000, 4 views at 800 x 800, synthetic scene_1):
the same batched step (rasterize_views, stacked, colour loss) with constant settings and with viewmatrix / projmatrix / campos / bg
requiring grad, timed with the library's event brackets per kernel class.  Prints the extra us per step.
Run it under `rocprofv3 --kernel-trace --stats -- python tools/camera_bwd_cost.py` (a separate run) for the per-kernel table."""
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

CLASSES = ["K7_render_bwd", "K8_preprocess_bwd", "K8_camera_bwd", "camera_sums"]


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
    T = lambda x, rg=False: torch.tensor(np.asarray(x, np.float32), device=dev, requires_grad=rg)  # noqa: E731
    inp = {k: T(g[k], True) for k in ("means3D", "opacities", "shs", "scales", "rotations")}
    settings = {}
    for grad in (False, True):
        settings[grad] = [dgr.GaussianRasterizationSettings(
            image_height=a.size, image_width=a.size, tanfovx=cam["tanfovx"], tanfovy=cam["tanfovy"], bg=T(sc["bg"], grad), scale_modifier=1.0,
            viewmatrix=T(cam["world_view_transform"], grad), projmatrix=T(cam["full_proj_transform"], grad), sh_degree=3,
            campos=T(cam["camera_center"], grad), prefiltered=False, debug=False) for cam in sc["cameras"][:a.views]]
    gen = torch.Generator(device=dev).manual_seed(0)
    target = torch.rand(a.views, 3, a.size, a.size, device=dev, generator=gen)

    def step(camera):
        m2d = [torch.zeros(a.P, 3, device=dev, requires_grad=True) for _ in range(a.views)]
        kws = [dict(means3D=inp["means3D"], means2D=m2d[i], **{k: inp[k] for k in ("opacities", "shs", "scales", "rotations")})
               for i in range(a.views)]
        colors, _outs = dgr.rasterize_views(settings[camera], kws, stacked=True)
        loss = (colors - target).abs().mean()
        loss.backward()
        for t in inp.values():
            t.grad = None
        for rs in settings[camera]:
            for t in (rs.viewmatrix, rs.projmatrix, rs.campos, rs.bg):
                t.grad = None

    res = {}
    for camera in (False, True, False, True):
        for _ in range(3):
            step(camera)
        torch.cuda.synchronize()
        native.prof_enable(CLASSES)
        for c in CLASSES:
            native.prof_read(c)
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record()
        for _ in range(a.steps):
            step(camera)
        ev1.record()
        torch.cuda.synchronize()
        per = {c: native.prof_read(c)[0] / a.steps for c in CLASSES}
        native.prof_enable([])
        key = "camera" if camera else "constant"
        res.setdefault(key, []).append(dict(step_ms=ev0.elapsed_time(ev1) / a.steps, **{k: round(v, 4) for k, v in per.items()}))
    for k, v in res.items():
        for r in v:
            print(k, {kk: round(vv, 4) for kk, vv in r.items()})
    best = {k: min(r["step_ms"] for r in v) for k, v in res.items()}
    print("extra_us_per_step", round(1000.0 * (best["camera"] - best["constant"]), 1))


if __name__ == "__main__":
    main()
