"""Extra backward cost of a depth loss on the flagship shape (P = 100 000, 4 views at 800 x 800, synthetic scene_1): the same batched step
(rasterize_views, stacked) with a colour loss only and with colour + depth loss, timed with the library's event brackets per kernel class.
Run it under `rocprofv3 --kernel-trace --stats -- python tools/depth_bwd_cost.py` for the per-kernel table."""
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

CLASSES = ["K7_render_bwd", "K8_preprocess_bwd", "K7_depth_partials", "K7_depth_bwd", "K8_depth_bwd"]


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
    settings = []
    for cam in sc["cameras"][:a.views]:
        settings.append(dgr.GaussianRasterizationSettings(
            image_height=a.size, image_width=a.size, tanfovx=cam["tanfovx"], tanfovy=cam["tanfovy"], bg=T(sc["bg"]), scale_modifier=1.0,
            viewmatrix=T(cam["world_view_transform"]), projmatrix=T(cam["full_proj_transform"]), sh_degree=3,
            campos=T(cam["camera_center"]), prefiltered=False, debug=False))
    gen = torch.Generator(device=dev).manual_seed(0)
    target = torch.rand(a.views, 3, a.size, a.size, device=dev, generator=gen)
    dtarget = torch.rand(a.views, 1, a.size, a.size, device=dev, generator=gen) * 4.0

    def step(depth):
        m2d = [torch.zeros(a.P, 3, device=dev, requires_grad=True) for _ in range(a.views)]
        kws = [dict(means3D=inp["means3D"], means2D=m2d[i], **{k: inp[k] for k in ("opacities", "shs", "scales", "rotations")})
               for i in range(a.views)]
        colors, outs = dgr.rasterize_views(settings, kws, stacked=True)
        loss = (colors - target).abs().mean()
        if depth:
            loss = loss + (torch.stack([o[2] for o in outs]) - dtarget).abs().mean()
        loss.backward()
        for t in inp.values():
            t.grad = None

    res = {}
    for depth in (False, True, False, True):
        for _ in range(3):
            step(depth)
        torch.cuda.synchronize()
        native.prof_enable(CLASSES)
        for c in CLASSES:
            native.prof_read(c)
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record()
        for _ in range(a.steps):
            step(depth)
        ev1.record()
        torch.cuda.synchronize()
        per = {c: native.prof_read(c)[0] / a.steps for c in CLASSES}
        native.prof_enable([])
        key = "colour+depth" if depth else "colour"
        res.setdefault(key, []).append(dict(step_ms=ev0.elapsed_time(ev1) / a.steps, **{k: round(v, 4) for k, v in per.items()}))
    for k, v in res.items():
        for r in v:
            print(k, {kk: round(vv, 4) for kk, vv in r.items()})


if __name__ == "__main__":
    main()
