"""Cost of feature channels and the alpha image on the flagship shape (P = 100 000, 4 views at 800 x 800, synthetic scene_1), eager
steps (rasterize_views, stacked), timed with the library's event brackets per kernel class, three ways:
  default     colour loss only (today's step)
  one_pass    features = F channels (default 2) + return_alpha, colour + feature + alpha loss in one rasterization
  workaround  the same loss through two extra rasterizations: colors_precomp = the features (zero-padded to 3 channels) with bg = 0,
              and all-ones colours with bg = 0 for alpha -- each repeats K1..K8 and its backward
Prints the step time of each and the extra us per step of the two feature forms over the default step.
Run it under `rocprofv3 --kernel-trace --stats -- python tools/feature_render_cost.py` (a separate run) for the per-kernel table."""
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

CLASSES = ["K6_render_fwd", "K7_render_bwd", "K8_preprocess_bwd", "K7_depth_partials", "K8_depth_bwd", "K6_features",
           "K7_feature_partials", "K7_feature_bwd", "feature_grads"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--P", type=int, default=100_000)
    ap.add_argument("--views", type=int, default=4)
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--features", type=int, default=2)
    ap.add_argument("--steps", type=int, default=20)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    sc = syn.scene_1(P=a.P, W=a.size, H=a.size, n_cams=a.views, seed=0)
    g = syn.gaussians_at(sc)
    T = lambda x, rg=False: torch.tensor(np.asarray(x, np.float32), device=dev, requires_grad=rg)  # noqa: E731
    inp = {k: T(g[k], True) for k in ("means3D", "opacities", "shs", "scales", "rotations")}
    gen = torch.Generator(device=dev).manual_seed(0)
    feats = torch.randn(a.P, a.features, device=dev, generator=gen).requires_grad_(True)
    target = torch.rand(a.views, 3, a.size, a.size, device=dev, generator=gen)
    ftarget = torch.randn(a.views, a.features, a.size, a.size, device=dev, generator=gen)
    atarget = torch.rand(a.views, 1, a.size, a.size, device=dev, generator=gen)
    zeros_bg = torch.zeros(3, device=dev)
    ones = torch.ones(a.P, 3, device=dev)

    def settings(bg):
        return [dgr.GaussianRasterizationSettings(
            image_height=a.size, image_width=a.size, tanfovx=cam["tanfovx"], tanfovy=cam["tanfovy"], bg=bg, scale_modifier=1.0,
            viewmatrix=T(cam["world_view_transform"]), projmatrix=T(cam["full_proj_transform"]), sh_degree=3,
            campos=T(cam["camera_center"]), prefiltered=False, debug=False) for cam in sc["cameras"][:a.views]]
    st, st0 = settings(T(sc["bg"])), settings(zeros_bg)

    def kws(**extra):
        return [dict(means3D=inp["means3D"], means2D=torch.zeros(a.P, 3, device=dev, requires_grad=True), opacities=inp["opacities"],
                     scales=inp["scales"], rotations=inp["rotations"], **extra) for _ in range(a.views)]

    def step(form):
        sh = dict(shs=inp["shs"])
        if form == "one_pass":
            colors, outs = dgr.rasterize_views(st, kws(**sh, features=feats, return_alpha=True), stacked=True)
            feat, alpha = torch.stack([o[3] for o in outs]), torch.stack([o[4] for o in outs])
        else:
            colors, _outs = dgr.rasterize_views(st, kws(**sh), stacked=True)
        loss = (colors - target).abs().mean()
        if form == "workaround":
            f3 = torch.cat([feats, torch.zeros(a.P, 3 - a.features, device=dev)], 1) if a.features < 3 else feats[:, :3]
            fimg, _o = dgr.rasterize_views(st0, kws(colors_precomp=f3), stacked=True)
            alpha, _o = dgr.rasterize_views(st0, kws(colors_precomp=ones), stacked=True)
            feat, alpha = fimg[:, :a.features], alpha[:, :1]
        if form != "default":
            loss = loss + (feat - ftarget).abs().mean() + (alpha - atarget).abs().mean()
        loss.backward()
        for t in list(inp.values()) + [feats]:
            t.grad = None

    res = {}
    forms = ("default", "one_pass", "workaround")
    for form in forms + forms:
        for _ in range(3):
            step(form)
        torch.cuda.synchronize()
        native.prof_enable(CLASSES)
        for c in CLASSES:
            native.prof_read(c)
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record()
        for _ in range(a.steps):
            step(form)
        ev1.record()
        torch.cuda.synchronize()
        per = {c: native.prof_read(c)[0] / a.steps for c in CLASSES}
        native.prof_enable([])
        res.setdefault(form, []).append(dict(step_ms=ev0.elapsed_time(ev1) / a.steps, **{k: round(v, 4) for k, v in per.items() if v}))
    for k, v in res.items():
        for r in v:
            print(k, {kk: round(vv, 4) for kk, vv in r.items()})
    best = {k: min(r["step_ms"] for r in v) for k, v in res.items()}
    print("step_ms", {k: round(v, 4) for k, v in best.items()})
    print("extra_us_per_step", {k: round(1000.0 * (best[k] - best["default"]), 1) for k in ("one_pass", "workaround")})


if __name__ == "__main__":
    main()
