"""Cost of antialiased rendering (GaussianRasterizer.forward(antialiasing=True), include/csplat.h CSPLAT_ANTIALIAS) on the flagship shape
(P = 100 000, 4 views at 800 x 800, SH 3, synthetic scene_1): one training-shaped step -- rasterize_views (stacked), L1 loss, backward --
with antialiasing off and on, timed two ways:
  eager     the step as Python calls it, with the library's event brackets per kernel class
  replayed  the same step recorded by csplat.graphs.ReplayedSteps (forward launched on faith) and replayed -- what bench.py times
Also prints the list entries R per view (the forward's counts) off and on.  R is set by the tile rectangle, which comes from the dilated
covariance and is the same with antialiasing; o' = o h <= o shrinks only the culling radius 2 lambda ln(255 o'), which K5b applies per
(list entry, 4x4 pixel block) -- so R stays, and what antialiasing saves or costs shows in the step time.
Run it under `rocprofv3 --kernel-trace --stats -- python tools/antialias_cost.py` (a separate run) for the per-kernel table."""
import argparse
import faulthandler
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "cloth-splatting_amd"), ROOT):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from csplat import graphs, native, synthetic as syn  # noqa: E402
import diff_gaussian_rasterization as dgr  # noqa: E402

CLASSES = ["K1_preprocess", "K2_scan", "K6_render_fwd", "K7_render_bwd", "K8_preprocess_bwd"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--P", type=int, default=100_000)
    ap.add_argument("--views", type=int, default=4)
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--steps", type=int, default=20)
    a = ap.parse_args()
    faulthandler.enable()
    dev = torch.device("cuda:0")
    sc = syn.scene_1(P=a.P, W=a.size, H=a.size, n_cams=a.views, seed=0)
    g = syn.gaussians_at(sc)
    T = lambda x, rg=False: torch.tensor(np.asarray(x, np.float32), device=dev, requires_grad=rg)  # noqa: E731
    inp = {k: T(g[k], True) for k in ("means3D", "opacities", "shs", "scales", "rotations")}
    target = torch.rand(a.views, 3, a.size, a.size, device=dev, generator=torch.Generator(device=dev).manual_seed(0))
    zeros = torch.zeros(a.views, a.P, 3, device=dev)
    one = torch.ones((), device=dev)
    st = [dgr.GaussianRasterizationSettings(
        image_height=a.size, image_width=a.size, tanfovx=cam["tanfovx"], tanfovy=cam["tanfovy"], bg=T(sc["bg"]), scale_modifier=1.0,
        viewmatrix=T(cam["world_view_transform"]), projmatrix=T(cam["full_proj_transform"]), sh_degree=3, campos=T(cam["camera_center"]),
        prefiltered=False, debug=False) for cam in sc["cameras"][:a.views]]

    def make_step(aa):
        def step():
            for t in inp.values():
                t.grad = None
            kws = [dict(means3D=inp["means3D"], means2D=zeros[i].detach().requires_grad_(), opacities=inp["opacities"], shs=inp["shs"],
                        scales=inp["scales"], rotations=inp["rotations"], **(dict(antialiasing=True) if aa else {}))
                   for i in range(a.views)]
            colors, _outs = dgr.rasterize_views(st, kws, stacked=True)
            loss = (colors - target).abs().mean()
            loss.backward(gradient=one)
            # detached results only: an output that keeps its autograd graph alive keeps the leaves' AccumulateGrad nodes, bound to the
            # stream of the step that made them -- a later recording's backward would then synchronise with that stream inside the capture
            return loss.detach(), colors.detach(), [t.grad for t in inp.values()], [k["means2D"].grad for k in kws]
        return step

    res, R, keep = {}, {}, []
    for aa in (False, True, False, True):
        name = "on" if aa else "off"
        step = make_step(aa)
        counts = graphs.counts_of_eager(step)[1]
        R[name] = [int(c[0]) for c in counts]
        for _ in range(3):
            step()
        torch.cuda.synchronize()
        native.prof_enable(CLASSES)
        for c in CLASSES:
            native.prof_read(c)
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record()
        for _ in range(a.steps):
            step()
        ev1.record()
        torch.cuda.synchronize()
        per = {c: round(native.prof_read(c)[0] / a.steps, 4) for c in CLASSES}
        native.prof_enable([])
        eager = ev0.elapsed_time(ev1) / a.steps
        rs = graphs.ReplayedSteps(step, dev, G=2)
        rs.record()
        for _ in range(3):
            rs.step()
        torch.cuda.synchronize()
        ev0.record()
        for _ in range(a.steps):
            rs.step()
        ev1.record()
        rs.check()
        replayed = ev0.elapsed_time(ev1) / a.steps
        keep.append(rs)         # (the recordings stay alive to the end of the run, as bench.py keeps its own)
        r = dict(eager_ms=round(eager, 4), replayed_ms=round(replayed, 4), **{k: v for k, v in per.items() if v})
        print(name, r)
        res.setdefault(name, []).append(r)
    best = {k: {m: min(r[m] for r in v) for m in ("eager_ms", "replayed_ms")} for k, v in res.items()}
    print("ms_per_step", best)
    print("R_per_view", R, "reduction", [round(1.0 - on / off, 4) for on, off in zip(R["on"], R["off"])])


if __name__ == "__main__":
    main()
