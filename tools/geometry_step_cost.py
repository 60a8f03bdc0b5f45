"""Cost of the depth and silhouette terms of csplat.train.train_step on the config-3 shape (3 cameras 800 x 800, P = 100 000, synthetic
scene_1), eager steps, four forms:
  plain        today's step (no weight set)
  depth        opt.lambda_depth > 0
  silhouette   opt.lambda_silhouette > 0
  both         both weights > 0
Each form runs twice, alternating with the others, after its warm-up; a run is timed with device events over `--steps` steps.  Prints the
ms per step of every run, the best of each form, the extra ms against the plain step of the same run, and the geometry kernels' own us
per step from the library's event brackets (classes geometry_loss_fwd: both forward launches, geometry_loss_bwd).
Targets come from the model itself: Z = D / A where A > 0.5 (else 0, a hole), S = (A > 0.5); the opacity logits are then lowered so that
the residuals are not all ties."""
import argparse
import os
import sys
from types import SimpleNamespace

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "cloth-splatting_amd"), ROOT):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import bench_train as bt  # noqa: E402
from csplat import native, train as tr  # noqa: E402
from csplat.optim import GroupedAdam  # noqa: E402
from gaussian_renderer import render_views  # noqa: E402

CLASSES = ["geometry_loss_fwd", "geometry_loss_bwd"]
FORMS = {"plain": {}, "depth": dict(lambda_depth=0.2), "silhouette": dict(lambda_silhouette=0.5),
         "both": dict(lambda_depth=0.2, lambda_silhouette=0.5)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--P", type=int, default=100_000)
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--grid", type=int, default=100)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    n_times = 30          # (bench_train.py's scene: three consecutive timesteps of one view)
    times = [k / (n_times - 1) for k in (9, 10, 11)]
    sc, pc, sim = bt.build(P=a.P, W=a.size, H=a.size, grid=a.grid, n_times=n_times, dev=dev)
    bg = torch.ones(3, device=dev)
    with torch.no_grad():
        res, alphas = render_views(bt.cameras(sc, times, dev), pc, sim, tr.DEFAULT_PIPE, bg, return_alpha=True)
        cams = bt.cameras(sc, times, dev, [r.render.clamp(0, 1).clone() for r in res])
        for cam, r, al in zip(cams, res, alphas):
            cam.depth = torch.where(al > 0.5, r.depth / al.clamp_min(1e-6), torch.zeros_like(al))
            cam.silhouette = (al > 0.5).float()
        pc._opacity.sub_(1.0)
    pc.training_setup(feature_lr=tr.DEFAULT_OPT.feature_lr)
    mopt = GroupedAdam(sim.parameters(), lr=tr.DEFAULT_OPT.meshnet_lr)
    opts = {k: SimpleNamespace(**vars(tr.DEFAULT_OPT), **kw) for k, kw in FORMS.items()}
    it = [0]

    def step(form):
        it[0] += 1
        return tr.train_step(it[0] % 999 + 1, cams, pc, sim, mopt, opt=opts[form], background=bg)

    res = {}
    for form in list(FORMS) + list(FORMS):
        for _ in range(a.warmup):
            step(form)
        torch.cuda.synchronize()
        native.prof_enable(CLASSES)
        for c in CLASSES:
            native.prof_read(c)
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record()
        for _ in range(a.steps):
            _ps, _loss, stats = step(form)
        ev1.record()
        torch.cuda.synchronize()
        per = {c: native.prof_read(c)[0] / a.steps for c in CLASSES}
        native.prof_enable([])
        row = dict(step_ms=round(ev0.elapsed_time(ev1) / a.steps, 4), **{c + "_us": round(1000.0 * v, 2) for c, v in per.items()})
        row.update({k: round(float(stats[k]), 6) for k in ("depth_loss", "silhouette_loss") if k in stats})
        res.setdefault(form, []).append(row)
        print(form, row, flush=True)
    best = {k: min(r["step_ms"] for r in v) for k, v in res.items()}
    print("shape", dict(P=a.P, cameras=len(cams), size=a.size, steps=a.steps))
    print("step_ms", {k: round(v, 4) for k, v in best.items()})
    print("extra_ms_against_plain", {k: round(v - best["plain"], 4) for k, v in best.items() if k != "plain"})
    print("geometry_kernels_us_per_step", {k: {c: min(r[c + "_us"] for r in v) for c in CLASSES} for k, v in res.items() if k != "plain"})


if __name__ == "__main__":
    main()
