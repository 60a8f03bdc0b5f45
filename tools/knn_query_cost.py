"""Cost of the exact two-cloud k-NN (simple_knn.knn_query: csplat_knn_query brute force / csplat_knn_query_ws Morton order + boxes), of
the Chamfer loss on top of it (csplat.pointcloud.chamfer_distance) and of the train step's Chamfer term, next to what they replace,
all from one run on one box.  Device events after warm-up, median / min of --reps, one process.
  table   brute against pruned, uniform-cube clouds, N in {1k, 4k, 16k, 100k} x Q in {1k, 16k, 100k} x K in {1, 8}: the table
          simple_knn.QUERY_BOXED_FROM is read from (the smallest N from which the pruned form wins at every Q)
  closest find_closest_gauss at 2 000 gt x 100 000 Gaussians: both forms; the reference's formulation (render.py:123-134: both clouds
          repeated to [M,N,3], norm, argmin over M) restated in torch on the same GPU, in chunks of gt points when [M,N,3] does not fit;
          host cKDTree.query with 16 workers (tree build included)
  loss    chamfer_distance forward + backward, 50 000 -> 100 000 one-sided, against the same loss composed from torch.cdist(...).min in
          chunks of queries
  step    a train step (eager) on bench_train's scene (P = 100k, 3 cameras 800 x 800) without the term and with it, 20 000 observed
          points per camera; wall clock per step after a synchronise, median
Write the output to profiles/knn_query_cost.txt."""
import argparse
import faulthandler
import os
import sys
import time
from types import SimpleNamespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "cloth-splatting_amd"), ROOT):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import simple_knn  # noqa: E402


def device_ms(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return float(np.median(ts)), float(np.min(ts))


def cube(n, seed, dev):
    return torch.tensor(np.random.default_rng(seed).uniform(-1, 1, (n, 3)).astype(np.float32), device=dev)


def reference_closest(gt, gauss, chunk):
    """the reference's find_closest_gauss on GPU tensors: [M,N,3] repeats, norm, argmin over the Gaussians -- `chunk` gt points a time"""
    out = []
    M = gauss.shape[0]
    for s in range(0, gt.shape[0], chunk):
        g = gt[s:s + chunk]
        a = g.unsqueeze(0).repeat(M, 1, 1)
        b = gauss.unsqueeze(1).repeat(1, g.shape[0], 1)
        out.append(torch.norm(a - b, dim=-1).argmin(dim=0))
    return torch.cat(out)


def composed_chamfer(a, b, chunk):
    """the one-sided loss from stock ops: torch.cdist(...).min over chunks of queries (differentiable through cdist)"""
    total = a.new_zeros(())
    for s in range(0, a.shape[0], chunk):
        total = total + (torch.cdist(a[s:s + chunk], b).min(dim=1).values ** 2).sum()
    return total / a.shape[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ns", type=int, nargs="+", default=[1_000, 4_000, 16_000, 100_000])
    ap.add_argument("--qs", type=int, nargs="+", default=[1_000, 16_000, 100_000])
    ap.add_argument("--ks", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--step-points", type=int, default=20_000)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--skip", nargs="*", default=[], choices=["table", "closest", "loss", "step"])
    a = ap.parse_args()
    faulthandler.enable()
    assert torch.cuda.is_available(), "knn_query_cost.py measures on the GPU"
    dev = torch.device("cuda:0")
    print(f"box: {torch.cuda.get_device_name(0)}; torch {torch.__version__}; reps {a.reps} (median / min of device events, ms)")
    run = lambda q, p, k, boxed: simple_knn._knn_query_i32(q, p, k, boxed=boxed)  # noqa: E731

    if "table" not in a.skip:
        print(f"{'N':>8} {'Q':>8} {'K':>3} {'pruned':>16} {'brute':>16} {'brute / pruned':>15}")
        wins = {}
        for N in a.ns:
            p = cube(N, 0, dev)
            for Q in a.qs:
                q = cube(Q, 1, dev)
                for K in a.ks:
                    w_med, w_min = device_ms(lambda: run(q, p, K, True), a.reps)
                    b_med, b_min = device_ms(lambda: run(q, p, K, False), a.reps)
                    wins.setdefault(N, []).append(w_med < b_med)
                    print(f"{N:8d} {Q:8d} {K:3d} {w_med:8.3f}/{w_min:7.3f} {b_med:8.3f}/{b_min:7.3f} {b_med / w_med:15.2f}", flush=True)
        ok = [N for N in sorted(wins) if all(all(wins[M]) for M in sorted(wins) if M >= N)]
        print(f"pruned wins at every Q and K of the table from N = {ok[0] if ok else 'none of the table'} "
              f"(simple_knn.QUERY_BOXED_FROM = {simple_knn.QUERY_BOXED_FROM})")

    if "closest" not in a.skip:
        from scipy.spatial import cKDTree
        n_gt, n_gauss = 2_000, 100_000
        rng = np.random.default_rng(7)
        gt_np, gauss_np = rng.normal(size=(n_gt, 3)).astype(np.float32), rng.normal(size=(n_gauss, 3)).astype(np.float32)
        gt, gauss = torch.tensor(gt_np, device=dev), torch.tensor(gauss_np, device=dev)
        w = device_ms(lambda: run(gt, gauss, 1, True), a.reps)
        b = device_ms(lambda: run(gt, gauss, 1, False), a.reps)
        chunk = 250             # [100 000, 250, 3] float32 = 300 MB per repeated tensor; all 2 000 at once would be 2.4 GB each, four alive
        r = device_ms(lambda: reference_closest(gt, gauss, chunk), max(3, a.reps // 4), warm=1)
        same = bool(torch.equal(reference_closest(gt, gauss, chunk), run(gt, gauss, 1, True)[1][:, 0].long()))
        t0 = time.perf_counter()
        _dd, ii = cKDTree(gauss_np).query(gt_np, 1, workers=16)
        host = (time.perf_counter() - t0) * 1e3
        same_host = bool(np.array_equal(ii, run(gt, gauss, 1, True)[1][:, 0].cpu().numpy()))
        print(f"find_closest_gauss {n_gt} x {n_gauss}: pruned {w[0]:.3f}/{w[1]:.3f}  brute {b[0]:.3f}/{b[1]:.3f}  reference formulation in torch "
              f"(chunks of {chunk} gt points) {r[0]:.3f}/{r[1]:.3f} (same indices: {same})  host cKDTree 16 workers {host:.1f} (same indices: {same_host})")
        print(f"  ratios to the pruned form: brute x {b[0] / w[0]:.2f}, torch formulation x {r[0] / w[0]:.1f}, host cKDTree x {host / w[0]:.1f}")

    if "loss" not in a.skip:
        from csplat.pointcloud import chamfer_distance
        x, y = cube(50_000, 2, dev).requires_grad_(), cube(100_000, 3, dev).requires_grad_()

        def ours():
            x.grad = y.grad = None
            chamfer_distance(x, y, two_sided=False).backward()

        def composed():
            x.grad = y.grad = None
            composed_chamfer(x, y, 5_000).backward()     # [5 000, 100 000] float32 = 2 GB per chunk, kept for backward: 20 GB
        o = device_ms(ours, a.reps)
        c = device_ms(composed, max(3, a.reps // 4), warm=1)
        print(f"chamfer_distance 50 000 -> 100 000 one-sided, forward + backward: kernels {o[0]:.3f}/{o[1]:.3f}  torch.cdist(...).min in chunks of "
              f"5 000 queries {c[0]:.3f}/{c[1]:.3f}  (x {c[0] / o[0]:.1f})")
        del x, y
        torch.cuda.empty_cache()

    if "step" not in a.skip:
        import bench_train as bt
        from csplat import train as tr
        from csplat.optim import GroupedAdam
        from gaussian_renderer import render_views
        n_times = 30
        times = [k / (n_times - 1) for k in (9, 10, 11)]

        def measure(lam):
            torch.manual_seed(0)
            sc, pc, sim = bt.build(100_000, 800, 800, 100, n_times, dev)
            bg = torch.ones(3, device=dev)
            with torch.no_grad():
                res = render_views(bt.cameras(sc, times, dev), pc, sim, tr.DEFAULT_PIPE, bg)
                targets = [r.render.clamp(0, 1).clone() for r in res]
                gen = torch.Generator(device=dev).manual_seed(1)
                clouds = [r.means3D_deform[torch.randperm(100_000, device=dev, generator=gen)[:a.step_points]] +
                          0.01 * torch.randn(a.step_points, 3, device=dev, generator=gen) for r in res]
            cams = bt.cameras(sc, times, dev, targets)
            for c, p in zip(cams, clouds):
                c.points = p.contiguous()
            pc.training_setup(feature_lr=tr.DEFAULT_OPT.feature_lr)
            mopt = GroupedAdam(sim.parameters(), lr=tr.DEFAULT_OPT.meshnet_lr)
            opt = SimpleNamespace(**vars(tr.DEFAULT_OPT), **({} if lam is None else dict(lambda_chamfer=lam)))
            ts = []
            for it in range(1, 6 + a.steps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                tr.train_step(it, cams, pc, sim, mopt, opt=opt, background=bg)
                torch.cuda.synchronize()
                ts.append((time.perf_counter() - t0) * 1e3)
            ts = ts[5:]
            return float(np.median(ts)), float(np.min(ts))
        off, on = measure(None), measure(0.5)
        print(f"train step (eager, P = 100k, 3 cameras 800 x 800), {a.steps} steps, wall ms median / min: without the term {off[0]:.3f}/{off[1]:.3f}  "
              f"with lambda_chamfer = 0.5 and {a.step_points} observed points per camera {on[0]:.3f}/{on[1]:.3f}  "
              f"(the term: + {on[0] - off[0]:.3f} ms)")


if __name__ == "__main__":
    main()
