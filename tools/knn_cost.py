"""Cost of exact k-NN with indices (simple_knn.knn: csplat_knn brute force / csplat_knn_ws Morton order + boxes) and of
farthest-point sampling (csplat_fps), next to what they replace, all from one run on one box:
  knn     uniform-cube and cloth-sheet (planar, jittered grid) clouds at P = 10k / 100k / 1M, K = 3 / 10 / 16 / 32; the pruned
          form always, the brute-force form where it is affordable (P <= 100k); device events after warm-up, median of --reps
  dist2   `simple_knn._C.distCUDA2` on the same cloud (its default form for that P) -- the comparator for K = 3
  host    the reference's method, `cKDTree(points).query(points, k + 1, workers=16)` (tree build included, one run)
  fps     N = 5k / 100k, S = 300, against the reference's method restated in numpy (float64, one O(N) pass per selection)
Run it under `rocprofv3 --kernel-trace --stats -- python tools/knn_cost.py` (a separate run) for the per-kernel table."""
import argparse
import faulthandler
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "cloth-splatting_amd"), ROOT):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import simple_knn  # noqa: E402
import simple_knn._C as knn_c  # noqa: E402


def make_cloud(kind, P, seed=0):
    rng = np.random.default_rng(seed)
    if kind == "cube":
        return rng.uniform(-1, 1, (P, 3)).astype(np.float32)
    n = int(np.ceil(np.sqrt(P)))                      # cloth sheet: an n x n grid in the plane, jittered by a fifth of its pitch
    u, v = np.meshgrid(np.linspace(-1, 1, n), np.linspace(-1, 1, n), indexing="ij")
    p = np.stack([u.ravel(), v.ravel(), np.zeros(n * n)], 1)[:P]
    p[:, :2] += rng.normal(0, 0.2 * 2 / n, (P, 2))
    p[:, 2] += rng.normal(0, 0.02 * 2 / n, P)
    return p[rng.permutation(P)].astype(np.float32)


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


def forced(boxed, fn):
    old = simple_knn.BOXED_FROM
    simple_knn.BOXED_FROM = 1 if boxed else 1 << 30
    try:
        return fn()
    finally:
        simple_knn.BOXED_FROM = old


def host_fps(points, S, start=0):
    p = points.astype(np.float64)
    sel = np.zeros(S, dtype=int)
    sel[0] = start
    dist = np.full(len(p), np.inf)
    for s in range(1, S):
        dist = np.minimum(dist, np.linalg.norm(p - p[sel[s - 1]], axis=1))
        sel[s] = np.argmax(dist)
    return sel


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[10_000, 100_000, 1_000_000])
    ap.add_argument("--ks", type=int, nargs="+", default=[3, 10, 16, 32])
    ap.add_argument("--fps-sizes", type=int, nargs="+", default=[5_000, 100_000])
    ap.add_argument("--fps-samples", type=int, default=300)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--brute-max", type=int, default=100_000)
    ap.add_argument("--no-host", action="store_true")
    a = ap.parse_args()
    faulthandler.enable()
    assert torch.cuda.is_available(), "knn_cost.py measures on the GPU"
    from scipy.spatial import cKDTree
    dev = torch.device("cuda:0")
    print(f"box: {torch.cuda.get_device_name(0)}; torch {torch.__version__}; reps {a.reps} (median / min of device events, ms)")
    print(f"{'cloud':6} {'P':>8} {'K':>3} {'pruned':>16} {'brute':>16} {'distCUDA2':>16} {'host cKDTree':>13}")
    for kind in ("cube", "sheet"):
        for P in a.sizes:
            pts = make_cloud(kind, P)
            t = torch.tensor(pts, device=dev)
            d_med, d_min = device_ms(lambda: knn_c.distCUDA2(t), a.reps)
            for K in a.ks:
                w_med, w_min = forced(True, lambda: device_ms(lambda: simple_knn.knn(t, K), a.reps))
                brute = "-"
                if P <= a.brute_max:
                    b_med, b_min = forced(False, lambda: device_ms(lambda: simple_knn.knn(t, K), a.reps))
                    brute = f"{b_med:8.3f}/{b_min:7.3f}"
                host = "-"
                if not a.no_host:
                    t0 = time.perf_counter()
                    cKDTree(pts).query(pts, K + 1, workers=16)
                    host = f"{(time.perf_counter() - t0) * 1e3:10.1f}"
                print(f"{kind:6} {P:8d} {K:3d} {w_med:8.3f}/{w_min:7.3f} {brute:>16} {d_med:8.3f}/{d_min:7.3f} {host:>13}", flush=True)
    print(f"{'fps':6} {'N':>8} {'S':>4} {'csplat_fps':>16} {'us/selection':>13} {'host numpy':>13}")
    for N in a.fps_sizes:
        pts = make_cloud("cube", N, seed=1)
        t = torch.tensor(pts, device=dev)
        S = a.fps_samples
        f_med, f_min = device_ms(lambda: simple_knn.fps(t, S, 0), a.reps)
        host = "-"
        if not a.no_host:
            t0 = time.perf_counter()
            sel = host_fps(pts, S)
            host = f"{(time.perf_counter() - t0) * 1e3:10.1f}"
            same = bool(np.array_equal(sel, simple_knn.fps(t, S, 0).cpu().numpy()))
            host += f" (same selection: {same})"
        print(f"{'fps':6} {N:8d} {S:4d} {f_med:8.3f}/{f_min:7.3f} {f_med * 1e3 / S:13.2f} {host:>13}", flush=True)


if __name__ == "__main__":
    main()
