"""Cost of the fused kNN-graph regularisers (csplat.knn_regs: csplat_knn_regs_graph / _fwd / _bwd) next to the same terms composed
from torch ops ON THE SAME GPU, at N in {10k, 100k} x K in {5, 20}, T = 3, all three terms on, means and rotations requiring
gradients.  Device events after warm-up, median / min of --reps, one process.
  graph     NeighbourGraph.from_points: the k-NN search (simple_knn.knn) + csplat_knn_regs_graph; the latter alone in brackets
  fused     neighbour_regularization forward; forward + backward
  composed  the terms as a user would compose them: [T,N,K,3] gathers, torch.norm, [T-1,N,K,4] gathers, quaternion product by
            unbind / stack, build_rotation into a [.,3,3] tensor, torch.bmm, autograd's index_add scatters in backward
The condition of the table: fused forward + backward is faster than composed forward + backward at every row.
Write the output to profiles/knn_regs_cost.txt."""
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

from csplat.knn_regs import NeighbourGraph, neighbour_regularization  # noqa: E402


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


def quat_mult(q1, q2):
    w1, x1, y1, z1 = q1.unbind(-1)
    w2, x2, y2, z2 = q2.unbind(-1)
    return torch.stack([w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2, w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2,
                        w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2, w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2], -1)


def build_rotation(q):
    q = q / torch.norm(q, dim=-1, keepdim=True)
    r, x, y, z = q.unbind(-1)
    return torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y),
                        2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x),
                        2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], -1).reshape(-1, 3, 3)


def composed(M, Q, graph, lams):
    """the three terms from stock ops, per time row as a training script would write them"""
    idx, T = graph.idx, M.shape[0]
    offs = [M[t][idx] - M[t][:, None] for t in range(T)]
    dists = [torch.norm(o, dim=-1) for o in offs]
    iso = torch.stack([(d - graph.d0).mean() for d in dists]).mean()
    spring, rigid = [], []
    inv = Q.new_tensor([1.0, -1.0, -1.0, -1.0])
    for t in range(1, T):
        spring.append((dists[t] - dists[t - 1]).abs().mean())
        rel = quat_mult(Q[t - 1][idx].reshape(-1, 4), (Q[t][idx] * inv).reshape(-1, 4))
        rot = build_rotation(rel)
        moved = torch.bmm(rot, offs[t].reshape(-1, 3, 1)).reshape(offs[t].shape)
        rigid.append(torch.sqrt(((moved - offs[t - 1]) ** 2).sum(-1) * graph.w + 1e-20).mean())
    return lams[0] * iso + lams[1] * torch.stack(spring).mean() + lams[2] * torch.stack(rigid).mean()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ns", type=int, nargs="+", default=[10_000, 100_000])
    ap.add_argument("--ks", type=int, nargs="+", default=[5, 20])
    ap.add_argument("--rows", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    faulthandler.enable()
    assert torch.cuda.is_available(), "knn_regs_cost.py measures on the GPU"
    dev = torch.device("cuda:0")
    lams = (1.0, 1.0, 1.0)
    print(f"box: {torch.cuda.get_device_name(0)}; torch {torch.__version__}; T = {a.rows}; reps {a.reps} (median / min of device events, ms)")
    print(f"{'N':>7} {'K':>3} | {'graph (regs_graph alone)':>30} | {'fused fwd':>14} {'fused fwd+bwd':>14} | {'composed fwd':>14} "
          f"{'composed fwd+bwd':>17} | {'fwd+bwd ratio':>13} | same loss")
    losing = []
    for N in a.ns:
        rng = np.random.default_rng(N)
        # a cloth-like cloud: a wavy sheet, so that neighbours are spatially coherent as Gaussians on a mesh are
        uv = rng.uniform(-1, 1, (N, 2))
        pts = torch.tensor(np.concatenate([uv, 0.1 * np.sin(3 * uv[:, :1]) * np.cos(2 * uv[:, 1:])], 1).astype(np.float32), device=dev)
        order = torch.argsort((pts[:, 0] * 32).floor() * 64 + (pts[:, 1] * 32).floor())      # coarse cells: nearby points, nearby indices
        pts = pts[order].contiguous()
        M = (pts[None] + 1e-2 * torch.randn(a.rows, N, 3, device=dev)).requires_grad_()
        Q = (torch.randn(1, N, 4, device=dev) + 1e-2 * torch.randn(a.rows, N, 4, device=dev)).requires_grad_()
        for K in a.ks:
            lw = 0.25 * N / K           # w = exp(-lambda_w d^2) of the order of exp(-1) at the K-th neighbour of a sheet of N points on 4 units^2
            g_all = device_ms(lambda: NeighbourGraph.from_points(pts, K, lw), a.reps)
            graph = NeighbourGraph.from_points(pts, K, lw)
            d2 = (graph.d0 * graph.d0).contiguous()
            g_own = device_ms(lambda: NeighbourGraph._build(graph.idx32, d2, lw), a.reps)

            def fused_fwd():
                with torch.no_grad():
                    return neighbour_regularization(M, Q, graph, *lams)[0]

            def fused_both():
                M.grad = Q.grad = None
                neighbour_regularization(M, Q, graph, *lams)[0].backward()

            def composed_fwd():
                with torch.no_grad():
                    return composed(M, Q, graph, lams)

            def composed_both():
                M.grad = Q.grad = None
                composed(M, Q, graph, lams).backward()

            f1, f2 = device_ms(fused_fwd, a.reps), device_ms(fused_both, a.reps)
            c1, c2 = device_ms(composed_fwd, a.reps), device_ms(composed_both, a.reps)
            lf, lc = float(fused_fwd()), float(composed_fwd())
            same = abs(lf - lc) <= 1e-4 * abs(lc)
            ratio = c2[0] / f2[0]
            if not ratio > 1.0:
                losing.append((N, K, ratio))
            print(f"{N:7d} {K:3d} | {g_all[0]:9.3f}/{g_all[1]:7.3f} ({g_own[0]:6.3f}) | {f1[0]:7.3f}/{f1[1]:6.3f} {f2[0]:7.3f}/{f2[1]:6.3f} | "
                  f"{c1[0]:7.3f}/{c1[1]:6.3f} {c2[0]:9.3f}/{c2[1]:7.3f} | {ratio:13.1f} | {same} ({lf:.6g} / {lc:.6g})", flush=True)
    print("fused forward + backward is faster than the composition at every row" if not losing else
          "fused forward + backward LOSES at: " + ", ".join(f"N={n} K={k} (x {r:.2f})" for n, k, r in losing))


if __name__ == "__main__":
    main()
