"""Cost of the Delaunay triangulation on the device (csplat.triangulate.delaunay -> csplat_delaunay), written to
profiles/delaunay_cost.txt: N in {300, 2 000, 10 000} points, as a seeded uniform cloud and as a regular grid (every step of a grid's walk
ties, so the exact stage's price shows), with and without the reference's length threshold, two forms:

1. kernel   delaunay() on a float32 GPU tensor [N,2]: its checks, its allocations, a memset, five kernels of its own and the scan's
            three, and the one blocking read of the counters that sizes the result;
2. host     the path a user had before: the cloud copied to the host, scipy.spatial.Delaunay, the reference's Python loop over simplices
            with its length filter (meshnet/data_utils.py:378-404), and the edges and faces copied back to the device.  On one host core,
            because such a loop cannot use more.  Left out with a note when SciPy is absent.

Both forms end synchronised with their result on the device, so both are timed on the host clock around `calls` back-to-back calls after a
warm-up; `calls` is chosen per form so that a timed window lasts about --window seconds (at least 2 calls); the forms alternate over
--rounds rounds and every round's figure is printed (their spread is the noise of this measurement); the table holds each form's best
round.  Where the kernel is slower than the host path the line says so.  A record, not a pass condition; the tool fails without a GPU."""
import argparse
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "cloth-splatting_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)


def _wall(fn, calls):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6 / calls          # us per call


def measure(forms, window, rounds):
    calls = {}
    for name, fn in forms.items():
        fn()
        est = _wall(fn, 1)
        calls[name] = int(min(max(math.ceil(window * 1e6 / max(est, 1e-3)), 2), 2000))
    runs = {name: [] for name in forms}
    for _ in range(rounds):
        for name, fn in forms.items():
            runs[name].append(round(_wall(fn, calls[name]), 1))
    return runs, calls


def host_path(points_gpu, norm_threshold, Delaunay):
    """download, SciPy, the reference's loop, upload"""
    import numpy as np
    import torch
    points2d = points_gpu.cpu().numpy()
    tri = Delaunay(points2d)
    edges, faces = set(), []
    for simplex in tri.simplices:
        valid_face = True
        for i in range(3):
            p1, p2 = simplex[i], simplex[(i + 1) % 3]
            norm = np.linalg.norm(points2d[p1] - points2d[p2])
            if norm_threshold is not None and norm > norm_threshold:
                valid_face = False
            else:
                edges.add((min(p1, p2), max(p1, p2)))
        if valid_face:
            faces.append(simplex)
    edge_index = torch.tensor(np.asarray(list(edges)).reshape(-1, 2), dtype=torch.long).t().contiguous().to(points_gpu.device)
    faces = torch.tensor(np.asarray(faces).reshape(-1, 3), dtype=torch.long).t().contiguous().to(points_gpu.device)
    return edge_index, faces


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, nargs="+", default=[300, 2000, 10000])
    ap.add_argument("--window", type=float, default=0.3, help="seconds of work per timed window")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "delaunay_cost.txt"))
    a = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("delaunay_cost: no GPU; a time is only measured on one")
    from csplat import triangulate
    try:
        from scipy.spatial import Delaunay
    except ImportError:
        Delaunay = None
    dev = torch.device("cuda:0")
    lines = []

    def say(*parts):
        lines.append(" ".join(str(p) for p in parts))
        print(lines[-1], flush=True)

    say("device", torch.cuda.get_device_name(0))
    say("shape", dict(points=a.points, window_s=a.window, rounds=a.rounds))
    if Delaunay is None:
        say("host: SciPy is absent on this machine -- the path a user had before is not timed, the host column is left out")
    table = []
    for N in a.points:
        side = max(int(round(math.sqrt(N))), 2)
        clouds = {"random": np.random.default_rng(N).random((N, 2), dtype=np.float32),
                  "grid": (np.stack(np.meshgrid(np.arange(side), np.arange(side), indexing="ij"), -1).reshape(-1, 2).astype(np.float32)
                           * np.float32(0.02))}
        for kind, pts in clouds.items():
            n = len(pts)
            P = torch.from_numpy(pts).to(dev)
            # a threshold that keeps the short edges: 1.2 x the spacing of a grid of this density (a grid's diagonals go, its sides stay)
            spacing = 0.02 if kind == "grid" else 1.0 / math.sqrt(n)
            for thr in (None, 1.2 * spacing):
                forms = {"kernel": lambda: triangulate.delaunay(P, thr)}
                if Delaunay is not None:
                    forms["host"] = lambda: host_path(P, thr, Delaunay)
                runs, calls = measure(forms, a.window, a.rounds)
                got = forms["kernel"]()
                note = ""
                if Delaunay is not None:
                    ei, faces = forms["host"]()
                    same_edges = set(map(tuple, ei.t().tolist())) == set(map(tuple, got.edge_index.t().tolist()))
                    note = (f"; host: {faces.shape[1]} faces, {ei.shape[1]} edges, the edge sets are " +
                            ("equal" if same_edges else "DIFFERENT (cocircular points: Qhull's choice is not the tie rule's)"))
                bk = min(runs["kernel"])
                bh = min(runs["host"]) if Delaunay is not None else None
                say(f"N={n} {kind} threshold={thr}: kernel rounds {runs['kernel']} ({calls['kernel']} calls)" +
                    ("" if bh is None else f", host rounds {runs['host']} ({calls['host']} calls)") +
                    f"; kernel: {got.faces.shape[1]} faces, {got.edge_index.shape[1]} edges, {got.exact_decisions} exact decisions{note}")
                table.append((n, kind, thr, bk, bh, got.exact_decisions))
    say("")
    say("     N |   cloud | threshold | kernel us |   host us | host / kernel | exact decisions")
    for n, kind, thr, bk, bh, exact in table:
        slow = "  <- the kernel is SLOWER than the host path here" if bh is not None and bk > bh else ""
        hs = "        - |             -" if bh is None else f"{bh:>9.0f} | {bh / bk:>13.1f}"
        say(f"{n:>6} | {kind:>7} | {'none' if thr is None else format(thr, '.4f'):>9} | {bk:>9.1f} | {hs} | {exact:>15}{slow}")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
