"""Cost of the trajectory smoothing (meshnet.data_utils.smooth_clouds -> csplat_traj_smooth), written to profiles/trajectory_cost.txt:
N in {300, 2 000, 16 000} points x T in {1, 30} frames x k in {8, 20}, sigma = 0.1, three forms:

1. kernel    smooth_clouds on a float32 GPU tensor [T,N,3]: one launch of csplat_traj_smooth for all frames (brute force per frame, the
             weighted mean formed from the K-best registers), with its checks and its one allocation;
2. composed  the same result from what the library had before: per frame one simple_knn.knn_query(frame, frame, k) (brute force below
             100 000 points) and a torch gather, exp, multiply and two sums on the GPU;
3. host      the reference's algorithm restated: per frame a SciPy KD-tree, then one tree.query(point, k) and one small weighted sum PER
             POINT in a Python loop -- on one host core, because such a loop cannot use more, whatever number the job is allowed.  It is
             timed on at most --host-frames frames and scaled to T (the frames are alike); the transfers a GPU user would pay around it
             (device -> host -> device) are NOT included.  Left out with a note when SciPy is absent.

The GPU forms: device events around `calls` back-to-back calls after a warm-up; `calls` is chosen per form so that a timed window lasts
about --window seconds; the forms alternate over --rounds rounds and every round's figure is printed (their spread is the noise of this
measurement).  Where the kernel is slower than the composition the line says so.  A record, not a pass condition; the tool fails without a
GPU."""
import argparse
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "cloth-splatting_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)


def _events(fn, calls):
    import torch
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    ev0.record()
    for _ in range(calls):
        fn()
    ev1.record()
    torch.cuda.synchronize()
    return ev0.elapsed_time(ev1) * 1000.0 / calls          # us per call


def measure(forms, window, rounds):
    """forms: {name: callable} -> {name: [us per call, one per round]}; warm-up, then `calls` sized to the window, forms alternating"""
    calls = {}
    for name, fn in forms.items():
        for _ in range(3):
            fn()
        est = _events(fn, 3)
        calls[name] = int(min(max(math.ceil(window * 1e6 / max(est, 1e-3)), 3), 20_000))
    runs = {name: [] for name in forms}
    for _ in range(rounds):
        for name, fn in forms.items():
            runs[name].append(round(_events(fn, calls[name]), 1))
    return runs, calls


def host_smoothing(cloud, k, sigma, KDTree):
    """the reference's algorithm on one frame (numpy float64 [N,3]): a tree, then one query and one weighted sum per point"""
    import numpy as np
    tree = KDTree(cloud)
    out = np.zeros_like(cloud)
    for i in range(len(cloud)):
        dist, near = tree.query(cloud[i], k=k)
        w = np.exp(-dist ** 2 / (2 * sigma ** 2))
        w /= w.sum()
        out[i] = (w[:, None] * cloud[near]).sum(axis=0)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, nargs="+", default=[300, 2000, 16000])
    ap.add_argument("--frames", type=int, nargs="+", default=[1, 30])
    ap.add_argument("--k", type=int, nargs="+", default=[8, 20])
    ap.add_argument("--sigma", type=float, default=0.1)
    ap.add_argument("--window", type=float, default=0.2, help="seconds of work per timed window")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--host-frames", type=int, default=1, help="frames the host form is timed on (scaled to T)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "trajectory_cost.txt"))
    a = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("trajectory_cost: no GPU; a time is only measured on one")
    import simple_knn
    from csplat import native
    from meshnet import data_utils as du
    try:
        from scipy.spatial import KDTree
    except ImportError:
        KDTree = None
    dev = torch.device("cuda:0")
    lines = []

    def say(*parts):
        lines.append(" ".join(str(p) for p in parts))
        print(lines[-1], flush=True)

    say("device", torch.cuda.get_device_name(0))
    say("shape", dict(points=a.points, frames=a.frames, k=a.k, sigma=a.sigma, window_s=a.window, rounds=a.rounds, host_frames=a.host_frames))
    if KDTree is None:
        say("host: SciPy is absent on this machine -- the reference's KD-tree loop is not timed, the host column is left out")
    c = du.weight_scale(a.sigma, torch.float32)

    def composed(P, k):
        outs = []
        for t in range(P.shape[0]):
            d2, idx = simple_knn.knn_query(P[t], P[t], k)
            w = torch.exp(-(d2 * c))
            outs.append((w[..., None] * P[t][idx]).sum(1) / w.sum(1, keepdim=True))
        return torch.stack(outs)

    table = []
    before = sum(native.FALLBACK_COUNTS.values())
    for N in a.points:
        side = max(int(round(math.sqrt(N))), 1)
        rng = np.random.default_rng(N)
        for T in a.frames:
            # a cloth-like sheet: a jittered grid of spacing 0.02 in xy, a ripple in z that moves with the frame
            ij = np.arange(N)
            xy = np.stack([(ij // side) * 0.02, (ij % side) * 0.02], 1) + rng.uniform(-0.004, 0.004, (N, 2))
            frames = np.stack([np.concatenate([xy, 0.02 * np.sin(8 * xy[:, :1] + 0.3 * t) + rng.uniform(-5e-4, 5e-4, (N, 1))], 1) for t in range(T)])
            P = torch.from_numpy(frames.astype(np.float32)).to(dev)
            for k in a.k:
                forms = {"kernel": lambda: du.smooth_clouds(P, k=k, sigma=a.sigma), "composed": lambda: composed(P, k)}
                runs, calls = measure(forms, a.window, a.rounds)
                got, ref = forms["kernel"](), forms["composed"]()
                diff = float((got - ref).abs().max())
                bk, bc = min(runs["kernel"]), min(runs["composed"])
                host = None
                if KDTree is not None:
                    F = min(T, max(a.host_frames, 1))
                    t0 = time.perf_counter()
                    h = [host_smoothing(frames[t].astype(np.float64), k, a.sigma, KDTree) for t in range(F)]
                    host = (time.perf_counter() - t0) * 1e6 * T / F
                    hdiff = float(np.abs(np.stack(h) - got[:F].cpu().numpy()).max())
                say(f"N={N} T={T} k={k}: kernel rounds {runs['kernel']} ({calls['kernel']} calls), composed rounds {runs['composed']} ({calls['composed']} calls); "
                    f"largest |kernel - composed| {diff:.2e}" + ("" if host is None else f"; host {host:.0f} us (timed on {F} of {T} frames), largest |host - kernel| {hdiff:.2e}"))
                table.append((N, T, k, bk, bc, host))
    assert sum(native.FALLBACK_COUNTS.values()) == before, "a kernel form took the composed path"
    say("")
    say("     N |  T |  k | kernel us | composed us | composed / kernel | host us | host / kernel")
    for N, T, k, bk, bc, host in table:
        slow = "  <- the kernel is SLOWER than the composition here" if bk > bc else ""
        hs = "       - |             -" if host is None else f"{host:>8.0f} | {host / bk:>13.0f}"
        say(f"{N:>6} | {T:>2} | {k:>2} | {bk:>9.1f} | {bc:>11.1f} | {bc / bk:>17.2f} | {hs}{slow}")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
