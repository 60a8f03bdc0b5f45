"""Cost of the observation kernels (csplat.observation) at the workload's size, written to profiles/observation_cost.txt:

1. unproject_depth: 4 views of 800 x 800, a silhouette that covers about a third of each image, stride 1 and 2, one launch for all views;
2. voxel_downsample of the stride-1 cloud at a voxel size that leaves about 1/20 of the points (found by bisection at set-up);
3. observable_nodes of the voxel centroids against 300 and 30 000 nodes, k = 2;

each through csplat.observation (the kernel path, with its checks, allocations and its one blocking read where it has one) and as the
torch composition on the same GPU tensors: boolean indexing (csplat.observation._unproject_composed), torch.unique(return_inverse) +
index_add_ (_voxel_composed, which also reads one count back), simple_knn.knn_query + torch.unique.  Device events around `calls`
back-to-back calls after a warm-up; `calls` is chosen per form so that a timed window lasts about --window seconds; the forms alternate
over --rounds rounds and every round's figure is printed (their spread is the noise of this measurement).  Where the kernel path is slower
than the composition at that size the line says so.  A record, not a pass condition; the tool fails without a GPU."""
import argparse
import math
import os
import sys

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
        est = _events(fn, 5)
        calls[name] = int(min(max(math.ceil(window * 1e6 / max(est, 1e-3)), 5), 20_000))
    runs = {name: [] for name in forms}
    for _ in range(rounds):
        for name, fn in forms.items():
            runs[name].append(round(_events(fn, calls[name]), 2))
    return runs, calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=4)
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--keep", type=float, default=1.0 / 20.0, help="the share of the points the voxel grid should leave")
    ap.add_argument("--window", type=float, default=0.2, help="seconds of work per timed window")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "observation_cost.txt"))
    a = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("observation_cost: no GPU; a time is only measured on one")
    import simple_knn
    from csplat import native, observation as ob, synthetic as syn
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(1)
    lines = []

    def say(*parts):
        lines.append(" ".join(str(p) for p in parts))
        print(lines[-1], flush=True)

    V, S = a.views, a.size
    say("device", torch.cuda.get_device_name(0))
    say("shape", dict(views=V, size=S, keep=round(a.keep, 4), window_s=a.window, rounds=a.rounds))
    cams = [syn.make_camera(-180.0 + 360.0 * v / V, S, S) for v in range(V)]
    K4 = torch.tensor([[S / (2 * c["tanfovx"]), S / (2 * c["tanfovy"]), (S - 1) / 2, (S - 1) / 2] for c in cams], dtype=torch.float32, device=dev)
    C2W = torch.from_numpy(np.stack([np.linalg.inv(c["world_view_transform"].astype(np.float64).T)[:3] for c in cams]).astype(np.float32)).to(dev)
    depth = 3.5 + torch.rand(V, S, S, device=dev, generator=gen)
    yy, xx = torch.meshgrid(torch.arange(S, device=dev), torch.arange(S, device=dev), indexing="ij")
    disc = (((yy - S / 2) ** 2 + (xx - S / 2) ** 2) < (S * S / 3.0) / math.pi).float()
    sil = disc[None].repeat(V, 1, 1).contiguous()
    say("silhouette covers", round(float(sil.mean()), 4), "of each image")

    def faster(kernel, composed):
        return "" if kernel <= composed else "  -- the kernel path is SLOWER than the composition at this size"

    def report(forms, runs, calls, pairs):
        for name in forms:
            say(f"{name}: best {min(runs[name])} us per call, rounds {runs[name]}, {calls[name]} calls per window")
        for what, k, c in pairs:
            bk, bc = min(runs[k]), min(runs[c])
            say(f"{what}: kernel path {bk} us, composed {bc} us, ratio composed / kernel {bc / bk:.2f}{faster(bk, bc)}")

    # ---- unproject
    forms = {}
    for stride in (1, 2):
        forms[f"unproject stride {stride} through csplat.observation"] = \
            lambda s=stride: ob.unproject_depth(depth, intrinsics=K4, cam_to_world=C2W, masks=sil, stride=s)
        forms[f"unproject stride {stride} composed"] = lambda s=stride: ob._unproject_composed(depth, sil, K4, C2W, s, 0.0, 0)
    before = sum(native.FALLBACK_COUNTS.values())
    runs, calls = measure(forms, a.window, a.rounds)
    for stride in (1, 2):
        k, c = forms[f"unproject stride {stride} through csplat.observation"](), forms[f"unproject stride {stride} composed"]()
        say(f"unproject stride {stride}: {k.points.shape[0]} points; kernel against composition: source equal {bool(torch.equal(k.source, c.source))}, "
            f"largest |point difference| {float((k.points - c.points).abs().max()):.3e}")
    report(forms, runs, calls, [(f"unproject stride {s}", f"unproject stride {s} through csplat.observation", f"unproject stride {s} composed")
                                for s in (1, 2)])

    # ---- voxel grid: a size that leaves about `keep` of the points
    cloud = ob.unproject_depth(depth, intrinsics=K4, cam_to_world=C2W, masks=sil).points.contiguous()
    M = int(cloud.shape[0])
    lo, hi = 1e-4, 4.0
    for _ in range(24):
        mid = math.sqrt(lo * hi)
        if ob.voxel_downsample(cloud, mid).counts.shape[0] > a.keep * M:
            lo = mid
        else:
            hi = mid
    size = hi
    forms = {"voxel through csplat.observation": lambda: ob.voxel_downsample(cloud, size),
             "voxel composed": lambda: ob._voxel_composed(cloud, size, None)}
    runs, calls = measure(forms, a.window, a.rounds)
    k, c = forms["voxel through csplat.observation"](), forms["voxel composed"]()[0]
    say(f"voxel: {M} points, size {size:.5f}, {k.counts.shape[0]} voxels ({k.counts.shape[0] / M:.4f} of the points); kernel against composition: "
        f"counts equal {bool(torch.equal(k.counts, c.counts))}, inverse equal {bool(torch.equal(k.inverse, c.inverse))}, "
        f"largest |centroid difference| {float((k.centroids - c.centroids).abs().max()):.3e}")
    report(forms, runs, calls, [("voxel", "voxel through csplat.observation", "voxel composed")])

    # ---- observable nodes of the centroids
    cents = k.centroids.contiguous()
    Q = int(cents.shape[0])
    forms, pairs = {}, []
    nodes_of = {}
    for N in (300, 30_000):
        pick = torch.randint(0, Q, (N,), device=dev, generator=gen)
        nodes_of[N] = (cents[pick] + 0.05 * torch.randn(N, 3, device=dev, generator=gen)).contiguous()
        forms[f"observable N={N} through csplat.observation"] = lambda n=N: ob.observable_nodes(cents, nodes_of[n], k=2)
        forms[f"observable N={N} composed"] = lambda n=N: torch.unique(simple_knn.knn_query(cents, nodes_of[n], 2)[1])
        pairs.append((f"observable N={N} (Q={Q}, k=2)", f"observable N={N} through csplat.observation", f"observable N={N} composed"))
    runs, calls = measure(forms, a.window, a.rounds)
    for N in (300, 30_000):
        flags, idx = forms[f"observable N={N} through csplat.observation"](), forms[f"observable N={N} composed"]()
        say(f"observable N={N}: {int(flags.sum())} nodes observable; kernel against composition: equal {bool(torch.equal(flags.nonzero()[:, 0], idx))}")
    report(forms, runs, calls, pairs)
    assert sum(native.FALLBACK_COUNTS.values()) == before, "a kernel form took the composed path"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
