"""Cost of the tracking kernels (csplat.tracking) at the workload's size, written to profiles/tracking_cost.txt:

1. csplat_track_visibility: 100 000 points x 12 view-frames in 800 x 800 depth images, one launch -- projecting, and the get_mask form
   (pixels given);
2. csplat_track_mte: 30 frames x 100 000 tracked points x 1000 ground-truth tracks, two launches (tracks, mean) -- aligned and plain;

each in three forms on the same GPU tensors: the library's entry point alone on buffers made once (the launches), the call through
csplat.tracking (plus its checks and allocations: where it costs more than the entry point alone, the host is what is measured), and the
torch composition of the same formulas (csplat.tracking._visibility_composed / _mte_composed).  Device events around `calls` back-to-back calls after a warm-up; `calls` is chosen per form so that a timed window lasts about
--window seconds; the forms alternate over --rounds rounds and every round's figure is printed (their spread is the noise of this
measurement).  The algorithmic bytes of a call (what the formulas must read and write, from the shapes) and the rate they imply at the
best time stand beside the times.  A record, not a pass condition; the tool fails without a GPU."""
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
        for _ in range(5):
            fn()
        est = _events(fn, 20)
        calls[name] = int(min(max(math.ceil(window * 1e6 / max(est, 1e-3)), 20), 50_000))
    runs = {name: [] for name in forms}
    for _ in range(rounds):
        for name, fn in forms.items():
            runs[name].append(round(_events(fn, calls[name]), 2))
    return runs, calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=100_000)
    ap.add_argument("--frames", type=int, default=12)
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--times", type=int, default=30)
    ap.add_argument("--gt", type=int, default=1000)
    ap.add_argument("--window", type=float, default=0.3, help="seconds of work per timed window")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tracking_cost.txt"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("tracking_cost: no GPU; a time is only measured on one")
    from csplat import native, tracking as tk
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(1)
    rand = lambda *s: torch.rand(*s, device=dev, generator=gen)  # noqa: E731
    lines = []

    def say(*parts):
        lines.append(" ".join(str(p) for p in parts))
        print(lines[-1], flush=True)

    say("device", torch.cuda.get_device_name(0))
    say("shape", dict(points=a.points, frames=a.frames, size=a.size, times=a.times, gt=a.gt, window_s=a.window, rounds=a.rounds))

    # ---- visibility
    F, N, S = a.frames, a.points, a.size
    X = torch.cat([2.0 * rand(F, N, 2) - 1.0, 2.0 + 2.0 * rand(F, N, 1)], 2)
    full = torch.zeros(4, 4, device=dev)
    full[0, 0] = full[1, 1] = 2.0
    full[2, 2], full[2, 3], full[3, 2] = 1.0001, 1.0, -0.010001
    full, centre = full[None].repeat(F, 1, 1), torch.zeros(F, 3, device=dev)
    depth = 2.0 + 2.5 * rand(F, S, S)
    pix = tk.track_visibility(X, full, centre, None, (S, S)).pixels
    # the library entry itself on buffers made once: what the launches cost without the Python layer's checks and allocations
    out_pix, flags, counts = torch.empty(F, N, 2, device=dev), torch.empty(2, F, N, dtype=torch.uint8, device=dev), \
        torch.empty(F, 2, dtype=torch.int32, device=dev)
    stream = native.stream_handle(dev)

    def raw_visibility(pixels_in):
        native.check(native.lib.csplat_track_visibility(stream, F, N, S, S, X.data_ptr(), None if pixels_in is None else pixels_in.data_ptr(),
                                                        full.data_ptr(), centre.data_ptr(), depth.data_ptr(), 0.2, 1.0, 1e4, out_pix.data_ptr(),
                                                        flags[0].data_ptr(), flags[1].data_ptr(), counts.data_ptr()), "csplat_track_visibility")

    forms = {
        "visibility entry point alone (projecting)": lambda: raw_visibility(None),
        "visibility entry point alone (pixels given)": lambda: raw_visibility(pix),
        "visibility through csplat.tracking (projecting)": lambda: tk.track_visibility(X, full, centre, depth, (S, S)),
        "visibility composed (projecting)": lambda: tk._visibility_composed(X, None, full, centre, depth, S, S, 0.2, 1.0, 1e4),
        "visibility through csplat.tracking (pixels given)": lambda: tk.track_visibility(X, None, centre, depth, (S, S), pixels=pix),
        "visibility composed (pixels given)": lambda: tk._visibility_composed(X, pix, full, centre, depth, S, S, 0.2, 1.0, 1e4),
    }
    before = sum(native.FALLBACK_COUNTS.values())
    runs, calls = measure(forms, a.window, a.rounds)
    assert sum(native.FALLBACK_COUNTS.values()) == before, "a kernel form took the composed path"
    k, c = forms["visibility through csplat.tracking (projecting)"](), forms["visibility composed (projecting)"]()
    say("visibility decisions, kernel against composition: in_image differs at", int((k.in_image != c[1]).sum()), "visible at",
        int((k.visible != c[2]).sum()), "of", F * N, "; visible", int(k.counts[:, 1].sum()))
    # per (frame, point): the point (12) [+ the given pixel (8)] + one depth tap (4) read; pixel (8) + two bytes written; per frame 8 of counts
    bytes_ = {"projecting": F * N * (12 + 4 + 8 + 2) + F * (76 + 8), "pixels given": F * N * (12 + 8 + 4 + 8 + 2) + F * (76 + 8)}
    for name in forms:
        best = min(runs[name])
        b = bytes_["projecting" if "projecting" in name else "pixels given"]
        say(f"{name}: best {best} us per call, rounds {runs[name]}, {calls[name]} calls per window; algorithmic bytes {b} "
            f"({b / best * 1e-3:.1f} GB/s at the best time)")

    # ---- trajectory error
    T, G = a.times, a.gt
    traj = rand(N, 3)[None] + 0.05 * torch.randn(T, N, 3, device=dev, generator=gen).cumsum(0)
    assoc = torch.randint(0, N, (G,), device=dev, generator=gen)
    gt = (traj[:, assoc] + 0.01 * torch.randn(T, G, 3, device=dev, generator=gen)).contiguous()
    rot = torch.randn(T, N, 4, device=dev, generator=gen)
    a32, out_al, out_err, out_mte = assoc.to(torch.int32), torch.empty(T, G, 3, device=dev), torch.empty(T, G, device=dev), \
        torch.empty(G + 1, device=dev)

    def raw_mte(rotations):
        native.check(native.lib.csplat_track_mte(stream, T, N, G, traj.data_ptr(), None if rotations is None else rotations.data_ptr(),
                                                 gt.data_ptr(), a32.data_ptr(), out_al.data_ptr(), out_err.data_ptr(), out_mte.data_ptr(),
                                                 out_mte[G:].data_ptr()), "csplat_track_mte")

    forms = {
        "mte entry point alone (aligned)": lambda: raw_mte(rot),
        "mte entry point alone (no alignment)": lambda: raw_mte(None),
        "mte through csplat.tracking (aligned)": lambda: tk._mte_kernel(gt, traj, rot, assoc),
        "mte composed (aligned)": lambda: tk._mte_composed(gt, traj, rot, assoc),
        "mte through csplat.tracking (no alignment)": lambda: tk._mte_kernel(gt, traj, None, assoc),
        "mte composed (no alignment)": lambda: tk._mte_composed(gt, traj, None, assoc),
    }
    runs, calls = measure(forms, a.window, a.rounds)
    k, c = forms["mte through csplat.tracking (aligned)"](), forms["mte composed (aligned)"]()
    say("mte, kernel against composition: mean", float(k[3]), float(c[3]), "largest |aligned difference|", float((k[0] - c[0]).abs().max()))
    # per (frame, track): gt (12) + the point's row (12) [+ its quaternion (16)] read, aligned (12) + err (4) written; per track 4 + 4 (assoc, mte)
    bytes_ = {"aligned": T * G * (12 + 12 + 16 + 12 + 4) + G * 8, "no alignment": T * G * (12 + 12 + 12 + 4) + G * 8}
    for name in forms:
        best = min(runs[name])
        b = bytes_["aligned" if "(aligned)" in name else "no alignment"]
        say(f"{name}: best {best} us per call, rounds {runs[name]}, {calls[name]} calls per window; algorithmic bytes {b} "
            f"({b / best * 1e-3:.2f} GB/s at the best time)")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
