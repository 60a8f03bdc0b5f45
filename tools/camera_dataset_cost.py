"""Cost of feeding a reconstruction train step its ground truth (csplat.camera_dataset), written to profiles/camera_dataset_cost.txt.

The ground-truth images and masks of one step's cameras, four ways:

  step       CameraDataset.step(view, time_ids): ONE launch (csplat_camera_batch) out of 8-bit levels resident on the device, the camera
             records; the slot indices went through one small pinned upload the first time this set of slots was asked for (the
             warm-up), the timed calls find them on the device;
  planned    the same after CameraDataset.plan(schedule): the indices of 4096 steps uploaded once (re-planned when they are used up: the
             re-plan is inside the timed window);
  cat        (a) what the parent commit lets a user write: float32 images and masks resident on the device, the torch.cat of
             csplat.train._gt_stack and the torch.cat of train_step's masks.  Timed TWICE per round (cat a, cat b): their difference is
             the run-to-run spread of this measurement;
  host       (b) the reference's way: float32 images and masks on the (pageable) host, `.to(device)` per camera and step, then the
             same two torch.cat.

Rows: 3 cameras at 800 x 800, 1 camera at 800 x 800, 3 cameras at 400 x 400, each with and without masks.  Beside each: one eager
train_step (100 000 Gaussians on a 100 x 100 mesh, bench_train.py's scene, at the row's resolution and camera count) on data-set cameras
and the share of it that each form costs; and the kernel's own time from device events around back-to-back launches, with the rate on its
algorithmic bytes -- (3 + m) H W read and 4 (3 + m) H W written per camera -- as a fraction of the 8.0 TB/s HBM peak (the memory bound is
the only bound of this kernel; a float4 copy reaches 6.29 TB/s, 79 %).

A host clock around `calls` back-to-back calls that end in a device synchronise (the forms are bound by the host: device events alone
would miss the time between launches); after a warm-up of every form; `calls` is chosen per form so that a timed window lasts about
--window seconds; the forms alternate over --rounds rounds, every round's figure is printed and the MEDIAN is the figure of a form.  A
record, not a pass condition; the tool fails without a GPU."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "cloth-splatting_amd"), ROOT, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

from meshnet_train_cost import measure  # noqa: E402  (warm-up, calls sized to the window, alternating rounds)

HBM_PEAK = 8.0e12       # bytes / s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.3, help="seconds of work per timed window")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--P", type=int, default=100_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "camera_dataset_cost.txt"))
    a = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("camera_dataset_cost: no GPU; a time is only measured on one")
    import bench_train as bt
    from csplat import native, synthetic as syn, train as tr
    from csplat.camera_dataset import CameraDataset
    from csplat.scene_io import CameraInfo
    dev = torch.device("cuda:0")
    lines = []

    def say(*parts):
        lines.append(" ".join(str(p) for p in parts))
        print(lines[-1], flush=True)

    def infos_of(sc, res, n_times, masks, gen):
        c = sc["cameras"][0]
        R, T = syn.c2w_to_RT(syn.pose_spherical(-180.0, -30.0, 4.0))
        out = []
        for t in range(n_times):
            img = torch.randint(0, 256, (3, res, res), dtype=torch.uint8, generator=gen) / 255.0
            msk = 1.0 - torch.randint(0, 256, (1, res, res), dtype=torch.uint8, generator=gen) / 255.0 if masks else None
            out.append(CameraInfo(uid=t, R=R, T=T, FovY=c["FoVy"], FovX=c["FoVx"], image=img, image_path="", image_name=f"r_0_{t}", width=res,
                                  height=res, time=t / (n_times - 1), view_id=0, time_id=t, flow=None, mask=msk))
        return out

    say("device", torch.cuda.get_device_name(0))
    say("measurement", dict(window_s=a.window, rounds=a.rounds, figure="median of the rounds", gaussians=a.P, train_step="eager, data-set cameras"))
    say("ground truth of one step, and one train_step on it, ms per call; share = form / train_step; kernel: device events, "
        "algorithmic bytes over time, as a fraction of the 8.0 TB/s HBM peak (the same slots and outputs every launch: at most 38 MB, which the "
        "256 MB Infinity Cache can hold, so the rate is an upper figure for a step that finds them cold)")
    say("cameras | H x W | masks | step | planned | cat a | cat b | cat spread | host | step / cat | train_step | share step | share planned | "
        "share cat | share host | kernel ms | kernel GB/s | of HBM peak | rounds (step; planned; cat a; cat b; host; train_step)")
    before = sum(native.FALLBACK_COUNTS.values())
    gen, n_times, verdicts = torch.Generator().manual_seed(5), 30, []
    for n_cams, res in ((3, 800), (1, 800), (3, 400)):
        torch.manual_seed(0)
        sc, pc, sim = bt.build(a.P, res, res, 100, n_times, dev)
        pc.training_setup()
        mopt = torch.optim.Adam(sim.parameters(), lr=3e-4)
        bg = torch.ones(3, device=dev)
        for masks in (True, False):
            infos = infos_of(sc, res, n_times, masks, gen)
            ds = CameraDataset(infos, device=dev, rng=np.random.default_rng(0))
            assert ds.storage == "uint8"
            times = [9, 10, 11][:n_cams]
            key = (0, times)
            resident = [(i.image.to(dev), None if i.mask is None else i.mask.to(dev)) for i in (infos[t] for t in times)]
            on_host = [(infos[t].image, infos[t].mask) for t in times]

            def step():
                return ds.step(*key)

            def planned():
                if ds._plan is None or ds._plan.at >= len(ds._plan.keys):
                    ds.plan([key] * 4096)
                return ds.step(*key)

            def cats(pairs):
                gt = torch.cat([im.unsqueeze(0) for im, _ in pairs], 0)
                return gt, (torch.cat([m.unsqueeze(0) for _, m in pairs], 0) if masks else None)

            def cat():
                return cats(resident)

            def host():
                return cats([(im.to(dev), None if m is None else m.to(dev)) for im, m in on_host])

            got, want = step(), cat()                 # the forms produce the same tensors
            assert torch.equal(got.gt, want[0]) and torch.equal(got.gt, host()[0]) and (not masks or torch.equal(got.mask, want[1]))
            cams = ds.step(*key)
            it = [0]

            def train():
                it[0] += 1
                return tr.train_step(it[0] % 900 + 1, cams, pc, sim, mopt, background=bg)

            runs, calls = measure({"step": step, "planned": planned, "cat a": cat, "cat b": cat, "host": host}, a.window, a.rounds)
            ds._plan = None
            step_runs, step_calls = measure({"train_step": train}, a.window, a.rounds, max_calls=200)
            # the kernel alone: device events around back-to-back launches on indices that are on the device already
            slots = list(got.slots)
            idx = torch.tensor(slots, dtype=torch.int32).to(dev)
            reps = 200
            out_gt, out_mask = torch.empty_like(got.gt), (torch.empty_like(got.mask) if masks else None)
            args = (native.stream_handle(dev), n_cams, res, res, 0, int(masks), ds.n_slots, ds._pitch, native.ptr(ds._store), native.ptr(idx),
                    native.ptr(out_gt), native.ptr(out_mask))
            for _ in range(20):
                native.check(native.lib.csplat_camera_batch(*args), "csplat_camera_batch")
            assert torch.equal(out_gt, got.gt)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            kernel = []
            for _ in range(a.rounds):
                torch.cuda.synchronize()
                e0.record()
                for _ in range(reps):
                    native.lib.csplat_camera_batch(*args)
                e1.record()
                torch.cuda.synchronize()
                kernel.append(e0.elapsed_time(e1) / reps)
            k_ms = statistics.median(kernel)
            nbytes = n_cams * (3 + int(masks)) * res * res * 5
            rate = nbytes / (k_ms * 1e-3)
            med = {k: statistics.median(v) for k, v in runs.items()}
            train_ms = statistics.median(step_runs["train_step"])
            spread, best = abs(med["cat a"] - med["cat b"]), min(med["cat a"], med["cat b"])
            share = lambda x: f"{100 * x / train_ms:.2f} %"  # noqa: E731
            say(f"{n_cams} | {res} x {res} | {'yes' if masks else 'no'} | {med['step']:.4f} | {med['planned']:.4f} | {med['cat a']:.4f} | "
                f"{med['cat b']:.4f} | {spread:.4f} | {med['host']:.4f} | {med['step'] / best:.3f} | {train_ms:.3f} | {share(med['step'])} | "
                f"{share(med['planned'])} | {share(best)} | {share(med['host'])} | {k_ms:.4f} | {rate / 1e9:.0f} | {100 * rate / HBM_PEAK:.1f} % | "
                f"{runs['step']}; {runs['planned']}; {runs['cat a']}; {runs['cat b']}; {runs['host']}; {step_runs['train_step']} "
                f"({calls['step']}; {calls['planned']}; {calls['cat a']}; {calls['cat b']}; {calls['host']}; {step_calls['train_step']} calls per window; "
                f"kernel rounds {[round(k, 4) for k in kernel]}, events around {reps} launches each: the launches' own gaps are inside)")
            ahead = med["step"] < best - spread
            verdicts.append((n_cams, res, masks, ahead))
            say(f"  verdict at {n_cams} cameras, {res} x {res}, masks {'yes' if masks else 'no'}: step() is " +
                ("AHEAD of" if ahead else "NOT ahead of") + " form (a), the resident torch.cat, beyond its run-to-run spread")
    assert sum(native.FALLBACK_COUNTS.values()) == before, "a form took a composed-torch branch"
    behind = [v[:3] for v in verdicts if not v[3]]
    say("rows in which step() is not ahead of form (a) (cameras, resolution, masks):", behind if behind else "none")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
