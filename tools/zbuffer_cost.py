"""Cost of the mesh z-buffer (csplat.zbuffer.rasterize_mesh) at the workload's sizes, written to profiles/zbuffer_cost.txt:

grid cloth meshes (csplat.synthetic.grid_mesh) of about 300, 2 000 and 10 000 nodes in 1 view of 400 x 400 and in 4 views of 800 x 800,
microseconds, the median of --rounds rounds of --calls back-to-back calls after a warm-up (device events): per call through
csplat.zbuffer (with its checks and allocations), and per kernel (k_zb_project / clear / draw / resolve) from one profiled call.  Beside it,
for scale: the library's own forward Gaussian render of the same views (the scene of bench.py, --gaussians Gaussians, one
GaussianRasterizer call per view), and the numpy oracle tests/zbuffer_ref.py on one host core (one run of view 0, reported per view).
The draw issues one 8-byte atomic request per covered (face, pixel) pair: their number in view 0 (from the oracle) stands beside the
draw's time.  A record, not a pass condition; every row where the call is slower than the render it is compared with says so.  The tool
fails without a GPU."""
import argparse
import os
import statistics
import sys
import time
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "cloth-splatting_amd"), os.path.join(ROOT, "tests"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

KERNELS = ("k_zb_project", "k_zb_clear", "k_zb_draw", "k_zb_resolve")


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


def median_us(fn, calls, rounds):
    for _ in range(3):
        fn()
    runs = [round(_events(fn, calls), 2) for _ in range(rounds)]
    return statistics.median(runs), runs


def per_kernel(fn):
    """{kernel: us} of one profiled call (after a warm-up), summed over the launches whose name holds the kernel's; {} without a profiler"""
    import torch
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        out = {}
        for ev in prof.events():
            for k in KERNELS:
                if k in ev.name:
                    out[k] = out.get(k, 0.0) + float(getattr(ev, "device_time", 0.0) or getattr(ev, "cuda_time", 0.0))
        return out
    except Exception as e:          # a record, not a pass condition: say what is missing
        print("per-kernel times unavailable:", repr(e), flush=True)
        return {}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--gaussians", type=int, default=100_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "zbuffer_cost.txt"))
    a = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("zbuffer_cost: no GPU; a time is only measured on one")
    import zbuffer_ref as R
    from csplat import native, observation as ob, synthetic as syn, zbuffer as zb
    from diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer
    dev = torch.device("cuda:0")
    lines = []

    def say(*parts):
        lines.append(" ".join(str(p) for p in parts))
        print(lines[-1], flush=True)

    say("device", torch.cuda.get_device_name(0))
    say("shape", dict(calls=a.calls, rounds=a.rounds, gaussians=a.gaussians), "-- microseconds, the median of the rounds")
    before = sum(native.FALLBACK_COUNTS.values())
    T = lambda x: torch.tensor(np.asarray(x, np.float32), device=dev)  # noqa: E731
    for V, S in ((1, 400), (4, 800)):
        cams = [syn.make_camera(-180.0 + 360.0 * v / V + 20.0, S, S) for v in range(V)]
        K4 = np.array([ob.camera_intrinsics(SimpleNamespace(**c), S, S) for c in cams], np.float32)
        W2C = np.stack([c["world_view_transform"].astype(np.float64).T[:3] for c in cams]).astype(np.float32)
        kg, mg = T(K4), T(W2C)
        # the Gaussian render of the same views, for scale
        g = syn.gaussians_at(syn.scene_1(P=a.gaussians, W=S, H=S, n_cams=1))
        inp = {k: T(g[k]) for k in ("means3D", "opacities", "shs", "scales", "rotations")}
        inp["means2D"] = torch.zeros(a.gaussians, 3, device=dev)
        settings = [GaussianRasterizationSettings(image_height=S, image_width=S, tanfovx=c["tanfovx"], tanfovy=c["tanfovy"], bg=T([0.0, 0.0, 0.0]),
                                                  scale_modifier=1.0, viewmatrix=T(c["world_view_transform"]), projmatrix=T(c["full_proj_transform"]),
                                                  sh_degree=3, campos=T(c["camera_center"]), prefiltered=False, debug=False) for c in cams]

        def render():
            with torch.no_grad():
                for s in settings:
                    GaussianRasterizer(s)(**inp)
        r_us, r_runs = median_us(render, max(a.calls // 5, 5), a.rounds)
        say(f"{V} x {S} x {S}: forward Gaussian render of {a.gaussians} Gaussians, {V} calls: {r_us} us, rounds {r_runs}")
        for g_side in (17, 45, 100):
            pos, faces, _edges = syn.grid_mesh(g_side)
            vg, fg = T(pos), torch.from_numpy(faces).to(dev)
            call = lambda: zb.rasterize_mesh(vg, fg, (S, S), intrinsics=kg, world_to_cam=mg)  # noqa: E731
            us, runs = median_us(call, a.calls, a.rounds)
            kern = per_kernel(call)
            images = zb.rasterize_mesh(vg, fg, (S, S), intrinsics=kg, world_to_cam=mg, return_screen=True)
            screen = images.screen[:1].cpu().numpy()
            t0 = time.perf_counter()
            r = R.raster(screen, faces, S, S)
            host = (time.perf_counter() - t0) * 1e6
            equal = bool(np.array_equal(images.face_id[0].cpu().numpy(), r["face32"][0]))
            pairs, covered = int(r["count"].sum()), float((r["count"] > 0).mean())
            what = f"{V} x {S} x {S}, {len(pos)} nodes, {len(faces)} faces"
            say(f"{what}: per call {us} us, rounds {runs}")
            say(f"{what}: per kernel " + ", ".join(f"{k[5:]} {kern[k]:.1f} us" for k in KERNELS if k in kern) + ("" if kern else "unavailable"))
            say(f"{what}: view 0 -- the mesh covers {covered:.3f} of the image, {pairs} covered (face, pixel) pairs = atomic requests of the draw"
                + (f", {pairs * V / kern['k_zb_draw']:.0f} requests per us over the views" if kern.get("k_zb_draw") else ""))
            say(f"{what}: numpy oracle on one host core {host:.0f} us per view ({host * V / us:.0f} x the call for {V} views); face_id of view 0 equal: {equal}")
            say(f"{what}: call / Gaussian render = {us / r_us:.3f}" + ("  -- the call is SLOWER than the render of the same views" if us > r_us else ""))
    assert sum(native.FALLBACK_COUNTS.values()) == before, "a kernel form took the composed path"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
