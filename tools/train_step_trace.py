#!/usr/bin/env python3
"""tools/train_step_trace.py -- every way through csplat.train.train_step once, for a kernel trace or a digest of its results.

  rocprofv3 --kernel-trace --output-format csv -d DIR -o t -- python3 tools/train_step_trace.py             (on the GPU)
  python3 tools/train_step_trace.py --list DIR/.../t_kernel_trace.csv                                         (anywhere)
  python3 tools/train_step_trace.py --summary DIR/.../t_kernel_trace.csv                                      (anywhere)
  python3 tools/train_step_trace.py --digest                                                                  (on the GPU)
  ... [--cases plain,masked,...]                                                          (a subset, in the order given)

The scene: bench_train's, P = 4000 Gaussians, 160 x 128, three cameras (the scene of tests/test_train_gpu.py's captured-step tests).
Every case starts from the same freshly built state and runs in the bit-reproducible mode (csplat_debug_flags 256):
  plain      three eager steps
  masked     the cameras carry a mask
  static     static=True (the rest mesh, no simulator)
  percam     batched_views=False
  geometry   opt.lambda_depth / lambda_silhouette on          chamfer    opt.lambda_chamfer on
  knn        opt.lambda_isometric / lambda_spring / lambda_rigidity on, k_nearest = 5
  allterms   the three optional terms together
  densify    densify_opt with a schedule that densifies, prunes and cleans up within the three steps
  captured   captured=True: an eager step, a recording, replays (four steps in the trace, three in the digest)
  dist       view_parallel=True on ONE rank with the collectives forced (csplat.dist.FORCE_DIST, backend nccl)
A flip kernel (nothing of the step launches one) is launched before and after each case's steps (what lies between two cases is the
next case's setup).  --list prints the kernel names of every case's steps in dispatch order, parameter lists cut off, a `----` line in
front of each case: two commits whose host side issues the same launches print the same text; --summary prints one line per case with a
sha256 of that text (profiles/train_step_dispatch_before_after.txt).  --digest prints per case a sha256 of the bits of every step's PSNR and loss and one
of every parameter and Adam moment after the last step: two commits that compute the same print the same lines
(profiles/train_step_digest_before_after.txt)."""
import hashlib
import os
import sys
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "cloth-splatting_amd"), ROOT, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

CASES = ("plain", "masked", "static", "percam", "geometry", "chamfer", "knn", "allterms", "densify", "captured", "dist")
TERMS = dict(geometry=dict(lambda_depth=0.2, lambda_silhouette=0.5), chamfer=dict(lambda_chamfer=0.7),
             knn=dict(lambda_isometric=1.0, lambda_spring=0.5, lambda_rigidity=0.3, k_nearest=5))
TERMS["allterms"] = {k: v for d in list(TERMS.values()) for k, v in d.items()}


def fixture(torch, dev):
    """the state every case starts from, and cameras that carry every optional field (the fields are only read by the cases that ask)"""
    import bench_train as bt
    from csplat import train as tr
    from csplat.optim import GroupedAdam
    from gaussian_renderer import render_views
    torch.manual_seed(3)
    sc, pc, sim = bt.build(P=4000, W=160, H=128, grid=16, n_times=6, dev=dev)
    bg = torch.ones(3, device=dev)
    times = [0.2, 0.4, 0.6]
    gen = torch.Generator().manual_seed(5)
    with torch.no_grad():
        pc._scaling.add_(0.9)
        sim.output.weight.copy_(1e-3 * torch.randn_like(sim.output.weight))
        keep = pc._features_dc.detach().clone()
        pc._features_dc.add_(0.5 * torch.randn_like(pc._features_dc))
        res, alphas = render_views(bt.cameras(sc, times, dev), pc, sim, tr.DEFAULT_PIPE, bg, return_alpha=True)
        cams = bt.cameras(sc, times, dev, [r.render.clamp(0, 1).clone() for r in res])
        for cam, r, a in zip(cams, res, alphas):
            cam.depth = torch.where(a > 0.5, r.depth / a.clamp_min(1e-6), torch.zeros_like(a))
            cam.silhouette = (a > 0.5).float()
            m = r.means3D_deform.detach().cpu()
            pick = torch.randperm(m.shape[0], generator=gen)[:500]
            cam.points = (m[pick] + 0.02 * torch.randn(500, 3, generator=gen)).to(dev).contiguous()
        pc._features_dc.copy_(keep)
        pc._opacity.sub_(1.0)
    pc.training_setup(feature_lr=0.01)
    pc.densification_setup(percent_dense=0.01)
    mopt = GroupedAdam(sim.parameters(), lr=3e-4)
    torch.cuda.synchronize()
    return pc, sim, mopt, cams, bg


def run(cases, digest):
    if "dist" in cases:
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")      # (as tests/rccl_child.py: read when the runtime starts)
    import torch
    from csplat import dist as cd, native, train as tr
    dev = torch.device("cuda:0")
    torch.cuda.set_device(0)

    def separator():
        torch.cuda.synchronize()
        torch.arange(8, device=dev).flip(0)
        torch.cuda.synchronize()

    native.lib.csplat_debug_flags(256)
    try:
        for name in cases:
            pc, sim, mopt, cams, bg = fixture(torch, dev)
            kw = {}
            if name in TERMS:
                kw["opt"] = SimpleNamespace(**vars(tr.DEFAULT_OPT), **TERMS[name])
            elif name == "masked":
                gen = torch.Generator().manual_seed(9)
                for cam in cams:
                    cam.mask = (torch.rand(1, 128, 160, generator=gen) > 0.3).float().to(dev)
            elif name == "static":
                kw["static"] = True
            elif name == "percam":
                kw["batched_views"] = False
            elif name == "densify":
                kw["densify_opt"] = SimpleNamespace(
                    densify_until_iter=100, densify_from_iter=2, densification_interval=3, opacity_reset_interval=9, pruning_from_iter=2,
                    pruning_interval=4, densify_grad_threshold_fine_init=2e-5, densify_grad_threshold_after=2e-5,
                    opacity_threshold_fine_init=0.05, opacity_threshold_fine_after=0.05, cameras_extent=1.0, white_background=False,
                    bary_cleanup=2)
            elif name == "captured":
                kw["captured"] = True
            elif name == "dist":
                import torch.distributed as dist
                os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
                os.environ.setdefault("MASTER_PORT", str(29500 + (os.getpid() % 2000)))
                if not dist.is_initialized():
                    dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
                cd.FORCE_DIST = True
                kw["view_parallel"] = True
            separator()                                 # after the case's setup, before its steps
            h = hashlib.sha256()
            for it in range(1, (5 if name == "captured" and not digest else 4)):
                torch.manual_seed(100 + it)             # (densification draws its samples from the global generator)
                ps, loss, _stats = tr.train_step(it, cams, pc, sim, mopt, background=bg, **kw)
                if digest:
                    h.update(ps.detach().cpu().numpy().tobytes() + loss.detach().cpu().numpy().tobytes())
            separator()
            if digest:
                hs = hashlib.sha256()
                for o, params in ((pc.optimizer, list(pc.parameters())), (mopt, list(sim.parameters()))):
                    for q in params:
                        st = o.state.get(q) or {}
                        for t in (q, st.get("exp_avg"), st.get("exp_avg_sq")):
                            if t is not None:
                                hs.update(t.detach().cpu().contiguous().numpy().tobytes())
                print(f"{name:9s} psnr+loss {h.hexdigest()[:32]}  state {hs.hexdigest()[:32]}  P {int(pc.num_gaussians)}", flush=True)
            if name == "dist":
                cd.FORCE_DIST = False
                dist.destroy_process_group()
    finally:
        native.lib.csplat_debug_flags(0)
    if not digest:
        print("ran", cases)


def listing(path, summary):
    """the launches of each case's steps (between its two separators; the setup between two cases is left out), a `----` line per case;
    summary: one line per case instead -- its launches, its distinct kernels and a sha256 of its listing"""
    import csv
    from backward_dispatch_trace import short
    rows = list(csv.DictReader(open(path)))
    key = "Dispatch_Id" if "Dispatch_Id" in rows[0] else "Start_Timestamp"
    rows.sort(key=lambda r: int(r[key]))
    inside, cases = False, []
    for r in rows:
        name = short(r["Kernel_Name"])
        if name.startswith("rocprim::"):                        # (as torch's kernels: by name only)
            name = name.split("<", 1)[0]
        if name == "----":
            inside = not inside
            if inside:
                cases.append([])
        elif inside and "arange" not in r["Kernel_Name"]:      # (the separator's operand)
            cases[-1].append(name)
    for i, names in enumerate(cases):
        if summary:
            print(f"case {i + 1:2d}  {len(names):4d} launches  {len(set(names)):3d} kernels  {hashlib.sha256(chr(10).join(names).encode()).hexdigest()[:32]}")
        else:
            print("\n".join(["----"] + names))


if __name__ == "__main__":
    args = sys.argv[1:]
    cases = CASES
    if "--cases" in args:
        i = args.index("--cases")
        cases = tuple(args[i + 1].split(","))
        del args[i:i + 2]
        if not set(cases) <= set(CASES):
            sys.exit(__doc__)
    if len(args) == 2 and args[0] in ("--list", "--summary"):
        listing(args[1], args[0] == "--summary")
    elif args in ([], ["--digest"]):
        run(cases, bool(args))
    else:
        sys.exit(__doc__)
