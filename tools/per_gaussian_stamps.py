"""tools/per_gaussian_stamps.py -- where a wave of the batched K1 (k_preprocess_views) and K8 (k_preprocess_bwd_views) spends its life, on the
step of bench.py (4 views 800x800, P = 100k): s_memtime stamps left by thread 0 of every workgroup (csplat_debug_stamps with a buffer of
8 u64 per workgroup of the two kernels: k_preprocess_views_stamps, k_preprocess_bwd_views_stamps), reduced to averages over the workgroups
whose thread 0 -- Gaussian 64 b of view 0 in K1, Gaussian 32 b of view 0 in K8 -- was visible and so passed every stamp.
GPU box:  python3 tools/per_gaussian_stamps.py"""
import os
import sys
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cloth-splatting_amd")); sys.path.insert(0, ROOT)
from csplat import native, synthetic as syn
from diff_gaussian_rasterization import GaussianRasterizationSettings, rasterize_views

dev = torch.device("cuda:0")
P, W, H, V = 100_000, 800, 800, 4
sc = syn.scene_1(P=P, W=W, H=H, n_cams=V)
g = syn.gaussians_at(sc)
T = lambda a, rg=False: torch.tensor(np.asarray(a, np.float32), device=dev, requires_grad=rg)  # noqa: E731
params = {k: T(g[k], True) for k in ("means3D", "opacities", "shs", "scales", "rotations")}
settings = [GaussianRasterizationSettings(image_height=H, image_width=W, tanfovx=c["tanfovx"], tanfovy=c["tanfovy"], bg=T(sc["bg"]), scale_modifier=1.0,
                                          viewmatrix=T(c["world_view_transform"]), projmatrix=T(c["full_proj_transform"]), sh_degree=3,
                                          campos=T(c["camera_center"]), prefiltered=False, debug=False) for c in sc["cameras"]]
n1, n8 = (P + 63) // 64, (P + 31) // 32
buf = torch.zeros((n1 + n8) * 8, dtype=torch.int64, device=dev)
dp = torch.randn(V, 3, H, W, device=dev)


def step(stamps):
    for p in params.values():
        p.grad = None
    m2d = [torch.zeros(P, 3, device=dev, requires_grad=True) for _ in range(V)]
    native.lib.csplat_debug_stamps(buf.data_ptr() if stamps else None, buf.numel() * 8 if stamps else 0)
    colors, _ = rasterize_views(settings, [dict(means3D=params["means3D"], means2D=m2d[i], opacities=params["opacities"], shs=params["shs"],
                                                scales=params["scales"], rotations=params["rotations"]) for i in range(V)], stacked=True)
    (colors * dp).sum().backward()
    torch.cuda.synchronize()
    native.lib.csplat_debug_stamps(None, 0)


for _ in range(3):
    step(False)
buf.zero_()
step(True)
s = buf.cpu().numpy().reshape(-1, 8).astype(np.int64)
# (s_memtime counts shader cycles per XCD: stamps of DIFFERENT workgroups are not comparable -- only the differences inside one workgroup are used)
for name, rows, waits in (("K1 k_preprocess_views", s[:n1], ("staging loads + barrier", "means3D arrive", "scales, rotations arrive", "opacity arrives",
                                                            "SH evaluation, stores issued")),
                          ("K8 k_preprocess_bwd_views", s[n1:], ("staging loads + barrier", "radius + record arrive", "conic arrives",
                                                                "means3D, cov3D, clamped, rotations, scales arrive (+ the arithmetic between)",
                                                                "rotation gradient, sums, stores issued"))):
    started = rows[:, 0] != 0
    full = rows[(rows[:, :6] != 0).all(1)]
    if not len(full):
        print(f"{name}: no stamps (a library without the stamped kernels, or another launch form)")
        continue
    d = np.diff(full[:, :6], axis=1)
    tot = full[:, 5] - full[:, 0]
    print(f"{name}: {int(started.sum())} workgroups stamped, {len(full)} with every stamp; thread 0 of wave 0 from entry to its last store: "
          f"mean {tot.mean():.0f} cycles, median {np.median(tot):.0f}")
    for k, nme in enumerate(waits):
        print(f"  {nme:80s} mean {d[:, k].mean():7.0f}  median {np.median(d[:, k]):7.0f}  p90 {np.percentile(d[:, k], 90):7.0f}   ({100 * d[:, k].mean() / tot.mean():.0f} %)")
