#!/usr/bin/env python3
"""bench_ssim.py: HIP-event timing on 3x3x800x800 of the fused image loss (csplat_image_loss_fwd / _bwd), of the standalone ssim()
(csplat_ssim_fwd / _bwd: forward alone, and forward + backward) and of GaussianBlur11 (csplat_blur11).  CSPLAT_LIB picks the library."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cloth-splatting_amd")); sys.path.insert(0, ROOT)
import torch
from types import SimpleNamespace
from csplat import train as tr
x = torch.rand(3, 3, 800, 800, device="cuda", requires_grad=True)
y = torch.rand(3, 3, 800, 800, device="cuda")
xc = x.detach()
opt = SimpleNamespace(lambda_dssim=0.2)
N = 50


def timed(first, second=None):
    """mean us of first() and of second(its result) over N rounds, after 5 warm-up rounds"""
    e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    t1 = t2 = 0.0
    for it in range(5 + N):
        x.grad = None
        e[0].record(); r = first(); e[1].record()
        if second is not None:
            second(r)
        e[2].record()
        torch.cuda.synchronize()
        if it >= 5:
            t1 += e[0].elapsed_time(e[1]); t2 += e[1].elapsed_time(e[2])
    return t1 / N * 1e3, t2 / N * 1e3


tf, tb = timed(lambda: tr.image_losses(x, y, opt), lambda l: l.backward())
print(f"fused image loss: fwd {tf:.1f} us  bwd {tb:.1f} us")
with torch.no_grad():
    tf, _ = timed(lambda: tr.ssim(xc, y))
print(f"ssim: fwd {tf:.1f} us")
tf, tb = timed(lambda: tr.ssim(x, y), lambda s: s.backward())
print(f"ssim: fwd+bwd {tf + tb:.1f} us  (fwd with partials {tf:.1f} us, bwd {tb:.1f} us)")
with torch.no_grad():
    tf, _ = timed(lambda: tr.GaussianBlur11.apply(xc))
print(f"GaussianBlur11: fwd {tf:.1f} us")

# the launches alone: the C entries on buffers made once, 200 back to back between two events (no allocation, no autograd in the span)
from csplat import native as n_
from csplat.image_loss import _taps
B, Cc, H, W = xc.shape
p, dx, out = torch.empty(3, *xc.shape, device="cuda"), torch.empty_like(xc), torch.empty_like(xc)
partial = torch.empty(int(n_.lib.csplat_ssim_partial_count(B * Cc, H, W)), device="cuda")
g = torch.ones(1, device="cuda")
P = [n_.ptr(p[k]) for k in range(3)]
entries = {
    "csplat_ssim_fwd (no partials)": lambda: n_.launch("csplat_ssim_fwd", xc.device, B * Cc, H, W, _taps(), n_.ptr(xc), n_.ptr(y), None, None, None, None, n_.ptr(partial)),
    "csplat_ssim_fwd": lambda: n_.launch("csplat_ssim_fwd", xc.device, B * Cc, H, W, _taps(), n_.ptr(xc), n_.ptr(y), *P, None, n_.ptr(partial)),
    "csplat_ssim_bwd": lambda: n_.launch("csplat_ssim_bwd", xc.device, B * Cc, H, W, _taps(), n_.ptr(xc), n_.ptr(y), *P, n_.ptr(g), 1.0 / xc.numel(), None, None, n_.ptr(dx)),
    "csplat_blur11": lambda: n_.launch("csplat_blur11", xc.device, B * Cc, H, W, _taps(), n_.ptr(xc), n_.ptr(out)),
}
for name, fn in entries.items():
    for _ in range(20):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(200):
        fn()
    e1.record()
    torch.cuda.synchronize()
    print(f"{name}: {e0.elapsed_time(e1) / 200 * 1e3:.1f} us per launch")
