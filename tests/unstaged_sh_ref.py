"""Inputs of the unstaged-SH tests (tests/test_raster_unstaged_sh_cpu.py, tests/test_raster_unstaged_sh_gpu.py; helper, not collected).

The per-Gaussian kernels of the rasterizer stage the 16 x 3 SH rows through LDS only when M == 16 and the SH tensor (for K8 also dL_dsh)
starts on a 16-byte boundary (include/csplat.h, at `M`); every other SH tensor is served by the unstaged kernels.  Such tensors are made
here from a case's [P, 16, 3] coefficients:
    short(shs, M)    M <= 16: the first M coefficient rows; M = 25: nine extra rows of ONES (a kernel that reads past (D+1)^2 shows)
    padded(shs, M)   the staged twin of short(shs, M): its first min(M, 16) rows, zero-filled to 16
    off16(t)         the same values in a contiguous leaf whose data_ptr() % 16 == 4
The oracles read the first (D+1)^2 rows only, so short and padded are the same computation (held bit for bit by the CPU file)."""
import numpy as np

# (M, D) of the short tensors; (16, D) is run with off16
PAIRS = [(1, 0), (4, 0), (4, 1), (9, 1), (9, 2), (25, 3)]
OFF16_DEGREES = [0, 1, 2, 3]
# the three configurations of tests/test_raster_gpu.py:CASES
CASES = [
    dict(P=2000, W=128, H=96, seed=7, grid=20, scale_mul=1.0),
    dict(P=3000, W=200, H=136, seed=8, grid=16, scale_mul=2.5),     # ragged: W,H not multiples of 16
    dict(P=800, W=64, H=64, seed=9, grid=10, scale_mul=4.0, radius=1.2),  # close camera: frustum clamp + culling
]
CULLING = 2     # index of the case whose culled Gaussians take K8's `!vis` branch


def short(shs, M):
    shs = np.asarray(shs)
    assert shs.ndim == 3 and shs.shape[1:] == (16, 3), shs.shape
    if M <= 16:
        return np.ascontiguousarray(shs[:, :M])
    assert M == 25, M
    return np.ascontiguousarray(np.concatenate([shs, np.ones((shs.shape[0], 9, 3), shs.dtype)], 1))


def padded(shs, M):
    shs = np.asarray(shs)
    assert shs.ndim == 3 and shs.shape[1:] == (16, 3), shs.shape
    out = np.zeros_like(shs)
    k = min(M, 16)
    out[:, :k] = shs[:, :k]
    return out


def off16(t):
    """a contiguous leaf with the values of `t`, 4 bytes past a 16-byte boundary: a view at element offset 1 of a flat allocation"""
    import torch
    assert t.element_size() == 4, t.dtype
    flat = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    assert flat.data_ptr() % 16 == 0
    v = flat[1:].view(t.shape)
    with torch.no_grad():
        v.copy_(t)
    return v.detach().requires_grad_()


def with_sh(case, shs, D):
    """the case with another SH tensor and active degree"""
    return dict(case, g=dict(case["g"], shs=shs), sh_degree=D)


def weights(case, F=0, seed=11):
    """random image weights of a loss: {"color", "depth", "alpha"[, "feat"]} -> float64 arrays"""
    rng = np.random.default_rng(seed)
    H, W = case["H"], case["W"]
    w = dict(color=rng.normal(size=(3, H, W)), depth=rng.normal(size=(1, H, W)), alpha=rng.normal(size=(1, H, W)))
    if F:
        w["feat"] = rng.normal(size=(F, H, W))
    return w


GRADS = ("mean3D", "mean2D", "opacity", "sh", "scale", "rot")
CAM_GRADS = ("view", "proj", "campos", "bg")


def fp64(kind, case, wts, terms=("color",), antialiasing=False, feats=None):
    """The loss sum over `terms` of (image * wts[term]).sum() through one of the fp64 torch references, fed the case's own SH tensor
    ([P, M, 3], any M >= (D+1)^2).  kind: "raster_torch" (oracle/raster_torch.py), "camera_ref", "antialias_ref", "feature_ref" (tests/).
    -> ({image name: float64 array}, {gradient name: float64 array}); gradient names: GRADS, and CAM_GRADS / "features" where the
    reference takes those tensors.  A leaf nothing reached has a zero gradient."""
    import torch
    import antialias_ref
    import camera_ref
    import feature_ref
    from oracle import raster_torch as rt
    from util import oracle_forward
    g, P = case["g"], case["P"]
    T = lambda a: torch.tensor(np.asarray(a, np.float64), requires_grad=True)  # noqa: E731
    o = oracle_forward(case, dtype=np.float64)
    lv = dict(mean3D=T(g["means3D"]), mean2D=T(np.zeros((P, 3))), opacity=T(g["opacities"]), sh=T(g["shs"]), scale=T(g["scales"]),
              rot=T(g["rotations"]))
    head = (o, lv["mean3D"], lv["mean2D"], lv["opacity"])
    ins = dict(shs=lv["sh"], scales=lv["scale"], rotations=lv["rot"])
    img = {}
    if kind == "raster_torch":
        img["color"], img["depth"], _ = rt.render(*head, **ins)
    else:
        lv.update(zip(CAM_GRADS, camera_ref.camera_tensors(o)))
        cam = tuple(lv[k] for k in CAM_GRADS)
        if feats is not None:
            lv["features"] = T(feats)
        if kind == "camera_ref":
            img["color"], img["depth"] = camera_ref.render(*head, *cam, **ins)
        elif kind == "feature_ref":
            img["color"], img["depth"], img["feat"], img["alpha"] = feature_ref.render(*head, *cam, lv["features"], **ins)
        else:
            assert kind == "antialias_ref", kind
            img["color"], img["depth"], img["feat"], img["alpha"] = antialias_ref.render(
                *head, *cam, features=lv.get("features"), antialiasing=antialiasing, **ins)[:4]
    sum((img[k] * torch.tensor(np.asarray(wts[k], np.float64))).sum() for k in terms).backward()
    grads = {k: (t.grad if t.grad is not None else torch.zeros_like(t)).numpy() for k, t in lv.items()}
    return {k: v.detach().numpy() for k, v in img.items() if v is not None}, grads
