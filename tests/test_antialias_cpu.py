"""The truth of the antialiasing GPU tests: tests/antialias_ref.py (the fp64 forward with the opacity compensation of CSPLAT_ANTIALIAS) is
pinned to the existing restatements with antialiasing off, its autograd agrees with finite differences, h has the known answers at both
ends, the closed-form dh the kernels use is autograd's, and the interface rejects what it must."""
import ctypes
import os
from types import SimpleNamespace

import numpy as np
import pytest

import util  # noqa: F401  (sys.path: the package and oracle/)
from util import make_case, oracle_forward

torch = pytest.importorskip("torch")
import antialias_ref  # noqa: E402
import camera_ref  # noqa: E402
import feature_ref  # noqa: E402

CASES = [
    dict(P=2000, W=128, H=96, seed=7, grid=20, scale_mul=1.0),
    dict(P=3000, W=200, H=136, seed=8, grid=16, scale_mul=2.5),
    dict(P=800, W=64, H=64, seed=9, grid=10, scale_mul=4.0, radius=1.2),
]


def _t(a, grad=False):
    return torch.tensor(np.asarray(a, np.float64), requires_grad=grad)


@pytest.mark.parametrize("cfg", CASES)
def test_off_equals_existing_restatements(cfg):
    """antialiasing=False: with the oracle's n_contrib the images are camera_ref's and feature_ref's bit for bit; with the termination
    computed by the restatement itself n_contrib is the oracle's and the images are the same again"""
    case = make_case(**cfg)
    o = oracle_forward(case, dtype=np.float64)
    V, Pm, campos, bg = camera_ref.camera_tensors(o, False)
    g, P = case["g"], case["P"]
    feats = _t(np.random.default_rng(5).normal(size=(P, 3)))
    args = (_t(g["means3D"]), _t(np.zeros((P, 3))), _t(g["opacities"]), V, Pm, campos, bg)
    kw = dict(shs=_t(g["shs"]), scales=_t(g["scales"]), rotations=_t(g["rotations"]))
    c0, d0 = camera_ref.render(o, *args, **kw)
    fc, fd, ff, fa = feature_ref.render(o, *args, feats, **kw)
    for own in (False, True):
        c, d, f, a, ncon, _h = antialias_ref.render(o, *args, feats, antialiasing=False, own_termination=own, **kw)
        assert torch.equal(c, c0) and torch.equal(d, d0)
        assert torch.equal(c, fc) and torch.equal(d, fd) and torch.equal(f, ff) and torch.equal(a, fa)
        assert np.array_equal(ncon.numpy(), o.n_contrib.astype(np.int64))


def test_antialiasing_changes_the_images_of_small_footprints():
    """with antialiasing every opacity shrinks (h <= 1) and sub-pixel Gaussians lose coverage: the alpha image drops where they are"""
    case = make_case(P=2000, W=128, H=96, seed=7, grid=20, scale_mul=0.05)
    o = oracle_forward(case, dtype=np.float64)
    V, Pm, campos, bg = camera_ref.camera_tensors(o, False)
    g, P = case["g"], case["P"]
    args = (_t(g["means3D"]), _t(np.zeros((P, 3))), _t(g["opacities"]), V, Pm, campos, bg)
    kw = dict(shs=_t(g["shs"]), scales=_t(g["scales"]), rotations=_t(g["rotations"]))
    _c0, _d0, _f0, a0, _n0, aux0 = antialias_ref.render(o, *args, antialiasing=False, **kw)
    _c1, _d1, _f1, a1, _n1, aux1 = antialias_ref.render(o, *args, antialiasing=True, **kw)
    h, h1 = aux0["h"], aux1["h"]
    vis = torch.from_numpy(o.radii > 0)
    assert torch.equal(h, h1) and float(h[vis].max()) <= 1.0 and float(h[vis].median()) < 0.5
    assert float((a0 - a1).min()) >= -1e-12 and float((a0 - a1).max()) > 0.1


def test_h_known_answers():
    """a footprint much wider than a pixel: h -> 1; a degenerate one (det0 = 0, a fold seen edge-on) hits the floor: h = 0.005 and h
    takes no covariance gradient; between them the closed form the kernels use (include/csplat.h) is autograd's derivative"""
    a0, b, c0 = _t([1e4, 1.0, 4.0], True), _t([0.0, 1.0, 0.0], True), _t([1e4, 1.0, 1e-8], True)
    h = antialias_ref.aa_factor(a0, b, c0)
    assert abs(float(h[0]) - 1.0) < 5e-5
    assert abs(float(h[1].detach()) - 0.005) < 1e-15 and abs(float(h[2].detach()) - 0.005) < 1e-15      # (det0 = 0; det0 / det1 = 1e-8 / 1.2 < 2.5e-5)
    h.sum().backward()
    for t in (a0, b, c0):
        assert float(t.grad[1]) == 0.0 and float(t.grad[2]) == 0.0
    rng = np.random.default_rng(1)
    x, y = rng.uniform(0.05, 3.0, 50), rng.uniform(0.05, 3.0, 50)
    z = rng.uniform(-0.9, 0.9, 50) * np.sqrt(x * y)
    X, Y, Z = _t(x, True), _t(y, True), _t(z, True)
    hh = antialias_ref.aa_factor(X, Z, Y)
    hh.sum().backward()
    w = 0.3
    det1 = (x + w) * (y + w) - z * z
    f = (x * y - z * z) / det1
    assert np.all(f > 2.5e-5)
    hv = np.sqrt(f)
    dfx, dfy, dfz = w * (y * y + w * y + z * z) / det1 ** 2, w * (x * x + w * x + z * z) / det1 ** 2, -2 * w * z * (x + y + w) / det1 ** 2
    for got, df in ((X.grad, dfx), (Y.grad, dfy), (Z.grad, dfz)):
        assert np.abs(got.numpy() - df / (2 * hv)).max() <= 1e-12 * np.abs(df / (2 * hv)).max() + 1e-15


def _fd_check(o, base, loss, eps=1e-6, pick=None, tol=1e-5):
    ga = loss(base, True)
    for k in base:
        fd = np.zeros_like(base[k])
        idxs = list(np.ndindex(*base[k].shape))
        if pick is not None and len(idxs) > pick:
            idxs = [idxs[j] for j in np.random.default_rng(len(k)).choice(len(idxs), pick, replace=False)]
        for idx in idxs:
            xp = {kk: v.copy() for kk, v in base.items()}
            xm = {kk: v.copy() for kk, v in base.items()}
            xp[k][idx] += eps
            xm[k][idx] -= eps
            fd[idx] = (loss(xp) - loss(xm)) / (2 * eps)
        sel = tuple(np.array(ix) for ix in zip(*idxs))
        err = np.abs(fd[sel] - ga[k][sel]).max() / max(np.abs(ga[k]).max(), 1e-12)
        assert err < tol, (k, err)
    return ga


@pytest.mark.parametrize("mode", ["sh", "precomp"])
def test_adjoint_matches_finite_differences(mode):
    """a tiny case (P = 30, 16 x 16) of footprints near pixel size (h between the floor and 1): autograd of colour + depth + feat + alpha
    through every input -- means3D, means2D, opacities, SH or colours, scales / rotations or cov3D, features and the camera tensors --
    against central differences (the lists and sorted ids stay the oracle's, the termination is the restatement's own)"""
    case = make_case(P=30, W=16, H=16, seed=3, grid=4, scale_mul=6.0)
    g, P = case["g"], case["P"]
    o0 = oracle_forward(case, dtype=np.float64)
    rng = np.random.default_rng(0)
    colors = rng.uniform(0, 1, size=(P, 3))
    o = o0 if mode == "sh" else oracle_forward(case, dtype=np.float64, shs=None, colors_precomp=colors, scales=None, rotations=None,
                                               cov3D_precomp=o0.cov3D)
    V0, Pm0, campos0, bg0 = (t.numpy() for t in camera_ref.camera_tensors(o, False))
    w = {k: rng.normal(size=s) for k, s in (("c", (3, 16, 16)), ("d", (1, 16, 16)), ("f", (2, 16, 16)), ("a", (1, 16, 16)))}
    base = dict(means3D=np.asarray(g["means3D"], np.float64), means2D=np.zeros((P, 3)), opacities=np.asarray(g["opacities"], np.float64),
                features=rng.normal(size=(P, 2)), V=V0.copy(), campos=campos0.copy(), bg=bg0.copy())
    if mode == "sh":
        base.update(shs=np.asarray(g["shs"], np.float64), scales=np.asarray(g["scales"], np.float64),
                    rotations=np.asarray(g["rotations"], np.float64))
    else:
        base.update(colors=colors, cov3D=np.asarray(o0.cov3D, np.float64))

    def loss(x, grad=False):
        t = {k: torch.tensor(v, requires_grad=grad) for k, v in x.items()}
        kw = dict(shs=t["shs"], scales=t["scales"], rotations=t["rotations"]) if mode == "sh" else \
            dict(colors_precomp=t["colors"], cov3D_precomp=t["cov3D"])
        c, d, f, a, _n, _h = antialias_ref.render(o, t["means3D"], t["means2D"], t["opacities"], t["V"], torch.tensor(Pm0), t["campos"],
                                                  t["bg"], t["features"], **kw)
        L = sum((img * torch.tensor(w[k])).sum() for img, k in ((c, "c"), (d, "d"), (f, "f"), (a, "a")))
        if grad:
            L.backward()
            return {k: (t[k].grad.numpy() if t[k].grad is not None else np.zeros_like(x[k])) for k in t}
        return float(L)

    _c, _d, _f, _a, _n, aux = antialias_ref.render(o, *(torch.tensor(base[k]) for k in ("means3D", "means2D", "opacities", "V")),
                                                 torch.tensor(Pm0), torch.tensor(base["campos"]), torch.tensor(base["bg"]),
                                                 **(dict(shs=torch.tensor(base["shs"]), scales=torch.tensor(base["scales"]),
                                                         rotations=torch.tensor(base["rotations"])) if mode == "sh" else
                                                    dict(colors_precomp=torch.tensor(colors), cov3D_precomp=torch.tensor(base["cov3D"]))))
    vis = torch.from_numpy(o.radii > 0)
    h = aux["h"]
    assert float(h[vis].min()) > 0.01 and float(h[vis].max()) < 0.95        # (away from the floor, and h matters)
    ga = _fd_check(o, base, loss, pick=60)
    assert np.abs(ga["opacities"]).max() > 0 and np.abs(ga["features"]).max() > 0


def test_rasterize_views_rejects_mixed_flags():
    import diff_gaussian_rasterization as dgr
    P = 10
    kw = dict(means3D=torch.zeros(P, 3), means2D=torch.zeros(P, 3), opacities=torch.ones(P, 1), shs=torch.zeros(P, 16, 3),
              scales=torch.ones(P, 3), rotations=torch.zeros(P, 4))
    with pytest.raises(ValueError, match="antialiasing"):
        dgr.rasterize_views([None, None], [dict(kw, antialiasing=True), dict(kw)])
    with pytest.raises(ValueError, match="antialiasing"):
        dgr.rasterize_views([None, None], [dict(kw, antialiasing=False), dict(kw, antialiasing=True)])


def test_header_declares_the_bit_and_abi_stays_9():
    from csplat import native
    import diff_gaussian_rasterization as dgr
    hdr = open(os.path.join(util.ROOT, "include", "csplat.h")).read()
    assert "#define CSPLAT_ANTIALIAS 2" in hdr
    assert native.ABI_VERSION == 9 and native.lib.csplat_abi_version() == 9
    assert dgr.CSPLAT_ANTIALIAS == 2
    # the single-view entry point has no backward that could see the bit: it refuses it before touching any device memory
    tk = ctypes.c_int(-1)
    never = native.ALLOC_FN(lambda ctx, chunk, nbytes: None)
    rc = native.lib.csplat_forward_begin(None, 0, 0, 0, None, 16, 16, None, None, None, None, None, 1.0, None, None, None, None, None,
                                         0.5, 0.5, 2, never, None, None, ctypes.byref(tk))
    assert rc != 0 and b"CSPLAT_ANTIALIAS" in native.lib.csplat_last_error()


def test_captured_step_key_holds_the_flag():
    """toggling pipe.antialiasing on the same pipe object gives another graph key (CapturedStep records a new graph)"""
    from csplat.train import CapturedStep
    cs = CapturedStep.__new__(CapturedStep)
    p = torch.zeros(2)
    cs.g = SimpleNamespace(num_gaussians=2, active_sh_degree=3, parameters=lambda: [p])
    cs.sim = SimpleNamespace(parameters=lambda: [p])
    cs.pipe = SimpleNamespace(compute_cov3D_python=False)
    cams = [SimpleNamespace(image_height=8, image_width=8, FoVx=1.0, FoVy=1.0)] * 2
    k0 = cs._key(cams)
    cs.pipe.antialiasing = False
    assert cs._key(cams) == k0
    cs.pipe.antialiasing = True
    assert cs._key(cams) != k0
