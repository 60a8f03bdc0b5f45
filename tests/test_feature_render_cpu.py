"""The truth of the feature / alpha GPU tests: tests/feature_ref.py (the fp64 forward with feature channels and the alpha image) is pinned
to the torch oracle, its autograd agrees with finite differences, and the library exports the ABI 9 interface."""
import numpy as np
import pytest

import util  # noqa: F401  (sys.path: the package and oracle/)
from util import make_case, oracle_forward

torch = pytest.importorskip("torch")
import feature_ref  # noqa: E402
from oracle import raster_torch as rt  # noqa: E402

CASES = [
    dict(P=2000, W=128, H=96, seed=7, grid=20, scale_mul=1.0),
    dict(P=3000, W=200, H=136, seed=8, grid=16, scale_mul=2.5),
    dict(P=800, W=64, H=64, seed=9, grid=10, scale_mul=4.0, radius=1.2),
]


def _precomp(case, colors):
    o0 = oracle_forward(case, dtype=np.float64)
    o = oracle_forward(case, dtype=np.float64, shs=None, colors_precomp=colors, scales=None, rotations=None, cov3D_precomp=o0.cov3D)
    return o, o0.cov3D


def _leaf(a):
    return torch.tensor(np.asarray(a, np.float64), requires_grad=True)


@pytest.mark.parametrize("cfg", CASES)
def test_feature_image_of_colours_is_the_colour_image(cfg):
    """features = colors_precomp and bg = 0: the feature image is raster_torch.render's colour; the alpha image is the colour of an
    all-ones render with bg = 0"""
    case = make_case(**cfg)
    P = case["P"]
    colors = np.random.default_rng(5).uniform(0, 1, size=(P, 3))
    o, cov = _precomp(case, colors)
    o._inputs.bg = np.zeros(3)
    V, Pm, campos, bg = feature_ref.camera_tensors(o, False)
    g = case["g"]
    args = (_leaf(g["means3D"]), _leaf(np.zeros((P, 3))), _leaf(g["opacities"]))
    _c, _d, feat, alpha = feature_ref.render(o, *args, V, Pm, campos, bg, torch.tensor(colors), colors_precomp=torch.tensor(colors),
                                             cov3D_precomp=torch.tensor(cov))
    c0, _d0, _ = rt.render(o, *args, colors_precomp=torch.tensor(colors), cov3D_precomp=torch.tensor(cov), own_termination=False)
    assert float((feat - c0).detach().abs().max()) <= 1e-12
    c1, _d1, _ = rt.render(o, *args, colors_precomp=torch.ones(P, 3, dtype=torch.float64), cov3D_precomp=torch.tensor(cov),
                           own_termination=False)
    for ch in range(3):
        assert float((alpha[0] - c1[ch]).detach().abs().max()) <= 1e-12
    assert float(alpha.detach().max()) > 0.5


def test_adjoint_matches_finite_differences():
    """a tiny case (P = 30, 16 x 16): autograd of feat + alpha through features, opacities, means and scales against central differences
    (the lists, sorted ids and n_contrib stay those of the oracle's forward: what the GPU's backward takes as constants too)"""
    case = make_case(P=30, W=16, H=16, seed=3, grid=4, scale_mul=3.0)
    o = oracle_forward(case, dtype=np.float64)
    V, Pm, campos, bg = feature_ref.camera_tensors(o, False)
    g, P = case["g"], case["P"]
    rng = np.random.default_rng(0)
    feats = rng.normal(size=(P, 2))
    dfeat, dalpha = rng.normal(size=(2, 16, 16)), rng.normal(size=(1, 16, 16))
    base = dict(means3D=np.asarray(g["means3D"], np.float64), opacities=np.asarray(g["opacities"], np.float64),
                scales=np.asarray(g["scales"], np.float64), features=feats)

    def loss(x, grad=False):
        t = {k: torch.tensor(v, requires_grad=grad) for k, v in x.items()}
        _c, _d, feat, alpha = feature_ref.render(o, t["means3D"], torch.zeros(P, 3, dtype=torch.float64), t["opacities"], V, Pm, campos,
                                                 bg, t["features"], shs=torch.tensor(np.asarray(g["shs"], np.float64)),
                                                 scales=t["scales"], rotations=torch.tensor(np.asarray(g["rotations"], np.float64)))
        L = (feat * torch.tensor(dfeat)).sum() + (alpha * torch.tensor(dalpha)).sum()
        if grad:
            L.backward()
            return {k: t[k].grad.numpy() for k in t}
        return float(L)

    ga = loss(base, True)
    assert np.abs(ga["features"]).max() > 0 and np.abs(ga["opacities"]).max() > 0
    eps = 1e-6
    for k in base:
        fd = np.zeros_like(base[k])
        for idx in np.ndindex(*base[k].shape):
            xp = {kk: v.copy() for kk, v in base.items()}
            xm = {kk: v.copy() for kk, v in base.items()}
            xp[k][idx] += eps
            xm[k][idx] -= eps
            fd[idx] = (loss(xp) - loss(xm)) / (2 * eps)
        err = np.abs(fd - ga[k]).max() / max(np.abs(ga[k]).max(), 1e-12)
        assert err < 1e-5, (k, err)


def test_abi_version_and_exports():
    from csplat import native
    assert native.ABI_VERSION == 9
    assert native.lib.csplat_abi_version() == 9
    assert hasattr(native.lib, "csplat_backward_feature_scratch_bytes")
    names = [f[0] for f in native.CsplatView._fields_]
    assert names[-7:] == ["features", "n_features", "out_features", "out_alpha", "dL_dfeatures", "dL_dalpha", "dL_dfeat_in"]
    assert native.MAX_FEATURES == 6
    assert {"K6_features", "K7_feature_partials", "K7_feature_bwd", "feature_grads"} <= set(native.PROF_CLASSES)
    # the feature layout holds the camera layout
    for P, R, W, H in ((2000, 50_000, 128, 96), (1, 0, 16, 16)):
        assert native.lib.csplat_backward_feature_scratch_bytes(P, R, W, H) > native.lib.csplat_backward_camera_scratch_bytes(P, R, W, H)


def test_bad_features_raise_before_any_launch():
    import diff_gaussian_rasterization as dgr
    m = torch.zeros(10, 3)
    for bad in (np.zeros((10, 2)), torch.zeros(10, 2, dtype=torch.float64), torch.zeros(9, 2), torch.zeros(10, 0), torch.zeros(10, 7),
                torch.zeros(10)):
        with pytest.raises(ValueError):
            dgr._check_features(bad, m)
    assert dgr._check_features(torch.zeros(10, 6), m) == 6
