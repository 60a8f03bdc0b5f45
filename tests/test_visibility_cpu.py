"""The truth of the visibility GPU tests: tests/visibility_ref.py agrees with feature_ref's fp64 walk on two identities (the alpha image is
the sum of the weights; weight_sum is the features gradient of an all-ones feature image), the library declares and exports the interface,
and bad arguments raise before any launch."""
import os
import re

import numpy as np
import pytest

import util
from util import make_case, oracle_forward

torch = pytest.importorskip("torch")
import feature_ref  # noqa: E402
import visibility_ref  # noqa: E402

CASES = [
    dict(P=2000, W=128, H=96, seed=7, grid=20, scale_mul=1.0),
    dict(P=3000, W=200, H=136, seed=8, grid=16, scale_mul=2.5),
    dict(P=800, W=64, H=64, seed=9, grid=10, scale_mul=4.0, radius=1.2),
]


def _f64(a, rg=False):
    return torch.tensor(np.asarray(a, np.float64), requires_grad=rg)


@pytest.mark.parametrize("cfg", CASES)
def test_restatement_identities(cfg):
    """sum_i weight_sum[i] == sum_pix alpha[pix] (alpha = 1 - T_final = sum_i w_i) and weight_sum == features.grad for features = ones(P, 1)
    and loss = feat.sum(), both against feature_ref.render under fp64 autograd"""
    case = make_case(**cfg)
    g, P = case["g"], case["P"]
    o = oracle_forward(case, dtype=np.float64)
    V, Pm, campos, bg = feature_ref.camera_tensors(o, False)
    f = torch.ones(P, 1, dtype=torch.float64, requires_grad=True)
    _c, _d, feat, alpha = feature_ref.render(o, _f64(g["means3D"]), torch.zeros(P, 3, dtype=torch.float64), _f64(g["opacities"]), V, Pm,
                                             campos, bg, f, shs=_f64(g["shs"]), scales=_f64(g["scales"]), rotations=_f64(g["rotations"]))
    feat.sum().backward()
    ref = visibility_ref.visibility(o, _f64(g["means3D"]), _f64(g["opacities"]), V, Pm, scales=_f64(g["scales"]),
                                    rotations=_f64(g["rotations"]))
    a = alpha.detach().numpy()
    assert abs(ref["weight_sum"].sum() - a.sum()) <= 1e-9 * a.sum()
    assert np.abs(ref["alpha"] - a[0]).max() <= 1e-12
    fg = f.grad.numpy()[:, 0]
    assert np.abs(ref["weight_sum"] - fg).max() <= 1e-12 * max(1.0, np.abs(fg).max())
    # the four outputs hang together
    wm, ws, pc = ref["weight_max"], ref["weight_sum"], ref["pixel_count"]
    assert np.array_equal(wm > 0, pc > 0) and np.array_equal(ws > 0, pc > 0)
    assert np.all(wm <= 0.99 + 1e-12) and np.all(wm <= ws + 1e-15)
    assert np.array_equal(ref["top_ids"] == -1, a[0] == 0)
    hist = np.bincount(ref["top_ids"][ref["top_ids"] >= 0], minlength=P)
    assert np.all(hist <= pc)
    assert np.all(visibility_ref.top_ties(visibility_ref.visibility(o, _f64(g["means3D"]), _f64(g["opacities"]), V, Pm,
                                                                    scales=_f64(g["scales"]), rotations=_f64(g["rotations"]),
                                                                    top_id=ref["top_ids"]), ref["top_ids"]))


def test_restatement_antialiased_alpha():
    """with antialiasing the summed weights are antialias_ref's alpha image"""
    import antialias_ref
    case = make_case(**CASES[2])
    g, P = case["g"], case["P"]
    o = oracle_forward(case, dtype=np.float64)
    V, Pm, campos, bg = antialias_ref.camera_tensors(o, False)
    _c, _d, _f, alpha, _n, _aux = antialias_ref.render(o, _f64(g["means3D"]), torch.zeros(P, 3, dtype=torch.float64), _f64(g["opacities"]),
                                                       V, Pm, campos, bg, shs=_f64(g["shs"]), scales=_f64(g["scales"]),
                                                       rotations=_f64(g["rotations"]))
    ref = visibility_ref.visibility(o, _f64(g["means3D"]), _f64(g["opacities"]), V, Pm, scales=_f64(g["scales"]),
                                    rotations=_f64(g["rotations"]), antialiasing=True)
    assert np.abs(ref["alpha"] - alpha.detach().numpy()[0]).max() <= 1e-12
    assert float(alpha.max()) > 0.5


def test_header_and_exports():
    from csplat import native
    hdr = open(os.path.join(util.ROOT, "include", "csplat.h")).read()
    assert re.search(r"typedef struct csplat_visibility \{", hdr)
    for name in ("csplat_visibility_scratch_bytes", "csplat_visibility_views"):
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
        assert name in native.EXPORTS and hasattr(native.lib, name)
    assert [f[0] for f in native.CsplatVisibility._fields_] == ["weight_max", "weight_sum", "pixel_count", "top_id", "scratch"]
    assert native.PROF_CLASSES[-1] == "visibility"
    assert native.ABI_VERSION == 9 and native.lib.csplat_abi_version() == 9
    sizes = [int(native.lib.csplat_visibility_scratch_bytes(2000, R, 128, 96)) for R in (0, 1, 1000, 50_000, 2_000_000)]
    assert sizes == sorted(sizes) and sizes[-1] > sizes[-2] > sizes[0] and sizes[-1] >= 3 * 4 * 2_000_000


def test_bad_arguments_raise_before_any_launch(monkeypatch):
    """a non-bool flag (TypeError) and a forward launched on faith (RuntimeError) raise before anything reaches the library"""
    import diff_gaussian_rasterization as dgr
    from csplat import native

    class _NoLib:
        def __getattr__(self, name):
            raise AssertionError(f"{name} was called")
    monkeypatch.setattr(native, "lib", _NoLib())
    m = torch.zeros(10, 3)
    rs = dgr.GaussianRasterizationSettings(image_height=16, image_width=16, tanfovx=0.5, tanfovy=0.5, bg=torch.zeros(3), scale_modifier=1.0,
                                           viewmatrix=torch.eye(4), projmatrix=torch.eye(4), sh_degree=0, campos=torch.zeros(3),
                                           prefiltered=False, debug=False)
    kw = dict(means3D=m, means2D=torch.zeros(10, 3), opacities=torch.ones(10, 1), colors_precomp=torch.ones(10, 3),
              scales=torch.ones(10, 3), rotations=torch.ones(10, 4))
    for bad in (1, "yes", None, np.bool_(True), torch.tensor(True)):
        with pytest.raises(TypeError, match="return_visibility"):
            dgr.GaussianRasterizer(rs)(**kw, return_visibility=bad)
        with pytest.raises(TypeError, match="return_visibility"):
            dgr.rasterize_views([rs], [dict(kw, return_visibility=bad)])
    faith = {"caps": (1, 1, 1), "valid": torch.zeros(1, dtype=torch.int32)}
    with dgr.forward_mode(faith=faith):
        with pytest.raises(RuntimeError, match="on faith"):
            dgr.GaussianRasterizer(rs)(**kw, return_visibility=True)
        with pytest.raises(RuntimeError, match="on faith"):
            dgr.rasterize_views([rs, rs], [kw, dict(kw, return_visibility=True)])
    assert dgr.forward_mode_is_default()
