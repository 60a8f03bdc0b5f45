"""What tests/test_raster_unstaged_sh_gpu.py leans on, held without a GPU: an SH tensor of M != 16 coefficients (unstaged_sh_ref.short)
and its 16-coefficient twin (unstaged_sh_ref.padded) are THE SAME computation to every oracle -- the C oracle (oracle/raster_ref.c, fp32
and fp64, forward and backward) and the fp64 torch references (oracle/raster_torch.py, tests/camera_ref.py, tests/antialias_ref.py,
tests/feature_ref.py) read the first (D+1)^2 coefficient rows only -- so every output and gradient is equal bit for bit, the SH gradient
in its first M rows; and with M = 25 (nine extra rows of ones) the result is that of the plain 16 coefficients and the gradient of the
extra rows is exactly zero."""
import numpy as np
import pytest

import util
import unstaged_sh_ref as us
from unstaged_sh_ref import PAIRS, padded, short, with_sh
from util import make_case, oracle_forward

torch = pytest.importorskip("torch")

FWD_FIELDS = ("depth", "radii", "xy", "conic_opacity", "rgb", "clamped", "cov3D", "tiles_touched", "keys", "ids", "ranges", "color",
              "out_depth", "final_T", "n_contrib")
BWD_FIELDS = ("mean2D", "conic", "opacity", "color", "mean3D", "cov3D", "scale", "rot")
SMALL = dict(P=300, W=48, H=40, seed=9, grid=8, scale_mul=4.0, radius=1.2)      # the torch references loop over tiles in Python
IDS = ["M%d_D%d" % p for p in PAIRS]


def _same(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, what
    assert a.tobytes() == b.tobytes(), what


def _twin(shs, M):
    """the 16-coefficient tensor short(shs, M) must be indistinguishable from"""
    return padded(shs, M) if M <= 16 else np.ascontiguousarray(shs)


def _mixed(o):
    vis = o.radii > 0
    assert vis.any() and not vis.all(), "the case must hold visible and culled Gaussians"


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["fp32", "fp64"])
@pytest.mark.parametrize("M,D", PAIRS, ids=IDS)
def test_c_oracle_short_equals_its_16_coefficient_twin(M, D, dtype):
    case = make_case(**us.CASES[us.CULLING])
    shs = case["g"]["shs"]
    a = oracle_forward(with_sh(case, short(shs, M), D), dtype=dtype)
    b = oracle_forward(with_sh(case, _twin(shs, M), D), dtype=dtype)
    _mixed(a)
    assert a.M == M and b.M == 16
    for k in FWD_FIELDS:
        _same(getattr(a, k), getattr(b, k), k)
    dpix = np.random.default_rng(3).normal(size=(3, case["H"], case["W"])).astype(np.float32)
    ga, gb = util.ro.backward(a, dpix), util.ro.backward(b, dpix)
    for k in BWD_FIELDS:
        _same(getattr(ga, k), getattr(gb, k), k)
    assert ga.sh.shape == (case["P"], M, 3)
    _same(ga.sh[:, :min(M, 16)], gb.sh[:, :min(M, 16)], "sh")
    n = (D + 1) ** 2
    assert not ga.sh[:, n:].any() and not gb.sh[:, n:].any(), "a coefficient row past (D+1)^2 has a gradient"
    assert not ga.sh[a.radii == 0].any(), "a culled Gaussian has an SH gradient"
    assert ga.sh[:, :n].any()


def test_short_padded_and_off16_are_what_they_say():
    shs = make_case(**SMALL)["g"]["shs"]
    for M, _D in PAIRS:
        s, p = short(shs, M), padded(shs, M)
        assert s.shape == (SMALL["P"], M, 3) and p.shape == (SMALL["P"], 16, 3) and s.flags["C_CONTIGUOUS"] and s.dtype == shs.dtype
        k = min(M, 16)
        assert np.array_equal(s[:, :k], shs[:, :k]) and np.array_equal(p[:, :k], shs[:, :k]) and not p[:, k:].any()
        if M > 16:
            assert (s[:, 16:] == 1.0).all()
    t = torch.tensor(shs)
    u = us.off16(t)
    assert u.data_ptr() % 16 == 4 and u.is_contiguous() and u.is_leaf and u.requires_grad and u.shape == t.shape
    assert torch.equal(u.detach(), t)


def _torch_ref(kind, case, M, D, which, **kw):
    shs = case["g"]["shs"]
    c = with_sh(case, short(shs, M) if which == "short" else _twin(shs, M), D)
    F = 0 if kw.get("feats") is None else kw["feats"].shape[1]
    return us.fp64(kind, c, us.weights(c, F), **kw)


def _features(case, F=2):
    return np.random.default_rng(5).normal(size=(case["P"], F))


TORCH_REFS = {
    "raster_torch": dict(terms=("color", "depth")),
    "camera_ref": dict(terms=("color", "depth")),
    "antialias_ref": dict(terms=("color", "depth", "alpha"), antialiasing=True),
    "feature_ref": dict(terms=("color", "feat", "alpha"), feats=True),
}


@pytest.mark.parametrize("kind", sorted(TORCH_REFS))
@pytest.mark.parametrize("M,D", PAIRS, ids=IDS)
def test_torch_references_short_equals_their_16_coefficient_twin(M, D, kind):
    """(antialias_ref.render, feature_ref.render: they accept [P, M, 3] at all)"""
    case = make_case(**SMALL)
    kw = dict(TORCH_REFS[kind])
    if kw.get("feats"):
        kw["feats"] = _features(case)
    img_a, g_a = _torch_ref(kind, case, M, D, "short", **kw)
    img_b, g_b = _torch_ref(kind, case, M, D, "twin", **kw)
    assert img_a.keys() == img_b.keys() and g_a.keys() == g_b.keys()
    for k in img_a:
        _same(img_a[k], img_b[k], k)
    for k in g_a:
        if k == "sh":
            assert g_a[k].shape == (case["P"], M, 3)
            _same(g_a[k][:, :min(M, 16)], g_b[k][:, :min(M, 16)], k)
            assert not g_a[k][:, (D + 1) ** 2:].any() and g_a[k].any()
        else:
            _same(g_a[k], g_b[k], k)
