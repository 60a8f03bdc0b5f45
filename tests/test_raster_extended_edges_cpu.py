"""The yardsticks of tests/test_raster_extended_edges_gpu.py pinned on its new shapes: a tame wild scene (util.wild_case, needles=False),
a ragged image size and a tile list of several segments.  With antialiasing off, tests/antialias_ref.py is camera_ref's and feature_ref's
restatement bit for bit, its own termination is the C oracle's n_contrib and its colour gradients are the fp64 C oracle's backward
(at the bars of tests/test_oracle_cpu.py);
tests/visibility_ref.py keeps the identities of tests/test_visibility_cpu.py.  A GPU failure there then points at a kernel."""
import numpy as np
import pytest

import util
from util import make_case, oracle_forward

torch = pytest.importorskip("torch")
import antialias_ref  # noqa: E402
import camera_ref  # noqa: E402
import feature_ref  # noqa: E402
import visibility_ref  # noqa: E402


def _t(a, grad=False):
    return torch.tensor(np.asarray(a, np.float64), requires_grad=grad)


def _wild():
    return util.wild_case(101, needles=False)


def _ragged():
    return make_case(P=1400, W=97, H=61, seed=3, scale_mul=2.0)


def _segments():
    return make_case(P=2500, W=64, H=48, seed=21, grid=12, scale_mul=6.0, radius=3.0)


CASES = {"wild_tame": _wild, "ragged": _ragged, "segments": _segments}


@pytest.mark.parametrize("name", list(CASES))
def test_cases_are_what_they_claim(name):
    case = CASES[name]()
    o = oracle_forward(case)
    L = o.ranges[:, 1] - o.ranges[:, 0]
    if name == "wild_tame":
        sc = case["g"]["scales"]
        assert (sc.max(1) / sc.min(1)).max() <= 30.0 + 1e-3
        assert case["W"] % 4 != 0 or case["H"] % 4 != 0
    elif name == "ragged":
        assert case["W"] % 4 != 0 and case["H"] % 4 != 0
    else:
        assert int(L.max()) > 4 * 256 and int(o.n_contrib.max()) > 256


@pytest.mark.parametrize("name", list(CASES))
def test_antialias_ref_off_is_the_existing_restatements_and_the_oracle(name):
    case = CASES[name]()
    g, P = case["g"], case["P"]
    o = oracle_forward(case, dtype=np.float64)
    V, Pm, campos, bg = camera_ref.camera_tensors(o, False)
    feats = _t(np.random.default_rng(5).normal(size=(P, 3)))
    args = (_t(g["means3D"]), _t(np.zeros((P, 3))), _t(g["opacities"]), V, Pm, campos, bg)
    kw = dict(shs=_t(g["shs"]), scales=_t(g["scales"]), rotations=_t(g["rotations"]))
    c0, d0 = camera_ref.render(o, *args, **kw)
    fc, fd, ff, fa = feature_ref.render(o, *args, feats, **kw)
    for own in (False, True):
        c, d, f, a, ncon, _aux = antialias_ref.render(o, *args, feats, antialiasing=False, own_termination=own, **kw)
        assert torch.equal(c, c0) and torch.equal(d, d0)
        assert torch.equal(c, fc) and torch.equal(d, fd) and torch.equal(f, ff) and torch.equal(a, fa)
        assert np.array_equal(ncon.numpy(), o.n_contrib.astype(np.int64))
    # colour gradients: the fp64 C oracle's backward
    dpix = np.random.default_rng(11).normal(size=(3, case["H"], case["W"]))
    ins = {k: _t(g[k], True) for k in ("means3D", "opacities", "shs", "scales", "rotations")}
    m2 = _t(np.zeros((P, 3)), True)
    c, *_rest = antialias_ref.render(o, ins["means3D"], m2, ins["opacities"], V, Pm, campos, bg, shs=ins["shs"], scales=ins["scales"],
                                     rotations=ins["rotations"], antialiasing=False)
    (c * torch.tensor(dpix)).sum().backward()
    gr = util.ro.backward(o, dpix)
    # 1e-10, except where the C backward's 1 / (det^2 + 1e-7) guard departs from exact autograd (tests/test_oracle_cpu.py,
    # test_c_backward_equals_autograd: mean3D 1e-6, scale / rot 1e-5; measured here up to 5.5e-9 and 7.6e-10)
    bars = dict(mean2D=(m2, 1e-10), opacity=(ins["opacities"], 1e-10), sh=(ins["shs"], 1e-10), mean3D=(ins["means3D"], 1e-6),
                scale=(ins["scales"], 1e-5), rot=(ins["rotations"], 1e-5))
    for k, (t, bar) in bars.items():
        a = t.grad.numpy().reshape(P, -1)
        b = np.asarray(getattr(gr, k), np.float64).reshape(P, -1)
        assert util.rel_err(a, b) < bar, (name, k, util.rel_err(a, b))


@pytest.mark.parametrize("name", list(CASES))
def test_visibility_ref_identities(name):
    case = CASES[name]()
    g, P = case["g"], case["P"]
    o = oracle_forward(case, dtype=np.float64)
    V, Pm, campos, bg = feature_ref.camera_tensors(o, False)
    f = torch.ones(P, 1, dtype=torch.float64, requires_grad=True)
    _c, _d, feat, alpha = feature_ref.render(o, _t(g["means3D"]), torch.zeros(P, 3, dtype=torch.float64), _t(g["opacities"]), V, Pm,
                                             campos, bg, f, shs=_t(g["shs"]), scales=_t(g["scales"]), rotations=_t(g["rotations"]))
    feat.sum().backward()
    ref = visibility_ref.visibility(o, _t(g["means3D"]), _t(g["opacities"]), V, Pm, scales=_t(g["scales"]), rotations=_t(g["rotations"]))
    a = alpha.detach().numpy()
    assert abs(ref["weight_sum"].sum() - a.sum()) <= 1e-9 * a.sum()
    assert np.abs(ref["alpha"] - a[0]).max() <= 1e-12
    fg = f.grad.numpy()[:, 0]
    assert np.abs(ref["weight_sum"] - fg).max() <= 1e-12 * max(1.0, np.abs(fg).max())
    wm, ws, pc = ref["weight_max"], ref["weight_sum"], ref["pixel_count"]
    assert np.array_equal(wm > 0, pc > 0) and np.array_equal(ws > 0, pc > 0)
    assert np.all(wm <= 0.99 + 1e-12) and np.all(wm <= ws + 1e-15)
    assert np.array_equal(ref["top_ids"] == -1, a[0] == 0)
    assert np.all(np.bincount(ref["top_ids"][ref["top_ids"] >= 0], minlength=P) <= pc)
