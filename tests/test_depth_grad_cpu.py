"""The truth the depth-gradient GPU tests use: autograd of the fp64 torch oracle's depth image (oracle/raster_torch.render) is the
derivative of that image -- central finite differences on a tiny case agree with it."""
import numpy as np
import pytest

import util  # noqa: F401  (sys.path: the package and oracle/)
from util import make_case, oracle_forward

torch = pytest.importorskip("torch")
from oracle import raster_torch as rt  # noqa: E402


def _depth_loss(case, ddepth, means3D, opacities):
    g = dict(case["g"], means3D=means3D, opacities=opacities)
    c = dict(case, g=g)
    o = oracle_forward(c, dtype=np.float64)
    T = lambda a, rg=False: torch.tensor(np.asarray(a, np.float64), requires_grad=rg)  # noqa: E731
    m3, op = T(means3D, True), T(opacities, True)
    _color, dimg, _ = rt.render(o, m3, T(np.zeros((case["P"], 3))), op, shs=T(g["shs"]), scales=T(g["scales"]),
                                rotations=T(g["rotations"]))
    loss = (dimg * torch.tensor(ddepth)).sum()
    return loss, m3, op


def test_oracle_depth_autograd_is_the_derivative():
    case = make_case(P=120, W=32, H=32, seed=3, grid=6, scale_mul=2.0)
    rng = np.random.default_rng(0)
    ddepth = rng.normal(size=(1, 32, 32))
    m0 = np.asarray(case["g"]["means3D"], np.float64)
    o0 = np.asarray(case["g"]["opacities"], np.float64)
    loss, m3, op = _depth_loss(case, ddepth, m0, o0)
    loss.backward()
    gm, go = m3.grad.numpy(), op.grad.numpy()
    assert np.abs(gm).max() > 0 and np.abs(go).max() > 0
    eps = 1e-6
    checked = 0
    for i in np.argsort(-np.abs(gm).max(axis=1))[:6]:
        for k in range(3):
            mp, mm = m0.copy(), m0.copy()
            mp[i, k] += eps
            mm[i, k] -= eps
            fd = (float(_depth_loss(case, ddepth, mp, o0)[0]) - float(_depth_loss(case, ddepth, mm, o0)[0])) / (2 * eps)
            assert abs(fd - gm[i, k]) < 1e-4 * np.abs(gm).max() + 1e-8, (i, k, fd, gm[i, k])
            checked += 1
    for i in np.argsort(-np.abs(go).reshape(-1))[:6]:
        opp, opm = o0.copy(), o0.copy()
        opp.reshape(-1)[i] += eps
        opm.reshape(-1)[i] -= eps
        fd = (float(_depth_loss(case, ddepth, m0, opp)[0]) - float(_depth_loss(case, ddepth, m0, opm)[0])) / (2 * eps)
        assert abs(fd - go.reshape(-1)[i]) < 1e-4 * np.abs(go).max() + 1e-8, (i, fd, go.reshape(-1)[i])
        checked += 1
    assert checked == 24
