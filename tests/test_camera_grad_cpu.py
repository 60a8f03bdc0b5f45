"""The truth of the camera-gradient GPU tests: tests/camera_ref.py (the fp64 forward with the camera tensors as inputs) is pinned to the
existing torch oracle, satisfies the translation identity, and csplat.camera.perturbed reproduces the repo's camera builder."""
import numpy as np
import pytest

import util  # noqa: F401  (sys.path: the package and oracle/)
from util import make_case, oracle_forward

torch = pytest.importorskip("torch")
import camera_ref  # noqa: E402
from oracle import raster_torch as rt  # noqa: E402

CASES = [
    dict(P=2000, W=128, H=96, seed=7, grid=20, scale_mul=1.0),
    dict(P=3000, W=200, H=136, seed=8, grid=16, scale_mul=2.5),
    dict(P=800, W=64, H=64, seed=9, grid=10, scale_mul=4.0, radius=1.2),
]


def _inputs(case):
    g, P = case["g"], case["P"]
    T = lambda a: torch.tensor(np.asarray(a, np.float64), requires_grad=True)  # noqa: E731
    return dict(means3D=T(g["means3D"]), means2D=T(np.zeros((P, 3))), opacities=T(g["opacities"]), shs=T(g["shs"]), scales=T(g["scales"]),
                rotations=T(g["rotations"]))


def _loss(case, color, depth):
    rng = np.random.default_rng(11)
    dpix = torch.tensor(rng.normal(size=(3, case["H"], case["W"])))
    ddepth = torch.tensor(rng.normal(size=(1, case["H"], case["W"])))
    return (color * dpix).sum() + (depth * ddepth).sum()


@pytest.mark.parametrize("cfg", CASES)
def test_restatement_pinned_to_the_oracle(cfg):
    case = make_case(**cfg)
    o = oracle_forward(case, dtype=np.float64)
    a, b = _inputs(case), _inputs(case)
    c0, d0, _ = rt.render(o, **a, own_termination=False)
    c1, d1 = camera_ref.render(o, b["means3D"], b["means2D"], b["opacities"], *camera_ref.camera_tensors(o, False), shs=b["shs"],
                               scales=b["scales"], rotations=b["rotations"])
    assert float((c0 - c1).detach().abs().max()) <= 1e-12 and float((d0 - d1).detach().abs().max()) <= 1e-12
    _loss(case, c0, d0).backward()
    _loss(case, c1, d1).backward()
    for k in a:
        ga, gb = a[k].grad.numpy(), b[k].grad.numpy()
        assert np.abs(ga - gb).max() <= 1e-10 * max(np.abs(ga).max(), 1.0), k


@pytest.mark.parametrize("cfg", CASES)
def test_translation_identity(cfg):
    """moving the world by delta (means, campos + delta; V' = A V, Pm' = A Pm with A = [[I, 0], [-delta, 1]]) changes nothing:
    sum_i dL/dm_i + dL/dcampos - V[:3,:] dL/dV[3,:] - Pm[:3,:] dL/dPm[3,:] = 0"""
    case = make_case(**cfg)
    o = oracle_forward(case, dtype=np.float64)
    x = _inputs(case)
    V, Pm, campos, bg = camera_ref.camera_tensors(o)
    color, depth = camera_ref.render(o, x["means3D"], x["means2D"], x["opacities"], V, Pm, campos, bg, shs=x["shs"], scales=x["scales"],
                                     rotations=x["rotations"])
    _loss(case, color, depth).backward()
    dm = x["means3D"].grad
    res = dm.sum(0) + campos.grad - V.detach()[:3, :] @ V.grad[3, :] - Pm.detach()[:3, :] @ Pm.grad[3, :]
    assert float(res.abs().max()) <= 1e-10 * float(dm.abs().sum()), res
    assert float(V.grad.abs().max()) > 0 and float(Pm.grad.abs().max()) > 0 and float(bg.grad.abs().max()) > 0


def test_perturbed_camera_matches_the_builder():
    from types import SimpleNamespace
    from csplat import camera, synthetic as syn
    c = syn.make_camera(30.0, 96, 64)
    wv, full, center = syn.camera_matrices(c["R"], c["T"], c["FoVx"], c["FoVy"])
    T = lambda a: torch.tensor(np.asarray(a, np.float32))  # noqa: E731
    cam = SimpleNamespace(world_view_transform=T(wv), full_proj_transform=T(full), camera_center=T(center), image_width=96, tag="kept")
    z = torch.zeros(3, requires_grad=True)
    p = camera.perturbed(cam, z, z)
    for got, want in ((p.world_view_transform, wv), (p.full_proj_transform, full), (p.camera_center, center)):
        got = got.detach().numpy()
        assert np.abs(got - want).max() <= 1e-6 * np.abs(want).max()
    assert p.tag == "kept" and p.image_width == 96
    omega, tau = torch.tensor([0.02, -0.05, 0.03]), torch.tensor([0.1, -0.2, 0.05])
    q = camera.perturbed(cam, omega, tau)
    x = torch.tensor([0.3, -0.2, 0.1, 1.0])
    pv, pv2 = (x @ cam.world_view_transform)[:3], (x @ q.world_view_transform)[:3]
    assert float((pv2 - (camera.rotation(omega) @ pv + tau)).abs().max()) <= 1e-5
    # the camera centre is the point that maps to the view-space origin
    ctr = torch.cat([q.camera_center, torch.ones(1)])
    assert float((ctr @ q.world_view_transform)[:3].abs().max()) <= 1e-5
