"""The train step's Chamfer term (opt.lambda_chamfer, camera.points) without a GPU: what is refused, in which order, before anything
of the step runs."""
from types import SimpleNamespace

import pytest
import torch

import util  # noqa: F401


class Untouchable:
    def __getattr__(self, name):
        raise AssertionError(f"the step touched .{name} before it checked its cameras")


def _step(cams, opt, **kw):
    from csplat import train as tr
    return tr.train_step(1, cams, Untouchable(), Untouchable(), Untouchable(), opt=opt, **kw)


def _opt(**kw):
    from csplat import train as tr
    return SimpleNamespace(**vars(tr.DEFAULT_OPT), **kw)


def _cam(**kw):
    return SimpleNamespace(image_height=6, image_width=8, mask=None, **kw)


def test_weights_are_read_as_the_geometry_weights_are():
    from csplat import train as tr
    assert tr._chamfer_weight(tr.DEFAULT_OPT) == (0.0, None) and not hasattr(tr.DEFAULT_OPT, "lambda_chamfer")
    assert tr._chamfer_weight(_opt(lambda_chamfer=0.5)) == (0.5, None)
    assert tr._chamfer_weight(_opt(lambda_chamfer=0.5, chamfer_max_dist=0.5)) == (0.5, 0.25)      # a distance: its square is the cap
    assert tr._chamfer_weight(_opt(lambda_chamfer=None)) == (0.0, None)
    for bad in (dict(lambda_chamfer=-0.5), dict(lambda_chamfer=float("nan")), dict(lambda_chamfer=1.0, chamfer_max_dist=-1.0)):
        with pytest.raises(ValueError):
            tr._chamfer_weight(_opt(**bad))


def test_refusals_in_their_order(monkeypatch):
    from csplat import train as tr
    good = torch.zeros(5, 3)
    on = _opt(lambda_chamfer=0.5)
    # 1. a negative weight, whatever else is wrong
    with pytest.raises(ValueError, match="lambda_chamfer"):
        _step([_cam()], _opt(lambda_chamfer=-1.0), batched_views=False)
    with pytest.raises(ValueError, match="chamfer_max_dist"):
        _step([_cam()], _opt(lambda_chamfer=1.0, chamfer_max_dist=-2.0), batched_views=False)
    # 2. the paths that do not carry the term, before the cameras are looked at
    with pytest.raises(NotImplementedError, match="batched_views"):
        _step([_cam()], on, batched_views=False)
    monkeypatch.setattr(tr.cd, "is_dist", lambda: True)
    with pytest.raises(NotImplementedError, match="view-parallel"):
        _step([_cam()], on, view_parallel=True)
    monkeypatch.undo()
    # 3. the cameras, before the simulator or anything else of the step runs
    for cams in ([_cam()],                                              # no points
                 [_cam(points=good), _cam()],                           # the second camera lacks them
                 [_cam(points=torch.zeros(5, 2))], [_cam(points=torch.zeros(5))], [_cam(points=torch.zeros(1, 5, 3))],      # shape
                 [_cam(points=torch.zeros(0, 3))],                      # empty
                 [_cam(points=good.double())], [_cam(points=good.half())],                                                   # dtype
                 [_cam(points=[[0.0, 0.0, 0.0]])]):                     # not a tensor
        with pytest.raises(ValueError, match="points"):
            _step(cams, on)
    # the weight 0 or absent: nothing is asked of the cameras -- the step goes on to its first use of the model
    for opt in (_opt(), _opt(lambda_chamfer=0.0), _opt(lambda_chamfer=None)):
        with pytest.raises(AssertionError, match="the step touched"):
            _step([_cam()], opt)
    # good cameras pass the checks
    with pytest.raises(AssertionError, match="the step touched"):
        _step([_cam(points=good), _cam(points=torch.zeros(9, 3))], on)


def test_a_step_with_the_term_is_not_coverable_by_the_captured_step():
    from csplat import train as tr
    cams = [_cam(FoVx=0.5, FoVy=0.5), _cam(FoVx=0.5, FoVy=0.5)]
    cs = tr.CapturedStep(Untouchable(), Untouchable(), Untouchable(), opt=_opt(lambda_chamfer=0.5))
    assert cs._coverable(cams) is False                       # (decided before the model is looked at)
    cs = tr.CapturedStep(Untouchable(), Untouchable(), Untouchable(), opt=_opt(lambda_chamfer=0.0))
    with pytest.raises(AssertionError, match="touched"):      # the weight 0: the decision passes on to the model, as before
        cs._coverable(cams)
