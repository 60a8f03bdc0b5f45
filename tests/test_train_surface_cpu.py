"""csplat.train as the way in, without a GPU: the names callers take from it, that they are re-exports of the modules the step's pieces
live in, that the step and its stages resolve what tests replace as globals of csplat.train, and the order in which the optional terms'
refusals are raised when more than one thing is wrong."""
from types import SimpleNamespace

import pytest
import torch

import util  # noqa: F401

# every name bench.py, bench_train.py, tests/ and tools/ take from csplat.train (written out, not computed)
SURFACE = ("train_step", "DEFAULT_OPT", "DEFAULT_PIPE", "CapturedStep", "step_stats",
           "l1_loss", "ssim", "psnr", "image_losses", "FusedImageLoss", "GaussianBlur11", "_L1_SCRATCH", "_IMG_SCRATCH",
           "geometry_losses",
           "regularization", "edge_csr", "simulator_step", "SimulatorStep", "FusedClothRegs", "launch_deferred",
           "_geometry_weights", "_chamfer_weight", "_neighbour_options",
           "render_views", "render", "cd", "_n")

STAGES = ("train_step", "_plan_optional_terms", "_add_optional_terms", "_optional_terms_on", "_refuse_view_parallel",
          "_refuse_camera_by_camera", "_bind_flat_grads", "_deform_all_cameras", "_render_cameras", "_image_term",
          "_exchange_step_results", "_densify_and_step")


def test_every_name_callers_take_from_train_is_there():
    from csplat import train as tr
    missing = [name for name in SURFACE if not hasattr(tr, name)]
    assert not missing, missing
    from csplat.train import l1_loss, step_stats      # noqa: F401  (the benchmark's import)


def test_the_moved_names_are_re_exports_not_copies():
    from csplat import captured_step, cloth_regs, geometry_loss, image_loss, native, train as tr
    assert tr.l1_loss is image_loss.l1_loss and tr.FusedImageLoss is image_loss.FusedImageLoss
    assert tr._L1_SCRATCH is image_loss._L1_SCRATCH and tr._IMG_SCRATCH is image_loss._IMG_SCRATCH
    assert tr.geometry_losses is geometry_loss.geometry_losses
    assert tr.regularization is cloth_regs.regularization and tr.launch_deferred is cloth_regs.launch_deferred
    assert tr._DEFERRED is cloth_regs._DEFERRED          # (train_step clears the queue the nodes append to)
    assert tr.CapturedStep is captured_step.CapturedStep
    assert tr._n is native and image_loss._n is native
    for cache in (image_loss._L1_SCRATCH, image_loss._IMG_SCRATCH, geometry_loss._GEOM_SCRATCH):
        assert any(c is cache for c in native.TICKET_CACHES)


def test_the_step_and_its_stages_resolve_their_globals_in_train(monkeypatch):
    """tests replace tr.render_views, tr.render, tr.geometry_losses and tr.cd.is_dist: what calls them looks them up in csplat.train"""
    from csplat import train as tr
    for name in STAGES:
        fn = getattr(tr, name)
        fn = getattr(fn, "__wrapped__", fn)               # (torch.no_grad() as a decorator)
        assert fn.__globals__ is vars(tr), name
    seen = []

    def sentinel(cams, *a, **kw):
        seen.append(kw)
        return [], None

    monkeypatch.setattr(tr, "render_views", sentinel)
    pkgs, stacked, alphas = tr._render_cameras([object()], None, None, None, None, False, None, want_alpha=False, batched=True)
    assert len(seen) == 1 and seen[0]["by_products"] is False and (pkgs, stacked, alphas) == ([], None, None)


class Untouchable:
    def __getattr__(self, name):
        raise AssertionError(f"the step touched .{name} before it checked its options and cameras")


def _step(cams, opt, **kw):
    from csplat import train as tr
    return tr.train_step(1, cams, Untouchable(), Untouchable(), Untouchable(), opt=opt, **kw)


def _opt(**kw):
    from csplat import train as tr
    return SimpleNamespace(**vars(tr.DEFAULT_OPT), **kw)


def _cam(**kw):
    return SimpleNamespace(image_height=6, image_width=8, mask=None, **kw)


def test_refusals_of_two_terms_at_once_the_earlier_term_wins(monkeypatch):
    """The terms are gone through in the order geometry, Chamfer, kNN regularisers, and EACH term in the order option value (ValueError),
    view-parallel, batched_views=False (NotImplementedError), cameras / Gaussian count (ValueError) -- a term is finished before the next
    one's options are read (so a bad Chamfer value is a ValueError whatever else is wrong with the Chamfer term or a later one, but NOT
    ahead of a refusal of the geometry term).  That order is the contract of _plan_optional_terms."""
    from csplat import train as tr
    depth, pts = torch.zeros(1, 6, 8), torch.zeros(5, 3)
    # a bad Chamfer value: ValueError whatever else is wrong with the Chamfer term or with a LATER term ...
    with pytest.raises(ValueError, match="lambda_chamfer"):
        _step([_cam()], _opt(lambda_chamfer=-1.0, lambda_spring=1.0), batched_views=False)
    # ... and with the geometry term on and in order (its cameras carry their field, the step is batched)
    with pytest.raises(ValueError, match="lambda_chamfer"):
        _step([_cam(depth=depth)], _opt(lambda_depth=0.5, lambda_chamfer=-1.0))
    # but the geometry term comes first with ALL its checks: with it on, batched_views=False is its refusal, and its camera check
    # precedes the Chamfer value too
    with pytest.raises(NotImplementedError, match="depth and silhouette terms need batched_views"):
        _step([_cam(depth=depth)], _opt(lambda_depth=0.5, lambda_chamfer=-1.0), batched_views=False)
    with pytest.raises(ValueError, match="`depth`"):
        _step([_cam()], _opt(lambda_depth=0.5, lambda_chamfer=-1.0))
    # a bad geometry value precedes everything
    with pytest.raises(ValueError, match="lambda_depth"):
        _step([_cam()], _opt(lambda_depth=-0.5, lambda_chamfer=-1.0, lambda_spring=-1.0), batched_views=False)
    # valid options, geometry and Chamfer on, a camera lacking both `depth` and `points`
    both = _opt(lambda_depth=0.5, lambda_chamfer=0.5)
    with pytest.raises(NotImplementedError, match="depth and silhouette terms need batched_views"):
        _step([_cam()], both, batched_views=False)
    with pytest.raises(ValueError, match="`depth`"):
        _step([_cam()], both)
    with pytest.raises(ValueError, match="`points`"):
        _step([_cam(depth=depth)], both)
    monkeypatch.setattr(tr.cd, "is_dist", lambda: True)
    with pytest.raises(NotImplementedError, match="depth and silhouette terms are not part of the view-parallel"):
        _step([_cam()], both, view_parallel=True, batched_views=False)
    with pytest.raises(NotImplementedError, match="Chamfer term is not part of the view-parallel"):
        _step([_cam()], _opt(lambda_chamfer=0.5, lambda_spring=1.0), view_parallel=True, batched_views=False)
    monkeypatch.undo()
    # Chamfer before the kNN regularisers: its refusal, its cameras, then the regularisers' value and refusal
    with pytest.raises(NotImplementedError, match="Chamfer term needs batched_views"):
        _step([_cam()], _opt(lambda_chamfer=0.5, lambda_spring=-1.0), batched_views=False)
    with pytest.raises(ValueError, match="`points`"):
        _step([_cam()], _opt(lambda_chamfer=0.5, lambda_spring=-1.0))
    with pytest.raises(ValueError, match="lambda_spring"):
        _step([_cam(points=pts)], _opt(lambda_chamfer=0.5, lambda_spring=-1.0))
    with pytest.raises(NotImplementedError, match="kNN-graph regularisers need batched_views"):
        _step([_cam()], _opt(lambda_spring=1.0), batched_views=False)
    # all three on and in order: the step goes on to its first use of the model (num_gaussians, which the stand-in refuses)
    with pytest.raises(AssertionError, match="touched .num_gaussians"):
        _step([_cam(depth=depth, points=pts)], _opt(lambda_depth=0.5, lambda_chamfer=0.5, lambda_spring=1.0, k_nearest=5))
    # the one predicate of the captured step: from the options alone
    assert tr._optional_terms_on(_opt()) is False
    for kw in (dict(lambda_depth=0.5), dict(lambda_silhouette=0.5), dict(lambda_chamfer=0.5), dict(lambda_rigidity=0.5)):
        assert tr._optional_terms_on(_opt(**kw)) is True
    with pytest.raises(ValueError, match="lambda_chamfer"):
        tr._optional_terms_on(_opt(lambda_chamfer=-1.0))
