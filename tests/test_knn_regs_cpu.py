"""The kNN-graph regularisers (csplat.knn_regs; include/csplat.h: csplat_knn_regs_graph / _fwd / _bwd) without a GPU: the float64
restatement's gradients against central differences (this pins the derivative of the quaternion normalisation), the C-ABI surface and
its argument errors, the CPU composition against the float32 restatement, every refusal of the Python entry points and of the train
step, T = 1, and the reverse lists of a hand-made graph."""
import ctypes as C
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import util
import knn_regs_ref as R


def small_case(N=12, K=3, T=3, seed=0):
    """a random in-range graph without self-loops, random rest lengths and weights, unnormalised quaternions"""
    rng = np.random.default_rng(seed)
    idx = np.stack([rng.choice([j for j in range(N) if j != i], K, replace=False) for i in range(N)]).astype(np.int64)
    d0 = rng.uniform(0.1, 1.0, (N, K)).astype(np.float32)
    w = rng.uniform(0.0, 1.0, (N, K)).astype(np.float32)
    M = rng.normal(size=(T, N, 3)).astype(np.float32)
    Q = (rng.normal(size=(T, N, 4)) * rng.uniform(0.3, 3.0, (T, N, 1))).astype(np.float32)
    return SimpleNamespace(N=N, K=K, T=T, idx=idx, d0=d0, w=w, M=M, Q=Q)


def graph_of(c, device="cpu"):
    from csplat.knn_regs import NeighbourGraph
    return NeighbourGraph.from_indices(torch.from_numpy(c.idx).to(device), torch.from_numpy(c.d0).to(device), torch.from_numpy(c.w).to(device))


@pytest.mark.parametrize("iso_abs", [False, True])
def test_float64_restatement_against_central_differences(iso_abs):
    c = small_case()
    lams = (0.7, 1.3, 2.1)
    assert np.abs(np.linalg.norm(c.Q, axis=-1) - 1).min() > 1e-3, "the quaternions are meant to be unnormalised"
    r = R.evaluate(c.M, c.Q, c.idx, c.d0, c.w, lams, iso_abs)
    idx, d0, w = torch.from_numpy(c.idx), torch.from_numpy(c.d0).double(), torch.from_numpy(c.w).double()

    def value(M, Q):
        p = R.terms(M, Q, idx, d0, w, iso_abs)
        return float((lams[0] * p[0] + lams[1] * p[1]) + lams[2] * p[2])

    h = 1e-6
    for name, base, other, first in (("dM", c.M, c.Q, True), ("dQ", c.Q, c.M, False)):
        x0 = torch.from_numpy(base).double()
        y0 = torch.from_numpy(other).double()
        num = np.zeros(x0.numel())
        for n in range(x0.numel()):
            xp, xm = x0.clone().reshape(-1), x0.clone().reshape(-1)
            xp[n] += h
            xm[n] -= h
            xp, xm = xp.reshape(x0.shape), xm.reshape(x0.shape)
            num[n] = ((value(xp, y0) - value(xm, y0)) if first else (value(y0, xp) - value(y0, xm))) / (2 * h)
        err = R.scale_err(r[name].reshape(-1), num)
        print(f"abs={iso_abs} {name}: autograd against central differences, scaled error {err:.2e}")
        assert np.abs(num).max() > 1e-3 and err <= 1e-7


def test_entry_points_are_exported_declared_and_bound():
    from csplat import native
    names = ("csplat_knn_regs_graph", "csplat_knn_regs_graph_temp_bytes", "csplat_knn_regs_fwd", "csplat_knn_regs_fwd_scratch_bytes",
             "csplat_knn_regs_bwd")
    hdr = open(os.path.join(util.ROOT, "include", "csplat.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = C.CDLL(native.LIB_PATH)
    for name in names:
        assert re.search(r"\b%s\s*\(" % name, code), f"include/csplat.h does not declare {name}"
        assert hasattr(lib, name), f"libcsplat.so does not export {name}"
        assert name in native.EXPORTS, f"csplat.native does not bind {name}"
    assert native.lib.csplat_knn_regs_graph_temp_bytes(100_000, 20) >= 100_000 * 20 * 32
    assert native.lib.csplat_knn_regs_fwd_scratch_bytes() >= 1024 * 24 + 4


def test_null_and_bad_sizes_are_errors_that_name_the_function():
    from csplat import native
    L = native.lib
    one = C.c_void_p(256)           # a non-NULL, 16-byte aligned address: the checks below fail before anything is read or launched
    calls = {
        "csplat_knn_regs_graph": [lambda: L.csplat_knn_regs_graph(None, 10, 3, None, None, 0.0, None, None, None, None, None),
                                  lambda: L.csplat_knn_regs_graph(None, 0, 3, one, None, 0.0, None, None, one, one, one),
                                  lambda: L.csplat_knn_regs_graph(None, 10, 33, one, None, 0.0, None, None, one, one, one),
                                  lambda: L.csplat_knn_regs_graph(None, 10, 0, one, None, 0.0, None, None, one, one, one),
                                  lambda: L.csplat_knn_regs_graph(None, 10, 3, one, one, 1.0, None, None, one, one, one),        # d2 without d0 / w
                                  lambda: L.csplat_knn_regs_graph(None, 10, 3, one, one, -1.0, one, one, one, one, one),
                                  lambda: L.csplat_knn_regs_graph(None, 10, 3, one, one, float("nan"), one, one, one, one, one)],
        "csplat_knn_regs_fwd": [lambda: L.csplat_knn_regs_fwd(None, 3, 10, 3, None, None, None, None, None, 1.0, 1.0, 0.0, 0, None, None),
                                lambda: L.csplat_knn_regs_fwd(None, 0, 10, 3, one, None, one, one, one, 1.0, 1.0, 0.0, 0, one, one),
                                lambda: L.csplat_knn_regs_fwd(None, 3, -1, 3, one, None, one, one, one, 1.0, 1.0, 0.0, 0, one, one),
                                lambda: L.csplat_knn_regs_fwd(None, 3, 10, 33, one, None, one, one, one, 1.0, 1.0, 0.0, 0, one, one),
                                lambda: L.csplat_knn_regs_fwd(None, 3, 10, 3, one, None, one, one, one, -1.0, 1.0, 0.0, 0, one, one),
                                lambda: L.csplat_knn_regs_fwd(None, 3, 10, 3, one, None, one, one, one, 1.0, float("nan"), 0.0, 0, one, one),
                                lambda: L.csplat_knn_regs_fwd(None, 3, 1 << 30, 4, one, None, one, one, one, 1.0, 1.0, 0.0, 0, one, one)],
        "csplat_knn_regs_bwd": [lambda: L.csplat_knn_regs_bwd(None, 3, 10, 3, None, None, None, None, None, None, None, 1.0, 1.0, 0.0, 0, None, None, None),
                                lambda: L.csplat_knn_regs_bwd(None, 0, 10, 3, one, None, one, one, one, one, one, 1.0, 1.0, 0.0, 0, one, one, None),
                                lambda: L.csplat_knn_regs_bwd(None, 3, 10, 0, one, None, one, one, one, one, one, 1.0, 1.0, 0.0, 0, one, one, None),
                                lambda: L.csplat_knn_regs_bwd(None, 3, 10, 3, one, None, one, one, one, one, one, 1.0, 1.0, 0.0, 0, one, None, None),   # no output
                                lambda: L.csplat_knn_regs_bwd(None, 3, 10, 3, one, None, one, one, one, one, one, 1.0, 1.0, 0.5, 0, one, one, None),    # rigidity without rotations
                                lambda: L.csplat_knn_regs_bwd(None, 3, 10, 3, one, None, one, one, one, one, one, 1.0, -1.0, 0.0, 0, one, one, None)],
    }
    for name, bad in calls.items():
        for n, call in enumerate(bad):
            assert call() != 0, f"{name}: bad call {n} was accepted"
            assert name.encode() in L.csplat_last_error(), f"{name}: bad call {n}: {L.csplat_last_error()!r}"


@pytest.mark.parametrize("iso_abs", [False, True])
@pytest.mark.parametrize("with_q", [True, False])
def test_cpu_path_equals_the_float32_restatement(with_q, iso_abs):
    from csplat.knn_regs import neighbour_regularization
    c = small_case(N=40, K=5, T=4, seed=1)
    lams = (0.7, 1.3, 2.1 if with_q else 0.0)
    M = torch.from_numpy(c.M).requires_grad_()
    Q = torch.from_numpy(c.Q).requires_grad_() if with_q else None
    loss, parts = neighbour_regularization(M, Q, graph_of(c), *lams, isometric_abs=iso_abs)
    assert loss.dtype == torch.float32 and loss.shape == () and parts.shape == (3,) and not parts.requires_grad
    (loss * 0.37).backward()
    r32 = R.evaluate(c.M, c.Q if with_q else None, c.idx, c.d0, c.w, lams, iso_abs, up=float(np.float32(0.37)), dtype=torch.float32)
    r64 = R.evaluate(c.M, c.Q if with_q else None, c.idx, c.d0, c.w, lams, iso_abs, up=float(np.float32(0.37)))
    # the same operations in the same order: the forward is the float32 restatement's to a rounding of the sums, the gradients to the
    # roundings of another order of the same products
    assert abs(float(loss.detach()) - r32["loss"]) <= 4 * R.U * abs(r64["loss"])
    assert np.abs(parts.numpy() - r32["parts"]).max() <= 4 * R.U * np.abs(r64["parts"]).max()
    assert R.scale_err(M.grad.numpy(), r32["dM"]) <= 4 * R.scale_err(r32["dM"], r64["dM"]) + 4 * R.U
    if with_q:
        assert R.scale_err(Q.grad.numpy(), r32["dQ"]) <= 4 * R.scale_err(r32["dQ"], r64["dQ"]) + 4 * R.U
        assert np.abs(r64["dQ"]).max() > 0


def test_one_time_row_has_no_spring_no_rigidity_and_no_rotation_gradient():
    from csplat.knn_regs import neighbour_regularization
    c = small_case(T=1)
    M, Q = torch.from_numpy(c.M).requires_grad_(), torch.from_numpy(c.Q).requires_grad_()
    loss, parts = neighbour_regularization(M, Q, graph_of(c), 0.5, 2.0, 3.0)
    loss.backward()
    assert float(parts[1]) == 0.0 and float(parts[2]) == 0.0 and float(loss) == 0.5 * float(parts[0])
    assert Q.grad is None or not Q.grad.any()
    assert M.grad.abs().max() > 0
    r = R.evaluate(c.M, c.Q, c.idx, c.d0, c.w, (0.5, 2.0, 3.0))
    assert r["parts"][1] == 0.0 and r["parts"][2] == 0.0 and not r["dQ"].any()


def test_reverse_lists_of_a_hand_made_graph():
    from csplat.knn_regs import NeighbourGraph
    idx = torch.tensor([[1, 2], [0, 0], [0, 1], [2, 2], [4, 0]])            # node 3 is named by nobody; a self-loop; a repeated neighbour
    ones = torch.ones(5, 2)
    g = NeighbourGraph.from_indices(idx, ones, ones * 0.5)
    assert (g.N, g.K) == (5, 2) and g.idx.dtype == torch.int64 and torch.equal(g.idx, idx)
    assert g.rev_offsets.tolist() == [0, 4, 6, 9, 9, 10]
    assert g.rev_entries.tolist() == [2, 3, 4, 9, 0, 5, 1, 6, 7, 8]
    flat = idx.numpy().reshape(-1)
    assert np.array_equal(g.rev_entries.numpy(), np.argsort(flat, kind="stable"))
    assert np.array_equal(g.rev_offsets.numpy(), np.concatenate([[0], np.cumsum(np.bincount(flat, minlength=5))]))
    off, ent = R.reverse_lists(idx.numpy(), 5)
    assert np.array_equal(off, g.rev_offsets.numpy()) and np.array_equal(ent, g.rev_entries.numpy())
    # int32 indices are taken too
    g32 = NeighbourGraph.from_indices(idx.to(torch.int32), ones, ones)
    assert torch.equal(g32.rev_entries, g.rev_entries) and g32.idx.dtype == torch.int64


def test_value_errors_of_the_python_entry_points():
    from csplat.knn_regs import NeighbourGraph, neighbour_regularization
    c = small_case()
    g = graph_of(c)
    M, Q = torch.from_numpy(c.M), torch.from_numpy(c.Q)
    bad_calls = [
        dict(means=M[0]), dict(means=M[..., :2]), dict(means=M.double()), dict(means=M.numpy()), dict(means=M[:0]),         # shape, dtype, T < 1
        dict(means=M[:, :5]),                                                                                                  # N != graph.N
        dict(means=M.to("meta")),                                                                                              # device
        dict(rotations=Q[..., :3]), dict(rotations=Q[:2]), dict(rotations=Q.double()), dict(rotations=Q.to("meta")), dict(rotations=Q.numpy()),
        dict(lams=(-1.0, 0.0, 0.0)), dict(lams=(0.0, float("nan"), 0.0)), dict(lams=(0.0, 0.0, -0.5)), dict(lams=(float("inf"), 0.0, 0.0)),
        dict(rotations=None, lams=(1.0, 1.0, 0.5)),                                                                           # rigidity without rotations
        dict(graph="graph"),
    ]
    for kw in bad_calls:
        a = dict(means=M, rotations=Q, graph=g, lams=(1.0, 1.0, 1.0))
        a.update(kw)
        with pytest.raises(ValueError):
            neighbour_regularization(a["means"], a["rotations"], a["graph"], *a["lams"])
    with pytest.raises(TypeError):
        neighbour_regularization(M, Q, g, 1.0, 1.0, 1.0, True)            # isometric_abs is keyword-only
    neighbour_regularization(M, None, g, 1.0, 1.0, 0.0)                   # rotations None with lambda_rigidity = 0 is fine
    # from_indices: range, shapes, dtypes
    ones = torch.ones(4, 2)
    ok = torch.tensor([[1, 2], [0, 2], [0, 1], [0, 1]])
    for idx, d0, w in ((ok + 3, ones, ones), (ok - 2, ones, ones), (ok.float(), ones, ones), (ok[:, 0], ones[:, 0], ones[:, 0]),
                       (ok, ones.double(), ones), (ok, ones, ones[:3]), (ok, ones, None), (torch.zeros(4, 33, dtype=torch.long),) + (torch.ones(4, 33),) * 2,
                       (torch.zeros(0, 2, dtype=torch.long),) + (torch.ones(0, 2),) * 2):
        with pytest.raises(ValueError):
            NeighbourGraph.from_indices(idx, d0, w)
    # from_points: N <= k, k outside 1 .. 32, shape, dtype, lambda_w -- all before the device is asked for
    for pts, k, lw in ((torch.zeros(5, 3), 5, 1.0), (torch.zeros(5, 3), 7, 1.0), (torch.zeros(50, 3), 0, 1.0), (torch.zeros(50, 3), 33, 1.0),
                       (torch.zeros(50, 2), 3, 1.0), (torch.zeros(50, 3).double(), 3, 1.0), (torch.zeros(50, 3), 3, -1.0),
                       (torch.zeros(50, 3), 3, float("nan"))):
        with pytest.raises(ValueError):
            NeighbourGraph.from_points(pts, k, lw)


# ---------------------------------------------------------------------------------------------------------------- the train step
class Untouchable:
    def __getattr__(self, name):
        raise AssertionError(f"the step touched .{name} before it checked its options")


def _step(cams, opt, gaussians=None, iteration=1, **kw):
    from csplat import train as tr
    return tr.train_step(iteration, cams, gaussians or Untouchable(), Untouchable(), Untouchable(), opt=opt, **kw)


def _opt(**kw):
    from csplat import train as tr
    return SimpleNamespace(**vars(tr.DEFAULT_OPT), **kw)


def _cam(**kw):
    return SimpleNamespace(image_height=6, image_width=8, mask=None, **kw)


class Counted:
    """a Gaussians stand-in that answers num_gaussians and nothing else"""

    def __init__(self, n):
        self.__dict__["num_gaussians"] = n

    def __getattr__(self, name):
        raise AssertionError(f"the step touched .{name} before it checked its options")


def test_train_step_options_are_read_with_their_defaults():
    from csplat import train as tr
    assert tr._neighbour_options(tr.DEFAULT_OPT) == dict(lams=(0.0, 0.0, 0.0), on=False)
    assert tr._neighbour_options(tr.DEFAULT_OPT, 1) is None
    for name in ("lambda_isometric", "lambda_spring", "lambda_rigidity", "lambda_w", "k_nearest", "knn_update_iter", "reg_iter", "isometric_abs"):
        assert not hasattr(tr.DEFAULT_OPT, name)
    o = tr._neighbour_options(_opt(lambda_spring=0.5), 1)
    assert o == dict(lams=(0.0, 0.5, 0.0), on=True, lambda_w=2000.0, k=20, update=1000, reg_iter=0, iso_abs=False)
    o = tr._neighbour_options(_opt(lambda_isometric=1.0, lambda_rigidity=2.0, lambda_w=100000, k_nearest=5, knn_update_iter=7, reg_iter=5000,
                                   isometric_abs=True), 5001)
    assert o == dict(lams=(1.0, 0.0, 2.0), on=True, lambda_w=100000.0, k=5, update=7, reg_iter=5000, iso_abs=True)
    # iteration <= reg_iter, or a static step: the term is off
    assert tr._neighbour_options(_opt(lambda_spring=0.5, reg_iter=5000), 5000) is None
    assert tr._neighbour_options(_opt(lambda_spring=0.5), 1, static=True) is None
    assert tr._neighbour_options(_opt(lambda_spring=None, lambda_isometric=0.0), 1) is None


def test_train_step_refusals_in_their_order(monkeypatch):
    from csplat import train as tr
    on = _opt(lambda_isometric=0.5, k_nearest=5)
    # 1. a bad option value, whatever else is wrong
    for bad in (dict(lambda_isometric=-1.0), dict(lambda_spring=float("nan")), dict(lambda_rigidity=-0.1), dict(lambda_spring=1.0, lambda_w=-1.0),
                dict(lambda_spring=1.0, k_nearest=0), dict(lambda_spring=1.0, k_nearest=33), dict(lambda_spring=1.0, k_nearest=2.5),
                dict(lambda_spring=1.0, knn_update_iter=0), dict(lambda_spring=1.0, reg_iter=-1)):
        with pytest.raises(ValueError):
            _step([_cam()], _opt(**bad), batched_views=False)
    # 2. the paths that do not carry the term, before anything of the model is looked at
    with pytest.raises(NotImplementedError, match="batched_views"):
        _step([_cam()], on, batched_views=False)
    monkeypatch.setattr(tr.cd, "is_dist", lambda: True)
    with pytest.raises(NotImplementedError, match="view-parallel"):
        _step([_cam()], on, view_parallel=True)
    monkeypatch.undo()
    # 3. too few Gaussians for the graph, before the simulator runs
    with pytest.raises(ValueError, match="k_nearest"):
        _step([_cam()], on, gaussians=Counted(5))
    with pytest.raises(ValueError, match="k_nearest"):
        _step([_cam()], _opt(lambda_rigidity=1.0), gaussians=Counted(20))        # the default k_nearest = 20
    # enough of them: the step goes on to its first use of the model
    with pytest.raises(AssertionError, match="the step touched"):
        _step([_cam()], on, gaussians=Counted(6))
    # weights 0 or absent, iteration <= reg_iter: the term is off and too few Gaussians are nobody's concern (a static step:
    # test_train_step_options_are_read_with_their_defaults)
    for opt, kw in ((_opt(), {}), (_opt(lambda_isometric=0.0, lambda_spring=0.0, lambda_rigidity=0.0, k_nearest=5), {}),
                    (_opt(lambda_spring=1.0, reg_iter=10), dict(iteration=10))):
        with pytest.raises(AssertionError, match="the step touched"):
            _step([_cam()], opt, gaussians=Counted(3), **kw)


def test_a_step_with_the_term_is_not_coverable_by_the_captured_step():
    from csplat import train as tr
    cams = [_cam(FoVx=0.5, FoVy=0.5), _cam(FoVx=0.5, FoVy=0.5)]
    for name in ("lambda_isometric", "lambda_spring", "lambda_rigidity"):
        cs = tr.CapturedStep(Untouchable(), Untouchable(), Untouchable(), opt=_opt(**{name: 0.5}))
        assert cs._coverable(cams) is False                   # (decided before the model is looked at)
    cs = tr.CapturedStep(Untouchable(), Untouchable(), Untouchable(), opt=_opt(lambda_spring=0.0))
    with pytest.raises(AssertionError, match="touched"):      # the weights 0: the decision passes on to the model, as before
        cs._coverable(cams)
    assert "lambda_isometric" in tr.CapturedStep.__doc__ and "lambda_isometric" in tr.train_step.__doc__
