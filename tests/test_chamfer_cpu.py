"""csplat.pointcloud.chamfer_distance without a GPU: the CPU composition against float64 autograd, the argument errors, the
definition of max_sq_dist."""
import numpy as np
import pytest
import torch

import util  # noqa: F401
import chamfer_ref as C
import knn_query_ref as R


def _clouds(n, m, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, 3, generator=g), torch.randn(m, 3, generator=g) * 0.9 + 0.1


def _chamfer64(x, y, two_sided, cap):
    """float64 autograd of the definition; the nearest index from float64 distances (the clouds have no near-ties)"""
    x64, y64 = x.detach().double().requires_grad_(), y.detach().double().requires_grad_()

    def one(a, b):
        d2 = ((b[None] - a[:, None]) ** 2).sum(-1)
        m = d2.min(1).values
        if cap is not None:
            m = torch.where(m.detach() <= cap, m, torch.zeros_like(m))
        return m.sum() / a.shape[0]
    loss = one(x64, y64) + (one(y64, x64) if two_sided else 0.0)
    loss.backward()
    return float(loss.detach()), x64.grad, y64.grad


@pytest.mark.parametrize("two_sided", [True, False])
@pytest.mark.parametrize("cap", [None, 0.05])
@pytest.mark.parametrize("n,m", [(1, 1), (7, 1), (300, 200), (1500, 40)])      # 1500: more than one chunk of the composition
def test_cpu_composition_against_float64_autograd(n, m, two_sided, cap):
    from csplat.pointcloud import chamfer_distance
    x, y = _clouds(n, m)
    d2 = R.sq_dists(x.numpy(), y.numpy())
    two = np.sort(d2, 1)[:, :2]
    assert m == 1 or ((two[:, 1] - two[:, 0]) > 64 * C.U * two[:, 1]).all(), "near-ties: choose another seed"
    x.requires_grad_(), y.requires_grad_()
    loss = chamfer_distance(x, y, two_sided=two_sided, max_sq_dist=cap)
    assert loss.dtype == torch.float32 and loss.shape == ()
    loss.backward()
    ref, gx, gy = _chamfer64(x, y, two_sided, cap)
    # the loss: five roundings per squared distance, at most n + m - 1 in the sums, two in the divisions
    assert abs(float(loss) - ref) <= (n + m + 8) * C.U * max(ref, 1e-30) + 1e-45
    # the gradients: per component (k + 8) U sum |t_i| <= (k + 8) U * k * max |t|, k the most terms a sum can have
    k = max(n, m) + 1
    for got, want in ((x.grad, gx), (y.grad, gy)):
        assert float((got.double() - want).abs().max()) <= (k + 8) * C.U * k * max(float(want.abs().max()), 1e-30)


def test_cpu_composition_follows_the_index_rule_and_the_restatement():
    """duplicated points: the gradient goes to the SMALLEST index among equal distances, as knn_query would choose"""
    from csplat.pointcloud import chamfer_distance
    rng = np.random.default_rng(3)
    xq, yp = R.lattice(rng, 400, 8, 4), R.lattice(rng, 300, 8, 4)
    x, y = torch.from_numpy(xq), torch.from_numpy(yp).requires_grad_()
    loss = chamfer_distance(x, y, two_sided=False)
    loss.backward()
    d2, idx = R.knn_query(xq, yp, 1)
    r = C.direction(xq, yp, idx[:, 0], d2[:, 0])
    assert (d2[:, 0] == R.knn_query(xq, yp, 2)[0][:, 1]).mean() > 0.1           # many tied nearest pairs on this lattice
    assert abs(float(loss) - r["loss"]) <= 4 * C.U * r["loss"]                  # (every d2 is exact here)
    assert (np.abs(y.grad.numpy() - r["dp"]) <= r["bound_p"]).all()
    assert not y.grad.numpy()[r["count"] == 0].any()


def test_max_sq_dist_is_inclusive_and_the_divisor_stays():
    from csplat.pointcloud import chamfer_distance
    x = torch.tensor([[0.0, 0, 0], [1.0, 0, 0], [5.0, 0, 0], [9.0, 0, 0]])
    y = torch.tensor([[0.5, 0, 0], [7.0, 0, 0]])            # squared distances 0.25, 0.25, 4, 4
    assert float(chamfer_distance(x, y, two_sided=False)) == (0.25 + 0.25 + 4 + 4) / 4
    assert float(chamfer_distance(x, y, two_sided=False, max_sq_dist=4.0)) == (0.25 + 0.25 + 4 + 4) / 4       # <=
    assert float(chamfer_distance(x, y, two_sided=False, max_sq_dist=3.999)) == 0.5 / 4                       # the divisor stays 4
    assert float(chamfer_distance(x, y, two_sided=False, max_sq_dist=0.0)) == 0.0
    # y -> x: 0.25 and 4; both directions summed
    assert float(chamfer_distance(x, y, two_sided=True, max_sq_dist=0.25)) == 0.5 / 4 + 0.25 / 2
    # a capped pair gets no gradient
    xg = x.clone().requires_grad_()
    chamfer_distance(xg, y, two_sided=False, max_sq_dist=1.0).backward()
    assert xg.grad[2:].abs().sum() == 0 and (xg.grad[:2, 0] == torch.tensor([-0.25, 0.25])).all()


def test_argument_errors_are_value_errors():
    from csplat.pointcloud import chamfer_distance
    ok = torch.zeros(4, 3)
    for x, y in ((torch.zeros(0, 3), ok), (ok, torch.zeros(0, 3)), (torch.zeros(4, 2), ok), (ok, torch.zeros(4)), (ok, torch.zeros(2, 4, 3)),
                 (ok.double(), ok), (ok, ok.double()), (ok.half(), ok.half()), (ok.numpy(), ok), (ok, None), (ok, torch.zeros(4, 3, device="meta"))):
        with pytest.raises(ValueError):
            chamfer_distance(x, y)
    for cap in (-1.0, float("nan")):
        with pytest.raises(ValueError):
            chamfer_distance(ok, ok, max_sq_dist=cap)
    with pytest.raises(TypeError):
        chamfer_distance(ok, ok, False)           # the options are keyword-only
    assert float(chamfer_distance(ok, ok)) == 0.0
