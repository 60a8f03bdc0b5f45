"""csplat.pointcloud.chamfer_distance on the GPU (csplat_knn_query K = 1, csplat_chamfer_fwd, csplat_chamfer_bwd) against the float64
restatement tests/chamfer_ref.py.

The loss is checked on the exact lattices of tests/knn_query_ref.py, where every squared distance and their sum are exact: the result
must lie within 2^-22 relative of the float64 value (the reciprocal or division and the product, 2^-24 each, times two) -- one dropped
term is seen at these sizes.  The gradients are checked given the kernel's own indices (pinned bit for bit by
tests/test_knn_query_gpu.py; the derivative is defined through them), per component: |got - ref| <= (n_j + 8) 2^-24 sum_i |t_i| with
t_i the float64 terms of that sum and n_j their number (chamfer_ref.direction states the derivation).  Rows of the points' gradient
that nobody selected must be exact zeros."""
import numpy as np
import pytest
import torch

import util  # noqa: F401
import chamfer_ref as C
import knn_query_ref as R

pytestmark = pytest.mark.gpu


def gpu(a, grad=False):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda().requires_grad_(grad)


def nearest(a, b):
    """the kernel's own (d2 float32 [Q], idx int64 [Q]) of a -> b, as numpy"""
    import simple_knn
    d2, idx = simple_knn.knn_query(gpu(a), gpu(b), 1)
    return d2[:, 0].cpu().numpy(), idx[:, 0].cpu().numpy()


# ---------------------------------------------------------------------------------------------------------------- the loss
@pytest.mark.parametrize("capped", [False, True])
@pytest.mark.parametrize("span,step", [(64, 16), (8, 4)])
@pytest.mark.parametrize("Q", [1, 255, 256, 257, 4097])
def test_loss_on_the_exact_lattices(Q, span, step, capped):
    from csplat.pointcloud import chamfer_distance
    rng = np.random.default_rng(Q + span)
    a, b = R.lattice(rng, Q, span, step), R.lattice(rng, 1500, span, step)
    d64, _ = R.brute64(a, b, 1)
    d64 = d64[:, 0]
    cap = None
    if capped:
        cap = float(np.sort(d64)[Q // 2])                 # a lattice distance that occurs: the <= edge is hit
        assert (d64 == cap).any() and (Q == 1 or ((d64 > cap).any() and cap > 0))
    ref = float(np.where(d64 <= (np.inf if cap is None else cap), d64, 0.0).sum() / Q)
    got = chamfer_distance(gpu(a), gpu(b), two_sided=False, max_sq_dist=cap)
    assert got.dtype == torch.float32 and got.shape == () and got.is_cuda
    err = abs(float(got) - ref)
    print(f"Q={Q} lattice {span}/{step} cap={cap}: loss {float(got):.9g} ref {ref:.17g} rel err {err / max(ref, 1e-300):.3e} "
          f"(bound {2.0 ** -22:.3e}); one term is at least {d64[d64 > 0].min() / Q / max(ref, 1e-300):.3e} of it")
    assert err <= 2.0 ** -22 * ref
    assert ref > 0 and d64[d64 > 0].min() / Q > 2.0 ** -22 * ref, "the case would not see a dropped term"


def test_two_sided_loss_is_the_sum_of_the_directions():
    from csplat.pointcloud import chamfer_distance
    rng = np.random.default_rng(5)
    a, b = R.lattice(rng, 700, 64, 16), R.lattice(rng, 300, 64, 16)
    ta, tb = gpu(a), gpu(b)
    both = chamfer_distance(ta, tb)
    ab, ba = chamfer_distance(ta, tb, two_sided=False), chamfer_distance(tb, ta, two_sided=False)
    assert float(both) == float(ab + ba)
    ref = R.brute64(a, b, 1)[0].sum() / 700 + R.brute64(b, a, 1)[0].sum() / 300
    assert abs(float(both) - ref) <= 3 * 2.0 ** -22 * ref


# ---------------------------------------------------------------------------------------------------------------- the gradients
def _clouds(kind, seed=0):
    rng = np.random.default_rng(seed)
    if kind == "skewed":          # 20 000 queries onto 300 points: runs of ~67 terms, the longest well above 100
        return rng.normal(size=(20_000, 3)), rng.normal(size=(300, 3)) * np.array([1.0, 0.3, 0.1])
    if kind == "balanced":
        return rng.normal(size=(4097, 3)), rng.normal(size=(4097, 3))
    if kind == "one_point":
        return rng.normal(size=(4097, 3)), rng.normal(size=(1, 3))
    if kind == "lattice":         # index ties: the gradient follows the smaller index
        return R.lattice(rng, 3000, 8, 4), R.lattice(rng, 700, 8, 4)
    raise KeyError(kind)


def _check_direction(name, got_q, got_p, r):
    for what, got, ref, bound in (("dq", got_q, r["dq"], r["bound_q"]), ("dp", got_p, r["dp"], r["bound_p"])):
        if got is None:
            continue
        err = np.abs(got.astype(np.float64) - ref)
        worst = float((err / np.maximum(bound, 1e-300)).max())
        print(f"{name} {what}: largest |got - ref| / bound {worst:.3f}; longest run {int(r['count'].max())}")
        assert (err <= bound).all(), f"{name} {what}: {int((err > bound).sum())} components beyond the bound (worst {worst:.2f} x)"
    if got_p is not None:
        assert r["count"].min() > 0 or not got_p[r["count"] == 0].view(np.uint32).any(), "an unselected row is not exactly zero"


@pytest.mark.parametrize("up", [1.0, 0.37])
@pytest.mark.parametrize("capped", [False, True])
@pytest.mark.parametrize("kind", ["skewed", "balanced", "one_point", "lattice"])
def test_one_sided_gradients_given_the_kernels_indices(kind, capped, up):
    from csplat.pointcloud import chamfer_distance
    a, b = _clouds(kind)
    a, b = a.astype(np.float32), b.astype(np.float32)
    d2, idx = nearest(a, b)
    cap = float(np.sort(d2)[len(d2) // 2]) if capped else None       # one of the float32 distances: the <= edge
    ta, tb = gpu(a, True), gpu(b, True)
    loss = chamfer_distance(ta, tb, two_sided=False, max_sq_dist=cap)
    (loss * up).backward()
    r = C.direction(a, b, idx, d2, cap, g=float(np.float32(up)))
    if kind == "balanced":
        assert (r["count"] == 0).any() and r["count"].max() > 1
    if kind == "skewed":
        assert r["count"].max() > 100
    if capped:
        assert 0 < r["w"].sum() < len(a)
    _check_direction(f"{kind} cap={cap} g={up}", ta.grad.cpu().numpy(), tb.grad.cpu().numpy(), r)


def test_two_sided_gradients_with_both_clouds_requiring_them():
    """x.grad = dq(x -> y) + dp(y -> x): the two bounds add, plus one rounding of the sum of the two parts"""
    from csplat.pointcloud import chamfer_distance
    rng = np.random.default_rng(2)
    x, y = rng.normal(size=(3000, 3)).astype(np.float32), (rng.normal(size=(2000, 3)) * 0.8).astype(np.float32)
    tx, ty = gpu(x, True), gpu(y, True)
    chamfer_distance(tx, ty, two_sided=True, max_sq_dist=0.02).backward()
    rxy = C.direction(x, y, nearest(x, y)[1], nearest(x, y)[0], 0.02)
    ryx = C.direction(y, x, nearest(y, x)[1], nearest(y, x)[0], 0.02)
    for name, got, ref, bound, mag in (("x", tx.grad, rxy["dq"] + ryx["dp"], rxy["bound_q"] + ryx["bound_p"], np.abs(rxy["dq"]) + np.abs(ryx["dp"])),
                                       ("y", ty.grad, ryx["dq"] + rxy["dp"], ryx["bound_q"] + rxy["bound_p"], np.abs(ryx["dq"]) + np.abs(rxy["dp"]))):
        err = np.abs(got.cpu().numpy().astype(np.float64) - ref)
        bound = bound + 2 * C.U * mag
        print(f"two-sided d{name}: largest |got - ref| / bound {float((err / np.maximum(bound, 1e-300)).max()):.3f}")
        assert (err <= bound).all()


@pytest.mark.parametrize("which", ["x", "y"])
def test_only_one_cloud_requires_a_gradient(which):
    from csplat.pointcloud import chamfer_distance
    a, b = _clouds("balanced", seed=4)
    a, b = a[:1000].astype(np.float32), b[:777].astype(np.float32)
    ta, tb = gpu(a, which == "x"), gpu(b, which == "y")
    loss = chamfer_distance(ta, tb, two_sided=False)
    loss.backward()
    d2, idx = nearest(a, b)
    r = C.direction(a, b, idx, d2)
    if which == "x":
        assert tb.grad is None
        _check_direction("only x", ta.grad.cpu().numpy(), None, r)
    else:
        assert ta.grad is None
        _check_direction("only y", None, tb.grad.cpu().numpy(), r)
    # neither: a forward-only value, the same bits
    assert float(chamfer_distance(gpu(a), gpu(b), two_sided=False)) == float(loss)


# ---------------------------------------------------------------------------------------------------------------- reproducibility, capture
def _run(ta, tb):
    from csplat.pointcloud import chamfer_distance
    loss = chamfer_distance(ta, tb, two_sided=True, max_sq_dist=0.5)
    ga, gb = torch.autograd.grad(loss * 0.37, (ta, tb))
    return loss.detach(), ga, gb


def test_two_runs_are_bit_equal():
    a, b = _clouds("skewed", seed=9)
    ta, tb = gpu(a, True), gpu(b, True)
    first, second = _run(ta, tb), _run(ta, tb)
    for x, y in zip(first, second):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))


def test_forward_and_backward_replayed_from_a_graph_equal_eager():
    from csplat import graphs
    a, b = _clouds("skewed", seed=9)
    ta, tb = gpu(a[:6000], True), gpu(b, True)
    eager = _run(ta, tb)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with graphs.capture(graph):
        recorded = _run(ta, tb)
    for r in recorded:
        r.zero_()
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    for e, r in zip(eager, recorded):
        assert torch.equal(e.view(torch.int32), r.view(torch.int32))
    # the backward alone, on a side stream: the same bits
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        on_side = _run(ta, tb)
    side.synchronize()
    for e, s in zip(eager, on_side):
        assert torch.equal(e.view(torch.int32), s.view(torch.int32))
