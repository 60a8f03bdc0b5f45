"""The train step's Chamfer term on the GPU (opt.lambda_chamfer, camera.points): the small scene of the geometry-step tests
(tests/test_geometry_loss_gpu.py: bench_train's scene, P = 2000, 64 x 64, three cameras), each camera with an observed cloud of a few
hundred points of its own size.

Bars.  Step comparisons that must not differ at all run in the bit-reproducible K7 mode and are compared for equality.  The loss with
the term on against the loss without it plus the float64 term: 16 x 2^-24 of (|loss| + lambda mean) -- five roundings in every float32
squared distance, two in a direction's mean, two in the mean over cameras, one each in the product with lambda, the sum with the
regularisers and the sum with the image loss, rounded up to a power of two.  Gradients: the rule of tests/test_train_kernels_gpu.py
(its check() is used), as the geometry-step test does: 8 x the error of the same restatement in float32, floor 1e-6, relative to the
larger of max |ref| and a unit that does not vanish -- for the difference of two steps' gradients that unit is the largest gradient of
the step without the term, whose rounding the difference carries."""
from types import SimpleNamespace

import numpy as np
import pytest

import util  # noqa: F401
import chamfer_ref as C
from test_geometry_loss_gpu import TIMES, _assert_same_bits, _opt, _scene, _three_steps
from test_train_kernels_gpu import TABLE, check

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
F64, F32 = torch.float64, torch.float32
SIZES = (300, 411, 257)


@pytest.fixture(scope="module", autouse=True)
def _table():
    yield
    print("\ngroup | comparisons | largest e32 | largest bar | largest kernel error | smallest bar / error")
    for g in sorted(k for k in TABLE if k.startswith("train_step chamfer")):
        n, e32, bar, err, margin = TABLE[g]
        print(f"{g} | {n} | {e32:.2e} | {bar:.2e} | {err:.2e} | {margin:.1f}")


def _observed(s):
    """three observed clouds: a sample of each camera's deformed Gaussian centres, moved by ~2 % of the cloth's size"""
    from csplat import train as tr
    from gaussian_renderer import render_views
    gen = torch.Generator().manual_seed(11)
    with torch.no_grad():
        res = render_views(s.plain, s.pc, s.sim, tr.DEFAULT_PIPE, s.bg)
        out = []
        for r, n in zip(res, SIZES):
            m = r.means3D_deform.detach().cpu()
            pick = torch.randperm(m.shape[0], generator=gen)[:n]
            out.append((m[pick] + 0.02 * torch.randn(n, 3, generator=gen) + torch.tensor([0.0, 0.0, 0.03])).cuda().contiguous())
    return out


def _with_points(s):
    if not hasattr(s, "cloud_cams"):
        s.cloud_cams = [SimpleNamespace(**vars(c), points=p) for c, p in zip(s.plain, _observed(s))]
    return s.cloud_cams


def test_train_step_unchanged_when_the_weight_is_zero_or_absent():
    plain = _three_steps(lambda s: s.plain, None)
    absent = _three_steps(_with_points, None)
    zero = _three_steps(_with_points, _opt(lambda_chamfer=0.0, chamfer_max_dist=0.1))
    assert plain["log"][0][2] == ["allreduce_ms", "radii", "viewspace_grad", "visibility_filter"]
    _assert_same_bits(plain, absent)
    _assert_same_bits(plain, zero)


def test_captured_step_with_the_term_runs_eagerly():
    opt = _opt(lambda_chamfer=0.7)
    eager = _three_steps(_with_points, opt, steps=2)
    cap = _three_steps(_with_points, opt, captured=True, steps=2)
    assert cap["cs"] is not None and cap["cs"].stats["eager"] == 2 and cap["cs"].stats["recorded"] == 0 and cap["cs"].stats["replayed"] == 0
    assert "chamfer_loss" in eager["log"][0][2]
    _assert_same_bits(eager, cap)


def _one_step(opt, monkeypatch):
    """step 1 on a fresh scene in the bit-reproducible mode -> what the step saw and produced: loss, stats, every camera's
    means3D_deform, every parameter's gradient (taken when the optimizers are asked to step), the parameters BEFORE the step"""
    import gaussian_renderer
    from csplat import native, train as tr
    native.lib.csplat_debug_flags(256)
    try:
        s = _scene()
        cams = _with_points(s)
        names = ["face_bary", "face_offset", "f_dc", "f_rest", "opacity", "scaling", "rotation"] + [f"sim.{n}" for n, _ in s.sim.named_parameters()]
        params = list(s.pc.parameters()) + list(s.sim.parameters())
        before = {n: p.detach().clone() for n, p in zip(names, params)}
        seen = {"grads": {}}
        inner = tr.render_views

        def spy(*a, **kw):
            out = inner(*a, **kw)
            seen["means"] = [r.means3D_deform.detach().clone() for r in out[0]]
            return out

        monkeypatch.setattr(tr, "render_views", spy)
        for o in (s.pc.optimizer, s.mopt):
            orig = getattr(o, "step_now", o.step)

            def snap(orig=orig):
                for n, p in zip(names, params):
                    if p.grad is not None and n not in seen["grads"]:
                        seen["grads"][n] = p.grad.detach().clone()
                return orig()
            o.step_now = snap
        _ps, loss, stats = tr.train_step(1, cams, s.pc, s.sim, s.mopt, opt=opt, background=s.bg)
        torch.cuda.synchronize()
        monkeypatch.setattr(tr, "render_views", inner)
        return SimpleNamespace(s=s, cams=cams, loss=loss, stats=stats, means=seen["means"], grads=seen["grads"], before=before)
    finally:
        native.lib.csplat_debug_flags(0)


def _term(run, lam, cap_sq, idx, dtype):
    """lambda * mean over the cameras of the one-sided Chamfer distance observed cloud -> Gaussian centres, for the GIVEN nearest indices,
    from the parameters before the step in `dtype` on the CPU: the simulator's MLP restated from its weights, the centres through
    MeshGaussians.get_xyz's formula.  -> (value, {parameter name: gradient})"""
    s, b = run.s, run.before
    leaf = lambda t: t.detach().cpu().to(dtype).clone().requires_grad_()  # noqa: E731
    _tt, enc, base = s.sim.times_on_device(TIMES)
    enc, base = enc.detach().cpu().to(dtype), base.detach().cpu().to(dtype)
    w = {n: leaf(b[n]) for n in b if n.startswith("sim.")}
    bary = leaf(b["face_bary"])
    h = torch.relu(enc @ w["sim.input.weight"].T + w["sim.input.bias"])
    h = torch.relu(h @ w["sim.hidden.weight"].T + w["sim.hidden.bias"])
    verts = base + (h @ w["sim.output.weight"].T + w["sim.output.bias"]).reshape(len(TIMES), -1, 3)
    vid = s.pc._vertex_ids().cpu()
    nb = bary / bary.sum(dim=1, keepdim=True)
    total = 0.0
    for c, cam in enumerate(run.cams):
        xyz = (nb.unsqueeze(-1) * verts[c][vid, :]).sum(dim=1)
        pts = cam.points.detach().cpu().to(dtype)
        d = xyz[idx[c]] - pts
        d2 = (d * d).sum(1)
        if cap_sq is not None:
            d2 = torch.where(d2.detach() <= cap_sq, d2, torch.zeros_like(d2))
        total = total + d2.sum() / pts.shape[0]
    value = lam * total / len(run.cams)
    leaves = dict(face_bary=bary, **w)
    grads = torch.autograd.grad(value, list(leaves.values()))
    return float(value.detach()), dict(zip(leaves, grads))


@pytest.mark.parametrize("max_dist", [None, 0.05])
def test_loss_and_gradients_with_the_term_on(monkeypatch, max_dist):
    import simple_knn
    lam = 0.7
    kw = {} if max_dist is None else dict(chamfer_max_dist=max_dist)
    cap_sq = None if max_dist is None else float(max_dist) ** 2
    off = _one_step(_opt(), monkeypatch)
    on = _one_step(_opt(lambda_chamfer=lam, **kw), monkeypatch)
    assert "chamfer_loss" not in off.stats and sorted(set(on.stats) - set(off.stats)) == ["chamfer_loss"]
    cl = on.stats["chamfer_loss"]
    assert cl.is_cuda and not cl.requires_grad and cl.shape == () and cl.dtype == F32
    # the same scene, the same forward: the centres the two steps rendered are the same bits
    assert all(torch.equal(a, b) for a, b in zip(on.means, off.means))
    # ---- the loss: the step's loss without the term + lambda * mean Chamfer, recomputed in float64 from the centres the step rendered
    idx, per_cam = [], []
    for cam, m in zip(on.cams, on.means):
        d2, i = simple_knn.knn_query(cam.points, m, 1)
        r = C.direction(cam.points.cpu().numpy(), m.cpu().numpy(), i[:, 0].cpu().numpy(), d2[:, 0].cpu().numpy(), cap_sq)
        idx.append(i[:, 0].cpu())
        per_cam.append(r["loss"])
        if cap_sq is not None:
            assert 0 < r["w"].sum() < len(r["w"]), "the cap should cut some of the pairs, not all"
    mean64 = float(np.mean(per_cam))
    tol = 16 * 2.0 ** -24
    print(f"chamfer_loss {float(cl):.9g} (float64 {mean64:.17g}); loss off {float(off.loss):.9g} on {float(on.loss):.9g}, "
          f"off + lambda mean {float(off.loss) + lam * mean64:.17g}")
    assert abs(float(cl) - mean64) <= tol * mean64
    assert abs(float(on.loss) - (float(off.loss) + lam * mean64)) <= tol * (abs(float(off.loss)) + lam * mean64)
    assert lam * mean64 > 100 * tol * abs(float(off.loss)), "the term would not be seen in the loss"
    # ---- the gradients: only the mesh transform's positions and the simulator receive more; everything else is the same bits
    v64, g64 = _term(on, lam, cap_sq, idx, F64)
    v32, g32 = _term(on, lam, cap_sq, idx, F32)
    # (the restatement reaches the centres the step rendered: they are float32, 2^-24 |x| off, which moves a squared distance by 2 d 2^-24 |x|)
    assert abs(v64 - lam * mean64) <= 1e-4 * v64
    assert set(on.grads) == set(off.grads)
    for name in on.grads:
        if name in g64:
            extra = on.grads[name].cpu().double() - off.grads[name].cpu().double()
            assert float(g64[name].abs().max()) > 0
            check("train_step chamfer grad", f"{name} cap={max_dist}", extra.reshape(g64[name].shape), g64[name], g32[name].double(),
                  float(off.grads[name].abs().max()))
        else:
            assert torch.equal(on.grads[name], off.grads[name]), f"{name} received a gradient from the Chamfer term"
