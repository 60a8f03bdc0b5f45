"""The calling contract of the 18 HIP autograd nodes outside meshnet/graph_ops.py, through tests/autograd_contract.py: one case per node
(and per form of a node), each through C1 strided inputs, C2 second backward, C3 accumulation, C4 needs_input_grad subsets, C5 upstream
gradient forms, C6 in-place edit before backward, C7 create_graph.  Every clause is compared with the case's PLAIN form (contiguous fp32
leaves, every differentiable output weighted, one backward), and test_plain_form_meets_the_fp64_bar anchors that form to the node's own
fp64 restatement under the bar rule of the node's own test file (imported, not restated).  Nodes whose backward sums with float atomics
run in their reproducible form: the rasterizer under debug flag 256, the cloth regularisers with the edge CSR, the mesh transform with
its incidence CSR.  The rasterizer's per-Gaussian inputs keep their refusal of strided tensors under STRICT ("refuses").
The nodes of meshnet/graph_ops.py, UpdatePrediction and _Length: tests/test_autograd_contract_meshnet_gpu.py (C1 with the "offset" kind too).

What the table showed on an MI355X when this file was written ("equal bits" = eq; wall time of the 225 tests: 7 s; the slowest
pairs 0.7 s and 0.6 s -- C5 of gaussian_step_inputs, 510 subsets of its 9 outputs, and of raster batch V=2 features, 254 of its 8):

  case                       | C1                    | C2 | C3 | C4 | C5                    | C6          | C7
  l1, l1 masked, l1 both     | eq                    | eq | eq | eq | eq                    | eq          | raises
  blur                       | eq                    | eq | eq | eq | eq                    | eq          | within bar (0.12)
  ssim, image_loss           | eq                    | eq | eq | eq | eq                    | raises      | raises
  image_loss add             | eq                    | eq | eq | eq | eq                    | eq / raises | raises
  mesh_transform[_views]     | eq                    | eq | eq | eq | eq                    | raises      | raises
  gaussian_activations       | eq / within bar (0.12)| eq | eq | eq | eq                    | eq          | raises
  gaussian_step_inputs       | eq / within bar (0.15)| eq | eq | eq | eq                    | eq / raises | raises
  unbind_views               | eq                    | eq | eq | eq | eq                    | raises      | raises
  cloth_regs                 | eq                    | eq | eq | eq | eq                    | eq          | raises
  cloth_regs tap [defer]     | eq                    | eq | eq | eq | eq                    | raises      | raises
  simulator_step             | eq                    | eq | eq | eq | eq                    | eq / raises | raises
  geometry_loss (both sizes) | eq                    | eq | eq | eq | eq                    | eq          | raises
  flow_loss                  | eq / within bar (0.13)| eq | eq | eq | eq                    | eq          | raises
  knn_regs, chamfer, project | eq                    | eq | eq | eq | eq                    | raises      | raises
  raster single V=1 (both)   | eq / refuses          | eq | eq | eq | eq                    | eq / raises | raises
  raster batch V=1 features  | eq / refuses          | eq | eq | eq | eq / within bar (0.06)| eq / raises | raises
  raster batch V=2 colour    | eq / refuses          | eq | eq | eq | eq / within bar (0.06)| eq / raises | raises
  raster batch V=2 depth     | eq / refuses          | eq | eq | eq | eq / within bar (0.07)| eq / raises | raises
  raster batch V=2 features  | eq / refuses          | eq | eq | eq | eq / within bar (0.08)| eq / raises | raises

An entry with two words: the inputs (C1, C6) or subsets (C5) of the case differ.  Why an entry is not "equal bits":
  C1 within bar   a strided activation parameter (pc.activations, and through it pc.step_inputs) and strided points of flow_losses leave
                  the HIP path as a counted "layout" fallback: torch operations, compared with the fp64 restatement.
  C1 refuses      the rasterizer's per-Gaussian inputs (CsplatError "would leave the HIP path (layout)" under STRICT,
                  test_strict_dispatch_rejects_non_fp32_and_strided_inputs): each of them must refuse that way; means2D and features
                  must be taken strided, with equal bits (as is the [P, 1] opacity as a transposed view, which is contiguous).
  C5 within bar   the rasterizer launches other kernels when a gradient image is absent -- K7's colour, depth and feature paths, the
                  per-view and the all-views K8, a view without any gradient leaves the call -- and they round differently
                  (largest difference seen: 1.2e-5 of 16); those subsets against fp64 at the plain form's bar.  Every non-empty subset
                  is run, the mixed ones of two views included (colour in one view, depth only in the other).
  C6 raises       the input is saved (or, for unbind_views and the tapped regularisers, the output is a view of it): autograd refuses
                  the backward.  "equal bits": the node kept what it needs (sign bytes, the gradient, its outputs) and reads no input.
  C7 raises       once_differentiable; blur's backward is the node itself, its second derivative is within the bar of F.conv2d in fp64.
No pair is n.a.  Plain forms against fp64, error / bar: 0.03 .. 0.24 (project_points 0.24, knn_regs 0.22)."""
import contextlib
import copy
from types import SimpleNamespace

import numpy as np
import pytest

import util
import autograd_contract as ac
import train_kernels_ref as R
import sim_rollout_ref as SR
import mesh_transform_ref as M
import chamfer_ref as CR
import test_train_kernels_gpu as TK
import test_sim_rollout_kernels_gpu as TS
import test_mesh_transform_gpu as TM
import test_geometry_loss_gpu as TG
import test_flow_loss_gpu as TF
import test_knn_regs_gpu as TN
import test_chamfer_gpu as TC
import test_raster_extended_edges_gpu as E
import test_raster_image_sizes_gpu as TI
import test_render_gpu as TR

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
F64, F32 = torch.float64, torch.float32
DEV = "cuda"
ROWS = {}
RATIOS = {}


def cuda(t):
    return None if t is None else t.detach().to(DEV).contiguous()


def cpu(t):
    return None if t is None else t.detach().cpu()


def _fallbacks():
    from csplat import native
    return native.allow_fallbacks("layout")


def _ratio(table, *groups):
    """the largest error / bar the check() calls of these groups saw (their TABLE keeps the smallest bar / error)"""
    return max(1.0 / table[g][4] for g in groups if g in table)


def _up(result, i=0):
    return float(result.ups[i])


def _leaf(t, dt):
    return t.detach().cpu().to(dt).clone().requires_grad_()


# ================================================================================================ image losses, [2, 3, 37, 53]
IMG = (2, 3, 37, 53)
LAM, W_IMG, W_ADD, PS = TK.LAM, TK.W_IMG, TK.W_ADD, TK.PS


def _l1(masked, both=False):
    """l1_loss(render, gt): gt a constant, as a train step calls it (both: the two operands differentiable, d/db = -d/da)"""
    from csplat.train import l1_loss
    x, y, mask = R.image_case("uniform", IMG, 1 if masked else 0, seed=3)
    mc, yc = cuda(mask), cuda(y)
    group = "contract l1" + (" masked" if masked else "") + (" both" if both else "")

    def bar(r):
        up, res = _up(r), []
        for dt in (F64, F32):
            a, b = _leaf(r.leaves["a"], dt), _leaf(r.leaves["b"] if both else y, dt)
            v = R.l1(a, b, mask, dt)
            (up * v).backward()
            res.append((v.detach(), a.grad, b.grad))
        TK.check(group, "value", r.outs[0], res[0][0], res[1][0], 1e-30)
        for k, n in (("a", 1), ("b", 2))[:2 if both else 1]:
            TK.check(group, f"d/d{k}", r.grads[k], res[0][n], res[1][n], abs(up) / x.numel())
        return _ratio(TK.TABLE, group)
    diff = dict(a=cuda(x), b=yc) if both else dict(a=cuda(x))
    return ac.Case(name=group[9:], call=lambda t: l1_loss(t["a"], t["b"] if both else yc, mc), diff=diff, bar=bar, fallbacks=_fallbacks)


def _taps64():
    g = torch.tensor([np.exp(-(i - 5) ** 2 / (2 * 1.5 ** 2)) for i in range(11)], dtype=F32)
    return (g / g.sum())


def _conv_blur(x, dt):
    """the 11 x 11 zero-padded Gaussian window through F.conv2d, planes as channels of one group each"""
    import torch.nn.functional as Fn
    g = _taps64().to(dt)
    n = x.shape[0] * x.shape[1]
    z = x.reshape(1, n, *x.shape[-2:])
    z = Fn.conv2d(z, g.view(1, 1, 1, 11).expand(n, 1, 1, 11).contiguous(), padding=(0, 5), groups=n)
    z = Fn.conv2d(z, g.view(1, 1, 11, 1).expand(n, 1, 11, 1).contiguous(), padding=(5, 0), groups=n)
    return z.reshape(x.shape)


def _blur():
    from csplat.train import GaussianBlur11
    x, _y, _ = R.image_case("uniform", IMG, 0, seed=4)
    group = "contract blur"

    def bar(r):
        res = []
        for dt in (F64, F32):
            b = _leaf(r.leaves["x"], dt)
            o = R.blur(b, dt)
            o.backward(cpu(r.ups[0]).to(dt))
            res.append((o.detach(), b.grad))
        TK.check(group, "value", r.outs[0], res[0][0], res[1][0], 1e-30)
        TK.check(group, "adjoint", r.grads["x"], res[0][1], res[1][1], 1e-30)
        return _ratio(TK.TABLE, group)

    def second(r):
        """d/d(upstream) of <blur^T(upstream), probe> = blur(probe), and nothing towards x (the node is linear), through F.conv2d"""
        dx = r["d_leaves"]["x"]
        assert dx is None or not bool(dx.any())
        res = []
        for dt in (F64, F32):
            xx, u = _leaf(r["leaves"]["x"], dt), _leaf(r["ups"][0], dt)
            first, = torch.autograd.grad(_conv_blur(xx, dt), xx, u, create_graph=True)
            res.append(torch.autograd.grad(first, u, cpu(r["probe"]["x"]).to(dt))[0])
        TK.check(group + " second", "d/d upstream", r["d_ups"][0], res[0], res[1], 1e-30)
        return _ratio(TK.TABLE, group + " second")
    return ac.Case(name="blur", call=lambda t: GaussianBlur11.apply(t["x"]), diff=dict(x=cuda(x)), bar=bar, second=second, fallbacks=_fallbacks)


def _ssim():
    from csplat.train import ssim
    x, y, _ = R.image_case("uniform", IMG, 0, seed=5)
    yc = cuda(y)
    group = "contract ssim"

    def bar(r):
        up, res = _up(r), []
        for dt in (F64, F32):
            a = _leaf(r.leaves["img1"], dt)
            s = R.ssim(a, y, dt)
            (up * s).backward()
            res.append((s.detach(), a.grad))
        TK.check(group, "value", r.outs[0], res[0][0], res[1][0], 1.0)
        TK.check(group, "d/dx", r.grads["img1"], res[0][1], res[1][1], abs(up) / x.numel())
        return _ratio(TK.TABLE, group)
    return ac.Case(name="ssim", call=lambda t: ssim(t["img1"], yc), diff=dict(img1=cuda(x)), bar=bar, fallbacks=_fallbacks)


def _image_loss(with_add):
    from csplat import train as tr
    x, y, mask = R.image_case("uniform", IMG, 1, seed=6)
    yc, mc = cuda(y), cuda(mask)
    group = f"contract image_loss{' add' if with_add else ''}"
    opt = SimpleNamespace(lambda_dssim=LAM)
    w_img, w_add, ps = (W_IMG, W_ADD, PS) if with_add else (1.0, 1.0, 1.0)

    def call(t):
        if with_add:      # (the sum with the regularisers: no wrapper but train_step itself)
            return tr.FusedImageLoss.apply(t["image"], yc, LAM, mc, t["add"], w_img, w_add, ps)
        return tr.image_losses(t["image"], yc, opt, mc)

    def bar(r):
        up, res = _up(r), []
        for dt in (F64, F32):
            a = _leaf(r.leaves["image"], dt)
            add = _leaf(r.leaves["add"], dt) if with_add else None
            out0, psn, il, _ = R.image_loss(a, y, LAM, mask, add, w_img, w_add, ps, dtype=dt)
            (up * out0).backward()
            res.append(dict(loss=out0.detach(), psnr=psn, il=il, dx=a.grad, dadd=add.grad if with_add else None))
        TK.check(group, "loss", r.outs[0], res[0]["loss"], res[1]["loss"], w_img * LAM)
        TK.check(group, "d/dx", r.grads["image"], res[0]["dx"], res[1]["dx"], abs(up) * w_img / x.numel())
        if with_add:
            TK.check(group, "image_loss", r.outs[2], res[0]["il"], res[1]["il"], LAM)
            TK.check(group, "psnr", r.outs[1], res[0]["psnr"], res[1]["psnr"], 1.0)
            TK.check(group, "d/dadd", r.grads["add"], res[0]["dadd"], res[1]["dadd"], 1e-30)
        return _ratio(TK.TABLE, group)
    diff = dict(image=cuda(x))
    if with_add:
        diff["add"] = torch.tensor(TK.ADD, device=DEV)
    return ac.Case(name=group[9:], call=call, diff=diff, bar=bar, fallbacks=_fallbacks)


# ================================================================================================ mesh transform and activations, P = 257, T = 3
def _mesh_case():
    return M.branch_case(257, T=3, seed=5)


def _pc_for(case):
    """a MeshGaussians on the case whose parameters the call replaces; its rest-pose record and incidence CSR are built once"""
    proto = TM._model(case)
    proto._rest()

    def make(t):
        pc = copy.copy(proto)
        pc.__dict__.pop("_fused_cache", None)
        for attr, key in (("face_bary", "bary"), ("_rotation", "rotation"), ("_opacity", "opacity"), ("_scaling", "scaling"),
                          ("_features_dc", "f_dc"), ("_features_rest", "f_rest")):
            if key in t:
                setattr(pc, attr, t[key])
        return pc
    return proto, make


def _mesh_bar(case, T, xyz_of, quat_of, extra=None):
    def bar(r):
        xyz, quat = xyz_of(r.outs).cpu().numpy(), quat_of(r.outs).cpu().numpy()
        r64, r32 = TM.reference(case, q_gpu=quat)
        worst = 0.0
        for name, got in (("xyz", xyz), ("quat", quat), ("d_vertices", r.grads["vertices"]), ("d_bary", r.grads["bary"]),
                          ("d_rotation", r.grads["rotation"])):
            e, b = TM.check(name, got.cpu().numpy() if torch.is_tensor(got) else got, r64, r32, "contract")
            worst = max(worst, e / b)
        return max(worst, extra(r) if extra is not None else 0.0)
    return bar


def _mesh_weights(case, T, n_xyz):
    """the loss weights of the restatement's case, by output position (T means3D rows, then T rotations; or the two [T,P,.] tensors)"""
    def weights(i, o):
        if n_xyz == 1:
            return torch.tensor(case["w_xyz" if i == 0 else "w_quat"], dtype=F32)
        return torch.tensor(case["w_xyz"][i] if i < T else case["w_quat"][i - T], dtype=F32)
    return weights


def _mesh_diff(case):
    return dict(vertices=torch.tensor(case["deformed"], device=DEV), bary=torch.tensor(case["bary"], device=DEV),
                rotation=torch.tensor(case["rot"], device=DEV))


def _mesh_transform():
    case = _mesh_case()
    _proto, make = _pc_for(case)

    def call(t):
        pc = make(t)
        return pc.get_xyz(t["vertices"]), pc.get_rotation(t["vertices"])
    return ac.Case(name="mesh_transform", call=call, diff=_mesh_diff(case), outputs=(0, 1), fallbacks=_fallbacks,
                   weights=_mesh_weights(case, 3, 1), bar=_mesh_bar(case, 3, lambda o: o[0], lambda o: o[1]))


def _mesh_views():
    case = _mesh_case()
    T = 3
    _proto, make = _pc_for(case)

    def call(t):
        xyz, quat = make(t).transform_views(t["vertices"])
        return tuple(xyz) + tuple(quat)
    return ac.Case(name="mesh_transform_views", call=call, diff=_mesh_diff(case), outputs=tuple(range(2 * T)), fallbacks=_fallbacks,
                   joins=(tuple(range(T)), tuple(range(T, 2 * T))), weights=_mesh_weights(case, T, T),
                   bar=_mesh_bar(case, T, lambda o: torch.stack(o[:T]), lambda o: torch.stack(o[T:2 * T])))


def _act_diff(proto):
    return dict(opacity=proto._opacity.detach().clone(), scaling=proto._scaling.detach().clone(), f_dc=proto._features_dc.detach().clone(),
                f_rest=proto._features_rest.detach().clone())


def _act_bar(group, at):
    """the activations' three outputs at positions at .. at + 2 against train_kernels_ref.gauss_act (the bars of test_train_kernels_gpu)"""
    def bar(r):
        raw = [cpu(r.leaves[k]) for k in ("opacity", "scaling", "f_dc", "f_rest")]
        ws = [cpu(r.ups[at + k]) for k in range(3)]
        res = [(R.gauss_act(*raw, dtype=dt), R.gauss_act_adjoint(raw, ws, dt)) for dt in (F64, F32)]
        for k, name in enumerate(("opacity", "scales")):
            TK.check(group, name, r.outs[at + k], res[0][0][k], res[1][0][k], 1e-30)
        for k, name in enumerate(("opacity", "scaling", "f_dc", "f_rest")):
            TK.check(group, "d_" + name, r.grads[name], res[0][1][k], res[1][1][k], 1e-30)
        assert torch.equal(r.outs[at + 2].cpu(), torch.cat((raw[2], raw[3]), 1))
        return _ratio(TK.TABLE, group)
    return bar


def _activations():
    case = _mesh_case()
    proto, make = _pc_for(case)

    def call(t):
        pc = make(t)
        out = pc.activations()      # (None: the fused form does not apply -- render() then takes the three properties)
        return out if out is not None else (pc.get_opacity, pc.get_scaling, pc.get_features)
    return ac.Case(name="gaussian_activations", call=call, diff=_act_diff(proto), outputs=(0, 1, 2), fallbacks=_fallbacks,
                   bar=_act_bar("contract activations", 0))


def _step_inputs():
    case = _mesh_case()
    T = 3
    proto, make = _pc_for(case)

    def call(t):
        pc = make(t)
        out = pc.step_inputs(t["vertices"])
        if out is None:             # (render_views' own composition when the one-node form does not apply)
            xyz, quat = pc.transform_views(t["vertices"])
            act = pc.activations()
            out = (xyz, quat) + (tuple(act) if act is not None else (pc.get_opacity, pc.get_scaling, pc.get_features))
        return tuple(out[0]) + tuple(out[1]) + tuple(out[2:])
    mesh_w = _mesh_weights(case, T, T)
    return ac.Case(name="gaussian_step_inputs", call=call, diff={**_mesh_diff(case), **_act_diff(proto)}, outputs=tuple(range(2 * T + 3)),
                   fallbacks=_fallbacks, joins=(tuple(range(T)), tuple(range(T, 2 * T))),
                   weights=lambda i, o: mesh_w(i, o) if i < 2 * T else 0.5 + torch.rand(o.shape, generator=torch.Generator().manual_seed(i)),
                   bar=_mesh_bar(case, T, lambda o: torch.stack(o[:T]), lambda o: torch.stack(o[T:2 * T]),
                                 extra=_act_bar("contract step_inputs", 2 * T)))


def _unbind_views():
    from csplat.gaussians import UnbindViews
    x = torch.randn(3, 257, 3, generator=torch.Generator().manual_seed(8))

    def bar(r):                     # (no arithmetic: the rows and the joined gradient are copies)
        assert all(torch.equal(o, r.leaves["x"][i]) for i, o in enumerate(r.outs))
        assert torch.equal(r.grads["x"], torch.stack([r.ups[i] for i in range(3)]))
        return 0.0
    return ac.Case(name="unbind_views", call=lambda t: UnbindViews.apply(t["x"]), diff=dict(x=cuda(x)), outputs=(0, 1, 2), joins=((0, 1, 2),),
                   bar=bar, fallbacks=_fallbacks)


# ================================================================================================ cloth regularisers and the simulator, (3, 257, 300)
LAMS = (0.01, 0.3, 0.1)
OPT = SimpleNamespace(lambda_deform_mag=LAMS[0], lambda_rigid=LAMS[1], lambda_momentum=LAMS[2])


def _cloth(tap, defer):
    from csplat import train as tr
    D, ei, rest, _info = SR.regs_case(3, 257, 300)
    g = SimpleNamespace(mesh=SimpleNamespace(edge_index=cuda(ei)), edge_norm=cuda(rest).reshape(-1, 1))
    group = "contract cloth_regs" + (" tap" if tap else "") + (" defer" if defer else "")

    def call(t):
        return tr.regularization(t["D"], g, OPT, tap=tap, defer=defer)

    def bar(r):
        gl = _up(r)
        res = []
        for dt in (F64, F32):
            l, gd = SR.cloth_regs(cpu(r.leaves["D"]), ei, rest, *LAMS, dt)
            res.append((l, gl * gd + (cpu(r.ups[1]).to(dt) if tap else 0.0)))
        TS.check(group, "loss", r.outs[0], res[0][0], res[1][0], 1e-30)
        TS.check(group, "d/dD", r.grads["D"], res[0][1], res[1][1], 1e-30)
        if tap:
            assert ac.same(r.outs[1], r.leaves["D"])
        return _ratio(TS.TABLE, group)
    return ac.Case(name=group[9:], call=call, diff=dict(D=cuda(D)), outputs=(0, 1) if tap else (0,), bar=bar, fallbacks=_fallbacks,
                   after=tr.launch_deferred if defer else None)


def _simulator_step():
    from csplat import train as tr
    s = TS._step_inputs()
    names = ("W1", "b1", "W2", "b2", "Wo", "bo")
    g = SimpleNamespace(mesh=SimpleNamespace(edge_index=cuda(s["ei"])), edge_norm=cuda(s["rest"]).reshape(-1, 1))
    enc, base = cuda(s["e"]), cuda(s["base"])
    group = "contract simulator_step"

    def call(t):
        lin = lambda w, b: SimpleNamespace(weight=t[w], bias=t[b])  # noqa: E731
        sim = SimpleNamespace(times_on_device=None, input=lin("W1", "b1"), hidden=lin("W2", "b2"), output=lin("Wo", "bo"))
        out = tr.simulator_step(sim, [0.0] * s["T"], g, OPT, static=(enc, base))
        assert out is not None
        return out

    def bar(r):
        gl = _up(r, 1)
        sc = dict(s, wD=cpu(r.ups[0]), **{k: cpu(r.leaves[k]) for k in names})
        r64, r32 = TS._step_reference(sc, gl, F64), TS._step_reference(sc, gl, F32)
        TS.check(group, "vertices", r.outs[0], r64["D"], r32["D"], 1e-30)
        TS.check(group, "loss", r.outs[1], r64["loss"], r32["loss"], 1e-30)
        for k in names:
            TS.check(group, f"d/d{k}", r.grads[k], r64[k], r32[k], 1e-30)
        return _ratio(TS.TABLE, group)
    return ac.Case(name="simulator_step", call=call, diff={k: cuda(s[k]) for k in names}, outputs=(0, 1), bar=bar, fallbacks=_fallbacks)


# ================================================================================================ geometry, flow, neighbourhood, Chamfer, projection
def _geometry(shape):
    from csplat import train as tr
    c = TG.make_case(shape, "weight")
    c["M"] = TG.make_case(shape, "mask_frac")["M"]
    V = shape[0]
    Z, S, Mk = ([cuda(t) for t in c[k]] for k in ("Z", "S", "M"))
    group = f"contract geometry {shape}"

    def call(t):
        return tr.geometry_losses([t[f"D{v}"] for v in range(V)], [t[f"A{v}"] for v in range(V)], Z, S, c["lam_d"], c["lam_s"], masks=Mk,
                                  add=t["add"], weight=c["weight"], add_weight=c["add_weight"])

    def bar(r):
        cc = dict(c, g=_up(r), D=[cpu(r.leaves[f"D{v}"]) for v in range(V)], A=[cpu(r.leaves[f"A{v}"]) for v in range(V)],
                  add=cpu(r.leaves["add"]))
        got = (r.outs[0], r.outs[1], r.outs[2], torch.stack([r.grads[f"D{v}"].reshape(shape[1:]) for v in range(V)]),
               torch.stack([r.grads[f"A{v}"].reshape(shape[1:]) for v in range(V)]))
        TG.compare(group, cc, got)
        assert float(r.grads["add"]) == np.float32(_up(r)) * np.float32(c["add_weight"])
        return _ratio(TK.TABLE, group, group + " grad")
    diff = {f"{k}{v}": cuda(c[k][v]) for k in ("D", "A") for v in range(V)}
    diff["add"] = cuda(c["add"])
    return ac.Case(name=f"geometry_loss {shape}", call=call, diff=diff, bar=bar, fallbacks=_fallbacks)


def _flow():
    from csplat import train as tr
    c = TF.make_case(257, 3, (37, 23), "scaled")
    c["masks"], c["cap"] = TF.make_case(257, 3, (37, 23), "mask_cap")["masks"], 6.0
    T = c["T"]
    full, flows, masks, vis = [cuda(f) for f in c["full"]], [cuda(f) for f in c["flows"]], [cuda(m) for m in c["masks"]], [cuda(v) for v in c["vis"]]
    group = "contract flow_loss"

    def call(t):
        return tr.flow_losses([t[f"X{k}"] for k in range(T)], full, flows, (c["H"], c["W"]), visible=vis, masks=masks, lambda_flow=c["lam"],
                              max_error=c["cap"], add=t["add"], weight=c["weight"], add_weight=c["add_weight"])

    def bar(r):
        cc = dict(c, g=_up(r), X=[cpu(r.leaves[f"X{k}"]) for k in range(T)], add=cpu(r.leaves["add"]))
        got = SimpleNamespace(total=r.outs[0], L=r.outs[1], count=int(r.outs[2]), grad=torch.stack([r.grads[f"X{k}"] for k in range(T)]))
        TF.compare(group, cc, got)
        return _ratio(TK.TABLE, group, group + " grad")
    diff = {f"X{k}": cuda(c["X"][k]) for k in range(T)}
    diff["add"] = cuda(c["add"])
    return ac.Case(name="flow_loss", call=call, diff=diff, bar=bar, fallbacks=_fallbacks)


def _knn_regs():
    from csplat.knn_regs import neighbour_regularization
    pts, Mm, Q = TN.rows(257, 3, "large", seed=3)
    graph = TN.knn_graph(pts, 5)

    def bar(r):
        before = TN.WORST["ratio"]
        TN.WORST["ratio"] = 0.0
        try:        # (compare() runs the kernel itself, on these rows with this upstream gradient: the plain form)
            got, _r64 = TN.compare("contract knn_regs", graph, cpu(r.leaves["means"]).numpy(), cpu(r.leaves["rotations"]).numpy(), TN.ALL, True,
                                   _up(r))
            ratio = TN.WORST["ratio"]
        finally:
            TN.WORST["ratio"] = max(before, TN.WORST["ratio"])
        assert np.array_equal(got["dM"], r.grads["means"].cpu().numpy()) and np.array_equal(got["dQ"], r.grads["rotations"].cpu().numpy())
        return ratio
    return ac.Case(name="knn_regs", call=lambda t: neighbour_regularization(t["means"], t["rotations"], graph, *TN.ALL, isometric_abs=True),
                   diff=dict(means=TN.gpu(Mm), rotations=TN.gpu(Q)), bar=bar, fallbacks=_fallbacks)


def _chamfer():
    from csplat.pointcloud import chamfer_distance
    rng = np.random.default_rng(9)
    a, b = rng.normal(size=(257, 3)).astype(np.float32), rng.normal(size=(300, 3)).astype(np.float32)
    cap = float(np.sort(TC.nearest(a, b)[0])[200])

    def bar(r):
        qa, pb = cpu(r.leaves["x"]).numpy(), cpu(r.leaves["y"]).numpy()
        d2, idx = TC.nearest(qa, pb)
        ref = CR.direction(qa, pb, idx, d2, cap, g=float(np.float32(_up(r))))
        TC._check_direction("contract chamfer", r.grads["x"].cpu().numpy(), r.grads["y"].cpu().numpy(), ref)
        worst = 0.0
        for got, want, bound in ((r.grads["x"], ref["dq"], ref["bound_q"]), (r.grads["y"], ref["dp"], ref["bound_p"])):
            worst = max(worst, float((np.abs(got.cpu().numpy().astype(np.float64) - want) / np.maximum(bound, 1e-300)).max()))
        return worst
    return ac.Case(name="chamfer", call=lambda t: chamfer_distance(t["x"], t["y"], two_sided=False, max_sq_dist=cap),
                   diff=dict(x=TC.gpu(a), y=TC.gpu(b)), bar=bar, fallbacks=_fallbacks)


def _project_points():
    import gaussian_renderer as gr
    from csplat import synthetic as syn
    W, H = 640, 360
    full = torch.tensor(syn.make_camera(33.0, W, H)["full_proj_transform"], device=DEV)
    cam = SimpleNamespace(full_proj_transform=full, image_width=W, image_height=H)
    pts = torch.rand(257, 3, generator=torch.Generator().manual_seed(10)) - 0.5

    def bar(r):
        """the bars of tests/test_render_gpu.py::test_projection_kernel_matches_reference_formula_and_has_a_gradient"""
        p64 = _leaf(r.leaves["points"], F64)
        ref = TR.projection_fp64(full.cpu(), p64, W, H)
        ref.backward(cpu(r.ups[0]).double())
        return TR.check_projection(r.outs[0], ref, r.grads["points"], p64.grad, W, H)
    return ac.Case(name="project_points", call=lambda t: gr._project(cam, t["points"]), diff=dict(points=cuda(pts)), bar=bar, fallbacks=_fallbacks)


# ================================================================================================ the rasterizer, P = 300, 40 x 24, SH degree 1
RASTER = dict(P=300, W=40, H=24, seed=12, grid=8, scale_mul=2.0)
GNAMES = E.GKEYS            # means3D, opacities, shs, scales, rotations


@contextlib.contextmanager
def _raster_scope(per_call=True):
    """the bit-reproducible K7 (debug flag 256); per_call=False: one view goes through _RasterizeGaussians (csplat_forward_begin / _finish)"""
    from csplat import native
    import diff_gaussian_rasterization as dgr
    old_flags, old_spec = int(native.lib.csplat_debug_flags_query()), dgr.PER_CALL_SPECULATION
    native.lib.csplat_debug_flags(old_flags | 256)
    dgr.PER_CALL_SPECULATION = per_call
    try:
        yield
    finally:
        dgr.PER_CALL_SPECULATION = old_spec
        native.lib.csplat_debug_flags(old_flags)


def _raster(form, V, node):
    """form: "colour" | "depth" | "features" (2 feature channels + alpha; the batched node only); V views of one Gaussian set;
    node: "single" = _RasterizeGaussians, "batch" = _RasterizeGaussiansBatch (GaussianRasterizer for V = 1, rasterize_views for V = 2)"""
    from csplat import native
    import diff_gaussian_rasterization as dgr
    F, alpha, depth = (2, True, True) if form == "features" else (0, False, form == "depth")
    cases = [dict(util.make_case(theta=-25.0 * i, **RASTER), sh_degree=1) for i in range(V)]
    views = [E._view(c, F=F, alpha=alpha, depth=depth, seed=40 + i) for i, c in enumerate(cases)]
    for v in views:
        v["feats"] = views[0]["feats"]          # (one Gaussian set, one feature tensor)
    settings = [util.gpu_settings(c) for c in cases]
    g = cases[0]["g"]
    diff = {k: torch.tensor(np.asarray(g[k], np.float32), device=DEV) for k in GNAMES}
    for i in range(V):
        diff[f"means2D_{i}"] = torch.zeros(RASTER["P"], 3, device=DEV)
    if F:
        diff["features"] = torch.tensor(views[0]["feats"], device=DEV)
    per_view = 3 + (1 if F else 0) + (1 if alpha else 0)          # colour, radii, depth[, feat][, alpha]
    want = [0] + ([2] if depth else []) + ([3, 4] if F else [])
    outputs = tuple(i * per_view + j for i in range(V) for j in want)
    wkey = {0: "color", 2: "depth", 3: "feat", 4: "alpha"}

    def call(t):
        kws = []
        for i in range(V):
            kw = dict(means3D=t["means3D"], means2D=t[f"means2D_{i}"], opacities=t["opacities"], shs=t["shs"], scales=t["scales"],
                      rotations=t["rotations"])
            if F:
                kw.update(features=t["features"], return_alpha=True)
            kws.append(kw)
        if V == 1:
            out = dgr.GaussianRasterizer(settings[0])(**kws[0])
            assert type(out[0].grad_fn).__name__.startswith("_RasterizeGaussiansBatch" if node == "batch" else "_RasterizeGaussiansBackward") \
                or not out[0].requires_grad
            return out
        return [o for view in dgr.rasterize_views(settings, kws) for o in view]

    def weights(i, o):
        return torch.tensor(np.asarray(views[i // per_view]["wts"][wkey[i % per_view]], np.float32))

    def bar(r):
        """images and gradients against the fp64 restatement over the fp32 oracle's lists (test_raster_extended_edges_gpu._compare_fp64);
        gradients at max(1e-4, 10 x the fp32 oracle's own error), the rule of test_raster_image_sizes_gpu"""
        refs = [E._ref(v) for v in views]
        lim = limit()
        n64 = lambda x: None if x is None else x.detach().cpu().numpy().astype(np.float64)  # noqa: E731
        shared = {k: sum(ref["grads"][k] for ref in refs) for k in GNAMES + (("features",) if F else ())}
        worst = 0.0
        for i, (v, ref) in enumerate(zip(views, refs)):
            o = r.outs[i * per_view:(i + 1) * per_view]
            got = dict(imgs=[n64(o[0]), n64(o[2]) if depth else None, n64(o[3]) if F else None, n64(o[4]) if F else None],
                       grads={**{k: n64(r.grads[k]) for k in shared}, "means2D": n64(r.grads[f"means2D_{i}"])}, cam=None)
            want_ = dict(imgs=ref["imgs"], grads={**shared, "means2D": ref["grads"]["means2D"]}, cam=None)
            E._compare_fp64(got, want_, v, bar=lim, cam=False, what=f"contract raster {form} view {i}")
            worst = max([worst] + [util.rel_err(got["grads"][k], want_["grads"][k]) / lim for k in want_["grads"]])
        return worst
    state = {}

    def limit():
        if "limit" not in state:
            state["limit"] = max(TI.TOL, TI.K * max(E._oracle_colour_err(c, v["wts"])[0] for c, v in zip(cases, views)))
        return state["limit"]

    def basis(i, kind):
        """the fp64 gradients of view i with only its `kind` image weighted (the gradient is linear in the weights)"""
        if (i, kind) not in state:
            w = views[i]["wts"]
            zero = lambda a: None if a is None else np.zeros_like(a)  # noqa: E731
            wts = dict(color=zero(w["color"]), depth=None, feat=zero(w["feat"]), alpha=zero(w["alpha"]))
            wts[kind] = w[kind]
            state[(i, kind)] = E._ref(dict(views[i], wts=wts))["grads"]
        return state[(i, kind)]

    def subset_bar(r):
        """the node takes other kernels when a gradient image is absent (the colour, depth and feature paths of K7, the per-view and the
        all-views K8; a view without any gradient leaves the call): those gradients against fp64, at the bar of the plain form"""
        names = GNAMES + (("features",) if F else ())
        want_ = {k: 0.0 for k in names}
        m2d = {i: np.zeros((RASTER["P"], 3)) for i in range(V)}
        for p in outputs:
            if bool(r.ups[p].any()):
                g_ = basis(p // per_view, wkey[p % per_view])
                for k in names:
                    want_[k] = want_[k] + g_[k]
                m2d[p // per_view] = m2d[p // per_view] + g_["means2D"]
        want_.update({f"means2D_{i}": m for i, m in m2d.items()})
        worst = max(util.rel_err(r.grads[k].cpu().numpy(), np.broadcast_to(want_[k], r.grads[k].shape)) / limit() for k in want_)
        assert worst < 1.0, worst
        return worst
    return ac.Case(name=f"raster {node} V={V} {form}", call=call, diff=diff, outputs=outputs, weights=weights, bar=bar, subset_bar=subset_bar,
                   scope=lambda: _raster_scope(per_call=(node == "batch")), fallbacks=None,
                   refuses=(native.CsplatError, "would leave the HIP path (layout)", GNAMES))


CASES = {
    "l1": lambda: _l1(False), "l1 masked": lambda: _l1(True), "l1 both": lambda: _l1(False, both=True), "blur": _blur, "ssim": _ssim,
    "image_loss": lambda: _image_loss(False), "image_loss add": lambda: _image_loss(True),
    "mesh_transform": _mesh_transform, "mesh_transform_views": _mesh_views, "gaussian_activations": _activations,
    "gaussian_step_inputs": _step_inputs, "unbind_views": _unbind_views,
    "cloth_regs": lambda: _cloth(False, False), "cloth_regs tap": lambda: _cloth(True, False), "cloth_regs tap defer": lambda: _cloth(True, True),
    "simulator_step": _simulator_step,
    "geometry_loss (2, 3, 5)": lambda: _geometry((2, 3, 5)), "geometry_loss (1, 16, 65)": lambda: _geometry((1, 16, 65)),
    "flow_loss": _flow, "knn_regs": _knn_regs, "chamfer": _chamfer, "project_points": _project_points,
    "raster single V=1 colour": lambda: _raster("colour", 1, "single"), "raster single V=1 depth": lambda: _raster("depth", 1, "single"),
    "raster batch V=1 features": lambda: _raster("features", 1, "batch"),
    "raster batch V=2 colour": lambda: _raster("colour", 2, "batch"), "raster batch V=2 depth": lambda: _raster("depth", 2, "batch"),
    "raster batch V=2 features": lambda: _raster("features", 2, "batch"),
}
_BUILT = {}


def built(name):
    """the case and its plain form, evaluated once and left unchanged"""
    if name not in _BUILT:
        case = CASES[name]()
        assert case.name == name, (case.name, name)
        _BUILT[name] = (case, ac.plain(case))
    return _BUILT[name]


@pytest.fixture(scope="module", autouse=True)
def _threads_and_table():
    old = torch.get_num_threads()
    torch.set_num_threads(min(16, old))
    yield
    torch.set_num_threads(old)
    rows = dict(ROWS)
    print("\n" + ac.table(rows, list(CASES)))
    print("plain form, error / bar against fp64: " + ", ".join(f"{k} {v:.2f}" for k, v in RATIOS.items()))
    for (name, clause), entry in rows.items():
        if entry == ac.NA:
            print(f"n.a. {name} {clause}: {_BUILT[name][0].na[clause]}")
    _BUILT.clear()


@pytest.mark.parametrize("name", list(CASES))
def test_plain_form_meets_the_fp64_bar(name):
    case, ref = built(name)
    RATIOS[name] = case.bar(ref)
    assert RATIOS[name] <= 1.0, RATIOS[name]


@pytest.mark.parametrize("clause", ac.CLAUSES)
@pytest.mark.parametrize("name", list(CASES))
def test_contract(name, clause):
    case, ref = built(name)
    ROWS[(name, clause)] = "FAILED"
    ROWS[(name, clause)] = ac.run_clause(case, clause, ref)


def test_at_most_one_pair_in_five_does_not_apply():
    na = sum(len(built(name)[0].na) for name in CASES)
    assert 5 * na <= len(CASES) * len(ac.CLAUSES), na
