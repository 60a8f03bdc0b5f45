"""The mesh -> Gaussian transform kernels (csplat_mesh_transform_fwd_views / _bwd_views / _bwd, include/csplat.h) against the fp64
restatement tests/mesh_transform_ref.py, per Gaussian and per vertex, on the cases it generates: every quaternion branch, rotations a few
float32 ulps from each branch boundary, small faces far out, un-normalised barycentric rows and raw rotations, T cameras, a vertex shared by
300 Gaussians, vertices no Gaussian references.  Both vertex-gradient paths (the incidence-CSR gather MeshTransform uses, the atomics
scatter of the C-ABI without incidence), GaussianStepInputs (what render_views / train_step use) and the argument edges.

Bars.  Every comparison is per row (a Gaussian's xyz of one camera, its quaternion, its d_bary / d_rotation row, a vertex's gradient of one
camera) through util.rowwise_rel_err, and its bar is derived from what float32 reaches on the same inputs: the same restatement evaluated in
float32 on the CPU gives a per-row error e32 against fp64, and the kernel must stay within K = 8 x max(e32) over the case, with a floor
of 1e-6 (8 float32 ulps of the row's scale; a single Gaussian's e32 can be far below its typical value).  Where float32 reaches it
the bar is therefore well below 1e-5; it is larger only where float32 itself loses digits (d_bary of faces of 1e-2 at a distance of 1:
y_k - xyz cancels).  The quaternion is compared up to its sign (the branch picks it); the loss weights of the fp64 gradient are multiplied
by the sign that aligns the reference with the GPU's OWN output quaternion, so a branch sign that differs from fp64 is no error while a
backward that differs in sign from its own forward is a 200 % error of that Gaussian's gradients."""
from types import SimpleNamespace

import numpy as np
import pytest

import util  # noqa: F401
import mesh_transform_ref as M
from util import rowwise_rel_err

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

K = 8.0
FLOOR = 1e-6


# ---------------------------------------------------------------- running the kernels
def _model(case):
    """a MeshGaussians on the case: rest mesh, faces, face ids, barycentric rows, raw rotations (+ activations for step_inputs)"""
    from csplat.gaussians import MeshGaussians
    dev = "cuda"
    P = case["face_ids"].shape[0]
    pc = MeshGaussians(3)
    pc.mesh = SimpleNamespace(pos=torch.tensor(case["rest"], device=dev), face=torch.tensor(case["faces"].T.copy(), device=dev),
                              edge_index=None)
    pc.face_ids = torch.tensor(case["face_ids"], device=dev)
    pc.face_bary = torch.nn.Parameter(torch.tensor(case["bary"], device=dev))
    pc._rotation = torch.nn.Parameter(torch.tensor(case["rot"], device=dev))
    g = torch.Generator(device=dev).manual_seed(0)
    pc._opacity = torch.nn.Parameter(torch.randn(P, 1, device=dev, generator=g))
    pc._scaling = torch.nn.Parameter(torch.randn(P, 3, device=dev, generator=g))
    pc._features_dc = torch.nn.Parameter(torch.randn(P, 1, 3, device=dev, generator=g))
    pc._features_rest = torch.nn.Parameter(torch.randn(P, 15, 3, device=dev, generator=g))
    return pc


def _loss(xyz, quat, case, w_xyz, w_quat):
    """sum_t <xyz_t, w_xyz_t> + <quat_t, w_quat_t> over the rows the flags keep (xyz, quat: sequences of T [P,3] / [P,4] tensors)"""
    wx, wq = torch.tensor(case["w_xyz"], device="cuda"), torch.tensor(case["w_quat"], device="cuda")
    terms = []
    for t in range(len(xyz)):
        if w_xyz:
            terms.append((xyz[t] * wx[t]).sum())
        if w_quat:
            terms.append((quat[t] * wq[t]).sum())
    return sum(terms)


def run_gather(case, w_xyz=True, w_quat=True, views=False):
    """MeshTransform (views=False: [T,P,*] outputs) or MeshTransformViews (views=True: the rows of pc.transform_views) with the incidence
    CSR, as MeshGaussians runs them -> numpy dict(xyz, quat, d_vertices, d_bary, d_rotation)"""
    from csplat.gaussians import MeshTransform
    pc = _model(case)
    dv = torch.tensor(case["deformed"], device="cuda").requires_grad_(True)
    if views:
        xyz, quat = pc.transform_views(dv)
        assert type(xyz[0].grad_fn).__name__ == "MeshTransformViewsBackward"
    else:
        r = pc._rest()
        xyz, quat = MeshTransform.apply(dv, pc.face_bary, pc._rotation, r[1], r[2], r[3], r[4])
    out = dict(xyz=torch.stack(list(xyz)).detach().cpu().numpy(), quat=torch.stack(list(quat)).detach().cpu().numpy())
    if w_xyz or w_quat:
        _loss(xyz, quat, case, w_xyz, w_quat).backward()
        out.update(d_vertices=dv.grad.cpu().numpy(), d_bary=pc.face_bary.grad.cpu().numpy(), d_rotation=pc._rotation.grad.cpu().numpy())
    return out


def run_atomics(case, w_xyz=True, w_quat=True, single=False):
    """the C-ABI's atomics scatter: csplat_mesh_transform_bwd_views with NULL incidence, or (single=True, T = 1) csplat_mesh_transform_bwd"""
    from csplat import native as n
    pc = _model(case)
    r = pc._rest()
    dv = torch.tensor(case["deformed"], device="cuda")
    T, V, P = dv.shape[0], dv.shape[1], case["face_ids"].shape[0]
    gx = torch.tensor(case["w_xyz"], device="cuda") if w_xyz else None
    gq = torch.tensor(case["w_quat"], device="cuda") if w_quat else None
    d_v = torch.full_like(dv, float("nan"))          # (the call zeroes it: NaN would survive in any entry it forgot)
    d_b = torch.full((P, 3), float("nan"), device="cuda")
    d_r = torch.full((P, 4), float("nan"), device="cuda")
    s = n.stream_handle(dv.device)
    if single:
        assert T == 1
        rc = n.lib.csplat_mesh_transform_bwd(s, P, V, n.ptr(r[1]), n.ptr(dv), n.ptr(pc.face_bary.data), n.ptr(pc._rotation.data), n.ptr(r[2]),
                                             n.ptr(gx), n.ptr(gq), n.ptr(d_v), n.ptr(d_b), n.ptr(d_r))
    else:
        rc = n.lib.csplat_mesh_transform_bwd_views(s, T, P, V, n.ptr(r[1]), n.ptr(dv), n.ptr(pc.face_bary.data), n.ptr(pc._rotation.data),
                                                   n.ptr(r[2]), n.ptr(gx), n.ptr(gq), n.ptr(d_v), n.ptr(d_b), n.ptr(d_r), None, None, None)
    n.check(rc, "csplat_mesh_transform_bwd")
    return dict(d_vertices=d_v.cpu().numpy(), d_bary=d_b.cpu().numpy(), d_rotation=d_r.cpu().numpy())


# ---------------------------------------------------------------- comparing
def _rows(arr):
    """rows of a result array: everything but its last axis (camera x Gaussian, camera x vertex, Gaussian)"""
    return int(np.prod(arr.shape[:-1]))


def quat_sign(q_gpu, q_ref):
    s = np.sign((np.asarray(q_gpu, np.float64) * q_ref).sum(-1))
    s[s == 0] = 1.0
    return s


def reference(case, w_xyz=True, w_quat=True, q_gpu=None):
    """(fp64 result, float32 result) of the restatement; with q_gpu (the GPU's own output quaternions) the quaternion loss weights of
    each evaluation are multiplied by the sign that aligns its quaternion with q_gpu"""
    if q_gpu is None:
        return M.evaluate(case, w_xyz, w_quat), M.evaluate(case, w_xyz, w_quat, dtype=torch.float32)
    r64 = M.evaluate(case, w_xyz, w_quat, quat_sign=quat_sign(q_gpu, M.evaluate(case, False, False)["quat"]))
    q32 = M.evaluate(case, False, False, dtype=torch.float32)["quat"]
    return r64, M.evaluate(case, w_xyz, w_quat, dtype=torch.float32, quat_sign=quat_sign(q_gpu, q32))


def bar_of(name, r32, r64):
    e32 = row_err(name, r32[name], r64)
    return max(K * float(e32.max()), FLOOR)


def row_err(name, got, r64):
    ref = r64[name]
    if name == "quat":
        got = np.asarray(got, np.float64) * quat_sign(got, ref)[..., None]
    return rowwise_rel_err(got, ref, _rows(ref))


def check(name, got, r64, r32, where=""):
    e = row_err(name, got, r64)
    bar = bar_of(name, r32, r64)
    worst = int(np.argmax(e))
    assert e.max() <= bar, f"{where} {name}: row {worst} error {e.max():.3e} > bar {bar:.3e} (float32 restatement: {bar / K:.3e})"
    return float(e.max()), bar


# ---------------------------------------------------------------- forward
SHAPES = [(T, P) for T in (1, 3, 5) for P in (1, 255, 256, 257)]


@pytest.mark.parametrize("T,P", SHAPES)
def test_forward_every_branch(T, P):
    """xyz and the quaternion (up to sign) of every Gaussian and camera, on branch_case (faces turned by 180 degrees about x, y, z, small
    and uniform rotations), at launch sizes around one 256-thread block"""
    case = M.branch_case(P, T=T, seed=100 * T + P)
    got = run_gather(case, False, False)
    r64, r32 = reference(case, False, False)
    for name in ("xyz", "quat"):
        check(name, got[name], r64, r32, f"T={T} P={P}")
    assert np.abs(np.linalg.norm(got["quat"], axis=-1) - 1).max() < 1e-6
    if P >= 255:
        counts = np.bincount(r64["branch"].reshape(-1), minlength=4)
        assert counts.min() >= 0.15 * T * P, counts


def test_forward_and_backward_at_the_train_step_size():
    """bench_train.py's default size: a 100 x 100 grid (10 000 vertices) carrying 100 000 Gaussians, 2 cameras"""
    case = M.bench_case(T=2, seed=1)
    got = run_gather(case)
    r64, r32 = reference(case, q_gpu=got["quat"])
    for name in ("xyz", "quat", "d_vertices", "d_bary", "d_rotation"):
        check(name, got[name], r64, r32, "bench")


# ---------------------------------------------------------------- backward
CASES = {
    "branch": lambda: M.branch_case(600, T=3, seed=11),
    "offset": lambda: M.branch_case(600, T=3, seed=12, size=1e-2, offset=1.0),
    "shared": lambda: M.shared_case(T=5, seed=13),
}
GRADS = {"both": (True, True), "xyz_only": (True, False), "quat_only": (False, True)}


@pytest.mark.parametrize("grad", list(GRADS))
@pytest.mark.parametrize("name", list(CASES))
def test_backward_gather_and_atomics(name, grad):
    """d_vertices, d_bary and d_rotation of the CSR-gather path (MeshTransform) and of the atomics path (csplat_mesh_transform_bwd_views
    without incidence) against fp64, with a gradient on xyz only, on the quaternion only and on both; the two paths agree with each other
    within the same bar (they differ only in the order of the vertex sums); the gather path is bit-equal from run to run."""
    case = CASES[name]()
    wx, wq = GRADS[grad]
    g1 = run_gather(case, wx, wq)
    r64, r32 = reference(case, wx, wq, q_gpu=g1["quat"])
    at = run_atomics(case, wx, wq)
    for k in ("d_vertices", "d_bary", "d_rotation"):
        if not np.abs(r64[k]).max() > 0:           # (d_rotation with a gradient on xyz only: exactly zero)
            assert np.abs(g1[k]).max() == 0 and np.abs(at[k]).max() == 0, k
            continue
        check(k, g1[k], r64, r32, f"{name}/{grad} gather")
        check(k, at[k], r64, r32, f"{name}/{grad} atomics")
        bar = bar_of(k, r32, r64)
        assert rowwise_rel_err(at[k], g1[k], _rows(g1[k])).max() <= bar, k
    g2 = run_gather(case, wx, wq)
    for k in ("d_vertices", "d_bary", "d_rotation"):
        assert np.array_equal(g1[k], g2[k]), k
    if name == "shared":
        un = M.unreferenced(case)
        assert un.sum() > 0 and (g1["d_vertices"][:, un] == 0).all() and (at["d_vertices"][:, un] == 0).all()


def test_single_camera_entry_point():
    """csplat_mesh_transform_bwd (the T = 1 atomics entry point of the header) against fp64 on the shared-vertex case"""
    case = M.shared_case(T=1, seed=14)
    q = run_gather(case, False, False)["quat"]
    r64, r32 = reference(case, q_gpu=q)
    got = run_atomics(case, single=True)
    for k in ("d_vertices", "d_bary", "d_rotation"):
        check(k, got[k], r64, r32, "csplat_mesh_transform_bwd")
    assert (got["d_vertices"][:, M.unreferenced(case)] == 0).all()


# ---------------------------------------------------------------- near ties
@pytest.mark.parametrize("T", [1, 3])
def test_near_tie_backward_takes_the_forward_branch(T):
    """rotations on every tie surface of the quaternion branch rule (R_ii = R_jj, R_ii = trace), nudged 0 .. 16 float32 ulps to either side:
    the GPU's forward picks one of the two tied formulas (either is right: the quaternion is compared up to sign) and its backward must
    differentiate THAT quaternion -- with the weights sign-aligned to the GPU's own output, every Gaussian's d_rotation and every vertex's
    gradient equals fp64 within the float32 bar.  A backward that picks the other formula of a pair with opposite signs is off by 200 %."""
    case = M.tie_case(reps=40, T=T, seed=20 + T)
    for views in (False, True):
        got = run_gather(case, False, True, views=views)
        r64, r32 = reference(case, False, True, q_gpu=got["quat"])
        check("quat", got["quat"], r64, r32, "tie")
        for k in ("d_vertices", "d_rotation"):
            check(k, got[k], r64, r32, f"tie views={views}")
        near = np.abs(r64["margin"]) < 2e-6
        assert near.mean() > 0.99
    at = run_atomics(case, False, True)
    check("d_rotation", at["d_rotation"], r64, r32, "tie atomics")


# ---------------------------------------------------------------- GaussianStepInputs
def test_step_inputs_against_fp64_with_sinks_and_silent_views():
    """pc.step_inputs (GaussianStepInputs: the transform and the activations as one autograd node, what render_views / train_step use):
    T = 4 cameras where view 1 receives no gradient at all and view 3 only on its quaternion; the parameter gradients are written into
    FlatGrads' sinks (csplat.dist) in place.  Values and gradients against fp64 (the silent view contributes nothing)."""
    from csplat import dist as cd
    case = M.shared_case(T=4, seed=15)
    mask = np.ones((4, 2), bool)
    mask[1] = False
    mask[3, 0] = False
    ref_case = dict(case, w_xyz=case["w_xyz"] * mask[:, None, None, 0], w_quat=case["w_quat"] * mask[:, None, None, 1])
    pc = _model(case)
    params = [pc.face_bary, pc._rotation, pc._opacity, pc._scaling, pc._features_dc, pc._features_rest]
    fg = cd.FlatGrads(params)
    try:
        fg.bind()
        dv = torch.tensor(case["deformed"], device="cuda").requires_grad_(True)
        out = pc.step_inputs(dv)
        assert out is not None and type(out[0][0].grad_fn).__name__ == "GaussianStepInputsBackward"
        xyz, quat = out[0], out[1]
        wx, wq = torch.tensor(case["w_xyz"], device="cuda"), torch.tensor(case["w_quat"], device="cuda")
        loss = sum((xyz[t] * wx[t]).sum() for t in range(4) if mask[t, 0]) + sum((quat[t] * wq[t]).sum() for t in range(4) if mask[t, 1])
        loss = loss + out[3].sum()                   # (an activation output too: the node's other half)
        loss.backward()
        q = torch.stack(list(quat)).detach().cpu().numpy()
        r64, r32 = reference(ref_case, q_gpu=q)
        check("xyz", torch.stack(list(xyz)).detach().cpu().numpy(), r64, r32, "step_inputs")
        check("quat", q, r64, r32, "step_inputs")
        check("d_vertices", dv.grad.cpu().numpy(), r64, r32, "step_inputs")
        assert (dv.grad[1] == 0).all()
        assert fg._placed[0] and fg._placed[1]       # d_bary, d_rotation written straight into their FlatGrads slices
        for k, p in (("d_bary", pc.face_bary), ("d_rotation", pc._rotation)):
            check(k, p.grad.cpu().numpy(), r64, r32, "step_inputs")
        np.testing.assert_allclose(pc._scaling.grad.cpu().numpy(), np.exp(pc._scaling.detach().cpu().numpy()), rtol=1e-6)
    finally:
        fg.unbind()
        fg.close()


# ---------------------------------------------------------------- argument edges
def test_empty_gaussians_and_empty_cameras():
    """P = 0: empty outputs, and a vertex gradient of exact zeros; T = 0: empty outputs, zero d_bary / d_rotation"""
    from csplat.gaussians import MeshTransform
    case = M.branch_case(8, T=2, seed=30)
    pc = _model(case)
    r = pc._rest()
    V = case["rest"].shape[0]
    dv = torch.tensor(case["deformed"], device="cuda").requires_grad_(True)
    b0 = torch.zeros(0, 3, device="cuda", requires_grad=True)
    q0 = torch.zeros(0, 4, device="cuda", requires_grad=True)
    vid0 = r[1][:0].contiguous()
    rest0 = torch.empty(256, dtype=torch.uint8, device="cuda")
    rowptr0 = torch.zeros(V + 1, dtype=torch.int32, device="cuda")
    corners0 = torch.zeros(1, dtype=torch.int32, device="cuda")
    for incidence in ((rowptr0, corners0), (None, None)):
        dv.grad = None
        xyz, quat = MeshTransform.apply(dv, b0, q0, vid0, rest0, *incidence)
        assert xyz.shape == (2, 0, 3) and quat.shape == (2, 0, 4)
        (xyz.sum() + quat.sum()).backward()
        assert dv.grad.shape == dv.shape and (dv.grad == 0).all()
    dv0 = torch.zeros(0, V, 3, device="cuda", requires_grad=True)
    xyz, quat = MeshTransform.apply(dv0, pc.face_bary, pc._rotation, r[1], r[2], r[3], r[4])
    assert xyz.shape == (0, 8, 3) and quat.shape == (0, 8, 4)
    (xyz.sum() + quat.sum()).backward()
    assert dv0.grad.shape == (0, V, 3)
    assert (pc.face_bary.grad == 0).all() and (pc._rotation.grad == 0).all()


def test_rotation_rows_that_need_normalising():
    """raw rotations with norms 1e-3 .. 1e3 (and one row scaled to each end): the quaternion is unit and d_rotation scales as 1 / |r|"""
    case = M.branch_case(256, T=1, seed=31)
    case["rot"][:4] *= np.float32([1e-3, 1e3, 1.0, 3e2])[:, None] / np.linalg.norm(case["rot"][:4], axis=1, keepdims=True)
    got = run_gather(case)
    r64, r32 = reference(case, q_gpu=got["quat"])
    for k in ("quat", "d_rotation"):
        check(k, got[k], r64, r32, "norms")
    assert np.abs(np.linalg.norm(got["quat"], axis=-1) - 1).max() < 1e-6
