"""The fp64 restatement of the mesh -> Gaussian transform (tests/mesh_transform_ref.py) and its case generators are what they claim, so that
test_mesh_transform_gpu.py can hold the HIP kernels to them: the reference's own run (tests/golden/mesh_transform.npz), scipy's
independent rotations, central differences, the branch coverage of every generator, and tie cases on both sides of every boundary."""
import numpy as np
import pytest

import util  # noqa: F401
import mesh_transform_ref as M
from util import golden

torch = pytest.importorskip("torch")
Rotation = pytest.importorskip("scipy.spatial.transform").Rotation

MIN_PER_BRANCH = {"branch": 150, "offset": 150, "tie": 400, "shared": 500}   # Gaussians per branch (all cameras) each generator must reach


def _cases():
    return {"branch": M.branch_case(256, T=3, seed=1), "offset": M.branch_case(256, T=3, seed=2, size=1e-2, offset=1.0),
            "tie": M.tie_case(reps=20, T=2, seed=3), "shared": M.shared_case(T=5, seed=4)}


def _golden_case(g):
    return dict(rest=g["pos"], deformed=g["deformed"][None], faces=g["face"].T.copy(), face_ids=g["face_ids"], bary=g["face_bary"],
                rot=g["rotation"], w_xyz=g["xyz_w"][None], w_quat=g["rot_w"][None])


def _rel(a, b):
    return float(np.abs(np.asarray(a) - b).max() / (np.abs(b).max() + 1e-300))


def test_restatement_reproduces_the_reference_run():
    """the reference's get_xyz (its torch arithmetic, float32, autograd) and get_rotation (roma served by scipy, float64; vertex gradient
    by central differences with h = 1e-4) on the fixture's float32 inputs.  Bars: float32 rounding of the fixture's own values (xyz
    1e-6, its gradients 1e-5), the float32 normalisation of the own rotation for the quaternion (1e-7), O(h^2) of the central differences for the rotation gradient."""
    g = golden("mesh_transform.npz")
    case = _golden_case(g)
    r = M.evaluate(case, w_quat=False)
    assert _rel(r["xyz"][0], g["xyz_deformed"]) < 1e-6
    assert _rel(r["d_vertices"][0], g["xyz_d_vertices"]) < 1e-5
    assert _rel(r["d_bary"], g["xyz_d_bary"]) < 1e-5
    q = r["quat"][0]
    sgn = np.sign((q * g["rot_deformed"]).sum(1))
    assert np.abs(q * sgn[:, None] - g["rot_deformed"]).max() < 1e-7       # (the reference normalises the float32 parameter in float32)
    rq = M.evaluate(case, w_xyz=False, quat_sign=sgn[None])
    assert _rel(rq["d_vertices"][0], g["rot_d_vertices_fd"]) < 1e-6
    assert M.branch_counts(case).tolist() == [4, 0, 145, 1]        # (why the fixture alone does not cover the branches)


def test_kabsch_closed_form_equals_svd_and_scipy():
    """kabsch_closed == kabsch_svd == scipy's align_vectors on every case and on random point triples (fp64 rounding: 1e-12)"""
    rng = np.random.default_rng(0)
    x, y = rng.normal(size=(300, 3, 3)), rng.normal(size=(300, 3, 3))
    pairs = [(x, y)]
    for c in _cases().values():
        vid = c["faces"][c["face_ids"]]
        pairs += [(c["rest"][vid].astype(np.float64), d[vid].astype(np.float64)) for d in c["deformed"]]
    for x, y in pairs:
        tx, ty = torch.tensor(x), torch.tensor(y)
        Rc, Rs = M.kabsch_closed(tx, ty).numpy(), M.kabsch_svd(tx, ty).numpy()
        Rsp = np.stack([Rotation.align_vectors(b - b.mean(0), a - a.mean(0))[0].as_matrix() for a, b in zip(x, y)])
        assert np.abs(Rc - Rs).max() < 1e-12 and np.abs(Rs - Rsp).max() < 1e-12
        assert np.abs(np.linalg.det(Rc) - 1).max() < 1e-12


def test_quaternion_and_product_equal_scipy():
    """rotmat_to_quat == scipy's from_matrix(R).as_quat() (same largest-of-(diagonal, trace) rule, so the same SIGN too) on random
    rotations and on rotations of each branch; hamilton(p, q) == (from_quat(p) * from_quat(q)).as_quat() up to sign"""
    rng = np.random.default_rng(1)
    Rs = [M._rotations(k, 200, rng) for k in M.KINDS] + [M.quat_to_rotmat(M.tie_quaternions(p, np.zeros(50), rng)) for p in M.TIE_PAIRS]
    R = np.concatenate(Rs)
    q = M.rotmat_to_quat(torch.tensor(R)).numpy()
    assert np.abs(q - Rotation.from_matrix(R).as_quat()).max() < 1e-14
    assert set(M.branch_and_margin(torch.tensor(R))[0].tolist()) == {0, 1, 2, 3}
    p = rng.normal(size=(R.shape[0], 4))
    p /= np.linalg.norm(p, axis=1, keepdims=True)
    h = M.hamilton(torch.tensor(p), torch.tensor(q)).numpy()
    ref = (Rotation.from_quat(p) * Rotation.from_quat(q)).as_quat()
    assert np.abs(h * np.sign((h * ref).sum(1, keepdims=True)) - ref).max() < 1e-14


@pytest.mark.parametrize("name", ["branch", "offset", "tie", "shared"])
def test_gradients_equal_central_differences(name):
    """the fp64 autograd gradients of every input against central differences of the fp64 forward (h = 1e-6 x the input's scale, x the row's norm for the raw rotations;
    bar 1e-6 relative: O(h^2) truncation plus 1e-16 / h cancellation), on a subset of the Gaussians of each case.  Near a tie a step
    can switch the branch and flip the quaternion's sign, so the difference quotient uses the sign-aligned quaternion."""
    c = _cases()[name]
    T = c["deformed"].shape[0]
    keep = np.random.default_rng(5).choice(c["face_ids"].shape[0], size=min(12, c["face_ids"].shape[0]), replace=False)
    sub = dict(c, face_ids=c["face_ids"][keep], bary=c["bary"][keep], rot=c["rot"][keep], w_xyz=c["w_xyz"][:, keep],
               w_quat=c["w_quat"][:, keep])
    sub = {k: (np.asarray(v, np.float64) if k in ("rest", "deformed", "bary", "rot", "w_xyz", "w_quat") else v) for k, v in sub.items()}
    r = M.evaluate(sub)
    q0 = r["quat"]

    def loss(s):
        e = M.evaluate(s, False, False)
        sg = np.sign((e["quat"] * q0).sum(-1, keepdims=True))
        return float((e["xyz"] * s["w_xyz"]).sum() + (e["quat"] * sg * s["w_quat"]).sum())
    vid_used = np.unique(sub["faces"][sub["face_ids"]])
    checks = [("d_vertices", "deformed", [(t, v, k) for t in range(T) for v in vid_used[:6] for k in range(3)]),
              ("d_bary", "bary", [(i, k) for i in range(len(keep)) for k in range(3)]),
              ("d_rotation", "rot", [(i, k) for i in range(len(keep)) for k in range(4)])]
    for gname, key, idxs in checks:
        num, ana = [], []
        for ix in idxs:
            h = 1e-6 * (np.linalg.norm(sub[key][ix[0]]) if key == "rot" else np.abs(sub[key]).max())    # (rot rows: norms 1e-3 .. 1e3)
            sp, sm = dict(sub), dict(sub)
            sp[key], sm[key] = sub[key].copy(), sub[key].copy()
            sp[key][ix] += h
            sm[key][ix] -= h
            num.append((loss(sp) - loss(sm)) / (2 * h))
            ana.append(r[gname][ix])
        num, ana = np.array(num), np.array(ana)
        assert np.abs(num - ana).max() < 1e-6 * np.abs(ana).max(), (name, gname, np.abs(num - ana).max() / np.abs(ana).max())


@pytest.mark.parametrize("name", ["branch", "offset", "tie", "shared"])
def test_every_generator_reaches_every_branch(name):
    c = _cases()[name]
    counts = M.branch_counts(c)
    assert counts.min() >= MIN_PER_BRANCH[name], counts


def test_tie_cases_land_on_both_sides_of_every_boundary():
    """for every tie surface (R_ii = R_jj and R_ii = trace): the fp64 branch on the float32 corners picks each of the two tied formulas for
    at least 5 Gaussians, every nudged Gaussian sits within 2e-6 of its boundary, and the nudges of +-16 ulps on the trace surfaces
    decide the side (rounding the corners moves a decision quantity by about one ulp)."""
    c = M.tie_case(reps=20, T=2, seed=3)
    r = M.evaluate(c, False, False)
    for i, (a, b) in enumerate(M.TIE_PAIRS):
        sel = c["tie_pair"] == i
        br = r["branch"][sel]
        assert np.isin(br, [a, b]).all()
        assert (br == a).sum() >= 5 and (br == b).sum() >= 5, ((a, b), np.bincount(br, minlength=4))
        assert np.abs(r["margin"][sel]).max() < 2e-6
        if b == 3:
            assert (r["branch"][sel & (c["tie_ulps"] == 16)] == a).all() and (r["branch"][sel & (c["tie_ulps"] == -16)] == b).all()


def test_shared_case_has_a_hub_and_unreferenced_vertices():
    c = M.shared_case(T=5, seed=4)
    uses = np.bincount(c["faces"][c["face_ids"]].reshape(-1), minlength=c["rest"].shape[0])
    assert uses.max() >= 300
    assert M.unreferenced(c).sum() >= 16 + 5          # the second grid and the loose vertices
    assert M.face_gaps(c).min() >= M.MIN_GAP


def test_generators_are_deterministic_and_float32():
    a, b = M.branch_case(64, T=2, seed=9), M.branch_case(64, T=2, seed=9)
    for k in ("rest", "deformed", "bary", "rot", "w_xyz", "w_quat"):
        assert a[k].dtype == np.float32 and np.array_equal(a[k], b[k])
    norms = np.linalg.norm(M.branch_case(2000, seed=3)["rot"], axis=1)
    assert norms.min() < 1e-2 and norms.max() > 1e2                 # raw rotations from 1e-3 to 1e3
    bs = M.branch_case(2000, seed=3)["bary"].sum(1)
    assert bs.min() < 0.7 and bs.max() > 1.5                        # rows that do not sum to 1
