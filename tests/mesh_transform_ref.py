"""fp64 restatement of the mesh -> Gaussian transform and the case generators of its edge tests (helper of the mesh-transform tests,
not collected).

What csplat_mesh_transform_* compute (include/csplat.h; the reference's MultiGaussianMesh.get_xyz / get_rotation with roma's
rigid_points_registration, rotmat_to_unitquat and quat_composition), per Gaussian with face corners x_k (rest) and y_k (deformed), a
barycentric row b and a raw rotation r:
    xyz  = sum_k b_k y_k / sum_k b_k
    R    = the Kabsch rotation of the centred rest triangle onto the centred deformed one (SVD with the determinant fix)
    qr   = the unit quaternion of R, XYZW, from the column of Shepperd's 4x4 matrix picked by the largest of (R00, R11, R22, trace),
           the first maximum winning
    quat = (r / |r|) * qr, the Hamilton product in XYZW
Values: `kabsch_svd`.  Gradients: fp64 autograd through `kabsch_closed`, the same rotation written as the polar factor of the 2x2
in-plane covariance (angles by atan2); test_mesh_transform_cpu.py pins it to kabsch_svd, to scipy and to central differences.

Every generator returns a dict: rest [V,3], deformed [T,V,3] (float32 values), faces [F,3], face_ids [P], bary [P,3], rot [P,4],
w_xyz [T,P,3], w_quat [T,P,4] (loss weights), and asserts that its faces are far from degenerate (`MIN_GAP`)."""
import numpy as np
import torch

F64 = torch.float64
MIN_GAP = 0.05      # every face, rest and deformed: second singular value of the centred corners >= MIN_GAP x the first
KINDS = ("x180", "y180", "z180", "small", "random")     # the rigid rotations of branch_case, in turn


# ---------------------------------------------------------------- the operation
def _centred(p):
    return p - p.mean(dim=-2, keepdim=True)


def kabsch_svd(x, y):
    """x, y [N,3,3] (rows = corners) -> R [N,3,3]"""
    H = torch.einsum("nki,nkj->nij", _centred(y), _centred(x))
    U, _, Vh = torch.linalg.svd(H)
    d = torch.where(torch.linalg.det(U @ Vh) < 0, -1.0, 1.0).to(H.dtype)
    fix = torch.stack([torch.ones_like(d), torch.ones_like(d), d], -1)
    return (U * fix.unsqueeze(-2)) @ Vh


def _frame(p):
    """right-handed orthonormal frame of the triangles p [N,3,3] as columns (first edge, in-plane normal of it, face normal)"""
    e = p[:, 1] - p[:, 0]
    nz = torch.linalg.cross(e, p[:, 2] - p[:, 0], dim=-1)
    e = e / e.norm(dim=-1, keepdim=True)
    nz = nz / nz.norm(dim=-1, keepdim=True)
    return torch.stack([e, torch.linalg.cross(nz, e, dim=-1), nz], -1)


def kabsch_closed(x, y):
    """kabsch_svd's rotation without an SVD: with frames Fx, Fy of the two triangles and M the 2x2 covariance of their in-plane
    coordinates, R = Fy diag(Q, det Q) Fx^T where Q is M's orthogonal polar factor -- the rotation by atan2(M10 - M01, M00 + M11)
    when det M > 0, the reflection [[c, s], [s, -c]] at atan2(M10 + M01, M00 - M11) when det M < 0."""
    Fx, Fy = _frame(x), _frame(y)
    px = _centred(x) @ Fx[..., :2]
    py = _centred(y) @ Fy[..., :2]
    M = torch.einsum("nki,nkj->nij", py, px)
    proper = M[:, 0, 0] * M[:, 1, 1] - M[:, 0, 1] * M[:, 1, 0] > 0
    th = torch.where(proper, torch.atan2(M[:, 1, 0] - M[:, 0, 1], M[:, 0, 0] + M[:, 1, 1]),
                     torch.atan2(M[:, 1, 0] + M[:, 0, 1], M[:, 0, 0] - M[:, 1, 1]))
    c, s = torch.cos(th), torch.sin(th)
    sg = torch.where(proper, 1.0, -1.0).to(M.dtype)
    z = torch.zeros_like(c)
    Z = torch.stack([c, -sg * s, z, s, sg * c, z, z, z, sg], -1).reshape(-1, 3, 3)
    return Fy @ Z @ Fx.transpose(-1, -2)


def decision(R):
    """[N,3,3] -> [N,4]: the quantities whose largest picks the quaternion formula (R00, R11, R22, trace)"""
    d = torch.diagonal(R, dim1=-2, dim2=-1)
    return torch.cat([d, d.sum(-1, keepdim=True)], -1)


def branch_and_margin(R):
    """-> (branch [N] int64: first index of the largest decision quantity, margin [N]: largest minus second largest)"""
    dec = decision(R).detach()
    top = dec.max(-1, keepdim=True).values
    branch = (dec == top).to(torch.int64).argmax(-1)
    srt = dec.sort(-1, descending=True).values
    return branch, srt[:, 0] - srt[:, 1]


def rotmat_to_quat(R):
    """[N,3,3] -> XYZW [N,4]: column `branch` of Shepperd's symmetric matrix K (K = 4 q q^T for the unit quaternion q of R),
    normalised"""
    r = lambda i, j: R[:, i, j]  # noqa: E731
    one = torch.ones_like(r(0, 0))
    K = torch.stack([
        one + r(0, 0) - r(1, 1) - r(2, 2), r(0, 1) + r(1, 0), r(0, 2) + r(2, 0), r(2, 1) - r(1, 2),
        r(0, 1) + r(1, 0), one - r(0, 0) + r(1, 1) - r(2, 2), r(1, 2) + r(2, 1), r(0, 2) - r(2, 0),
        r(0, 2) + r(2, 0), r(1, 2) + r(2, 1), one - r(0, 0) - r(1, 1) + r(2, 2), r(1, 0) - r(0, 1),
        r(2, 1) - r(1, 2), r(0, 2) - r(2, 0), r(1, 0) - r(0, 1), one + r(0, 0) + r(1, 1) + r(2, 2)], -1).reshape(-1, 4, 4)
    b, _ = branch_and_margin(R)
    col = K.gather(2, b.view(-1, 1, 1).expand(-1, 4, 1)).squeeze(-1)
    return col / col.norm(dim=-1, keepdim=True)


def hamilton(p, q):
    """XYZW Hamilton product p * q as L(p) q"""
    x, y, z, w = p.unbind(-1)
    L = torch.stack([w, -z, y, x, z, w, -x, y, -y, x, w, z, -x, -y, -z, w], -1).reshape(*p.shape[:-1], 4, 4)
    return (L @ q.unsqueeze(-1)).squeeze(-1)


def transform(rest, verts, vid, bary, rot, kabsch=kabsch_closed):
    """one camera: rest [V,3], verts [V,3], vid [P,3] int64, bary [P,3], rot [P,4] -> dict(xyz, quat, R, branch, margin)"""
    x, y = rest[vid], verts[vid]
    xyz = (bary.unsqueeze(-1) * y).sum(1) / bary.sum(1, keepdim=True)
    R = kabsch(x, y)
    quat = hamilton(rot / rot.norm(dim=-1, keepdim=True), rotmat_to_quat(R))
    branch, margin = branch_and_margin(R)
    return dict(xyz=xyz, quat=quat, R=R, branch=branch, margin=margin)


def evaluate(case, w_xyz=True, w_quat=True, dtype=F64, quat_sign=None, kabsch=kabsch_closed):
    """the whole case in `dtype`: values of every camera and the gradients of
        L = sum_t <xyz_t, w_xyz_t> + <quat_t, s_t * w_quat_t>
    (w_* False: that term left out; s = quat_sign [T,P] or 1) w.r.t. the deformed vertices [T,V,3], bary [P,3] and rot [P,4]."""
    t = lambda a: torch.tensor(np.asarray(a), dtype=dtype)  # noqa: E731
    vid = torch.tensor(case["faces"][case["face_ids"]], dtype=torch.int64).reshape(-1, 3)
    rest, verts = t(case["rest"]), t(case["deformed"]).requires_grad_(True)
    bary, rot = t(case["bary"]).requires_grad_(True), t(case["rot"]).requires_grad_(True)
    outs = [transform(rest, verts[i], vid, bary, rot, kabsch) for i in range(verts.shape[0])]
    xyz = torch.stack([o["xyz"] for o in outs])
    quat = torch.stack([o["quat"] for o in outs])
    loss = torch.zeros((), dtype=dtype)
    if w_xyz:
        loss = loss + (xyz * t(case["w_xyz"])).sum()
    if w_quat:
        wq = t(case["w_quat"])
        if quat_sign is not None:
            wq = wq * t(quat_sign).unsqueeze(-1)
        loss = loss + (quat * wq).sum()
    res = dict(xyz=xyz.detach().numpy(), quat=quat.detach().numpy(), branch=torch.stack([o["branch"] for o in outs]).numpy(),
               margin=torch.stack([o["margin"] for o in outs]).numpy(), R=torch.stack([o["R"] for o in outs]).detach().numpy())
    if (w_xyz or w_quat) and loss.requires_grad:
        gv, gb, gr = torch.autograd.grad(loss, (verts, bary, rot), allow_unused=True)
        z = lambda g, like: np.zeros(like.shape) if g is None else g.numpy()  # noqa: E731
        res.update(d_vertices=z(gv, verts), d_bary=z(gb, bary), d_rotation=z(gr, rot))
    return res


def branch_counts(case):
    """Gaussians per branch [4], over all cameras of the case (fp64, on the float32 inputs)"""
    return np.bincount(evaluate(case, False, False)["branch"].reshape(-1), minlength=4)


def face_gaps(case):
    """second over first singular value of every face's centred corners, rest and every camera: [1 + T, F]"""
    f = torch.tensor(case["faces"], dtype=torch.int64)
    out = []
    for pts in [case["rest"]] + list(case["deformed"]):
        S = torch.linalg.svdvals(_centred(torch.tensor(np.asarray(pts, np.float64))[f]))
        out.append((S[:, 1] / S[:, 0]).numpy())
    return np.stack(out)


# ---------------------------------------------------------------- the cases
def quat_to_rotmat(q):
    """unit XYZW [N,4] (numpy, fp64) -> [N,3,3]"""
    x, y, z, w = q.T
    return np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                     2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                     2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], -1).reshape(-1, 3, 3)


def _axis_angle(axis, angle):
    axis = axis / np.linalg.norm(axis, axis=-1, keepdims=True)
    return quat_to_rotmat(np.concatenate([axis * np.sin(angle / 2)[:, None], np.cos(angle / 2)[:, None]], -1))


def _rotations(kind, n, rng):
    """n rigid rotations of one KINDS entry: 180 +- 20 degrees about an axis within 0.2 rad of x / y / z, up to 50 degrees about
    any axis, uniform on SO(3)"""
    if kind == "random":
        q = rng.normal(size=(n, 4))
        return quat_to_rotmat(q / np.linalg.norm(q, axis=1, keepdims=True))
    if kind == "small":
        return _axis_angle(rng.normal(size=(n, 3)), rng.uniform(0, np.radians(50), n))
    axis = np.zeros((n, 3))
    axis[:, "xyz".index(kind[0])] = 1.0
    axis += 0.2 * rng.uniform(-1, 1, (n, 3))
    return _axis_angle(axis, np.pi + rng.uniform(-1, 1, n) * np.radians(20))


def _triangles(n, rng, size):
    """n well-shaped rest triangles [n,3,3], centred at 0, edge lengths ~size, random orientation"""
    ang = np.array([0.0, 2 * np.pi / 3, 4 * np.pi / 3])[None] + rng.uniform(-0.35, 0.35, (n, 3))
    rad = rng.uniform(0.6, 1.0, (n, 3))
    tri = np.stack([rad * np.cos(ang), rad * np.sin(ang), np.zeros((n, 3))], -1) * size
    return _centred(torch.tensor(tri)).numpy() @ _rotations("random", n, rng).transpose(0, 2, 1)


def _gaussians(case, P, rng, face_ids=None, rot_norms=(1e-3, 1e3)):
    """the per-Gaussian rows of a case: faces picked at random (or given), barycentric rows in (0.02, 1] scaled by 0.5 .. 2 (so that they
    do not sum to 1), raw rotations with norms log-uniform in rot_norms, unit-normal loss weights"""
    F, T = case["faces"].shape[0], case["deformed"].shape[0]
    case["face_ids"] = (rng.integers(0, F, P) if face_ids is None else np.asarray(face_ids)).astype(np.int64)
    b = rng.uniform(0.02, 1.0, (P, 3))
    case["bary"] = (b / b.sum(1, keepdims=True) * rng.uniform(0.5, 2.0, (P, 1))).astype(np.float32)
    r = rng.normal(size=(P, 4))
    r *= np.exp(rng.uniform(np.log(rot_norms[0]), np.log(rot_norms[1]), (P, 1))) / np.linalg.norm(r, axis=1, keepdims=True)
    case["rot"] = r.astype(np.float32)
    case["w_xyz"] = rng.normal(size=(T, P, 3)).astype(np.float32)
    case["w_quat"] = rng.normal(size=(T, P, 4)).astype(np.float32)
    case["rest"] = np.asarray(case["rest"], np.float32)
    case["deformed"] = np.asarray(case["deformed"], np.float32)
    gaps = face_gaps(case)
    assert gaps.min() >= MIN_GAP, f"a face of the case is near-degenerate: singular-value ratio {gaps.min():.3g}"
    return case


def branch_case(P, T=1, seed=0, size=1.0, offset=0.0, noise=0.02):
    """a triangle soup (every face has its own three vertices, P // 2 faces, two Gaussians per face on average) whose faces camera t
    turns by a rigid rotation of KINDS[(f + t) % 5] -- 180 degrees about x, y or z (branches 0, 1, 2), a small or a uniform rotation --
    moves to a random place within `offset` of the origin, and disturbs by `noise` x size (non-rigid).  size ~ 1e-2 with offset ~ 1 is the
    small-faces-far-out case."""
    rng = np.random.default_rng(seed)
    F = max(P // 2, 1)
    rest = _triangles(F, rng, size) + rng.uniform(-1, 1, (F, 1, 3)) * offset
    deformed = []
    for t in range(T):
        R = np.empty((F, 3, 3))
        for k, kind in enumerate(KINDS):
            sel = (np.arange(F) + t) % len(KINDS) == k
            R[sel] = _rotations(kind, int(sel.sum()), rng)
        y = _centred(torch.tensor(rest)).numpy() @ R.transpose(0, 2, 1) + rng.uniform(-1, 1, (F, 1, 3)) * offset
        deformed.append((y + noise * size * rng.uniform(-1, 1, y.shape)).reshape(-1, 3))
    case = dict(rest=rest.reshape(-1, 3), deformed=np.stack(deformed), faces=np.arange(3 * F).reshape(F, 3))
    return _gaussians(case, P, rng)


TIE_PAIRS = ((0, 1), (0, 2), (1, 2), (0, 3), (1, 3), (2, 3))     # decision quantities made equal: R_ii = R_jj, R_ii = trace
TIE_ULPS = (-16, -4, -2, -1, 0, 1, 2, 4, 16)                       # the signed margin between them, in float32 ulps of their value


def tie_quaternions(pair, ulps, rng):
    """unit quaternions (XYZW, fp64) whose rotation has decision quantities `pair` the two largest and `ulps` float32 ulps apart
    (decision[a] - decision[b]).  With q_3 = w, R_ii = 2 (q_i^2 + w^2) - 1 and trace = 4 w^2 - 1, so decision[a] - decision[b] =
    2 (q_a^2 - q_b^2): q_a^2 + q_b^2 = 1 - rr^2 with the other two components of norm rr < 0.5, and q_a^2 - q_b^2 = margin / 2."""
    ulps = np.asarray(ulps, np.float64)
    n = ulps.shape[0]
    a, b = pair
    rest_idx = [i for i in range(4) if i not in pair]
    q = np.zeros((n, 4))
    uv = rng.normal(size=(n, 2))
    uv *= rng.uniform(0.0, 0.5, (n, 1)) / np.linalg.norm(uv, axis=1, keepdims=True)
    q[:, rest_idx] = uv
    S = 1.0 - (uv ** 2).sum(1)
    for _ in range(2):      # the ulp is that of the tied value, which depends (weakly) on the margin itself
        qa2 = S / 2
        probe = q.copy()
        probe[:, a], probe[:, b] = np.sqrt(qa2), np.sqrt(S - qa2)
        dec = np.concatenate([np.diagonal(quat_to_rotmat(probe), axis1=1, axis2=2),
                              np.trace(quat_to_rotmat(probe), axis1=1, axis2=2)[:, None]], 1)
        ulp = np.spacing(np.abs(dec[:, a]).astype(np.float32)).astype(np.float64)
    margin = ulps * ulp
    q[:, a] = np.sqrt(S / 2 + margin / 4) * rng.choice([-1.0, 1.0], n)
    q[:, b] = np.sqrt(S / 2 - margin / 4) * rng.choice([-1.0, 1.0], n)
    return q


def tie_case(reps=20, T=1, seed=0):
    """a triangle soup of rigid copies of unit-size rest faces (no offset, so that rounding the corners to float32 moves the decision
    quantities by about one ulp): face f of camera t is turned by a rotation on the tie surface TIE_PAIRS[.] nudged by TIE_ULPS[.]; every
    (pair, ulps) combination appears `reps` times per camera.  One Gaussian per face."""
    rng = np.random.default_rng(seed)
    combos = [(p, u) for p in TIE_PAIRS for u in TIE_ULPS] * reps
    F = len(combos)
    rest = _triangles(F, rng, 1.0)
    deformed, pairs, ulps = [], [], []
    for t in range(T):
        R = np.empty((F, 3, 3))
        order = rng.permutation(F)        # face f of camera t: combos[order[f]]
        for pair in TIE_PAIRS:
            sel = np.array([combos[i][0] == pair for i in order])
            R[sel] = quat_to_rotmat(tie_quaternions(pair, [combos[i][1] for i in order[sel]], rng))
        deformed.append((rest @ R.transpose(0, 2, 1)).reshape(-1, 3))
        pairs.append([TIE_PAIRS.index(combos[i][0]) for i in order])
        ulps.append([combos[i][1] for i in order])
    case = dict(rest=rest.reshape(-1, 3), deformed=np.stack(deformed), faces=np.arange(3 * F).reshape(F, 3),
                tie_pair=np.array(pairs), tie_ulps=np.array(ulps))     # [T, P]: index into TIE_PAIRS, the nudge in ulps
    return _gaussians(case, F, rng, face_ids=np.arange(F))


def grid_mesh(n, size=1.0):
    """an n x n vertex grid in the z = 0 plane, two triangles per cell: (pos [n*n, 3], faces [2 (n-1)^2, 3])"""
    xs = np.linspace(-size / 2, size / 2, n)
    pos = np.stack([np.tile(xs, n), np.repeat(xs, n), np.zeros(n * n)], 1)
    c = (np.arange(n - 1)[None] + n * np.arange(n - 1)[:, None]).reshape(-1)
    faces = np.concatenate([np.stack([c, c + 1, c + n], 1), np.stack([c + 1, c + n + 1, c + n], 1)])
    return pos, faces


def _cloth_deform(pos, T, rng, amp=0.05, noise=0.002):
    """camera t: a smooth wave, vertex noise, then the whole mesh turned by a rotation of KINDS[t % 5] and moved"""
    out = []
    for t in range(T):
        p = pos.copy()
        p[:, 2] += amp * np.sin(3 * pos[:, 0] + t) * np.cos(2 * pos[:, 1])
        p += noise * rng.normal(size=p.shape)
        R = _rotations(KINDS[t % len(KINDS)], 1, rng)[0]
        out.append(p @ R.T + rng.uniform(-0.5, 0.5, 3))
    return np.stack(out)


def shared_case(T=5, seed=0, hub_gaussians=300, n=8):
    """a cloth grid plus a fan of 12 faces around one hub vertex carrying `hub_gaussians` Gaussians (the hub is a corner of every one of
    them), a second grid part with no Gaussian, and 5 vertices in no face; the other Gaussians sit on the first grid's faces.  Camera t
    turns the whole mesh by a rotation of KINDS[t % 5] (so T >= 4 covers the four branches).  unreferenced(case) lists the vertices no
    Gaussian touches."""
    rng = np.random.default_rng(seed)
    pos, faces = grid_mesh(n)
    ang = np.linspace(0, 2 * np.pi, 13)[:-1]
    hub = np.concatenate([[[0.0, 0.0, 0.3]], np.stack([0.2 * np.cos(ang), 0.2 * np.sin(ang), 0.3 + 0.03 * np.sin(3 * ang)], 1)])
    V0 = pos.shape[0]
    fan = np.stack([np.full(12, V0), V0 + 1 + np.arange(12), V0 + 1 + (np.arange(12) + 1) % 12], 1)
    pos2, faces2 = grid_mesh(4, 0.3)
    pos2[:, 2] -= 0.4
    loose = rng.uniform(-1, 1, (5, 3))
    V1 = V0 + hub.shape[0]
    all_pos = np.concatenate([pos, hub, pos2, loose])
    all_faces = np.concatenate([faces, fan, faces2 + V1])
    n_grid = faces.shape[0]
    ids = np.concatenate([rng.integers(0, n_grid, 3 * n_grid), n_grid + rng.integers(0, 12, hub_gaussians)])
    case = dict(rest=all_pos, deformed=_cloth_deform(all_pos, T, rng), faces=all_faces)
    return _gaussians(case, ids.shape[0], rng, face_ids=rng.permutation(ids))


def unreferenced(case):
    """bool [V]: vertices that are a corner of no Gaussian's face"""
    used = np.zeros(case["rest"].shape[0], bool)
    used[case["faces"][case["face_ids"]].reshape(-1)] = True
    return ~used


def bench_case(T=1, seed=0, n=100, P=100_000):
    """the train-step benchmark's size: a 100 x 100 grid (10 000 vertices, 19 602 faces) and 100 000 Gaussians"""
    rng = np.random.default_rng(seed)
    pos, faces = grid_mesh(n)
    case = dict(rest=pos, deformed=_cloth_deform(pos, T, rng, amp=0.02, noise=0.001), faces=faces)
    return _gaussians(case, P, rng)
