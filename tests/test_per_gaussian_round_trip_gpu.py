"""The two per-Gaussian streaming kernels of the batched rasterizer, K1 (k_preprocess_views, csrc/csplat_raster_k1.h) and K8
(k_preprocess_bwd_views*, csrc/csplat_k8_views_body.h), request all of a wave's global loads at the top, visible or not.  What they compute
must not have moved by a bit:

  - tests/golden/per_gaussian_parent.npz (tests/golden/make_per_gaussian_parent.py) holds, from the library of the commit before the load
    order changed, every per-Gaussian scratch field K1 writes and -- with the compositing backward in its bit-reproducible mode
    (csplat_debug_flags 256) -- every gradient K8 writes, for the scene of `scene()` below: P = 161 (5 x 32 + 1 Gaussians for K8's
    workgroups, 2 x 64 + 33 for K1's), 64 x 64 images, SH degree 3, V in {1, 2, 3, 4, 5, 8}, shared and per-view means3D / rotations, and the
    antialiased, depth and camera kernels at V = 4 and V = 5.  Every eighth Gaussian stands behind all cameras, view 1 looks away from the
    cloth (everything culled), view 2 stands close (part of the cloth outside its frustum), and three culled Gaussians sit at a camera
    centre, behind the cameras and 1e30 away.  Float arrays are kept as their bits; the SH gradient ([P, 48] per case, by far the largest
    output) as one CRC-32 per Gaussian row, and in full for the four-view case.  The test asserts bit equality, and that a culled
    (Gaussian, view) leaves exact zeros and nothing that is not finite.
  - P at the edges of the workgroups (1, 31, 32, 33, 63, 64, 65) at V in {1, 4, 5}: against the per-view K8 launches and fp64 autograd, the
    two bars of tests/test_k8_views_gpu.py.
  - a P = 161 call, a P = 33 call and the P = 161 call again in one process: the two P = 161 results are bit-equal (nothing a lane past P
    or a lane without a view requested reaches a result)."""
import ctypes as C
import os
import zlib

import numpy as np
import pytest

import util
import antialias_ref
from util import oracle_forward, rel_err

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

FIXTURE = os.path.join(util.GOLDEN, "per_gaussian_parent.npz")
P0, W, H = 161, 64, 64
NV = 8
TURNED, CLOSE = 1, 2                    # view 1 looks away from the cloth, view 2 stands close to it
AT_CENTRE, BEHIND, FAR = 0, 77, 131     # the three hostile Gaussians
TOL = 1e-4                              # against fp64 (tests/test_k8_views_gpu.py: TOL)
TOL_K8 = 1e-6                           # batched against per-view K8 (tests/test_k8_views_gpu.py: TOL_K8)
CAM_KEYS = ("view", "proj", "campos", "bg")
K1_FIELDS = ("depth", "xy", "conic_opacity", "rgb", "cov3D", "clamped", "tiles_touched")
VARIANTS = dict(default={}, aa=dict(aa=True), depth=dict(depth=True), cam=dict(cam=True))


def _flags(f):
    from csplat import native
    native.lib.csplat_debug_flags(f)


def _axis():
    """the axis the cameras of syn.make_camera circle around, pointing to their side of the cloth"""
    a = util.syn.make_camera(0.0, W, H)["camera_center"].astype(np.float64) + util.syn.make_camera(180.0, W, H)["camera_center"]
    return a / np.linalg.norm(a)


def _turn_away(cam):
    """the same camera after half a turn about its own vertical axis: same centre, everything in front of it now behind"""
    syn = util.syn
    wv = cam["world_view_transform"].astype(np.float64) @ np.diag([-1.0, 1.0, -1.0, 1.0])
    pr = syn.projection_matrix(syn.ZNEAR, syn.ZFAR, cam["FoVx"], cam["FoVy"]).transpose().astype(np.float64)
    return dict(cam, world_view_transform=np.ascontiguousarray(wv, np.float32), full_proj_transform=np.ascontiguousarray(wv @ pr, np.float32))


def scene(V, P=P0, own=False):
    """-> (cases, weights): V views of one cloth of P Gaussians.  own: every view has its own means3D / rotations."""
    up = _axis()
    cases = []
    for i in range(V):
        c = util.make_case(P=P, W=W, H=H, seed=11, grid=6, scale_mul=3.0, theta=-60.0 + 17.0 * i, radius=1.2 if i == CLOSE else 4.0)
        if i == TURNED:
            c["cam"] = _turn_away(c["cam"])
        cases.append(c)
    base = cases[0]["g"]
    for i, c in enumerate(cases):
        if i and not own:
            c["g"] = cases[0]["g"]                           # one set of Gaussians for every view
            continue
        g = c["g"] = dict(base)
        m = np.array(base["means3D"], np.float64)
        if own:
            m = m + 0.001 * i
            g["rotations"] = (base["rotations"] * (1.0 + 0.01 * i)).astype(np.float32)
        m[5::8] += 50.0 * up                                 # behind every camera
        if P == P0:
            m[AT_CENTRE] = c["cam"]["camera_center"]         # (shared means: view 0's centre)
            m[BEHIND] = 50.0 * up
            m[FAR] = -1e30 * up
        g["means3D"] = m.astype(np.float32)
    rng = np.random.default_rng(21)
    wts = [dict(color=rng.normal(size=(3, H, W)), depth=rng.normal(size=(1, H, W))) for _ in range(V)]
    return cases, wts


def _cut2(view, P):
    """the culling radius K1 leaves behind `offsets` in the GEOM chunk, and the 48-byte pack records at its end (csrc: geom_offsets; every
    field is padded to 256 bytes), as bits"""
    from csplat import native as n
    a256 = lambda b: (b + 255) // 256 * 256  # noqa: E731
    o8 = (C.c_size_t * 8)(); n.lib.csplat_geom_layout(P, o8)
    n.lib.csplat_geom_bytes.restype = C.c_size_t
    geom = view.chunks[0].cpu().numpy().tobytes()
    total = int(n.lib.csplat_geom_bytes(P))
    cut2 = np.frombuffer(geom[o8[7] + a256(4 * P):o8[7] + a256(4 * P) + 4 * P], np.uint32)
    pack = np.frombuffer(geom[total - a256(48 * P):total - a256(48 * P) + 48 * P], np.uint32).reshape(P, 12)
    return cut2, pack


def step(cases, wts, own, depth=False, cam=False, aa=False, flags=256):
    """one rasterize_views step under csplat_debug_flags(flags) -> (K1's fields per view as bits, {gradient name: float32 array})"""
    import diff_gaussian_rasterization as dgr
    V, P = len(cases), cases[0]["P"]
    T = lambda a: torch.tensor(np.asarray(a, np.float32), device="cuda", requires_grad=True)  # noqa: E731
    t = lambda a: torch.tensor(np.asarray(a, np.float32), device="cuda")  # noqa: E731
    _flags(flags)
    try:
        inp = util.gpu_inputs(cases[0])
        means = [T(c["g"]["means3D"]) for c in cases] if own else [inp["means3D"]] * V
        rots = [T(c["g"]["rotations"]) for c in cases] if own else [inp["rotations"]] * V
        m2d = [torch.zeros(P, 3, device="cuda", requires_grad=True) for _ in range(V)]
        settings, leaves = [], []
        for c in cases:
            rs = util.gpu_settings(c)
            if cam:
                k = c["cam"]
                lv = dict(view=T(k["world_view_transform"]), proj=T(k["full_proj_transform"]), campos=T(k["camera_center"]), bg=T(c["bg"]))
                rs = rs._replace(viewmatrix=lv["view"], projmatrix=lv["proj"], campos=lv["campos"], bg=lv["bg"])
                leaves.append(lv)
            settings.append(rs)
        kws = [dict(means3D=means[i], means2D=m2d[i], opacities=inp["opacities"], shs=inp["shs"], scales=inp["scales"], rotations=rots[i],
                    antialiasing=aa) for i in range(V)]
        outs = dgr.rasterize_views(settings, kws)
        torch.cuda.synchronize()
        k1 = []
        for i, v in enumerate(outs[0][0].grad_fn.views):
            st = util.gpu_chunks(v.chunks, P, W, H, int(v.layout_rendered))
            f = {k: st[k].view(np.uint32).reshape(P, -1) for k in K1_FIELDS}
            f["radii"] = outs[i][1].cpu().numpy().astype(np.int32).reshape(P, 1)
            cut2, pack = _cut2(v, P)
            f["cut2"] = cut2.reshape(P, 1)
            # the pack record repeats (x, y, conic a, b | conic c, opacity, r, g | b, depth, cut2, 0): checked here, not recorded
            rebuilt = np.concatenate([f["xy"], f["conic_opacity"], f["rgb"], f["depth"], f["cut2"], np.zeros((P, 1), np.uint32)], 1)
            assert np.array_equal(pack, rebuilt), "view %d: the pack records differ from the fields they repeat" % i
            k1.append(f)
        loss = sum((outs[i][0] * t(wts[i]["color"])).sum() for i in range(V))
        if depth:
            loss = loss + sum((outs[i][2] * t(wts[i]["depth"])).sum() for i in range(V) if i != 3)      # (view 3 has no depth gradient)
        loss.backward()
        torch.cuda.synchronize()
    finally:
        _flags(0)
    got = dict(opacity=inp["opacities"].grad.reshape(P, 1), sh=inp["shs"].grad.reshape(P, 48), scale=inp["scales"].grad)
    for i in range(V):
        got["mean2D_%d" % i] = m2d[i].grad
        if own:
            got["mean3D_%d" % i], got["rot_%d" % i] = means[i].grad, rots[i].grad
        if cam:
            got.update({"%s_%d" % (k, i): leaves[i][k].grad.reshape(1, -1) for k in CAM_KEYS})
    if not own:
        got["mean3D"], got["rot"] = inp["means3D"].grad, inp["rotations"].grad
    return k1, {k: v.detach().cpu().numpy() for k, v in got.items()}


def reference(cases, wts, own, depth=False, cam=False, aa=False):
    """the same step in fp64 autograd (tests/antialias_ref.py)"""
    V, P = len(cases), cases[0]["P"]
    T = lambda a: torch.tensor(np.asarray(a, np.float64), requires_grad=True)  # noqa: E731
    g0 = cases[0]["g"]
    op, sh, sc = T(g0["opacities"]), T(g0["shs"]), T(g0["scales"])
    means = [T(c["g"]["means3D"]) for c in cases] if own else [T(g0["means3D"])] * V
    rots = [T(c["g"]["rotations"]) for c in cases] if own else [T(g0["rotations"])] * V
    m2d = [T(np.zeros((P, 3))) for _ in range(V)]
    loss, cams = 0.0, []
    for i, c in enumerate(cases):
        o = oracle_forward(c, dtype=np.float64)
        lv = dict(zip(CAM_KEYS, antialias_ref.camera_tensors(o)))
        cams.append(lv)
        color, dimg = antialias_ref.render(o, means[i], m2d[i], op, lv["view"], lv["proj"], lv["campos"], lv["bg"], shs=sh, scales=sc,
                                           rotations=rots[i], antialiasing=aa)[:2]
        loss = loss + (color * torch.tensor(wts[i]["color"])).sum()
        if depth and i != 3:
            loss = loss + (dimg * torch.tensor(wts[i]["depth"])).sum()
    loss.backward()
    G = lambda x: x.grad if x.grad is not None else torch.zeros_like(x)  # noqa: E731  (a leaf no visible Gaussian of any view reached)
    ref = dict(opacity=G(op).reshape(P, 1), sh=G(sh).reshape(P, 48), scale=G(sc))
    for i in range(V):
        ref["mean2D_%d" % i] = G(m2d[i])
        if own:
            ref["mean3D_%d" % i], ref["rot_%d" % i] = G(means[i]), G(rots[i])
        if cam:
            ref.update({"%s_%d" % (k, i): G(cams[i][k]).reshape(1, -1) for k in CAM_KEYS})
    if not own:
        ref["mean3D"], ref["rot"] = G(means[0]), G(rots[0])
    return {k: v.numpy() for k, v in ref.items()}


def cases_recorded():
    """(name, V, own, variant) of every recorded case"""
    out = [("default_V%d_%s" % (V, "own" if own else "shared"), V, own, "default") for V in (1, 2, 3, 4, 5, 8) for own in (False, True)]
    out += [("%s_V%d_%s" % (var, V, "own" if own else "shared"), V, own, var) for var in ("aa", "depth", "cam")
            for V, own in ((4, False), (5, True))]
    return out


def row_crc(a):
    """one CRC-32 per row of the array's bits"""
    a = np.ascontiguousarray(a)
    return np.array([zlib.crc32(r.tobytes()) for r in a.reshape(a.shape[0], -1)], np.uint32)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32) if a.dtype == np.float32 else a


def k1_key(own, aa, i, field):
    """K1's output for view i depends on the view, on whose means it reads and on antialiasing, not on V or on the backward's variant: one
    record per (means, antialiasing, view), which every case with that view is held to"""
    return "k1/%s/%s/%d/%s" % ("own" if own else "shared", "aa" if aa else "plain", i, field)


def check_scene_properties(k1_views):
    """what the scene promises, on the radii of one call's views (V = 8)"""
    vis = np.stack([f["radii"][:, 0] > 0 for f in k1_views])               # [V, P]
    assert not vis[TURNED].any(), "the turned-away view sees something"
    assert not vis[:, [AT_CENTRE, BEHIND, FAR]].any() and not vis[:, 5::8].any(), "a Gaussian meant to be culled is visible"
    for v in range(len(k1_views)):
        if v == TURNED:
            continue
        for G in (32, 64):                      # K8's and K1's workgroups
            for lo in range(0, P0 - 1, G):      # (the last Gaussian is a workgroup of its own in both)
                w = vis[v, lo:min(lo + G, P0)]
                assert w.any() and not w.all(), ("view %d Gaussians %d..: not a mix of visible and culled" % (v, lo))
    quad = vis[:4]                              # a quad of K8 lanes = one Gaussian in views 0..3
    assert (quad.any(0) & ~quad.all(0)).any(), "no Gaussian is visible in one of the first four views and culled in another"
    part = vis[CLOSE] != vis[0]
    assert part[np.arange(P0) % 8 != 5].any(), "the close view culls nothing of the cloth"


# ------------------------------------------------------------------------------------------------ against the recorded parent
@pytest.fixture(scope="module")
def parent():
    return dict(np.load(FIXTURE))


@pytest.mark.parametrize("name,V,own,variant", cases_recorded(), ids=[c[0] for c in cases_recorded()])
def test_bit_equal_to_the_parent(parent, name, V, own, variant):
    kw = VARIANTS[variant]
    cases, wts = scene(V, own=own)
    k1, got = step(cases, wts, own, **kw)
    if V == NV:
        check_scene_properties(k1)
    aa = bool(kw.get("aa"))
    for i, f in enumerate(k1):
        for k, a in f.items():
            want = parent[k1_key(own, aa, i, k)]
            bad = np.nonzero((a != want).any(1))[0]
            assert bad.size == 0, "%s: K1 field %s of view %d differs from the parent at Gaussians %s" % (name, k, i, bad[:8])
        culled = f["radii"][:, 0] == 0
        assert culled[[AT_CENTRE, BEHIND, FAR]].all() and culled[5::8].all(), (name, i)
        for k in ("depth", "xy", "conic_opacity", "rgb", "clamped", "tiles_touched"):       # (cov3D is written before the culling tests)
            assert not f[k][culled].any(), "%s: K1 field %s of view %d is not zero for a culled Gaussian" % (name, k, i)
        for k in ("depth", "xy", "conic_opacity", "rgb", "cov3D"):
            assert np.isfinite(f[k].view(np.float32)[~culled]).all(), (name, i, k)
    vis = np.stack([f["radii"][:, 0] > 0 for f in k1])
    for k, a in got.items():
        assert a.dtype == np.float32
        assert np.isfinite(a).all(), "%s: %s holds a value that is not finite" % (name, k)
        if k == "sh":
            bad = np.nonzero(row_crc(a) != parent["k8/%s/sh_crc" % name])[0]
            if "k8/%s/sh" % name in parent:
                assert np.array_equal(bits(a), parent["k8/%s/sh" % name]), (name, k)
        else:
            bad = np.nonzero((bits(a) != parent["k8/%s/%s" % (name, k)]).reshape(a.shape[0], -1).any(1))[0]
        assert bad.size == 0, "%s: %s differs from the parent in rows %s" % (name, k, bad[:8])
        if k.split("_")[0] in CAM_KEYS:
            continue
        view = int(k.split("_")[1]) if "_" in k else None
        culled = ~vis[view] if view is not None else ~vis.any(0)      # a shared gradient: culled in every view
        assert (a[culled] == 0).all(), "%s: %s is not exactly zero for a culled Gaussian" % (name, k)
    if kw.get("cam"):
        for k in ("view", "proj", "campos"):       # nothing of the turned-away view reaches its camera
            assert (got["%s_%d" % (k, TURNED)] == 0).all(), (name, k)


# ------------------------------------------------------------------------------------------------ P at the workgroups' edges
@pytest.mark.parametrize("V", [1, 4, 5])
@pytest.mark.parametrize("P", [1, 31, 32, 33, 63, 64, 65])
def test_p_edges_against_per_view_k8_and_fp64(P, V):
    cases, wts = scene(V, P=P)
    _, one = step(cases, wts, False, flags=256)
    _, per_view = step(cases, wts, False, flags=256 | 128)
    ref = reference(cases, wts, False)
    assert one.keys() == per_view.keys() == ref.keys()
    for k in one:
        assert np.isfinite(one[k]).all(), k
        e = rel_err(one[k], per_view[k])
        print("P=%d V=%d against the per-view K8: %-10s %.3e" % (P, V, k, e))
        assert e < TOL_K8, (k, e)
        e = rel_err(one[k], ref[k])
        print("P=%d V=%d against fp64:            %-10s %.3e" % (P, V, k, e))
        assert e < TOL, (k, e)


def test_a_smaller_call_in_between_changes_nothing():
    big, small = scene(4), scene(4, P=33)
    a = step(big[0], big[1], False)
    step(small[0], small[1], False)
    b = step(big[0], big[1], False)
    for fa, fb in zip(a[0], b[0]):
        for k in fa:
            assert np.array_equal(fa[k], fb[k]), k
    for k in a[1]:
        assert np.array_equal(bits(a[1][k]), bits(b[1][k])), k
