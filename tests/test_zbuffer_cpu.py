"""The mesh z-buffer without a GPU: the oracle tests/zbuffer_ref.py against known answers (the half-open rectangle, watertightness, a
sliver, the perspective-correct midpoint), the Python surface of csplat.zbuffer on CPU tensors (its composed branch) against the oracle,
every ValueError, and the library's surface (header block, exports, bindings, argument checks before any launch)."""
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import zbuffer_ref as R
from csplat import zbuffer as zb  # noqa: E402  (absent: every test of this file fails)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN, INF = float("nan"), float("inf")
T = torch.from_numpy


def screen_of(pix, z=1.0):
    """pixel coordinates [N,2] (multiples of 1/256) and depths -> one view's screen records [1,N,4]"""
    pix = np.asarray(pix, np.float64)
    s = np.rint(pix * R.SUB)
    assert np.array_equal(s, pix * R.SUB)
    iz = (np.float32(1) / np.broadcast_to(np.asarray(z, np.float32), (len(pix),))).astype(np.float32)
    return np.stack([s[:, 0].astype(np.int32), s[:, 1].astype(np.int32), iz.view(np.int32), np.ones(len(pix), np.int32)], -1)[None]


def camera(theta, W, H, **kw):
    from csplat import synthetic as syn
    c = syn.make_camera(theta, W, H, **kw)
    return SimpleNamespace(world_view_transform=torch.from_numpy(c["world_view_transform"]), full_proj_transform=torch.from_numpy(c["full_proj_transform"]),
                           FoVx=c["FoVx"], FoVy=c["FoVy"], image_width=W, image_height=H, camera_center=torch.from_numpy(c["camera_center"]))


# ------------------------------------------------------------------------------------------------------------------ the oracle's own answers
def test_an_integer_grid_covers_the_half_open_rectangle():
    g = 5
    i, j = np.meshgrid(np.arange(g), np.arange(g), indexing="xy")
    pix = np.stack([3 + 8 * i, 2 + 8 * j], -1).reshape(-1, 2)                 # (3, 2) .. (35, 34)
    r = R.raster(screen_of(pix), R.grid_faces(g, np.random.default_rng(0)), 40, 40)
    want = np.zeros((40, 40), np.int32)
    want[2:34, 3:35] = 1
    assert np.array_equal(r["count"][0], want) and r["count"].sum() == 1024
    assert np.array_equal(r["face32"][0] >= 0, want == 1) and np.array_equal(r["face32"], r["face64"])
    assert (r["z32"][0][want == 1] == 1.0).all() and np.isinf(r["z32"][0][want == 0]).all()


def test_a_random_winding_grid_is_watertight():
    rng = np.random.default_rng(1)
    g = 9
    i, j = np.meshgrid(np.arange(g), np.arange(g), indexing="xy")
    pix = np.stack([2 + 4 * i, 3 + 4 * j], -1).astype(np.float64)
    pix[1:-1, 1:-1] += rng.integers(-1, 2, (g - 2, g - 2, 2))                  # interior vertices move, all stay on pixel centres
    r = R.raster(screen_of(pix.reshape(-1, 2)), R.grid_faces(g, rng), 40, 40)
    want = np.zeros((40, 40), np.int32)
    want[3:35, 2:34] = 1
    assert np.array_equal(r["count"][0], want)                                 # every interior pixel has exactly one owner
    t = r["t32"][0].sum(0)
    assert np.abs(t[want == 1] - 1).max() < 1e-6 and (t[want == 0] == 0).all()


def test_a_sliver_covers_no_centre_and_the_midpoint_depth_is_perspective_correct():
    r = R.raster(screen_of([[0.25, 0.25], [30.75, 0.5], [0.25, 0.75]]), [[0, 1, 2]], 8, 32)
    assert r["count"].sum() == 0 and (r["face32"] == -1).all()
    # an edge from z = 1 to z = 4: its midpoint lies at 1 / (0.5 / 1 + 0.5 / 4) = 1.6, not at 2.5
    for faces in ([[0, 1, 2]], [[0, 2, 1]], [[1, 2, 0]]):
        r = R.raster(screen_of([[0, 0], [8, 0], [0, 8]], [1.0, 4.0, 1.0]), faces, 10, 10)
        assert r["face32"][0, 0, 4] == 0 and r["z32"][0, 0, 4] == np.float32(1.6) and abs(r["z64"][0, 0, 4] - 1.6) < 1e-7
        assert r["z32"][0, 0, 0] == 1.0 and r["face32"][0, 0, 8] == -1 and r["face32"][0, 8, 0] == -1      # right and bottom ends are open
        k = [faces[0].index(c) for c in range(3)]                                                           # the weights follow the corner order
        assert np.allclose(r["t32"][0, :, 0, 4][k], [0.8, 0.2, 0.0], atol=1e-6)
    # equal depths: the lower face index wins
    r = R.raster(screen_of([[0, 0], [8, 0], [0, 8]], 2.0), [[0, 1, 2], [2, 0, 1]], 10, 10)
    assert (r["count"][0, :3, :3] == 2).all() and (r["face32"][0, :3, :3] == 0).all() and (r["face64"][0, :3, :3] == 0).all()
    assert (r["second64"][0, :3, :3] == 2.0).all()


# ------------------------------------------------------------------------------------------------------------------ the composed path
def compare_exact(images, r, screen, intr, kind, what):
    ids = images.face_id.numpy()
    assert np.array_equal(ids, r["face32"]), what
    assert np.array_equal(images.silhouette.numpy()[:, 0], (r["face32"] >= 0).astype(np.float32)), what
    r32, r64 = R.depth_image(r["z32"], intr, kind, np.float32), R.depth_image(r["z32"], intr, kind, np.float64)
    got = images.depth.numpy()[:, 0]
    if kind == "z":
        assert np.array_equal(got, r32), what
    else:                                                                      # (the ray factor holds a square root: the project's bar)
        assert np.array_equal(got == 0, r32 == 0) and np.abs(got - r64).max() <= R.depth_bar(r32, r64), what
    if images.bary is not None:
        assert np.array_equal(images.bary.numpy(), r["t32"]), what
    if images.screen is not None:
        assert np.array_equal(images.screen.numpy(), screen), what


@pytest.mark.parametrize("kind", ["z", "ray"])
def test_dyadic_fixtures_on_cpu_tensors_equal_the_oracle(kind):
    rng = np.random.default_rng(2)
    H, W = 29, 37
    intr, w2c = R.dyadic_camera(H, W)
    sv, sf, names = R.special(H, W, intr[0])
    uv, uf = R.soup(rng, 60, H, W, intr[0])
    gv, gf = R.folded_grid(10, H, W, intr[0], rng)
    verts = np.concatenate([sv, uv, gv])
    faces = np.concatenate([sf, uf + len(sv), gf + len(sv) + len(uv)])
    screen = R.project(verts, intr, w2c)["screen"]
    assert not screen[0, len(sv) - 2:len(sv), 3].any() and screen[0, :len(sv) - 2, 3].all()      # behind near, beyond the guard
    r = R.raster(screen, faces, H, W)
    assert r["count"].max() >= 3 and (r["face32"] == -1).sum() == 0                             # (the "whole image" face lies behind)
    images = zb.rasterize_mesh(T(verts), T(faces), (H, W), intrinsics=T(intr), world_to_cam=T(w2c), kind=kind, with_bary=True, return_screen=True)
    assert images.depth.shape == (1, 1, H, W) and images.depth.dtype == torch.float32 and images.face_id.dtype == torch.int32
    compare_exact(images, r, screen, intr, kind, kind)
    # the reference's [3,F] faces, int32, float64 vertices, one camera for all views without a leading axis: the same images
    again = zb.rasterize_mesh(T(verts).double(), T(faces).t().to(torch.int32), (H, W), intrinsics=T(intr[0]), world_to_cam=T(w2c[0]), kind=kind)
    assert again.bary is None and again.screen is None and torch.equal(again.face_id, images.face_id) and torch.equal(again.depth, images.depth)
    # the coincident pair: the copy is the last face and never wins
    assert (r["face32"] != len(faces) - 1).all() and (r["face32"] == len(faces) - 2).any()
    fv, nv = zb.mesh_visibility(images.face_id, T(faces), len(verts))
    wf, wn = R.visibility(r["face32"], faces, len(verts))
    assert fv.dtype == torch.bool and np.array_equal(fv.numpy(), wf) and np.array_equal(nv.numpy(), wn) and 0 < wf.sum() < wf.size


def test_per_view_vertices_an_empty_view_and_no_faces():
    rng = np.random.default_rng(3)
    H, W, V = 20, 24, 3
    intr, w2c = R.dyadic_camera(H, W, V)
    uv, uf = R.soup(rng, 40, H, W, intr[0])
    verts = np.stack([uv, uv + np.float32([0, 0, -8]), uv * np.float32([1, 1, 2])])              # view 1: everything behind the camera
    screen = R.project(verts, intr, w2c)["screen"]
    r = R.raster(screen, uf, H, W)
    images = zb.rasterize_mesh(T(verts), T(uf), (H, W), intrinsics=T(intr), world_to_cam=T(w2c), with_bary=True, return_screen=True)
    compare_exact(images, r, screen, intr, "z", "per view")
    assert (r["face32"][1] == -1).all() and (r["face32"][0] >= 0).any() and not np.array_equal(r["face32"][0], r["face32"][2])
    none = zb.rasterize_mesh(T(uv), torch.zeros(0, 3, dtype=torch.int64), (H, W), intrinsics=T(intr), world_to_cam=T(w2c), with_bary=True)
    assert none.depth.shape == (V, 1, H, W) and not none.depth.any() and not none.silhouette.any() and (none.face_id == -1).all() and not none.bary.any()
    fv, nv = zb.mesh_visibility(none.face_id, torch.zeros(0, 3, dtype=torch.int64), 7)
    assert fv.shape == (V, 0) and nv.shape == (V, 7) and not nv.any()


def test_rotated_cameras_through_the_screen_and_the_round_trip():
    """general cameras: the composed screen against the float64 stage P (valid equal away from the limits, sx and sy within one unit),
    then the images against the oracle run on that screen, exactly; the depth unprojects onto the faces' planes"""
    from csplat import observation as ob, synthetic as syn, tracking as tk
    H, W = 48, 64
    cams = [camera(-40.0, W, H), camera(75.0, W, H, phi_deg=-60.0, radius=3.0)]
    pos, faces, _edges = syn.grid_mesh(12)
    pos = (pos * np.float32(1.5)).astype(np.float32)
    for kind in ("z", "ray"):
        images = zb.rasterize_mesh(T(pos), T(faces.astype(np.int64)), (H, W), cameras=cams, kind=kind, return_screen=True)
        intr = np.array([ob.camera_intrinsics(c, H, W) for c in cams], np.float32)
        w2c = np.stack([c.world_view_transform.numpy().astype(np.float64).T[:3] for c in cams]).astype(np.float32)
        screen = images.screen.numpy()
        p64 = R.project(pos, intr, w2c, dtype=np.float64)
        assert np.array_equal(screen[..., 3] != 0, p64["valid"]) and p64["valid"].all() and np.abs(p64["px"]).max() < 2048
        off = max(np.abs(screen[..., 0] - R.SUB * p64["px"]).max(), np.abs(screen[..., 1] - R.SUB * p64["py"]).max())
        assert off <= 1.0, off
        r = R.raster(screen, faces, H, W)
        compare_exact(images, r, screen, intr, kind, kind)
        assert 0.05 < (r["face32"] >= 0).mean() < 0.9
        cloud = ob.unproject_depth(images.depth[:, 0], cameras=cams, kind=kind)
        ids = images.face_id.reshape(-1)[cloud.source].numpy()
        tri = pos[faces[ids]].astype(np.float64)
        n = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
        dist = np.abs(((cloud.points.numpy() - tri[:, 0]) * n).sum(1)) / np.linalg.norm(n, axis=1)
        assert len(ids) == (r["face32"] >= 0).sum() and dist.max() < 2e-3, dist.max()      # (snapping moves a vertex by <= 1/512 pixel)
        for v, cam in enumerate(cams):
            on = cloud.view == v
            src = cloud.source[on] - v * H * W
            want = torch.stack([src % W, src // W], 1).float()
            assert float((tk.project(cloud.points[on], cam) - want).abs().max()) < 1e-3


def test_splat_points_known_answers():
    intr = torch.tensor([2.0, 2.0, 1.0, 1.0])
    eye = torch.tensor(R.EYE34)
    #          nearest of three   tie: lower index      x = 0.25 -> px 1.5 -> 2 (even); px 2.5 -> 2       outside      behind near
    pts = torch.tensor([[0.0, 0, 3], [0, 0, 2], [0, 0, 2], [0.25, 0.5, 1], [0.75, 0.5, 1], [9.0, 0, 1], [-9.0, 0, 1], [0, 0, 0.005], [0, 0, -1.0],
                        [NAN, 0, 1]])
    out = zb.splat_points(pts, (3, 4), intrinsics=intr, world_to_cam=eye)
    assert isinstance(out, zb.PointImages) and out.depth.shape == (1, 1, 3, 4) and out.point_id.dtype == torch.int32
    want = np.full((3, 4), -1)
    want[1, 1], want[2, 2] = 1, 3
    assert np.array_equal(out.point_id[0].numpy(), want)
    assert out.depth[0, 0, 1, 1] == 2.0 and out.depth[0, 0, 2, 2] == 1.0 and out.depth.sum() == 3.0
    z, ids = R.points(pts.numpy(), intr[None].numpy(), R.EYE34[None], 3, 4)
    assert np.array_equal(ids[0], want)
    ray = zb.splat_points(pts[None], (3, 4), intrinsics=intr, world_to_cam=eye, kind="ray")
    assert ray.depth[0, 0, 1, 1] == 2.0 and abs(float(ray.depth[0, 0, 2, 2]) - 1.5 ** 0.5) < 1e-6      # (u, w) = (0.5, 0.5) at z = 1
    rng = np.random.default_rng(4)
    H, W = 9, 13
    k, m = R.dyadic_camera(H, W, 2)
    cloud = R.unproject_pixels(np.round(rng.uniform(-2, 15, (2, 400, 2)) * 4) / 4, rng.choice([1.0, 2.0, 4.0], (2, 400)), k[0])
    z, ids = R.points(cloud, k, m, H, W)
    got = zb.splat_points(T(cloud), (H, W), intrinsics=T(k), world_to_cam=T(m))
    assert np.array_equal(got.point_id.numpy(), ids) and np.array_equal(got.depth.numpy()[:, 0], R.depth_image(z, k, "z", np.float32))
    assert (ids >= 0).mean() > 0.5


def test_argument_errors():
    v, f, k, m = torch.zeros(5, 3), torch.tensor([[0, 1, 2]]), torch.ones(4), torch.tensor(R.EYE34)
    cams = [camera(0.0, 4, 3), camera(10.0, 4, 3)]
    bad = [
        (dict(vertices=torch.zeros(5, 2)), r"\[n,3\]"), (dict(vertices=torch.zeros(5, 3, dtype=torch.int64)), "floating point"), (dict(vertices="x"), "tensor or numpy"),
        (dict(vertices=torch.zeros(2, 2, 5, 3)), r"\[n,3\]"), (dict(size=(0, 4)), "size"), (dict(size=5), "size"), (dict(size=(3,)), "size"),
        (dict(kind="w"), "kind"), (dict(near=-1.0), "near"), (dict(near=NAN), "near"), (dict(near=INF), "near"),
        (dict(intrinsics=None), "pass `cameras`, or both"), (dict(world_to_cam=None), "pass `cameras`, or both"), (dict(cameras=cams), "not both"),
        (dict(intrinsics=torch.ones(3)), "intrinsics"), (dict(intrinsics=torch.ones(2, 2, 4)), "intrinsics"), (dict(world_to_cam=torch.ones(3, 3)), "world_to_cam"),
        (dict(intrinsics=torch.ones(2, 4), world_to_cam=torch.ones(3, 3, 4)), "disagree"), (dict(vertices=torch.zeros(3, 5, 3), intrinsics=torch.ones(2, 4)), "disagree"),
        (dict(faces=torch.tensor([[0, 1, 5]])), r"0 \.\. 4, found 0 \.\. 5"), (dict(faces=torch.tensor([[0, -1, 2]])), "found -1"),
        (dict(faces=torch.tensor([[0.0, 1.0, 2.0]])), "int32 / int64"), (dict(faces=torch.tensor([0, 1, 2])), r"\[F,3\]"), (dict(faces=torch.zeros(2, 4, dtype=torch.int64)), r"\[F,3\]"),
        (dict(faces=[[0, 1, 2]]), "int32 / int64"),
    ]
    for kw, text in bad:
        args = dict(vertices=v, faces=f, size=(3, 4), intrinsics=k, world_to_cam=m)
        args.update(kw)
        with pytest.raises(ValueError, match=text):
            zb.rasterize_mesh(args.pop("vertices"), args.pop("faces"), args.pop("size"), **args)
        if not {"faces", "vertices"} & set(kw):
            args = dict(size=(3, 4), intrinsics=k, world_to_cam=m)
            args.update(kw)
            with pytest.raises(ValueError, match=text):
                zb.splat_points(v, args.pop("size"), **args)
    with pytest.raises(ValueError, match="empty"):
        zb.rasterize_mesh(v, f, (3, 4), cameras=[])
    with pytest.raises(ValueError, match="world_view_transform"):
        zb.rasterize_mesh(v, f, (3, 4), cameras=[SimpleNamespace(world_view_transform=torch.ones(3, 3), FoVx=1.0, FoVy=1.0)])
    with pytest.raises(ValueError, match=r"\[n,3\]"):
        zb.splat_points(torch.zeros(5, 2), (3, 4), intrinsics=k, world_to_cam=m)
    ids = torch.zeros(1, 3, 4, dtype=torch.int32)
    for args, text in (((ids.float(), f, 5), "face_id"), ((ids[0, 0], f, 5), r"\[V,H,W\]"), ((ids, f, -1), "num_nodes"), ((ids, f, 2.0), "num_nodes"),
                       ((ids, f, 2), "face indices"), ((ids + 1, f, 5), "the mesh has 1 faces"), ((ids, torch.zeros(2, 2, dtype=torch.int64), 5), r"\[F,3\]")):
        with pytest.raises(ValueError, match=text):
            zb.mesh_visibility(*args)


# ------------------------------------------------------------------------------------------------------------------ the library's surface
ENTRIES = (("int", "csplat_zb_mesh", 20), ("int", "csplat_zb_points", 15), ("int", "csplat_zb_mark", 10))


def test_header_exports_and_bindings():
    from csplat import native
    header = open(os.path.join(ROOT, "include", "csplat.h")).read()
    for res, name, n_args in ENTRIES:
        assert re.search(r"\b" + res + " " + name + r"\s*\(", header), name
        assert name in native.EXPORTS and hasattr(native.lib, name) and len(native.EXPORTS[name][1]) == n_args
        decl = header[header.index(res + " " + name + "("):]
        decl = re.sub(r"/\*.*?\*/", "", decl[:decl.index(";")], flags=re.S)
        assert decl.count(",") + 1 == n_args, (name, decl)
    block = header[header.index("/* Mesh z-buffer"):header.index("int csplat_zb_mesh(")]
    assert block.rstrip().endswith("Added exports: CSPLAT_ABI_VERSION is unchanged. */")
    block = re.sub(r"\n \* *", " ", block)                                  # (a phrase may run over the end of a line)
    for word in ("pixel centres at the integers", "p_cam = R p_world + t", "z > near", "|px| <= 16384", "rint(256 px)", "round-half-even", "NO CLIPPING",
                 "dropped", "two-sided", "E = dx (Py - ya) - dy (Px - xa)", "dy < 0", "dy == 0 and dx > 0", "top-left rule", "(float)E_i / (float)A",
                 "z = 1 / q", "lower face index", "(float bits of z) << 32 | face", "on every call", "atomicMin", "NO float atomics", "bit-reproducible",
                 "sqrt(u u + w w + 1)", "-1 on the background", "(b_i iz_i) / q", "(rint(px), rint(py))", "zeroes the flags on the stream", "align256(8 V H W) + align256(16 V n)",
                 "exports no size query"):
        assert word.lower() in block.lower(), word
    assert "typedef struct" not in block and native.ABI_VERSION == 9 and native.lib.csplat_abi_version() == 9
    src = open(os.path.join(ROOT, "cloth-splatting_amd", "csrc", "csplat_zbuffer.hip")).read()
    code = re.sub(r"//.*", "", src)
    assert '#include "csplat_device.h"' in code and "#pragma clang fp contract(off)" in code and "csplat_raster" not in code
    assert set(re.findall(r"\batomic\w*", code)) == {"atomicMin"} and "unsigned long long *__restrict__ keys" in code      # the integer minimum only
    assert sorted(set(re.findall(r"\bk_zb_\w+", code))) == ["k_zb_clear", "k_zb_draw", "k_zb_mark", "k_zb_points", "k_zb_project", "k_zb_resolve"]
    assert zb.SUB == R.SUB == int(re.search(r"ZB_SUB = (\d+)", src).group(1)) and zb.GUARD == R.GUARD == float(re.search(r"ZB_GUARD = (\d+)", src).group(1))


def test_the_library_refuses_bad_arguments_before_any_launch():
    """fake, distinct, aligned addresses 2^32 apart: every call here must be refused (or be a no-op) before a launch could touch them"""
    from csplat import native
    L = native.lib
    A = lambda i: (i + 1) << 32  # noqa: E731
    assert not hasattr(L, "csplat_zb_temp_bytes")                    # sized in Python by the header's words; the library checks temp_bytes
    assert zb.temp_bytes(4, 10000, 800, 800) == 4 * 800 * 800 * 8 + 4 * 10000 * 16 and zb.temp_bytes(1, 0, 1, 1) == 256
    assert zb.temp_bytes(2, 10, 3, 4) == 256 + 512 and zb.temp_bytes(1, 17, 1, 33) == 512 + 512
    mesh = lambda V=2, N=10, F=5, H=3, W=4, vtx=A(0), pv=0, faces=A(1), intr=A(2), w2c=A(3), near=0.01, kind=0, depth=A(4), sil=A(5), ids=A(6), bary=A(7), \
        screen=A(8), tmp=A(9), size=768: L.csplat_zb_mesh(None, V, N, F, H, W, vtx, pv, faces, intr, w2c, near, kind, depth, sil, ids, bary, screen, tmp, size)  # noqa: E731
    for kw in (dict(V=-1), dict(V=65536), dict(N=-1), dict(N=2 ** 31), dict(F=-1), dict(F=2 ** 31), dict(H=-1), dict(W=-1), dict(V=40000, H=40000, W=2),
               dict(H=50000, W=50000), dict(V=3, N=2 ** 30), dict(kind=2), dict(kind=-1), dict(near=-0.5), dict(near=NAN), dict(near=INF), dict(pv=2),
               dict(vtx=None), dict(faces=None), dict(intr=None), dict(w2c=None), dict(depth=None), dict(sil=None), dict(ids=None), dict(tmp=None),
               dict(vtx=A(0) + 2), dict(faces=A(1) + 1), dict(depth=A(4) + 2), dict(bary=A(7) + 1), dict(screen=A(8) + 4), dict(tmp=A(9) + 8),
               dict(depth=A(0)), dict(sil=A(4) + 16), dict(ids=A(1) + 8), dict(bary=A(2)), dict(screen=A(3) + 16), dict(tmp=A(6)), dict(tmp=A(0) - 256),
               dict(bary=A(4) + 2 * 3 * 4 * 4 - 4), dict(size=767), dict(size=0), dict(N=17, size=768)):
        assert mesh(**kw) == 2, kw
        assert b"csplat_zb_mesh" in L.csplat_last_error(), kw
    assert mesh(V=0) == 0 and mesh(H=0, screen=None) == 0 and mesh(W=0, N=0) == 0 and mesh(V=0, vtx=None, faces=None, depth=None, tmp=None) == 0
    pts = lambda V=2, M=10, H=3, W=4, p=A(0), pv=0, intr=A(1), w2c=A(2), near=0.01, kind=0, depth=A(3), ids=A(4), tmp=A(5), size=768: \
        L.csplat_zb_points(None, V, M, H, W, p, pv, intr, w2c, near, kind, depth, ids, tmp, size)  # noqa: E731
    for kw in (dict(V=-1), dict(V=65536), dict(M=-1), dict(M=2 ** 31), dict(H=-1), dict(V=40000, H=40000, W=2), dict(kind=3), dict(near=NAN), dict(near=-1.0),
               dict(pv=-1), dict(p=None), dict(intr=None), dict(w2c=None), dict(depth=None), dict(ids=None), dict(tmp=None), dict(p=A(0) + 1),
               dict(depth=A(3) + 2), dict(tmp=A(5) + 4), dict(depth=A(0)), dict(ids=A(3) + 8), dict(tmp=A(1)), dict(ids=A(2) + 4), dict(size=767), dict(M=17)):
        assert pts(**kw) == 2, kw
        assert b"csplat_zb_points" in L.csplat_last_error(), kw
    assert pts(V=0) == 0 and pts(W=0) == 0 and pts(H=0, p=None, depth=None, ids=None, tmp=None) == 0
    mark = lambda V=2, N=10, F=5, H=3, W=4, ids=A(0), faces=A(1), fv=A(2), nv=A(3): L.csplat_zb_mark(None, V, N, F, H, W, ids, faces, fv, nv)  # noqa: E731
    for kw in (dict(V=-1), dict(V=65536), dict(N=-1), dict(F=-1), dict(F=2 ** 31), dict(V=3, F=2 ** 30), dict(H=-1), dict(V=40000, H=40000, W=2),
               dict(fv=None), dict(nv=None), dict(ids=None), dict(faces=None), dict(ids=A(0) + 2), dict(faces=A(1) + 1), dict(fv=A(0) + 8), dict(nv=A(1) + 4),
               dict(nv=A(2) + 9)):
        assert mark(**kw) == 2, kw
        assert b"csplat_zb_mark" in L.csplat_last_error(), kw
    assert mark(V=0) == 0 and mark(V=0, ids=None, faces=None, fv=None, nv=None) == 0
