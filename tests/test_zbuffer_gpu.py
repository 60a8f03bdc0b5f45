"""csplat.zbuffer on the GPU (csrc/csplat_zbuffer.hip: csplat_zb_mesh, csplat_zb_points, csplat_zb_mark) against the numpy oracle
tests/zbuffer_ref.py, under strict dispatch.

Exact parts -- coverage, silhouette, the hole pattern, point_id, the visibility flags -- are compared for equality.  face_id is set-valued
(two faces may lie closer than float32 resolves): the kernel's face must cover the pixel by the integer rule, its float64 depth must lie
within the depth bar of the float64 minimum, and where the runner-up is farther than that bar the id must be the oracle's; two faces with
identical snapped corners and 1 / z go to the lower index.  Depth and bary values follow the rule of tests/test_train_kernels_gpu.py (its
check() and TABLE are used): within 8 x the float32 restatement's own error against float64, floor 1e-6, unit 1.  Beyond that the images
are compared, bit for bit, with the float32 restatement run on the kernel's own screen records: that isolates the raster stage from the
projection (whose roundings may differ with fused multiply-adds), and on the dyadic fixtures, where stage P is exact, it compares directly.

Shapes.  A workgroup draws one (view, face): its four waves stride over the 8 x 8 blocks of the clipped bounding box.  1 x 1 (one lane
of one block), 37 x 29 (no multiple of 8: partial blocks on two borders), 300 x 260 with one face over the whole image (38 x 33 = 1254
blocks for one workgroup) among 200 small ones, 5000 small faces on 64 x 64 (many workgroups on the same pixels), three views with their
own vertices, no faces at all."""
from types import SimpleNamespace

import numpy as np
import pytest

import scratch_guard as G
import zbuffer_ref as R
from test_train_kernels_gpu import FLOOR, K, TABLE, check  # noqa: F401  (the project's rule for a bar, and the table of its comparisons)

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
from csplat import zbuffer as zb  # noqa: E402  (absent: every test of this file fails)

assert (K, FLOOR) == (R.K_BAR, R.FLOOR)


@pytest.fixture(scope="module", autouse=True)
def _table():
    yield
    print("\ngroup | comparisons | largest e32 | largest bar | largest kernel error | smallest bar / error")
    for g in sorted(g for g in TABLE if g.startswith("zbuffer")):
        n, e32, bar, err, margin = TABLE[g]
        print(f"{g} | {n} | {e32:.2e} | {bar:.2e} | {err:.2e} | {margin:.1f}")


DEV = "cuda"


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def camera(theta, W, H, **kw):
    from csplat import synthetic as syn
    c = syn.make_camera(theta, W, H, **kw)
    return SimpleNamespace(world_view_transform=torch.from_numpy(c["world_view_transform"]), full_proj_transform=torch.from_numpy(c["full_proj_transform"]),
                           FoVx=c["FoVx"], FoVy=c["FoVy"], image_width=W, image_height=H, camera_center=torch.from_numpy(c["camera_center"]))


def judge(what, images, screen, faces, intr, kind, r=None):
    """the rules of the module's docstring for one call's images against the oracle on `screen`; -> the oracle's result"""
    V, H, W = images.face_id.shape
    r = R.raster(screen, faces, H, W) if r is None else r
    ids, depth, sil = images.face_id.cpu().numpy(), images.depth.cpu().numpy()[:, 0], images.silhouette.cpu().numpy()[:, 0]
    hole = r["count"] == 0
    # equality: coverage, silhouette, the hole pattern
    assert np.array_equal(sil, (~hole).astype(np.float32)), what
    assert np.array_equal(depth == 0, hole) and np.array_equal(ids == -1, hole), what
    # the set-valued face id
    cov, zk = R.at_faces(screen, faces, ids)
    assert np.array_equal(cov, ~hole), what
    z32, z64 = np.where(hole, 0, r["z32"]), np.where(hole, 0, r["z64"])
    bar = R.depth_bar(z32, z64)
    with np.errstate(invalid="ignore"):                                         # (inf - inf on the background)
        assert (np.where(hole, 0, zk - r["z64"]) <= bar).all(), what
        clear = ~hole & (r["second64"] - r["z64"] > bar)
    assert np.array_equal(ids[clear], r["face64"][clear]), what
    # values, by the project's rule
    check("zbuffer depth", f"{what} {kind}", depth, R.depth_image(r["z64"], intr, kind, np.float64), R.depth_image(r["z32"], intr, kind, np.float32), 1.0)
    same = (ids == r["face64"]) & (r["face32"] == r["face64"])                  # (weights are a face's own: compared where all three agree)
    assert same.mean() > 0.99, (what, same.mean())
    if images.bary is not None:
        m = same[:, None]
        check("zbuffer bary", what, np.where(m, images.bary.cpu().numpy(), 0), np.where(m, r["t64"], 0), np.where(m, r["t32"], 0), 1.0)
    # the float32 restatement on the same screen records: bit for bit
    assert np.array_equal(ids, r["face32"]), what
    if kind == "z":
        assert np.array_equal(depth, R.depth_image(r["z32"], intr, kind, np.float32)), what
    if images.bary is not None:
        assert np.array_equal(images.bary.cpu().numpy(), r["t32"]), what
    return r


def dyadic_case(what, verts, faces, H, W, intr, w2c, kind="z"):
    """stage P is exact: the kernel's screen must be the oracle's, and the images compare directly; two runs give the same bits"""
    args = dict(intrinsics=cu(intr), world_to_cam=cu(w2c), kind=kind, with_bary=True, return_screen=True)
    vg, fg = cu(verts), cu(np.asarray(faces, np.int64))
    images = zb.rasterize_mesh(vg, fg, (H, W), **args)
    again = zb.rasterize_mesh(vg, fg, (H, W), **args)
    assert all(torch.equal(a, b) for a, b in zip(images, again)), what
    screen = R.project(verts, intr, w2c)["screen"]
    assert np.array_equal(images.screen.cpu().numpy(), screen), what
    plain = zb.rasterize_mesh(vg, fg, (H, W), intrinsics=cu(intr), world_to_cam=cu(w2c), kind=kind)      # (screen in temp, no weights)
    assert plain.bary is None and plain.screen is None and all(torch.equal(a, b) for a, b in zip(plain[:3], images[:3])), what
    return images, judge(what, images, screen, faces, intr, kind)


# ------------------------------------------------------------------------------------------------------------------ dyadic fixtures
@pytest.mark.parametrize("kind", ["z", "ray"])
def test_special_faces_a_soup_and_a_folded_grid_on_37_by_29(kind):
    rng = np.random.default_rng(2)
    H, W = 29, 37
    intr, w2c = R.dyadic_camera(H, W)
    sv, sf, names = R.special(H, W, intr[0])
    uv, uf = R.soup(rng, 60, H, W, intr[0])
    gv, gf = R.folded_grid(10, H, W, intr[0], rng)
    verts = np.concatenate([sv, uv, gv])
    faces = np.concatenate([sf, uf + len(sv), gf + len(sv) + len(uv)])
    images, r = dyadic_case("special + soup + folded grid", verts, faces, H, W, intr, w2c, kind)
    assert r["count"].max() >= 3 and not (r["count"] == 0).any()
    # each special face alone: off the image, dropped, or cut by a border (compared with the oracle either way)
    alone = {}
    for k, name in enumerate(names):
        one, r1 = dyadic_case(name, sv, sf[k:k + 1], H, W, intr, w2c, kind)
        alone[name] = int((one.face_id >= 0).sum())
    for name in ("off left", "off right", "off top", "off bottom", "no area", "repeated corner", "behind near", "beyond the guard"):
        assert alone[name] == 0, name
    for name in ("cut left", "cut right", "cut top", "cut bottom", "ccw", "cw", "centres", "through centres"):
        assert alone[name] > 0, name
    assert alone["ccw"] == alone["cw"] and alone["whole image"] == H * W
    # the coincident pair (identical snapped corners and 1 / z): the copy is the last face and never wins; the original is seen
    ids = images.face_id.cpu().numpy()
    assert (ids != len(faces) - 1).all() and (ids == len(faces) - 2).any()
    fv, nv = zb.mesh_visibility(images.face_id, cu(faces), len(verts))
    wf, wn = R.visibility(ids, faces, len(verts))
    assert fv.dtype == torch.bool and np.array_equal(fv.cpu().numpy(), wf) and np.array_equal(nv.cpu().numpy(), wn) and 0 < wf.sum() < wf.size


def test_one_pixel_images():
    intr = np.array([[16.0, 16.0, 0.0, 0.0]], np.float32)
    w2c = R.EYE34[None]
    verts = R.unproject_pixels(np.array([[-2.0, -2], [5, -2], [-2, 5], [0, 0], [3, 0], [0, 3], [0.25, 0.25], [3, 0.25], [0.25, 3]]), np.array([2.0] * 3 + [1.0] * 6), intr[0])
    images, r = dyadic_case("1x1, two faces", verts, [[0, 1, 2], [3, 4, 5]], 1, 1, intr, w2c)
    assert images.face_id.tolist() == [[[1]]] and images.depth.tolist() == [[[[1.0]]]] and images.bary[0, :, 0, 0].tolist() == [1.0, 0.0, 0.0]
    images, r = dyadic_case("1x1, the centre just outside", verts, [[6, 7, 8]], 1, 1, intr, w2c)
    assert images.face_id.tolist() == [[[-1]]] and images.depth.tolist() == [[[[0.0]]]] and images.silhouette.tolist() == [[[[0.0]]]]


def test_one_face_over_the_whole_300_by_260_image_among_200_small_ones():
    rng = np.random.default_rng(5)
    H, W = 260, 300
    intr, w2c = R.dyadic_camera(H, W)
    uv, uf = R.soup(rng, 200, H, W, intr[0], extent=9.0)
    big = R.unproject_pixels(np.array([[-7.0, -5.0], [2.0 * W + 20, -5.0], [-7.0, 2.0 * H + 20]]), np.array([4.0, 2.0, 4.0]), intr[0])
    verts, faces = np.concatenate([uv, big]), np.concatenate([uf[:100], [[600, 601, 602]], uf[100:]])
    images, r = dyadic_case("300x260", verts, faces, H, W, intr, w2c, "ray")
    ids = images.face_id.cpu().numpy()
    assert not (ids == -1).any() and (ids == 100).mean() > 0.5 and len(np.unique(ids)) > 50


def test_5000_small_faces_on_64_by_64():
    rng = np.random.default_rng(6)
    H = W = 64
    intr, w2c = R.dyadic_camera(H, W)
    uv, uf = R.soup(rng, 5000, H, W, intr[0], extent=4.0)
    images, r = dyadic_case("5000 faces", uv, uf, H, W, intr, w2c)
    assert r["count"].mean() > 4 and r["count"].max() >= 10                     # contended pixels


def test_three_views_with_their_own_vertices_one_sees_nothing_and_no_faces():
    rng = np.random.default_rng(3)
    H, W, V = 29, 37, 3
    intr, w2c = R.dyadic_camera(H, W, V)
    intr[2, 2:] += [1.5, -2.25]
    uv, uf = R.soup(rng, 80, H, W, intr[0])
    verts = np.stack([uv, uv + np.float32([0, 0, -8]), uv * np.float32([1, 1, 2])])              # view 1: everything behind the camera
    images, r = dyadic_case("three views", verts, uf, H, W, intr, w2c)
    ids = images.face_id.cpu().numpy()
    assert (ids[1] == -1).all() and (ids[0] >= 0).any() and (ids[2] >= 0).any() and not np.array_equal(ids[0], ids[2])
    shared, r = dyadic_case("three views of one mesh", uv, uf, H, W, intr, w2c)
    assert torch.equal(shared.face_id[0], images.face_id[0]) and torch.equal(shared.face_id[0], shared.face_id[1])
    none = zb.rasterize_mesh(cu(uv), torch.zeros(0, 3, dtype=torch.int64, device=DEV), (H, W), intrinsics=cu(intr), world_to_cam=cu(w2c), with_bary=True)
    assert none.depth.shape == (V, 1, H, W) and not none.depth.any() and not none.silhouette.any() and bool((none.face_id == -1).all()) and not none.bary.any()
    fv, nv = zb.mesh_visibility(none.face_id, torch.zeros(0, 3, dtype=torch.int64, device=DEV), 7)
    assert fv.shape == (V, 0) and nv.shape == (V, 7) and not nv.any()
    fv, nv = zb.mesh_visibility(images.face_id, cu(uf), uv.shape[0])
    wf, wn = R.visibility(ids, uf, uv.shape[0])
    assert np.array_equal(fv.cpu().numpy(), wf) and np.array_equal(nv.cpu().numpy(), wn) and not wf[1].any() and wf[0].any()


def test_mesh_visibility_with_a_face_hidden_behind_another():
    H, W = 29, 37
    intr, w2c = R.dyadic_camera(H, W)
    pix = np.array([[2.0, 2], [30, 2], [2, 26], [6, 6], [12, 6], [6, 12], [20, 20], [34, 20], [20, 27.5]])
    verts = R.unproject_pixels(pix, np.array([1.0] * 3 + [2.0] * 3 + [2.0] * 3), intr[0])          # face 1 lies wholly behind face 0
    verts = np.concatenate([verts, np.zeros((2, 3), np.float32)])                                   # two nodes of no face
    faces = np.array([[0, 1, 2], [3, 4, 5], [6, 7, 8], [0, 4, 8]])
    images, r = dyadic_case("a hidden face", verts, faces, H, W, intr, w2c)
    fv, nv = zb.mesh_visibility(images.face_id, cu(faces), len(verts))
    assert fv.tolist() == [[True, False, True, True]] and nv.tolist() == [[True, True, True, False, True, False, True, True, True, False, False]]
    assert (r["count"] == 2).sum() > 10 and torch.equal(fv, zb.mesh_visibility(images.face_id[0], cu(faces.T.copy()), len(verts))[0])


# ------------------------------------------------------------------------------------------------------------------ general cameras
@pytest.mark.parametrize("kind", ["z", "ray"])
def test_rotated_cameras_through_the_screen_and_the_round_trip(kind):
    from csplat import observation as ob, synthetic as syn, tracking as tk
    H, W = 48, 64
    cams = [camera(-40.0, W, H), camera(75.0, W, H, phi_deg=-60.0, radius=3.0), camera(160.0, W, H, radius=2.0)]
    pos, faces, _edges = syn.grid_mesh(14)
    pos = (pos * np.float32(1.5)).astype(np.float32)
    pos = np.concatenate([pos, np.float32([[0, 0, 50.0], [0, 0, -50.0], [40.0, 0, 0]])])          # far off, behind some camera: in no face
    images = zb.rasterize_mesh(cu(pos), cu(faces), (H, W), cameras=cams, kind=kind, with_bary=True, return_screen=True)
    intr = np.array([ob.camera_intrinsics(c, H, W) for c in cams], np.float32)
    w2c = np.stack([c.world_view_transform.numpy().astype(np.float64).T[:3] for c in cams]).astype(np.float32)
    # stage P against float64: valid equal away from the limits, sx and sy within one unit (8 ulp of px < 2048 is half a unit, rounding half)
    screen = images.screen.cpu().numpy()
    p64 = R.project(pos, intr, w2c, dtype=np.float64)
    sure = (np.abs(p64["z"] - 0.01) > 1e-4) & (np.abs(np.abs(p64["px"]) - R.GUARD) > 1) & (np.abs(np.abs(p64["py"]) - R.GUARD) > 1)
    assert np.array_equal((screen[..., 3] != 0)[sure], p64["valid"][sure]) and sure.all() and not p64["valid"].all() and p64["valid"][:, :-3].all()
    on = p64["valid"]
    assert max(np.abs(p64["px"][on]).max(), np.abs(p64["py"][on]).max()) < 2048
    off = max(np.abs(screen[..., 0] - R.SUB * p64["px"])[on].max(), np.abs(screen[..., 1] - R.SUB * p64["py"])[on].max())
    same = np.array_equal(screen, R.project(pos, intr, w2c)["screen"])
    print(f"\nzbuffer stage P {kind}: largest |snapped - 256 x float64 pixel| = {off:.3f} units; equal to the float32 restatement: {same}")
    assert off <= 1.0 and not screen[~on].any()
    # the raster stage on the kernel's own screen
    r = judge("rotated cameras", images, screen, faces, intr, kind)
    assert all(0.03 < (r["count"][v] > 0).mean() < 0.95 for v in range(3))
    # round trip: the unprojected depth lies on the plane of its face_id's face.  Snapping moves a corner by at most 1/512 pixel per axis,
    # z / (512 f) in space; on faces tilted up to ~80 degrees against the ray that is at most ~6 x as much along the normal, and the float32
    # chain (bar of the depth group) adds its part: 8 z / (512 f) + 1e-5 z
    inv = np.linalg.inv(np.concatenate([w2c.astype(np.float64), np.tile([[[0, 0, 0, 1.0]]], (3, 1, 1))], 1))[:, :3]
    cloud = ob.unproject_depth(images.depth[:, 0].contiguous(), intrinsics=cu(intr), cam_to_world=cu(inv.astype(np.float32)), kind=kind)
    src = cloud.source.cpu().numpy()
    ids = images.face_id.cpu().numpy().reshape(-1)[src]
    assert len(src) == (r["count"] > 0).sum() and (ids >= 0).all()
    tri = pos[faces[ids]].astype(np.float64)
    nrm = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    dist = np.abs(((cloud.points.cpu().numpy() - tri[:, 0]) * nrm).sum(1)) / np.linalg.norm(nrm, axis=1)
    zmax = float(r["z64"][r["count"] > 0].max())
    bar = 8 * zmax / (2 * R.SUB * float(intr[:, :2].min())) + 1e-5 * zmax
    print(f"zbuffer round trip {kind}: largest distance from the face's plane {dist.max():.3e}, bar {bar:.3e}")
    assert dist.max() <= bar
    # with cameras=, tracking.project returns the pixel centres
    back = ob.unproject_depth(images.depth[:, 0].contiguous(), cameras=cams, kind=kind)
    for v, cam in enumerate(cams):
        sel = back.view == v
        s = back.source[sel] - v * H * W
        want = torch.stack([s % W, s // W], 1).float()
        assert float((tk.project(back.points[sel].contiguous(), cam) - want).abs().max()) < 1e-3


# ------------------------------------------------------------------------------------------------------------------ temp and outputs
def raw_mesh(verts, faces, H, W, intr, w2c, kind, temp=None, fill=0xFF):
    """csplat_zb_mesh itself on guarded outputs and a guarded temp of exactly the size the header words -> (outputs, temp)"""
    from csplat import native as n
    V, N, F = intr.shape[0], verts.shape[-2], len(faces)
    vg, fg, kg, mg = cu(verts), cu(np.asarray(faces, np.int32)), cu(intr), cu(w2c)
    shapes = dict(depth=((V, H, W), torch.float32), sil=((V, H, W), torch.float32), ids=((V, H, W), torch.int32), bary=((V, 3, H, W), torch.float32),
                  screen=((V, N, 4), torch.int32))
    outs, checks = {}, []
    for name, (shape, dtype) in shapes.items():
        outs[name], c = G.guarded_out(shape, dtype, "cuda")
        checks.append((name, c))
    if temp is None:
        temp, c = G.guarded(zb.temp_bytes(V, N, H, W), fill, "cuda")
        checks.append(("temp", c))
    n.check(n.lib.csplat_zb_mesh(n.stream_handle(vg.device), V, N, F, H, W, n.ptr(vg), int(verts.ndim == 3), n.ptr(fg), n.ptr(kg), n.ptr(mg), 0.01,
                                 0 if kind == "z" else 1, outs["depth"].data_ptr(), outs["sil"].data_ptr(), outs["ids"].data_ptr(), outs["bary"].data_ptr(),
                                 outs["screen"].data_ptr(), temp.data_ptr(), zb.temp_bytes(V, N, H, W)), "csplat_zb_mesh")
    torch.cuda.synchronize()
    for name, c in checks:
        c(name)
    return outs, temp


@pytest.mark.parametrize("fill", G.FILLS)
def test_guard_bytes_hostile_temp_and_temp_reuse(fill):
    from csplat import native as n
    rng = np.random.default_rng(7)
    H, W = 29, 37
    intr, w2c = R.dyadic_camera(H, W, 2)
    big_v, big_f = R.soup(rng, 300, H, W, intr[0])
    small_v, small_f = R.soup(rng, 5, H, W, intr[0], margin=-8.0)                # a few faces in the middle: most pixels stay empty
    want_big = zb.rasterize_mesh(cu(big_v), cu(big_f), (H, W), intrinsics=cu(intr), world_to_cam=cu(w2c), kind="ray", with_bary=True, return_screen=True)
    want_small = zb.rasterize_mesh(cu(small_v), cu(small_f), (H, W), intrinsics=cu(intr), world_to_cam=cu(w2c), kind="ray", with_bary=True, return_screen=True)
    assert bool((want_small.face_id == -1).any()) and not torch.equal(want_small.face_id, want_big.face_id)
    outs, temp = raw_mesh(big_v, big_f, H, W, intr, w2c, "ray", fill=fill)
    for name, t in zip(("depth", "sil", "ids", "bary", "screen"), want_big):
        assert torch.equal(outs[name].reshape(t.shape), t), (name, fill)
    assert zb.temp_bytes(2, small_v.shape[0], H, W) <= temp.numel()
    outs, _ = raw_mesh(small_v, small_f, H, W, intr, w2c, "ray", temp=temp)      # the same temp, now full of the large mesh's keys
    for name, t in zip(("depth", "sil", "ids", "bary", "screen"), want_small):
        assert torch.equal(outs[name].reshape(t.shape), t), (name, fill)


# ------------------------------------------------------------------------------------------------------------------ points
def test_splat_points():
    NAN = float("nan")
    intr = torch.tensor([2.0, 2.0, 1.0, 1.0], device=DEV)
    eye = cu(R.EYE34)
    #          nearest of three   tie: lower index      px = 1.5 and 2.5 both go to the even pixel 2      outside         behind near, NaN
    pts = torch.tensor([[0.0, 0, 3], [0, 0, 2], [0, 0, 2], [0.25, 0.5, 1], [0.75, 0.5, 1], [9.0, 0, 1], [-9.0, 0, 1], [0, 0, 0.005], [0, 0, -1.0],
                        [NAN, 0, 1]], device=DEV)
    out = zb.splat_points(pts, (3, 4), intrinsics=intr, world_to_cam=eye)
    want = np.full((3, 4), -1)
    want[1, 1], want[2, 2] = 1, 3
    assert np.array_equal(out.point_id[0].cpu().numpy(), want) and out.point_id.dtype == torch.int32
    assert out.depth[0, 0, 1, 1] == 2.0 and out.depth[0, 0, 2, 2] == 1.0 and float(out.depth.sum()) == 3.0
    rng = np.random.default_rng(4)
    H, W, V = 29, 37, 2
    k, m = R.dyadic_camera(H, W, V)
    cloud = R.unproject_pixels(np.round(rng.uniform(-4, 41, (V, 3000, 2)) * 4) / 4, rng.choice([1.0, 2.0, 4.0], (V, 3000)), k[0])
    cloud[1, :5] = [[0, 0, -1], [0, 0, 0.005], [NAN, 0, 1], [0, np.inf, 1], [0, 0, 0]]
    z, ids = R.points(cloud, k, m, H, W)
    for kind in ("z", "ray"):
        got = zb.splat_points(cu(cloud), (H, W), intrinsics=cu(k), world_to_cam=cu(m), kind=kind)
        assert torch.equal(got.depth, zb.splat_points(cu(cloud), (H, W), intrinsics=cu(k), world_to_cam=cu(m), kind=kind).depth)
        assert np.array_equal(got.point_id.cpu().numpy(), ids) and 0.5 < (ids >= 0).mean() < 1.0
        if kind == "z":
            assert np.array_equal(got.depth.cpu().numpy()[:, 0], R.depth_image(z, k, "z", np.float32))
        check("zbuffer points", kind, got.depth[:, 0], R.depth_image(z, k, kind, np.float64), R.depth_image(z, k, kind, np.float32), 1.0)
    one = zb.splat_points(cu(cloud[0]), (H, W), intrinsics=cu(k), world_to_cam=cu(m))               # one cloud for both views
    assert np.array_equal(one.point_id[0].cpu().numpy(), ids[0]) and torch.equal(one.point_id[0], one.point_id[1])
    none = zb.splat_points(torch.zeros(0, 3, device=DEV), (H, W), intrinsics=cu(k), world_to_cam=cu(m))
    assert none.depth.shape == (V, 1, H, W) and not none.depth.any() and bool((none.point_id == -1).all())
