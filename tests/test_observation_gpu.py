"""csplat.observation on the GPU (csrc/csplat_observation.hip: csplat_obs_unproject, csplat_obs_voxel, csplat_obs_mark) against the
restatement tests/observation_ref.py, under strict dispatch.

Exact parts -- the selection, `source`, `view`, the count; the voxels' order, `counts`, `inverse`; the observable flags -- are compared
for equality with the float32 restatement, which states cells and selection in the kernels' own arithmetic.  Values (points, centroids,
the Chamfer value of the end-to-end case) follow the rule of tests/test_train_kernels_gpu.py (its check() and TABLE are used): within
8 x the float32 restatement's own error against float64, floor 1e-6, relative to the largest reference magnitude (unit 1).

Shapes.  The unproject kernels walk a view's plane in slots of four pixels from the first 16-byte boundary: 37 x 29 = 1073 pixels (odd:
every view of a stack begins at another offset from the boundary, so scalar heads, vector bodies and scalar tails all occur), a 1 x 1
image (no whole slot), a depth tensor that itself begins 4 bytes off the boundary, and one 300 x 260 view (78 000 pixels: 77 workgroups
of k_obs_select and several blocks of the scan inside csplat_mask_to_map).  The voxel kernels: one point, 5000 points in ~125 cells, 3000
points in one cell (a segment longer than a workgroup: 47 rounds of the wave that owns it), every point in its own cell (K = M), points on
exact multiples of the size, non-finite rows, a cloud outside the grid."""
from types import SimpleNamespace

import numpy as np
import pytest

import util
import observation_ref as R
from test_train_kernels_gpu import FLOOR, K, TABLE, check  # noqa: F401  (the project's rule for a bar, and the table of its comparisons)

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
from csplat import observation as ob  # noqa: E402  (absent: every test of this file fails)

NAN, INF = float("nan"), float("inf")


@pytest.fixture(scope="module", autouse=True)
def _table():
    yield
    print("\ngroup | comparisons | largest e32 | largest bar | largest kernel error | smallest bar / error")
    for g in sorted(g for g in TABLE if g.startswith("observation")):
        n, e32, bar, err, margin = TABLE[g]
        print(f"{g} | {n} | {e32:.2e} | {bar:.2e} | {err:.2e} | {margin:.1f}")


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def depth_case(V, H, W, layout, seed=0):
    """float32 depth with holes of every kind (0, negative, NaN, +-Inf), a mask with values on both sides of 0.5, per-view cameras.
    layout "mixed": every view has holes;  "edges" (V >= 3): view 1 has nothing but holes, view 2 none (and a mask of ones)"""
    from csplat import synthetic as syn
    rng = np.random.default_rng(seed)
    d = rng.uniform(0.5, 6.0, (V, H, W)).astype(np.float32)
    kind = rng.integers(0, 12, d.shape)
    mask = rng.choice(np.array([0.0, 0.5, 0.75, 1.0], np.float32), d.shape)
    if layout == "edges":
        kind[1] %= 5
        kind[2] = 11
        mask[2] = 1.0
    for code, value in ((0, 0.0), (1, -1.5), (2, NAN), (3, INF), (4, -INF)):
        d[kind == code] = value
    intr = np.stack([[40.0 + v, 38.0 - v, (W - 1) / 2 + 0.25 * v, (H - 1) / 2] for v in range(V)]).astype(np.float32)
    c2w = np.stack([np.linalg.inv(syn.make_camera(30.0 * v - 20, 64, 48)["world_view_transform"].astype(np.float64).T)[:3] for v in range(V)])
    return d, mask, intr, c2w.astype(np.float32)


def unproject_case(group, what, d, mask, intr, c2w, stride, max_depth, kind, depth_gpu=None):
    V, H, W = d.shape
    args = dict(intrinsics=cu(intr), cam_to_world=cu(c2w), masks=None if mask is None else cu(mask), stride=stride, max_depth=max_depth, kind=kind)
    dg = cu(d) if depth_gpu is None else depth_gpu
    got = ob.unproject_depth(dg, **args)
    again = ob.unproject_depth(dg, **args)
    k = 0 if kind == "z" else 1
    r32, src, view = R.unproject(d, intr, c2w, mask, stride, max_depth or 0.0, k, np.float32)
    r64 = R.unproject(d, intr, c2w, mask, stride, max_depth or 0.0, k, np.float64)[0]
    assert got.points.dtype == torch.float32 and got.source.dtype == torch.int64 and got.view.dtype == torch.int64
    assert got.points.shape == (len(src), 3), (what, got.points.shape, len(src))                       # the count
    assert np.array_equal(got.source.cpu().numpy(), src) and np.array_equal(got.view.cpu().numpy(), view), what
    assert torch.equal(got.points, again.points) and torch.equal(got.source, again.source), what       # two runs: the same bits
    if len(src):
        check(group, what, got.points, r64, r32, 1.0)
    return got, src


@pytest.mark.parametrize("layout", ["mixed", "edges"])
@pytest.mark.parametrize("masked,stride,max_depth,kind", [(False, 1, None, "z"), (True, 1, None, "ray"), (True, 3, 4.0, "z"), (False, 3, 3.0, "ray")])
def test_unproject_three_views_of_37_by_29(layout, masked, stride, max_depth, kind):
    d, mask, intr, c2w = depth_case(3, 29, 37, layout)
    assert all(np.isnan(d).any() and (d == v).any() for v in (0.0, -1.5, INF, -INF))
    got, src = unproject_case("observation unproject", f"{layout} mask{masked} stride{stride} max{max_depth} {kind}", d, mask if masked else None,
                              intr, c2w, stride, max_depth, kind)
    per_view = np.bincount(src // (29 * 37), minlength=3)
    if layout == "edges":
        assert per_view[1] == 0 and per_view[0] > 0
        if stride == 1 and max_depth is None:
            assert per_view[2] == 29 * 37                                                            # a view with everything selected
    else:
        assert (per_view > 0).all()


def test_unproject_one_pixel_images_and_an_offset_tensor():
    eye = np.array([[1.0, 0, 0, 0], [0, 1.0, 0, 0], [0, 0, 1.0, 0]], np.float32)
    intr = np.array([[1.0, 1.0, 0.0, 0.0]], np.float32)
    got, src = unproject_case("observation unproject", "1x1", np.full((1, 1, 1), 2.0, np.float32), None, intr, eye[None], 1, None, "z")
    assert got.points.tolist() == [[0.0, 0.0, 2.0]] and src.tolist() == [0]
    d = np.array([0.0, 3.0, NAN, 5.0], np.float32).reshape(4, 1, 1)
    got, src = unproject_case("observation unproject", "1x1 x 4 views", d, None, np.repeat(intr, 4, 0), np.repeat(eye[None], 4, 0), 1, None, "ray")
    assert src.tolist() == [1, 3] and got.points.tolist() == [[0.0, 0.0, 3.0], [0.0, 0.0, 5.0]]
    none = ob.unproject_depth(torch.zeros(2, 5, 7, device="cuda"), intrinsics=cu(intr[0]), cam_to_world=cu(eye))
    assert none.points.shape == (0, 3) and none.source.shape == (0,) and none.view.shape == (0,)
    # a depth (and mask) tensor that begins 4, 8 and 12 bytes off a 16-byte boundary
    d, mask, intr, c2w = depth_case(3, 29, 37, "mixed", seed=4)
    for off in (1, 2, 3):
        buf = torch.zeros(d.size + off, device="cuda")
        buf[off:] = cu(d).reshape(-1)
        dg = buf[off:].view(d.shape)
        assert dg.is_contiguous() and dg.data_ptr() % 16 == 4 * off
        unproject_case("observation unproject", f"offset {off}", d, mask, intr, c2w, 1, None, "z", depth_gpu=dg)


def test_unproject_one_300_by_260_view():
    d, mask, intr, c2w = depth_case(1, 260, 300, "mixed", seed=2)
    got, src = unproject_case("observation unproject", "300x260 masked", d, mask, intr, c2w, 1, 5.0, "z")
    assert 10_000 < len(src) < 40_000
    unproject_case("observation unproject", "300x260 stride 2", d, None, intr, c2w, 2, None, "ray")


def test_unproject_beyond_the_capacity_reports_the_full_count():
    from csplat import native as n
    d, mask, intr, c2w = depth_case(3, 29, 37, "mixed", seed=6)
    r32, src, _view = R.unproject(d, intr, c2w)
    cap = 100
    assert len(src) > 10 * cap
    pts = torch.full((cap + 8, 3), -7.0, device="cuda")
    source = torch.full((cap + 8,), -7, dtype=torch.int32, device="cuda")
    count = torch.zeros(1, dtype=torch.int32, device="cuda")
    temp = torch.empty(int(n.lib.csplat_obs_unproject_temp_bytes(3, 29, 37)), dtype=torch.uint8, device="cuda")
    dg, kg, cg = cu(d), cu(intr), cu(c2w)
    n.check(n.lib.csplat_obs_unproject(n.stream_handle(dg.device), 3, 29, 37, n.ptr(dg), None, n.ptr(kg), n.ptr(cg), 1, 0.0, 0, cap, n.ptr(pts),
                                       n.ptr(source), n.ptr(count), n.ptr(temp)), "csplat_obs_unproject")
    assert int(count) == len(src)
    assert np.array_equal(source[:cap].cpu().numpy(), src[:cap]) and bool((source[cap:] == -7).all()) and bool((pts[cap:] == -7.0).all())
    check("observation unproject", "first rows of a full buffer", pts[:cap], R.unproject(d, intr, c2w, dtype=np.float64)[0][:cap], r32[:cap], 1.0)


# ------------------------------------------------------------------------------------------------------------------ voxel grid
def voxel_case(what, points, size, origin=None):
    pg = cu(points)
    got = ob.voxel_downsample(pg, size, origin=origin)
    again = ob.voxel_downsample(pg, size, origin=origin)
    r32, r64 = R.voxel(points, size, origin, np.float32), R.voxel(points, size, origin, np.float64)
    assert got.centroids.dtype == torch.float32 and got.counts.dtype == torch.int32 and got.inverse.dtype == torch.int64
    assert np.array_equal(got.counts.cpu().numpy(), r32["counts"]), what                              # (with the order: ascending key)
    assert np.array_equal(got.inverse.cpu().numpy(), r32["inverse"]), what
    assert all(torch.equal(a, b) for a, b in zip(got, again)), what                                   # two runs: the same bits
    assert got.centroids.shape == r32["centroids"].shape
    if len(r32["counts"]):
        check("observation voxel", what, got.centroids, r64["centroids"], r32["centroids"], 1.0)
    return got, r32


def test_voxel_generic_single_and_one_long_segment():
    rng = np.random.default_rng(3)
    generic = rng.uniform(-1.0, 1.0, (5000, 3)).astype(np.float32)
    got, w = voxel_case("5000 points", generic, 0.4)
    assert 100 <= len(w["counts"]) <= 216 and int(got.counts.sum()) == 5000
    voxel_case("5000 points, explicit origin", generic, 0.4, origin=[-1.3, -1.1, -2.0])
    voxel_case("one point", np.array([[1.0, -2.0, 3.0]], np.float32), 0.25)
    one_cell = (rng.uniform(0.1, 0.2, (3000, 3)) + [5.0, -3.0, 0.0]).astype(np.float32)
    got, w = voxel_case("3000 points in one cell", one_cell, 1.0)
    assert got.counts.tolist() == [3000]


def test_voxel_own_cells_faces_and_non_finite_rows():
    rng = np.random.default_rng(8)
    own = (np.stack(np.meshgrid(np.arange(17), np.arange(13), np.arange(11), indexing="ij"), -1).reshape(-1, 3) + 0.5).astype(np.float32)
    got, w = voxel_case("every point its own cell", own[rng.permutation(len(own))], 1.0)
    assert len(w["counts"]) == len(own) == 2431 and bool((got.counts == 1).all())
    # exact multiples of the size (a size that float32 holds exactly, and one it does not)
    faces = (rng.integers(0, 9, (2000, 3)) * np.float32(0.25)).astype(np.float32)
    got, w = voxel_case("multiples of 0.25", faces, 0.25, origin=[0.0, 0.0, 0.0])
    assert np.array_equal(w["keys"], np.unique((faces / np.float32(0.25)).astype(np.int64) @ np.array([1, 1 << 21, 1 << 42])))
    tenth = (rng.integers(0, 9, (2000, 3)).astype(np.float32) * np.float32(0.1)).astype(np.float32)
    voxel_case("multiples of 0.1", tenth, 0.1)
    rows = rng.uniform(-1.0, 1.0, (300, 3)).astype(np.float32)
    rows[[3, 50, 299], [0, 1, 2]] = [NAN, INF, -INF]
    got, w = voxel_case("non-finite rows", rows, 0.4)
    assert got.inverse[[3, 50, 299]].tolist() == [-1, -1, -1] and int(got.counts.sum()) == 297
    allnan = np.full((5, 3), NAN, np.float32)
    got, w = voxel_case("only non-finite rows", allnan, 0.4)
    assert got.centroids.shape == (0, 3) and got.inverse.tolist() == [-1] * 5


def test_voxel_a_cloud_outside_the_grid_raises():
    p = torch.tensor([[0.0, 0.0, 0.0], [0.0, float(2 ** 21), 0.0], [5.0, 5.0, 5.0]], device="cuda")
    with pytest.raises(ValueError, match="1 finite points lie outside"):
        ob.voxel_downsample(p, 1.0)
    with pytest.raises(ValueError, match="2 finite points lie outside"):
        ob.voxel_downsample(p, 1.0, origin=[0.0, 0.0, 1.0])
    ok = ob.voxel_downsample(p, 2.0)
    assert ok.counts.tolist() == [1, 1, 1] and ok.inverse.tolist() == [0, 1, 2]


# ------------------------------------------------------------------------------------------------------------------ observable nodes
def test_observable_nodes_on_the_fixture():
    g = util.golden("observation.npz")
    V, H, W = g["depth"].shape
    cloud = ob.unproject_depth(cu(g["depth"]), intrinsics=cu(g["intrinsics"].astype(np.float32)),
                               cam_to_world=cu(np.linalg.inv(g["world_to_camera"])[:, :3].astype(np.float32)))
    assert np.array_equal(cloud.source.cpu().numpy(), np.flatnonzero(g["depth"].reshape(-1) > 0))
    nodes = cu(g["particles"])
    for v in range(V):
        pts = cloud.points[cloud.view == v].contiguous()
        for k, key in ((2, "observable_k2"), (1, "observable_k1")):
            flags = ob.observable_nodes(pts, nodes, k=k)
            assert flags.dtype == torch.bool and np.array_equal(flags.cpu().numpy(), g[key][v]), (v, k)


def test_observable_nodes_against_the_restatement():
    rng = np.random.default_rng(5)
    cloud, nodes = rng.normal(size=(2000, 3)).astype(np.float32), (2.0 * rng.normal(size=(300, 3))).astype(np.float32)
    cg, ng = cu(cloud), cu(nodes)
    for k, max_dist in ((1, None), (2, None), (2, 0.3), (5, 0.5), (3, 1.0)):
        want = R.observable(cloud, nodes, k, max_dist)
        got = ob.observable_nodes(cg, ng, k=k, max_dist=max_dist)
        assert np.array_equal(got.cpu().numpy(), want) and 0 < want.sum() < 300, (k, max_dist)
        assert torch.equal(got, ob.observable_nodes(cg, ng, k=k, max_dist=max_dist))
    assert not bool(ob.observable_nodes(cg, ng, k=2, max_dist=1e-6).any()) and not R.observable(cloud, nodes, 2, 1e-6).any()
    assert ob.observable_nodes(cg[:1], ng[:1], k=1).tolist() == [True]
    assert ob.observable_nodes(cg[:1], ng[:1], k=1, max_dist=1e-3).tolist() == [False]
    assert ob.observable_nodes(cg[:0], ng, k=2).tolist() == [False] * 300
    # an odd number of entries off the 16-byte boundary: Q * k = 3 * 3
    assert np.array_equal(ob.observable_nodes(cg[:3], ng, k=3).cpu().numpy(), R.observable(cloud[:3], nodes, 3))


# ------------------------------------------------------------------------------------------------------------------ end to end
def test_camera_points_of_rendered_depth_feeds_the_chamfer_distance():
    from csplat import pointcloud
    from diff_gaussian_rasterization import GaussianRasterizer
    W, H = 128, 96
    cams, depths = [], []
    for theta in (0.0, 40.0, -70.0):
        case = util.make_case(P=2000, W=W, H=H, theta=theta)
        inp = util.gpu_inputs(case, requires_grad=False)
        _color, _radii, depth = GaussianRasterizer(util.gpu_settings(case))(means3D=inp["means3D"], means2D=inp["means2D"], opacities=inp["opacities"],
                                                                             shs=inp["shs"], scales=inp["scales"], rotations=inp["rotations"])
        c = case["cam"]
        cams.append(SimpleNamespace(world_view_transform=torch.from_numpy(c["world_view_transform"]), FoVx=c["FoVx"], FoVy=c["FoVy"],
                                    depth=depth.detach().reshape(1, H, W)))
        depths.append(depth.detach().reshape(H, W).cpu().numpy())
    means = inp["means3D"].detach()
    d = np.stack(depths)
    sil = (d > 1.0).astype(np.float32)                                                                # where the cloth covers the pixel well
    for cam, s in zip(cams, sil):
        cam.silhouette = cu(s)[None]
    intr = np.stack([R.camera_intrinsics(c.FoVx, c.FoVy, H, W) for c in cams]).astype(np.float32)
    c2w = np.stack([ob.camera_to_world(c) for c in cams]).astype(np.float32)
    pts = ob.camera_points(cams)
    r32, src, _view = R.unproject(d, intr, c2w, sil)
    r64 = R.unproject(d, intr, c2w, sil, dtype=np.float64)[0]
    assert pts.shape == r32.shape and 1000 < len(src) < d.size
    check("observation end to end", "camera_points", pts, r64, r32, 1.0)
    m = means.cpu().numpy()
    value = pointcloud.chamfer_distance(pts, means, two_sided=False)
    d2 = np.concatenate([R.sq_dists(r32[lo:lo + 2048], m).min(1) for lo in range(0, len(r32), 2048)])
    check("observation end to end", "chamfer(camera_points -> centres)", value, R.chamfer_one_sided(r64, m), d2.mean(dtype=np.float32), 0.0)
    # thinned: the voxels of the cloud the GPU produced, restated on that cloud
    thin = ob.camera_points(cams, voxel_size=0.1, stride=2, max_depth=50.0)
    cloud = ob.unproject_depth([c.depth for c in cams], cameras=cams, masks=[c.silhouette for c in cams], stride=2, max_depth=50.0).points.cpu().numpy()
    v32, v64 = R.voxel(cloud, 0.1), R.voxel(cloud, 0.1, dtype=np.float64)
    assert thin.shape == v32["centroids"].shape and len(v32["counts"]) < len(cloud) / 2
    check("observation end to end", "camera_points, voxels", thin, v64["centroids"], v32["centroids"], 1.0)
    value = pointcloud.chamfer_distance(thin, means, two_sided=False)
    d2 = np.concatenate([R.sq_dists(v32["centroids"][lo:lo + 2048], m).min(1) for lo in range(0, len(v32["centroids"]), 2048)])
    check("observation end to end", "chamfer(voxels -> centres)", value, R.chamfer_one_sided(v64["centroids"], m), d2.mean(dtype=np.float32), 0.0)
