"""Observation clouds without a GPU: the restatement tests/observation_ref.py against the reference's own get_world_coords and
get_observable_particle_index (tests/golden/observation.npz, tests/golden/make_observation_golden.py), the Python surface of
csplat.observation on CPU tensors (its composed branch) against the restatement and against known answers, every ValueError, and the
library's surface (header, exports, bindings, ABI number, argument checks before any launch)."""
import math
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import util
import observation_ref as R
from csplat import observation as ob  # noqa: E402  (absent: every test of this file fails)

F64, F32 = torch.float64, torch.float32
NAN, INF = float("nan"), float("inf")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EYE34 = [[1.0, 0.0, 0.0, 0.0], [0.0, 1.0, 0.0, 0.0], [0.0, 0.0, 1.0, 0.0]]


@pytest.fixture(scope="module")
def gold():
    g = dict(util.golden("observation.npz"))
    g["cam_to_world"] = np.linalg.inv(g["world_to_camera"])[:, :3, :]
    g["intr"] = np.broadcast_to(g["intrinsics"], (g["depth"].shape[0], 4)).copy()
    return g


def camera(theta, W, H, **kw):
    from csplat import synthetic as syn
    c = syn.make_camera(theta, W, H, **kw)
    return SimpleNamespace(world_view_transform=torch.from_numpy(c["world_view_transform"]), full_proj_transform=torch.from_numpy(c["full_proj_transform"]),
                           FoVx=c["FoVx"], FoVy=c["FoVy"], image_width=W, image_height=H, camera_center=torch.from_numpy(c["camera_center"]))


# ------------------------------------------------------------------------------------------------------------------ the fixture
def test_the_fixture_is_small_and_keeps_its_tie_margin(gold):
    assert os.path.getsize(os.path.join(util.GOLDEN, "observation.npz")) < 100_000
    V, H, W = gold["depth"].shape
    assert (V, H, W) == (2, 30, 40) and gold["particles"].shape == (25 * 12, 3)
    holes = 1.0 - (gold["depth"] > 0).mean()
    assert 0.25 < holes < 0.42 and (gold["depth"] == 0).any() and (gold["depth"] < 0).any()
    cloud = gold["world"][gold["depth"] > 0]
    # 64 x the float32 rounding of the squared distances at the scene's scale, as the generator states it
    margin = 64.0 * 2.0 ** -23 * float(R.sq_dists(cloud, gold["particles"], np.float64).max())
    assert margin == float(gold["margin"]) and margin > 0
    for k in (1, 2):
        assert float(R.tie_margins(cloud, gold["particles"], k).min()) >= margin, k


def test_the_restatement_reproduces_the_reference(gold):
    V, H, W = gold["depth"].shape
    p64, src, view = R.unproject(gold["depth"], gold["intr"], gold["cam_to_world"], dtype=np.float64)
    assert np.array_equal(src, np.flatnonzero(gold["depth"].reshape(-1) > 0)) and np.array_equal(view, src // (H * W))
    want = gold["world"].reshape(-1, 3)[src]
    # the float64 form reads float32 matrices and intrinsics: 2^-24 relative on numbers of size <= 8
    assert np.abs(p64 - want).max() < 8 * 2.0 ** -24 * 8
    p32 = R.unproject(gold["depth"], gold["intr"], gold["cam_to_world"], dtype=np.float32)[0]
    assert p32.dtype == np.float32 and np.abs(p32 - p64).max() < 1e-5
    # the observable sets, per view, with 0 cases excluded: from the float32 cloud on float32 distances
    for v in range(V):
        cloud = p32[view == v]
        assert np.array_equal(R.observable(cloud, gold["particles"], 2), gold["observable_k2"][v])
        assert np.array_equal(R.observable(cloud, gold["particles"], 1), gold["observable_k1"][v])
    assert 0 < gold["observable_k1"].sum() < gold["observable_k2"].sum() < gold["observable_k2"].size


def test_the_python_surface_reproduces_the_reference_on_cpu_tensors(gold):
    V, H, W = gold["depth"].shape
    for dt in (F32, F64):
        cloud = ob.unproject_depth(torch.from_numpy(gold["depth"]).to(dt), intrinsics=torch.from_numpy(gold["intrinsics"]),
                                   cam_to_world=torch.from_numpy(np.linalg.inv(gold["world_to_camera"])))
        assert isinstance(cloud, ob.Cloud) and cloud.points.dtype == dt and cloud.source.dtype == torch.int64 and cloud.view.dtype == torch.int64
        assert np.array_equal(cloud.source.numpy(), np.flatnonzero(gold["depth"].reshape(-1) > 0))
        assert np.abs(cloud.points.numpy() - gold["world"].reshape(-1, 3)[cloud.source.numpy()]).max() < (1e-5 if dt == F32 else 1e-12)
        for v in range(V):
            pts = cloud.points[cloud.view == v]
            nodes = torch.from_numpy(gold["particles"]).to(dt)
            for k, key in ((2, "observable_k2"), (1, "observable_k1")):
                flags = ob.observable_nodes(pts, nodes, k=k)
                assert flags.dtype == torch.bool and np.array_equal(flags.numpy(), gold[key][v]), (dt, v, k)


# ------------------------------------------------------------------------------------------------------------------ unproject
def _depth_case(V=3, H=29, W=37, seed=0):
    rng = np.random.default_rng(seed)
    d = rng.uniform(0.5, 6.0, (V, H, W)).astype(np.float32)
    kind = rng.integers(0, 12, d.shape)
    for code, value in ((0, 0.0), (1, -1.5), (2, NAN), (3, INF), (4, -INF)):
        d[kind == code] = value
    mask = rng.choice(np.array([0.0, 0.5, 0.75, 1.0], np.float32), d.shape)
    intr = np.stack([[40.0 + v, 38.0 - v, (W - 1) / 2 + 0.25 * v, (H - 1) / 2] for v in range(V)]).astype(np.float32)
    from csplat import synthetic as syn
    c2w = np.stack([np.linalg.inv(syn.make_camera(30.0 * v - 20, W, H)["world_view_transform"].astype(np.float64).T)[:3] for v in range(V)])
    return d, mask, intr, c2w.astype(np.float32)


@pytest.mark.parametrize("masked,stride,max_depth,kind", [(False, 1, None, "z"), (True, 1, None, "ray"), (True, 3, 4.0, "z"), (False, 2, 3.0, "ray")])
def test_unproject_on_cpu_tensors_equals_the_restatement(masked, stride, max_depth, kind):
    d, mask, intr, c2w = _depth_case()
    T = torch.from_numpy
    for dt, npdt in ((F32, np.float32), (F64, np.float64)):
        got = ob.unproject_depth(T(d).to(dt), intrinsics=T(intr), cam_to_world=T(c2w), masks=T(mask) if masked else None, stride=stride,
                                 max_depth=max_depth, kind=kind)
        pts, src, view = R.unproject(d, intr, c2w, mask if masked else None, stride, max_depth or 0.0, 0 if kind == "z" else 1, npdt)
        assert np.array_equal(got.source.numpy(), src) and np.array_equal(got.view.numpy(), view) and 0 < len(src) < d.size
        assert got.points.dtype == dt and np.abs(got.points.numpy() - pts).max() <= (2e-6 if dt == F32 else 1e-14)
    # the selection itself: no hole of any kind, the stride grid, the maximum, the mask
    V, H, W = d.shape
    y, x = (src % (H * W)) // W, src % W
    ds = d.reshape(-1)[src]
    assert np.isfinite(ds).all() and (ds > 0).all() and (y % stride == 0).all() and (x % stride == 0).all()
    assert max_depth is None or (ds <= max_depth).all()
    assert not masked or (mask.reshape(-1)[src] > 0.5).all()
    assert (np.diff(src) > 0).all()


def test_unproject_known_answers():
    one = ob.unproject_depth(torch.tensor([[2.0]]), intrinsics=torch.tensor([1.0, 1.0, 0.0, 0.0]), cam_to_world=torch.tensor(EYE34))
    assert one.points.tolist() == [[0.0, 0.0, 2.0]] and one.source.tolist() == [0] and one.view.tolist() == [0]
    # an identity camera: ((x - cx) d / fx, (y - cy) d / fy, d)
    d = torch.tensor([[1.0, 2.0, 0.0], [4.0, NAN, 8.0]])
    c = ob.unproject_depth(d, intrinsics=torch.tensor([2.0, 4.0, 1.0, 0.5]), cam_to_world=torch.tensor(EYE34))
    assert c.source.tolist() == [0, 1, 3, 5]
    assert c.points.tolist() == [[-0.5, -0.125, 1.0], [0.0, -0.25, 2.0], [-2.0, 0.5, 4.0], [4.0, 1.0, 8.0]]
    # a translation and an axis swap, [4,4] accepted; one matrix for all views; a list of [1,H,W]
    m = torch.tensor([[0.0, 1.0, 0.0, 10.0], [1.0, 0.0, 0.0, 20.0], [0.0, 0.0, -1.0, 30.0], [0.0, 0.0, 0.0, 1.0]])
    c2 = ob.unproject_depth([d[None], d[None]], intrinsics=torch.tensor([2.0, 4.0, 1.0, 0.5]), cam_to_world=m)
    assert c2.view.tolist() == [0] * 4 + [1] * 4 and c2.source.tolist() == [0, 1, 3, 5, 6, 7, 9, 11]
    assert c2.points[:4].tolist() == [[10 - 0.125, 20 - 0.5, 29.0], [10 - 0.25, 20.0, 28.0], [10.5, 18.0, 26.0], [11.0, 24.0, 22.0]]
    assert torch.equal(c2.points[4:], c2.points[:4])
    # along the ray: (u, w, 1) = (2, 2, 1) has length 3
    ray = ob.unproject_depth(torch.tensor([[0.0, 0.0, 6.0]]), intrinsics=torch.tensor([1.0, 0.5, 0.0, -1.0]), cam_to_world=torch.tensor(EYE34), kind="ray")
    assert ray.points.tolist() == [[4.0, 4.0, 2.0]] and ray.source.tolist() == [2]
    # nothing selected; max_depth <= 0 is none
    none = ob.unproject_depth(torch.zeros(2, 3, 4), intrinsics=torch.ones(4), cam_to_world=torch.tensor(EYE34))
    assert none.points.shape == (0, 3) and none.source.shape == (0,) and none.view.shape == (0,)
    assert ob.unproject_depth(d, intrinsics=torch.ones(4), cam_to_world=m, max_depth=0).source.tolist() == [0, 1, 3, 5]
    assert ob.unproject_depth(d, intrinsics=torch.ones(4), cam_to_world=m, max_depth=2.0).source.tolist() == [0, 1]
    assert ob.unproject_depth(d, intrinsics=torch.ones(4), cam_to_world=m, stride=2).source.tolist() == [0]
    assert ob.unproject_depth(d, intrinsics=torch.ones(4), cam_to_world=m, masks=torch.tensor([[1.0, 0.5, 1.0], [0.51, 1.0, NAN]])).source.tolist() == [0, 3]


@pytest.mark.parametrize("dt", [F32, F64])
def test_project_of_unproject_returns_the_pixel_centres(dt):
    """with `cameras=` the intrinsics are the renderer's: tracking.project lands on the integers again, and the view-space z is the depth.
    The cameras' matrices are float32 data (2^-24 relative) and a pixel coordinate reaches 40: 1e-3 pixel covers either dtype."""
    from csplat import tracking as tk
    W, H = 41, 23
    cams = [camera(-40.0, W, H), camera(75.0, W, H, phi_deg=-60.0, radius=3.0)]
    rng = np.random.default_rng(1)
    depth = torch.from_numpy(rng.uniform(1.0, 6.0, (2, H, W))).to(dt)
    depth[0, 3, 4] = 0.0
    cloud = ob.unproject_depth(depth, cameras=cams)
    assert cloud.points.shape == (2 * H * W - 1, 3) and cloud.points.dtype == dt
    for v, cam in enumerate(cams):
        on = cloud.view == v
        pix = tk.project(cloud.points[on].float(), cam)
        src = cloud.source[on] - v * H * W
        want = torch.stack([src % W, src // W], 1).to(pix.dtype)
        assert float((pix - want).abs().max()) < 1e-3
        z = (torch.cat([cloud.points[on].double(), torch.ones(int(on.sum()), 1, dtype=F64)], 1) @ cam.world_view_transform.double())[:, 2]
        assert float((z - depth[v].reshape(-1)[src].double()).abs().max()) < 1e-5
    # the reference's convention differs by half a pixel: explicit intrinsics
    k = [W / (2 * math.tan(cams[0].FoVx / 2)), H / (2 * math.tan(cams[0].FoVy / 2)), W / 2, H / 2]
    c2w = torch.from_numpy(ob.camera_to_world(cams[0]))
    ref = ob.unproject_depth(depth[0], intrinsics=torch.tensor(k, dtype=F64), cam_to_world=c2w)
    pix = tk.project(ref.points.float(), cams[0])
    want = torch.stack([ref.source % W, ref.source // W], 1).to(pix.dtype) - 0.5
    assert float((pix - want).abs().max()) < 1e-3


def test_unproject_argument_errors():
    d, k, m = torch.ones(2, 3, 4), torch.ones(2, 4), torch.tensor([EYE34, EYE34])
    cams = [camera(0.0, 4, 3), camera(10.0, 4, 3)]
    bad = [
        (dict(depth=torch.ones(2, 2, 3, 4)), r"\[V,H,W\]"), (dict(depth=[]), "empty list"), (dict(depth=[torch.ones(2, 3, 4)]), r"\[1,H,W\]"),
        (dict(depth=[torch.ones(3, 4), torch.ones(3, 5)]), "share one size"), (dict(depth=torch.ones(2, 3, 4, dtype=torch.int32)), "floating point"),
        (dict(depth="x"), "tensor or numpy"), (dict(depth=torch.ones(2, 0, 4)), "1 to 65535 views"), (dict(kind="w"), "kind"),
        (dict(stride=0), "stride"), (dict(stride=1.5), "stride"), (dict(stride=True), "stride"), (dict(max_depth=NAN), "max_depth"),
        (dict(intrinsics=None), "pass `cameras`, or both"), (dict(cam_to_world=None), "pass `cameras`, or both"),
        (dict(cameras=cams), "not both"), (dict(intrinsics=torch.ones(3, 4)), "intrinsics"), (dict(intrinsics=torch.ones(2, 3)), "intrinsics"),
        (dict(cam_to_world=torch.ones(2, 3, 3)), "cam_to_world"), (dict(cam_to_world=torch.ones(3, 3, 4)), "cam_to_world"),
        (dict(masks=torch.ones(2, 3, 5)), "masks"), (dict(masks=torch.ones(1, 3, 4)), "masks"),
    ]
    for kw, text in bad:
        args = dict(depth=d, intrinsics=k, cam_to_world=m)
        args.update(kw)
        with pytest.raises(ValueError, match=text):
            ob.unproject_depth(args.pop("depth"), **args)
    with pytest.raises(ValueError, match="1 cameras for 2 views"):
        ob.unproject_depth(d, cameras=cams[:1])
    broken = SimpleNamespace(world_view_transform=torch.ones(3, 3), FoVx=1.0, FoVy=1.0)
    with pytest.raises(ValueError, match="world_view_transform"):
        ob.unproject_depth(d[:1], cameras=[broken])


# ------------------------------------------------------------------------------------------------------------------ voxel grid
def _check_voxels(points, size, origin=None):
    for dt, npdt, tol in ((F32, np.float32, 2e-6), (F64, np.float64, 1e-12)):
        got = ob.voxel_downsample(torch.from_numpy(points).to(dt), size, origin=origin)
        want = R.voxel(points, size, origin, npdt)
        assert isinstance(got, ob.Voxels) and got.centroids.dtype == dt and got.counts.dtype == torch.int32 and got.inverse.dtype == torch.int64
        if dt == F32:          # (the float64 path takes its cells in float64: they can differ on a face)
            assert np.array_equal(got.counts.numpy(), want["counts"]) and np.array_equal(got.inverse.numpy(), want["inverse"])
            scale = max(float(np.abs(want["centroids"]).max()), 1.0) if len(want["counts"]) else 1.0
            assert got.centroids.shape == want["centroids"].shape
            assert len(want["counts"]) == 0 or np.abs(got.centroids.numpy() - want["centroids"]).max() <= tol * scale
    return want


def test_voxel_on_cpu_tensors_equals_the_restatement():
    rng = np.random.default_rng(3)
    generic = rng.uniform(-1.0, 1.0, (5000, 3)).astype(np.float32)
    w = _check_voxels(generic, 0.4)
    assert 100 <= len(w["counts"]) <= 216 and w["counts"].sum() == 5000 and (np.diff(w["keys"]) > 0).all() and w["outside"] == 0
    # the centroid of a voxel is the mean of its points (float64), and lies in its cell
    c64 = R.voxel(generic, 0.4, None, np.float64)
    for q in (0, len(w["counts"]) // 2, len(w["counts"]) - 1):
        assert np.abs(c64["centroids"][q] - generic[c64["inverse"] == q].astype(np.float64).mean(0)).max() < 1e-12
    assert np.abs(w["centroids"] - c64["centroids"]).max() < 1e-5
    one_cell = (rng.uniform(0.1, 0.2, (3000, 3)) + [5.0, -3.0, 0.0]).astype(np.float32)
    w = _check_voxels(one_cell, 1.0)
    assert w["counts"].tolist() == [3000]
    own = (np.stack(np.meshgrid(np.arange(7), np.arange(5), np.arange(3), indexing="ij"), -1).reshape(-1, 3) + 0.5).astype(np.float32)
    w = _check_voxels(own[rng.permutation(len(own))], 1.0)
    assert (w["counts"] == 1).all() and len(w["counts"]) == 105
    _check_voxels(np.array([[1.0, 2.0, 3.0]], np.float32), 0.25)
    rows = generic[:200].copy()
    rows[[3, 50, 199], [0, 1, 2]] = [NAN, INF, -INF]
    w = _check_voxels(rows, 0.4)
    assert (w["inverse"][[3, 50, 199]] == -1).all() and (np.delete(w["inverse"], [3, 50, 199]) >= 0).all() and w["counts"].sum() == 197


def test_voxel_known_answers():
    below = float(np.nextafter(np.float32(0.5), np.float32(0.0)))
    # points exactly on cell faces belong to the upper cell; explicit origin
    p = torch.tensor([[0.0, 0.0, 0.0], [0.5, 0.0, 0.0], [below, 0.0, 0.0], [1.0, 0.0, 0.0], [1.5, 0.5, 0.0], [0.25, 0.0, 0.5]])
    v = ob.voxel_downsample(p, 0.5, origin=[0.0, 0.0, 0.0])
    assert v.inverse.tolist() == [0, 1, 0, 2, 3, 4] and v.counts.tolist() == [2, 1, 1, 1, 1]            # ascending (cz, cy, cx)
    assert v.centroids.tolist() == [[below / 2, 0.0, 0.0], [0.5, 0.0, 0.0], [1.0, 0.0, 0.0], [1.5, 0.5, 0.0], [0.25, 0.0, 0.5]]
    # an origin that is no multiple of the size shifts the faces
    v = ob.voxel_downsample(p[:4], 0.5, origin=(-0.25, -1.0, -8.0))
    assert v.inverse.tolist() == [0, 1, 1, 2] and v.counts.tolist() == [1, 2, 1]
    # negative coordinates: the default origin is the minimum, so every cell is >= 0
    n = torch.tensor([[-3.0, -1.0, -2.0], [-2.75, -1.0, -2.0], [-1.0, 5.0, -1.5], [NAN, -100.0, 0.0]])
    v = ob.voxel_downsample(n, 0.5)
    assert v.inverse.tolist() == [0, 0, 1, -1] and v.counts.tolist() == [2, 1] and v.centroids.tolist() == [[-2.875, -1.0, -2.0], [-1.0, 5.0, -1.5]]
    # below an explicit origin, or 2^21 cells away: outside the grid
    with pytest.raises(ValueError, match="1 finite points lie outside"):
        ob.voxel_downsample(n, 0.5, origin=[-2.9, -1.0, -2.0])
    with pytest.raises(ValueError, match="outside"):
        ob.voxel_downsample(torch.tensor([[0.0, 0.0, 0.0], [0.0, float(2 ** 21), 0.0]]), 1.0)
    far = ob.voxel_downsample(torch.tensor([[0.0, 0.0, 0.0], [0.0, float(2 ** 21 - 1), 0.0]]), 1.0)
    assert far.counts.tolist() == [1, 1]
    empty = ob.voxel_downsample(torch.zeros(0, 3), 1.0)
    assert empty.centroids.shape == (0, 3) and empty.counts.shape == (0,) and empty.inverse.shape == (0,)
    cloud = ob.Cloud(p, torch.arange(6), torch.zeros(6, dtype=torch.int64))
    assert torch.equal(ob.voxel_downsample(cloud, 0.5, origin=[0.0, 0.0, 0.0]).inverse, torch.tensor([0, 1, 0, 2, 3, 4]))
    for kw, text in ((dict(voxel_size=0.0), "voxel_size"), (dict(voxel_size=-1.0), "voxel_size"), (dict(voxel_size=NAN), "voxel_size"),
                     (dict(voxel_size=INF), "voxel_size"), (dict(origin=[0.0, 1.0]), "origin"), (dict(origin=[0.0, NAN, 0.0]), "origin"),
                     (dict(points=torch.ones(4, 2)), r"\[n,3\]"), (dict(points=torch.ones(4, 3, dtype=torch.int64)), "floating point")):
        args = dict(points=p, voxel_size=0.5)
        args.update(kw)
        with pytest.raises(ValueError, match=text):
            ob.voxel_downsample(args.pop("points"), args.pop("voxel_size"), **args)


# ------------------------------------------------------------------------------------------------------------------ observable nodes
def test_observable_nodes_on_cpu_tensors():
    rng = np.random.default_rng(5)
    cloud, nodes = rng.normal(size=(700, 3)).astype(np.float32), (2.0 * rng.normal(size=(300, 3))).astype(np.float32)
    for k, max_dist in ((1, None), (2, None), (2, 0.3), (5, 0.5), (2, 1e-6)):
        got = ob.observable_nodes(torch.from_numpy(cloud), torch.from_numpy(nodes), k=k, max_dist=max_dist)
        assert np.array_equal(got.numpy(), R.observable(cloud, nodes, k, max_dist)), (k, max_dist)
    assert not R.observable(cloud, nodes, 2, 1e-6).any() and 0 < R.observable(cloud, nodes, 2, 0.3).sum() < R.observable(cloud, nodes, 2).sum()
    # known answers: nodes on a line, ties to the smaller index
    line = torch.tensor([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [2.0, 0.0, 0.0], [3.0, 0.0, 0.0]])
    q = torch.tensor([[0.5, 0.0, 0.0], [2.9, 0.0, 0.0]])
    assert ob.observable_nodes(q, line, k=1).tolist() == [True, False, False, True]
    assert ob.observable_nodes(q, line, k=2).tolist() == [True, True, True, True]
    assert ob.observable_nodes(q, line, k=2, max_dist=0.5).tolist() == [True, True, False, True]
    assert ob.observable_nodes(q[:1], line[:1], k=1).tolist() == [True]
    assert ob.observable_nodes(torch.zeros(0, 3), line, k=2).tolist() == [False] * 4
    vox = ob.Voxels(q, torch.ones(2, dtype=torch.int32), torch.arange(2))
    assert ob.observable_nodes(vox, line, k=1).tolist() == [True, False, False, True]
    import simple_knn
    for kw, text in ((dict(k=0), "k is an integer"), (dict(k=5), "k is an integer"), (dict(k=2.0), "k is an integer"), (dict(max_dist=-1.0), "max_dist"),
                     (dict(max_dist=NAN), "max_dist"), (dict(nodes=torch.ones(4, 2)), r"\[n,3\]"), (dict(cloud=torch.ones(3)), r"\[n,3\]")):
        args = dict(cloud=q, nodes=line)
        args.update(kw)
        with pytest.raises(ValueError, match=text):
            ob.observable_nodes(args.pop("cloud"), args.pop("nodes"), **args)
    with pytest.raises(ValueError, match="k is an integer"):
        ob.observable_nodes(q, torch.zeros(100, 3), k=simple_knn.MAX_K + 1)


def test_camera_points_reads_depth_and_silhouette_or_mask():
    W, H = 13, 9
    rng = np.random.default_rng(2)
    cams = [camera(20.0 * i, W, H) for i in range(3)]
    depth = rng.uniform(2.0, 5.0, (3, H, W)).astype(np.float32)
    sil = (rng.random((3, H, W)) < 0.4).astype(np.float32)
    cams[0].depth, cams[0].silhouette, cams[0].mask = torch.from_numpy(depth[0])[None], torch.from_numpy(sil[0])[None], torch.zeros(1, H, W)
    cams[1].depth, cams[1].mask = torch.from_numpy(depth[1]), torch.from_numpy(sil[1])
    cams[2].depth = torch.from_numpy(depth[2])[None]
    sil[2] = 1.0
    intr = np.stack([R.camera_intrinsics(c.FoVx, c.FoVy, H, W) for c in cams]).astype(np.float32)
    c2w = np.stack([ob.camera_to_world(c) for c in cams]).astype(np.float32)
    want = R.unproject(depth, intr, c2w, sil)[0]
    got = ob.camera_points(cams)
    assert got.shape == want.shape and got.dtype == F32 and np.abs(got.numpy() - want).max() < 2e-6
    thin = ob.camera_points(cams, voxel_size=0.3, stride=2, max_depth=4.5)
    w2 = R.voxel(R.unproject(depth, intr, c2w, sil, 2, 4.5)[0], 0.3)
    assert thin.shape == w2["centroids"].shape and np.abs(thin.numpy() - w2["centroids"]).max() < 1e-5
    with pytest.raises(ValueError, match="empty"):
        ob.camera_points([])
    with pytest.raises(ValueError, match="depth"):
        ob.camera_points([camera(0.0, W, H)])


# ------------------------------------------------------------------------------------------------------------------ the library's surface
ENTRIES = (("int", "csplat_obs_unproject", 16), ("size_t", "csplat_obs_unproject_temp_bytes", 3), ("int", "csplat_obs_voxel", 11),
           ("size_t", "csplat_obs_voxel_temp_bytes", 1), ("int", "csplat_obs_mark", 8))


def test_header_exports_and_bindings():
    from csplat import native
    header = open(os.path.join(ROOT, "include", "csplat.h")).read()
    for res, name, n_args in ENTRIES:
        assert re.search(r"\b" + res + " " + name + r"\s*\(", header), name
        assert name in native.EXPORTS and hasattr(native.lib, name) and len(native.EXPORTS[name][1]) == n_args
        decl = header[header.index(res + " " + name + "("):]
        decl = re.sub(r"/\*.*?\*/", "", decl[:decl.index(";")], flags=re.S)
        assert decl.count(",") + 1 == n_args, (name, decl)
    block = header[header.index("/* Observation clouds"):header.index("size_t csplat_obs_unproject_temp_bytes(")]
    assert block.rstrip().endswith("Added exports: CSPLAT_ABI_VERSION is unchanged. */")
    for word in ("pixel centres at the integers", "(v H + y) W + x", "FULL count", "NO atomics", "bit-reproducible", "floorf((p - o) / voxel)",
                 "cz << 42 | cy << 21 | cx", "[0, 2^21)", "inverse = -1", "correctly rounded", "zeroes flags on the stream", "mask > 0.5"):
        assert word.lower() in block.lower(), word
    assert native.ABI_VERSION == 9 and native.lib.csplat_abi_version() == 9
    src = open(os.path.join(ROOT, "cloth-splatting_amd", "csrc", "csplat_observation.hip")).read()
    device = open(os.path.join(ROOT, "cloth-splatting_amd", "csrc", "csplat_device.h")).read()
    code = re.sub(r"//.*", "", src)
    assert '#include "csplat_device.h"' in code and "atomic" not in re.sub(r"//.*", "", device).lower()      # all the code the file runs
    assert "atomic" not in code.lower() and "#pragma clang fp contract(off)" in code and "__fdiv_rn(__fsub_rn(" in code
    assert ob.CELL_BITS == R.CELL_BITS == int(re.search(r"OB_CELL_BITS = (\d+)", src).group(1)) == 21


def test_the_library_refuses_bad_arguments_before_any_launch():
    """fake, distinct, aligned addresses 2^32 apart: every call here must be refused (or be a no-op) before a launch could touch them"""
    from csplat import native
    L = native.lib
    A = lambda i: (i + 1) << 32  # noqa: E731
    assert L.csplat_obs_unproject_temp_bytes(4, 800, 800) >= 4 * 800 * 800 * 5 and L.csplat_obs_unproject_temp_bytes(0, 8, 8) == 0
    assert L.csplat_obs_unproject_temp_bytes(1, 1, 1) > 0 and L.csplat_obs_voxel_temp_bytes(1000) >= 1000 * 36 and L.csplat_obs_voxel_temp_bytes(0) > 0
    un = lambda V=2, H=3, W=4, depth=A(0), mask=A(1), intr=A(2), c2w=A(3), stride=1, far=0.0, kind=0, cap=24, pts=A(4), src=A(5), cnt=A(6), tmp=A(7): \
        L.csplat_obs_unproject(None, V, H, W, depth, mask, intr, c2w, stride, far, kind, cap, pts, src, cnt, tmp)  # noqa: E731
    for kw in (dict(V=0), dict(V=65536), dict(H=0), dict(W=-1), dict(V=40000, H=40000, W=2), dict(stride=0), dict(kind=2), dict(kind=-1), dict(far=NAN),
               dict(cap=-1), dict(cap=2 ** 31), dict(depth=None), dict(intr=None), dict(c2w=None), dict(cnt=None), dict(tmp=None), dict(pts=None),
               dict(src=None), dict(depth=A(0) + 2), dict(pts=A(4) + 1), dict(tmp=A(7) + 4), dict(pts=A(0)), dict(src=A(0) + 16), dict(cnt=A(4) + 8),
               dict(tmp=A(1)), dict(pts=A(5) - 8), dict(mask=A(4) + 16), dict(intr=A(7))):
        assert un(**kw) == 2, kw
        assert b"csplat_obs_unproject" in L.csplat_last_error(), kw
    vx = lambda M=10, pts=A(0), size=0.5, org=A(1), cen=A(2), cnt=A(3), inv=A(4), nv=A(5), no=A(6), tmp=A(7): \
        L.csplat_obs_voxel(None, M, pts, size, org, cen, cnt, inv, nv, no, tmp)  # noqa: E731
    for kw in (dict(M=-1), dict(M=2 ** 31), dict(size=0.0), dict(size=-1.0), dict(size=NAN), dict(size=INF), dict(nv=None), dict(no=None), dict(pts=None),
               dict(cen=None), dict(cnt=None), dict(inv=None), dict(tmp=None), dict(pts=A(0) + 2), dict(tmp=A(7) + 8), dict(nv=A(5) + 1), dict(cen=A(0)),
               dict(inv=A(3) + 4), dict(nv=A(6)), dict(no=A(2) + 8), dict(org=A(2) + 12), dict(tmp=A(0))):
        assert vx(**kw) == 2, kw
        assert b"csplat_obs_voxel" in L.csplat_last_error(), kw
    mk = lambda Q=10, K=2, N=5, idx=A(0), d2=A(1), cap=-1.0, flags=A(2): L.csplat_obs_mark(None, Q, K, N, idx, d2, cap, flags)  # noqa: E731
    for kw in (dict(Q=-1), dict(K=0), dict(Q=2 ** 30, K=2), dict(Q=2 ** 31), dict(N=-1), dict(cap=NAN), dict(flags=None), dict(idx=None), dict(d2=None),
               dict(idx=A(0) + 2), dict(d2=A(1) + 1), dict(flags=A(0) + 8), dict(flags=A(1) - 2)):
        assert mk(**kw) == 2, kw
        assert b"csplat_obs_mark" in L.csplat_last_error(), kw
    assert mk(N=0) == 0 and mk(N=0, flags=None, idx=None, d2=None) == 0          # nothing to mark: no launch, no error
