"""The Delaunay triangulation on the GPU (csrc/csplat_delaunay.hip behind csplat.triangulate) against tests/delaunay_ref.py: its faces equal
the Python walk's face for face, pass the definition's check in integers, and are bit-equal on a second run; on the tie-free fixture clouds
they equal SciPy's; the length filter equals the reference's loop restated; and the delaunay=True paths above it -- compute_edges_index,
process_traj, the sample data set, compute_mesh, MeshGaussians.from_vertices, get_mesh.  Every comparison is exact.

Shapes.  One wave per point, its 64 lanes strided over the candidates, four waves a workgroup: N = 0, 1, 2, 3 (no launch; no neighbour; no
face; one face), 63, 64, 65 (a wave's lanes and one over) and 96; the degenerate clouds of delaunay_ref.degenerate_clouds (every step of a
grid's walk ties; a centre that owns more faces than the counting walk keeps per point; denormal, huge and mixed magnitudes); the
fixture's N = 2048 is the largest shape."""
import ctypes as C
import types

import numpy as np
import pytest

import util  # noqa: F401
import delaunay_ref as R

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
from csplat import native, triangulate  # noqa: E402
from csplat.gaussians import MeshGaussians  # noqa: E402
from meshnet import data_utils as du  # noqa: E402
from meshnet import gaussian_sampling  # noqa: E402
from meshnet.dataloader_sim import SamplesClothSimDataset, face_to_edge  # noqa: E402

DEGENERATE = R.degenerate_clouds()
SIZES = R.size_clouds()


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def rows(t):
    """[3,M] or [2,E] tensor -> list of tuples"""
    return [tuple(r) for r in t.t().cpu().numpy().tolist()]


def run_twice(pts, thr=None):
    a, b = triangulate.delaunay(cu(pts), thr), triangulate.delaunay(cu(pts), thr)
    assert a.faces.dtype == a.edge_index.dtype == torch.int64 and a.faces.shape[0] == 3 and a.edge_index.shape[0] == 2
    assert a.faces.is_cuda and a.faces.is_contiguous() and a.edge_index.is_contiguous()
    assert torch.equal(a.faces, b.faces) and torch.equal(a.edge_index, b.edge_index) and a[2:] == b[2:]
    return a


@pytest.fixture(scope="module")
def fixture():
    return R.load_fixture()


# ------------------------------------------------------------------------------------------------------------------------------ the faces
@pytest.mark.parametrize("name", list(SIZES))
def test_sizes_around_a_wave(name):
    pts = SIZES[name]
    t = run_twice(pts)
    want = R.walk(pts)
    assert rows(t.faces) == want and R.check(pts, rows(t.faces)) == 0
    assert rows(t.edge_index) == R.edges_of(want) and t.n_skipped == 0
    if len(pts) < 3:
        assert t.faces.shape == (3, 0) and t.edge_index.shape == (2, 0) and t.exact_decisions == 0


@pytest.mark.parametrize("name", list(DEGENERATE))
def test_degenerate_clouds_face_for_face(name):
    pts, skipped = DEGENERATE[name]
    t = run_twice(pts)
    got, want = rows(t.faces), R.walk(pts)
    print(f"{name}: N = {len(pts)}, M = {len(got)}, exact decisions = {t.exact_decisions}, skipped = {t.n_skipped}")
    assert got == want
    ties = R.check(pts, got)
    assert rows(t.edge_index) == R.edges_of(want) and t.n_skipped == skipped
    if name.startswith(("grid", "circle", "square")):
        assert t.exact_decisions > 0
    if name.startswith("grid") or name in ("square", "circle65"):
        assert ties > 0
    if name == "collinear4":
        # known answer: per point two searches for an apex with two collinear candidates each (4 orientations that the filter cannot
        # take), and points 1 and 3 have their two neighbours equally far (1 distance comparison each)
        assert got == [] and t.edge_index.shape == (2, 0) and t.exact_decisions == 4 * 4 + 2
    if name == "square":
        # per point: its two neighbours along the sides are equally far (1), and one apex search has the two cocircular candidates (1)
        assert t.exact_decisions == 4 * 2
    if name == "circle65_centre":
        # point 0, the centre, owns more faces and edges than the counting walk keeps per point: its segments come from the second walk
        assert sum(f[0] == 0 for f in want) == 36 and sum(e[0] == 0 for e in R.edges_of(want)) == 36


def test_scaling_by_a_power_of_two_changes_no_decision():
    """the same lattice circle with every coordinate a float32 denormal: the faces and the number of exact decisions are those of the
    unscaled cloud (a power of two scales every filter value and its bound alike)"""
    a, b = triangulate.delaunay(cu(DEGENERATE["circle65"][0])), triangulate.delaunay(cu(DEGENERATE["circle65_denormal"][0]))
    assert torch.equal(a.faces, b.faces) and torch.equal(a.edge_index, b.edge_index) and a.exact_decisions == b.exact_decisions > 0


def test_fixture_clouds_equal_scipy(fixture):
    for n, (pts, faces) in fixture.items():
        t = run_twice(pts)
        got = rows(t.faces)
        assert set(got) == {tuple(f) for f in faces.tolist()} and len(got) == len(faces), n
        assert got == sorted(got) and R.check(pts, got) == 0 and t.n_skipped == 0
        assert rows(t.edge_index) == R.edges_of(got)


# -------------------------------------------------------------------------------------------------------------------------- the threshold
def test_threshold_equals_the_reference_loop(fixture):
    for pts, faces in (fixture[300], (DEGENERATE["circle65_inner"][0], None), (DEGENERATE["hull_collinear"][0], None)):
        full = triangulate.delaunay(cu(pts))
        all_faces = rows(full.faces)
        if faces is not None:
            assert all_faces == [tuple(f) for f in faces.tolist()]
        thr = R.gap_threshold(pts, all_faces)
        edges, kept = R.threshold_loop(pts, all_faces, thr)
        t = run_twice(pts, thr)
        assert rows(t.edge_index) == edges and rows(t.faces) == kept
        assert 0 < len(edges) < full.edge_index.shape[1] and len(kept) < len(all_faces)
        every, same = R.threshold_loop(pts, all_faces, None)
        assert rows(full.edge_index) == every and all_faces == same
        wide = triangulate.delaunay(cu(pts), 1e300)                              # (float)1e300 = +inf: nothing is longer
        assert torch.equal(wide.faces, full.faces) and torch.equal(wide.edge_index, full.edge_index)
        none = triangulate.delaunay(cu(pts), 0.0)
        assert none.faces.shape == (3, 0) and none.edge_index.shape == (2, 0)


def test_temp_is_exactly_sized_and_needs_no_initial_state(fixture):
    """hostile temp contents, guard bytes behind the size the library reports, sentinels behind the rows the counters name"""
    pts, faces = fixture[257]
    N = len(pts)
    want = triangulate.delaunay(cu(pts))
    need = triangulate.temp_bytes(N)
    dev = torch.device("cuda:0")
    for fill in (0xFF, 0x00, 0xA5):
        temp = torch.full((need + 512,), fill, dtype=torch.uint8, device=dev)
        temp[need:] = 0x5A
        f = torch.full((2 * N, 3), -7, dtype=torch.int32, device=dev)
        e = torch.full((3 * N, 2), -7, dtype=torch.int32, device=dev)
        c = torch.full((5,), -7, dtype=torch.int64, device=dev)
        native.launch("csplat_delaunay", dev, N, native.ptr(cu(pts)), 0, 0.0, native.ptr(f), native.ptr(e), native.ptr(c), native.ptr(temp))
        M, E, skipped, exact, status = c.tolist()
        assert (M, E, skipped, exact, status) == (want.faces.shape[1], want.edge_index.shape[1], 0, want.exact_decisions, 0)
        assert torch.equal(f[:M].t().long(), want.faces) and torch.equal(e[:E].t().long(), want.edge_index)
        assert bool((f[M:] == -7).all()) and bool((e[E:] == -7).all()) and bool((temp[need:] == 0x5A).all())
    c = torch.full((5,), -7, dtype=torch.int64, device=dev)
    native.launch("csplat_delaunay", dev, 0, None, 0, 0.0, None, None, native.ptr(c), None)          # N = 0: the counters alone
    assert c.tolist() == [0, 0, 0, 0, 0]
    size = C.c_size_t(1)
    assert native.lib.csplat_delaunay_temp_bytes(0, C.byref(size)) == 0 and size.value == 0


# --------------------------------------------------------------------------------------------------------------------- the paths above it
def cloud3(pts2, sim_data, seed=0):
    """[N,2] -> [N,3] with the plane's coordinates where the projection reads them and noise in the third"""
    other = np.random.default_rng(seed).random(len(pts2)).astype(np.float32)
    cols = (pts2[:, 0], other, pts2[:, 1]) if sim_data else (pts2[:, 0], pts2[:, 1], other)
    return np.stack(cols, 1).astype(np.float32)


def test_compute_edges_index_delaunay(fixture):
    pts2, faces = fixture[300]
    thr = R.gap_threshold(pts2, [tuple(f) for f in faces.tolist()])
    for sim_data in (False, True):
        p3 = cloud3(pts2, sim_data)
        for t in (None, thr):
            want = triangulate.delaunay(cu(pts2), t)
            for given in (cu(p3), p3, cu(p3).double(), p3.astype(np.float64)):
                ei, f = du.compute_edges_index(given, k=3, delaunay=True, sim_data=sim_data, norm_threshold=t)
                assert ei.is_cuda and f.is_cuda and ei.dtype == f.dtype == torch.int64
                assert torch.equal(ei, want.edge_index) and torch.equal(f, want.faces)
    # the other projection is another triangulation: the argument is read
    assert not torch.equal(du.compute_edges_index(cu(cloud3(pts2, True)), delaunay=True, sim_data=False, norm_threshold=None)[1],
                           triangulate.delaunay(cu(pts2)).faces)
    # the default threshold is the reference's 0.01
    ei, f = du.compute_edges_index(cu(cloud3(pts2, False)), delaunay=True)
    want = triangulate.delaunay(cu(pts2), 0.01)
    assert torch.equal(ei, want.edge_index) and torch.equal(f, want.faces)
    # delaunay=False is what it was: one tensor, the kNN graph
    knn = du.compute_edges_index(cu(cloud3(pts2, False)), k=3)
    assert torch.is_tensor(knn) and knn.shape[0] == 2


def jittered_grid(n=9, spacing=0.05, seed=4):
    rng = np.random.default_rng(seed)
    g = R.grid(n, spacing).astype(np.float64) + rng.uniform(-0.3, 0.3, (n * n, 2)) * spacing
    return g.astype(np.float32)


def test_process_traj_delaunay():
    pts2 = jittered_grid()
    N = len(pts2)
    for sim_data in (False, True):
        p0 = cloud3(pts2, sim_data)
        p0[:, 1 if sim_data else 2] *= np.float32(0.01)                         # nearly flat: 3-D lengths are close to the plane's
        traj = cu(np.stack([p0, p0 * np.float32(1.1), p0 * np.float32(1.2)]))
        tri = triangulate.delaunay(cu(pts2))
        thr = R.gap_threshold(pts2, rows(tri.faces), quantile=0.8)
        ei0, f0 = du.compute_edges_index(traj[0], delaunay=True, sim_data=sim_data, norm_threshold=thr)
        d = du.process_traj(traj, 0.05, k=3, delaunay=True, sim_data=sim_data, norm_threshold=thr)
        M = f0.shape[1]
        assert 0 < M < tri.faces.shape[1]
        assert d["edge_faces"].shape == (3, 3, M) and all(torch.equal(d["edge_faces"][t], f0) for t in range(3))
        assert d["pos"].shape == (3, N, 3) and d["velocity"].shape == (3, N, 3) and d["node_type"].shape == (3, N, 1)
        if sim_data:                                                            # the frame-1 pruning stays: edges whose frame-1 norm is >= thr go
            _v, _disp, norm = du.trajectory_features(traj, ei0, 0.05)
            keep = norm[1, :, 0] < thr
            assert 0 < int(keep.sum()) < ei0.shape[1]
            want = ei0[:, keep]
        else:
            want = ei0
        E = want.shape[1]
        assert d["edge_index"].shape == (3, 2, E) and torch.equal(d["edge_index"][0], want) and torch.equal(d["edge_index"][2], want)
        assert d["edge_displacement"].shape == (3, E, 3) and d["edge_norm"].shape == (3, E, 1)
        _v, disp, _n = du.trajectory_features(traj, want, 0.05)
        assert torch.equal(d["edge_displacement"][2], disp[2]) and torch.equal(d["edge_displacement"][0], disp[1])
        # an explicit edge_index still wins: nothing is triangulated, the given faces are carried
        given, gf = torch.tensor([[0, 1, 2], [1, 2, 3]], device="cuda"), torch.tensor([[0], [1], [2]], device="cuda")
        e = du.process_traj(traj, 0.05, delaunay=True, sim_data=False, edge_index=given, faces=gf)
        assert torch.equal(e["edge_index"][0], given) and torch.equal(e["edge_faces"][1], gf)
        assert du.process_traj(traj, 0.05, delaunay=True, edge_index=given)["edge_faces"] is None
    # numpy in: CPU tensors out, the same triangulation
    n = du.process_traj(traj.cpu().numpy(), 0.05, delaunay=True, sim_data=True, norm_threshold=thr)
    assert all(torch.is_tensor(n[k]) and n[k].device.type == "cpu" for k in n) and torch.equal(n["edge_faces"], d["edge_faces"].cpu())
    assert torch.equal(n["edge_index"], d["edge_index"].cpu())


def test_dataset_chain_with_delaunay():
    """SamplesClothSimDataset(delaunay=True): collect_observation(first=True) -> batch(): the network's edges are face_to_edge(faces)"""
    pts2 = jittered_grid()
    N, T_ = len(pts2), 6
    p0 = cloud3(pts2, True)                                                     # sim_data swaps y and z: the plane is (x, z) before, (x, y) after
    p0[:, 1] = 0.0
    pos = cu(np.stack([p0 + np.float32(0.001 * t) for t in range(T_)]))
    grip = cu(np.stack([p0[5] + np.float32(0.001 * t) for t in range(T_)]))
    obs = {"pos": pos, "gripper_pos": grip, "pick": cu(p0[5]), "place": cu(p0[60]), "actions": torch.full((T_, 3), 0.001, device="cuda")}
    ds = SamplesClothSimDataset(None, 2, types.SimpleNamespace(action_steps=1, future_sequence_length=2), dt=0.05, delaunay=True)
    ds.collect_observation(obs, first=True)
    tr = ds.trajectory(0)
    want = triangulate.delaunay(cu(pts2), 0.1)                                  # get_data_traj's norm_threshold
    assert tr["faces"] is not None and torch.equal(tr["faces"], want.faces) and want.faces.shape[1] > 100
    edges = face_to_edge(want.faces, N)
    assert torch.equal(tr["edge_index"], edges)
    b = ds.batch([0])
    assert b.positions.shape == (N, 3) and torch.equal(b.edge_index, edges)
    b2 = ds.batch([0, len(ds) - 1])
    assert torch.equal(b2.edge_index, torch.cat([edges, edges + N], 1))
    ds.collect_observation(obs, first=False)                                    # the next round replaces the trajectory: the same mesh
    assert ds.num_trajectories == 1 and torch.equal(ds.trajectory(0)["faces"], want.faces)


def test_compute_mesh_from_vertices_and_get_mesh():
    pts2 = jittered_grid(7)
    N = len(pts2)
    flat = np.concatenate([pts2, np.full((N, 1), 0.25, np.float32)], 1)
    verts = cu(flat)
    tri = triangulate.delaunay(cu(pts2))
    mesh = du.compute_mesh(verts)
    assert torch.equal(mesh.pos, verts) and torch.equal(mesh.face, tri.faces) and torch.equal(mesh.edge_index, face_to_edge(tri.faces, N))
    assert mesh.edge_index.shape[1] == 2 * tri.edge_index.shape[1]
    assert mesh.norm.shape == (N, 3) and torch.equal(mesh.norm, torch.tensor([0.0, 0.0, 1.0], device="cuda").expand(N, 3))
    bumpy = flat.copy()
    bumpy[:, 2] += np.random.default_rng(1).uniform(-0.01, 0.01, N).astype(np.float32)
    nb = du.compute_mesh(bumpy).norm                                            # numpy in: on the GPU
    assert nb.is_cuda and bool((nb[:, 2] > 0).all()) and float((nb.norm(dim=1) - 1).abs().max()) < 1e-6
    # from_vertices = compute_mesh, then from_mesh
    g = MeshGaussians(0).from_vertices(verts, gaussian_init_factor=2, generator=torch.Generator(device="cuda").manual_seed(0))
    M = tri.faces.shape[1]
    assert g.face_bary.shape == (2 * M, 3) and torch.equal(g.mesh.face, tri.faces) and torch.equal(g.mesh.norm, mesh.norm)
    xyz = g.get_xyz().detach()
    corners = verts[tri.faces.t()[g.face_ids]]                                  # [P,3,3]
    a, b_, c = corners[:, 0, :2].double(), corners[:, 1, :2].double(), corners[:, 2, :2].double()
    p = xyz[:, :2].double()
    cross = lambda u, v: u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0]  # noqa: E731
    area = cross(b_ - a, c - a)
    bary = torch.stack([cross(b_ - p, c - p), cross(c - p, a - p), cross(a - p, b_ - p)], 1) / area[:, None]
    assert bool((area > 0).all()) and float(bary.min()) > -1e-5 and float((xyz[:, 2] - 0.25).abs().max()) < 1e-6
    # get_mesh: the edges once each, the triangles' corners
    edges, tv = gaussian_sampling.get_mesh(verts)
    assert torch.equal(edges, tri.edge_index.t()) and torch.equal(tv, verts[tri.faces.t()]) and tv.shape == (M, 3, 3)
    edges_np, tv_np = gaussian_sampling.get_mesh(flat.astype(np.float64))
    assert isinstance(edges_np, np.ndarray) and np.array_equal(edges_np, edges.cpu().numpy()) and tv_np.dtype == np.float64
    assert np.array_equal(tv_np, flat.astype(np.float64)[tri.faces.t().cpu().numpy()])
    means = gaussian_sampling.sample_gaussian_means(tv, torch.full((2, M, 3), 1.0 / 3.0, device="cuda"), 2)
    assert means.shape == (2, M, 3) and float((means[0] - tv.mean(1)).abs().max()) < 1e-6
