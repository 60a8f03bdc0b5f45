"""Trajectory preprocessing on the GPU (csplat_traj_smooth in csrc/csplat_knn.hip, csplat_traj_features in csrc/csplat_trajectory.hip, behind
meshnet.data_utils) against the restatement tests/trajectory_ref.py, under strict dispatch.

Exact parts are compared for equality: the neighbour lists with simple_knn.knn_query(frame, frame, k) and with the float32 restatement, a
[T,N,3] call with T single-frame calls, two runs, k = 1 and a vanishing sigma with the input bits, a non-finite point with the cloud
without it; velocities and displacements (one float32 rounding per operation) with the float32 restatement.  Values -- the smoothed
points, the edge lengths, the cost of the end-to-end case -- follow the rule of tests/test_train_kernels_gpu.py (its check() and TABLE are
used): within 8 x the float32 restatement's own error against float64, floor 1e-6, relative to the largest reference magnitude.  The
float64 values are taken on the float32 selection, so rounding is all that separates the three; for the jittered grid the float32 and
float64 selections themselves agree for every point and frame (asserted), so that comparison cannot hide a selection difference.

Shapes.  One lane per point, 256 lanes a workgroup, the frame through a 1024-point LDS slab four candidates at a time: N = 1; 5 with
k = 20 (fewer points than k); 256 and 257 (the workgroup edge); 1024 and 1029 (the slab edge, and a tail the four-wide loop leaves).
k in {1, 4, 5, 20, 32} at every N: the capacities 4, 8 and 32 of KBest, full (4, 32) and with dead slots (1, 5, 20); k in {8, 9, 16, 17} at
N = 257: the capacity 16 and both of its borders; k in {9, 16} at N = 1025: that capacity over two slabs.  T in {1, 3}, and 65538 frames of 3 points: more than the grid's second axis holds."""
import numpy as np
import pytest

import util  # noqa: F401
import trajectory_ref as R
from test_train_kernels_gpu import FLOOR, K, TABLE, check  # noqa: F401  (the project's rule for a bar, and the table of its comparisons)

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
import simple_knn  # noqa: E402
from meshnet.data_utils import (compute_edge_features, gaussian_smoothing, get_data_traj, process_traj, smooth_clouds,  # noqa: E402,F401
                                trajectory_features)  # (absent: every test of this file fails)
from meshnet.dataloader_sim import get_goal_fold  # noqa: E402

NAN, INF = float("nan"), float("inf")


@pytest.fixture(scope="module", autouse=True)
def _table():
    yield
    print("\ngroup | comparisons | largest e32 | largest bar | largest kernel error | smallest bar / error")
    for g in sorted(g for g in TABLE if g.startswith("trajectory")):
        n, e32, bar, err, margin = TABLE[g]
        print(f"{g} | {n} | {e32:.2e} | {bar:.2e} | {err:.2e} | {margin:.1f}")


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def cloud(T, N, seed):
    """frame 0 uniform in a cube; every later frame is the one before plus 1e-4: a look into another frame changes the result"""
    rng = np.random.default_rng(seed)
    P0 = rng.uniform(-1, 1, (N, 3)).astype(np.float32)
    return np.stack([P0 + np.float32(1e-4 * t) for t in range(T)]).astype(np.float32)


REFS = {}


def reference(T, N, k, sigma, seed):
    """the restatement of one case, computed once and shared (never written)"""
    key = (T, N, k, sigma, seed)
    if key not in REFS:
        P = cloud(T, N, seed)
        r32, d2, idx = R.smooth(P, k, sigma, np.float32)
        r64 = R.smooth(P, k, sigma, np.float64)[0]
        REFS[key] = (P, r32, r64, d2, idx)
    return REFS[key]


def smooth_case(T, N, k, sigma=0.3, seed=0, points_gpu=None):
    P, r32, r64, d2, idx = reference(T, N, k, sigma, seed)
    Pg = cu(P) if points_gpu is None else points_gpu
    out, gd2, gidx = smooth_clouds(Pg, k=k, sigma=sigma, return_neighbours=True)
    assert out.dtype == torch.float32 and gd2.dtype == torch.float32 and gidx.dtype == torch.int64
    assert out.shape == (T, N, 3) and gd2.shape == (T, N, k) and gidx.shape == (T, N, k)
    # the neighbour lists: the restatement's, and the two-cloud search's of every frame with itself, bit for bit
    assert np.array_equal(gidx.cpu().numpy(), idx) and np.array_equal(gd2.cpu().numpy(), d2), (T, N, k)
    for t in range(T):
        qd2, qidx = simple_knn.knn_query(Pg[t].contiguous(), Pg[t].contiguous(), k)
        assert torch.equal(qd2, gd2[t]) and torch.equal(qidx, gidx[t]), (T, N, k, t)
    # without the lists: the same bits; a second run: the same bits; frame by frame: the same bits
    plain = smooth_clouds(Pg, k=k, sigma=sigma)
    assert torch.equal(plain, out) and torch.equal(smooth_clouds(Pg, k=k, sigma=sigma), plain)
    for t in range(T):
        assert torch.equal(smooth_clouds(Pg[t], k=k, sigma=sigma), out[t]), (T, N, k, t)
    check("trajectory smooth", f"T{T} N{N} k{k} sigma{sigma}", out, r64, r32, 1.0)
    return out


@pytest.mark.parametrize("N", [1, 256, 257, 1024, 1029])
@pytest.mark.parametrize("k", [1, 4, 5, 20, 32])
def test_smoothing_at_the_launch_edges_and_every_capacity(N, k):
    smooth_case(3 if N in (257, 1029) else 1, N, k, seed=N)


@pytest.mark.parametrize("k", [8, 9, 16, 17])
def test_smoothing_at_the_borders_of_the_sixteen_slot_list(k):
    smooth_case(3, 257, k, seed=257)


@pytest.mark.parametrize("k", [9, 16])
def test_the_sixteen_slot_list_over_two_slabs(k):
    smooth_case(1, 1025, k, seed=1025)


@pytest.mark.parametrize("T", [1, 3])
def test_fewer_points_than_k(T):
    out = smooth_case(T, 5, 20, seed=5)
    _o, d2, idx = smooth_clouds(cu(cloud(T, 5, 5)), k=20, sigma=0.3, return_neighbours=True)
    assert (idx[:, :, 5:] == -1).all() and torch.isinf(d2[:, :, 5:]).all() and (idx[:, :, :5] >= 0).all() and torch.isfinite(out).all()


def test_exact_answers():
    P = cu(cloud(3, 300, 1))
    assert torch.equal(smooth_clouds(P, k=1), P)                                             # k = 1: the input bits
    neg = P[0].clone()
    neg[3] = -0.0
    assert torch.equal(smooth_clouds(neg, k=1).view(torch.int32), neg.view(torch.int32))     # (a -0 included)
    # spacing 0.01 and sigma = 1e-4: every other weight underflows to 0 -- the input bits
    grid = torch.stack(torch.meshgrid(torch.arange(9.0), torch.arange(7.0), torch.arange(5.0), indexing="ij"), -1).reshape(-1, 3).cuda() * 0.01
    assert torch.equal(smooth_clouds(grid, k=8, sigma=1e-4), grid) and torch.equal(smooth_clouds(grid, k=32, sigma=1e-4), grid)
    # 40 coincident points, k = 8: ties by index -- every list is 0 .. 7, a point's own index may fall outside its list
    same = torch.full((40, 3), 0.25, device="cuda")
    out, d2, idx = smooth_clouds(same, k=8, return_neighbours=True)
    assert torch.equal(out, same) and not d2.any() and (idx == torch.arange(8, device="cuda")[None]).all()
    # sigma = 1e4: c = 5e-9 rounds every weight of this cube (d2 <= 12) to within 6e-8 of 1 -- the plain mean of the k neighbours
    out, d2, idx = smooth_clouds(P, k=20, sigma=1e4, return_neighbours=True)
    Pd = P.double()
    mean64 = torch.stack([Pd[t][idx[t]].mean(1) for t in range(3)])
    mean32 = torch.stack([P[t][idx[t]].cpu().mean(1) for t in range(3)])
    check("trajectory smooth", "sigma 1e4: the plain mean", out, mean64, mean32, 1.0)


def test_more_frames_than_the_grid_axis_holds():
    """the frame is the grid's second axis, 65535 at most: a workgroup loops over the frames beyond it.  65538 frames of 3 points: the
    frames a workgroup reaches in its second round equal the same frames given on their own, and so do the first"""
    T = 65535 + 3
    P = torch.rand(T, 3, 3, device="cuda", generator=torch.Generator(device="cuda").manual_seed(3))
    out, d2, idx = smooth_clouds(P, k=2, sigma=0.5, return_neighbours=True)
    for part in (slice(65535, T), slice(0, 3), slice(65530, 65536)):
        o, d, i = smooth_clouds(P[part].contiguous(), k=2, sigma=0.5, return_neighbours=True)
        assert torch.equal(out[part], o) and torch.equal(d2[part], d) and torch.equal(idx[part], i), part
    assert (idx[:, :, 0] == torch.arange(3, device="cuda")[None]).all() and bool((out != P).any(2).all())
    vel, disp, norm = trajectory_features(P, torch.tensor([[0, 1], [1, 2]], device="cuda"), 0.5)
    assert torch.equal(vel[1:], (P[1:] - P[:-1]) * 2.0) and not vel[0].any() and torch.equal(disp, P[:, [1, 2]] - P[:, [0, 1]])


def test_a_non_finite_point_comes_back_unchanged_and_moves_no_other():
    P = cloud(1, 600, 2)[0]
    Q = P.copy()
    Q[7, 1], Q[300, 0], Q[599] = NAN, INF, (-INF, NAN, 1.0)
    keep = np.array([i for i in range(600) if i not in (7, 300, 599)])
    for k in (5, 20):
        out, d2, idx = smooth_clouds(cu(Q), k=k, sigma=0.5, return_neighbours=True)
        assert torch.equal(out[cu(keep)], smooth_clouds(cu(Q[keep]), k=k, sigma=0.5))
        assert np.array_equal(out[[7, 300, 599]].cpu().numpy().view(np.int32), Q[[7, 300, 599]].view(np.int32))
        assert (idx[[7, 300, 599]] == -1).all() and torch.isinf(d2[[7, 300, 599]]).all()
        assert not ((idx == 7) | (idx == 300) | (idx == 599)).any() and torch.isfinite(d2[cu(keep)]).all()
        r32, rd2, ridx = R.smooth(Q[None], k, 0.5, np.float32)
        assert np.array_equal(idx.cpu().numpy(), ridx[0])


def test_a_points_tensor_four_bytes_off_the_sixteen_byte_boundary():
    P, r32, r64, d2, idx = reference(3, 257, 20, 0.3, 257)
    flat = torch.empty(3 * 257 * 3 + 4, dtype=torch.float32, device="cuda")
    view = flat[1:1 + 3 * 257 * 3].view(3, 257, 3)
    view.copy_(cu(P))
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    smooth_case(3, 257, 20, seed=257, points_gpu=view)


def test_the_jittered_grid_and_the_reference_spelling():
    """the fixture's cloud in float32: the float32 and float64 selections agree for every point and frame, so the value comparison stands
    for the whole computation; gaussian_smoothing is the reference's name, k = 20 and sigma = 0.1 its defaults"""
    P = R.jittered_grid().astype(np.float32)
    for X in P:
        assert np.array_equal(R.select(X, 20, np.float32)[1], R.select(X, 20, np.float64)[1])
    r32, r64 = R.smooth(P, 20, 0.1, np.float32)[0], R.smooth(P, 20, 0.1, np.float64)[0]
    out = gaussian_smoothing(cu(P))
    check("trajectory smooth", "jittered grid, k 20, sigma 0.1", out, r64, r32, 1.0)
    assert torch.equal(gaussian_smoothing(cu(P[1]), k=20, sigma=0.1), out[1])
    as_np = gaussian_smoothing(P.astype(np.float64))                                         # numpy: float32 on the GPU, back in its dtype
    assert isinstance(as_np, np.ndarray) and as_np.dtype == np.float64 and np.array_equal(as_np.astype(np.float32), out.cpu().numpy())


# ------------------------------------------------------------------------------------------------------------------ features
@pytest.mark.parametrize("T,N,E", [(1, 1, 1), (2, 300, 0), (2, 300, 1), (5, 300, 257)])
def test_trajectory_features(T, N, E):
    rng = np.random.default_rng(E + T)
    P = cloud(T, N, 11) * np.float32(1.0 + 0.1 * np.arange(T))[:, None, None]
    ei = rng.integers(0, N, (2, E))
    if E:
        ei[:, 0] = N - 1                                                                     # an edge (i, i)
    vel, disp, norm = trajectory_features(cu(P), cu(ei), 0.05)
    v32, d32, n32 = R.features(P, ei, 1.0 / 0.05, np.float32)
    n64 = R.features(P, ei, 1.0 / 0.05, np.float64)[2]
    assert vel.shape == (T, N, 3) and disp.shape == (T, E, 3) and norm.shape == (T, E, 1) and vel.dtype == disp.dtype == norm.dtype == torch.float32
    assert np.array_equal(vel.cpu().numpy(), v32) and np.array_equal(disp.cpu().numpy(), d32) and not vel[0].any()
    if E:
        check("trajectory features", f"norm T{T} N{N} E{E}", norm, n64, n32, 1.0)
        assert not disp[:, 0].any() and not norm[:, 0].any()
    d1, n1 = compute_edge_features(cu(P), cu(ei))
    assert torch.equal(d1, disp) and torch.equal(n1, norm)
    d0, n0 = compute_edge_features(cu(P[T - 1]), cu(ei))
    assert d0.shape == (E, 3) and n0.shape == (E, 1) and torch.equal(d0, disp[T - 1]) and torch.equal(n0, norm[T - 1])
    again = trajectory_features(cu(P), cu(ei), 0.05)
    assert all(torch.equal(a, b) for a, b in zip(again, (vel, disp, norm)))


def test_process_traj_on_the_gpu():
    P, ei = R.jittered_grid().astype(np.float32), R.grid_edges()
    d = process_traj(cu(P), 0.05, edge_index=cu(ei))
    r = R.process_traj(P, ei, 0.05, np.float32)
    for key in ("pos", "velocity", "node_type", "edge_displacement", "edge_index"):
        assert d[key].is_cuda and np.array_equal(d[key].cpu().numpy(), r[key]), key
    check("trajectory features", "process_traj edge_norm", d["edge_norm"], R.process_traj(P, ei, 0.05, np.float64)["edge_norm"], r["edge_norm"], 1.0)
    assert torch.equal(d["edge_displacement"][0], d["edge_displacement"][1]) and d["edge_faces"] is None
    # the graph builders: a missing edge_index is compute_edges_index, subsampling is farthest_point_sampling
    np.random.seed(0)
    s = process_traj(cu(P), 0.05, k=3, subsample=True, num_samples=50)
    sel = s["sampled_point_indeces"]
    assert sel.shape == (50,) and len(set(sel.tolist())) == 50 and torch.equal(s["pos"], cu(P)[:, sel])
    E = s["edge_index"].shape[2]
    assert s["edge_index"].shape == (3, 2, E) and 50 <= E <= 150 and int(s["edge_index"].max()) < 50
    norm1 = R.features(P, ei, 1.0, np.float32)[2][1, :, 0]
    order = np.sort(norm1.astype(np.float64))
    thr = float(order[110] + order[111]) / 2                                                 # between two lengths, far from either in ulps
    assert order[111] - order[110] > 1e-6
    pruned = process_traj(cu(P), 0.05, edge_index=cu(ei), sim_data=True, norm_threshold=thr)
    assert pruned["edge_index"].shape == (3, 2, 111) and np.array_equal(pruned["edge_index"][0].cpu().numpy(), ei[:, norm1 < thr])


# ------------------------------------------------------------------------------------------------------------------ end to end
def test_depth_to_cloud_to_trajectory_to_planner_cost():
    """depth -> cloud -> voxel centroids -> a rigidly shifted trajectory -> smoothed -> graph state -> fold goal -> candidate cost, without
    a host round trip of the data; against the same chain through the restatements, from the same centroids"""
    from csplat import observation as ob
    from meshnet import mpc
    import observation_ref as OR
    V, H, W = 2, 24, 32
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    depth = np.stack([2.0 + 0.1 * np.sin(0.3 * xx + v) * np.cos(0.2 * yy) for v in range(V)]).astype(np.float32)
    depth[:, :2, :3] = 0.0                                                                   # holes
    intr = np.array([30.0, 30.0, (W - 1) / 2, (H - 1) / 2], np.float32)
    c2w = np.array([[1.0, 0.0, 0.0, 0.0], [0.0, 1.0, 0.0, 0.0], [0.0, 0.0, 1.0, 0.0]], np.float32)
    cl = ob.unproject_depth(cu(depth), intrinsics=cu(intr), cam_to_world=cu(c2w))
    cen = ob.voxel_downsample(cl.points, 0.12).centroids
    N = int(cen.shape[0])
    assert 100 < N < 1500
    shifts = torch.tensor([[0.0, 0.0, 0.0], [0.01, -0.005, 0.002], [0.02, -0.01, 0.004]], device="cuda")
    traj = (cen[None] + shifts[:, None]).contiguous()
    sm = smooth_clouds(traj, k=20, sigma=0.1)
    ei = R.grid_edges(4, N // 4, 3 * N)                                                      # some valid edge list over the first nodes
    d = process_traj(sm, 0.05, edge_index=cu(ei))
    pick, place = sm[0, 0].clone(), sm[0, N - 1].clone()
    goal = get_goal_fold(d["pos"][0], pick, place)
    weights = ob.observable_nodes(cl.points[::7].contiguous(), d["pos"][2], k=2).float()
    cost = mpc.candidate_costs(d["pos"], goal, weights)
    # the same chain through the restatements
    P = traj.cpu().numpy()
    s32, s64 = R.smooth(P, 20, 0.1, np.float32)[0], R.smooth(P, 20, 0.1, np.float64)[0]
    check("trajectory end to end", "smoothed", sm, s64, s32, 1.0)
    w = weights.cpu().numpy()
    assert np.array_equal(w > 0, OR.observable(cl.points[::7].cpu().numpy(), d["pos"][2].cpu().numpy(), 2)) and 0 < w.sum() < N

    def chain(s, dtype):
        g = R.goal_fold_loop(s[0], s[0, 0], s[0, N - 1])
        return ((w[None, :, None].astype(dtype) * (s - g[None]) ** 2).sum((1, 2)) / (3 * N)).astype(dtype), g
    c32, g32 = chain(s32, np.float32)
    c64, g64 = chain(s64, np.float64)
    check("trajectory end to end", "fold goal", goal, g64, g32, 1.0)
    check("trajectory end to end", "candidate cost", cost, c64, c32, float(c64.max()))
    r = R.process_traj(sm.cpu().numpy(), ei, 0.05, np.float32)
    assert np.array_equal(d["velocity"].cpu().numpy(), r["velocity"]) and np.array_equal(d["edge_displacement"].cpu().numpy(), r["edge_displacement"])


def test_get_data_traj_on_the_gpu():
    P = R.jittered_grid(T=4).astype(np.float32)
    grip = np.stack([[0.1 + 0.02 * t, 0.2 - 0.01 * t, 0.05 + 0.005 * t] for t in range(4)]).astype(np.float32)
    obs = dict(pos=cu(P), gripper_pos=cu(grip), pick=cu(grip[0]), place=cu(np.array([0.5, 0.4, 0.0], np.float32)))
    d = get_data_traj(None, None, (0.05, 3, False, False, 300, 2, 1), observations=obs)
    cloud_ = np.concatenate([P, (grip + np.array([0.0, -0.03, 0.02], np.float32))[:, None]], 1)
    s32, s64 = R.smooth(cloud_, 20, 0.1, np.float32)[0], R.smooth(cloud_, 20, 0.1, np.float64)[0]
    s32[:, :, 2] = s64[:, :, 2] = 0
    assert d["pos"].shape == (5, 133, 3) and d["pos"].is_cuda and torch.equal(d["pos"][0], d["pos"][1]) and not d["pos"][:, :, 2].any()
    check("trajectory end to end", "get_data_traj pos", d["pos"][1:], s64, s32, 1.0)
    g = d["grasped_particle"]
    near = np.argmin(((d["pos"][1].cpu().numpy().astype(np.float64) - grip[0]) ** 2).sum(1))
    assert isinstance(g, int) and g == int(near) and (d["node_type"][:, g] == 1).all() and float(d["node_type"].sum()) == 5
    assert d["edge_index"].shape[0] == 5 and not d["actions"][:2].any() and torch.equal(d["actions"][2:], cu(grip[1:] - grip[:-1]))
