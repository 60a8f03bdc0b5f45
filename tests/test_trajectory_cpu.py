"""Trajectory preprocessing without a GPU: the composed float64 path of meshnet.data_utils / meshnet.dataloader_sim against what the
reference's own functions return (tests/golden/trajectory_reference.npz, tools/make_trajectory_golden.py), against the restatement
tests/trajectory_ref.py and against known answers; the reference behaviours that are kept and the deliberate deviations, each pinned;
every ValueError; and the library's surface (header, exports, bindings, ABI number, argument checks before any launch).

The fixture's bar is 1e-12 of the largest magnitude: both sides are float64 evaluations of one formula and differ only in rounding order
(the reference takes a square root and squares it again, normalises the weights before it sums, divides by dt where this multiplies by
1 / dt) -- over k <= 32 terms that is ~4e-15; a wrong neighbour or weight shows at the 1e-4 level on this input."""
import math
import os
import re

import numpy as np
import pytest
import torch

import util
import trajectory_ref as R
from meshnet import data_utils as du  # noqa: E402
from meshnet.data_utils import (compute_edge_features, expand_init_data, flip_trajectory, gaussian_smoothing, get_data_traj,  # noqa: F401
                                process_traj, smooth_clouds, trajectory_features)  # (absent: every test of this file fails)
from meshnet.dataloader_sim import get_goal_fold

F64, F32 = torch.float64, torch.float32
NAN, INF = float("nan"), float("inf")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAR = 1e-12
T = torch.from_numpy


@pytest.fixture(scope="module")
def gold():
    return dict(util.golden("trajectory_reference.npz"))


def same_or_one_ulp(got, want):
    """a length: torch's vectorised CPU sqrt is within one ulp of the correctly rounded root that numpy (and the device's sqrtf) returns"""
    got, want = got.numpy() if torch.is_tensor(got) else got, np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape
    return bool((np.abs(got.astype(np.float64) - want.astype(np.float64)) <= np.spacing(np.abs(want)).astype(np.float64)).all())


def close(got, want, bar=BAR):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    err = float(np.abs(got - want).max()) / max(float(np.abs(want).max()), 1e-30)
    assert err <= bar, err
    return err


# ------------------------------------------------------------------------------------------------------------------ the fixture
def test_the_fixture_is_small_is_its_stated_input_and_has_no_tie(gold):
    assert os.path.getsize(os.path.join(util.GOLDEN, "trajectory_reference.npz")) < 64 * 1024
    traj = gold["t3_pos"]
    assert traj.shape == (3, 132, 3) and traj.dtype == np.float64 and np.array_equal(traj, R.jittered_grid())
    assert np.array_equal(gold["edge_index"], R.grid_edges()) and gold["edge_index"].shape == (2, 221)
    k = int(gold["k"])
    assert (k, float(gold["sigma"])) == (20, 0.1)
    for X in traj:
        d = np.sort(np.sqrt(R.sq_dists(X, np.float64)), axis=1)
        assert (d[:, k] - d[:, k - 1]).min() > 1e-9
    # and the float32 and float64 selections agree for every point and frame: a float32 run averages the same points
    for X in traj.astype(np.float32):
        assert np.array_equal(R.select(X, k, np.float32)[1], R.select(X, k, np.float64)[1])


def test_smoothing_reproduces_the_reference(gold):
    traj, k, sigma = gold["t3_pos"], int(gold["k"]), float(gold["sigma"])
    got = smooth_clouds(T(traj), k=k, sigma=sigma)
    assert got.dtype == F64 and got.shape == (3, 132, 3)
    close(got, gold["smoothed"])
    assert float(np.abs(gold["smoothed"] - traj).max()) > 1e-3              # (it does move the points)
    for t in range(3):                                                       # the reference's name and signature: one cloud
        assert torch.equal(gaussian_smoothing(T(traj[t]), k=k, sigma=sigma), got[t])
    assert torch.equal(gaussian_smoothing(T(traj)), got)                     # its defaults are k = 20, sigma = 0.1
    # numpy in, numpy out, the input's dtype (no GPU here: the composed CPU path in that dtype)
    as_np = smooth_clouds(traj, k=k, sigma=sigma)
    assert isinstance(as_np, np.ndarray) and as_np.dtype == np.float64
    if not torch.cuda.is_available():
        assert np.array_equal(as_np, got.numpy())
    # the restatement gives the same: float64 values on the float64 selection
    close(R.smooth(traj, k, sigma, np.float64, selection=np.float64, sigma32=False)[0], gold["smoothed"])


def test_process_traj_reproduces_the_reference(gold):
    traj, ei, dt = gold["t3_pos"], gold["edge_index"], float(gold["dt"])
    for tag, sub in (("t3", traj), ("t1", traj[:1])):
        n = len(sub)
        d = process_traj(T(sub), dt, edge_index=T(ei), sim_data=False)
        assert list(d.keys()) == ["pos", "velocity", "node_type", "edge_index", "edge_displacement", "edge_norm", "edge_faces", "sampled_point_indeces"]
        shapes = {"pos": (n, 132, 3), "velocity": (n, 132, 3), "node_type": (n, 132, 1), "edge_index": (n, 2, 221), "edge_displacement": (n, 221, 3),
                  "edge_norm": (n, 221, 1), "sampled_point_indeces": (132,)}
        for key, shape in shapes.items():
            assert torch.is_tensor(d[key]) and tuple(d[key].shape) == shape, (tag, key)
            want = sub if key == "pos" else gold[f"{tag}_{key}"]
            assert tuple(want.shape) == shape, (tag, key)
            if d[key].dtype.is_floating_point:
                assert d[key].dtype == F64
                if np.abs(want).max() > 0:
                    close(d[key], want)
                else:
                    assert not d[key].any()
            else:
                assert d[key].dtype == torch.int64 and np.array_equal(d[key].numpy(), want)
        assert d["edge_faces"] is None
        assert d["edge_index"][0].data_ptr() == d["edge_index"][-1].data_ptr() and (n == 1 or d["edge_index"].stride(0) == 0)   # a view of one [2,E]
    assert torch.equal(d["velocity"], torch.zeros(1, 132, 3, dtype=F64))     # T = 1: one frame, zero velocity


def test_goal_fold_reproduces_the_reference_and_its_loop(gold):
    X, pick, place = gold["t3_pos"][0], gold["pick"], gold["place"]
    got = get_goal_fold(T(X), T(pick), T(place))
    assert got.dtype == F64
    close(got, gold["goal"])
    close(got, R.goal_fold_loop(X, pick, place))
    moved = (got.numpy() != X).any(1)
    assert 20 < moved.sum() < 112
    # a node exactly on the fold line stays; one a hair to the negative side goes across; float32 works too
    pick, place = torch.tensor([0.0, 0.0, 0.0]), torch.tensor([2.0, 0.0, 0.0])
    nodes = torch.tensor([[1.0, 5.0, -3.0], [0.5, 1.0, 2.0], [1.5, 1.0, 2.0], [1.0 - 2.0 ** -20, 0.0, 0.0]])
    out = get_goal_fold(nodes, pick, place)
    assert out.dtype == F32 and out.tolist() == [[1.0, 5.0, -3.0], [1.5, 1.0, 2.0], [1.5, 1.0, 2.0], [1.0 + 2.0 ** -20, 0.0, 0.0]]
    assert nodes.tolist()[1] == [0.5, 1.0, 2.0]                              # the input is not written
    assert np.array_equal(out.numpy(), R.goal_fold_loop(nodes.numpy(), pick.numpy(), place.numpy()))
    g = get_goal_fold(nodes.clone().requires_grad_(True), pick, place)
    assert not g.requires_grad


# ------------------------------------------------------------------------------------------------------------------ smoothing
def cloud(N, seed=0, T_=1):
    rng = np.random.default_rng(seed)
    return rng.uniform(-1, 1, (T_, N, 3)).astype(np.float32)


@pytest.mark.parametrize("N,k", [(1, 1), (5, 20), (40, 8), (300, 5), (1100, 32)])
def test_smoothing_on_cpu_tensors_equals_the_restatement(N, k):
    P = cloud(N, seed=N, T_=2)
    for dt, npdt, bar in ((F32, np.float32, 2e-6), (F64, np.float64, 1e-13)):
        out, d2, idx = smooth_clouds(T(P).to(dt), k=k, sigma=0.3, return_neighbours=True)
        r_out, r_d2, r_idx = R.smooth(P, k, 0.3, npdt, selection=npdt, sigma32=dt == F32)
        assert out.dtype == dt and d2.dtype == dt and idx.dtype == torch.int64 and out.shape == (2, N, 3) and idx.shape == (2, N, k)
        assert np.array_equal(idx.numpy(), r_idx) and np.array_equal(d2.numpy(), r_d2)
        assert (idx[:, :, 0] == torch.arange(N)[None]).all() and not d2[:, :, 0].any()       # the point itself comes first, at distance 0
        if k > N:
            assert (idx[:, :, N:] == -1).all() and torch.isinf(d2[:, :, N:]).all()
        close(out, r_out, bar)
    one = smooth_clouds(T(P[0]), k=k, sigma=0.3)
    assert one.shape == (N, 3) and torch.equal(one, smooth_clouds(T(P), k=k, sigma=0.3)[0])


def test_smoothing_known_answers():
    P = T(cloud(50, T_=2))
    assert torch.equal(smooth_clouds(P, k=1), P)                                             # k = 1: the input bits
    grid = torch.stack(torch.meshgrid(torch.arange(6.0), torch.arange(5.0), torch.arange(2.0), indexing="ij"), -1).reshape(-1, 3) * 0.01
    assert torch.equal(smooth_clouds(grid, k=8, sigma=1e-4), grid)                           # the other weights underflow to 0
    # sigma = 1e4: c = 5e-9 and d2 <= 12 in this cube, so every weight is within 6e-8 of 1: the plain mean of the k neighbours
    out, d2, idx = smooth_clouds(P.double(), k=6, sigma=1e4, return_neighbours=True)
    close(out, torch.stack([P[t].double()[idx[t]].mean(1) for t in range(2)]), 1e-7)
    # ties by index: 40 coincident points, k = 8 -- every list is 0 .. 7, the point's own index may fall outside it
    same = torch.full((40, 3), 0.25)
    out, d2, idx = smooth_clouds(same, k=8, return_neighbours=True)
    assert torch.equal(out, same) and not d2.any() and (idx == torch.arange(8)[None]).all()
    # a point with a NaN or Inf coordinate comes back unchanged and moves no other point
    Q = P[0].clone()
    Q[7, 1], Q[20, 0] = NAN, INF
    out, d2, idx = smooth_clouds(Q, k=5, sigma=0.5, return_neighbours=True)
    keep = [i for i in range(50) if i not in (7, 20)]
    assert torch.equal(out[keep], smooth_clouds(Q[keep], k=5, sigma=0.5))
    assert torch.equal(out[[7, 20]].isnan(), Q[[7, 20]].isnan()) and out[20, 0] == INF and torch.equal(out[7, [0, 2]], Q[7, [0, 2]])
    assert (idx[[7, 20]] == -1).all() and torch.isinf(d2[[7, 20]]).all() and not ((idx == 7) | (idx == 20)).any()
    # another frame is never read: frame 1 = frame 0 + 1e-4
    two = torch.stack([P[0], P[0] + 1e-4])
    assert torch.equal(smooth_clouds(two, k=4)[0], smooth_clouds(P[0], k=4)) and torch.equal(smooth_clouds(two, k=4)[1], smooth_clouds(two[1], k=4))
    # empty inputs
    assert smooth_clouds(torch.zeros(0, 3)).shape == (0, 3) and smooth_clouds(torch.zeros(2, 0, 3)).shape == (2, 0, 3)
    assert smooth_clouds(torch.zeros(0, 4, 3), return_neighbours=True)[2].shape == (0, 4, 20)
    assert not smooth_clouds(P.clone().requires_grad_(True)).requires_grad
    assert du.weight_scale(1e-30, F32) == du.FLT_MAX and du.weight_scale(0.1, F64) == 1.0 / (2.0 * 0.1 * 0.1)


# ------------------------------------------------------------------------------------------------------------------ features
@pytest.mark.parametrize("T_,N,E", [(1, 1, 1), (2, 7, 0), (5, 30, 257)])
def test_features_on_cpu_tensors_equal_the_restatement(T_, N, E):
    rng = np.random.default_rng(E)
    P = cloud(N, seed=3, T_=T_)
    ei = rng.integers(0, N, (2, E))
    if E:
        ei[:, 0] = N - 1                                                                     # an edge (i, i)
    for dt, npdt in ((F32, np.float32), (F64, np.float64)):
        vel, disp, norm = trajectory_features(T(P).to(dt), T(ei), 0.05)
        r = R.features(P, ei, 1.0 / 0.05, npdt)
        for got, want, shape in zip((vel, disp, norm), r, ((T_, N, 3), (T_, E, 3), (T_, E, 1))):
            assert got.dtype == dt and tuple(got.shape) == shape
            assert same_or_one_ulp(got, want) if got is norm else np.array_equal(got.numpy(), want)
        assert not vel[0].any()
        d1, n1 = compute_edge_features(T(P).to(dt), ei)                                      # (a numpy edge list is accepted)
        assert torch.equal(d1, disp) and torch.equal(n1, norm)
        d0, n0 = compute_edge_features(T(P[0]).to(dt), T(ei))                                # the reference's signature: ([E,3], [E,1])
        assert d0.shape == (E, 3) and n0.shape == (E, 1) and torch.equal(d0, disp[0]) and torch.equal(n0, norm[0])
        if E:
            assert not disp[:, 0].any() and not norm[:, 0].any()


def test_the_displacement_has_the_sign_of_the_reference():
    """receiver minus sender, points[edge_index[1]] - points[edge_index[0]]: the opposite of meshnet.rollout.edge_features"""
    P = torch.tensor([[0.0, 0.0, 0.0], [3.0, 4.0, 0.0]])
    disp, norm = compute_edge_features(P, torch.tensor([[0], [1]]))
    assert disp.tolist() == [[3.0, 4.0, 0.0]] and norm.tolist() == [[5.0]]
    from meshnet import rollout
    assert "OPPOSITE" in compute_edge_features.__doc__ and "opposite" in trajectory_features.__doc__
    assert "data_utils.compute_edge_features" in rollout.edge_features.__doc__ and "opposite" in rollout.edge_features.__doc__.lower()


# ------------------------------------------------------------------------------------------------------------------ process_traj
def test_process_traj_keeps_the_reference_behaviours():
    traj, ei = R.jittered_grid().astype(np.float32), R.grid_edges()
    d = process_traj(T(traj), 0.05, edge_index=T(ei))
    r = R.process_traj(traj, ei, 0.05, np.float32)
    for key in ("pos", "velocity", "node_type", "edge_displacement", "edge_norm", "edge_index"):
        assert same_or_one_ulp(d[key], r[key]) if key == "edge_norm" else np.array_equal(d[key].numpy(), r[key]), key
        assert d[key].dtype == (torch.int64 if key == "edge_index" else F32)
    # frame 0's edge features are a copy of frame 1's, not its own
    own0 = compute_edge_features(T(traj[0]), T(ei))
    assert torch.equal(d["edge_displacement"][0], d["edge_displacement"][1]) and torch.equal(d["edge_norm"][0], d["edge_norm"][1])
    assert not torch.equal(d["edge_displacement"][0], own0[0])
    assert not d["velocity"][0].any() and torch.equal(d["velocity"][2], (T(traj[2]) - T(traj[1])) * 20.0)
    # T = 1: one frame, its own edge features, zero velocity
    one = process_traj(T(traj[:1]), 0.05, edge_index=T(ei))
    assert one["pos"].shape == (1, 132, 3) and not one["velocity"].any() and torch.equal(one["edge_displacement"][0], own0[0])
    # faces are carried along, expanded over the frames; explicit sample indices select the nodes
    faces = torch.tensor([[0, 1], [1, 2], [12, 13]])
    pick = np.array([5, 0, 17, 40])
    sub = process_traj(T(traj), 0.05, sampled_points_indeces=pick, edge_index=torch.tensor([[0, 1], [2, 3]]), faces=faces)
    assert sub["edge_faces"].shape == (3, 3, 2) and torch.equal(sub["edge_faces"][2], faces)
    assert torch.equal(sub["pos"], T(traj)[:, pick]) and sub["sampled_point_indeces"].tolist() == [5, 0, 17, 40]
    assert torch.equal(sub["edge_displacement"][2], T(traj)[2, [17, 40]] - T(traj)[2, [5, 0]])
    # numpy in: CPU tensors in the input's dtype
    as_np = process_traj(traj.astype(np.float64), 0.05, edge_index=ei)
    assert all(torch.is_tensor(as_np[key]) and as_np[key].device.type == "cpu" for key in r) and as_np["pos"].dtype == F64
    with pytest.raises(NotImplementedError):
        process_traj(T(traj), 0.05, delaunay=True)


def test_process_traj_prunes_once_where_the_reference_would_crash():
    """sim_data: the edges whose frame-1 norm is >= norm_threshold go, in stable order.  The reference indexes the already pruned [2,E']
    list with the [E] mask a second time and raises IndexError whenever E' < E; once is what it computes whenever it does not crash."""
    traj, ei = R.jittered_grid().astype(np.float64), R.grid_edges()
    norm1 = R.features(traj, ei, 1.0, np.float64)[2][1, :, 0]
    thr = float(np.median(norm1))
    keep = norm1 < thr
    assert 50 < keep.sum() < 171
    d = process_traj(T(traj), 0.05, edge_index=T(ei), sim_data=True, norm_threshold=thr)
    E = int(keep.sum())
    assert d["edge_index"].shape == (3, 2, E) and np.array_equal(d["edge_index"][0].numpy(), ei[:, keep])
    r = R.process_traj(traj, ei, 0.05, np.float64, sim_data=True, norm_threshold=thr)
    for key in ("edge_displacement", "edge_norm", "velocity"):
        assert same_or_one_ulp(d[key], r[key]) if key == "edge_norm" else np.array_equal(d[key].numpy(), r[key]), key
    assert (d["edge_norm"][1] < thr).all() and d["edge_norm"].shape == (3, E, 1)
    # nothing pruned: the reference's result, unchanged
    full = process_traj(T(traj), 0.05, edge_index=T(ei), sim_data=True, norm_threshold=10.0)
    plain = process_traj(T(traj), 0.05, edge_index=T(ei))
    assert all(torch.equal(full[key], plain[key]) for key in ("edge_index", "edge_displacement", "edge_norm"))
    # T = 1 prunes on its only frame; everything pruned leaves E = 0
    one = process_traj(T(traj[:1]), 0.05, edge_index=T(ei), sim_data=True, norm_threshold=float(np.median(R.features(traj[:1], ei, 1.0, np.float64)[2])))
    assert 0 < one["edge_index"].shape[2] < 221
    none = process_traj(T(traj), 0.05, edge_index=T(ei), sim_data=True, norm_threshold=0.0)
    assert none["edge_index"].shape == (3, 2, 0) and none["edge_displacement"].shape == (3, 0, 3) and none["edge_norm"].shape == (3, 0, 1)


# ------------------------------------------------------------------------------------------------------------------ get_data_traj
def observations(T_=4, dtype=np.float64):
    traj = R.jittered_grid(T=T_).astype(dtype)
    grip = np.stack([[0.1 + 0.02 * t, 0.2 - 0.01 * t, 0.05 + 0.005 * t] for t in range(T_)]).astype(dtype)
    return dict(pos=traj, gripper_pos=grip, pick=grip[0].copy(), place=np.array([0.5, 0.4, 0.0], dtype))


def test_get_data_traj_bookkeeping(monkeypatch):
    obs = observations()
    ei = R.grid_edges(12, 11, 100)
    # the graph builders need the GPU: the edge list is given through process_traj here
    real = du.process_traj
    monkeypatch.setattr(du, "process_traj", lambda *a, **kw: real(*a, **dict(kw, edge_index=T(ei))))
    obs_t = {key: T(v) for key, v in obs.items()}
    keep = {key: v.clone() for key, v in obs_t.items()}
    d = get_data_traj(None, None, (0.05, 3, False, False, 300, 1, 1), observations=obs_t)
    assert all(torch.equal(obs_t[key], keep[key]) for key in keep) and "actions" not in obs_t          # the observations are not written
    Tn, N = 4, 133
    # the gripper point is appended to every frame, all frames are smoothed, z is zero
    grip = T(obs["gripper_pos"])
    cloud = torch.cat([T(obs["pos"]), (grip + torch.tensor([0.0, -0.03, 0.02], dtype=F64))[:, None]], 1)
    want = smooth_clouds(cloud, k=20, sigma=0.1)
    want[:, :, 2] = 0
    assert d["pos"].shape == (Tn, N, 3) and d["pos"].dtype == F64 and torch.equal(d["pos"], want) and not d["pos"][:, :, 2].any()
    # actions: ones in frame 0 and differences from then on; the shift puts zeros in front of actions[1:]
    assert not d["actions"][0].any() and torch.equal(d["actions"][1:], grip[1:] - grip[:-1])
    assert torch.equal(d["gripper_pos"], grip) and not d["gripper_vel"][0].any() and torch.equal(d["gripper_vel"][1:], (grip[1:] - grip[:-1]) * (1.0 / 0.05))
    assert torch.equal(d["pick"], T(obs["pick"])) and torch.equal(d["place"], T(obs["place"]))
    # process_traj ran with sim_data=False: nothing pruned at norm_threshold 0.1, frame 0's features are frame 1's
    assert d["edge_index"].shape == (Tn, 2, 100) and torch.equal(d["edge_displacement"][0], d["edge_displacement"][1])
    assert torch.equal(d["velocity"][1], (want[1] - want[0]) * (1.0 / 0.05))
    # the grasped node: the nearest to `pick` in frame 0; node_type 1 there in every frame, 0 elsewhere
    g = d["grasped_particle"]
    assert isinstance(g, int) and g == int(np.argmin(np.linalg.norm(want[0].numpy() - obs["pick"], axis=1)))
    assert d["node_type"].shape == (Tn, N, 1) and (d["node_type"][:, g] == 1).all() and d["node_type"].sum() == Tn
    # input_length_sequence = 3: the first element twice more in front of the listed entries, the others as they were
    e = get_data_traj(None, None, (0.05, 3, False, False, 300, 3, 1), observations=obs_t)
    for key in ("actions", "pos", "velocity", "gripper_pos", "gripper_vel", "node_type", "edge_index", "edge_displacement", "edge_norm"):
        assert e[key].shape[0] == Tn + 2 and torch.equal(e[key][2:], d[key]) and torch.equal(e[key][0], d[key][0]) and torch.equal(e[key][1], d[key][0]), key
    assert torch.equal(e["pick"], d["pick"]) and e["grasped_particle"] == g
    # without rw_processing the cloud goes through as it is and the given actions are shifted
    act = torch.arange(12.0, dtype=F64).reshape(4, 3)
    raw = get_data_traj(None, None, (0.05, 3, False, False, 300, 1, 1), observations=dict(obs_t, actions=act), rw_processing=False)
    assert torch.equal(raw["pos"], obs_t["pos"]) and torch.equal(raw["actions"][1:], act[1:]) and not raw["actions"][0].any()
    # sim_data swaps the y and z columns first
    sim = get_data_traj(None, None, (0.05, 3, False, False, 300, 1, 1), observations=dict(obs_t, actions=act), sim_data=True)
    assert torch.equal(sim["pos"], obs_t["pos"][:, :, [0, 2, 1]]) and torch.equal(sim["pick"], obs_t["pick"][[0, 2, 1]]) and \
        torch.equal(sim["actions"][1:], act[1:][:, [0, 2, 1]])
    # numpy observations: CPU tensors in the dtype of pos
    as_np = get_data_traj(None, None, (0.05, 3, False, False, 300, 1, 1), observations=obs)
    assert as_np["pos"].dtype == F64 and as_np["pos"].device.type == "cpu" and as_np["grasped_particle"] == g
    with pytest.raises(NotImplementedError):
        get_data_traj("some/file.h5", ["pos"], (0.05, 3, False, False, 300, 1, 1))


def test_the_grasped_node_of_a_tie_is_the_smaller_index(monkeypatch):
    real = du.process_traj
    monkeypatch.setattr(du, "process_traj", lambda *a, **kw: real(*a, **dict(kw, edge_index=torch.tensor([[0], [1]]))))
    pos = torch.tensor([[[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, -1.0, 0.0], [-1.0, 0.0, 0.0], [3.0, 3.0, 0.0]]]).repeat(2, 1, 1)
    obs = dict(pos=pos, gripper_pos=torch.zeros(2, 3), pick=torch.zeros(3), place=torch.ones(3), actions=torch.zeros(2, 3))
    d = get_data_traj(None, None, (0.1, 3, False, False, 300, 1, 1), observations=obs, rw_processing=False)
    assert d["grasped_particle"] == 0 and d["node_type"][:, :, 0].tolist() == [[1.0, 0.0, 0.0, 0.0, 0.0]] * 2
    obs["pick"] = torch.tensor([-0.5, -0.5, 0.0])                                           # nodes 2 and 3 are equally near
    assert get_data_traj(None, None, (0.1, 3, False, False, 300, 1, 1), observations=obs, rw_processing=False)["grasped_particle"] == 2


def test_expand_and_flip_are_the_reference_one_liners():
    a = np.arange(12.0).reshape(4, 3)
    assert np.array_equal(expand_init_data(a, 3), np.concatenate([a[:1], a[:1], a]))
    assert torch.equal(expand_init_data(T(a), 2), torch.cat([T(a)[:1], T(a)])) and expand_init_data(a, 1) is a
    traj = dict(pos=np.arange(24.0).reshape(2, 4, 3), vel=np.arange(24.0).reshape(2, 4, 3), gripper_pos=a.copy(), pick=np.array([1.0, 2.0, 3.0]),
                place=np.array([4.0, 5.0, 6.0]))
    out = flip_trajectory(traj, ["pos", "gripper_pos", "pick"])
    assert out is traj and out["pick"].tolist() == [1.0, 3.0, 2.0] and out["place"].tolist() == [4.0, 5.0, 6.0]
    assert np.array_equal(out["pos"], np.arange(24.0).reshape(2, 4, 3)[:, :, [0, 2, 1]]) and np.array_equal(out["gripper_pos"], a[:, [0, 2, 1]])
    assert np.array_equal(out["vel"], np.arange(24.0).reshape(2, 4, 3))                      # not in load_keys


# ------------------------------------------------------------------------------------------------------------------ every ValueError
def test_argument_errors():
    P, ei = torch.zeros(2, 5, 3), torch.tensor([[0, 1], [1, 4]])
    bad_smooth = [dict(points=[[0.0, 0.0, 0.0]]), dict(points=torch.zeros(5, 3, dtype=torch.int64)), dict(points=torch.zeros(5, 2)), dict(points=torch.zeros(3)),
                  dict(points=torch.zeros(1, 2, 5, 3)), dict(k=0), dict(k=33), dict(k=2.0), dict(k=True), dict(sigma=0.0), dict(sigma=-1.0), dict(sigma=NAN),
                  dict(sigma=INF), dict(sigma="wide"), dict(sigma=1e-60), dict(points=torch.zeros(1, 1, 3).expand(2 ** 16, 2 ** 11, 3), k=16)]
    for kw in bad_smooth:
        with pytest.raises(ValueError, match="smooth_clouds"):
            smooth_clouds(**dict(dict(points=P), **kw))
    with pytest.raises(ValueError):
        gaussian_smoothing(P, k=40)
    for fn, args in ((compute_edge_features, (P,)), (trajectory_features, (P,)), (process_traj, (P, 0.1))):
        tail = () if fn is compute_edge_features else (0.1,)
        for bad in (torch.tensor([[0, 1], [1, 5]]), torch.tensor([[0, -1], [1, 2]]), torch.zeros(3, 4, dtype=torch.int64), torch.zeros(2, dtype=torch.int64),
                    torch.zeros(2, 4), [[0], [1]]):
            with pytest.raises(ValueError, match=fn.__name__):
                fn(P, bad, *tail) if fn is not process_traj else fn(P, 0.1, edge_index=bad)
    for bad in (torch.zeros(5, 3), torch.zeros(2, 5, 2), np.zeros((2, 5, 3), np.int32)):
        with pytest.raises(ValueError, match="trajectory_features"):
            trajectory_features(bad, ei, 0.1)
    for bad in (0.0, NAN, INF, "fast", 1e-60):
        with pytest.raises(ValueError, match="trajectory_features"):
            trajectory_features(P, ei, bad)
        with pytest.raises(ValueError, match="process_traj"):
            process_traj(P, bad, edge_index=ei)
    with pytest.raises(ValueError, match="compute_edge_features"):
        compute_edge_features(torch.zeros(5, 4), ei)
    for kw in (dict(traj=torch.zeros(5, 3)), dict(traj=torch.zeros(0, 5, 3)), dict(traj=torch.zeros(2, 5, 3, dtype=torch.int32)), dict(norm_threshold=NAN),
               dict(norm_threshold="x"), dict(sampled_points_indeces=[0, 5]), dict(sampled_points_indeces=[-1]), dict(sampled_points_indeces=[0.5]),
               dict(sampled_points_indeces=[[0, 1]]), dict(edge_index=None, k=0), dict(edge_index=None, k=40), dict(edge_index=None, subsample=True, num_samples=0)):
        with pytest.raises(ValueError, match="process_traj"):
            process_traj(**dict(dict(traj=P, dt=0.1, edge_index=ei), **kw))
    X, a, b = torch.zeros(4, 3), torch.zeros(3), torch.ones(3)
    for args in ((X, a, a), (X, a, torch.tensor([NAN, 0.0, 0.0])), (X[:, :2], a, b), (X, a[:2], b), (X, a, torch.ones(1, 3)), (X.long(), a, b),
                 (X.numpy(), a, b), (X, a, [1.0, 1.0, 1.0])):
        with pytest.raises(ValueError, match="get_goal_fold"):
            get_goal_fold(*args)
    obs = {key: T(v) for key, v in observations().items()}
    params = (0.05, 3, False, False, 300, 1, 1)
    for o, p, kw in ((obs, (0.05, 3), {}), (obs, (0.0,) + params[1:], {}), ({k: v for k, v in obs.items() if k != "pick"}, params, {}), (obs, params, dict(rw_processing=False)),
                     (obs, params, dict(sim_data=True)), (dict(obs, pos=obs["pos"][0]), params, {}), (dict(obs, gripper_pos=obs["gripper_pos"][:2]), params, {}),
                     (dict(obs, place=torch.zeros(2)), params, {}), (dict(obs, pick=[0.0, 0.0, 0.0]), params, {}), (dict(obs, pos=obs["pos"][:, :0]), params, {})):
        with pytest.raises(ValueError, match="get_data_traj"):
            get_data_traj(None, None, p, observations=o, **kw)


# ------------------------------------------------------------------------------------------------------------------ the library's surface
ENTRIES = (("int", "csplat_traj_smooth", 9), ("int", "csplat_traj_features", 10))


def test_header_exports_and_bindings():
    from csplat import native
    header = open(os.path.join(ROOT, "include", "csplat.h")).read()
    for res, name, n_args in ENTRIES:
        assert re.search(r"\b" + res + " " + name + r"\s*\(", header), name
        assert name in native.EXPORTS and hasattr(native.lib, name) and len(native.EXPORTS[name][1]) == n_args
        decl = header[header.index(res + " " + name + "("):]
        decl = re.sub(r"/\*.*?\*/", "", decl[:decl.index(";")], flags=re.S)
        assert decl.count(",") + 1 == n_args, (name, decl)
    block = header[header.index("/* Trajectory preprocessing"):header.index("int csplat_traj_smooth(")]
    assert block.rstrip().endswith("Added exports: CSPLAT_ABI_VERSION is unchanged. */")
    flat = re.sub(r"\s*\n \*\s*", " ", block)                                               # the comment's lines joined
    for word in ("the point itself included", "as csplat_knn_query orders them", "ties to the smaller index", "No other frame is ever read", "nobody's neighbour",
                 "(+inf, -1)", "rounded once to float32 and limited to FLT_MAX", "expf(-(d2_j * c))", "ascending order", "K = 1 returns the input bits",
                 "written through unchanged", "bit-reproducible", "No atomics", "T * N * K < 2^31", "vel[0][i] = 0", "each rounded once", "OPPOSITE",
                 "sqrtf(dx*dx + dy*dy + dz*dz)", "ONE launch", "brute-force"):
        assert word.lower() in flat.lower(), word
    assert native.ABI_VERSION == 9 and native.lib.csplat_abi_version() == 9
    src = open(os.path.join(ROOT, "cloth-splatting_amd", "csrc", "csplat_trajectory.hip")).read()
    code = re.sub(r"//.*", "", src)
    assert "atomic" not in code.lower() and "#pragma clang fp contract(off)" in code and "__fmul_rn(__fsub_rn(" in code and "k_traj_features" in code
    csrc = os.path.join(ROOT, "cloth-splatting_amd", "csrc")
    device = re.sub(r"//.*", "", open(os.path.join(csrc, "csplat_device.h")).read())       # the helpers the smoothing kernel calls
    assert "atomic" not in device.lower()
    knn = "".join(open(os.path.join(csrc, f)).read() for f in sorted(os.listdir(csrc)) if f.startswith("csplat_knn"))   # the knn sources
    smooth = re.sub(r"//.*", "", knn[knn.index("void k_traj_smooth("):knn.index('extern "C" int csplat_traj_smooth(')])
    assert "KBest<CAP>" in smooth and "knn_scan_slabs(" in smooth and "atomic" not in smooth.lower()
    assert "s_p[" not in smooth and "offer" not in smooth                                      # the kernel holds no candidate loop of its own
    for once in ("struct KBest", "void offer(", "void offer4("):                              # used, not copied: one definition of each,
        assert knn.count(once) == 1, once                                                      # whatever its parameters are called
    for fn in ("knn_scan_slabs", "knn_d2", "knn_box_d2"):                                      # (a definition starts its line with __device__)
        assert len(re.findall(r"^__device__[^\n;]*\b" + fn + r"\(", knn, flags=re.M)) == 1, fn
    assert du.FLT_MAX == R.FLT_MAX and du.GRIPPER_OFFSET == (0.0, -0.03, 0.02)


def test_the_device_helpers_are_defined_once_and_used_not_copied():
    """csplat_device.h holds the wave and block reductions, the pixel projection and the finite test: one definition of each in csrc/
    (the rasterizer's files, which do not include it and keep their own reductions, aside), and no butterfly written out again in a file
    that includes it"""
    csrc = os.path.join(ROOT, "cloth-splatting_amd", "csrc")
    text = {f: re.sub(r"//.*", "", open(os.path.join(csrc, f)).read()) for f in sorted(os.listdir(csrc))
            if f.endswith((".hip", ".h")) and not f.startswith(("csplat_raster", "csplat_k8_views_body"))}
    everything = "\n".join(text.values())
    overloads = {"block_put": 2, "block_sum": 2}                    # (the end of block_put's recursion; block_sum for one plain row of slots)
    for fn in ("finite_f32", "wave_reduce_each", "wave_reduce", "wave_sum", "wave_min", "wave_max", "wave_sum_each", "block_put", "block_stash",
               "block_join", "block_sum", "project_pixel", "relu_keep_nan"):      # (a definition starts its line with `template <...>` or __device__)
        where = [f for f, t in text.items() for _ in re.findall(r"^(?:template <[^\n]*> )?__device__[^\n;(]*\b" + fn + r"\(", t, flags=re.M)]
        assert where == (["csplat_common.h"] if fn == "relu_keep_nan" else ["csplat_device.h"] * overloads.get(fn, 1)), (fn, where)
    for once in ("struct PixelProj", "typedef float f32x16", "struct OpSum", "struct OpMin", "struct OpMax"):
        assert everything.count(once) == 1 and once in text["csplat_device.h"], once
    # a (value, index) pair does not fit the helpers: the farthest point of k_fps (csplat_knn.hip), the apex and the nearest point of the
    # triangulation (csplat_delaunay.hip).  Kept for speed, each with a comment that says so: the minimum and maximum in step of
    # block_minmax6_store (csplat_knn.hip), the block sum and the G-lane sums of the regularisers (csplat_knn_regs.hip)
    allowed = {"csplat_device.h": [r"v = op\(v, __shfl_xor\(v, o, 64\)\)"],
               "csplat_knn.hip": [r"const float ov = __shfl_xor\(bv, o, 64\);", r"const int oi = __shfl_xor\(bi, o, 64\);"] * 2 +
                                 [r"lo = fminf\(lo, __shfl_xor\(lo, o, 64\)\); hi = fmaxf\(hi, __shfl_xor\(hi, o, 64\)\);"],
               "csplat_knn_regs.hip": [r"v \+= __shfl_xor\(v, o, 64\);", r"am\[a\] \+= __shfl_xor\(am\[a\], o, 64\);",
                                       r"aq\[a\] \+= __shfl_xor\(aq\[a\], o, 64\);"],
               "csplat_delaunay.hip": [r"const int other = __shfl_xor\(best, off, CSPLAT_WAVE\);"] * 2}
    in_scope = ("csplat_device.h", "csplat_sim.hip", "csplat_gnn.hip", "csplat_plan.hip", "csplat_observation.hip", "csplat_knn.hip",
                "csplat_knn_regs.hip", "csplat_image.hip", "csplat_tracking.hip", "csplat_flow_loss.hip", "csplat_mesh.hip", "csplat_delaunay.hip",
                "csplat_edge_mlp.hip", "csplat_gemm.hip")
    for f in in_scope:
        rest = text[f]
        for pat in allowed.get(f, []):
            assert re.search(pat, rest), (f, pat)
            rest = re.sub(pat, "", rest, count=1)
        assert "__shfl_xor(" not in rest, f
        assert f in ("csplat_device.h", "csplat_knn_regs.hip") or '#include "csplat_device.h"' in rest, f
    for f, t in text.items():                                       # (the raw text: a comment says why a site stayed)
        raw = open(os.path.join(csrc, f)).read()
        kept = len(re.findall(r"its own loops?[,:]? not \w+(?:<G>)? of csplat_device\.h|its own loop: minimum and maximum in step", raw))
        assert kept == {"csplat_knn.hip": 1, "csplat_knn_regs.hip": 2}.get(f, 0), (f, kept)
    assert "fp contract" not in text["csplat_device.h"] and "half_sum(" not in text["csplat_gnn.hip"]


def test_the_library_refuses_bad_arguments_before_any_launch():
    """fake, distinct, aligned addresses 2^32 apart: every call here must be refused (or be a no-op) before a launch could touch them"""
    from csplat import native
    L = native.lib
    A = lambda i: (i + 1) << 32  # noqa: E731
    sm = lambda T_=3, N=100, K=20, pts=A(0), sigma=0.1, out=A(1), d2=A(2), idx=A(3): L.csplat_traj_smooth(None, T_, N, K, pts, sigma, out, d2, idx)  # noqa: E731
    for kw in (dict(K=0), dict(K=33), dict(K=-1), dict(sigma=0.0), dict(sigma=-1.0), dict(sigma=NAN), dict(sigma=INF), dict(T_=-1), dict(N=-1),
               dict(T_=2 ** 15, N=2 ** 15, K=2), dict(T_=1, N=2 ** 30, K=2), dict(T_=65536, N=32768, K=1), dict(pts=None), dict(out=None),
               dict(pts=A(0) + 2), dict(out=A(1) + 1), dict(d2=A(2) + 3), dict(idx=A(3) + 2), dict(out=A(0)), dict(out=A(0) + 3 * 100 * 12 - 4),
               dict(d2=A(0) + 16), dict(idx=A(0) + 8), dict(d2=A(1) + 8), dict(idx=A(1)), dict(idx=A(2) + 3 * 100 * 20 * 4 - 4)):
        assert sm(**kw) == 2, kw
        assert b"csplat_traj_smooth" in L.csplat_last_error(), kw
    assert sm(T_=0) == 0 and sm(N=0) == 0 and sm(T_=0, pts=None, out=None) == 0 and sm(N=0, pts=None, out=None, d2=None, idx=None) == 0
    ft = lambda T_=3, N=100, E=50, pos=A(0), ei=A(1), inv=20.0, vel=A(2), disp=A(3), norm=A(4): \
        L.csplat_traj_features(None, T_, N, E, pos, ei, inv, vel, disp, norm)  # noqa: E731
    for kw in (dict(T_=-1), dict(N=-1), dict(E=-1), dict(T_=2 ** 16, N=2 ** 15), dict(T_=2, E=2 ** 30), dict(E=2 ** 31), dict(inv=NAN), dict(inv=INF),
               dict(disp=None), dict(norm=None), dict(pos=None), dict(ei=None), dict(pos=A(0) + 2), dict(ei=A(1) + 4), dict(vel=A(2) + 1), dict(disp=A(3) + 2),
               dict(norm=A(4) + 3), dict(vel=A(0)), dict(disp=A(0) + 3 * 100 * 12 - 4), dict(norm=A(1) + 8), dict(vel=A(1) + 2 * 50 * 8 - 4), dict(disp=A(2) + 16),
               dict(norm=A(2)), dict(norm=A(3) + 3 * 50 * 12 - 4)):
        assert ft(**kw) == 2, kw
        assert b"csplat_traj_features" in L.csplat_last_error(), kw
    # nothing to do: no launch, no error -- T = 0; N = 0 (no node an edge could name); E = 0 when the velocities are not wanted either
    assert ft(T_=0) == 0 and ft(N=0) == 0 and ft(N=0, E=0) == 0 and ft(E=0, vel=None) == 0 and ft(vel=None, disp=None, norm=None) == 0
    assert ft(T_=0, pos=None, ei=None, vel=None, disp=None, norm=None) == 0
