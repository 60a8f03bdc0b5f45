"""The MeshNet sample data set (meshnet/dataloader_sim.py: SamplesClothSimDataset and its helpers) without a GPU: the index table and the
composed CPU path against the numpy restatement tests/dataset_ref.py -- every field with torch.equal, in float32 and float64 -- the edge
rules against hand-written lists, and the C-ABI of csplat_dataset_batch / csplat_dataset_rollout_error: exports, header block, and every
refusal through the library itself with a NULL stream and fake addresses (each is refused before a launch could touch them).

tests/test_dataset_gpu.py runs the kernels; which launch constant each of its sizes crosses is stated there and checked here against the
source (test_which_launch_constant_each_gpu_size_crosses)."""
import os
import re
import types

import numpy as np
import pytest

import util  # noqa: F401
import dataset_ref as R

torch = pytest.importorskip("torch")
from meshnet import data_utils as du  # noqa: E402
from meshnet import dataloader_sim as dl  # noqa: E402  (absent: every test of this file fails)
from meshnet.dataloader_sim import SamplesClothSimDataset, face_to_edge, get_goal_fold, rollout_errors, symmetric_edges  # noqa: E402

ROOT = util.ROOT
SRC = os.path.join(ROOT, "cloth-splatting_amd", "csrc", "csplat_dataset.hip")
SHAPES = ((7, 5, 6), (4, 3, 0), (12, 8, 10))           # (T, N, E) of the three trajectories; the second is shorter than H + F from 5 on
NP = {torch.float32: np.float32, torch.float64: np.float64}


def flags(F=1):
    return types.SimpleNamespace(action_steps=1, future_sequence_length=F)


def build(H, F, dtype=np.float32, shapes=SHAPES, grasped=(0, 2, 7)):
    trajs = [R.trajectory(T, N, E, g, seed=10 * k + H, dtype=dtype) for k, ((T, N, E), g) in enumerate(zip(shapes, grasped))]
    ds = SamplesClothSimDataset(None, H, flags(F))
    for tr in trajs:
        ds.add_trajectory(R.as_input(tr), symmetric=False)
    return ds, trajs


def same(batch, ref, what=""):
    for k in R.FIELDS + ("ptr", "grasped_rows"):
        got, want = getattr(batch, k), torch.from_numpy(ref[k])
        assert got.dtype == want.dtype and got.shape == want.shape, (what, k, got.dtype, got.shape, want.dtype, want.shape)
        assert torch.equal(got.cpu(), want), (what, k)


# ------------------------------------------------------------------------------------------------------------------ the index table
@pytest.mark.parametrize("H", [1, 2, 3])
@pytest.mark.parametrize("F", [1, 2, 3])
def test_index_table_and_lookup(H, F):
    ds, _trajs = build(H, 1)
    ds.set_future_sequence_length(F)
    Ts = [s[0] for s in SHAPES]
    per = R.lengths(Ts, H, F)
    assert len(ds) == sum(per) and ds._data_lengths == per and ds._precompute_cumlengths.tolist() == np.cumsum(per).tolist()
    if H + F > 4:
        assert per[1] == 0                                          # a trajectory shorter than H + F contributes none
    edges = {len(ds) - 1}
    start = 0
    for n in per:
        if n:
            edges |= {start, start + n - 1}                         # the first and the last sample of every trajectory
        start += n
    for idx in sorted(edges) + list(range(len(ds))):
        j, t = ds.locate([idx])
        assert (int(j[0]), int(t[0])) == R.locate(Ts, H, F, idx), idx
    j, t = ds.locate(np.arange(len(ds)))
    assert [(int(a), int(b)) for a, b in zip(j, t)] == [R.locate(Ts, H, F, i) for i in range(len(ds))]
    for bad in (-1, len(ds)):
        with pytest.raises(IndexError, match="outside"):
            ds.batch([bad])
        with pytest.raises(IndexError):
            ds[bad]


def test_the_reference_spelling_of_the_curriculum_recomputes_the_table():
    ds, trajs = build(2, 1, np.float64)
    n1 = len(ds)
    ds._future_sequence_length = 3
    with pytest.raises(ValueError, match="_compute_cumulative_lengths"):           # a stale table is refused, not read past a trajectory
        ds.batch([0])
    ds._compute_cumulative_lengths()
    Ts = [s[0] for s in SHAPES]
    assert len(ds) == sum(R.lengths(Ts, 2, 3)) < n1
    pairs = [R.locate(Ts, 2, 3, i) for i in range(len(ds))]
    same(ds.batch(range(len(ds))), R.batch(trajs, pairs, 2, 3, np.float64))
    with pytest.raises(ValueError, match="future_sequence_length"):
        ds.set_future_sequence_length(0)


def test_argument_errors():
    with pytest.raises(NotImplementedError, match="data_path=None"):
        SamplesClothSimDataset("some/dir", 2, flags())
    with pytest.raises(ValueError, match="input_length_sequence"):
        SamplesClothSimDataset(None, 17, flags())
    ds, trajs = build(2, 1)
    good = R.as_input(trajs[0])
    for key in ("pos", "velocity", "node_type", "actions", "grasped_particle"):
        with pytest.raises(ValueError, match=key):
            ds.add_trajectory({k: v for k, v in good.items() if k != key})
    for bad in (dict(velocity=good["velocity"][:-1]), dict(actions=good["actions"][:, :2]), dict(grasped_particle=1.5),
                dict(edge_index=None), dict(pos=good["pos"].astype(np.int64)), dict(edge_index=good["edge_index"] + 5)):
        with pytest.raises(ValueError, match="add_trajectory"):
            ds.add_trajectory(dict(good, **bad))
    with pytest.raises(ValueError, match="integers"):
        ds.batch([0.5])
    with pytest.raises(ValueError, match="candidate_actions"):
        ds.batch([0, 1], torch.zeros(2, 2, 3))
    with pytest.raises(ValueError, match="batch_size"):
        next(ds.batches(0))
    with pytest.raises(TypeError):
        ds[[0, 1]]
    with pytest.raises(ValueError, match="future"):
        ds.val_item(0, future=-2)
    assert ds.num_trajectories == 3 and len(ds.batch([]).ptr) == 1 and ds.batch([]).velocity.shape == (0, 6)


# ------------------------------------------------------------------------------------------------------------------ the composed path
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("H,F", [(1, 1), (2, 3), (3, 2)])
def test_composed_batch_equals_the_restatement(dtype, H, F):
    ds, trajs = build(H, F, NP[dtype])
    Ts = [s[0] for s in SHAPES]
    n = len(ds)
    order = np.random.default_rng(H).permutation(n)
    for what, idx in (("all", np.arange(n)), ("shuffled with a repeat", np.concatenate([order, order[:1]])), ("one", [n - 1])):
        b = ds.batch(idx)
        assert b.velocity.dtype == dtype
        same(b, R.batch(trajs, [R.locate(Ts, H, F, int(i)) for i in idx], H, F, NP[dtype]), what)
    same(ds[0], R.batch(trajs, [R.locate(Ts, H, F, 0)], H, F, NP[dtype]), "ds[0]")
    same(ds.batch(torch.tensor([1, 0])), R.batch(trajs, [R.locate(Ts, H, F, 1), R.locate(Ts, H, F, 0)], H, F, NP[dtype]), "a CPU tensor")
    # the first seven fields are the tuple of train_step, and the edge features have the sign and layout of rollout.edge_features
    assert dl.Batch._fields[:7] == ("velocity", "node_types", "edge_index", "edge_features", "target_velocities", "particle_actions", "positions")
    b = ds.batch(np.arange(n))
    d = b.positions[b.edge_index[0]] - b.positions[b.edge_index[1]]
    assert torch.equal(b.edge_features[:, :3], d)
    assert torch.allclose(b.edge_features[:, 3], d.norm(dim=1), rtol=1e-6 if dtype == torch.float32 else 1e-14, atol=0)


def test_a_trajectory_without_a_grasped_node_moves_nothing():
    ds, trajs = build(2, 2, np.float64, grasped=(-1, 3, 8))
    Ts = [s[0] for s in SHAPES]
    b = ds.batch(range(len(ds)))
    same(b, R.batch(trajs, [R.locate(Ts, 2, 2, i) for i in range(len(ds))], 2, 2, np.float64))
    assert (b.grasped_rows == -1).all() and not b.particle_actions.any()


def test_candidate_batch_is_the_batch_of_hand_composed_samples():
    H, F, A = 2, 3, 4
    ds, trajs = build(H, F, np.float32)
    Ts = [s[0] for s in SHAPES]
    idx = len(ds) - 1
    acts = np.random.default_rng(3).normal(0, 1e-2, (A, F, 3)).astype(np.float32)
    c = ds.get_batch_with_candidate_actions(idx, torch.from_numpy(acts))
    j, t = R.locate(Ts, H, F, idx)
    same(c, R.batch(trajs, [(j, t)] * A, H, F, np.float32, actions=acts))
    N = SHAPES[j][1]
    assert (c.B, c.N) == (A, N) and c.pos is c.positions and c.node_type is c.node_types
    assert c.hist.shape == (H, A * N, 3) and torch.equal(torch.cat(list(c.hist), 1), c.velocity)
    assert c.batch.tolist() == [a for a in range(A) for _ in range(N)]
    from meshnet.mpc import CandidateBatch
    assert set(CandidateBatch._fields) <= set(c._fields)
    with pytest.raises(ValueError, match="candidate_actions"):
        ds.get_batch_with_candidate_actions(idx, torch.zeros(A, F + 1, 3))


@pytest.mark.parametrize("H", [1, 2, 3])
def test_val_item_views_future_minus_one_and_the_clamp(H):
    ds, trajs = build(H, 1, np.float64)
    Ts = [s[0] for s in SHAPES]
    for idx in range(len(ds)):
        j, t = R.locate(Ts, H, 1, idx)
        for future in (1, 2, 5, 100, -1):
            got, want = ds.__get_val_item__(idx, future), R.val_item(trajs[j], t, H, future)
            for k, v in want.items():
                assert (got[k] == v) if k == "grasped_particle" else torch.equal(got[k], torch.from_numpy(np.ascontiguousarray(v))), (idx, future, k)
            assert got["faces"] is None and len(got["actions"]) == len(got["pos"]) - 1 == len(got["vel"]) - H
            if future == -1:
                assert len(got["pos"]) == Ts[j] - H + 1
            else:
                assert len(got["actions"]) == min(future, Ts[j] - 1 - t)
    item = ds.val_item(0, 2)
    assert item["pos"].data_ptr() == ds.trajectory(0)["pos"][H - 1].data_ptr()                # a view of the store


def test_batches_is_batch_of_the_same_slices():
    ds, _trajs = build(2, 1, np.float32)
    n = len(ds)
    g = torch.Generator().manual_seed(11)
    order = torch.randperm(n, generator=torch.Generator().manual_seed(11)).tolist()
    got = list(ds.batches(4, shuffle=True, generator=g))
    assert len(got) == -(-n // 4)
    for k, b in enumerate(got):
        want = ds.batch(order[4 * k:4 * k + 4])
        assert all(torch.equal(x, y) for x, y in zip(b, want)), k
    assert [int(b.ptr.shape[0]) - 1 for b in ds.batches(4, shuffle=False, drop_last=True)] == [4] * (n // 4)
    first = next(ds.batches(3, shuffle=False))
    assert all(torch.equal(x, y) for x, y in zip(first, ds.batch([0, 1, 2])))
    assert list(SamplesClothSimDataset(None, 2, flags()).batches(4)) == []


def test_the_store_grows_geometrically_and_replaces_its_last_trajectory():
    ds = SamplesClothSimDataset(None, 2, flags())
    trs = [R.trajectory(6, 40, 30, 1, seed=s, dtype=np.float64) for s in range(12)]
    ds.add_trajectory(R.as_input(trs[0]), symmetric=False)
    first = ds.allocations
    for tr in trs[1:4]:
        ds.add_trajectory(R.as_input(tr), symmetric=False)            # 4 x 240 rows fit the first 1024
    assert ds.allocations == first == 5
    for tr in trs[4:]:
        ds.add_trajectory(R.as_input(tr), symmetric=False)
    assert ds.allocations == first + 6 and ds._buf["pos"].shape[0] == 4096          # the three node buffers doubled twice, nothing else grew
    for j, tr in enumerate(trs):
        assert torch.equal(ds.trajectory(j)["pos"], torch.from_numpy(tr["pos"])) and torch.equal(ds.trajectory(j)["edge_index"], torch.from_numpy(tr["edges"]))
    n = len(ds)
    ds._pop_last()
    ds.add_trajectory(R.as_input(R.trajectory(9, 7, 3, 0, seed=99, dtype=np.float64)), symmetric=False)
    assert ds.num_trajectories == 12 and len(ds) == n - 4 + 7 and ds.trajectory(11)["pos"].shape == (9, 7, 3)
    assert ds.trajectory(0)["faces"] is None


# ------------------------------------------------------------------------------------------------------------------ edges
def test_face_to_edge_and_the_symmetric_rule_against_hand_written_lists():
    faces = torch.tensor([[0, 1], [1, 2], [2, 3]])                                  # the triangles (0,1,2) and (1,2,3)
    assert face_to_edge(faces, 4).tolist() == [[0, 0, 1, 1, 1, 2, 2, 2, 3, 3], [1, 2, 0, 2, 3, 0, 1, 3, 1, 2]]
    assert face_to_edge(faces, 4).dtype == torch.int64
    ei = torch.tensor([[2, 0, 0, 1], [0, 1, 1, 1]])                                  # a duplicate and a self loop
    assert symmetric_edges(ei, 3).tolist() == [[0, 0, 1, 1, 2], [1, 2, 0, 1, 0]]
    assert symmetric_edges(torch.zeros(2, 0, dtype=torch.int64), 3).shape == (2, 0)
    rng = np.random.default_rng(0)
    f = rng.integers(0, 9, (3, 14))
    assert face_to_edge(torch.from_numpy(f), 9).tolist() == R.face_to_edge(f, 9).tolist()
    for bad in (torch.zeros(2, 3, dtype=torch.int64), torch.zeros(3, 2)):
        with pytest.raises(ValueError, match="face_to_edge"):
            face_to_edge(bad, 4)
    with pytest.raises(ValueError, match="face_to_edge"):
        face_to_edge(torch.tensor([[0], [1], [4]]), 4)
    # add_trajectory: faces win, otherwise edge_index made symmetric unless told not to
    tr = R.trajectory(5, 4, 4, 0, seed=1)
    ds = SamplesClothSimDataset(None, 1, flags())
    ds.add_trajectory(dict(R.as_input(tr), edge_faces=np.broadcast_to(faces.numpy()[None], (5, 3, 2))))
    ds.add_trajectory(R.as_input(tr))
    ds.add_trajectory(R.as_input(tr), symmetric=False)
    assert ds.trajectory(0)["edge_index"].tolist() == face_to_edge(faces, 4).tolist() and ds.trajectory(0)["faces"].tolist() == faces.tolist()
    assert ds.trajectory(1)["edge_index"].tolist() == R.symmetric(tr["edges"], 4).tolist()
    assert ds.trajectory(2)["edge_index"].tolist() == tr["edges"].tolist()


# ------------------------------------------------------------------------------------------------------------------ the online trajectory
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_collect_observation_all_three_modalities_and_replace_last(monkeypatch, dtype):
    H, F, N = 2, 2, 6
    ei = torch.tensor([[0, 1, 2, 3, 4, 0], [1, 2, 3, 4, 5, 5]])
    real = du.process_traj
    monkeypatch.setattr(du, "process_traj", lambda *a, **kw: real(*a, **dict(kw, edge_index=ei)))      # (the kNN graph needs the GPU)
    rng = np.random.default_rng(5)

    def observation(T):
        t = lambda a: torch.from_numpy(a).to(dtype)  # noqa: E731
        pos = rng.uniform(-1, 1, (1, N, 3)) + np.cumsum(rng.normal(0, 1e-2, (T, N, 3)), 0)
        grip = np.cumsum(rng.normal(0, 1e-2, (T, 3)), 0)
        return {"pos": t(pos), "gripper_pos": t(grip), "actions": t(rng.normal(0, 1e-2, (T, 3))), "pick": t(pos[0, 2] + 1e-3), "place": t(pos[0, 4]),
                "refined_pos": t(pos + rng.normal(0, 1e-3, (T, N, 3))), "predicted_pos": t(pos + rng.normal(0, 1e-3, (T, N, 3)))}

    ds = SamplesClothSimDataset(None, H, flags(F), dt=0.05, sim_data=False)
    params = (0.05, 3, False, False, 300, H, 1)
    with pytest.raises(ValueError, match="first=True"):
        ds.collect_observation(observation(4))
    for T, first, modality in ((4, True, "gt"), (5, False, "cloth_splatting"), (6, False, "open_loop"), (7, False, "gt")):
        obs = observation(T)
        goal = ds.collect_observation(obs, first=first, modality=modality)
        td = du.get_data_traj(None, ds.load_keys, params, observations=obs, sim_data=False, rw_processing=False,
                              sampled_points_indices=torch.arange(N))
        pos, vel = td["pos"].numpy(), td["velocity"].numpy()
        assert pos.shape == (T + H - 1, N, 3)
        if modality != "gt":
            new = obs["refined_pos" if modality == "cloth_splatting" else "predicted_pos"].numpy()
            pos, vel = R.substitute(pos, vel, new, H)
            assert not np.array_equal(pos, td["pos"].numpy()) and np.array_equal(vel[H + 1], new[2] - new[1])      # (not divided by dt)
        tr = {"pos": pos, "velocity": vel, "node_type": td["node_type"].numpy(), "actions": td["actions"].numpy(),
              "edges": R.symmetric(ei.numpy(), N), "grasped": td["grasped_particle"]}
        assert tr["grasped"] == 2
        assert ds.num_trajectories == 1 and len(ds) == T + H - 1 - H - F + 1                     # appended once, replaced afterwards
        assert torch.equal(goal, get_goal_fold(td["pos"][0], td["pick"], td["place"]))
        got = ds.trajectory(0)
        assert torch.equal(got["gt_pos"], td["pos"]) and torch.equal(got["gt_vel"], td["velocity"]) and torch.equal(got["pick"], td["pick"])
        assert torch.equal(got["pos"], torch.from_numpy(pos)) and torch.equal(got["velocity"], torch.from_numpy(vel))
        same(ds.batch(range(len(ds))), R.batch([tr], [(0, H + i) for i in range(len(ds))], H, F, NP[dtype]), modality)
    assert torch.equal(ds.sampled_point_indeces, torch.arange(N))
    with pytest.raises(ValueError, match="modality"):
        ds.collect_observation(observation(4), modality="other")
    with pytest.raises(ValueError, match="refined_pos"):
        ds.collect_observation({k: v for k, v in observation(4).items() if k != "refined_pos"}, modality="cloth_splatting")


# ------------------------------------------------------------------------------------------------------------------ validation
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_rollout_errors_composed(dtype):
    rng = np.random.default_rng(2)
    pos0, pred, gt = rng.uniform(-1, 1, (9, 3)), rng.normal(0, 1e-2, (5, 9, 3)), rng.uniform(-1, 1, (5, 9, 3))
    got = rollout_errors(*(torch.from_numpy(a).to(dtype) for a in (pos0, pred, gt)))
    want = R.rollout_errors(pos0, pred, gt, np.float64)
    assert got.dtype == dtype and got.shape == (5,)
    assert np.abs(got.double().numpy() - want).max() <= (1e-6 if dtype == torch.float32 else 1e-14) * want.max()
    by_hand = ((pos0 + pred[:3].sum(0) - gt[2]) ** 2).mean()
    assert abs(want[2] - by_hand) <= 1e-14 * by_hand
    assert rollout_errors(torch.zeros(4, 3), torch.zeros(0, 4, 3), torch.zeros(0, 4, 3)).shape == (0,)
    for args in ((torch.zeros(4, 2), torch.zeros(1, 4, 3), torch.zeros(1, 4, 3)), (torch.zeros(4, 3), torch.zeros(1, 5, 3), torch.zeros(1, 5, 3)),
                 (torch.zeros(4, 3), torch.zeros(2, 4, 3), torch.zeros(1, 4, 3)), (torch.zeros(0, 3), torch.zeros(1, 0, 3), torch.zeros(1, 0, 3))):
        with pytest.raises(ValueError, match="rollout_errors"):
            rollout_errors(*args)


def test_validate_rolls_the_validation_item(monkeypatch):
    """validate around a stand-in rollout: the history, the actions and the ground truth it hands over, and [0, err_1 .. err_S]"""
    from meshnet import rollout as ro
    H = 2
    ds, trajs = build(H, 1, np.float64)
    seen = {}

    def fake(sim, pos, hist, node_type, edge_index, actions, grasped, nsteps):
        seen.update(pos=pos, hist=hist, actions=actions, grasped=grasped, nsteps=nsteps)
        return actions[:, None, :].expand(nsteps, pos.shape[0], 3) * 2.0, None
    monkeypatch.setattr(ro, "rollout", fake)
    idx = 1
    out = dl.validate(object(), ds, idx, future=3)
    tr, t = trajs[0], H + idx
    assert seen["nsteps"] == 3 and seen["grasped"] == tr["grasped"]
    assert torch.equal(seen["hist"], torch.from_numpy(tr["velocity"][t - H:t])) and torch.equal(seen["pos"], torch.from_numpy(tr["pos"][t - 1]))
    pred = np.broadcast_to(tr["actions"][t - 1:t + 2, None, :] * 2.0, (3, 5, 3))
    want = R.rollout_errors(tr["pos"][t - 1], pred, tr["pos"][t:t + 3], np.float64)
    assert out.shape == (4,) and float(out[0]) == 0.0 and np.abs(out[1:].numpy() - want).max() <= 1e-14 * want.max()
    last = R.lengths([7], H, 1)[0] - 1                                           # t = T - 1: the clamp at T - 1 leaves no step, t = T - 2 one
    assert dl.validate(object(), ds, last, future=3).tolist() == [0.0] and dl.validate(object(), ds, last - 1, future=3).shape == (2,)


# ------------------------------------------------------------------------------------------------------------------ the C-ABI
ENTRIES = (("int", "csplat_dataset_batch", 27), ("int", "csplat_dataset_rollout_error", 7))


def test_header_exports_and_bindings():
    from csplat import native
    header = open(os.path.join(ROOT, "include", "csplat.h")).read()
    for res, name, n_args in ENTRIES:
        m = re.search(r"\b" + res + r"\s+" + name + r"\s*\(([^;]*)\)\s*;", re.sub(r"/\*.*?\*/", "", header, flags=re.S))
        assert m, name
        assert len(m.group(1).split(",")) == n_args, name
        assert len(native.EXPORTS[name][1]) == n_args and hasattr(native.lib, name), name
    block = header[header.index("/* MeshNet sample data set"):]
    block = block[:block.index("*/") + 2]
    assert block.rstrip().endswith("Added exports: CSPLAT_ABI_VERSION is unchanged. */")
    assert native.ABI_VERSION == 9 and native.lib.csplat_abi_version() == 9 and re.search(r"#define\s+CSPLAT_ABI_VERSION\s+9\b", header)
    assert int(re.search(r"#define\s+CSPLAT_DATASET_TABLE_WORDS\s+(\d+)", header).group(1)) == dl.TABLE_WORDS
    code = re.sub(r"//[^\n]*", "", open(SRC).read())
    assert "#pragma clang fp contract(off)" in code and "atomic" not in code.lower() and code.count("<<<") == 2      # one launch each


def test_which_launch_constant_each_gpu_size_crosses():
    """tests/test_dataset_gpu.py runs N = 1, 2, WORKGROUP - 1 / + 0 / + 1: a sample's work items are its N (3H + 4 + 9F) node floats, then
    its E edges, over ceil(items / WORKGROUP) workgroups -- with N = 1, 2 everything sits in one workgroup and the seams between the
    output arrays fall inside a wave; from N = 255 on the velocity block alone spans several workgroups and the seams fall inside,
    on and one past a workgroup edge; B = 33 with the grid's second axis, B = 1 without."""
    code = open(SRC).read()
    assert int(re.search(r"constexpr int DATASET_THREADS = (\d+);", code).group(1)) == R.WORKGROUP == 256
    assert int(re.search(r"constexpr int DATASET_MAX_GRID_X = (\d+);", code).group(1)) * R.WORKGROUP > 257 * (3 * 3 + 4 + 9 * 3) + 3 * 257 + 1


def A(k):
    return 0x100000000 * (k + 1)


def test_the_library_refuses_bad_arguments_before_any_launch():
    """fake, distinct, aligned addresses 2^32 apart: every call here must be refused (or be a no-op) before a launch could touch them"""
    from csplat import native
    L = native.lib
    names = ("pos", "vel", "nt", "act", "edges", "table", "desc", "over", "o_vel", "o_nt", "o_pos", "o_tv", "o_pt", "o_pa", "o_ei", "o_ef")

    def call(**kw):
        a = dict(B=2, H=2, F=2, n_traj=1, rows=100, frames=10, n_edges=20, R=20, Q=30, items=100, **{n: A(k) for k, n in enumerate(names)})
        a.update(kw)
        return L.csplat_dataset_batch(None, a["B"], a["H"], a["F"], a["n_traj"], a["rows"], a["frames"], a["n_edges"], *(a[n] for n in names[:8]),
                                      a["R"], a["Q"], a["items"], *(a[n] for n in names[8:]))
    for kw in (dict(H=0), dict(H=17), dict(F=0), dict(B=-1), dict(R=-1), dict(n_traj=-1), dict(R=2 ** 31), dict(R=2 ** 28), dict(Q=2 ** 29),
               dict(rows=2 ** 31), dict(pos=None), dict(vel=None), dict(nt=None), dict(act=None), dict(edges=None), dict(table=None), dict(desc=None),
               dict(o_vel=None), dict(o_pa=None), dict(o_ei=None), dict(o_ef=None), dict(pos=A(0) + 2), dict(over=A(7) + 1), dict(table=A(5) + 4),
               dict(o_ei=A(14) + 4), dict(desc=A(6) + 8), dict(o_ef=A(15) + 8), dict(o_vel=A(0)), dict(o_vel=A(0) + 100 * 12 - 4),
               dict(o_pos=A(8) + 20 * 24 - 4), dict(o_nt=A(6) + 16), dict(o_pa=A(7)), dict(o_ei=A(4) + 20 * 16 - 8), dict(o_ef=A(5) + 48),
               dict(o_tv=A(12))):
        assert call(**kw) == 2, kw
        assert b"csplat_dataset_batch" in L.csplat_last_error(), kw
    assert call(B=0) == 0 and call(R=0, Q=0) == 0 and call(B=0, pos=None, desc=None) == 0

    def err(**kw):
        a = dict(S=3, N=10, pos0=A(0), pred=A(1), gt=A(2), err=A(3))
        a.update(kw)
        return L.csplat_dataset_rollout_error(None, a["S"], a["N"], a["pos0"], a["pred"], a["gt"], a["err"])
    for kw in (dict(S=-1), dict(N=-1), dict(N=0), dict(S=2 ** 15, N=2 ** 15), dict(pos0=None), dict(pred=None), dict(gt=None), dict(err=None),
               dict(gt=A(2) + 2), dict(err=A(1) + 3 * 120 - 4), dict(err=A(0)), dict(err=A(2))):
        assert err(**kw) == 2, kw
        assert b"csplat_dataset_rollout_error" in L.csplat_last_error(), kw
    assert err(S=0) == 0 and err(S=0, pos0=None, err=None) == 0
