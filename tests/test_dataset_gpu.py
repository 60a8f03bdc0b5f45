"""The MeshNet sample data set on the GPU (csplat_dataset_batch / csplat_dataset_rollout_error in csrc/csplat_dataset.hip, behind
meshnet.dataloader_sim) against the numpy restatement tests/dataset_ref.py, under strict dispatch.

Batches: every field of Batch is compared with torch.equal against the float32 restatement -- the outputs are gathers plus one exactly
rounded add or subtract, so there is no tolerance -- and edge_features with torch.equal against meshnet.rollout.edge_features on the
batch's own positions and edge_index.  Two runs are compared bit for bit.

Sizes, and the launch constant each crosses (DATASET_THREADS = 256 work items per workgroup; a sample's work items are the floats of its
node outputs, one array after the other -- N * 3H velocity, N node types, 3N positions, three times N * 3F -- and then its E edges; the
grid is (ceil(largest sample / 256), B)): N = 1, 2 put a whole sample into one workgroup, every seam between two output arrays inside one
wave; N = 255, 256, 257 spread the arrays over 10 .. 40 workgroups with the seams before, on and behind a workgroup edge (N = 256, H = 1:
the velocity block ends exactly on one).  E = 0 (no edge part, NULL edge outputs), E = 1 and E = 3N + 1 with a duplicate and a self loop;
the grasped node first (0) and last (N - 1); B = 1, 2 and 33 (the grid's second axis; repeats of a sample among them); one batch mixing
three trajectories of different N and E with the first and the last sample of each.  (H, F) = (1, 1), (3, 2), (2, 3).

rollout_errors: S = 1, 2, 17 at the same N, against the float64 restatement under the bar rule of tests/test_train_kernels_gpu.py (its
check() and TABLE: 8 x the float32 restatement's own error, floor 1e-6, relative to the largest error of the rollout); two runs bit-equal.

What the table showed on an MI355X when this file was written (group | comparisons | largest e32 | largest bar | largest kernel error |
smallest bar / error):
  dataset rollout_errors | 15 | 2.47e-05 | 1.97e-04 | 2.46e-05 | 8.0
The kernel adds the predictions in the restatement's order, so its error IS the float32 restatement's (13 of the 15 rows agree to the
printed digits; the other two differ in the order of the final sum): 1.6e-7 .. 2.4e-6 from N = 255 on, where the mean runs over 765
components and more, and up to 2.5e-5 at N = 1, S = 17, where it is three components after seventeen rounded additions each.  The smallest
bar / error, 8.0, is therefore the rule's own factor.  Every Batch field was equal to the restatement bit for bit at every size.
Wall time 6 s for the 16 tests of this file (the slowest, the train step on two copies of the simulator, 2 s)."""
import copy

import numpy as np
import pytest

import util  # noqa: F401
import dataset_ref as R
from test_dataset_cpu import NP, flags, same  # noqa: F401  (the comparison of a Batch with the restatement, field by field)
from test_train_kernels_gpu import FLOOR, K, TABLE, check  # noqa: F401  (the project's rule for a bar, and the table of its comparisons)
from test_train_sim_gpu import simulator  # noqa: F401  (the small ClothMeshSimulator: latent 128, H = 2, trained normalisers)

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
from csplat import native  # noqa: E402
from meshnet import dataloader_sim as dl, rollout  # noqa: E402  (absent: every test of this file fails)
from meshnet.dataloader_sim import SamplesClothSimDataset, rollout_errors  # noqa: E402
from meshnet.train_sim import collate, train_step  # noqa: E402

W = R.WORKGROUP
SIZES = [1, 2, W - 1, W, W + 1]


@pytest.fixture(scope="module", autouse=True)
def _table():
    yield
    print("\ngroup | comparisons | largest e32 | largest bar | largest kernel error | smallest bar / error")
    for g in sorted(g for g in TABLE if g.startswith("dataset")):
        n, e32, bar, err, margin = TABLE[g]
        print(f"{g} | {n} | {e32:.2e} | {bar:.2e} | {err:.2e} | {margin:.1f}")


def on_gpu(tr, dtype=torch.float32):
    d = {k: (torch.from_numpy(np.array(v)).cuda() if isinstance(v, np.ndarray) else v) for k, v in R.as_input(tr).items()}
    return {k: (v.to(dtype) if torch.is_tensor(v) and v.dtype.is_floating_point else v) for k, v in d.items()}


def dataset(trajs, H, F, dtype=torch.float32):
    ds = SamplesClothSimDataset(None, H, flags(F))
    for tr in trajs:
        ds.add_trajectory(on_gpu(tr, dtype), symmetric=False)
    return ds


def pairs(trajs, H, F, idx):
    Ts = [tr["pos"].shape[0] for tr in trajs]
    return [R.locate(Ts, H, F, int(i)) for i in idx]


def whole(ds, trajs, H, F, idx, what, actions=None):
    """one batch on the kernel: every field against the restatement, the edge features against the rollout's kernel, two runs"""
    act = None if actions is None else torch.from_numpy(actions).cuda()
    b = ds.batch(idx, act)
    assert all(t.is_cuda for t in b) and b.velocity.dtype == torch.float32
    same(b, R.batch(trajs, pairs(trajs, H, F, idx), H, F, np.float32, actions=actions), what)
    assert torch.equal(b.edge_features, rollout.edge_features(b.positions, b.edge_index)), what
    again = ds.batch(idx, act)
    assert all(torch.equal(x, y) for x, y in zip(b, again)), what
    return b


@pytest.mark.parametrize("N", SIZES)
def test_batch_fields_at_the_launch_edges(N):
    for E, (H, F) in ((0, (1, 1)), (1, (3, 2)), (3 * N + 1, (2, 3))):
        for g in sorted({0, N - 1}):
            trajs = [R.trajectory(H + F + 2, N, E, g, seed=N + E)]
            ds = dataset(trajs, H, F)
            assert len(ds) == 3
            for B in (1, 2, 33):
                idx = (np.arange(B) * 2 + 1) % 3 if B > 1 else np.array([2])
                whole(ds, trajs, H, F, idx, f"N{N} E{E} H{H} F{F} g{g} B{B}")


def test_a_batch_that_mixes_trajectories_of_different_sizes():
    H, F = 2, 2
    trajs = [R.trajectory(T, N, E, g, seed=T) for T, N, E, g in ((6, W + 1, 700, 5), (4, 3, 0, 2), (9, 40, 1, 39), (12, 300, 1801, 0))]
    ds = dataset(trajs, H, F)
    per = R.lengths([6, 4, 9, 12], H, F)
    ends, start = [], 0
    for n in per:
        ends += [start, start + n - 1]
        start += n
    b = whole(ds, trajs, H, F, np.array(ends[::-1] + ends), "mixed")
    assert b.ptr[-1] == 4 * (W + 1 + 3 + 40 + 300) and b.edge_index.shape[1] == 4 * (700 + 1 + 1801)


def test_an_epoch_of_batches_is_batch_of_the_same_slices():
    H, F = 2, 1
    trajs = [R.trajectory(T, N, E, 1, seed=T) for T, N, E in ((9, 30, 50), (3, 7, 4), (8, 12, 0))]
    ds = dataset(trajs, H, F)
    n = len(ds)
    order = torch.randperm(n, generator=torch.Generator().manual_seed(4)).tolist()
    got = list(ds.batches(4, shuffle=True, generator=torch.Generator().manual_seed(4)))
    assert len(got) == -(-n // 4) and n % 4 != 0
    for k, b in enumerate(got):
        idx = order[4 * k:4 * k + 4]
        same(b, R.batch(trajs, pairs(trajs, H, F, idx), H, F, np.float32), f"slice {k}")
        assert all(torch.equal(x, y) for x, y in zip(b, ds.batch(idx))), k
        assert b.velocity.data_ptr() % 16 == 0


def test_candidate_batch_is_the_batch_of_hand_composed_samples():
    H, F, A, N = 2, 3, 33, 300
    trajs = [R.trajectory(8, N, 1801, 17, seed=3)]
    ds = dataset(trajs, H, F)
    acts = np.random.default_rng(1).normal(0, 1e-2, (A, F, 3)).astype(np.float32)
    c = ds.get_batch_with_candidate_actions(2, torch.from_numpy(acts).cuda())
    same(c, R.batch(trajs, [(0, H + 2)] * A, H, F, np.float32, actions=acts), "candidates")
    assert torch.equal(c.edge_features, rollout.edge_features(c.positions, c.edge_index))
    assert (c.B, c.N) == (A, N) and c.hist.shape == (H, A * N, 3) and torch.equal(torch.cat(list(c.hist), 1), c.velocity)
    assert torch.equal(c.batch, torch.arange(A, device="cuda").repeat_interleave(N))
    whole(ds, trajs, H, F, np.full(A, 2), "override", actions=acts)


def test_what_the_kernels_do_not_cover_is_refused_or_reported():
    trajs = [R.trajectory(6, 9, 12, 0, seed=1, dtype=np.float64)]
    ds = dataset(trajs, 2, 1)
    with pytest.raises(ValueError, match="blocking read"):
        ds.batch(torch.tensor([0], device="cuda"))
    ds64 = dataset(trajs, 2, 1, torch.float64)
    with pytest.raises(native.CsplatError, match="dataloader_sim.batch"):
        ds64.batch([0])
    with native.allow_fallbacks("dtype"):
        b = ds64.batch([0, 2])
    ref = R.batch(trajs, [(0, 2), (0, 4)], 2, 1, np.float64)
    for k in R.FIELDS + ("ptr", "grasped_rows"):
        got, want = getattr(b, k).cpu(), torch.from_numpy(ref[k])
        if k == "edge_features":              # (the device's float64 square root)
            assert torch.equal(got[:, :3], want[:, :3]) and torch.allclose(got[:, 3], want[:, 3], rtol=1e-15, atol=0)
        else:
            assert torch.equal(got, want), k
    p = torch.zeros(4, 3, dtype=torch.float64, device="cuda")
    with pytest.raises(native.CsplatError, match="rollout_errors"):
        rollout_errors(p, p[None], p[None])


# ================================================================================================ the train step takes a batch as it is
def cloth_trajectory(T, seed=0):
    """a 15 x 20 jittered grid of spacing 0.02 drifting by a quarter of the spacing per frame, every node receiving an edge from each of
    its 7 nearest (2100 edges), one grasped node"""
    rng = np.random.default_rng(40 + seed)
    xs, ys = np.meshgrid(np.arange(15.0), np.arange(20.0), indexing="ij")
    rest = np.stack([xs.reshape(-1), ys.reshape(-1), np.zeros(300)], 1) * 0.02 + (rng.random((300, 3)) - 0.5) * 0.004
    pos = (rest[None] + np.cumsum(rng.normal(0, 5e-3, (T, 300, 3)), 0)).astype(np.float32)
    d2 = ((rest[:, None] - rest[None]) ** 2).sum(2)
    near = np.argsort(d2, 1, kind="stable")[:, 1:8]
    edges = np.stack([near.reshape(-1), np.repeat(np.arange(300), 7)]).astype(np.int64)
    vel = np.zeros_like(pos)
    vel[1:] = pos[1:] - pos[:-1]
    g = 153 + seed
    nt = np.zeros((T, 300, 1), np.float32)
    nt[:, g] = 1
    return {"pos": pos, "velocity": vel, "node_type": nt, "actions": rng.normal(0, 5e-3, (T, 3)).astype(np.float32), "edges": edges, "grasped": g}


def by_hand(tr, t, H, F):
    """one sample from torch operations and rollout.edge_features: the path a user had before the data set"""
    P, V, A, nt = (torch.from_numpy(tr[k]).cuda() for k in ("pos", "velocity", "actions", "node_type"))
    ei, g = torch.from_numpy(tr["edges"]).cuda(), tr["grasped"]
    vel = torch.cat([V[t - H + h] for h in range(H)], 1)
    vel[g, 3 * (H - 1):] = V[t, g]
    pos = P[t - 1].clone()
    pos[g] += A[t - 1]
    pa = torch.zeros(P.shape[1], F, 3, device="cuda")
    pa[g] = A[t - 1:t - 1 + F]
    return vel, nt[t - 1], ei, rollout.edge_features(pos, ei), V[t:t + F].transpose(0, 1).contiguous(), pa, pos


def test_train_step_takes_the_batch_and_gives_the_loss_of_the_hand_collated_samples(simulator):  # noqa: F811
    H, F = 2, 3
    trajs = [cloth_trajectory(8, 0), cloth_trajectory(6, 1)]
    ds = dataset(trajs, H, F)
    idx = [0, len(ds) - 1, 2]
    b = ds.batch(idx)
    hand = collate([by_hand(trajs[j], t, H, F) for j, t in pairs(trajs, H, F, idx)])
    assert all(torch.equal(x, y) for x, y in zip(b[:7], hand))
    results, sims = [], [copy.deepcopy(simulator).train() for _ in range(2)]
    for sim, batch in zip(sims, (b, hand)):
        opt = torch.optim.Adam(sim.parameters(), lr=1e-3)
        results.append(train_step(sim, opt, batch, future_sequence_length=F, noise_std=0.0))          # (the Batch itself, unchanged)
    assert torch.equal(results[0][0], results[1][0]) and len(results[0][1]) == F and bool(torch.isfinite(results[0][0]))
    assert all(torch.equal(x, y) for x, y in zip(results[0][1], results[1][1]))
    assert all(torch.equal(p, q) for p, q in zip(sims[0].parameters(), sims[1].parameters()))
    assert any(not torch.equal(p, q) for p, q in zip(sims[0].parameters(), simulator.parameters()))


# ================================================================================================ validation
@pytest.mark.parametrize("N", SIZES)
def test_rollout_errors_against_float64(N):
    for S in (1, 2, 17):
        rng = np.random.default_rng(100 * N + S)
        pos0 = rng.uniform(-1, 1, (N, 3)).astype(np.float32)
        pred = rng.normal(0, 1e-2, (S, N, 3)).astype(np.float32)
        gt = (pos0[None].astype(np.float64) + np.cumsum(pred.astype(np.float64), 0) + rng.normal(0, 3e-3, (S, N, 3))).astype(np.float32)
        args = [torch.from_numpy(a).cuda() for a in (pos0, pred, gt)]
        got = rollout_errors(*args)
        assert got.shape == (S,) and got.dtype == torch.float32
        check("dataset rollout_errors", f"N{N} S{S}", got, R.rollout_errors(pos0, pred, gt, np.float64), R.rollout_errors(pos0, pred, gt, np.float32), 0.0)
        assert torch.equal(rollout_errors(*args), got)


def test_validate_is_the_rollout_of_the_validation_item(simulator):  # noqa: F811
    H = 2
    trajs = [cloth_trajectory(9, 0)]
    ds = dataset(trajs, H, 1)
    out = dl.validate(simulator, ds, 1, future=4)
    item = ds.val_item(1, 4)
    assert len(item["actions"]) == 4 and out.shape == (5,) and float(out[0]) == 0.0
    pred, _final = rollout.rollout(simulator, item["pos"][0], item["vel"][:H], item["node_type"], item["edge_index"], item["actions"],
                                   item["grasped_particle"], 4)
    assert torch.equal(out[1:], rollout_errors(item["pos"][0], pred.contiguous(), item["pos"][1:]))
    want = R.rollout_errors(item["pos"][0].cpu().numpy(), pred.cpu().numpy(), item["pos"][1:].cpu().numpy(), np.float64)
    assert np.abs(out[1:].cpu().numpy() - want).max() <= 1e-4 * want.max() and bool((out[1:] > 0).all())      # (a sanity check: the bars are above)
