"""Cost of assembling a MeshNet training batch (meshnet.dataloader_sim), written to profiles/meshnet_dataset_cost.txt.

One block-diagonal batch of B samples in front of a training step, two ways:

  batch      SamplesClothSimDataset.batch(indices): descriptors built on the host, one upload, ONE launch (csplat_dataset_batch);
  composed   what the parent commit lets a user write: every sample from torch operations on the trajectory's tensors on the GPU (the
             history side by side, the grasped row's velocity, position and actions written over, the targets transposed), its edge
             features from meshnet.rollout.edge_features, then meshnet.train_sim.collate.  Timed TWICE per round (composed a, composed b):
             their difference is the run-to-run spread of this measurement.

Configurations: B = 1 and B = 32 at 300 nodes / 1800 edges (the reference's cloth and batch size) and B = 1 at 10 000 nodes / 300 000
edges (bench_gnn.py's size), input sequence length 2, future sequence length 1, 2, 3.  Beside each: one train_step on that batch (a
ClothMeshSimulator at latent 128 with 15 message-passing steps, the loss, backward, Adam) and the share of it that assembling the batch
costs either way.

A host clock around `calls` back-to-back calls that end in a device synchronise (both forms are bound by the host: device events alone
would miss the time between launches); after a warm-up of every form; `calls` is chosen per form so that a timed window lasts about
--window seconds; the forms alternate over --rounds rounds, every round's figure is printed and the MEDIAN is the figure of a form.  A
record, not a pass condition; the tool fails without a GPU."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "cloth-splatting_amd"), ROOT, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

from meshnet_train_cost import measure  # noqa: E402  (warm-up, calls sized to the window, alternating rounds)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.3, help="seconds of work per timed window")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--mp-steps", type=int, default=15)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "meshnet_dataset_cost.txt"))
    a = ap.parse_args()
    import types
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("meshnet_dataset_cost: no GPU; a time is only measured on one")
    from bench_gnn import cloth_graph
    from csplat import native
    from meshnet import rollout as ro, train_sim as ts
    from meshnet.cloth_network import ClothMeshSimulator
    from meshnet.dataloader_sim import SamplesClothSimDataset
    dev = torch.device("cuda:0")
    lines = []

    def say(*parts):
        lines.append(" ".join(str(p) for p in parts))
        print(lines[-1], flush=True)

    def small_cloth(gen):
        """a 15 x 20 jittered grid, every node receiving an edge from each of its 6 nearest: 300 nodes, 1800 edges, sorted by (row, col)"""
        xs, ys = torch.meshgrid(torch.arange(15.0), torch.arange(20.0), indexing="ij")
        pos = torch.stack([xs.reshape(-1), ys.reshape(-1), torch.zeros(300)], 1) * 0.02 + (torch.rand(300, 3, generator=gen) - 0.5) * 0.004
        near = torch.cdist(pos.double(), pos.double()).topk(7, largest=False).indices[:, 1:]
        src, dst = near.reshape(-1), torch.arange(300).repeat_interleave(6)
        order = torch.argsort(src * 300 + dst)
        return pos, torch.stack([src[order], dst[order]]).contiguous()

    def trajectories(pos0, ei, n_traj, T, gen):
        out = []
        for k in range(n_traj):
            N = pos0.shape[0]
            pos = pos0[None] + torch.cumsum(torch.randn(T, N, 3, generator=gen) * 2e-3, 0)
            vel = torch.zeros_like(pos)
            vel[1:] = pos[1:] - pos[:-1]
            g = (N // 2 + 7 * k) % N
            nt = torch.zeros(T, N, 1)
            nt[:, g] = 1
            out.append({"pos": pos.to(dev), "velocity": vel.to(dev), "node_type": nt.to(dev), "actions": (torch.randn(T, 3, generator=gen) * 2e-3).to(dev),
                        "edge_index": ei.to(dev), "grasped_particle": g})
        return out

    def sample_by_hand(tr, t, H, F):
        P, V, A, g, ei = tr["pos"], tr["velocity"], tr["actions"], tr["grasped_particle"], tr["edge_index"]
        vel = torch.cat([V[t - H + h] for h in range(H)], 1)
        vel[g, 3 * (H - 1):] = V[t, g]
        pos = P[t - 1].clone()
        pos[g] += A[t - 1]
        pa = torch.zeros(P.shape[1], F, 3, device=dev)
        pa[g] = A[t - 1:t - 1 + F]
        return vel, tr["node_type"][t - 1], ei, ro.edge_features(pos, ei), V[t:t + F].transpose(0, 1).contiguous(), pa, pos

    say("device", torch.cuda.get_device_name(0))
    say("measurement", dict(window_s=a.window, rounds=a.rounds, figure="median of the rounds", history=2, message_passing_steps=a.mp_steps))
    say("assembling one batch, and one train_step on it, ms per call; share = assembling / train_step")
    say("N | E | B | F | batch | composed a | composed b | composed spread | batch / composed | train_step | share batch | share composed | "
        "rounds (batch; composed a; composed b; train_step)")
    before = sum(native.FALLBACK_COUNTS.values())
    H, gen = 2, torch.Generator().manual_seed(8)
    torch.manual_seed(0)
    sim = ClothMeshSimulator(3, 8, 4, 128, a.mp_steps, 2, 128, 2, 2, normalize=True, device=dev).train()
    opt = torch.optim.Adam(sim.parameters(), lr=1e-4)
    small, large = small_cloth(gen), cloth_graph(10_000, 30, gen)
    verdicts = []
    for (pos0, ei), n_traj, T, Bs in ((small, 8, 12, (1, 32)), (large, 2, 8, (1,))):
        trajs = trajectories(pos0, ei, n_traj, T, gen)
        ds = SamplesClothSimDataset(None, H, types.SimpleNamespace(action_steps=1, future_sequence_length=1))
        for tr in trajs:
            ds.add_trajectory(tr, symmetric=False)
        N, E = int(pos0.shape[0]), int(ei.shape[1])
        for B in Bs:
            for F in (1, 2, 3):
                ds.set_future_sequence_length(F)
                idx = torch.randperm(len(ds), generator=gen)[:B].numpy()
                j, t = ds.locate(idx)
                where = [(int(x), int(y)) for x, y in zip(j, t)]

                def fused():
                    return ds.batch(idx)

                def composed():
                    return ts.collate([sample_by_hand(trajs[x], y, H, F) for x, y in where])

                got, want = fused(), composed()          # the two assemble the same batch
                assert all(torch.equal(x, y) for x, y in zip(got[:7], want)), (N, B, F)

                def step():
                    return ts.train_step(sim, opt, got, future_sequence_length=F, noise_std=3e-4)

                runs, calls = measure({"batch": fused, "composed a": composed, "composed b": composed}, a.window, a.rounds)
                step_runs, step_calls = measure({"step": step}, a.window, a.rounds, max_calls=200)
                med = {k: statistics.median(v) for k, v in runs.items()}
                train = statistics.median(step_runs["step"])
                spread, best = abs(med["composed a"] - med["composed b"]), min(med["composed a"], med["composed b"])
                say(f"{N} | {E} | {B} | {F} | {med['batch']:.4f} | {med['composed a']:.4f} | {med['composed b']:.4f} | {spread:.4f} | "
                    f"{med['batch'] / best:.3f} | {train:.3f} | {100 * med['batch'] / train:.2f} % | {100 * best / train:.2f} % | "
                    f"{runs['batch']}; {runs['composed a']}; {runs['composed b']}; {step_runs['step']} "
                    f"({calls['batch']}; {calls['composed a']}; {calls['composed b']}; {step_calls['step']} calls per window)")
                ahead = med["batch"] < best - spread
                verdicts.append((N, B, F, ahead))
                say(f"  verdict at N = {N}, B = {B}, F = {F}: the one-launch batch is " + ("AHEAD of" if ahead else "NOT ahead of") +
                    " the composed path beyond its run-to-run spread")
    assert sum(native.FALLBACK_COUNTS.values()) == before, "a form took a composed-torch branch"
    behind = [v[:3] for v in verdicts if not v[3]]
    say("rows in which the one-launch batch is not ahead (N, B, F):", behind if behind else "none")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
