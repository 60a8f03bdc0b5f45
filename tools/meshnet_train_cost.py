"""Cost of the unrolled MeshNet training step (meshnet.train_sim), written to profiles/meshnet_train_cost.txt.

One transition, forward + backward (the state update between two predictions of a training step, gradients arriving at the edge features
and the new positions and leaving at pred_acc and init_position), at N = 6400 nodes / E = 64 000 edges (the reference's 200 nodes x batch
32) and at N = 10 000 / E = 300 000 (bench_gnn.py's size), velocity history 2, the output normaliser folded in:

  kernels    meshnet.train_sim's autograd node: csplat_train_update_fwd + csplat_train_update_bwd, one launch each;
  composed   what the parent commit lets a user write: Normalizer.inverse, the masks and the history shift from torch indexing
             operations with torch's autograd behind them, the edge features from the existing csplat_gnn_edge_features
             (meshnet.rollout.edge_features) wrapped in an autograd node whose backward is torch's: a division, a multiply-add and two
             index_add_ (float scatter-adds).  The most favourable composed form: pure torch (index_select + norm) records more nodes.
             Timed TWICE per round (composed a, composed b): their difference is the run-to-run spread of this measurement.

Then, for information, the whole train_step (F predictions of a ClothMeshSimulator at latent 128 with 15 message-passing steps, the loss,
backward, Adam) at F = 1, 2, 3 at the second size.

A host clock around `calls` back-to-back calls that end in a device synchronise (the step is bound by the host: device events alone
would miss the time between launches); after a warm-up of every form; `calls` is chosen per form so that a timed window lasts about
--window seconds; the forms alternate over --rounds rounds, every round's figure is printed and the MEDIAN is the figure of a form.  A
record, not a pass condition; the tool fails without a GPU."""
import argparse
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "cloth-splatting_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)


def _timed(fn, calls):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / calls          # ms per call


def measure(forms, window, rounds, max_calls=5000):
    """forms: {name: callable} -> ({name: [ms per call, one per round]}, {name: calls}); warm-up, `calls` sized to the window, alternating"""
    calls = {}
    for name, fn in forms.items():
        for _ in range(3):
            fn()
        est = _timed(fn, 2)
        calls[name] = int(min(max(math.ceil(window * 1e3 / max(est, 1e-6)), 2), max_calls))
    runs = {name: [] for name in forms}
    for _ in range(rounds):
        for name, fn in forms.items():
            runs[name].append(round(_timed(fn, calls[name]), 4))
    return runs, calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.3, help="seconds of work per timed window")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--mp-steps", type=int, default=15)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "meshnet_train_cost.txt"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("meshnet_train_cost: no GPU; a time is only measured on one")
    from bench_gnn import cloth_graph
    from csplat import native
    from meshnet import rollout as ro, train_sim as ts
    from meshnet.cloth_network import ClothMeshSimulator
    dev = torch.device("cuda:0")
    lines = []

    def say(*parts):
        lines.append(" ".join(str(p) for p in parts))
        print(lines[-1], flush=True)

    class EdgeFeatures(torch.autograd.Function):
        """csplat_gnn_edge_features with the backward torch gives index_select + norm"""

        @staticmethod
        def forward(ctx, pos, ei):
            ef = ro.edge_features(pos, ei)
            ctx.save_for_backward(ef, ei)
            ctx.n = pos.shape[0]
            return ef

        @staticmethod
        def backward(ctx, g):
            ef, ei = ctx.saved_tensors
            length = ef[:, 3:]
            term = g[:, :3] + torch.where(length > 0, g[:, 3:] / length, torch.zeros_like(length)) * ef[:, :3]
            gp = torch.zeros(ctx.n, 3, dtype=g.dtype, device=g.device)
            gp.index_add_(0, ei[0], term)
            gp.index_add_(0, ei[1], -term)
            return gp, None

    def composed(noise, vel, pred, init, ei, old, act, H, omean, ostd):
        vn = vel if noise is None else vel + noise
        pa = pred * ostd + omean
        last = vn[:, 3 * (H - 1):]
        nv = torch.where(old != 0, old, last + pa)
        new_pos = torch.where(act == 0, init + nv, init) + act
        hist = torch.cat([vn[:, 3:], torch.where(act != 0, act, last)], 1)
        return hist, EdgeFeatures.apply(new_pos, ei), new_pos

    say("device", torch.cuda.get_device_name(0))
    say("measurement", dict(window_s=a.window, rounds=a.rounds, figure="median of the rounds", history=2, normaliser="folded"))
    before = sum(native.FALLBACK_COUNTS.values())
    say("one transition forward + backward, ms per call")
    say("N | E | kernels | composed a | composed b | composed spread | kernels / composed | rounds (kernels; composed a; composed b)")
    H, sizes, state = 2, ((6400, 10), (10_000, 30)), {}
    for N, deg in sizes:
        gen = torch.Generator().manual_seed(3)
        pos0, ei_cpu = cloth_graph(N, deg, gen)
        ei, E = ei_cpu.to(dev), int(ei_cpu.shape[1])
        vel = (torch.randn(N, 3 * H, generator=gen) * 0.01).to(dev)
        old, act = torch.zeros(N, 3), torch.zeros(N, 3)
        grasped = torch.arange(0, N, 200)                         # one grasped node per 200 (a batch of 200-node samples)
        old[grasped], act[grasped] = torch.randn(len(grasped), 3, generator=gen) * 0.005, torch.randn(len(grasped), 3, generator=gen) * 0.005
        old, act, pos0 = old.to(dev), act.to(dev), pos0.to(dev)
        pred = torch.randn(N, 3, generator=gen).to(dev).requires_grad_()
        init = pos0.clone().requires_grad_()
        omean, ostd = (torch.randn(3, generator=gen) * 1e-4).to(dev), (torch.rand(3, generator=gen) * 1e-3 + 5e-4).to(dev)
        g_ef, g_pos = torch.randn(E, 4, generator=gen).to(dev), torch.randn(N, 3, generator=gen).to(dev)

        def run(fn):
            _h, ef, new_pos = fn()
            return torch.autograd.grad((ef, new_pos), (pred, init), (g_ef, g_pos))

        def kernels():
            return run(lambda: ts._transition(None, vel, pred, init, ei, old, act, H, omean, ostd, "meshnet_train_cost"))

        def composed_form():
            return run(lambda: composed(None, vel, pred, init, ei, old, act, H, omean, ostd))

        # the two compute the same gradients
        gk, gc = kernels(), composed_form()
        for x, y in zip(gk, gc):
            d = float((x - y).abs().max() / y.abs().max())
            assert d < 1e-4, (N, d)
        runs, calls = measure({"kernels": kernels, "composed a": composed_form, "composed b": composed_form}, a.window, a.rounds)
        med = {k: statistics.median(v) for k, v in runs.items()}
        spread = abs(med["composed a"] - med["composed b"])
        best = min(med["composed a"], med["composed b"])
        say(f"{N} | {E} | {med['kernels']:.4f} | {med['composed a']:.4f} | {med['composed b']:.4f} | {spread:.4f} | "
            f"{med['kernels'] / best:.2f} | {runs['kernels']}; {runs['composed a']}; {runs['composed b']} "
            f"({calls['kernels']}; {calls['composed a']}; {calls['composed b']} calls per window)")
        say(f"  verdict at N = {N}: the kernels are " + ("NOT slower" if med["kernels"] <= best + spread else "SLOWER") +
            " than the composed path beyond its run-to-run spread")
        state[N] = (ei, pos0, vel, act)

    # ---- the whole train step, for information
    N = sizes[-1][0]
    ei, pos0, vel, act1 = state[N]
    gen = torch.Generator().manual_seed(4)
    torch.manual_seed(0)
    sim = ClothMeshSimulator(3, 8, 4, 128, a.mp_steps, 2, 128, 2, 2, normalize=True, device=dev).train()
    opt = torch.optim.Adam(sim.parameters(), lr=1e-4)
    ntype = (act1.abs().sum(1, keepdim=True) > 0).float()
    S = 3
    actions = act1[:, None, :].repeat(1, S, 1).contiguous()
    targets = (torch.randn(N, S, 3, generator=gen) * 0.01).to(dev)
    batch = (vel, ntype, ei, ro.edge_features(pos0, ei), targets, actions, pos0)
    say(f"train_step (N = {N}, E = {int(ei.shape[1])}, latent 128, {a.mp_steps} message-passing steps, Adam), ms per call")
    say("F | train_step | rounds")
    for F in (1, 2, 3):
        runs, calls = measure({"step": lambda: ts.train_step(sim, opt, batch, future_sequence_length=F, noise_std=3e-4)}, a.window, a.rounds, max_calls=200)
        say(f"{F} | {statistics.median(runs['step']):.3f} | {runs['step']} ({calls['step']} calls per window)")
    assert sum(native.FALLBACK_COUNTS.values()) == before, "a form took a composed-torch branch"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
