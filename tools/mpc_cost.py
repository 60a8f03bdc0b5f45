"""Cost of planning with batched candidates (meshnet.mpc), written to profiles/mpc_cost.txt.

Workload: one cloth of N = 300 nodes with about 6 directed edges per node, velocity history 2, a ClothMeshSimulator at latent 128 with 15
message-passing steps, horizon H = 6.  For B in {1, 16, 100, 256, 1024} candidates:

  batch   one meshnet.mpc.rollout_candidates call with a goal (B candidates as one block-diagonal graph; per step: edge features,
          predict_velocity on B * N nodes, csplat_plan_integrate with the cost term), the block-diagonal graph built once outside the
          timed window as a planner does;
  loop    the same B candidates as a Python loop over meshnet.rollout.rollout (one call per candidate, graph replay on, as a planner
          written against rollout() would run) -- the baseline.

Milliseconds per call (all B candidates) and candidates per second for both, and their ratio.  Also the planning kernels alone at B = 100
and 1024 (csplat_plan_cost, csplat_plan_select with K = 10, csplat_plan_refit_sample), microseconds per call.

A host clock around `calls` back-to-back calls that end in a device synchronise (both forms contain a host read of their overflow word
per rollout, so device events alone would miss host time between launches); after a warm-up of every shape; `calls` is chosen per form so
that a timed window lasts about --window seconds; the forms alternate over --rounds rounds and every round's figure is printed (their
spread is the noise of this measurement).  A record, not a pass condition; the tool fails without a GPU."""
import argparse
import math
import os
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


def measure(forms, window, rounds, max_calls=2000):
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
    ap.add_argument("--nodes", type=int, default=300)
    ap.add_argument("--degree", type=int, default=6, help="directed edges per node")
    ap.add_argument("--horizon", type=int, default=6)
    ap.add_argument("--mp-steps", type=int, default=15)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 16, 100, 256, 1024])
    ap.add_argument("--loop-cap", type=int, default=1024, help="largest B the per-candidate loop is timed at")
    ap.add_argument("--window", type=float, default=0.5, help="seconds of work per timed window")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mpc_cost.txt"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("mpc_cost: no GPU; a time is only measured on one")
    from csplat import native
    from meshnet import mpc, rollout as ro
    from meshnet.cloth_network import ClothMeshSimulator
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(1)
    lines = []

    def say(*parts):
        lines.append(" ".join(str(p) for p in parts))
        print(lines[-1], flush=True)

    N, E, H = a.nodes, a.nodes * a.degree, a.horizon
    say("device", torch.cuda.get_device_name(0))
    say("shape", dict(nodes=N, edges=E, history=2, latent=128, message_passing_steps=a.mp_steps, horizon=H, window_s=a.window, rounds=a.rounds))
    torch.manual_seed(0)
    sim = ClothMeshSimulator(3, 8, 4, 128, a.mp_steps, 2, 128, 2, 2, normalize=False, device=dev).eval()
    pos = torch.randn(N, 3, generator=gen).to(dev)
    ei = torch.stack([torch.randint(0, N, (E,), generator=gen), torch.randint(0, N, (E,), generator=gen)]).to(dev)
    hist = (0.01 * torch.randn(2, N, 3, generator=gen)).to(dev)
    ntype = torch.randint(0, 2, (N, 1), generator=gen).to(dev)
    goal = (pos.cpu() + 0.05 * torch.randn(N, 3, generator=gen)).to(dev)
    grasped = 7
    before = sum(native.FALLBACK_COUNTS.values())
    say("B | batch ms per call | batch candidates/s | loop ms per B candidates | loop candidates/s | loop / batch | rounds (batch; loop)")
    for B in a.batches:
        actions = (0.01 * torch.randn(B, H, 3, generator=gen)).to(dev)
        batch = mpc.batch_candidates(pos, hist, ntype, ei, B)

        def batched():
            return mpc.rollout_candidates(sim, pos, hist, ntype, ei, actions, grasped, H, goal=goal, batch=batch)

        def looped():
            out = None
            for b in range(B):
                out = ro.rollout(sim, pos, hist, ntype, ei, actions[b], grasped, H)
            return out

        forms = {"batch": batched}
        if B <= a.loop_cap:
            forms["loop"] = looped
        runs, calls = measure(forms, a.window, a.rounds)
        # the two compute the same plan: every candidate's final state, batch against loop, at the first and the last candidate
        r = batched()
        for b in sorted({0, B - 1}):
            _p, pe = ro.rollout(sim, pos, hist, ntype, ei, actions[b], grasped, H)
            d = float((r.final_positions[b] - pe).abs().max() / pe.abs().max())
            assert d < 1e-4, (B, b, d)
        tb = min(runs["batch"])
        if "loop" in runs:
            tl = min(runs["loop"])
            say(f"{B} | {tb:.3f} | {B / tb * 1e3:.0f} | {tl:.3f} | {B / tl * 1e3:.0f} | {tl / tb:.2f} | {runs['batch']}; {runs['loop']} "
                f"({calls['batch']}; {calls['loop']} calls per window)")
        else:
            say(f"{B} | {tb:.3f} | {B / tb * 1e3:.0f} | not measured | not measured | not measured | {runs['batch']} ({calls['batch']} calls per window)")
    assert sum(native.FALLBACK_COUNTS.values()) == before, "a form took a composed-torch branch"

    # ---- the planning kernels alone
    say("kernel | B | us per call (best) | rounds")
    stream = native.stream_handle(dev)
    for B in (100, 1024):
        fp = torch.randn(B, N, 3, generator=gen).to(dev)
        cost = torch.empty(B, device=dev)
        order, best = torch.empty(10, dtype=torch.int32, device=dev), torch.empty(10, device=dev)
        acts, noise = (0.01 * torch.randn(B, H, 3, generator=gen)).to(dev), torch.randn(B, H, 3, generator=gen).to(dev)
        mu, sg = torch.zeros(H, 3, device=dev), torch.full((H, 3), 0.01, device=dev)
        forms = {
            "csplat_plan_cost": lambda: native.check(native.lib.csplat_plan_cost(stream, B, N, fp.data_ptr(), goal.data_ptr(), None, 1.0, 0,
                                                                                 cost.data_ptr()), "csplat_plan_cost"),
            "csplat_plan_select K=10": lambda: native.check(native.lib.csplat_plan_select(stream, B, 10, cost.data_ptr(), order.data_ptr(),
                                                                                          best.data_ptr()), "csplat_plan_select"),
            "csplat_plan_refit_sample K=10": lambda: native.check(native.lib.csplat_plan_refit_sample(
                stream, B, H, 10, acts.data_ptr(), order.data_ptr(), mu.data_ptr(), sg.data_ptr(), noise.data_ptr(), 0.1, 1e-4, 0.05),
                "csplat_plan_refit_sample"),
        }
        runs, calls = measure(forms, min(a.window, 0.2), a.rounds, max_calls=20_000)
        for name in forms:
            say(f"{name} | {B} | {min(runs[name]) * 1e3:.2f} | {[round(x * 1e3, 2) for x in runs[name]]} ({calls[name]} calls per window)")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
