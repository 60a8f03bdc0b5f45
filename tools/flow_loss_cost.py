"""Cost of the optical-flow term (csplat.flow_loss, opt.lambda_flow), two tables:

1. the term alone at T = 3 frames, P = 100 000 Gaussians, 800 x 800 flow images: the FlowLoss node (forward + backward: three launches)
   against the torch composition of the same formulas on the same GPU tensors, device events over `--calls` calls after a warm-up;
2. the config-3 train step (3 cameras 800 x 800, P = 100 000, synthetic scene_1, eager) with the term off and on in THIS tree, and the
   plain step of a checkout of the parent commit (`--parent DIR`, built), each form in a process of its own, the forms alternating,
   `--rounds` processes per form and `--repeats` timed runs of `--steps` steps per process.

The spread of the parent's runs (largest - smallest ms per step over all its runs) is the run-to-run noise of this measurement; the
one condition the tool checks is that the best run with the term OFF is not slower than the parent's best run by more than that spread
(exit status 1 otherwise).  Without --parent only this tree is measured and nothing is checked."""
import argparse
import json
import os
import subprocess
import sys
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _paths(tree):
    for p in (os.path.join(tree, "cloth-splatting_amd"), tree):
        if p not in sys.path:
            sys.path.insert(0, p)


def _events(fn, calls, warmup):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ev0.record()
    for _ in range(calls):
        fn()
    ev1.record()
    torch.cuda.synchronize()
    return ev0.elapsed_time(ev1) / calls


def term_alone(a):
    """table 1: us per forward + backward of the node and of the composition"""
    _paths(ROOT)
    import torch
    from csplat import flow_loss as fl, native
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(1)
    T, P, S = 3, a.P, a.size
    x0 = torch.cat([2.0 * torch.rand(P, 2, device=dev, generator=gen) - 1.0, 2.0 + 2.0 * torch.rand(P, 1, device=dev, generator=gen)], 1)
    X = [(x0 + 0.02 * t * torch.randn(P, 3, device=dev, generator=gen)).requires_grad_() for t in range(T)]
    full = torch.zeros(4, 4, device=dev)
    full[0, 0] = full[1, 1] = 2.0
    full[2, 2], full[2, 3], full[3, 2] = 1.0001, 1.0, -0.010001
    flows = [3.0 * torch.randn(2, S, S, device=dev, generator=gen) for _ in range(T - 1)]
    vis = [torch.randint(0, 6, (P,), device=dev, generator=gen).to(torch.int32) for _ in range(T)]

    def node():
        for x in X:
            x.grad = None
        total, _l, _n = fl.flow_losses(X, [full] * T, flows, (S, S), visible=vis, lambda_flow=0.1)
        total.backward()
        return total

    def composed():
        for x in X:
            x.grad = None
        lf, _c = fl._flow_composed(X, [full] * T, flows, S, S, vis, None, None)
        (0.1 * lf).backward()
        return lf

    before = sum(native.FALLBACK_COUNTS.values())
    res = dict(node_us=round(1000.0 * _events(node, a.calls, 5), 2), composed_us=round(1000.0 * _events(composed, a.calls, 5), 2))
    assert sum(native.FALLBACK_COUNTS.values()) == before, "the node's timing took the composed path"
    res["L_node"], res["L_composed"] = float(node().detach()) / 0.1, float(composed().detach())
    return res


def step_runs(a):
    """child: the step of `--tree` in form `--form`, `--repeats` runs -> one JSON line"""
    _paths(a.tree)
    import torch
    import bench_train as bt
    from csplat import train as tr
    from csplat.optim import GroupedAdam
    from gaussian_renderer import render_views
    dev = torch.device("cuda:0")
    n_times = 30
    times = [k / (n_times - 1) for k in (9, 10, 11)]
    sc, pc, sim = bt.build(P=a.P, W=a.size, H=a.size, grid=a.grid, n_times=n_times, dev=dev)
    bg = torch.ones(3, device=dev)
    with torch.no_grad():
        res = render_views(bt.cameras(sc, times, dev), pc, sim, tr.DEFAULT_PIPE, bg)
        cams = bt.cameras(sc, times, dev, [r.render.clamp(0, 1).clone() for r in res])
        pc._opacity.sub_(1.0)
    kw = {}
    if a.form != "plain":          # the cameras carry a flow image in both forms of this tree; the weight switches the term
        for cam in cams:
            cam.flow = torch.zeros(2, a.size, a.size, device=dev)
        kw = dict(lambda_flow=0.05 if a.form == "on" else 0.0)
    opt = SimpleNamespace(**vars(tr.DEFAULT_OPT), **kw)
    pc.training_setup(feature_lr=tr.DEFAULT_OPT.feature_lr)
    mopt = GroupedAdam(sim.parameters(), lr=tr.DEFAULT_OPT.meshnet_lr)
    it = [0]
    last = {}

    def step():
        it[0] += 1
        last["stats"] = tr.train_step(it[0] % 999 + 1, cams, pc, sim, mopt, opt=opt, background=bg)[2]

    runs = [round(_events(step, a.steps, a.warmup if k == 0 else 1), 4) for k in range(a.repeats)]
    row = dict(form=a.form, tree=os.path.relpath(a.tree, ROOT), step_ms=runs)
    row.update({k: float(last["stats"][k]) for k in ("flow_loss", "flow_valid") if k in last["stats"]})
    print("RESULT " + json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--P", type=int, default=100_000)
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--grid", type=int, default=100)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit")
    ap.add_argument("--tree", default=ROOT, help=argparse.SUPPRESS)
    ap.add_argument("--form", default=None, choices=["plain", "off", "on"], help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.form is not None:
        return step_runs(a)
    print("shape", dict(P=a.P, frames=3, size=a.size, calls=a.calls, steps=a.steps, repeats=a.repeats, rounds=a.rounds))
    print("term_alone", term_alone(a), flush=True)
    forms = ([("parent", os.path.abspath(a.parent), "plain")] if a.parent else []) + [("off", ROOT, "off"), ("on", ROOT, "on")]
    runs = {name: [] for name, _t, _f in forms}
    extra = {}
    for _round in range(a.rounds):
        for name, tree, form in forms:          # a fresh process per form and round, one at a time
            cmd = [sys.executable, os.path.abspath(__file__), "--tree", tree, "--form", form] + \
                  [f"--{k}={getattr(a, k)}" for k in ("P", "size", "grid", "steps", "warmup", "repeats")]
            out = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
            line = [ln for ln in out.stdout.splitlines() if ln.startswith("RESULT ")]
            if out.returncode != 0 or not line:
                print(out.stdout[-2000:], out.stderr[-2000:])
                raise SystemExit(f"the {name} step failed (exit status {out.returncode})")
            row = json.loads(line[-1][7:])
            runs[name] += row["step_ms"]
            extra[name] = {k: v for k, v in row.items() if k in ("flow_loss", "flow_valid")}
            print(name, row, flush=True)
    best = {k: min(v) for k, v in runs.items()}
    print("step_ms_best", best)
    print("step_ms_all", runs)
    print("extra_ms_on_against_off", round(best["on"] - best["off"], 4), extra.get("on", {}))
    if a.parent:
        spread = max(runs["parent"]) - min(runs["parent"])
        ok = best["off"] <= best["parent"] + spread
        print("parent_spread_ms", round(spread, 4), "off_minus_parent_ms", round(best["off"] - best["parent"], 4),
              "term off not slower than the parent beyond its spread:", ok)
        if not ok:
            raise SystemExit(1)


if __name__ == "__main__":
    main()
