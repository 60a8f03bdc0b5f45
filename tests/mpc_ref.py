"""Plain torch restatement, on the CPU, of what the planning kernels of csrc/csplat_plan.hip compute (include/csplat.h, "Planning"):
integrate (the batched rollout step's tail with the step's cost term), cost (the same term on stored positions), select (the stable sort's
first K) and refit_sample (one cross-entropy-method update), for tests/test_mpc_cpu.py (which checks THIS file against closed forms and
numpy) and tests/test_mpc_gpu.py (which checks the kernels against this file in float64 and derives its bars from this file in float32).
Written from the formulas of the header; nothing is imported from csplat or meshnet.  Every function takes the dtype it computes in.

Also here, because both test files need them: the SIZE TABLES and the case builders of the GPU file (a test without a GPU checks that
every size lies beyond the launch constant it is meant to cross)."""
import torch

F64, F32 = torch.float64, torch.float32
NAN, INF = float("nan"), float("inf")

# the launch constants of csrc/csplat_plan.hip (tests/test_mpc_cpu.py asserts them against the source's literals)
PL_THREADS, PL_SEL_TILE, PL_BATCH = 256, 1024, 8


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# ------------------------------------------------------------------------------------------------ the four functions
def cost(pos, goal, node_w=None, dtype=F64):
    """[B]: (1 / 3N) sum_{n,c} node_w[n] (pos[b][n][c] - goal[n][c])^2; pos [B,N,3], goal [N,3], node_w [N] or None (ones)"""
    d = pos.to(dtype) - goal.to(dtype)[None]
    t = d * d
    if node_w is not None:
        t = node_w.to(dtype).reshape(1, -1, 1) * t
    return t.sum(dim=(1, 2)) / (3 * pos.shape[1])


def integrate(B, N, k, v, actions, grasped, pos, hist, preds=None, goal=None, node_w=None, step_w=None, cost_in=None, dtype=F64):
    """One step's tail for all candidates.  v [B*N,3], actions [B,T,3], pos [B*N,3], hist [H,B*N,3], preds [steps,B*N,3] or None, goal [N,3]
    or None, cost_in [B].  Nothing is modified -> dict(v, pos, hist, preds, cost) of new tensors.  A grasped index outside [0, N) pins
    nothing.  step_w None: the weight is 1 at k == T-1 and 0 before it, and an earlier step leaves the cost as it is."""
    T = actions.shape[1]
    v = v.to(dtype).clone().reshape(B, N, 3)
    if 0 <= grasped < N:
        v[:, grasped] = actions.to(dtype)[:, k]
    v = v.reshape(B * N, 3)
    pos = pos.to(dtype) + v
    hist = torch.cat([hist.to(dtype)[1:], v[None]], 0)
    out = dict(v=v, pos=pos, hist=hist, preds=None, cost=None if cost_in is None else cost_in.to(dtype).clone())
    if preds is not None:
        out["preds"] = preds.to(dtype).clone()
        out["preds"][k] = v
    if goal is not None and (step_w is not None or k == T - 1):
        term = cost(pos.reshape(B, N, 3), goal, node_w, dtype)
        out["cost"] = out["cost"] + (term if step_w is None else step_w.to(dtype)[k] * term)
    return out


def select(costs, K):
    """(order [K] int64, best [K]): torch.sort(stable=True) truncated to K -- numbers ascending with -0.0 == 0.0, +inf before NaN, NaN
    last, equal costs by ascending index"""
    val, idx = torch.sort(costs, stable=True)
    return idx[:K], val[:K]


def refit_sample(actions, order, mu, sigma, noise, alpha, sigma_min, a_max, dtype=F64):
    """One cross-entropy-method update.  actions [B,T,3], order [K] (K may be 0: no refit), mu / sigma [T,3], noise [B,T,3].  Nothing is
    modified -> (actions, mu, sigma) of new tensors.  Elite sums in the order r = 0 .. K-1"""
    a, mu, sigma, noise = (t.to(dtype) for t in (actions, mu, sigma, noise))
    K = int(order.shape[0])
    if K > 0:
        el = a[order.long()]
        m = torch.zeros_like(mu)
        for r in range(K):
            m = m + el[r]
        m = m / K
        s = torch.zeros_like(mu)
        for r in range(K):
            s = s + (el[r] - m) * (el[r] - m)
        s = (s / K).sqrt()
        mu = alpha * mu + (1 - alpha) * m
        sigma = torch.clamp(alpha * sigma + (1 - alpha) * s, min=sigma_min)
    new = mu[None] + sigma[None] * noise
    new[0] = mu
    if a_max > 0:
        new = torch.clamp(new, -a_max, a_max)
    return new, mu, sigma


# ------------------------------------------------------------------------------------------------ size tables and case builders
# integrate / cost: (B, N, H).  N around one workgroup's threads (a candidate's 3N elements are walked PL_THREADS at a time: 3N below,
# at and above it, and many rounds), B = 1, 2 and more than a wave of workgroups, H = 1 (no shift), 2, 3; each value with the extremes
# of the others
INTEGRATE_SIZES = [(1, 1, 1), (65, 1, 3), (1, 1000, 3), (65, 1000, 1), (2, 255, 2), (2, 256, 1), (1, 257, 3), (65, 257, 2), (2, 1000, 2),
                   (65, 255, 1), (1, 256, 2), (2, 1, 3), (1, 85, 1), (2, 86, 2)]
INTEGRATE_T = 3
# select: B around the wave, the workgroup and the LDS tile; K = 1, min(B, 10), B
SELECT_B = [1, 2, 63, 64, 65, 255, 256, 257, 1000, 4099]
# refit_sample: (T, B), each with K in (1, min(10, B), B)
REFIT_SIZES = [(1, 2), (1, 257), (6, 2), (6, 100), (6, 257), (33, 2), (33, 100), (33, 257), (1, 100)]
REFIT_ALPHAS = [0.0, 0.1, 1.0]


def select_ks(B):
    return sorted({1, min(B, 10), B})


def integrate_case(B, N, H, T=INTEGRATE_T, seed=0):
    """float32 CPU inputs of T consecutive csplat_plan_integrate calls: positions O(1), velocities and actions O(0.01), node weights with
    zeros, non-trivial step weights"""
    g = _gen(1000003 * seed + 7919 * B + 31 * N + H)
    c = dict(B=B, N=N, H=H, T=T)
    c["pos"] = torch.randn(B * N, 3, generator=g)
    c["hist"] = 0.01 * torch.randn(H, B * N, 3, generator=g)
    c["v"] = [0.01 * torch.randn(B * N, 3, generator=g) for _ in range(T)]          # the network's output of each step
    c["actions"] = 0.01 * torch.randn(B, T, 3, generator=g)
    c["goal"] = torch.randn(N, 3, generator=g)
    w = torch.rand(N, generator=g) + 0.5
    w[::3] = 0.0
    c["node_w"] = w
    c["step_w"] = torch.tensor([0.25, 0.0, 1.5])[:T].clone()
    return c


def select_case(B, seed=0):
    """[B] float32 costs from 7 levels (many duplicates) with NaN, +inf, -inf, 0.0 and -0.0 spread in"""
    g = _gen(77 * seed + B)
    levels = torch.tensor([-2.5, -1.0, 0.5, 0.75, 1.0, 3.0, 1e30])
    c = levels[torch.randint(0, 7, (B,), generator=g)].clone()
    special = torch.tensor([NAN, INF, -INF, 0.0, -0.0, NAN, -0.0, 0.0, INF, -INF])
    where = torch.randperm(B, generator=g)[:min(B, 3 * len(special))]
    c[where] = special[torch.arange(len(where)) % len(special)]
    return c


def refit_case(T, B, K, seed=0):
    """float32 CPU inputs of one csplat_plan_refit_sample call; the elites hold row 0 and the last row (both are overwritten by the same
    call: the read-before-overwrite hazard)"""
    g = _gen(5003 * seed + 101 * T + 7 * B + K)
    c = dict(T=T, B=B, K=K)
    c["actions"] = 0.05 * torch.randn(B, T, 3, generator=g)
    c["mu"] = 0.02 * torch.randn(T, 3, generator=g)
    c["sigma"] = 0.01 + 0.02 * torch.rand(T, 3, generator=g)
    c["noise"] = torch.randn(B, T, 3, generator=g)
    perm = torch.randperm(B, generator=g)
    rest = perm[(perm != 0) & (perm != B - 1)]
    head = torch.tensor([B - 1, 0]) if (K >= 2 and B >= 2) else torch.tensor([B - 1])
    c["order"] = torch.cat([head, rest])[:K].to(torch.int32)
    return c
