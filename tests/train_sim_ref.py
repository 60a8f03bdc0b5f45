"""Restatement of the MeshNet training transition (include/csplat.h, "MeshNet training transition") in plain torch, written from the
formulas there: forward and backward, in float64 or float32.  forward() runs where its inputs live (CPU tensors in the kernel tests; the
end-to-end test differentiates it on the device of its network), backward() on the CPU.  In float32 every line below is one rounded
operation per element (eager torch does not contract), so forward() gives the bits csplat_train_update_fwd must give for hist and
new_pos.  The backward is the
stated gather written as two index_add_ calls, NOT torch's autograd of the forward: tests/test_train_sim_cpu.py holds the two against
each other and against finite differences."""
import torch

F64, F32 = torch.float64, torch.float32
ACTION_CASES = ("all zero", "grasped, three components", "grasped, one component exactly 0", "old non-zero where the next is zero",
                "next non-zero where the old is zero")
WORKGROUP = 256      # TRAIN_SIM_THREADS of csrc/csplat_train_sim.hip (tests/test_train_sim_cpu.py reads it from the source)


def _c(t, dtype):
    return None if t is None else t.detach().cpu().to(dtype)


def _k(t, dtype):
    """the dtype alone: the device and torch's autograd are kept (the hand-written loops of the tests differentiate forward(), on the
    device of their network)"""
    return None if t is None else t.to(dtype)


def forward(velocity, noise, pred_acc, init_position, old_actions, actions, ei, H, dtype, omean=None, ostd=None):
    """-> (hist [N,3H], edge_feat [E,4], new_pos [N,3]) in `dtype`"""
    vel, noise, pa, p0, old, act, omean, ostd = (_k(t, dtype) for t in (velocity, noise, pred_acc, init_position, old_actions, actions, omean, ostd))
    ei = ei.detach().to(vel.device)
    vn = vel if noise is None else vel + noise
    if ostd is not None:
        pa = pa * ostd.reshape(1, 3)
        pa = pa + omean.reshape(1, 3)
    last = vn[:, 3 * (H - 1):3 * H]
    nv = torch.where(old != 0, old, last + pa)
    moved = torch.where(act == 0, p0 + nv, p0)
    new_pos = moved + act
    hist = torch.cat([vn[:, 3:3 * H], torch.where(act != 0, act, last)], 1)
    d = new_pos[ei[0]] - new_pos[ei[1]]
    length = torch.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])
    return hist, torch.cat([d, length[:, None]], 1), new_pos


def backward(edge_feat, g_edge, g_pos, old_actions, actions, ei, dtype, ostd=None):
    """-> (g_pred_acc, g_init_position) [N,3] in `dtype`; edge_feat as forward() left it in `dtype`; g_edge [E,4] or None, g_pos [N,3] or None"""
    ef, g_edge, g_pos, old, act, ostd = (_c(t, dtype) for t in (edge_feat, g_edge, g_pos, old_actions, actions, ostd))
    ei = ei.detach().cpu()
    gp = torch.zeros(act.shape, dtype=dtype) if g_pos is None else g_pos.clone()
    if g_edge is not None and ef.shape[0]:
        d, length = ef[:, :3], ef[:, 3:]
        k = torch.where(length > 0, g_edge[:, 3:] / torch.where(length > 0, length, torch.ones_like(length)), torch.zeros_like(length))
        term = g_edge[:, :3] + k * d
        gp.index_add_(0, ei[0], term)
        gp.index_add_(0, ei[1], -term)
    free = (act == 0) & (old == 0)
    g_pred = torch.where(free, gp if ostd is None else gp * ostd.reshape(1, 3), torch.zeros_like(gp))
    return g_pred, gp


def _gen(seed):
    return torch.Generator().manual_seed(int(seed))


def actions_case(N, kind, seed=0):
    """(old_actions, actions) [N,3] float32 for one of ACTION_CASES; the grasped node is N // 3"""
    g = _gen(4100 + seed)
    old, act = torch.zeros(N, 3), torch.zeros(N, 3)
    n = N // 3
    a, b = torch.randn(3, generator=g) * 0.01 + 0.02, torch.randn(3, generator=g) * 0.01 + 0.02      # (no component is 0)
    if kind == "all zero":
        pass
    elif kind == "grasped, three components":
        old[n], act[n] = a, b
    elif kind == "grasped, one component exactly 0":
        old[n], act[n] = a, b
        old[n, 1] = 0.0
        act[n, 1] = 0.0
        if N > 1:           # and a second node whose zero component differs between the two steps
            m = (n + 1) % N
            old[m], act[m] = b, a
            old[m, 0] = 0.0
            act[m, 2] = 0.0
    elif kind == "old non-zero where the next is zero":
        old[n] = a
    elif kind == "next non-zero where the old is zero":
        act[n] = b
    else:
        raise ValueError(kind)
    return old, act


def inputs(N, H, kind="grasped, one component exactly 0", with_noise=True, fold=False, seed=0):
    """float32 CPU inputs of one transition on N nodes: a cloth-like cloud, velocities of 1e-2, accelerations of 1e-3"""
    g = _gen(4000 + 7 * N + H + seed)
    old, act = actions_case(N, kind, seed)
    d = dict(velocity=torch.randn(N, 3 * H, generator=g) * 0.01, noise=torch.randn(N, 3 * H, generator=g) * 1e-3 if with_noise else None,
             pred_acc=torch.randn(N, 3, generator=g) * (1.0 if fold else 1e-3), init_position=torch.rand(N, 3, generator=g) - 0.5,
             old_actions=old, actions=act, omean=None, ostd=None)
    if fold:
        d["omean"], d["ostd"] = torch.randn(3, generator=g) * 1e-4, torch.rand(3, generator=g) * 1e-3 + 5e-4
    return d


def random_graph(N, E, seed=0):
    return torch.randint(0, max(N, 1), (2, E), generator=_gen(4200 + N + E + seed)).long()


def incoming(N, E, seed=0):
    """the gradients that arrive at (edge_feat, new_pos): O(1) values"""
    g = _gen(4300 + N + E + seed)
    return torch.randn(E, 4, generator=g), torch.randn(N, 3, generator=g)
