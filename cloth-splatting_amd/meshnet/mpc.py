"""Model-predictive planning with the MeshNet simulator: candidate action sequences rolled out AS ONE BATCH, a goal cost, selection and a
cross-entropy-method (CEM) refinement, all on the device.

The reference's planner (its manipulation/planning.py:289-311) builds `MPC(meshnet, A=A, H=H, input_sequence_length=...)`,
rolls the model out for A candidate action sequences over a horizon H (`mpc.model_rollout`) and picks the cheapest with
`mpc.compute_cost(model_rollouts, goal_particles) -> (best_action_idx, best_actions, cost_action)`; the cost is
`(pos - goal).pow(2).mean()` (:425) and the candidates form one block-diagonal graph (`get_batch_with_candidate_actions`,
meshnet/dataloader_sim.py:248-288 there, `Batch.from_data_list`).  Its `MPC` class itself (`manipulation.planner.mpc`) is not
shipped: the interface here is shaped after those call sites.

Layout (PyG's `Batch`): node n of candidate b is row b * N + n; positions [B*N,3], history [H,B*N,3] (oldest first), actions [B,T,3], the
goal [N,3] is shared by all candidates.  A cloth of 300 nodes cannot fill the chip (one `meshnet.rollout.rollout` call per candidate is
~35 launches on a graph smaller than one XCD's worth of work); a hundred candidates in one graph are 30 000 nodes and ~200 000 edges, the size the
fused inference kernels were built for.  Per step: `rollout.edge_features` on the batched positions, `simulator.predict_velocity` on the
batched graph (latent 128 under no_grad: the fused inference path with N' = B * N), `csplat_plan_integrate` (pin, integrate, history
shift, the step's cost term).  The time loop itself is sequential.

Out of scope: recording the batched step into a hipGraph, `real_world=True` (the edge-length refinement) for candidates, multi-GPU
sharding of candidates, the reference's action sampler (`init_sampler`, `get_action_traj`: not shipped)."""
import collections

import torch

from csplat import native as _n

from .rollout import edge_features

CandidateBatch = collections.namedtuple("CandidateBatch", ["pos", "hist", "node_type", "edge_index", "batch", "B", "N"])
CandidateBatch.__doc__ = """the block-diagonal tensors of B copies of one graph: pos [B*N,3], hist [H,B*N,3], node_type [B*N,1],
edge_index [2,B*E] (candidate b's copy has b * N added), batch [B*N] (the candidate of a row).  Holding this object keeps the batched
edge_index alive, and with it the CSR orderings GraphCSR.get caches for it."""

_CandidateRollouts = collections.namedtuple("CandidateRollouts", ["final_positions", "costs", "predictions", "actions"])


class CandidateRollouts(_CandidateRollouts):
    """final_positions [B,N,3]; costs [B] or None (no goal was given); predictions [nsteps,B,N,3] or None (not asked for); actions
    [B,nsteps,3]: the candidate actions that were rolled (what `MPC.compute_cost` returns the best row of)"""
    __slots__ = ()

    def __new__(cls, final_positions, costs=None, predictions=None, actions=None):
        return super().__new__(cls, final_positions, costs, predictions, actions)


def batch_candidates(positions, velocity_history, node_type, edge_index, B):
    """B copies of one graph as one block-diagonal graph (stock torch ops: once per plan, not per step) -> CandidateBatch"""
    B = int(B)
    if B < 1:
        raise ValueError("batch_candidates: B must be >= 1")
    if positions.dim() != 2 or velocity_history.dim() != 3 or velocity_history.shape[1] != positions.shape[0] or \
            edge_index.dim() != 2 or edge_index.shape[0] != 2:
        raise ValueError("batch_candidates: positions [N,D], velocity_history [H,N,D], edge_index [2,E]")
    N, E = int(positions.shape[0]), int(edge_index.shape[1])
    if node_type.numel() != N:
        raise ValueError("batch_candidates: node_type holds one entry per node")
    pos = positions.repeat(B, 1)
    hist = velocity_history.repeat(1, B, 1)
    nt = node_type.reshape(N, 1).repeat(B, 1)
    offs = torch.arange(B, dtype=edge_index.dtype, device=edge_index.device) * N
    ei = (edge_index[:, None, :] + offs[None, :, None]).reshape(2, B * E).contiguous()
    batch = torch.arange(B, dtype=torch.int64, device=positions.device).repeat_interleave(N)
    return CandidateBatch(pos, hist, nt, ei, batch, B, N)


def _on_kernels(grasped_particle, *tensors):
    """the library path takes GPU float32 tensors and a plain int as the grasped node"""
    return isinstance(grasped_particle, int) and not isinstance(grasped_particle, bool) and \
        all(t is None or (t.is_cuda and t.dtype == torch.float32) for t in tensors)


def _cost_composed(pos_b, goal, node_weights):
    """[B]: (1 / 3N) sum_{n,c} node_w[n] (pos[b,n,c] - goal[n,c])^2 -- (pos - goal).pow(2).mean() per candidate with all-one weights"""
    d2 = (pos_b - goal[None]) ** 2
    if node_weights is not None:
        d2 = node_weights.reshape(1, -1, 1) * d2
    return d2.sum(dim=(1, 2)) / (3 * pos_b.shape[1])


def candidate_costs(final_positions, goal, node_weights=None):
    """cost [B] of stored positions [B,N,3] against goal [N,3] (csplat_plan_cost).  Bit-equal to the cost rollout_candidates accumulates
    for the same final positions under the default step weights."""
    B, N = int(final_positions.shape[0]), int(final_positions.shape[1])
    if tuple(goal.shape) != (N, 3) or (node_weights is not None and node_weights.numel() != N):
        raise ValueError("candidate_costs: goal [N,3], node_weights [N]")
    if _on_kernels(0, final_positions, goal, node_weights):
        dev = final_positions.device
        p, g = final_positions.contiguous(), goal.contiguous()
        w = None if node_weights is None else node_weights.reshape(-1).contiguous()
        cost = torch.empty(B, dtype=torch.float32, device=dev)
        _n.launch("csplat_plan_cost", dev, B, N, _n.ptr(p), _n.ptr(g), _n.ptr(w), 1.0, 0, _n.ptr(cost))
        return cost
    _n.composed_fallback("mpc.candidate_costs", "dtype", final_positions, goal)
    return _cost_composed(final_positions, goal, node_weights)


def select_candidates(costs, k=1):
    """(order [k] int32, best_costs [k]): the k cheapest candidates, cheapest first; equal costs by ascending index, NaN last -- the first k
    of torch.sort(costs, stable=True) (csplat_plan_select)"""
    B, k = int(costs.shape[0]), int(k)
    if costs.dim() != 1 or not 0 <= k <= B:
        raise ValueError("select_candidates: costs [B], 0 <= k <= B")
    if costs.is_cuda and costs.dtype == torch.float32 and B <= 65536:
        dev = costs.device
        c = costs.contiguous()
        order = torch.empty(k, dtype=torch.int32, device=dev)
        best = torch.empty(k, dtype=torch.float32, device=dev)
        _n.launch("csplat_plan_select", dev, B, k, _n.ptr(c), _n.ptr(order), _n.ptr(best))
        return order, best
    _n.composed_fallback("mpc.select_candidates", "dtype" if costs.dtype != torch.float32 else "shape", costs)
    val, idx = torch.sort(costs, stable=True)
    return idx[:k].to(torch.int32), val[:k]


def refit_sample(actions, order, mu, sigma, noise, alpha, sigma_min, a_max):
    """one CEM update IN PLACE (csplat_plan_refit_sample): mu / sigma [T,3] move towards the mean / deviation of the elite rows
    actions[order], then actions [B,T,3] <- row 0 = clamp(mu), row b = clamp(mu + sigma * noise[b])"""
    B, T = int(actions.shape[0]), int(actions.shape[1])
    K = int(order.shape[0])
    if _on_kernels(0, actions, mu, sigma, noise) and order.is_cuda and order.dtype == torch.int32 and \
            all(t.is_contiguous() for t in (actions, mu, sigma)):
        dev = actions.device
        _n.launch("csplat_plan_refit_sample", dev, B, T, K, _n.ptr(actions), _n.ptr(order.contiguous()), _n.ptr(mu), _n.ptr(sigma),
                  _n.ptr(noise.contiguous()), float(alpha), float(sigma_min), float(a_max))
        return actions, mu, sigma
    _n.composed_fallback("mpc.refit_sample", "dtype", actions, mu, sigma, noise, order)
    if K > 0:
        el = actions[order.long()]
        m = el.mean(0)
        s = ((el - m[None]) ** 2).mean(0).sqrt()
        mu.copy_(alpha * mu + (1 - alpha) * m)
        sigma.copy_(torch.clamp(alpha * sigma + (1 - alpha) * s, min=sigma_min))
    new = mu[None] + sigma[None] * noise
    new[0] = mu
    actions.copy_(torch.clamp(new, -a_max, a_max) if a_max > 0 else new)
    return actions, mu, sigma


@torch.no_grad()
def rollout_candidates(simulator, positions, velocity_history, node_type, edge_index, candidate_actions, grasped_particle, nsteps, goal=None,
                       node_weights=None, step_weights=None, return_trajectories=False, real_world=False, batch=None):
    """Roll B candidate action sequences out together.  positions [N,3], velocity_history [H,N,3], node_type [N(,1)], edge_index [2,E] of
    ONE cloth; candidate_actions [B,T,3] with T >= nsteps (only [:, :nsteps] is used): the velocity of the grasped node of candidate b at
    step k; grasped_particle: the node index inside one candidate (an int outside [0, N) pins nothing).
    goal [N,3]: also cost[b] = sum_k step_weights[k] * mean_{n,c}(node_weights[n] * (pos_k[b,n,c] - goal[n,c])^2); step_weights None = the
    final state only (planning.py:425), node_weights None = all ones.
    -> CandidateRollouts(final_positions [B,N,3], costs [B] | None, predictions [nsteps,B,N,3] | None, actions [B,nsteps,3]).
    `batch`: a CandidateBatch of the same graph and B made earlier (batch_candidates) -- a planner builds it once per plan.
    No host read apart from the one overflow word behind the loop: if a step left fp16's range the rollout runs once more from its start
    with bf16 pieces, as rollout() does."""
    from .graph_network import deferred_overflow_check
    if real_world:
        raise NotImplementedError("rollout_candidates: real_world=True (the edge-length refinement) is not implemented for candidates")
    nsteps = int(nsteps)
    if candidate_actions.dim() != 3 or candidate_actions.shape[2] != 3:
        raise ValueError("rollout_candidates: candidate_actions is [B,T,3]")
    B, N, H = int(candidate_actions.shape[0]), int(positions.shape[0]), int(velocity_history.shape[0])
    if B < 1 or nsteps < 0 or int(candidate_actions.shape[1]) < nsteps:
        raise ValueError("rollout_candidates: needs B >= 1 candidates and at least nsteps actions per candidate")
    if positions.dim() != 2 or positions.shape[1] != 3 or tuple(velocity_history.shape[1:]) != (N, 3):
        raise ValueError("rollout_candidates: positions [N,3], velocity_history [H,N,3]")
    if goal is not None and tuple(goal.shape) != (N, 3):
        raise ValueError("rollout_candidates: goal is [N,3]")
    if node_weights is not None and node_weights.numel() != N:
        raise ValueError("rollout_candidates: node_weights is [N]")
    if step_weights is not None and int(step_weights.numel()) < nsteps:
        raise ValueError("rollout_candidates: step_weights holds at least nsteps entries")
    if batch is None:
        batch = batch_candidates(positions, velocity_history, node_type, edge_index, B)
    elif batch.B != B or batch.N != N or tuple(batch.hist.shape) != (H, B * N, 3):
        raise ValueError("rollout_candidates: `batch` was made for another B, N or history length")
    dev, dt = positions.device, positions.dtype
    acts = candidate_actions[:, :nsteps].contiguous()          # (only what is used: ADVICE.md, second item)
    node_w = None if node_weights is None else node_weights.reshape(-1).contiguous()
    step_w = None if step_weights is None else step_weights.reshape(-1)[:nsteps].contiguous()
    kernels = _on_kernels(grasped_particle, positions, velocity_history, candidate_actions, goal, node_w, step_w) and \
        edge_index.dtype == torch.int64
    if not kernels:
        _n.composed_fallback("mpc.rollout_candidates", "dtype", positions, velocity_history, candidate_actions)
    if nsteps == 0:
        cost = None if goal is None else torch.zeros(B, dtype=dt, device=dev)
        preds = torch.empty(0, B, N, 3, dtype=dt, device=dev) if return_trajectories else None
        return CandidateRollouts(batch.pos.clone().view(B, N, 3), cost, preds, acts)
    for attempt in range(2):
        pos, hist = batch.pos.clone(), batch.hist.clone()
        cost = None if goal is None else torch.zeros(B, dtype=dt, device=dev)
        preds = torch.empty(nsteps, B * N, 3, dtype=dt, device=dev) if return_trajectories else None
        with deferred_overflow_check() as chk:
            for k in range(nsteps):
                ef = edge_features(pos, batch.edge_index)
                vel = torch.cat([hist[h] for h in range(H)], 1)                       # [B*N, 3H], oldest first
                v = simulator.predict_velocity(velocities=vel, node_type=batch.node_type, edge_index=batch.edge_index,
                                               edge_features=ef).contiguous()
                if kernels:
                    _n.launch("csplat_plan_integrate", dev, B, N, H, nsteps, k, _n.ptr(v), _n.ptr(acts), grasped_particle, _n.ptr(pos), _n.ptr(hist),
                              _n.ptr(preds), _n.ptr(goal if goal is None else goal.contiguous()), _n.ptr(node_w), _n.ptr(step_w), _n.ptr(cost))
                    continue
                # the composed step: the same rule for an int as the kernel's (outside [0, N) pins nothing); an index tensor as torch takes it
                vb = v.view(B, N, 3)
                if not isinstance(grasped_particle, int) or 0 <= grasped_particle < N:
                    vb[:, grasped_particle] = acts[:, k].to(v.dtype) if isinstance(grasped_particle, int) else acts[:, k, None].to(v.dtype)
                pos += v
                if H > 1:
                    hist[:H - 1] = hist[1:].clone()
                hist[-1] = v
                if preds is not None:
                    preds[k] = v
                if goal is not None and (step_w is not None or k == nsteps - 1):
                    term = _cost_composed(pos.view(B, N, 3), goal, node_w)
                    cost += term if step_w is None else step_w[k] * term
            if attempt == 0 and chk.overflowed():          # (the one host read of the rollout)
                continue        # a step left fp16's range: the module now runs bf16 pieces -- the rollout again, from its start
        break
    return CandidateRollouts(pos.view(B, N, 3), cost, None if preds is None else preds.view(nsteps, B, N, 3), acts)


class MPC:
    """The planner object of the reference's manipulation/planning.py:289-311: A candidates, horizon H.
        mpc = MPC(simulator, A=100, H=6, input_sequence_length=2)
        rollouts = mpc.model_rollout(positions, velocity_history, node_type, edge_index, candidate_actions, grasped_particle)
        best_action_idx, best_actions, cost_action = mpc.compute_cost(rollouts, goal_particles)
    and, beyond the reference, a CEM refinement of the candidates (`refine`) with the receding-horizon `shift`."""

    def __init__(self, simulator, A=100, H=6, input_sequence_length=2):
        self.simulator, self.A, self.H, self.input_sequence_length = simulator, int(A), int(H), int(input_sequence_length)
        self._batch_key, self._batch = None, None

    def _candidate_batch(self, positions, velocity_history, node_type, edge_index, B):
        """the block-diagonal graph, kept while the same tensors come back: its CSR orderings are then built once"""
        key = (id(edge_index), edge_index._version, id(node_type), node_type._version, B, tuple(positions.shape), tuple(velocity_history.shape),
               positions.dtype, positions.device)
        if self._batch_key != key or self._batch[0] is not edge_index:
            b = batch_candidates(positions, velocity_history, node_type, edge_index, B)
            self._batch_key, self._batch = key, (edge_index, node_type, b)
            return b
        b = self._batch[2]
        return b._replace(pos=positions.repeat(B, 1), hist=velocity_history.repeat(1, B, 1))

    def _check_history(self, velocity_history):
        if int(velocity_history.shape[0]) != self.input_sequence_length:
            raise ValueError(f"MPC: velocity_history holds {int(velocity_history.shape[0])} steps, input_sequence_length is "
                             f"{self.input_sequence_length}")

    def model_rollout(self, positions, velocity_history, node_type, edge_index, candidate_actions, grasped_particle, goal=None,
                      node_weights=None, return_trajectories=False):
        """candidate_actions [A,T,3] rolled min(H, T) steps -> CandidateRollouts"""
        self._check_history(velocity_history)
        if int(candidate_actions.shape[0]) != self.A:
            raise ValueError(f"MPC.model_rollout: {int(candidate_actions.shape[0])} candidates given, A is {self.A}")
        nsteps = min(self.H, int(candidate_actions.shape[1]))
        return rollout_candidates(self.simulator, positions, velocity_history, node_type, edge_index, candidate_actions, grasped_particle,
                                  nsteps, goal=goal, node_weights=node_weights, return_trajectories=return_trajectories,
                                  batch=self._candidate_batch(positions, velocity_history, node_type, edge_index, self.A))

    def compute_cost(self, rollouts, goal_particles, node_weights=None):
        """-> (best_action_idx [] int64, best_actions [T,3], cost_action []), all on the rollouts' device: nothing is read back here.  The
        cheapest candidate, the lowest index on a tie.  Costs the rollout did not carry are formed from its final positions."""
        costs = rollouts.costs
        if costs is None:
            costs = candidate_costs(rollouts.final_positions, goal_particles.to(rollouts.final_positions.dtype), node_weights)
        order, best = select_candidates(costs, 1)
        idx = order.long()
        best_actions = None if rollouts.actions is None else rollouts.actions.index_select(0, idx)[0]
        return idx[0], best_actions, best[0]

    def refine(self, positions, velocity_history, node_type, edge_index, grasped_particle, goal_particles, mu, sigma, iterations=3,
               elites=10, alpha=0.1, sigma_min=1e-4, a_max=0.0, generator=None, node_weights=None):
        """Cross-entropy method over the action sequence: mu / sigma [T,3] (T >= 1; min(H, T) steps are rolled).  Iteration 0 samples the A
        candidates from the given mu, sigma (the refit kernel with alpha = 1: an identity refit); every iteration rolls them out against
        the goal, selects the `elites` cheapest and refits mu, sigma towards them (smoothing alpha), then samples again -- row 0 is always
        clamp(mu), the incumbent.  -> (best_actions [T,3], best_cost [], mu, sigma): the cheapest candidate of ANY iteration (the earliest on
        a tie), so more iterations never return a worse plan.  No host read apart from the one overflow word per rollout."""
        self._check_history(velocity_history)
        A, T = self.A, int(mu.shape[0])
        elites = int(elites)
        if tuple(mu.shape) != (T, 3) or tuple(sigma.shape) != (T, 3) or T < 1 or not 1 <= elites <= A or iterations < 1:
            raise ValueError("MPC.refine: mu and sigma are [T,3], 1 <= elites <= A, iterations >= 1")
        dev, dt = positions.device, positions.dtype
        mu, sigma = mu.to(device=dev, dtype=dt).clone().contiguous(), sigma.to(device=dev, dtype=dt).clone().contiguous()
        nsteps = min(self.H, T)
        batch = self._candidate_batch(positions, velocity_history, node_type, edge_index, A)
        actions = torch.zeros(A, T, 3, dtype=dt, device=dev)
        order = torch.arange(elites, dtype=torch.int32, device=dev)
        gdev = dev if generator is None else generator.device

        def noise():
            return torch.randn(A, T, 3, dtype=dt, device=gdev, generator=generator).to(dev)

        refit_sample(actions, order, mu, sigma, noise(), 1.0, sigma_min, a_max)          # the first candidates: zeros refit with alpha = 1
        best_cost = best_actions = None
        for it in range(int(iterations)):
            r = rollout_candidates(self.simulator, positions, velocity_history, node_type, edge_index, actions, grasped_particle, nsteps,
                                   goal=goal_particles, node_weights=node_weights, batch=batch)
            order, best = select_candidates(r.costs, elites)
            # the cheapest candidate seen so far, kept on the device (row 0 of the next iteration is clamp(mu), the refitted mean -- not
            # the cheapest sample itself, which may be cheaper than anything the next iterations draw)
            cand = actions.index_select(0, order[:1].long())[0]
            if best_cost is None:
                best_cost, best_actions = best[0], cand
            else:
                better = best[0] < best_cost
                best_cost, best_actions = torch.where(better, best[0], best_cost), torch.where(better, cand, best_actions)
            if it < int(iterations) - 1:
                refit_sample(actions, order, mu, sigma, noise(), alpha, sigma_min, a_max)
        return best_actions, best_cost, mu, sigma

    @staticmethod
    def shift(mu, sigma, action_repetition, sigma_init):
        """the receding-horizon shift (planning.py:334-336, `candidate_actions[:, action_repetition:]`): the executed actions are dropped,
        the tail is padded with the last mean and `sigma_init` -> (mu, sigma) of the same length"""
        T, r = int(mu.shape[0]), max(0, min(int(action_repetition), int(mu.shape[0])))
        if r == 0:
            return mu.clone(), sigma.clone()
        mu2 = torch.cat([mu[r:], mu[-1:].expand(r, -1)], 0)
        pad = sigma_init if torch.is_tensor(sigma_init) and sigma_init.dim() == 2 else torch.as_tensor(sigma_init, dtype=sigma.dtype,
                                                                                                     device=sigma.device).expand(T, 3)
        sigma2 = torch.cat([sigma[r:], pad[T - r:].to(sigma)], 0)
        return mu2.contiguous(), sigma2.contiguous()
