"""The training step of the reference's `train()` (train_meshnet_sim.py:478-532) on the HIP kernels of this library: the loss unrolled over
`future_sequence_length` predictions, with the graph state advanced between them by `update_prediction` (:322-359) so that the next step's
positions and edge features stay differentiable functions of the previous step's predicted acceleration.

  update_prediction     the reference's function under its own signature.  It returns NEW tensors (the reference shifts `velocity` in
                        place and returns it).  One launch forward (csplat_train_update_fwd: history shift, new positions and the edge
                        features of the new positions) and one backward (csplat_train_update_bwd: the position gradient gathered per node
                        over the two CSR orderings of GraphCSR -- no float scatter-add, bit-reproducible); include/csplat.h, "MeshNet
                        training transition", states the arithmetic and the quirks that are kept
  UpdatePrediction      its autograd node: gradients flow to pred_acc and init_position only
  unrolled_loss         the loop :500-526 -> (loss, per-step losses); the output normaliser's inverse is folded into the transition
  train_step            one optimizer step on a batch, in the reference's order: zero_grad, backward, step (:530-532)
  curriculum_length, learning_rate      the schedule (:480-489, :552)
  collate               one block-diagonal batch of several samples: what PyG's DataLoader(batch_size=32) hands the reference

Dispatch as in meshnet.data_utils: float32 contiguous GPU tensors take the kernels; anything else composes the same definitions from torch
operations in the dtype of `velocity` (reported through csplat.native.composed_fallback for GPU tensors: raises under STRICT; it is the
CPU path).  `edge_index` is validated once per tensor object (dtype, shape [2,E], range: one blocking read), never per step.

The sample data set, its batches and the validation rollout's errors are meshnet.dataloader_sim (SamplesClothSimDataset; train_step takes
its Batch as it is).  Loading trajectory files, logging and checkpoints are host-side plumbing and stay out of scope."""
import types
import weakref

import torch
from torch.autograd.function import once_differentiable

from csplat import native as _n
from .model_utils import Normalizer, get_velocity_noise

BATCH_FIELDS = ("velocity", "node_types", "edge_index", "edge_features", "target_velocities", "particle_actions", "positions")
_EDGES = {}       # id(edge_index) -> (weak reference, in-place version, N, device, the checked copy or None when the tensor itself fits)


def _checked_edges(edge_index, N, device, what):
    """`edge_index` as contiguous int64 [2,E] on `device` with entries inside 0 .. N-1 -- checked (one blocking read) the first time this
    tensor OBJECT is seen at its current in-place version, remembered afterwards.  An int64 contiguous tensor on `device` is returned
    itself, so that GraphCSR.get finds the CSR the network built for it."""
    hit = _EDGES.get(id(edge_index))
    if hit is not None and hit[0]() is edge_index and hit[1] == edge_index._version and hit[2] == N and hit[3] == device:
        return edge_index if hit[4] is None else hit[4]
    if not torch.is_tensor(edge_index) or edge_index.dtype.is_floating_point or edge_index.dtype in (torch.bool, torch.complex64, torch.complex128):
        raise ValueError(f"{what}: `edge_index` is an integer tensor [2,E], got {getattr(edge_index, 'dtype', type(edge_index).__name__)}")
    if edge_index.dim() != 2 or edge_index.shape[0] != 2:
        raise ValueError(f"{what}: `edge_index` is [2,E], got {tuple(edge_index.shape)}")
    fits = edge_index.dtype == torch.int64 and edge_index.device == device and edge_index.is_contiguous() and not edge_index.requires_grad
    ei = edge_index if fits else edge_index.detach().to(device=device, dtype=torch.int64).contiguous()
    if ei.shape[1]:
        lo, hi = torch.stack((ei.min(), ei.max())).tolist()          # the one blocking read
        if lo < 0 or hi >= N:
            raise ValueError(f"{what}: `edge_index` entries must lie in 0 .. N-1 = {N - 1}, got {lo} .. {hi}")
    for k in [k for k, v in _EDGES.items() if v[0]() is None]:
        del _EDGES[k]
    _EDGES[id(edge_index)] = (weakref.ref(edge_index), edge_index._version, N, device, None if fits else ei)      # (never a strong reference to its own key)
    return ei


def _composed(velocity_noise, velocity, pred_acc, init_position, ei, old_actions, actions, H, omean=None, ostd=None):
    """the definitions of csplat_train_update_fwd from torch operations, torch's autograd behind them"""
    dt = velocity.dtype
    vn = (velocity if velocity_noise is None else velocity + velocity_noise.to(dt)).detach()
    old_actions, actions = old_actions.detach().to(dt), actions.detach().to(dt)
    pa = pred_acc.to(dt)
    if ostd is not None:
        pa = pa * ostd.to(dt).reshape(1, 3) + omean.to(dt).reshape(1, 3)
    last = vn[:, 3 * (H - 1):3 * H]
    nv = torch.where(old_actions != 0, old_actions, last + pa)
    p0 = init_position.to(dt)
    new_pos = torch.where(actions == 0, p0 + nv, p0) + actions
    hist = torch.cat([vn[:, 3:3 * H], torch.where(actions != 0, actions, last)], 1)
    d = new_pos[ei[0]] - new_pos[ei[1]]
    return hist, torch.cat([d, torch.linalg.vector_norm(d, dim=1, keepdim=True)], 1), new_pos


class UpdatePrediction(torch.autograd.Function):
    """(hist, edge_feat, new_pos) of csplat_train_update_fwd for float32 contiguous GPU tensors; `ei` a checked edge list, `omean` / `ostd`
    [3] or None.  Gradients to pred_acc and init_position (csplat_train_update_bwd); hist carries none."""

    @staticmethod
    def forward(ctx, velocity_noise, velocity, pred_acc, init_position, ei, old_actions, actions, H, omean=None, ostd=None):
        from .graph_ops import GraphCSR
        ctx.set_materialize_grads(False)
        N, E, dev = int(velocity.shape[0]), int(ei.shape[1]), velocity.device
        f32 = dict(dtype=torch.float32, device=dev)
        hist, new_pos = torch.empty(N, 3 * H, **f32), torch.empty(N, 3, **f32)
        edge_feat = torch.empty(E, 4, **f32)
        pred_acc, init_position = pred_acc.detach(), init_position.detach()
        if N > 0:
            _n.launch("csplat_train_update_fwd", dev, N, E, H, _n.ptr(velocity), _n.ptr(velocity_noise), _n.ptr(pred_acc), _n.ptr(omean),
                      _n.ptr(ostd), _n.ptr(init_position), _n.ptr(old_actions), _n.ptr(actions), _n.ptr(ei) if E else None, _n.ptr(hist),
                      _n.ptr(edge_feat) if E else None, _n.ptr(new_pos))
        ctx.csr = GraphCSR.get(ei, N) if (E and N) else None
        ctx.ostd = ostd
        ctx.save_for_backward(edge_feat, old_actions, actions)
        ctx.mark_non_differentiable(hist)
        return hist, edge_feat, new_pos

    @staticmethod
    @once_differentiable
    def backward(ctx, _g_hist, g_edge, g_pos):
        edge_feat, old_actions, actions = ctx.saved_tensors
        want_pred, want_init = ctx.needs_input_grad[2], ctx.needs_input_grad[3]
        if (g_edge is None and g_pos is None) or not (want_pred or want_init):
            return (None,) * 10
        N, E, dev, csr = int(actions.shape[0]), int(edge_feat.shape[0]), actions.device, ctx.csr
        g_edge = None if (g_edge is None or csr is None) else g_edge.to(torch.float32).contiguous()
        if g_edge is not None and g_edge.data_ptr() % 16:
            g_edge = g_edge.clone()
        g_pos = None if g_pos is None else g_pos.to(torch.float32).contiguous()
        g_pred = torch.empty(N, 3, dtype=torch.float32, device=dev) if want_pred else None
        g_init = torch.empty(N, 3, dtype=torch.float32, device=dev) if want_init else None
        if N > 0:
            rp, pm = (csr.rowptr, csr.perm) if g_edge is not None else ({"src": None, "dst": None},) * 2
            _n.launch("csplat_train_update_bwd", dev, N, E, _n.ptr(edge_feat) if g_edge is not None else None, _n.ptr(g_edge), _n.ptr(g_pos),
                      _n.ptr(old_actions), _n.ptr(actions), _n.ptr(ctx.ostd), _n.ptr(rp["src"]), _n.ptr(pm["src"]), _n.ptr(rp["dst"]),
                      _n.ptr(pm["dst"]), _n.ptr(g_pred), _n.ptr(g_init))
        return None, None, g_pred, g_init, None, None, None, None, None, None


def _rows(t, name, cols, N, what):
    if not torch.is_tensor(t) or t.dim() != 2 or t.shape[1] != cols or (N is not None and t.shape[0] != N):
        shape = tuple(t.shape) if torch.is_tensor(t) else type(t).__name__
        raise ValueError(f"{what}: `{name}` is a tensor [{'N' if N is None else N},{cols}], got {shape}")
    return t


def _transition(velocity_noise, velocity, pred_acc, init_position, edge_index, old_actions, actions, H, omean, ostd, what):
    """update_prediction with the output normaliser's statistics (omean, ostd [3], or None) folded in"""
    if not torch.is_tensor(velocity) or velocity.dim() != 2 or not velocity.dtype.is_floating_point:
        raise ValueError(f"{what}: `velocity` is a floating point tensor [N,3H], got "
                         f"{(velocity.dtype, tuple(velocity.shape)) if torch.is_tensor(velocity) else type(velocity).__name__}")
    N = int(velocity.shape[0])
    if H is None:
        H = int(velocity.shape[1]) // 3
    if not isinstance(H, int) or isinstance(H, bool) or not 1 <= H <= 16 or velocity.shape[1] != 3 * H:
        raise ValueError(f"{what}: input_sequence_length is an integer in 1 .. 16 and `velocity` [N,3 * input_sequence_length], got "
                         f"{H!r} next to {tuple(velocity.shape)}")
    if velocity_noise is not None and (not torch.is_tensor(velocity_noise) or velocity_noise.shape != velocity.shape):
        raise ValueError(f"{what}: `velocity_noise` is None or shaped like `velocity`, got {tuple(getattr(velocity_noise, 'shape', ()))}")
    for t, name in ((pred_acc, "pred_acc"), (init_position, "init_position"), (old_actions, "old_particle_actions"), (actions, "particle_actions")):
        _rows(t, name, 3, N, what)
    if N * 3 * H >= 2 ** 31 or 4 * int(edge_index.shape[1] if torch.is_tensor(edge_index) and edge_index.dim() == 2 else 0) >= 2 ** 31:
        raise ValueError(f"{what}: N * 3H and 4E must stay below 2^31")
    dev = velocity.device
    ei = _checked_edges(edge_index, N, dev, what)
    tensors = (velocity_noise, velocity, pred_acc, init_position, old_actions, actions, omean, ostd)
    if any(t is not None and t.device != dev for t in tensors):
        raise ValueError(f"{what}: every tensor lives on the device of `velocity` ({dev})")
    if velocity.is_cuda:
        why = _n.why_not_f32c(*tensors)
        if why is None:
            return UpdatePrediction.apply(None if velocity_noise is None else velocity_noise.detach(), velocity.detach(), pred_acc, init_position, ei,
                                          old_actions.detach(), actions.detach(), H, omean, ostd)
        _n.composed_fallback("train_sim.update_prediction", why, velocity)
    return _composed(velocity_noise, velocity, pred_acc, init_position, ei, old_actions, actions, H, omean, ostd)


def update_prediction(velocity_noise, velocity, pred_acc, init_position, edge_index, old_particle_actions, particle_actions, device=None,
                      input_sequence_length=None):
    """The reference's update_prediction (train_meshnet_sim.py:322-359) -> (velocity history [N,3H], edge features [E,4], new positions
    [N,3]), all NEW tensors on the inputs' device (`device` is the reference's argument and is not needed).  pred_acc is the de-normalised
    acceleration.  input_sequence_length defaults to velocity.shape[1] / 3.  The result is differentiable in pred_acc and init_position;
    velocity, the noise and the actions are data.  Edge features have the sign of meshnet.rollout.edge_features (PyG Cartesian +
    Distance, norm=False) and are bit-equal to it on the new positions."""
    return _transition(velocity_noise, velocity, pred_acc, init_position, edge_index, old_particle_actions, particle_actions,
                       input_sequence_length, None, None, "update_prediction")


def _output_statistics(simulator, like):
    """(mean, std) [3] of the simulator's output normaliser as the transition folds them in, or (None, None) for the identity"""
    on = simulator._output_normalizer
    if not isinstance(on, Normalizer):
        return None, None
    return (on._mean().detach().reshape(-1).to(device=like.device, dtype=like.dtype).contiguous(),
            on._std_with_epsilon().detach().reshape(-1).to(device=like.device, dtype=like.dtype).contiguous())


def unrolled_loss(simulator, velocity, node_types, edge_index, edge_features, target_velocities, particle_actions, positions,
                  future_sequence_length, velocity_noise=None):
    """The loss of one training step as the reference unrolls it (train_meshnet_sim.py:500-526): for f in 0 .. F-1 one
    simulator.predict_acceleration(..., target_velocities[:, f], noise) and loss += mean((pred - target)^2); between predictions the state
    goes through the transition with particle_actions[:, f] and [:, f + 1] (the output normaliser's inverse folded into its kernel).  The
    noise is applied at f = 0 only.  target_velocities, particle_actions [N,>=F,3].  -> (loss, [the F per-step losses])."""
    what = "unrolled_loss"
    F = future_sequence_length
    if not isinstance(F, int) or isinstance(F, bool) or F < 1:
        raise ValueError(f"{what}: future_sequence_length is an integer >= 1, got {F!r}")
    for t, name in ((target_velocities, "target_velocities"), (particle_actions, "particle_actions")):
        if not torch.is_tensor(t) or t.dim() != 3 or t.shape[2] != 3 or t.shape[1] < F:
            raise ValueError(f"{what}: `{name}` is [N,S,3] with S >= future_sequence_length = {F}, got "
                             f"{tuple(t.shape) if torch.is_tensor(t) else type(t).__name__}")
    H = int(velocity.shape[1]) // 3
    # (one copy for all steps: step f's actions as a contiguous [N,3])
    actions = particle_actions.detach()[:, :F].transpose(0, 1).contiguous() if F > 1 else None
    loss, steps, init = None, [], positions
    for f in range(F):
        noise = velocity_noise if f == 0 else None
        pred, target = simulator.predict_acceleration(velocity, node_types, edge_index, edge_features, target_velocities[:, f], velocity_noise=noise)
        step = torch.mean((pred - target) ** 2)
        steps.append(step)
        loss = step if loss is None else loss + step
        if f < F - 1:
            omean, ostd = _output_statistics(simulator, pred)
            velocity, edge_features, init = _transition(noise, velocity, pred, init, edge_index, actions[f], actions[f + 1], H, omean, ostd, what)
    return loss, steps


def train_step(simulator, optimizer, batch, future_sequence_length=1, noise_std=0.0):
    """One optimizer step on `batch` = (velocity, node_types, edge_index, edge_features, target_velocities, particle_actions, positions),
    the 7-tuple of the reference's `_graph_to_data` (a collate() of several is one too).  The noise is get_velocity_noise's: normal(0,
    noise_std) of the velocity's shape, drawn where the reference draws it.  Order as the reference's: zero_grad, backward, step.
    -> (loss, per-step losses), detached.  A meshnet.dataloader_sim.Batch is taken as it is: its first seven fields are this tuple."""
    if getattr(batch, "_fields", ())[:7] == BATCH_FIELDS:
        batch = batch[:7]
    try:
        velocity, node_types, edge_index, edge_features, target_velocities, particle_actions, positions = batch
    except (TypeError, ValueError):
        raise ValueError("train_step: batch is (velocity, node_types, edge_index, edge_features, target_velocities, particle_actions, "
                         "positions)") from None
    H = int(velocity.shape[1]) // 3
    noise = get_velocity_noise(types.SimpleNamespace(x=velocity), noise_std=noise_std, input_sequence_length=H, device=velocity.device)
    loss, steps = unrolled_loss(simulator, velocity, node_types, edge_index, edge_features, target_velocities, particle_actions, positions,
                                future_sequence_length, velocity_noise=noise.to(velocity.dtype))
    optimizer.zero_grad()
    loss.backward()
    optimizer.step()
    return loss.detach(), [s.detach() for s in steps]


def curriculum_length(step, ntraining_steps):
    """future_sequence_length under the reference's --curriculum (train_meshnet_sim.py:480-489), which starts at 1: 2 once
    0.33 < step / ntraining_steps, 3 once 0.66 < step / ntraining_steps, both strict (at a ratio of exactly 0.66 neither of the reference's
    conditions holds and the length stays 2)."""
    if ntraining_steps <= 0:
        raise ValueError(f"curriculum_length: ntraining_steps must be > 0, got {ntraining_steps!r}")
    r = step / ntraining_steps
    return 3 if 0.66 < r else (2 if 0.33 < r else 1)


def learning_rate(step, lr_init, decay_rate, decay_steps):
    """lr_init * decay_rate ** (step / decay_steps) + 1e-6 (train_meshnet_sim.py:552)"""
    if decay_steps == 0:
        raise ValueError("learning_rate: decay_steps must not be 0")
    return lr_init * (decay_rate ** (step / decay_steps)) + 1e-6


def collate(samples):
    """Several samples (7-tuples as train_step takes them) -> ONE block-diagonal batch of the same form: node and edge rows concatenated in
    order, each sample's edge_index offset by the number of nodes in front of it.  The transition and the network are per node and per
    edge, so a batch needs nothing else."""
    samples = list(samples)
    if not samples:
        raise ValueError("collate: no samples")
    for s in samples:
        if not isinstance(s, (tuple, list)) or len(s) != 7:
            raise ValueError("collate: a sample is (velocity, node_types, edge_index, edge_features, target_velocities, particle_actions, positions)")
        N = int(s[0].shape[0])
        if any(int(s[i].shape[0]) != N for i in (1, 4, 5, 6)) or s[2].dim() != 2 or s[2].shape[0] != 2 or s[3].shape[0] != s[2].shape[1]:
            raise ValueError("collate: a sample's node tensors share N rows, its edge_index is [2,E] and its edge_features have E rows")
    for i in (0, 1, 3, 4, 5, 6):
        if any(s[i].shape[1:] != samples[0][i].shape[1:] for s in samples):
            raise ValueError("collate: the samples' tensors differ in their trailing shapes")
    offsets, n = [], 0
    for s in samples:
        offsets.append(n)
        n += int(s[0].shape[0])
    cat = lambda i: torch.cat([s[i] for s in samples], 0)  # noqa: E731
    edge_index = torch.cat([s[2] + off for s, off in zip(samples, offsets)], 1)
    return cat(0), cat(1), edge_index, cat(3), cat(4), cat(5), cat(6)
