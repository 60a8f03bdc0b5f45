"""The unrolled MeshNet training step without a GPU: the composed path of meshnet.train_sim against the restatement tests/train_sim_ref.py
(forward in float32 and float64, the backward that torch's autograd gives the composed path against the restated gather and against
float64 central differences), the reference's quirks each pinned, the loop of unrolled_loss / train_step around a small stand-in
simulator, the schedule helpers, collate, every ValueError, and the library's surface (header, exports, bindings, ABI number, argument
checks before any launch).

Bars.  Composed path against restatement in one dtype: the same operations in the same order, compared with torch.equal -- except the
edge length, where torch.linalg.vector_norm and sqrt(dx*dx + dy*dy + dz*dz) round differently: 4 ulp of the length.  Gradients in float64:
1e-12 of the largest magnitude (two evaluations of one formula that differ in summation order over at most 12 edges per node).  Central
differences with h = 1e-6 on O(1) float64 values: truncation h^2 f''' / 6 ~ 1e-12 / |d|^2 with |d| >= 0.1 on the 6-node graph, rounding
2^-53 / h ~ 1e-10: bar 1e-7 of the largest gradient."""
import os
import re

import pytest
import torch

import util  # noqa: F401
import train_sim_ref as R
from meshnet import train_sim as ts  # (absent: every test of this file fails)
from meshnet.model_utils import IdentityNormalizer, Normalizer
from meshnet.train_sim import collate, curriculum_length, learning_rate, train_step, unrolled_loss, update_prediction

F64, F32 = torch.float64, torch.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIX = torch.tensor([[0, 1, 2, 3, 4, 5, 0, 2, 5, 1], [1, 2, 3, 4, 5, 0, 3, 5, 1, 0]])      # 6 nodes, 10 edges, node 4 has two, (0,1) both ways


def rel(got, want):
    got, want = got.detach().double(), want.detach().double()
    return float((got - want).abs().max()) / max(float(want.abs().max()), 1e-30)


def call(d, ei, H, dtype, grad=False):
    """update_prediction on the inputs `d` (train_sim_ref.inputs) in `dtype`, the normaliser's inverse applied by the caller"""
    c = lambda t: None if t is None else t.to(dtype)  # noqa: E731
    pa = c(d["pred_acc"])
    if d["ostd"] is not None:
        pa = pa * c(d["ostd"]) + c(d["omean"])
    pa, p0 = pa.clone().requires_grad_(grad), c(d["init_position"]).clone().requires_grad_(grad)
    out = update_prediction(c(d["noise"]), c(d["velocity"]), pa, p0, ei, c(d["old_actions"]), c(d["actions"]), "cpu", H)
    return out, pa, p0


# ------------------------------------------------------------------------------------------------------------------ forward
@pytest.mark.parametrize("H", [1, 2, 3, 4])
@pytest.mark.parametrize("kind", R.ACTION_CASES)
def test_composed_forward_equals_the_restatement(kind, H):
    N, ei = 40, R.random_graph(40, 130, seed=H)
    for noise in (True, False):
        d = R.inputs(N, H, kind, with_noise=noise)
        for dt in (F32, F64):
            (hist, ef, pos), _pa, _p0 = call(d, ei, H, dt)
            r_hist, r_ef, r_pos = R.forward(d["velocity"], d["noise"], d["pred_acc"], d["init_position"], d["old_actions"], d["actions"], ei, H, dt)
            assert hist.dtype == dt and ef.dtype == dt and pos.dtype == dt
            assert hist.shape == (N, 3 * H) and ef.shape == (130, 4) and pos.shape == (N, 3)
            assert torch.equal(hist, r_hist) and torch.equal(pos, r_pos) and torch.equal(ef[:, :3], r_ef[:, :3])
            assert ((ef[:, 3] - r_ef[:, 3]).abs() <= 4 * torch.finfo(dt).eps * r_ef[:, 3]).all()
            assert not hist.requires_grad


def test_new_tensors_come_back_and_the_inputs_are_not_written():
    d = R.inputs(12, 3)
    keep = {k: v.clone() for k, v in d.items() if v is not None}
    (hist, ef, pos), _pa, _p0 = call(d, R.random_graph(12, 30), 3, F32)
    assert all(torch.equal(d[k], keep[k]) for k in keep)
    assert hist.data_ptr() != d["velocity"].data_ptr() and pos.data_ptr() != d["init_position"].data_ptr()
    # input_sequence_length defaults to the width of the history; `device` is optional
    out = update_prediction(d["noise"], d["velocity"], d["pred_acc"], d["init_position"], R.random_graph(12, 30), d["old_actions"], d["actions"])
    assert torch.equal(out[0], hist) and torch.equal(out[2], pos)


# ------------------------------------------------------------------------------------------------------------------ the quirks
def test_the_masks_are_per_component():
    """a grasped node whose action has one component exactly 0 integrates the predicted velocity in that component"""
    v = torch.tensor([[0.5, 0.25, 0.125]], dtype=F64)
    acc = torch.tensor([[1.0, 2.0, 4.0]], dtype=F64)
    p0 = torch.tensor([[10.0, 20.0, 30.0]], dtype=F64)
    old = torch.tensor([[7.0, 0.0, 9.0]], dtype=F64)
    act = torch.tensor([[0.0, 3.0, 0.0]], dtype=F64)
    hist, ef, pos = update_prediction(None, v, acc, p0, torch.zeros(2, 0, dtype=torch.int64), old, act)
    # x: next action 0 -> integrates nv = old action 7;  y: next action 3 -> p0 + 3;  z: next action 0, old 9 -> p0 + 9
    assert pos.tolist() == [[17.0, 23.0, 39.0]] and ef.shape == (0, 4)
    # with old action 0 in x: nv = v + acc = 1.5
    pos = update_prediction(None, v, acc, p0, torch.zeros(2, 0, dtype=torch.int64), torch.zeros(1, 3, dtype=F64), act)[2]
    assert pos.tolist() == [[11.5, 23.0, 34.125]]


def test_the_last_history_slot_is_the_old_velocity_with_the_next_action_over_it():
    """not nv: the predicted acceleration never enters the history"""
    v = torch.tensor([[1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0, 8.0, 9.0]], dtype=F64)
    noise = torch.full((1, 9), 0.5, dtype=F64)
    acc = torch.tensor([[100.0, 100.0, 100.0]], dtype=F64)
    act = torch.tensor([[0.0, -2.0, 0.0]], dtype=F64)
    hist = update_prediction(noise, v, acc, torch.zeros(1, 3, dtype=F64), torch.zeros(2, 0, dtype=torch.int64), torch.ones(1, 3, dtype=F64), act)[0]
    assert hist.tolist() == [[4.5, 5.5, 6.5, 7.5, 8.5, 9.5, 7.5, -2.0, 9.5]]
    # H = 1 shifts nothing: the one slot is the last slot
    hist = update_prediction(None, v[:, :3], acc, torch.zeros(1, 3, dtype=F64), torch.zeros(2, 0, dtype=torch.int64), torch.zeros(1, 3, dtype=F64), act)[0]
    assert hist.tolist() == [[1.0, -2.0, 3.0]]


def test_the_overlapping_slice_copy_of_the_reference_is_this_shift():
    """the reference writes velocity[:, :-3] = velocity[:, 3:] in place; on this torch that is the shift, for H = 2, 3 and 4"""
    for H in (2, 3, 4):
        v = torch.arange(5 * 3 * H, dtype=F32).reshape(5, 3 * H)
        w = v.clone()
        w[:, :-3] = w[:, 3:]
        hist = update_prediction(None, v, torch.zeros(5, 3), torch.zeros(5, 3), torch.zeros(2, 0, dtype=torch.int64), torch.zeros(5, 3), torch.zeros(5, 3))[0]
        assert torch.equal(hist, w)


def test_edge_features_have_the_sign_of_the_rollout():
    p0 = torch.tensor([[0.0, 0.0, 0.0], [3.0, 4.0, 0.0]])
    z = torch.zeros(2, 3)
    ef = update_prediction(None, z, z, p0, torch.tensor([[0], [1]]), z, z)[1]
    assert ef.tolist() == [[-3.0, -4.0, 0.0, 5.0]]          # pos[row] - pos[col], the opposite of data_utils.compute_edge_features


# ------------------------------------------------------------------------------------------------------------------ gradients
def _weighted(out, w_ef, w_pos):
    return (out[1] * w_ef).sum() + (out[2] * w_pos).sum()


@pytest.mark.parametrize("kind", R.ACTION_CASES)
def test_autograd_of_the_composed_path_against_the_restated_gather_and_finite_differences(kind):
    N, H, E = 6, 2, int(SIX.shape[1])
    d = R.inputs(N, H, kind, fold=False, seed=5)
    d["pred_acc"] = d["pred_acc"] * 100.0           # (steps of 0.1: edges of 0.1 .. 1 between the six nodes)
    w_ef, w_pos = (t.double() for t in R.incoming(N, E))
    out, pa, p0 = call(d, SIX, H, F64, grad=True)
    g_pa, g_p0 = torch.autograd.grad(_weighted(out, w_ef, w_pos), (pa, p0), retain_graph=True)
    r_ef = R.forward(d["velocity"], d["noise"], d["pred_acc"], d["init_position"], d["old_actions"], d["actions"], SIX, H, F64)[1]
    assert float(r_ef[:, 3].min()) > 0.05
    r_pa, r_p0 = R.backward(r_ef, w_ef, w_pos, d["old_actions"], d["actions"], SIX, F64)
    assert rel(g_pa, r_pa) <= 1e-12 and rel(g_p0, r_p0) <= 1e-12
    # masked components are exactly 0, the others are the position's gradient
    free = (d["actions"] == 0) & (d["old_actions"] == 0)
    assert not g_pa[~free].any() and torch.equal(g_pa[free], g_p0[free])
    # central differences in float64, every element of both inputs
    h = 1e-6
    for name, g in (("pred_acc", g_pa), ("init_position", g_p0)):
        fd = torch.zeros(N, 3, dtype=F64)
        for n in range(N):
            for c in range(3):
                vals = []
                for s in (+h, -h):
                    e = {k: (v.double() if v is not None else None) for k, v in d.items()}
                    e[name] = e[name].clone()
                    e[name][n, c] += s
                    vals.append(float(_weighted(call(e, SIX, H, F64)[0], w_ef, w_pos)))
                fd[n, c] = (vals[0] - vals[1]) / (2 * h)
        assert rel(g, fd) <= 1e-7, (name, rel(g, fd))
    # only one incoming gradient
    only_pos = torch.autograd.grad((out[2] * w_pos).sum(), (pa, p0), retain_graph=True)
    assert torch.equal(only_pos[1], w_pos) and torch.equal(only_pos[0], torch.where(free, w_pos, torch.zeros_like(w_pos)))
    only_ef = torch.autograd.grad((out[1] * w_ef).sum(), (pa, p0))
    assert rel(only_ef[1], R.backward(r_ef, w_ef, None, d["old_actions"], d["actions"], SIX, F64)[1]) <= 1e-12


def test_nothing_flows_to_the_velocity_the_noise_or_the_actions():
    d = {k: (v.double().requires_grad_() if v is not None else None) for k, v in R.inputs(6, 2, "all zero").items()}
    out = update_prediction(d["noise"], d["velocity"], d["pred_acc"], d["init_position"], SIX, d["old_actions"], d["actions"])
    assert not out[0].requires_grad
    (out[1].sum() + out[2].sum()).backward()
    assert d["pred_acc"].grad is not None and d["init_position"].grad is not None
    assert all(d[k].grad is None for k in ("velocity", "noise", "old_actions", "actions"))


def test_a_zero_length_edge_has_a_zero_length_gradient():
    """two nodes at one place (and a self loop): the length term is 0 there, as with torch.norm, and nothing is NaN"""
    z = torch.zeros(3, 3, dtype=F64)
    p0 = torch.tensor([[1.0, 2.0, 3.0], [1.0, 2.0, 3.0], [0.0, 0.0, 0.0]], dtype=F64).requires_grad_()
    pa = z.clone().requires_grad_()
    ei = torch.tensor([[0, 2, 1], [1, 2, 2]])
    ef = update_prediction(None, z, pa, p0, ei, z, z)[1]
    assert ef[0].tolist() == [0.0, 0.0, 0.0, 0.0] and ef[1].tolist() == [0.0, 0.0, 0.0, 0.0]
    ef[:, 3].sum().backward()
    n = torch.tensor([1.0, 2.0, 3.0], dtype=F64) / 14.0 ** 0.5
    assert torch.isfinite(p0.grad).all() and not p0.grad[0].any()
    assert rel(p0.grad[1], n) <= 1e-15 and rel(p0.grad[2], -n) <= 1e-15 and torch.equal(pa.grad, p0.grad)
    r = R.backward(ef, torch.tensor([[0.0, 0.0, 0.0, 1.0]] * 3, dtype=F64), None, z, z, ei, F64)[1]
    assert rel(p0.grad, r) <= 1e-15


# ------------------------------------------------------------------------------------------------------------------ the loop
class StandIn(torch.nn.Module):
    """a simulator of a few lines with ClothMeshSimulator's predict_acceleration contract, whose prediction reads the edge features
    (summed per destination node), so that the path through them carries a gradient on the CPU"""

    def __init__(self, H, normalize, dtype=F64):
        super().__init__()
        self.lin = torch.nn.Linear(3 * H + 4, 3).to(dtype)
        self._output_normalizer = Normalizer(3, device="cpu") if normalize else IdentityNormalizer(3, device="cpu")
        self.calls = []

    def predict_acceleration(self, velocity, node_type, edge_index, edge_features, target_velocities=None, velocity_noise=None):
        self.calls.append(velocity_noise is not None)
        base = velocity if velocity_noise is None else velocity + velocity_noise
        agg = torch.zeros(velocity.shape[0], 4, dtype=velocity.dtype).index_add(0, edge_index[1], edge_features)
        pred = self.lin(torch.cat([base, agg], 1))
        return pred, self._output_normalizer(target_velocities - base[:, -3:], self.training)


def batch(N, E, H, S, seed=0, dtype=F64):
    g = torch.Generator().manual_seed(500 + seed)
    src = torch.randint(0, N, (E,), generator=g)
    ei = torch.stack([src, (src + 1 + torch.randint(0, N - 1, (E,), generator=g)) % N])      # (no self loop: hand_loop differentiates a sqrt)
    pos = torch.rand(N, 3, generator=g).to(dtype)
    act = torch.zeros(N, S, 3, dtype=dtype)
    act[N // 2] = torch.randn(S, 3, generator=g).to(dtype) * 0.05
    act[N // 2, 1, 1] = 0.0
    d = pos[ei[0]] - pos[ei[1]]
    return ((torch.randn(N, 3 * H, generator=g) * 0.05).to(dtype), torch.zeros(N, 1, dtype=dtype), ei, torch.cat([d, d.norm(dim=1, keepdim=True)], 1),
            (torch.randn(N, S, 3, generator=g) * 0.05).to(dtype), act, pos)


def hand_loop(sim, b, F, noise):
    """the reference's loop, the transition from the restatement with torch's autograd behind it"""
    vel, nt, ei, ef, tgt, act, pos = b
    loss, steps = 0, []
    for f in range(F):
        nz = noise if f == 0 else None
        pred, target = sim.predict_acceleration(vel, nt, ei, ef, tgt[:, f], velocity_noise=nz)
        steps.append(((pred - target) ** 2).mean())
        loss = loss + steps[-1]
        if f < F - 1:
            vel, ef, pos = R.forward(vel, nz, sim._output_normalizer.inverse(pred), pos, act[:, f], act[:, f + 1], ei, vel.shape[1] // 3, F64)
    return loss, steps


@pytest.mark.parametrize("normalize", [False, True])
def test_unrolled_loss_is_the_reference_loop(normalize):
    torch.manual_seed(3)
    H, S = 2, 3
    sim = StandIn(H, normalize)
    b = batch(30, 90, H, S)
    if normalize:
        sim._output_normalizer(torch.randn(50, 3, dtype=F64).float() * 0.03 + 0.01, True)      # some statistics
        sim.eval()
    noise = torch.randn(30, 3 * H, dtype=F64) * 1e-3
    grads = {}
    for F in (1, 2, 3):
        sim.calls = []
        loss, steps = unrolled_loss(sim, *b, F, velocity_noise=noise)
        assert sim.calls == [True] + [False] * (F - 1)                   # the noise at f = 0 only
        assert len(steps) == F and rel(loss, sum(steps).detach()) <= 1e-15
        got = torch.autograd.grad(loss, list(sim.parameters()))
        want_loss, want_steps = hand_loop(sim, b, F, noise)
        want = torch.autograd.grad(want_loss, list(sim.parameters()))
        assert rel(loss.detach(), want_loss.detach()) <= 1e-12 and all(rel(a, c.detach()) <= 1e-12 for a, c in zip(steps, want_steps))
        assert all(rel(a, c) <= 1e-11 for a, c in zip(got, want))
        grads[F] = got
    # F = 1 is the single-step loss, bit for bit
    pred, target = sim.predict_acceleration(b[0], b[1], b[2], b[3], b[4][:, 0], velocity_noise=noise)
    assert torch.equal(unrolled_loss(sim, *b, 1, velocity_noise=noise)[0], ((pred - target) ** 2).mean())
    # the second step's loss reaches the parameters through the first prediction as well: cut that path and the gradient changes
    vel, nt, ei, ef, tgt, act, pos = b
    pred, target = sim.predict_acceleration(vel, nt, ei, ef, tgt[:, 0], velocity_noise=noise)
    vel2, ef2, _ = R.forward(vel, noise, sim._output_normalizer.inverse(pred).detach(), pos, act[:, 0], act[:, 1], ei, H, F64)
    pred2, target2 = sim.predict_acceleration(vel2, nt, ei, ef2, tgt[:, 1])
    cut = torch.autograd.grad(((pred - target) ** 2).mean() + ((pred2 - target2) ** 2).mean(), list(sim.parameters()))
    assert rel(grads[2][0], cut[0]) > 1e-6


def test_train_step_draws_the_noise_steps_the_optimizer_and_takes_a_collated_batch():
    H, S = 2, 3
    sim = StandIn(H, False, F32)
    samples = [batch(n, e, H, S, seed=i, dtype=F32) for i, (n, e) in enumerate(((10, 30), (7, 0), (12, 40)))]
    one = collate(samples)
    # collate: rows in order, edge_index offset by the nodes in front
    assert [tuple(t.shape) for t in one] == [(29, 6), (29, 1), (2, 70), (70, 4), (29, 3, 3), (29, 3, 3), (29, 3)]
    assert torch.equal(one[2][:, :30], samples[0][2]) and torch.equal(one[2][:, 30:], samples[2][2] + 17) and one[2].dtype == torch.int64
    assert torch.equal(one[0][10:17], samples[1][0]) and torch.equal(one[6][17:], samples[2][6]) and torch.equal(one[3][30:], samples[2][3])
    before = [p.detach().clone() for p in sim.parameters()]
    opt = torch.optim.SGD(sim.parameters(), lr=0.1)
    sim.lin.weight.grad = torch.full_like(sim.lin.weight, 1e6)            # zero_grad comes before backward: this must not survive
    torch.manual_seed(11)
    loss, steps = train_step(sim, opt, one, future_sequence_length=2, noise_std=1e-3)
    assert not loss.requires_grad and len(steps) == 2
    # the same step by hand: the noise is normal(0, noise_std) of the velocity's shape from the same generator state
    ref = StandIn(H, False, F32)
    ref.load_state_dict({k: v for k, v in zip(ref.state_dict().keys(), [before[0], before[1]])})
    torch.manual_seed(11)
    noise = torch.normal(mean=0.0, std=1e-3, size=one[0].shape)
    want, _ = unrolled_loss(ref, *one, 2, velocity_noise=noise)
    assert torch.equal(loss, want.detach())
    want.backward()
    for p, q, b0 in zip(sim.parameters(), ref.parameters(), before):
        assert rel(p.detach(), b0 - 0.1 * q.grad) <= 1e-6 and not torch.equal(p.detach(), b0)
    # the block-diagonal batch is the sum of its samples: per-sample losses weighted by their node counts
    parts = [unrolled_loss(ref, *s, 1)[0] * s[0].shape[0] for s in samples]
    assert rel(unrolled_loss(ref, *one, 1)[0].detach(), (sum(parts) / 29).detach()) <= 1e-5


def test_schedule_helpers():
    n = 100
    assert [curriculum_length(s, n) for s in (0, 33, 34, 65, 66, 67, 99)] == [1, 1, 2, 2, 2, 3, 3]      # 0.33 < and 0.66 <, both strict
    assert curriculum_length(330, 1000) == 1 and curriculum_length(331, 1000) == 2 and curriculum_length(660, 1000) == 2 and curriculum_length(661, 1000) == 3
    assert learning_rate(0, 1e-3, 0.1, 300) == 1e-3 + 1e-6
    assert learning_rate(300, 1e-3, 0.1, 300) == 1e-3 * 0.1 + 1e-6
    assert learning_rate(150, 1e-3, 0.1, 300) == 1e-3 * (0.1 ** 0.5) + 1e-6
    with pytest.raises(ValueError, match="curriculum_length"):
        curriculum_length(1, 0)
    with pytest.raises(ValueError, match="learning_rate"):
        learning_rate(1, 1e-3, 0.1, 0)


# ------------------------------------------------------------------------------------------------------------------ every ValueError
def test_argument_errors():
    d = R.inputs(6, 2)
    good = dict(velocity_noise=d["noise"], velocity=d["velocity"], pred_acc=d["pred_acc"], init_position=d["init_position"], edge_index=SIX,
                old_particle_actions=d["old_actions"], particle_actions=d["actions"], input_sequence_length=2)
    bad = [dict(velocity=torch.zeros(6)), dict(velocity=torch.zeros(6, 6, dtype=torch.int64)), dict(velocity=[[0.0] * 6] * 6), dict(input_sequence_length=3),
           dict(input_sequence_length=0), dict(input_sequence_length=2.0), dict(velocity=torch.zeros(6, 51), velocity_noise=None, input_sequence_length=17),
           dict(velocity=torch.zeros(6, 5), velocity_noise=None, input_sequence_length=None), dict(velocity_noise=torch.zeros(6, 3)),
           dict(pred_acc=torch.zeros(5, 3)), dict(pred_acc=torch.zeros(6, 2)), dict(init_position=torch.zeros(6)), dict(old_particle_actions=torch.zeros(7, 3)),
           dict(particle_actions=torch.zeros(6, 4)), dict(particle_actions=None), dict(edge_index=torch.tensor([[0, 6], [1, 2]])),
           dict(edge_index=torch.tensor([[0, -1], [1, 2]])), dict(edge_index=torch.zeros(3, 4, dtype=torch.int64)), dict(edge_index=torch.zeros(2, dtype=torch.int64)),
           dict(edge_index=torch.zeros(2, 4)), dict(edge_index=[[0], [1]])]
    for kw in bad:
        with pytest.raises(ValueError, match="update_prediction"):
            update_prediction(**dict(good, **kw))
    b = batch(8, 20, 2, 3)
    for F, kw in ((0, {}), (True, {}), (2.0, {}), (4, {}), (3, dict(tv=b[4][:, :2])), (3, dict(pa=b[5][:, :2])), (2, dict(tv=b[4][:, 0])),
                  (2, dict(pa=b[5][..., :2])), (2, dict(tv=None))):
        with pytest.raises(ValueError, match="unrolled_loss"):
            unrolled_loss(StandIn(2, False), b[0], b[1], b[2], b[3], kw.get("tv", b[4]), kw.get("pa", b[5]), b[6], F)
    with pytest.raises(ValueError, match="train_step"):
        train_step(StandIn(2, False), None, b[:6])
    for samples in ([], [b[:6]], [b, (b[0][:5],) + b[1:]], [b, b[:2] + (b[2][0],) + b[3:]], [b, batch(8, 20, 3, 3)], [b, b[:3] + (b[3][:5],) + b[4:]]):
        with pytest.raises(ValueError, match="collate"):
            collate(samples)


def test_edge_index_is_checked_once_per_tensor_object(monkeypatch):
    d = R.inputs(6, 2)
    ei = SIX.clone()
    args = lambda e: (d["noise"], d["velocity"], d["pred_acc"], d["init_position"], e, d["old_actions"], d["actions"])  # noqa: E731
    update_prediction(*args(ei))
    reads = []
    real = torch.Tensor.tolist
    monkeypatch.setattr(torch.Tensor, "tolist", lambda self: reads.append(1) or real(self))
    for _ in range(3):
        update_prediction(*args(ei))
    assert reads == []                                           # the same object at the same version: no second range check
    ei[0, 0] = 5                                                 # an in-place edit is a new version
    update_prediction(*args(ei))
    assert reads == [1]
    ei[0, 0] = 6
    with pytest.raises(ValueError, match="0 .. N-1"):
        update_prediction(*args(ei))
    update_prediction(*args(SIX.to(torch.int32)))               # another integer dtype is converted
    assert len(ts._EDGES) < 16 and all(v[4] is None or v[4] is not v[0]() for v in ts._EDGES.values())


# ------------------------------------------------------------------------------------------------------------------ the library's surface
ENTRIES = (("int", "csplat_train_update_fwd", 16), ("int", "csplat_train_update_bwd", 15))
SRC = os.path.join(ROOT, "cloth-splatting_amd", "csrc", "csplat_train_sim.hip")


def test_header_exports_and_bindings():
    from csplat import native
    header = open(os.path.join(ROOT, "include", "csplat.h")).read()
    for res, name, n_args in ENTRIES:
        assert re.search(r"\b" + res + " " + name + r"\s*\(", header), name
        assert name in native.EXPORTS and hasattr(native.lib, name) and len(native.EXPORTS[name][1]) == n_args
        decl = header[header.index(res + " " + name + "("):]
        decl = re.sub(r"/\*.*?\*/", "", decl[:decl.index(";")], flags=re.S)
        assert decl.count(",") + 1 == n_args, (name, decl)
    block = header[header.index("/* MeshNet training transition"):header.index("int csplat_train_update_fwd(")]
    assert block.rstrip().endswith("Added exports: CSPLAT_ABI_VERSION is unchanged. */")
    flat = re.sub(r"\s*\n \*\s*", " ", block)
    for word in ("old_actions[n][c] != 0 ? old_actions[n][c] : vn[n][3(H-1)+c] + pa[n][c]", "actions[n][c] == 0 ? init_position[n][c] + nv[n][c]",
                 "H = 1 shifts nothing", "per component", "not nv", "bit-equal to csplat_gnn_edge_features", "rounded once", "ONE launch",
                 "CSR by source, then the CSR by destination", "0 for a zero-length edge", "No atomics", "two runs give equal bits",
                 "actions[n][c] == 0 && old_actions[n][c] == 0", "times ostd[c]", "H outside 1 .. 16", "omean without ostd", "beyond 2^31", "no-op"):
        assert word.lower() in flat.lower(), word
    assert native.ABI_VERSION == 9 and native.lib.csplat_abi_version() == 9
    code = re.sub(r"//.*", "", open(SRC).read())
    assert "atomic" not in code.lower() and "#pragma clang fp contract(off)" in code and "__fmaf_rn(" in code
    # plain operators under the pragma: the __fmul_rn / __fadd_rn header functions are compiled before it and fuse into an fma (the file's header)
    assert not re.search(r"__f(mul|add|sub|div)_rn\(", code) and "acc * in.ostd[c] + in.omean[c]" in code
    assert code.count("<<<") == 2 and "k_train_update_fwd" in code and "k_train_update_bwd" in code       # one launch each way


def test_which_launch_constant_each_gpu_size_crosses():
    """tests/test_train_sim_gpu.py runs N = 1, 2, WORKGROUP - 1 / + 0 / + 1 and 1000 with E chosen so that N + E is not a multiple of the
    workgroup: the forward's grid is ceil((N + E) / WORKGROUP) workgroups whose first N threads take nodes -- the node / edge seam falls
    inside a wave (N = 1, 2, 255), on a workgroup edge (256), one past it (257) and in the fourth workgroup (1000); the backward's grid
    is ceil(N / WORKGROUP): one workgroup up to 256, two from 257, four at 1000.  The hub of 3000 edges is one backward thread's loop."""
    src = open(SRC).read()
    m = re.search(r"constexpr int TRAIN_SIM_THREADS = (\d+);", src)
    assert m and int(m.group(1)) == R.WORKGROUP == 256
    assert "cdiv((int64_t)N + n_edge, TRAIN_SIM_THREADS)" in src and "cdiv(N, TRAIN_SIM_THREADS)" in src
    assert "__launch_bounds__(TRAIN_SIM_THREADS)" in src and src.count("__launch_bounds__(TRAIN_SIM_THREADS)") == 2
    import gnn_kernels_ref as G
    assert G.HUB_DEGREE == 3000 and int(G.graph(1000, "hub").shape[1]) == 3000


def test_the_library_refuses_bad_arguments_before_any_launch():
    """fake, distinct, aligned addresses 2^32 apart: every call here must be refused (or be a no-op) before a launch could touch them"""
    from csplat import native
    L = native.lib
    A = lambda i: (i + 1) << 32  # noqa: E731
    names = ("vel", "noise", "pred", "omean", "ostd", "init", "old", "act", "ei", "hist", "ef", "pos")

    def fwd(N=100, E=50, H=3, **kw):
        p = {k: A(i) for i, k in enumerate(names)}
        p.update(kw)
        return L.csplat_train_update_fwd(None, N, E, H, *[p[k] for k in names])
    for kw in (dict(N=-1), dict(E=-1), dict(H=0), dict(H=17), dict(H=-2), dict(N=2 ** 28, H=3), dict(N=2 ** 27, H=16), dict(E=2 ** 29), dict(omean=None),
               dict(ostd=None), dict(vel=None), dict(pred=None), dict(init=None), dict(old=None), dict(act=None), dict(ei=None), dict(vel=A(0) + 2),
               dict(noise=A(1) + 1), dict(pred=A(2) + 3), dict(omean=A(3) + 2), dict(ostd=A(4) + 1), dict(init=A(5) + 2), dict(old=A(6) + 2), dict(act=A(7) + 1),
               dict(ei=A(8) + 4), dict(hist=A(9) + 2), dict(ef=A(10) + 8), dict(ef=A(10) + 4), dict(pos=A(11) + 1), dict(hist=A(0)),
               dict(hist=A(0) + 100 * 9 * 4 - 4), dict(hist=A(1) + 16), dict(pos=A(2)), dict(pos=A(5) + 100 * 12 - 4), dict(pos=A(6)), dict(pos=A(7) + 12),
               dict(ef=A(8)), dict(ef=A(8) + 2 * 50 * 8 - 16), dict(pos=A(3) + 8), dict(hist=A(4) + 8), dict(pos=A(9) + 16), dict(ef=A(9)),
               dict(ef=A(11) + 100 * 12 - 16)):
        assert fwd(**kw) == 2, kw
        assert b"csplat_train_update_fwd" in L.csplat_last_error(), kw
    nothing = dict(hist=None, ef=None, pos=None)
    assert fwd(N=0) == 0 and fwd(**nothing) == 0 and fwd(N=0, vel=None, pred=None, init=None) == 0
    assert fwd(E=0, hist=None, pos=None) == 0                            # edge features of no edges: nothing wanted
    bnames = ("ef", "gef", "gpos", "old", "act", "ostd", "srp", "spm", "drp", "dpm", "gpred", "ginit")

    def bwd(N=100, E=50, **kw):
        p = {k: A(i) for i, k in enumerate(bnames)}
        p.update(kw)
        return L.csplat_train_update_bwd(None, N, E, *[p[k] for k in bnames])
    for kw in (dict(N=-1), dict(E=-1), dict(E=2 ** 29), dict(ef=None), dict(srp=None), dict(spm=None), dict(drp=None), dict(dpm=None), dict(old=None),
               dict(act=None), dict(ef=A(0) + 8), dict(gef=A(1) + 4), dict(gpos=A(2) + 2), dict(old=A(3) + 1), dict(act=A(4) + 2), dict(ostd=A(5) + 3),
               dict(srp=A(6) + 2), dict(spm=A(7) + 1), dict(drp=A(8) + 2), dict(dpm=A(9) + 3), dict(gpred=A(10) + 2), dict(ginit=A(11) + 1),
               dict(gpred=A(0)), dict(gpred=A(1) + 50 * 16 - 4), dict(ginit=A(2)), dict(ginit=A(3) + 100 * 12 - 4), dict(gpred=A(4) + 12), dict(ginit=A(5) + 8),
               dict(gpred=A(6) + 100 * 4), dict(ginit=A(7) + 16), dict(gpred=A(8)), dict(ginit=A(9) + 50 * 4 - 4), dict(ginit=A(10)),
               dict(gpred=A(11) + 100 * 12 - 4)):
        assert bwd(**kw) == 2, kw
        assert b"csplat_train_update_bwd" in L.csplat_last_error(), kw
    assert bwd(N=0) == 0 and bwd(gpred=None, ginit=None) == 0 and bwd(N=0, ef=None, old=None, act=None) == 0
