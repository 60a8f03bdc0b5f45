"""The hot loop of the reference's rollout (/root/reference/train_meshnet_sim.py:92-265, the part between the data set and the
bookkeeping): per step

    graph features from the CURRENT node positions   (:147-152: `_data_to_graph` + FaceToEdge / Cartesian / Distance; the
                                                      connectivity of a fixed triangulation does not change, the features do)
    v_next = simulator.predict_velocity(cat(velocity history), node_type, edge_index, edge_features)     (:156-160)
    v_next[grasped] = action[step]                                                                        (:176)
    positions += v_next;  history <- (history[1:], v_next)                                                (:256-262)

with the per-step edge features from one HIP kernel (csplat_gnn_edge_features) instead of two PyG transforms.
Returns the predicted velocities [nsteps, N, 3] like the reference's `predictions`."""
import torch

from csplat import native as _n


def refine_scratch_floats(N):
    """floats of the scratch of csplat_gnn_edge_length_refine.  include/csplat.h, at csplat_gnn_edge_length_refine: "scratch = 9 N floats,
    contents irrelevant" (the second velocity buffer and the two Adam moments of the double-buffered iteration)."""
    return 9 * N


def edge_features(pos, edge_index):
    """[E, 4] = (pos[row] - pos[col], norm), row / col = edge_index[0] / [1] (PyG Cartesian + Distance, norm=False).  The sign is the
    opposite of meshnet.data_utils.compute_edge_features (the reference's own: pos[edge_index[1]] - pos[edge_index[0]])."""
    if pos.is_cuda and pos.dtype == torch.float32 and edge_index.dtype == torch.int64:
        pos, edge_index = pos.contiguous(), edge_index.contiguous()
        E = int(edge_index.shape[1])
        out = torch.empty(E, 4, dtype=torch.float32, device=pos.device)
        _n.launch("csplat_gnn_edge_features", pos.device, E, _n.ptr(pos), _n.ptr(edge_index), _n.ptr(out))
        return out
    _n.composed_fallback("rollout.edge_features", "dtype", pos)
    d = pos[edge_index[0]] - pos[edge_index[1]]
    return torch.cat([d, d.norm(dim=1, keepdim=True)], 1)


def refine_edge_lengths(pos, v, edge_index, rest_len, grasped_particle=None, iters=10, lr=1e-3, edge_w=None, in_place=False):
    """The `real_world` branch of the reference's rollout (/root/reference/train_meshnet_sim.py:211-250), per rollout step: `iters`
    iterations of a FRESH torch.optim.Adam(lr) on the predicted velocities v [N,3] against
        sum_e (|(pos + v)[edge_index[0][e]] - (pos + v)[edge_index[1][e]]| - rest_len[e])^2
    with the one entry zeroed that the reference zeroes (`length_deviation[grasped_particle] *= 0` indexes the EDGE array with the node
    index -- kept as is).  Returns the refined velocities (a new tensor).  On the GPU: csplat_gnn_edge_length_refine, one launch per
    iteration, no autograd graph, no atomics; elsewhere the reference's own torch formulation (reported as a composed fallback)."""
    E = int(edge_index.shape[1])
    if v.is_cuda and v.dtype == torch.float32 and pos.dtype == torch.float32 and edge_index.dtype == torch.int64:
        from .graph_ops import GraphCSR
        dev = v.device
        N = int(v.shape[0])
        csr = GraphCSR.get(edge_index, N)
        out = v if (in_place and v.is_contiguous()) else v.detach().clone().contiguous()      # (in_place: the kernel updates v itself)
        w = edge_w          # (a rollout builds the weights once for all its steps)
        if w is None and grasped_particle is not None and E > 0:
            w = torch.ones(E, dtype=torch.float32, device=dev)
            w[grasped_particle] = 0.0
        scratch = torch.empty(refine_scratch_floats(max(N, 1)), dtype=torch.float32, device=dev)
        rl = rest_len.to(device=dev, dtype=torch.float32).contiguous()
        p_ = pos.contiguous()
        _n.launch("csplat_gnn_edge_length_refine", dev, N, E, _n.ptr(p_), _n.ptr(out), _n.ptr(csr.ei), _n.ptr(rl), _n.ptr(w),
                  _n.ptr(csr.rowptr["dst"]), _n.ptr(csr.perm["dst"]), _n.ptr(csr.rowptr["src"]), _n.ptr(csr.perm["src"]), int(iters), float(lr),
                  0.9, 0.999, 1e-8, _n.ptr(scratch))
        return out
    _n.composed_fallback("rollout.refine_edge_lengths", "dtype", v)
    with torch.enable_grad():
        vo = v.detach().clone().requires_grad_(True)
        opt = torch.optim.Adam([vo], lr=lr)
        for _ in range(iters):
            opt.zero_grad()
            x = pos.detach() + vo
            d = x[edge_index[0]] - x[edge_index[1]]
            dev_ = torch.norm(d, dim=1) - rest_len
            if grasped_particle is not None:
                keep = torch.ones_like(dev_)
                keep[grasped_particle] = 0
                dev_ = dev_ * keep
            torch.sum(dev_ ** 2).backward()
            opt.step()
    return vo.detach()


import os as _os

# the rollout loop recorded: one eager step (weight images packed, caches filled), one step recorded into a hipGraph, the rest replays.
# CSPLAT_ROLLOUT_GRAPH=0 keeps the launch-by-launch loop.
ROLLOUT_GRAPH = _os.environ.get("CSPLAT_ROLLOUT_GRAPH", "1") not in ("", "0")
# a ClothMeshSimulator at latent 128 in eval mode: the step as library launches only (_FusedClothStep); CSPLAT_ROLLOUT_FUSED=0: the generic step
FUSED_STEP = _os.environ.get("CSPLAT_ROLLOUT_FUSED", "1") not in ("", "0")
ROLLOUT_STATS = {"eager_steps": 0, "replayed_steps": 0, "recorded": 0, "record_failed": 0, "repeated_bf16": 0}


# ---- the two steppers.  Each owns the state buffers of a rollout and offers: begin(...) -- a new rollout into the buffers; before(step) /
# after(step) -- what the host does around a step; step(recording) -- the step launch by launch, safe to capture; finish(...) -- the
# results, or None when the step left fp16's range; references() -- what a kept recording must keep alive.  _run() drives either.
class _GenericStep:
    """One rollout step through simulator.predict_velocity and stock tensor operations, on state tensors `pos` [N,3] / `hist` [H,N,3]
    (updated in place), the step's grasped-node velocity `act` [3] and the step's output `out` [N,3]: the host copies the action in before
    a step and the output row out behind it.  Works on CPU tensors too (never recorded there)."""

    def __init__(self, simulator, positions, velocity_history, node_type, edge_index, grasped_particle, real_world, original_edge_lengths):
        dev = positions.device
        self.sim, self.node_type, self.edge_index, self.grasped, self.real_world = simulator, node_type, edge_index, grasped_particle, real_world
        self.pos, self.hist = torch.empty_like(positions), torch.empty_like(velocity_history)
        self.act = None
        self.out = torch.empty_like(self.pos)
        self.L0 = torch.empty(original_edge_lengths.shape, dtype=torch.float32, device=dev) if real_world else None
        self.edge_w = None
        if real_world and positions.is_cuda and int(edge_index.shape[1]) > 0:
            self.edge_w = torch.ones(int(edge_index.shape[1]), dtype=torch.float32, device=dev)
            self.edge_w[grasped_particle] = 0.0          # (`length_deviation[grasped_particle] *= 0`, train_meshnet_sim.py:234)
        self.graph, self.kept = None, False
        # the fp16-piece arithmetic of the one-launch kernels reports an overflow as a device word per predict_velocity call: the words of
        # eager steps are collected in `items` and read ONCE behind the loop (no host read per step); a recorded step ANDs its words into
        # `fine`, which lives across the replays (they overwrite the step's own words)
        self.items, self.fine, self.mods = [], None, []
        self.actions = self.preds = None

    def references(self):
        """strong references: whatever the recording's raw pointers point into stays alive (and its addresses un-reusable) as long as the
        recording can be replayed"""
        from .graph_ops import GraphCSR
        return (self.sim, self.edge_index, self.node_type, GraphCSR.get(self.edge_index, self.pos.shape[0]))

    def begin(self, positions, velocity_history, actions, original_edge_lengths, nsteps, will_record):
        self.pos.copy_(positions); self.hist.copy_(velocity_history)
        if self.L0 is not None:
            self.L0.copy_(original_edge_lengths)
        if nsteps and self.act is None:
            self.act = torch.empty(actions.shape[1:], dtype=actions.dtype, device=self.pos.device)
        self.actions = actions
        self.preds = torch.empty(nsteps, positions.shape[0], positions.shape[1], dtype=positions.dtype, device=self.pos.device)
        self.items = []
        if self.fine is not None:
            self.fine.fill_(True)
        elif will_record:
            self.fine = torch.ones((), dtype=torch.bool, device=self.pos.device)      # (set here, OUTSIDE the recording: replays only AND into it)

    def before(self, step):
        self.act.copy_(self.actions[step])

    def after(self, step):
        self.preds[step].copy_(self.out)

    def step(self, recording=False):
        from .graph_network import _OVERFLOW_COLLECT
        pos, hist, grasped = self.pos, self.hist, self.grasped
        H = hist.shape[0]
        words = [] if recording else self.items
        _OVERFLOW_COLLECT.append(words)
        try:
            ef = edge_features(pos, self.edge_index)
            vel = torch.cat([hist[h] for h in range(H)], 1)                       # [N, 3H], oldest first (:145)
            v_next = self.sim.predict_velocity(velocities=vel, node_type=self.node_type, edge_index=self.edge_index, edge_features=ef)
            if self.real_world:
                # (ADVICE: the reference pins the grasped node BEFORE the refinement too, train_meshnet_sim.py:176 -- a change of its own)
                v_next = refine_edge_lengths(pos, v_next, self.edge_index, self.L0, grasped, edge_w=self.edge_w)
            v_next[grasped] = self.act
            self.out.copy_(v_next)
            pos += v_next
            if H > 1:
                hist[:H - 1] = hist[1:].clone()
            hist[-1] = v_next
        finally:
            _OVERFLOW_COLLECT.pop()
        if recording:
            # (inside the recording; `words` holds tensors of the capture's private pool and is dropped here, with every other local)
            for _m, ok in words:
                self.fine.logical_and_(ok)
            self.mods = list({id(m): m for m, _ok in words}.values())

    def finish(self, nsteps, check_overflow=True):
        from .graph_network import deferred_overflow_check
        preds, self.actions, self.preds = self.preds, None, None
        if check_overflow:
            chk = deferred_overflow_check()
            chk.items = self.items + ([(m, self.fine) for m in self.mods] if self.graph is not None else [])
            self.items = []
            if chk.overflowed():         # (the one host read of the rollout; the modules concerned now run with bf16 pieces)
                return None
        # (the state buffers belong to a kept recording: hand back a copy)
        return preds, (self.pos.clone() if self.kept else self.pos)


class _FusedClothStep:
    """One rollout step of a ClothMeshSimulator (latent 128, the fused inference kernels) as LIBRARY LAUNCHES ONLY (round 6): head
    (history + node type -> normalised node features), edge features in destination order, the two encoder launches, the processor's
    30 launches, the decoder's two hidden layers (csplat_linear128), decode (last Linear + de-normalisation + last velocity + finite
    check), [edge-length refinement], integrate (pin, predictions row, positions, history shift).  The step number lives on the device
    (the head launch counts it up; integrate reads the step's action and writes the step's row of the predictions by it), so a recorded
    step needs NOTHING from the host per step.  State buffers belong to this object."""

    @staticmethod
    def applicable(sim, positions, velocity_history, node_type, edge_index, actions, grasped_particle):
        from .cloth_network import ClothMeshSimulator
        from .graph_network import ENCODER_FUSED
        from .graph_ops import edge_mlp3_mode, is_mlp3_128, _linears
        if not (isinstance(sim, ClothMeshSimulator) and not sim.training and isinstance(grasped_particle, int) and positions.is_cuda):
            return False
        epd = sim._encode_process_decode
        if getattr(epd, "_bf16_latched", False) or edge_mlp3_mode() != 0 or not ENCODER_FUSED:
            return False
        if not (positions.dtype == torch.float32 and velocity_history.dtype == torch.float32 and actions.dtype == torch.float32 and
                positions.dim() == 2 and positions.shape[1] == 3 and velocity_history.dim() == 3 and velocity_history.shape[2] == 3 and
                actions.dim() == 2 and actions.shape[1] == 3 and edge_index.dtype == torch.int64 and int(edge_index.shape[1]) > 0):
            return False
        N, H, T = int(positions.shape[0]), int(velocity_history.shape[0]), int(sim._node_type_embedding_size)
        if not 0 <= grasped_particle < N:        # (k_rollout_integrate pins nothing outside [0, N); `v_next[-1] = act` of the generic step does)
            return False
        F = 3 * H + T
        if not (F % 4 == 0 and F <= 32 and is_mlp3_128(epd._encoder.node_fn[0], k_in=F) and is_mlp3_128(epd._encoder.edge_fn[0], k_in=4) and
                is_mlp3_128(epd._decoder.node_fn, k_in=128, n_out=3) and _linears(epd._decoder.node_fn)[2].weight.is_contiguous() and
                node_type.numel() == N):
            return False
        # (the processor's one-launch kernels in destination order: asked on tensors of the right shape)
        probe_x = torch.empty(N, 128, dtype=torch.float32, device=positions.device)
        probe_e = torch.empty(int(edge_index.shape[1]), 128, dtype=torch.float32, device=positions.device)
        with torch.no_grad():
            return epd._processor.takes_destination_order(probe_x, probe_e)

    def __init__(self, sim, positions, velocity_history, node_type, edge_index, cap, grasped_particle, real_world):
        from .graph_ops import GraphCSR
        dev = positions.device
        self.sim, self.epd, self.node_type = sim, sim._encode_process_decode, node_type
        self.N, self.H, self.T = int(positions.shape[0]), int(velocity_history.shape[0]), int(sim._node_type_embedding_size)
        self.F, self.E, self.cap = 3 * self.H + self.T, int(edge_index.shape[1]), int(cap)
        self.edge_index, self.grasped, self.real_world = edge_index, int(grasped_particle), bool(real_world)
        f32 = dict(dtype=torch.float32, device=dev)
        self.pos = torch.empty(self.N, 3, **f32)
        self.hist = torch.empty(self.H, self.N, 3, **f32)
        self.v = torch.empty(self.N, 3, **f32)
        self.feats = torch.empty(self.N, self.F, **f32)
        self.ef = torch.empty(self.E, 4, **f32)
        self.actions = torch.zeros(self.cap, 3, **f32)
        self.preds = torch.empty(self.cap, self.N, 3, **f32)
        self.nt = node_type.reshape(-1).to(device=dev, dtype=torch.int32).contiguous()
        self.counter = torch.zeros(1, dtype=torch.int32, device=dev)
        self.fine = torch.ones(1, dtype=torch.int32, device=dev)
        self.am = torch.zeros(2, **f32)             # max |node feature|, max |edge feature| of the step (float bits by atomicMax)
        self.norm = {k: torch.empty(n_, **f32) for k, n_ in (("nm", self.F), ("ns", self.F), ("om", 3), ("os", 3))}
        self.has_node_norm = self.has_out_norm = False
        self.csr = GraphCSR.get(edge_index, self.N)
        self.plan = self.csr.agg_plan()
        self.L0 = torch.empty(self.E, **f32) if real_world else None
        self.edge_w = None
        if real_world:
            self.edge_w = torch.ones(self.E, **f32)
            self.edge_w[self.grasped] = 0.0          # (`length_deviation[grasped_particle] *= 0`, train_meshnet_sim.py:234)
        self.graph, self.kept = None, False

    def references(self):
        return (self.sim, self.edge_index, self.node_type)

    def begin(self, positions, velocity_history, actions, original_edge_lengths, nsteps, will_record):
        """the state of a new rollout -> the buffers (stock copies, once per rollout); the normalisers' statistics as plain vectors"""
        from .model_utils import Normalizer
        self.pos.copy_(positions); self.hist.copy_(velocity_history)
        # (ADVICE: sized by cap, not by what is used -- more rows than cap raise, fewer than nsteps are padded with zeros; a change of its own)
        self.actions[:actions.shape[0]].copy_(actions)
        self.counter.zero_(); self.fine.fill_(1); self.am.zero_()
        if self.L0 is not None:
            self.L0.copy_(original_edge_lengths)
        nn_, on_ = self.sim._node_normalizer, self.sim._output_normalizer
        self.has_node_norm, self.has_out_norm = isinstance(nn_, Normalizer), isinstance(on_, Normalizer)
        if self.has_node_norm:
            self.norm["nm"].copy_(nn_._mean().reshape(-1)); self.norm["ns"].copy_(nn_._std_with_epsilon().reshape(-1))
        if self.has_out_norm:
            self.norm["om"].copy_(on_._mean().reshape(-1)); self.norm["os"].copy_(on_._std_with_epsilon().reshape(-1))

    def before(self, step):         # (the step number lives on the device: nothing for the host to do around a step)
        pass

    after = before

    def step(self, recording=False):
        from .graph_network import _encode_inference
        from .graph_ops import rows_chain, _linears
        dev = self.pos.device
        epd, N, H, T = self.epd, self.N, self.H, self.T
        nm, ns = (self.norm["nm"], self.norm["ns"]) if self.has_node_norm else (None, None)
        om, os_ = (self.norm["om"], self.norm["os"]) if self.has_out_norm else (None, None)
        _n.launch("csplat_rollout_head", dev, N, H, T, _n.ptr(self.hist), _n.ptr(self.nt), _n.ptr(nm), _n.ptr(ns), _n.ptr(self.feats),
                  _n.ptr(self.counter), self.am.data_ptr())
        _n.launch("csplat_gnn_edge_features_ordered", dev, self.E, _n.ptr(self.pos), _n.ptr(self.csr.ei), _n.ptr(self.plan["perm"]),
                  _n.ptr(self.ef), self.am.data_ptr() + 4)
        # the encoders (one launch each) with the absmax words the two launches above left: no absmax pass of their own
        xe = _encode_inference(epd._encoder.node_fn, self.feats, self.am[0:1])
        ee = _encode_inference(epd._encoder.edge_fn, self.ef, self.am[1:2])
        if xe is None or ee is None:         # (an encoder the one-launch form does not cover: the module's own path)
            xe, ee = epd._encoder(self.feats, self.ef)
        # the first layer's x_i / x_j products and the decoder's two hidden layers: ONE launch each on pre-packed 16-bit pieces
        # (csplat_gnn_rows_chain) instead of four exact-fp32 launches of 16 us; the images are the modules' own, packed per weight version
        xp, _e = epd._processor(xe, self.edge_index, ee, edges_out=False, dst_order=(self.plan, epd._edge_latent_bound()),
                                first_products=rows_chain(xe, epd._processor.gnn_stacks[0].first_products_image(), 0))
        dec = _linears(epd._decoder.node_fn)
        h = rows_chain(xp, epd._decoder.hidden_image(), 1, dec[0].bias, dec[1].bias)
        last = self.hist[H - 1]
        _n.launch("csplat_rollout_decode", dev, N, 3, _n.ptr(h), _n.ptr(dec[2].weight.detach()), _n.ptr(dec[2].bias.detach().contiguous()),
                  _n.ptr(om), _n.ptr(os_), _n.ptr(last), _n.ptr(self.v), _n.ptr(self.fine))
        if self.real_world:
            # (ADVICE: the reference pins the grasped node BEFORE the refinement too, train_meshnet_sim.py:176 -- a change of its own)
            refine_edge_lengths(self.pos, self.v, self.edge_index, self.L0, self.grasped, edge_w=self.edge_w, in_place=True)
        _n.launch("csplat_rollout_integrate", dev, N, H, 3, _n.ptr(self.v), _n.ptr(self.actions), _n.ptr(self.counter), self.grasped,
                  _n.ptr(self.pos), _n.ptr(self.hist), _n.ptr(self.preds), _n.ptr(self.am))

    def finish(self, nsteps, check_overflow=True):
        preds, pos = self.preds[:nsteps].clone(), self.pos.clone()
        if int(self.fine.item()) == 0:          # (the one host read of the rollout)
            self.epd.latch_bf16()
            return None
        return preds, pos


# recorded steps are kept across rollout() calls (recording costs ~40 ms: a collection pass, the capture, the instantiation -- two steps'
# worth of a 20-step rollout): keyed on everything the recording's raw pointers and baked-in host decisions depend on
_ROLLOUT_CACHE = {}
_ROLLOUT_CACHE_MAX = 2


def _rollout_key(simulator, positions, velocity_history, node_type, edge_index, actions, grasped_particle, real_world):
    from .graph_ops import edge_mlp3_mode
    if not isinstance(grasped_particle, int):
        return None                 # (an index tensor / array: its values are baked into the recording -- not cached)
    parts = [(int(t.data_ptr()), int(t._version)) for t in simulator.state_dict(keep_vars=True).values() if torch.is_tensor(t)]
    for name in ("_output_normalizer", "_node_normalizer"):
        nz = getattr(simulator, name, None)
        if nz is not None:
            for k, v in sorted(vars(nz).items()):
                if torch.is_tensor(v):
                    parts.append((k, int(v.data_ptr()), int(v._version)))
                elif isinstance(v, (int, float, bool, str)) or v is None:
                    parts.append((k, v))
    epd = getattr(simulator, "_encode_process_decode", None)
    return (id(simulator), tuple(parts), tuple(positions.shape), positions.dtype, tuple(velocity_history.shape), tuple(actions.shape[1:]),
            int(node_type.data_ptr()), int(node_type._version), tuple(node_type.shape), int(edge_index.data_ptr()), int(edge_index._version),
            tuple(edge_index.shape), grasped_particle, bool(real_world), edge_mlp3_mode(), bool(getattr(epd, "_bf16_latched", False)),
            bool(simulator.training), _n.SCRATCH_EPOCH[0], positions.device.index)


def _run(make, key, use_graph, nsteps, state, check_overflow=True):
    """One rollout on the stepper kept under `key` (made by make() and kept, first in first out, when there is none; key None: made for
    this rollout only).  With use_graph the first rollout of a stepper runs step 0 launch by launch (weight images packed, caches
    filled) and RECORDS step 1 into a hipGraph; every later step -- of this and of later rollouts on the stepper -- is one replay.  A
    capture that fails leaves the launch-by-launch loop.  -> (predictions, final positions), or None when a step left fp16's range."""
    ent = _ROLLOUT_CACHE.get(key) if key is not None else None
    if ent is None:
        st = make()
        if key is not None:
            st.kept = True
            while len(_ROLLOUT_CACHE) >= _ROLLOUT_CACHE_MAX:
                _ROLLOUT_CACHE.pop(next(iter(_ROLLOUT_CACHE)))
            _ROLLOUT_CACHE[key] = {"step": st, "keep": st.references()}
    else:
        st = ent["step"]
    dev = st.pos.device
    st.begin(*state, nsteps, use_graph)
    for step in range(nsteps):
        st.before(step)
        if use_graph and st.graph is not None:
            st.graph.replay()
            ROLLOUT_STATS["replayed_steps"] += 1
        elif use_graph and step == 1:
            try:
                from csplat.graphs import capture
                torch.cuda.synchronize(dev)
                g = torch.cuda.CUDAGraph()
                with capture(g):
                    st.step(recording=True)
                st.graph = g
                ROLLOUT_STATS["recorded"] += 1
                g.replay()          # (the capture itself executed nothing)
                ROLLOUT_STATS["replayed_steps"] += 1
            except Exception:
                # (a capture that failed half way leaves the state buffers as they were: nothing of a capture executes)
                st.graph, use_graph = None, False
                ROLLOUT_STATS["record_failed"] += 1
                torch.cuda.synchronize(dev)
                st.step()
                ROLLOUT_STATS["eager_steps"] += 1
        else:
            st.step()
            ROLLOUT_STATS["eager_steps"] += 1
        st.after(step)
    res = st.finish(nsteps, check_overflow)
    if res is None:
        _ROLLOUT_CACHE.pop(key, None)           # (recorded with the fp16 pieces: not to be replayed for the latched module)
    return res


@torch.no_grad()
def rollout(simulator, positions, velocity_history, node_type, edge_index, actions, grasped_particle, nsteps, real_world=False,
            original_edge_lengths=None, graph=None):
    """positions [N,3] (updated in place on a copy), velocity_history [H,N,3], actions [nsteps,3] (velocity of the grasped
    node), grasped_particle: index of the pinned node.  -> (predicted velocities [nsteps,N,3], final positions [N,3]).
    real_world=True (train_meshnet_sim.py:211-250, as meshnet/generate_rw_predictions.py:152 calls it): every predicted velocity is
    refined by ten Adam iterations against the deviation of the edge lengths from `original_edge_lengths` (default: the lengths of the
    initial positions, :114-116) before the grasped node is pinned.
    graph (default: ROLLOUT_GRAPH on the GPU, nsteps >= 4): the first rollout of a (simulator weights, graph, shapes) combination runs
    step 0 launch by launch and RECORDS step 1 into a hipGraph on state buffers (positions, history, the step's action, the step's output
    row); every later step -- and every step of later rollouts with the same combination -- is one replay: the same launches in the same
    order on the same buffers, so the result equals the eager loop bit for bit; the host issues one graph launch and two small copies
    per step instead of ~35 launches."""
    if real_world and original_edge_lengths is None:
        original_edge_lengths = torch.norm(positions[edge_index[1]] - positions[edge_index[0]], dim=1)
    use_graph = (ROLLOUT_GRAPH if graph is None else bool(graph)) and positions.is_cuda and nsteps >= 4
    state = (positions, velocity_history, actions, original_edge_lengths)

    def key():
        return _rollout_key(simulator, positions, velocity_history, node_type, edge_index, actions, grasped_particle, real_world)
    if nsteps > 0 and FUSED_STEP and _FusedClothStep.applicable(simulator, positions, velocity_history, node_type, edge_index, actions, grasped_particle):
        cap = max(64, 1 << max(int(nsteps) - 1, 0).bit_length())
        res = _run(lambda: _FusedClothStep(simulator, positions, velocity_history, node_type, edge_index, cap, grasped_particle, real_world),
                   key() + ("fused", cap), use_graph, nsteps, state)
        if res is not None:
            return res
        ROLLOUT_STATS["repeated_bf16"] += 1          # (a step left fp16's range: the module now runs bf16 pieces -- the generic step below)
    for attempt in range(2):
        res = _run(lambda: _GenericStep(simulator, positions, velocity_history, node_type, edge_index, grasped_particle, real_world,
                                        original_edge_lengths),
                   key() if use_graph else None, use_graph, nsteps, state, check_overflow=attempt == 0)
        if res is not None:
            return res
        ROLLOUT_STATS["repeated_bf16"] += 1      # a step left fp16's range: the modules concerned now run bf16 pieces -- once more, from the start
    raise AssertionError("unreachable")
