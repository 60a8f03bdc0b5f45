"""Drop-in for the reference's `meshnet/dataloader_sim.py`: the goal cloud of a fold (`get_goal_fold`, :12-48) and the sample data set
`SamplesClothSimDataset` (:50-425 on its base class meshnet/dataloader.py:9-60), with the trajectories resident on the device and a whole
block-diagonal batch assembled by ONE launch (include/csplat.h, "MeshNet sample data set").

  SamplesClothSimDataset   the reference's class under its signature.  add_trajectory() appends a dictionary as meshnet.data_utils.get_data_traj /
                        process_traj return it to packed device buffers that grow geometrically; the flat sample index -> (trajectory,
                        time index) table is the reference's (dataloader.py:40-48, dataloader_sim.py:152-158)
    batch(indices)      the samples `indices` as one Batch: what the reference's __getitem__ + _data_to_graph + FaceToEdge / Cartesian /
                        Distance + PyG's collate + _graph_to_data hand its training step -- csplat_dataset_batch, one launch, descriptors
                        built on the host with numpy and uploaded in one non-blocking copy.  ds[idx] is a batch of one
    batches(batch_size) one epoch: the descriptors of ALL its batches are built and uploaded once, then one launch per batch
    get_batch_with_candidate_actions   A copies of one sample, each with its own actions (what the reference's planner calls every step)
    __get_val_item__ / val_item        the validation dictionary (:186-246), as views of the store
    collect_observation                keeps the one online trajectory of the closed loop up to date (:290-348)
  face_to_edge          PyG's FaceToEdge followed by coalesce, from stock torch operations: once per trajectory, not a hot path
  rollout_errors, validate   the arithmetic of the reference's validate (train_meshnet_sim.py:293-308): csplat_dataset_rollout_error

Dispatch as in meshnet.data_utils: a store of float32 data on the GPU takes the kernels; a store on the CPU composes the same definitions
from torch operations in its own dtype; a GPU store of another dtype reports through csplat.native.composed_fallback (raises under STRICT)
and composes.  Everything here is data: detached, no gradients.

delaunay=True, the reference's default: collect_observation's trajectory then carries the faces of the Delaunay triangulation of its
sampled nodes (meshnet.data_utils.process_traj, on the device), and the network's edges are face_to_edge(faces).  Loading trajectory
files (`data_path`) is host-side plumbing and stays out of scope."""
import collections

import numpy as np
import torch

from csplat import native as _n
from . import data_utils as _du


def get_goal_fold(init_particles, pick, place):
    """Fold the cloth in half along the pick -> place direction: with a = (place - pick) / |place - pick| and m = (pick + place) / 2, a node p
    whose projection s = (p - m) . a is NEGATIVE is reflected across the plane through m with normal a, p - 2 s a; every other node -- one
    exactly on the fold line included -- stays.  init_particles [N,3], pick [3], place [3], tensors of one floating dtype on one device;
    returns a new [N,3] tensor (detached: a goal is an observation).  Vectorised torch operations, no per-node loop (the reference loops
    over the nodes in Python).  pick == place has no direction and raises ValueError (the reference divides by zero)."""
    what = "get_goal_fold"
    for name, t, shape in (("init_particles", init_particles, None), ("pick", pick, (3,)), ("place", place, (3,))):
        if not torch.is_tensor(t) or not t.dtype.is_floating_point:
            raise ValueError(f"{what}: `{name}` is a floating-point tensor, got {getattr(t, 'dtype', type(t).__name__)}")
        if shape is None and (t.dim() != 2 or t.shape[1] != 3):
            raise ValueError(f"{what}: `init_particles` is [N,3], got {tuple(t.shape)}")
        if shape is not None and tuple(t.shape) != shape:
            raise ValueError(f"{what}: `{name}` is [3], got {tuple(t.shape)}")
    X = init_particles.detach()
    pick, place = pick.detach().to(device=X.device, dtype=X.dtype), place.detach().to(device=X.device, dtype=X.dtype)
    axis = place - pick
    length = torch.sqrt((axis * axis).sum())
    if not bool(length > 0) or not bool(torch.isfinite(length)):        # the call's one blocking read
        raise ValueError(f"{what}: pick and place must be two different finite points (the fold has no direction otherwise)")
    axis = axis / length
    rel = X - ((pick + place) / 2)[None]
    s = rel[:, 0] * axis[0] + rel[:, 1] * axis[1] + rel[:, 2] * axis[2]
    return torch.where((s < 0)[:, None], X - (2 * s)[:, None] * axis[None], X)


# ------------------------------------------------------------------------------------------------------------------ the sample data set
Batch = collections.namedtuple("Batch", ["velocity", "node_types", "edge_index", "edge_features", "target_velocities", "particle_actions",
                                         "positions", "pos_target", "ptr", "grasped_rows"])
Batch.__doc__ = """one block-diagonal batch of B samples, R = the sum of their nodes, Q = the sum of their edges: velocity [R,3H], node_types
[R,1], edge_index int64 [2,Q], edge_features [Q,4], target_velocities / particle_actions [R,F,3], positions [R,3] -- these seven, batch[:7],
are the tuple meshnet.train_sim.train_step takes -- then pos_target [R,F,3], ptr int64 [B+1] (the first row of every sample, and R) and
grasped_rows int64 [B] (the batched row of every grasped node; -1 for a trajectory without one)."""

CandidateSamples = collections.namedtuple("CandidateSamples", Batch._fields + ("pos", "hist", "node_type", "batch", "B", "N"))
CandidateSamples.__doc__ = """a Batch of A copies of one sample with the fields meshnet.mpc.CandidateBatch has beside it, so that
mpc.rollout_candidates(..., batch=this) takes it: pos [A*N,3] (= positions), hist [H,A*N,3] (the velocity, oldest first), node_type [A*N,1],
batch int64 [A*N] (the candidate of a row), B = A, N."""

TABLE_WORDS = 8                     # include/csplat.h: CSPLAT_DATASET_TABLE_WORDS and the words of a row
NODE_BASE, FRAME_BASE, EDGE_BASE, T_N, T_E, T_T, T_G = range(7)
MIN_CAPACITY = 1024                 # rows of a fresh store buffer


def symmetric_edges(edge_index, num_nodes):
    """[2,E] int64 with entries in 0 .. num_nodes-1 -> both directions of every edge, sorted by (row, col), duplicates removed: the layout
    PyG's FaceToEdge (to_undirected -> coalesce) yields"""
    both = torch.cat([edge_index, edge_index.flip(0)], 1)
    key = torch.unique(both[0] * num_nodes + both[1])                   # sorted
    n = max(int(num_nodes), 1)
    return torch.stack((torch.div(key, n, rounding_mode="floor"), key % n)).contiguous()


def face_to_edge(faces, num_nodes):
    """PyG's FaceToEdge followed by coalesce: faces [3,M] integers in 0 .. num_nodes-1 -> the edges (0,1), (1,2), (0,2) of every triangle in
    both directions, sorted by (row, col), each once: int64 [2,E] on the device of `faces`.  Stock torch operations; it runs once per
    trajectory."""
    f = torch.as_tensor(faces)
    if f.dtype.is_floating_point or f.dtype == torch.bool or f.dim() != 2 or f.shape[0] != 3:
        raise ValueError(f"face_to_edge: `faces` is an integer tensor [3,M], got {f.dtype} {tuple(f.shape)}")
    f = f.detach().to(torch.int64)
    ei = _du._checked_edges(torch.cat([f[:2], f[1:], f[::2]], 1), int(num_nodes), f.device, "face_to_edge")
    return symmetric_edges(ei, int(num_nodes))


def _edge_length(d):
    """|d| of rows [.,3] as the kernels form it: float32 rows take sqrt(fma(dz, dz, fma(dx, dx, dy * dy))) -- csplat_gnn_edge_features'
    form; the fused multiply-adds are evaluated in float64, where the product is exact, and rounded once -- other dtypes the same order
    of sums with every operation rounded.  The square root is the correctly rounded one: the GPU's, and on the CPU numpy's (torch's
    vectorised CPU sqrt is sometimes one ulp off, in float32 and in float64)"""
    dx, dy, dz = d[:, 0], d[:, 1], d[:, 2]
    if d.dtype == torch.float32:
        inner = (dx.double() * dx.double() + (dy * dy).double()).float()
        squared = (dz.double() * dz.double() + inner.double()).float()
    else:
        squared = dz * dz + (dx * dx + dy * dy)
    return torch.sqrt(squared) if squared.is_cuda else torch.from_numpy(np.sqrt(squared.numpy()))


_Plan = collections.namedtuple("_Plan", ["B", "j", "t", "ptr", "eptr", "grasped_rows", "max_items", "words"])


class SamplesClothSimDataset:
    """The reference's SamplesClothSimDataset(data_path, input_length_sequence, FLAGS, dt, knn, delaunay, subsample, num_samples, transform,
    sim_data): FLAGS supplies `action_steps` and `future_sequence_length`.  Only data_path=None (an empty start, filled by add_trajectory or
    collect_observation) is provided; a path raises NotImplementedError, as data_utils.get_data_traj does for files.

    Sample `idx` of a data set with input sequence length H and future sequence length F is (trajectory j, time index t): trajectory j
    contributes T_j - H - F + 1 samples, t = H + (idx - the samples in front of j), the reference's table and lookup.  DIFFERENT from the
    reference: a trajectory shorter than H + F contributes NO samples (the reference's negative length corrupts its cumulative table).
    set_future_sequence_length(F) recomputes the table; so does the reference's own spelling, `ds._future_sequence_length = F` followed by
    `ds._compute_cumulative_lengths()`, which is what its curriculum does.

    The first trajectory fixes the store's device and dtype; later ones are converted to them.  Results are views or fresh tensors on that
    device.  An epoch in flight (batches()) and the views of val_item stay valid while trajectories are appended; replacing the last
    trajectory (collect_observation(first=False)) rewrites its rows in place."""

    def __init__(self, data_path, input_length_sequence, FLAGS, dt=1., knn=3, delaunay=False, subsample=False, num_samples=300, transform=None,
                 sim_data=True):
        if data_path is not None:
            raise NotImplementedError("SamplesClothSimDataset: only data_path=None (an empty start; add_trajectory / collect_observation fill "
                                      "it) is provided; loading trajectory files is host-side plumbing and out of scope")
        H = int(input_length_sequence)
        if not 1 <= H <= 16:
            raise ValueError(f"SamplesClothSimDataset: input_length_sequence is an integer in 1 .. 16, got {input_length_sequence!r}")
        self._dt, self.k, self.delaunay, self.subsample, self.num_samples = dt, knn, delaunay, subsample, num_samples
        self._input_length_sequence = H
        self._action_steps = FLAGS.action_steps
        self._future_sequence_length = int(FLAGS.future_sequence_length)
        self.sim_data, self.transform = sim_data, transform
        self.load_keys = ["pos", "actions", "gripper_pos", "pick", "place"]
        self.sampled_point_indeces = None
        self.device = self.dtype = None
        self._buf = {"pos": None, "velocity": None, "node_type": None, "actions": None, "edges": None}
        self._rows = self._frames = self._n_edges = 0
        self._table = np.zeros((0, TABLE_WORDS), np.int64)          # the host's copy of the per-trajectory table
        self._table_dev = None
        self._extras = []                                           # per trajectory: what add_trajectory was given beside the stored arrays
        self.allocations = 0                                        # (tests: appending must not allocate while the capacity suffices)
        self._compute_cumulative_lengths()

    # ---- the store ------------------------------------------------------------------------------------------------------------------
    def _reserve(self, name, need, tail, dtype):
        buf = self._buf[name]
        if buf is None or buf.shape[0] < need:
            cap = max(need, MIN_CAPACITY, 2 * (0 if buf is None else int(buf.shape[0])))
            new = torch.empty((cap,) + tail, dtype=dtype, device=self.device)
            live = {"pos": self._rows, "velocity": self._rows, "node_type": self._rows, "actions": self._frames, "edges": 2 * self._n_edges}[name]
            if buf is not None and live:
                new[:live].copy_(buf[:live])
            self._buf[name] = new
            self.allocations += 1
        return self._buf[name]

    def _pop_last(self):
        if len(self._table):
            last = self._table[-1]
            self._rows, self._frames, self._n_edges = int(last[NODE_BASE]), int(last[FRAME_BASE]), int(last[EDGE_BASE])
            self._table = self._table[:-1]
            self._extras.pop()

    def add_trajectory(self, d, symmetric=True):
        """Append one trajectory: a dictionary as data_utils.get_data_traj / process_traj return it -- pos, velocity [T,N,3], node_type
        [T,N,1], edge_index [T,2,E] (or [2,E]) and / or edge_faces [T,3,M] (or [3,M]) -- plus actions [T,3] and grasped_particle (an int;
        outside 0 .. N-1: no grasped node).  Tensors or numpy arrays.  The network's edges, stored once per trajectory: with edge_faces,
        face_to_edge(faces, N); otherwise edge_index[0] made symmetric (both directions, sorted by (row, col), duplicates removed: the
        layout FaceToEdge yields); symmetric=False takes edge_index[0] as given.  Every other entry of `d` is kept and comes back from
        trajectory(j).  Returns the trajectory's number."""
        what = "add_trajectory"
        for key in ("pos", "velocity", "node_type", "actions", "grasped_particle"):
            if key not in d:
                raise ValueError(f"{what}: the trajectory lacks `{key}`")
        pos = torch.as_tensor(d["pos"]).detach()
        if not pos.dtype.is_floating_point or pos.dim() != 3 or pos.shape[2] != 3 or pos.shape[0] < 1 or pos.shape[1] < 1:
            raise ValueError(f"{what}: `pos` is a floating point [T,N,3] with T, N >= 1, got {pos.dtype} {tuple(pos.shape)}")
        T, N = int(pos.shape[0]), int(pos.shape[1])
        vel, nt, act = (torch.as_tensor(d[k]).detach() for k in ("velocity", "node_type", "actions"))
        if tuple(vel.shape) != (T, N, 3) or nt.numel() != T * N or tuple(act.shape) != (T, 3):
            raise ValueError(f"{what}: next to pos [{T},{N},3], velocity is [T,N,3], node_type [T,N,1] and actions [T,3]; got "
                             f"{tuple(vel.shape)}, {tuple(nt.shape)}, {tuple(act.shape)}")
        g = d["grasped_particle"]
        if isinstance(g, bool) or not isinstance(g, (int, np.integer)):
            raise ValueError(f"{what}: `grasped_particle` is an int, got {type(g).__name__}")
        faces = d.get("edge_faces")
        if faces is None and d.get("edge_index") is None:
            raise ValueError(f"{what}: the trajectory needs `edge_faces` or `edge_index`")
        if self.device is None:
            self.device, self.dtype = pos.device, pos.dtype
        dev = self.device
        if faces is not None:
            faces = faces[0] if faces.ndim == 3 else faces
            faces = torch.as_tensor(np.array(faces) if isinstance(faces, np.ndarray) else faces).detach().to(dev)
            ei = face_to_edge(faces, N)
        else:
            ei = d["edge_index"] if torch.is_tensor(d["edge_index"]) else np.asarray(d["edge_index"])
            ei = ei[0] if ei.ndim == 3 else ei
            ei = _du._checked_edges(ei if torch.is_tensor(ei) else torch.from_numpy(np.array(ei)), N, dev, what)      # (numpy: a copy)
            if symmetric:
                ei = symmetric_edges(ei, N)
        E = int(ei.shape[1])
        rows, frames, n_edges = self._rows + T * N, self._frames + T, self._n_edges + E
        if max(rows, frames, n_edges) >= 2 ** 31:
            raise ValueError(f"{what}: the store's node rows, frames and edges must each stay below 2^31")
        cast = dict(device=dev, dtype=self.dtype)
        self._reserve("pos", rows, (3,), self.dtype)[self._rows:rows].copy_(pos.reshape(T * N, 3).to(**cast))
        self._reserve("velocity", rows, (3,), self.dtype)[self._rows:rows].copy_(vel.reshape(T * N, 3).to(**cast))
        self._reserve("node_type", rows, (), self.dtype)[self._rows:rows].copy_(nt.reshape(T * N).to(**cast))
        self._reserve("actions", frames, (3,), self.dtype)[self._frames:frames].copy_(act.to(**cast))
        self._reserve("edges", 2 * n_edges, (), torch.int64)[2 * self._n_edges:2 * n_edges].copy_(ei.reshape(-1))
        row = np.array([[self._rows, self._frames, self._n_edges, N, E, T, int(g), 0]], np.int64)
        self._table = np.concatenate([self._table, row])
        self._table_dev = torch.from_numpy(self._table.copy()).to(dev)
        self._rows, self._frames, self._n_edges = rows, frames, n_edges
        stored = ("pos", "velocity", "node_type", "actions", "grasped_particle", "edge_index", "edge_faces")
        self._extras.append(dict({k: v for k, v in d.items() if k not in stored}, faces=faces))
        self._compute_cumulative_lengths()
        return len(self._table) - 1

    def __bool__(self):
        return True

    @property
    def num_trajectories(self):
        return len(self._table)

    def trajectory(self, j):
        """trajectory j as views of the store: pos, velocity [T,N,3], node_type [T,N,1], actions [T,3], edge_index [2,E] (the network's
        edges), grasped_particle, faces ([3,M] or None), and whatever else add_trajectory was given (pick, place, gt_pos ...)"""
        j = int(j)
        if not 0 <= j < len(self._table):
            raise IndexError(f"trajectory: {j} is outside 0 .. {len(self._table) - 1}")
        nb, fb, eb, N, E, T, g = (int(v) for v in self._table[j][:7])
        b = self._buf
        out = dict(self._extras[j])
        out.update(pos=b["pos"][nb:nb + T * N].view(T, N, 3), velocity=b["velocity"][nb:nb + T * N].view(T, N, 3),
                   node_type=b["node_type"][nb:nb + T * N].view(T, N, 1), actions=b["actions"][fb:fb + T],
                   edge_index=b["edges"][2 * eb:2 * (eb + E)].view(2, E), grasped_particle=g)
        return out

    # ---- the index table ------------------------------------------------------------------------------------------------------------
    def _compute_cumulative_lengths(self):
        """the table of dataloader.py:40-48 from the current _input_length_sequence and _future_sequence_length (a trajectory shorter
        than their sum contributes none)"""
        H, F = int(self._input_length_sequence), int(self._future_sequence_length)
        if F < 1:
            raise ValueError(f"SamplesClothSimDataset: future_sequence_length is an integer >= 1, got {self._future_sequence_length!r}")
        self._data_lengths = [max(int(T) - H - F + 1, 0) for T in self._table[:, T_T]]
        self._length = int(sum(self._data_lengths))
        self._precompute_cumlengths = np.cumsum(np.asarray(self._data_lengths, dtype=np.int64)).astype(np.int64)
        self._table_future = F

    def set_future_sequence_length(self, future_sequence_length):
        self._future_sequence_length = int(future_sequence_length)
        self._compute_cumulative_lengths()

    def __len__(self):
        return self._length

    def _indices(self, indices, what):
        """a host sequence, numpy array or CPU tensor of sample numbers -> int64 numpy [B], every one inside 0 .. len-1"""
        if torch.is_tensor(indices):
            if indices.is_cuda:
                raise ValueError(f"{what}: `indices` is a host sequence, numpy array or CPU tensor -- the sizes of the outputs depend on it, so an "
                                 "index tensor on the GPU would need a blocking read; keep the indices on the host")
            indices = indices.detach().numpy()
        idx = np.asarray(indices)
        if idx.dtype == bool or not (np.issubdtype(idx.dtype, np.integer) or idx.size == 0):
            raise ValueError(f"{what}: `indices` holds integers, got {idx.dtype}")
        idx = idx.reshape(-1).astype(np.int64)
        if idx.size and (int(idx.min()) < 0 or int(idx.max()) >= self._length):
            raise IndexError(f"{what}: sample {int(idx.min()) if int(idx.min()) < 0 else int(idx.max())} is outside 0 .. {self._length - 1}")
        return idx

    def locate(self, indices):
        """(trajectory, time index) of every sample number, as int64 numpy arrays: the lookup of dataloader_sim.py:152-158"""
        idx = self._indices(indices, "locate")
        cum = self._precompute_cumlengths
        j = np.searchsorted(cum - 1, idx, side="left")
        start = np.where(j > 0, cum[np.maximum(j - 1, 0)], 0) if idx.size else idx
        return j.astype(np.int64), self._input_length_sequence + (idx - start)

    # ---- batches --------------------------------------------------------------------------------------------------------------------
    def _plan(self, idx, what):
        """the descriptors of one batch, on the host: [desc int32 [B][4] | ptr [B+1] | grasped_rows [B] | padding to an even count] as
        int64 words -- the descriptor block first and every batch an even number of words, so that it stays 16-byte aligned inside an
        epoch's buffer"""
        H, F = self._input_length_sequence, int(self._future_sequence_length)
        if F != self._table_future:
            raise ValueError(f"{what}: _future_sequence_length changed to {F} after the index table was computed for {self._table_future}; call "
                             "_compute_cumulative_lengths() (or set_future_sequence_length)")
        j, t = self.locate(idx)
        B = int(j.shape[0])
        N, E, T, g = (self._table[j, c] for c in (T_N, T_E, T_T, T_G))
        if B and (int((t - H).min()) < 0 or bool((t + F > T).any())):
            raise ValueError(f"{what}: a sample's window leaves its trajectory")          # (unreachable through the table)
        ptr = np.zeros(B + 1, np.int64)
        eptr = np.zeros(B + 1, np.int64)
        np.cumsum(N, out=ptr[1:])
        np.cumsum(E, out=eptr[1:])
        if ptr[-1] * 3 * max(H, F) >= 2 ** 31 or eptr[-1] >= 2 ** 29 or B * 3 * F >= 2 ** 31:
            raise ValueError(f"{what}: the batch's rows * 3H, rows * 3F and 4 * edges must stay below 2^31")
        grasped_rows = np.where((g >= 0) & (g < N), ptr[:-1] + g, -1)
        words = np.zeros(4 * B + 2, np.int64)
        desc = words[:2 * B].view(np.int32).reshape(B, 4)
        desc[:, 0], desc[:, 1], desc[:, 2], desc[:, 3] = j, t, ptr[:-1], eptr[:-1]
        words[2 * B:3 * B + 1] = ptr
        words[3 * B + 1:4 * B + 1] = grasped_rows
        max_items = int((N * (3 * H + 4 + 9 * F) + E).max()) if B else 0
        return _Plan(B, j, t, ptr, eptr, grasped_rows, max_items, words)

    def _upload(self, words):
        t = torch.from_numpy(words)
        if self.device is not None and self.device.type == "cuda":
            return t.pin_memory().to(self.device, non_blocking=True)          # the one host-to-device copy
        return t

    def _override(self, candidate_actions, B, what):
        if candidate_actions is None:
            return None
        F = int(self._future_sequence_length)
        a = torch.as_tensor(candidate_actions).detach()
        if tuple(a.shape) != (B, F, 3) or not a.dtype.is_floating_point:
            raise ValueError(f"{what}: `candidate_actions` is a floating point [{B},{F},3] (one [future_sequence_length,3] per sample), got "
                             f"{a.dtype} {tuple(a.shape)}")
        return a.to(device=self.device, dtype=self.dtype).contiguous()

    def _assemble(self, plan, words, override, what):
        """one Batch from a plan and its uploaded words"""
        H, F, B = self._input_length_sequence, int(self._future_sequence_length), plan.B
        R, Q = int(plan.ptr[-1]), int(plan.eptr[-1])
        dev, dt = self.device, self.dtype
        ptr, grasped_rows = words[2 * B:3 * B + 1], words[3 * B + 1:4 * B + 1]
        if dev is not None and dev.type == "cuda":
            if dt == torch.float32:
                f32 = dict(dtype=torch.float32, device=dev)
                velocity, node_types, positions = torch.empty(R, 3 * H, **f32), torch.empty(R, 1, **f32), torch.empty(R, 3, **f32)
                target, pos_target, actions = torch.empty(R, F, 3, **f32), torch.empty(R, F, 3, **f32), torch.empty(R, F, 3, **f32)
                edge_index, edge_features = torch.empty(2, Q, dtype=torch.int64, device=dev), torch.empty(Q, 4, **f32)
                if B and (R or Q):
                    b = self._buf
                    _n.launch("csplat_dataset_batch", dev, B, H, F, len(self._table), self._rows, self._frames, self._n_edges, _n.ptr(b["pos"]),
                              _n.ptr(b["velocity"]), _n.ptr(b["node_type"]), _n.ptr(b["actions"]), _n.ptr(b["edges"]), _n.ptr(self._table_dev),
                              _n.ptr(words[:2 * B]), _n.ptr(override), R, Q, plan.max_items, _n.ptr(velocity), _n.ptr(node_types),
                              _n.ptr(positions), _n.ptr(target), _n.ptr(pos_target), _n.ptr(actions), _n.ptr(edge_index) if Q else None,
                              _n.ptr(edge_features) if Q else None)
                return Batch(velocity, node_types, edge_index, edge_features, target, actions, positions, pos_target, ptr, grasped_rows)
            _n.composed_fallback(f"dataloader_sim.{what}", "dtype", self._buf["pos"])
        parts = [self._sample_composed(int(plan.j[b]), int(plan.t[b]), None if override is None else override[b]) for b in range(B)]
        if not parts:
            e = dict(dtype=dt or torch.float32, device=dev)
            return Batch(torch.empty(0, 3 * H, **e), torch.empty(0, 1, **e), torch.empty(2, 0, dtype=torch.int64, device=dev), torch.empty(0, 4, **e),
                         torch.empty(0, F, 3, **e), torch.empty(0, F, 3, **e), torch.empty(0, 3, **e), torch.empty(0, F, 3, **e), ptr, grasped_rows)
        cat = lambda i: torch.cat([p[i] for p in parts], 0)  # noqa: E731
        edge_index = torch.cat([p[2] + int(r) for p, r in zip(parts, plan.ptr[:-1])], 1)
        return Batch(cat(0), cat(1), edge_index, cat(3), cat(4), cat(5), cat(6), cat(7), ptr, grasped_rows)

    def _sample_composed(self, j, t, override):
        """the definitions of csplat_dataset_batch for one sample from torch operations, in the store's dtype"""
        H, F = self._input_length_sequence, int(self._future_sequence_length)
        tr = self.trajectory(j)
        P, V, g, ei = tr["pos"], tr["velocity"], tr["grasped_particle"], tr["edge_index"]
        N = int(P.shape[1])
        grasped = 0 <= g < N
        a = tr["actions"][t - 1:t - 1 + F] if override is None else override
        velocity = V[t - H:t].permute(1, 0, 2).reshape(N, 3 * H).clone()
        positions = P[t - 1].clone()
        actions = torch.zeros(N, F, 3, dtype=P.dtype, device=P.device)
        if grasped:
            velocity[g, 3 * (H - 1):] = V[t, g]
            positions[g] = positions[g] + a[0]
            actions[g] = a
        d = positions[ei[0]] - positions[ei[1]]
        edge_features = torch.cat([d, _edge_length(d)[:, None]], 1)
        return (velocity, tr["node_type"][t - 1].clone(), ei, edge_features, V[t:t + F].permute(1, 0, 2).contiguous(), actions, positions,
                P[t:t + F].permute(1, 0, 2).contiguous())

    def batch(self, indices, candidate_actions=None):
        """The samples `indices` (a host sequence, numpy array or CPU tensor of sample numbers; repeats allowed) as ONE block-diagonal
        Batch.  For sample (j, t), H = input sequence length, F = future sequence length, g the grasped node, a[f] = actions_j[t - 1 + f]
        (or candidate_actions[b][f] when given, [B,F,3]):
          velocity = vel_j[t-H .. t-1] side by side, oldest first; the grasped row's last three columns are vel_j[t][g] (the reference's
                     _data_to_graph: the grasped node already carries its target velocity)
          node_types = node_type_j[t-1];  positions = pos_j[t-1], the grasped row moved by a[0]
          target_velocities[:, f] = vel_j[t+f],  pos_target[:, f] = pos_j[t+f];  particle_actions = 0, the grasped row a
          edge_index = the trajectory's edges plus the sample's first row;  edge_features = (p[row] - p[col], length) on `positions`,
                     bit-equal to meshnet.rollout.edge_features(positions, edge_index)
        On a float32 GPU store: the descriptors are built with numpy and uploaded in one non-blocking copy, then one launch
        (csplat_dataset_batch); nothing is read back.  A GPU index tensor raises ValueError, an index outside 0 .. len-1 IndexError."""
        what = "batch"
        plan = self._plan(self._indices(indices, what), what)
        return self._assemble(plan, self._upload(plan.words), self._override(candidate_actions, plan.B, what), what)

    def __getitem__(self, idx):
        if isinstance(idx, bool) or not isinstance(idx, (int, np.integer)):
            raise TypeError(f"SamplesClothSimDataset: a sample number is an int, got {type(idx).__name__} (several: batch(indices))")
        return self.batch([int(idx)])

    def batches(self, batch_size, shuffle=True, generator=None, drop_last=False):
        """One epoch as a generator of Batches of `batch_size` samples (the last one shorter unless drop_last): the order is
        torch.randperm(len, generator=generator) when `shuffle`, else ascending.  The descriptors of the WHOLE epoch are built and
        uploaded once, at the first batch; every batch afterwards is one launch with no further host-to-device traffic."""
        what = "batches"
        if isinstance(batch_size, bool) or not isinstance(batch_size, (int, np.integer)) or batch_size < 1:
            raise ValueError(f"{what}: batch_size is an integer >= 1, got {batch_size!r}")
        n, bs = len(self), int(batch_size)
        order = torch.randperm(n, generator=generator).numpy() if shuffle else np.arange(n, dtype=np.int64)
        stop = n - n % bs if drop_last else n
        plans = [self._plan(self._indices(order[lo:min(lo + bs, stop)], what), what) for lo in range(0, stop, bs)]
        if not plans:
            return
        words = self._upload(np.concatenate([p.words for p in plans]))
        at = 0
        for p in plans:
            yield self._assemble(p, words[at:at + len(p.words)], None, what)
            at += len(p.words)

    def get_batch_with_candidate_actions(self, idx, candidate_actions):
        """A copies of sample `idx`, copy b with candidate_actions[b] ([A,F,3], F = future sequence length) in place of the stored
        actions: the reference's Batch.from_data_list of A _data_to_graph calls, in one launch.  -> CandidateSamples: the Batch and the
        fields of meshnet.mpc.CandidateBatch.  As in the reference's graphs, `pos` has the grasped node already moved by its candidate's
        first action and the grasped row of the newest history slot holds vel[t][g]."""
        what = "get_batch_with_candidate_actions"
        if isinstance(idx, bool) or not isinstance(idx, (int, np.integer)):
            raise ValueError(f"{what}: `idx` is one sample number, got {type(idx).__name__}")
        a = torch.as_tensor(candidate_actions)
        if a.dim() != 3 or a.shape[0] < 1:
            raise ValueError(f"{what}: `candidate_actions` is [A,F,3] with A >= 1, got {tuple(a.shape)}")
        A, H = int(a.shape[0]), self._input_length_sequence
        b = self.batch(np.full(A, int(idx), np.int64), a)
        R = int(b.velocity.shape[0])
        N = R // A
        hist = b.velocity.view(R, H, 3).permute(1, 0, 2).contiguous()
        which = torch.arange(A, dtype=torch.int64, device=b.velocity.device).repeat_interleave(N)
        return CandidateSamples(*b, pos=b.positions, hist=hist, node_type=b.node_types, batch=which, B=A, N=N)

    # ---- validation and the online trajectory ---------------------------------------------------------------------------------------
    def __get_val_item__(self, idx, future=1):
        """The reference's validation item (:186-246) for sample `idx`, as VIEWS of the store: with (j, t) the sample and
        end = min(t + future, T - 1) -- or, for future = -1, t = H and end = T, the whole trajectory --
          pos = pos_j[t-1 : end], vel = vel_j[t-H : end], actions = actions_j[t-1 : end-1], node_type = node_type_j[t-1] [N,1],
          edge_index [2,E] (the network's edges), faces ([3,M] or None), grasped_particle
        so that vel[:H] is the rollout's initial history, pos[0] its first cloud, len(actions) its number of steps and pos[1:] their
        ground truth."""
        what = "__get_val_item__"
        if isinstance(future, bool) or not isinstance(future, (int, np.integer)) or future < -1:
            raise ValueError(f"{what}: future is an integer >= -1, got {future!r}")
        j, t = self.locate([idx])
        tr = self.trajectory(int(j[0]))
        H, T = self._input_length_sequence, int(tr["pos"].shape[0])
        if future == -1:
            t, past, end = H, 0, T
        else:
            t = int(t[0])
            past, end = t - H, min(t + int(future), T - 1)
        return {"pos": tr["pos"][t - 1:end], "vel": tr["velocity"][past:end], "actions": tr["actions"][t - 1:max(end - 1, t - 1)],
                "node_type": tr["node_type"][t - 1], "edge_index": tr["edge_index"], "faces": tr["faces"],
                "grasped_particle": tr["grasped_particle"]}

    val_item = __get_val_item__

    def collect_observation(self, observation, first=False, modality="gt", rw_processing=False):
        """The reference's collect_observation (:290-348) for the one online trajectory of a closed loop: data_utils.get_data_traj on the
        observation (with the sampled points of the first call), then the trajectory is appended when `first`, else it REPLACES the last
        one.  -> get_goal_fold(frame 0, pick, place).  The trajectory keeps `gt_pos` / `gt_vel`, copies of what the observation gave.
        modality 'cloth_splatting' / 'open_loop' substitutes observation['refined_pos'] / ['predicted_pos'] ([T,N,3], the frames of the
        observation) for the positions from frame H-1 on -- the frames in front are the repetitions of the first one -- and their plain
        differences for the velocities from frame H on.  Kept from the reference: those differences are NOT divided by dt.  The kNN
        edges of get_data_traj (each undirected pair once) are made symmetric, as FaceToEdge makes the reference's."""
        what = "collect_observation"
        if modality not in ("gt", "cloth_splatting", "open_loop"):
            raise ValueError(f"{what}: modality is 'gt', 'cloth_splatting' or 'open_loop', got {modality!r}")
        if not first and (not len(self._table) or self.sampled_point_indeces is None):
            raise ValueError(f"{what}: the first observation of a trajectory is collected with first=True")
        H = self._input_length_sequence
        params = (self._dt, self.k, self.delaunay, self.subsample, self.num_samples, H, self._action_steps)
        td = _du.get_data_traj(None, self.load_keys, params, observations=observation, sim_data=self.sim_data,
                               sampled_points_indices=None if first else self.sampled_point_indeces, rw_processing=rw_processing)
        goal = get_goal_fold(td["pos"][0], td["pick"], td["place"])
        td["gt_pos"], td["gt_vel"] = td["pos"].clone(), td["velocity"].clone()
        if modality != "gt":
            key = "refined_pos" if modality == "cloth_splatting" else "predicted_pos"
            if key not in observation:
                raise ValueError(f"{what}: modality {modality!r} needs observation['{key}']")
            new = torch.as_tensor(observation[key]).detach().to(device=td["pos"].device, dtype=td["pos"].dtype)
            if tuple(new.shape) != tuple(td["pos"][H - 1:].shape):
                raise ValueError(f"{what}: observation['{key}'] is {list(td['pos'][H - 1:].shape)} next to this observation, got {list(new.shape)}")
            td["pos"][H - 1:] = new
            td["velocity"][H:] = new[1:] - new[:-1]                    # (the reference's: no division by dt)
        if first:
            self.sampled_point_indeces = td["sampled_point_indeces"]
        else:
            self._pop_last()
        self.add_trajectory(td)
        return goal


def rollout_errors(pos0, predictions, gt):
    """err [S]: err[s] = mean over the N x 3 components of (pos0 + predictions[0] + ... + predictions[s] - gt[s])^2 -- the per-step error
    of the reference's validate (train_meshnet_sim.py:303-308).  pos0 [N,3]; predictions [S,N,3], the predicted displacement of every
    step; gt [S,N,3], the true positions of steps 1 .. S.  float32 contiguous GPU tensors: one launch (csplat_dataset_rollout_error), a
    fixed order of sums, two runs bit-equal; anything else composes the definition in the dtype of pos0."""
    what = "rollout_errors"
    for name, t in (("pos0", pos0), ("predictions", predictions), ("gt", gt)):
        if not torch.is_tensor(t) or not t.dtype.is_floating_point:
            raise ValueError(f"{what}: `{name}` is a floating point tensor, got {getattr(t, 'dtype', type(t).__name__)}")
    if pos0.dim() != 2 or pos0.shape[1] != 3 or pos0.shape[0] < 1:
        raise ValueError(f"{what}: `pos0` is [N,3] with N >= 1, got {tuple(pos0.shape)}")
    N = int(pos0.shape[0])
    if predictions.dim() != 3 or tuple(predictions.shape[1:]) != (N, 3) or gt.shape != predictions.shape:
        raise ValueError(f"{what}: `predictions` and `gt` are [S,{N},3], got {tuple(predictions.shape)} and {tuple(gt.shape)}")
    S = int(predictions.shape[0])
    if S * N * 3 >= 2 ** 31:
        raise ValueError(f"{what}: S * N * 3 must stay below 2^31")
    if predictions.device != pos0.device or gt.device != pos0.device:
        raise ValueError(f"{what}: every tensor lives on the device of `pos0` ({pos0.device})")
    pos0, predictions, gt = pos0.detach(), predictions.detach(), gt.detach()
    if pos0.is_cuda:
        why = _n.why_not_f32c(pos0, predictions, gt)
        if why is None:
            err = torch.empty(S, dtype=torch.float32, device=pos0.device)
            if S:
                _n.launch("csplat_dataset_rollout_error", pos0.device, S, N, _n.ptr(pos0), _n.ptr(predictions), _n.ptr(gt), _n.ptr(err))
            return err
        _n.composed_fallback("dataloader_sim.rollout_errors", why, pos0, predictions, gt)
    dt = pos0.dtype
    err, at = torch.empty(S, dtype=dt, device=pos0.device), pos0
    for s in range(S):
        at = at + predictions[s].to(dt)
        d = at - gt[s].to(dt)
        err[s] = (d * d).mean()
    return err


def validate(simulator, ds, idx, future=10):
    """The reference's validate (train_meshnet_sim.py:293-308) for sample `idx` of `ds`: meshnet.rollout.rollout over the steps of
    ds.val_item(idx, future) under no_grad, then [0, err_1, ..., err_S] like the reference's `losses` -- as a tensor [S+1] on the device
    (nothing is read back), err_s = rollout_errors' mean squared distance between the rolled and the true cloud after s steps.  The
    reference draws `idx` at random until the item has `future` steps and plots; here the caller chooses and nothing is plotted."""
    from .rollout import rollout
    item = ds.val_item(idx, future)
    H, S = ds._input_length_sequence, int(item["actions"].shape[0])
    pos0 = item["pos"][0]
    if S == 0:
        return torch.zeros(1, dtype=pos0.dtype, device=pos0.device)
    with torch.no_grad():
        predictions, _final = rollout(simulator, pos0, item["vel"][:H], item["node_type"], item["edge_index"], item["actions"],
                                      item["grasped_particle"], S)
        err = rollout_errors(pos0, predictions.contiguous(), item["pos"][1:1 + S])
    return torch.cat([err.new_zeros(1), err])
