"""Restatement of the MeshNet sample data set in plain numpy, written from the semantics of the reference's SamplesClothSimDataset
(meshnet/dataloader_sim.py:50-425 on meshnet/dataloader.py:9-60, whose file does not parse: SURVEY.md F3) as include/csplat.h, "MeshNet
sample data set", states them -- not from its text.  Per-sample loops over Python lists, as the reference works; float32 or float64.

In float32 every value below is a gather or ONE rounded numpy operation, so batch() gives the bits csplat_dataset_batch must give.  The one
exception is the edge length, sqrt(fma(dz, dz, fma(dx, dx, dy * dy))): numpy has no fused multiply-add, so each is evaluated in float64 --
where the product of two float32 numbers is exact -- and rounded to float32.  (That rounds twice; the results differ from a true fma only
when the float64 sum lands exactly on a float32 tie, about once in 2^29 values.  The GPU tests also hold the kernel's length column against
csplat_gnn_edge_features itself.)

Trajectories are dictionaries of numpy arrays: pos, velocity [T,N,3], node_type [T,N,1], actions [T,3], edges int64 [2,E] (the network's
edges), grasped (an int; outside 0 .. N-1: none)."""
import numpy as np

FIELDS = ("velocity", "node_types", "edge_index", "edge_features", "target_velocities", "particle_actions", "positions", "pos_target")
WORKGROUP = 256      # DATASET_THREADS of csrc/csplat_dataset.hip (tests/test_dataset_cpu.py reads it from the source)


# ---------------------------------------------------------------------------------------------------------------------- the index table
def lengths(Ts, H, F):
    """samples per trajectory: T - H - F + 1, none from a trajectory shorter than H + F"""
    return [max(T - H - F + 1, 0) for T in Ts]


def locate(Ts, H, F, idx):
    """sample number -> (trajectory, time index): walk the trajectories, skipping those in front of the one that holds sample idx"""
    left = idx
    for j, n in enumerate(lengths(Ts, H, F)):
        if left < n:
            return j, H + left
        left -= n
    raise IndexError(idx)


# ---------------------------------------------------------------------------------------------------------------------- edges
def symmetric(edges, N):
    pairs = set()
    for r, c in zip(*np.asarray(edges).tolist()):
        pairs.add((r, c))
        pairs.add((c, r))
    out = sorted(pairs)
    return np.array(out, np.int64).reshape(-1, 2).T.copy()


def face_to_edge(faces, N):
    pairs = []
    for a, b, c in np.asarray(faces).T.tolist():
        pairs += [(a, b), (b, c), (a, c)]
    return symmetric(np.array(pairs, np.int64).reshape(-1, 2).T, N)


def edge_length(d):
    dx, dy, dz = d[:, 0], d[:, 1], d[:, 2]
    if d.dtype == np.float32:
        inner = (dx.astype(np.float64) * dx.astype(np.float64) + (dy * dy).astype(np.float64)).astype(np.float32)
        return np.sqrt((dz.astype(np.float64) * dz.astype(np.float64) + inner.astype(np.float64)).astype(np.float32))
    return np.sqrt(dz * dz + (dx * dx + dy * dy))


# ---------------------------------------------------------------------------------------------------------------------- samples
def sample(tr, t, H, F, dtype, actions=None):
    """the fields of one sample of trajectory `tr` at time index t; actions [F,3] replaces the stored actions"""
    P, V = tr["pos"].astype(dtype), tr["velocity"].astype(dtype)
    T, N = P.shape[:2]
    assert t - H >= 0 and t + F <= T
    g = tr["grasped"]
    a = (tr["actions"][t - 1:t - 1 + F] if actions is None else np.asarray(actions)).astype(dtype)
    velocity = np.concatenate([V[t - H + h] for h in range(H)], 1)
    positions = P[t - 1].copy()
    particle_actions = np.zeros((N, F, 3), dtype)
    if 0 <= g < N:
        velocity[g, 3 * (H - 1):] = V[t, g]
        positions[g] = positions[g] + a[0]
        particle_actions[g] = a
    ei = tr["edges"]
    d = positions[ei[0]] - positions[ei[1]]
    return {"velocity": velocity, "node_types": tr["node_type"][t - 1].astype(dtype).reshape(N, 1), "edge_index": ei.copy(),
            "edge_features": np.concatenate([d, edge_length(d)[:, None]], 1), "target_velocities": np.stack([V[t + f] for f in range(F)], 1),
            "particle_actions": particle_actions, "positions": positions, "pos_target": np.stack([P[t + f] for f in range(F)], 1)}


def batch(trajs, pairs, H, F, dtype, actions=None):
    """the block-diagonal batch of the samples `pairs` = [(trajectory, time index), ...]; actions [B,F,3] or None"""
    parts, ptr, grasped_rows = [], [0], []
    for b, (j, t) in enumerate(pairs):
        parts.append(sample(trajs[j], t, H, F, dtype, None if actions is None else actions[b]))
        N, g = trajs[j]["pos"].shape[1], trajs[j]["grasped"]
        grasped_rows.append(ptr[-1] + g if 0 <= g < N else -1)
        ptr.append(ptr[-1] + N)
    out = {}
    for k in FIELDS:
        if k == "edge_index":
            out[k] = np.concatenate([p[k] + off for p, off in zip(parts, ptr)], 1) if parts else np.zeros((2, 0), np.int64)
        else:
            out[k] = np.concatenate([p[k] for p in parts], 0)
    out["ptr"], out["grasped_rows"] = np.array(ptr, np.int64), np.array(grasped_rows, np.int64)
    return out


def val_item(tr, t, H, future):
    T = tr["pos"].shape[0]
    if future == -1:
        t, past, end = H, 0, T
    else:
        past, end = t - H, min(t + future, T - 1)
    return {"pos": tr["pos"][t - 1:end], "vel": tr["velocity"][past:end], "actions": tr["actions"][t - 1:max(end - 1, t - 1)],
            "node_type": tr["node_type"][t - 1], "edge_index": tr["edges"], "grasped_particle": tr["grasped"]}


def substitute(pos, velocity, new, H):
    """collect_observation's 'cloth_splatting' / 'open_loop': positions from frame H-1 on, plain differences from frame H on"""
    pos, velocity = pos.copy(), velocity.copy()
    pos[H - 1:] = new
    velocity[H:] = new[1:] - new[:-1]
    return pos, velocity


def rollout_errors(pos0, pred, gt, dtype):
    pos0, pred, gt = (np.asarray(a).astype(dtype) for a in (pos0, pred, gt))
    at, err = pos0, []
    for s in range(pred.shape[0]):
        at = at + pred[s]
        d = at - gt[s]
        err.append((d * d).mean(dtype=dtype))
    return np.array(err, dtype)


# ---------------------------------------------------------------------------------------------------------------------- test data
def random_edges(N, E, rng):
    """E directed edges, self loops and duplicates among them (whenever E >= 3)"""
    ei = rng.integers(0, N, (2, E)).astype(np.int64)
    if E >= 3:
        ei[:, 1] = ei[:, 0]                      # a duplicate
        ei[1, 2] = ei[0, 2]                      # a self loop
    return ei


def trajectory(T, N, E, grasped, seed, dtype=np.float32):
    """a cloth-like trajectory: positions of order 1 drifting by steps of order 1e-2, velocities their differences times 20"""
    rng = np.random.default_rng(seed)
    pos = (rng.uniform(-1, 1, (1, N, 3)) + np.cumsum(rng.normal(0, 1e-2, (T, N, 3)), 0)).astype(dtype)
    vel = np.zeros_like(pos)
    vel[1:] = (pos[1:] - pos[:-1]) * dtype(20.0)
    node_type = np.zeros((T, N, 1), dtype)
    if 0 <= grasped < N:
        node_type[:, grasped] = 1
    return {"pos": pos, "velocity": vel, "node_type": node_type, "actions": rng.normal(0, 1e-2, (T, 3)).astype(dtype),
            "edges": random_edges(N, E, rng), "grasped": int(grasped)}


def as_input(tr):
    """the dictionary add_trajectory takes (edges as given: pass symmetric=False)"""
    T, E = tr["pos"].shape[0], tr["edges"].shape[1]
    return {"pos": tr["pos"], "velocity": tr["velocity"], "node_type": tr["node_type"], "actions": tr["actions"],
            "edge_index": np.broadcast_to(tr["edges"][None], (T, 2, E)), "grasped_particle": tr["grasped"]}
