"""Numpy restatement of the trajectory preprocessing (include/csplat.h, "Trajectory preprocessing"; meshnet/data_utils.py and
meshnet/dataloader_sim.py).  No SciPy.

The neighbour SELECTION is stated in the kernel's own float32 arithmetic -- d = candidate - point, dx*dx + dy*dy + dz*dz, a stable argsort,
so ties go to the smaller index -- and the VALUES (weights, weighted means, velocities, edge features) are evaluated in float32 and in
float64 on that same selection: the two differ in rounding alone, never in which points they average."""
import numpy as np

FLT_MAX = float(np.finfo(np.float32).max)


def jittered_grid(nx=12, ny=11, T=3, spacing=0.05, jitter=0.004, seed=0):
    """[T, nx * ny, 3] float64: a grid in xy with uniform jitter, a sine in z, later frames drift and ripple a little (the input of
    tests/golden/trajectory_reference.npz; tools/make_trajectory_golden.py imports this function)"""
    rng = np.random.default_rng(seed)
    gx, gy = np.meshgrid(np.arange(nx) * spacing, np.arange(ny) * spacing, indexing="ij")
    xy = np.stack([gx.ravel(), gy.ravel()], 1) + rng.uniform(-jitter, jitter, (nx * ny, 2))
    frames = []
    for t in range(T):
        z = 0.02 * np.sin(8.0 * xy[:, 0] + 0.6 * t) * np.cos(5.0 * xy[:, 1])
        shift = np.array([0.003 * t, -0.002 * t, 0.0])
        frames.append(np.concatenate([xy, z[:, None]], 1) + shift + rng.uniform(-0.0005, 0.0005, (nx * ny, 3)) * (t > 0))
    return np.stack(frames)


def grid_edges(nx=12, ny=11, E=221):
    """[2,E] int64: the 4-neighbour edges of the grid, each once as (i, j) with i < j, in ascending order; the first E of them (12 x 11 has
    241; 221 is the edge count of the shape table in process_traj's tests)"""
    idx = np.arange(nx * ny).reshape(nx, ny)
    pairs = np.concatenate([np.stack([idx[:-1].ravel(), idx[1:].ravel()], 1), np.stack([idx[:, :-1].ravel(), idx[:, 1:].ravel()], 1)])
    pairs = pairs[np.lexsort((pairs[:, 1], pairs[:, 0]))][:E]
    return np.ascontiguousarray(pairs.T).astype(np.int64)


def sq_dists(X, dtype):
    """[N,N]: row i holds the squared distances of every candidate j to point i, d = candidate - point, each operation rounded to dtype"""
    X = np.asarray(X, dtype)
    with np.errstate(invalid="ignore", over="ignore"):
        d = X[None, :, :] - X[:, None, :]
        return d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]


def select(X, k, dtype=np.float32):
    """(d2 [N,k] dtype, idx [N,k] int64) of one frame: ascending (d2, index), a non-finite distance is nobody's neighbour, empty slots
    (+inf, -1)"""
    N = len(X)
    d2 = sq_dists(X, dtype)
    d2 = np.where(np.isfinite(d2), d2, np.inf).astype(dtype)
    order = np.argsort(d2, axis=1, kind="stable")[:, :k]
    near = np.take_along_axis(d2, order, 1)
    out_d = np.full((N, k), np.inf, dtype)
    out_i = np.full((N, k), -1, np.int64)
    kk = min(k, N)
    out_d[:, :kk] = near
    out_i[:, :kk] = np.where(np.isfinite(near), order, -1)
    return out_d, out_i


def weight_scale(sigma, dtype, sigma32=True):
    s = float(np.float32(sigma)) if sigma32 else float(sigma)      # the library receives sigma as a float32 number
    c = 1.0 / (2.0 * s * s)
    return np.float32(min(c, FLT_MAX)) if dtype == np.float32 else np.float64(c)


def smooth(P, k, sigma, dtype, selection=np.float32, sigma32=True):
    """P [T,N,3] (float32 data) -> (out [T,N,3] dtype, d2 [T,N,k] float32-selection distances, idx [T,N,k]): the values in `dtype` on the
    selection made in `selection` arithmetic.  The sum runs over the list in its order and begins with its first term.  sigma32: sigma
    is the float32 number the library receives (False: the double as given, what the composed float64 path of the Python surface takes)."""
    P = np.asarray(P)
    T, N, _ = P.shape
    c = weight_scale(sigma, dtype, sigma32)
    out = P.astype(dtype).copy()
    D2 = np.full((T, N, k), np.inf, selection)
    IDX = np.full((T, N, k), -1, np.int64)
    for t in range(T):
        X = P[t].astype(dtype)
        d2s, idx = select(P[t], k, selection)
        D2[t], IDX[t] = d2s, idx
        if N == 0:
            continue
        valid = idx >= 0
        nb = X[np.maximum(idx, 0)]                                   # [N,k,3]
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            d = nb - X[:, None, :]
            d2 = d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]
            w = np.exp(-(d2 * c)).astype(dtype)
            term = w[..., None] * nb
            acc, sw = term[:, 0], w[:, 0]
            for j in range(1, k):
                acc = np.where(valid[:, j, None], acc + term[:, j], acc)
                sw = np.where(valid[:, j], sw + w[:, j], sw)
            whole = np.isfinite(X).all(1)                            # a point with a non-finite coordinate goes through unchanged
            out[t] = np.where(whole[:, None], acc / sw[:, None], X)
    return out, D2, IDX


def features(P, ei, inv_dt, dtype):
    """(vel [T,N,3], disp [T,E,3], norm [T,E,1]) in dtype: vel[0] = 0, vel[t] = (P[t] - P[t-1]) * inv_dt; disp = P[:, ei[1]] - P[:, ei[0]]"""
    P = np.asarray(P).astype(dtype)
    vel = np.zeros_like(P)
    vel[1:] = (P[1:] - P[:-1]) * dtype(inv_dt)
    disp = P[:, ei[1]] - P[:, ei[0]]
    norm = np.sqrt(disp[..., 0] * disp[..., 0] + disp[..., 1] * disp[..., 1] + disp[..., 2] * disp[..., 2])[..., None]
    return vel, disp, norm


def process_traj(P, ei, dt, dtype, sim_data=False, norm_threshold=0.01):
    """the reference's dictionary from `features`: frame 0's edge features are a copy of frame 1's (T > 1); with sim_data the edges whose
    frame-min(1, T-1) norm is >= norm_threshold go, once, in stable order"""
    T = len(P)
    vel, disp, norm = features(P, ei, 1.0 / dt, dtype)
    if sim_data:
        keep = norm[min(1, T - 1), :, 0] < norm_threshold
        ei, disp, norm = ei[:, keep], disp[:, keep], norm[:, keep]
    if T > 1:
        disp[0], norm[0] = disp[1], norm[1]
    return dict(pos=np.asarray(P).astype(dtype), velocity=vel, node_type=np.zeros((T, P.shape[1], 1), dtype), edge_index=np.broadcast_to(ei, (T,) + ei.shape),
                edge_displacement=disp, edge_norm=norm)


def goal_fold_loop(X, pick, place):
    """get_goal_fold node by node, as the reference's loop states it"""
    X = np.asarray(X)
    axis = (place - pick) / np.sqrt(((place - pick) ** 2).sum())
    mid = (pick + place) / 2
    out = X.copy()
    for i in range(len(X)):
        s = float(np.dot(X[i] - mid, axis))
        if s < 0:
            out[i] = X[i] - 2 * s * axis
    return out
