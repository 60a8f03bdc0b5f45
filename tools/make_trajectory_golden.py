"""Writes tests/golden/trajectory_reference.npz: what the REFERENCE's own gaussian_smoothing, process_traj and get_goal_fold return on a
small jittered grid (tests/trajectory_ref.py: jittered_grid, grid_edges -- 12 x 11 points, spacing 0.05, xy jitter 0.004, a sine in z, three
frames, seed 0).  tests/test_trajectory_cpu.py compares the composed float64 path of meshnet.data_utils with it.

    python tools/make_trajectory_golden.py <path to a checkout of the reference>

Needs SciPy (the reference's KD-tree) and that checkout; neither is needed to run the tests.  Nothing of the reference is stored here: its
functions are pulled out of the checkout when this runs --
  * meshnet/data_utils.py cannot be imported (torch_geometric, h5py and its own viz module are absent), so the three function
    definitions are taken out of its syntax tree (`ast`) and compiled on their own, with numpy, torch and SciPy's KDTree in their globals;
  * meshnet/dataloader_sim.py holds merge-conflict markers and does not parse, so get_goal_fold is cut out of its text: from its `def`
    line to the next top-level statement.
The reference's k-NN branch of compute_edges_index fails under this numpy (np.vstack of a set), hence the explicit edge list.
Its process_traj converts positions with `dtype=torch.float` before the edge features; the name `torch.float` is bound to float64 for
that call, so that the fixture records a float64 evaluation of the reference's formula, as for every other entry (the comparison's bar
is a float64 bar)."""
import ast
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import trajectory_ref as R  # noqa: E402

K, SIGMA, DT = 20, 0.1, 0.05


class _Torch64(types.ModuleType):
    """torch, with `float` naming float64"""

    def __getattr__(self, name):
        return torch.float64 if name == "float" else getattr(torch, name)


def functions_by_ast(path, names, env):
    tree = ast.parse(open(path).read())
    keep = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in names]
    assert sorted(n.name for n in keep) == sorted(names), [n.name for n in keep]
    exec(compile(ast.Module(body=keep, type_ignores=[]), path, "exec"), env)
    return [env[n] for n in names]


def function_by_text(path, name, env):
    lines = open(path).read().split("\n")
    first = next(i for i, ln in enumerate(lines) if ln.startswith(f"def {name}("))
    last = next(i for i in range(first + 1, len(lines)) if lines[i] and not lines[i][0].isspace())
    exec(compile("\n".join(lines[first:last]), path, "exec"), env)
    return env[name]


def main(ref):
    from scipy.spatial import KDTree
    env = {"np": np, "torch": _Torch64("torch64"), "KDTree": KDTree}
    smoothing, process, _edge = functions_by_ast(os.path.join(ref, "meshnet", "data_utils.py"),
                                                 ["gaussian_smoothing", "process_traj", "compute_edge_features"], env)
    fold = function_by_text(os.path.join(ref, "meshnet", "dataloader_sim.py"), "get_goal_fold", {"torch": torch})
    traj, ei = R.jittered_grid(), R.grid_edges()
    assert traj.shape == (3, 132, 3) and ei.shape == (2, 221) and traj.dtype == np.float64
    # no tie at the edge of any list: every point's k-th and (k+1)-th distances differ (by far more than float64 rounding)
    for X in traj:
        d = np.sort(np.sqrt(R.sq_dists(X, np.float64)), axis=1)
        gap = (d[:, K] - d[:, K - 1]).min()
        assert gap > 1e-9, gap
    # (the input itself is the entry t3_pos: the reference returns the positions as they came)
    out = {"k": np.int64(K), "sigma": np.float64(SIGMA), "dt": np.float64(DT), "edge_index": ei}
    out["smoothed"] = np.stack([smoothing(X.copy(), k=K, sigma=SIGMA) for X in traj])
    for tag, sub in (("t3", traj), ("t1", traj[:1])):
        d = process(sub.copy(), DT, edge_index=torch.from_numpy(ei), sim_data=False, faces=torch.zeros(3, 1, dtype=torch.long))
        for key in ("pos", "velocity", "node_type", "edge_index", "edge_displacement", "edge_norm", "sampled_point_indeces"):
            out[f"{tag}_{key}"] = np.asarray(d[key])
        assert out[f"{tag}_edge_displacement"].dtype == np.float64 and np.array_equal(out[f"{tag}_pos"], sub)
    del out["t1_pos"]
    pick, place = np.array([0.05, 0.02, 0.0]), np.array([0.50, 0.45, 0.01])
    out["pick"], out["place"] = pick, place
    out["goal"] = fold(torch.from_numpy(traj[0].copy()), torch.from_numpy(pick), torch.from_numpy(place)).numpy()
    assert 20 < (np.abs(out["goal"] - traj[0]).max(1) > 0).sum() < 112      # some nodes fold, some stay
    path = os.path.join(ROOT, "tests", "golden", "trajectory_reference.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes;", {k: v.shape for k, v in out.items()})
    assert os.path.getsize(path) < 64 * 1024


if __name__ == "__main__":
    main(sys.argv[1])
