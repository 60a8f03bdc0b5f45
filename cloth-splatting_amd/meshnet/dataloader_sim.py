"""Drop-in for the one function of the reference's `meshnet/dataloader_sim.py` that the planner needs: `get_goal_fold` (:12-48), the goal
cloud of a fold.  The dataset classes of that module are PyG plumbing and stay out of scope."""
import torch


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
