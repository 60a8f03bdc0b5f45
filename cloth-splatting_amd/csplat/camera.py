"""Camera refinement helper: a reference-style camera whose pose is a differentiable function of a small correction.

`perturbed(camera, omega, tau)` returns a shallow copy of `camera` (every attribute kept) in which world_view_transform,
full_proj_transform and camera_center follow an axis-angle rotation `omega` [3] and a translation `tau` [3] applied in the camera frame,
p_view' = R(omega) p_view + tau.  In the transposed row-vector convention of the reference cameras (scene_reconstruction/cameras.py):
    world_view_transform' = world_view_transform @ E,  E = [[R(omega)^T, 0], [tau, 1]]
    full_proj_transform'  = world_view_transform' @ Proj,  Proj = world_view_transform^-1 @ full_proj_transform (a constant)
    camera_center'        = (world_view_transform')^-1 [3, :3]
The rasterizer propagates gradients to the three tensors (include/csplat.h, csplat_view.dL_dview), so a loss through
gaussian_renderer.render() on the returned camera reaches omega and tau."""
import copy

import torch


def rotation(omega):
    """Rodrigues: the rotation matrix of the axis-angle vector omega [3] (differentiable, also at omega = 0)"""
    th2 = (omega * omega).sum()
    small = th2 < 1e-8
    th = torch.sqrt(torch.where(small, torch.ones_like(th2), th2))
    a = torch.where(small, 1.0 - th2 / 6.0, torch.sin(th) / th)
    b = torch.where(small, 0.5 - th2 / 24.0, (1.0 - torch.cos(th)) / (th * th))
    z = torch.zeros_like(omega[0])
    K = torch.stack([torch.stack([z, -omega[2], omega[1]]), torch.stack([omega[2], z, -omega[0]]),
                     torch.stack([-omega[1], omega[0], z])])
    return torch.eye(3, dtype=omega.dtype, device=omega.device) + a * K + b * (K @ K)


def perturbed(camera, omega, tau):
    wv = camera.world_view_transform
    omega = omega.to(device=wv.device, dtype=wv.dtype)
    tau = tau.to(device=wv.device, dtype=wv.dtype)
    with torch.no_grad():
        proj = torch.linalg.inv(wv) @ camera.full_proj_transform
    E = torch.cat([torch.cat([rotation(omega).T, torch.zeros(3, 1, dtype=wv.dtype, device=wv.device)], 1),
                   torch.cat([tau, torch.ones(1, dtype=wv.dtype, device=wv.device)])[None]], 0)
    wv2 = wv.detach() @ E
    out = copy.copy(camera)
    out.world_view_transform = wv2
    out.full_proj_transform = wv2 @ proj
    out.camera_center = torch.linalg.inv(wv2)[3, :3]
    return out
