"""Online refinement: the reference's SingleStepOptimizer (scene_reconstruction/train_utils.py:348-556, called from
manipulation/planning.py:258-269, 404-418).  A static reconstruction of the first frame, then, every round of the control loop, a
refinement of the mesh predictions over a time window that has grown by the round's observation; `refined_meshes()` is what
meshnet.dataloader_sim.SamplesClothSimDataset.collect_observation(modality='cloth_splatting') takes as `refined_pos`.

What feeds the steps is a csplat.camera_dataset.CameraDataset: the images stay on the device, `update_data` uploads only the cells a
round has added, and every step's ground truth is one launch.

Kept from the reference: `update_data` creates a FRESH simulator (:405-408), so the residual MLP starts anew every round, and both loops
create a fresh Adam on it; the iteration count continues from `last_iters`; the camera of iteration `it` is view `it % len(data)`; for
n_times >= 3 the step's time is drawn with weights linspace(0.5, 1.5, n_times - 2).
DEVIATION: the reference forms the triple as `time_id - 1 + i`, i = 0, 1, 2, with time_id from range(n_times - 2) (:484-487); for
time_id == 0 that indexes time -1, the LAST frame, by numpy's wrap-around.  Here the drawn value is the triple's first time: the centre is
c = time_id + 1 and the triple (c - 1, c, c + 1) -- the evident intent, and the same weights on the same number of triples.
The draws come from the `rng` (numpy Generator) given at construction, not from Python's global `random`.  The report blocks of the
loops (:429-456, :505-534) are `evaluate()`; no PNG is written."""
import os
from types import SimpleNamespace

import numpy as np
import torch

from . import train as _train
from .camera_dataset import CameraDataset
from .gaussians import MeshGaussians
from .scene_io import nerf_normalization, read_cloth_scene_info


def _positions(meshes, device):
    """[T,V,3] of a list of meshes (objects with .pos, dicts with "pos") or of a tensor / array"""
    if torch.is_tensor(meshes) or isinstance(meshes, np.ndarray):
        return torch.as_tensor(meshes, dtype=torch.float32).to(device)
    return torch.stack([torch.as_tensor(m["pos"] if isinstance(m, dict) else m.pos, dtype=torch.float32).to(device) for m in meshes])


class SingleStepOptimizer:
    def __init__(self, opt=_train.DEFAULT_OPT, pipe=_train.DEFAULT_PIPE, densify_opt=None, sh_degree=3, white_background=False,
                 gaussian_init_factor=2, n_times_max=-1, static_iterations=1000, iterations=1000, save_path=None, device="cuda", rng=None,
                 storage="auto", generator=None):
        """opt / pipe: what train_step takes (opt.meshnet_lr is the simulator's learning rate); densify_opt: the reference's
        densification schedule for the STATIC reconstruction (None: none), `cameras_extent` and `white_background` are filled in;
        static_iterations / iterations: the defaults of static_reconstruction / update_mesh_predictions (opt_params.static_reconst_iteration /
        .iterations); n_times_max: the simulator's time table length (-1: that of the mesh predictions); generator: for from_mesh."""
        self.opt, self.pipe, self.densify_opt = opt, pipe, densify_opt
        self.sh_degree, self.white_background, self.gaussian_init_factor = sh_degree, bool(white_background), gaussian_init_factor
        self.n_times_max, self.static_iterations, self.iterations = n_times_max, static_iterations, iterations
        self.save_path, self.device, self.storage, self.generator = save_path, torch.device(device), storage, generator
        self.rng = rng if rng is not None else np.random.default_rng()
        self.background = torch.tensor([1.0, 1.0, 1.0] if white_background else [0.0, 0.0, 0.0], dtype=torch.float32, device=self.device)
        self.last_iters = 0
        self.camera_data = self.gaussians = self.simulator = None
        self.cameras_extent = None

    # ---- data -------------------------------------------------------------------------------------------------------------------------
    def _new_simulator(self, mesh_predictions):
        from meshnet.meshnet_network import ResidualMeshSimulator
        self.mesh_predictions = mesh_predictions
        self.simulator = ResidualMeshSimulator(_positions(mesh_predictions, self.device), n_times=self.n_times_max, device=self.device)
        self.simulator.train()

    def initialize(self, camera_infos, initial_mesh, mesh_predictions, cameras_extent=None):
        """:380-394 on records already read: the data set, the Gaussians on the initial mesh with their optimizer, the simulator"""
        camera_infos = list(camera_infos)
        self.camera_data = CameraDataset(camera_infos, device=self.device, storage=self.storage, rng=self.rng)
        self.cameras_extent = float(nerf_normalization(camera_infos)["radius"] if cameras_extent is None else cameras_extent)
        mesh = initial_mesh if isinstance(initial_mesh, dict) else {k: getattr(initial_mesh, k) for k in ("pos", "face", "edge_index")}
        dev = self.device
        self.initial_mesh = initial_mesh
        self.gaussians = MeshGaussians(self.sh_degree).from_mesh(torch.as_tensor(mesh["pos"], dtype=torch.float32).to(dev),
                                                                  torch.as_tensor(mesh["face"]).long().to(dev),
                                                                  torch.as_tensor(mesh["edge_index"]).long().to(dev),
                                                                  self.gaussian_init_factor, generator=self.generator)
        o = self.opt
        self.gaussians.training_setup(position_lr=o.position_lr_init, feature_lr=o.feature_lr, opacity_lr=o.opacity_lr,
                                      scaling_lr=o.scaling_lr, rotation_lr=o.rotation_lr)
        self._new_simulator(mesh_predictions)
        return self

    def initialize_from_path(self, path, eval=False):
        """:380-394: read_cloth_scene_info(path, white_background, eval=False), then initialize()"""
        scene_info, initial_mesh, mesh_predictions = read_cloth_scene_info(path, self.white_background, eval=eval)
        self.scene_info = scene_info
        return self.initialize(scene_info.train_cameras, initial_mesh, mesh_predictions, scene_info.nerf_normalization["radius"])

    def update_data(self, camera_infos, mesh_predictions, n_times=-1):
        """:396-408: the round's scene.  The cells that are not in the data set yet are uploaded (the reference re-reads everything),
        n_times > 0 keeps the first n_times times and mesh predictions, and a FRESH simulator is created: its residual starts anew."""
        self.camera_data.add_frames(camera_infos)
        if n_times > 0:
            self.camera_data.truncate_times(n_times)
            mesh_predictions = mesh_predictions[:n_times]
        self._new_simulator(mesh_predictions)
        return self

    def update_data_from_path(self, path, n_times=-1):
        scene_info, _mesh, mesh_predictions = read_cloth_scene_info(path, self.white_background)
        self.scene_info = scene_info
        return self.update_data(scene_info.train_cameras, mesh_predictions, n_times)

    # ---- the two loops ----------------------------------------------------------------------------------------------------------------
    def _optimizer(self):
        return torch.optim.Adam(self.simulator.parameters(), lr=self.opt.meshnet_lr)

    def _densify_opt(self):
        if self.densify_opt is None:
            return None
        return SimpleNamespace(**{**vars(self.densify_opt), "cameras_extent": self.cameras_extent, "white_background": self.white_background})

    def static_reconstruction(self, train_steps=None):
        """:410-466: iteration it = 1 .. steps trains on the camera (it % len(data), time 0) with static=True"""
        meshnet_optimizer = self._optimizer()
        self.static_iterations = train_steps if train_steps is not None else self.static_iterations
        densify_opt = self._densify_opt()
        self.history = []
        for iteration in range(1, self.static_iterations + 1):
            cams = self.camera_data.step(iteration % len(self.camera_data), [0])
            psnr_, loss, _stats = _train.train_step(iteration, cams, self.gaussians, self.simulator, meshnet_optimizer, self.pipe, self.opt,
                                                    self.background, static=True, densify_opt=densify_opt)
            self.history.append((psnr_, loss))
        self.last_iters = self.static_iterations
        return self.gaussians, self.simulator

    def step_times(self):
        """the time positions of one refinement step (:481-496, with the deviation stated above)"""
        n_times = self.camera_data.n_times
        if n_times >= 3:
            probabilities = np.linspace(0.5, 1.5, n_times - 2)
            probabilities /= probabilities.sum()
            centre = int(self.rng.choice(n_times - 2, p=probabilities)) + 1
            return [centre - 1, centre, centre + 1]
        if n_times < 1:
            raise ValueError("No cameras to train on")
        return list(range(n_times))

    def update_mesh_predictions(self, train_steps=None):
        """:468-545: iterations last_iters + 1 .. last_iters + steps, a fresh Adam on the simulator, static=False"""
        meshnet_optimizer = self._optimizer()
        iterations = train_steps if train_steps is not None else self.iterations
        iteration = self.last_iters
        self.history = []
        for iteration in range(self.last_iters + 1, self.last_iters + iterations + 1):
            cams = self.camera_data.step(iteration % len(self.camera_data), self.step_times())
            psnr_, loss, _stats = _train.train_step(iteration, cams, self.gaussians, self.simulator, meshnet_optimizer, self.pipe, self.opt,
                                                    self.background, static=False)
            self.history.append((psnr_, loss))
        self.last_iters = iteration
        return self.gaussians, self.simulator

    # ---- results ----------------------------------------------------------------------------------------------------------------------
    def refined_meshes(self):
        """[n_times,V,3]: the simulator at every time of the data set (planning.py:410-418), on the device; nothing goes to the host"""
        times = [float(t) for t in self.camera_data.times[:self.camera_data.n_times]]
        with torch.no_grad():
            return self.simulator.forward_times(times)

    @torch.no_grad()
    def evaluate(self, n_views=3, time_id=-1):
        """the report of :429-456 / :505-534 without the PNGs: [{"view", "l1", "psnr"}] for views 0 .. n_views-1 at time position time_id
        (-1: the last)"""
        from gaussian_renderer import render
        t = time_id if time_id >= 0 else self.camera_data.n_times + time_id
        out = []
        for j in range(min(n_views, len(self.camera_data))):
            cam = self.camera_data.get_one_item(j, t)
            image = torch.clamp(render(cam, self.gaussians, self.simulator, self.pipe, self.background).render, 0.0, 1.0)
            gt = torch.clamp(cam.original_image, 0.0, 1.0)
            out.append(dict(view=j, l1=_train.l1_loss(image, gt).mean().double(), psnr=_train.psnr(image[None], gt[None]).mean().double()))
        return out

    def save(self, path=None):
        """:547-556: <path>/point_cloud/iteration_<n>/ (save_ply) and <path>/meshnet/model-<n>.pt, n = static_iterations + iterations"""
        path = path if path is not None else self.save_path
        iteration = self.static_iterations + self.iterations
        self.gaussians.save_ply(os.path.join(path, "point_cloud/iteration_{}".format(iteration)))
        meshnet_path = os.path.join(path, "meshnet")
        os.makedirs(meshnet_path, exist_ok=True)
        self.simulator.save(os.path.join(meshnet_path, "model-" + str(iteration) + ".pt"))
        return iteration
