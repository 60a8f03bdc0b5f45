"""The camera data set (csplat/camera_dataset.py), the online-refinement driver (csplat/refine.py) and the scene reader's additions
(csplat/scene_io.py) without a GPU: the grid rules against hand-written lists and the restatement tests/camera_dataset_ref.py, the storage
decisions, the composed CPU batch bit for bit against scene_io.camera_from_info, a tiny scene on disk, the driver's (view, times, static,
iteration) sequence with train_step replaced by a recorder, and the C-ABI of csplat_camera_batch: export, header block, and every refusal
through the library itself with a NULL stream and fake addresses (each is refused before a launch could touch them).

tests/test_camera_dataset_gpu.py runs the kernel; the launch constants its sizes are built from are read from the source here too
(test_launch_constants_named_in_the_source)."""
import json
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

import util  # noqa: F401
import camera_dataset_ref as R

torch = pytest.importorskip("torch")
from csplat import camera_dataset as cdm  # noqa: E402  (absent: every test of this file fails)
from csplat import refine, scene_io  # noqa: E402
from csplat.camera_dataset import CameraBatch, CameraDataset, MDNerfDataset  # noqa: E402
from csplat.scene_io import camera_from_info  # noqa: E402

ROOT = util.ROOT
SRC = os.path.join(ROOT, "cloth-splatting_amd", "csrc", "csplat_camera_dataset.hip")
VIEWS, TIMES = (3, 7, 9), (0, 2, 5)


def constants():
    code = open(SRC).read()
    return (int(re.search(r"constexpr int CAMERA_THREADS = (\d+);", code).group(1)),
            int(re.search(r"constexpr int CAMERA_PIXELS_PER_LANE = (\d+);", code).group(1)))


def bits(t):
    return t.contiguous().view(torch.int32)


def same_camera(got, want, what=""):
    """every field of scene_io.camera_from_info, tensors bit for bit"""
    for k, v in vars(want).items():
        g = getattr(got, k)
        if torch.is_tensor(v):
            assert g.dtype == v.dtype and g.shape == v.shape and torch.equal(bits(g.cpu()), bits(v.cpu())), (what, k)
        else:
            assert g == v and type(g) is type(v), (what, k, g, v)


def shuffled(views=VIEWS, times=TIMES, H=5, W=7, mask=True, seed=3, drop=()):
    infos = [R.make_info(v, t, H, W, mask, n_times=6) for v in views for t in times if (v, t) not in drop]
    order = np.random.default_rng(seed).permutation(len(infos))
    return [infos[k] for k in order]


# ------------------------------------------------------------------------------------------------------------------ the grid rules
def test_grid_is_ordered_by_the_positions_of_the_sorted_unique_ids():
    infos = shuffled()
    ds = CameraDataset(infos, device="cpu", rng=np.random.default_rng(0))
    assert MDNerfDataset is CameraDataset
    assert ds.viewpoint_ids.tolist() == [3, 7, 9] and ds.time_ids.tolist() == [0, 2, 5] and ds.times.tolist() == [0.0, 0.4, 1.0]
    assert (ds.n_viewpoints, ds.n_times, len(ds)) == (3, 3, 3)
    views, times, cells = R.grid(infos)
    assert views == [3, 7, 9] and times == [0, 2, 5]
    for v in range(3):
        for t in range(3):
            cam = ds.get_one_item(v, t)
            assert (cam.view_id, cam.time_id, cam.image_name) == (VIEWS[v], TIMES[t], f"r_{VIEWS[v]}_{TIMES[t]}")      # the RAW ids
            same_camera(cam, camera_from_info(cells[(v, t)], "cpu"), (v, t))
    for bad in ((-1, 0), (3, 0), (0, -1), (0, 3)):
        with pytest.raises(IndexError, match="outside"):
            ds.get_one_item(*bad)
    with pytest.raises(IndexError):
        ds.step(0, [0, 3])
    with pytest.raises(IndexError, match="slot"):
        ds._gather([ds.n_slots])


def test_getitem_triples_against_hand_written_lists():
    ds = CameraDataset(shuffled(), device="cpu", rng=np.random.default_rng(11))
    for v in (0, 1, 2):                                       # three times: the middle can only be 1
        assert [c.time_id for c in ds[v]] == [0, 2, 5] and [c.view_id for c in ds[v]] == [VIEWS[v]] * 3
    times5 = (0, 2, 5, 6, 9)
    ds = CameraDataset(shuffled(times=times5), device="cpu", rng=np.random.default_rng(11))
    # default_rng(11).integers(1, 4) gives 1, 1, 3, 2, 2, 2, 3, 1: the middles, uniform in [1, n_times - 2]
    want = [[0, 2, 5], [0, 2, 5], [5, 6, 9], [2, 5, 6], [2, 5, 6], [2, 5, 6], [5, 6, 9], [0, 2, 5]]
    got = [[c.time_id for c in ds[k % 3]] for k in range(8)]
    assert got == want
    rng = np.random.default_rng(11)
    assert got == [[times5[t] for t in R.item_times(5, rng)] for _ in range(8)]
    for n_times, want in ((2, [0, 2]), (1, [0])):             # fewer than three times: all of them
        ds = CameraDataset(shuffled(times=TIMES[:n_times]), device="cpu", rng=np.random.default_rng(11))
        assert [c.time_id for c in ds[1]] == want
    batch = ds[0]
    assert isinstance(batch, CameraBatch) and batch.gt.shape == (1, 3, 5, 7) and batch.mask.shape == (1, 1, 5, 7)


def test_a_missing_cell_falls_back_to_a_uniformly_chosen_view_with_that_time():
    infos = shuffled(drop={(7, 2)})
    ds = CameraDataset(infos, device="cpu", rng=np.random.default_rng(11))
    # default_rng(11).integers(2) gives 0, 0, 1, 0, 1, 1, 1, 0 over the two views (3 and 9) that have time 2
    assert [ds.get_one_item(1, 1).view_id for _ in range(8)] == [3, 3, 9, 3, 9, 9, 9, 3]
    assert ds.get_one_item(1, 0).view_id == 7                 # a cell that is there draws nothing
    views, times, cells = R.grid(infos)
    rng = np.random.default_rng(11)
    assert [R.resolve(cells, 3, 1, 1, rng).view_id for _ in range(8)] == [3, 3, 9, 3, 9, 9, 9, 3]
    assert int(ds.rng.integers(1 << 30)) == int(rng.integers(1 << 30))            # eight draws each: the generators are level
    # one view per time: each cell that is missing is served by the only view that has its time; a time nobody has is an error
    lone = [R.make_info(3, 0, 5, 7), R.make_info(7, 2, 5, 7)]
    ds = CameraDataset(lone, device="cpu", rng=np.random.default_rng(0))
    assert ds.get_one_item(0, 1).view_id == 7 and ds.get_one_item(1, 0).view_id == 3
    ds._grid[:, 1] = -1
    with pytest.raises(ValueError, match="No cam info"):
        ds.get_one_item(0, 1)


def test_truncate_times_and_add_frames_skip_present_cells():
    infos = shuffled()
    ds = CameraDataset(infos, device="cpu", rng=np.random.default_rng(0), capacity=2)
    assert ds.n_slots == 9 and ds.uploaded_cells == 9 and ds.capacity == 16               # 2 -> 4 -> 8 -> 16
    ds.truncate_times(2)
    assert ds.n_times == 2 and [c.time_id for c in ds[0]] == [0, 2] and ds.n_slots == 9
    with pytest.raises(IndexError):
        ds.get_one_item(0, 2)
    for bad in (0, 3):
        with pytest.raises(ValueError, match="truncate_times"):
            ds.truncate_times(bad)
    # the growing scene of the online loop: everything again plus one more time; only the new cells are uploaded
    more = infos + [R.make_info(v, 6, 5, 7, n_times=6) for v in VIEWS]
    store_before = ds._store[:9 * ds.planes * ds._pitch].clone()
    assert ds.add_frames(more) == 3 and ds.n_slots == 12 and ds.uploaded_cells == 12 and ds.n_times == 4
    assert torch.equal(ds._store[:9 * ds.planes * ds._pitch], store_before)
    assert ds.add_frames(more) == 0 and ds.uploaded_cells == 12
    assert ds.time_ids.tolist() == [0, 2, 5, 6] and [c.time_id for c in ds.step(2, [0, 1, 2, 3])] == [0, 2, 5, 6]
    # replace=True writes over the slot of a cell that is present
    other = R.make_info(7, 2, 5, 7, seed=9, n_times=6)
    slot = ds.get_one_item(1, 1)
    assert ds.add_frames([other]) == 0 and torch.equal(ds.get_one_item(1, 1).original_image, slot.original_image)
    assert ds.add_frames([other], replace=True) == 1 and ds.n_slots == 12
    same_camera(ds.get_one_item(1, 1), camera_from_info(other, "cpu"))
    same_camera(ds.get_one_item(1, 0), camera_from_info(R.grid(infos)[2][(1, 0)], "cpu"))


def test_size_and_mask_mismatches_raise_and_change_nothing():
    infos = shuffled()
    ds = CameraDataset(infos, device="cpu")
    for bad in (R.make_info(3, 6, 5, 8), R.make_info(3, 6, 7, 5), R.make_info(3, 6, 5, 7, mask=False)):
        with pytest.raises(ValueError, match="one size|a mask"):
            ds.add_frames([R.make_info(7, 6, 5, 7), bad])
        assert ds.n_slots == 9 and ds.n_times == 3
    with pytest.raises(ValueError, match="one size"):
        CameraDataset([R.make_info(3, 0, 5, 7), R.make_info(3, 1, 6, 7)], device="cpu")
    with pytest.raises(ValueError, match="a mask"):
        CameraDataset([R.make_info(3, 0, 5, 7, mask=False), R.make_info(3, 1, 5, 7)], device="cpu")
    with pytest.raises(ValueError, match="storage"):
        CameraDataset([], device="cpu", storage="float16")


# ------------------------------------------------------------------------------------------------------------------ storage
def all_levels():
    """[3,16,16]: all 256 levels in every channel, each channel in another order"""
    base = torch.arange(256, dtype=torch.uint8)
    return torch.stack([base, base.flip(0), base.roll(37)]).reshape(3, 16, 16)


def test_auto_storage_decisions():
    img = all_levels() / 255.0
    info = R.make_info(0, 0, 16, 16, image=img)
    ds = CameraDataset([info], device="cpu")
    assert ds.storage == "uint8" and ds._pitch == 256 and ds._store.dtype == torch.uint8
    assert torch.equal(ds._store[:3 * 256].reshape(3, 16, 16), all_levels())
    same_camera(ds.get_one_item(0, 0), camera_from_info(info, "cpu"))
    # the restatement's division is torch's; a multiply by the reciprocal is not (the issue counts 126 of the 256 levels)
    lv = np.arange(256, dtype=np.uint8)
    assert torch.equal(R.image_of(lv), torch.from_numpy(lv) / 255.0) and torch.equal(R.mask_of(lv), 1.0 - torch.from_numpy(lv) / 255.0)
    assert int((torch.from_numpy(lv).float() * np.float32(1.0 / 255.0) != R.image_of(lv)).sum()) == 126
    half = img.clone()
    half[1, 3, 4] = 0.5
    info_half = R.make_info(0, 1, 16, 16, image=half)
    ds2 = CameraDataset([info_half], device="cpu")
    assert ds2.storage == "float32" and ds2._pitch == 1024
    same_camera(ds2.get_one_item(0, 0), camera_from_info(info_half, "cpu"))
    with pytest.raises(ValueError, match="storage='uint8'"):
        CameraDataset([info_half], device="cpu", storage="uint8")
    # an exact image with a mask that is not: float32 too; -0.0 is not a level (0 / 255 is +0.0)
    odd_mask = R.mask_of(R.levels((1, 16, 16), 1))
    odd_mask[0, 0, 0] = 0.3
    assert CameraDataset([R.make_info(0, 0, 16, 16, image=img, mask_image=odd_mask)], device="cpu").storage == "float32"
    neg = img.clone()
    neg[0, 0, 0] = -0.0
    assert cdm.quantise_image(neg) is None and cdm.quantise_image(img) is not None
    assert cdm.quantise_image(torch.full((3, 2, 2), float("nan"))) is None
    assert CameraDataset([info], device="cpu", storage="float32").storage == "float32"
    # later frames that are not exact levels turn an "auto" store into float32 words; what was there keeps its bits
    ds.add_frames([info_half])
    assert ds.storage == "float32" and ds.n_slots == 2
    same_camera(ds.get_one_item(0, 0), camera_from_info(info, "cpu"))
    same_camera(ds.get_one_item(0, 1), camera_from_info(info_half, "cpu"))


# ------------------------------------------------------------------------------------------------------------------ the CPU batch
@pytest.mark.parametrize("mask", [True, False])
@pytest.mark.parametrize("storage", ["uint8", "float32"])
def test_cpu_step_is_bit_equal_to_camera_from_info(mask, storage):
    infos = shuffled(H=6, W=9, mask=mask)
    ds = CameraDataset(infos, device="cpu", storage=storage, rng=np.random.default_rng(0))
    _, _, cells = R.grid(infos)
    batch = ds.step(2, [2, 0, 0, 1])                                       # a repeat among them
    assert len(batch) == 4 and batch.gt.shape == (4, 3, 6, 9) and (batch.mask is None) == (not mask)
    for i, (cam, t) in enumerate(zip(batch, (2, 0, 0, 1))):
        same_camera(cam, camera_from_info(cells[(2, t)], "cpu"), (storage, t))
        assert cam.gt_stack is batch.gt and cam.gt_index == i and cam.mask_stack is batch.mask
        assert cam.original_image.data_ptr() == batch.gt[i].data_ptr()
    again = ds.step(2, [2, 0, 0, 1])
    assert torch.equal(bits(again.gt), bits(batch.gt)) and batch.slots == again.slots
    for a, b in zip(batch, again):                                         # the matrix tensors keep their identity across steps
        assert a.world_view_transform is b.world_view_transform and a.full_proj_transform is b.full_proj_transform and \
            a.camera_center is b.camera_center
    # plan(): the same batches, the rng consumed in the same order
    sched = [(0, [0, 1, 2]), (1, [1]), (2, [2, 1])]
    plain = [ds.step(v, t) for v, t in sched]
    ds.plan(sched)
    for (v, t), want in zip(sched, plain):
        got = ds.step(v, t)
        assert got.slots == want.slots and torch.equal(bits(got.gt), bits(want.gt))
    assert ds._plan.at == 3
    assert ds.step(0, [0]).slots == plain[0].slots[:1]                     # beyond the plan: served the usual way


def test_train_fast_paths_hand_the_batch_tensors_through():
    from csplat import train as tr
    ds = CameraDataset(shuffled(), device="cpu", rng=np.random.default_rng(0))
    batch = ds.step(0, [0, 1, 2])
    cpu = torch.device("cpu")
    assert tr._gt_stack(batch, cpu) is batch.gt
    assert tr._batch_stack(batch, "mask_stack", "mask", cpu) is batch.mask
    assert tr._batch_stack(list(batch)[::-1], "gt_stack", "original_image", cpu) is None          # another order: today's code
    assert tr._batch_stack(list(batch)[:2], "gt_stack", "original_image", cpu) is None            # a part of the batch
    plain = [camera_from_info(i, "cpu") for i in shuffled()[:3]]
    assert tr._batch_stack(plain, "gt_stack", "original_image", cpu) is None
    stack = tr._gt_stack(plain, cpu)
    assert torch.equal(stack, torch.cat([c.original_image[None] for c in plain]))
    batch[1].original_image = batch[1].original_image.clone()                                    # a camera whose image was replaced
    assert tr._batch_stack(batch, "gt_stack", "original_image", cpu) is None
    assert torch.equal(tr._gt_stack(batch, cpu), batch.gt)


# ------------------------------------------------------------------------------------------------------------------ the disk
def write_scene(path, n_views=2, n_times=3, H=6, W=8, masks=True):
    from PIL import Image
    from csplat import hdf5min, synthetic as syn
    rng = np.random.default_rng(4)
    os.makedirs(os.path.join(path, "mesh_predictions"))
    if masks:
        os.makedirs(os.path.join(path, "masks_gripper"))
    pos, faces, edge_index = syn.grid_mesh(3)
    for name, p in [("init_mesh.hdf5", pos)] + [(f"mesh_predictions/mesh_{t:03d}.hdf5", pos + 0.01 * t) for t in range(n_times)]:
        hdf5min.save(os.path.join(path, name), {"pos": p.astype(np.float32), "norm": np.zeros_like(pos), "face": faces.T.copy(),
                                                "edge_index": edge_index})
    for split, views in (("train", range(n_views)), ("test", [n_views])):
        frames = []
        for v in views:
            c2w = syn.pose_spherical(40.0 * v, -30.0, 4.0)
            for t in range(n_times):
                name = f"r_{v}_{t}"
                Image.fromarray(rng.integers(0, 256, (H, W, 4), dtype=np.uint8), "RGBA").save(os.path.join(path, name + ".png"))
                if masks:
                    Image.fromarray(rng.integers(0, 256, (H, W), dtype=np.uint8), "L").save(os.path.join(path, "masks_gripper", name + ".png"))
                frames.append({"file_path": name, "time": t / (n_times - 1), "transform_matrix": c2w.tolist()})
        with open(os.path.join(path, f"transforms_{split}.json"), "w") as f:
            json.dump({"camera_angle_x": 0.69, "camera_angle_y": 0.55, "frames": frames}, f)
    return pos


def test_read_cloth_scene_info_and_nerf_normalization_on_a_tiny_scene(tmp_path):
    path = str(tmp_path / "scene")
    pos = write_scene(path)
    info, mesh, preds = scene_io.read_cloth_scene_info(path, white_background=True)
    assert len(info.train_cameras) == 6 and len(info.test_cameras) == 3 and info.video_cameras is None and info.maxtime == 1.0
    assert info.initial_mesh is mesh and info.mesh_predictions is preds and len(preds) == 3
    assert torch.equal(mesh.pos, torch.from_numpy(pos)) and mesh.face.shape == (3, 8) and mesh.edge_index.shape[0] == 2 and mesh.norm.shape == (9, 3)
    assert all(torch.equal(p.pos, torch.from_numpy((pos + 0.01 * t).astype(np.float32))) for t, p in enumerate(preds))
    merged, _, _ = scene_io.read_cloth_scene_info(path, white_background=True, eval=False)
    assert len(merged.train_cameras) == 9 and merged.test_cameras == []
    assert len(scene_io.read_cloth_scene_info(path, True, time_skip=2)[2]) == 2
    with pytest.raises(FileNotFoundError):
        scene_io.read_cloth_scene_info(path + "_none", True)
    # getNerfppNorm (dataset_readers.py:58-79), restated: every camera sits 4 from the origin
    norm = info.nerf_normalization
    centers = np.stack([np.linalg.inv(np.block([[np.asarray(c.R).T, np.asarray(c.T)[:, None]], [np.zeros((1, 3)), np.ones((1, 1))]]))[:3, 3]
                        for c in info.train_cameras], 1)
    mean = centers.mean(1, keepdims=True)
    assert np.allclose(norm["translate"], -mean[:, 0], atol=1e-6)
    assert abs(norm["radius"] - 1.1 * np.linalg.norm(centers - mean, axis=0).max()) < 1e-5
    assert np.allclose(np.linalg.norm(centers, axis=0), 4.0, atol=1e-5)
    assert scene_io.nerf_normalization(merged.train_cameras)["radius"] != norm["radius"]
    # the loader's images are 8-bit levels: the data set keeps them as such, and serves the loader's floats
    ds = CameraDataset(merged.train_cameras, device="cpu")
    assert ds.storage == "uint8" and (ds.n_viewpoints, ds.n_times) == (3, 3) and ds.has_mask
    _, _, cells = R.grid(merged.train_cameras)
    for v in range(3):
        for cam, t in zip(ds.step(v, [0, 1, 2]), range(3)):
            same_camera(cam, camera_from_info(cells[(v, t)], "cpu"))


# ------------------------------------------------------------------------------------------------------------------ the driver
class FakeGaussians:
    def __init__(self, sh_degree):
        self.sh_degree = sh_degree

    def from_mesh(self, pos, face, edge_index, factor, generator=None):
        self.mesh = SimpleNamespace(pos=pos, face=face, edge_index=edge_index)
        self.factor = factor
        return self

    def training_setup(self, **lrs):
        self.lrs = lrs


def driver(n_times, monkeypatch, seed=5, n_views=2, extra_times=0):
    from csplat import synthetic as syn
    total = n_times + extra_times
    infos = [R.make_info(v, t, 4, 6, n_times=max(total, 2)) for v in range(n_views) for t in range(total)]
    pos, faces, edge_index = syn.grid_mesh(3)
    mesh = SimpleNamespace(pos=torch.from_numpy(pos), face=torch.from_numpy(faces.T.copy()), edge_index=torch.from_numpy(edge_index))
    preds = [SimpleNamespace(pos=torch.from_numpy(pos + 0.01 * t)) for t in range(total)]
    calls = []

    def recorder(iteration, cams, gaussians, simulator, meshnet_optimizer, pipe, opt, background, static=False, densify_opt=None):
        assert isinstance(meshnet_optimizer, torch.optim.Adam) and meshnet_optimizer.param_groups[0]["lr"] == opt.meshnet_lr
        assert meshnet_optimizer.param_groups[0]["params"][0] is next(iter(simulator.parameters()))
        calls.append(([c.view_id for c in cams], [c.time_id for c in cams], static, iteration, densify_opt, simulator, meshnet_optimizer))
        return torch.tensor(20.0), torch.tensor(0.5), {}

    monkeypatch.setattr(refine, "MeshGaussians", FakeGaussians)
    monkeypatch.setattr(refine._train, "train_step", recorder)
    so = refine.SingleStepOptimizer(device="cpu", rng=np.random.default_rng(seed), n_times_max=max(total, 2),
                                    densify_opt=SimpleNamespace(densify_until_iter=7))
    so.initialize([i for i in infos if i.time_id < n_times], mesh, preds[:n_times])
    return so, infos, preds, calls


@pytest.mark.parametrize("n_times", [1, 2, 3, 5])
def test_driver_sequence_and_last_iters_across_two_rounds(n_times, monkeypatch):
    so, infos, preds, calls = driver(n_times, monkeypatch)
    assert so.camera_data.n_times == n_times and so.gaussians.factor == 2 and so.gaussians.lrs["position_lr"] == so.opt.position_lr_init
    assert abs(so.cameras_extent - float(scene_io.nerf_normalization(infos)["radius"])) < 1e-12
    assert so.simulator.training and so.simulator.n_times == max(n_times, 2) and so.simulator.mesh_predictions.shape == (n_times, 9, 3)
    so.static_reconstruction(5)
    assert so.last_iters == 5 and so.static_iterations == 5
    so.update_mesh_predictions(4)
    assert so.last_iters == 9
    so.update_mesh_predictions(3)
    assert so.last_iters == 12
    want = R.driver_sequence(2, n_times, 5, (4, 3), np.random.default_rng(5))
    got = [(c[0][0], c[1], c[2], c[3]) for c in calls]
    assert got == want and [c[3] for c in calls] == list(range(1, 13))
    assert all(len(set(c[0])) == 1 for c in calls)                                   # one view per step
    if n_times >= 3:
        assert all(t == [t[0], t[0] + 1, t[0] + 2] and t[0] >= 0 and t[2] <= n_times - 1 for _, t, s, _ in got if not s)     # never time -1
    # the densification schedule rides on the static steps only, with the extent and the background filled in
    assert all((c[4] is not None) == c[2] for c in calls)
    assert calls[0][4].cameras_extent == so.cameras_extent and calls[0][4].white_background is False and calls[0][4].densify_until_iter == 7
    # a fresh Adam per loop on the same simulator
    assert calls[0][6] is calls[4][6] and calls[5][6] is calls[8][6] and calls[4][6] is not calls[5][6] and calls[8][6] is not calls[9][6]
    assert all(c[5] is so.simulator for c in calls)


def test_update_data_adds_the_new_cells_and_creates_a_fresh_simulator(monkeypatch):
    so, infos, preds, calls = driver(3, monkeypatch, extra_times=2)
    old = so.simulator
    assert so.camera_data.n_slots == 6
    so.update_data([i for i in infos if i.time_id < 4], preds[:4])
    assert so.camera_data.n_slots == 8 and so.camera_data.n_times == 4 and so.camera_data.uploaded_cells == 8      # + one cell per view
    assert so.simulator is not old and so.simulator.training and so.simulator.mesh_predictions.shape[0] == 4
    so.update_data(infos, preds, n_times=4)                                          # [:, :n_times] of the reference's update_data
    assert so.camera_data.n_slots == 10 and so.camera_data.n_times == 4 and so.simulator.mesh_predictions.shape[0] == 4
    meshes = so.refined_meshes()
    assert meshes.shape == (4, 9, 3) and not meshes.requires_grad
    table = torch.stack([p.pos for p in preds[:4]]).float()
    assert float((meshes - table).abs().max()) < 1e-3                                # the table plus a residual that starts near zero


def test_save_writes_under_the_reference_names(tmp_path, monkeypatch):
    so, *_ = driver(2, monkeypatch)
    so.gaussians.save_ply = lambda p: (os.makedirs(p), open(os.path.join(p, "point_cloud.ply"), "w").close())
    so.static_iterations, so.iterations = 30, 12
    assert so.save(str(tmp_path)) == 42
    assert os.path.exists(tmp_path / "point_cloud" / "iteration_42" / "point_cloud.ply")
    state = torch.load(tmp_path / "meshnet" / "model-42.pt")
    assert set(state) == set(so.simulator.state_dict())


# ------------------------------------------------------------------------------------------------------------------ the C-ABI
def test_header_exports_and_bindings():
    from csplat import native
    header = open(os.path.join(ROOT, "include", "csplat.h")).read()
    m = re.search(r"\bint\s+csplat_camera_batch\s*\(([^;]*)\)\s*;", re.sub(r"/\*.*?\*/", "", header, flags=re.S))
    assert m and len(m.group(1).split(",")) == 12
    assert len(native.EXPORTS["csplat_camera_batch"][1]) == 12 and hasattr(native.lib, "csplat_camera_batch")
    block = header[header.index("/* Camera data set"):]
    block = block[:block.index("*/") + 2]
    assert block.rstrip().endswith("Added exports: CSPLAT_ABI_VERSION is unchanged. */")
    assert native.ABI_VERSION == 9 and native.lib.csplat_abi_version() == 9 and re.search(r"#define\s+CSPLAT_ABI_VERSION\s+9\b", header)
    for name, code in cdm.STORAGES.items():
        assert int(re.search(r"#define\s+CSPLAT_CAMERA_" + name.upper() + r"\s+(\d+)", header).group(1)) == code
    code = re.sub(r"//[^\n]*", "", open(SRC).read())
    assert "#pragma clang fp contract(off)" in code and "atomic" not in code.lower() and code.count("<<<") == 1       # one launch
    assert "255.0f" in code and "1.0f / 255" not in code and "rcp" not in code.lower()                                  # a division


def test_launch_constants_named_in_the_source():
    threads, per_lane = constants()
    assert (threads, per_lane) == (256, 16) and cdm.PITCH_ALIGN == per_lane == 16      # a lane's 16 pixels are one 16-byte load
    assert threads % 64 == 0


def A(k):
    return 0x100000000 * (k + 1)


def test_the_library_refuses_bad_arguments_before_any_launch():
    """fake, distinct, aligned addresses 2^32 apart: every call here must be refused (or be a no-op) before a launch could touch them"""
    from csplat import native
    L = native.lib

    def call(**kw):
        a = dict(n=3, H=10, W=10, storage=0, has_mask=1, n_slots=5, pitch=112, store=A(0), slots=A(1), gt=A(2), mask=A(3))
        a.update(kw)
        return L.csplat_camera_batch(None, a["n"], a["H"], a["W"], a["storage"], a["has_mask"], a["n_slots"], a["pitch"], a["store"], a["slots"],
                                     a["gt"], a["mask"])
    for kw in (dict(n=-1), dict(H=-1), dict(W=-1), dict(n_slots=-1), dict(pitch=-16), dict(storage=2), dict(storage=-1), dict(has_mask=2),
               dict(pitch=100), dict(pitch=120), dict(pitch=96), dict(storage=1), dict(storage=1, pitch=384), dict(H=2 ** 16, W=2 ** 15),
               dict(n_slots=2 ** 31), dict(store=None), dict(slots=None), dict(gt=None), dict(mask=None), dict(has_mask=0),
               dict(store=A(0) + 8), dict(slots=A(1) + 2), dict(gt=A(2) + 1), dict(mask=A(3) + 2), dict(gt=A(0)), dict(gt=A(0) + 5 * 4 * 112 - 4),
               dict(mask=A(0) + 16), dict(gt=A(1) + 8), dict(mask=A(1)), dict(mask=A(2) + 3 * 3 * 400 - 4), dict(gt=A(3) - 3 * 3 * 400 + 4)):
        assert call(**kw) == 2, kw
        assert b"csplat_camera_batch" in L.csplat_last_error(), kw
    assert call(n=0) == 0 and call(H=0) == 0 and call(n=0, store=None, slots=None, gt=None, mask=None) == 0
    assert call(W=0, pitch=0) == 0
