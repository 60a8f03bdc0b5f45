"""The camera data set on the GPU (csplat_camera_batch in csrc/csplat_camera_dataset.hip, behind csplat.camera_dataset), the train step's
two fast paths and the online-refinement driver (csplat.refine), under strict dispatch.

Batches: `gt` and `mask` are compared BIT FOR BIT (as int32 words, so that NaN payloads and -0.0 count) against the restatement
tests/camera_dataset_ref.py -- uint8 / 255.0 in float32 and 1.0 - that, computed on the CPU -- for both storages.  There is no tolerance:
each output is one or two exactly rounded operations, or a copied word.  Every case runs twice and the two runs are compared bit for bit.

Sizes, by H * W, and the launch constant each crosses (CAMERA_THREADS = 256 lanes of CAMERA_PIXELS_PER_LANE = 16 pixels, read from the
source: a lane takes 16 pixels as four groups of 4, a wave's instruction covers 256 consecutive pixels, a pass of the workgroup 1024, the
workgroup wg = 4096): 1, 15, 16, 17 (below, on and one past a lane's share), 63, 64, 65, 255, 256, 257 (a wave's instruction), 1025 (one
past a pass: the second group of lane 0), wg - 1, wg, wg + 1 (the second workgroup holds one pixel).  H * W % 4 == 0 (16, 64, 256, 4096)
puts every output plane on a 16-byte boundary: the 16-byte path; H * W % 4 == 1 (17, 65, 257, 1025, 4097) and == 3 (15, 63, 255, 4095)
leave only every fourth plane aligned: the scalar path, and the aligned planes' last one or three pixels.  Batches of n = 1, 3 and 17
cameras; a batch that repeats a slot;
the first and the last slot of the store; a batch taken before and after the store grew past its first capacity (the buffer has moved);
with and without masks; plan() followed by steps against step() alone; a slot index outside the store (through the C-ABI; the Python
surface raises IndexError first) gives NaN planes and reads nothing.  float32 storage also with NaN (with a payload), -0.0 and a denormal.

train_step in the bit-reproducible mode (debug-flags bit 8): two steps on data-set cameras and two on scene_io.camera_from_info cameras
from equal states -- loss, PSNR and every parameter bit-equal, with and without masks, and the tensors handed to the image loss ARE the
batch's.  SingleStepOptimizer: static_reconstruction(6) + update_mesh_predictions(6) against a hand-written loop of train_step over
camera_from_info cameras in the recorded order -- Gaussian parameters and simulator weights bit-equal; refined_meshes() against a float64
restatement of table + MLP under the bar rule of tests/test_train_kernels_gpu.py (check(): 8 x the float32 restatement's own error, floor
1e-6); update_data with one more time adds one slot per view.

What the table showed on an MI355X when this file was written (group | comparisons | largest e32 | largest bar | largest kernel error |
smallest bar / error):
  camera refined_meshes | 1 | 5.75e-08 | 1.00e-06 | 5.75e-08 | 17.4
The simulator's kernels gave the float32 restatement's own error (5.75e-8 of the largest coordinate: one rounding of the table row plus the
residual), so the bar is the rule's floor.  Every gt and mask was equal to the restatement bit for bit at every size and in both storages;
loss, PSNR, every Gaussian parameter and every simulator weight of the two train-step arms and of the two driver arms were bit-equal.
Wall time 6 s for the 71 tests of this file (the slowest, the first train step of the process, 2 s)."""
import numpy as np
import pytest

import util  # noqa: F401
import camera_dataset_ref as R
from test_camera_dataset_cpu import bits, constants, same_camera
from test_train_kernels_gpu import FLOOR, K, TABLE, check  # noqa: F401  (the project's rule for a bar, and the table of its comparisons)

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
from csplat import native, refine  # noqa: E402
from csplat import train as tr  # noqa: E402
from csplat.camera_dataset import CameraDataset  # noqa: E402  (absent: every test of this file fails)
from csplat.scene_io import camera_from_info  # noqa: E402

THREADS, PER_LANE = constants()
WG = THREADS * PER_LANE
SHAPES = {1: (1, 1), 15: (3, 5), 16: (4, 4), 17: (1, 17), 63: (7, 9), 64: (8, 8), 65: (5, 13), 255: (15, 17), 256: (16, 16), 257: (1, 257),
          1025: (25, 41), WG - 1: (63, 65), WG: (64, 64), WG + 1: (17, 241)}
N_TIMES = 9
DET = 256       # csplat_debug_flags bit 8: every kernel of the step sums in a fixed order (tests/test_train_gpu.py)


@pytest.fixture(scope="module", autouse=True)
def _strict_and_table():
    old, native.STRICT = native.STRICT, True
    yield
    native.STRICT = old
    print("\ngroup | comparisons | largest e32 | largest bar | largest kernel error | smallest bar / error")
    for g in sorted(g for g in TABLE if g.startswith("camera")):
        n, e32, bar, err, margin = TABLE[g]
        print(f"{g} | {n} | {e32:.2e} | {bar:.2e} | {err:.2e} | {margin:.1f}")


def test_the_sizes_are_the_launch_constants_edges():
    assert (THREADS, PER_LANE, WG) == (256, 16, 4096) and all(h * w == hw for hw, (h, w) in SHAPES.items())
    assert {hw % 4 for hw in SHAPES} == {0, 1, 3}


def expected(infos):
    """(gt [n,3,H,W], mask [n,1,H,W] or None) of the records as scene_io.camera_from_info serves them, on the CPU"""
    gt = torch.stack([i.image.clamp(0.0, 1.0).float() for i in infos])
    mask = None if infos[0].mask is None else torch.stack([i.mask.float() for i in infos])
    return gt, mask


def same_batch(batch, infos, what):
    gt, mask = expected(infos)
    assert batch.gt.is_cuda and batch.gt.dtype == torch.float32 and batch.gt.shape == gt.shape, what
    assert torch.equal(bits(batch.gt.cpu()), bits(gt)), what
    assert (batch.mask is None) == (mask is None), what
    if mask is not None:
        assert batch.mask.shape == mask.shape and torch.equal(bits(batch.mask.cpu()), bits(mask)), what
    for i, cam in enumerate(batch):
        assert cam.original_image.data_ptr() == batch.gt[i].data_ptr() and cam.gt_stack is batch.gt and cam.gt_index == i
        assert cam.mask_stack is batch.mask and (cam.mask is None or cam.mask.data_ptr() == batch.mask[i].data_ptr())


def twice(ds, view, times, infos, what):
    a = ds.step(view, times)
    same_batch(a, [infos[t] for t in times], what)
    b = ds.step(view, times)
    assert torch.equal(bits(a.gt), bits(b.gt)) and (a.mask is None or torch.equal(bits(a.mask), bits(b.mask))), what
    return a


@pytest.mark.parametrize("mask", [True, False])
@pytest.mark.parametrize("storage", ["uint8", "float32"])
@pytest.mark.parametrize("hw", sorted(SHAPES))
def test_batches_at_the_launch_edges(hw, storage, mask):
    H, W = SHAPES[hw]
    infos = [R.make_info(0, t, H, W, mask, seed=hw, n_times=N_TIMES) for t in range(N_TIMES)]
    ds = CameraDataset(infos[:4], device="cuda", storage=storage, capacity=4)
    assert ds.capacity == 4 and ds.n_slots == 4 and ds.storage == storage
    before = twice(ds, 0, [0, 1, 2, 3], infos, (hw, "before the store grew"))
    where = ds._store.data_ptr()
    assert ds.add_frames(infos) == N_TIMES - 4 and ds.capacity == 16 and ds._store.data_ptr() != where          # the buffer has moved
    after = twice(ds, 0, [0, 1, 2, 3], infos, (hw, "after the store grew"))
    assert torch.equal(bits(after.gt), bits(before.gt))
    twice(ds, 0, [N_TIMES - 1], infos, (hw, "n = 1, the last slot"))
    twice(ds, 0, [0, N_TIMES - 1, 4], infos, (hw, "n = 3, the first and the last slot"))
    twice(ds, 0, [5, 5, 2], infos, (hw, "a repeated slot"))
    long = [(7 * k + 3) % N_TIMES for k in range(17)]
    alone = twice(ds, 0, long, infos, (hw, "n = 17"))
    # plan() followed by steps against step() alone
    sched = [(0, [0, 1, 2]), (0, long), (0, [8])]
    ds.plan(sched)
    for (v, t) in sched:
        same_batch(ds.step(v, t), [infos[k] for k in t], (hw, "planned", t))
    assert ds._plan.at == 3 and torch.equal(bits(ds.step(0, long).gt), bits(alone.gt))
    for cam, t in zip(ds.step(0, [0, 8]), (0, 8)):
        same_camera(cam, camera_from_info(infos[t], "cuda"), (hw, t))
    with pytest.raises(IndexError):
        ds.step(0, [N_TIMES])


@pytest.mark.parametrize("hw", [16, 17, 63, WG + 1])
def test_float32_storage_keeps_every_bit(hw):
    H, W = SHAPES[hw]
    # the words of a NaN with a payload, -0.0, the smallest denormal and a signalling NaN, written as integers (no float conversion on the way)
    payload = torch.tensor([0x7FC12345, -0x80000000, 1, 0x7F800001], dtype=torch.int32)
    infos = []
    for t in range(3):
        i = R.make_info(0, t, H, W, True, seed=hw, n_times=3)
        img, msk = i.image.clone(), i.mask.clone()
        for k in range(min(4, hw)):
            msk.view(torch.int32).view(-1)[(5 * t + k * 3) % hw] = payload[k]
            img.view(torch.int32).view(-1)[(7 * t + k * 5) % (3 * hw)] = payload[k % 3]
        infos.append(i._replace(image=img, mask=msk))
    ds = CameraDataset(infos, device="cuda")
    assert ds.storage == "float32"                                          # "auto": these are not 8-bit levels
    a = twice(ds, 0, [2, 0, 1, 0], infos, (hw, "float32 words"))
    want = torch.stack([infos[t].mask for t in (2, 0, 1, 0)])
    got = a.mask.cpu()
    assert torch.equal(bits(got), bits(want))
    words = set(bits(got).view(-1).tolist())
    assert set(payload.tolist()) <= words                                   # the payload, -0.0, the denormal and the signalling NaN arrived


@pytest.mark.parametrize("storage", ["uint8", "float32"])
@pytest.mark.parametrize("hw", [17, 64, WG + 1])
def test_a_slot_outside_the_store_gives_nan_planes_through_the_c_abi(hw, storage):
    H, W = SHAPES[hw]
    infos = [R.make_info(0, t, H, W, True, seed=hw, n_times=3) for t in range(3)]
    ds = CameraDataset(infos, device="cuda", storage=storage)
    with pytest.raises(IndexError, match="slot"):
        ds._gather([0, 3])
    slots = torch.tensor([1, 3, -1, 2], dtype=torch.int32, device="cuda")
    gt = torch.zeros(4, 3, H, W, device="cuda")
    mask = torch.zeros(4, 1, H, W, device="cuda")
    native.launch("csplat_camera_batch", gt.device, 4, H, W, 0 if storage == "uint8" else 1, 1, ds.n_slots, ds._pitch, native.ptr(ds._store),
                  native.ptr(slots), native.ptr(gt), native.ptr(mask))
    want_gt, want_mask = expected([infos[1], infos[2]])
    assert torch.equal(gt[[0, 3]].cpu(), want_gt) and torch.equal(mask[[0, 3]].cpu(), want_mask)
    assert bool(torch.isnan(gt[1:3]).all()) and bool(torch.isnan(mask[1:3]).all())


# ------------------------------------------------------------------------------------------------------------------ train_step
def small_scene(mask, n_views=2, n_times=4, res=32):
    return [R.make_info(v, t, res, res, mask, seed=77, n_times=n_times) for v in range(n_views) for t in range(n_times)]


def model(P=300, n_times=4):
    import bench_train as bt
    torch.manual_seed(0)
    sc, pc, sim = bt.build(P=P, W=32, H=32, grid=6, n_times=n_times, dev=torch.device("cuda:0"))
    with torch.no_grad():
        pc._scaling.add_(1.2)              # larger splats: the 32 x 32 image is covered
    pc.training_setup()
    return pc, sim, torch.optim.Adam(sim.parameters(), lr=3e-4)


@pytest.mark.parametrize("mask", [True, False])
def test_train_step_on_dataset_cameras_equals_camera_from_info_cameras(mask, monkeypatch):
    infos = small_scene(mask)
    ds = CameraDataset(infos, device="cuda")
    assert ds.storage == "uint8"
    seen = []
    fusable = tr._image_loss_fusable

    def spy(image, gt, opt, mask_tensor):
        seen.append((gt, mask_tensor))
        return fusable(image, gt, opt, mask_tensor)

    monkeypatch.setattr(tr, "_image_loss_fusable", spy)
    bg = torch.ones(3, device="cuda")
    native.lib.csplat_debug_flags(DET)
    try:
        results = []
        for arm in ("dataset", "camera_from_info"):
            pc, sim, mopt = model()
            out = []
            for it, times in ((1, [0, 1, 2]), (2, [1, 2, 3])):
                if arm == "dataset":
                    cams = ds.step(1, times)
                else:
                    cams = [camera_from_info(infos[4 + t], "cuda") for t in times]
                psnr_, loss, _ = tr.train_step(it, cams, pc, sim, mopt, background=bg)
                gt, mask_tensor = seen[-1]
                if arm == "dataset":                                          # the fast paths: the loss reads the batch's own storage
                    assert gt is cams.gt and mask_tensor is cams.mask
                else:
                    assert gt.data_ptr() not in [c.original_image.data_ptr() for c in cams]
                out.append((psnr_.clone(), loss.clone()))
            results.append((out, [p.detach().clone() for p in pc.parameters()], [p.detach().clone() for p in sim.parameters()]))
    finally:
        native.lib.csplat_debug_flags(0)
    (out_a, pc_a, sim_a), (out_b, pc_b, sim_b) = results
    for (pa, la), (pb, lb) in zip(out_a, out_b):
        assert torch.equal(pa, pb) and torch.equal(la, lb) and bool(torch.isfinite(la))
    assert all(torch.equal(a, b) for a, b in zip(pc_a, pc_b)) and all(torch.equal(a, b) for a, b in zip(sim_a, sim_b))
    assert float(out_a[0][1]) > 0.0 and len(seen) == 4


# ------------------------------------------------------------------------------------------------------------------ the driver
def optimizer(infos, n_times, seed=3):
    from csplat import synthetic as syn
    pos, faces, edge_index = syn.grid_mesh(6)
    traj = syn.mesh_trajectory(pos, 4)
    mesh = dict(pos=torch.from_numpy(pos), face=torch.from_numpy(faces.T.copy()), edge_index=torch.from_numpy(edge_index))
    torch.manual_seed(0)
    so = refine.SingleStepOptimizer(device="cuda:0", rng=np.random.default_rng(seed), gaussian_init_factor=6, n_times_max=4,
                                    generator=torch.Generator(device="cuda:0").manual_seed(1))
    so.initialize([i for i in infos if i.time_id < n_times], mesh, torch.from_numpy(traj[:n_times]))
    with torch.no_grad():
        so.gaussians._scaling.add_(1.0)
    return so, traj


def simulator_restated(sim, times, dtype):
    """table + MLP of ResidualMeshSimulator.forward_times in `dtype` on the CPU (meshnet_network.py: SinusoidalEncoder, two ReLU layers,
    the output layer, the table row round(t / dt))"""
    p = {k: v.detach().cpu().to(dtype) for k, v in sim.state_dict().items()}
    t32 = np.asarray(times, np.float32)
    t = torch.from_numpy(t32).to(dtype)[:, None]
    freqs = (2.0 ** torch.linspace(0.0, 5.0, 6, dtype=dtype)).reshape(6, 1)
    angles = t.unsqueeze(-2) * freqs
    feats = torch.sin(torch.stack((angles, angles + torch.pi / 2), dim=-2).flatten(start_dim=-3, end_dim=-1))
    h = torch.cat([t, feats], dim=-1)
    h = torch.relu(h @ p["input.weight"].T + p["input.bias"])
    h = torch.relu(h @ p["hidden.weight"].T + p["hidden.bias"])
    out = h @ p["output.weight"].T + p["output.bias"]
    ids = np.round(t32 / np.float32(sim.time_delta)).astype(np.int64)
    return sim.mesh_predictions.detach().cpu().to(dtype)[ids] + out.reshape(len(times), -1, 3)


def test_single_step_optimizer_equals_a_hand_written_loop(monkeypatch):
    infos = small_scene(True, n_views=2, n_times=4)
    by_cell = {(i.view_id, i.time_id): i for i in infos}
    order = []
    step = tr.train_step

    def recording(iteration, cams, *a, **kw):
        order.append((cams[0].view_id, [c.time_id for c in cams], kw.get("static", False), iteration))
        return step(iteration, cams, *a, **kw)

    native.lib.csplat_debug_flags(DET)
    try:
        so, traj = optimizer(infos, 4)
        assert so.gaussians.num_gaussians == 300 and so.camera_data.n_slots == 8 and so.camera_data.storage == "uint8"
        monkeypatch.setattr(tr, "train_step", recording)
        so.static_reconstruction(6)
        so.update_mesh_predictions(6)
        monkeypatch.setattr(tr, "train_step", step)
        assert order == R.driver_sequence(2, 4, 6, (6,), np.random.default_rng(3)) and so.last_iters == 12
        # the hand-written loop: equal state, camera_from_info cameras, a fresh Adam per phase
        hand, _ = optimizer(infos, 4)
        for phase in (True, False):
            mopt = torch.optim.Adam(hand.simulator.parameters(), lr=hand.opt.meshnet_lr)
            for view, times, static, it in order:
                if static == phase:
                    cams = [camera_from_info(by_cell[(view, t)], "cuda") for t in times]
                    tr.train_step(it, cams, hand.gaussians, hand.simulator, mopt, hand.pipe, hand.opt, hand.background, static=static)
    finally:
        native.lib.csplat_debug_flags(0)
    for a, b in zip(so.gaussians.parameters(), hand.gaussians.parameters()):
        assert torch.equal(a, b)
    start, _ = optimizer(infos, 4)
    assert not torch.equal(so.gaussians._features_dc, start.gaussians._features_dc)                # the steps did train
    assert any(not torch.equal(a, b) for a, b in zip(so.simulator.parameters(), start.simulator.parameters()))
    for a, b in zip(so.simulator.parameters(), hand.simulator.parameters()):
        assert torch.equal(a, b)
    # refined_meshes: one forward_times call, on the device, against table + MLP in float64
    meshes = so.refined_meshes()
    assert meshes.is_cuda and meshes.shape == (4, 36, 3) and not meshes.requires_grad
    times = [float(t) for t in so.camera_data.times]
    assert times == [0.0, 1 / 3, 2 / 3, 1.0]
    check("camera refined_meshes", "4 times x 36 vertices", meshes, simulator_restated(so.simulator, times, torch.float64),
          simulator_restated(so.simulator, times, torch.float32), 0.0)
    report = so.evaluate(n_views=3)
    assert [r["view"] for r in report] == [0, 1] and all(bool(torch.isfinite(r["l1"])) and bool(torch.isfinite(r["psnr"])) for r in report)


def test_update_data_with_one_more_time_adds_one_slot_per_view():
    infos = small_scene(False, n_views=2, n_times=4)
    so, traj = optimizer(infos, 3)
    ds, old = so.camera_data, so.simulator
    assert ds.n_slots == 6 and ds.n_times == 3
    so.update_data(infos, torch.from_numpy(traj))
    assert so.camera_data is ds and ds.n_slots == 8 and ds.uploaded_cells == 8 and ds.n_times == 4 and so.simulator is not old
    assert so.refined_meshes().shape == (4, 36, 3)
    for cam, t in zip(ds.step(1, [0, 3]), (0, 3)):
        same_camera(cam, camera_from_info(infos[4 + t], "cuda"))
