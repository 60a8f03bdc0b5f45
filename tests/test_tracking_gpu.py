"""The tracking kernels (csplat_track_visibility, csplat_track_mte) through csplat.tracking on the GPU, against the float64 restatement of
tests/tracking_ref.py, and track() end to end on the synthetic scene.

Decisions (in_image, visible, counts) are compared for EQUALITY, outside ties.  A point is a tie when a float64 margin of the restatement
is below tau = 64 * 2^-24 * max(W, H) pixels (distance to an image border or, inside the image, to the next pixel cell), or when one of
the two depth margins (|(|X - c| - thr) - d| and |d - min_depth|) is below 64 * 2^-24 * max(|X - c|, d).  Ties are excluded; a case may
exclude at most 1 % of its points, and the float32 restatement on the CPU must take the float64 decision for every kept point.  counts is
compared as it is when a case has no tie; otherwise kernel and restatement run once more with the tie points made invalid (NaN).

Values (pixels_out, aligned, err, mte, mean) by the rule of tests/test_train_kernels_gpu.py (its check() and TABLE are used): within 8 x
the float32 restatement's own error against float64, floor 1e-6, relative to max |ref|.

Inputs.  A pinhole full_proj with tan(fov / 2) = 0.5 per axis, per frame a 0.02 rad yaw and a 0.01 shift (as tests/test_flow_loss_gpu.py);
points uniform in x, y in [-2.4, 2.4], z in [2, 4], every 11th behind the camera; a smooth depth image in [2, 4.5] with a lattice of NaN
pixels and a patch below min_depth; quaternions N(0, 1)^4, not normalised; many ground-truth tracks share a tracked point.

Shapes.  One thread per (frame, point) or per ground-truth track, a 256-thread workgroup of 64-lane waves, no grid stride: N = 1, 63, 64,
65, 255, 256, 257, 1000, 4099; F = 1, 2, 17; images 1x1, 5x1, 1x5, 37x23, 128x96; G = 1, 63, 64, 65, 255, 256, 257, 1000; T = 1, 2, 30; N = 1, 5, 1000
for the MTE.

What the table showed on an MI355X when this file was written (largest e32 / bar / kernel error of a group; smallest bar / error):
  visibility plain          1.65e-07 / 1.32e-06 / 1.43e-07   7.6        visibility no_depth, min_depth_off   9.33e-08 / 1.00e-06 / 9.33e-08   10.7
  visibility all_outside    2.27e-07 / 1.81e-06 / 1.61e-07   11.2
  mte aligned               2.48e-07 / 1.99e-06 / 2.48e-07   6.5        mte plain                            2.29e-07 / 1.83e-06 / 2.29e-07   8.0
The pixels are float32-rounding of the projection, the kernel's error is that of the float32 restatement; every decision outside the ties
was equal.  Ties (checked on the CPU): at most 40 of 69 683 points of a case (0.06 %), none at all in 18 of the 22 cases; float32 pixel
coordinates differ from float64 by at most 6e-5 px at 128 x 96 (tau there: 4.9e-4 px).  Wall time of the 41 tests: 3 to 4 s."""
from types import SimpleNamespace

import numpy as np
import pytest

import util  # noqa: F401
import tracking_ref as R
from test_train_kernels_gpu import FLOOR, K, TABLE, check  # noqa: F401  (the project's rule for a bar, and the table of its comparisons)

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
F64, F32 = torch.float64, torch.float32
NAN = float("nan")
THR, MIN_DEPTH, FAR = 0.2, 1.0, 1e4


@pytest.fixture(scope="module", autouse=True)
def _threads_and_table():
    """torch gets at most 16 host threads for the restatement; afterwards the table of this module's bars (pytest -rP shows it)"""
    old = torch.get_num_threads()
    torch.set_num_threads(min(16, old))
    yield
    torch.set_num_threads(old)
    print("\ngroup | comparisons | largest e32 | largest bar | largest kernel error | smallest bar / error")
    for g in sorted(k for k in TABLE if k.startswith("tracking")):
        n, e32, bar, err, margin = TABLE[g]
        print(f"{g} | {n} | {e32:.2e} | {bar:.2e} | {err:.2e} | {margin:.1f}")


def pinhole(t, W, H):
    """(full_proj, camera centre) of frame t, float64, in the transposed convention (hom = [X, 1] @ full): yaw 0.02 t, shift 0.01 t,
    tan(fov / 2) = 0.5"""
    a = 0.02 * t
    view = torch.eye(4, dtype=F64)
    view[0, 0], view[0, 2], view[2, 0], view[2, 2] = np.cos(a), -np.sin(a), np.sin(a), np.cos(a)
    view[3, :3] = torch.tensor([0.01 * t, -0.01 * t, 0.0], dtype=F64)
    proj = torch.zeros(4, 4, dtype=F64)
    proj[0, 0] = proj[1, 1] = 2.0
    proj[2, 2], proj[2, 3], proj[3, 2] = 1.0001, 1.0, -0.010001
    centre = -view[3, :3] @ torch.linalg.inv(view[:3, :3])          # [c, 1] @ view = 0
    return view @ proj, centre


VIS_VARIANTS = ["plain", "pixels_in", "no_depth", "min_depth_off", "all_outside"]


def vis_case(N, Fr, size, variant="plain", seed=0):
    """float32 CPU inputs of one csplat_track_visibility call"""
    W, H = size
    gen = torch.Generator().manual_seed(100003 * seed + 31 * N + 7 * Fr + 13 * W + H)
    X = torch.cat([4.8 * torch.rand(Fr, N, 2, generator=gen) - 2.4, 2.0 + 2.0 * torch.rand(Fr, N, 1, generator=gen)], 2)
    X[:, ::11, 2] *= -1.0                                                # every 11th behind the camera
    if variant == "all_outside":
        X[..., 0] += 40.0
    cams = [pinhole(t, W, H) for t in range(Fr)]
    full, centre = torch.stack([c[0] for c in cams]).float(), torch.stack([c[1] for c in cams]).float()
    ys, xs = torch.meshgrid(torch.arange(H, dtype=F32), torch.arange(W, dtype=F32), indexing="ij")
    depth = torch.stack([3.25 + 1.25 * torch.sin(0.37 * xs + 0.5 * f) * torch.cos(0.29 * ys - 0.3 * f) for f in range(Fr)])
    depth[:, 2::5, 3::7] = NAN                                           # a lattice of NaN pixels
    depth[:, H // 3:H // 3 + max(1, H // 4), W // 4:W // 4 + max(1, W // 4)] = 0.5          # a patch below min_depth
    c = SimpleNamespace(N=N, F=Fr, W=W, H=H, X=X, full=full, centre=centre, depth=depth, pixels=None, min_depth=MIN_DEPTH, variant=variant)
    if variant == "pixels_in":          # the get_mask form: projections arrive (here: of a slightly different camera, so that they are data)
        x, y, _w = R.project(X.double(), torch.stack([pinhole(t + 0.5, W, H)[0] for t in range(Fr)]), W, H)
        c.pixels = torch.stack([x, y], -1).float()
    elif variant == "no_depth":
        c.depth = None
    elif variant == "min_depth_off":
        c.min_depth = 0.0
    return c


def vis_ref(c, dtype, X=None, pixels=None):
    return R.visibility(c.X if X is None else X, c.full, c.centre, c.depth, c.W, c.H, pixels=c.pixels if pixels is None else pixels,
                        thr=THR, min_depth=c.min_depth, far=FAR, dtype=dtype)


def vis_cpu_side(c):
    """the restatement in both precisions, the ties and what the test asserts about them without a GPU -> (r64, r32, tie [F,N])"""
    r64, r32 = vis_ref(c, F64), vis_ref(c, F32)
    tie = R.ties(r64, c.W, c.H)
    assert int(tie.sum()) <= 0.01 * tie.numel(), f"{int(tie.sum())} of {tie.numel()} points are ties"
    keep = ~tie
    assert torch.equal(r32["in_image"][keep], r64["in_image"][keep]) and torch.equal(r32["visible"][keep], r64["visible"][keep])
    return r64, r32, tie


def vis_kernel(c, X=None, pixels=None):
    from csplat import tracking as tk
    X = c.X if X is None else X
    pixels = c.pixels if pixels is None else pixels
    return tk.track_visibility(X.cuda(), c.full.cuda(), c.centre.cuda(), None if c.depth is None else c.depth.cuda(), (c.H, c.W),
                               pixels=None if pixels is None else pixels.cuda(), depth_threshold=THR, min_depth=c.min_depth, far_value=FAR)


def vis_check(c, group):
    from csplat import native
    before = sum(native.FALLBACK_COUNTS.values())
    r64, r32, tie = vis_cpu_side(c)
    got, again = vis_kernel(c), vis_kernel(c)
    assert sum(native.FALLBACK_COUNTS.values()) == before
    assert got.pixels.shape == (c.F, c.N, 2) and got.in_image.dtype == torch.bool and got.counts.dtype == torch.int32
    for a, b in zip(got, again):                                         # two calls on the same inputs are bit-equal in every output
        assert torch.equal(a.view(torch.uint8) if a.dtype == torch.bool else a.view(torch.int32), b.view(torch.uint8) if b.dtype == torch.bool else b.view(torch.int32))
    keep = ~tie
    assert torch.equal(got.in_image.cpu()[keep], r64["in_image"][keep]) and torch.equal(got.visible.cpu()[keep], r64["visible"][keep])
    if c.variant == "all_outside":
        assert not got.in_image.any() and not got.visible.any() and not got.counts.any()
    if c.depth is None:
        assert torch.equal(got.visible, got.in_image)
    if c.pixels is None:
        check(group, f"pixels N={c.N} F={c.F} {c.W}x{c.H} {c.variant}", got.pixels, r64["pixels"], r32["pixels"], 1.0)
    else:
        assert torch.equal(got.pixels.cpu(), c.pixels)
    if tie.any():                                                        # the tie points made invalid on both sides
        X = torch.where(tie[..., None], torch.full_like(c.X, NAN), c.X)
        pixels = None if c.pixels is None else torch.where(tie[..., None], torch.full_like(c.pixels, NAN), c.pixels)
        ref, got = vis_ref(c, F64, X, pixels), vis_kernel(c, X, pixels)
        assert not R.ties(ref, c.W, c.H).any()
        assert torch.equal(got.in_image.cpu(), ref["in_image"]) and torch.equal(got.visible.cpu(), ref["visible"])
    else:
        ref = r64
    assert torch.equal(got.counts.cpu().long(), ref["counts"])
    assert torch.equal(got.counts.cpu().long(), torch.stack([got.in_image.sum(1), got.visible.sum(1)], 1).cpu())


NS = [1, 63, 64, 65, 255, 256, 257, 1000, 4099]
FS = [1, 2, 17]
IMAGES = [(1, 1), (5, 1), (1, 5), (37, 23), (128, 96)]          # (W, H)
VIS_CASES = [(N, 2, (37, 23), "plain") for N in NS] + [(257, Fr, (37, 23), "plain") for Fr in FS if Fr != 2] + \
            [(1000, 2, size, "plain") for size in IMAGES if size != (37, 23)] + [(4099, 17, (128, 96), "plain")] + \
            [(1000, 2, (37, 23), v) for v in VIS_VARIANTS[1:]] + [(65, 17, (5, 1), "pixels_in"), (257, 1, (128, 96), "no_depth")]


@pytest.mark.parametrize("N,Fr,size,variant", VIS_CASES)
def test_track_visibility_at_the_launch_edges(N, Fr, size, variant):
    vis_check(vis_case(N, Fr, size, variant), f"tracking visibility {variant}")


def test_track_visibility_of_no_points_and_of_one_frame_without_the_frame_axis():
    from csplat import tracking as tk
    c = vis_case(65, 1, (37, 23))
    none = tk.track_visibility(torch.zeros(3, 0, 3, device="cuda"), c.full.cuda()[0], c.centre.cuda()[0], torch.ones(3, 23, 37, device="cuda"), (23, 37))
    assert none.pixels.shape == (3, 0, 2) and none.visible.shape == (3, 0) and none.counts.tolist() == [[0, 0]] * 3
    whole, one = vis_kernel(c), tk.track_visibility(c.X[0].cuda(), c.full[0].cuda(), c.centre[0].cuda(), c.depth[0].cuda(), (c.H, c.W),
                                                    depth_threshold=THR)
    assert one.pixels.shape == (65, 2) and one.counts.shape == (2,)
    assert all(torch.equal(a[0], b) for a, b in zip(whole, one))


# ================================================================================================ the trajectory error
def mte_case(G, T, N, align=True, seed=0):
    gen = torch.Generator().manual_seed(100003 * seed + 31 * G + 7 * T + N)
    traj = torch.randn(N, 3, generator=gen)[None] + 0.1 * torch.randn(T, N, 3, generator=gen).cumsum(0)
    assoc = torch.randint(0, N, (G,), generator=gen)                     # many ground-truth tracks share a point when G > N
    gt = traj[:, assoc] + 0.3 * torch.randn(1, G, 3, generator=gen) + 0.05 * torch.randn(T, G, 3, generator=gen)
    rot = torch.randn(T, N, 4, generator=gen) if align else None          # not normalised
    return SimpleNamespace(G=G, T=T, N=N, traj=traj, gt=gt, rot=rot, assoc=assoc)


def mte_check(c, group):
    from csplat import native, tracking as tk
    before = sum(native.FALLBACK_COUNTS.values())
    r64, r32 = (R.mte(c.gt, c.traj, c.rot, c.assoc, dtype=dt) for dt in (F64, F32))
    cu = lambda t: None if t is None else t.cuda()  # noqa: E731
    got = tk._mte_kernel(cu(c.gt), cu(c.traj), cu(c.rot), cu(c.assoc))
    again = tk._mte_kernel(cu(c.gt), cu(c.traj), cu(c.rot), cu(c.assoc))
    res = tk.mean_trajectory_error(cu(c.gt), cu(c.traj), cu(c.rot), align=c.rot is not None, assoc=c.assoc)
    assert sum(native.FALLBACK_COUNTS.values()) == before
    for a, b in zip(got, again):                                         # bit-equal
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    for a, b in zip((res.aligned, res.per_track, res.mean), (got[0], got[2], got[3])):          # the public call is the same launch
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert res.assoc.dtype == torch.int64 and torch.equal(res.assoc.cpu(), c.assoc)
    tag = f"G={c.G} T={c.T} N={c.N}"
    # relative to max |ref|.  The one exception: an aligned track of ONE frame is gt[0] itself, its error is 0 in exact arithmetic and
    # pure rounding of the positions in float32 -- there the unit is the size of the positions that were subtracted
    unit = float(c.gt.abs().max()) if (c.rot is not None and c.T == 1) else 0.0
    for name, g in zip(("aligned", "err", "mte", "mean"), got):
        check(group, f"{name} {tag}", g, r64[name], r32[name], 0.0 if name == "aligned" else unit)
    if c.rot is None:
        assert torch.equal(got[0].cpu(), c.traj[:, c.assoc])


GS, TS, MTE_NS = [1, 63, 64, 65, 255, 256, 257, 1000], [1, 2, 30], [1, 5, 1000]      # (255, 256, 257: k_track_mean's 256 threads)
MTE_CASES = [(G, 2, 5) for G in GS] + [(257, T, 1000) for T in TS] + [(65, 30, 1), (1000, 30, 1000), (64, 1, 5)]


@pytest.mark.parametrize("G,T,N", MTE_CASES)
def test_track_mte_at_the_launch_edges(G, T, N):
    mte_check(mte_case(G, T, N), "tracking mte aligned")


@pytest.mark.parametrize("G,T,N", [(65, 2, 5), (257, 30, 1000), (1, 1, 1)])
def test_track_mte_without_rotations_is_indexing(G, T, N):
    mte_check(mte_case(G, T, N, align=False), "tracking mte plain")


def test_default_association_and_a_zero_quaternion():
    from csplat import tracking as tk
    c = mte_case(64, 3, 200)
    res = tk.mean_trajectory_error(c.gt.cuda(), c.traj.cuda(), c.rot.cuda())
    d2 = ((c.gt[0].double()[:, None] - c.traj[0].double()[None]) ** 2).sum(-1)
    assert torch.equal(res.assoc.cpu(), d2.argmin(1))                    # nearest at the first frame
    rot = c.rot.clone()
    rot[1, c.assoc[7]] = 0.0
    res = tk.mean_trajectory_error(c.gt.cuda(), c.traj.cuda(), rot.cuda(), assoc=c.assoc)
    hit = (c.assoc == c.assoc[7])
    assert bool(torch.isnan(res.per_track.cpu()[hit]).all()) and bool(torch.isfinite(res.per_track.cpu()[~hit]).all())
    assert bool(torch.isnan(res.mean))                                   # as in the reference: not guarded


# ================================================================================================ track() end to end
def _scene():
    from csplat import synthetic as syn
    from csplat.gaussians import MeshGaussians
    from meshnet.meshnet_network import ResidualMeshSimulator
    W = H = 64
    sc = syn.scene_1(P=600, W=W, H=H, n_cams=1, grid=16, n_times=5, seed=31)
    T = lambda a, dt=torch.float32: torch.tensor(a, device="cuda", dtype=dt)  # noqa: E731
    pc = MeshGaussians(3).from_arrays(T(sc["mesh_pos"][0]), T(sc["faces"].T.copy(), torch.long), T(sc["edge_index"], torch.long),
                                      T(sc["face_ids"], torch.long), T(sc["bary"]), T(sc["log_scales"] + np.log(2.5)), T(sc["quats"]),
                                      T(sc["opacity_logits"]), T(sc["sh"]))
    pc.active_sh_degree = 3
    sim = ResidualMeshSimulator(T(sc["mesh_pos"]), device="cuda")
    with torch.no_grad():
        torch.manual_seed(0)
        sim.output.weight.normal_(0, 1e-3)
    views = []
    for vid, theta in enumerate((0.0, 40.0)):
        for tid, time in enumerate((0.0, 0.2, 0.4)):
            cam = syn.make_camera(theta, W, H, time=time)
            t = lambda a: torch.tensor(a)  # noqa: E731
            views.append(SimpleNamespace(image_height=H, image_width=W, FoVx=cam["FoVx"], FoVy=cam["FoVy"], time=time, view_id=vid, time_id=tid,
                                         world_view_transform=t(cam["world_view_transform"]), full_proj_transform=t(cam["full_proj_transform"]),
                                         camera_center=t(cam["camera_center"])))
    pipe = SimpleNamespace(compute_cov3D_python=False, convert_SHs_python=False, debug=False)
    return views, pc, sim, pipe, torch.ones(3, device="cuda")


@pytest.mark.parametrize("vertices", [False, True])
def test_track_end_to_end_on_the_synthetic_scene(vertices, tmp_path):
    from csplat import tracking as tk
    from gaussian_renderer import render
    views, pc, sim, pipe, bg = _scene()
    # (the vertex rotations are recorded as track() receives them: get_vertice_rotation sums face normals with atomics, and gives NaN for
    #  a vertex whose normal did not move -- a second call is no reference for the bits of the first)
    calls, inner = [], pc.get_vertice_rotation
    pc.get_vertice_rotation = lambda verts: calls.append((verts, inner(verts))) or calls[-1][1]
    tr = tk.track(views, pc, sim, pipe, bg, track_vertices=vertices)
    pc.get_vertice_rotation = inner
    assert len(calls) == (3 if vertices else 0)                          # once per distinct time, not once per view
    N = 256 if vertices else 600
    assert isinstance(tr, tk.Tracks) and tr.times.tolist() == [0.0, 0.2, 0.4]
    assert tr.traj.shape == (3, N, 3) and tr.rotations.shape == (3, N, 4) and tr.pixels.shape == (6, N, 2)
    assert tr.view_ids.tolist() == [0, 0, 0, 1, 1, 1] and tr.time_ids.tolist() == [0, 1, 2, 0, 1, 2]
    assert tr.in_image.shape == (6, N) and tr.visible.dtype == torch.bool and torch.equal(tr.gt_idxs.cpu(), torch.arange(N))
    depths = []
    with torch.no_grad():
        for f, v in enumerate(views):
            res = render(v, pc, sim, pipe, bg, project_vertices=vertices)
            k = int(tr.time_ids[f])
            pos, proj = (res.vertice_deform, res.vertice_projections) if vertices else (res.means3D_deform, res.projections)
            assert torch.equal(tr.traj[k], pos)
            assert torch.equal(tr.pixels[f].view(torch.int32), proj.view(torch.int32))          # bit for bit
            want_rot = [out for verts, out in calls if torch.equal(verts, pos)][0] if vertices else res.rotations
            assert torch.equal(tr.rotations[k].view(torch.int32), want_rot.view(torch.int32))
            depths.append(res.depth[0])
    by_hand = tk.track_visibility(tr.traj[tr.time_ids.cuda()], torch.stack([v.full_proj_transform for v in views]).cuda(),
                                  torch.stack([v.camera_center for v in views]).cuda(), torch.stack(depths), (64, 64))
    assert torch.equal(tr.visible, by_hand.visible) and torch.equal(tr.in_image, by_hand.in_image) and torch.equal(tr.counts, by_hand.counts)
    assert bool(tr.in_image.any()) and bool(tr.visible.any())
    assert float(tr.mte(tr.traj, align=False).mean) == 0.0
    own = tr.mte(tr.traj)                                                # the track against itself: t0 = 0, every aligned point is its own
    assert torch.equal(own.assoc.cpu(), torch.arange(N))
    sound = torch.isfinite(tr.rotations).all(2).all(0)                   # (a NaN vertex rotation makes its track NaN, as in the reference)
    assert bool(sound.any()) and not own.per_track[sound].any() and bool(torch.isnan(own.per_track[~sound]).all())
    assert vertices or (bool(sound.all()) and float(own.mean) == 0.0)
    tr.save_npz(str(tmp_path / "all_trajs.npz"))
    back = np.load(str(tmp_path / "all_trajs.npz"))
    assert np.array_equal(back["traj"], tr.traj.cpu().numpy()) and np.array_equal(back["rotations"], tr.rotations.cpu().numpy())
    # with ground truth: gt_idxs are the nearest tracked points at the first time
    gt = tr.traj[:, [5, 17, 5]] + 1e-4
    with_gt = tk.track(views[:1], pc, sim, pipe, bg, track_vertices=vertices, gt=gt)
    assert with_gt.gt_idxs.tolist() == [5, 17, 5]
