"""Point tracking without a GPU: the restatement tests/tracking_ref.py against tests/golden/tracking.npz (a run of the reference's own
`project`, `get_mask`, `find_traj`, `align_traj` and `compute_mte`; tests/golden/make_tracking_golden.py), known answers, the Python
surface of csplat.tracking on CPU tensors (its composed path), and the library's surface (header, exports, bindings, ABI number).

The fixture has no ties (its generator redraws a point whose decision margin is below the bar of tests/test_tracking_gpu.py), so its masks
must be reproduced EXACTLY; its values are float32 results of the reference and are held to the project's rule, check() of
tests/test_train_kernels_gpu.py: within 8 x the float32 restatement's own error against float64, floor 1e-6, relative to max |ref|."""
import math
import os
import re

import numpy as np
import pytest
import torch

import util
import tracking_ref as R
from test_train_kernels_gpu import FLOOR, K, check  # noqa: F401  (the project's rule for a bar)

F64, F32 = torch.float64, torch.float32
NAN = float("nan")


@pytest.fixture(scope="module")
def gold():
    g = util.golden("tracking.npz")
    return {k: (torch.from_numpy(g[k]) if g[k].ndim else g[k].item()) for k in g.files}


def _frames(g, key):
    T = g["traj"].shape[0]
    return g[key][None].expand(T, *g[key].shape)


def pinhole_full(dtype=F64):
    """camera at the origin looking down +z, tan(fov / 2) = 0.5 per axis, in the transposed convention (hom = [X, 1] @ full): w = z"""
    full = torch.zeros(4, 4, dtype=dtype)
    full[0, 0] = full[1, 1] = 2.0
    full[2, 2], full[2, 3], full[3, 2] = 1.0001, 1.0, -0.010001
    return full


# ------------------------------------------------------------------------------------------------------------------ restatement vs fixture
def test_the_fixture_is_the_small_scene_the_generator_describes(gold):
    T, N, _ = gold["traj"].shape
    assert (T, N, gold["gt"].shape[1], gold["W"], gold["H"]) == (6, 200, 25, 40, 30)
    share = 1.0 - float(gold["mask"].float().mean())
    assert 0.2 < share < 0.5 and bool((gold["in_image"] & ~gold["mask"]).any()) and bool((~gold["in_image"]).any())
    assert bool((gold["depth_raw"] < gold["min_depth"]).any()) and os.path.getsize(os.path.join(util.GOLDEN, "tracking.npz")) < 100_000


@pytest.mark.parametrize("form", ["projecting", "get_mask"])
def test_restatement_reproduces_the_references_masks_exactly_and_its_pixels_within_rounding(gold, form):
    W, H = gold["W"], gold["H"]
    kw = dict(thr=gold["depth_threshold"], far=gold["far_value"])
    if form == "projecting":          # on the raw depth, with the min_depth rule inside
        args = (gold["traj"], _frames(gold, "full_proj"), _frames(gold, "cam_center"), _frames(gold, "depth_raw"), W, H)
        kw["min_depth"] = gold["min_depth"]
    else:                             # the reference's own call: its projections, the depth its caller prepared, no rule inside
        args = (gold["traj"], _frames(gold, "full_proj"), _frames(gold, "cam_center"), _frames(gold, "depth_used"), W, H)
        kw.update(pixels=gold["pixels"], min_depth=0.0)
    r64, r32 = R.visibility(*args, dtype=F64, **kw), R.visibility(*args, dtype=F32, **kw)
    assert not bool(R.ties(r64, W, H).any())                       # the excluded share of the committed case is 0
    for r in (r64, r32):
        assert torch.equal(r["in_image"], gold["in_image"]) and torch.equal(r["visible"], gold["mask"])
        assert torch.equal(r["counts"], torch.stack([gold["in_image"].sum(1), gold["mask"].sum(1)], 1))
    if form == "projecting":
        check("tracking fixture", "pixels", gold["pixels"], r64["pixels"], r32["pixels"], 1.0)


def test_restatement_reproduces_the_references_alignment_and_mte(gold):
    # the association: nearest point at the first frame (the fixture's nearest neighbours are unique)
    d2 = ((gold["gt"][0].double()[:, None] - gold["traj"][0].double()[None]) ** 2).sum(-1)
    assert torch.equal(d2.argmin(1), gold["assoc"])
    r64, r32 = (R.mte(gold["gt"], gold["traj"], gold["rotations"], gold["assoc"], dtype=dt) for dt in (F64, F32))
    check("tracking fixture", "aligned", gold["aligned"], r64["aligned"], r32["aligned"], 1.0)
    check("tracking fixture", "mte", gold["mte"], r64["mte"], r32["mte"], 0.0)
    check("tracking fixture", "mean", torch.tensor(gold["mean"]), r64["mean"], r32["mean"], 0.0)


# ------------------------------------------------------------------------------------------------------------------ known answers
def _vis(points, depth=None, W=8, H=4, **kw):
    X = torch.tensor(points, dtype=F64)[None]
    D = None if depth is None else depth[None]
    return R.visibility(X, pinhole_full()[None], torch.zeros(1, 3, dtype=F64), D, W, H, **kw)


def test_a_point_on_the_optical_axis_lands_at_the_image_centre():
    r = _vis([[0.0, 0.0, 3.0]])
    assert r["pixels"][0, 0].tolist() == [(8 - 1) / 2, (4 - 1) / 2] and bool(r["in_image"][0, 0]) and bool(r["visible"][0, 0])


def test_the_right_border_is_outside_and_the_left_border_inside():
    # x = ((X / z * 2 + 1) W - 1) / 2: X / z = (2 x + 1) / (2 W) - 1/2; W = 8 and z = 4 keep every step exact
    at = lambda x: [4.0 * ((2 * x + 1) / 16.0 - 0.5), 0.0, 4.0]  # noqa: E731
    r = _vis([at(8.0), at(0.0), at(7.5), at(-0.25)])
    assert r["pixels"][0, :, 0].tolist() == [8.0, 0.0, 7.5, -0.25]
    assert r["in_image"][0].tolist() == [False, True, True, False]
    assert r["margin_border"][0, :2].tolist() == [0.0, 0.0] and R.ties(r, 8, 4)[0].tolist() == [True, True, False, False]


def test_a_point_behind_the_camera_is_never_in_the_image():
    r = _vis([[0.0, 0.0, -3.0], [0.1, 0.1, -2.0], [0.0, 0.0, 0.0]])
    assert bool(((r["pixels"][0, :2] >= 0) & (r["pixels"][0, :2] < 4)).all())          # mirrored into the image: the reference would keep them
    assert not r["in_image"].any() and not r["visible"].any() and r["counts"].tolist() == [[0, 0]]
    # the get_mask form receives projections and has no test of w
    g = _vis([[0.0, 0.0, -3.0]], pixels=torch.tensor([[[3.5, 1.5]]], dtype=F64))
    assert bool(g["in_image"][0, 0])


def test_min_depth_turns_a_small_depth_into_visible_and_a_nan_depth_into_hidden():
    D = torch.full((4, 8), 0.5, dtype=F64)
    p = [[0.0, 0.0, 3.0]]
    assert not bool(_vis(p, D, min_depth=0.0)["visible"][0, 0])            # 3 - 0.2 > 0.5: hidden while the rule is off
    on = _vis(p, D, min_depth=1.0, far=1e4)
    assert bool(on["visible"][0, 0]) and float(on["margin_min"][0, 0]) == 0.5
    assert bool(_vis(p, torch.full((4, 8), 2.8, dtype=F64))["visible"][0, 0])          # `<=`: exactly dist - thr is visible
    assert not bool(_vis(p, torch.full((4, 8), 2.75, dtype=F64))["visible"][0, 0])
    D[1, 3] = NAN                                                          # the tap of the centre (3.5, 1.5) is [1][3]: C truncation
    r = _vis(p, D)
    assert bool(r["in_image"][0, 0]) and not bool(r["visible"][0, 0]) and r["counts"].tolist() == [[1, 0]]
    r = _vis([[NAN, 0.0, 3.0]], torch.full((4, 8), 9.0, dtype=F64))
    assert not bool(r["in_image"][0, 0]) and not bool(r["visible"][0, 0])


def _rigid_case(q_of_k):
    T, N = 4, 3
    gen = torch.Generator().manual_seed(3)
    traj = torch.randn(T, N, 3, generator=gen, dtype=F64)
    rot = torch.stack([torch.tensor(q_of_k(k), dtype=F64).expand(N, 4) for k in range(T)])
    return traj, rot


def test_identity_quaternions_align_by_a_pure_translation():
    traj, rot = _rigid_case(lambda k: [2.0, 0.0, 0.0, 0.0])                # any norm: normalised inside
    shift = torch.tensor([0.25, -0.5, 1.0], dtype=F64)
    r = R.mte(traj + shift, traj, rot, torch.arange(3))
    assert torch.allclose(r["aligned"], traj + shift, atol=1e-15) and float(r["mean"]) < 1e-15 and float(r["mte"].max()) < 1e-15
    # without alignment the shift is the error
    n = R.mte(traj + shift, traj, None, torch.arange(3))
    assert torch.equal(n["aligned"], traj) and abs(float(n["mean"]) - float(shift.norm())) < 1e-15


def test_a_quarter_turn_about_z_turns_the_translation():
    h = math.sqrt(0.5)
    traj, rot = _rigid_case(lambda k: [1.0, 0.0, 0.0, 0.0] if k == 0 else [h, 0.0, 0.0, h])
    gt = traj.clone()
    gt[0] += torch.tensor([1.0, 0.0, 0.0], dtype=F64)
    r = R.mte(gt, traj, rot, torch.arange(3))
    assert torch.allclose(r["aligned"][0], traj[0] + torch.tensor([1.0, 0.0, 0.0], dtype=F64), atol=1e-15)
    assert torch.allclose(r["aligned"][1:], traj[1:] + torch.tensor([0.0, 1.0, 0.0], dtype=F64), atol=1e-15)       # x turned into y
    assert torch.allclose(r["err"][1:], torch.ones(3, 3, dtype=F64), atol=1e-15) and abs(float(r["mean"]) - 0.75) < 1e-15


def test_a_zero_quaternion_gives_nan_as_in_the_reference():
    traj, rot = _rigid_case(lambda k: [1.0, 0.0, 0.0, 0.0])
    rot[2, 1] = 0.0
    r = R.mte(traj + 0.5, traj, rot, torch.arange(3))
    assert bool(torch.isnan(r["mte"][1])) and bool(torch.isfinite(r["mte"][[0, 2]]).all()) and bool(torch.isnan(r["mean"]))


# ------------------------------------------------------------------------------------------------------------------ the Python surface
def test_track_visibility_on_cpu_tensors_equals_the_restatement_and_the_fixture(gold):
    from csplat import tracking as tk
    W, H = gold["W"], gold["H"]
    for dt in (F32, F64):
        v = tk.track_visibility(gold["traj"].to(dt), gold["full_proj"], gold["cam_center"], _frames(gold, "depth_raw"), (H, W),
                                depth_threshold=gold["depth_threshold"], min_depth=gold["min_depth"], far_value=gold["far_value"])
        assert isinstance(v, tk.Visibility) and v._fields == ("pixels", "in_image", "visible", "counts")
        assert v.pixels.shape == (6, 200, 2) and v.pixels.dtype == dt
        assert v.in_image.dtype == torch.bool and v.visible.dtype == torch.bool and v.counts.dtype == torch.int32 and v.counts.shape == (6, 2)
        assert torch.equal(v.in_image, gold["in_image"]) and torch.equal(v.visible, gold["mask"])
        assert torch.equal(v.counts.long(), torch.stack([gold["in_image"].sum(1), gold["mask"].sum(1)], 1))
        assert float((v.pixels.double() - gold["pixels"].double()).abs().max()) < 1e-4
    # [N,3]: one frame, every result without the leading axis; a [4,4] / [3] camera serves all frames
    one = tk.track_visibility(gold["traj"][2], gold["full_proj"], gold["cam_center"], gold["depth_raw"], (H, W))
    assert one.pixels.shape == (200, 2) and one.in_image.shape == (200,) and one.counts.shape == (2,)
    assert torch.equal(one.visible, gold["mask"][2]) and torch.equal(one.pixels, v32_row(tk, gold, 2))
    # no depth: visible = in_image; pixels given: used as they are
    nod = tk.track_visibility(gold["traj"], gold["full_proj"], None, None, (H, W))
    assert torch.equal(nod.visible, nod.in_image) and torch.equal(nod.in_image, gold["in_image"])
    pix = tk.track_visibility(gold["traj"], None, gold["cam_center"], _frames(gold, "depth_used")[:, None], (H, W), pixels=gold["pixels"],
                              min_depth=0.0)
    assert torch.equal(pix.pixels, gold["pixels"]) and torch.equal(pix.visible, gold["mask"])
    # numpy in
    npv = tk.track_visibility(gold["traj"].numpy(), gold["full_proj"].numpy(), gold["cam_center"].numpy(), _frames(gold, "depth_raw").numpy(),
                              (H, W))
    assert torch.equal(npv.visible, gold["mask"])


def v32_row(tk, gold, k):
    return tk.track_visibility(gold["traj"], gold["full_proj"], gold["cam_center"], None, (gold["H"], gold["W"])).pixels[k]


def test_get_mask_and_project_carry_the_references_signatures_and_results(gold):
    import inspect
    from types import SimpleNamespace
    from csplat import tracking as tk
    assert list(inspect.signature(tk.get_mask).parameters) == ["projections", "gaussian_positions", "depth", "cam_center", "height", "width",
                                                               "depth_threshold"]
    assert [p.default for p in inspect.signature(tk.get_mask).parameters.values()][4:] == [800, 800, 0.2]
    assert list(inspect.signature(tk.project).parameters) == ["means3D_deform", "viewpoint_camera"]
    cam = SimpleNamespace(full_proj_transform=gold["full_proj"], image_height=gold["H"], image_width=gold["W"])
    for k in (0, 3):
        m, i = tk.get_mask(projections=gold["pixels"][k].numpy(), gaussian_positions=gold["traj"][k].numpy(),
                           depth=gold["depth_used"][None].numpy(), cam_center=gold["cam_center"].numpy(), height=gold["H"], width=gold["W"])
        assert isinstance(m, np.ndarray) and isinstance(i, np.ndarray) and m.dtype == bool and i.dtype == bool and m.shape == (200,)
        assert np.array_equal(m, gold["mask"][k].numpy()) and np.array_equal(i, gold["in_image"][k].numpy())
        # the raw depth: get_mask does NOT apply the min_depth rule, its caller does
        raw, _ = tk.get_mask(gold["pixels"][k], gold["traj"][k], gold["depth_raw"], gold["cam_center"], gold["H"], gold["W"])
        xi, yi = gold["pixels"][k][:, 0].long(), gold["pixels"][k][:, 1].long()
        patch = (gold["in_image"][k] & (xi >= 6) & (xi < 12) & (yi >= 4) & (yi < 9)).numpy()          # where depth_raw is 0.5
        assert patch.any() and not raw[patch].any() and m[patch].all() and np.array_equal(raw[~patch], m[~patch])
        p = tk.project(gold["traj"][k].numpy(), cam)
        assert torch.is_tensor(p) and p.shape == (200, 2) and p.dtype == F32
        assert float((p.cpu() - gold["pixels"][k]).abs().max()) < 1e-4
    with pytest.raises(ValueError, match="`depth` is required"):
        tk.get_mask(gold["pixels"][0], gold["traj"][0], None, gold["cam_center"])
    with pytest.raises(ValueError, match=r"\[N,3\]"):
        tk.project(torch.zeros(5, 2), cam)


def test_mean_trajectory_error_on_cpu_tensors(gold):
    from csplat import tracking as tk
    for dt in (F32, F64):
        r = tk.mean_trajectory_error(gold["gt"].to(dt), gold["traj"].to(dt), gold["rotations"].to(dt))
        assert isinstance(r, tk.TrajectoryError) and r._fields == ("mean", "per_track", "aligned", "assoc")
        assert r.mean.shape == () and r.per_track.shape == (25,) and r.aligned.shape == (6, 25, 3) and r.mean.dtype == dt
        assert r.assoc.dtype == torch.int64 and torch.equal(r.assoc, gold["assoc"])          # the default association: nearest at frame 0
        assert float((r.aligned.double() - gold["aligned"].double()).abs().max()) < 1e-5
        assert float((r.per_track.double() - gold["mte"].double()).abs().max()) < 1e-6 and abs(float(r.mean) - gold["mean"]) < 1e-6
    ref = R.mte(gold["gt"], gold["traj"], gold["rotations"], gold["assoc"])
    assert float((r.aligned - ref["aligned"]).abs().max()) < 1e-13 and abs(float(r.mean) - float(ref["mean"])) < 1e-14
    # align=False equals indexing; a given association (numpy, int32) is used as it is, many tracks may share a point
    n = tk.mean_trajectory_error(gold["gt"], gold["traj"], align=False)
    assert torch.equal(n.aligned, gold["traj"][:, gold["assoc"]])
    want = (gold["gt"] - gold["traj"][:, gold["assoc"]]).double().norm(dim=-1).mean(0)
    assert float((n.per_track.double() - want).abs().max()) < 1e-6
    shared = tk.mean_trajectory_error(gold["gt"], gold["traj"], gold["rotations"], assoc=np.full(25, 7, np.int32))
    assert torch.equal(shared.assoc, torch.full((25,), 7)) and shared.aligned.shape == (6, 25, 3)
    # a tie of the default association goes to the smaller index
    tie = tk.mean_trajectory_error(torch.zeros(2, 1, 3), torch.tensor([[[1.0, 0, 0], [0, 1.0, 0], [-1.0, 0, 0]]] * 2), align=False)
    assert tie.assoc.tolist() == [0]


def test_every_malformed_argument_is_a_value_error(gold):
    from csplat import tracking as tk
    X, full, cam, D = gold["traj"], gold["full_proj"], gold["cam_center"], _frames(gold, "depth_raw")
    good = dict(points=X, full_proj=full, cam_center=cam, depth=D, size=(30, 40))

    def bad(match, **kw):
        with pytest.raises(ValueError, match=match):
            tk.track_visibility(**{**good, **kw})

    bad("`points` is", points=torch.zeros(5, 2))
    bad("`points` is", points=torch.zeros(2, 5, 3, 1))
    bad("`points` must be floating", points=torch.zeros(5, 3, dtype=torch.int32))
    bad("`points` is a tensor", points=[[0.0, 0.0, 1.0]])
    bad("frames", points=torch.zeros(0, 5, 3))
    bad("`size`", size=40)
    bad("`size`", size=(0, 40))
    bad("`full_proj` is", full_proj=torch.zeros(3, 4, 4))
    bad("`full_proj` is", full_proj=torch.zeros(4, 3))
    bad("`full_proj` may be None", full_proj=None)
    bad("`cam_center` is", cam_center=torch.zeros(4))
    bad("`cam_center` may be None", cam_center=None)
    bad("`depth` is", depth=torch.zeros(6, 30, 41))
    bad("`depth` is", depth=torch.zeros(30, 40))
    bad("`pixels` is", pixels=torch.zeros(6, 199, 2))
    bad("numbers", depth_threshold=NAN)
    bad("numbers", far_value=NAN)

    gt, rot = gold["gt"], gold["rotations"]

    def bad_mte(match, *a, **kw):
        with pytest.raises(ValueError, match=match):
            tk.mean_trajectory_error(*a, **kw)

    bad_mte("align=True needs `rotations`", gt, X)
    bad_mte(r"\[T,G,3\]", gt[0], X, rot)
    bad_mte("share T", gt[:5], X, rot)
    bad_mte("`rotations` is", gt, X, rot[:, :, :3])
    bad_mte("`assoc` holds", gt, X, rot, assoc=torch.zeros(24, dtype=torch.int64))
    bad_mte("`assoc` holds", gt, X, rot, assoc=torch.zeros(25))
    bad_mte("`assoc` must lie", gt, X, rot, assoc=torch.full((25,), 200))
    bad_mte("`assoc` must lie", gt, X, rot, assoc=torch.full((25,), -1))
    bad_mte("floating point", gt.long(), X, rot)
    with pytest.raises(ValueError, match="`views` is empty"):
        tk.track([], None, None, None, None)


def test_tracks_record_round_trip_and_mte(gold, tmp_path):
    from csplat import tracking as tk
    T, N = 6, 200
    v = tk.track_visibility(gold["traj"], gold["full_proj"], gold["cam_center"], _frames(gold, "depth_raw"), (30, 40))
    tr = tk.Tracks(torch.arange(T, dtype=F64), gold["traj"], gold["rotations"], torch.zeros(T, dtype=torch.int64), torch.arange(T),
                   v.pixels, v.in_image, v.visible, torch.arange(N), v.counts)
    assert tr._fields[:9] == ("times", "traj", "rotations", "view_ids", "time_ids", "pixels", "in_image", "visible", "gt_idxs")
    path = str(tmp_path / "all_trajs.npz")
    tr.save_npz(path)
    back = np.load(path)
    assert sorted(back.files) == ["rotations", "traj"]                      # the keys of the reference's all_trajs.npz
    assert np.array_equal(back["traj"], gold["traj"].numpy()) and np.array_equal(back["rotations"], gold["rotations"].numpy())
    r = tr.mte(gold["gt"])
    assert abs(float(r.mean) - gold["mean"]) < 1e-6 and torch.equal(r.assoc, gold["assoc"])
    assert float(tr.mte(gold["traj"]).mean) == 0.0 and float(tr.mte(gold["traj"], align=False).mean) == 0.0


# ------------------------------------------------------------------------------------------------------------------ the library's surface
def test_header_exports_and_bindings():
    from csplat import native
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "csplat.h")).read()
    for name, n_args in (("csplat_track_visibility", 17), ("csplat_track_mte", 12)):
        assert re.search(r"\b" + name + r"\s*\(", header), name
        assert name in native.EXPORTS and hasattr(native.lib, name) and len(native.EXPORTS[name][1]) == n_args
    block = header[header.index("Point tracking"):header.index("int csplat_track_mte(")]
    assert "Added exports: CSPLAT_ABI_VERSION is unchanged" in block
    for word in ("w > 0", "deliberate divergence", "ZERO quaternion", "C truncation", "min_depth", "INTEGER sums"):
        assert word.lower() in block.lower(), word
    assert native.ABI_VERSION == 9 and native.lib.csplat_abi_version() == 9


def test_the_library_refuses_bad_arguments_before_any_launch():
    from csplat import native
    vis = lambda F=2, N=4, w=8, h=4, pts=16, pix=None, full=16, cam=16, depth=16, thr=0.2, far=1e4, po=16, ii=16, vv=16, cnt=16: \
        native.lib.csplat_track_visibility(None, F, N, w, h, pts, pix, full, cam, depth, thr, 1.0, far, po, ii, vv, cnt)  # noqa: E731
    for kw in (dict(F=0), dict(F=65536), dict(N=-1), dict(N=2 ** 31), dict(w=0), dict(h=0), dict(w=65536, h=65536), dict(pts=None),
               dict(full=None), dict(cam=None), dict(ii=None), dict(vv=None), dict(thr=NAN), dict(far=NAN), dict(pts=18), dict(depth=18),
               dict(pix=17), dict(cnt=18)):
        assert vis(**kw) == 2, kw
        assert b"csplat_track_visibility" in native.lib.csplat_last_error()
    mte = lambda T=2, N=4, G=3, traj=16, rot=16, gt=16, assoc=16, al=16, err=16, m=16, mean=16: \
        native.lib.csplat_track_mte(None, T, N, G, traj, rot, gt, assoc, al, err, m, mean)  # noqa: E731
    for kw in (dict(T=0), dict(N=-1), dict(G=-1), dict(G=2 ** 31), dict(traj=None), dict(gt=None), dict(assoc=None), dict(m=None),
               dict(mean=None), dict(rot=18), dict(al=17)):
        assert mte(**kw) == 2, kw
        assert b"csplat_track_mte" in native.lib.csplat_last_error()
    assert mte(N=0) == 0 and mte(G=0) == 0          # nothing to do: no launch, no error
