"""Edge coverage of the rasterizer's extended outputs -- depth gradient, camera and background gradients, feature channels and the alpha
image, antialiasing, visibility -- at the edges the colour path's tests already reach: wild scenes (util.wild_case), long multi-segment
tile lists up to the global-sort fallback, mixed batches (ragged sizes, per-view Gaussian sets, an empty and an all-culled view, outputs
asked for by some views only) and calls of more than 8 views.  Every image and gradient is checked against tests/antialias_ref.py and
tests/visibility_ref.py (fp64 arithmetic over the tile lists the GPU built: the fp32 C oracle's, which the GPU matches bit for bit), and
batched calls against per-view calls.  Bars: util.image_err 1e-4 for images, util.rel_err 1e-4 for gradients (or the fuzz's rule:
k x the fp32 oracle's own error where it cannot reach 1e-4 itself); batched vs per-view: images and visibility bit-equal, gradients and
camera gradients 1e-5, in the bit-reproducible mode (csplat_debug_flags bit 8)."""
import numpy as np
import pytest

import util
import antialias_ref
import visibility_ref
from util import image_err, make_case, oracle_forward, rel_err

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

TOL = 1e-4
CAM_KEYS = ("view", "proj", "campos", "bg")
GKEYS = ("means3D", "opacities", "shs", "scales", "rotations")


def _flags(f):
    from csplat import native
    native.lib.csplat_debug_flags(f)


def _np(t):
    return t.detach().cpu().numpy()


# ------------------------------------------------------------------------------------------------ views, GPU calls, fp64 restatement
def _view(case, F=0, alpha=False, vis=False, depth=True, seed=0):
    """one view of a call: its scene, F feature channels (0: none), which extra outputs it asks for and the weights of its loss"""
    rng = np.random.default_rng(seed)
    H, W, P = case["H"], case["W"], case["P"]
    return dict(case=case, F=F, alpha=alpha, vis=vis, feats=rng.normal(size=(P, F)).astype(np.float32) if F else None,
                wts=dict(color=rng.normal(size=(3, H, W)), depth=rng.normal(size=(1, H, W)) if depth else None,
                         feat=rng.normal(size=(F, H, W)) if F else None, alpha=rng.normal(size=(1, H, W)) if alpha else None))


def _loss(v, color, depth, feat, alpha, t):
    w = v["wts"]
    s = (color * t(w["color"])).sum()
    if w["depth"] is not None:
        s = s + (depth * t(w["depth"])).sum()
    if feat is not None:
        s = s + (feat * t(w["feat"])).sum()
    if alpha is not None:
        s = s + (alpha * t(w["alpha"])).sum()
    return s


def _gpu(views, aa=False, cam=False, shared=False, batched=True, flags=256):
    """views in one rasterize_views call (batched) or one call per view; shared: every view renders views[0]'s Gaussian (and feature)
    tensors.  -> per view dict(imgs=[color, depth, feat, alpha], vis=Visibility or None, radii, grads={name: array}, cam={key: array})"""
    import diff_gaussian_rasterization as dgr
    dev = "cuda"
    f32 = lambda a, rg=True: torch.tensor(np.asarray(a, np.float32), device=dev, requires_grad=rg)  # noqa: E731
    t = lambda a: torch.tensor(np.asarray(a, np.float32), device=dev)  # noqa: E731
    _flags(flags)
    try:
        inps, feats, leaves, settings, kws = [], [], [], [], []
        for i, v in enumerate(views):
            case = v["case"]
            if shared and i > 0:
                inp = dict(inps[0], means2D=torch.zeros(case["P"], 3, device=dev, requires_grad=True))
                f = feats[0]
            else:
                inp = util.gpu_inputs(case)
                f = f32(v["feats"]) if v["F"] else None
            inps.append(inp)
            feats.append(f)
            c = case["cam"]
            lv = dict(view=f32(c["world_view_transform"], cam), proj=f32(c["full_proj_transform"], cam),
                      campos=f32(c["camera_center"], cam), bg=f32(case["bg"], cam))
            leaves.append(lv)
            settings.append(util.gpu_settings(case)._replace(viewmatrix=lv["view"], projmatrix=lv["proj"], campos=lv["campos"], bg=lv["bg"]))
            kw = {k: inp[k] for k in GKEYS + ("means2D",)}
            kw.update(antialiasing=aa, return_alpha=v["alpha"], return_visibility=v["vis"])
            if f is not None:
                kw["features"] = f
            kws.append(kw)
        if batched:
            outs = dgr.rasterize_views(settings, kws)
        else:
            outs = [dgr.rasterize_views([s], [k])[0] for s, k in zip(settings, kws)]
        loss = 0.0
        res = []
        for v, o in zip(views, outs):
            o = list(o)
            vis = o.pop() if v["vis"] else None
            color, radii, depth = o[:3]
            feat = o[3] if v["F"] else None
            alpha = o[-1] if v["alpha"] else None
            loss = loss + _loss(v, color, depth, feat, alpha, t)
            res.append(dict(imgs=[color, depth, feat, alpha], vis=vis, radii=radii))
        loss.backward()
        torch.cuda.synchronize()
    finally:
        _flags(0)
    for i, r in enumerate(res):
        inp = inps[i]
        r["imgs"] = [None if x is None else _np(x).astype(np.float64) for x in r["imgs"]]
        r["radii"] = _np(r["radii"])
        if r["vis"] is not None:
            r["vis"] = [_np(x) for x in r["vis"]]
        g = {k: inp[k].grad for k in GKEYS + ("means2D",)}
        if feats[i] is not None:
            g["features"] = feats[i].grad
        r["grads"] = {k: (None if x is None else _np(x).astype(np.float64)) for k, x in g.items()}
        r["cam"] = {k: _np(leaves[i][k].grad).astype(np.float64) for k in CAM_KEYS} if cam else None
    return res


def _gpu_lists(case):
    """the colour-only forward's saved state (lists, n_contrib) and a check that its lists are the fp32 C oracle's, bit for bit"""
    o = oracle_forward(case)
    _c, _r, _d, st = util.gpu_forward_raw(case, settings=util.gpu_settings(case))
    assert st["R"] == o.R
    np.testing.assert_array_equal(st["ids"], o.ids)
    np.testing.assert_array_equal(st["ranges"], o.ranges)
    return o, st


def _ref(v, aa=False, o=None):
    """fp64 autograd through antialias_ref.render over the fp32 C oracle's lists -> imgs, grads, cam grads, visibility restatement"""
    case = v["case"]
    g, P = case["g"], case["P"]
    o = o if o is not None else oracle_forward(case)
    T = lambda a: torch.tensor(np.asarray(a, np.float64), requires_grad=True)  # noqa: E731
    cam = dict(zip(CAM_KEYS, antialias_ref.camera_tensors(o)))
    ins = {k: T(g[k]) for k in GKEYS}
    m2 = T(np.zeros((P, 3)))
    f = T(v["feats"]) if v["F"] else None
    c, d, fi, a, ncon, _aux = antialias_ref.render(o, ins["means3D"], m2, ins["opacities"], cam["view"], cam["proj"], cam["campos"],
                                                   cam["bg"], f, shs=ins["shs"], scales=ins["scales"], rotations=ins["rotations"],
                                                   antialiasing=aa)
    _loss(v, c, d, fi, a if v["alpha"] else None, torch.tensor).backward()
    grads = {k: ins[k].grad.numpy() for k in GKEYS}
    grads["means2D"] = m2.grad.numpy()
    if f is not None:
        grads["features"] = f.grad.numpy()
    imgs = [c.detach().numpy(), d.detach().numpy(), None if fi is None else fi.detach().numpy(), a.detach().numpy()]
    f64 = lambda a: torch.tensor(np.asarray(a, np.float64))  # noqa: E731
    V, Pm, _cp, _bg = antialias_ref.camera_tensors(o, False)
    vis = visibility_ref.visibility(o, f64(g["means3D"]), f64(g["opacities"]), V, Pm, scales=f64(g["scales"]),
                                    rotations=f64(g["rotations"]), antialiasing=aa) if v["vis"] else None
    # (None: no path from that tensor to the loss -- campos at SH degree 0)
    return dict(imgs=imgs, grads=grads, cam={k: None if cam[k].grad is None else cam[k].grad.numpy() for k in CAM_KEYS}, ncon=ncon.numpy(),
                vis=vis, o=o)


def _oracle_colour_err(case, wts):
    """the fp32 C oracle's own error against the fp64 one on the colour gradients of this case (the conditioning of its sums)"""
    o32, o64 = oracle_forward(case), oracle_forward(case, dtype=np.float64)
    dpix = np.asarray(wts["color"], np.float32)
    g32, g64 = util.ro.backward(o32, dpix), util.ro.backward(o64, dpix)
    return max(rel_err(getattr(g32, k), getattr(g64, k)) for k in ("mean3D", "opacity", "sh", "scale", "rot")), \
        max(image_err(o32.color, o64.color, outlier_frac=1e-3), image_err(o32.out_depth, o64.out_depth, outlier_frac=1e-3))


def _compare_fp64(got, ref, v, bar=TOL, img_bar=TOL, cam=True, what=""):
    """images, every gradient and (cam) the camera / background gradients of one view against the fp64 restatement"""
    names = ("color", "depth", "feat", "alpha")
    for name, a, b in zip(names, got["imgs"], ref["imgs"]):
        if a is None:
            continue
        assert np.isfinite(a).all(), (what, name)
        e = image_err(a, b, outlier_frac=1e-3)
        assert e < img_bar, (what, name, e, img_bar)
    for k, b in ref["grads"].items():
        a = got["grads"][k]
        assert a is not None and np.isfinite(a).all(), (what, k)
        e = rel_err(a, b)
        assert e < bar, (what, k, e, bar)
    if cam:
        for k in CAM_KEYS:
            a, b = got["cam"][k], ref["cam"][k]
            assert np.isfinite(a).all(), (what, k)
            if b is None:
                assert not np.any(a), (what, k)
                continue
            e = rel_err(a, b)
            assert e < bar, (what, k, e, bar)
        # the view matrix' column 3 and the projection's column 2 take no gradient (include/csplat.h, ABI 8)
        assert np.all(got["cam"]["view"].reshape(4, 4)[:, 3] == 0.0) and np.all(got["cam"]["proj"].reshape(4, 4)[:, 2] == 0.0), what


def _compare_vis(got, ref, what=""):
    wm, ws, pc, top = got["vis"]
    r = ref["vis"]
    assert rel_err(wm, r["weight_max"]) < TOL, (what, rel_err(wm, r["weight_max"]))
    assert rel_err(ws, r["weight_sum"]) < TOL, (what, rel_err(ws, r["weight_sum"]))
    d = np.abs(pc.astype(np.int64) - r["pixel_count"])
    assert d.sum() <= max(4, 1e-3 * r["pixel_count"].sum()), (what, int(d.sum()), int(r["pixel_count"].sum()))
    assert np.array_equal(top[0] == -1, got["imgs"][3][0] == 0) if got["imgs"][3] is not None else True


def _check_consistent(got):
    """the identities inside one GPU result (tests/test_visibility_gpu.py) -- they hold whatever the conditioning"""
    wm, ws, pc, top = got["vis"]
    alpha = got["imgs"][3]
    assert np.array_equal(wm > 0, pc > 0) and np.array_equal(ws > 0, pc > 0)
    assert np.all(got["radii"][pc > 0] > 0)
    assert wm.max(initial=0.0) <= np.float32(0.99) and wm.min(initial=0.0) >= 0.0
    assert np.array_equal(top[0] == -1, alpha[0] == 0)
    ids = top[top >= 0]
    assert np.all(np.bincount(ids, minlength=wm.shape[0]) <= pc)
    assert abs(ws.astype(np.float64).sum() - alpha.sum()) <= 1e-5 * max(alpha.sum(), 1.0)


# ------------------------------------------------------------------------------------------------ A. wild scenes
def _wild_seeds():
    return util.fuzz_seeds("CSPLAT_EDGE_FUZZ_SEEDS", "100:112")


def _wild_view(seed, needles):
    case = util.wild_case(seed, needles=needles)
    F = int(np.random.default_rng(seed + 7).integers(1, 7))
    return _view(case, F=F, alpha=True, vis=True, depth=True, seed=seed)


@pytest.mark.parametrize("seed", _wild_seeds())
def test_wild_tame_scenes_every_output_matches_fp64(seed):
    """wild_case(needles=False): features (F of 1..6), alpha, depth in the loss, camera and background gradients and visibility, with and
    without antialiasing, against fp64 over the GPU's own lists.  Bar: 1e-4, or 10x the fp32 oracle's own error on the scene's colour
    gradients where that is larger (the sums of the scene are that ill-conditioned in fp32 whoever computes them)."""
    v = _wild_view(seed, needles=False)
    case = v["case"]
    o, st = _gpu_lists(case)
    e32, i32 = _oracle_colour_err(case, v["wts"])
    bar, img_bar = max(TOL, 10.0 * e32), max(TOL, 10.0 * i32)
    for aa in (False, True):
        got = _gpu([v], aa=aa, cam=True)[0]
        np.testing.assert_array_equal(got["radii"], o.radii)
        ref = _ref(v, aa, o)
        if not aa:     # the restatement's own termination is the GPU's (but for threshold ties)
            assert (ref["ncon"] != st["n_contrib"].astype(np.int64)).mean() < 2e-3
        _compare_fp64(got, ref, v, bar, img_bar, what=f"seed {seed} aa={aa}")
        _check_consistent(got)
        _compare_vis(got, ref, what=f"seed {seed} aa={aa}")
    assert int((o.radii > 0).sum()) > 0       # (the scene draws something)


@pytest.mark.parametrize("seed", _wild_seeds())
def test_wild_scenes_with_needles_identities(seed):
    """wild_case with its needles: no fp64 bar (fp32 cannot hold the needles to it), but what conditioning cannot spoil -- every output
    finite, the visibility identities, features = precomputed colours gives feat = colour - (1 - alpha) bg, features = view-space z gives
    feat = the depth image, sum weight_sum = sum alpha"""
    case = util.wild_case(seed)
    o = oracle_forward(case)
    rng = np.random.default_rng(seed)
    colors = rng.uniform(0, 1, size=(case["P"], 3)).astype(np.float32)
    Vm = np.asarray(case["cam"]["world_view_transform"], np.float64).reshape(4, 4)
    z = (np.c_[case["g"]["means3D"].astype(np.float64), np.ones(case["P"])] @ Vm)[:, 2:3].astype(np.float32)
    import diff_gaussian_rasterization as dgr
    for aa in (False, True):
        inp = util.gpu_inputs(case, requires_grad=False)
        t = lambda a: torch.tensor(a, device="cuda")  # noqa: E731
        rs = util.gpu_settings(case)
        base = dict(means3D=inp["means3D"], means2D=inp["means2D"], opacities=inp["opacities"], scales=inp["scales"],
                    rotations=inp["rotations"], antialiasing=aa, return_alpha=True)
        col, radii, _d, feat, alpha, vis = dgr.GaussianRasterizer(rs)(colors_precomp=t(colors), features=t(colors), return_visibility=True,
                                                                       **base)
        col, feat, alpha = (_np(x).astype(np.float64) for x in (col, feat, alpha))
        bg = case["bg"].astype(np.float64)[:, None, None]
        for x in (col, feat, alpha):
            assert np.isfinite(x).all()
        assert np.abs(feat - (col - (1.0 - alpha) * bg)).max() <= 1e-5 * max(1.0, np.abs(col).max())
        got = dict(imgs=[col, None, feat, alpha], radii=_np(radii), vis=[_np(x) for x in vis])
        _check_consistent(got)
        np.testing.assert_array_equal(got["radii"], o.radii)
        _c2, _r2, depth, featz, _a2 = dgr.GaussianRasterizer(rs)(shs=inp["shs"], features=t(z), **base)
        depth, featz = _np(depth).astype(np.float64), _np(featz).astype(np.float64)
        assert np.isfinite(depth).all()
        assert np.abs(featz - depth).max() <= 1e-5 * max(1.0, np.abs(depth).max())


# ------------------------------------------------------------------------------------------------ B. long lists, segment boundaries
def _prefix(case, P):
    c = dict(case, P=P)
    c["g"] = {k: v[:P].copy() for k, v in case["g"].items()}
    return c


def _longest(case):
    o = oracle_forward(case)
    return int((o.ranges[:, 1] - o.ranges[:, 0]).max())


def _exact_longest(case, target):
    """the shortest prefix of the cloud whose longest tile list has exactly `target` entries (adding one Gaussian adds at most one entry
    to any list, so the longest list grows by 0 or 1 along the prefixes)"""
    lo, hi = 1, case["P"]
    assert _longest(case) >= target
    while lo < hi:
        mid = (lo + hi) // 2
        if _longest(_prefix(case, mid)) >= target:
            hi = mid
        else:
            lo = mid + 1
    c = _prefix(case, lo)
    assert _longest(c) == target
    return c


LISTS = {    # name -> (make_case arguments, the range its longest list must fall in, or an exact length)
    "short": (dict(P=120, W=40, H=36, seed=21, grid=12, scale_mul=6.0, radius=3.0), (1, 256)),
    "seg_multiple": (dict(P=1500, W=48, H=40, seed=21, grid=12, scale_mul=6.0, radius=3.0), 768),
    "2k": (dict(P=2500, W=64, H=48, seed=21, grid=12, scale_mul=6.0, radius=3.0), (1500, 2500)),
    "8k": (dict(P=10000, W=64, H=48, seed=21, grid=12, scale_mul=6.0, radius=3.0), (7000, 8192)),
    "global_sort": (dict(P=11000, W=32, H=32, seed=21, grid=12, scale_mul=6.0, radius=3.0), (8193, 20000)),
}


def _list_case(name, regime):
    cfg, want = LISTS[name]
    case = make_case(**cfg)
    if isinstance(want, int):
        case = _exact_longest(case, want)
    g = case["g"] = dict(case["g"])
    if regime == "translucent":
        g["opacities"] = np.full_like(g["opacities"], 0.02) + 0.01 * (g["opacities"] - 0.5)
    else:
        g["opacities"] = np.clip(g["opacities"] + 0.95, 0.95, 0.995).astype(np.float32)
    g["opacities"] = g["opacities"].astype(np.float32)
    return case, want


@pytest.mark.parametrize("regime", ["translucent", "opaque"])
@pytest.mark.parametrize("name", list(LISTS))
def test_long_lists_every_output_matches_fp64(name, regime):
    """colour, depth, features, alpha, visibility and every gradient (camera and background included) on lists of 1..256 entries, of
    exactly 3 segments, of ~2k, of ~8k and of more than 8192 entries (the global-sort fallback).  Translucent: some pixel
    blends more than 4 segments deep (n_contrib > 1024 where the list is that long); opaque: most pixels stop in segment 0 while the
    list runs on.  Bar: 1e-4, or 10x the fp32 oracle's own error where a sum of thousands of terms is beyond fp32's 1e-4."""
    case, want = _list_case(name, regime)
    o, st = _gpu_lists(case)
    L = (o.ranges[:, 1] - o.ranges[:, 0])
    longest = int(L.max())
    if isinstance(want, int):
        assert longest == want and longest % 256 == 0
    else:
        assert want[0] <= longest <= want[1], longest
    nc = st["n_contrib"].astype(np.int64)
    if regime == "translucent" and longest > 1100:
        assert int(nc.max()) > 4 * 256, int(nc.max())
    if regime == "opaque" and longest > 256:
        # (measured: 0.50 of the pixels stop in segment 0 on the 8k and global-sort lists, 0.8-0.9 on the shorter ones; the rest lie
        # where only the far tails of the large footprints reach, alphas under the 1/255 skip that the walk steps over)
        assert (nc <= 256).mean() >= 0.45 and int(nc.max()) < longest, float((nc <= 256).mean())
    v = _view(case, F=3, alpha=True, vis=True, depth=True, seed=5)
    e32, i32 = _oracle_colour_err(case, v["wts"])
    bar, img_bar = max(TOL, 10.0 * e32), max(TOL, 10.0 * i32)
    got = _gpu([v], aa=False, cam=True)[0]
    ref = _ref(v, False, o)
    assert np.array_equal(ref["ncon"], nc) or (ref["ncon"] != nc).mean() < 1e-3
    _compare_fp64(got, ref, v, bar, img_bar, what=f"{name} {regime} L={longest} bar={bar:.1e}")
    _check_consistent(got)
    _compare_vis(got, ref, what=f"{name} {regime}")


# ------------------------------------------------------------------------------------------------ C. mixed batches
def _culled(case):
    """the case with every Gaussian moved behind the camera (view-space z = -1): all culled"""
    Vm = np.asarray(case["cam"]["world_view_transform"], np.float64).reshape(4, 4)
    axis = Vm[:3, 2] / np.dot(Vm[:3, 2], Vm[:3, 2])
    m = case["g"]["means3D"].astype(np.float64)
    pz = m @ Vm[:3, 2] + Vm[3, 2]
    c = dict(case)
    c["g"] = dict(case["g"], means3D=(m + np.outer(-1.0 - pz, axis)).astype(np.float32))
    return c


def _empty(like):
    c = dict(like, P=0)
    c["g"] = {k: v[:0].copy() for k, v in like["g"].items()}
    return c


def _mixed_views(F=2, seed=0):
    """5 views: ragged sizes (97x61, 33x200), a Gaussian set of its own in each, an empty view, an all-culled view; alpha, visibility and
    a depth term on some views only, the same F in every view"""
    a = make_case(P=1400, W=97, H=61, seed=3 + seed, scale_mul=2.0)
    b = make_case(P=600, W=33, H=200, seed=9 + seed, theta=30.0, scale_mul=3.0)
    c = make_case(P=900, W=64, H=48, seed=11 + seed, theta=-20.0, scale_mul=1.5)
    d = _culled(make_case(P=300, W=50, H=30, seed=13 + seed))
    e = _empty(make_case(P=10, W=40, H=24, seed=15 + seed))
    return [_view(a, F, alpha=True, vis=True, depth=True, seed=1), _view(b, F, alpha=False, vis=True, depth=False, seed=2),
            _view(e, F, alpha=True, vis=False, depth=True, seed=3), _view(d, F, alpha=True, vis=True, depth=True, seed=4),
            _view(c, F, alpha=False, vis=False, depth=True, seed=5)]


def _equal_batched_per_view(bat, one, cam, what=""):
    for i, (x, y) in enumerate(zip(bat, one)):
        for a, b in zip(x["imgs"], y["imgs"]):
            assert (a is None) == (b is None) and (a is None or np.array_equal(a, b)), (what, i)
        np.testing.assert_array_equal(x["radii"], y["radii"])
        if x["vis"] is not None:
            for a, b in zip(x["vis"], y["vis"]):
                assert np.array_equal(a, b), (what, i)
        for k, b in y["grads"].items():
            a = x["grads"][k]
            if b is None or b.size == 0:
                assert a is None or not np.any(a), (what, i, k)
                continue
            assert rel_err(a, b) < 1e-5 if np.abs(b).max() > 0 else not np.any(a), (what, i, k, rel_err(a, b))
        if cam:     # (1e-5: a per-view call sums its K8 slab in other rows than the batched K8 -- measured up to 1.1e-6 on campos)
            for k in CAM_KEYS:
                assert rel_err(x["cam"][k], y["cam"][k]) < 1e-5 or (not np.any(x["cam"][k]) and not np.any(y["cam"][k])), (what, i, k)


@pytest.mark.parametrize("aa", [False, True])
@pytest.mark.parametrize("cam", [False, True])
def test_mixed_batch_equals_per_view_calls_and_fp64(cam, aa):
    views = _mixed_views()
    assert any(v["case"]["W"] % 4 or v["case"]["H"] % 4 for v in views)
    assert views[2]["case"]["P"] == 0
    bat = _gpu(views, aa=aa, cam=cam)
    one = _gpu(views, aa=aa, cam=cam, batched=False)
    _equal_batched_per_view(bat, one, cam, what=f"cam={cam} aa={aa}")
    # the empty view: background colour, zero depth / features / alpha; the all-culled view: the same, and no radius
    for i in (2, 3):
        c = views[i]["case"]
        g = bat[i]
        assert np.array_equal(g["imgs"][0], np.broadcast_to(c["bg"].astype(np.float64)[:, None, None], g["imgs"][0].shape))
        assert not np.any(g["imgs"][1]) and not np.any(g["imgs"][2]) and not np.any(g["imgs"][3])
    assert bat[3]["radii"].size == 300 and not np.any(bat[3]["radii"])
    if cam:     # all background: dL/dbg = the sum of the colour weights, and no camera gradient
        for i in (2, 3):
            want = views[i]["wts"]["color"].sum((1, 2))
            assert np.abs(bat[i]["cam"]["bg"] - want).max() <= 1e-5 * np.abs(want).max(), (i, bat[i]["cam"]["bg"], want)
            assert not any(np.any(bat[i]["cam"][k]) for k in ("view", "proj", "campos")), i
    assert not np.any(bat[3]["vis"][0]) and np.all(bat[3]["vis"][3] == -1)
    for i in (0, 1, 4):
        ref = _ref(views[i], aa)
        _compare_fp64(bat[i], ref, views[i], cam=cam, what=f"view {i} cam={cam} aa={aa}")
        if views[i]["vis"]:
            _compare_vis(bat[i], ref, what=f"view {i}")


# ------------------------------------------------------------------------------------------------ D. more than 8 views
def _equal_views(V, W=64, H=48, P=1500, F=2):
    from csplat import synthetic as syn
    base = make_case(P=P, W=W, H=H, seed=7, scale_mul=1.5)
    return [dict(base, cam=syn.make_camera(-60.0 + 120.0 * i / (V - 1), W, H)) for i in range(V)]


PATHS = {    # which outputs every view asks for, and whether the call takes camera / background gradients
    "features_alpha": dict(F=2, alpha=True, vis=False, depth=False, cam=False, aa=False),
    "visibility": dict(F=0, alpha=False, vis=True, depth=False, cam=False, aa=False),
    "depth": dict(F=0, alpha=False, vis=False, depth=True, cam=False, aa=False),
    "camera_bg": dict(F=0, alpha=False, vis=False, depth=False, cam=True, aa=False),
    "antialiased_all": dict(F=3, alpha=True, vis=True, depth=True, cam=True, aa=True),
}


@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("V", [9, 17])
def test_more_than_8_views_shared_gaussians(V, path):
    """V = 9 and 17 equal-size views of ONE Gaussian set (and one feature tensor): the library runs them in groups of at most 8 views
    that add into the same gradient buffers; equal to V per-view calls"""
    p = PATHS[path]
    views = [_view(c, F=p["F"], alpha=p["alpha"], vis=p["vis"], depth=p["depth"], seed=i) for i, c in enumerate(_equal_views(V))]
    bat = _gpu(views, aa=p["aa"], cam=p["cam"], shared=True)
    one = _gpu(views, aa=p["aa"], cam=p["cam"], shared=True, batched=False)
    assert len(bat) == V > 8
    _equal_batched_per_view(bat, one, p["cam"], what=f"V={V} {path}")


@pytest.mark.parametrize("aa", [False, True])
def test_more_than_8_mixed_views(aa):
    """11 views: the 5 mixed views of C, then 6 more of their own Gaussian sets, every output and camera gradients, against per-view
    calls; the last view is also checked against fp64"""
    views = _mixed_views() + _mixed_views(seed=1)[:2] + [_view(make_case(P=500 + 100 * i, W=40 + 3 * i, H=36, seed=40 + i), 2,
                                                               alpha=bool(i % 2), vis=True, depth=bool(i % 2 == 0), seed=40 + i)
                                                         for i in range(4)]
    assert len(views) == 11
    bat = _gpu(views, aa=aa, cam=True)
    one = _gpu(views, aa=aa, cam=True, batched=False)
    _equal_batched_per_view(bat, one, True, what=f"11 mixed aa={aa}")
    ref = _ref(views[-1], aa)
    _compare_fp64(bat[-1], ref, views[-1], what="view 10")
    _compare_vis(bat[-1], ref, what="view 10")
