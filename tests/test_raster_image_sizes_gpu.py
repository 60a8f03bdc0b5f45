"""The rasterizer from a 1-pixel image to beyond BUCKET_TILES = 12288 tiles, where its host code leaves the tile-bucket path on its own (no
bucket table, no mailbox, rasterize_views view by view, P-scan + k_emit_keys + global radix sort + k_tile_ranges) -- the sizes and scenes of
tests/image_sizes_ref.py, whose claims tests/test_raster_image_sizes_cpu.py holds.

Bars (none new): lists, keys, ranges, radii, tiles_touched bit-exact against the fp32 C oracle; images image_err 1e-4 (tests/test_raster_gpu.py);
gradients rel_err 1e-4, or 10 x the fp32 oracle's own error against the fp64 oracle where that is larger (the rule of
test_raster_extended_edges_gpu._oracle_colour_err); extended outputs through _compare_fp64 / _compare_vis / _check_consistent of that file,
unchanged (the degenerate grids; over the limit the restatement costs seconds per case, see test_extended_outputs_over_the_limit);
batched against per-view calls: images and visibility bit-equal, gradients 1e-5 in the bit-reproducible mode.  On images of
fewer pixels than 1 / outlier_frac, image_sizes_ref.image_err exempts no pixel.

The tests print e32 (fp32 oracle against fp64 oracle) / bar / kernel error per case: pytest -s."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest

import util
import image_sizes_ref as S
import test_raster_extended_edges_gpu as E
from image_sizes_ref import SIZES
from util import oracle_forward, rel_err

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

TOL = 1e-4
K = 10.0            # the factor of the extended-edge tests on the fp32 oracle's own error
GRADS = ("mean3D", "mean2D", "opacity", "sh", "scale", "rot")
ORACLE_KEYS = ("mean3D", "opacity", "sh", "scale", "rot")       # what _oracle_colour_err takes the oracle's own error over


def _flags(f):
    from csplat import native
    native.lib.csplat_debug_flags(f)


# ------------------------------------------------------------------------------------------------ 2. colour path, single view
@functools.lru_cache(maxsize=1)
def _colour(name):
    """scene, both oracles and their backwards, kept for the LAST size asked for only: the size is the outer loop of the stacked
    parametrize decorators below (the decorator next to the function), so the four flag runs of a size come back to back; in any
    other order the cache only costs the oracle runs again.  _drop_cached_scene frees the last one behind the module."""
    case = S.colour_case(name)
    o, o64 = oracle_forward(case), oracle_forward(case, dtype=np.float64)
    return SimpleNamespace(case=case, o=o, o64=o64)


@functools.lru_cache(maxsize=1)
def _colour_grads(name):
    """_colour(name) with the loss weights and both oracle backwards (the backward tests only)"""
    c = _colour(name)
    W, H = SIZES[name]
    dpix = np.random.default_rng(3).normal(size=(3, H, W)).astype(np.float32)
    return SimpleNamespace(case=c.case, o=c.o, o64=c.o64, dpix=dpix, g32=util.ro.backward(c.o, dpix), g64=util.ro.backward(c.o64, dpix))


@pytest.fixture(scope="module", autouse=True)
def _drop_cached_scene():
    yield
    _colour_grads.cache_clear()
    _colour.cache_clear()       # (the 4096 x 4112 oracles and weights: several hundred MB)


def _forward(case, flags):
    _flags(flags)
    try:
        color, radii, depth, st = util.gpu_forward_raw(case)
    finally:
        _flags(0)
    st.pop("_binning_raw")
    st.update(color=color.cpu().numpy(), out_depth=depth.cpu().numpy(), radii=radii.cpu().numpy())
    return st


@pytest.mark.parametrize("name", list(SIZES))
def test_lists_bit_exact_and_image(name):
    """every size, default flags: R, radii, tiles_touched, per-Gaussian depth / xy, sorted keys, ids and tile ranges bit-exact; colour, depth
    and final_T within 1e-4 of the fp64 and the fp32 oracle, in both forms of K6.  Over the limit the natural path must be bit for bit the
    forced one (csplat_debug_flags bit 1), and at the two large bucket sizes the bucket path must be bit for bit the global sort."""
    c = _colour(name)
    case, o, o64 = c.case, c.o, c.o64
    st = _forward(case, 0)
    assert st["R"] == o.R
    np.testing.assert_array_equal(st["radii"], o.radii)
    np.testing.assert_array_equal(st["tiles_touched"], o.tiles_touched)
    np.testing.assert_array_equal(st["depth"].view(np.uint32), o.depth.view(np.uint32))
    np.testing.assert_array_equal(st["xy"].view(np.uint32), o.xy.view(np.uint32))
    np.testing.assert_array_equal(st["keys"], o.keys)
    np.testing.assert_array_equal(st["ids"], o.ids)
    np.testing.assert_array_equal(st["ranges"], o.ranges)
    if name in S.OVER_LIMIT:        # (the P-scan of the global-sort path)
        np.testing.assert_array_equal(st["offsets"], np.cumsum(o.tiles_touched, dtype=np.uint64).astype(np.uint32))
    for form, got in (("columns", st), ("rows", _forward(case, 32768))):
        assert np.isfinite(got["color"]).all() and np.isfinite(got["out_depth"]).all()
        errs = [S.image_err(got["color"], o64.color), S.image_err(got["out_depth"], o64.out_depth), S.image_err(got["final_T"], o.final_T)]
        if form == "columns":       # (the row form differs from it in the order of a pixel's sums only: the fp64 oracle is enough)
            errs += [S.image_err(got["color"], o.color), S.image_err(got["out_depth"], o.out_depth)]
        print(f"{name} K6 {form}: colour, depth against fp64, final_T against fp32 (, colour, depth against fp32) / bar: "
              + " ".join(f"{e:.2e}" for e in errs) + f" / {TOL:.0e}")
        assert max(errs) < TOL, (form, errs)
        assert (got["n_contrib"] != o.n_contrib).mean() < 2e-4
        np.testing.assert_array_equal(got["ids"], o.ids)
    if name in S.OVER_LIMIT + S.LAST_BUCKET:
        forced = _forward(case, 2)
        for k in ("R", "keys", "ids", "ranges", "radii", "tiles_touched", "n_contrib", "final_T", "color", "out_depth"):
            assert np.array_equal(st[k], forced[k]), k


def _bars(c, rows=None):
    """max(1e-4, 10 x the fp32 oracle's own error over the colour gradients) -- over all Gaussians, or over `rows` of them"""
    sub = lambda a: np.asarray(a, np.float64).reshape(c.case["P"], -1)[slice(None) if rows is None else rows]  # noqa: E731
    e32 = max(rel_err(sub(getattr(c.g32, k)), sub(getattr(c.g64, k))) for k in ORACLE_KEYS)
    return e32, max(TOL, K * e32), sub


@pytest.mark.parametrize("flags", [0, 256, 32768, 256 | 32768], ids=["k7_atomics", "k7_reproducible", "k6_rows", "k6_rows_k7_reproducible"])
@pytest.mark.parametrize("name", list(SIZES))
def test_backward_grads(name, flags):
    """every size, both K7 modes behind both K6 forms: the six gradients against the fp64 oracle, over all Gaussians and once more over the
    3000 cloth Gaussians alone (so that the large gradients of the markers cannot carry the small ones)"""
    import diff_gaussian_rasterization as dgr
    c = _colour_grads(name)
    case = c.case
    _flags(flags)
    try:
        inp = util.gpu_inputs(case)
        color, radii, _depth = dgr.GaussianRasterizer(util.gpu_settings(case))(
            means3D=inp["means3D"], means2D=inp["means2D"], opacities=inp["opacities"], shs=inp["shs"], scales=inp["scales"],
            rotations=inp["rotations"])
        (color * torch.tensor(c.dpix, device="cuda")).sum().backward()
        torch.cuda.synchronize()
    finally:
        _flags(0)
    np.testing.assert_array_equal(radii.cpu().numpy(), c.o.radii)
    got = dict(mean3D=inp["means3D"].grad, mean2D=inp["means2D"].grad, opacity=inp["opacities"].grad.reshape(-1), sh=inp["shs"].grad,
               scale=inp["scales"].grad, rot=inp["rotations"].grad)
    got = {k: v.cpu().numpy() for k, v in got.items()}
    for what, rows in (("all", None), ("cloth", slice(0, 3000))):
        e32, bar, sub = _bars(c, rows)
        errs = {k: rel_err(sub(got[k]), sub(getattr(c.g64, k))) for k in GRADS}
        print(f"{name} flags {flags} {what}: e32 / bar / kernel  {e32:.2e} / {bar:.2e} / {max(errs.values()):.2e}  "
              + " ".join(f"{k} {v:.1e}" for k, v in errs.items()))
        for k, e in errs.items():
            assert np.isfinite(got[k]).all() and e < bar, (name, what, k, e, bar)


# ------------------------------------------------------------------------------------------------ 3. the batched entry over the limit
def _view(case, F=0, alpha=False, vis=False, depth=True, seed=0, feats=None):
    """E._view with loss weights that repeat one random 61 x 67 block over the image (drawing 7 x 8 M normal deviates per view costs
    more than the render they weigh)"""
    rng = np.random.default_rng(seed)
    H, W, P = case["H"], case["W"], case["P"]

    def wt(C):
        return np.tile(rng.normal(size=(C, 61, 67)), (1, H // 61 + 1, W // 67 + 1))[:, :H, :W]
    feats = rng.normal(size=(P, F)).astype(np.float32) if F and feats is None else feats
    return dict(case=case, F=F, alpha=alpha, vis=vis, feats=feats,
                wts=dict(color=wt(3), depth=wt(1) if depth else None, feat=wt(F) if F else None, alpha=wt(1) if alpha else None))


def _shared_views(name, V, F=1):
    from csplat import synthetic as syn
    W, H = SIZES[name]
    base = S.colour_case(name)
    cams = [syn.make_camera(-40.0 + 80.0 * i / (V - 1), W, H) for i in range(V)]
    return [_view(dict(base, cam=cam), F=F, alpha=True, vis=True, depth=True, seed=i) for i, cam in enumerate(cams)]


@pytest.mark.parametrize("V", [2, 4])
@pytest.mark.parametrize("name", list(S.EXTENDED_OVER))
def test_batched_views_over_the_limit_equal_per_view_calls(name, V):
    """rasterize_views with V views of one Gaussian set over the tile limit (the library goes view by view): colour, depth, feature and
    alpha images and visibility bit-equal to V calls of one view, gradients (camera and background included) within 1e-5 in the
    bit-reproducible mode -- the bars of test_raster_extended_edges_gpu.test_more_than_8_views_shared_gaussians"""
    views = _shared_views(name, V)
    assert all(S.tiles_of(v["case"]["W"], v["case"]["H"]) > S.BUCKET_TILES for v in views)
    bat = E._gpu(views, cam=True, shared=True)
    one = E._gpu(views, cam=True, shared=True, batched=False)
    E._equal_batched_per_view(bat, one, True, what=f"{name} V={V}")
    for r in bat:
        assert all(np.isfinite(x).all() for x in r["imgs"]) and r["imgs"][3].max() > 0.5 and np.any(r["grads"]["means3D"])


def test_mixed_batch_under_over_and_one_tile_row():
    """one call with a 2048 x 1536 view (the last bucket size), a 2064 x 1536 view (over the limit) and a 17 x 1 view, each with Gaussians
    of its own: equal to per-view calls"""
    views = [_view(S.colour_case("2048x1536"), F=2, alpha=True, vis=True, depth=True, seed=1),
             _view(S.colour_case("2064x1536"), F=2, alpha=True, vis=True, depth=True, seed=2),
             _view(S.colour_case("17x1"), F=2, alpha=True, vis=False, depth=True, seed=3)]
    bat = E._gpu(views, cam=True)
    one = E._gpu(views, cam=True, batched=False)
    E._equal_batched_per_view(bat, one, True, what="mixed sizes")
    for v, r in zip(views, bat):        # (and each view's colour, depth and alpha = 1 - final T are the oracle's)
        o64 = oracle_forward(v["case"], dtype=np.float64)
        assert S.image_err(r["imgs"][0], o64.color) < TOL and S.image_err(r["imgs"][1], o64.out_depth) < TOL
        assert r["imgs"][3].max() > 0.5 and S.image_err(r["imgs"][3], 1.0 - o64.final_T[None]) < TOL


def _rasterize(views_settings_kws):
    import diff_gaussian_rasterization as dgr
    settings, kws = views_settings_kws
    return dgr.rasterize_views(settings, kws)


def _plain_views(name, V):
    from csplat import synthetic as syn
    W, H = SIZES[name]
    base = E._prefix(S.colour_case(name), 8400)     # (a Gaussian count no other test has: the library's launch history holds no such shape)
    inp = util.gpu_inputs(base, requires_grad=False)
    cases = [dict(base, cam=syn.make_camera(-20.0 + 40.0 * i / max(V - 1, 1), W, H)) for i in range(V)]
    kw = {k: inp[k] for k in E.GKEYS}
    return [util.gpu_settings(c) for c in cases], [dict(kw, means2D=torch.zeros(base["P"], 3, device="cuda")) for _ in range(V)]


def test_deferred_and_faith_entries_over_the_limit():
    """include/csplat.h, "Images of more than 12288 tiles": csplat_forward_views_deferred completes such a call itself (*pending = 0, view
    by view: nothing to settle, every call waits for its counts however often the shape repeats) and csplat_forward_views_faith refuses it
    (the views do not qualify for the one-launch-per-stage path).  At exactly 12288 tiles the first call of the shape waits and the
    second is launched speculatively, on the first one's counts: a hit."""
    import diff_gaussian_rasterization as dgr
    for name, over in (("2064x1536", True), ("2048x1536", False)):
        sk = _plain_views(name, 2)
        before = dict(dgr.SPEC_STATS)
        a = _rasterize(sk)
        b = _rasterize(sk)
        torch.cuda.synchronize()
        d = {k: dgr.SPEC_STATS[k] - before[k] for k in ("wait", "hit", "miss")}
        assert d == (dict(wait=2, hit=0, miss=0) if over else dict(wait=1, hit=1, miss=0)), (name, d)
        for x, y in zip(a, b):
            assert all(torch.equal(p, q) for p, q in zip(x, y))
    sk = _plain_views("2064x1536", 2)
    faith = dict(caps=(1 << 20, 4096, 12384), valid=torch.zeros(1, dtype=torch.int32, device="cuda"))
    with pytest.raises(RuntimeError, match="do not qualify for the one-launch-per-stage path"):
        with dgr.forward_mode(faith=faith):
            _rasterize(sk)
    assert dgr.forward_mode_is_default()
    c = _rasterize(sk)                  # (the refusal released its tickets: the library goes on)
    torch.cuda.synchronize()
    assert all(torch.isfinite(x[0]).all() and bool(x[0].std() > 0) for x in c)


@pytest.mark.parametrize("G", [1, 3])
def test_backward_in_parts_over_the_limit_equals_the_whole_backward(G):
    """tests/test_raster_gpu.py::test_backward_in_parts_equals_the_whole_backward at 2064 x 1536: the forward went view by view, the backward
    is still one launch per stage and can be cut -- every gradient BIT-equal to the one-call backward"""
    import diff_gaussian_rasterization as dgr
    V, P, (W, H) = 3, 2901, SIZES["2064x1536"]
    names = ("means3D", "opacities", "shs", "scales", "rotations")
    _flags(256)
    try:
        def run(parts):
            inp = util.gpu_inputs(util.make_case(P=P, W=W, H=H, seed=4, theta=-30.0, scale_mul=2.0))
            cases = [util.make_case(P=P, W=W, H=H, seed=4, theta=-30.0 + 30.0 * i, scale_mul=2.0) for i in range(V)]
            m2d = [torch.zeros(P, 3, device="cuda", requires_grad=True) for _ in range(V)]
            kws = [dict(means3D=inp["means3D"], means2D=m2d[i], opacities=inp["opacities"], shs=inp["shs"], scales=inp["scales"],
                        rotations=inp["rotations"]) for i in range(V)]
            colors, _outs = dgr.rasterize_views([util.gpu_settings(c) for c in cases], kws, stacked=True)
            gen = torch.Generator(device="cuda").manual_seed(3)
            loss = ((colors - torch.rand(V, 3, H, W, device="cuda", generator=gen)) ** 2).mean()
            rows = []
            if parts:
                with dgr.deferred_k8() as h:
                    loss.backward()
                assert len(h.entries) == 1
                for t in [inp[k].grad for k in names] + [m.grad for m in m2d]:
                    t.fill_(float("nan"))
                for g_ in range(G):
                    rows.append(h.rows(g_, G))
                    h.launch(g_, G)
                    if g_ + 1 < G:
                        assert torch.isnan(inp["scales"].grad[rows[-1][1]:]).all() and torch.isfinite(inp["scales"].grad[:rows[-1][1]]).all()
            else:
                loss.backward()
            torch.cuda.synchronize()
            return [inp[k].grad.clone() for k in names] + [m.grad.clone() for m in m2d], rows
        whole, _ = run(False)
        cut, rows = run(True)
    finally:
        _flags(0)
    assert rows[0][0] == 0 and rows[-1][1] == P and all(a[1] == b[0] for a, b in zip(rows, rows[1:])) and all(lo % 32 == 0 for lo, _hi in rows)
    for a, b in zip(whole, cut):
        assert torch.equal(a, b) and torch.isfinite(a).all() and bool(a.abs().max() > 0)


# ------------------------------------------------------------------------------------------------ 4. extended outputs at the edges
@pytest.mark.parametrize("aa", [False, True], ids=["plain", "aa"])
@pytest.mark.parametrize("name", list(S.DEGENERATE))
def test_extended_outputs_match_fp64(name, aa):
    """depth gradient, camera and background gradients, F = 2 feature channels and alpha, visibility, with and without antialiasing, on the
    degenerate grids, against tests/antialias_ref.py / visibility_ref.py in fp64 over the oracle's lists"""
    case = S.sparse_case(name)
    o, _st = E._gpu_lists(case)
    v = E._view(case, F=2, alpha=True, vis=True, depth=True, seed=5)
    e32, i32 = E._oracle_colour_err(case, v["wts"])
    bar, img_bar = max(TOL, K * e32), max(TOL, K * i32)
    got = E._gpu([v], aa=aa, cam=True)[0]
    np.testing.assert_array_equal(got["radii"], o.radii)
    threads = torch.get_num_threads()
    torch.set_num_threads(1)        # (thousands of tile-sized operations: a thread team per operation costs ten times the operation)
    try:
        ref = E._ref(v, aa, o)
    finally:
        torch.set_num_threads(threads)
    E._compare_fp64(got, ref, v, bar, img_bar, what=f"{name} aa={aa}")
    E._check_consistent(got)
    E._compare_vis(got, ref, what=f"{name} aa={aa}")
    errs = {n_: S.image_err(a, b, outlier_frac=1e-3) for n_, a, b in zip(("color", "depth", "feat", "alpha"), got["imgs"], ref["imgs"])}
    gerr = max(rel_err(got["grads"][k], b) for k, b in ref["grads"].items())
    cerr = max(rel_err(got["cam"][k], b) for k, b in ref["cam"].items() if b is not None)
    print(f"{name} aa={aa}: e32 / bar / kernel  images {i32:.2e} / {img_bar:.2e} / {max(errs.values()):.2e}  "
          f"gradients {e32:.2e} / {bar:.2e} / {gerr:.2e}  camera {cerr:.2e}")
    assert all(e < img_bar for e in errs.values()), errs      # (no exempt pixel on the images of a few pixels)
    m = case["marks"]
    assert np.all(got["vis"][2][m["corners"] + m["edges"]] > 0)       # the markers at the grid's ends are seen


@pytest.mark.parametrize("aa", [False, True], ids=["plain", "aa"])
@pytest.mark.parametrize("name", list(S.EXTENDED_OVER))
def test_extended_outputs_over_the_limit(name, aa):
    """The same outputs at 2064 x 1536 and 3841 x 2161, WITHOUT the fp64 torch restatement: it walks the tiles in Python, 2 ms per non-empty
    tile (1.5 to 11 s per case here, measured), against 0.6 s of the slowest test of tests/test_raster_extended_edges_gpu.py.  These sizes
    are therefore checked against the C fp64 oracle on the colour path only (colour, depth, alpha = 1 - final T; antialiasing off, which
    is what the oracle renders), plus what needs no reference: features = (view-space z, 1) must give feat = (depth image, alpha image),
    the visibility identities of _check_consistent, every gradient finite and present.  Their gradients are held to per-view calls by
    test_batched_views_over_the_limit_equal_per_view_calls and, on the colour path, to the fp64 oracle by test_backward_grads."""
    case = S.sparse_case(name)
    o, _st = E._gpu_lists(case)
    Vm = np.asarray(case["cam"]["world_view_transform"], np.float64).reshape(4, 4)
    z = (np.c_[case["g"]["means3D"].astype(np.float64), np.ones(case["P"])] @ Vm)[:, 2]
    v = _view(case, F=2, alpha=True, vis=True, depth=True, seed=5, feats=np.c_[z, np.ones_like(z)].astype(np.float32))
    got = E._gpu([v], aa=aa, cam=True)[0]
    np.testing.assert_array_equal(got["radii"], o.radii)
    color, depth, feat, alpha = got["imgs"]
    assert all(np.isfinite(x).all() for x in got["imgs"]) and alpha.max() > 0.5
    assert np.abs(feat[0] - depth[0]).max() <= 1e-5 * max(1.0, np.abs(depth).max())       # (the bar of test_wild_scenes_with_needles_identities)
    assert np.abs(feat[1] - alpha[0]).max() <= 1e-5
    if not aa:
        o64 = oracle_forward(case, dtype=np.float64)
        errs = (S.image_err(color, o64.color), S.image_err(depth, o64.out_depth), S.image_err(alpha, 1.0 - o64.final_T[None]))
        print(f"{name}: colour, depth, alpha against the fp64 oracle {errs[0]:.2e} {errs[1]:.2e} {errs[2]:.2e} / {TOL:.0e}")
        assert max(errs) < TOL, errs
    E._check_consistent(got)
    m = case["marks"]
    assert np.all(got["vis"][2][m["corners"] + m["edges"] + [m["full"]]] > 0)      # the markers and the full-grid Gaussian are seen
    assert got["vis"][2][m["full"]] > 0.3 * case["W"] * case["H"]
    for k, g_ in list(got["grads"].items()) + list(got["cam"].items()):
        assert g_ is not None and np.isfinite(g_).all() and (np.any(g_) or k == "campos"), k


# ------------------------------------------------------------------------------------------------ 5. gaussian_renderer over the limit
def test_render_and_render_views_over_the_limit():
    """gaussian_renderer.render at 2064 x 1536 (the wrappers' chunk handling without a table chunk) against the fp64 oracle on the same
    rasterizer-level inputs, and render_views of two cameras against render per camera (test_render_gpu's bars)"""
    import test_render_gpu as R
    from gaussian_renderer import render, render_views
    W, H = SIZES["2064x1536"]
    sc = R._scene(W=W, H=H)
    pc, sim = R._build(sc)
    with torch.no_grad():
        torch.manual_seed(0)
        sim.output.weight.normal_(0, 1e-3)
    cams = [R._camera(sc["cameras"][0], time=t) for t in (0.25, 0.75)]
    pipe = SimpleNamespace(compute_cov3D_python=False, convert_SHs_python=False, debug=False)
    bg = torch.ones(3, device="cuda")
    plist = [pc.face_bary, pc._features_dc, pc._features_rest, pc._opacity, pc._scaling, pc._rotation, sim.output.weight]

    def run(batched):
        for p in plist:
            p.grad = None
        res = render_views(cams, pc, sim, pipe, bg) if batched else [render(c, pc, sim, pipe, bg) for c in cams]
        sum((r.render - 0.4).abs().mean() for r in res).backward()
        return res, [p.grad.clone() for p in plist], [r.viewspace_points.grad.clone() for r in res]

    r1, g1, v1 = run(False)
    r2, g2, v2 = run(True)
    for a, b in zip(r1, r2):
        assert torch.equal(a.render, b.render) and torch.equal(a.radii, b.radii) and torch.equal(a.depth, b.depth)
    for a, b in zip(g1 + v1, g2 + v2):
        assert torch.isfinite(b).all() and rel_err(b.cpu().numpy(), a.cpu().numpy()) < 1e-5
    n = lambda t: t.detach().cpu().numpy()  # noqa: E731
    c0 = sc["cameras"][0]
    res = r1[0]
    o = util.ro.forward(n(res.means3D_deform), n(pc.get_opacity), c0["world_view_transform"], c0["full_proj_transform"], c0["camera_center"],
                        c0["tanfovx"], c0["tanfovy"], W, H, np.ones(3), shs=n(pc.get_features), sh_degree=3, scales=n(pc.get_scaling),
                        rotations=n(res.rotations), dtype=np.float64)
    assert S.tiles_of(W, H) > S.BUCKET_TILES and int((o.radii > 0).sum()) > 1000
    assert S.image_err(n(res.render), o.color) < TOL and S.image_err(n(res.depth), o.out_depth) < TOL
