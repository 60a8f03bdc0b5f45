"""The launch shapes of the forward's binning kernels: the tile sort's instantiations (2 / 4 / 6 / 8 keys per lane, chosen by the host from
the launch's longest list, walking the longest-first tile order, the views of a batched launch interleaved), its fallbacks, the global
path behind BUCKET_CAP, the one-round tile scan (up to 12 consecutive tiles per thread) and the batched K1 at its 64-Gaussian chunk edges.

Scenes are built so that the list lengths are KNOWN: tiny Gaussians placed at chosen pixels and view-space depths, one tile each, and
Gaussians behind the camera, which pass through K1 and reach no list.  Expected values come from the C oracle (fp32 build: bit-exact lists)
and from numpy (the stable order of (tile, depth bits, id)); batched calls are also held to the per-view call, bit for bit.  Nothing is
compared against the kernel under test.  Bars: those of tests/test_raster_gpu.py::test_indices_bit_exact, none new."""
import ctypes as C

import numpy as np
import pytest

import util
from util import oracle_forward, rel_err, syn

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

BUCKET_CAP = 8192       # longest list the in-LDS sort takes (csrc/csplat_raster_binning.h)
INFO_BUSY = 64          # word offset of the busy list inside the info block; the longest-first order follows at INFO_BUSY + tiles + 4
RADIX_ONLY = 2048       # csplat_debug_flags bit 11
FORCED_FALLBACK = 4096  # bit 12: bucket limit 1
GEOM = ("depth", "xy", "conic_opacity", "rgb", "cov3D", "clamped", "tiles_touched")


def _flags(f):
    from csplat import native
    native.lib.csplat_debug_flags(f)


# ------------------------------------------------------------------------------------------------ scenes with known lists
def _depths(pattern, n, rng):
    """view-space depths of n Gaussians and whether their centres may be jittered (bit-equal depths need ONE world point)"""
    if pattern == "distinct":
        return 4.0 + rng.uniform(-0.5, 0.5, n), True
    if pattern == "equal":                  # no depth byte varies: the full-key radix passes
        return np.full(n, 4.0), False
    if pattern == "two":                    # runs of n / 2 equal depths: longer than TIE_RUN = 8 from n = 18 on
        return np.where(np.arange(n) % 2 == 0, 4.0, 4.25), False
    if pattern == "outlier":                # the rest of the tile lands in a few of the 4096 buckets: more than TSORT_LONG = 64 in one
        z = 4.0 + rng.uniform(-1e-3, 1e-3, n)
        z[n // 2] = 60.0
        return z, True
    raise ValueError(pattern)


def _scene(W, H, groups, behind=0, seed=0, theta=0.0):
    """groups: [(px, py, depths, jitter)] -- Gaussians of ~2 pixels radius centred within a pixel of (px, py); `behind` more behind the camera"""
    cam = syn.make_camera(theta, W, H)
    Vm = np.asarray(cam["world_view_transform"], np.float64).reshape(4, 4)
    rng = np.random.default_rng(seed)
    pv = []
    for px, py, z, jitter in groups:
        z = np.asarray(z, np.float64)
        j = rng.uniform(-1.0, 1.0, (2, len(z))) if jitter else np.zeros((2, len(z)))
        x = ((2.0 * (px + j[0]) + 1.0) / W - 1.0) * cam["tanfovx"] * z
        y = ((2.0 * (py + j[1]) + 1.0) / H - 1.0) * cam["tanfovy"] * z
        pv.append(np.stack([x, y, z], 1))
    pv.append(np.tile([0.0, 0.0, -3.0], (behind, 1)))
    pv = np.concatenate(pv)
    P = len(pv)
    order = rng.permutation(P)              # ids in no relation to the place in a list
    pv = pv[order]
    means = (pv - Vm[3, :3]) @ np.linalg.inv(Vm[:3, :3])
    quats = np.tile([1.0, 0.0, 0.0, 0.0], (P, 1))
    shs = np.concatenate([rng.normal(0, 1.0, (P, 1, 3)), rng.normal(0, 0.1, (P, 15, 3))], 1)
    sigma = 0.05 * 4.0 * 2.0 * cam["tanfovx"] / W          # 0.05 pixels at depth 4: the footprint is the 0.3-pixel dilation, radius 2
    g = dict(means3D=means.astype(np.float32), scales=np.full((P, 3), sigma, np.float32), rotations=quats.astype(np.float32),
             opacities=rng.uniform(0.05, 0.6, (P, 1)).astype(np.float32), shs=shs.astype(np.float32))
    return dict(g=g, cam=cam, W=W, H=H, P=P, bg=np.array([0.2, 0.4, 0.6], np.float32), sh_degree=3)


def _one_tile(n, pattern, seed=0, behind=0):
    rng = np.random.default_rng(1000 + seed)
    z, jitter = _depths(pattern, n, rng)
    return _scene(16, 16, [(7.5, 7.5, z, jitter)], behind=behind, seed=seed)


def _stable_order(o, tiles_x):
    """numpy restatement of the lists: every visible Gaussian touches one tile here; (tile, depth bits, id) ascending"""
    vis = np.flatnonzero(o.radii > 0)
    assert np.all(o.tiles_touched[vis] == 1)
    tile = (o.xy[vis, 1] // 16).astype(np.uint64) * np.uint64(tiles_x) + (o.xy[vis, 0] // 16).astype(np.uint64)
    bits = o.depth[vis].view(np.uint32).astype(np.uint64)
    k = np.lexsort((vis, bits, tile))
    return (tile[k] << np.uint64(32)) | bits[k], vis[k].astype(np.uint32)


def _check_lists(st, o, what, tiles_x=1):
    assert st["R"] == o.R, what
    for k in ("keys", "ids"):
        assert np.array_equal(st[k][:o.R], getattr(o, k)), (what, k)
    assert np.array_equal(st["ranges"], o.ranges), what
    keys, ids = _stable_order(o, tiles_x)
    assert np.array_equal(st["keys"][:o.R], keys) and np.array_equal(st["ids"][:o.R], ids), what


def _view_of(out):
    """the state object behind a forward's colour image: .chunks (GEOM, BINNING, IMAGE), .num_rendered, and the layout size"""
    fn = out[0].grad_fn
    v = fn.views[0] if hasattr(fn, "views") else fn.view_state
    return v, int(getattr(v, "layout_rendered", v.num_rendered))


def _forward(case, flags=0):
    _flags(flags)
    try:
        color, radii, depth, st = util.gpu_forward_raw(case)
    finally:
        _flags(0)
    st["radii"] = radii.cpu().numpy()
    return st


# ------------------------------------------------------------------------------------------------ the tile sort
SORT_N = (1, 2, 63, 64, 65, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096, 4097, 8191, 8192, 8193)


@pytest.mark.parametrize("flags", [0, RADIX_ONLY], ids=["bucket_sort", "radix_only"])
@pytest.mark.parametrize("pattern", ["distinct", "equal", "two", "outlier"])
def test_one_tile_list_of_n(pattern, flags):
    """a 16 x 16 image is one tile: n small Gaussians inside it are one list of exactly n entries -- at every edge of the keys-per-lane
    instantiations (1024 keys a step, 2 / 4 / 6 / 8 per lane) and one past BUCKET_CAP, where the call takes the global sort"""
    for n in SORT_N:
        case = _one_tile(n, pattern, seed=n)
        o = oracle_forward(case)
        assert o.R == n and np.array_equal(o.ranges, [[0, n]]), (n, o.R)         # (the scene is what it is meant to be)
        bits = np.unique(o.depth.view(np.uint32))
        assert len(bits) == {"equal": 1, "two": min(n, 2)}.get(pattern, len(bits)), (pattern, n, len(bits))
        st = _forward(case, flags)
        _check_lists(st, o, f"{pattern} n={n} flags={flags}")
        assert np.array_equal(st["radii"], o.radii) and np.array_equal(st["depth"].view(np.uint32), o.depth.view(np.uint32))


def _three_tiles(counts, patterns, seed, behind=0, theta=0.0):
    rng = np.random.default_rng(2000 + seed)
    groups = []
    for i, (n, pat) in enumerate(zip(counts, patterns)):
        z, jitter = _depths(pat, n, rng)
        groups.append((16 * i + 7.5, 7.5, z, jitter))
    return _scene(48, 16, groups, behind=behind, seed=seed, theta=theta)


@pytest.mark.parametrize("flags", [0, RADIX_ONLY, FORCED_FALLBACK], ids=["bucket_sort", "radix_only", "bucket_sort_forced_fallback"])
def test_every_size_class_in_one_launch(flags):
    """48 x 16: lists of 5000, 1 and 300 entries in one launch (the instantiation is chosen for the longest, the others run in it),
    sorted longest first"""
    case = _three_tiles((5000, 1, 300), ("distinct", "distinct", "two"), seed=3)
    o = oracle_forward(case)
    assert sorted((o.ranges[:, 1] - o.ranges[:, 0]).tolist()) == [1, 300, 5000]
    _check_lists(_forward(case, flags), o, f"three tiles flags={flags}", tiles_x=3)


def _many_tiles(n_long, pattern, seed, behind=0):
    """a strip of 704 tiles, every one non-empty (1 to 20 entries), the first with a list of n_long: more non-empty tiles than 2.5 per CU
    of a 256-CU device, where the host takes the two-workgroups-per-CU instantiations of the sort"""
    rng = np.random.default_rng(3000 + seed)
    z, jitter = _depths(pattern, n_long, rng)
    groups = [(7.5, 7.5, z, jitter)]
    for t in range(1, 704):
        groups.append((16.0 * t + 7.5, 7.5, 4.0 + rng.uniform(-0.5, 0.5, int(rng.integers(1, 21))), True))
    return _scene(16 * 704, 16, groups, behind=behind, seed=seed)


@pytest.mark.parametrize("flags", [0, RADIX_ONLY], ids=["bucket_sort", "radix_only"])
@pytest.mark.parametrize("n_long,pattern", [(300, "distinct"), (2048, "two"), (2049, "outlier"), (4096, "equal"), (5000, "distinct"),
                                            (6144, "outlier"), (6145, "distinct")])
def test_launches_of_many_tiles(n_long, pattern, flags):
    """704 non-empty tiles in one view and 2 x 704 in a batched call, the longest list in every keys-per-lane class (6145: past the last
    class that has a two-workgroups-per-CU form), the long list in each depth pattern: lists bit-equal to the oracle's, batched to per-view"""
    case = _many_tiles(n_long, pattern, seed=n_long)
    o = oracle_forward(case)
    length = o.ranges[:, 1] - o.ranges[:, 0]
    assert length[0] == n_long and length.min() >= 1 and length[1:].max() <= 20
    one = _forward(case, flags)
    _check_lists(one, o, f"704 tiles n_long={n_long} flags={flags}", tiles_x=704)
    other = _many_tiles(n_long // 2 + 1, "distinct", seed=n_long + 1)
    pad = abs(case["P"] - other["P"])
    if case["P"] < other["P"]:
        case = _many_tiles(n_long, pattern, seed=n_long, behind=pad)
        o = oracle_forward(case)
    else:
        other = _many_tiles(n_long // 2 + 1, "distinct", seed=n_long + 1, behind=pad)
    cases = _share([case, other])
    _flags(flags)
    try:
        bat = _batched(cases)
    finally:
        _flags(0)
    _check_lists(bat[0], o, f"2 x 704 tiles n_long={n_long} flags={flags}", tiles_x=704)
    _check_lists(bat[1], oracle_forward(cases[1]), f"2 x 704 tiles, second view, flags={flags}", tiles_x=704)


def _batched(cases, twice=False, aa=False):
    """rasterize_views over `cases` (same P, W, H; shared opacities / SH / scales; own means): per view the decoded chunks"""
    import diff_gaussian_rasterization as dgr
    c0 = cases[0]
    inp = util.gpu_inputs(c0)
    settings = [util.gpu_settings(c) for c in cases]
    extra = dict(antialiasing=True) if aa else {}
    means = [torch.tensor(c["g"]["means3D"], device="cuda", requires_grad=True) for c in cases]
    out = None
    for _ in range(2 if twice else 1):     # (the second call of a shape is launched speculatively, on the first one's counts)
        kws = [dict(means3D=means[i], means2D=torch.zeros(c0["P"], 3, device="cuda", requires_grad=True), opacities=inp["opacities"],
                    shs=inp["shs"], scales=inp["scales"], rotations=inp["rotations"], **extra) for i in range(len(cases))]
        outs = dgr.rasterize_views(settings, kws)
        torch.cuda.synchronize()
        views = outs[0][0].grad_fn.views
        out = []
        for i, v in enumerate(views):
            st = util.gpu_chunks(v.chunks, c0["P"], c0["W"], c0["H"], int(v.layout_rendered))
            st.update(R=int(v.num_rendered), radii=outs[i][1].cpu().numpy(), color=outs[i][0].detach().cpu().numpy(), view=v)
            out.append(st)
    return out


def _share(cases):
    """the batched launch needs ONE set of opacities / SH / scales / rotations: every view takes view 0's (means stay per view)"""
    for c in cases[1:]:
        c["g"] = dict(cases[0]["g"], means3D=c["g"]["means3D"])
    return cases


MIXES = [((5000, 1, 300), ("distinct", "distinct", "two")), ((300, 4097, 1), ("outlier", "equal", "distinct")),
         ((1, 65, 2049), ("distinct", "two", "outlier")), ((1025, 1024, 1023), ("equal", "distinct", "distinct"))]


@pytest.mark.parametrize("V", [1, 3, 4])
def test_batched_views_sort_equals_per_view_calls(V):
    """the same scenes through rasterize_views, a different mix of list lengths and depth patterns per view (every view pads its
    Gaussians to one P behind the camera): lists bit-equal to the oracle's and to the per-view call's, in the first call of the shape
    (exact capacities) and in the second (speculative capacities)"""
    P = 5301 + 17
    cases = _share([_three_tiles(n, pat, seed=10 * V + i, behind=P - sum(n)) for i, (n, pat) in enumerate(MIXES[:V])])
    bat = _batched(cases, twice=True)
    for i, (case, st) in enumerate(zip(cases, bat)):
        o = oracle_forward(case)
        assert sorted((o.ranges[:, 1] - o.ranges[:, 0]).tolist()) == sorted(MIXES[i][0])
        _check_lists(st, o, f"V={V} view {i}", tiles_x=3)
        one = _forward(case)
        for k in ("keys", "ids"):
            assert np.array_equal(st[k][:o.R], one[k]), (V, i, k)
        assert np.array_equal(st["ranges"], one["ranges"]) and np.array_equal(st["radii"], one["radii"])


# ------------------------------------------------------------------------------------------------ K1 for all views
def _geom_pack(view, P):
    """the two per-Gaussian fields csplat_geom_layout does not name, by their place in the chunk (csrc: geom_offsets -- cut2 follows
    `offsets`, pack is the chunk's last field; every field is padded to 256 bytes)"""
    from csplat import native as n
    a256 = lambda b: (b + 255) // 256 * 256  # noqa: E731
    o8 = (C.c_size_t * 8)(); n.lib.csplat_geom_layout(P, o8)
    n.lib.csplat_geom_bytes.restype = C.c_size_t
    geom = view.chunks[0].cpu().numpy().tobytes()
    total = int(n.lib.csplat_geom_bytes(P))
    cut2 = np.frombuffer(geom[o8[7] + a256(4 * P):o8[7] + a256(4 * P) + 4 * P], np.uint32)
    pack = np.frombuffer(geom[total - a256(48 * P):total - a256(48 * P) + 48 * P], np.uint32)
    return cut2, pack


@pytest.mark.parametrize("aa", [False, True], ids=["plain", "aa"])
@pytest.mark.parametrize("V", [1, 2, 3, 4, 5, 8])
def test_k1_chunk_edges_batched_equals_per_view_and_oracle(V, aa):
    """k_preprocess_views takes 64 Gaussians per workgroup, wave w the views w, w + 4, ...: P at 1 and around one and two chunks, every
    per-Gaussian field bitwise equal between the batched and the per-view call, and against the oracle under the bars of
    test_raster_gpu.py::test_indices_bit_exact (antialiasing: the oracle renders without it -- the fields it does not touch)"""
    import diff_gaussian_rasterization as dgr
    for P in (1, 63, 64, 65, 127, 128, 129):
        cases = [util.make_case(P=P, W=96, H=64, seed=40 + P, grid=6, scale_mul=3.0, theta=-60.0 + 17.0 * i) for i in range(V)]
        bat = _batched(cases, aa=aa)
        for i, (case, st) in enumerate(zip(cases, bat)):
            inp = util.gpu_inputs(case)
            out = dgr.GaussianRasterizer(util.gpu_settings(case))(means3D=inp["means3D"], means2D=inp["means2D"], opacities=inp["opacities"],
                                                                  shs=inp["shs"], scales=inp["scales"], rotations=inp["rotations"],
                                                                  antialiasing=aa)
            torch.cuda.synchronize()
            v1, layout = _view_of(out)
            one = util.gpu_chunks(v1.chunks, P, 96, 64, layout)
            what = f"P={P} V={V} view {i} aa={aa}"
            assert torch.equal(out[1].cpu(), torch.from_numpy(st["radii"])), what
            for k in GEOM:
                assert np.array_equal(st[k].view(np.uint32), one[k].view(np.uint32)), (what, k)
            for a, b in zip(_geom_pack(st["view"], P), _geom_pack(v1, P)):
                assert np.array_equal(a, b), what
            o = oracle_forward(case)
            vis = o.radii > 0
            assert np.array_equal(st["radii"], o.radii) and np.array_equal(st["tiles_touched"], o.tiles_touched), what
            for k in ("depth", "xy", "cov3D") + (() if aa else ("conic_opacity",)):
                assert np.array_equal(st[k].view(np.uint32), getattr(o, k).view(np.uint32)), (what, k)
            clamped = np.stack([(st["clamped"] >> ch) & 1 for ch in range(3)], 1).astype(np.uint8)
            assert (clamped[vis] != o.clamped[vis]).sum() <= 2 and rel_err(st["rgb"], o.rgb) < 1e-5, what


# ------------------------------------------------------------------------------------------------ the scans
def _info(view, W, H):
    """(R, longest list, non-empty tiles), the busy list and the longest-first order the tile scan left in the IMAGE chunk"""
    from csplat import native as n
    n.lib.csplat_image_info_offset.restype = C.c_size_t
    tiles = ((W + 15) // 16) * ((H + 15) // 16)
    off = int(n.lib.csplat_image_info_offset(W, H))
    words = np.frombuffer(view.chunks[2].cpu().numpy().tobytes()[off:off + 4 * (INFO_BUSY + 2 * tiles + 4)], np.uint32)
    nbusy = int(words[INFO_BUSY])
    return words[:3], words[INFO_BUSY + 1:INFO_BUSY + 1 + nbusy], words[INFO_BUSY + tiles + 4:INFO_BUSY + 2 * tiles + 4]


def _check_scan(view, o, W, H, what):
    tiles = len(o.ranges)
    length = (o.ranges[:, 1] - o.ranges[:, 0]).astype(np.int64)
    head, busy, order = _info(view, W, H)
    assert head.tolist() == [o.R, int(length.max()), int((length > 0).sum())], (what, head)
    assert np.array_equal(busy, np.flatnonzero(length > 0)), what
    assert np.array_equal(np.sort(order), np.arange(tiles)), what                 # a permutation of the tiles
    nb = len(busy)
    assert np.all(length[order[:nb]] > 0) and np.all(length[order[nb:]] == 0), what
    bins = np.minimum(length[order[:nb]] // 16, 511)
    assert np.all(np.diff(bins) <= 0), what                                        # non-increasing floor(length / 16)


def _strip(tiles_x, P, seed):
    """a 16-pixel-high strip of tiles_x tiles: P small Gaussians over it, a quarter of the tiles left empty, list lengths from 1 to
    a few hundred (length / 16 takes many values)"""
    rng = np.random.default_rng(seed)
    W = 16 * tiles_x
    busy = np.flatnonzero(rng.random(tiles_x) < 0.75) if tiles_x > 1 else np.array([0])
    wts = rng.random(len(busy)) ** 3 + 1e-3
    tile = busy[rng.choice(len(busy), size=P, p=wts / wts.sum())]
    groups = [(16.0 * t + 7.5, 7.5, 4.0 + rng.uniform(-0.5, 0.5, int((tile == t).sum())), True) for t in busy if (tile == t).any()]
    return _scene(W, 16, groups, seed=seed)


@pytest.mark.parametrize("tiles_x", [1, 255, 256, 257, 1023, 1024, 1025])
@pytest.mark.parametrize("P", [1024 * k + d for k in (1, 8, 16) for d in (-1, 0, 1)])
def test_scans_counts_ranges_and_order(P, tiles_x):
    """P around 1, 8 and 16 counting workgroups (the column scan's batches of 8 rows) x strips of 1 to 1025 tiles (the tile scan's 1024
    threads take one or two tiles each): R, the longest list, the non-empty tiles, ranges and sorted lists bit-equal to the oracle's; the
    longest-first order a permutation of the tiles with the non-empty ones in front, in non-increasing floor(length / 16)"""
    import diff_gaussian_rasterization as dgr
    case = _strip(tiles_x, P, seed=P + tiles_x)
    o = oracle_forward(case)
    assert o.R == P
    inp = util.gpu_inputs(case)
    out = dgr.GaussianRasterizer(util.gpu_settings(case))(means3D=inp["means3D"], means2D=inp["means2D"], opacities=inp["opacities"],
                                                          shs=inp["shs"], scales=inp["scales"], rotations=inp["rotations"])
    torch.cuda.synchronize()
    v, layout = _view_of(out)
    st = util.gpu_chunks(v.chunks, P, case["W"], 16, layout)
    st["R"] = int(v.num_rendered)
    _check_lists(st, o, f"P={P} tiles={tiles_x}", tiles_x=tiles_x)
    _check_scan(v, o, case["W"], 16, f"P={P} tiles={tiles_x}")


@pytest.mark.parametrize("fit", [True, False], ids=["capacities_fit", "capacities_do_not_fit"])
def test_scan_order_and_validity_under_a_launch_on_faith(fit):
    """csplat_forward_views_faith: both phases launched with capacities given beforehand.  Capacities that hold the counts: valid = 1,
    lists and order as above for every view.  A longest-list capacity below the longest list: valid = 0, and the counts the scan left
    (what the caller sizes the repeat from) are still the oracle's."""
    import diff_gaussian_rasterization as dgr
    mixes = MIXES[:3]
    P = 5301 + 17
    cases = _share([_three_tiles(n, pat, seed=70 + i, behind=P - sum(n)) for i, (n, pat) in enumerate(mixes)])
    inp = util.gpu_inputs(cases[0], requires_grad=False)
    means = [torch.tensor(c["g"]["means3D"], device="cuda") for c in cases]
    kws = [dict(means3D=means[i], means2D=torch.zeros(P, 3, device="cuda"), opacities=inp["opacities"], shs=inp["shs"], scales=inp["scales"],
                rotations=inp["rotations"]) for i in range(3)]
    faith = dict(caps=(8192, 5120 if fit else 4000, 3), valid=torch.full((1,), 7, dtype=torch.int32, device="cuda"))
    with dgr.forward_mode(faith=faith):
        outs = dgr.rasterize_views([util.gpu_settings(c) for c in cases], kws)
    torch.cuda.synchronize()
    assert dgr.forward_mode_is_default()
    assert int(faith["valid"].cpu()[0]) == (1 if fit else 0)
    os_ = [oracle_forward(c) for c in cases]
    for o, words in zip(os_, faith["info"]):
        length = o.ranges[:, 1] - o.ranges[:, 0]
        assert words.cpu().tolist() == [o.R, int(length.max()), int((length > 0).sum())]
    if fit:
        for i, (o, out) in enumerate(zip(os_, outs)):
            assert np.array_equal(out[1].cpu().numpy(), o.radii)
            assert util.image_err(out[0].cpu().numpy(), o.color, outlier_frac=0.0) < 1e-4
