"""The size table and scenes of tests/image_sizes_ref.py are what they claim (CPU): every size crosses the host-code switch it is in the
table for (the constants restated from csplat_raster*.{hip,h} / csplat_sort.hip and compared with the sources, as tests/test_train_kernels_cpu.py
does for the train-step launches), the scenes put visible Gaussians where the tile grid ends, and the reference pair of the GPU test -- the
C oracle in fp32 against fp64 -- itself stays inside the bars and the threshold-tie allowances the GPU test applies, so that an allowance
cannot hide a GPU error that the references do not show themselves."""
import os
import re

import numpy as np
import pytest

import util
import image_sizes_ref as S
from image_sizes_ref import SIZES, grid_of, tiles_of
from util import oracle_forward, rel_err

TOL = 1e-4


# ------------------------------------------------------------------------------------------------ the table
def test_constants_are_the_sources():
    c = S.source_constants()
    assert c["BUCKET_TILES"] == S.BUCKET_TILES == 12288 and c["BUCKET_TILES"] * 4 == 48 * 1024          # the 48 KB LDS histogram
    assert c["can_bucket"].replace(" ", "").startswith("tiles<=BUCKET_TILES&&")
    assert c["small_cap"] == S.TILE_SORT_SMALL_CAP < c["BUCKET_CAP"] == 8192
    assert c["end_bit"].replace(" ", "") == "32+higher_msb((uint32_t)tiles)"
    assert "while ((1u << b) < n && b < 31) b++;" in c["higher_msb"] and "return b == 0 ? 1 : b;" in c["higher_msb"]
    assert c["RADIX"] == 1 << S.RADIX_DIGIT_BITS
    assert c["passes"].replace(" ", "") == "(end_bit+7)/8" and c["shifts"] == ["p * 8", "p * 8"]
    assert c["digit_masks"] and all(int(m, 16) == c["RADIX"] - 1 for m in c["digit_masks"])


def test_every_raster_part_is_included_once_by_the_rasterizer_only():
    csrc = os.path.join(util.ROOT, "cloth-splatting_amd", "csrc")
    parts = sorted(f for f in os.listdir(csrc) if re.fullmatch(r"csplat_raster_\w+\.h", f))
    assert parts
    included = {f: re.findall(r'^\s*#\s*include\s*["<](?:[^">]*/)?(csplat_raster_\w+\.h)[">]', open(os.path.join(csrc, f)).read(), re.M)
                for f in sorted(os.listdir(csrc)) if os.path.isfile(os.path.join(csrc, f))}
    assert sorted(included["csplat_raster.hip"]) == parts                  # each one, once
    assert all(not inc for f, inc in included.items() if f != "csplat_raster.hip"), included
    # what source_constants reads is the whole translation unit: no part's #include line is left in it
    assert not S.RASTER_PART.search(S.raster_source(csrc))


TABLE = {   # name -> (tiles, gx, gy, higher_msb, key bits, radix passes)
    "1x1": (1, 1, 1, 1, 33, 5), "1x17": (2, 1, 2, 1, 33, 5), "17x1": (2, 2, 1, 1, 33, 5), "15x15": (1, 1, 1, 1, 33, 5),
    "16x16": (1, 1, 1, 1, 33, 5), "17x17": (4, 2, 2, 2, 34, 5), "4099x17": (514, 257, 2, 10, 42, 6), "17x4099": (514, 2, 257, 10, 42, 6),
    "1920x1080": (8160, 120, 68, 13, 45, 6), "2048x1536": (12288, 128, 96, 14, 46, 6), "2064x1536": (12384, 129, 96, 14, 46, 6),
    "3841x2161": (32776, 241, 136, 16, 48, 6), "4096x4112": (65792, 256, 257, 17, 49, 7),
}


@pytest.mark.parametrize("name", list(SIZES))
def test_size_crosses_what_the_table_says(name):
    W, H = SIZES[name]
    tiles, gx, gy, msb, bits, passes = TABLE[name]
    assert grid_of(W, H) == (gx, gy) and tiles_of(W, H) == tiles
    assert S.higher_msb(tiles) == msb and (1 << msb) >= tiles and (tiles <= 2 or (1 << (msb - 1)) < tiles)
    assert S.end_bit(tiles) == bits and S.radix_passes(tiles) == passes
    assert (name in S.OVER_LIMIT) == (tiles > S.BUCKET_TILES)


def test_table_covers_every_switch():
    t = {n: tiles_of(*wh) for n, wh in SIZES.items()}
    assert t["2048x1536"] == S.BUCKET_TILES and t["2064x1536"] == S.BUCKET_TILES + 96     # the last bucket size, the first over it
    assert t["2064x1536"] > max(t[n] for n in SIZES if n not in S.OVER_LIMIT)
    assert t["1920x1080"] > 3 * 2500                                                       # the 800 x 800 config has 2500 tiles
    assert 1 << 15 < t["3841x2161"] < 1 << 16 < t["4096x4112"]
    assert SIZES["3841x2161"][0] % 16 == 1 and SIZES["3841x2161"][1] % 16 == 1             # ragged on both edges
    assert S.radix_passes(t["4096x4112"]) == 1 + max(S.radix_passes(v) for n, v in t.items() if n != "4096x4112")
    assert grid_of(*SIZES["1x17"])[0] == 1 and grid_of(*SIZES["17x1"])[1] == 1             # gx == 1, gy == 1, each with a ragged last tile
    assert SIZES["1x17"][1] % 16 == 1 and SIZES["17x1"][0] % 16 == 1
    assert grid_of(*SIZES["4099x17"])[0] > 256 and grid_of(*SIZES["17x4099"])[1] > 256
    assert [tiles_of(*SIZES[n]) for n in ("15x15", "16x16", "17x17")] == [1, 1, 4]
    # single-workgroup kernels (k_tile_scan, k_seg_plan: 1024 threads striding over the tiles) loop more than once from 1025 tiles on;
    # the tile id passes 16 bits in k_tile_ranges' keys at the largest size only
    assert sum(v > 1024 for v in t.values()) >= 5 and t["4096x4112"] - 1 > 0xFFFF
    assert set(S.OVER_LIMIT) | set(S.LAST_BUCKET) | set(S.DEGENERATE) <= set(SIZES) and set(S.EXTENDED_OVER) <= set(S.OVER_LIMIT)


# ------------------------------------------------------------------------------------------------ the scenes
def _placement(case, o):
    """markers: each visible, in the tile it was meant for, and blended at the pixel it sits on; the four corner tiles and the last row and
    column have list entries"""
    W, H = case["W"], case["H"]
    gx, gy = grid_of(W, H)
    m = case["marks"]
    L = S.lists_of(o)
    for t in (0, gx - 1, (gy - 1) * gx, gy * gx - 1):
        assert L[t] > 0, t
    for i, (x, y) in zip(m["corners"] + m["edges"], m["pixels"]):
        assert o.radii[i] > 0 and o.tiles_touched[i] >= 1
        assert abs(o.xy[i, 0] - x) < 1e-2 and abs(o.xy[i, 1] - y) < 1e-2, (i, o.xy[i], x, y)
        t = (int(y) // 16) * gx + int(x) // 16
        assert i in o.ids[o.ranges[t, 0]:o.ranges[t, 1]]
        assert o.n_contrib[int(y), int(x)] > 0
    corner_tiles = {(int(y) // 16) * gx + int(x) // 16 for x, y in m["pixels"][:4]}
    assert corner_tiles == {0, gx - 1, (gy - 1) * gx, gy * gx - 1}
    ex, ey = m["pixels"][4], m["pixels"][5]
    assert int(ex[1]) // 16 == gy - 1 and int(ey[0]) // 16 == gx - 1              # the last tile row, the last tile column
    if W % 16:
        assert all(int(x) >= (gx - 1) * 16 for x, _y in (m["pixels"][1], m["pixels"][3], m["pixels"][5]))      # ... the ragged ones
    # the full-grid Gaussian: its rectangle is the whole grid, and it is in every tile's list
    assert o.tiles_touched[m["full"]] == gx * gy and tuple(o.rect[m["full"]]) == (0, 0, gx, gy)
    assert L.min() >= 1


@pytest.mark.parametrize("name", list(SIZES))
def test_colour_scene_placement_and_oracle_pair(name):
    """placement, the long list, and the fp32 oracle against the fp64 one at the bars the GPU test applies to the kernels (image_err 1e-4
    with at most 1e-4 of the pixels as threshold ties)"""
    case = S.colour_case(name)
    W, H = SIZES[name]
    o, o64 = oracle_forward(case), oracle_forward(case, dtype=np.float64)
    _placement(case, o)
    tiles = tiles_of(W, H)
    L = S.lists_of(o)
    if tiles >= 8160:
        lo, hi, t = case["marks"]["cluster"]
        assert S.TILE_SORT_SMALL_CAP < L[t] == L.max() <= 8192        # longer than the small capacity, within the LDS sort's large one
        assert np.all(o.radii[lo:hi] > 0)
    if name in S.OVER_LIMIT:
        assert o.tiles_touched.max() == tiles > 12288 and o.R > 250_000
    assert S.image_err(o.color, o64.color) < TOL and S.image_err(o.out_depth, o64.out_depth) < TOL
    dpix = np.random.default_rng(3).normal(size=(3, H, W)).astype(np.float32)
    g32, g64 = util.ro.backward(o, dpix), util.ro.backward(o64, dpix)
    P = case["P"]
    for k in ("mean3D", "mean2D", "opacity", "sh", "scale", "rot"):
        a, b = (np.asarray(getattr(g, k), np.float64).reshape(P, -1) for g in (g32, g64))
        assert np.isfinite(b).all() and np.abs(b[:3000]).max() > 0, k            # (the cloth takes a gradient: the markers do not hide it)
        # the oracle pair's own error stays where 10 x it is still a check: at most twice what was measured -- over all Gaussians 4.7e-3
        # (4096 x 4112), over the 3000 cloth Gaussians alone 2.9e-3 (scale at 1920 x 1080: footprints of a hundred pixels and more,
        # sums of 1e5 fp32 terms; the markers and the cluster are not in those rows)
        assert rel_err(a, b) < 1e-2, (k, rel_err(a, b))
        assert rel_err(a[:3000], b[:3000]) < 6e-3, (k, rel_err(a[:3000], b[:3000]))


@pytest.mark.parametrize("name", list(S.DEGENERATE) + list(S.EXTENDED_OVER))
def test_sparse_scene_placement_and_oracle_pair(name):
    """the extended outputs' scenes: placement, and the oracle pair inside image_err's 1e-3 allowance of the extended-output bars"""
    case = S.sparse_case(name)
    W, H = SIZES[name]
    o, o64 = oracle_forward(case), oracle_forward(case, dtype=np.float64)
    _placement(case, o)
    assert S.image_err(o.color, o64.color, outlier_frac=1e-3) < TOL and S.image_err(o.out_depth, o64.out_depth, outlier_frac=1e-3) < TOL
    assert util.image_err(o.color, o64.color, outlier_frac=1e-3) < TOL
    assert np.array_equal(o.n_contrib, o64.n_contrib) or (o.n_contrib != o64.n_contrib).mean() < 1e-3


def test_image_err_on_a_one_pixel_image_exempts_nothing():
    a, b = np.full((3, 1, 1), 0.5), np.full((3, 1, 1), 0.505)
    assert abs(util.image_err(a, b) - 0.01 / 1.01) < 1e-3 and abs(S.image_err(a, b) - util.image_err(a, b)) < 1e-15
    # 17 pixels, one of them off: util.image_err's allowance rounds up to that pixel, image_sizes_ref.image_err has none there
    a, b = np.zeros((1, 1, 17)), np.ones((1, 1, 17))
    a[:] = 1.0
    a[0, 0, 5] = 1.005
    assert util.image_err(a, b) == 0.0 and abs(S.image_err(a, b) - 0.005) < 1e-12
