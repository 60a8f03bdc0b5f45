"""Image sizes and scenes of tests/test_raster_image_sizes_{cpu,gpu}.py (helper, not collected): from a 1-pixel image to beyond the
tile count at which the rasterizer's host code changes path.

What the host code switches on (restated here, asserted against the sources by the CPU test):
    tiles = ceil(W / 16) * ceil(H / 16)
    tiles <= BUCKET_TILES (12288): per-tile buckets (LDS histogram of tiles * 4 bytes), the batched launchers, the speculative second phase;
    tiles  > BUCKET_TILES: no bucket table -- P-scan, k_emit_keys, the global radix sort over end_bit = 32 + higher_msb(tiles) key bits
    (ceil(end_bit / 8) passes of 8-bit digits), k_tile_ranges, and rasterize_views goes view by view.

Two kinds of scene per size:
  colour_case(name)  the dense cloth of tests/test_raster_gpu.py's ragged CASE (make_case(P=3000, grid=16, scale_mul=2.5)) plus MARKERS:
                     a small (sigma 2 px, opacity 0.35) Gaussian in each corner pixel and in the middle of the last tile row and column, one translucent
                     Gaussian whose rectangle spans the whole tile grid (tiles_touched == tiles), and, from 8160 tiles up, a cluster of
                     5500 small translucent Gaussians inside one tile (a tile list longer than the tile sort's small capacity, 5120).
                     Checked with the C oracle in fp32 and fp64 only.
  sparse_case(name)  60 small cloth Gaussians plus the same markers (the cluster left out): what the fp64 torch restatement
                     (tests/antialias_ref.py + autograd, one Python iteration per tile) can afford.

Measured on this project's CPU machine (seconds).  colour_case, C oracle forward and backward in fp32 and in fp64 together: under 0.5 up to
the 514-tile strips, 1.5 at 1920 x 1080 and 2048 x 1536, 0.8 at 2064 x 1536, 1.1 at 3841 x 2161, 7.7 at 4096 x 4112.  sparse_case,
antialias_ref.render + its backward + visibility_ref on ONE torch thread (sixteen cost ten times as much on tile-sized operations): under 1
on the degenerate sizes (514 non-empty tiles on the strips); 36.5 at 2064 x 1536, where the full-grid Gaussian leaves none of the 12 384
tiles empty (2 ms each, plus the 1.2 M-pixel images), against 0.6 s of the slowest test of tests/test_raster_extended_edges_gpu.py: over
the limit the GPU test therefore checks the extended outputs without the restatement, against the C fp64 oracle on the colour path.
"""
import os
import re

import numpy as np

import util
from util import make_case

BUCKET_TILES = 12288          # csplat_raster_binning.h: most tiles of the bucket path
RADIX_DIGIT_BITS = 8          # csplat_sort.hip: RADIX = 256
TILE_SORT_SMALL_CAP = 5120    # csplat_raster.hip: tile_sort_cap() when the device refuses 96 KB of LDS per workgroup
TILE = 16

SIZES = {   # name -> (W, H); the order is the order of the tests (small first)
    "1x1": (1, 1), "1x17": (1, 17), "17x1": (17, 1), "15x15": (15, 15), "16x16": (16, 16), "17x17": (17, 17),
    "4099x17": (4099, 17), "17x4099": (17, 4099), "1920x1080": (1920, 1080), "2048x1536": (2048, 1536), "2064x1536": (2064, 1536),
    "3841x2161": (3841, 2161), "4096x4112": (4096, 4112),
}
OVER_LIMIT = ("2064x1536", "3841x2161", "4096x4112")
LAST_BUCKET = ("1920x1080", "2048x1536")           # bucket path, compared with the forced global sort
DEGENERATE = ("1x1", "17x1", "1x17", "16x16", "4099x17", "17x4099")
EXTENDED_OVER = ("2064x1536", "3841x2161")        # the over-limit sizes of the extended-output and batched tests
CLUSTER = 5500                                     # Gaussians of the one-tile cluster (> TILE_SORT_SMALL_CAP)


def grid_of(W, H):
    return (W + TILE - 1) // TILE, (H + TILE - 1) // TILE


def tiles_of(W, H):
    gx, gy = grid_of(W, H)
    return gx * gy


def higher_msb(n):
    """csplat_raster.hip (host half) higher_msb: bits needed for tile ids < n, at least 1"""
    b = 0
    while (1 << b) < n and b < 31:
        b += 1
    return b if b else 1


def end_bit(tiles):
    return 32 + higher_msb(tiles)


def radix_passes(tiles):
    return (end_bit(tiles) + RADIX_DIGIT_BITS - 1) // RADIX_DIGIT_BITS


RASTER_PART = re.compile(r'^#include "(csplat_raster_\w+\.h)"[^\n]*$', re.M)


def raster_source(csrc):
    """csplat_raster.hip with its parts (csrc/csplat_raster_*.h) in the place of their #include lines: the rasterizer's text in include order"""
    return RASTER_PART.sub(lambda m: open(os.path.join(csrc, m.group(1))).read(), open(os.path.join(csrc, "csplat_raster.hip")).read())


def source_constants():
    """the launch constants this module restates, read from the HIP sources"""
    csrc = os.path.join(util.ROOT, "cloth-splatting_amd", "csrc")
    raster = raster_source(csrc)
    sort = open(os.path.join(csrc, "csplat_sort.hip")).read()
    one = lambda pat, text: re.search(pat, text, re.S).group(1)  # noqa: E731
    return dict(
        BUCKET_TILES=int(one(r"constexpr int BUCKET_TILES = (\d+);", raster)),
        BUCKET_CAP=int(one(r"constexpr int BUCKET_CAP = (\d+);", raster)),
        small_cap=int(one(r"return s_lds_big \? \(uint32_t\)BUCKET_CAP : (\d+)u;", raster)),
        can_bucket=one(r"const bool can_bucket = ([^;]+);", raster),
        end_bit=one(r"const int end_bit = ([^;]+);", raster),
        higher_msb=one(r"int higher_msb\(uint32_t n\) \{[^\n]*\n(.*?)\n\}", raster),
        RADIX=int(one(r"constexpr int RADIX = (\d+);", sort)),
        passes=one(r"const int passes = ([^;]+);", sort),
        shifts=re.findall(r"k_sort_(?:hist|scatter)<<<[^;]*?, (p \* \d+), nb\);", sort),
        digit_masks=re.findall(r">> shift\) & (0x[0-9A-Fa-f]+)", sort),
    )


# ------------------------------------------------------------------------------------------------ scenes
def _unproject(cam, W, H, px, py, z):
    """world position of the point that projects to pixel centre (px, py) at view-space depth z (row-vector matrices, util / oracle)"""
    ndcx, ndcy = (2.0 * px + 1.0) / W - 1.0, (2.0 * py + 1.0) / H - 1.0
    pv = np.array([ndcx * cam["tanfovx"] * z, ndcy * cam["tanfovy"] * z, z, 1.0])
    Vm = np.asarray(cam["world_view_transform"], np.float64).reshape(4, 4)
    return (pv @ np.linalg.inv(Vm))[:3]


def marker_pixels(W, H):
    """pixel centres of the small markers: the four corner tiles, the middle of the last tile row and of the last tile column"""
    x0, y0, x1, y1 = 0, 0, W - 1, H - 1          # the image's own corner pixels: the last column / row may be one pixel wide
    # (a third of a pixel off the pixel centres: a Gaussian centred exactly on the only pixel it covers takes no shape gradient)
    return [(x + 0.3, y + 0.2) for x, y in [(x0, y0), (x1, y0), (x0, y1), (x1, y1), (W // 2, y1), (x1, H // 2)]]


def _append(case, means, scales, opac, rng):
    g = case["g"]
    n = len(means)
    quat = np.tile(np.array([1.0, 0.0, 0.0, 0.0], np.float32), (n, 1))
    shs = np.concatenate([rng.normal(0, 1.0, (n, 1, 3)), rng.normal(0, 0.2, (n, 15, 3))], 1).astype(np.float32)
    case["g"] = dict(means3D=np.concatenate([g["means3D"], np.asarray(means, np.float32)]),
                     scales=np.concatenate([g["scales"], np.asarray(scales, np.float32)]),
                     rotations=np.concatenate([g["rotations"], quat]),
                     opacities=np.concatenate([g["opacities"], np.asarray(opac, np.float32).reshape(n, 1)]),
                     shs=np.concatenate([g["shs"], shs]))
    case["P"] += n
    return case


def _with_markers(case, cluster, seed):
    """appends (in this order) the 6 small markers, the full-grid Gaussian and, if asked, the one-tile cluster; case["marks"] names them"""
    W, H, cam = case["W"], case["H"], case["cam"]
    rng = np.random.default_rng(seed)
    focal = W / (2.0 * cam["tanfovx"])
    P0 = case["P"]
    z = 3.0                                      # in front of the cloth (camera radius 4)
    pix = marker_pixels(W, H)
    means = [_unproject(cam, W, H, x, y, z) for x, y in pix]
    scales = [np.full(3, 2.0 * z / focal)] * len(pix)           # sigma = 2 px
    opac = [0.35] * len(pix)                     # (translucent: on a one-tile image all six lie on top of each other)
    # the full-grid Gaussian: radius = ceil(3 sigma) reaches every tile from the image centre
    sig_px = (0.5 * max(W, H) + 2 * TILE) / 3.0 * 1.05
    means.append(_unproject(cam, W, H, 0.5 * (W - 1), 0.5 * (H - 1), 2.5))
    scales.append(np.full(3, sig_px * 2.5 / focal))
    opac.append(0.2)
    case = _append(case, means, scales, opac, rng)
    marks = dict(corners=list(range(P0, P0 + 4)), edges=[P0 + 4, P0 + 5], full=P0 + 6, cluster=None, pixels=pix)
    if cluster:
        gx, gy = grid_of(W, H)
        tx, ty = gx // 3, gy // 3                  # a tile off the centre
        cx = rng.uniform(tx * TILE + 2.0, tx * TILE + 13.0, cluster)
        cy = rng.uniform(ty * TILE + 2.0, ty * TILE + 13.0, cluster)
        cz = rng.uniform(2.6, 3.4, cluster)
        cm = [_unproject(cam, W, H, x, y, d) for x, y, d in zip(cx, cy, cz)]
        cs = [np.full(3, 0.25 * d / focal) for d in cz]           # sigma 0.25 px (+ the 0.3 px^2 dilation): radius 2 px, inside the tile
        co = rng.uniform(0.01, 0.03, cluster)
        marks["cluster"] = (case["P"], case["P"] + cluster, ty * gx + tx)
        case = _append(case, cm, cs, co, rng)
    case["marks"] = marks
    return case


def _fovx(W, H):
    """the standard field of view along the LONGER side (a 17 x 4099 image with it along its 17 pixels would see 179 degrees along the
    other axis, where every footprint is the frustum clamp's)"""
    return 2.0 * np.arctan(np.tan(0.5 * util.syn.CAMERA_ANGLE_X) * W / max(W, H))


def colour_case(name):
    W, H = SIZES[name]
    case = make_case(P=3000, W=W, H=H, seed=8, grid=16, scale_mul=2.5, fovx=_fovx(W, H))
    return _with_markers(case, CLUSTER if tiles_of(W, H) >= 8160 else 0, seed=1000 + W + H)


def sparse_case(name, seed=0):
    W, H = SIZES[name]
    case = make_case(P=60, W=W, H=H, seed=9 + seed, grid=16, scale_mul=1.5, fovx=_fovx(W, H))
    return _with_markers(case, 0, seed=2000 + W + H + seed)


def lists_of(o):
    return o.ranges[:, 1] - o.ranges[:, 0]


def image_err(a, b, outlier_frac=1e-4):
    """util.image_err; on an image too small for its threshold-tie allowance to be a whole pixel (pixels * outlier_frac < 1; util.image_err
    rounds the allowance UP, which on a 1-pixel image exempts the only pixel) no pixel is exempt: the plain relative max error"""
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    if a.shape[-1] * a.shape[-2] * outlier_frac < 1.0:
        return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-30))
    return util.image_err(a, b, outlier_frac=outlier_frac)
