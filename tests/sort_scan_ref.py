"""The two device-wide primitives of csrc/csplat_sort.hip restated in numpy -- csplat_sort_pairs_u64 (stable LSD radix sort of
(u64 key, u32 value) pairs, whole 8-bit digits) and csplat_scan_u32 (inclusive scan modulo 2^32) -- and the case tables that
tests/test_sort_scan_cpu.py and tests/test_sort_scan_gpu.py share.  No GPU, no library: numpy only."""
import numpy as np

SORT_TILE = 4096          # keys per workgroup of the sort
SCAN_TILE = 2048          # values per workgroup of the scan
U64 = np.uint64


def passes(end_bit):
    """8-bit passes of the sort: their parity decides whether the result ends in the output or the temporary buffers"""
    return (end_bit + 7) // 8


def ordered_bits(end_bit):
    """the sort orders key bits [0, ordered_bits): whole digits"""
    return 8 * passes(end_bit)


def mask(bits):
    return U64((1 << bits) - 1)


def sort_pairs(keys, vals, end_bit):
    keys, vals = np.asarray(keys, U64), np.asarray(vals, np.uint32)
    order = np.argsort(keys & mask(ordered_bits(end_bit)), kind="stable")
    return keys[order], vals[order]


def inclusive_scan(x):
    return np.cumsum(np.asarray(x, np.uint32), dtype=U64).astype(np.uint32)


# ---------------------------------------------------------------- the sort's cases
# wave (64), workgroup (256), 1024, tile (4096) and two-tile edges; 65537 = 17 tiles is the first size whose 256 x tiles histogram table
# (4352 entries) needs the second 4096-entry sweep of the single-workgroup scan; 69633 = 17 tiles + 1; 1 000 003 is ragged, 245 tiles
SORT_SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 8192, 8193, 65536, 65537, 69633, 1_000_003)
# both sides of every byte edge: pass counts 1..8
SORT_END_BITS = (1, 7, 8, 9, 16, 17, 24, 25, 31, 32, 33, 40, 41, 48, 49, 56, 57, 63, 64)
SORT_CROSS_UP_TO = 8193
# above the full cross every size meets every pass count once; between them the four rows use every end_bit
SORT_LARGE = {65536: (1, 9, 17, 25, 33, 41, 49, 57),
              65537: (8, 16, 24, 32, 40, 48, 56, 64),
              69633: (7, 16, 17, 31, 40, 41, 56, 63),
              1_000_003: (8, 9, 24, 25, 33, 48, 49, 64)}
SORT_FAMILIES = ("uniform", "equal", "few", "sorted", "reversed", "top byte", "low byte", "tile digit", "chamfer")
HIGH_BITS_END_BITS = (10, 33, 63)
HIGH_BITS_SIZES = (1, 65, 4097, 8193, 69633)
HIGH_BITS_FAMILIES = ("above the digits", "inside the last digit")


def sort_cases():
    """(n, end_bit): the full cross up to SORT_CROSS_UP_TO, SORT_LARGE above"""
    out = [(n, b) for n in SORT_SIZES if n <= SORT_CROSS_UP_TO for b in SORT_END_BITS]
    for n in SORT_SIZES:
        if n > SORT_CROSS_UP_TO:
            out += [(n, b) for b in SORT_LARGE[n]]
    return out


def _uniform(rng, n, bits):
    if bits <= 0:
        return np.zeros(n, U64)
    return rng.integers(0, (1 << bits) - 1, n, dtype=U64, endpoint=True)


def _bytes_of(byte, end_bit):
    """`byte` in every byte, cut to below 2^end_bit"""
    return U64(int.from_bytes(bytes([byte]) * 8, "little") & ((1 << end_bit) - 1))


def chamfer_n(end_bit):
    """a cloud size that is no power of two (but for end_bit 1: one point) whose indices need end_bit bits or fewer"""
    return max(1, (3 << end_bit) // 4) | 1 if end_bit > 1 else 1


def sort_values(rng, n):
    """random u32 with 0 and 0xFFFFFFFF among them"""
    v = rng.integers(0, 1 << 32, n, dtype=np.uint32)
    v[0] = 0
    v[-1] = 0xFFFFFFFF
    return v


def sort_family(family, n, end_bit, rng):
    """(keys u64 [n], vals u32 [n]) of one family; every key is below 2^end_bit"""
    top_shift = 8 * (passes(end_bit) - 1)          # the top used byte: bits [top_shift, end_bit)
    vals = sort_values(rng, n)
    if family == "uniform":
        keys = _uniform(rng, n, end_bit)
    elif family == "equal":                          # pure stability: the values must come out as they went in
        keys = np.full(n, _uniform(rng, 1, end_bit)[0], U64)
        vals = np.arange(n, dtype=np.uint32)
    elif family == "few":                            # at most 7 distinct keys
        keys = _uniform(rng, 7, end_bit)[rng.integers(0, 7, n)]
    elif family == "sorted":
        keys = np.sort(_uniform(rng, n, end_bit))
    elif family == "reversed":
        # strictly decreasing over the whole range where 2^end_bit has n values; else non-increasing through every value
        i = np.arange(n - 1, -1, -1, dtype=U64)
        if (1 << end_bit) >= n:
            keys = i * U64(((1 << end_bit) - 1) // max(n - 1, 1))
        else:
            keys = (i << U64(end_bit)) // U64(n)
    elif family == "top byte":                       # only the last pass moves anything
        keys = _uniform(rng, 1, top_shift)[0] | (_uniform(rng, n, end_bit - top_shift) << U64(top_shift))
    elif family == "low byte":                       # only the first pass moves anything
        low = min(8, end_bit)
        keys = ((_uniform(rng, 1, end_bit)[0] >> U64(low)) << U64(low)) | _uniform(rng, n, low)
    elif family == "tile digit":
        # every whole tile holds one key (one digit in every pass: a histogram column of 4096), the ragged tail another that differs in
        # every used byte and is smaller: the tail moves in front of all tiles
        keys = np.full(n, _bytes_of(0xC3, end_bit), U64)
        keys[n - n % SORT_TILE:] = _bytes_of(0x3C, end_bit)
    elif family == "chamfer":                        # the Chamfer backward's (nearest index, query) pairs
        keys = rng.integers(0, chamfer_n(end_bit), n, dtype=U64)
        vals = np.arange(n, dtype=np.uint32)
    else:
        raise KeyError(family)
    assert keys.dtype == U64 and keys.shape == (n,) and (end_bit == 64 or int(keys.max()) < (1 << end_bit)), (family, n, end_bit)
    return keys, vals


def sort_high_bits(family, n, end_bit, rng):
    """uniform keys below 2^end_bit with random bits set above them.
    "above the digits": at or above ordered_bits(end_bit) -- they travel with their key and must not affect the order (there is no such
    bit for end_bit 63: the keys are then plain uniform ones);
    "inside the last digit": in [end_bit, ordered_bits(end_bit)) as well -- those take part in the order, as the header states."""
    keys = _uniform(rng, n, end_bit)
    ob = ordered_bits(end_bit)
    if ob < 64:
        keys = keys | (_uniform(rng, n, 64 - ob) << U64(ob))
    if family == "inside the last digit":
        keys = keys | (_uniform(rng, n, ob - end_bit) << U64(end_bit))
    elif family != "above the digits":
        raise KeyError(family)
    return keys, sort_values(rng, n)


# ---------------------------------------------------------------- the scan's cases
# item (8 per thread) and tile edges; 4096, 4097: two tiles and the third; 8 388 608 = 4096 tiles fills the first sweep of the block sums'
# scan exactly, 8 388 609 is one block sum past it
SCAN_SIZES = (1, 7, 8, 9, 2047, 2048, 2049, 4096, 4097, 1_000_001, 8_388_608, 8_388_609)
SCAN_FAMILIES = ("all 1", "all 0", "first", "last", "below 2^16", "full u32", "raster")


def scan_family(family, n, rng):
    """u32 [n].  Every family but "full u32" has a total below 2^32: the modular reference is then the plain sum"""
    if family == "all 1":
        return np.ones(n, np.uint32)
    if family == "all 0":
        return np.zeros(n, np.uint32)
    if family in ("first", "last"):
        x = np.zeros(n, np.uint32)
        x[0 if family == "first" else -1] = 1
        return x
    if family == "below 2^16":                       # capped so that n * (largest value) stays below 2^32
        return rng.integers(0, min(1 << 16, ((1 << 32) - 1) // n + 1), n, dtype=np.uint32)
    if family == "full u32":                         # the sums wrap many times
        x = rng.integers(0, 1 << 32, n, dtype=np.uint32)
        x[-1] = 0xFFFFFFFF
        return x
    if family == "raster":                           # tiles_touched: mostly 0, now and then up to 4096
        return np.where(rng.random(n) < 0.05, rng.integers(1, 4097, n), 0).astype(np.uint32)
    raise KeyError(family)
