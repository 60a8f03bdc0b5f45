"""The radix sort and the scan of csrc/csplat_sort.hip as entry points of their own (csplat_sort_pairs_u64, csplat_scan_u32): everything
that can be checked without a GPU -- the C-ABI surface, every refusal (made before any launch: NULL streams and pointers suffice), the
temp sizes against what the wrappers carve, the numpy restatement (tests/sort_scan_ref.py) against Python's own stable `sorted` and a
running sum, and the case tables of tests/test_sort_scan_gpu.py against the list they were written from."""
import ctypes as C
import os
import re

import numpy as np

import util
import sort_scan_ref as R

NAMES = ("csplat_sort_pairs_temp_bytes", "csplat_sort_pairs_u64", "csplat_scan_u32_temp_bytes", "csplat_scan_u32")
A, B, T = 0x10000, 0x20000, 0x30000      # stand-ins for device pointers: a refusal reads none of them


def test_new_names_are_exported_declared_and_bound():
    from csplat import native
    hdr = open(os.path.join(util.ROOT, "include", "csplat.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = C.CDLL(native.LIB_PATH)
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, code), f"include/csplat.h does not declare {name}"
        assert hasattr(lib, name), f"libcsplat.so does not export {name}"
        assert name in native.EXPORTS, f"csplat.native does not bind {name}"
    assert re.search(r"#define\s+CSPLAT_ABI_VERSION\s+9\b", code)
    assert native.ABI_VERSION == 9 and native.lib.csplat_abi_version() == 9
    # the contract for high key bits stands next to the declaration
    assert "8 * ceil(end_bit / 8)" in hdr[hdr.index("csplat_sort_pairs_u64:"):hdr.index("size_t csplat_sort_pairs_temp_bytes")]


def test_sort_refusals_each_with_its_own_message():
    from csplat.native import lib
    err = lambda: lib.csplat_last_error().decode()  # noqa: E731
    sort = lib.csplat_sort_pairs_u64
    assert sort(None, -1, 8, A, A, B, B, T) != 0 and "csplat_sort_pairs_u64: bad n" in err()
    for bad in (0, -1, 65, 1 << 20):
        assert sort(None, 10, bad, A, A, B, B, T) != 0 and "csplat_sort_pairs_u64: end_bit" in err(), bad
    for hole in range(5):
        p = [A, A + 0x1000, B, B + 0x1000, T]
        p[hole] = None
        assert sort(None, 10, 8, *p) != 0 and "csplat_sort_pairs_u64: NULL" in err(), hole
    assert sort(None, 10, 8, A, A + 0x1000, A, B, T) != 0 and "csplat_sort_pairs_u64: in place (keys_out" in err()
    assert sort(None, 10, 8, A, A + 0x1000, B, A + 0x1000, T) != 0 and "csplat_sort_pairs_u64: in place (vals_out" in err()
    for end_bit in (1, 8, 33, 64):                  # n = 0: a no-op that accepts NULL
        assert sort(None, 0, end_bit, None, None, None, None, None) == 0


def test_scan_refusals_each_with_its_own_message():
    from csplat.native import lib
    err = lambda: lib.csplat_last_error().decode()  # noqa: E731
    scan = lib.csplat_scan_u32
    assert scan(None, -1, A, B, T) != 0 and "csplat_scan_u32: bad n" in err()
    for hole in range(3):
        p = [A, B, T]
        p[hole] = None
        assert scan(None, 10, *p) != 0 and "csplat_scan_u32: NULL" in err(), hole
    assert scan(None, 10, A, A, T) != 0 and "csplat_scan_u32: in place" in err()
    assert scan(None, 0, None, None, None) == 0


def test_temp_bytes_grow_with_n_and_cover_what_the_wrappers_carve():
    from csplat.native import lib
    a256 = lambda x: (x + 255) // 256 * 256  # noqa: E731
    sizes = sorted(set(R.SORT_SIZES + R.SCAN_SIZES + (0, 3, 4098, 12289, 1 << 24, (1 << 31) - 1)))
    prev_sort = prev_scan = 0
    for n in sizes:
        st, ct = int(lib.csplat_sort_pairs_temp_bytes(n)), int(lib.csplat_scan_u32_temp_bytes(n))
        tiles = -(-n // R.SORT_TILE)
        # a second key buffer, a second value buffer and the 256 x tiles table of u32, each on a 256-byte boundary -- and no more than that
        assert st >= a256(8 * n) + a256(4 * n) + a256(1024 * tiles), (n, st)
        assert st >= 12 * n + 1024 * tiles
        assert st <= 12 * n + 1024 * max(tiles, 1) + 3 * 256, (n, st)
        # one u32 per 2048-value tile and the total
        assert ct >= 4 * (-(-n // R.SCAN_TILE) + 1), (n, ct)
        assert ct <= 4 * (-(-n // R.SCAN_TILE) + 1) + 2 * 256, (n, ct)
        assert st >= prev_sort and ct >= prev_scan, n
        prev_sort, prev_scan = st, ct
    assert lib.csplat_sort_pairs_temp_bytes(1 << 20) > lib.csplat_sort_pairs_temp_bytes(1 << 10) > 0
    assert lib.csplat_scan_u32_temp_bytes(1 << 24) > lib.csplat_scan_u32_temp_bytes(1 << 10) > 0


def test_restatement_equals_pythons_stable_sort_and_a_running_sum():
    rng = np.random.default_rng(0)
    n_cases = 0
    for trial in range(40):
        n = int(rng.integers(1, 200))
        for end_bit in (1, 7, 8, 10, 33, 63, 64):
            for family in R.SORT_FAMILIES + R.HIGH_BITS_FAMILIES:
                make = R.sort_high_bits if family in R.HIGH_BITS_FAMILIES else R.sort_family
                keys, vals = make(family, n, end_bit, rng)
                k, v = R.sort_pairs(keys, vals, end_bit)
                m = (1 << R.ordered_bits(end_bit)) - 1
                want = sorted(zip(keys.tolist(), vals.tolist()), key=lambda kv: kv[0] & m)      # sorted() is stable
                assert list(zip(k.tolist(), v.tolist())) == want, (n, end_bit, family)
                assert k.dtype == np.uint64 and v.dtype == np.uint32
                n_cases += 1
        for family in R.SCAN_FAMILIES:
            x = R.scan_family(family, n, rng)
            run, want = 0, []
            for xi in x.tolist():
                run = (run + xi) & 0xFFFFFFFF
                want.append(run)
            got = R.inclusive_scan(x)
            assert got.dtype == np.uint32 and got.tolist() == want, (n, family)
            if family != "full u32":
                assert int(x.sum(dtype=np.uint64)) < (1 << 32)
            n_cases += 1
    assert n_cases > 300
    # the order ignores bits above the digits and heeds bits inside the last one (end_bit 10: bits 10..15 take part, 16.. do not)
    keys = np.array([1 << 16, (1 << 10) | 1, 2, 0], np.uint64)
    k, v = R.sort_pairs(keys, np.arange(4, dtype=np.uint32), 10)
    assert v.tolist() == [0, 3, 2, 1] and k.tolist() == [1 << 16, 0, 2, (1 << 10) | 1]


def test_families_are_what_their_names_say():
    rng = np.random.default_rng(1)
    for n in (1, 2, 257, 4097, 9000):
        for end_bit in R.SORT_END_BITS:
            fam = {f: R.sort_family(f, n, end_bit, rng) for f in R.SORT_FAMILIES}
            top = 8 * (R.passes(end_bit) - 1)
            assert (fam["equal"][0] == fam["equal"][0][0]).all() and (fam["equal"][1] == np.arange(n)).all()
            assert np.unique(fam["few"][0]).size <= 7
            assert (np.diff(fam["sorted"][0].astype(object)) >= 0).all()
            d = np.diff(fam["reversed"][0].astype(object))
            assert (d < 0).all() if (1 << end_bit) >= n else (d <= 0).all() and np.unique(fam["reversed"][0]).size == 1 << end_bit
            assert np.unique(fam["top byte"][0] & R.mask(top)).size == 1
            assert np.unique(fam["low byte"][0] >> np.uint64(8)).size == 1
            k = fam["tile digit"][0]
            whole = n - n % R.SORT_TILE
            assert np.unique(k[:whole]).size <= 1 and np.unique(k[whole:]).size <= 1
            if 0 < whole < n:
                assert all(((int(k[0]) ^ int(k[-1])) >> s) & 0xFF & ((1 << end_bit) - 1 >> s) for s in range(0, end_bit, 8)) and k[-1] < k[0]
            N = R.chamfer_n(end_bit)
            assert (end_bit == 1 or N & (N - 1)) and N.bit_length() <= end_bit and int(fam["chamfer"][0].max()) < N
            for f, (keys, vals) in fam.items():
                if f not in ("equal", "chamfer"):
                    assert vals[-1] == 0xFFFFFFFF and (n == 1 or vals[0] == 0), f
        for end_bit in R.HIGH_BITS_END_BITS:
            ob = R.ordered_bits(end_bit)
            above, _ = R.sort_high_bits("above the digits", n, end_bit, rng)
            assert ((above & R.mask(ob)) >> np.uint64(end_bit) == 0).all()
            if ob < 64 and n > 100:
                assert ((above >> np.uint64(ob)) != 0).any()
                inside, _ = R.sort_high_bits("inside the last digit", n, end_bit, rng)
                assert (((inside & R.mask(ob)) >> np.uint64(end_bit)) != 0).any()


def test_case_tables_hold_every_listed_size_width_and_family():
    assert set(R.SORT_SIZES) == {1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 8192, 8193, 65536, 65537, 69633,
                                 1_000_003}
    assert set(R.SORT_END_BITS) == {1, 7, 8, 9, 16, 17, 24, 25, 31, 32, 33, 40, 41, 48, 49, 56, 57, 63, 64}
    assert {R.passes(b) for b in R.SORT_END_BITS} == set(range(1, 9))
    cases = R.sort_cases()
    assert len(set(cases)) == len(cases)
    for n in R.SORT_SIZES:
        mine = {b for m, b in cases if m == n}
        if n <= 8193:
            assert mine == set(R.SORT_END_BITS), n                              # the full cross
        else:
            assert {R.passes(b) for b in mine} == set(range(1, 9)), n           # every pass count
            assert mine <= set(R.SORT_END_BITS)
    assert {b for n, b in cases if n > 8193} == set(R.SORT_END_BITS)
    assert len(R.SORT_FAMILIES) == 9 and set(R.HIGH_BITS_END_BITS) == {10, 33, 63}
    assert set(R.SCAN_SIZES) == {1, 7, 8, 9, 2047, 2048, 2049, 4096, 4097, 1_000_001, 8_388_608, 8_388_609}
    assert len(R.SCAN_FAMILIES) == 7
    # 65537 keys are the first to need the second sweep of the histogram table's scan; 8 388 609 values the first past 4096 block sums
    assert 256 * -(-65536 // R.SORT_TILE) == 4096 and 256 * -(-65537 // R.SORT_TILE) > 4096
    assert -(-8_388_608 // R.SCAN_TILE) == 4096 and -(-8_388_609 // R.SCAN_TILE) == 4097
