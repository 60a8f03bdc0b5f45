"""The two device-wide primitives everything else is built on -- csplat_sort_pairs_u64 (k_sort_hist, k_scan_single, k_sort_scatter) and
csplat_scan_u32 (k_scan_block_sums, k_scan_single, k_scan_final) of csrc/csplat_sort.hip -- against the numpy restatement
tests/sort_scan_ref.py, bit for bit.  Their consumers cannot witness them: the k-NN searches are exact for any order of the sorted codes,
the rasterizer reaches one or two pass counts at three scenes, csplat_mask_to_map scans 0 / 1 flags only.

Sizes: wave, workgroup and tile edges, the first size whose histogram table needs the second sweep of its scan (65537 keys), a ragged
245-tile size; every pass count 1..8 (its parity decides which buffer the result ends in) on both sides of every byte edge; nine key
families; key bits above the sorted ones.  The scan: item and tile edges, one past 4096 block sums, sums that wrap.

Every call (the discipline of _scatter_case in tests/test_train_kernels_gpu.py): the outputs are pre-filled with a sentinel and compared
WHOLE, 64 sentinel words past n included; `temp` is exactly *_temp_bytes(n) long plus 256 guard bytes that must survive; the inputs are
compared with their host copies afterwards.  There is no tolerance anywhere in this file: integers, equality."""
import numpy as np
import pytest

import util  # noqa: F401
import sort_scan_ref as R

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

PAST = 64                                     # sentinel words past n in every output
GUARD = 256                                   # guard bytes past temp_bytes(n)
KEY_SENTINEL, VAL_SENTINEL, GUARD_BYTE = 0x7A7A7A7A7A7A7A7A, 0x5B5B5B5B, 0xA5


def _lib():
    from csplat import native as n_
    return n_, torch.device("cuda")


def _dev(a, dev):
    """a host array of u64 / u32 as a device tensor of the same bits (torch has no arithmetic on unsigned 32 / 64: bits only)"""
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view({8: np.int64, 4: np.int32}[a.dtype.itemsize])).to(dev)


def _host(t, dtype):
    return t.cpu().numpy().view(dtype)


def _first_difference(got, want):
    bad = np.flatnonzero(got != want)
    return f"{bad.size} rows differ, first {bad[0]}: {int(got[bad[0]]):#x} != {int(want[bad[0]]):#x}" if bad.size else None


def _run_sort(keys, vals, end_bit):
    """one call of csplat_sort_pairs_u64 on the current stream -> (keys_out [n], vals_out [n]) after the buffer checks"""
    n_, dev = _lib()
    n = keys.shape[0]
    k_in, v_in = _dev(keys, dev), _dev(vals, dev)
    k_out = _dev(np.full(n + PAST, KEY_SENTINEL, np.uint64), dev)
    v_out = _dev(np.full(n + PAST, VAL_SENTINEL, np.uint32), dev)
    nbytes = int(n_.lib.csplat_sort_pairs_temp_bytes(n))
    temp = torch.full((nbytes + GUARD,), GUARD_BYTE, dtype=torch.uint8, device=dev)
    n_.check(n_.lib.csplat_sort_pairs_u64(n_.stream_handle(dev), n, end_bit, n_.ptr(k_in), n_.ptr(v_in), n_.ptr(k_out), n_.ptr(v_out),
                                          n_.ptr(temp)), "csplat_sort_pairs_u64")
    torch.cuda.current_stream().synchronize()
    got_k, got_v = _host(k_out, np.uint64), _host(v_out, np.uint32)
    assert (got_k[n:] == KEY_SENTINEL).all() and (got_v[n:] == VAL_SENTINEL).all(), f"n {n} end_bit {end_bit}: a write past n"
    assert bool((temp[nbytes:] == GUARD_BYTE).all()), f"n {n} end_bit {end_bit}: a write past csplat_sort_pairs_temp_bytes(n)"
    assert np.array_equal(_host(k_in, np.uint64), keys) and np.array_equal(_host(v_in, np.uint32), vals), \
        f"n {n} end_bit {end_bit}: the inputs were written"
    return got_k[:n], got_v[:n]


def _check_sort(n, end_bit, family, keys, vals):
    got_k, got_v = _run_sort(keys, vals, end_bit)
    want_k, want_v = R.sort_pairs(keys, vals, end_bit)
    bad = _first_difference(got_k, want_k) or _first_difference(got_v, want_v)
    if bad:
        raise AssertionError(f"n {n} end_bit {end_bit} ({R.passes(end_bit)} passes) family {family}: "
                             f"{'keys' if not np.array_equal(got_k, want_k) else 'values'}: {bad}")
    return got_k, got_v


@pytest.mark.parametrize("n,end_bit", R.sort_cases())
def test_sort_pairs_equals_the_stable_reference_bit_for_bit(n, end_bit):
    """all nine key families at one (n, end_bit); values are random u32 with 0 and 0xFFFFFFFF among them (arange where the family says so)"""
    for j, family in enumerate(R.SORT_FAMILIES):
        keys, vals = R.sort_family(family, n, end_bit, np.random.default_rng([n, end_bit, j]))
        got_k, got_v = _check_sort(n, end_bit, family, keys, vals)
        if family == "equal":       # pure stability across waves and workgroups, said once more without the reference
            assert np.array_equal(got_v, np.arange(n, dtype=np.uint32)), f"n {n} end_bit {end_bit}: equal keys changed their order"


@pytest.mark.parametrize("end_bit", R.HIGH_BITS_END_BITS)
@pytest.mark.parametrize("n", R.HIGH_BITS_SIZES)
def test_sort_key_bits_above_the_sorted_digits_travel_and_do_not_order(n, end_bit):
    """bits at or above 8 * ceil(end_bit / 8) come out with their key and leave the order alone; bits in [end_bit, 8 * ceil(end_bit / 8))
    take part in it -- the contract include/csplat.h states (the reference masks to whole digits)"""
    for j, family in enumerate(R.HIGH_BITS_FAMILIES):
        keys, vals = R.sort_high_bits(family, n, end_bit, np.random.default_rng([n, end_bit, 100 + j]))
        got_k, got_v = _check_sort(n, end_bit, family, keys, vals)
        # whatever the order: the output is a permutation of the input PAIRS, high bits included
        assert np.array_equal(np.sort(got_k), np.sort(keys))
        if R.ordered_bits(end_bit) < 64 and family == "above the digits":
            low_k, low_v = _run_sort(keys & R.mask(R.ordered_bits(end_bit)), vals, end_bit)
            assert np.array_equal(low_v, got_v) and np.array_equal(low_k, got_k & R.mask(R.ordered_bits(end_bit))), \
                f"n {n} end_bit {end_bit}: bits above the digits changed the order"


def _run_scan(x):
    n_, dev = _lib()
    n = x.shape[0]
    d_in = _dev(x, dev)
    d_out = _dev(np.full(n + PAST, VAL_SENTINEL, np.uint32), dev)
    nbytes = int(n_.lib.csplat_scan_u32_temp_bytes(n))
    temp = torch.full((nbytes + GUARD,), GUARD_BYTE, dtype=torch.uint8, device=dev)
    n_.check(n_.lib.csplat_scan_u32(n_.stream_handle(dev), n, n_.ptr(d_in), n_.ptr(d_out), n_.ptr(temp)), "csplat_scan_u32")
    torch.cuda.current_stream().synchronize()
    got = _host(d_out, np.uint32)
    assert (got[n:] == VAL_SENTINEL).all(), f"n {n}: a write past n"
    assert bool((temp[nbytes:] == GUARD_BYTE).all()), f"n {n}: a write past csplat_scan_u32_temp_bytes(n)"
    assert np.array_equal(_host(d_in, np.uint32), x), f"n {n}: the input was written"
    return got[:n]


@pytest.mark.parametrize("n", R.SCAN_SIZES)
def test_scan_equals_the_running_sum_modulo_2_32(n):
    """values above 1: every family of tests/sort_scan_ref.py; the full-u32 family wraps, the others stay below 2^32 in total"""
    for j, family in enumerate(R.SCAN_FAMILIES):
        x = R.scan_family(family, n, np.random.default_rng([n, j]))
        want = R.inclusive_scan(x)
        if family != "full u32":
            assert int(want[-1]) == int(x.sum(dtype=np.uint64)), (n, family)     # the case does not wrap: the sums are the plain sums
        bad = _first_difference(_run_scan(x), want)
        if bad:
            raise AssertionError(f"n {n} family {family}: {bad}")


def test_a_non_default_stream_gives_the_bits_of_the_default_stream():
    n_, dev = _lib()
    rng = np.random.default_rng(5)
    n, end_bit = 69633, 41
    keys, vals = R.sort_family("uniform", n, end_bit, rng)
    x = R.scan_family("full u32", 1_000_001, rng)
    base_k, base_v = _check_sort(n, end_bit, "uniform", keys, vals)
    base_s = _run_scan(x)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        assert n_.stream_handle(dev) == side.cuda_stream != 0
        side_k, side_v = _run_sort(keys, vals, end_bit)
        side_s = _run_scan(x)
    torch.cuda.synchronize()
    assert np.array_equal(side_k, base_k) and np.array_equal(side_v, base_v)
    assert np.array_equal(side_s, base_s) and np.array_equal(base_s, R.inclusive_scan(x))


def test_the_sort_is_deterministic():
    """17 tiles + 1 key, 8 passes, twice on the same input: identical outputs (few distinct keys: long runs whose order only stability fixes)"""
    rng = np.random.default_rng(6)
    n, end_bit = 69633, 63
    for family in ("uniform", "few"):
        keys, vals = R.sort_family(family, n, end_bit, rng)
        a_k, a_v = _check_sort(n, end_bit, family, keys, vals)
        b_k, b_v = _run_sort(keys, vals, end_bit)
        assert np.array_equal(a_k, b_k) and np.array_equal(a_v, b_v)
