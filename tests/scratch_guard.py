"""Guarded buffers for the tests of the scratch / temp contracts of include/csplat.h (a plain helper module, not a conftest).

A `*_temp_bytes` / `*_scratch_bytes` / `*_workspace_bytes` query promises two things that a `torch.empty(max(bytes, 256))` from a fresh
allocator cannot witness: that the entry writes nothing outside the bytes the query names, and that it reads no word of them before it
has written it (where the header says "any contents").  `guarded` gives a buffer of EXACTLY the queried size, filled with a hostile byte,
between two guard regions whose bytes must survive the call.

FILLS: 0x00 (what a fresh allocator usually returns -- the fill under which a read-before-write passes), 0xFF (float NaN, int32 -1,
uint32 / uint64 maximum: a counter or ticket that starts "full", a partial sum that poisons), 0x7F (float 3.39e38 -- finite, so it survives
a NaN guard and overflows a sum -- and a huge positive integer)."""
import numpy as np
import torch

FILLS = (0x00, 0xFF, 0x7F)
GUARD_BYTES = 4096           # on either side of the view
GUARD_VALUES = (0xA5, 0x5A)  # the guard byte is the first of these that differs from the fill
OUT_FILL = 0xCD              # what guarded outputs hold before a call: float -4.316e8, int32 -842150451 (no valid index, count or loss)


def guarded(nbytes, fill, device, align=256, zero_words=()):
    """-> (view, check).  view: uint8 [nbytes] (exactly: no minimum size), every byte == fill, starting at an `align`-aligned address
    inside a larger allocation with >= GUARD_BYTES guard bytes before and behind it.  zero_words: indices of 4-byte words of the view
    (negative = from its end) cleared after the fill, for contracts of the form "word k is zero on entry".
    check(what=""): asserts that both guards are intact, naming the first damaged offset relative to the view (negative = in front).
    check.ptr: the view's address as an integer -- valid also when nbytes == 0 (torch reports no address for an empty tensor).
    check.restored(what=""): asserts that the zero_words are zero (again)."""
    nbytes = int(nbytes)
    assert nbytes >= 0 and align >= 1 and 0 <= fill <= 0xFF
    guard = next(g for g in GUARD_VALUES if g != fill)
    base = torch.full((GUARD_BYTES + align + nbytes + GUARD_BYTES,), guard, dtype=torch.uint8, device=device)
    off = GUARD_BYTES + (-(base.data_ptr() + GUARD_BYTES)) % align
    view = base[off:off + nbytes]
    view.fill_(fill)
    words = [int(k) for k in zero_words]
    for k in words:
        assert -(nbytes // 4) <= k < nbytes // 4, f"zero word {k} outside a view of {nbytes} bytes"
        start = 4 * k if k >= 0 else nbytes + 4 * k
        view[start:start + 4] = 0

    def check(what=""):
        front, back = base[:off], base[off + nbytes:]
        assert back.numel() >= GUARD_BYTES and front.numel() >= GUARD_BYTES
        bad = torch.nonzero(front != guard)
        assert bad.numel() == 0, (f"{what}: {bad.numel()} guard bytes in FRONT of the {nbytes}-byte buffer were written, first at offset "
                                  f"{int(bad[0]) - off} (now {int(front[int(bad[0])]):#04x})")
        bad = torch.nonzero(back != guard)
        assert bad.numel() == 0, (f"{what}: {bad.numel()} guard bytes BEHIND the {nbytes}-byte buffer were written, first at offset "
                                  f"{nbytes + int(bad[0])} (now {int(back[int(bad[0])]):#04x})")

    def restored(what=""):
        for k in words:
            start = 4 * k if k >= 0 else nbytes + 4 * k
            got = view[start:start + 4].cpu().numpy()
            assert not got.any(), f"{what}: word {k} of the buffer is {got.view(np.uint32)[0]:#010x} after the call, not 0"

    check.ptr = base.data_ptr() + off
    check.restored = restored
    check.base = base
    return view, check


def guarded_out(shape, dtype, device, fill=OUT_FILL, align=256):
    """-> (tensor, check): an output tensor of `shape` / `dtype` whose bytes are all `fill`, laid over a guarded view -- the guard
    bytes behind it are the sentinel rows past n, those in front catch a negative index"""
    shape = tuple(int(s) for s in (shape if isinstance(shape, (tuple, list)) else (shape,)))
    item = torch.empty((), dtype=dtype).element_size()
    n = int(np.prod(shape, dtype=np.int64)) if shape else 1
    view, check = guarded(n * item, fill, device, align=max(align, item))
    return view.view(dtype).view(shape), check

