"""tests/scratch_guard.py on CPU tensors, and the coverage of tests/test_scratch_contracts_gpu.py: every size query include/csplat.h
declares is either run there under hostile scratch contents or excluded for one of the reasons fixed below.  A size query added later
fails here until someone decides about it."""
import os
import re

import numpy as np
import pytest

import util
from scratch_guard import FILLS, GUARD_BYTES, guarded, guarded_out

torch = pytest.importorskip("torch")
CPU = torch.device("cpu")


# ================================================================================================ the helper
@pytest.mark.parametrize("fill", FILLS)
@pytest.mark.parametrize("nbytes,align", [(0, 256), (1, 256), (4, 16), (1000, 256), (4096, 512), (70_001, 64)])
def test_view_has_the_requested_length_alignment_and_fill(nbytes, align, fill):
    view, check = guarded(nbytes, fill, CPU, align=align)
    assert view.dtype == torch.uint8 and view.shape == (nbytes,) and view.is_contiguous()
    assert check.ptr % align == 0 and (nbytes == 0 or view.data_ptr() == check.ptr)
    assert bool((view == fill).all())
    base = check.base
    off = check.ptr - base.data_ptr()
    assert off >= GUARD_BYTES and base.numel() - off - nbytes >= GUARD_BYTES            # 4096 guard bytes on either side
    guard = int(base[0])
    assert guard != fill and bool((base[:off] == guard).all()) and bool((base[off + nbytes:] == guard).all())
    check("untouched")
    check.restored("no zero words")


def test_fills_decode_as_the_hostile_values_they_are_meant_to_be():
    assert FILLS == (0x00, 0xFF, 0x7F)
    ff, _ = guarded(8, 0xFF, CPU)
    assert bool(torch.isnan(ff.view(torch.float32)).all()) and ff.view(torch.int32).tolist() == [-1, -1]
    assert ff.numpy().view(np.uint32).tolist() == [0xFFFFFFFF] * 2 and int(ff.numpy().view(np.uint64)[0]) == 2 ** 64 - 1
    sf, _ = guarded(8, 0x7F, CPU)
    f = sf.view(torch.float32)
    assert bool(torch.isfinite(f).all()) and float(f[0]) > 1e38 and int(sf.view(torch.int32)[0]) == 0x7F7F7F7F > 2 ** 30
    zero, _ = guarded(8, 0x00, CPU)
    assert zero.view(torch.float32).tolist() == [0.0, 0.0]


@pytest.mark.parametrize("nbytes", [0, 12, 1000])
def test_a_byte_written_outside_the_view_fails_the_check_and_names_the_offset(nbytes):
    for where in (-1, nbytes, nbytes + GUARD_BYTES - 1, -GUARD_BYTES):
        view, check = guarded(nbytes, 0xFF, CPU)
        base, off = check.base, check.ptr - check.base.data_ptr()
        base[off + where] = 0x01
        with pytest.raises(AssertionError, match=rf"first at offset {where} "):
            check("damaged")
    view, check = guarded(nbytes, 0xFF, CPU)
    if nbytes:
        view[0], view[nbytes - 1] = 3, 4                         # writes INSIDE the view are the entry's business
    check("inside")


def test_zero_words_are_cleared_and_their_restoration_is_checked():
    view, check = guarded(64, 0xFF, CPU, zero_words=[0, -1, 5])
    w = view.view(torch.int32)
    assert w[0] == 0 and w[15] == 0 and w[5] == 0 and int((w == -1).sum()) == 13
    check.restored("cleared")
    w[5] = 1                                                     # (a ticket the call did not put back)
    with pytest.raises(AssertionError, match="word 5 of the buffer is 0x00000001"):
        check.restored("left at one")
    w[5] = 0
    w[15] = -5
    with pytest.raises(AssertionError, match="word -1 of the buffer"):
        check.restored("last word")
    check("the guards do not care")
    with pytest.raises(AssertionError):
        guarded(8, 0xFF, CPU, zero_words=[2])                    # a word outside the view


def test_guarded_outputs_are_typed_views_with_guards_behind_them():
    for shape, dtype, item in (((5, 3), torch.float32, 4), (7, torch.int32, 4), ((2, 3, 4), torch.int8, 1), (0, torch.int32, 4), ((3,), torch.float64, 8)):
        t, check = guarded_out(shape, dtype, CPU)
        assert t.dtype == dtype and tuple(t.shape) == (tuple(shape) if isinstance(shape, tuple) else (shape,)) and t.is_contiguous()
        assert check.ptr % 256 == 0 and (t.numel() == 0 or t.data_ptr() == check.ptr)
        t.fill_(1)
        check("filled")
        check.base[check.ptr - check.base.data_ptr() + t.numel() * item] = 0      # one element past the end
        with pytest.raises(AssertionError, match=f"first at offset {t.numel() * item} "):
            check("past the end")


# ================================================================================================ coverage of the header
ALLOWED_EXCLUSIONS = {
    "csplat_geom_bytes", "csplat_image_bytes", "csplat_binning_bytes", "csplat_temp_bytes",      # the forward chunks
    "csplat_backward_camera_scratch_bytes", "csplat_backward_feature_scratch_bytes",             # batched view records only
    "csplat_mesh_rest_bytes", "csplat_gnn_node_update_image_bytes", "csplat_gnn_edge_mlp3_image_bytes",      # persistent data
    "csplat_sort_pairs_temp_bytes", "csplat_scan_u32_temp_bytes",                                # tests/test_sort_scan_gpu.py
}


def _header():
    return open(os.path.join(util.ROOT, "include", "csplat.h")).read()


def declared_size_queries(header):
    return re.findall(r"^size_t (csplat_\w+_bytes)\(", header, re.M)


def uncovered(queries, table, excluded):
    return [q for q in queries if q not in table and q not in excluded]


def test_every_size_query_of_the_header_is_tested_or_excluded_with_a_reason():
    import test_scratch_contracts_gpu as G
    queries = declared_size_queries(_header())
    assert len(queries) == len(set(queries)) >= 33
    assert uncovered(queries, G.TABLE, G.EXCLUDED) == []
    assert set(G.EXCLUDED) <= ALLOWED_EXCLUSIONS and all(isinstance(r, str) and r for r in G.EXCLUDED.values())
    assert not set(G.TABLE) & set(G.EXCLUDED)
    assert set(G.TABLE) | set(G.EXCLUDED) == set(queries), "a name that the header does not declare"
    for names in list(G.TABLE.values()) + list(G.SIZED_IN_PYTHON.values()):
        assert names and all(callable(getattr(G, t, None)) and t.startswith("test_") for t in names), names
    # the detector detects: without one row the query behind it is reported
    for q in G.TABLE:
        assert uncovered(queries, {k: v for k, v in G.TABLE.items() if k != q}, G.EXCLUDED) == [q]


def test_the_gpu_file_is_marked_gpu_and_the_native_table_knows_every_query():
    import test_scratch_contracts_gpu as G
    from csplat import native
    assert getattr(G.pytestmark, "name", None) == "gpu"
    for q in declared_size_queries(_header()):
        assert q in native.EXPORTS and native.EXPORTS[q][0] is native._sz, q


def test_the_two_sizes_computed_in_python_follow_the_header():
    """csplat/gaussians.py and meshnet/rollout.py size their scratch by the words of the header, which exports no query for them"""
    from csplat.gaussians import corner_scratch_floats
    from meshnet.rollout import refine_scratch_floats
    header = _header()
    assert "corner_scratch (T*P*9 floats" in header and corner_scratch_floats(3, 7) == 3 * 7 * 9
    assert "scratch = 9 N" in header and refine_scratch_floats(11) == 99
