"""A view without Gaussians has nothing to differentiate and need not have chunks, scratch or gradient outputs: every door into the
rasterizer backward (csplat_backward, csplat_backward_depth with and without a depth gradient, csplat_backward_views with one view, colour
and depth path) returns 0 for P = 0 before it looks at any of the view's pointers.  No GPU: nothing is launched, so NULL pointers are safe."""
import ctypes as C

import pytest

from csplat import native as n

W, H = 33, 17


def _flat_args(depth_arg):
    """the flat entries' argument list with P = 0 and every pointer NULL (depth_arg: [] or [dL_ddepth] in front of the scratch)"""
    head = [None, 0, 3, 16, 0, None, W, H, None, None, None, None, 1.0, None, None, None, None, None, 0.5, 0.5, None, None, None, None, None, None]
    return head + depth_arg + [None] * 10


@pytest.mark.parametrize("flags", [0, 256])
def test_a_view_without_gaussians_or_chunks_returns_0_through_every_entry(flags):
    ddepth = (C.c_float * (W * H))()       # (never read: a view without Gaussians launches nothing)
    old = int(n.lib.csplat_debug_flags_query())
    try:
        n.lib.csplat_debug_flags(flags)
        assert n.lib.csplat_backward(*_flat_args([])) == 0, n.lib.csplat_last_error()
        assert n.lib.csplat_backward_depth(*_flat_args([None])) == 0, n.lib.csplat_last_error()
        assert n.lib.csplat_backward_depth(*_flat_args([C.cast(ddepth, C.c_void_p)])) == 0, n.lib.csplat_last_error()
        for depth in (None, C.cast(ddepth, C.c_void_p)):
            w = n.CsplatView()
            w.D, w.M, w.W, w.H = 3, 16, W, H
            w.scale_modifier, w.tanfovx, w.tanfovy = 1.0, 0.5, 0.5
            w.dL_ddepth = depth
            assert n.lib.csplat_backward_views(1, C.addressof(w), None) == 0, n.lib.csplat_last_error()
    finally:
        n.lib.csplat_debug_flags(old)
