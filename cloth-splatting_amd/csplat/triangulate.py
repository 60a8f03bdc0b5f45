"""Delaunay triangulation of a planar cloud on the device (include/csplat.h, "Delaunay triangulation": csplat_delaunay).

The reference leaves the device for this: scipy.spatial.Delaunay (Qhull) and a Python loop over simplices, once per trajectory and once per
closed-loop round (meshnet/data_utils.py:371-405).  Here the cloud stays where it is; one blocking read of five counters sizes the result.
The triangulation is a pure function of the coordinates and the index order: cocircular points -- a cloth at rest on a grid is nothing
else -- are resolved by the symbolic tie rule of the header, not by Qhull's joggle, and two runs give equal bits."""
import collections
import ctypes as C
import math

import torch

from . import native as _n

MAX_POINTS = 1 << 24
STATUS_STEPS, STATUS_LAYOUT = 1, 2

Triangulation = collections.namedtuple("Triangulation", ["faces", "edge_index", "n_skipped", "exact_decisions"])
Triangulation.__doc__ = """faces [3,M] int64: each column a face, lowest index first, counter-clockwise, the columns in lexicographic order;
edge_index [2,E] int64: each edge once, i < j, sorted by (i, j); n_skipped: points with a non-finite coordinate or the coordinates of a
lower-indexed point; exact_decisions: how many decisions of the walk the exact stage took"""


def checked_threshold(norm_threshold, what):
    """None, or the threshold as a float; a NaN or something that is no number is a ValueError"""
    if norm_threshold is None:
        return None
    try:
        thr = float(norm_threshold)
    except (TypeError, ValueError):
        raise ValueError(f"{what}: norm_threshold is a number or None, got {norm_threshold!r}") from None
    if math.isnan(thr):
        raise ValueError(f"{what}: norm_threshold is a number or None, got NaN")
    return thr


def temp_bytes(n):
    size = C.c_size_t(0)
    # (a size query that can refuse its argument, takes no stream: check(), not native.launch)
    _n.check(_n.lib.csplat_delaunay_temp_bytes(int(n), C.byref(size)), "csplat_delaunay_temp_bytes")
    return int(size.value)


def delaunay(points2d, norm_threshold=None):
    """points2d: float32 GPU tensor [N,2], N < 2^24 -> Triangulation.  With norm_threshold an edge of a face is dropped when its float32
    length sqrtf(du*du + dv*dv) > (float)norm_threshold and a face is kept when none of its three is dropped, the reference's filter;
    None keeps everything.  All points collinear or fewer than three usable: no faces, no error."""
    what = "delaunay"
    if not torch.is_tensor(points2d):
        raise ValueError(f"{what}: points2d is a tensor, got {type(points2d).__name__}")
    if points2d.dim() != 2 or points2d.shape[1] != 2:
        raise ValueError(f"{what}: points2d is [N, 2], got {tuple(points2d.shape)}")
    if points2d.dtype != torch.float32:
        raise ValueError(f"{what}: points2d is float32, got {points2d.dtype}")
    N = int(points2d.shape[0])
    if N >= MAX_POINTS:
        raise ValueError(f"{what}: N must stay below 2^24, got {N}")
    thr = checked_threshold(norm_threshold, what)
    _n.require_cuda(points2d)
    dev = points2d.device
    pts = points2d.detach().contiguous()
    if pts.data_ptr() % 8:
        pts = pts.clone()
    with _n.on_device(dev):
        faces = torch.empty(max(2 * N, 1), 3, dtype=torch.int32, device=dev)
        edges = torch.empty(max(3 * N, 1), 2, dtype=torch.int32, device=dev)
        counters = torch.empty(5, dtype=torch.int64, device=dev)
        temp = _n.temp(dev, temp_bytes(N))
        _n.launch("csplat_delaunay", dev, N, _n.ptr(pts), 0 if thr is None else 1, 0.0 if thr is None else thr, _n.ptr(faces), _n.ptr(edges),
                  _n.ptr(counters), _n.ptr(temp))
        return _result(faces, edges, counters)


def _result(faces, edges, counters):
    """the buffers csplat_delaunay wrote -> Triangulation; a non-zero status word is a CsplatError"""
    M, E, skipped, exact, status = counters.tolist()                           # the one blocking read
    if status:
        why = "a walk exceeded N steps" if status & STATUS_STEPS else "the counting and the writing walk disagree"
        raise _n.CsplatError(f"csplat_delaunay failed (status={status}): {why}")
    return Triangulation(faces[:M].t().to(torch.int64).contiguous(), edges[:E].t().to(torch.int64).contiguous(), int(skipped), int(exact))
