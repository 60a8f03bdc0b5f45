"""The host side of the rasterizer forward (csplat_raster.hip: tickets, the batched second phase, deferred / settle), through the C entries
alone (ctypes, csplat.native): what a call leaves behind when it FAILS (none of the 64 tickets), and the bookkeeping of a call whose one
host read is deferred -- pending or not, which array settles it, what happens without a free pending slot, and a settle that finds the
counts over the capacities and launches the phase again.  Every error here is a refusal on the host (arguments, allocator).
Shape: P = 300 Gaussians, a 64 x 48 image (12 tiles), SH degree 3 -- the case of test_two_phase_forward_tickets_and_errors."""
import ctypes as C

import pytest

import util

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

NO_SPECULATION = 1024
CHUNK_BINNING = 1
MAX_TICKETS, MAX_PENDING = 64, 8


class _Alloc:
    """csplat_alloc_fn: torch-owned chunks, all kept alive; `requests` lists (view, chunk kind); `refuse`: the kind answered with NULL"""

    def __init__(self, refuse=None):
        from csplat import native as n
        self.kept, self.requests, self.refuse = [], [], refuse
        self.cb = n.ALLOC_FN(self._alloc)

    def _alloc(self, ctx, chunk, nbytes):
        self.requests.append((int(ctx or 0), int(chunk)))
        if chunk == self.refuse:
            return None
        self.kept.append(torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device="cuda"))
        return self.kept[-1].data_ptr()


class _Scene:
    """the device tensors of one case, shared by every view made from it"""

    def __init__(self, P=300, W=64, H=48, scale_mul=2.0, **over):
        self.P, self.W, self.H = P, W, H
        self.case = util.make_case(P=P, W=W, H=H, seed=2, scale_mul=scale_mul, **over)
        self.inp = util.gpu_inputs(self.case, requires_grad=False)
        self.st = util.gpu_settings(self.case)

    def views(self, V, P_of=None):
        """(array of V csplat_view on the current stream, [(colour, depth, radii)]); P_of[i]: view i takes the first P_of[i] Gaussians"""
        from csplat import native as n
        inp, st, W, H = self.inp, self.st, self.W, self.H
        arr, outs = (n.CsplatView * V)(), []
        for i in range(V):
            w, Pi = arr[i], (P_of[i] if P_of else self.P)
            outs.append((torch.zeros(3, H, W, device="cuda"), torch.zeros(1, H, W, device="cuda"),
                         torch.zeros(Pi, dtype=torch.int32, device="cuda")))
            w.stream = _stream()
            w.P, w.D, w.M, w.W, w.H = Pi, 3, 16, W, H
            w.scale_modifier, w.tanfovx, w.tanfovy = 1.0, float(st.tanfovx), float(st.tanfovy)
            w.bg, w.means3D, w.shs, w.opacities = n.ptr(st.bg), n.ptr(inp["means3D"]), n.ptr(inp["shs"]), n.ptr(inp["opacities"])
            w.scales, w.rotations = n.ptr(inp["scales"]), n.ptr(inp["rotations"])
            w.view, w.proj, w.campos = n.ptr(st.viewmatrix), n.ptr(st.projmatrix), n.ptr(st.campos)
            w.alloc_ctx = i
            w.out_color, w.out_depth, w.radii = (n.ptr(t) for t in outs[-1])
        return arr, outs


def _stream():
    from csplat import native as n
    return n.stream_handle(torch.device("cuda"))


def _err():
    from csplat import native as n
    return n.lib.csplat_last_error().decode()


def _forward_views(arr, alloc):
    from csplat import native as n
    return n.lib.csplat_forward_views(len(arr), C.cast(arr, C.c_void_p), alloc.cb, _stream())


def _deferred(arr, alloc):
    from csplat import native as n
    pending = C.c_int(-1)
    rc = n.lib.csplat_forward_views_deferred(len(arr), C.cast(arr, C.c_void_p), alloc.cb, _stream(), C.byref(pending))
    return rc, pending.value


def _settle(arr, V=None):
    from csplat import native as n
    relaunched = C.c_int(-1)
    rc = n.lib.csplat_forward_views_settle(len(arr) if V is None else V, C.cast(arr, C.c_void_p), _stream(), C.byref(relaunched))
    return rc, relaunched.value


class _flags:
    def __init__(self, flags):
        self.flags = flags

    def __enter__(self):
        from csplat import native as n
        self.old = int(n.lib.csplat_debug_flags_query())
        n.lib.csplat_debug_flags(self.flags)

    def __exit__(self, *a):
        from csplat import native as n
        n.lib.csplat_debug_flags(self.old)


def _without_speculation(scene, V=1):
    """csplat_forward_views of V views, every call waiting for its own counts: the images a speculative call has to equal"""
    arr, outs = scene.views(V)
    alloc = _Alloc()
    with _flags(NO_SPECULATION):
        assert _forward_views(arr, alloc) == 0, _err()
    torch.cuda.synchronize()
    return arr, outs


def _forget():
    """The library sizes a speculative launch from its last eight batched calls (a ring, entries by shape): after eight calls of
    another shape that each wait for their counts it knows nothing of the shapes of this file, whatever ran before in the process"""
    other = _Scene(P=40, W=16, H=16)
    calls = [(other.views(1), _Alloc()) for _ in range(8)]      # (arrays, outputs and chunks all live until the synchronize)
    with _flags(NO_SPECULATION):
        for (arr, _outs), alloc in calls:
            assert _forward_views(arr, alloc) == 0, _err()
    torch.cuda.synchronize()


def _equal(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("how", ["view_refused_in_prepare", "faith_views_do_not_qualify", "allocator_refuses_binning", "begin_refuses_antialias"])
def test_failing_calls_leak_no_ticket(how):
    """40 failing calls of two or three views (70 of the flat begin) would hold more than the 64 tickets if they kept any: afterwards 64
    forwards can still be begun before the first is finished"""
    from csplat import native as n
    scene = _Scene()
    inp, st, P, W, H = scene.inp, scene.st, scene.P, scene.W, scene.H
    keep = []

    def begin(prefiltered=0):
        alloc, radii, tk = _Alloc(), torch.empty(P, dtype=torch.int32, device="cuda"), C.c_int(-1)
        rc = n.lib.csplat_forward_begin(
            _stream(), P, 3, 16, n.ptr(st.bg), W, H, n.ptr(inp["means3D"]), n.ptr(inp["shs"]), None, n.ptr(inp["opacities"]),
            n.ptr(inp["scales"]), 1.0, n.ptr(inp["rotations"]), None, n.ptr(st.viewmatrix), n.ptr(st.projmatrix), n.ptr(st.campos),
            float(st.tanfovx), float(st.tanfovy), prefiltered, alloc.cb, None, n.ptr(radii), C.byref(tk))
        keep.append((alloc, radii))
        return rc, tk.value

    def finish(tk):
        color, depth = torch.empty(3, H, W, device="cuda"), torch.empty(1, H, W, device="cuda")
        R, g, b, i = C.c_int(0), C.c_void_p(), C.c_void_p(), C.c_void_p()
        rc = n.lib.csplat_forward_finish(tk, n.ptr(color), n.ptr(depth), C.byref(R), C.byref(g), C.byref(b), C.byref(i))
        return rc, color, R.value

    for _ in range(70 if how == "begin_refuses_antialias" else 40):
        if how == "view_refused_in_prepare":
            arr, outs = scene.views(3)
            arr[2].shs = None                       # (neither shs nor colors_precomp)
            keep.append((outs, _Alloc()))
            assert _forward_views(arr, keep[-1][1]) != 0 and "provide exactly one of shs / colors_precomp" in _err()
        elif how == "faith_views_do_not_qualify":
            arr, outs = scene.views(2, P_of=[P, P - 1])
            caps, valid = (C.c_uint32 * 3)(4096, 512, 12), torch.zeros(1, dtype=torch.int32, device="cuda")
            keep.append((outs, _Alloc(), valid))
            rc = n.lib.csplat_forward_views_faith(2, C.cast(arr, C.c_void_p), keep[-1][1].cb, _stream(), C.cast(caps, C.c_void_p), n.ptr(valid))
            assert rc != 0 and "do not qualify" in _err()
        elif how == "allocator_refuses_binning":
            arr, outs = scene.views(3)
            keep.append((outs, _Alloc(refuse=CHUNK_BINNING)))
            assert _forward_views(arr, keep[-1][1]) != 0 and "allocator returned NULL" in _err()
            assert (0, CHUNK_BINNING) in keep[-1][1].requests
        else:
            rc, _tk = begin(prefiltered=2)          # CSPLAT_ANTIALIAS
            assert rc != 0 and "CSPLAT_ANTIALIAS needs a csplat_view entry point" in _err()
    tickets = []
    for _ in range(MAX_TICKETS):
        rc, tk = begin()
        assert rc == 0, _err()
        tickets.append(tk)
    assert len(set(tickets)) == MAX_TICKETS
    ref = None
    for tk in tickets:
        rc, color, R = finish(tk)
        assert rc == 0 and R > 0, _err()
        ref = color if ref is None else ref
        assert torch.equal(color, ref)
    torch.cuda.synchronize()                        # (the chunks of the refused calls lived until here)
    assert bool(ref.std() > 0)


def test_deferred_and_settle_bookkeeping():
    scene = _Scene()
    V = 2
    want = _without_speculation(scene, V)[1]
    _forget()
    allocs = [_Alloc() for _ in range(2)]
    first, outs1 = scene.views(V)
    rc, pending = _deferred(first, allocs[0])       # nothing known of the shape: the call waits for its counts and is complete
    assert rc == 0 and pending == 0, _err()
    assert all(0 < w.num_rendered == w.layout_rendered for w in first)
    arr, outs = scene.views(V)
    rc, pending = _deferred(arr, allocs[1])
    assert rc == 0 and pending == 1, _err()
    assert all(w.num_rendered == -1 and w.layout_rendered > 0 for w in arr)
    other, _outs = scene.views(V)
    for rc, _rl in (_settle(other), _settle(arr, V=1)):
        assert rc != 0 and "no pending call" in _err()
    rc, relaunched = _settle(arr)
    assert rc == 0 and relaunched == 0, _err()
    assert all(0 < w.num_rendered <= w.layout_rendered for w in arr)
    assert [w.num_rendered for w in arr] == [w.num_rendered for w in first]
    rc, _rl = _settle(arr)
    assert rc != 0 and "no pending call" in _err()
    torch.cuda.synchronize()
    for got in (outs1, outs):
        assert all(_equal(g, w) for g, w in zip(got, want))
    assert bool(want[0][0].std() > 0) and bool((want[0][2] > 0).any())


def test_more_pending_calls_than_slots():
    """eight pending slots: the ninth deferred call reads its counts itself, and the eight settle in any order"""
    scene = _Scene()
    want = _without_speculation(scene)[1][0]        # (also the warm-up: the library now knows the shape's counts)
    calls = []
    for k in range(MAX_PENDING + 1):
        arr, outs = scene.views(1)
        alloc = _Alloc()
        rc, pending = _deferred(arr, alloc)
        assert rc == 0 and pending == (1 if k < MAX_PENDING else 0), (k, _err())
        calls.append((arr, outs, alloc))
    last = calls[-1][0][0]
    assert 0 < last.num_rendered <= last.layout_rendered
    for arr, _outs, _alloc in reversed(calls[:-1]):
        assert arr[0].num_rendered == -1
        rc, relaunched = _settle(arr)
        assert rc == 0 and relaunched == 0, _err()
        assert arr[0].num_rendered == last.num_rendered
    torch.cuda.synchronize()
    for _arr, outs, _alloc in calls:
        assert _equal(outs[0], want)


def test_settle_that_must_relaunch():
    """the lists of the warm-up are short (longest: 112 entries, capacity 112 + 112 / 4 + 64 = 204); with four times the scales the
    longest has 241: the speculative launch left the view untouched and settle repeats the phase with the exact counts"""
    small, big = _Scene(scale_mul=2.0, radius=1.5), _Scene(scale_mul=8.0, radius=1.5)
    want = _without_speculation(big)[1][0]
    _forget()
    _without_speculation(small)
    arr, outs = big.views(1)
    alloc = _Alloc()
    rc, pending = _deferred(arr, alloc)
    assert rc == 0 and pending == 1, _err()
    capacity, asked = arr[0].layout_rendered, alloc.requests.count((0, CHUNK_BINNING))
    assert asked == 1
    rc, relaunched = _settle(arr)
    assert rc == 0 and relaunched == 1, _err()
    assert 0 < arr[0].num_rendered == arr[0].layout_rendered != capacity
    assert alloc.requests.count((0, CHUNK_BINNING)) == asked + 1
    torch.cuda.synchronize()
    assert _equal(outs[0], want) and bool(want[0].std() > 0)
