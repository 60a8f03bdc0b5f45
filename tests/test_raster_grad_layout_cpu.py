"""Where every gradient of a batched rasterizer backward lands (diff_gaussian_rasterization._GradLayout and the csplat_view array
_RasterizeGaussiansBatch._plan_backward fills from it): which views share a buffer and carry which CSPLAT_ACC_* bit, the offsets inside
the one allocation, the CSPLAT_K8_OUTPUTS_UNREAD and CSPLAT_SCRATCH_ZEROED bits, the returned (slot, offset, shape) triples.  Overlapping
offsets, a missing accumulate bit or a wrong "unread" bit are silent on the GPU; here they are assertions.  No GPU: the layout is pure, and
the planner runs on CPU tensors with a zeroed csplat_view array.
tests/golden/raster_grad_layout.json was recorded once from the planner as it was before the layout became an object of its own (one loop
that decided, laid out, claimed sinks and filled the array), never from the code under test -- tests/golden/make_raster_grad_layout.py, which
takes the cases from this module.  Both modes are pinned: "256" is the bit-reproducible mode (csplat_debug_flags bit 8: per-call scratch inside
the allocation); "0" is the default mode, where the persistent zeroed records (_acc_scratch) lie outside the allocation -- on the CPU, in the
recording and here alike, `_acc_scratch` is replaced by a stub that returns a 256-byte CPU buffer and True (the real one keys on a HIP stream)."""
import functools
import itertools
import json
from math import prod
import os
import types

import pytest
import torch

import util
import diff_gaussian_rasterization as dgr
from csplat import native

NIN = 8
SLOT = {"means3D": 0, "means2D": 1, "sh": 2, "colors_precomp": 3, "opacities": 4, "scales": 5, "rotations": 6, "cov3Ds_precomp": 7}
SHAPES = {0: lambda P, M: (P, 3), 1: lambda P, M: (P, 3), 2: lambda P, M: (P, M, 3), 3: lambda P, M: (P, 3), 4: lambda P, M: (P, 1),
          5: lambda P, M: (P, 3), 6: lambda P, M: (P, 4), 7: lambda P, M: (P, 6)}
FIELDS = ("dL_dconic", "dL_dmean3D", "dL_dmean2D", "dL_dsh", "dL_dcolor", "dL_dopacity", "dL_dscale", "dL_drot", "dL_dcov3D")
ACC = {0: 4, 2: 16, 3: 2, 4: 1, 5: 32, 6: 64, 7: 8}        # csplat.h: CSPLAT_ACC_* by slot (means2D: formed from one view's K7 records, never shared)
TEMP = (3, 7)                                              # dL_dcolor, dL_dcov3D: K8's temporaries, returned only to a precomputed input
ZEROED, UNREAD, BIT_REPRODUCIBLE = 256, 512, 256
CPU = torch.device("cpu")


class Case(types.SimpleNamespace):
    """V views of P Gaussians with M SH coefficients; share: "all" = every view gets the same tensor objects, "none" = its own, "mixed" =
    view i its own for slot s where (i + s) % 3 == 0 and the shared object otherwise, "otherP" = the last view its own, of another P;
    precomp: which of colors_precomp / cov3Ds_precomp replace sh / (scales, rotations); active: the views whose images got a gradient
    (None: all); sh_off: the SH storage starts that many floats off a 16-byte boundary"""

    @property
    def name(self):
        return "V%d_P%d_M%d_%s%s%s%s" % (self.V, self.P, self.M, self.share, "_" + "+".join(self.precomp) if self.precomp else "",
                                         "" if self.active is None else "_act" + "".join(map(str, self.active)), "_shoff%d" % self.sh_off if self.sh_off else "")


def case(V, P, M, share, precomp=(), active=None, sh_off=0):
    return Case(V=V, P=P, M=M, share=share, precomp=tuple(precomp), active=active, sh_off=sh_off)


def pinned_cases():
    for P, M, V, share in itertools.product((1, 33), (1, 4, 16), (1, 2, 3, 9), ("all", "none")):
        yield case(V, P, M, share)
    for share in ("mixed", "otherP"):
        yield case(3, 33, 16, share)
        yield case(9, 33, 4, share)
    for share, precomp in itertools.product(("all", "none"), (("color",), ("cov",), ("color", "cov"))):
        yield case(2, 33, 16, share, precomp)
    for share, active in itertools.product(("all", "none"), ([0, 2], [1, 2])):
        yield case(3, 33, 16, share, active=active)
    yield case(2, 33, 16, "all", sh_off=1)
    yield case(3, 33, 16, "mixed", sh_off=1)


def all_cases():
    for P, M, V, share, precomp in itertools.product((1, 33), (1, 4, 16), (1, 2, 3, 9), ("all", "none", "mixed", "otherP"),
                                                     ((), ("color",), ("cov",), ("color", "cov"))):
        for active in (None, [0, 2], [1, 2]) if V == 3 else (None,):
            for sh_off in (0, 1) if M == 16 and "color" not in precomp else (0,):
                yield case(V, P, M, share, precomp, active, sh_off)


def inputs_of(c):
    """per view (P, its NIN input tensors in slot order, None where absent): CPU tensors of the real shapes"""
    def make(P):
        sh = None
        if "color" not in c.precomp:
            flat = torch.zeros(P * c.M * 3 + 4)
            lead = (-flat.data_ptr() // 4) % 4 + c.sh_off       # floats up to the next 16-byte boundary, + sh_off
            sh = flat[lead:lead + P * c.M * 3].view(P, c.M, 3)
            assert sh.data_ptr() % 16 == 4 * c.sh_off
        cov = "cov" in c.precomp
        return [torch.zeros(P, 3), torch.zeros(P, 3), sh, torch.zeros(P, 3) if sh is None else None, torch.zeros(P, 1),
                None if cov else torch.zeros(P, 3), None if cov else torch.zeros(P, 4), torch.zeros(P, 6) if cov else None]
    shared = make(c.P)
    views = []
    for i in range(c.V):
        P = c.P
        if c.share == "all":
            g = shared
        elif c.share == "mixed":
            own = make(P)
            g = [own[s] if (i + s) % 3 == 0 else shared[s] for s in range(NIN)]
        elif c.share == "otherP" and i < max(c.V - 1, 1):
            g = shared
        else:
            P = c.P if c.share == "none" else 34 - c.P
            g = make(P)
        views.append((P, list(g)))
    return views


def first_of(groups):
    return [[next(j for j in range(i + 1) if groups[j][k] is groups[i][k]) for k in range(NIN)] for i in range(len(groups))]


def rendered(i):
    return 300 + 17 * i       # what each view's binning chunk was laid out for (sizes the per-call scratch of the bit-reproducible mode)


def view_records(c):
    ins = inputs_of(c)
    M = lambda g: int(g[2].shape[1]) if g[2] is not None else 0      # noqa: E731
    return [types.SimpleNamespace(P=P, M=M(g), layout_rendered=rendered(i), dev=CPU, present=[t is not None for t in g],
                                  staged=g[2] is not None and M(g) == 16 and g[2].data_ptr() % 16 == 0)
            for i, (P, g) in enumerate(ins)], [g for _P, g in ins]


def active_of(c):
    return list(range(c.V)) if c.active is None else list(c.active)


def acc_stub(_dev, _P, _slot):
    return torch.zeros(256, dtype=torch.uint8), True


class flags:
    """csplat_debug_flags for the scope; in the default mode `_acc_scratch` is the CPU stub"""

    def __init__(self, mode):
        self.mode = int(mode)

    def __enter__(self):
        self.old, self.real = int(native.lib.csplat_debug_flags_query()), dgr._acc_scratch
        native.lib.csplat_debug_flags(self.mode)
        if not self.mode:
            dgr._acc_scratch = acc_stub

    def __exit__(self, *exc):
        native.lib.csplat_debug_flags(self.old)
        dgr._acc_scratch = self.real


def read_array(sub, n, big, out):
    """the materialised plan as the golden file records it: offsets in floats from the allocation's start (None: NULL; scratch None: outside
    the allocation)"""
    base, end = big.data_ptr(), big.data_ptr() + 4 * big.numel()

    def off(p):
        if not p:
            return None
        assert base <= p < end and (p - base) % 4 == 0, "a pointer outside the allocation"
        return (p - base) // 4
    views, ret = [], []
    for a in range(n):
        w = sub[a]
        views.append([int(w.accmask), off(w.scratch) if not int(w.accmask) & ZEROED else None] + [off(getattr(w, f)) for f in FIELDS])
    for g in out:
        if g is not None:
            ret.append([[s, off(t.data_ptr()), list(t.shape)] for s, t in enumerate(g) if t is not None])
    return {"total": int(big.numel()), "views": views, "ret": ret}


@functools.lru_cache(maxsize=None)
def expected():
    with open(os.path.join(util.GOLDEN, "raster_grad_layout.json")) as f:
        return json.load(f)


# ---- the code under test, through its two doors
def specs_of(c, mode):
    """the plain values _GradLayout takes, gathered the way _plan_backward gathers them"""
    views, groups = view_records(c)
    fo = first_of(groups)
    specs = []
    for i, (v, g) in enumerate(zip(views, groups)):
        scratch = int(native.lib.csplat_backward_scratch_bytes(v.P, v.layout_rendered)) // 4 + 64 if mode else None
        specs.append((v.P, v.M, v.present, fo[i], v.staged, scratch))
    return specs


def pure(c, mode, sunk=()):
    with flags(mode):
        specs = specs_of(c, mode)
    asked = []          # the (view, slot, numel) the layout asks a sink for, in its order
    lay = dgr._GradLayout(specs, active_of(c), lambda i, slot, numel: asked.append((i, slot, numel)) or (i, slot) in sunk)
    return lay, specs, asked


def as_recorded(lay):
    views = [[lay.mask[a], lay.scratch[a]] + list(lay.fields[a]) for a in range(len(lay.active))]
    ret = [[[s, o, list(shape)] for s, o, shape in sorted(lay.ret[a])] for a in range(len(lay.active))]
    return {"total": max(lay.total, 64), "views": views, "ret": ret}


def materialised(c, mode, sinks=False):
    views, groups = view_records(c)
    arr = (native.CsplatView * c.V)()
    with flags(mode):
        return dgr._RasterizeGaussiansBatch._plan_backward(views, arr, first_of(groups), active_of(c), groups if sinks else None), groups


def test_the_pinned_cases_cover_what_the_table_is_for():
    names = [c.name for c in pinned_cases()]
    EXPECTED = expected()
    assert len(set(names)) == len(names) and set(EXPECTED) == {"0", "256"}
    for mode in EXPECTED:
        assert sorted(EXPECTED[mode]) == sorted(names)
    assert EXPECTED["256"]["V1_P33_M16_all"]["total"] == 46656 and EXPECTED["256"]["V1_P33_M16_all"]["views"][0][0] == UNREAD
    # the back-to-back rows: offsets that are no multiple of 4 floats
    assert any(o % 4 for v in EXPECTED["0"]["V2_P33_M16_none"]["views"] for o in v[2:] if o is not None)


@pytest.mark.parametrize("mode", (0, BIT_REPRODUCIBLE))
def test_pure_layout_reproduces_the_recorded_plans(mode):
    for c in pinned_cases():
        lay, _specs, _asked = pure(c, mode)
        assert as_recorded(lay) == expected()[str(mode)][c.name], (mode, c.name)


@pytest.mark.parametrize("mode", (0, BIT_REPRODUCIBLE))
def test_materialised_view_array_reproduces_the_recorded_plans(mode):
    for c in pinned_cases():
        plan, _groups = materialised(c, mode)
        assert plan.active == active_of(c) and plan.sinks == [] and len(plan.acc) == len(plan.active), (mode, c.name)
        assert all((t is None) == bool(mode) for t in plan.acc), (mode, c.name)
        assert read_array(plan.sub, len(plan.active), plan.big, plan.out) == expected()[str(mode)][c.name], (mode, c.name)


@pytest.mark.parametrize("mode", (0, BIT_REPRODUCIBLE))
def test_layout_properties_over_the_full_product(mode):
    ncases = 0
    for c in all_cases():
        lay, specs, asked = pure(c, mode)
        active = active_of(c)
        ncases += 1
        where = {}          # offset -> (extent, the (view, slot) or name that owns it)
        packed = set()      # offsets inside a back-to-back block
        for slot in (0, 6):     # means3D / rotations of distinct, equally sized, present inputs: one block, view after view
            if len(active) > 1 and all(specs[i][3][slot] == i and specs[i][2][slot] for i in active) and len({specs[i][0] for i in active}) == 1:
                offs, size = [lay.fields[a][1 + slot] for a in range(len(active))], prod(SHAPES[slot](specs[active[0]][0], 0))
                assert offs[0] % 64 == 0 and offs == [offs[0] + a * size for a in range(len(active))], (c.name, slot)
                packed.update(offs)
        for a, i in enumerate(active):
            P, M, present, fo, staged, scratch = specs[i]
            mask, f = lay.mask[a], lay.fields[a]
            assert (lay.scratch[a] is None) == (scratch is None) == bool(mask & ZEROED), c.name
            own = [("scratch", lay.scratch[a], scratch)] if scratch is not None else []
            own.append(("conic", f[0], 4 * P))
            returned = {s: (o, shape) for s, o, shape in lay.ret[a]}
            for slot in range(NIN):
                o, numel = f[1 + slot], prod(SHAPES[slot](P, M))
                j = fo[slot]
                shares = slot in ACC and bool(mask & ACC[slot])
                if not present[slot] and slot not in TEMP:
                    assert o is None and lay.owner[a][slot] is None and slot not in returned and not shares, (c.name, i, slot)
                    continue
                assert o is not None, (c.name, i, slot)
                # two views point at one buffer exactly when the later one carries the row's bit and the owner is earlier in `active`
                expect_share = slot in ACC and present[slot] and j != i and j in active and (slot != 2 or staged)
                assert shares == expect_share, (c.name, i, slot)
                if shares:
                    assert active.index(j) < a and o == lay.fields[active.index(j)][1 + slot] and slot not in returned, (c.name, i, slot)
                    assert lay.owner[a][slot] == j, (c.name, i, slot)
                else:
                    own.append(((i, slot), o, numel))
                    assert lay.owner[a][slot] == i, (c.name, i, slot)
                    assert (slot in returned) == present[slot], (c.name, i, slot)      # (temp rows: allocated always, returned when present)
                if slot in returned:
                    assert returned[slot] == (o, SHAPES[slot](P, M)), (c.name, i, slot)
                if slot == 2 and shares:
                    assert staged, (c.name, i)
            assert bool(mask & UNREAD) == (not any(present[s] for s in TEMP)), (c.name, i)
            assert mask & ~(ZEROED | UNREAD | sum(ACC.values())) == 0, (c.name, i)
            for what, o, numel in own:
                assert o % 64 == 0 or o in packed, (c.name, what, o)
                assert o not in where, (c.name, what, "two buffers at one offset")
                where[o] = (numel, what)
        at = sorted(where)
        for o, nxt in zip(at, at[1:] + [lay.total]):
            assert o + where[o][0] <= nxt, (c.name, where[o][1], "overlaps", where.get(nxt))
        assert lay.total % 64 == 0, c.name
        # the order the sinks are asked for: views in `active` order, K8's rows in table order, owners only, never a back-to-back row
        want = [(i, s) for i in active for s in (0, 2, 3, 4, 5, 6, 7)
                if specs[i][2][s] and lay.owner[active.index(i)][s] == i and lay.fields[active.index(i)][1 + s] not in packed]
        assert [(i, s) for i, s, _n in asked] == want and all(n == prod(SHAPES[s](specs[i][0], specs[i][1])) for i, s, n in asked), c.name
    assert ncases > 500


def test_a_claimed_sink_takes_the_field_and_a_second_plan_gets_fresh_memory():
    import weakref
    c = case(2, 33, 16, "all")
    views, groups = view_records(c)
    del views
    flat = torch.zeros(64 + 33 * 48 + 33 * 3)
    sh, means = groups[0][2], groups[0][0]
    try:
        # what csplat.dist.FlatGrads.bind registers per parameter: (weak reference, flat buffer, offset, shape, [claimed]) -- by hand,
        # because bind() registers sinks for a flat buffer on the GPU only (`if self.flat.is_cuda`)
        native.GRAD_SINK[id(sh)] = (weakref.ref(sh), flat, 64, (33, 16, 3), [False])
        native.GRAD_SINK[id(means)] = (weakref.ref(means), flat, 64 + 33 * 48, (33, 3), [False])

        def plan_with(groups_):
            views_, _g = view_records(c)
            with flags(0):
                return dgr._RasterizeGaussiansBatch._plan_backward(views_, (native.CsplatView * 2)(), first_of(groups_), [0, 1], groups_)
        first = plan_with(groups)
        base = flat.data_ptr()
        for a in range(2):      # both views write the one claimed slice, the second adding into it
            assert first.sub[a].dL_dsh == base + 4 * 64 and first.sub[a].dL_dmean3D == base + 4 * (64 + 33 * 48)
        assert first.sub[1].accmask & (ACC[2] | ACC[0]) == ACC[2] | ACC[0]
        assert first.out[0][2].data_ptr() == base + 4 * 64 and tuple(first.out[0][2].shape) == (33, 16, 3) and first.out[1][2] is None
        assert sorted(int(sk[1]) for sk in first.sinks) == [64, 64 + 33 * 48] and all(sk[0] is flat for sk in first.sinks)
        # the other fields lie where they lie without sinks, less the two buffers that moved out of the allocation
        big0, big1 = first.big.data_ptr(), first.big.data_ptr() + 4 * first.big.numel()
        assert all(big0 <= getattr(first.sub[0], f) < big1 for f in FIELDS if f not in ("dL_dsh", "dL_dmean3D"))
        second = plan_with(groups)
        assert second.sinks == []
        for f in ("dL_dsh", "dL_dmean3D"):
            p = getattr(second.sub[0], f)
            assert not base <= p < base + 4 * flat.numel(), f
        native.grad_release(first.sinks)
        third = plan_with(groups)
        assert len(third.sinks) == 2 and third.sub[0].dL_dsh == base + 4 * 64
    finally:
        native.GRAD_SINK.pop(id(sh), None)
        native.GRAD_SINK.pop(id(means), None)
