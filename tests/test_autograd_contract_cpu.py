"""tests/autograd_contract.py on the CPU.

(a) The harness on toy torch.autograd.Function nodes.  `toy(flaw)` is y = a b m, z = a - b with one defect switched on; every defect is
one a real wrapper of this library could have (and "contiguous" is the one FusedL1.forward had): each must fail ITS clause and pass the
six others (C3 has no toy of its own: it is C2's accumulation twin), and the two correct toys (once-differentiable, and twice
differentiable) pass all seven.  This is the evidence that tests/test_autograd_contract_gpu.py can fail.

(b) The composed torch branches behind the public wrappers -- neighbour_regularization, geometry_losses, flow_losses, l1_loss, ssim,
regularization(fused=False) -- on CPU tensors through C1..C6: the semantics the HIP nodes must match.  C7 does not apply to them: they are
stock torch operations, the second derivative is torch's own.  UnbindViews and the _join_views it shares with the mesh-transform nodes
launch no kernel and are tested here as they are."""
from types import SimpleNamespace

import pytest

import util  # noqa: F401
import autograd_contract as ac

torch = pytest.importorskip("torch")
from torch.autograd.function import once_differentiable  # noqa: E402

FLAWS = {"contiguous": "C1", "inplace": "C2", "constant": "C4", "stride0": "C5", "stash": "C6", "detached": "C7"}


def _dense(g):
    """what a kernel that takes g.data_ptr() and assumes a dense layout would read (an expanded scalar is densified first: the dense
    read of a one-element storage would leave it)"""
    if g.untyped_storage().nbytes() < (g.storage_offset() + g.numel()) * g.element_size():
        return g.contiguous()
    strides, acc = [], 1
    for d in reversed(g.shape):
        strides.append(acc)
        acc *= d
    return g.as_strided(g.shape, tuple(reversed(strides)))


def toy(flaw=None, twice=False):
    """y = a b m, z = a - b (m a constant) as one node.  flaw:
         contiguous  `need` is read from the copies .contiguous() returns inside forward            (FusedL1.forward before its fix)
         inplace     the gradient kept from forward is scaled in place by backward, the way a kernel writes: past the version counter
         constant    needs_input_grad is ignored and the constant m gets a gradient
         stride0     the upstream gradient is read through its pointer as if it were dense (in bounds: the values of other elements)
         stash       the inputs are kept on ctx, not through save_for_backward
         detached    not once_differentiable, and the result carries no graph
         misaligned  `a` is read as 16-byte vectors whatever its address: a contiguous view that starts one float past a 16-byte
                     boundary gets another gradient (seen by C1 only under the opt-in kind "offset": it is not in FLAWS)"""
    def backward(ctx, gy, gz):
        if flaw == "stash":
            a, b, m = ctx.stash
        elif flaw == "inplace":
            da, db = ctx.saved_tensors
        else:
            a, b, m = ctx.saved_tensors
        ga = gb = gm = None
        if gy is not None:
            if flaw == "stride0":
                gy = _dense(gy)
            if flaw == "inplace":
                ga, gb = da.data.mul_(gy), db.data.mul_(gy)
            else:
                ga, gb = gy * b * m, gy * a * m
            if flaw == "constant":
                gm = gy * a * b
        if gz is not None:
            ga, gb = (gz if ga is None else ga + gz), (-gz if gb is None else gb - gz)
        if flaw == "detached":
            ga, gb = ga.detach(), gb.detach()
        if flaw == "misaligned" and ctx.misaligned:
            ga = ga.roll(1, -1)       # (the elements a vector load at the boundary below the address would pair up)
        if flaw != "constant":
            ga, gb = (ga if ctx.needs_input_grad[0] else None), (gb if ctx.needs_input_grad[1] else None)
        return ga, gb, gm

    class Toy(torch.autograd.Function):
        @staticmethod
        def forward(ctx, a, b, m):
            ctx.set_materialize_grads(False)
            y, z = a * b * m, a - b
            ctx.misaligned = a.contiguous().data_ptr() % 16 != 0      # (a strided view is copied, as a wrapper's .contiguous() does)
            if flaw == "contiguous":
                a, b = a.contiguous(), b.contiguous()
                if a.requires_grad or b.requires_grad:
                    ctx.save_for_backward(a, b, m)
            elif flaw == "stash":
                ctx.stash = (a, b, m)
            elif flaw == "inplace":
                ctx.save_for_backward(b * m, a * m)
            else:
                ctx.save_for_backward(a, b, m)
            return y, z

    Toy.backward = staticmethod(backward if (twice or flaw == "detached") else once_differentiable(backward))
    return Toy


def _second(r):
    """C7 reference of the twice-differentiable toy: the same double backward through stock torch operations, in float64"""
    a, b = (r["leaves"][k].double().requires_grad_() for k in ("a", "b"))
    m = MASK.double()
    ups = [r["ups"][i].double().requires_grad_() for i in (0, 1)]
    first = torch.autograd.grad([a * b * m, a - b], [a, b], ups, create_graph=True)
    torch.autograd.backward(first, [r["probe"][k].double() for k in ("a", "b")])
    want = [t.grad for t in [a, b] + ups]
    got = [r["d_leaves"]["a"], r["d_leaves"]["b"], r["d_ups"][0], r["d_ups"][1]]
    worst = 0.0
    for g, w in zip(got, want):
        assert (g is None) == (w is None)
        if g is not None:       # (products of three float32 numbers and a sum: 4 roundings)
            err = float((g.double() - w).abs().max() / w.abs().max())
            assert err <= 4 * 2.0 ** -24, err
            worst = max(worst, err / (4 * 2.0 ** -24))
    return worst


GEN = torch.Generator().manual_seed(5)
MASK = (torch.rand(6, 5, generator=GEN) > 0.3).float()


OFFSET = ("columns", "transposed", "offset")


def toy_case(flaw=None, twice=False, kinds=None):
    gen = torch.Generator().manual_seed(11)
    fn = toy(flaw, twice)
    diff, const = dict(a=torch.randn(6, 5, generator=gen), b=torch.randn(6, 5, generator=gen)), dict(m=MASK)
    if flaw == "contiguous":          # (as l1_loss(render, gt): the second operand is a constant)
        const["b"] = diff.pop("b")
    return ac.Case(name=f"toy {flaw}", call=lambda t: fn.apply(t["a"], t["b"], t["m"]), diff=diff, const=const, outputs=(0, 1),
                   second=_second if twice else None, **({} if kinds is None else dict(kinds=kinds)))


def outcome(case, clause):
    try:
        return "passes", ac.run_clause(case, clause)
    except Exception as e:            # a violation the harness states, or the node's own crash (FusedL1's was a ValueError)
        return "fails", f"{type(e).__name__}: {e}"


@pytest.mark.parametrize("clause", ac.CLAUSES)
@pytest.mark.parametrize("twice", [False, True], ids=["once_differentiable", "twice_differentiable"])
def test_a_correct_node_passes_every_clause(twice, clause):
    verdict, what = outcome(toy_case(None, twice), clause)
    assert verdict == "passes", what
    if clause == "C7":
        assert (what == ac.EQUAL or what.startswith("within bar")) if twice else what == ac.RAISES, what
    elif clause == "C6":
        assert what == ac.RAISES, what                 # (save_for_backward: autograd's version check)
    else:
        assert what == ac.EQUAL, what


@pytest.mark.parametrize("clause", ac.CLAUSES)
@pytest.mark.parametrize("flaw", list(FLAWS))
def test_each_flawed_node_fails_its_own_clause_and_no_other(flaw, clause):
    verdict, what = outcome(toy_case(flaw), clause)
    assert verdict == ("fails" if FLAWS[flaw] == clause else "passes"), f"toy {flaw}, {clause}: {what}"


def test_the_violations_say_what_was_seen():
    for flaw, word in (("constant", "gradient was computed for a constant"), ("stash", "no error, and d/d"), ("detached", "came back as a constant"),
                       ("inplace", "of the second backward differs from the first"), ("stride0", "a transposed upstream gradient: d/d")):
        with pytest.raises(ac.ContractViolation, match=word):
            ac.run_clause(toy_case(flaw), FLAWS[flaw])
    with pytest.raises(ValueError, match="not enough values to unpack"):        # the crash the issue reports for l1_loss of a cropped render
        ac.run_clause(toy_case("contiguous"), "C1")


@pytest.mark.parametrize("clause", ac.CLAUSES)
def test_the_misaligned_node_fails_c1_under_the_offset_kind_only(clause):
    """kinds = (..., "offset") hands every input as a contiguous view 4 bytes past a 16-byte boundary: the toy that reads `a` as 16-byte
    vectors fails C1 there and nowhere else, and passes C1 under the default kinds; a correct node passes with the kind switched on"""
    verdict, what = outcome(toy_case("misaligned", kinds=OFFSET), clause)
    assert verdict == ("fails" if clause == "C1" else "passes"), f"toy misaligned, {clause}: {what}"
    if clause == "C1":
        assert "a as a offset view: d/da differs from the plain form" in what, what
        assert toy_case("misaligned").kinds == ("columns", "transposed")          # (the default: today's two forms)
        assert outcome(toy_case("misaligned"), "C1") == ("passes", ac.EQUAL)
        for twice in (False, True):
            assert outcome(toy_case(None, twice, kinds=OFFSET), "C1") == ("passes", ac.EQUAL)


def test_the_offset_kind_is_a_contiguous_view_four_bytes_past_a_16_byte_boundary():
    """every rank the harness takes (a scalar, a vector, rows): the view, its base leaf and the mask of the viewed elements"""
    for shape in ((), (7,), (6, 5), (2, 3, 4)):
        v = torch.arange(1, 1 + max(1, int(torch.tensor(shape).prod())) if shape else 2, dtype=torch.float32).reshape(shape)
        base, view, mask, pick = ac._strided(v, "offset")
        assert base.is_leaf and base.requires_grad and base.dim() == 1 and base.data_ptr() % 16 == 0
        assert view.is_contiguous() and view.data_ptr() % 16 == 4 and view.shape == v.shape and torch.equal(view.detach(), v)
        assert int(mask.sum()) == v.numel() and not bool(mask[0]) and torch.equal(pick(base).detach(), v)


def test_a_refusal_is_held_to_its_inputs_and_its_message():
    """C1 "refuses": the inputs a case names must refuse a strided tensor with the stated error, every other input must be taken"""
    fn = toy()

    def call(t):
        if not t["a"].is_contiguous():
            raise ValueError("a would leave the fast path (layout)")
        return fn.apply(t["a"], t["b"], t["m"])
    case = toy_case()
    case.call, case.refuses = call, (ValueError, "(layout)", ("a",))
    assert ac.run_clause(case, "C1") == f"{ac.EQUAL} / {ac.REFUSES}"
    case.refuses = (ValueError, "(dtype)", ("a",))                   # another message: not the refusal that is meant
    with pytest.raises(ValueError, match="layout"):
        ac.run_clause(case, "C1")
    case.refuses = (ValueError, "(layout)", ("a", "b"))              # b is named and is taken: its refusal is gone
    with pytest.raises(ac.ContractViolation, match="its refusal is gone"):
        ac.run_clause(case, "C1")
    case.refuses = (ValueError, "(layout)", ("b",))                  # a refuses and is not named
    with pytest.raises(ValueError, match="layout"):
        ac.run_clause(case, "C1")


def test_a_clause_that_does_not_apply_is_recorded_not_skipped():
    case = toy_case()
    case.na["C5"] = "for the test"
    assert ac.run_clause(case, "C5") == ac.NA
    text = ac.table({("toy None", "C5"): ac.NA, ("toy None", "C1"): ac.EQUAL}, ["toy None"])
    assert "n.a." in text and "equal bits" in text and text.splitlines()[0].startswith("case")


# ------------------------------------------------------------------------------------------------ (b) the composed branches
NO_C7 = {"C7": "stock torch operations on CPU tensors: the second derivative is torch's own"}


def _knn_case():
    from csplat.knn_regs import NeighbourGraph, neighbour_regularization
    gen = torch.Generator().manual_seed(1)
    N, K, T = 17, 3, 3
    idx = torch.stack([(torch.arange(N) + s) % N for s in (1, 2, 5)], 1)
    graph = NeighbourGraph.from_indices(idx, 0.5 + torch.rand(N, K, generator=gen), torch.rand(N, K, generator=gen))
    return ac.Case(name="knn_regs._composed", na=NO_C7,
                   call=lambda t: neighbour_regularization(t["means"], t["rotations"], graph, 0.7, 1.3, 2.1, isometric_abs=True),
                   diff=dict(means=torch.randn(T, N, 3, generator=gen), rotations=torch.randn(T, N, 4, generator=gen)))


def _geometry_case():
    from csplat.geometry_loss import geometry_losses
    gen = torch.Generator().manual_seed(2)
    V, H, W = 2, 3, 5
    img = lambda: torch.rand(1, H, W, generator=gen)  # noqa: E731
    Z = [1.0 + img() for _ in range(V)]
    Z[0][0, 1, 2] = float("nan")
    Z[1][0, 0, 0] = -1.0
    S, M = [(img() > 0.5).float() for _ in range(V)], [(img() > 0.2).float() * (0.25 + img()) for _ in range(V)]

    def call(t):
        return geometry_losses([t["D0"], t["D1"]], [t["A0"], t["A1"]], Z, S, 0.8, 1.2, masks=M, add=t["add"], weight=0.37, add_weight=0.5)
    return ac.Case(name="geometry_loss._geometry_composed", call=call, na=NO_C7,
                   diff=dict(D0=2 * img(), D1=2 * img(), A0=img(), A1=img(), add=torch.tensor(0.4321)))


def _flow_case():
    from csplat.flow_loss import flow_losses
    from test_flow_loss_gpu import make_case
    c = make_case(23, 3, (9, 7), "mask_cap")
    vis = [v.clone() for v in c["vis"]]

    def call(t):
        return flow_losses([t["X0"], t["X1"], t["X2"]], c["full"], c["flows"], (c["H"], c["W"]), visible=vis, masks=c["masks"],
                           lambda_flow=0.7, max_error=c["cap"], add=t["add"], weight=0.37, add_weight=0.5)
    return ac.Case(name="flow_loss._flow_composed", call=call, na=NO_C7,
                   diff=dict(X0=c["X"][0], X1=c["X"][1], X2=c["X"][2], add=torch.tensor(-1.25)))


def _images(seed):
    gen = torch.Generator().manual_seed(seed)
    return torch.rand(2, 3, 13, 17, generator=gen), torch.rand(2, 3, 13, 17, generator=gen), (torch.rand(2, 1, 13, 17, generator=gen) > 0.3).float()


def _mean_in_another_order(got, ref):
    """torch's mean walks a strided operand in memory order: the same n terms of one sign summed in two orders differ by at most
    2 (n - 1) 2^-24 of the sum (each order is within (n - 1) 2^-24 of the exact one); the gradients are elementwise and keep their bits"""
    n = got.leaves["a"].numel()
    for k, g in ref.grads.items():
        assert ac.same(got.grads[k], g), k
    err = abs(float(got.outs[0]) - float(ref.outs[0])) / abs(float(ref.outs[0]))
    bound = 2 * (n - 1) * 2.0 ** -24
    assert err <= bound, (err, bound)
    return err / bound


def _l1_case(masked):
    from csplat.image_loss import l1_loss
    x, y, m = _images(3)
    return ac.Case(name=f"l1_loss composed{' masked' if masked else ''}", na=NO_C7, diff=dict(a=x, b=y), reorder=_mean_in_another_order,
                   call=lambda t: l1_loss(t["a"], t["b"], m if masked else None))


def _ssim_case():
    from csplat.image_loss import ssim
    x, y, _ = _images(4)
    return ac.Case(name="ssim composed", na=NO_C7, diff=dict(img1=x, img2=y), call=lambda t: ssim(t["img1"], t["img2"]))


def _regs_case():
    from csplat.cloth_regs import regularization
    gen = torch.Generator().manual_seed(6)
    V, E = 19, 31
    ei = torch.randint(0, V, (2, E), generator=gen)
    ei[1] = torch.where(ei[1] == ei[0], (ei[1] + 1) % V, ei[1])          # (no self-loop: the norm of a zero edge has no gradient in torch)
    g = SimpleNamespace(mesh=SimpleNamespace(edge_index=ei), edge_norm=0.25 + torch.rand(E, 1, generator=gen))
    opt = SimpleNamespace(lambda_deform_mag=0.01, lambda_rigid=0.3, lambda_momentum=0.1)
    return ac.Case(name="regularization(fused=False)", na=NO_C7, diff=dict(D=torch.randn(3, V, 3, generator=gen)),
                   call=lambda t: regularization(t["D"], g, opt, fused=False))


def _unbind_case():
    from csplat.gaussians import UnbindViews          # (no kernel: the node is the same on CPU tensors)
    x = torch.randn(3, 7, 4, generator=torch.Generator().manual_seed(8))
    return ac.Case(name="UnbindViews", call=lambda t: UnbindViews.apply(t["x"]), diff=dict(x=x), outputs=(0, 1, 2), joins=((0, 1, 2),))


COMPOSED = {"knn": _knn_case, "geometry": _geometry_case, "flow": _flow_case, "l1": lambda: _l1_case(False), "l1_masked": lambda: _l1_case(True),
            "ssim": _ssim_case, "regularization": _regs_case}


@pytest.mark.parametrize("clause", ac.CLAUSES)
def test_unbind_views_on_cpu_tensors(clause):
    got = ac.run_clause(_unbind_case(), clause)
    assert got == (ac.RAISES if clause in ("C6", "C7") else ac.EQUAL), got        # (C6: its outputs are views of the input)


def test_join_views_is_a_view_only_of_rows_that_sit_back_to_back(monkeypatch):
    """csplat.gaussians._join_views: T gradients laid out back to back in one buffer come back as a VIEW of it; the same values in
    separate buffers, rows in another order, a gap, a strided row or a missing row (zeros) as a copy; no row at all as None.  And the
    harness's joined consumer of C5 really hands the node back-to-back rows."""
    from csplat import gaussians as G
    buf = torch.arange(3 * 5 * 2, dtype=torch.float32).reshape(3, 5, 2)
    rows = list(buf.unbind(0))
    args = ((5, 2), torch.float32, buf.device)
    v = G._join_views(rows, *args)
    assert torch.equal(v, buf) and v.data_ptr() == buf.data_ptr() and v.is_contiguous()
    off = torch.zeros(31)
    shifted = list(off[1:].view(3, 5, 2).copy_(buf).unbind(0))                    # (a buffer that does not start at its storage's first element)
    v = G._join_views(shifted, *args)
    assert torch.equal(v, buf) and v.data_ptr() == shifted[0].data_ptr()
    for what, grads, want in (("separate", [r.clone() for r in rows], buf), ("reordered", [rows[1], rows[0], rows[2]], buf[[1, 0, 2]]),
                              ("gap", list(torch.cat([buf, buf])[::2].unbind(0)), torch.cat([buf, buf])[::2]),
                              ("strided row", list(buf.transpose(1, 2).contiguous().transpose(1, 2).unbind(0)), buf),
                              ("one missing", [rows[0], None, rows[2]], buf * torch.tensor([1.0, 0.0, 1.0]).view(3, 1, 1)),
                              ("first missing", [None, rows[1], rows[2]], buf * torch.tensor([0.0, 1.0, 1.0]).view(3, 1, 1))):
        v = G._join_views(grads, *args)
        assert torch.equal(v, want) and v.data_ptr() != buf.data_ptr() and v.is_contiguous(), what
    assert G._join_views([None, None, None], *args) is None
    seen, real = [], G._join_views

    def spy(grads, rest, dtype, dev):
        out = real(grads, rest, dtype, dev)
        seen.append(out is not None and grads[0] is not None and out.data_ptr() == grads[0].data_ptr())
        return out
    monkeypatch.setattr(G, "_join_views", spy)
    case = _unbind_case()
    ref = ac.plain(case)
    assert seen == [False]                                                        # (the plain form: a gradient per output, each in its own buffer)
    del seen[:]
    case.subsets = []
    assert ac.c5(case, ref) == ac.EQUAL and seen[-1] is True and False in seen    # (the joined consumer comes last)


@pytest.mark.parametrize("clause", ac.CLAUSES)
@pytest.mark.parametrize("name", list(COMPOSED))
def test_composed_branches_keep_the_contract(name, clause):
    case = COMPOSED[name]()
    got = ac.run_clause(case, clause)
    if clause == "C7":
        assert got == ac.NA
    elif clause == "C6":
        assert set(got.split(" / ")) <= {ac.EQUAL, ac.RAISES}, got
    elif clause == "C1" and case.reorder is not None:
        assert all(v == ac.EQUAL or v.startswith("within bar") for v in got.split(" / ")), got
    else:
        assert got == ac.EQUAL, got
