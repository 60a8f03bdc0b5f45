"""The calling contract of an autograd node, checked from the outside: a node-agnostic harness.

A kernel-against-fp64 test varies the values a node sees; this harness varies HOW autograd reaches the node -- strided inputs, a second
backward, accumulation into .grad, subsets of needs_input_grad, the forms an upstream gradient arrives in, an input edited between
forward and backward, create_graph.  A `Case` names the public callable a user would call, its differentiable tensor inputs, its
constants and which outputs are differentiable; the harness evaluates the PLAIN FORM once (contiguous fp32 leaves that all require a
gradient, every differentiable output weighted with fixed dense random weights, one backward) and each clause C1..C7 against it.

"equal" is equality of bits (in C5, against explicit zero gradients for the unused outputs, up to the sign of a zero: x + 0 turns -0
into +0).  A clause that cannot be bit-equal for a stated reason (a strided input that leaves the HIP path through a
counted "layout" fallback) is compared through `Case.bar`, the node's own fp64 bar rule, which returns error / bar.  A clause returns
what it observed -- "equal bits", "within bar (ratio)", "raises", "refuses" -- and raises ContractViolation otherwise; `Case.na` holds
the clauses that do not apply to a node, with the reason.  C1 hands every input as a column slice and as a transpose; `Case.kinds` may
add "offset", a CONTIGUOUS view that starts one float past a 16-byte boundary (what a kernel's 16-byte accesses cannot read: the node
copies it or refuses it in forward, never in backward).  tests/test_autograd_contract_cpu.py runs the harness on toy nodes that each
break one clause; tests/test_autograd_contract_gpu.py and tests/test_autograd_contract_meshnet_gpu.py run it on the HIP nodes."""
import contextlib
import itertools
from dataclasses import dataclass, field
from typing import Callable, Optional

import torch

CLAUSES = ("C1", "C2", "C3", "C4", "C5", "C6", "C7")
TITLES = {"C1": "strided inputs", "C2": "second backward", "C3": "accumulation", "C4": "needs_input_grad subsets",
          "C5": "upstream gradient forms", "C6": "in-place edit before backward", "C7": "create_graph"}
EQUAL, RAISES, REFUSES, NA = "equal bits", "raises", "refuses", "n.a."


class ContractViolation(AssertionError):
    pass


@dataclass
class Case:
    """call(tensors) -> a tensor or a sequence of tensors, `tensors` = {name: tensor} holding the differentiable inputs (`diff`: name ->
    contiguous float32 values; the harness makes the leaves) and the constants (`const`, passed as they are).  `outputs`: positions of
    the differentiable outputs in what call() returns."""
    name: str
    call: Callable
    diff: dict
    const: dict = field(default_factory=dict)
    outputs: tuple = (0,)
    na: dict = field(default_factory=dict)            # clause -> why it does not apply to this node
    bar: Optional[Callable] = None                    # bar(result) -> error / bar against the node's fp64 restatement (asserts its own rule)
    scope: Optional[Callable] = None                  # context manager around every evaluation (e.g. the rasterizer's reproducible mode)
    fallbacks: Optional[Callable] = None              # context manager yielding the Counter of (site, kind) fallbacks; None: nothing counts
    refuses: Optional[tuple] = None                   # (exception type, words of its message, the inputs that refuse a strided tensor):
    #                                                   those inputs MUST refuse that way ("refuses"), every other input must be taken
    joins: tuple = ()                                 # groups of output positions whose gradients the node joins (_join_views)
    second: Optional[Callable] = None                 # second(result) -> error / bar of the second derivative (C7); None: must raise
    weights: Optional[Callable] = None                # weights(position, output) -> the plain form's upstream gradient (default: random)
    after: Optional[Callable] = None                  # called after every forward (e.g. launch_deferred)
    subsets: Optional[list] = None                    # the subsets of `outputs` C5 uses alone (None: every non-empty proper subset)
    subset_bar: Optional[Callable] = None             # subset_bar(result) -> error / bar against fp64 for the weights in result.ups, where the
    #                                                   node takes other kernels for a subset of its outputs (C5; None: bits must be equal)
    reorder: Optional[Callable] = None                # reorder(got, plain) -> error / bound, for a composed torch branch whose reduction
    #                                                   runs over the strided memory in another order (C1; None: bits must be equal)
    kinds: tuple = ("columns", "transposed")          # the forms C1 hands every input in; "offset" (opt-in): a CONTIGUOUS view that starts
    #                                                   one float past a 16-byte boundary -- what a kernel's float4 access cannot read


@dataclass
class Result:
    outs: list                                        # every output, detached copies
    grads: dict                                       # name -> gradient of the leaf (a copy) or None
    leaves: dict
    raw: list                                         # the outputs themselves (graph attached)
    ups: dict                                         # position -> the upstream gradient used


def bits(t):
    t = t.detach().contiguous()
    if t.dtype == torch.float32:
        return t.view(torch.int32)
    if t.dtype == torch.float64:
        return t.view(torch.int64)
    return t


def same(a, b, signed_zero=True):
    """equal bits; signed_zero=False: a -0 equals a +0 (x + 0 turns one into the other: the explicit zero gradients of C5)"""
    if a is None or b is None:
        return a is None and b is None
    if not signed_zero and a.dtype.is_floating_point and b.dtype.is_floating_point:
        a, b = a.detach() + 0.0, b.detach() + 0.0
    return a.shape == b.shape and a.dtype == b.dtype and bool(torch.equal(bits(a), bits(b)))


def _require(cond, clause, case, what):
    if not cond:
        raise ContractViolation(f"{case.name} {clause} ({TITLES[clause]}): {what}")


def _same_all(clause, case, what, got, ref, names=None):
    for k in (names if names is not None else ref.grads):
        _require(same(got.grads[k], ref.grads[k]), clause, case, f"{what}: d/d{k} differs from the plain form"
                 + _diff(got.grads[k], ref.grads[k]))
    for i, (a, b) in enumerate(zip(got.outs, ref.outs)):
        _require(same(a, b), clause, case, f"{what}: output {i} differs from the plain form" + _diff(a, b))


def _diff(a, b):
    if a is None or b is None:
        return f" ({'None' if a is None else 'a tensor'} against {'None' if b is None else 'a tensor'})"
    if a.shape != b.shape or not a.dtype.is_floating_point:
        return f" ({tuple(a.shape)} {a.dtype} against {tuple(b.shape)} {b.dtype})"
    d = (a.double() - b.double()).abs().max().item() if a.numel() else 0.0
    return f" (largest difference {d:.3e}, largest value {b.double().abs().max().item() if b.numel() else 0.0:.3e})"


def _tuple(out):
    return [out] if torch.is_tensor(out) else list(out)


def _scope(case):
    return case.scope() if case.scope is not None else contextlib.nullcontext()


def _forward(case, tensors):
    with _scope(case):
        raw = _tuple(case.call(tensors))
        if case.after is not None:
            case.after()
    return raw


def upstream(case, raw):
    """position -> the fixed dense weights of the plain form"""
    ups = {}
    for i in case.outputs:
        o = raw[i]
        if case.weights is not None:
            ups[i] = case.weights(i, o).to(o.device, o.dtype).contiguous()
        else:
            g = torch.Generator().manual_seed(1000 + 17 * i + o.numel())
            ups[i] = (0.5 + torch.rand(o.shape, generator=g, dtype=torch.float32)).to(o.device, o.dtype)
    return ups


def leaves_of(case, requires=None):
    return {k: v.detach().clone().contiguous().requires_grad_(requires is None or k in requires) for k, v in case.diff.items()}


def _backward(case, raw, ups, positions=None, **kw):
    positions = [i for i in (case.outputs if positions is None else positions) if raw[i].requires_grad]
    if not positions:
        return
    with _scope(case):
        torch.autograd.backward([raw[i] for i in positions], [ups[i].clone() for i in positions], **kw)


def evaluate(case, leaves=None, ups=None, positions=None, backward=True):
    leaves = leaves_of(case) if leaves is None else leaves
    raw = _forward(case, {**case.const, **leaves})
    ups = upstream(case, raw) if ups is None else ups
    if backward:
        _backward(case, raw, ups, positions)
    return Result([o.detach().clone() if torch.is_tensor(o) else o for o in raw],
                  {k: (None if v.grad is None else v.grad.detach().clone()) for k, v in leaves.items()}, leaves, raw, ups)


def plain(case):
    r = evaluate(case)
    for i in case.outputs:
        if not (torch.is_tensor(r.raw[i]) and r.raw[i].requires_grad):
            raise ContractViolation(f"{case.name}: output {i} of the plain form requires no gradient")
    for k, g in r.grads.items():
        if g is None:
            raise ContractViolation(f"{case.name}: the plain form leaves d/d{k} at None")
        if not bool(torch.isfinite(g).all()):
            raise ContractViolation(f"{case.name}: the plain form's d/d{k} is not finite")
    return r


# ------------------------------------------------------------------------------------------------ C1
def _strided(values, kind):
    """(base leaf, view of it with `values`, mask of the viewed elements in the base)"""
    v = values.detach()
    if kind == "offset":                               # contiguous, and 4 bytes past a 16-byte boundary: a slice of a flat buffer
        n = v.numel()
        base = torch.zeros(n + 1, dtype=v.dtype, device=v.device)
        pick = lambda b: b[1:1 + n].view(v.shape)  # noqa: E731
    elif v.dim() == 0:                                 # (a scalar has no stride: an element inside a larger buffer)
        base = torch.zeros(3, dtype=v.dtype, device=v.device)
        pick = lambda b: b[1]  # noqa: E731
    elif v.dim() == 1:                                 # a column of a [n, 2] buffer
        base = torch.zeros(v.shape[0], 2, dtype=v.dtype, device=v.device)
        pick = lambda b: b[:, 1]  # noqa: E731
    elif kind == "columns":                            # a column slice of a wider buffer
        base = torch.zeros(tuple(v.shape[:-1]) + (v.shape[-1] + 3,), dtype=v.dtype, device=v.device)
        pick = lambda b: b[..., 1:1 + v.shape[-1]]  # noqa: E731
    else:                                              # the transpose of a buffer laid out the other way round
        base = torch.zeros(tuple(v.shape[:-2]) + (v.shape[-1], v.shape[-2]), dtype=v.dtype, device=v.device)
        pick = lambda b: b.transpose(-1, -2)  # noqa: E731
    pick(base).copy_(v)
    base = base.clone().requires_grad_()
    view = pick(base)
    if kind == "offset":
        assert view.is_contiguous() and view.data_ptr() % 16 == 4, (view.is_contiguous(), view.data_ptr() % 16)
    mask = torch.zeros_like(base, dtype=torch.bool)
    pick(mask).fill_(True)
    return base, view, mask, pick


def c1(case, ref):
    verdicts = []
    for name, kind in itertools.product(case.diff, case.kinds):
        leaves = leaves_of(case)
        base, view, mask, pick = _strided(case.diff[name], kind)
        leaves[name] = view
        # (a [P, 1] tensor is contiguous as a transposed view too: an offset into a larger buffer, nothing to refuse)
        refusing = case.refuses is not None and name in case.refuses[2] and not view.is_contiguous()
        scope = case.fallbacks() if case.fallbacks is not None else contextlib.nullcontext({})
        try:
            with scope as counts:
                before = dict(counts)
                raw = _forward(case, {**case.const, **leaves})
                _backward(case, raw, ref.ups)
                moved = {k: n - before.get(k, 0) for k, n in dict(counts).items() if n != before.get(k, 0)}
        except Exception as e:
            if refusing and isinstance(e, case.refuses[0]) and case.refuses[1] in str(e):
                verdicts.append(REFUSES)
                continue
            raise
        _require(not refusing, "C1", case, f"{name} as a {kind} view was taken: its refusal is gone")
        got = Result([o.detach().clone() if torch.is_tensor(o) else o for o in raw],
                     {k: (None if v.grad is None else v.grad.detach().clone()) for k, v in leaves.items() if k != name}, leaves, raw, ref.ups)
        _require(base.grad is not None, "C1", case, f"{name} as a {kind} view: its base leaf received no gradient")
        _require(not bool(base.grad[~mask].ne(0).any()), "C1", case, f"{name} as a {kind} view: a gradient outside the viewed elements")
        got.grads[name] = pick(base.grad).detach().clone().contiguous()
        # (reorder speaks of strided memory: a contiguous view, the "offset" kind, stays held to the plain form's bits)
        if not moved and case.reorder is not None and not view.is_contiguous() and not all(same(a, b) for a, b in zip(got.outs, ref.outs)):
            verdicts.append(f"within bar ({case.reorder(got, ref):.2f})")
        elif not moved:
            _same_all("C1", case, f"{name} as a {kind} view", got, ref)
            verdicts.append(EQUAL)
        else:
            _require(all(k[1] == "layout" for k in moved), "C1", case, f"{name} as a {kind} view left the HIP path as {sorted(moved)}")
            _require(case.bar is not None, "C1", case, "a fallback was counted and the case has no bar rule")
            verdicts.append(f"within bar ({case.bar(got):.2f})")
    return _worst(verdicts)


def _worst(verdicts):
    if all(v == EQUAL for v in verdicts):
        return EQUAL
    if all(v == REFUSES for v in verdicts):
        return REFUSES
    rest = sorted({v for v in verdicts if v != EQUAL})
    return " / ".join(([EQUAL] if EQUAL in verdicts else []) + rest)


# ------------------------------------------------------------------------------------------------ C2, C3
def c2(case, ref):
    leaves = leaves_of(case)
    raw = _forward(case, {**case.const, **leaves})
    ins = {k: v.detach().clone() for k, v in leaves.items()}
    cons = {k: v.detach().clone() for k, v in case.const.items() if torch.is_tensor(v)}
    outs = [o.detach().clone() if torch.is_tensor(o) else o for o in raw]
    _backward(case, raw, ref.ups, retain_graph=True)
    first = {k: v.grad.detach().clone() for k, v in leaves.items()}
    for v in leaves.values():
        v.grad = None
    _backward(case, raw, ref.ups)
    for k, v in leaves.items():
        _require(same(v.grad, first[k]), "C2", case, f"d/d{k} of the second backward differs from the first" + _diff(v.grad, first[k]))
        _require(same(first[k], ref.grads[k]), "C2", case, f"d/d{k} under retain_graph differs from the plain form")
        _require(same(v, ins[k]), "C2", case, f"input {k} was changed")
    for k, v in cons.items():
        _require(same(case.const[k], v), "C2", case, f"constant {k} was changed")
    for i, (a, b) in enumerate(zip(raw, outs)):
        _require(not torch.is_tensor(a) or same(a, b), "C2", case, f"output {i} was changed by a backward")
    _same_all("C2", case, "a fresh call after two backward passes", evaluate(case, ups=ref.ups), ref)
    return EQUAL


def c3(case, ref):
    leaves = leaves_of(case)
    for _ in range(2):
        _backward(case, _forward(case, {**case.const, **leaves}), ref.ups)
    for k, v in leaves.items():
        _require(same(v.grad, 2 * ref.grads[k]), "C3", case, f"two passes leave d/d{k} != 2 g" + _diff(v.grad, 2 * ref.grads[k]))
    return EQUAL


# ------------------------------------------------------------------------------------------------ C4
def _custom_nodes(raw):
    """every node of a torch.autograd.Function in the graphs of `raw`"""
    seen, stack, found = set(), [o.grad_fn for o in raw if torch.is_tensor(o) and o.grad_fn is not None], []
    while stack:
        fn = stack.pop()
        if fn is None or fn in seen:
            continue
        seen.add(fn)
        if isinstance(fn, torch.autograd.function.BackwardCFunction):
            found.append(fn)
        stack += [f for f, _ in fn.next_functions]
    return found


def c4(case, ref):
    # a gradient for a constant: in the plain form every edge that leads nowhere belongs to a constant
    leaves = leaves_of(case)
    raw = _forward(case, {**case.const, **leaves})
    offenders = []

    def watch(fn):
        dead = [i for i, (f, _) in enumerate(fn.next_functions) if f is None]

        def hook(grad_inputs, _grad_outputs):
            offenders.extend(f"{type(fn).__name__} input {i}" for i in dead if i < len(grad_inputs) and grad_inputs[i] is not None)
        return fn.register_hook(hook)
    handles = [watch(fn) for fn in _custom_nodes(raw)]
    _backward(case, raw, ref.ups)
    for h in handles:
        h.remove()
    _require(not offenders, "C4", case, f"a gradient was computed for a constant: {sorted(set(offenders))}")
    for name in case.diff:
        got = evaluate(case, leaves_of(case, requires=(name,)), ups=ref.ups)
        _require(same(got.grads[name], ref.grads[name]), "C4", case, f"{name} alone requiring a gradient: d/d{name} differs from the "
                 "plain form" + _diff(got.grads[name], ref.grads[name]))
        for other in case.diff:
            _require(other == name or got.leaves[other].grad is None, "C4", case, f"{name} alone requiring a gradient: {other}.grad is set")
        for i, (a, b) in enumerate(zip(got.outs, ref.outs)):
            _require(same(a, b), "C4", case, f"{name} alone requiring a gradient: output {i} differs")
    for what, ctx, requires in (("no input requiring a gradient", contextlib.nullcontext(), ()), ("torch.no_grad()", torch.no_grad(), None)):
        tensors = {**case.const, **leaves_of(case, requires=requires)}
        with ctx:
            raw = _forward(case, tensors)
        for i, (a, b) in enumerate(zip(raw, ref.outs)):
            if torch.is_tensor(a):
                _require(same(a, b), "C4", case, f"{what}: output {i} differs from the plain form" + _diff(a, b))
                # (an output that IS an input, or a view of one, carries the input's own flag: a node that passes a tensor through)
                passed = any(a is t or a._base is t for t in tensors.values() if torch.is_tensor(t))
                _require(passed or not a.requires_grad, "C4", case, f"{what}: output {i} requires a gradient")
    return EQUAL


# ------------------------------------------------------------------------------------------------ C5
def c5(case, ref):
    pos = list(case.outputs)
    # the stride-0 gradient of out.sum() against an explicit tensor of ones
    ones = {i: torch.ones_like(ref.ups[i]) for i in pos}
    want = evaluate(case, ups=ones)
    leaves = leaves_of(case)
    raw = _forward(case, {**case.const, **leaves})
    with _scope(case):
        sum(raw[i].sum() for i in pos).backward()
    for k, v in leaves.items():
        _require(same(v.grad, want.grads[k]), "C5", case, f"the expanded gradient of out.sum(): d/d{k} differs from explicit ones"
                 + _diff(v.grad, want.grads[k]))
    # a non-contiguous gradient: the consumer works on out.transpose(-1, -2)
    if any(ref.ups[i].dim() >= 2 for i in pos):
        leaves = leaves_of(case)
        raw = _forward(case, {**case.const, **leaves})
        terms = []
        for i in pos:
            if ref.ups[i].dim() >= 2:
                terms.append((raw[i].transpose(-1, -2) * ref.ups[i].transpose(-1, -2).contiguous()).sum())
            else:
                terms.append((raw[i] * ref.ups[i]).sum())
        with _scope(case):
            sum(terms).backward()
        for k, v in leaves.items():
            _require(same(v.grad, ref.grads[k]), "C5", case, f"a transposed upstream gradient: d/d{k} differs from the plain form"
                     + _diff(v.grad, ref.grads[k]))
    # every non-empty proper subset of the outputs against explicit zeros for the others
    ratios = []
    if len(pos) > 1:
        subsets = case.subsets if case.subsets is not None else [sub for n in range(1, len(pos)) for sub in itertools.combinations(pos, n)]
        for sub in subsets:
            zeros = {i: (ref.ups[i] if i in sub else torch.zeros_like(ref.ups[i])) for i in pos}
            want = evaluate(case, ups=zeros)
            got = evaluate(case, ups=ref.ups, positions=sub)
            for k in case.diff:
                if got.grads[k] is None:
                    got.grads[k] = torch.zeros_like(want.grads[k])
            differ = [k for k in case.diff if not same(got.grads[k], want.grads[k], signed_zero=False)]
            if differ and case.subset_bar is not None:      # (the node runs other kernels when a gradient is absent: the fp64 bar decides)
                got.ups = zeros
                ratios.append(case.subset_bar(got))
                continue
            k = differ[0] if differ else None
            _require(not differ, "C5", case, f"outputs {sub} used alone: d/d{k} differs from explicit zeros for the others"
                     + (_diff(got.grads[k], want.grads[k]) if differ else ""))
    # the joined siblings: back to back in one buffer (the stack's backward hands out views of one tensor), and apart
    for group in case.joins:
        group = list(group)
        leaves = leaves_of(case)
        raw = _forward(case, {**case.const, **leaves})
        stacked = torch.stack([ref.ups[i] for i in group])
        rest = [i for i in pos if i not in group]
        with _scope(case):
            torch.autograd.backward([torch.stack([raw[i] for i in group])] + [raw[i] for i in rest],
                                    [stacked.clone()] + [ref.ups[i].clone() for i in rest])
        for k, v in leaves.items():
            _require(same(v.grad, ref.grads[k]), "C5", case, f"outputs {tuple(group)} with back-to-back gradients: d/d{k} differs from "
                     "gradients in separate buffers" + _diff(v.grad, ref.grads[k]))
    return EQUAL if not ratios else f"{EQUAL} / within bar ({max(ratios):.2f})"


# ------------------------------------------------------------------------------------------------ C6
def c6(case, ref):
    verdicts = []
    for name in case.diff:
        leaves = leaves_of(case)
        raw = _forward(case, {**case.const, **leaves})
        with torch.no_grad():
            leaves[name].mul_(0.5)
        try:
            _backward(case, raw, ref.ups)
        except RuntimeError as e:
            # (autograd's two refusals: the version check of a saved tensor, and the check of a node whose outputs are views of the input)
            _require("modified by an inplace operation" in str(e) or "has been modified inplace" in str(e), "C6", case,
                     f"{name} edited in place: backward raised {e!r}")
            verdicts.append(RAISES)
            continue
        for k, v in leaves.items():
            _require(same(v.grad, ref.grads[k]), "C6", case, f"{name} edited in place between forward and backward: no error, and d/d{k} "
                     "differs from the plain form" + _diff(v.grad, ref.grads[k]))
        verdicts.append(EQUAL)
    return _worst(verdicts)


# ------------------------------------------------------------------------------------------------ C7
def c7(case, ref):
    leaves = leaves_of(case)
    raw = _forward(case, {**case.const, **leaves})
    pos = list(case.outputs)
    ups = [ref.ups[i].clone().requires_grad_() for i in pos]
    names = list(leaves)
    try:
        with _scope(case):
            first = torch.autograd.grad([raw[i] for i in pos], [leaves[k] for k in names], ups, create_graph=True, allow_unused=True)
        for k, g in zip(names, first):
            _require(g is not None and same(g, ref.grads[k]), "C7", case, f"d/d{k} under create_graph differs from the plain form")
        # (the gradient is linear in the upstream gradient, which requires one here: a result that requires none is a constant)
        for k, g in zip(names, first):
            _require(g.requires_grad, "C7", case, f"d/d{k} came back as a constant under create_graph (no error, no graph)")
        probe = {k: torch.rand(g.shape, generator=torch.Generator().manual_seed(7 + n), dtype=torch.float32).to(g.device, g.dtype)
                 for n, (k, g) in enumerate(zip(names, first))}
        # (backward(), not grad(): the node once_differentiable leaves behind hangs on detached stand-ins, so grad(..., allow_unused=True)
        #  would never run it and return None for everything)
        with _scope(case):
            torch.autograd.backward(list(first), [probe[k] for k in names])
        secondd = [leaves[k].grad for k in names] + [u.grad for u in ups]
    except RuntimeError as e:
        _require("once_differentiable" in str(e) or "differentiate twice" in str(e), "C7", case, f"create_graph raised {e!r}")
        return RAISES
    _require(case.second is not None, "C7", case, "a second derivative came back and the case states no reference for it")
    ratio = case.second(dict(leaves={k: v.detach() for k, v in leaves.items()}, ups=dict(zip(pos, [u.detach() for u in ups])), probe=probe,
                             d_leaves=dict(zip(names, secondd[:len(names)])), d_ups=dict(zip(pos, secondd[len(names):]))))
    return EQUAL if ratio == 0.0 else f"within bar ({ratio:.2f})"


RUN = {"C1": c1, "C2": c2, "C3": c3, "C4": c4, "C5": c5, "C6": c6, "C7": c7}


def run_clause(case, clause, ref=None):
    """what the clause observed on `case` ("equal bits", "within bar (r)", "raises", "refuses", "n.a."); ContractViolation otherwise"""
    if clause in case.na:
        return NA
    return RUN[clause](case, plain(case) if ref is None else ref)


def table(rows, cases, clauses=CLAUSES):
    """the case x clause table as text; rows: {(case name, clause): entry}"""
    width = max(len(c) for c in cases) + 1
    lines = ["case".ljust(width) + " | " + " | ".join(clauses)]
    for c in cases:
        lines.append(c.ljust(width) + " | " + " | ".join(rows.get((c, k), "-") for k in clauses))
    return "\n".join(lines)
