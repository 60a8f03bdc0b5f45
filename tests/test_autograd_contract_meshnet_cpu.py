"""The CPU parts of tests/test_autograd_contract_meshnet_gpu.py: every case of that file built without a GPU, with the float32
restatement standing in for the node (Build("cpu")).

(a) Every ReLU'd input is drawn by gnn_autograd_ref.draw_without_ties inside its own round cap (building a case asserts it).
(b) Every case's bar rule runs on its plain form: the float32 restatement against float64 under the owning file's rule.  The stand-in's
    error IS e32, so the ratio is 1 / 8 under the 8 x e32 rules (and e32 / (4 e32 + 4 u) under test_knn_regs_gpu.py's); what this
    checks is that no bar passes its file's ill-conditioning cap (BAR_MAX) on the shapes and upstream gradients the GPU file uses, and that
    the bar code itself runs.
(c) _Length is torch operations: the node itself through all seven clauses on CPU tensors, C7 a true second derivative."""
import pytest

import util  # noqa: F401
import autograd_contract as ac

torch = pytest.importorskip("torch")
import test_autograd_contract_meshnet_gpu as G  # noqa: E402


@pytest.mark.parametrize("name", list(G.CASES))
def test_the_draws_succeed_and_the_float32_restatement_meets_every_bar(name):
    case, ref = G.built(name, "cpu")
    assert case.kinds == ("columns", "transposed", "offset") and not case.na
    ratio = case.bar(ref)
    assert ratio <= 1.0, ratio


@pytest.mark.parametrize("clause", ac.CLAUSES)
def test_length_on_cpu_tensors(clause):
    from csplat.knn_regs import _Length
    case = G.CASES["_Length"](G.Build("cpu"))
    case.call = lambda t: _Length.apply(t["off"])
    got = ac.run_clause(case, clause)
    if clause == "C7":
        assert got.startswith("within bar"), got
    else:
        assert got == (ac.RAISES if clause == "C6" else ac.EQUAL), got        # (C6: off is saved)
