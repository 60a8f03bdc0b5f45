"""Host-side logic of the MeshNet half that needs no GPU and launches nothing: the version-keyed pack cache of
meshnet/graph_network.py and the two shape predicates of meshnet/graph_ops.py that decide whether the simulator's fused nodes apply."""
import types

import pytest

torch = pytest.importorskip("torch")

import util  # noqa: E402,F401


def test_pack_cache_builds_once_per_key_and_keeps_the_key_readable():
    """graph_network._cached(owner, slot, key, build): the same key builds once; a bumped `_version` of a tensor in the key or another
    mode value in the key builds again; the stored key can be read back (a layer's node image is keyed on the NEXT layer's stored
    weight-split key); the build runs under no_grad."""
    from meshnet.graph_network import _cached
    owner = types.SimpleNamespace()
    w = torch.zeros(4, requires_grad=True)
    calls = []

    def build():
        calls.append(torch.is_grad_enabled())
        return len(calls)

    def key(mode):
        return (w._version, w.data_ptr(), mode)
    assert _cached(owner, "_img", key(0), build) == 1
    assert _cached(owner, "_img", key(0), build) == 1 and len(calls) == 1
    assert owner._img_key == key(0) and owner._img == 1
    with torch.no_grad():
        w.add_(1.0)                                  # an optimizer step: the version moves, the address does not
    assert _cached(owner, "_img", key(0), build) == 2 and owner._img_key == key(0)
    assert _cached(owner, "_img", key(1), build) == 3 and owner._img_key == key(1)      # another arithmetic mode
    assert _cached(owner, "_img", key(1), build) == 3
    assert _cached(owner, "_other", key(1), build) == 4 and owner._img == 3              # slots are independent
    assert calls == [False] * 4


class _T:
    """what the predicates read of a tensor: device kind, rank, shape, element count, requires_grad"""

    def __init__(self, *shape, cuda=True, requires_grad=False):
        self.shape, self.is_cuda, self.requires_grad = tuple(shape), cuda, requires_grad

    def dim(self):
        return len(self.shape)

    def numel(self):
        n = 1
        for d in self.shape:
            n *= d
        return n


def _lin(out_f, in_f, bias=True):
    return types.SimpleNamespace(weight=_T(out_f, in_f), bias=_T(out_f) if bias else None)


R_OUT = 30
# (what differs from the ordinary case T = 3, K0 = 13, R = 30 with table rows) -> (sim_hidden applies, sim_residual applies), read off the
# conditions: e on the GPU, 2-D, 0 < T <= 8, K0 <= 16, lin1 [256, K0] and lin2 [256, 256] with biases, e without gradient; the residual
# form also wants lin_out [., 256] with a bias and base (when given) on the GPU with T * R elements
PREDICATE_TABLE = [
    ("ordinary",             dict(),                                   True,  True),
    ("T = 0",                dict(T=0),                                False, False),
    ("T = 8",                dict(T=8),                                True,  True),
    ("T = 9",                dict(T=9),                                False, False),
    ("K0 = 16",              dict(K0=16),                              True,  True),
    ("K0 = 17",              dict(K0=17),                              False, False),
    ("lin1 without bias",    dict(bias1=False),                        False, False),
    ("lin2 without bias",    dict(bias2=False),                        False, False),
    ("lin_out without bias", dict(bias_out=False),                     True,  False),
    ("e.requires_grad",      dict(e_grad=True),                        False, False),
    ("base: wrong count",    dict(base_numel_off=1),                   True,  False),
    ("no base",              dict(base=False),                         True,  True),
    ("base on the CPU",      dict(base_cuda=False),                    True,  False),
    ("e on the CPU",         dict(e_cuda=False),                       False, False),
    ("e with three axes",    dict(e_extra_axis=True),                  False, False),
    ("lin1 of another K0",   dict(lin1_in_off=1),                      False, False),
    ("lin2 not 256 x 256",   dict(lin2_shape=(256, 128)),              False, False),
    ("lin_out of 128 columns", dict(out_in=128),                       True,  False),
]


@pytest.mark.parametrize("name,case,hidden,residual", PREDICATE_TABLE, ids=[r[0] for r in PREDICATE_TABLE])
def test_sim_fused_form_predicates(name, case, hidden, residual):
    from meshnet import graph_ops as go
    T, K0 = case.get("T", 3), case.get("K0", 13)
    shape = (T, K0, 1) if case.get("e_extra_axis") else (T, K0)
    e = _T(*shape, cuda=case.get("e_cuda", True), requires_grad=case.get("e_grad", False))
    lin1 = _lin(256, K0 + case.get("lin1_in_off", 0), case.get("bias1", True))
    lin2 = _lin(*case.get("lin2_shape", (256, 256)), case.get("bias2", True))
    lin_out = _lin(R_OUT, case.get("out_in", 256), case.get("bias_out", True))
    base = _T(T * R_OUT + case.get("base_numel_off", 0), cuda=case.get("base_cuda", True)) if case.get("base", True) else None
    assert go.sim_hidden_applies(e, lin1, lin2) is hidden
    assert go.sim_residual_applies(e, lin1, lin2, lin_out, base) is residual
