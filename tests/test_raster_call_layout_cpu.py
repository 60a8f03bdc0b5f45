"""The call layout of the batched rasterizer Function (diff_gaussian_rasterization._CallLayout): which tensor argument, which output and
which entry of backward's return value belongs to which view.  No GPU and no library call: placeholder tensors stand in for the inputs,
distinct sentinels for the outputs and gradients.  A gradient handed to the wrong input is silent on the GPU; here it is an assertion."""
import itertools

import pytest
import torch

import diff_gaussian_rasterization as dgr
from diff_gaussian_rasterization import GaussianRasterizationSettings, Visibility, _CallLayout, _call_layout

NIN = 8
NAMES = ("color", "radii", "depth", "feat", "alpha") + Visibility._fields
FEATS = {"none": lambda i: (0, False), "F2": lambda i: (2, False), "alpha_some": lambda i: (0, i % 2 == 0),
         "F2_alpha_some": lambda i: (2, i % 2 == 0)}
VIS = {"none": lambda i: False, "all": lambda i: True, "some": lambda i: i % 3 == 0}
# the number of tensor arguments of apply(), as the Function has taken them since each option was added: 8 per view, + 4 per view when a
# settings tensor wants a gradient, + 1 per view when any view asks for features or alpha; antialiasing and visibility add none
EXPECTED_ARGS = {
    ("default", 1): 8, ("default", 2): 16, ("default", 3): 24, ("default", 9): 72,
    ("camera", 1): 12, ("camera", 2): 24, ("camera", 3): 36, ("camera", 9): 108,
    ("features", 1): 9, ("features", 2): 18, ("features", 3): 27, ("features", 9): 81,
    ("all", 1): 13, ("all", 2): 26, ("all", 3): 39, ("all", 9): 117,
}


def _settings(V, requires_grad=False):
    t = lambda *s: torch.zeros(*s, requires_grad=requires_grad)      # noqa: E731
    return [GaussianRasterizationSettings(8, 8, 1.0, 1.0, t(3), 1.0, t(4, 4), t(4, 4), 3, t(3), False, False) for _ in range(V)]


def _cases():
    for V, stacked, cam, aa, f, v in itertools.product((1, 2, 3, 9), (False, True), (False, True), (False, True), FEATS, VIS):
        yield V, stacked, cam, aa, f, v


def _layout(V, stacked, cam, aa, f, v):
    return _CallLayout(_settings(V), stacked, cam, aa, [FEATS[f](i) for i in range(V)], [VIS[v](i) for i in range(V)])


def _has(L, i, name):
    """what the documentation of rasterize_views promises view i"""
    F, alpha = L.feat[i]
    return {"color": not L.stacked, "radii": True, "depth": True, "feat": F > 0, "alpha": alpha}.get(name, L.vis[i])


def test_inputs_round_trip_and_indices_are_a_bijection():
    for case in _cases():
        L = _layout(*case)
        V = L.V
        inputs = [tuple(torch.zeros(1) for _ in range(NIN)) for _ in range(V)]
        feats = [torch.zeros(1) if L.feat[i][0] else None for i in range(V)]
        tensors = L.pack(inputs, feats)
        assert len(tensors) == L.n_tensors, case
        seen = []
        for i in range(V):
            got = L.view_inputs(tensors, i)
            assert len(got) == NIN and all(a is b for a, b in zip(got, inputs[i])), case
            for slot in range(NIN):
                assert tensors[L.index(i, slot)] is inputs[i][slot], case
                seen.append(L.index(i, slot))
            cam = dgr._cam_tensors(L.settings[i])
            if L.cam:
                got = L.cam_group(tensors, i)
                assert len(got) == 4 and all(a is b for a, b in zip(got, cam)), case
                for k in range(4):
                    assert tensors[L.cam_index(i, k)] is cam[k], case
                    seen.append(L.cam_index(i, k))
            else:
                assert len(L.cam_group(tensors, i)) == 0 and all(L.cam_index(i, k) is None for k in range(4)), case
            if L.has_feat:
                assert L.features(tensors, i) is feats[i] and tensors[L.feat_index(i)] is feats[i], case
                seen.append(L.feat_index(i))
            else:
                assert L.features(tensors, i) is None and L.feat_index(i) is None, case
        assert sorted(seen) == list(range(L.n_tensors)), case


def test_output_indices_partition_the_outputs():
    for case in _cases():
        L = _layout(*case)
        seen = [] if L.stacked_output is None else [L.stacked_output]
        assert (L.stacked_output == 0) if L.stacked else (L.stacked_output is None), case
        for i in range(L.V):
            for name in NAMES:
                j = L.outputs[i].get(name)
                assert (j is not None) == _has(L, i, name), (case, i, name)
                assert L.output(list(range(L.n_outputs)), i, name) == j, (case, i, name)
                if j is not None:
                    seen.append(j)
        assert sorted(seen) == list(range(L.n_outputs)), case


def test_split_returns_the_documented_order():
    for case in _cases():
        L = _layout(*case)
        res = tuple(object() for _ in range(L.n_outputs))
        if L.stacked:
            res = (tuple(object() for _ in range(L.V)),) + res[1:]       # (the stacked colours: indexed per view)
        got = L.split(res)
        rest = iter(res[1:] if L.stacked else res)
        if L.stacked:
            assert isinstance(got, tuple) and len(got) == 2 and got[0] is res[0], case
            got = got[1]
        assert isinstance(got, list) and len(got) == L.V, case
        for i, view in enumerate(got):
            F, alpha = L.feat[i]
            want = [res[0][i] if L.stacked else next(rest), next(rest), next(rest)]      # colour, radii, depth
            want += [next(rest) for flag in (F > 0, alpha) if flag]                      # feat, alpha
            assert isinstance(view, tuple) and len(view) == len(want) + (1 if L.vis[i] else 0), (case, i)
            assert all(a is b for a, b in zip(view, want)), (case, i)
            if L.vis[i]:                                                                 # Visibility, last
                vis = view[-1]
                assert isinstance(vis, Visibility) and all(a is next(rest) for a in vis), (case, i)
        assert next(rest, None) is None, case


def test_backward_return_puts_each_gradient_at_its_input():
    for case in _cases():
        L = _layout(*case)
        V = L.V
        assert L.grads() == (None,) * (1 + L.n_tensors), case
        per = [[object() for _ in range(NIN)] if i % 2 == 0 else None for i in range(V)]
        per[0][3] = None
        cam = [tuple(object() for _ in range(4)) if i % 3 != 1 else None for i in range(V)] if L.cam else None
        feat = [object() if i != 1 else None for i in range(V)] if L.has_feat else None
        for kw in ({"per_gaussian": per}, {"cam": cam}, {"feat": feat}, {"per_gaussian": per, "cam": cam, "feat": feat}):
            out = L.grads(**kw)
            assert isinstance(out, tuple) and len(out) == 1 + L.n_tensors, case
            want = [None] * (1 + L.n_tensors)
            for i in range(V):
                if kw.get("per_gaussian") is not None and per[i] is not None:
                    for slot in range(NIN):
                        want[1 + L.index(i, slot)] = per[i][slot]
                if kw.get("cam") is not None and cam[i] is not None:
                    for k in range(4):
                        want[1 + L.cam_index(i, k)] = cam[i][k]
                if kw.get("feat") is not None:
                    want[1 + L.feat_index(i)] = feat[i]
            assert all(a is b for a, b in zip(out, want)), (case, list(kw))


@pytest.mark.parametrize("V", (1, 2, 3, 9))
def test_tensor_argument_counts_are_the_ones_of_before(V):
    every = [(2, i % 2 == 0) for i in range(V)]
    none = [(0, False)] * V
    for stacked in (False, True):
        assert _CallLayout(_settings(V), stacked, False, False, none, [False] * V).n_tensors == EXPECTED_ARGS["default", V]
        assert _CallLayout(_settings(V), stacked, True, False, none, [False] * V).n_tensors == EXPECTED_ARGS["camera", V]
        assert _CallLayout(_settings(V), stacked, False, False, every, [False] * V).n_tensors == EXPECTED_ARGS["features", V]
        assert _CallLayout(_settings(V), stacked, True, True, every, [True] * V).n_tensors == EXPECTED_ARGS["all", V]
        # antialiasing and visibility are no tensor arguments; alpha alone brings the (empty) feature group, as it always did
        assert _CallLayout(_settings(V), stacked, False, True, none, [True] * V).n_tensors == EXPECTED_ARGS["default", V]
        assert _CallLayout(_settings(V), stacked, False, False, [(0, i == 0) for i in range(V)], [False] * V).n_tensors == \
            EXPECTED_ARGS["features", V]


def test_builder_passes_the_camera_groups_only_for_a_wanted_gradient():
    none, vis = [(0, False)] * 2, [False] * 2
    assert not _call_layout(_settings(2), False, False, none, vis).cam
    mixed = [_settings(1)[0], _settings(1, requires_grad=True)[0]]
    assert _call_layout(mixed, False, False, none, vis).cam
    with torch.no_grad():
        assert not _call_layout(mixed, False, False, none, vis).cam
    with pytest.raises(ValueError, match="same number of feature channels"):
        _call_layout(_settings(2), False, False, [(2, False), (3, False)], vis)


def test_saved_tensors_round_trip_and_indices_are_a_bijection():
    """the saved order: per view means3D, sh, colors_precomp, scales, rotations, cov3Ds_precomp, radii and -- unless stacked -- its colour;
    then the stacked colours; then, when a view asks for features or alpha, the views' feature tensors"""
    names = ("means3D", "sh", "colors_precomp", "scales", "rotations", "cov3Ds_precomp", "radii", "color")
    for case in _cases():
        L = _layout(*case)
        V = L.V
        per_view = [tuple(object() for _ in names) for _ in range(V)]
        colors = [v[-1] for v in per_view] if L.stacked else None        # (the stacked colours: row i is view i's colour)
        feats = [object() if L.feat[i][0] else None for i in range(V)]
        saved = L.pack_saved(per_view, colors, feats)
        assert len(saved) == L.n_saved == V * (7 if L.stacked else 8) + (1 if L.stacked else 0) + (V if L.has_feat else 0), case
        seen = []           # positions of the saved list the accessors reach: together every one, each once
        where = lambda t: next(j for j, u in enumerate(saved) if u is t)      # noqa: E731
        for i in range(V):
            for name, want in zip(names, per_view[i]):
                got = L.saved_input(saved, i, name)
                if name == "color" and L.stacked:
                    assert got is colors and got[i] is want and where(got) == V * 7, case
                    seen += [where(got)] if i == 0 else []
                else:
                    assert got is want, (case, i, name)
                    seen.append(where(got))
        got = L.saved_features(saved)
        if L.has_feat:
            assert len(got) == V and all(a is b for a, b in zip(got, feats)), case
            seen += range(L.n_saved - V, L.n_saved)
        else:
            assert len(got) == 0, case
        assert sorted(seen) == list(range(L.n_saved)), case
