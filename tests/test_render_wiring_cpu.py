"""The build's render() fed with the REFERENCE's own MultiGaussianMesh / Camera objects (INTEGRATION.md's promise).  The objects are
replayed from tests/golden/render_wiring_objects.npz: every attribute render() reads and every getter it calls, as the reference's
objects built from the seeded arrays of render_wiring.npz returned them (tests/golden/make_golden.py:gen_render_wiring_objects).
What the build hands the rasterizer must equal what the reference's render() handed it (render_wiring.npz), field by field."""
import types

import numpy as np
import torch

import util


def test_fixture_holds_the_references_wiring_facts():
    """facts of gaussian_renderer/__init__.py:49-164 the fixture must show (guards the generator, runs everywhere)"""
    G = util.golden("render_wiring.npz")
    fovx, fovy = float(G["in.cam_FoVx"]), float(G["in.cam_FoVy"])
    assert abs(float(G["default.settings.tanfovx"]) - np.tan(fovx * 0.5)) < 1e-12           # tan(FoV * 0.5), :56-57
    assert abs(float(G["default.settings.tanfovy"]) - np.tan(fovy * 0.5)) < 1e-12
    assert int(G["default.settings.sh_degree"]) == 2                                         # pc.active_sh_degree, not max (:70)
    assert float(G["scale_mod.settings.scale_modifier"]) == 1.7 and float(G["default.settings.scale_modifier"]) == 1.0
    assert bool(G["default.arg.colors_precomp.none"]) and not bool(G["default.arg.shs.none"])
    assert bool(G["override_color.arg.shs.none"]) and not bool(G["override_color.arg.colors_precomp.none"])     # :146-147
    np.testing.assert_array_equal(G["override_color.arg.colors_precomp"], G["in.override_color"])
    # python-covariance branch: scales None, cov3D given -- and rotations STILL passed (:83-88,156-164)
    assert bool(G["cov_python.arg.scales.none"]) and not bool(G["cov_python.arg.cov3D_precomp.none"]) and \
        not bool(G["cov_python.arg.rotations.none"])
    assert int(G["static.sim_calls"]) == 0 and int(G["default.sim_calls"]) == 1               # render_static skips the simulator
    np.testing.assert_array_equal(G["static.res.vertice_deform"], G["in.pos"])
    V = G["in.pos"].shape[0]
    assert G["default.sim_time_vector"].shape == (V, 1) and np.all(G["default.sim_time_vector"] == np.float32(G["in.cam_time"]))
    assert bool(G["default.res.vertice_projections.none"]) and not bool(G["project_vertices.res.vertice_projections.none"])
    assert all(bool(G[f"default.res.{f}.none"]) for f in ("shadows", "shadows_mean", "shadows_std"))
    assert float(np.abs(G["default.arg.means2D"]).max()) == 0.0


class _ReplayedMesh:
    """the reference's MultiGaussianMesh as render() sees it, replayed from the recording: getters of the deformed pose check that
    they are asked for the pose the reference's object was asked for"""

    def __init__(self, O):
        self.O = O
        self.active_sh_degree = int(O["pc.active_sh_degree"])
        self.mesh = types.SimpleNamespace(pos=self._t("pc.mesh.pos"))

    def _t(self, k):
        return torch.from_numpy(self.O[k].copy())

    def _posed(self, name, vertice_deform):
        if vertice_deform is None:
            return self._t(f"pc.{name}.rest")
        np.testing.assert_array_equal(vertice_deform.detach().numpy(), self.O["deformed"], err_msg=name)
        return self._t(f"pc.{name}.deformed")

    get_opacity = property(lambda self: self._t("pc.get_opacity"))
    get_scaling = property(lambda self: self._t("pc.get_scaling"))
    get_features = property(lambda self: self._t("pc.get_features"))

    def get_covariance(self, scaling_modifier=1.0):
        return self._t(f"pc.get_covariance.{float(scaling_modifier)}")

    def get_xyz(self, vertice_deform=None):
        return self._posed("get_xyz", vertice_deform)

    def get_rotation(self, vertice_deform=None):
        return self._posed("get_rotation", vertice_deform)


class _RecordingRasterizer:
    """stand-in for the HIP rasterizer: records the settings and every tensor render() hands it, returns zeros of the documented
    shapes (color [3,H,W], radii [P] int32, depth [1,H,W]) -- a test of the host-side wiring, not of the kernels"""
    calls = []

    def __init__(self, raster_settings):
        self.raster_settings = raster_settings

    def __call__(self, means3D, means2D, opacities, shs=None, colors_precomp=None, scales=None, rotations=None, cov3D_precomp=None):
        _RecordingRasterizer.calls.append((self.raster_settings, dict(means3D=means3D, means2D=means2D, opacities=opacities, shs=shs,
                                                                      colors_precomp=colors_precomp, scales=scales, rotations=rotations,
                                                                      cov3D_precomp=cov3D_precomp)))
        rs = self.raster_settings
        return (torch.zeros(3, rs.image_height, rs.image_width), torch.zeros(means3D.shape[0], dtype=torch.int32),
                torch.zeros(1, rs.image_height, rs.image_width))


WIRING_CASES = {"default": dict(), "scale_mod": dict(scaling_modifier=1.7), "override_color": dict(override_color=True),
                "static": dict(render_static=True), "project_vertices": dict(project_vertices=True), "cov_python": dict(pipe_cov=True)}


def test_build_render_accepts_reference_objects(monkeypatch):
    import gaussian_renderer as build_gr
    G, O = util.golden("render_wiring.npz"), util.golden("render_wiring_objects.npz")
    monkeypatch.setattr(build_gr, "GaussianRasterizer", _RecordingRasterizer)

    def close(a, b, tol=1e-6):
        a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
        return a.shape == b.shape and float(np.abs(a - b).max()) <= tol * (float(np.abs(b).max()) + 1e-30)

    def same_quats(a, b, tol):
        a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
        return float(np.abs(a * np.sign((a * b).sum(1, keepdims=True)) - b).max()) <= tol

    pos, wave = torch.from_numpy(G["in.pos"].copy()), torch.from_numpy(G["in.wave"].copy())
    for name, kw in WIRING_CASES.items():
        pc = _ReplayedMesh(O)
        cam = types.SimpleNamespace(**{a: (O[f"cam.{a}"].item() if O[f"cam.{a}"].ndim == 0 else torch.from_numpy(O[f"cam.{a}"].copy()))
                                       for a in ("image_height", "image_width", "FoVx", "FoVy", "time", "world_view_transform",
                                                 "full_proj_transform", "camera_center")})
        seen = []

        def simulator(time_vector):
            seen.append(time_vector.detach().clone())
            return pos + wave * time_vector            # [V,3] + [V,3] * [V,1]
        kw = dict(kw)
        pipe = types.SimpleNamespace(compute_cov3D_python=bool(kw.pop("pipe_cov", False)), convert_SHs_python=False, debug=False)
        if kw.get("override_color"):
            kw["override_color"] = torch.from_numpy(G["in.override_color"].copy())
        _RecordingRasterizer.calls.clear()
        res = build_gr.render(cam, pc, simulator, pipe, torch.from_numpy(G["in.bg"].copy()), **kw)
        assert len(_RecordingRasterizer.calls) == 1, name
        rs, args = _RecordingRasterizer.calls[0]
        g = lambda k: G[f"{name}.{k}"]  # noqa: E731
        for f in rs._fields:
            v = getattr(rs, f)
            v = v.detach().numpy() if torch.is_tensor(v) else np.asarray(v)
            assert close(v, g(f"settings.{f}"), 1e-12), (name, f, v, g(f"settings.{f}"))
        for k, v in args.items():
            assert (v is None) == bool(g(f"arg.{k}.none")), (name, k)
            if v is None:
                continue
            ok = same_quats(v.detach().numpy(), g(f"arg.{k}"), 5e-6) if k == "rotations" else close(v.detach().numpy(), g(f"arg.{k}"), 2e-6)
            assert ok, (name, k)
        assert len(seen) == int(g("sim_calls")) and (not seen or np.array_equal(seen[0].numpy(), g("sim_time_vector"))), name
        for f in res._fields:
            v = getattr(res, f)
            assert (v is None) == bool(g(f"res.{f}.none")), (name, f)
            if v is None or f in ("viewspace_points",):
                continue
            v = v.detach().numpy()
            if f == "rotations":
                assert same_quats(v, g("res.rotations"), 5e-6), name
            elif f in ("projections", "vertice_projections"):
                assert float(np.abs(v - g(f"res.{f}")).max()) < 2e-3, (name, f)
            else:
                assert close(v, g(f"res.{f}"), 2e-6), (name, f)
        assert res.viewspace_points.requires_grad and float(res.viewspace_points.abs().max()) == 0.0
