"""The Delaunay triangulation without a GPU: the fixture and the Python restatement (tests/delaunay_ref.py) against SciPy and against the
definition in integers; the predicates of csrc/csplat_delaunay_predicates.h, compiled for the host, against integer arithmetic on
adversarial inputs; the library's surface (header block, exports, bindings); every argument error before the device is touched; and the
CPU behaviour that stays: a CPU tensor with delaunay=True raises NotImplementedError.

Every comparison is exact."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import util  # noqa: F401
import delaunay_ref as R
from csplat import native, triangulate
from meshnet import data_utils as du
from meshnet import gaussian_sampling

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cloth-splatting_amd", "csrc")
NAN = float("nan")


# ------------------------------------------------------------------------------------------------------- the fixture and the restatement
def test_fixture_is_a_fresh_scipy_run_without_ties():
    """the condition under which comparing with SciPy means anything: no four cocircular points, so the triangulation is unique"""
    pytest.importorskip("scipy.spatial")
    fix = R.load_fixture()
    assert sorted(fix) == [257, 300, 2048]
    for (n, seed) in R.FIXTURE_CLOUDS:
        pts, faces = fix[n]
        assert pts.dtype == np.float32 and pts.shape == (n, 2) and np.array_equal(pts, R.fixture_cloud(n, seed))
        assert np.array_equal(faces, R.scipy_faces(pts))
        assert R.check(pts, faces) == 0
    assert os.path.getsize(R.GOLDEN) < 200 * 1024


def test_walk_is_the_definition_on_degenerate_clouds():
    ties = {}
    for name, (pts, _skipped) in R.degenerate_clouds().items():
        faces = R.walk(pts)
        ties[name] = R.check(pts, faces)
        assert faces == R.canonical(faces, R.to_ints(pts)), name                # lowest index first, counter-clockwise, sorted
    assert ties["square"] == 1 and ties["collinear4"] == 0 and ties["grid9"] == ties["grid9_permuted"] == 64 and ties["grid17"] == 256
    assert ties["grid8_small"] == 49 and ties["circle65"] == 33 and ties["hull_collinear"] > 0
    assert R.walk(R.degenerate_clouds()["collinear4"][0]) == []
    assert R.walk(R.degenerate_clouds()["square"][0]) == [(0, 1, 3), (1, 2, 3)]  # eps_0 largest: point 0 is lifted out of the circle of 1, 2, 3
    dup, skipped = R.degenerate_clouds()["duplicates_nan"]
    assert skipped == 5 and sum(not m for m in R.usable(dup)[1]) == 5
    used = {v for f in R.walk(dup) for v in f}
    assert used == {i for i, m in enumerate(R.usable(dup)[1]) if m} and not used & {7, 19, 33, 25, 30}


def test_walk_equals_scipy_where_there_are_no_ties():
    pytest.importorskip("scipy.spatial")
    fix = R.load_fixture()
    for n in (257, 300):
        pts, faces = fix[n]
        assert R.walk(pts) == [tuple(f) for f in faces.tolist()]
    for name, pts in R.size_clouds().items():
        faces = R.walk(pts)
        assert R.check(pts, faces) == 0, name
        if len(pts) >= 3:
            assert faces == [tuple(f) for f in R.scipy_faces(pts).tolist()], name
        else:
            assert faces == []


def test_threshold_loop_and_gap():
    pts, faces = R.load_fixture()[257]
    thr = R.gap_threshold(pts, faces)
    edges, kept = R.threshold_loop(pts, faces, thr)
    every, all_faces = R.threshold_loop(pts, faces, None)
    assert every == R.edges_of(faces) and len(all_faces) == len(faces)
    assert 0 < len(edges) < len(every) and 0 < len(kept) < len(faces)
    # float32 lengths fall on the same side of a threshold taken from a gap
    p = pts.astype(np.float32)
    for a, b in every:
        d = p[a] - p[b]
        assert (np.sqrt(d[0] * d[0] + d[1] * d[1]) > np.float32(thr)) == ((a, b) not in set(edges))


# --------------------------------------------------------------------------------------------------------------- the predicates, on the host
def test_host_predicates_equal_integer_arithmetic(tmp_path):
    """csplat_delaunay_predicates.h compiled by the host compiler into a stand-alone program: every sign equals the integers', perturbed
    ties included, from denormals to 1e30.  A failed compile is a failure."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "delaunay_predicates_main")
    subprocess.run([cxx, "-O2", "-std=c++17", "-ffp-contract=off", "-I", CSRC, os.path.join(ROOT, "tests", "delaunay_predicates_main.cpp"), "-o", exe],
                   check=True)
    rec = R.adversarial_records()
    (tmp_path / "records.bin").write_bytes(R.pack_records(rec))
    subprocess.run([exe, str(tmp_path / "records.bin"), str(tmp_path / "signs.bin")], check=True)
    got = np.fromfile(str(tmp_path / "signs.bin"), np.int32).reshape(-1, 2)
    want = np.array(R.expected_signs(rec), np.int32)
    assert got.shape == (len(rec), 2) and len(rec) > 4000
    wrong = np.flatnonzero(got[:, 0] != want)
    assert wrong.size == 0, [(rec[i][0], rec[i][1], rec[i][2].tolist(), int(got[i, 0]), int(want[i])) for i in wrong[:5]]
    kinds = np.array([r[0] for r in rec])
    # the inputs do what they are for: each predicate has exact zeros, decisions of the exact stage, and decisions the filter takes alone;
    # an in-circle tie is always broken (0 only when all four points are collinear)
    for kind in (R.ORIENT, R.NEARER, R.INCIRCLE):
        sel = kinds == kind
        assert got[sel, 1].sum() > 100 and (got[sel, 1] == 0).sum() > 100, kind
    assert (want[kinds == R.ORIENT] == 0).sum() > 50 and (want[kinds == R.NEARER] == 0).sum() > 50
    tied = [i for i in np.flatnonzero(kinds == R.INCIRCLE) if R.incircle_det(*R.to_ints(rec[i][2])) == 0]
    assert len(tied) > 200 and all(got[i, 1] == 1 for i in tied)
    assert sum(want[i] > 0 for i in tied) > 50 and sum(want[i] < 0 for i in tied) > 50


# ------------------------------------------------------------------------------------------------------------------ the library's surface
ENTRIES = (("int", "csplat_delaunay_temp_bytes", 2), ("int", "csplat_delaunay", 9))


def test_header_exports_and_bindings():
    header = open(os.path.join(ROOT, "include", "csplat.h")).read()
    for res, name, n_args in ENTRIES:
        assert name in native.EXPORTS and hasattr(native.lib, name) and len(native.EXPORTS[name][1]) == n_args
        decl = header[header.index(res + " " + name + "("):]
        decl = re.sub(r"/\*.*?\*/", "", decl[:decl.index(";")], flags=re.S)
        assert decl.count(",") + 1 == n_args, (name, decl)
    assert header.index("/* Observation clouds") < header.index("/* Trajectory preprocessing") < header.index("/* Delaunay triangulation")
    block = header[header.index("/* Delaunay triangulation"):header.index("int csplat_delaunay_temp_bytes(")]
    assert block.rstrip().endswith("Added exports: CSPLAT_ABI_VERSION is unchanged. */")
    flat = re.sub(r"\s*\n \*\s*", " ", block)
    for word in ("meshnet/data_utils.py:371-405", ":419-440", "gaussian_mesh.py:52,204", "0 <= N < 2^24", "-0.0 == 0.0", "strictly inside",
                 "eps_0 >> eps_1", "first non-zero cofactor", "ascending point index", "+orient(b,c,d), -orient(a,c,d), +orient(a,b,d), -orient(a,b,c)",
                 "a collinear triple is never a face", "zero faces, no error", "ties to the lower index", "lowest index", "exact predicate",
                 "denormals", "two-sum", "explicit fma", "No float atomics", "bit-reproducible", "sqrtf(du*du + dv*dv)", "len > (float)norm_threshold",
                 "a NaN threshold is an error", "sorted by (i, j)", "lexicographic", "exceeded N steps", "fixed order"):
        assert word.lower() in flat.lower(), word
    assert native.ABI_VERSION == 9 and native.lib.csplat_abi_version() == 9
    src = open(os.path.join(CSRC, "csplat_delaunay.hip")).read()
    code = re.sub(r"//.*", "", src)
    assert '#include "csplat_delaunay_predicates.h"' in code and "#pragma clang fp contract(off)" in code
    assert [a for a in re.findall(r"\batomic\w*", code)] == ["atomicOr"] and "csplat_inclusive_scan_u32(" in code
    pred = re.sub(r"//.*", "", open(os.path.join(CSRC, "csplat_delaunay_predicates.h")).read())
    assert "#pragma clang fp contract(off)" in pred and pred.count("__builtin_fma(") == 1 and "__host__ __device__" in pred
    assert "float" not in pred.replace("float32", "")                           # fp64 throughout


def test_the_library_refuses_bad_arguments_before_any_launch():
    """fake, distinct, aligned addresses 2^32 apart: every call here is refused before a launch could touch them"""
    L = native.lib
    A = lambda i: (i + 1) << 32  # noqa: E731
    size = C.c_size_t(0)
    for n in (-1, 2 ** 24):
        assert L.csplat_delaunay_temp_bytes(n, C.byref(size)) == 2 and b"csplat_delaunay_temp_bytes" in L.csplat_last_error()
    assert L.csplat_delaunay_temp_bytes(10, None) == 2
    assert L.csplat_delaunay_temp_bytes(0, C.byref(size)) == 0 and size.value == 0
    assert L.csplat_delaunay_temp_bytes(300, C.byref(size)) == 0 and triangulate.temp_bytes(300) == size.value
    # ok u8[N], counts and scan u32[2N], exact u32[N], faces int2[2N], edges int[3N], the slabs int2[16N] and int[16N], each rounded up to
    # 256, and the scan's own scratch
    raw = 300 + 2 * 2400 + 1200 + 4800 + 3600 + 38400 + 19200
    assert raw <= size.value <= raw + 10 * 256 + 1024
    assert L.csplat_delaunay_temp_bytes(2 ** 24 - 1, C.byref(size)) == 0 and size.value > 2 ** 24 * 240
    dl = lambda N=100, pts=A(0), has=0, thr=0.0, faces=A(1), edges=A(2), counters=A(3), temp=A(4): \
        L.csplat_delaunay(None, N, pts, has, thr, faces, edges, counters, temp)  # noqa: E731
    for kw in (dict(N=-1), dict(N=2 ** 24), dict(has=2), dict(has=-1), dict(has=1, thr=NAN), dict(pts=None), dict(faces=None), dict(edges=None),
               dict(counters=None), dict(temp=None), dict(pts=A(0) + 4), dict(faces=A(1) + 2), dict(edges=A(2) + 1), dict(counters=A(3) + 4),
               dict(temp=A(4) + 128), dict(faces=A(0)), dict(edges=A(0) + 792), dict(counters=A(0) + 8), dict(temp=A(0) + 512), dict(edges=A(1) + 2396),
               dict(counters=A(1) + 2392), dict(temp=A(1) + 2304), dict(counters=A(2) + 16), dict(temp=A(2) + 2304), dict(counters=A(4) + 1024),
               dict(N=0, counters=None), dict(N=0, counters=A(3) + 4)):
        assert dl(**kw) == 2, kw
        assert b"csplat_delaunay" in L.csplat_last_error() and b"temp_bytes" not in L.csplat_last_error(), kw


def test_argument_errors_come_before_the_device():
    """CPU tensors: a ValueError for every malformed argument; a well-formed request on a CPU tensor is refused as a CPU tensor"""
    ok = torch.zeros(10, 2)
    for bad in (np.zeros((10, 2), np.float32), [[0.0, 1.0]], torch.zeros(10, 3), torch.zeros(10), torch.zeros(2, 10, 2),
                torch.zeros(10, 2, dtype=torch.float64), torch.zeros(10, 2, dtype=torch.int32)):
        with pytest.raises(ValueError, match="delaunay"):
            triangulate.delaunay(bad)
    for thr in (NAN, "x", [1.0]):
        with pytest.raises(ValueError, match="norm_threshold"):
            triangulate.delaunay(ok, thr)
    with pytest.raises(ValueError, match="2\\^24"):
        triangulate.delaunay(torch.empty(2 ** 24, 2))
    with pytest.raises(native.CsplatError, match="GPU"):
        triangulate.delaunay(ok)
    with pytest.raises(native.CsplatError, match="GPU"):
        triangulate.delaunay(ok, 0.5)
    pts = torch.zeros(10, 3)
    for fn in (lambda p: du.compute_edges_index(p, delaunay=True), du.compute_mesh, gaussian_sampling.get_mesh):
        for bad in (torch.zeros(10, 2), np.zeros((10, 4)), torch.zeros(10)):
            with pytest.raises(ValueError, match=r"\[N, 3\]"):
                fn(bad)
    with pytest.raises(ValueError, match="norm_threshold"):
        du.compute_edges_index(pts, delaunay=True, norm_threshold=NAN)
    with pytest.raises(ValueError, match="norm_threshold"):
        du.process_traj(torch.zeros(2, 10, 3), 0.05, delaunay=True, norm_threshold=NAN)
    from csplat.gaussians import MeshGaussians
    with pytest.raises(native.CsplatError):
        MeshGaussians(0).from_vertices(pts)


def test_cpu_tensors_still_raise_with_the_scipy_advice():
    pts, traj = torch.rand(12, 3), torch.rand(3, 12, 3)
    for call in (lambda: du.compute_edges_index(pts, k=3, delaunay=True), lambda: du.compute_edges_index(pts.double(), delaunay=True, sim_data=True),
                 lambda: du.process_traj(traj, 0.05, delaunay=True), lambda: du.compute_mesh(pts), lambda: gaussian_sampling.get_mesh(pts)):
        with pytest.raises(NotImplementedError, match="SciPy"):
            call()
    obs = {"pos": traj, "gripper_pos": torch.rand(3, 3), "pick": torch.rand(3), "place": torch.rand(3), "actions": torch.rand(3, 3)}
    with pytest.raises(NotImplementedError, match="SciPy"):
        du.get_data_traj(None, None, (0.05, 3, True, False, 300, 1, 1), observations=obs, rw_processing=False)
    # an explicit edge_index wins: nothing is triangulated, so nothing is refused; delaunay=False is untouched
    ei = torch.tensor([[0, 1], [1, 2]])
    d = du.process_traj(traj, 0.05, delaunay=True, edge_index=ei)
    plain = du.process_traj(traj, 0.05, delaunay=False, edge_index=ei)
    assert d["edge_faces"] is None and all(torch.equal(d[k], plain[k]) for k in ("pos", "velocity", "edge_index", "edge_displacement", "edge_norm"))


def test_a_status_word_raises():
    """what the binding makes of the counters: the first rows of the buffers, or CsplatError when a walk gave up"""
    faces, edges = torch.arange(12, dtype=torch.int32).reshape(4, 3), torch.arange(12, dtype=torch.int32).reshape(6, 2)
    t = triangulate._result(faces, edges, torch.tensor([2, 3, 1, 7, 0]))
    assert t.faces.tolist() == [[0, 3], [1, 4], [2, 5]] and t.edge_index.tolist() == [[0, 2, 4], [1, 3, 5]] and t[2:] == (1, 7)
    assert t.faces.dtype == t.edge_index.dtype == torch.int64
    for status, why in ((1, "exceeded N steps"), (2, "disagree"), (3, "exceeded N steps")):
        with pytest.raises(native.CsplatError, match=f"status={status}.*{why}"):
            triangulate._result(faces, edges, torch.tensor([2, 3, 0, 0, status]))


def test_sample_gaussian_means_is_the_barycentric_sum():
    rng = np.random.default_rng(0)
    tv, bc = rng.random((7, 3, 3)), rng.random((4, 7, 3))
    want = np.einsum("smv,mvc->smc", bc, tv)
    got = gaussian_sampling.sample_gaussian_means(tv, bc, 4)
    assert isinstance(got, np.ndarray) and got.shape == (4, 7, 3) and np.abs(got - want).max() < 1e-15
    got_t = gaussian_sampling.sample_gaussian_means(torch.from_numpy(tv), torch.from_numpy(bc), 4)
    assert torch.is_tensor(got_t) and np.array_equal(got_t.numpy(), got)
    with pytest.raises(ValueError):
        gaussian_sampling.sample_gaussian_means(tv, bc, 3)
