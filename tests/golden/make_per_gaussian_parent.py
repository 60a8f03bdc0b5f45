"""tests/golden/per_gaussian_parent.npz: what K1 and the batched K8 computed before their global loads moved to the top of the kernels, on
the cases of tests/test_per_gaussian_round_trip_gpu.py (its docstring describes the scene and what is kept) -- from a build of the library
at commit a188511, the last one whose kernels read each input where it is used.  To regenerate (on an MI355X, from the repository root):
    CSPLAT_LIB=<libcsplat.so built from a188511> python tests/golden/make_per_gaussian_parent.py [output directory]"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [os.path.join(ROOT, "cloth-splatting_amd"), os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402
from csplat import native as n  # noqa: E402
import test_per_gaussian_round_trip_gpu as T  # noqa: E402

out = {}
for name, V, own, variant in T.cases_recorded():
    kw = T.VARIANTS[variant]
    cases, wts = T.scene(V, own=own)
    k1, got = T.step(cases, wts, own, **kw)
    if V == T.NV:
        T.check_scene_properties(k1)
    aa = bool(kw.get("aa"))
    for i, f in enumerate(k1):
        for k, a in f.items():
            key = T.k1_key(own, aa, i, k)
            if key in out:      # the same (means, antialiasing, view) in another case: K1 must have written the same bits
                assert np.array_equal(out[key], a), (name, key)
            out[key] = a
    for k, a in got.items():
        assert a.dtype == np.float32 and np.isfinite(a).all(), (name, k)
        if k == "sh":
            out["k8/%s/sh_crc" % name] = T.row_crc(a)
            if name == "default_V4_shared":
                out["k8/%s/sh" % name] = T.bits(a)
        else:
            out["k8/%s/%s" % (name, k)] = T.bits(a)
dest = os.path.join(sys.argv[1] if len(sys.argv) > 1 else HERE, "per_gaussian_parent.npz")
np.savez_compressed(dest, **out)
size = os.path.getsize(dest)
assert size < 1 << 20, size
print("wrote", len(out), "arrays,", size, "bytes, from", n.LIB_PATH)
