"""tests/golden/raster_grad_layout.json: the backward plans of the batched rasterizer Function on the pinned cases of
tests/test_raster_grad_layout_cpu.py (its docstring says what is kept), as `_RasterizeGaussiansBatch._plan_backward` made them at commit
67d9dc3 -- the last one where it decided, laid out and filled the csplat_view array in one loop and returned a dict.  No GPU: CPU tensors,
a zeroed csplat_view array, torch.device("cpu"); in the default mode `_acc_scratch` is the test module's CPU stub.  To regenerate, from
the repository root, with <parent> a directory that holds the package diff_gaussian_rasterization of that commit:
    PYTHONPATH=<parent> python tests/golden/make_raster_grad_layout.py [output directory]
(the test module is imported for its cases and readers only; what it reads of the package under test is not used here)"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path += [os.path.join(ROOT, "cloth-splatting_amd"), os.path.join(ROOT, "tests")]      # (behind PYTHONPATH: the parent's package wins)

import torch  # noqa: E402
from csplat import native  # noqa: E402
import diff_gaussian_rasterization as dgr  # noqa: E402
import test_raster_grad_layout_cpu as T  # noqa: E402

assert not hasattr(dgr, "_GradLayout"), "record from the parent's package, not from the code under test"
out = {}
for mode in (0, T.BIT_REPRODUCIBLE):
    table = out[str(mode)] = {}
    for c in T.pinned_cases():
        views, groups = T.view_records(c)
        saved = [t for v, g in zip(views, groups)
                 for t in (g[0], g[2], g[3], g[5], g[6], g[7], torch.zeros(v.P, dtype=torch.int32), torch.zeros(3, 16, 16))]
        arr = (native.CsplatView * c.V)()
        with T.flags(mode):
            plan = dgr._RasterizeGaussiansBatch._plan_backward(views, saved, 8, arr, T.first_of(groups), T.active_of(c), T.CPU)
        assert plan["active"] == T.active_of(c) and not plan["sinks"]
        table[c.name] = T.read_array(plan["sub"], len(plan["active"]), plan["big"], plan["out"])
dest = os.path.join(sys.argv[1] if len(sys.argv) > 1 else HERE, "raster_grad_layout.json")
with open(dest, "w") as f:
    f.write("{\n" + ",\n".join('"%s": {\n%s\n}' % (mode, ",\n".join('  "%s": %s' % (k, json.dumps(v)) for k, v in table.items()))
                               for mode, table in out.items()) + "\n}\n")
print(dest, os.path.getsize(dest), "bytes,", sum(len(t) for t in out.values()), "plans")
