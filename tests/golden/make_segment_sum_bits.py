"""tests/golden/segment_sum_parent_bits.npz: csplat_gnn_segment_sum on the cases of tests/test_gnn_kernels_gpu.py:_parent_cases (five graph
shapes on 300 nodes, widths 32 and 6, ordinary / cancelling / zero messages), as raw float32 bits, from a build of the library at commit
f37f7e8 -- the last one whose k_segment_sum returned acc + comp whatever acc was.  tests/test_gnn_kernels_gpu.py holds the current kernel
to these bits: every finite sum is unchanged.  To regenerate (on an MI355X, from the repository root):
    CSPLAT_LIB=<libcsplat.so built from f37f7e8> python tests/golden/make_segment_sum_bits.py [output directory]"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [os.path.join(ROOT, "cloth-splatting_amd"), os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402
import torch  # noqa: E402
from csplat import native as n  # noqa: E402
import test_gnn_kernels_gpu as T  # noqa: E402

out = {}
for name, ei, L, msg in T._parent_cases():
    rowptr, perm = n.group_by_key(ei[1].cuda(), 300)
    m, agg = msg.cuda(), torch.empty(300, L, device="cuda")
    n.check(n.lib.csplat_gnn_segment_sum(n.stream_handle(torch.device("cuda")), 300, m.shape[0], L, m.data_ptr(), rowptr.data_ptr(),
                                         perm.contiguous().data_ptr(), agg.data_ptr()), "csplat_gnn_segment_sum")
    assert bool(torch.isfinite(agg).all())
    out[name] = agg.view(torch.int32).cpu().numpy()
dest = sys.argv[1] if len(sys.argv) > 1 else HERE
np.savez_compressed(os.path.join(dest, "segment_sum_parent_bits.npz"), **out)
print("wrote", len(out), "arrays from", n.LIB_PATH)
