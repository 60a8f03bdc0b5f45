"""tests/golden/sim_hidden_parent_bits.npz: h1 / h2 of csplat_sim_hidden_fwd (T = 8) on the cases of tests/sim_rollout_ref.py:sim_hidden_case,
as raw float32 bits, from a build of the library at commit fe6a150 -- the last one whose k_sim_hidden_fwd applied ReLU as fmaxf(x, 0).
tests/test_sim_rollout_kernels_gpu.py holds the current kernel to these bits on finite data.  To regenerate (on an MI355X, from the
repository root):    CSPLAT_LIB=<libcsplat.so built from fe6a150> python tests/golden/make_sim_hidden_bits.py"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [os.path.join(ROOT, "cloth-splatting_amd"), os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402
import torch  # noqa: E402
import sim_rollout_ref as R  # noqa: E402
from csplat import native as n  # noqa: E402

out = {}
for K0 in R.SIM_HIDDEN_K0:
    e8, W1, b1, W2, b2, _ = R.sim_hidden_case(K0)
    e, W1c, b1c, W2c, b2c = (t.contiguous().cuda() for t in (e8, W1, b1, W2, b2))
    h1, h2 = torch.empty(8, 256, device="cuda"), torch.empty(8, 256, device="cuda")
    n.check(n.lib.csplat_sim_hidden_fwd(n.stream_handle(torch.device("cuda")), 8, K0, e.data_ptr(), W1c.data_ptr(), b1c.data_ptr(), W2c.data_ptr(),
                                        b2c.data_ptr(), h1.data_ptr(), h2.data_ptr()), "csplat_sim_hidden_fwd")
    out[f"h1_{K0}_8"] = h1.view(torch.int32).cpu().numpy()
    out[f"h2_{K0}_8"] = h2.view(torch.int32).cpu().numpy()
np.savez_compressed(os.path.join(HERE, "sim_hidden_parent_bits.npz"), **out)
print("wrote", len(out), "arrays from", n.LIB_PATH)
