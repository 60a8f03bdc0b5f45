#!/usr/bin/env python3
"""tools/step_launch_stats.py <kernel_trace.csv>: the batched K1 and K8 rows of a rocprofv3 --kernel-trace run of bench.py, per population.
bench.py launches k_preprocess_views in full steps (forward + backward: a k_preprocess_bwd_views launch follows) and in forward-only calls
(the eager forward passes and checks around the timed window, on inputs the previous call left in the caches): the --stats row mixes both.
This prints average / min / max / std of K8, of the K1 launches that a K8 launch follows (the step's), and of the other K1 launches."""
import bisect
import csv
import sys
import numpy as np

rows = list(csv.DictReader(open(sys.argv[1])))
span = lambda key: sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"])) for r in rows if key in r["Kernel_Name"])  # noqa: E731
k1, k8 = span("k_preprocess_views<"), span("k_preprocess_bwd_views<")
starts = [s for s, _ in k1]
in_step = sorted({bisect.bisect_right(starts, s) - 1 for s, _ in k8})
dur = lambda xs: np.array([e - s for s, e in xs], np.float64)  # noqa: E731
for name, d in (("K8 k_preprocess_bwd_views", dur(k8)), ("K1 k_preprocess_views, in a step", dur([k1[i] for i in in_step])),
                ("K1 k_preprocess_views, forward only", dur([k1[i] for i in range(len(k1)) if i not in set(in_step)]))):
    if len(d):
        print("%-38s calls %4d  average %7.0f ns  min %6.0f  max %6.0f  std %5.0f" % (name, len(d), d.mean(), d.min(), d.max(), d.std()))
