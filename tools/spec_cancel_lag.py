#!/usr/bin/env python3
"""Lag of the eigen stream behind accepted steps, from a rocprofv3 kernel trace of the lone-chain benchmark.

For every accepted step k: the time from the start of its k_step_finish launch (its regression has ended) to the start of the
k_posterior_eigen_rr launch that decomposes its posterior, tabulated by what came before step k (an accepted step, or a run of
1, 2, 3+ rejected ones).  The decomposition of an accepted step is the eigen launch that ended last before the NEXT step's finish
launch started: that step's front draws from its basis, and a later speculative launch cannot end before that step's own regression.
A decomposition that is launched ahead of its input starts BEFORE the finish launch and waits inside (negative lag: the stream was
free); a positive lag is time the accepted step spends behind earlier launches of the stream.

usage: spec_cancel_lag.py <kernel_trace.csv> <records.npy of the same command> [label]   (markdown table on stdout)
The records are those of bench.py --dump-outputs (column 1: accepted); the chain is deterministic, so an untraced run's serve."""
import bisect
import csv
import statistics
import sys

import numpy as np

rows = list(csv.DictReader(open(sys.argv[1])))
acc = np.load(sys.argv[2])[:, 1] != 0
label = sys.argv[3] if len(sys.argv) > 3 else "lag"
fin = sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"])) for r in rows if "k_step_finish" in r["Kernel_Name"])
eig = sorted((int(r["End_Timestamp"]), int(r["Start_Timestamp"])) for r in rows if "k_posterior_eigen_rr" in r["Kernel_Name"])
fin = fin[len(fin) - len(acc):]  # the timed steps are the last ones (the warm-up's come first)
assert len(fin) == len(acc), "fewer finish launches than records"
eig_end = [e[0] for e in eig]
groups = {"accepted": [], "1 rejected": [], "2 rejected": [], "3+ rejected": []}
dur = {k: [] for k in groups}
run = 0  # rejected steps in a row before step k
for k in range(len(acc) - 1):
    if acc[k]:
        j = bisect.bisect_left(eig_end, fin[k + 1][0]) - 1
        if j >= 0 and eig[j][0] > fin[k][0]:  # (it ended after this step's finish started: it is this step's)
            key = "accepted" if run == 0 else ("%d rejected" % run if run < 3 else "3+ rejected")
            groups[key].append((eig[j][1] - fin[k][0]) / 1e3)
            dur[key].append((eig[j][0] - eig[j][1]) / 1e3)
        run = 0
    else:
        run += 1
print("| before the accepted step | steps | %s: median us | p10 | p90 | share > 5 us | launch duration, median us |" % label)
print("|---|---:|---:|---:|---:|---:|---:|")
for key, v in groups.items():
    if not v:
        print("| %s | 0 | | | | | |" % key)
        continue
    v.sort()
    print("| %s | %d | %.1f | %.1f | %.1f | %.0f %% | %.1f |" % (key, len(v), statistics.median(v), v[len(v) // 10], v[(9 * len(v)) // 10],
                                                              100.0 * sum(x > 5.0 for x in v) / len(v), statistics.median(dur[key])))
