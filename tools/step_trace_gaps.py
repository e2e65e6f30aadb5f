#!/usr/bin/env python3
"""The two chains of a rejected lone-chain step, from a rocprofv3 kernel trace of the benchmark.

Finish chain: from the start of a finish launch (k_step_finish*) to the start of the next one, and the gap between the end of one
and the start of the next.  Front chain: start-to-start distance of the first launches (k_step_begin*) that belong to consecutive
finish launches (a step's first launch is the last one that started before its finish launch; fronts dropped after an accepted
step have no finish launch and are left out).  With one finish launch per step (no twin passes) the records of the same command
(bench.py --dump-outputs, column 1: accepted) tell rejected from accepted steps: the interval behind step k is a rejected step's
if step k was rejected.  With twin passes a finish launch serves one or two steps: the intervals are tabulated by the kind of the
launch they start at (twin or one-lane) instead — and, given the records of EVERY step of the process (warm-up included) and the
lengths of its runs, by the step that was served LAST from the launch: the steps are laid along the finish launches from the first
one on (a twin launch serves lane 0 alone where lane 0 was accepted, lanes 0 and 1 where lane 0 was rejected: the lone chain's
harness always asks for the step lane 1 was made for), which tells the intervals behind "lane 1 used and accepted" — the pass whose
next first launch waits for lane 1's KL basis — from the others.

usage: step_trace_gaps.py <kernel_trace.csv> [records.npy] [label] [runs=<steps>,<steps>…]   (markdown on stdout)"""
import bisect
import csv
import statistics
import sys

rows = list(csv.DictReader(open(sys.argv[1])))
records = sys.argv[2] if len(sys.argv) > 2 and sys.argv[2].endswith(".npy") else None
labels = [a for a in sys.argv[2:] if not a.endswith(".npy") and not a.startswith("runs=")]
label = labels[0] if labels else "trace"


def spans(word):
    return sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), "twin" in r["Kernel_Name"]) for r in rows if word in r["Kernel_Name"])


begin, finish = spans("k_step_begin"), spans("k_step_finish")
begin_start = [b[0] for b in begin]
own_begin = [begin[max(bisect.bisect_left(begin_start, f[0]) - 1, 0)][0] for f in finish]  # the first launch of each finish launch's step(s)


def line(name, v):
    if not v:
        return "| %s | 0 | | | | |" % name
    v = sorted(v)
    return "| %s | %d | %.1f | %.1f | %.1f | %.1f |" % (name, len(v), statistics.median(v), v[len(v) // 10], v[(9 * len(v)) // 10],
                                                        sum(v) / len(v))


n = len(finish)
groups = {}
if records:
    import numpy as np
    acc = np.load(records)[:, 1] != 0
    if len(acc) <= n and not any(f[2] for f in finish):
        kind = [None] * (n - len(acc)) + ["accepted" if a else "rejected" for a in acc]  # (the timed steps are the last ones)
    else:
        records = None
if not records:
    kind = ["twin pass" if f[2] else "one-lane" for f in finish]
for k in range(n - 1):
    if kind[k] is None:
        continue
    g = groups.setdefault(kind[k], {"f2f": [], "gap": [], "b2b": []})
    g["f2f"].append((finish[k + 1][0] - finish[k][0]) / 1e3)
    g["gap"].append((finish[k + 1][0] - finish[k][1]) / 1e3)
    g["b2b"].append((own_begin[k + 1] - own_begin[k]) / 1e3)
print("# %s: intervals between the launches of consecutive steps\n" % label)
print("| interval (us), by the step / launch it starts at | count | median | p10 | p90 | mean |")
print("|---|---:|---:|---:|---:|---:|")
for key in sorted(groups):
    print(line("%s: begin start -> next begin start" % key, groups[key]["b2b"]))
    print(line("%s: finish start -> next finish start" % key, groups[key]["f2f"]))
    print(line("%s: finish end -> next finish start" % key, groups[key]["gap"]))
names = {}
for r in rows:
    nm = r["Kernel_Name"]
    if "k_step_" in nm:
        k = nm.split("k_step_")[1].split("(")[0].split("<")[0]
        names.setdefault(k, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)


def lay_steps(acc, runs):
    """-> {finish index: kind of the step served last from it}, or None where steps and launches do not come out even.  Forwards
    from the first launch: a twin launch serves lane 0 alone where lane 0 was accepted (or was the last step of its run: what is
    launched ahead is dropped there), lanes 0 and 1 where lane 0 was rejected."""
    ends, e = set(), 0
    for r in runs:
        e += r
        ends.add(e - 1)
    served, k = {}, 0
    for j, f in enumerate(finish):
        if k >= len(acc):
            return None
        if not f[2]:
            served[j] = "one-lane, " + ("accepted" if acc[k] else "rejected")
        elif acc[k] or k in ends:
            served[j] = "twin, lane 0 " + ("accepted" if acc[k] else "rejected (end of a run)")
        else:
            k += 1
            served[j] = "twin, lane 1 used and " + ("accepted" if acc[k] else "rejected")
        k += 1
    return served if k == len(acc) else None


runs = [a for a in sys.argv[3:] if a.startswith("runs=")]
if len(sys.argv) > 2 and sys.argv[2].endswith(".npy") and runs and any(f[2] for f in finish):
    import numpy as np
    served = lay_steps(list(np.load(sys.argv[2])[:, 1] != 0), [int(v) for v in runs[0][5:].split(",")])
    if served is None:
        print("\n(the records do not fit the finish launches: no table by the step served last)")
    else:
        by = {}
        for j, what in served.items():
            if j + 1 < n:
                by.setdefault(what, []).append((finish[j + 1][0] - finish[j][0]) / 1e3)
        print("\n| finish start -> next finish start (us), by the step served last from the launch | count | median | p10 | p90 | mean |")
        print("|---|---:|---:|---:|---:|---:|")
        for key in sorted(by):
            print(line(key, by[key]))
print("\n| launch | calls | avg us | median us |")
print("|---|---:|---:|---:|")
for k in sorted(names):
    print("| k_step_%s | %d | %.2f | %.2f |" % (k, len(names[k]), sum(names[k]) / len(names[k]), statistics.median(names[k])))
