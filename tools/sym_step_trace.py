"""The launches of the equal-mass leapfrog step in a rocprofv3 --kernel-trace CSV of bench.py: per kind of launch (kick-drift,
diagonal blocks, storing / adding / single symmetric launch, finish) the durations, the GAPS between consecutive launches of
a step (end stamp to next start stamp), the span of a step (kick-drift start to finish end) and the gap to the next step.
   python tools/sym_step_trace.py <..._kernel_trace.csv> [label]
A step = the launches from one kick_drift_kernel up to the next finish_kernel; steps holding any other kernel are dropped."""
import csv
import statistics
import sys
from collections import defaultdict


def kind(name, wgs, first_sym):
    if "kick_drift_kernel" in name:
        return "kick-drift"
    if "finish_kernel" in name:
        return "finish"
    if "accel_sym" in name:
        return f"sym[{wgs}]" + ("" if not first_sym else " first")
    if "accel_kernel" in name:
        return "diagonal"
    return None


def stats(v):
    v = sorted(v)
    q = lambda f: v[min(len(v) - 1, int(f * len(v)))]
    return (f"n {len(v):5d}  mean {statistics.fmean(v):8.2f}  median {q(0.5):8.2f}  sd {statistics.pstdev(v):6.2f}  "
            f"p5 {q(0.05):8.2f}  p95 {q(0.95):8.2f}")


def main():
    rows = []
    with open(sys.argv[1], newline="") as f:
        for r in csv.DictReader(f):
            wgs = int(r["Grid_Size_X"]) // max(int(r["Workgroup_Size_X"]), 1)
            rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"], wgs))
    rows.sort()
    steps, cur = [], None
    for s, e, name, wgs in rows:
        if "kick_drift_kernel" in name:
            cur = []
        if cur is None:
            continue
        k = kind(name, wgs, not any(c[2].startswith("sym") for c in cur))
        if k is None:
            cur = None
            continue
        cur.append((s, e, k))
        if k == "finish":
            steps.append(cur)
            cur = None
    dur, gap, span, between = defaultdict(list), defaultdict(list), [], []
    for i, st in enumerate(steps):
        for j, (s, e, k) in enumerate(st):
            dur[k].append((e - s) / 1e3)
            if j:
                gap[f"{st[j - 1][2]} -> {k}"].append((s - st[j - 1][1]) / 1e3)
        span.append((st[-1][1] - st[0][0]) / 1e3)
        if i + 1 < len(steps):
            between.append((steps[i + 1][0][0] - st[-1][1]) / 1e3)
    label = sys.argv[2] if len(sys.argv) > 2 else sys.argv[1]
    print(f"== {label}: {len(steps)} steps, launches per step {sorted(set(len(s) for s in steps))}  (microseconds)")
    for k, v in dur.items():
        print(f"  duration {k:28s} {stats(v)}")
    for k, v in gap.items():
        print(f"  gap      {k:28s} {stats(v)}")
    tot_gap = [sum((st[j][0] - st[j - 1][1]) / 1e3 for j in range(1, len(st))) for st in steps]
    print(f"  gaps inside a step, summed          {stats(tot_gap)}")
    print(f"  step span (first start - last end)  {stats(span)}")
    # the next step's gap takes in whatever the host does between steps (bench.py's window bookkeeping): the median counts
    print(f"  gap to the next step                {stats(between)}")


if __name__ == "__main__":
    main()
