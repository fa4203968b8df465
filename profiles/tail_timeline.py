#!/usr/bin/env python
"""kernel_trace.csv of `rocprofv3 --kernel-trace -- python bench.py --full --no-cpu --no-extras --step-only --steps N` ->
one line per kernel of the step: median start -> end in us from the start of the step's first kernel, over the last N - 1 steps
(a step ends with the K = 1 apply kernel).  `python profiles/tail_timeline.py kernel_trace.csv [N]`"""
import csv
import sys
from collections import defaultdict


def short(name):
    return name.split("(")[0].split("<")[0].replace("void ", "").replace("xr::", "").strip()


def med(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2]


def main():
    path, steps = sys.argv[1], int(sys.argv[2]) if len(sys.argv) > 2 else 10
    ker = sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), short(r["Kernel_Name"])) for r in csv.DictReader(open(path)))
    ends = [i for i, k in enumerate(ker) if k[2].startswith("k_apply_rows1") or k[2].startswith("k_apply_tail1")][-steps:]
    spans = defaultdict(list)
    lengths = []
    for a, b in zip(ends[:-1], ends[1:]):
        step = ker[a + 1:b + 1]
        t0 = step[0][0]
        seen = defaultdict(int)
        for s, e, name in step:
            seen[name] += 1
            spans[(name, seen[name])].append((s - t0, e - t0))
        lengths.append(step[-1][1] - ker[a][1])
    for (name, k), xs in sorted(spans.items(), key=lambda kv: med([x[0] for x in kv[1]])):
        s, e = med([x[0] for x in xs]) / 1e3, med([x[1] for x in xs]) / 1e3
        print("  %-26s %7.1f -> %7.1f  (dur %5.1f)%s" % (name + ("" if k == 1 else " #%d" % k), s, e, e - s, "" if len(xs) == len(lengths) else "  [%d of %d steps]" % (len(xs), len(lengths))))
    print("  step (end of apply to end of apply), median: %.1f us" % (med(lengths) / 1e3))


if __name__ == "__main__":
    main()
