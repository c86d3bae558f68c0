"""Reduce a `rocprofv3 --kernel-trace` of tools/msda_window_bench.py to launch times per window-kernel form and burst: the tool
alternates the fill schedules, and then the lane layouts, burst by burst, so consecutive launches of one instantiation are one
burst, and bursts of the two schedules (or the two layouts) of a form that follow one another are a pair.

    python tools/msda_window_trace.py <kernel_trace.csv>"""
import collections
import csv
import re
import sys


def main():
    rows = []
    for r in csv.DictReader(open(sys.argv[1])):
        m = re.search(r"msda_window_kernel<([^>]*)>", r["Kernel_Name"])
        if m:
            p = [x.strip() for x in m.group(1).split(",")]
            rows.append((int(r["Start_Timestamp"]), "level-%s tiles" % p[5], (int(p[6]) if len(p) > 6 else 0, int(p[7]) if len(p) > 7 else 8),
                         (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-3))
    rows.sort()
    bursts = collections.defaultdict(list)                   # form -> [((schedule, lanes per pair), [us])] in time order
    for _, form, key, us in rows:
        b = bursts[form]
        if b and b[-1][0] == key:
            b[-1][1].append(us)
        else:
            b.append((key, [us]))
    for form in sorted(bursts):
        seq = [(s, sum(v) / len(v), len(v)) for s, v in bursts[form] if len(v) >= 5]      # (single launches: the bit-identity calls)
        pairs = [(a, b) for a, b in zip(seq, seq[1:]) if a[0][1] == b[0][1] and a[0][0] == 0 and b[0][0] == 1]
        for i, (a, b) in enumerate(pairs):
            print("%s, %d lanes, pair %2d: one fill at a time %.1f us (%d launches) -> overlapped %.1f us (%d launches)  %+.1f us"
                  % (form, a[0][1], i, a[1], a[2], b[1], b[2], b[1] - a[1]))
        print("%s: overlapped faster in %d of %d pairs" % (form, sum(b[1] < a[1] for a, b in pairs), len(pairs)))
        # the lane layouts: a burst of the 8-lane kernel followed by one of the 4-lane kernel under the same schedule
        pairs = [(a, b) for a, b in zip(seq, seq[1:]) if a[0][0] == b[0][0] and a[0][1] == 8 and b[0][1] == 4]
        for i, (a, b) in enumerate(pairs):
            print("%s, schedule %d, pair %2d: eight lanes %.1f us (%d launches) -> four lanes %.1f us (%d launches)  %+.1f us"
                  % (form, a[0][0], i, a[1], a[2], b[1], b[2], b[1] - a[1]))
        print("%s: four lanes faster in %d of %d pairs" % (form, sum(b[1] < a[1] for a, b in pairs), len(pairs)))


if __name__ == "__main__":
    main()
