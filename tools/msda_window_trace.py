"""Reduce a `rocprofv3 --kernel-trace` of tools/msda_window_bench.py to launch times per window-kernel form and burst: the tool
alternates the fill schedules burst by burst, so consecutive launches of one instantiation are one burst, and bursts of the two
schedules of a form that follow one another are a pair.

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
            rows.append((int(r["Start_Timestamp"]), "level-%s tiles" % p[5], int(p[6]) if len(p) > 6 else 0,
                         (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-3))
    rows.sort()
    bursts = collections.defaultdict(list)                   # form -> [(schedule, mean us, launches)] in time order
    for _, form, sched, us in rows:
        b = bursts[form]
        if b and b[-1][0] == sched:
            b[-1][1].append(us)
        else:
            b.append((sched, [us]))
    for form in sorted(bursts):
        seq = [(s, sum(v) / len(v), len(v)) for s, v in bursts[form] if len(v) >= 5]      # (single launches: the bit-identity calls)
        pairs = [(a, b) for a, b in zip(seq, seq[1:]) if a[0] == 0 and b[0] == 1]
        for i, (a, b) in enumerate(pairs):
            print("%s pair %2d: one fill at a time %.1f us (%d launches) -> overlapped %.1f us (%d launches)  %+.1f us"
                  % (form, i, a[1], a[2], b[1], b[2], b[1] - a[1]))
        print("%s: overlapped faster in %d of %d pairs" % (form, sum(b[1] < a[1] for a, b in pairs), len(pairs)))


if __name__ == "__main__":
    main()
