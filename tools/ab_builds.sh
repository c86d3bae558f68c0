#!/bin/bash
# same-box A/B of two builds of the library: gpurun_ab/lib_old.so against gpurun_ab/lib_new.so, alternating
tmp=$(mktemp -d)  # each run's JSON line and stderr
for rnd in 1 2 3; do
  for which in old new; do
    cp gpurun_ab/lib_$which.so gomatching_amd/libgomatching_hip.so
    timeout 300 python3 bench.py --full --no-alt-backends --no-cpu-baseline --no-config-legs --steps 15 > $tmp/bench_ab.json 2> $tmp/bench_ab.err
    python3 - "$which" $tmp/bench_ab.json <<'PY'
import json, sys
d = json.loads(open(sys.argv[2]).read().strip().splitlines()[-1])
print("%-6s %8.2f frames/s  (hbm-resident %8.2f)  %7.3f ms/step" % (sys.argv[1], d["value"], d.get("value_hbm_resident"), d["ms_per_step"]))
PY
  done
done
