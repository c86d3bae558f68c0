"""Time the per-frame matching of the detection protocol on one synthetic video at two sizes: 44 objects per frame over 100
frames and 300 per frame over 1000 frames (DSText's worst case), a tenth of the ground truth "don't care" (the videos of
tools/score_bench.py).

In one process, alternating and after a warm-up of each:
  host      `score_det.host_quad_det_match`: numpy float64 pairs (both measures) and the greedy sweep in Python
  composed  `score_det.composed_quad_det_match`: `ops.quad_pairs` twice (upload, count, scan, emit, copy back of every kept
            pair) and the same sweep on the host -- what the fused launch replaces
  fused     `score_det.device_quad_det_match`: upload, ONE launch of `ops.quad_det_match`, copy back of det_care, match and
            the per-frame counts
and, on its own, the fused launch between device events with the inputs resident (20 launches per window, time per launch).
Prints the median and the range of each over the rounds and whether the three paths returned the same bytes (asserted).  The
reference's own script is not timed: its polygon library is not available here."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from gomatching_amd import ops, score_det                            # noqa: E402
from score_bench import stats, video                                 # noqa: E402


def arrays(v):
    """score_bench's video (care / don't-care / detections) -> the CSR arrays of one `quad_det_match` call; within a frame
    the don't-care objects come after the care objects."""
    (cq, coff), (dq, doff), (det, det_off) = v["care"], v["dont"], v["det"]
    F = len(coff) - 1
    quads, care = [], []
    for f in range(F):
        quads += [cq[coff[f]:coff[f + 1]], dq[doff[f]:doff[f + 1]]]
        care += [np.ones(coff[f + 1] - coff[f], dtype=np.int32), np.zeros(doff[f + 1] - doff[f], dtype=np.int32)]
    return (np.concatenate(quads).astype(np.int32), det, (coff + doff).astype(np.int32), det_off, np.concatenate(care), 0.5, 0.5)


def kernel_only(a, rounds, reps=20):
    dev = torch.device("cuda:0")
    t = [torch.from_numpy(np.ascontiguousarray(x, dtype=np.int32)).to(dev) for x in a[:5]]
    most = int((a[3][1:] - a[3][:-1]).max())
    times = []
    for _ in range(rounds + 1):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(reps):
            ops.quad_det_match(*t, 0.5, 0.5, max_det=most)
        e.record()
        torch.cuda.synchronize()
        times.append(s.elapsed_time(e) * 1e-3 / reps)
    return times[1:]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--sizes", default="44x100,300x1000")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "score_det_bench needs the GPU"
    print("device: %s" % torch.cuda.get_device_name(0))
    for size in args.sizes.split(","):
        per_frame, frames = [int(s) for s in size.split("x")]
        a = arrays(video(per_frame, frames, seed=per_frame))
        paths = (("host", score_det.host_quad_det_match), ("composed", score_det.composed_quad_det_match),
                 ("fused", score_det.device_quad_det_match))
        outs = {name: fn(*a) for name, fn in paths}               # the warm-up of each, and the comparison
        same = all(x.tobytes() == y.tobytes() for name in ("composed", "fused") for x, y in zip(outs["host"], outs[name]))
        assert same, "the three paths disagree"
        times = {name: [] for name, _ in paths}
        for _ in range(args.rounds):
            for name, fn in paths:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn(*a)
                torch.cuda.synchronize()
                times[name].append(time.perf_counter() - t0)
        kt = kernel_only(a, args.rounds)
        st = outs["fused"][2].sum(0)
        pairs = int(((a[2][1:] - a[2][:-1]).astype(np.int64) * (a[3][1:] - a[3][:-1])).sum())
        print("%d objects per frame x %d frames: %d ground truth (%d don't care), %d detections, %d pairs; matched %d of %d care "
              "objects, %d care detections; host, composed and fused outputs bytewise equal: %s"
              % (per_frame, frames, len(a[0]), int((a[4] == 0).sum()), len(a[1]), pairs, st[0], st[1], st[2], same))
        for name, _ in paths:
            print("  %-22s %s" % (name, stats(times[name])))
        print("  %-22s %s" % ("fused launch alone", stats(kt)))


if __name__ == "__main__":
    main()
