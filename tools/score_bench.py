"""Time the pairwise polygon measure of scoring on one synthetic video at two sizes: 44 objects per frame over 100 frames (the
headline workload's density) and 300 per frame over 1000 frames (DSText's worst case: every query of every frame).

A tenth of the ground truth is "don't care", so a video takes the two calls `score.score_video` makes: the overlap of the
don't-care regions with the detections, then the IoU of the rest.  In one process, alternating and after a warm-up:
  host    `score.host_quad_pairs` (numpy float64) for both calls
  device  `score.device_quad_pairs` for both calls: upload, count launch, prefix sum, emit launch, copy back
and, on their own, the four launches (count + emit of both calls) between device events with the inputs resident (20
passes per window, time per pass).
Prints the median and the range of each over the rounds, pairs per second (pairs = ground truth x detections summed over the
frames, both calls), and whether the two paths returned the same bytes.  The reference's own protocol script is not timed:
its polygon library is not available here."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gomatching_amd import ops, score                                # noqa: E402
from gomatching_amd.ops import _L, _p, _stream                       # noqa: E402


def video(per_frame, frames, seed):
    rng = np.random.RandomState(seed)
    n = per_frame * frames
    x, y = rng.randint(0, 1200, size=n), rng.randint(0, 640, size=n)
    w, h = rng.randint(8, 81, size=n), rng.randint(8, 81, size=n)
    gt = np.stack([x, y, x + w, y, x + w, y + h, x, y + h], 1) + rng.randint(-6, 7, size=(n, 8))
    det = gt + rng.randint(-9, 10, size=(n, 8))
    keep = rng.rand(n) < 0.85
    frame = np.repeat(np.arange(frames), per_frame)
    dont = rng.rand(n) < 0.1
    off = lambda mask: np.concatenate([[0], np.cumsum(np.bincount(frame[mask], minlength=frames))]).astype(np.int32)
    q = lambda a: np.maximum(a, 0).astype(np.int32)
    return {"care": (q(gt[~dont]), off(~dont)), "dont": (q(gt[dont]), off(dont)), "det": (q(det[keep]), off(keep))}


def calls(v):
    """The two (gt_quads, det_quads, gt_off, det_off, gt_key, det_key, measure, threshold) calls of a video."""
    dq, doff = v["det"]
    out = []
    for name, measure in (("dont", 1), ("care", 0)):
        gq, goff = v[name]
        out.append((gq, dq, goff, doff, np.zeros(len(gq), dtype=np.int32), np.zeros(len(dq), dtype=np.int32), measure, 0.5))
    return out


def stats(ts):
    ts = sorted(ts)
    return "median %9.3f ms  (min %9.3f, max %9.3f, n = %d)" % (ts[len(ts) // 2] * 1e3, ts[0] * 1e3, ts[-1] * 1e3, len(ts))


def kernels_only(cs, rounds, reps=20):
    """The raw launches between device events, inputs and prefix sums resident; `reps` passes per window, time per pass."""
    dev = torch.device("cuda:0")
    prepared = []
    for gq, dq, goff, doff, gk, dk, measure, thr in cs:
        t = [torch.from_numpy(a).to(dev) for a in (gq, dq, goff, doff, gk, dk)]
        pairs = int(((goff[1:] - goff[:-1]).astype(np.int64) * (doff[1:] - doff[:-1])).sum())
        counts, det, val = ops.quad_pairs(*t, measure, thr, pairs=pairs)
        scan = torch.cumsum(counts, 0, dtype=torch.int64) - counts
        args = tuple(_p(a) for a in t) + (len(gq), len(dq), len(goff) - 1, pairs, measure, thr)
        prepared.append((t, args, counts, scan, det, val))
    times = []
    for _ in range(rounds + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            for t, args, counts, scan, det, val in prepared:
                ops.check(_L().gom_quad_pairs_count_f64(*args, _p(counts), _stream()))
                ops.check(_L().gom_quad_pairs_emit_f64(*args, _p(scan), det.numel(), _p(det), _p(val), _stream()))
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b) * 1e-3 / reps)
    return times[1:]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--sizes", default="44x100,300x1000")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "score_bench needs the GPU"
    print("device: %s" % torch.cuda.get_device_name(0))
    for size in args.sizes.split(","):
        per_frame, frames = [int(s) for s in size.split("x")]
        cs = calls(video(per_frame, frames, seed=per_frame))
        pairs = sum(int(((c[2][1:] - c[2][:-1]).astype(np.int64) * (c[3][1:] - c[3][:-1])).sum()) for c in cs)
        host = lambda: [score.host_quad_pairs(*c) for c in cs]
        device = lambda: [score.device_quad_pairs(*c) for c in cs]
        h, d = host(), device()                                   # the warm-up of both, and the comparison
        same = all(x.tobytes() == y.tobytes() for a, b in zip(h, d) for x, y in zip(a, b))
        kept = [len(r[1]) for r in d]
        times = {"host": [], "device": []}
        for _ in range(args.rounds):
            for name, fn in (("host", host), ("device", device)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                times[name].append(time.perf_counter() - t0)
        kt = kernels_only(cs, args.rounds)
        print("%d objects per frame x %d frames: %d ground truth (%d don't care), %d detections, %d pairs in two calls, kept %d + %d; "
              "host and device outputs bytewise equal: %s" % (per_frame, frames, len(cs[0][0]) + len(cs[1][0]), len(cs[0][0]),
                                                             len(cs[0][1]), pairs, kept[0], kept[1], same))
        for name in ("host", "device"):
            print("  %-22s %s  %10.3e pairs/s" % (name, stats(times[name]), pairs / sorted(times[name])[len(times[name]) // 2]))
        print("  %-22s %s  %10.3e pairs/s" % ("kernels (4 launches)", stats(kt), pairs / sorted(kt)[len(kt) // 2]))


if __name__ == "__main__":
    main()
