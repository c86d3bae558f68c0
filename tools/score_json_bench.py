"""Time the mask measure of ArTVideo scoring on one synthetic video: 1280 x 720, 44 objects per frame over 100 frames, every
result a 50-point boundary polygon around a curved text line, every ground-truth mask a COCO RLE.

A tenth of the ground truth is ignored ("###"), so the video takes the two calls `score_json.score_artvideo` makes with
--e2e: the ignored masks against the results, then the counted ones.  The mask sets (boxes, offsets, vertices, run ends: the
O(vertices + runs) host description) are built once and shared.  In one process, alternating and after a warm-up:
  host    `score_json.host_mask_pairs` for both calls: rasterisation, popcounts and IoU in numpy
  device  `score_json.device_mask_pairs` for both calls: upload, the fill launches, count launch, prefix sum, emit launch, copy back
and, on their own, the launches (RLE fill, polygon fill, count, emit of both calls) between device events with the inputs
resident (20 passes per window, time per pass).
Prints the median and the range of each over the rounds, pairs per second (pairs = ground truth x results summed over the
frames, both calls), and whether the two paths returned the same bytes.  The reference's own protocol script is not timed:
cv2 and pycocotools, which it needs, are not available here; the comparison is against the host path of this same tree."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gomatching_amd import ops, score_json as sj                     # noqa: E402
from gomatching_amd.ops import _L, _p, _stream                       # noqa: E402

H, W = 720, 1280


def curved_polygon(rng):
    """50 points: 25 along the upper side of a bent text line, left to right, 25 back along the lower side."""
    length, thick = rng.randint(60, 260), rng.randint(10, 36)
    x0, cy = rng.randint(0, W - length), rng.randint(40, H - 40)
    amp = rng.randint(-30, 31)
    t = np.linspace(0.0, 1.0, 25)
    x = x0 + t * length
    y = cy + amp * np.sin(np.pi * t)
    top = np.stack([x, y - thick / 2], 1)
    bottom = np.stack([x[::-1], y[::-1] + thick / 2], 1)
    return np.concatenate([top, bottom]).astype(np.int64)


def rle_of(contour):
    """The run lengths of a polygon's mask, from its bit rows (column-major order over the whole image)."""
    mset = sj.MaskSet([("poly", [contour])], H, W)
    y0, y1, wx0, wx1 = (int(v) for v in mset.boxes[0])
    rows = sj.fill_polygon_rows([contour], mset.boxes[0], W)
    bits = np.unpackbits(rows.view(np.uint8).reshape(y1 - y0, -1), axis=1, bitorder="little").astype(bool)
    ys, xs = np.nonzero(bits)
    p = np.sort((xs + 32 * wx0).astype(np.int64) * H + ys + y0)
    if len(p) == 0:
        return [H * W]
    brk = np.nonzero(np.diff(p) > 1)[0]
    starts, stops = np.concatenate([[p[0]], p[brk + 1]]), np.concatenate([p[brk], [p[-1]]]) + 1
    ends = np.stack([starts, stops], 1).reshape(-1)
    counts = np.diff(np.concatenate([[0], ends, [H * W]]))
    return [int(c) for c in counts]


def video(per_frame, frames, seed):
    """-> the two calls (gt set, det set, gt_off, det_off, gt_key, det_key, threshold): ignored, then counted ground truth."""
    rng = np.random.RandomState(seed)
    care, dont, dets = [[] for _ in range(frames)], [[] for _ in range(frames)], [[] for _ in range(frames)]
    for f in range(frames):
        for _ in range(per_frame):
            c = curved_polygon(rng)
            (dont if rng.rand() < 0.1 else care)[f].append(("rle", rle_of(c)))
            if rng.rand() < 0.85:
                dets[f].append(("poly", [c + rng.randint(-4, 5, size=c.shape)]))
    det_set = sj.MaskSet([s for x in dets for s in x], H, W)
    det_off = sj._off(dets)
    out = []
    for objs, thr in ((dont, 0.5), (care, float(np.nextafter(0.5, 0.0)))):
        gs = sj.MaskSet([s for x in objs for s in x], H, W)
        out.append((gs, det_set, sj._off(objs), det_off, np.zeros(gs.N, dtype=np.int32), np.zeros(det_set.N, dtype=np.int32), thr))
    return out


def stats(ts):
    ts = sorted(ts)
    return "median %9.3f ms  (min %9.3f, max %9.3f, n = %d)" % (ts[len(ts) // 2] * 1e3, ts[0] * 1e3, ts[-1] * 1e3, len(ts))


def n_pairs(c):
    return int(((c[2][1:] - c[2][:-1]) * (c[3][1:] - c[3][:-1])).sum())


def kernels_only(cs, rounds, reps=20):
    """The raw launches between device events, descriptions and prefix sums resident; `reps` passes per window."""
    dev = torch.device("cuda:0")

    def up(a, dtype):
        return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(dev)
    prepared = []
    for gs, ds, goff, doff, gk, dk, thr in cs:
        sets = []
        for ms_ in (gs, ds):
            t = {"boxes": up(ms_.boxes, np.int32), "woff": up(ms_.woff, np.int64), "ends": up(ms_.ends, np.int32),
                 "roff": up(ms_.roff, np.int32), "points": up(ms_.points, np.int32), "coff": up(ms_.coff, np.int32),
                 "mcoff": up(ms_.mcoff, np.int32), "words": torch.empty((int(ms_.woff[-1]),), dtype=torch.int32, device=dev),
                 "area": torch.zeros((ms_.N,), dtype=torch.int32, device=dev), "rle": bool(len(ms_.ends))}
            sets.append(t)
        g, d = sets
        fill(g)
        fill(d)
        t = [up(a, np.int32) for a in (goff, doff, gk, dk)]
        pairs = n_pairs((gs, ds, goff, doff))
        counts, det, val = ops.mask_pairs(g["words"], g["boxes"], g["woff"], g["area"], d["words"], d["boxes"], d["woff"], d["area"],
                                          *t, thr, pairs=pairs)
        scan = torch.cumsum(counts, 0, dtype=torch.int64) - counts
        args = (_p(g["words"]), _p(g["boxes"]), _p(g["woff"]), _p(g["area"]), g["words"].numel(), _p(d["words"]), _p(d["boxes"]),
                _p(d["woff"]), _p(d["area"]), d["words"].numel()) + tuple(_p(a) for a in t) + (gs.N, ds.N, len(goff) - 1, pairs, thr)
        prepared.append((g, d, t, args, counts, scan, det, val))
    times = []
    for _ in range(rounds + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            for g, d, t, args, counts, scan, det, val in prepared:
                fill(g)
                fill(d)
                ops.check(_L().gom_mask_pairs_count_f64(*args, _p(counts), _stream()))
                ops.check(_L().gom_mask_pairs_emit_f64(*args, _p(scan), det.numel(), _p(det), _p(val), _stream()))
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b) * 1e-3 / reps)
    return times[1:]


def fill(t):
    if t["rle"]:
        ops.mask_fill_rle(t["ends"], t["roff"], t["boxes"], t["woff"], H, W, t["words"], t["area"])
    else:
        ops.mask_fill_polygons(t["points"], t["coff"], t["mcoff"], t["boxes"], t["woff"], H, W, t["words"], t["area"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--size", default="44x100")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "score_json_bench needs the GPU"
    print("device: %s" % torch.cuda.get_device_name(0))
    per_frame, frames = [int(s) for s in args.size.split("x")]
    cs = video(per_frame, frames, seed=per_frame)
    pairs = sum(n_pairs(c) for c in cs)
    host = lambda: [sj.host_mask_pairs(*c) for c in cs]
    device = lambda: [sj.device_mask_pairs(*c) for c in cs]
    h, d = host(), device()                                       # the warm-up of both, and the comparison
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
    words = sum(int(c[0].woff[-1]) for c in cs) + 2 * int(cs[0][1].woff[-1])
    print("%d x %d, %d objects per frame x %d frames: %d ground-truth masks (%d ignored), %d results of 50 points, %d pairs in two "
          "calls, %d mask words (%.1f MiB), kept %d + %d; host and device outputs bytewise equal: %s" % (
              W, H, per_frame, frames, cs[0][0].N + cs[1][0].N, cs[0][0].N, cs[0][1].N, pairs, words, words * 4 / 2 ** 20, kept[0],
              kept[1], same))
    for name in ("host", "device"):
        print("  %-22s %s  %10.3e pairs/s" % (name, stats(times[name]), pairs / sorted(times[name])[len(times[name]) // 2]))
    print("  %-22s %s  %10.3e pairs/s" % ("kernels (8 launches)", stats(kt), pairs / sorted(kt)[len(kt) // 2]))


if __name__ == "__main__":
    main()
