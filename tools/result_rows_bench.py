"""Time result-row building on the headline workload: 1280x720 frames resized to 1000x1778, 100 queries, one 100-frame chunk,
synthetic weights calibrated as bench.py calibrates them.  The model runs once; then, alternating and after a warm-up,
(i) the per-frame host path `[frame_lines(...) for r in results]` and (ii) `clip_lines(results)` on the same results, each
window ending when the rows exist on the host (the device path's window holds its launch, the copy and the finishing).
Prints instances per frame, ms per clip, ms per frame and us per instance for both, and the model's ms per frame from the
same run."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench                                                       # noqa: E402  (build_model / calibrate: the bench's own set-up)
from gomatching_amd import ops, results                               # noqa: E402
from gomatching_amd.config import setup_cfg                        # noqa: E402
from gomatching_amd.predictor import GoMBatchPredictor, TextDecoder, new_time_cost   # noqa: E402
from gomatching_amd.synth import make_clip                         # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--detect-frac", type=float, default=0.3)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    cfg = setup_cfg(builtin="icdar15")
    cfg.MODEL.DEVICE = "cuda"
    clip = [np.ascontiguousarray(f[:, :, ::-1]) for f in make_clip(args.frames, bench.SRC_HW[0], bench.SRC_HW[1], clip_id=0,
                                                                  num_rects=12)]
    model, _ = bench.build_model(cfg, dev)
    cal, _ = GoMBatchPredictor(cfg, None).prepare(clip[:1])
    shift, _ = bench.calibrate(model, [dict(x, image=x["image"].to(dev)) for x in cal], frac=args.detect_frac)
    spotter = GoMBatchPredictor(cfg, model, device_ingest=True)
    dec = TextDecoder(cfg.MODEL.TRANSFORMER.VOC_SIZE)
    spotter(clip[:8], [], 0, 0, True, new_time_cost())             # warm-up: graphs, pools, lazy weight images
    torch.cuda.synchronize()
    preds, seconds = results.spot_video(spotter, clip, new_time_cost())
    n = sum(len(r["instances"]) for r in preds)
    per_frame = n / len(preds)
    print("workload: %d frames %dx%d, %d queries, class-bias shift %+.3f (detect-frac %.2f), instances %d = %.1f per frame"
          % (len(preds), bench.SRC_HW[1], bench.SRC_HW[0], cfg.MODEL.TRANSFORMER.NUM_QUERIES, shift, args.detect_frac, n,
             per_frame))
    if per_frame < 10:
        print("fewer than 10 instances per frame: raise --detect-frac")
    print("model (detector + tracker, timed window): %.3f ms per frame" % (seconds / len(preds) * 1e3))

    def host():
        return [results.frame_lines(r["instances"], dec) for r in preds]

    def device():
        return results.clip_lines(preds, dec)

    same = host() == device()                                      # also the warm-up of both
    kept = sum(len(rows) for rows in device())
    times = {"host": [], "device": []}
    for _ in range(args.rounds):
        for name, fn in (("host", host), ("device", device)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            times[name].append(time.perf_counter() - t0)
    print("rows identical on both paths: %s, rows kept %d of %d instances" % (same, kept, n))
    med = {}
    for name in ("host", "device"):
        t = sorted(times[name])
        med[name] = t[len(t) // 2]
        print("%-6s rows: %9.3f ms per clip  %7.4f ms per frame  %8.2f us per instance   (median of %d, min %.3f max %.3f ms)"
              % (name, med[name] * 1e3, med[name] / len(preds) * 1e3, med[name] / max(n, 1) * 1e6, len(t), t[0] * 1e3,
                 t[-1] * 1e3))
    print("host / device ratio: %.1f" % (med["host"] / med["device"]))
    # where the device path's window goes: the launch alone (events), then the copy, then the host finishing
    live = [r["instances"] for r in preds if len(r["instances"])]
    bd = torch.cat([x.bd.reshape(-1, 25, 4) for x in live])
    recs = torch.cat([x.recs.reshape(-1, 25) for x in live])
    ids = torch.cat([x.track_ids.reshape(-1) for x in live]).to(bd.device)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ops.result_rows(bd, recs, dec.voc_size, ids)
    a.record()
    for _ in range(20):
        words = ops.result_rows(bd, recs, dec.voc_size, ids)
    b.record()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    host_words = words.cpu().numpy()
    t1 = time.perf_counter()
    results.finish_rows(host_words, dec)
    t2 = time.perf_counter()
    print("device path breakdown: kernel %.1f us per launch (%d instances, %.3f us each), copy %.3f ms, finishing %.3f ms"
          % (a.elapsed_time(b) * 1e3 / 20, n, a.elapsed_time(b) * 1e3 / 20 / max(n, 1), (t1 - t0) * 1e3, (t2 - t1) * 1e3))
    ok = med["device"] / len(preds) < seconds / len(preds)
    print("device rows per frame below model per frame: %s (%.4f ms < %.3f ms)" % (ok, med["device"] / len(preds) * 1e3,
                                                                                  seconds / len(preds) * 1e3))
    return 0 if ok and same else 1


if __name__ == "__main__":
    sys.exit(main())
