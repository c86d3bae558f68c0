"""The result files of one video written by the host writer (`results.write_video(device_rows=True)`: the baseline) and from
text formatted on the GPU (`device_text=True`, csrc/result_text.hip), on the 400-frame 1280x720 video of tools/online_bench.py
(ICDAR15 config, synthetic weights, the benchmark's own model set-up and class-bias calibration), one process, the paths
alternating, median and range.  The files of both paths are compared byte for byte before anything is timed.

  writing    seconds "building rows and writing files" for the video's predictions (already on the GPU), per path, and their
             split: host = rows launch + copy back | finish_rows | json / minidom + file write; device = rows and text launches
             (with the one synchronising read) | copy back (the words finish_points needs, then the text) | finish_points |
             file write.
  command    frames/s of `results.spot_video` + `results.write_video` (what `eval` does per video, frames already decoded),
             without and with the device text.

    python tools/result_text_bench.py [--frames 400] [--rounds 5] > profiles/result_text_bench.log
"""
import argparse
import os
import statistics
import sys
import tempfile
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


def fmt(xs, unit="s"):
    return "%8.3f %s (%.3f .. %.3f)" % (statistics.median(xs), unit, min(xs), max(xs))


def host_write(preds, out, dec, split):
    """`results.write_video(device_rows=True)` with a clock between its parts (the same calls in the same order)."""
    insts = [r["instances"] for r in preds]
    counts = [len(x) for x in insts]
    live = [x for x, c in zip(insts, counts) if c]
    t0 = time.perf_counter()
    bd = torch.cat([x.bd.detach().reshape(-1, 25, 4) for x in live])
    recs = torch.cat([x.recs.detach().reshape(-1, 25) for x in live]).to(torch.int64)
    ids = torch.cat([x.track_ids.detach().reshape(-1) for x in live]).to(device=bd.device, dtype=torch.int64)
    words = ops.result_rows(bd.to(torch.float32), recs, dec.voc_size, ids).cpu().numpy()
    t1 = time.perf_counter()
    rows = results.finish_rows(words, dec)
    annotation, o = {}, 0
    for i, c in enumerate(counts):
        annotation[str(i + 1)] = [r for r in rows[o:o + c] if r is not None]
        o += c
    t2 = time.perf_counter()
    os.makedirs(os.path.join(out, "jsons"), exist_ok=True)
    os.makedirs(os.path.join(out, "preds"), exist_ok=True)
    results.write_video_results(annotation, os.path.join(out, "jsons", "Video_1_1_1.json"), os.path.join(out, "preds", "res_video_1.xml"))
    t3 = time.perf_counter()
    for k, v in (("launch+copy", t1 - t0), ("finish", t2 - t1), ("write", t3 - t2)):
        split.setdefault(k, []).append(v)
    return t3 - t0


def device_write(preds, out, dec, split):
    timing = {}
    t0 = time.perf_counter()
    results.write_video(preds, "Video_1_1_1", "ICDAR15", out, dec, device_rows=True, device_text=True, rows=False, timing=timing)
    dt = time.perf_counter() - t0
    for k in ("launch", "copy", "finish", "write"):
        split.setdefault(k, []).append(timing.get(k, 0.0))
    return dt


def files(out):
    return {sub + "/" + f: open(os.path.join(out, sub, f), "rb").read() for sub in ("jsons", "preds")
            for f in sorted(os.listdir(os.path.join(out, sub)))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=400)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--detect-frac", type=float, default=0.3)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    cfg = setup_cfg(builtin="icdar15")
    cfg.MODEL.DEVICE = "cuda"
    base = [np.ascontiguousarray(f[:, :, ::-1]) for f in make_clip(100, bench.SRC_HW[0], bench.SRC_HW[1], clip_id=0, num_rects=12)]
    clip = [base[i % 100] if (i // 100) % 2 == 0 else base[99 - i % 100] for i in range(args.frames)]     # back and forth: no jump
    model, _ = bench.build_model(cfg, dev)
    cal, _ = GoMBatchPredictor(cfg, None).prepare(clip[:1])
    shift, _ = bench.calibrate(model, [dict(x, image=x["image"].to(dev)) for x in cal], frac=args.detect_frac)
    spotter = GoMBatchPredictor(cfg, model, device_ingest=True)
    dec = TextDecoder(cfg.MODEL.TRANSFORMER.VOC_SIZE)
    print("torch %s, %s; %d frames %dx%d, %d queries, class-bias shift %+.3f, frames_per_step %d, %d rounds"
          % (torch.__version__, torch.cuda.get_device_name(0), len(clip), bench.SRC_HW[1], bench.SRC_HW[0],
             cfg.MODEL.TRANSFORMER.NUM_QUERIES, shift, model.frames_per_step, args.rounds))
    tmp = tempfile.mkdtemp()
    preds, _ = results.spot_video(spotter, clip, new_time_cost())
    n_rows = sum(len(r["instances"]) for r in preds)

    # ---- the files first
    host_write(preds, os.path.join(tmp, "h0"), dec, {})
    device_write(preds, os.path.join(tmp, "d0"), dec, {})
    fh, fd = files(os.path.join(tmp, "h0")), files(os.path.join(tmp, "d0"))
    assert sorted(fh) == sorted(fd) and all(fh[k] == fd[k] for k in fh), "the device text differs from the host writer's"
    print("files equal: %s; %d instances in, %.1f MB of JSON, %.1f MB of XML"
          % (", ".join(sorted(fh)), n_rows, len(fh["jsons/Video_1_1_1.json"]) / 1e6, len(fh["preds/res_video_1.xml"]) / 1e6))

    # ---- writing alone, the paths alternating
    th, td, sh, sd = [], [], {}, {}
    for r in range(args.rounds):
        th.append(host_write(preds, os.path.join(tmp, "h%d" % (r + 1)), dec, sh))
        td.append(device_write(preds, os.path.join(tmp, "d%d" % (r + 1)), dec, sd))
    print("\nbuilding rows and writing files, %d frames (median and range of %d)" % (len(clip), args.rounds))
    print("  host writer (baseline)   %s" % fmt(th))
    for k in ("launch+copy", "finish", "write"):
        print("      %-22s %s" % ({"launch+copy": "rows launch + copy back", "finish": "finish_rows", "write": "json / minidom + write"}[k], fmt(sh[k])))
    print("  device text              %s" % fmt(td))
    for k in ("launch", "copy", "finish", "write"):
        print("      %-22s %s" % ({"launch": "launches + totals read", "copy": "copies back", "finish": "finish_points", "write": "file write"}[k], fmt(sd[k])))
    print("  host / device            %8.2f x" % (statistics.median(th) / statistics.median(td)))

    # ---- the whole command per video: spotting and writing
    fh, fd = [], []
    for r in range(args.rounds):
        for path, acc in ((host_write, fh), (device_write, fd)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            p, _ = results.spot_video(spotter, clip, new_time_cost())
            path(p, os.path.join(tmp, "c%d%s" % (r, path.__name__)), dec, {})
            acc.append(len(clip) / (time.perf_counter() - t0))
            del p
    print("\nspot_video + write_video, frames already decoded (median and range of %d)" % args.rounds)
    print("  without --device-write   %s" % fmt(fh, "frames/s"))
    print("  with    --device-write   %s" % fmt(fd, "frames/s"))


if __name__ == "__main__":
    main()
