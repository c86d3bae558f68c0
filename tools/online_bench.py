"""Online against offline spotting of one video at the headline size (1280x720, ICDAR15 config, synthetic weights, the
benchmark's own model set-up and class-bias calibration), one process, the paths alternating, median and range.

  throughput   frames/s of `results.spot_video` + `results.write_video(device_rows=True)` (offline: everything after the last
               frame) against `online.OnlineSpotter` + `results.VideoResultWriter` at pushes of 8 and of 32 frames, frames
               already decoded in both.  `--offline-only` runs the first alone: it uses nothing this tool's commit added, so the
               same file runs in a tree of the parent commit for the baseline figure on the same box.
  memory       `torch.cuda.max_memory_allocated` over a run of 100 and of 400 frames, both paths (after a reset and with the
               model, its graphs and pools warm; a peak holds the transients of the steps in flight, one 20 MB query-feature
               copy each), and `torch.cuda.memory_allocated` with the frames in: offline after `spot_video` (every frame's
               Instances alive), online after the pushes that complete frames 100, 200, ...; and the peak of every single
               push of a 400-frame online run (reset and synchronised around each push).
  wait         largest and mean wait of a frame, in frames, between being tracked and leaving the session.
  gather       the `ops.result_rows_gather` launch alone (descriptor resident, device events) beside the offline chain it
               replaces for the same instances: `torch.cat` + `index_select` + `scale_xy_` + `result_rows`.
  where        the online run's seconds split: detector + tracker window, gather launch + copy back (the per-push
               synchronisation), `finish_rows`, writer.

    python tools/online_bench.py [--frames 400] [--rounds 5] > profiles/online_bench.log
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


def fmt(xs, unit="frames/s"):
    return "%8.1f %s (%.1f .. %.1f)" % (statistics.median(xs), unit, min(xs), max(xs))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=400)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--detect-frac", type=float, default=0.3)
    ap.add_argument("--offline-only", action="store_true")
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
    runs = [0]
    held = []                                                      # (frames in, memory_allocated, peak of the push) probes of the running path
    probing = [False]                                              # the per-push probes synchronise: not in the timed rounds

    def offline(frames):
        runs[0] += 1
        out = os.path.join(tmp, "off%d" % runs[0])
        t0 = time.perf_counter()
        preds, _ = results.spot_video(spotter, frames, new_time_cost())
        held.append((len(frames), torch.cuda.memory_allocated(), 0))  # every frame's Instances are alive here
        results.write_video(preds, "Video_1_1_1", "ICDAR15", out, dec, device_rows=True)
        return time.perf_counter() - t0, out, sum(len(r["instances"]) for r in preds), None

    def online(frames, push):
        from gomatching_amd.online import OnlineSpotter
        runs[0] += 1
        out = os.path.join(tmp, "on%d" % runs[0])
        t0 = time.perf_counter()
        s = OnlineSpotter(cfg, model, dec, device_ingest=True)
        w = results.VideoResultWriter("Video_1_1_1", "ICDAR15", out)
        t_write, rows = 0.0, 0
        for i in range(0, len(frames), push):
            if probing[0]:
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats()
            got = s.push(frames[i:i + push])
            if probing[0]:                                           # what the session holds after this push, and the push's own peak
                torch.cuda.synchronize()
                held.append((min(i + push, len(frames)), torch.cuda.memory_allocated(), torch.cuda.max_memory_allocated()))
            t1 = time.perf_counter()
            for f, r in got:
                w.add(f, r)
                rows += len(r)
            t_write += time.perf_counter() - t1
        got = s.close()
        t1 = time.perf_counter()
        for f, r in got:
            w.add(f, r)
            rows += len(r)
        w.close()
        t_write += time.perf_counter() - t1
        return time.perf_counter() - t0, out, rows, (s, t_write)

    def same_files(a, b):
        for sub, name in (("preds", "res_video_1.xml"), ("jsons", "Video_1_1_1.json")):
            with open(os.path.join(a, sub, name), "rb") as fa, open(os.path.join(b, sub, name), "rb") as fb:
                if fa.read() != fb.read():
                    return False
        return True

    paths = [("offline", lambda fr: offline(fr))]
    if not args.offline_only:
        paths += [("online, push 8", lambda fr: online(fr, 8)), ("online, push 32", lambda fr: online(fr, 32))]
    outs = {}
    for name, fn in paths:                                          # warm-up of every path: graphs, pools, lazy weight images
        outs[name] = fn(clip[:64])[1]
    if not args.offline_only:
        print("files of the warm-up runs identical: push 8 %s, push 32 %s" % (same_files(outs["offline"], outs["online, push 8"]),
                                                                             same_files(outs["offline"], outs["online, push 32"])))
    times, last = {n: [] for n, _ in paths}, {}
    for _ in range(args.rounds):
        for name, fn in paths:
            torch.cuda.synchronize()
            dt, out, count, extra = fn(clip)
            times[name].append(len(clip) / dt)
            last[name] = (out, count, extra, dt)
    print("throughput, %d frames, decoded frames in, result files out:" % len(clip))
    for name, _ in paths:
        print("   %-16s %s" % (name, fmt(times[name])))
    if not args.offline_only:
        for name in ("online, push 8", "online, push 32"):
            out, rows, (s, t_write), dt = last[name]
            print("   %s: files identical to offline %s; rows %d; largest wait %d frames (bound %d), mean %.2f; gather launches %d; "
                  "seconds: detector + tracker + gather window %.3f (of it gather launch + copy back %.3f), finish_rows %.3f, "
                  "writer %.3f, rest %.3f" % (name, same_files(last["offline"][0], out), rows, s.max_wait, s.latency_bound,
                                             s.settler.wait_sum / max(len(clip), 1), s.gather_launches, s.seconds,
                                             s.time_cost["post_process"], s.rows_seconds, t_write,
                                             dt - s.seconds - s.rows_seconds - t_write))
            lo, hi = min(times[name]), max(times[name])
            olo, ohi = min(times["offline"]), max(times["offline"])
            print("   %s is %s" % (name, "slower than offline beyond the spread" if hi < olo else
                                   ("faster than offline beyond the spread" if lo > ohi else "within the spread of offline")))
    print("peak device memory (torch.cuda.max_memory_allocated after a reset, model warm):")
    for name, fn in paths:
        peaks = []
        for n in (100, len(clip)):
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            before = torch.cuda.memory_allocated()
            del held[:]
            probing[0] = name != "offline"
            fn(clip[:n])
            probing[0] = False
            torch.cuda.synchronize()
            # (a probed run resets the statistic around every push: its peak is the largest push's, the last of them `close()`'s)
            top = max([torch.cuda.max_memory_allocated()] + [p for _, _, p in held])
            peaks.append((n, top - before))
        print("   %-16s peak: %s   growth %+.1f MB" % (name, ", ".join("%d frames %.1f MB above the resident model" % (n, p / 1e6) for n, p in peaks),
                                                        (peaks[-1][1] - peaks[0][1]) / 1e6))
        print("   %-16s held (memory_allocated with the frames in, %d-frame run): %s" % (
            "", len(clip), ", ".join("after %d frames %.1f MB" % (n, (m - before) / 1e6) for k, (n, m, _) in enumerate(held)
                                     if n == len(clip) or (k and held[k - 1][0] // 100 < n // 100))))
        if name != "offline":                                       # a second run, synchronised and reset around every push
            probing[0] = True
            del held[:]
            torch.cuda.synchronize()
            before = torch.cuda.memory_allocated()
            fn(clip)
            probing[0] = False
            print("   %-16s peak of each push above the resident model, MB: %s" % ("", " ".join("%.0f" % ((p - before) / 1e6) for _, _, p in held)))
    if args.offline_only:
        return
    # the gather launch alone beside the chain it replaces, for the instances of one 32-frame push
    preds, _ = spotter.run_prepared(*spotter.prepare_device(clip[:32]), [], 0, 0, False, new_time_cost())
    n_inst = [len(x) for x in preds]
    total = sum(n_inst)
    bd_ring = torch.cat([x.bd.reshape(-1, 25, 4) for x in preds]).contiguous()
    recs_ring = torch.cat([x.recs.reshape(-1, 25) for x in preds]).contiguous()
    keep = np.sort(np.random.default_rng(0).permutation(total)[:total * 9 // 10]).astype(np.int64)
    ids = np.arange(len(keep), dtype=np.int64)
    sx, sy = model.output_scale(preds[0].image_size, bench.SRC_HW)
    desc = ops.result_rows_desc(keep, ids, sx, sy)
    desc_d = torch.from_numpy(desc).to(dev)
    idx_d, ids_d = torch.from_numpy(keep).to(dev), torch.from_numpy(ids).to(dev)
    out = torch.empty((len(keep), ops.RESULT_ROWS_WORDS), dtype=torch.int32, device=dev)
    L = ops._L()

    def gather():
        ops.check(L.gom_result_rows_gather_i32(ops._p(bd_ring), ops._p(recs_ring), total, ops._p(desc_d), len(keep),
                                               dec.voc_size, ops._p(out), ops.RESULT_ROWS_WORDS, ops._stream()))
        return out

    def chain():
        bd = torch.cat([x.bd.reshape(-1, 25, 4) for x in preds]).index_select(0, idx_d)
        recs = torch.cat([x.recs.reshape(-1, 25) for x in preds]).index_select(0, idx_d)
        return ops.result_rows(ops.scale_xy_(bd, sx, sy), recs, dec.voc_size, ids_d)
    assert torch.equal(gather(), chain())
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    for name, fn in (("gather launch", gather), ("offline chain (cat, index_select, scale_xy_, result_rows)", chain)):
        ts = []
        for _ in range(22):
            ev[0].record()
            fn()
            ev[1].record()
            ev[1].synchronize()
            ts.append(ev[0].elapsed_time(ev[1]) * 1e3)
        print("   %-60s %s for %d instances of 32 frames [same words]" % (name, fmt(ts[2:], "us"), len(keep)))
    model.close()


if __name__ == "__main__":
    main()
