"""Measure the drawing chain on frames that lie in device memory.  One process, the paths alternating, median and range over
the rounds, outputs asserted equal first.  None of it is a gate.

  show     `python -m gomatching_amd.show` (called in-process) on the 100-frame 1280 x 720 video of tools/overlay_bench.py (44
           rows per frame), its frames written as JPEG files: without flags, with `--device-encode`, and with `--device-decode
           --device-encode`; wall time, and the growth of the process's resident set during each run (sampled every 5 ms).
  stream   the 400-frame video of tools/online_bench.py (the benchmark's model set-up), its frames as JPEG files: the offline
           path of `eval --show --device-decode --device-encode` (spot, write, decode again and draw chunk by chunk) against
           `eval.spot_video_online` at pushes of 32 with the same flags, in frames/s; and the device memory a drawing session
           holds after 100 / 200 / 300 / 400 frames.
  gather   the gather-compose launch alone (32 frames out of a ring of 41 slots, wrapping) against `index_select` + the dense
           compose launch in place, between device events.

    python tools/online_draw_bench.py [--rounds 5] [--frames 400] > profiles/online_draw_bench.log
"""
import argparse
import contextlib
import io
import json
import os
import shutil
import statistics
import sys
import tempfile
import threading
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import bench                                                       # noqa: E402
import overlay_bench                                               # noqa: E402
from gomatching_amd import eval as E                               # noqa: E402
from gomatching_amd import ops, results, show                      # noqa: E402
from gomatching_amd.config import setup_cfg                        # noqa: E402
from gomatching_amd.predictor import GoMBatchPredictor, TextDecoder, new_time_cost   # noqa: E402
from gomatching_amd.synth import make_clip                         # noqa: E402


def fmt(xs, unit):
    return "median %9.1f %s (%.1f .. %.1f, n = %d)" % (statistics.median(xs), unit, min(xs), max(xs), len(xs))


def rss():
    with open("/proc/self/statm") as fp:
        return int(fp.read().split()[1]) * os.sysconf("SC_PAGE_SIZE")


class RssPeak:
    """The largest resident set seen while the block runs, sampled every 5 ms, above the one at its start."""

    def __enter__(self):
        self.start = self.peak = rss()
        self._stop = threading.Event()
        self._t = threading.Thread(target=self._loop, daemon=True)
        self._t.start()
        return self

    def _loop(self):
        while not self._stop.wait(0.005):
            self.peak = max(self.peak, rss())

    def __exit__(self, *exc):
        self._stop.set()
        self._t.join()
        self.growth = max(self.peak, rss()) - self.start


def write_jpegs(frames_bgr, directory):
    from PIL import Image
    os.makedirs(directory)
    for i, f in enumerate(frames_bgr):
        Image.fromarray(np.ascontiguousarray(f[:, :, ::-1])).save(os.path.join(directory, "%d.jpg" % (i + 1)), quality=90)


def files(directory):
    out = {}
    for root, _, names in os.walk(directory):
        for n in names:
            with open(os.path.join(root, n), "rb") as fp:
                out[os.path.relpath(os.path.join(root, n), directory)] = fp.read()
    return out


def show_part(tmp, rounds):
    fr, rows = overlay_bench.video(44, 100, seed=44)
    data = os.path.join(tmp, "ICDAR15_show")
    write_jpegs(fr, os.path.join(data, "Video_1_1_1"))
    del fr
    res = os.path.join(tmp, "show_results")
    os.makedirs(os.path.join(res, "jsons"))
    with open(os.path.join(res, "jsons", "Video_1_1_1.json"), "w") as fp:
        json.dump({str(f + 1): [{"points": r[:8], "ID": r[8], "transcription": r[9], "segmentation": r[10]} for r in fr_rows]
                   for f, fr_rows in enumerate(rows)}, fp)
    paths = {"no flags": [], "--device-encode": ["--device-encode"], "--device-decode": ["--device-decode"],
             "--device-decode --device-encode": ["--device-decode", "--device-encode"]}
    runs = [0]

    def run(flags):
        runs[0] += 1
        out = os.path.join(tmp, "show_out%d" % runs[0])
        torch.cuda.synchronize()
        with RssPeak() as peak:
            t0 = time.perf_counter()
            with contextlib.redirect_stdout(io.StringIO()):
                status = show.main(["--input", data, "--results", res, "--output", out] + flags)
            assert status == 0
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
        return dt, peak.growth, out
    got = {}
    for name, flags in paths.items():                              # warm-up of every path, and the comparison
        got[name] = files(run(flags)[2])
    assert got["--device-decode"] == got["no flags"] and got["--device-decode --device-encode"] == got["--device-encode"]
    print("show command, 100 frames 1280 x 720, 44 rows per frame; pictures of --device-decode equal those without it, with and "
          "without --device-encode: True")
    for d in os.listdir(tmp):
        if d.startswith("show_out"):
            shutil.rmtree(os.path.join(tmp, d))
    times, growth = {n: [] for n in paths}, {n: [] for n in paths}
    for _ in range(rounds):
        for name, flags in paths.items():
            dt, g, out = run(flags)
            times[name].append(dt * 1e3)
            growth[name].append(g / 1e6)
            shutil.rmtree(out)
    for name in paths:
        print("   %-34s %s; resident set growth %s" % (name, fmt(times[name], "ms"), fmt(growth[name], "MB")))


def stream_part(tmp, rounds, frames):
    dev = torch.device("cuda:0")
    cfg = setup_cfg(builtin="icdar15")
    cfg.MODEL.DEVICE = "cuda"
    base = [np.ascontiguousarray(f[:, :, ::-1]) for f in make_clip(100, bench.SRC_HW[0], bench.SRC_HW[1], clip_id=0, num_rects=12)]
    data = os.path.join(tmp, "ICDAR15_stream", "Video_1_1_1")
    write_jpegs([base[i % 100] if (i // 100) % 2 == 0 else base[99 - i % 100] for i in range(frames)], data)
    paths = E.frame_paths(data)
    model, _ = bench.build_model(cfg, dev)
    cal, _ = GoMBatchPredictor(cfg, None).prepare(base[:1])
    shift, _ = bench.calibrate(model, [dict(x, image=x["image"].to(dev)) for x in cal], frac=0.3)
    spotter = GoMBatchPredictor(cfg, model, device_ingest=True)
    dec = TextDecoder(cfg.MODEL.TRANSFORMER.VOC_SIZE)
    voc = cfg.MODEL.TRANSFORMER.VOC_SIZE
    print("stream: torch %s, %s; %d JPEG frames %dx%d, %d queries, class-bias shift %+.3f, frames_per_step %d"
          % (torch.__version__, torch.cuda.get_device_name(0), frames, bench.SRC_HW[1], bench.SRC_HW[0],
             cfg.MODEL.TRANSFORMER.NUM_QUERIES, shift, model.frames_per_step))
    runs = [0]
    atlas = show.Atlas()

    def routes():
        return {k: 0 for k in E.DECODE_ROUTES}

    def offline(ps, pool):
        runs[0] += 1
        out = os.path.join(tmp, "off%d" % runs[0])
        t0 = time.perf_counter()
        preds, _, _ = E.spot_video_device_decode(spotter, pool, ps, new_time_cost(), routes(), dev, walk="auto")
        annotation = results.write_video(preds, "Video_1_1_1", "ICDAR15", out, dec, device_rows=True)
        del preds
        show.draw_video(show.DecodedChunks(ps, pool, routes(), dev, "auto"), annotation, ps, "Video_1_1_1", out, voc, pool, atlas,
                        encode="device", quality=95)
        return time.perf_counter() - t0, out

    def online(ps, pool):
        runs[0] += 1
        out = os.path.join(tmp, "on%d" % runs[0])
        args = argparse.Namespace(push=32, host_ingest=False, device_write=False, device_vote=False, decode_walk="auto", output=out)
        t0 = time.perf_counter()
        E.spot_video_online(cfg, model, dec, pool, ps, "Video_1_1_1", "ICDAR15", args, new_time_cost(), routes(), None,
                            draw=(atlas, "device", 95))
        return time.perf_counter() - t0, out
    with ThreadPoolExecutor(max_workers=E.DECODE_THREADS) as pool:
        a, b = offline(paths[:64], pool)[1], online(paths[:64], pool)[1]          # warm-up, and the comparison
        fa, fb = files(a), files(b)
        assert sorted(fa) == sorted(fb) and all(fa[k] == fb[k] for k in fa) and len(fa) == 64 + 2, sorted(fa)[:5]
        print("   files of the 64-frame warm-up runs (64 pictures, json, xml) identical: True")
        shutil.rmtree(a)
        shutil.rmtree(b)
        fps = {"offline": [], "online, push 32": []}
        for _ in range(rounds):
            for name, fn in (("offline", offline), ("online, push 32", online)):
                torch.cuda.synchronize()
                dt, out = fn(paths, pool)
                fps[name].append(len(paths) / dt)
                shutil.rmtree(out)
        for name in fps:
            print("   %-18s --show --device-decode --device-encode: %s" % (name, fmt(fps[name], "frames/s")))
        # what a drawing session holds
        from gomatching_amd.online import OnlineSpotter
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated()
        s = OnlineSpotter(cfg, model, dec, device_ingest=True, draw=atlas)
        held, drawn_frames = [], 0
        for f0 in range(0, len(paths), 32):
            part = paths[f0:f0 + 32]
            s.push(E.decode_frames(part, [E.read_bytes(p) for p in part], routes(), dev, "auto"))
            drawn_frames += sum(int(t.shape[0]) for _, t in s.take_drawn())
            if (f0 + 32) // 100 > f0 // 100 or f0 + 32 >= len(paths):
                torch.cuda.synchronize()
                held.append((min(f0 + 32, len(paths)), torch.cuda.memory_allocated() - before))
        s.close()
        drawn_frames += sum(int(t.shape[0]) for _, t in s.take_drawn())
        assert drawn_frames == len(paths)
        print("   online session with draw: pixel ring %d slots, %.1f MB; device memory held above the resident model: %s" % (
            s.cap_frames, s.ring_px.numel() / 1e6, ", ".join("after %d frames %.1f MB" % (n, m / 1e6) for n, m in held)))
    model.close()


def gather_part(rounds):
    dev = torch.device("cuda:0")
    fr, rows = overlay_bench.video(44, 32, seed=44)
    H, W, cap = fr.shape[1], fr.shape[2], 41
    ring = torch.randint(0, 256, (cap, H, W, 3), dtype=torch.uint8, device=dev)
    table = [(25 + i) % cap for i in range(32)]                    # a push whose slots wrap
    slots = torch.tensor(table, dtype=torch.int32, device=dev)
    ring[slots.long()] = torch.from_numpy(fr).to(dev)
    scene = show._scene_of_rows(rows, 37, show.Atlas(), H, W, True)
    arrays = show.device_arrays(scene, dev)
    up, face, line, _ = arrays
    (_, _, _, boxes, woff, inst_off, inst_rgb, label_off, label_pos, label_glyph, label_rgb, gwh, gwoff, gwords) = up
    show.launch(ring, scene, arrays, slots=slots)                  # fills the two word buffers
    out = torch.empty((32, H, W, 3), dtype=torch.uint8, device=dev)
    rest = (face, line, boxes, woff, inst_off, inst_rgb, label_off, label_pos, label_glyph, label_rgb, gwh, gwoff, gwords,
            show.A_FACE, show.A_BOX)
    idx = slots.long()

    def gather():
        return ops.overlay_compose(ring, *rest, out=out, slots=slots)

    def chain():
        sel = ring.index_select(0, idx)
        return ops.overlay_compose(sel, *rest, out=sel)
    assert torch.equal(gather(), chain())
    print("gather: 32 frames %d x %d out of a ring of %d slots, 44 rows per frame [same bytes]" % (W, H, cap))
    for name, fn in (("gather-compose launch", gather), ("index_select + dense compose in place", chain)):
        ts = [t * 1e6 for t in overlay_bench.event_times(fn, rounds, 10)]
        print("   %-40s %s" % (name, fmt(ts, "us")))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--frames", type=int, default=400)
    ap.add_argument("--parts", default="show,stream,gather")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "online_draw_bench needs the GPU"
    tmp = tempfile.mkdtemp()
    try:
        for part in args.parts.split(","):
            if part == "show":
                show_part(tmp, args.rounds)
            elif part == "stream":
                stream_part(tmp, args.rounds, args.frames)
            elif part == "gather":
                gather_part(args.rounds)
            sys.stdout.flush()
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
