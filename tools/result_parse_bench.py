"""Measure reading result JSON on the GPU (`show --device-read`) against the path the tree keeps behind the absent flag:
json.loads + `show.rows_of_json` + `show._scene_of_rows`.  One process, the two paths alternating, median and range over the
rounds, outputs asserted equal first.  None of it is a gate.

  inputs   the 100-frame video of tools/overlay_bench.py (44 rows per frame, 1280 x 720) and a 400-frame video made the same
           way (the rows only: 17 600 instances), each as the text the result writer writes (json.dumps(indent=4,
           ensure_ascii=False)).
  rows     a video's rows and the scenes of its chunks of 100 frames, both ways, each step apart; on the new path the host's
           label work (anchors, label colours, atlas indices, the chunk's label arrays) is split out.
  launches the three parse calls with their reads between device events against a device-to-device copy of as many bytes; the
           scene launches of one chunk alone.
  bytes    up (the file) and back (the compact arrays).
  command  `python -m gomatching_amd.show --device-decode --device-encode` (called in-process) on the 100-frame video with and
           without `--device-read`.

    python tools/result_parse_bench.py [--rounds 5] > profiles/result_parse_bench.log
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
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import overlay_bench                                               # noqa: E402
from gomatching_amd import ops, results, show                      # noqa: E402

H, W = overlay_bench.H, overlay_bench.W


def fmt(xs, unit="ms"):
    return "median %9.2f %s (%.2f .. %.2f, n = %d)" % (statistics.median(xs), unit, min(xs), max(xs), len(xs))


def rows_only(per_frame, frames, seed):
    """The rows of `overlay_bench.video` without its frames."""
    rng = np.random.RandomState(seed)
    base = [overlay_bench.curved_polygon(rng) for _ in range(per_frame)]
    rows = []
    for f in range(frames):
        fr = []
        for k, c in enumerate(base):
            poly = c + rng.randint(-3, 4, size=2)
            fr.append([0] * 8 + [k + 1, overlay_bench.WORDS[(k + f // 25) % len(overlay_bench.WORDS)], [poly.tolist()]])
        rows.append(fr)
    return rows


def text_of(rows):
    a = {str(f + 1): [{"points": r[:8], "ID": r[8], "transcription": r[9], "segmentation": r[10]} for r in fr]
         for f, fr in enumerate(rows)}
    return json.dumps(a, indent=4, ensure_ascii=False).encode("utf-8")


class Clock:
    """Wall milliseconds of named steps, the device idle at both ends of each."""

    def __init__(self):
        self.ms = {}

    @contextlib.contextmanager
    def step(self, name):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        yield
        torch.cuda.synchronize()
        self.ms[name] = self.ms.get(name, 0.0) + (time.perf_counter() - t0) * 1e3


def baseline(text, atlas, clock):
    with clock.step("json.loads"):
        doc = json.loads(text.decode("utf-8"))
    with clock.step("rows_of_json"):
        ann = show.rows_of_json(doc)
        rows = [ann[str(i + 1)] for i in range(len(ann))]
    scenes = []
    with clock.step("_scene_of_rows"):
        for f0 in range(0, len(rows), show.CHUNK):
            scenes.append(show._scene_of_rows(rows[f0:f0 + show.CHUNK], 37, atlas, H, W, True))
    with clock.step("upload of the scenes"):
        arrays = [show.device_arrays(s, torch.device("cuda:0")) for s in scenes]
    return scenes, arrays


def device_read(text, atlas, clock, dev):
    with clock.step("parse_json_device"):
        parsed = results.parse_json_device(text, dev)
    assert parsed.status == 0
    with clock.step("host labels: anchors, colours"):
        scenes = show.ParsedScenes(parsed, 37, atlas)
    with clock.step("host labels: atlas indices"):
        for f0 in range(0, parsed.F, show.CHUNK):
            f1 = min(f0 + show.CHUNK, parsed.F)
            scenes.glyphs(show.font_px(H, W), int(parsed.frame_rows[f0]), int(parsed.frame_rows[f1]))
    out = []
    with clock.step("chunks: scene_polygons, label arrays, upload"):
        for f0 in range(0, parsed.F, show.CHUNK):
            out.append(scenes.chunk(f0, min(f0 + show.CHUNK, parsed.F), H, W, dev))
    return parsed, out


def same_scenes(host_scenes, dev_chunks):
    for s, (dims, (arr, face, line, area)) in zip(host_scenes, dev_chunks):
        ms = s.mset
        want = [ms.points.astype(np.int32), ms.coff.astype(np.int32), ms.mcoff.astype(np.int32), ms.boxes.astype(np.int32),
                ms.woff.astype(np.int64), s.inst_off, s.inst_rgb, s.label_off, s.label_pos, s.label_glyph, s.label_rgb,
                s.glyph_wh.astype(np.int32), s.glyph_woff.astype(np.int64), s.glyph_words.astype(np.uint32).view(np.int32)]
        for g, w in zip(arr, want):
            if not np.array_equal(g.cpu().numpy().reshape(w.shape), w):
                return False
    return len(host_scenes) == len(dev_chunks)


def rows_part(name, rows, rounds, dev):
    text = text_of(rows)
    n = sum(len(fr) for fr in rows)
    atlas_a, atlas_b = show.Atlas(), show.Atlas()
    hs, _ = baseline(text, atlas_a, Clock())                      # warm-up of both paths, and the comparison
    parsed, chunks = device_read(text, atlas_b, Clock(), dev)
    assert parsed.to_annotation() == show.rows_of_json(json.loads(text.decode("utf-8")))
    assert same_scenes(hs, chunks)
    back = sum(getattr(parsed, k).nbytes for k in ("frame_rows", "ids", "t_off", "t_len", "has_seg", "poly_off", "poly_xy"))
    print("%s: %d frames, %d instances, %d points; file %d bytes up (%.0f per instance), %d bytes back (%.0f per instance); "
          "rows and scenes of the two paths equal: True" % (name, len(rows), n, parsed.P, len(text), len(text) / n, back, back / n))
    del hs, chunks
    a, b = {}, {}
    for _ in range(rounds):
        ca, cb = Clock(), Clock()
        baseline(text, atlas_a, ca)
        device_read(text, atlas_b, cb, dev)
        for k, v in ca.ms.items():
            a.setdefault(k, []).append(v)
        for k, v in cb.ms.items():
            b.setdefault(k, []).append(v)
    print("   json.load path:")
    for k in a:
        print("      %-48s %s" % (k, fmt(a[k])))
    print("      %-48s %s" % ("all of it", fmt([sum(v[i] for v in a.values()) for i in range(rounds)])))
    print("   --device-read path:")
    for k in b:
        print("      %-48s %s" % (k, fmt(b[k])))
    print("      %-48s %s" % ("all of it", fmt([sum(v[i] for v in b.values()) for i in range(rounds)])))
    print("      %-48s %s" % ("of which host label work",
                              fmt([sum(v[i] for k, v in b.items() if k.startswith("host labels")) for i in range(rounds)])))
    # ---- the launches alone
    buf = torch.frombuffer(bytearray(text), dtype=torch.uint8).to(dev)
    ts = [t * 1e3 for t in overlay_bench.event_times(lambda: ops.result_parse(buf), rounds, 3)]
    print("   parse calls alone (three calls, three reads)        %s" % fmt(ts))
    ts = [t * 1e3 for t in overlay_bench.event_times(lambda: buf.clone(), rounds, 3)]
    print("   device-to-device copy of the file's %9d bytes  %s" % (len(text), fmt(ts)))
    f1 = min(show.CHUNK, parsed.F)
    i1 = int(parsed.frame_rows[f1])
    d = parsed.dev
    pal = show._device_palette(dev)
    kept = int((np.diff(parsed.poly_off[:i1 + 1]) > 0).sum())
    fn = lambda: ops.scene_polygons(d["frame_rows"], d["ids"], d["poly_off"], d["poly_xy"], 0, f1, i1, kept, 0,
                                    int(parsed.poly_off[i1]), H, W, pal, True)
    ts = [t * 1e6 for t in overlay_bench.event_times(fn, rounds, 10)]
    print("   scene launches alone, one chunk of %d frames, %d instances   %s" % (f1, i1, fmt(ts, "us")))


def command_part(tmp, rounds):
    from online_draw_bench import files, write_jpegs
    fr, rows = overlay_bench.video(44, 100, seed=44)
    data = os.path.join(tmp, "ICDAR15_show")
    write_jpegs(fr, os.path.join(data, "Video_1_1_1"))
    del fr
    res = os.path.join(tmp, "show_results")
    os.makedirs(os.path.join(res, "jsons"))
    with open(os.path.join(res, "jsons", "Video_1_1_1.json"), "wb") as fp:
        fp.write(text_of(rows))
    base = ["--device-decode", "--device-encode"]
    paths = {"--device-decode --device-encode": base, "--device-decode --device-encode --device-read": base + ["--device-read"]}
    runs = [0]

    def run(flags):
        runs[0] += 1
        out = os.path.join(tmp, "show_out%d" % runs[0])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with contextlib.redirect_stdout(io.StringIO()):
            status = show.main(["--input", data, "--results", res, "--output", out] + flags)
        assert status == 0
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out
    got = [files(run(flags)[1]) for flags in paths.values()]
    assert got[0] == got[1] and len(got[0]) == 100
    print("show command, 100 frames 1280 x 720, 44 rows per frame; pictures with --device-read equal those without: True")
    for d in os.listdir(tmp):
        if d.startswith("show_out"):
            shutil.rmtree(os.path.join(tmp, d))
    times = {n: [] for n in paths}
    for _ in range(rounds):
        for name, flags in paths.items():
            dt, out = run(flags)
            times[name].append(dt * 1e3)
            shutil.rmtree(out)
    for name in paths:
        print("   %-50s %s" % (name, fmt(times[name])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--parts", default="rows100,rows400,command")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "result_parse_bench needs the GPU"
    dev = torch.device("cuda:0")
    print("torch %s, %s" % (torch.__version__, torch.cuda.get_device_name(0)))
    tmp = tempfile.mkdtemp()
    try:
        for part in args.parts.split(","):
            if part == "rows100":
                rows_part("100-frame video", rows_only(44, 100, 44), args.rounds, dev)
            elif part == "rows400":
                rows_part("400-frame video", rows_only(44, 400, 44), args.rounds, dev)
            elif part == "command":
                command_part(tmp, args.rounds)
            sys.stdout.flush()
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
