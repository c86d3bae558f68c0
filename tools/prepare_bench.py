"""Time the quad -> Bezier step of `python -m gomatching_amd.prepare` on one synthetic dataset of 1 000 000 quads drawn from
the families of tests/test_prepare_gpu.py (tests/prepare_statement.py, seeded).  One process; the numpy path
(`prepare.quad_bezier_host`) and the device path (`prepare.quad_bezier_device`: one upload, one launch, one copy back, the
window ending when the 16 integers per quad are on the host) alternate after a warm-up of both, median and range of
--rounds; the outputs of the two are compared in the same run.  Then the launch alone between device events, with the bytes it
has to move (40 in, 64 out per quad) per second beside a device-to-device copy that moves the same number of bytes (half of
them read, half written).  Last, the whole `bezier` command in this process, once per path, on a json with one annotation
per quad: parsing and dumping are part of that window.

    python tools/prepare_bench.py > profiles/prepare_bench.log
"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import prepare_statement as S                                      # noqa: E402  (the input families)
from gomatching_amd import ops, prepare                            # noqa: E402


def say(*a):
    print(*a, flush=True)


def stats(ts):
    ts = sorted(ts)
    return ts[len(ts) // 2], ts[0], ts[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quads", type=int, default=1000000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--no-command", action="store_true", help="skip the whole-command leg")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("prepare_bench: no GPU; nothing is measured without one")
    n = args.quads
    quads, hw, fam = S.mixed_batch(n)
    say("dataset: %d quads, %d families (%s), %d image sizes" % (n, len(S.FAMILIES), ", ".join(S.FAMILIES), len(S.SIZES)))
    say("device: %s" % torch.cuda.get_device_name(0))

    host = prepare.quad_bezier_host(quads, hw)                      # warm-up of both paths, and the comparison
    dev = prepare.quad_bezier_device(quads, hw)
    same = bool(np.array_equal(host, dev))
    say("outputs identical on both paths: %s (%d words)" % (same, host.size))
    if n <= 50000:
        say("outputs identical to the plain-Python statement: %s" % bool(np.array_equal(S.quad_bezier_all(quads, hw), dev)))
    times = {"numpy": [], "device": []}
    for _ in range(args.rounds):
        for name, fn in (("numpy", prepare.quad_bezier_host), ("device", prepare.quad_bezier_device)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn(quads, hw)
            times[name].append(time.perf_counter() - t0)
    med = {}
    for name in ("numpy", "device"):
        med[name], lo, hi = stats(times[name])
        say("%-6s path: %9.2f ms per dataset  %7.4f us per quad   (median of %d, min %.2f max %.2f ms)"
            % (name, med[name] * 1e3, med[name] / n * 1e6, args.rounds, lo * 1e3, hi * 1e3))
    say("numpy / device ratio, end to end: %.2f" % (med["numpy"] / med["device"]))

    # the launch alone, and a device-to-device copy that moves as many bytes
    dq, dhw = torch.from_numpy(quads).cuda(), torch.from_numpy(hw).cuda()
    moved = n * (32 + 8 + 64)
    src = torch.empty(moved // 2, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)

    def events(fn):
        fn()
        out = []
        for _ in range(args.rounds):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(args.launches):
                fn()
            b.record()
            torch.cuda.synchronize()
            out.append(a.elapsed_time(b) * 1e-3 / args.launches)
        return stats(out)

    k, klo, khi = events(lambda: ops.quad_bezier(dq, dhw))
    c, clo, chi = events(lambda: dst.copy_(src))
    say("launch alone: %8.1f us (min %.1f max %.1f; median of %d x %d launches)  %.3f ns per quad  %.1f GB/s over %d bytes"
        % (k * 1e6, klo * 1e6, khi * 1e6, args.rounds, args.launches, k / n * 1e9, moved / k * 1e-9, moved))
    say("d2d copy:     %8.1f us (min %.1f max %.1f)  %.1f GB/s over the same %d bytes (read + written)" % (c * 1e6, clo * 1e6, chi * 1e6, moved / c * 1e-9, moved))
    say("launch / copy time: %.2f" % (k / c))

    if not args.no_command:
        tmp = tempfile.mkdtemp(prefix="prepare_bench_")
        try:
            sizes = sorted(set(map(tuple, hw.tolist())))
            image_of = {s: i + 1 for i, s in enumerate(sizes)}
            doc = {"images": [{"file_name": "v/%d.jpg" % i, "id": i, "height": s[0], "width": s[1], "frame_id": i, "prev_image_id": -1,
                               "next_image_id": -1, "video_id": 1} for s, i in image_of.items()],
                   "annotations": [{"id": k + 1, "category_id": 1, "text_category": "alphanumeric", "transcription": "text", "image_id": image_of[s],
                                    "instance_id": k + 1, "bbox": [0, 0, 1, 1], "poly": q, "anno_type": "word", "box_type": "quadrilateral",
                                    "iscrowd": 0} for k, (q, s) in enumerate(zip(quads.reshape(n, 4, 2).tolist(), map(tuple, hw.tolist())))],
                   "categories": prepare.CATEGORIES, "videos": [{"id": 1, "file_name": "v", "data_source": "synthetic"}]}
            src_json = os.path.join(tmp, "in.json")
            with open(src_json, "w", encoding="utf-8") as f:
                json.dump(doc, f)
            del doc
            say("command input: %s, %.1f MB" % (os.path.basename(src_json), os.path.getsize(src_json) / 1e6))
            outs = {}
            for name, extra in (("device", []), ("numpy", ["--host-bezier"])):
                outs[name] = os.path.join(tmp, name + ".json")
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                status = prepare.main(["bezier", "--json", src_json, "--output", outs[name]] + extra)
                t = time.perf_counter() - t0
                say("bezier command, %-6s path: %7.2f s (status %d, output %.1f MB); the quad step is %.2f %% of it"
                    % (name, t, status, os.path.getsize(outs[name]) / 1e6, med[name] / t * 100))
            with open(outs["device"], "rb") as f, open(outs["numpy"], "rb") as g:
                same_files = f.read() == g.read()
            say("command outputs byte-identical: %s" % same_files)
            same = same and same_files
        finally:
            shutil.rmtree(tmp, ignore_errors=True)
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
