"""Time JPEG decoding of source frames: 100 files of 1280 x 720 at quality 95, 4:2:0, as Pillow writes them (no restart markers:
one segment per file) and with a restart interval per MCU row (45 segments per file).  One process, the paths alternating,
after a warm-up of each; median and range over the rounds; the outputs are asserted equal first:
  pillow x1 / x4   `eval.read_frame`'s decode (from bytes in memory) on one thread / on the command's pool of DECODE_THREADS
  device path      from the files' bytes on the host to pixels resident in HBM: `jpeg.parse` + `jpeg.plan` (the host's share,
                   timed apart as well), three uploads, four launches, the copy of the status words
  launches         the entropy launch (+ the status fold) and the two pixel launches apart, between device events, over a
                   workspace and uploads made once; and a device-to-device copy of the output's bytes for scale
and the spotting of one video of --frames frames from a tree of .jpg files the way `eval` does it with and without
--device-decode (`read_frame` on the pool + `results.spot_video` against `eval.spot_video_device_decode`; the bench's own model
set-up, as tools/online_bench.py): seconds reading and decoding, frames/s over the whole run, and the largest growth of the
process's resident set over the run (sampled after the read and after every chunk; /proc/self/statm).

    python tools/jpeg_decode_bench.py [--frames 400] [--rounds 5] > profiles/jpeg_decode_bench.log

--chunks measures the chunked entropy walk (walk="chunks") against the segment walk (walk="segments", the baseline) instead: the
same 100 files as Pillow writes them, with restart_marker_rows 8 and 1, and a noisier set (the pass count depends on content).
Per set, pixels asserted equal to Pillow's for every row first, then, alternating, median and range over the rounds of the
entropy launch alone (segments; chunks at 64 .. 1024 bytes, with the largest `passes` word and the count of segments routed to
the serial walk) and of the path from file bytes to pixels (segments, chunks at the default, Pillow's pool); then the video with
and without the flag, the flag with --decode-walk segments and auto.

    python tools/jpeg_decode_bench.py --chunks [--frames 400] [--rounds 5] > profiles/jpeg_decode_chunks_bench.log
"""
import argparse
import io
import os
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from gomatching_amd import eval as E                                      # noqa: E402
from gomatching_amd import jpeg, ops, results                             # noqa: E402
from overlay_bench import event_times, stats                             # noqa: E402

QUALITY = 95


def rss():
    with open("/proc/self/statm") as f:
        return int(f.read().split()[1]) * os.sysconf("SC_PAGE_SIZE")


def pillow_decode(blob):
    from PIL import Image
    with Image.open(io.BytesIO(blob)) as im:
        return np.ascontiguousarray(np.asarray(im.convert("RGB"))[:, :, ::-1])


def encode(frames, **kw):
    from PIL import Image
    out = []
    for f in frames:
        buf = io.BytesIO()
        Image.fromarray(np.ascontiguousarray(f[:, :, ::-1])).save(buf, "JPEG", quality=QUALITY, **kw)
        out.append(buf.getvalue())
    return out


def decode_part(name, blobs, rounds, dev):
    H, W = 720, 1280

    def pillow_path(n):
        with ThreadPoolExecutor(max_workers=n) as pool:
            return list(pool.map(pillow_decode, blobs))

    def host_share():
        return jpeg.plan(blobs, [jpeg.parse(b) for b in blobs])

    def device_path():
        out, status = ops.jpeg_decode(host_share(), True, dev)
        return out, status.cpu()

    out, status = device_path()
    want = np.stack(pillow_path(E.DECODE_THREADS))
    same = int(status.abs().sum()) == 0 and bool((out.cpu().numpy() == want).all())
    assert same, "device pixels and Pillow's differ"
    times = {"pillow x1": [], "pillow x%d" % E.DECODE_THREADS: [], "device path": [], "  of it parse + plan": []}
    for _ in range(rounds):
        for key, fn in (("pillow x1", lambda: pillow_path(1)), ("pillow x%d" % E.DECODE_THREADS, lambda: pillow_path(E.DECODE_THREADS)),
                        ("device path", device_path), ("  of it parse + plan", host_share)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times[key].append(time.perf_counter() - t0)

    # the launches alone
    p = host_share()
    L = ops._L()
    F, nseg, nsets = p.F, p.desc.shape[0], p.sets.shape[0]
    geo = (F, p.H, p.W, p.ncomp, p.hs, p.vs)
    nbytes = L.gom_jpeg_decode_workspace_bytes(*geo)
    data = np.zeros(((len(p.data) + 3) // 4 * 4,), dtype=np.uint8)
    data[:len(p.data)] = p.data
    d_data, d_desc = torch.from_numpy(data).to(dev), torch.from_numpy(p.desc).to(dev)
    d_off, d_fs, d_sets = torch.from_numpy(p.seg_off).to(dev), torch.from_numpy(p.frame_set).to(dev), torch.from_numpy(p.sets).to(dev)
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
    seg_st, fr_st = torch.empty((nseg,), dtype=torch.int32, device=dev), torch.empty((F,), dtype=torch.int32, device=dev)
    pixels = torch.empty((F, H, W, 3), dtype=torch.uint8, device=dev)

    def entropy():
        ops.check(L.gom_jpeg_decode_entropy_i16(ops._p(d_data), len(p.data), ops._p(d_desc), nseg, ops._p(d_off), ops._p(d_sets), nsets,
                                                *geo, ops._p(ws), nbytes, ops._p(seg_st), ops._p(fr_st), ops._stream()))

    def pix():
        ops.check(L.gom_jpeg_decode_pixels_u8(ops._p(d_sets), nsets, ops._p(d_fs), *geo, 1, ops._p(ws), nbytes, ops._p(pixels), ops._stream()))
    entropy()
    pix()
    assert bool((pixels == out).all())
    t_ent, t_pix = event_times(entropy, rounds, 3), event_times(pix, rounds, 10)
    dst = torch.empty_like(pixels)
    t_copy = event_times(lambda: dst.copy_(pixels), rounds, 10)
    med = lambda ts: sorted(ts)[len(ts) // 2]
    print("%s: %d files of %d x %d, %d segments, %d table set(s); device pixels == Pillow's: %s" % (name, F, W, H, nseg, nsets, same))
    print("  bytes to the device: %.1f MB of pixels without --device-decode, %.1f MB of entropy bytes + %.2f MB of descriptors and "
          "tables with it; workspace %.0f MB" % (pixels.numel() / 1e6, len(p.data) / 1e6,
                                                 (p.desc.nbytes + p.sets.nbytes + p.seg_off.nbytes + p.frame_set.nbytes) / 1e6, nbytes / 1e6))
    for key in times:
        print("  %-28s %s" % (key, stats(times[key])))
    print("  %-28s %s" % ("launches: entropy + status", stats(t_ent)))
    print("  %-28s %s  %.1f MB written: %.3f TB/s" % ("launches: idct + colour", stats(t_pix), pixels.numel() / 1e6,
                                                     pixels.numel() / med(t_pix) / 1e12))
    print("  %-28s %s  %.1f MB read (and as much written): %.3f TB/s" % ("device-to-device copy", stats(t_copy), pixels.numel() / 1e6,
                                                                        pixels.numel() / med(t_copy) / 1e12))


CHUNK_SWEEP = (64, 128, 256, 512, 1024)


def chunks_part(name, blobs, rounds, dev):
    H, W = 720, 1280
    p = jpeg.plan(blobs, [jpeg.parse(b) for b in blobs])
    L = ops._L()
    F, nseg, nsets = p.F, p.desc.shape[0], p.sets.shape[0]
    geo = (F, p.H, p.W, p.ncomp, p.hs, p.vs)
    nbytes = L.gom_jpeg_decode_workspace_bytes(*geo)
    data = np.zeros(((len(p.data) + 3) // 4 * 4,), dtype=np.uint8)
    data[:len(p.data)] = p.data
    d_data, d_desc = torch.from_numpy(data).to(dev), torch.from_numpy(p.desc).to(dev)
    d_off, d_fs, d_sets = torch.from_numpy(p.seg_off).to(dev), torch.from_numpy(p.frame_set).to(dev), torch.from_numpy(p.sets).to(dev)
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
    seg_st, fr_st = torch.empty((nseg,), dtype=torch.int32, device=dev), torch.empty((F,), dtype=torch.int32, device=dev)
    info = torch.empty((nseg, 2), dtype=torch.int32, device=dev)
    pixels = torch.empty((F, H, W, 3), dtype=torch.uint8, device=dev)
    head = (ops._p(d_data), len(p.data), ops._p(d_desc), nseg, ops._p(d_off), ops._p(d_sets), nsets) + geo + \
           (ops._p(ws), nbytes, ops._p(seg_st), ops._p(fr_st))

    def entropy(chunk):
        if chunk is None:
            ops.check(L.gom_jpeg_decode_entropy_i16(*head, ops._stream()))
        else:
            ops.check(L.gom_jpeg_decode_entropy_chunks_i16(*head, chunk, ops._p(info), ops._stream()))

    def pix():
        ops.check(L.gom_jpeg_decode_pixels_u8(ops._p(d_sets), nsets, ops._p(d_fs), *geo, 1, ops._p(ws), nbytes, ops._p(pixels), ops._stream()))

    def pillow_path():
        with ThreadPoolExecutor(max_workers=E.DECODE_THREADS) as pool:
            return list(pool.map(pillow_decode, blobs))

    want = torch.from_numpy(np.stack(pillow_path())).to(dev)
    variants = (None,) + CHUNK_SWEEP
    notes = {}
    for chunk in variants:                                                   # equal pixels first, for every row
        ws.fill_(0x5A)
        entropy(chunk)
        pix()
        assert int(fr_st.abs().sum()) == 0 and bool((pixels == want).all()), "device pixels and Pillow's differ (chunk %r)" % (chunk,)
        if chunk is not None:
            notes[chunk] = (int(info[:, 1].max()), int((info[:, 0] != 0).sum()))
    times = {chunk: [] for chunk in variants}
    for r in range(rounds + 1):                                              # alternating; the first round warms up
        for chunk in variants:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(3):
                entropy(chunk)
            b.record()
            torch.cuda.synchronize()
            if r:
                times[chunk].append(a.elapsed_time(b) * 1e-3 / 3)
    t_pix = event_times(pix, rounds, 10)

    def device_path(walk):
        def run():
            plan = jpeg.plan(blobs, [jpeg.parse(b) for b in blobs])
            out, status = ops.jpeg_decode(plan, True, dev, walk=walk)
            return out, status.cpu()
        return run
    paths = {"pillow x%d" % E.DECODE_THREADS: pillow_path, "device path, segments": device_path("segments"),
             "device path, chunks %d" % jpeg.CHUNK_BYTES: device_path("chunks")}
    t_path = {k: [] for k in paths}
    for r in range(rounds + 1):
        for key, fn in paths.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if r:
                t_path[key].append(time.perf_counter() - t0)
    med = lambda ts: sorted(ts)[len(ts) // 2]
    mean_seg = float((p.desc[:, 1] - p.desc[:, 0]).sum()) / nseg
    print("%s: %d files of %d x %d, %.1f MB of entropy bytes, %d segments of %.0f bytes in the mean (auto: %s); pixels == Pillow's "
          "on every row: True" % (name, F, W, H, len(p.data) / 1e6, nseg, mean_seg, jpeg.resolve_walk("auto", p)))
    base = med(times[None])
    print("  %-34s %s" % ("entropy launch, segments", stats(times[None])))
    for chunk in CHUNK_SWEEP:
        print("  %-34s %s  %6.2fx segments; ranges %s; most passes %d, serial route %d of %d"
              % ("entropy launch, chunks %d" % chunk, stats(times[chunk]), base / med(times[chunk]),
                 "apart" if max(times[chunk]) < min(times[None]) or min(times[chunk]) > max(times[None]) else "overlap",
                 notes[chunk][0], notes[chunk][1], nseg))
    print("  %-34s %s" % ("launches: idct + colour", stats(t_pix)))
    for key in paths:
        print("  %-34s %s" % (key, stats(t_path[key])))
    return {chunk: med(times[chunk]) for chunk in variants}


def eval_part(frames, rounds, dev):
    import bench
    from gomatching_amd.config import setup_cfg
    from gomatching_amd.predictor import GoMBatchPredictor, TextDecoder, new_time_cost
    from gomatching_amd.synth import make_clip
    cfg = setup_cfg(builtin="icdar15")
    cfg.MODEL.DEVICE = "cuda"
    base = [np.ascontiguousarray(f[:, :, ::-1]) for f in make_clip(100, bench.SRC_HW[0], bench.SRC_HW[1], clip_id=0, num_rects=12)]
    blobs = encode(base)
    model, _ = bench.build_model(cfg, dev)
    cal, _ = GoMBatchPredictor(cfg, None).prepare([pillow_decode(blobs[0])])
    bench.calibrate(model, [dict(x, image=x["image"].to(dev)) for x in cal], frac=0.3)
    spotter = GoMBatchPredictor(cfg, model, device_ingest=True)
    dec = TextDecoder(cfg.MODEL.TRANSFORMER.VOC_SIZE)
    tmp = tempfile.mkdtemp()
    video = os.path.join(tmp, "ICDAR15_frames", "Video_1_1_1")
    os.makedirs(video)
    for i in range(frames):                                                  # back and forth: no jump
        with open(os.path.join(video, "%d.jpg" % (i + 1)), "wb") as f:
            f.write(blobs[i % 100] if (i // 100) % 2 == 0 else blobs[99 - i % 100])
    paths = E.frame_paths(video)
    runs = [0]

    def plain(pool):
        runs[0] += 1
        r0, t0 = rss(), time.perf_counter()
        fr = list(pool.map(E.read_frame, paths))
        read, grow = time.perf_counter() - t0, rss() - r0
        preds, _ = results.spot_video(spotter, fr, new_time_cost())
        out = os.path.join(tmp, "plain%d" % runs[0])
        results.write_video(preds, "Video_1_1_1", "ICDAR15", out, dec, device_rows=True)
        return time.perf_counter() - t0, read, max(grow, rss() - r0), out

    def flagged(pool, walk="auto"):
        runs[0] += 1
        counts = {k: 0 for k in E.DECODE_ROUTES}
        r0, t0 = rss(), time.perf_counter()
        grow = [0]

        class Probe(dict):                                                   # a time_cost that samples the resident set per chunk
            def __setitem__(self, k, v):
                if k == "total_time":
                    grow[0] = max(grow[0], rss() - r0)
                dict.__setitem__(self, k, v)
        preds, _, read = E.spot_video_device_decode(spotter, pool, paths, Probe(new_time_cost()), counts, dev, walk=walk)
        out = os.path.join(tmp, "flag%d" % runs[0])
        results.write_video(preds, "Video_1_1_1", "ICDAR15", out, dec, device_rows=True)
        assert counts["device"] == len(paths), counts
        return time.perf_counter() - t0, read, max(grow[0], rss() - r0), out

    def same(a, b):
        for sub, name in (("preds", "res_video_1.xml"), ("jsons", "Video_1_1_1.json")):
            with open(os.path.join(a, sub, name), "rb") as fa, open(os.path.join(b, sub, name), "rb") as fb:
                if fa.read() != fb.read():
                    return False
        return True

    res = {"eval": [], "eval --device-decode --decode-walk segments": [], "eval --device-decode": []}
    with ThreadPoolExecutor(max_workers=E.DECODE_THREADS) as pool:
        a, b, c = plain(pool), flagged(pool, "segments"), flagged(pool)      # warm-up, and the comparison
        equal = same(a[3], b[3]) and same(a[3], c[3])
        assert equal, "result files differ"
        for _ in range(rounds):
            res["eval"].append(plain(pool))
            res["eval --device-decode --decode-walk segments"].append(flagged(pool, "segments"))
            res["eval --device-decode"].append(flagged(pool))
    print("one video of %d frames 1280 x 720 from .jpg files (%.1f MB on disk), offline, result files bytewise equal: %s"
          % (frames, sum(os.path.getsize(p) for p in paths) / 1e6, equal))
    for key, rs in res.items():
        med = lambda i: sorted(r[i] for r in rs)[len(rs) // 2]
        print("  %-46s %7.1f frames/s (%.1f .. %.1f); reading + decoding %6.3f s (%.3f .. %.3f); resident set grows by %7.1f MB (%.1f .. %.1f)"
              % (key, frames / med(0), frames / max(r[0] for r in rs), frames / min(r[0] for r in rs), med(1), min(r[1] for r in rs),
                 max(r[1] for r in rs), med(2) / 1e6, min(r[2] for r in rs) / 1e6, max(r[2] for r in rs) / 1e6))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--frames", type=int, default=400)
    ap.add_argument("--skip-eval", action="store_true")
    ap.add_argument("--chunks", action="store_true", help="the chunked entropy walk against the segment walk")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "jpeg_decode_bench needs the GPU"
    dev = torch.device("cuda:0")
    print("device: %s" % torch.cuda.get_device_name(0))
    from gomatching_amd.synth import make_clip
    frames = [np.ascontiguousarray(f[:, :, ::-1]) for f in make_clip(100, 720, 1280, clip_id=0, num_rects=12)]
    if args.chunks:
        print("walk=\"chunks\": default chunk %d bytes, auto from a mean segment length of %d bytes" % (jpeg.CHUNK_BYTES, jpeg.AUTO_SEGMENT_BYTES))
        chunks_part("no restart markers", encode(frames), args.rounds, dev)
        chunks_part("a restart interval per 8 MCU rows", encode(frames, restart_marker_rows=8), args.rounds, dev)
        chunks_part("a restart interval per MCU row", encode(frames, restart_marker_rows=1), args.rounds, dev)
        rng = np.random.RandomState(5)
        noisy = [np.clip(f.astype(np.int16) + rng.randint(-24, 25, size=f.shape), 0, 255).astype(np.uint8) for f in frames]
        chunks_part("no restart markers, noise of +-24 added", encode(noisy), args.rounds, dev)
    else:
        decode_part("no restart markers", encode(frames), args.rounds, dev)
        decode_part("a restart interval per MCU row", encode(frames, restart_marker_rows=1), args.rounds, dev)
    if not args.skip_eval:
        eval_part(args.frames, args.rounds, dev)


if __name__ == "__main__":
    main()
