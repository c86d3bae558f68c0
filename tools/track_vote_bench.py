"""preds/res_<video>.txt of one video written by the host step (`results.write_track_transcriptions` over the video's XML: the
baseline, what `eval` does without the flag) and by the device vote (`results.TrackVote`, csrc/track_vote.hip), one process,
the paths alternating, median and range.  The txt files of both paths are compared byte for byte before anything is timed.

  video A    the 400-frame 1280x720 video of tools/online_bench.py (ICDAR15 config, synthetic weights, the benchmark's own
             model set-up and class-bias calibration).
  video B    a synthetic 3000-frame video of 100 rows per frame: 99 row slots whose track changes every 150 frames and one
             track that spans the whole video; a row reads one of its track's three words (60 / 25 / 15 %).

  host       `write_track_transcriptions` on a directory that holds the video's XML alone (written by `--device-write`'s path).
  device     end to end: one records launch per 100-frame call, the ordering (stable sort, cut into tracks), the vote, the
             scan and the emit, the copy back and the file write.  The words and keep flags of every call are on the device
             when the clock starts, as they are in `results.rows_text`.
  launches   the records, vote + scan and emit launches alone, by events on the stream (the ordering left out).
  command    frames/s of `results.spot_video` + `results.write_video(device_text=True)` on video A, with the host step at the
             end and with the device vote.

    python tools/track_vote_bench.py [--frames 400] [--long-frames 3000] [--rounds 5] > profiles/track_vote_bench.log
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
from gomatching_amd import lib, ops, results                       # noqa: E402
from gomatching_amd.config import setup_cfg                        # noqa: E402
from gomatching_amd.predictor import GoMBatchPredictor, TextDecoder, new_time_cost   # noqa: E402
from gomatching_amd.synth import make_clip                         # noqa: E402


def fmt(xs, unit="s"):
    return "%8.4f %s (%.4f .. %.4f)" % (statistics.median(xs), unit, min(xs), max(xs))


class Rows:
    """What the writers read of a frame's Instances."""

    def __init__(self, bd, recs, track_ids):
        self.bd, self.recs, self.track_ids = bd, recs, track_ids

    def __len__(self):
        return int(self.bd.shape[0])


def synthetic_video(frames, rows, span, dev, seed=5):
    rng = np.random.RandomState(seed)
    slot = np.arange(rows)
    x0, y0 = 10.0 + (slot % 10) * 120.0, 10.0 + (slot // 10) * 70.0
    t = np.arange(25, dtype=np.float32) / 24.0
    bd = np.zeros((rows, 25, 4), dtype=np.float32)
    bd[:, :, 0] = bd[:, :, 2] = x0[:, None] + 100.0 * t[None, :]
    bd[:, :, 1] = y0[:, None]
    bd[:, :, 3] = y0[:, None] + 40.0
    bd_d = torch.from_numpy(bd).to(dev)
    words = {}                                                     # track id -> three variants of 25 class ids (36 is the blank)

    def variants(tid):
        if tid not in words:
            v = np.full((3, 25), 36, dtype=np.int64)
            for k in range(3):
                n = rng.randint(3, 11)
                v[k, 0:2 * n:2] = rng.randint(0, 36, size=n)       # a blank between two characters: nothing collapses
            words[tid] = v
        return words[tid]

    out = []
    for f in range(frames):
        ids = np.where(slot == rows - 1, 10 ** 6, slot * 1000 + (f + slot * 7) // span)
        pick = rng.choice(3, size=rows, p=[0.6, 0.25, 0.15])
        recs = np.stack([variants(int(i))[p] for i, p in zip(ids, pick)])
        out.append({"instances": Rows(bd_d, torch.from_numpy(recs).to(dev), torch.from_numpy(ids.astype(np.int64)).to(dev))})
    return out


def calls_of(preds, dec):
    """The (words, keep) pair of every 100-frame call, on the device: what `rows_text` hands to the vote."""
    out = []
    insts = [r["instances"] for r in preds]
    for first in range(0, len(insts), results.TEXT_FRAMES_PER_CALL):
        live = [x for x in insts[first:first + results.TEXT_FRAMES_PER_CALL] if len(x)]
        if not live:
            continue
        bd = torch.cat([x.bd.detach().reshape(-1, 25, 4) for x in live]).to(torch.float32)
        recs = torch.cat([x.recs.detach().reshape(-1, 25) for x in live]).to(torch.int64)
        ids = torch.cat([x.track_ids.detach().reshape(-1) for x in live]).to(device=bd.device, dtype=torch.int64)
        words_d = ops.result_rows(bd, recs, dec.voc_size, ids)
        _, keep = results.finish_points(words_d.cpu().numpy())
        out.append((words_d, torch.from_numpy(keep.astype(np.uint8)).to(bd.device)))
    return out


def device_vote(calls, dec, path):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    vote = results.TrackVote(dec)
    for words_d, keep_d in calls:
        vote.add(words_d, keep_d)
    data = vote.finish()
    with open(path, "wb") as f:
        f.write(data)
    return time.perf_counter() - t0


def launches_alone(calls, dec):
    """Milliseconds by events: the records launches, then the vote + scan and the emit on a prepared ordering."""
    K = lib.CONSTANTS
    dev = calls[0][0].device
    table = results.device_txt_table(dec, dev)
    e = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    torch.cuda.synchronize()
    e[0].record()
    parts = [ops.track_vote_records(w, k, table) for w, k in calls]
    e[1].record()
    records = torch.cat(parts)
    m = records.shape[0]
    ids = records[:, :2].contiguous().view(torch.int64).reshape(m)
    voters = torch.nonzero(records[:, K["GOM_TV_LEN"]] != K["GOM_TV_LEN_DROPPED"]).reshape(-1)
    sorted_ids, perm = torch.sort(ids[voters], stable=True)
    order = voters[perm].to(torch.int32)
    track_ids, sizes = torch.unique_consecutive(sorted_ids, return_counts=True)
    T, nv = int(track_ids.shape[0]), int(voters.shape[0])
    seg = torch.zeros((T + 1,), dtype=torch.int32, device=dev)
    seg[1:] = torch.cumsum(sizes, 0)
    winner = torch.empty((T, K["GOM_TV_WINNER_WORDS"]), dtype=torch.int32, device=dev)
    line_off = torch.empty((T + 1,), dtype=torch.int64, device=dev)
    totals = torch.empty((K["GOM_TV_TOTALS"],), dtype=torch.int64, device=dev)
    p = ops._p
    v = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    torch.cuda.synchronize()
    v[0].record()
    ops._call("gom_track_vote_count_scan", p(records), m, p(order), nv, p(seg), T, p(winner), p(line_off), p(totals), ops._stream())
    v[1].record()
    total, status = totals.tolist()
    assert status == 0
    out = torch.empty((total,), dtype=torch.uint8, device=dev)
    v[2].record()
    ops._call("gom_track_vote_emit", p(records), m, p(winner), p(line_off), T, p(out), total, ops._stream())
    v[3].record()
    torch.cuda.synchronize()
    return e[0].elapsed_time(e[1]), v[0].elapsed_time(v[1]), v[2].elapsed_time(v[3]), m, T, int(sizes.max().item())


def measure(name, preds, dec, tmp, rounds):
    out = os.path.join(tmp, name)
    results.write_video(preds, "Video_1_1_1", "ICDAR15", out, dec, device_text=True, rows=False)
    xml_dir = os.path.join(out, "preds")
    txt = os.path.join(xml_dir, "res_video_1.txt")
    dev_txt = os.path.join(tmp, name + "_device.txt")
    calls = calls_of(preds, dec)
    # ---- the files first
    results.write_track_transcriptions(xml_dir)
    device_vote(calls, dec, dev_txt)
    want, got = open(txt, "rb").read(), open(dev_txt, "rb").read()
    assert want == got, "the device vote's txt differs from the host's"
    through = os.path.join(tmp, name + "_flag")                     # and through write_video itself
    results.write_video(preds, "Video_1_1_1", "ICDAR15", through, dec, device_text=True, rows=False, device_vote=True)
    assert open(os.path.join(through, "preds", "res_video_1.txt"), "rb").read() == want
    ms = launches_alone(calls, dec)
    print("\nvideo %s: %d frames, %d rows, %d tracks (the longest %d rows), %.1f MB of XML, %d bytes of txt; files equal"
          % (name, len(preds), ms[3], ms[4], ms[5], os.path.getsize(os.path.join(xml_dir, "res_video_1.xml")) / 1e6, len(want)))
    th, td, tl = [], [], []
    for _ in range(rounds):
        t0 = time.perf_counter()
        results.write_track_transcriptions(xml_dir)
        th.append(time.perf_counter() - t0)
        td.append(device_vote(calls, dec, dev_txt))
        tl.append(launches_alone(calls, dec)[:3])
    print("  host step (baseline)       %s" % fmt(th))
    print("  device vote, end to end    %s" % fmt(td))
    print("  host / device              %8.1f x" % (statistics.median(th) / statistics.median(td)))
    for k, label in enumerate(("records launches", "vote + scan launches", "emit launch")):
        print("      %-22s %s" % (label, fmt([x[k] for x in tl], "ms")))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=400)
    ap.add_argument("--long-frames", type=int, default=3000)
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
    print("torch %s, %s; video A %d frames %dx%d, %d queries, class-bias shift %+.3f, frames_per_step %d; %d rounds"
          % (torch.__version__, torch.cuda.get_device_name(0), len(clip), bench.SRC_HW[1], bench.SRC_HW[0],
             cfg.MODEL.TRANSFORMER.NUM_QUERIES, shift, model.frames_per_step, args.rounds))
    tmp = tempfile.mkdtemp()
    preds, _ = results.spot_video(spotter, clip, new_time_cost())
    measure("A", preds, dec, tmp, args.rounds)

    # ---- the whole command per video: spotting and writing, the host step at the end against the device vote
    fh, fd = [], []
    for r in range(args.rounds):
        for vote, acc in ((False, fh), (True, fd)):
            out = os.path.join(tmp, "c%d%d" % (r, vote))
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            p, _ = results.spot_video(spotter, clip, new_time_cost())
            results.write_video(p, "Video_1_1_1", "ICDAR15", out, dec, device_text=True, rows=False, device_vote=vote)
            if not vote:
                results.write_track_transcriptions(os.path.join(out, "preds"))
            acc.append(len(clip) / (time.perf_counter() - t0))
            del p
    print("\nspot_video + write_video(device_text=True) + txt, video A, frames already decoded (median and range of %d)" % args.rounds)
    print("  --device-write, host step  %s" % fmt(fh, "frames/s"))
    print("  --device-write --device-vote %s" % fmt(fd, "frames/s"))
    del preds

    if args.long_frames:
        measure("B", synthetic_video(args.long_frames, 100, 150, dev), dec, tmp, args.rounds)


if __name__ == "__main__":
    main()
