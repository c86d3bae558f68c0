"""The corrected result files of one video, OUT/lexicon/{jsons,preds}, written by the end-of-run host step
(`lexicon.correct_results` after `results.write_video(device_text=True, device_vote=True)`: the baseline, what
`eval --device-write --device-vote --lexicon L` does) and by the device path (`write_video(lexicon=RowCorrection)`,
csrc/lexicon_rows.hip: what `--device-lexicon` adds), on the 400-frame 1280x720 video of tools/result_text_bench.py and the
seeded 90 000-word vocabulary of tools/lexicon_bench.py, one process, the paths alternating, median and range.  Every second
distinct transcription of the video itself is put into the vocabulary, and every word has a display form that differs from
it (a pair list), so that rows are accepted and take a display form: the run asserts that some do (with the synthetic weights
all kept rows of this video carry ONE transcription, so all of them do; rows that are not accepted are the business of
tests/test_eval_device_lexicon_gpu.py).  The files of both paths are compared byte for byte before anything is timed.

  write stage   seconds for the video's predictions (already on the GPU) -> all six files, per path; the baseline split into the
                original files and the host step, the device path's "lexicon" seconds (the added launches, their one read back
                and the copy of the corrected text) shown beside it.
  one chunk     the added launches of one 100-frame chunk, device time between two synchronisations: all of them (queries,
                match, apply, the `_ov` text, the `_ov` records), and the match launch alone -- it sees every row, not every
                distinct string.  The synthetic weights give the video's rows few distinct transcriptions, so the match launch is
                also timed on as many queries made the way tools/lexicon_bench.py makes them: lexicon words with 0 to 3 random
                edits, all different.

    python tools/lexicon_rows_bench.py [--frames 400] [--words 90000] [--rounds 5] > profiles/lexicon_rows_bench.log
"""
import argparse
import json
import os
import random
import statistics
import string
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench                                                       # noqa: E402  (build_model / calibrate: the bench's own set-up)
from gomatching_amd import lexicon, ops, results                    # noqa: E402
from gomatching_amd.config import setup_cfg                        # noqa: E402
from gomatching_amd.predictor import GoMBatchPredictor, TextDecoder, new_time_cost   # noqa: E402
from gomatching_amd.synth import make_clip                         # noqa: E402

VIDEO, STEM = "Video_1_1_1", "video_1"


def fmt(xs, unit="s"):
    return "%9.4f %s (%.4f .. %.4f)" % (statistics.median(xs), unit, min(xs), max(xs))


def baseline(preds, out, dec, lex_path, pair_path, split):
    t0 = time.perf_counter()
    results.write_video(preds, VIDEO, "ICDAR15", out, dec, device_rows=True, device_text=True, rows=False, device_vote=True)
    t1 = time.perf_counter()
    figures = lexicon.correct_results(out, None, lex_path, pair_path, 1, "keep")
    t2 = time.perf_counter()
    split.setdefault("original files", []).append(t1 - t0)
    split.setdefault("host step", []).append(t2 - t1)
    return t2 - t0, figures


def device(preds, out, dec, lex, split):
    timing = {}
    fix = lexicon.RowCorrection(lexicon.DeviceLexicon.of(lex, dec, torch.device("cuda:0")), 1, "keep", video=VIDEO)
    t0 = time.perf_counter()
    results.write_video(preds, VIDEO, "ICDAR15", out, dec, device_rows=True, device_text=True, rows=False, device_vote=True,
                        timing=timing, lexicon=fix)
    dt = time.perf_counter() - t0
    split.setdefault("lexicon", []).append(timing.get("lexicon", 0.0))
    return dt, fix


def files(out):
    return {sub + "/" + f: open(os.path.join(out, sub, f), "rb").read()
            for sub in ("jsons", "preds", "lexicon/jsons", "lexicon/preds") for f in sorted(os.listdir(os.path.join(out, sub)))}


def timed(fn, rounds):
    out = []
    for _ in range(rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=400)
    ap.add_argument("--words", type=int, default=90000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--detect-frac", type=float, default=0.3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("lexicon_rows_bench: no GPU; nothing is measured without one")
    dev = torch.device("cuda:0")
    cfg = setup_cfg(builtin="icdar15")
    cfg.MODEL.DEVICE = "cuda"
    base = [np.ascontiguousarray(f[:, :, ::-1]) for f in make_clip(100, bench.SRC_HW[0], bench.SRC_HW[1], clip_id=0, num_rects=12)]
    clip = [base[i % 100] if (i // 100) % 2 == 0 else base[99 - i % 100] for i in range(args.frames)]
    model, _ = bench.build_model(cfg, dev)
    cal, _ = GoMBatchPredictor(cfg, None).prepare(clip[:1])
    shift, _ = bench.calibrate(model, [dict(x, image=x["image"].to(dev)) for x in cal], frac=args.detect_frac)
    spotter = GoMBatchPredictor(cfg, model, device_ingest=True)
    dec = TextDecoder(cfg.MODEL.TRANSFORMER.VOC_SIZE)
    rng = random.Random(2024)
    words = ["".join(rng.choice(string.ascii_lowercase) for _ in range(rng.randint(3, 12))) for _ in range(args.words)]
    tmp = tempfile.mkdtemp(prefix="lexicon_rows_bench_")
    print("torch %s, %s; %d frames %dx%d, %d queries, class-bias shift %+.3f, frames_per_step %d, %d words, %d rounds"
          % (torch.__version__, torch.cuda.get_device_name(0), len(clip), bench.SRC_HW[1], bench.SRC_HW[0],
             cfg.MODEL.TRANSFORMER.NUM_QUERIES, shift, model.frames_per_step, len(words), args.rounds))
    preds, window = results.spot_video(spotter, clip, new_time_cost())
    n_rows = sum(len(r["instances"]) for r in preds)
    # ---- the vocabulary: the seeded words plus every second distinct transcription of the video, display forms that differ
    results.write_video(preds, VIDEO, "ICDAR15", os.path.join(tmp, "t"), dec, device_rows=True, device_text=True, rows=False)
    with open(os.path.join(tmp, "t", "jsons", VIDEO + ".json"), encoding="utf-8") as f:
        own = sorted({r["transcription"] for rows in json.load(f).values() for r in rows
                      if r["transcription"] and r["transcription"].split() == [r["transcription"]]})
    taken = own[::2]
    lex_words = words + [t for t in taken if t not in set(words)]
    lex_path, pair_path = os.path.join(tmp, "generic.txt"), os.path.join(tmp, "pairs.txt")
    with open(lex_path, "w", encoding="utf-8") as f:
        f.write("".join(w + "\n" for w in lex_words))
    with open(pair_path, "w", encoding="utf-8") as f:
        f.write("".join("%s <%s> & co\n" % (w.upper(), w.capitalize()) for w in lex_words))
    lex = lexicon.load_lexicon(lex_path, pair_path)
    print("vocabulary: %d seeded words + %d of the video's %d distinct transcriptions, a pair list of display forms \"<Word> & co\""
          % (len(words), len(lex_words) - len(words), len(own)))

    # ---- the files first
    _, figures = baseline(preds, os.path.join(tmp, "h0"), dec, lex_path, pair_path, {})
    _, fix = device(preds, os.path.join(tmp, "d0"), dec, lex, {})
    fh, fd = files(os.path.join(tmp, "h0")), files(os.path.join(tmp, "d0"))
    assert sorted(fh) == sorted(fd) and all(fh[k] == fd[k] for k in fh), "the device path's files differ from the host step's"
    assert fix.accepted > 0 and figures["changed"] > 0, "the comparison needs rows that take a display form"
    print("files equal: %d files; %d instances in, %d kept rows, %d accepted, %d dropped (host step: %d rows, %d distinct, %d changed); "
          "%.1f MB of corrected JSON" % (len(fh), n_rows, fix.rows, fix.accepted, fix.dropped, figures["rows"], figures["distinct"],
                                         figures["changed"], len(fh["lexicon/jsons/%s.json" % VIDEO]) / 1e6))

    # ---- the write stage, the paths alternating
    th, td, sh, sd = [], [], {}, {}
    for r in range(args.rounds):
        th.append(baseline(preds, os.path.join(tmp, "h%d" % (r + 1)), dec, lex_path, pair_path, sh)[0])
        td.append(device(preds, os.path.join(tmp, "d%d" % (r + 1)), dec, lex, sd)[0])
    print("\nthe write stage: predictions on the GPU -> six files, %d frames (median and range of %d)" % (len(clip), args.rounds))
    print("  --device-write --device-vote, then the host step (baseline)  %s" % fmt(th))
    for k in ("original files", "host step"):
        print("      %-24s %s" % (k, fmt(sh[k])))
    print("  with --device-lexicon                                        %s" % fmt(td))
    print("      %-24s %s" % ("of which lexicon", fmt(sd["lexicon"])))
    print("  baseline / device path   %8.2f x" % (statistics.median(th) / statistics.median(td)))

    # ---- one chunk: the added launches, and the match alone
    part = [r["instances"] for r in preds[:results.TEXT_FRAMES_PER_CALL]]
    live = [x for x in part if len(x)]
    bd = torch.cat([x.bd.detach().reshape(-1, 25, 4) for x in live]).to(torch.float32)
    recs = torch.cat([x.recs.detach().reshape(-1, 25) for x in live]).to(torch.int64)
    ids = torch.cat([x.track_ids.detach().reshape(-1) for x in live]).to(device=dev, dtype=torch.int64)
    words_d = ops.result_rows(bd, recs, dec.voc_size, ids)
    frame_rows = np.concatenate(([0], np.cumsum([len(x) for x in part]))).astype(np.int32)
    pts, keep = results.finish_points(words_d.cpu().numpy())
    pts_d, keep_d = torch.from_numpy(pts).to(dev), torch.from_numpy(keep.astype(np.uint8)).to(dev)
    dl = lexicon.DeviceLexicon.of(lex, dec, dev)
    n = int(words_d.shape[0])
    seg = torch.zeros((n,), dtype=torch.int32, device=dev)
    q_chars, q_off, q_len, q_status = ops.lexicon_rows_queries(words_d, keep_d, dl.norm_tab)
    one = lexicon.RowCorrection(dl, 1, "keep", results.TrackVote(dec), video=VIDEO)
    added = timed(lambda: results.corrected_text(words_d, pts_d, keep_d, frame_rows, 0, dec, one), 4 * args.rounds)
    match = timed(lambda: ops.lexicon_match(q_chars, q_off, seg, dl.w_chars, dl.w_off, dl.seg_off, max_len=lexicon.MAX_LEN),
                  4 * args.rounds)
    queries = timed(lambda: ops.lexicon_rows_queries(words_d, keep_d, dl.norm_tab), 4 * args.rounds)
    edited = []
    for _ in range(n):                                          # (tools/lexicon_bench.py `corrupt`: substitute, delete or insert)
        w = list(rng.choice(words))
        for _ in range(rng.randint(0, 3)):
            kind, at = rng.randint(0, 2), rng.randint(0, max(len(w) - 1, 0))
            if kind == 0 and w:
                w[at] = rng.choice(string.ascii_lowercase)
            elif kind == 1 and len(w) > 1:
                del w[at]
            else:
                w.insert(at, rng.choice(string.ascii_lowercase))
        edited.append(lexicon.norm("".join(w)))
    e_chars, e_off = (torch.from_numpy(a).to(dev) for a in lexicon.pack(edited))
    match_edited = timed(lambda: ops.lexicon_match(e_chars, e_off, seg, dl.w_chars, dl.w_off, dl.seg_off, max_len=lexicon.MAX_LEN),
                         4 * args.rounds)
    distinct = len(set(tuple(q) for q in np.split(q_chars.cpu().numpy()[:int(q_off[-1])], q_off.cpu().numpy()[1:-1])))
    chunk_ms = window / len(clip) * len(part) * 1e3
    print("\none chunk of %d frames, %d rows (%d kept), device time between two synchronisations (median and range of %d)"
          % (len(part), n, int(keep.sum()), 4 * args.rounds))
    print("  all added launches + their read back   %s" % fmt(added, "ms"))
    print("  the three query launches               %s" % fmt(queries, "ms"))
    print("  the match launch, %5d queries         %s   (%d distinct strings among them)" % (n, fmt(match, "ms"), distinct))
    print("  the match launch, %5d edited words    %s   (%d distinct)" % (n, fmt(match_edited, "ms"), len(set(edited))))
    print("  the chunk's detector and tracker time  %9.1f ms: the match is %.2f %% of it, %.2f %% on the edited words"
          % (chunk_ms, 100.0 * statistics.median(match) / chunk_ms, 100.0 * statistics.median(match_edited) / chunk_ms))


if __name__ == "__main__":
    main()
