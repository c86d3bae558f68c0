"""Time the lexicon match of `python -m gomatching_amd.lexicon` on one synthetic video: 100 frames of 44 rows whose
transcriptions are corrupted copies (0 to 3 random edits) of words of a seeded synthetic vocabulary of 90 000 words of 3 to 12
letters -- no real vocabulary file ships with the project.  The distinct strings of the video are the queries.

One process.  The numpy path (`lexicon.host_match`) and the device path (`lexicon.device_match`: one upload, one launch, one
copy back, the window ending when both result arrays are on the host) alternate after a warm-up of both, median and range of
--rounds.  The numpy path is too slow to repeat over all queries, so it is TIMED on the first --host-queries of them (the
figure for all is that time scaled by the query count, and is labelled so); its distances for the first --check-queries
queries (all of them where the lexicon is small; the queries are in shuffled order) are computed once, untimed, and the
device path's index and distance of each of those queries is compared with them.  Then the launch alone between device
events, as cell updates per second: a cell is one (query character, word character) pair of the dynamic programme, counted
over all (query, word) pairs and over the pairs the kernel actually evaluates -- the kernel's prune is replayed on the host
from those distances (lane t of 256 visits the words t, t + 256, .. and skips one whose length differs from the query's by at
least the lane's running best).  The same again with the video's own 50-word lexicon as the one segment.  Last, the whole
command in this process beside the json parse and the dump it wraps.

    python tools/lexicon_bench.py > profiles/lexicon_bench.log
"""
import argparse
import os
import random
import shutil
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gomatching_amd import lexicon, ops, results                   # noqa: E402

LETTERS = "abcdefghijklmnopqrstuvwxyz"
THREADS = 256                                                      # LX_THREADS of csrc/lexicon.hip


def say(*a):
    print(*a, flush=True)


def stats(ts):
    ts = sorted(ts)
    return ts[len(ts) // 2], ts[0], ts[-1]


def corrupt(rng, word, edits):
    s = list(word)
    for _ in range(edits):
        kind, pos = rng.randrange(3), rng.randrange(len(s) + 1)
        if kind == 0 or not s:
            s.insert(pos, rng.choice(LETTERS))
        elif kind == 1:
            del s[min(pos, len(s) - 1)]
        else:
            s[min(pos, len(s) - 1)] = rng.choice(LETTERS)
    return "".join(s)


def make_video(rng, words, frames=100, rows=44):
    """-> ({frame: [rows]}, the tracks' words): track k reads its word with 0..3 edits in every frame."""
    base = [rng.choice(words) for _ in range(rows)]
    ann = {}
    for f in range(frames):
        ann[str(f + 1)] = []
        for k, w in enumerate(base):
            text = corrupt(rng, w, rng.choice((0, 0, 0, 1, 1, 2, 2, 3))).upper()
            x, y = 10 + 20 * (k % 11) + f % 7, 10 + 40 * (k // 11)
            quad = [x, y, x + 60, y, x + 60, y + 24, x, y + 24]
            ann[str(f + 1)].append(quad + [k + 1, text, [[[x, y], [x + 60, y], [x + 60, y + 24], [x, y + 24]]]])
    return ann, base


def replay_prune(d, lens, m):
    """Which words lane-strided scanning with the exact prune evaluates, from all distances `d` [n]: bool [n]."""
    n = d.size
    pad = (-n) % THREADS
    dd = np.concatenate([d, np.full(pad, 1000)]).reshape(-1, THREADS)
    ll = np.concatenate([lens, np.full(pad, 10 ** 6)]).reshape(-1, THREADS)
    # a lane's best before iteration r: min(100, the distances it EVALUATED earlier); a skipped word has d >= that best, so
    # the minimum over all earlier words is the same number
    run = np.minimum.accumulate(np.vstack([np.full((1, THREADS), lexicon.NO_MATCH_DIST), dd[:-1]]), axis=0)
    return (np.abs(ll - m) < run).reshape(-1)[:n]


def time_launch(csr, max_len, args):
    """The launch alone between device events, on resident arguments -> (median, min, max) seconds per launch."""
    dev = [torch.from_numpy(a).cuda() for a in csr]
    out = torch.empty((2, csr[2].size), dtype=torch.int32, device="cuda")
    fn = lambda: ops.lexicon_match(*dev, max_len=max_len, out=out)  # noqa: E731
    fn()
    ts = []
    for _ in range(args.rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(args.launches):
            fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) * 1e-3 / args.launches)
    return stats(ts)


def leg(name, items, lexicons, args):
    q_chars, q_off = lexicon.pack([s for _, s in items])
    q_seg = np.asarray([g for g, _ in items], dtype=np.int32)
    w_chars, w_off = lexicon.pack([w for lex in lexicons for w in lex.normal])
    seg_off = np.zeros(len(lexicons) + 1, dtype=np.int32)
    np.cumsum([len(lex) for lex in lexicons], out=seg_off[1:])
    csr = (q_chars, q_off, q_seg, w_chars, w_off, seg_off)
    S, W = q_seg.size, w_off.size - 1
    qlen, wlen = np.diff(q_off).astype(np.int64), np.diff(w_off).astype(np.int64)
    say("---- %s: %d queries (%d code points), %d words (%d code points) in %d segment(s)" % (name, S, q_chars.size, W, w_chars.size, len(lexicons)))

    # all distances of the first `nc` queries (the queries are in shuffled order) once, untimed: the comparison, and the replay
    # of the prune
    nc = S if W * S <= 2000000 else min(args.check_queries, S)
    t0 = time.perf_counter()
    h_index, h_dist = np.empty(nc, np.int32), np.empty(nc, np.int32)
    cells_all = cells_eval = pairs_all = pairs_eval = 0
    mats = {}
    for s in range(nc):
        g = int(q_seg[s])
        if g not in mats:
            mats[g] = lexicon.segment_matrix(w_chars, w_off, int(seg_off[g]), int(seg_off[g + 1]))
        mat, lens = mats[g]
        d = lexicon.distances(q_chars[q_off[s]:q_off[s + 1]], mat, lens)
        k = int(np.argmin(d))
        h_index[s], h_dist[s] = k, d[k]
        ev = replay_prune(d.astype(np.int64), lens, int(qlen[s]))
        cells_all += int(qlen[s]) * int(lens.sum())
        cells_eval += int(qlen[s]) * int(lens[ev].sum())
        pairs_all += lens.size
        pairs_eval += int(ev.sum())
    say("numpy distances of the first %d of %d queries, once, untimed leg: %.1f s" % (nc, S, time.perf_counter() - t0))
    d_index, d_dist = lexicon.device_match(*csr)                    # warm-up of the device path, and the comparison
    same = bool(np.array_equal(h_index, d_index[:nc]) and np.array_equal(h_dist, d_dist[:nc]))
    say("outputs identical on both paths: %s (%d indices, %d distances compared; accepted at <= 1 among all %d: %d)"
        % (same, nc, nc, S, int((d_dist <= 1).sum())))

    nh = min(args.host_queries, S)
    part = (q_chars[:q_off[nh]], q_off[:nh + 1], q_seg[:nh], w_chars, w_off, seg_off)
    lexicon.host_match(*part)
    times = {"numpy": [], "device": []}
    for _ in range(args.rounds):
        for key, fn, a in (("numpy", lexicon.host_match, part), ("device", lexicon.device_match, csr)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn(*a)
            times[key].append(time.perf_counter() - t0)
    hm, hlo, hhi = stats(times["numpy"])
    dm, dlo, dhi = stats(times["device"])
    say("numpy  path, the first %d of %d queries: %9.2f ms  (median of %d, min %.2f max %.2f)  %.3f ms per query; scaled to all "
        "queries: %.1f s (not measured as a whole)" % (nh, S, hm * 1e3, args.rounds, hlo * 1e3, hhi * 1e3, hm / nh * 1e3, hm / nh * S))
    say("device path, all %d queries, upload + launch + copy back: %9.2f ms  (median of %d, min %.2f max %.2f)" % (S, dm * 1e3, args.rounds, dlo * 1e3, dhi * 1e3))
    say("numpy (scaled) / device ratio, end to end: %.0f" % (hm / nh * S / dm))

    k, klo, khi = time_launch(csr, int(max(qlen.max(), wlen.max())), args)
    say("launch alone: %9.1f us (min %.1f max %.1f; median of %d x %d launches)" % (k * 1e6, klo * 1e6, khi * 1e6, args.rounds, args.launches))
    share_p, share_c = pairs_eval / max(pairs_all, 1), cells_eval / max(cells_all, 1)
    say("of the %d checked queries: pairs %d, evaluated %d (%.1f %%; the rest pruned by length); cells %d, evaluated %d (%.1f %%)"
        % (nc, pairs_all, pairs_eval, 100.0 * share_p, cells_all, cells_eval, 100.0 * share_c))
    total_pairs = sum(int((q_seg == g).sum()) * int(seg_off[g + 1] - seg_off[g]) for g in range(len(lexicons)))
    total_cells = sum(int(qlen[q_seg == g].sum()) * int(wlen[seg_off[g]:seg_off[g + 1]].sum()) for g in range(len(lexicons)))
    say("the launch: %d pairs, %d cells in all (exact)%s" % (total_pairs, total_cells,
        "" if nc == S else "; evaluated = the checked queries' shares applied to these totals"))
    say("cell updates per second: %.3e over the evaluated cells, %.3e over all cells; %.3f ns per evaluated pair, %.3f ns per pair"
        % (total_cells * share_c / k, total_cells / k, k / max(total_pairs * share_p, 1) * 1e9, k / max(total_pairs, 1) * 1e9))
    return same


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--words", type=int, default=90000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--host-queries", type=int, default=48, help="queries the numpy path is timed on")
    ap.add_argument("--check-queries", type=int, default=256,
                    help="queries whose numpy distances are compared and whose prune is replayed when all would take too long")
    ap.add_argument("--no-command", action="store_true", help="skip the whole-command leg")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("lexicon_bench: no GPU; nothing is measured without one")
    rng = random.Random(2024)
    words = ["".join(rng.choice(LETTERS) for _ in range(rng.randint(3, 12))) for _ in range(args.words)]
    ann, base = make_video(rng, words)
    strings = sorted(set(lexicon.norm(r[9]) for rows in ann.values() for r in rows))
    rng.shuffle(strings)
    say("device: %s" % torch.cuda.get_device_name(0))
    say("video: %d frames x %d rows = %d rows, %d distinct strings" % (len(ann), 44, sum(len(r) for r in ann.values()), len(strings)))
    big = lexicon.Lexicon(words, {lexicon.norm(w): w for w in words})
    strong_words = sorted(set(base))
    strong_words += [w for w in words[:200] if w not in strong_words][:50 - len(strong_words)]
    strong = lexicon.Lexicon(strong_words, {lexicon.norm(w): w for w in strong_words})
    same = leg("generic lexicon", [(0, s) for s in strings], [big], args)
    same = leg("the video's own 50-word lexicon", [(0, s) for s in strings], [strong], args) and same

    if not args.no_command:
        tmp = tempfile.mkdtemp(prefix="lexicon_bench_")
        try:
            res = os.path.join(tmp, "res")
            os.makedirs(os.path.join(res, "jsons"))
            os.makedirs(os.path.join(res, "preds"))
            results.write_video_results(ann, os.path.join(res, "jsons", "video.json"), os.path.join(res, "preds", "res_video.xml"))
            results.write_track_transcriptions(os.path.join(res, "preds"))
            big_path, strong_dir = os.path.join(tmp, "generic.txt"), os.path.join(tmp, "strong")
            os.makedirs(strong_dir)
            for path, ws in ((big_path, words), (os.path.join(strong_dir, "video.txt"), strong_words)):
                with open(path, "w", encoding="utf-8") as f:
                    f.write("".join(w + "\n" for w in ws))
            say("---- the command: RES/jsons/video.json is %.2f MB" % (os.path.getsize(os.path.join(res, "jsons", "video.json")) / 1e6))
            t0 = time.perf_counter()
            lexicon.load_lexicon(big_path)
            t_load = time.perf_counter() - t0
            t0 = time.perf_counter()
            parsed = lexicon.read_annotation(os.path.join(res, "jsons", "video.json"))
            t_parse = time.perf_counter() - t0
            t0 = time.perf_counter()
            dump = os.path.join(tmp, "dump")
            os.makedirs(os.path.join(dump, "preds"))
            results.write_video_results(parsed, os.path.join(dump, "video.json"), os.path.join(dump, "preds", "res_video.xml"))
            results.write_track_transcriptions(os.path.join(dump, "preds"))
            t_dump = time.perf_counter() - t0
            say("what the command wraps: loading the %d-word lexicon %.3f s, json parse %.3f s, json + xml + txt dump %.3f s"
                % (len(words), t_load, t_parse, t_dump))
            trees = {}
            for name, extra in (("generic, device", ["--lexicon", big_path]), ("strong, device", ["--lexicon", strong_dir]),
                                ("strong, numpy", ["--lexicon", strong_dir, "--host-match"])):
                out = os.path.join(tmp, name.replace(", ", "_"))
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                status = lexicon.main(["--results", res, "--output", out] + extra)
                say("command, %-15s: %7.3f s (status %d)" % (name, time.perf_counter() - t0, status))
                trees[name] = {f: open(os.path.join(dp, f), "rb").read() for dp, _, fs in os.walk(out) for f in fs}
            same_files = trees["strong, device"] == trees["strong, numpy"] and len(trees["strong, numpy"]) == 3
            say("command outputs byte-identical on both paths (strong lexicon): %s; the generic lexicon's command was run on the "
                "device path only (numpy: see the scaled figure above)" % same_files)
            same = same and same_files
        finally:
            shutil.rmtree(tmp, ignore_errors=True)
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
