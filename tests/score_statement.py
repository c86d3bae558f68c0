"""Plain statements of what the scoring feature computes (shared by test_score_cpu.py and test_score_gpu.py; no test in
here).

1. `fixture_video`: the seeded synthetic video the GPU tests run on.
2. `write_tree`: ground-truth and result files of a small synthetic method, written with the package's own writers.
3. The geometry of one (ground truth, detection) pair in numpy float64 -- what `gom_quad_pairs_*_f64` (csrc/score.hip) and
   `score.host_quad_pairs` compute: convex hull of each 4-gon by Andrew's monotone chain on integer cross products (popping on
   cross <= 0: any point order, duplicate and collinear points collapse), 0 when either hull has no area, otherwise the
   detection hull clipped by every edge of the ground-truth hull (Sutherland-Hodgman, inside = cross >= 0, a crossing at
   prev + t (cur - prev) with t = dp / (dp - dc)) and the shoelace area; IoU = inter / (area_g + area_d - inter), overlap =
   inter / area_d.  Written the direct way, with hulls of their true length: the kernel's four-slot hulls with repeated
   vertices are an implementation matter that must not show.
4. `pairs_statement`: the count / emit contract over a whole video, pair by pair.
"""
import os

import numpy as np


# ------------------------------------------------------------------------------------------ 3. geometry of one pair
def hull(quad):
    """8 integers -> the hull's points, counter-clockwise (y up) from the smallest (x, y), as Python integers."""
    pts = sorted(set((int(quad[2 * i]), int(quad[2 * i + 1])) for i in range(4)))
    if len(pts) <= 2:
        return pts

    def cross(o, a, b):
        return (a[0] - o[0]) * (b[1] - o[1]) - (a[1] - o[1]) * (b[0] - o[0])
    lower, upper = [], []
    for p in pts:
        while len(lower) >= 2 and cross(lower[-2], lower[-1], p) <= 0:
            lower.pop()
        lower.append(p)
    for p in reversed(pts):
        while len(upper) >= 2 and cross(upper[-2], upper[-1], p) <= 0:
            upper.pop()
        upper.append(p)
    return lower[:-1] + upper[:-1]


def area2(poly):
    """Twice the signed area of an integer polygon (exact)."""
    return sum(poly[i - 1][0] * poly[i][1] - poly[i][0] * poly[i - 1][1] for i in range(len(poly)))


def clip(subject, clipper):
    """Sutherland-Hodgman: `subject` (list of float64 points) inside every edge of the counter-clockwise `clipper`."""
    f = np.float64
    poly = [(f(x), f(y)) for x, y in subject]
    for k in range(len(clipper)):
        if not poly:
            break
        ax, ay = f(clipper[k][0]), f(clipper[k][1])
        bx, by = f(clipper[(k + 1) % len(clipper)][0]), f(clipper[(k + 1) % len(clipper)][1])
        ex, ey = bx - ax, by - ay
        out = []
        px, py = poly[-1]
        dp = ex * (py - ay) - ey * (px - ax)
        for cx, cy in poly:
            dc = ex * (cy - ay) - ey * (cx - ax)
            if (dc >= 0) != (dp >= 0):
                t = dp / (dp - dc)
                out.append((px + t * (cx - px), py + t * (cy - py)))
            if dc >= 0:
                out.append((cx, cy))
            px, py, dp = cx, cy, dc
        poly = out
    return poly


def pair_value(gt_quad, det_quad, measure):
    """measure 0: IoU of the two hulls; 1: intersection over the detection hull's area.  float64."""
    hg, hd = hull(gt_quad), hull(det_quad)
    if len(hg) < 3 or len(hd) < 3:
        return 0.0
    ag2, ad2 = area2(hg), area2(hd)
    if ag2 <= 0 or ad2 <= 0:
        return 0.0
    poly = clip(hd, hg)
    if len(poly) < 3:
        return 0.0
    s = np.float64(0.0)
    px, py = poly[-1]
    for cx, cy in poly:
        s = s + (px * cy - cx * py)
        px, py = cx, cy
    inter = abs(s) * np.float64(0.5)
    ag, ad = np.float64(ag2) * 0.5, np.float64(ad2) * 0.5
    if measure == 1:
        return float(inter / ad)
    uni = ag + ad - inter
    return 0.0 if uni == 0 else float(inter / uni)


# ------------------------------------------------------------------------------------------ 4. a whole video
def pairs_statement(gt_quads, det_quads, gt_off, det_off, gt_key, det_key, measure, threshold):
    """-> (counts [G], kept [(g, detection index within the frame, value)] ordered by g, then detection,
    eligible [(g, j, value)] for EVERY pair of equal keys, kept or not)."""
    G = len(gt_quads)
    counts, kept, eligible = np.zeros(G, dtype=np.int32), [], []
    for f in range(len(gt_off) - 1):
        for g in range(int(gt_off[f]), int(gt_off[f + 1])):
            for j in range(int(det_off[f + 1]) - int(det_off[f])):
                d = int(det_off[f]) + j
                if int(gt_key[g]) != int(det_key[d]):
                    continue
                v = pair_value(gt_quads[g], det_quads[d], measure)
                eligible.append((g, j, v))
                if v > threshold:
                    counts[g] += 1
                    kept.append((g, j, v))
    return counts, kept, eligible


# ------------------------------------------------------------------------------------------ 1. the GPU tests' video
def fixture_video(seed=20240917, frames=40):
    """40 frames of random integer quads: 1-6 ground-truth boxes per frame (8-80 px, corners jittered by up to 6 px);
    detections = the same boxes jittered by up to 9 px, each kept with probability 0.85, plus 0-2 strays per frame.
    -> dict of int32 arrays: gt_quads, det_quads, gt_off, det_off."""
    rng = np.random.RandomState(seed)
    gt, det, goff, doff = [], [], [0], [0]

    def box(x, y, w, h, jitter):
        q = np.array([x, y, x + w, y, x + w, y + h, x, y + h], dtype=np.int64)
        return np.maximum(q + rng.randint(-jitter, jitter + 1, size=8), 0)
    for _ in range(frames):
        for _ in range(rng.randint(1, 7)):
            x, y, w, h = rng.randint(10, 600), rng.randint(10, 400), rng.randint(8, 81), rng.randint(8, 81)
            g = box(x, y, w, h, 6)
            gt.append(g)
            if rng.rand() < 0.85:
                det.append(np.maximum(g + rng.randint(-9, 10, size=8), 0))
        for _ in range(rng.randint(0, 3)):
            det.append(box(rng.randint(10, 600), rng.randint(10, 400), rng.randint(8, 81), rng.randint(8, 81), 6))
        goff.append(len(gt))
        doff.append(len(det))
    return {"gt_quads": np.asarray(gt, dtype=np.int32).reshape(-1, 8), "det_quads": np.asarray(det, dtype=np.int32).reshape(-1, 8),
            "gt_off": np.asarray(goff, dtype=np.int32), "det_off": np.asarray(doff, dtype=np.int32)}


# ------------------------------------------------------------------------------------------ 2. files of a small method
def _gt_xml(frames):
    """frames: [(frame id, [(object id, transcription, quad)])] -> the ground-truth XML text."""
    lines = ['<?xml version="1.0" encoding="utf-8"?>', "<Frames>"]
    for fid, objs in frames:
        lines.append('  <frame ID="%d">' % fid)
        for oid, text, q in objs:
            lines.append('    <object ID="%d" Transcription="%s" Language="English" Quality="HIGH">' % (oid, text))
            for i in range(4):
                lines.append('      <Point x="%d" y="%d"/>' % (q[2 * i], q[2 * i + 1]))
            lines.append("    </object>")
        lines.append("  </frame>")
    lines.append("</Frames>")
    return "\n".join(lines) + "\n"


def method_tree():
    """Two small videos, by hand.  -> {video: (gt frames, gt text {id: text}, result annotation {frame: rows})} where rows are
    `results.frame_lines` rows ([x1..y4, track id, text]).

    Video_1_1_1, 4 frames.  Object 1 "Hello!" (a 40 x 20 box moving right), object 2 "##" (don't care), object 3 "AB-c".
      track 10 follows object 1 exactly in frames 1-2, track 11 takes it over in frames 3-4 (one switch);
      track 12 sits inside the don't-care region in every frame (dropped);
      track 13 follows object 3 shifted by 5 px in frames 1-3 and is absent in frame 4 (one miss);
      track 14 is a stray in frame 2 (one false positive).  Frame 4 of the ground truth also has object 4 "zz", never detected.
    Video_2_1_1, 2 frames, one object, no result file."""
    def rect(x, y, w, h):
        return [x, y, x + w, y, x + w, y + h, x, y + h]
    gt1, ann1 = [], {}
    for k in range(4):
        fid = k + 1
        objs = [(1, "Hello!", rect(10 + 5 * k, 10, 40, 20)), (2, "##", rect(200, 100, 60, 40)), (3, "AB-c", rect(100, 200, 30, 30))]
        if fid == 4:
            objs.append((4, "zz", rect(300, 300, 20, 20)))
        gt1.append((fid, objs))
        rows = [rect(10 + 5 * k, 10, 40, 20) + [10 if fid <= 2 else 11, "hello"],
                rect(210, 110, 30, 20) + [12, "x"]]
        if fid <= 3:
            rows.append(rect(105, 200, 30, 30) + [13, "abc"])
        if fid == 2:
            rows.append(rect(400, 50, 25, 25) + [14, "stray"])
        ann1[str(fid)] = rows
    gt2 = [(1, [(7, "word", rect(5, 5, 50, 20))]), (2, [(7, "word", rect(6, 5, 50, 20))])]
    return {"Video_1_1_1": (gt1, {1: "Hello!", 3: "AB-c", 4: "zz"}, ann1), "Video_2_1_1": (gt2, {7: "word"}, None)}


# what the protocol gives for `method_tree`, worked out by hand (tracking: transcriptions are not compared).
# Video_1_1_1: objects 1 (4 frames), 3 (4 frames), 4 (1 frame) = 9 object appearances; track 12 is dropped everywhere.
#   frames 1-2: 1 <-> 10 (IoU 1, distance 0), 3 <-> 13 (30 x 30 boxes 5 px apart: IoU 750 / 1050 = 5/7, distance 2/7)
#   frame 2: track 14 is a false positive;  frame 3: 1 <-> 11 is a SWITCH, 3 <-> 13 a match
#   frame 4: 1 <-> 11 a match, 3 and 4 missed.
#   matches 6, switches 1, misses 2, false positives 1, detections 7, objects 9, predictions 8
#   MOTA = 1 - 4/9;  motp = (3 * 2/7) / 7 = 6/49, MOTP = 43/49;  MOTAN = 0.5 * (1 + 1) / 8 + 0.5 * 2 / 9
#   track ratios: object 1: 4/4, object 3: 3/4 (partially), object 4: 0 -> MT 1, PT 1, ML 1
#   ID measures: best one-to-one mapping 1 -> 10 or 11 (2 frames each), 3 -> 13 (3): IDTP 5, IDF1 = 2 * 5 / (9 + 8) = 10/17
# Video_2_1_1: no detections -> every figure 0.
TRACKING_EXPECTED = {
    "1_1_1": {"MA": 6, "SW": 1, "MS": 2, "FP": 1, "DE": 7, "OB": 9, "PR": 8, "UO": 3, "MT": 1, "PT": 1, "ML": 1,
              "MOTA": 1 - 4 / 9, "MOTP": 43 / 49, "MOTAN": 0.5 * 2 / 8 + 0.5 * 2 / 9, "IDF1": 10 / 17, "num_frames": 4},
    "2_1_1": {"MOTA": 0, "MOTP": 0, "MOTAN": 0, "IDF1": 0, "MT": 0, "PT": 0, "ML": 0, "DE": 0},
}
# End to end: ground-truth texts normalise to HELLO, ABC, ZZ; detections "hello" -> HELLO, "abc" -> ABC: the same pairs as in
# tracking are eligible, so the figures are the same -- except that `results.write_track_transcriptions` gives every track
# one text, and nothing here changes that.  A second result set with track 13 reading "abd" loses object 3's matches:
#   matches 3 (object 1), switches 1, misses 2 + 3 = 5, false positives 1 + 3 = 4, detections 4, objects 9, predictions 8
#   MOTA = 1 - 10/9;  motp = 0, MOTP = 1;  MOTAN = 0.5 * 5 / 8 + 0.5 * 5 / 9;  MT 1, PT 0, ML 2
#   IDTP = 2 (object 1 with track 10 or 11), IDF1 = 4 / 17
E2E_WRONG_TEXT_EXPECTED = {"MA": 3, "SW": 1, "MS": 5, "FP": 4, "DE": 4, "OB": 9, "PR": 8, "MT": 1, "PT": 0, "ML": 2,
                           "MOTA": 1 - 10 / 9, "MOTP": 1.0, "MOTAN": 0.5 * 5 / 8 + 0.5 * 5 / 9, "IDF1": 4 / 17}


def write_tree(root, wrong_text=False, zipped=False):
    """Write `method_tree` under `root`: gt/ (XML + GT.txt) and res/preds/ (through `results.write_video_results` and
    `write_track_transcriptions`).  -> (gt path, results path); with zipped=True both are .zip files of those directories."""
    import zipfile
    from gomatching_amd import results
    gt_dir, res_dir = os.path.join(root, "gt"), os.path.join(root, "res", "preds")
    os.makedirs(gt_dir)
    os.makedirs(res_dir)
    os.makedirs(os.path.join(root, "res", "jsons"))
    for name, (gt, text, ann) in method_tree().items():
        with open(os.path.join(gt_dir, name + "_GT.xml"), "w") as f:
            f.write(_gt_xml(gt))
        with open(os.path.join(gt_dir, name + "_GT.txt"), "w") as f:
            f.writelines('"%d","%s"\n' % kv for kv in sorted(text.items()))
        if ann is not None:
            if wrong_text:
                ann = {k: [r[:9] + ["abd" if r[8] == 13 else r[9]] for r in rows] for k, rows in ann.items()}
            results.write_video_results(ann, os.path.join(root, "res", "jsons", name + ".json"),
                                        os.path.join(res_dir, "res_%s.xml" % name))
    results.write_track_transcriptions(res_dir)
    if not zipped:
        return gt_dir, res_dir
    out = []
    for d, z in ((gt_dir, os.path.join(root, "gt.zip")), (res_dir, os.path.join(root, "res.zip"))):
        with zipfile.ZipFile(z, "w") as zf:
            for n in sorted(os.listdir(d)):
                zf.write(os.path.join(d, n), n)
        out.append(z)
    return tuple(out)
