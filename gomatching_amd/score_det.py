"""Score result files by the DSText DETECTION protocol: ICDAR15-style precision / recall / hmean per frame.

    python -m gomatching_amd.score --det --gt GT --results RES [--host-iou] [--per-frame] [--output scores.json]

The figures are those of the reference's tools/Evaluation_Protocol_DSText/Evaluation_DSText_Det: `toicdar15gt.py` cuts each
XML into per-frame quadrilaterals, `script.py:evaluate_method` marks the detections on "don't care" regions, matches ground
truth and detections one-to-one greedily at IoU > 0.5 and counts.  GT and RES are what the tracking protocol reads
(`Video_<a>_<b>_<c>_GT.xml`, `res_Video_<a>_<b>_<c>.xml`, directories or .zip).

Reading, as the converter does it: frames are taken BY POSITION (the i-th frame element is frame i + 1, whatever its ID says);
per object integer `x` / `y` attributes, NOT clamped at 0 (the tracking reader clamps), exactly four points; `order_points`
(the two leftmost points lower one first, then the two rightmost upper one first); an object whose ordered points fail
`validate_clockwise_points` is dropped and counted (`invalid_gt` / `invalid_det`); a ground-truth Transcription of
"##DONT#CARE##" or "###" means don't care.  The ground truth goes through the same steps (the block the converter keeps
commented out).

The rule per frame (stated once in include/gomatching_hip.h): a detection leaves when a don't-care object covers more than
half of its area; care objects in file order each take the first remaining, not yet taken detection with IoU > threshold.
On the device this is one launch of `ops.quad_det_match` per video (csrc/score_det.hip); `--host-iou` runs the same rule in
numpy float64 (`host_quad_det_match`) and writes the same bytes.  All quads of a video are shifted by one common integer
offset so that no coordinate is negative (the hull's sort key wants that; IoU does not change); a coordinate of 2^24 or more
after the shift is an error, and so is, on the device path, a frame with more than 4096 detections.

Figures: per frame `script.py`'s expressions (recall 1 without care objects, precision 0 if care detections remain there, else
1); the method's precision / recall / hmean from the global sums; AP = 0 (results carry no confidences).  `per_video` holds
the same aggregate over one video's sums: that one is ours, not the script's.

PINNED by tests/golden/score_det.json, which the reference's own script and converter functions produced: the reading, the
ordering, the validity drop, the don't-care marking, the greedy matching and every figure.  UNPINNED: the geometry (shapely is
not available to the generator; it is held to tests/score_statement.py as in the other protocols).

Deliberate differences:
  * the geometry is the convex hull's, not shapely's polygon of the ordered points: identical for convex quads; ordered quads
    that are not convex are counted as `nonconvex_gt` / `nonconvex_det`.
  * a video or a frame without results counts as one without detections (`evaluate_method`'s behaviour; `eval_2015` builds its
    archives from the result files alone and silently drops such frames).
  * a result XML with more frames than its ground truth is an error (`validate_data`).
  * not written: `iouMat`, `evaluationLog`, `evaluationParams` and the point lists of `per_sample`.
"""
import xml.etree.ElementTree as ET

import numpy as np

from . import score
from .score import ScoreError

AREA_PRECISION_CONSTRAINT = 0.5
MAX_FRAME_DETECTIONS = 4096
_DONT_CARE = ("##DONT#CARE##", "###")


# ------------------------------------------------------------------------------------------ the converter's steps
def order_points(pts):
    """[(x, y)] * 4 -> the converter's order: stable sort by x; the left two by y descending, the right two by y ascending
    (ties keep the order of numpy's argsort on four elements, which is stable)."""
    by_x = sorted(pts, key=lambda p: p[0])
    left, right = by_x[:2], by_x[2:]
    left = sorted(left, key=lambda p: p[1])[::-1]
    right = sorted(right, key=lambda p: p[1])
    return left + right


def clockwise_valid(p):
    """`validate_clockwise_points` on four ordered points."""
    s = 0
    for i in range(4):
        a, b = p[i], p[(i + 1) & 3]
        s += (b[0] - a[0]) * (b[1] + a[1])
    return s <= 0


def read_quads(raw, what, ground_truth):
    """A protocol XML -> (frames, dropped): frames[i] = [(quad as 8 ints in the converter's order, don't care)] of the i-th
    frame element, dropped = [(frame position, object position)] of the objects that failed the clockwise test."""
    try:
        root = ET.fromstring(raw)
    except ET.ParseError as e:
        raise ScoreError("%s: not well-formed XML (%s)" % (what, e))
    frames, dropped = [], []
    for i, frame in enumerate(root):
        objs = []
        for k, obj in enumerate(frame):
            try:
                pts = [(int(pt.attrib["x"]), int(pt.attrib["y"])) for pt in obj]
            except (KeyError, ValueError) as e:
                raise ScoreError("%s: object %d of frame %d: missing or non-integer coordinate (%s)" % (what, k + 1, i + 1, e))
            if len(pts) != 4:
                raise ScoreError("%s: object %d of frame %d has %d points, not four" % (what, k + 1, i + 1, len(pts)))
            text = obj.attrib.get("Transcription")
            if ground_truth and text is None:
                raise ScoreError("%s: object %d of frame %d has no Transcription" % (what, k + 1, i + 1))
            pts = order_points(pts)
            if not clockwise_valid(pts):
                dropped.append((i, k))
                continue
            objs.append(([c for p in pts for c in p], ground_truth and text in _DONT_CARE))
        frames.append(objs)
    return frames, dropped


# ------------------------------------------------------------------------------------------ the rule on the host
def _sweep(gt_off, det_off, gt_care, det_care, counts, det):
    """The greedy matching over compacted pairs (`counts` kept detections per CARE object, `det` their indices within the
    frame, ascending): -> (match [G], frame_stats [F,3])."""
    G, F = len(gt_care), len(gt_off) - 1
    match = np.full(G, -1, dtype=np.int32)
    stats = np.zeros((F, 3), dtype=np.int32)
    care_idx = np.nonzero(gt_care != 0)[0]
    ends = np.cumsum(counts, dtype=np.int64)
    det = det.tolist()
    k = 0
    for f in range(F):
        g0, g1, d0, d1 = int(gt_off[f]), int(gt_off[f + 1]), int(det_off[f]), int(det_off[f + 1])
        free = det_care[d0:d1].astype(bool).tolist()
        matched = ncare = 0
        while k < len(care_idx) and care_idx[k] < g1:
            ncare += 1
            for d in det[int(ends[k] - counts[k]):int(ends[k])]:
                if free[d]:
                    free[d] = False
                    match[care_idx[k]] = d
                    matched += 1
                    break
            k += 1
        stats[f] = (matched, ncare, int(det_care[d0:d1].sum()))
    return match, stats


def _match_from_pairs(pairs_fn, gt_quads, det_quads, gt_off, det_off, gt_care, iou_thr, area_thr):
    """The rule composed from the pair compaction: `pairs_fn` (score.host_quad_pairs or score.device_quad_pairs) once for the
    don't-care objects (overlap), once for the care objects (IoU), then the sweep on the host."""
    gt_quads = np.asarray(gt_quads, dtype=np.int64).reshape(-1, 8)
    det_quads = np.asarray(det_quads, dtype=np.int64).reshape(-1, 8)
    gt_off, det_off = np.asarray(gt_off, dtype=np.int64), np.asarray(det_off, dtype=np.int64)
    gt_care = np.asarray(gt_care, dtype=np.int32)
    G, D, F = len(gt_quads), len(det_quads), len(gt_off) - 1
    frame = np.repeat(np.arange(F), gt_off[1:] - gt_off[:-1])

    def subset(mask):
        off = np.zeros(F + 1, dtype=np.int64)
        off[1:] = np.cumsum(np.bincount(frame[mask], minlength=F))
        return gt_quads[mask], off
    det_care = np.ones(D, dtype=np.int32)
    zeros = lambda n: np.zeros(n, dtype=np.int32)
    dc_quads, dc_off = subset(gt_care == 0)
    if len(dc_quads) and D:
        counts, di, _ = pairs_fn(dc_quads, det_quads, dc_off, det_off, zeros(len(dc_quads)), zeros(D), 1, area_thr)
        f_of = np.repeat(np.repeat(np.arange(F), dc_off[1:] - dc_off[:-1]), counts)
        det_care[det_off[f_of] + di] = 0
    care_quads, care_off = subset(gt_care != 0)
    if len(care_quads) and D:
        counts, di, _ = pairs_fn(care_quads, det_quads, care_off, det_off, zeros(len(care_quads)), zeros(D), 0, iou_thr)
    else:
        counts, di = zeros(len(care_quads)), zeros(0)
    match, stats = _sweep(gt_off, det_off, gt_care, det_care, counts, di)
    return det_care, match, stats


def host_quad_det_match(gt_quads, det_quads, gt_off, det_off, gt_care, iou_thr=0.5, area_thr=AREA_PRECISION_CONSTRAINT):
    """`ops.quad_det_match` on the host, numpy float64: -> (det_care int32 [D], match int32 [G], frame_stats int32 [F,3])."""
    return _match_from_pairs(score.host_quad_pairs, gt_quads, det_quads, gt_off, det_off, gt_care, iou_thr, area_thr)


def composed_quad_det_match(gt_quads, det_quads, gt_off, det_off, gt_care, iou_thr=0.5, area_thr=AREA_PRECISION_CONSTRAINT):
    """The same through `ops.quad_pairs` twice and the host sweep (what the fused launch replaces; tools/score_det_bench.py)."""
    return _match_from_pairs(score.device_quad_pairs, gt_quads, det_quads, gt_off, det_off, gt_care, iou_thr, area_thr)


def device_quad_det_match(gt_quads, det_quads, gt_off, det_off, gt_care, iou_thr=0.5, area_thr=AREA_PRECISION_CONSTRAINT):
    """`host_quad_det_match` through the kernel: one upload, one launch, one copy back."""
    import torch
    from . import ops
    if not torch.cuda.is_available():
        raise ScoreError("no GPU: the matching runs in csrc/score_det.hip (use --host-iou for the numpy path)")
    dev = torch.device("cuda", torch.cuda.current_device())

    def up(a, shape):
        return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32).reshape(shape)).to(dev)
    det_off = np.asarray(det_off, dtype=np.int64)
    most = int((det_off[1:] - det_off[:-1]).max()) if len(det_off) > 1 else 0
    out = ops.quad_det_match(up(gt_quads, (-1, 8)), up(det_quads, (-1, 8)), up(gt_off, (-1,)), up(det_off, (-1,)),
                             up(gt_care, (-1,)), iou_thr, area_thr, max_det=most)
    return tuple(t.cpu().numpy() for t in out)


# ------------------------------------------------------------------------------------------ figures
def frame_figures(matched, gt_care, det_care):
    """`script.py:269-281` -> (precision, recall, hmean) of one frame."""
    if gt_care == 0:
        recall = float(1)
        precision = float(0) if det_care > 0 else float(1)
    else:
        recall = float(matched) / gt_care
        precision = float(0) if det_care == 0 else float(matched) / det_care
    hmean = float(0) if (precision + recall) == 0 else 2.0 * precision * recall / (precision + recall)
    return precision, recall, hmean


def sum_figures(matched, gt_care, det_care):
    """`script.py:306-308` -> (precision, recall, hmean) from sums."""
    recall = float(0) if gt_care == 0 else float(matched) / gt_care
    precision = float(0) if det_care == 0 else float(matched) / det_care
    hmean = float(0) if recall + precision == 0 else 2 * recall * precision / (recall + precision)
    return precision, recall, hmean


def _nonconvex(quads):
    """How many ordered quads differ from their hull (twice the polygon's area against twice the hull's)."""
    if len(quads) == 0:
        return 0
    q = np.asarray(quads, dtype=np.int64).reshape(-1, 8)
    x, y = q[:, 0::2], q[:, 1::2]
    poly2 = np.abs((x * np.roll(y, -1, 1) - np.roll(x, -1, 1) * y).sum(1))
    return int((score.quad_hulls(q)[2] != poly2).sum())


def score_video(gt_xml, det_xml, threshold=0.5, match_fn=host_quad_det_match, name="video", per_frame=False):
    """One video -> (its sums and counts, {frame number: per_sample entry} or None).  det_xml None: no result."""
    gt_frames, gt_dropped = read_quads(gt_xml, "ground truth of " + name, True)
    F = len(gt_frames)
    det_frames, det_dropped = ([], []) if det_xml is None else read_quads(det_xml, "res_" + name, False)
    if len(det_frames) > F:
        raise ScoreError("res_%s: %d frames, the ground truth has %d" % (name, len(det_frames), F))
    det_frames += [[] for _ in range(F - len(det_frames))]
    gt_off, gt_quads = score._csr([[q for q, _ in x] for x in gt_frames])
    det_off, det_quads = score._csr([[q for q, _ in x] for x in det_frames])
    gt_care = np.asarray([0 if dc else 1 for x in gt_frames for _, dc in x], dtype=np.int32)
    res = {"invalid_gt": len(gt_dropped), "invalid_det": len(det_dropped),
           "nonconvex_gt": _nonconvex(gt_quads), "nonconvex_det": _nonconvex(det_quads)}
    low = min([0] + [int(a.min()) for a in (gt_quads, det_quads) if a.size])
    gt_quads, det_quads = gt_quads - low, det_quads - low
    for a, off, what in ((gt_quads, gt_off, "ground truth of " + name), (det_quads, det_off, "res_" + name)):
        if a.size and int(a.max()) >= 2 ** 24:
            bad = int(np.searchsorted(off, int(np.argmax(a.max(1))), side="right"))
            raise ScoreError("%s: frame %d has a coordinate of 2^24 or more (after the shift by %d)" % (what, bad, -low))
    if match_fn is not host_quad_det_match and F:
        per = det_off[1:] - det_off[:-1]
        if int(per.max()) > MAX_FRAME_DETECTIONS:
            raise ScoreError("res_%s: frame %d has %d detections, the matching kernel takes at most %d per frame (use "
                             "--host-iou)" % (name, int(np.argmax(per)) + 1, int(per.max()), MAX_FRAME_DETECTIONS))
    if F:
        det_care, match, stats = match_fn(gt_quads, det_quads, gt_off, det_off, gt_care, threshold, AREA_PRECISION_CONSTRAINT)
    else:
        det_care, match, stats = np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros((0, 3), np.int32)
    sums = [int(v) for v in stats.sum(0)] if F else [0, 0, 0]
    res.update({"matched": sums[0], "gt_care": sums[1], "det_care": sums[2], "frames": F})
    res["precision"], res["recall"], res["hmean"] = sum_figures(*sums)
    samples = None
    if per_frame:
        samples = {}
        for f in range(F):
            g0, g1, d0, d1 = int(gt_off[f]), int(gt_off[f + 1]), int(det_off[f]), int(det_off[f + 1])
            p, r, h = frame_figures(*[int(v) for v in stats[f]])
            samples[f + 1] = {"precision": p, "recall": r, "hmean": h,
                              "pairs": [{"gt": g - g0, "det": int(match[g])} for g in range(g0, g1) if match[g] >= 0],
                              "gtDontCare": [g - g0 for g in range(g0, g1) if gt_care[g] == 0],
                              "detDontCare": [d - d0 for d in range(d0, d1) if det_care[d] == 0]}
    return res, samples


_SUMS = ("matched", "gt_care", "det_care", "invalid_gt", "invalid_det", "nonconvex_gt", "nonconvex_det")


def score_method(gt_path, res_path, threshold=0.5, host_iou=False, per_frame=False):
    """`evaluate_method` over every frame of every video: -> {"method", "per_video"[, "per_sample"]}."""
    gt = score.load_source(gt_path, score.GT_XML)
    subm = score.load_source(res_path, score.DET_XML)
    if not gt:
        raise ScoreError("no Video_<a>_<b>_<c>_GT.xml in %r" % gt_path)
    for k in subm:
        if k not in gt:
            raise ScoreError("the video ID %s is not present in GT" % k)
    match_fn = host_quad_det_match if host_iou else device_quad_det_match
    per_video, per_sample = {}, {}
    for k in gt:
        per_video[k], samples = score_video(gt[k], subm.get(k), threshold, match_fn, "Video_" + k, per_frame)
        for n, s in (samples or {}).items():
            per_sample["res_Video_%s_%d.txt" % (k, n)] = s
    method = {key: sum(v[key] for v in per_video.values()) for key in _SUMS}
    method["precision"], method["recall"], method["hmean"] = sum_figures(method["matched"], method["gt_care"], method["det_care"])
    method["AP"] = 0
    out = {"method": method, "per_video": per_video}
    if per_frame:
        out["per_sample"] = per_sample
    return out


def print_scores(res):
    line = "precision %.4f  recall %.4f  hmean %.4f  matched %d  care GT %d  care detections %d"
    keys = ("precision", "recall", "hmean", "matched", "gt_care", "det_care")
    print("method: " + line % tuple(res["method"][k] for k in keys))
    for k, v in res["per_video"].items():
        print(("Video_%s: " % k) + line % tuple(v[k2] for k2 in keys))
