"""A plain statement of the detection protocol's rule (shared by test_score_det_cpu.py, test_score_det_gpu.py and
tools/gen_golden_score_det.py; no test in here, nothing shared with the product code).

Per frame, pair by pair, in Python float64 on top of score_statement.py's geometry (`pair_value`: hull, clip, shoelace):
  det_care[d] = 0 iff some don't-care g has over(g, d) > area_thr (strict);
  for g ascending over the care objects: match[g] = the smallest d with det_care[d] == 1, not taken by an earlier g and
  iou(g, d) > iou_thr (strict), else -1; don't-care g get -1;
  stats = (matched, care objects, care detections).
Written as `script.py:evaluate_method` of the reference's detection protocol walks it: the full double loop with the two
"already matched" flags, not a first-hit search."""
import numpy as np

import score_statement as S


def frame_statement(gt_quads, gt_care, det_quads, iou_thr=0.5, area_thr=0.5):
    """One frame -> (det_care list, match list, (matched, care objects, care detections), closest): `closest` is the smallest
    |value - threshold| over every pair the rule looks at, for the tests' margin condition."""
    G, D = len(gt_quads), len(det_quads)
    closest = 1.0
    det_care = [1] * D
    for d in range(D):
        for g in range(G):
            if gt_care[g]:
                continue
            v = S.pair_value(gt_quads[g], det_quads[d], 1)
            closest = min(closest, abs(v - area_thr))
            if v > area_thr:
                det_care[d] = 0
                break
    iou = [[S.pair_value(gt_quads[g], det_quads[d], 0) for d in range(D)] for g in range(G)]
    for row in iou:
        for v in row:
            closest = min(closest, abs(v - iou_thr))
    match = [-1] * G
    g_done, d_done = [0] * G, [0] * D
    for g in range(G):
        for d in range(D):
            if g_done[g] == 0 and d_done[d] == 0 and gt_care[g] and det_care[d]:
                if iou[g][d] > iou_thr:
                    g_done[g] = d_done[d] = 1
                    match[g] = d
    stats = (sum(1 for m in match if m >= 0), sum(1 for c in gt_care if c), sum(det_care))
    return det_care, match, stats, closest


def video_statement(gt_quads, det_quads, gt_off, det_off, gt_care, iou_thr=0.5, area_thr=0.5):
    """CSR arrays of a video -> (det_care [D], match [G], frame_stats [F,3], closest)."""
    det_care, match, stats, closest = [], [], [], 1.0
    for f in range(len(gt_off) - 1):
        g0, g1, d0, d1 = int(gt_off[f]), int(gt_off[f + 1]), int(det_off[f]), int(det_off[f + 1])
        dc, m, st, c = frame_statement(gt_quads[g0:g1], [int(x) for x in gt_care[g0:g1]], det_quads[d0:d1], iou_thr, area_thr)
        det_care += dc
        match += m
        stats.append(st)
        closest = min(closest, c)
    return (np.asarray(det_care, dtype=np.int32), np.asarray(match, dtype=np.int32),
            np.asarray(stats, dtype=np.int32).reshape(-1, 3), closest)


# ------------------------------------------------------------------------------------------ seeded random frames
def rotated_rect(cx, cy, w, h, deg):
    """Corners of a rotated rectangle, rounded to integers (any point order is fine for the hull)."""
    a = np.deg2rad(deg)
    c, s = np.cos(a), np.sin(a)
    out = []
    for dx, dy in ((-w / 2, -h / 2), (w / 2, -h / 2), (w / 2, h / 2), (-w / 2, h / 2)):
        out += [int(round(cx + c * dx - s * dy)), int(round(cy + s * dx + c * dy))]
    return out


def random_video(seed, frames, max_gt=7):
    """Frames of rotated rectangles with about a fifth of the ground truth "don't care"; detections are near-duplicates of the
    ground truth (jittered, sometimes twice, so that several pass the same object and objects compete), small boxes inside
    don't-care regions, and strays.  Coordinates stay non-negative.  -> dict of int32 arrays."""
    rng = np.random.RandomState(seed)
    gt, det, care, goff, doff = [], [], [], [0], [0]
    for _ in range(frames):
        frame_gt = []
        for _ in range(rng.randint(0, max_gt + 1)):
            cx, cy = rng.randint(80, 560), rng.randint(80, 400)
            w, h = rng.randint(12, 90), rng.randint(10, 50)
            deg = float(rng.choice([0, 0, 15, 30, 45, 90, -20]))
            if frame_gt and rng.rand() < 0.25:                    # a near-duplicate object: they compete for detections
                q = [v + int(rng.randint(-2, 3)) for v in frame_gt[-1]]
            else:
                q = rotated_rect(cx, cy, w, h, deg)
            frame_gt.append(q)
            dont = rng.rand() < 0.2
            care.append(0 if dont else 1)
            for _ in range(int(rng.choice([0, 1, 1, 1, 2]))):
                det.append([v + int(rng.randint(-3, 4)) for v in q])
            if dont and rng.rand() < 0.7:                         # a detection inside the don't-care region
                det.append(rotated_rect(cx, cy, max(4, w // 2), max(4, h // 2), deg))
        for _ in range(rng.randint(0, 3)):
            det.append(rotated_rect(rng.randint(80, 560), rng.randint(80, 400), rng.randint(10, 60), rng.randint(10, 40),
                                    float(rng.randint(0, 180))))
        gt += frame_gt
        n_new = len(det) - doff[-1]
        order = rng.permutation(n_new)                            # detections in no particular order
        det[doff[-1]:] = [det[doff[-1] + int(k)] for k in order]
        goff.append(len(gt))
        doff.append(len(det))
    i32 = lambda a, shape: np.asarray(a, dtype=np.int32).reshape(shape)
    return {"gt_quads": i32(gt, (-1, 8)), "det_quads": i32(det, (-1, 8)), "gt_off": i32(goff, (-1,)), "det_off": i32(doff, (-1,)),
            "gt_care": i32(care, (-1,))}


# ------------------------------------------------------------------------------------------ the GPU tests' edge video
def rect(x, y, w, h):
    return [x, y, x + w, y, x + w, y + h, x, y + h]


def edge_video():
    """70 frames built from the smallest shapes at which the matching kernel can go wrong (named in `notes`: frame index ->
    what it holds).  -> (dict of int32 arrays, notes)."""
    rng = np.random.RandomState(5)
    gt, det, care, goff, doff, notes = [], [], [], [0], [0], {}

    def close(note=None):
        if note:
            notes[len(goff) - 1] = note
        goff.append(len(gt))
        doff.append(len(det))

    def far(k):                                                  # a small detection far from everything else
        return rect(3000 + 30 * (k % 40), 2000 + 30 * (k // 40), 10, 10)
    # 0: no ground truth, no detections
    close("G = 0 and D = 0")
    # 1: no ground truth
    det += [rect(10, 10, 30, 20), rect(100, 10, 30, 20)]
    close("G = 0")
    # 2: no detections
    gt += [rect(10, 10, 30, 20), rect(100, 10, 30, 20)]
    care += [1, 0]
    close("D = 0")
    # 3: 1 x 1
    gt.append(rect(10, 10, 30, 30))
    care.append(1)
    det.append(rect(12, 11, 30, 30))
    close("1 x 1")
    # 4: D = 65, the only passing detection of the object is index 64
    gt.append(rect(100, 100, 60, 40))
    care.append(1)
    det += [far(k) for k in range(64)] + [rect(101, 101, 60, 40)]
    close("D = 65, only index 64 passes")
    # 5: index 64 wins only because an earlier object took the passing detection at index 3
    gt += [rect(100, 100, 60, 40), rect(101, 100, 60, 40)]
    care += [1, 1]
    d5 = [far(k) for k in range(64)] + [rect(101, 101, 60, 40)]
    d5[3] = rect(100, 101, 60, 40)
    det += d5
    close("index 64 after index 3 was taken")
    # 6: G = 130 objects in a grid, a detection for every second one, in reverse order, plus near-duplicates
    boxes = [rect(20 + 50 * (k % 13), 20 + 30 * (k // 13), 40, 20) for k in range(130)]
    gt += boxes
    care += [0 if k % 11 == 5 else 1 for k in range(130)]
    d6 = [[v + int(rng.randint(-2, 3)) for v in boxes[k]] for k in range(129, -1, -2)]
    d6 += [[v + int(rng.randint(-1, 2)) for v in boxes[k]] for k in (0, 2, 4, 7)]
    det += d6
    close("G = 130")
    # 7: the first candidate of the object is a don't-care detection
    gt += [rect(200, 200, 80, 40), rect(190, 190, 100, 35)]       # the don't-care region covers the object's upper part
    care += [1, 0]
    det += [rect(200, 200, 80, 30), rect(200, 200, 80, 31)]       # IoU 0.75 / 0.775, but 25/30 and 25/31 of them are covered
    det += [rect(200, 212, 80, 28)]                               # IoU 0.7, 13/28 covered: stays, and is the match
    close("first candidates are don't-care detections")
    # 8: exactly 0.5: IoU 0.5 does not match, overlap 0.5 does not drop; beside them IoU just above (matches)
    gt += [rect(0, 0, 20, 10), rect(100, 0, 30, 10), rect(0, 100, 20, 10)]
    care += [1, 0, 1]
    det += [rect(0, 0, 10, 10),                                   # IoU with object 0: 100 / 200 = 0.5 exactly
            rect(120, 0, 20, 10),                                 # overlap with the don't-care object: 100 / 200 = 0.5 exactly
            rect(0, 100, 20, 9)]                                  # IoU 0.9
    close("IoU exactly 0.5 and overlap exactly 0.5")
    # 9: zero-area quads on both sides
    gt += [[0, 0, 10, 10, 20, 20, 30, 30], rect(40, 40, 20, 20), [5, 5, 5, 5, 5, 5, 5, 5], rect(0, 0, 40, 40)]
    care += [1, 1, 0, 0]
    det += [rect(0, 0, 30, 30), [45, 45, 45, 45, 45, 45, 45, 45], [40, 40, 60, 60, 60, 40, 40, 60], [10, 10, 20, 20, 30, 30, 15, 15]]
    close("zero-area quads on both sides")
    # 10..69: seeded random frames, so that F = 70 is more frames than waves in a workgroup
    r = random_video(77, 60)
    base_g, base_d = len(gt), len(det)
    gt += r["gt_quads"].tolist()
    det += r["det_quads"].tolist()
    care += r["gt_care"].tolist()
    goff += [base_g + int(v) for v in r["gt_off"][1:]]
    doff += [base_d + int(v) for v in r["det_off"][1:]]
    i32 = lambda a, shape: np.asarray([list(map(int, q)) for q in a] if shape[-1] == 8 else a, dtype=np.int32).reshape(shape)
    v = {"gt_quads": i32(gt, (-1, 8)), "det_quads": i32(det, (-1, 8)), "gt_off": i32(goff, (-1,)), "det_off": i32(doff, (-1,)),
         "gt_care": i32(care, (-1,))}
    assert len(v["gt_off"]) == 71
    return v, notes
