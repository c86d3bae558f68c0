"""Hand-made BOVText and ArTVideo videos for the json protocols of scoring, with the figures that follow from the protocols'
rules (not collected: shared by tests/test_score_json_cpu.py and tests/test_mask_pairs_gpu.py).

Every box is an axis-aligned rectangle, so that each IoU is a ratio of small integers:
  A            the counted object 1 ("Hel-lo": the regular expression and lower() make it "hello")
  B, C         ignored objects ("###"; in ArTVideo also `Straight`, for --curve)
  D            the counted object 4 ("world")
  frame 1      hypothesis 10 covers exactly half of A (IoU 0.5: kept at the threshold), 11 covers 16/30 of B (IoU above 0.5:
               swallowed), 12 exactly half of C (IoU 0.5: not swallowed, a false positive)
  frame 2      hypothesis 10 = A with the text "hellp" (edit distance 1: similarity 0.95, accepted), 13 = D with "wxyzd"
               (similarity 0.4: rejected with --e2e)
  frame 3      is missing from the result
and a second video has no result file at all.
"""
import json
import os

import numpy as np

import mask_statement as ms

A, B, C, D = (0, 0, 30, 10), (40, 0, 70, 10), (0, 20, 30, 30), (0, 30, 30, 40)      # x0, y0, x1, y1


def _quad(r):
    x0, y0, x1, y1 = r
    return [x0, y0, x1, y0, x1, y1, x0, y1]


def write_bovtext(root):
    """-> (GT directory, RES directory)."""
    gt_dir, res_dir = os.path.join(root, "gt"), os.path.join(root, "jsons")

    def obj(r, oid, text):
        return {"points": [float(v) + 0.75 * (v > 0) for v in _quad(r)], "ID": oid, "transcription": text, "ID_transcription": text}
    half = lambda r: (r[0], r[1], r[0] + 15, r[3])
    gt1 = {"1": [obj(A, 1, "Hel-lo"), obj(B, 2, "###"), obj(C, 3, "#1")],
           "2": [obj(A, 1, "Hel-lo"), obj(D, 4, "world")],
           "3": [obj(A, 1, "Hel-lo"), obj(D, 4, "world")]}
    res1 = {"1": [{"points": _quad(half(A)), "ID": 10, "transcription": "hello"},
                  {"points": _quad((B[0], B[1], B[0] + 16, B[3])), "ID": 11, "transcription": "x"},
                  {"points": _quad(half(C)), "ID": 12, "transcription": "y"}],
            "2": [{"points": _quad(A), "ID": 10, "transcription": "hellp"},
                  {"points": _quad(D), "ID": 13, "transcription": "wxyzd"}],
            "9": [{"points": _quad(A), "ID": 99, "transcription": "beyond the ground truth: never read"}]}
    gt2 = {"1": [obj(A, 7, "abc")], "2": [obj(A, 7, "abc")]}
    files = {os.path.join(gt_dir, "Cls2_Cartoon", "Cls2_Cartoon_video1.json"): gt1,
             os.path.join(gt_dir, "Cls3_Sports", "Cls3_Sports_video2.json"): gt2,
             os.path.join(gt_dir, "Cls1_Livestreaming", "Cls1_Livestreaming_video40.json"): {"1": "left out by name"},
             os.path.join(gt_dir, ".ipynb_checkpoints", "x.json"): {"1": "left out"},
             os.path.join(res_dir, "Cls2_Cartoon_video1.json"): res1}
    for path, doc in files.items():
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, "w") as f:
            json.dump(doc, f)
    return gt_dir, res_dir


H, W = 40, 80


def _pixels(r):
    """The pixel rectangle x0 .. x1-1, y0 .. y1-1 as an image."""
    img = np.zeros((H, W), dtype=bool)
    img[r[1]:r[3], r[0]:r[2]] = True
    return img


def _rle(r, as_string):
    counts = ms.rle_encode(_pixels(r))
    return {"size": [H, W], "counts": ms.rle_to_string(counts) if as_string else counts}


def _poly(r):
    """The polygon whose rasterisation is the pixel rectangle: vertices on the outermost pixels."""
    x0, y0, x1, y1 = r[0], r[1], r[2] - 1, r[3] - 1
    return [[x0, y0], [x1, y0], [x1, y1], [x0, y1]]


def write_artvideo(root):
    gt_dir, res_dir = os.path.join(root, "gt"), os.path.join(root, "jsons")

    def ann(frame, r, oid, text, kind, as_string):
        return {"frame_id": frame, "point": [v for p in _poly(r) for v in p], "obj_id": oid, "segmentation": _rle(r, as_string),
                "text_type": kind, "Transcription": text}
    frames = [{"height": H, "width": W, "id": k} for k in (1, 2, 3)]
    gt1 = {"frame": frames, "annotations": [
        ann(1, A, 1, "Hel-lo", "Curve", True), ann(1, B, 2, "###", "Straight", False), ann(1, C, 3, "#1", "Straight", True),
        ann(2, A, 1, "Hel-lo", "Curve", False), ann(2, D, 4, "world", "Curve", True),
        ann(3, A, 1, "Hel-lo", "Curve", True), ann(3, D, 4, "world", "Curve", True)]}
    half = lambda r: (r[0], r[1], r[0] + 15, r[3])
    flat = lambda r: [float(v) for p in _poly(r) for v in p]
    res1 = {"1": [{"points": flat(half(A)), "ID": 10, "transcription": "hello"},
                  {"points": flat(A), "ID": 11, "transcription": "x", "segmentation": [_poly((B[0], B[1], B[0] + 16, B[3]))]},
                  {"points": flat(A), "ID": 12, "transcription": "y", "segmentation": [_poly(half(C))]}],
            "2": [{"points": flat(D), "ID": 10, "transcription": "hellp", "segmentation": [_poly(A)]},
                  {"points": flat(A), "ID": 13, "transcription": "wxyzd", "segmentation": _rle(D, True)}]}
    gt2 = {"frame": frames[:2], "annotations": [ann(1, A, 7, "abc", "Curve", True), ann(2, A, 7, "abc", "Curve", True)]}
    files = {os.path.join(gt_dir, "video_1.json"): gt1, os.path.join(gt_dir, "video_2.json"): gt2,
             os.path.join(res_dir, "video_1.json"): res1}
    for path, doc in files.items():
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, "w") as f:
            json.dump(doc, f)
    return gt_dir, res_dir


def _m(frames, matches, fp, misses, objects, ious):
    return {"num_frames": frames, "num_matches": matches, "num_switches": 0, "num_false_positives": fp, "num_misses": misses,
            "num_objects": objects, "num_detections": matches, "mota": 1 - (fp + misses) / objects,
            "motp": sum(ious) / matches if matches else 0.0}


NO_RESULT = _m(2, 0, 0, 2, 2, [])
# video 1 of both protocols; key: (e2e, curve)
TRACKING = _m(3, 3, 1, 2, 5, [0.5, 1.0, 1.0])                                       # B, C ignored: 11 swallowed, 12 a false positive
E2E = _m(3, 2, 2, 3, 5, [0.5, 1.0])                                                 # and 13 / object 4 no longer pair
ART_TRACKING_ALL = _m(3, 5, 0, 2, 7, [0.5, 160 / 300, 0.5, 1.0, 1.0])               # eval_trk ignores nothing without --curve
EXPECTED = {
    ("bovtext", False, False): TRACKING, ("bovtext", True, False): E2E,
    ("artvideo", False, False): ART_TRACKING_ALL, ("artvideo", False, True): TRACKING,
    ("artvideo", True, False): E2E, ("artvideo", True, True): E2E,
}
