"""Write tests/golden/score_det.json: what the reference's own detection protocol gives for the hand-written XML under
tests/golden/score_det_raw/ (two small videos; tests/golden/score_det_raw holds gt/Video_*_GT.xml and res/res_Video_*.xml).

    python tools/gen_golden_score_det.py --reference <reference checkout>

CPU only.  Imported UNMODIFIED from tools/Evaluation_Protocol_DSText/Evaluation_DSText_Det of the reference: `script.py` and
`rrc_evaluation_funcs.py` whole, and from `toicdar15gt.py` the functions `order_points`, `validate_clockwise_points`,
`parse_xml` and `getBboxesAndLabels_icd13` (the converter's `__main__` block stops on an undefined name and keeps its
ground-truth half commented out; the loop below is this generator's restatement of it, for results and ground truth alike,
through those four functions).  `cv2`, `tqdm` and `shapely.geometry` are not installed: stand-ins go into sys.modules first.
The first two are never called.  The `Polygon` stand-in (`area`, `intersects`, `&`) is this generator's own code over
tests/det_statement.py's geometry, so the GEOMETRY IS UNPINNED; every fixture quad that survives the validity test is
convex, so the hull / polygon difference cannot enter.  PINNED by the written file: the reading, the point ordering, the
validity drop, the don't-care marking, the greedy matching and every figure.
Only data is written: names, indices and figures.  gomatching_amd/score_det.py is held to it by tests/test_score_det_cpu.py.
"""
import argparse
import json
import os
import re
import sys
import tempfile
import types
import zipfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RAW = os.path.join(ROOT, "tests", "golden", "score_det_raw")
sys.path.insert(0, os.path.join(ROOT, "tests"))
import score_statement as S                                          # noqa: E402


class Polygon:
    """The three things `evaluate_method` asks of shapely's Polygon, over the statement's hull geometry."""

    def __init__(self, points=None, hull=None):
        self.hull = hull if hull is not None else S.hull([int(v) for p in np.asarray(points).tolist() for v in p])

    @property
    def area(self):
        if len(self.hull) < 3:
            return 0.0
        s = 0.0
        for i in range(len(self.hull)):
            (px, py), (cx, cy) = self.hull[i - 1], self.hull[i]
            s += float(px) * float(cy) - float(cx) * float(py)
        return abs(s) * 0.5

    def __and__(self, other):
        if len(self.hull) < 3 or len(other.hull) < 3 or self.area == 0 or other.area == 0:
            return Polygon(hull=[])
        return Polygon(hull=S.clip(self.hull, other.hull))

    def intersects(self, other):
        return (self & other).area > 0


def stand_ins():
    cv2 = types.ModuleType("cv2")
    cv2.VideoWriter = cv2.VideoWriter_fourcc = None
    tqdm = types.ModuleType("tqdm")
    tqdm.tqdm = lambda x, *a, **k: x
    shapely = types.ModuleType("shapely")
    geometry = types.ModuleType("shapely.geometry")
    geometry.Polygon = Polygon
    geometry.MultiPoint = None
    shapely.geometry = geometry
    for name, mod in (("cv2", cv2), ("tqdm", tqdm), ("shapely", shapely), ("shapely.geometry", geometry)):
        sys.modules.setdefault(name, mod)


def convert(conv, xml_path, with_words):
    """The converter's loop for one XML -> (per frame the text of its icdar15 file, dropped [[frame position, object
    position]])."""
    bboxess, wordss = conv.parse_xml(xml_path)
    files, dropped = [], []
    for i in range(len(wordss)):
        lines = []
        for k, (bboxes, word) in enumerate(zip(bboxess[i], wordss[i])):
            points = np.array([int(float(c)) for c in bboxes])
            points = np.reshape(points, (4, 2))
            points = conv.order_points(points)
            points = np.reshape(points, -1)
            if not conv.validate_clockwise_points(points):
                dropped.append([i, k])
                continue
            lines.append(",".join(str(p) for p in points) + (("," + word) if with_words else "") + "\r\n")
        files.append("".join(lines))
    return files, dropped


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reference", required=True, help="checkout of the reference project")
    ap.add_argument("--output", default=os.path.join(ROOT, "tests", "golden", "score_det.json"))
    args = ap.parse_args()
    proto = os.path.join(args.reference, "tools", "Evaluation_Protocol_DSText", "Evaluation_DSText_Det")
    if not os.path.isfile(os.path.join(proto, "script.py")):
        sys.exit("error: no detection protocol under %s" % proto)
    stand_ins()
    sys.path.insert(0, proto)
    import script
    import toicdar15gt as conv
    videos = sorted(re.fullmatch(r"(Video_[0-9_]+)_GT\.xml", n).group(1) for n in os.listdir(os.path.join(RAW, "gt")))
    dropped = {"gt": {}, "det": {}}
    frames = {}
    with tempfile.TemporaryDirectory() as tmp:
        gt_zip, res_zip = os.path.join(tmp, "gt.zip"), os.path.join(tmp, "res.zip")
        with zipfile.ZipFile(gt_zip, "w") as gz, zipfile.ZipFile(res_zip, "w") as rz:
            for v in videos:
                files, dropped["gt"][v] = convert(conv, os.path.join(RAW, "gt", v + "_GT.xml"), True)
                frames[v] = len(files)
                for i, text in enumerate(files):                  # (the protocol names the ground truth after the results)
                    gz.writestr("res_%s_%d.txt" % (v, i + 1), text)
                res = os.path.join(RAW, "res", "res_%s.xml" % v)
                if os.path.exists(res):
                    files, dropped["det"][v] = convert(conv, res, False)
                    for i, text in enumerate(files):
                        rz.writestr("res_%s_%d.txt" % (v, i + 1), text)
        params = script.default_evaluation_params()
        script.validate_data(gt_zip, res_zip, params)
        res, hmean = script.evaluate_method(gt_zip, res_zip, params)
    per_sample = {}
    for name, s in res["per_sample"].items():
        per_sample[name] = {"precision": float(s["precision"]), "recall": float(s["recall"]), "hmean": float(s["hmean"]),
                            "AP": float(s["AP"]), "pairs": [{"gt": int(p["gt"]), "det": int(p["det"])} for p in s["pairs"]],
                            "gtDontCare": [int(x) for x in s["gtDontCare"]], "detDontCare": [int(x) for x in s["detDontCare"]]}
    doc = {"params": {"IOU_CONSTRAINT": params["IOU_CONSTRAINT"], "AREA_PRECISION_CONSTRAINT": params["AREA_PRECISION_CONSTRAINT"]},
           "videos": videos, "frames": frames, "dropped": dropped,
           "method": {k: float(v) for k, v in res["method"].items()}, "per_sample": per_sample}
    assert float(hmean) == doc["method"]["hmean"]
    with open(args.output, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(doc["method"]), len(per_sample), "frames", dropped)


if __name__ == "__main__":
    main()
