"""Writes the fixtures of the prepare command under tests/golden/: what the REFERENCE's own programs compute.  CPU only;
needs the reference tree (oracle/ref_shim.py names its place).

(a) tests/golden/prepare_geometry.json.  The reference's gomatching/data/datasets/bezier_tools.py is imported unmodified with an
    EMPTY stand-in `cv2` module in `sys.modules` (the functions recorded here never call it; no arithmetic lives in the
    stand-in).  Recorded on seeded inputs: `get_tight_rect` on integer corner sets (with x-ties and y-ties, corners outside
    the image), `cpt_bezier_pts` on integer rectangles (with equal edges), `polygon_to_bezier_pts` on 14-gons with distinct
    points, and beside each 14-gon the 2-norm condition numbers of the two Bernstein matrices the reference handed to
    `numpy.linalg.pinv` (observed by wrapping that call for the duration; the matrix is the reference's, not rebuilt here).

(b) tests/golden/prepare_raw/.  A tiny raw tree of this project's own making -- two ICDAR15-style videos, two DSText videos in two
    class directories, two BOVText videos in two classes; a duplicate object id, `##DONT#CARE##` entries, every language
    branch, negative and out-of-image coordinates, the two Video_18_3_1 exclusions -- is built in a temporary `datasets/`
    with real .jpg frames, and the reference's tools/convert_gom_label/{icdar15,dstext,bovtext}.py are run UNMODIFIED from
    that directory with `runpy`.  `cv2.imread` is a Pillow stand-in, `tqdm.tqdm` an identity stand-in; every class directory
    BOVText's list names is present (empty) in the temporary tree.  Committed: the raw annotation files, the three resulting
    json files, the order in which the scripts took the videos (read off their output) and the frame count and size of every
    video (frames.json; the tests regenerate the frames from it).  All of it is data those programs read or wrote.

    python tools/gen_golden_prepare.py
"""
import contextlib
import importlib
import io
import json
import os
import runpy
import shutil
import sys
import tempfile
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import ref_shim  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
RAW = os.path.join(GOLDEN, "prepare_raw")


# ------------------------------------------------------------------------------------------------- (a) geometry helpers
def geometry():
    sys.modules["cv2"] = types.ModuleType("cv2")
    for name, path in (("gomatching", "gomatching"), ("gomatching.data", "gomatching/data"),
                       ("gomatching.data.datasets", "gomatching/data/datasets")):         # skip the reference's __init__ files
        m = types.ModuleType(name)
        m.__path__ = [os.path.join(ref_shim.REF_ROOT, path)]
        sys.modules[name] = m
    bt = importlib.import_module("gomatching.data.datasets.bezier_tools")
    rng = np.random.Generator(np.random.Philox(key=0xBE21))
    sizes = [(720, 1280), (97, 131), (361, 203), (1080, 1920)]

    tight = []
    for k in range(160):
        H, W = sizes[k % len(sizes)]
        c = np.stack([rng.integers(-40, W + 40, 4), rng.integers(-40, H + 40, 4)], 1)
        if k % 4 == 1:                                           # x-ties: the stable sort decides
            c[rng.integers(0, 4), 0] = c[rng.integers(0, 4), 0]
            c[1 + k % 3, 0] = c[0, 0]
        if k % 4 == 2:                                           # y-ties: `>` is false
            c[[0, 1], 1] = c[0, 1]
            c[[2, 3], 1] = c[3, 1]
        if k % 4 == 3:                                           # an axis-aligned rectangle in a random corner order
            x0, x1, y0, y1 = c[0, 0], c[1, 0], c[0, 1], c[1, 1]
            c = np.array([[x0, y0], [x1, y0], [x1, y1], [x0, y1]])[rng.permutation(4)]
        out = bt.get_tight_rect(np.array(c, dtype="int"), 0, 0, H, W, 1)
        tight.append({"corners": c.tolist(), "H": H, "W": W, "out": [int(v) for v in out]})

    cpt = []
    for k in range(120):
        r = rng.integers(1, 1300, (4, 2))
        if k % 3 == 1:                                           # a square: four equal edges, the first two win
            s = int(rng.integers(1, 200))
            x0, y0 = int(r[0, 0]), int(r[0, 1])
            r = np.array([[x0, y0], [x0 + s, y0], [x0 + s, y0 + s], [x0, y0 + s]])
        if k % 3 == 2:                                           # a rectangle: two pairs of equal edges
            w, h = int(rng.integers(0, 300)), int(rng.integers(0, 60))
            x0, y0 = int(r[0, 0]), int(r[0, 1])
            r = np.roll(np.array([[x0, y0], [x0 + w, y0], [x0 + w, y0 + h], [x0, y0 + h]]), k % 4, axis=0)
        cpt.append({"rect": r.tolist(), "out": [int(v) for v in np.asarray(bt.cpt_bezier_pts(r.tolist())).reshape(-1)]})

    conds = []
    real_pinv = np.linalg.pinv

    def watching_pinv(a, *args, **kw):
        conds.append(float(np.linalg.cond(np.asarray(a, dtype=np.float64))))
        return real_pinv(a, *args, **kw)

    curved = []
    np.linalg.pinv = watching_pinv
    try:
        for k in range(40):
            x = np.cumsum(rng.integers(3, 60, 7)) + rng.integers(0, 600)
            base = rng.integers(40, 600)
            top = np.stack([x, base + np.rint(rng.uniform(5, 40) * np.sin(np.linspace(0, rng.uniform(1, 3), 7))).astype(int)], 1)
            height = int(rng.integers(8, 60))
            bottom = np.stack([x[::-1] + rng.integers(-2, 3, 7), top[::-1, 1] + height + rng.integers(0, 3, 7)], 1)
            poly = np.concatenate([top, bottom]).astype(np.float32)
            assert len(set(map(tuple, poly.tolist()))) == 14
            del conds[:]
            out = bt.polygon_to_bezier_pts(poly)
            curved.append({"poly": poly.astype(int).reshape(-1).tolist(), "out": [float(v) for v in np.asarray(out).reshape(-1)],
                           "cond": list(conds)})
    finally:
        np.linalg.pinv = real_pinv
    path = os.path.join(GOLDEN, "prepare_geometry.json")
    with open(path, "w") as f:
        json.dump({"get_tight_rect": tight, "cpt_bezier_pts": cpt, "polygon_to_bezier_pts": curved}, f, indent=None, separators=(",", ":"))
    print("wrote %s: %d tight rects, %d rects, %d 14-gons (cond %.1f .. %.1f), %d bytes" % (
        path, len(tight), len(cpt), len(curved), min(min(c["cond"]) for c in curved), max(max(c["cond"]) for c in curved),
        os.path.getsize(path)))


# ------------------------------------------------------------------------------------------------- (b) the raw tree
def _xml_object(oid, text, pts, lang=None, lang_key="Language"):
    attrs = 'Transcription="%s" ID="%s"' % (text, oid)
    if lang is not None:
        attrs += ' %s="%s"' % (lang_key, lang)
    body = "".join('      <Point x="%d" y="%d" />\n' % (x, y) for x, y in pts)
    return '    <object %s Quality="HIGH">\n%s    </object>\n' % (attrs, body)


def _xml(frames):
    """frames: [(frame id, [object xml])]"""
    out = ['<?xml version="1.0" encoding="utf-8"?>\n<Frames>\n']
    for fid, objs in frames:
        out.append('  <frame ID="%d">\n%s  </frame>\n' % (fid, "".join(objs)))
    out.append("</Frames>\n")
    return "".join(out)


def _quad(x, y, w, h, skew=0):
    return [(x, y), (x + w, y + skew), (x + w, y + h + skew), (x, y + h)]


def raw_tree():
    """-> ({relative path: text}, {relative frame directory: [count, H, W]})"""
    files, frames = {}, {}
    # ---- ICDAR15: every branch of the language test, a repeated id, a don't-care, coordinates outside the image, and the
    # Video_18_3_1 exclusions (ids 65007 after frame 133, 65001 after frame 135)
    o = _xml_object
    v5 = [(1, [o(1001, "Hello", _quad(10, 12, 40, 10, 2), "English"), o(1002, "hola", _quad(60, 30, 30, 8), "Spanish"),
               o(1001, "again", _quad(1, 1, 5, 5), "English"), o(1003, "##DONT#CARE##", _quad(-5, -3, 20, 9), "English")]),
          (2, [o(1001, "Hello", _quad(12, 12, 40, 10, 3), "French"), o(1004, "plaça", _quad(70, 40, 30, 12), "Catalan"),
               o(1005, "テキスト", _quad(100, 70, 40, 30), "Japanese"), o(1006, "NoLang", _quad(90, 5, 50, 9, -4))]),
          (3, [o(1002, "hola", [(150, 80), (170, 95), (160, 110), (140, 93)], "Spanish"),
               o(1007, "edge", _quad(120, 85, 60, 20), "English")])]
    files["ICDAR15/ICDAR15_train/Video_5_2_0_GT.xml"] = _xml(v5)
    frames["ICDAR15/frame/Video_5_2_0"] = [3, 96, 160]
    v18 = []
    for fid in range(1, 138):
        objs = []
        if fid in (1, 133, 134, 135, 136, 137):
            objs = [o(65007, "seven", _quad(20, 10, 30, 8), "English"), o(65001, "one", _quad(20, 30, 30, 8, 1), "English"),
                    o(65002, "two", _quad(60, 40, 25, 9), "English")]
        v18.append((fid, objs))
    files["ICDAR15/ICDAR15_train/Video_18_3_1_GT.xml"] = _xml(v18)
    frames["ICDAR15/frame/Video_18_3_1"] = [137, 72, 128]
    # ---- DSText: ids compared as strings ("7" and "07" are two objects with one instance id), `language`
    d = lambda *a: _xml_object(*a, lang_key="language")
    files["DSText/Train_annotation/Activity/Video_163_6_3_GT.xml"] = _xml([
        (1, [d("7", "SALE", _quad(5, 5, 30, 9), "English"), d("07", "sale", _quad(40, 5, 30, 9, 2), "English"),
             d("7", "dup", _quad(1, 1, 4, 4), "English"), d("9", "中文", _quad(50, 30, 40, 14), "Chinese")]),
        (2, [d("9", "##DONT#CARE##", _quad(52, 31, 40, 14), "Chinese"), d("11", "Out", _quad(110, 60, 40, 20), "English")])])
    frames["DSText/frame/Activity/Video_163_6_3"] = [2, 64, 120]
    files["DSText/Train_annotation/Driving/Video_44_6_4_GT.xml"] = _xml([
        (1, [d("3", "STOP", [(30, 20), (60, 10), (66, 24), (36, 35)], "English")]),
        (2, []),
        (3, [d("3", "STOP", [(32, 22), (62, 12), (68, 26), (38, 37)], "English"), d("4", "##DONT#CARE##", _quad(-4, 50, 12, 20), "English")])])
    frames["DSText/frame/Driving/Video_44_6_4"] = [3, 80, 100]
    # ---- BOVText: float points (truncated toward zero, negative ones included), `line` annotations
    files["BOVText/Train/train_annotation/Cls1_Livestreaming/Cls1_Livestreaming_video12.json"] = json.dumps({
        "1": [{"ID": "1", "transcription": "直播", "language": "Chinese", "points": [10.7, 20.2, 90.9, 22.5, 90.1, 40.99, 10.2, 38.4], "category": "caption"},
              {"ID": "2", "transcription": "LIVE now", "language": "English", "points": [-3.9, -0.5, 30.5, 2.5, 29.5, 14.5, -4.2, 11.8], "category": "title"}],
        "2": [{"ID": "1", "transcription": "##DONT#CARE##", "language": "Chinese", "points": [11, 21, 91, 23, 90, 41, 10, 39], "category": "caption"}],
        "3": []}, ensure_ascii=False, indent=1)
    frames["BOVText/frame/Cls1_Livestreaming/Cls1_Livestreaming_video12"] = [3, 90, 150]
    files["BOVText/Train/train_annotation/Cls7_Game/Cls7_Game_video3.json"] = json.dumps({
        "1": [{"ID": "5", "transcription": "Score 10", "language": "English", "points": [100.5, 50.5, 170.25, 60.75, 168.0, 75.5, 98.5, 65.0], "category": "scene"}],
        "2": [{"ID": "5", "transcription": "Score 11", "language": "English", "points": [101.5, 50.5, 171.25, 60.75, 169.0, 75.5, 99.5, 65.0], "category": "scene"},
              {"ID": "6", "transcription": "外", "language": "Chinese", "points": [150.0, 90.0, 190.0, 90.0, 190.0, 110.0, 150.0, 110.0], "category": "scene"}]},
        ensure_ascii=False, indent=1)
    frames["BOVText/frame/Cls7_Game/Cls7_Game_video3"] = [2, 100, 180]
    return files, frames


def write_frames(root, frames):
    """The .jpg frames of `frames` ({relative directory: [count, H, W]}) under `root`: one encoded image per video, copied."""
    from PIL import Image
    for rel, (count, H, W) in frames.items():
        d = os.path.join(root, rel)
        os.makedirs(d, exist_ok=True)
        buf = io.BytesIO()
        Image.new("RGB", (W, H), (90, 120, 150)).save(buf, format="JPEG")
        for k in range(1, count + 1):
            with open(os.path.join(d, "%d.jpg" % k), "wb") as f:
                f.write(buf.getvalue())


def converters():
    from PIL import Image
    from gomatching_amd.prepare import BOVTEXT_CLASSES
    files, frames = raw_tree()
    cv2 = types.ModuleType("cv2")
    cv2.imread = lambda path: np.asarray(Image.open(path).convert("RGB"))[:, :, ::-1]
    tqdm = types.ModuleType("tqdm")
    tqdm.tqdm = lambda it, *a, **k: it
    sys.modules["cv2"], sys.modules["tqdm"] = cv2, tqdm
    if os.path.isdir(RAW):
        shutil.rmtree(RAW)
    order = {}
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        ds = os.path.join(tmp, "datasets")
        for rel, text in files.items():
            for base in (ds, RAW):
                os.makedirs(os.path.dirname(os.path.join(base, rel)), exist_ok=True)
                with open(os.path.join(base, rel), "w", encoding="utf-8") as f:
                    f.write(text)
        for c in BOVTEXT_CLASSES:                                # the script lists every class directory
            os.makedirs(os.path.join(ds, "BOVText/Train/train_annotation", c), exist_ok=True)
        write_frames(ds, frames)
        os.chdir(tmp)
        try:
            for name, ds_dir, suffix in (("icdar15", "ICDAR15", "_GT.xml"), ("dstext", "DSText", "_GT.xml"), ("bovtext", "BOVText", ".json")):
                with contextlib.redirect_stdout(io.StringIO()):
                    runpy.run_path(os.path.join(ref_shim.REF_ROOT, "tools", "convert_gom_label", name + ".py"), run_name="__main__")
                with open(os.path.join(ds, ds_dir, "train.json"), "rb") as f:
                    raw = f.read()
                with open(os.path.join(RAW, name + "_train.json"), "wb") as f:
                    f.write(raw)
                doc = json.loads(raw.decode("utf-8"))
                first = {}
                for im in doc["images"]:
                    first.setdefault(im["video_id"], im["file_name"])
                order[name] = [(v["file_name"] + suffix) if name == "icdar15" else
                               (first[v["id"]].split("/")[0] + "/" + v["file_name"] + suffix) for v in doc["videos"]]
                print("%s: %d videos, %d images, %d annotations, order %s" % (name, len(doc["videos"]), len(doc["images"]),
                                                                             len(doc["annotations"]), order[name]))
        finally:
            os.chdir(cwd)
    with open(os.path.join(RAW, "video_order.json"), "w") as f:
        json.dump(order, f, indent=1)
    with open(os.path.join(RAW, "frames.json"), "w") as f:
        json.dump(frames, f, indent=1)


def main():
    if not ref_shim.reference_available():
        raise SystemExit("reference tree not present at %s" % ref_shim.REF_ROOT)
    geometry()
    converters()


if __name__ == "__main__":
    main()
