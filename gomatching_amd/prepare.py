"""Raw annotations -> the `train.json` the train command reads, with the Bezier control points precomputed.

    python -m gomatching_amd.prepare icdar15 --annotations DIR --frames DIR --output train.json
    python -m gomatching_amd.prepare dstext  --annotations DIR --frames DIR --output train.json
    python -m gomatching_amd.prepare bovtext --annotations DIR --frames DIR --output train.json
    python -m gomatching_amd.prepare bezier  --json IN.json --output OUT.json
            [--host-bezier] [--no-bezier]

The three converters restate tools/convert_gom_label/{icdar15,dstext,bovtext}.py: record layout, key order, id numbering,
`prev_image_id` / `next_image_id`, duplicate-object skipping (DSText compares ids as strings, ICDAR15 as ints), the two
`Video_18_3_1` exclusions, the language tables, BOVText's float32 -> int32 truncation and its fixed class list.  Deliberate
differences: videos are taken in SORTED order (the reference takes `os.listdir` order, so its ids depend on the file system;
`video_order=` reproduces any order), the frame size comes from Pillow's header read of `1.jpg`, BOVText classes missing from
the annotation directory are skipped, nothing is printed per video.

The reference's converters write `poly` and never `bezier_pts`; its loader derives the control points on every load with cv2
and shapely (datasets/vts.py:154-166).  `data.load_video_json` does not: a `poly`-only annotation loads without its point
fields.  Here the points are computed ONCE and written into the json as `bezier_pts` (both loaders prefer that field), right
after `poly`, for every annotation that has `poly` and no `bezier_pts`:
  * a quad goes through the integer / fp64 rule of include/gomatching_hip.h ("Quad -> Bezier control points"): all quads of
    the dataset in ONE upload, ONE `gom_quad_bezier_i32` launch (csrc/prepare.hip) and ONE copy back; `--host-bezier` runs
    `quad_bezier_host`, the same rule in numpy vectorised over the annotations, and writes the same bytes;
  * a 14-gon (curved text) is fitted on the host: `fit_14gon`, the reference's chord-length least squares;
  * any other point count is an error naming the annotation.
`--no-bezier` writes the reference's file exactly.  Parity of the quad rule with cv2.minAreaRect / cv2.boxPoints /
shapely's is_ccw is UNPINNED (README, "prepare").

Exit status 2, with a message naming the file: a missing directory or file, a video without `1.jpg`, a frame-count mismatch,
a bad point count.  Without a GPU and without `--host-bezier` the command refuses (status 1): the numpy path is a choice, not a
fall-back.
"""
import argparse
import glob
import json
import os
import sys
import xml.etree.ElementTree as ET

import numpy as np

CATEGORIES = [{"supercategory": "beverage", "id": 1,
               "keypoints": ["mean", "xmin", "x2", "x3", "xmax", "ymin", "y2", "y3", "ymax", "cross"],
               "name": "text"}]
BOVTEXT_CLASSES = ["Cls1_Livestreaming", "Cls2_Cartoon", "Cls3_Sports", "Cls4_Celebrity", "Cls5_Advertising", "Cls6_NewsReport",
                   "Cls7_Game", "Cls8_Comedy", "Cls9_Activity", "Cls10_Program", "Cls11_Movie", "Cls12_Interview",
                   "Cls13_Introduction", "Cls14_Talent", "Cls15_Photograph", "Cls16_Government", "Cls17_Speech", "Cls18_Travel",
                   "Cls19_Fashion", "Cls20_Campus", "Cls21_Vlog", "Cls22_Driving", "Cls23_International", "Cls24_Fishery",
                   "Cls25_ShortVideo", "Cls26_Technology", "Cls27_Education", "Cls28_BeautyIndustry", "Cls29_Makeup", "Cls30_Dance",
                   "Cls31_Eating", "Cls32_Unknown"]
ICDAR15_ALPHANUMERIC = ("English", "Catalan", "Spanish", "French")
DEFAULTS = {"icdar15": ("datasets/ICDAR15/ICDAR15_train/", "datasets/ICDAR15/frame", "datasets/ICDAR15/train.json"),
            "dstext": ("datasets/DSText/Train_annotation/", "datasets/DSText/frame", "datasets/DSText/train.json"),
            "bovtext": ("datasets/BOVText/Train/train_annotation/", "datasets/BOVText/frame", "datasets/BOVText/train.json")}


class PrepareError(Exception):
    """An input the command cannot convert; the message names the file.  Exit status 2."""


class NoDeviceError(Exception):
    """The device path was asked for and there is no GPU.  Exit status 1: there is no quiet fall-back to numpy."""


# ------------------------------------------------------------------------------------------------- converters
def _listdir(path):
    if not os.path.isdir(path):
        raise PrepareError("%s: no such directory" % path)
    return sorted(os.listdir(path))


def _frames_of(image_path):
    """-> (number of .jpg frames, height, width); the size from the header of 1.jpg, nothing is decoded."""
    from PIL import Image
    first = os.path.join(image_path, "1.jpg")
    if not os.path.isfile(first):
        raise PrepareError("%s: the video has no first frame (1.jpg)" % first)
    try:
        with Image.open(first) as im:
            w, h = im.size
    except OSError as e:
        raise PrepareError("%s: not a readable image (%s)" % (first, e))
    return len(glob.glob(image_path + "/*.jpg")), h, w


def _new_doc():
    return {"images": [], "annotations": [], "categories": [dict(c, keypoints=list(c["keypoints"])) for c in CATEGORIES], "videos": []}


def _image_info(name, img_id, h, w, frame_id, num_images, video_id):
    return {"file_name": name, "id": img_id, "height": h, "width": w, "frame_id": frame_id,
            "prev_image_id": img_id - 1 if frame_id > 1 else -1,
            "next_image_id": img_id + 1 if frame_id < num_images else -1,
            "video_id": video_id}


def _ann_info(ann_cnt, text_category, transcription, img_id, obj_id, xs, ys, poly, anno_type):
    x_min, y_min = min(xs), min(ys)
    return {"id": ann_cnt, "category_id": 1, "text_category": text_category, "transcription": transcription,
            "image_id": img_id, "instance_id": int(obj_id), "bbox": [x_min, y_min, max(xs) - x_min, max(ys) - y_min],
            "poly": poly, "anno_type": anno_type, "box_type": "quadrilateral", "iscrowd": 0}


def _xml_frames(xml_path, num_images):
    try:
        frames = ET.parse(xml_path).getroot().findall("frame")
    except (OSError, ET.ParseError) as e:
        raise PrepareError("%s: cannot be read as XML (%s)" % (xml_path, e))
    if num_images != len(frames):
        raise PrepareError("%s: video %s has %d frames on disk and %d in its annotation"
                           % (xml_path, os.path.basename(xml_path).split("_GT")[0], num_images, len(frames)))
    return frames


def _xml_points(obj):
    xs, ys, poly = [], [], []
    for point in obj.findall("Point"):
        x, y = int(point.attrib["x"]), int(point.attrib["y"])
        xs.append(x)
        ys.append(y)
        poly.append([x, y])
    return xs, ys, poly


def convert_icdar15(annotations, frames, video_order=None):
    """tools/convert_gom_label/icdar15.py: `annotations` holds <video>_GT.xml files, `frames` one directory of N.jpg per
    video.  `video_order`: the xml file names in the order to take them (default: sorted)."""
    out = _new_doc()
    xml_files = [f for f in (video_order if video_order is not None else _listdir(annotations)) if ".xml" in f]
    video_id = img_id = ann_cnt = 0
    for xml_file in xml_files:
        video_id += 1
        file_name = xml_file.split("_GT")[0]
        out["videos"].append({"id": video_id, "file_name": file_name, "data_source": "ICDAR15_video"})
        num_images, h, w = _frames_of(os.path.join(frames, file_name))
        for frame in _xml_frames(os.path.join(annotations, xml_file), num_images):
            frame_id = int(frame.attrib["ID"])
            img_id += 1
            out["images"].append(_image_info("{}/{}".format(file_name, str(frame_id) + ".jpg"), img_id, h, w, frame_id,
                                             num_images, video_id))
            obj_ids = []
            for obj in frame.findall("object"):
                detail = obj.attrib
                obj_id = int(detail["ID"])
                if file_name == "Video_18_3_1" and frame_id > 133 and obj_id == 65007:
                    continue
                if file_name == "Video_18_3_1" and frame_id > 135 and obj_id == 65001:
                    continue
                if obj_id in obj_ids:
                    continue
                obj_ids.append(obj_id)
                ann_cnt += 1
                if detail["Transcription"] == "##DONT#CARE##":
                    transcription, text_category = "###", "other"
                else:
                    transcription = detail["Transcription"]
                    text_category = "alphanumeric" if "Language" not in detail or detail["Language"] in ICDAR15_ALPHANUMERIC \
                        else "nonalphanumeric"
                xs, ys, poly = _xml_points(obj)
                out["annotations"].append(_ann_info(ann_cnt, text_category, transcription, img_id, obj_id, xs, ys, poly, "word"))
    return out


def _class_files(annotations, classes, video_order):
    """-> [(class directory, file)] in the order to take them: `video_order` ("class/file" strings) or sorted."""
    if video_order is not None:
        return [tuple(v.split("/", 1)) for v in video_order]
    return [(c, f) for c in classes for f in _listdir(os.path.join(annotations, c))]


def convert_dstext(annotations, frames, video_order=None):
    """tools/convert_gom_label/dstext.py: `annotations`/<class>/<video>_GT.xml, `frames`/<class>/<video>/N.jpg.
    `video_order`: "class/file.xml" strings in the order to take them (default: classes sorted, files sorted)."""
    out = _new_doc()
    video_id = img_id = ann_cnt = 0
    for seq_dir, xml_file in _class_files(annotations, _listdir(annotations) if video_order is None else None, video_order):
        video_id += 1
        file_name = xml_file.split("_GT")[0]
        xml_path = os.path.join(annotations, seq_dir, xml_file)
        out["videos"].append({"id": video_id, "file_name": file_name, "data_source": "DSText"})
        num_images, h, w = _frames_of(os.path.join(frames, seq_dir, file_name))
        for frame in _xml_frames(xml_path, num_images):
            frame_id = int(frame.attrib["ID"])
            img_id += 1
            out["images"].append(_image_info("{}/{}/{}".format(seq_dir, file_name, str(frame_id) + ".jpg"), img_id, h, w,
                                             frame_id, num_images, video_id))
            obj_ids = []
            for obj in frame.findall("object"):
                detail = obj.attrib
                obj_id = detail["ID"]                            # compared as a string
                if obj_id in obj_ids:
                    continue
                obj_ids.append(obj_id)
                ann_cnt += 1
                if detail["Transcription"] == "##DONT#CARE##":
                    transcription, text_category = "###", "other"
                else:
                    transcription = detail["Transcription"]
                    if "language" not in detail:
                        raise PrepareError("%s: object %s of frame %d has no `language`" % (xml_path, obj_id, frame_id))
                    text_category = "nonalphanumeric" if detail["language"] == "Chinese" else "alphanumeric"
                xs, ys, poly = _xml_points(obj)
                out["annotations"].append(_ann_info(ann_cnt, text_category, transcription, img_id, obj_id, xs, ys, poly, "word"))
    return out


def convert_bovtext(annotations, frames, video_order=None):
    """tools/convert_gom_label/bovtext.py: `annotations`/<class>/<video>.json = {frame id: [objects]}, `frames`/<class>/<video>/
    N.jpg.  The classes are the fixed list, in its order; one that `annotations` does not hold is skipped.  `video_order`:
    "class/file.json" strings in the order to take them (default: files sorted within each class)."""
    if not os.path.isdir(annotations):
        raise PrepareError("%s: no such directory" % annotations)
    out = _new_doc()
    classes = [c for c in BOVTEXT_CLASSES if os.path.isdir(os.path.join(annotations, c))]
    video_id = img_id = ann_cnt = 0
    for seq_dir, json_file in _class_files(annotations, classes, video_order):
        video_id += 1
        file_name = json_file.split(".")[0]
        json_path = os.path.join(annotations, seq_dir, json_file)
        out["videos"].append({"id": video_id, "file_name": file_name, "data_source": "BOVText"})
        num_images, h, w = _frames_of(os.path.join(frames, seq_dir, file_name))
        try:
            with open(json_path, "r", encoding="utf-8") as f:
                video = json.load(f)
        except (OSError, ValueError) as e:
            raise PrepareError("%s: cannot be read as json (%s)" % (json_path, e))
        for frame_id, objects in video.items():
            frame_id = int(frame_id)
            img_id += 1
            out["images"].append(_image_info("{}/{}/{}".format(seq_dir, file_name, str(frame_id) + ".jpg"), img_id, h, w,
                                             frame_id, num_images, video_id))
            for obj in objects:
                ann_cnt += 1
                if obj["transcription"] == "##DONT#CARE##":
                    transcription, text_category = "###", "other"
                else:
                    transcription = obj["transcription"]
                    text_category = "nonalphanumeric" if obj["language"] == "Chinese" else "alphanumeric"
                points = np.array(obj["points"], dtype=np.float32).astype(np.int32)
                out["annotations"].append(_ann_info(ann_cnt, text_category, transcription, img_id, obj["ID"], points[::2].tolist(),
                                                    points[1::2].tolist(), points.reshape(-1, 2).tolist(), "line"))
    return out


CONVERTERS = {"icdar15": convert_icdar15, "dstext": convert_dstext, "bovtext": convert_bovtext}


# ------------------------------------------------------------------------------------------------- quads, on the host
def _take(a, idx):
    return np.take_along_axis(a, idx, axis=1)


def quad_bezier_host(quads, hw):
    """The rule of `gom_quad_bezier_i32` (include/gomatching_hip.h) in numpy, vectorised over the quads: quads int [n,8],
    hw int [n,2] (H, W) -> int32 [n,16].  Integers in int64, the rest in float64 with every product, sum, quotient and square
    root an array operation of its own (numpy fuses nothing), so each is rounded once, as in the kernel."""
    q = np.asarray(quads).reshape(-1, 4, 2).astype(np.int64)
    hw = np.asarray(hw).reshape(-1, 2).astype(np.int64)
    n = q.shape[0]
    if hw.shape[0] != n:
        raise ValueError("quad_bezier_host: %d quads but %d image sizes" % (n, hw.shape[0]))
    if n == 0:
        return np.zeros((0, 16), dtype=np.int32)
    rows = np.arange(n)
    # 1. hull: the distinct points sorted by (x, y), monotone chain with `cross <= 0` popping, lower[:-1] + upper[:-1]
    order = np.lexsort((q[:, :, 1], q[:, :, 0]), axis=1)
    sx, sy = _take(q[:, :, 0], order), _take(q[:, :, 1], order)
    valid = np.ones((n, 4), dtype=bool)
    valid[:, 1:] = (sx[:, 1:] != sx[:, :-1]) | (sy[:, 1:] != sy[:, :-1])

    def chain(seq):
        st, sz = np.zeros((n, 4), dtype=np.int64), np.zeros(n, dtype=np.int64)
        for i in seq:
            act = valid[:, i]
            for _ in range(2):                                   # at most two pops: the stack holds three points or fewer
                a, b = st[rows, np.maximum(sz - 2, 0)], st[rows, np.maximum(sz - 1, 0)]
                ax, ay = sx[rows, a], sy[rows, a]
                cr = (sx[rows, b] - ax) * (sy[:, i] - ay) - (sy[rows, b] - ay) * (sx[:, i] - ax)
                sz = sz - (act & (sz >= 2) & (cr <= 0))
            st[rows[act], sz[act]] = i
            sz = sz + act
        return st, sz

    lo, nl = chain(range(4))
    up, nup = chain(range(3, -1, -1))
    single = valid.sum(1) == 1
    nh = np.where(single, 1, nl + nup - 2)
    hidx = np.zeros((n, 4), dtype=np.int64)
    for k in range(4):
        in_lower = k < nl - 1
        hidx[:, k] = np.where(in_lower, lo[rows, min(k, 3)], up[rows, np.clip(k - (nl - 1), 0, 3)])
    hidx[single, 0] = 0
    hx, hy = _take(sx, hidx).astype(np.float64), _take(sy, hidx).astype(np.float64)
    # 2. minimum-area rectangle over the hull's edges in hull order, the first strict minimum wins
    has = np.zeros(n, dtype=bool)
    best = np.zeros(n)
    keep = np.zeros((6, n))                                       # ux, uy, umin, umax, vmin, vmax of the best edge
    with np.errstate(invalid="ignore", divide="ignore"):
        for i in range(4):
            ok = (i < nh) & (nh >= 2)
            nxt = np.where(i + 1 == nh, 0, min(i + 1, 3))
            ex, ey = hx[rows, nxt] - hx[:, i], hy[rows, nxt] - hy[:, i]
            norm = np.sqrt(ex * ex + ey * ey)
            ok &= norm != 0
            ux, uy = ex / norm, ey / norm
            for j in range(4):
                pu = hx[:, j] * ux + hy[:, j] * uy
                pv = hy[:, j] * ux - hx[:, j] * uy
                if j == 0:
                    umin, umax, vmin, vmax = pu, pu, pv, pv
                else:
                    m = j < nh
                    umax = np.where(m & (pu > umax), pu, umax)
                    umin = np.where(m & (pu < umin), pu, umin)
                    vmax = np.where(m & (pv > vmax), pv, vmax)
                    vmin = np.where(m & (pv < vmin), pv, vmin)
            area = (umax - umin) * (vmax - vmin)
            better = ok & (~has | (area < best))
            best = np.where(better, area, best)
            keep = np.where(better[None], np.stack([ux, uy, umin, umax, vmin, vmax]), keep)
            has |= better
    ux, uy, umin, umax, vmin, vmax = keep
    # 3. corners straight from the unit vector, truncated toward zero
    cu, cv = np.stack([umin, umax, umax, umin], 1), np.stack([vmin, vmin, vmax, vmax], 1)
    cx = (cu * ux[:, None] - cv * uy[:, None]).astype(np.int64)
    cy = (cu * uy[:, None] + cv * ux[:, None]).astype(np.int64)
    one = nh == 1
    cx[one], cy[one] = sx[one, :1], sy[one, :1]
    # 4. get_tight_rect: stable sort by x, the two `>` comparisons on y, the clamp
    o = np.argsort(cx, axis=1, kind="stable")
    px, py = _take(cx, o), _take(cy, o)
    left, right = py[:, 1] > py[:, 0], py[:, 3] > py[:, 2]
    pick = np.stack([np.where(left, 0, 1), np.where(right, 2, 3), np.where(right, 3, 2), np.where(left, 1, 0)], 1)
    rx = np.minimum(np.maximum(_take(px, pick), 1), hw[:, 1:2] - 1)
    ry = np.minimum(np.maximum(_take(py, pick), 1), hw[:, 0:1] - 1)
    # 5. orientation: reversed iff the shoelace sum is negative
    s = (rx * np.roll(ry, -1, axis=1) - np.roll(rx, -1, axis=1) * ry).sum(1)
    rx = np.where((s < 0)[:, None], rx[:, ::-1], rx)
    ry = np.where((s < 0)[:, None], ry[:, ::-1], ry)
    # 6. cpt_bezier_pts: the two longest edges, ties to the lower index, thirds truncated toward zero
    dx, dy = np.roll(rx, -1, axis=1) - rx, np.roll(ry, -1, axis=1) - ry
    first = np.argsort(-(dx * dx + dy * dy), axis=1, kind="stable")[:, :2]
    second = (first + 1) % 4
    out = np.empty((n, 2, 4, 2), dtype=np.int64)
    for c, r in enumerate((rx, ry)):
        p1, p2 = _take(r, first), _take(r, second)
        out[:, :, 0, c], out[:, :, 3, c] = p1, p2
        for k in (1, 2):
            t = k / 3
            out[:, :, k, c] = ((1 - t) * p1.astype(np.float64) + t * p2.astype(np.float64)).astype(np.int64)
    return out.reshape(n, 16).astype(np.int32)


def quad_bezier_device(quads, hw):
    """The same through `ops.quad_bezier`: one upload (quads and sizes in one buffer), one launch, one copy back."""
    import torch
    from . import ops
    quads = np.ascontiguousarray(np.asarray(quads, dtype=np.int32).reshape(-1, 8))
    hw = np.ascontiguousarray(np.asarray(hw, dtype=np.int32).reshape(-1, 2))
    n = quads.shape[0]
    if not torch.cuda.is_available():
        raise NoDeviceError("no GPU: the control points of quads are computed by gom_quad_bezier_i32; pass --host-bezier for the "
                            "numpy path")
    packed = torch.from_numpy(np.concatenate([quads.reshape(-1), hw.reshape(-1)])).cuda()
    return ops.quad_bezier(packed[:8 * n].view(n, 8), packed[8 * n:].view(n, 2)).cpu().numpy()


# ------------------------------------------------------------------------------------------------- 14-gons, on the host
def _bezier_fit(x, y):
    """`bezier_fit` of bezier_tools.py: chord-length parameters, pinv of the Bernstein matrix -> the two middle control
    points.  x, y are float32 as vts.py:156 makes them, so the chord lengths and parameters are float32 values too."""
    dy, dx = y[1:] - y[:-1], x[1:] - x[:-1]
    dt = (dx ** 2 + dy ** 2) ** 0.5
    t = np.hstack(([0], dt / dt.sum())).cumsum()
    bern = np.array([[tt ** k * (1 - tt) ** (3 - k) * (1.0, 3.0, 3.0, 1.0)[k] for k in range(4)] for tt in t])
    return np.linalg.pinv(bern).dot(np.column_stack((x, y)))[1:-1], bern


def fit_14gon(poly):
    """`polygon_to_bezier_pts` for 14 points (7 along the top, then 7 along the bottom): per side a cubic whose end control
    points are the first and last data points and whose middle ones come from `_bezier_fit`.  -> 16 floats."""
    p = np.asarray(poly).reshape(-1, 2).astype(np.float32)
    out = []
    for side in (p[:7], p[7:]):
        mid, _ = _bezier_fit(side[:, 0], side[:, 1])
        out += [float(side[0, 0]), float(side[0, 1])] + [float(v) for v in mid.reshape(-1)] + [float(side[-1, 0]), float(side[-1, 1])]
    return out


# ------------------------------------------------------------------------------------------------- bezier_pts into a json
def needs_bezier(doc):
    return [a for a in doc.get("annotations", []) if "poly" in a and "bezier_pts" not in a]


def add_bezier(doc, host=False, name="<json>"):
    """Adds `bezier_pts` (right after `poly`) to every annotation of `doc` that has `poly` and no `bezier_pts`; in place.
    -> (number of quads, number of 14-gons)."""
    todo = needs_bezier(doc)
    size = {im["id"]: (im["height"], im["width"]) for im in doc.get("images", [])}
    quads, hw, where, curved = [], [], [], 0
    for ann in todo:
        pts = np.asarray(ann["poly"]).reshape(-1)
        if pts.size == 8:
            if ann["image_id"] not in size:
                raise PrepareError("%s: annotation %r names image %r, which the json does not list" % (name, ann.get("id"), ann["image_id"]))
            quads.append(pts)
            hw.append(size[ann["image_id"]])
            where.append(ann)
        elif pts.size == 28:
            ann["bezier_pts"] = fit_14gon(pts)
            curved += 1
        else:
            raise PrepareError("%s: annotation %r: Error Num of points (%d numbers in `poly`; a quad has 8, a 14-gon 28)"
                               % (name, ann.get("id"), pts.size))
    if quads:
        q = np.trunc(np.asarray(quads, dtype=np.float64)).astype(np.int32)
        res = (quad_bezier_host if host else quad_bezier_device)(q, np.asarray(hw, dtype=np.int32))
        for ann, row in zip(where, res.tolist()):
            ann["bezier_pts"] = row
    for ann in todo:                                             # `bezier_pts` right after `poly`
        items = list(ann.items())
        ann.clear()
        for k, v in items:
            if k != "bezier_pts":
                ann[k] = v
            if k == "poly":
                ann["bezier_pts"] = dict(items)["bezier_pts"]
    return len(quads), curved


def dumps(doc):
    return json.dumps(doc, indent=2, ensure_ascii=False)


def _write(path, text):
    d = os.path.dirname(os.path.abspath(path))
    if not os.path.isdir(d):
        raise PrepareError("%s: the output's directory does not exist" % path)
    with open(path, "w", encoding="utf-8") as f:
        f.write(text)


# ------------------------------------------------------------------------------------------------- command line
def _parser():
    ap = argparse.ArgumentParser(prog="python -m gomatching_amd.prepare", description=__doc__.split("\n\n")[0])
    sub = ap.add_subparsers(dest="command", required=True)
    for name, (ann, frames, output) in DEFAULTS.items():
        p = sub.add_parser(name, help="convert raw %s annotations" % name)
        p.add_argument("--annotations", default=ann)
        p.add_argument("--frames", default=frames)
        p.add_argument("--output", default=output)
        p.add_argument("--no-bezier", action="store_true", help="write `poly` only: the reference's file exactly")
        p.add_argument("--host-bezier", action="store_true", help="compute the control points in numpy instead of on the GPU")
    p = sub.add_parser("bezier", help="add bezier_pts to an existing json")
    p.add_argument("--json", required=True)
    p.add_argument("--output", required=True)
    p.add_argument("--host-bezier", action="store_true")
    return ap


def run(args):
    if args.command == "bezier":
        try:
            with open(args.json, "rb") as f:
                raw = f.read()
            doc = json.loads(raw.decode("utf-8"))
        except (OSError, ValueError) as e:
            raise PrepareError("%s: cannot be read as json (%s)" % (args.json, e))
        if not needs_bezier(doc):                                # nothing to add: the file goes through as it is
            d = os.path.dirname(os.path.abspath(args.output))
            if not os.path.isdir(d):
                raise PrepareError("%s: the output's directory does not exist" % args.output)
            with open(args.output, "wb") as f:
                f.write(raw)
            return 0, 0
        counts = add_bezier(doc, host=args.host_bezier, name=args.json)
        _write(args.output, dumps(doc))
        return counts
    for d in (args.annotations, args.frames):
        if not os.path.isdir(d):
            raise PrepareError("%s: no such directory" % d)
    doc = CONVERTERS[args.command](args.annotations, args.frames)
    counts = (0, 0) if args.no_bezier else add_bezier(doc, host=args.host_bezier, name=args.annotations)
    _write(args.output, dumps(doc))
    print("%s: %d videos, %d images, %d instances (%d quads, %d curved) -> %s" % (
        args.command, len(doc["videos"]), len(doc["images"]), len(doc["annotations"]), counts[0], counts[1], args.output))
    return counts


def main(argv=None):
    args = _parser().parse_args(argv)
    try:
        run(args)
    except PrepareError as e:
        sys.stderr.write("prepare: %s\n" % e)
        return 2
    except NoDeviceError as e:
        sys.stderr.write("prepare: %s\n" % e)
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
