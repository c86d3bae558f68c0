"""Score result files: MOTA / MOTP / IDF1 of the DSText protocols.

    python -m gomatching_amd.score --gt GT --results RES [--e2e] [--threshold 0.5] [--host-iou] [--output scores.json]
    python -m gomatching_amd.score --protocol {dstext,bovtext,artvideo} ...
    python -m gomatching_amd.score --det --gt GT --results RES [--host-iou] [--per-frame] [--output scores.json]

`--det` is DSText's third protocol, the detection task (ICDAR15-style precision / recall / hmean per frame, the reference's
Evaluation_DSText_Det): it lives in score_det.py with its own reading rules (frames by position, no clamping, the converter's
point order and validity drop), its greedy per-frame matching in one launch per video (`ops.quad_det_match`,
csrc/score_det.hip) and its own list of deliberate differences; `--per-frame` adds its `per_sample` entries.  It does not
combine with --e2e, --curve or another --protocol.

`--protocol dstext` (the default) is what this module describes; `bovtext` and `artvideo` score the `<out>/jsons` of
`python -m gomatching_amd.eval` and live in score_json.py (the json readers, the OVERALL row, the transcription similarity
and ArTVideo's mask IoU on the pixel grid, csrc/mask_pairs.hip), with their own list of deliberate differences and of
UNPINNED libraries (cv2.fillPoly, pycocotools, Levenshtein, shapely).  Not built in any protocol: XSD validation, the
per-frame event dump, the Excel summary.

GT and RES are directories or .zip files.  GT holds `Video_<a>_<b>_<c>_GT.xml` (and `..._GT.txt` for --e2e); RES holds the
`res_Video_<a>_<b>_<c>.xml` / `.txt` that `python -m gomatching_amd.eval` writes into `<out>/preds`.  The figures are those of the
reference's tools/Evaluation_Protocol_DSText/{Evaluation_DSText_tracking/Track_video_2_0.py, Evaluation_DSText_E2E/E2E_video_2_0.py}
(`evaluate_method`), which need Polygon3, lxml, Levenshtein and motmetrics; here:

  * the pairwise polygon measure of a whole video (IoU of the convex hulls; for "don't care" regions the intersection over the
    detection's area) is two count / emit calls of `ops.quad_pairs` (csrc/score.hip); `--host-iou` runs the same arithmetic in
    numpy float64 instead (`host_quad_pairs`).  PARITY UNPINNED against Polygon3, which is not available to the tests: the
    geometry is held to tests/score_statement.py.
  * the CLEAR-MOT bookkeeping is `MOTAccumulator` below: `motmetrics.MOTAccumulator.update` and the metrics the protocols read,
    restated over the sparse kept pairs without pandas, every assignment through `ops.linear_sum_assignment`; pinned by
    tests/golden/score_mot.json, which the reference's own motmetrics produced.
  * the readers use zipfile and xml.etree (the protocol's XSD validation is left out; UNPINNED against lxml).

Where the two protocol scripts differ or fail, this module takes the better defined behaviour: a video without a single
counted detection scores zero in every figure (the tracking script stops with a KeyError there); videos are keyed by the
whole `<a>_<b>_<c>` (the scripts key by `<a>` alone, so that two videos sharing it overwrite each other); entries that match
no pattern are ignored; the overlap that drops detections on "don't care" regions is compared with 0.5 as in the scripts,
`--threshold` is the IoU threshold.
"""
import argparse
import json
import math
import os
import re
import sys
import xml.etree.ElementTree as ET
import zipfile

import numpy as np

GT_XML = r"Video_([0-9]+)_([0-9]+)_([0-9]+)_GT\.xml"
GT_TXT = r"Video_([0-9]+)_([0-9]+)_([0-9]+)_GT\.txt"
DET_XML = r"res_Video_([0-9]+)_([0-9]+)_([0-9]+)\.xml"
DET_TXT = r"res_Video_([0-9]+)_([0-9]+)_([0-9]+)\.txt"
DONT_CARE_OVERLAP = 0.5
_TXT_LINE = re.compile(r'^"([0-9]+)","(.*)"$')
_GT_TEXT_STRIP = re.compile(u"([^\u4e00-\u9fa5\u0030-\u0039\u0041-\u005a\u0061-\u007a])")


class ScoreError(Exception):
    """Bad input: reported as `error: ...` with exit status 2."""


# ------------------------------------------------------------------------------------------ geometry on the host
def _cross(ox, oy, ax, ay, bx, by):
    return (ax - ox) * (by - oy) - (ay - oy) * (bx - ox)


def quad_hulls(quads):
    """int [N,8] -> (hx, hy int64 [N,4], area2 int64 [N]): the convex hull of each 4-gon in four slots, counter-clockwise from
    the smallest (x, y) point, a dropped point's slot repeating a neighbour; twice the area.  The layout and the decisions
    are those of `quad_hull` in csrc/score.hip (monotone chain over four sorted points, integer cross products)."""
    q = np.asarray(quads, dtype=np.int64).reshape(-1, 8)
    x, y = q[:, 0::2], q[:, 1::2]
    order = np.lexsort((y, x))                                   # per row: by x, then y
    x, y = np.take_along_axis(x, order, 1), np.take_along_axis(y, order, 1)
    x0, x1, x2, x3 = x.T
    y0, y1, y2, y3 = y.T
    c1, c2 = _cross(x0, y0, x3, y3, x1, y1), _cross(x0, y0, x3, y3, x2, y2)
    l1, l2, u1, u2 = c1 < 0, c2 < 0, c1 > 0, c2 > 0
    both = l1 & l2
    drop1 = both & (_cross(x0, y0, x1, y1, x2, y2) <= 0)
    drop2 = both & ~drop1 & (_cross(x1, y1, x2, y2, x3, y3) <= 0)
    l1, l2 = l1 & ~drop1, l2 & ~drop2
    both = u1 & u2
    drop2 = both & (_cross(x3, y3, x2, y2, x1, y1) <= 0)
    drop1 = both & ~drop2 & (_cross(x2, y2, x1, y1, x0, y0) <= 0)
    u1, u2 = u1 & ~drop1, u2 & ~drop2

    def slots(p0, p1, p2, p3):
        w = np.where
        return np.stack([p0, w(l1, p1, w(l2, p2, p3)),
                         w(l1, w(l2, p2, p3), w(l2, p3, w(u2, p2, w(u1, p1, p3)))),
                         w(u1, p1, w(u2, p2, p3))], 1)
    hx, hy = slots(x0, x1, x2, x3), slots(y0, y1, y2, y3)
    area2 = np.zeros(len(q), dtype=np.int64)
    for i in range(4):
        j = (i + 1) & 3
        area2 += hx[:, i] * hy[:, j] - hx[:, j] * hy[:, i]
    return hx, hy, area2


def _clip_values(ghx, ghy, ga2, dhx, dhy, da2, measure):
    """The measure of N pairs given as hulls ([N,4] slots and twice the areas): `pair_value` of csrc/score.hip, the same fp64
    operations in the same order, over all pairs at once."""
    N = len(ga2)
    val = np.zeros(N, dtype=np.float64)
    if N == 0:
        return val
    ok = (ga2 > 0) & (da2 > 0)
    gx, gy = ghx.astype(np.float64), ghy.astype(np.float64)
    X, Y = np.zeros((N, 8)), np.zeros((N, 8))
    X[:, :4], Y[:, :4] = dhx, dhy
    n = np.full(N, 4, dtype=np.int64)
    rows = np.arange(N)
    with np.errstate(divide="ignore", invalid="ignore"):
        for e in range(4):
            e1 = (e + 1) & 3
            act = ok & ~((ghx[:, e] == ghx[:, e1]) & (ghy[:, e] == ghy[:, e1])) & (n > 0)
            if not act.any():
                continue
            ax, ay = gx[:, e], gy[:, e]
            ex, ey = gx[:, e1] - ax, gy[:, e1] - ay
            NX, NY = np.zeros((N, 8)), np.zeros((N, 8))
            m = np.zeros(N, dtype=np.int64)
            last = np.maximum(n - 1, 0)
            px, py = X[rows, last], Y[rows, last]
            dp = ex * (py - ay) - ey * (px - ax)
            for i in range(8):
                live = act & (i < n)
                if not live.any():
                    break
                cx, cy = X[:, i], Y[:, i]
                dc = ex * (cy - ay) - ey * (cx - ax)
                crossing = live & ((dc >= 0) != (dp >= 0))
                t = dp / (dp - dc)
                r = np.nonzero(crossing & (m < 8))[0]
                NX[r, m[r]] = (px + t * (cx - px))[r]
                NY[r, m[r]] = (py + t * (cy - py))[r]
                m += crossing
                inside = live & (dc >= 0)
                r = np.nonzero(inside & (m < 8))[0]
                NX[r, m[r]] = cx[r]
                NY[r, m[r]] = cy[r]
                m += inside
                px, py, dp = np.where(live, cx, px), np.where(live, cy, py), np.where(live, dc, dp)
            X, Y = np.where(act[:, None], NX, X), np.where(act[:, None], NY, Y)
            n = np.where(act, np.minimum(m, 8), n)
        s = np.zeros(N)
        last = np.maximum(n - 1, 0)
        px, py = X[rows, last], Y[rows, last]
        for i in range(8):
            live = i < n
            cx, cy = X[:, i], Y[:, i]
            s = np.where(live, s + (px * cy - cx * py), s)
            px, py = np.where(live, cx, px), np.where(live, cy, py)
        inter = np.abs(s) * 0.5
        ag, ad = ga2.astype(np.float64) * 0.5, da2.astype(np.float64) * 0.5
        if measure == 1:
            v = inter / ad
        else:
            uni = ag + ad - inter
            v = np.where(uni == 0, 0.0, inter / uni)
    good = ok & (n >= 3)
    val[good] = v[good]
    return val


def host_quad_pairs(gt_quads, det_quads, gt_off, det_off, gt_key, det_key, measure, threshold):
    """`ops.quad_pairs` on the host, numpy float64: -> (counts int32 [G], det int32 [K], value fp64 [K])."""
    gt_quads = np.asarray(gt_quads, dtype=np.int64).reshape(-1, 8)
    det_quads = np.asarray(det_quads, dtype=np.int64).reshape(-1, 8)
    G = len(gt_quads)
    ghx, ghy, ga2 = quad_hulls(gt_quads)
    dhx, dhy, da2 = quad_hulls(det_quads)
    gi, di, dl = [], [], []
    for f in range(len(gt_off) - 1):
        g0, g1, d0, d1 = int(gt_off[f]), int(gt_off[f + 1]), int(det_off[f]), int(det_off[f + 1])
        if g1 == g0 or d1 == d0:
            continue
        gs, ds = slice(g0, g1), slice(d0, d1)
        meet = (dhx[ds].min(1)[None, :] <= ghx[gs].max(1)[:, None]) & (ghx[gs].min(1)[:, None] <= dhx[ds].max(1)[None, :]) & \
            (dhy[ds].min(1)[None, :] <= ghy[gs].max(1)[:, None]) & (ghy[gs].min(1)[:, None] <= dhy[ds].max(1)[None, :]) & \
            (np.asarray(gt_key[gs])[:, None] == np.asarray(det_key[ds])[None, :])
        a, b = np.nonzero(meet)                                   # ground truth ascending, then detection ascending
        gi.append(a + g0)
        di.append(b + d0)
        dl.append(b)
    if not gi:
        return np.zeros(G, dtype=np.int32), np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.float64)
    gi, di, dl = np.concatenate(gi), np.concatenate(di), np.concatenate(dl)
    val = _clip_values(ghx[gi], ghy[gi], ga2[gi], dhx[di], dhy[di], da2[di], measure)
    keep = val > threshold
    counts = np.bincount(gi[keep], minlength=G).astype(np.int32)
    return counts, dl[keep].astype(np.int32), val[keep]


def device_quad_pairs(gt_quads, det_quads, gt_off, det_off, gt_key, det_key, measure, threshold):
    """`host_quad_pairs` through the kernels: one upload, the count and the emit launch, one copy back."""
    import torch
    from . import ops
    if not torch.cuda.is_available():
        raise ScoreError("no GPU: the polygon measure runs in csrc/score.hip (use --host-iou for the numpy path)")
    dev = torch.device("cuda", torch.cuda.current_device())

    def up(a, shape):
        return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32).reshape(shape)).to(dev)
    gt_off, det_off = np.asarray(gt_off, dtype=np.int64), np.asarray(det_off, dtype=np.int64)
    pairs = int(((gt_off[1:] - gt_off[:-1]) * (det_off[1:] - det_off[:-1])).sum())
    if pairs > 2 ** 31 - 1:
        raise ScoreError("a video with more than 2^31 - 1 (ground truth, detection) pairs is not supported")
    counts, det, val = ops.quad_pairs(up(gt_quads, (-1, 8)), up(det_quads, (-1, 8)), up(gt_off, (-1,)), up(det_off, (-1,)),
                                      up(gt_key, (-1,)), up(det_key, (-1,)), measure, threshold, pairs=pairs)
    return counts.cpu().numpy(), det.cpu().numpy(), val.cpu().numpy()


# ------------------------------------------------------------------------------------------ CLEAR-MOT accumulator
def _quiet_divide(a, b):
    a, b = float(a), float(b)
    if b == 0:
        return float("nan") if a == 0 or math.isnan(a) else math.copysign(float("inf"), a)
    return a / b


def _assign(costs):
    """motmetrics' `linear_sum_assignment` with its scipy solver: absent (NaN) edges become the large constant of
    `add_expensive_edges`, the solution's absent edges are dropped.  The solver is the library's own."""
    from . import ops
    if costs.size == 0:
        return np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)
    valid = np.isfinite(costs)
    if valid.all():
        finite = costs
    elif not valid.any():
        finite = np.zeros_like(costs)
    else:
        c = np.abs(costs[valid]).max() + 1
        finite = np.where(valid, costs, 2 * min(costs.shape) * c + 1)
    rids, cids = ops.linear_sum_assignment(finite)
    keep = valid[rids, cids]
    return rids[keep], cids[keep]


class MOTAccumulator:
    """`motmetrics.MOTAccumulator` (auto_id=False) restated for sparse distances, keeping only what the metrics read.
    Ids are integers.  `update` takes the frame's finite distances as (i, j, d) triples: object index, hypothesis index."""

    def __init__(self, max_switch_time=float("inf")):
        self.max_switch_time = max_switch_time
        self.m = {}                    # object -> hypothesis of its latest match
        self.last_occurrence = {}
        self.frames = set()
        self.num_matches = self.num_switches = self.num_false_positives = self.num_misses = 0
        self.obj_total, self.obj_tracked = {}, {}
        self.distances = []            # D of every MATCH / SWITCH event, in event order
        self.obj_frames, self.hyp_frames, self.pair_raw = {}, {}, {}     # the RAW events' counts (ID measures)

    def update(self, oids, hids, pairs, frameid):
        oids, hids = [int(o) for o in oids], [int(h) for h in hids]
        no, nh = len(oids), len(hids)
        dists = np.full((no, nh), np.nan)
        for i, j, d in pairs:
            if math.isfinite(d):
                dists[int(i), int(j)] = d
                key = (oids[int(i)], hids[int(j)])
                self.pair_raw[key] = self.pair_raw.get(key, 0) + 1
        self.frames.add(frameid)
        for ids, seen in ((oids, self.obj_frames), (hids, self.hyp_frames)):
            for k in set(ids):
                s = seen.setdefault(k, set())
                s.add(frameid)
        omask, hmask = np.zeros(no, dtype=bool), np.zeros(nh, dtype=bool)
        matched = []                                             # (object, distance) of this frame's MATCH / SWITCH events
        if no * nh > 0:
            # 1. re-establish the previous correspondences
            where = {}
            for j, h in enumerate(hids):
                where.setdefault(h, []).append(j)
            for i, o in enumerate(oids):
                if o not in self.m:
                    continue
                js = [j for j in where.get(self.m[o], ()) if not hmask[j]]
                if not js:
                    continue
                j = js[0]
                if np.isfinite(dists[i, j]):
                    omask[i] = hmask[j] = True
                    self.num_matches += 1
                    matched.append((o, dists[i, j]))
            # 2. assign the rest
            dists[omask, :] = np.nan
            dists[:, hmask] = np.nan
            if np.isfinite(dists).any():
                rids, cids = _assign(dists)
            else:
                rids = cids = ()
            for i, j in zip(rids, cids):
                o, h = oids[i], hids[j]
                # 3. a correspondence that contradicts the object's previous one is a SWITCH
                if o in self.m and self.m[o] != h and abs(frameid - self.last_occurrence[o]) <= self.max_switch_time:
                    self.num_switches += 1
                else:
                    self.num_matches += 1
                matched.append((o, dists[i, j]))
                omask[i] = hmask[j] = True
                self.m[o] = h
        for o, d in matched:
            self.obj_total[o] = self.obj_total.get(o, 0) + 1
            self.obj_tracked[o] = self.obj_tracked.get(o, 0) + 1
            self.distances.append(float(d))
        for i, o in enumerate(oids):
            if not omask[i]:
                self.num_misses += 1
                self.obj_total[o] = self.obj_total.get(o, 0) + 1
        self.num_false_positives += int((~hmask).sum())
        for o in oids:
            self.last_occurrence[o] = frameid

    def _id_measures(self):
        """`id_global_assignment`, `idfp`, `idfn`: the min-cost one-to-one mapping of objects to hypotheses."""
        ocs = {o: len(s) for o, s in self.obj_frames.items()}
        hcs = {h: len(s) for h, s in self.hyp_frames.items()}
        oids, hids = sorted(ocs), sorted(hcs)
        oi, hi = {o: i for i, o in enumerate(oids)}, {h: i for i, h in enumerate(hids)}
        no, nh = len(oids), len(hids)
        fp, fn = np.zeros((no + nh, no + nh)), np.zeros((no + nh, no + nh))
        fp[no:, :nh] = np.nan
        fn[:no, nh:] = np.nan
        for o, oc in ocs.items():
            fn[oi[o], :nh] = oc
            fn[oi[o], nh + oi[o]] = oc
        for h, hc in hcs.items():
            fp[:no, hi[h]] = hc
            fp[hi[h] + no, hi[h]] = hc
        for (o, h), ex in self.pair_raw.items():
            fp[oi[o], hi[h]] -= ex
            fn[oi[o], hi[h]] -= ex
        rids, cids = _assign(fp + fn)
        return float(fp[rids, cids].sum()), float(fn[rids, cids].sum())

    def metrics(self):
        """The metrics of `motmetrics.metrics` that the protocols read, by their names."""
        r = {"num_frames": len(self.frames), "num_matches": self.num_matches, "num_switches": self.num_switches,
             "num_false_positives": self.num_false_positives, "num_misses": self.num_misses}
        r["num_detections"] = det = self.num_matches + self.num_switches
        r["num_objects"] = nobj = det + self.num_misses
        r["num_predictions"] = npred = det + self.num_false_positives
        r["num_unique_objects"] = len(self.obj_total)
        ratios = [self.obj_tracked.get(o, 0) / t for o, t in self.obj_total.items()]
        r["mostly_tracked"] = sum(1 for v in ratios if v >= 0.8)
        r["partially_tracked"] = sum(1 for v in ratios if 0.2 <= v < 0.8)
        r["mostly_lost"] = sum(1 for v in ratios if v < 0.2)
        r["mota"] = 1.0 - _quiet_divide(self.num_misses + self.num_switches + self.num_false_positives, nobj)
        r["motp"] = 0.0 if det == 0 else _quiet_divide(float(np.sum(np.asarray(self.distances, dtype=np.float64))), det)
        r["precision"] = _quiet_divide(det, self.num_false_positives + det)
        r["recall"] = _quiet_divide(det, nobj)
        idfp, idfn = self._id_measures()
        idtp = nobj - idfn
        r["idp"] = _quiet_divide(idtp, idtp + idfp)
        r["idr"] = _quiet_divide(idtp, idtp + idfn)
        r["idf1"] = _quiet_divide(2 * idtp, nobj + npred)
        return r


# ------------------------------------------------------------------------------------------ readers
def load_source(path, pattern):
    """Directory or .zip -> {"<a>_<b>_<c>": bytes} of the entries whose base name matches `pattern`."""
    rx = re.compile(pattern)
    out = {}
    if os.path.isdir(path):
        for name in sorted(os.listdir(path)):
            m = rx.fullmatch(name)
            if m and os.path.isfile(os.path.join(path, name)):
                with open(os.path.join(path, name), "rb") as f:
                    out["_".join(m.groups())] = f.read()
    elif os.path.isfile(path):
        try:
            archive = zipfile.ZipFile(path, mode="r", allowZip64=True)
        except (zipfile.BadZipFile, OSError):
            raise ScoreError("%r is neither a directory nor a ZIP archive" % path)
        with archive:
            for name in archive.namelist():
                m = rx.fullmatch(os.path.basename(name))
                if m:
                    out["_".join(m.groups())] = archive.read(name)
    else:
        raise ScoreError("%r not found" % path)
    return out


def read_transcriptions(raw, what):
    """`"ID","text"` lines -> {ID (str): text}; later lines win, as in the protocol's `evaluate_method`."""
    out = {}
    for line in raw.decode("utf-8-sig", errors="replace").split("\n"):
        line = line.replace("\r", "").replace("\n", "")
        if line == "":
            continue
        m = _TXT_LINE.match(line)
        if m is None:
            raise ScoreError('%s: line %r is not "ID","Transcription"' % (what, line))
        out[m.group(1)] = m.group(2)
    return out


def read_frames(raw, what):
    """A protocol XML -> [(frame ID (str), [(object ID (str), Transcription or None, [x1, y1, .., x4, y4])])] in document
    order.  Coordinates are clamped with max(0, .); a duplicated object ID within a frame, a duplicated frame ID, fewer than
    four points and non-integer IDs or coordinates are errors."""
    try:
        root = ET.fromstring(raw)
    except ET.ParseError as e:
        raise ScoreError("%s: not well-formed XML (%s)" % (what, e))
    frames, seen_frames = [], set()
    for frame in root.iter("frame"):
        try:
            fid = frame.attrib["ID"]
            int(fid)
            if fid in seen_frames:
                raise ScoreError("%s: duplicated frame ID %s" % (what, fid))
            seen_frames.add(fid)
            objs, seen = [], set()
            for obj in frame.iter("object"):
                oid = obj.attrib["ID"]
                int(oid)
                if oid in seen:
                    raise ScoreError("%s: duplicated object ID in frame %s" % (what, fid))
                seen.add(oid)
                coords = []
                for pt in obj.iter("Point"):
                    coords.append(max(0, int(pt.attrib["x"])))
                    coords.append(max(0, int(pt.attrib["y"])))
                if len(coords) < 8:
                    raise ScoreError("%s: object %s of frame %s has fewer than four points" % (what, oid, fid))
                if max(coords[:8]) >= 2 ** 24:
                    raise ScoreError("%s: object %s of frame %s has a coordinate of 2^24 or more" % (what, oid, fid))
                objs.append((oid, obj.attrib.get("Transcription"), coords[:8]))
        except (KeyError, ValueError) as e:
            raise ScoreError("%s: missing or non-integer attribute (%s)" % (what, e))
        frames.append((fid, objs))
    return frames


# ------------------------------------------------------------------------------------------ one video, one method
def _csr(per_frame):
    off = np.zeros(len(per_frame) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(x) for x in per_frame])
    flat = [q for x in per_frame for q in x]
    return off, np.asarray(flat, dtype=np.int64).reshape(-1, 8)


def _split(counts, det, val, off):
    """The compacted pairs of one call -> per frame [(object index within the frame, detection index, value)]."""
    F = len(off) - 1
    out = [[] for _ in range(F)]
    gi = np.repeat(np.arange(len(counts)), counts)
    frame = np.searchsorted(off, gi, side="right") - 1
    for g, f, d, v in zip(gi.tolist(), frame.tolist(), det.tolist(), val.tolist()):
        out[f].append((g - int(off[f]), d, v))
    return out


_ZERO = {"MOTA": 0, "MOTAN": 0, "MOTP": 0, "IDF1": 0, "DE": 0, "MT": 0, "PT": 0, "ML": 0, "MA": 0, "SW": 0, "FP": 0, "MS": 0}
_ALIAS = {"mota": "MOTA", "num_matches": "MA", "num_switches": "SW", "num_false_positives": "FP", "num_misses": "MS",
          "num_detections": "DE", "num_objects": "OB", "num_predictions": "PR", "mostly_tracked": "MT",
          "partially_tracked": "PT", "mostly_lost": "ML", "num_unique_objects": "UO", "idf1": "IDF1"}


def score_video(gt_xml, det_xml, gt_txt=None, det_txt=None, e2e=False, threshold=0.5, pairs_fn=host_quad_pairs, name="video"):
    """`evaluate_method`'s loop body for one video -> its `per_sample` figures.  det_xml None: the video has no result."""
    gt_frames = read_frames(gt_xml, "ground truth of " + name)
    gt_text = read_transcriptions(gt_txt, "ground-truth text of " + name) if e2e else {}
    frame_index = {fid: k for k, (fid, _) in enumerate(gt_frames)}
    F = len(gt_frames)
    care = [[] for _ in range(F)]           # per frame: (ID, quad)
    dont = [[] for _ in range(F)]           # per frame: quads of the "don't care" objects
    for k, (fid, objs) in enumerate(gt_frames):
        for oid, text, quad in objs:
            if text is None:
                raise ScoreError("ground truth of %s: object %s of frame %s has no Transcription" % (name, oid, fid))
            if "#" in text or (e2e and oid not in gt_text):
                dont[k].append(quad)
            else:
                care[k].append((oid, quad))
    dets = [[] for _ in range(F)]
    det_text = {}
    if det_xml is not None:
        det_text = read_transcriptions(det_txt, "text of res_" + name) if e2e else {}
        for fid, objs in read_frames(det_xml, "res_" + name):
            if fid not in frame_index:
                raise ScoreError("res_%s: frame %s is not in the ground truth" % (name, fid))
            dets[frame_index[fid]] = [(oid, quad) for oid, _, quad in objs if not e2e or oid in det_text]
    # detections on "don't care" regions leave: overlap (intersection over the detection's area) above 0.5 with any of them
    det_off, det_quads = _csr([[q for _, q in x] for x in dets])
    dc_off, dc_quads = _csr(dont)
    dc_dets = 0
    if len(dc_quads) and len(det_quads):
        counts, di, _ = pairs_fn(dc_quads, det_quads, dc_off, det_off, np.zeros(len(dc_quads), dtype=np.int32),
                                 np.zeros(len(det_quads), dtype=np.int32), 1, DONT_CARE_OVERLAP)
        for k, hits in enumerate(_split(counts, di, np.zeros(len(di)), dc_off)):
            drop = set(d for _, d, _ in hits)
            dc_dets += len(drop)
            dets[k] = [x for j, x in enumerate(dets[k]) if j not in drop]
    sample = {"DC_GT": int(len(dc_quads)), "DC_DT": dc_dets}
    if sum(len(x) for x in dets) == 0:      # (motmetrics fails without a single detection: the protocol's special case)
        sample.update(_ZERO)
        return sample
    # distances: 1 - IoU where IoU > threshold between objects of equal key (tracking: one key; end to end: the transcription)
    det_off, det_quads = _csr([[q for _, q in x] for x in dets])
    gt_off, gt_quads = _csr([[q for _, q in x] for x in care])
    gt_key, det_key = np.zeros(len(gt_quads), dtype=np.int32), np.zeros(len(det_quads), dtype=np.int32)
    if e2e:
        codes = {}
        gt_key = np.asarray([codes.setdefault(_GT_TEXT_STRIP.sub("", gt_text[oid].upper()).upper(), len(codes))
                             for x in care for oid, _ in x], dtype=np.int32).reshape(-1)
        det_key = np.asarray([codes.setdefault(det_text[oid].upper(), len(codes)) for x in dets for oid, _ in x],
                             dtype=np.int32).reshape(-1)
    if len(gt_quads) and len(det_quads):
        counts, di, iou = pairs_fn(gt_quads, det_quads, gt_off, det_off, gt_key, det_key, 0, threshold)
        kept = _split(counts, di, iou, gt_off)
    else:
        kept = [[] for _ in range(F)]
    acc = MOTAccumulator()
    for k, (fid, _) in enumerate(gt_frames):
        acc.update([oid for oid, _ in care[k]], [oid for oid, _ in dets[k]], [(i, j, 1 - v) for i, j, v in kept[k]], int(fid))
    m = acc.metrics()
    for key, alias in _ALIAS.items():
        sample[alias] = m[key]
    for key in ("num_frames", "idp", "idr", "precision", "recall"):
        sample[key] = m[key]
    if det_xml is not None:
        sample["motp"] = 0 if math.isnan(m["motp"]) else m["motp"]
        sample["MOTAN"] = 0 if sample["PR"] == 0 or sample["OB"] == 0 else \
            0.5 * (sample["FP"] + sample["SW"]) / sample["PR"] + 0.5 * sample["MS"] / sample["OB"]
    else:
        sample["motp"] = 0
        sample["MOTAN"] = 0
    sample["MOTP"] = 0 if sample["DE"] == 0 else 1 - float(sample["motp"])     # "motp as MOTchallenge"
    return sample


def score_method(gt_path, res_path, e2e=False, threshold=0.5, host_iou=False):
    """`evaluate_method`: -> {"method": {...}, "per_sample": {video: {...}}}."""
    gt = load_source(gt_path, GT_XML)
    subm = load_source(res_path, DET_XML)
    if not gt:
        raise ScoreError("no Video_<a>_<b>_<c>_GT.xml in %r" % gt_path)
    gt_txt = load_source(gt_path, GT_TXT) if e2e else {}
    subm_txt = load_source(res_path, DET_TXT) if e2e else {}
    for k in subm:
        if k not in gt:
            raise ScoreError("the video ID %s is not present in GT" % k)
        if e2e and k not in subm_txt:
            raise ScoreError("the text file for the video ID %s is not present in the detection" % k)
    pairs_fn = host_quad_pairs if host_iou else device_quad_pairs
    per_sample = {}
    for k in gt:
        if e2e and k not in gt_txt:
            raise ScoreError("the text file for the video ID %s is not present in GT" % k)
        per_sample[k] = score_video(gt[k], subm.get(k), gt_txt.get(k), subm_txt.get(k), e2e, threshold, pairs_fn,
                                    name="Video_" + k)
    n = len(gt)
    method = {key: sum(s[key] for s in per_sample.values()) / n for key in ("MOTP", "MOTA", "IDF1", "MOTAN")}
    method.update({key: sum(s[key] for s in per_sample.values()) for key in ("MT", "PT", "ML")})
    return {"method": method, "per_sample": per_sample}


# ------------------------------------------------------------------------------------------ command line
def build_parser():
    p = argparse.ArgumentParser(prog="python -m gomatching_amd.score",
                                description="MOTA / MOTP / IDF1 of result files against DSText-style ground truth")
    p.add_argument("--gt", required=True, help="directory or .zip with Video_<a>_<b>_<c>_GT.xml (and _GT.txt for --e2e)")
    p.add_argument("--results", required=True, help="directory or .zip with res_Video_<a>_<b>_<c>.xml (and .txt for --e2e)")
    p.add_argument("--e2e", action="store_true", help="end-to-end protocol: a pair also needs equal transcriptions")
    p.add_argument("--threshold", type=float, default=0.5, help="a pair counts when its IoU is above this (default 0.5)")
    p.add_argument("--host-iou", action="store_true", help="polygon measure in numpy float64 instead of the HIP kernels")
    p.add_argument("--output", default="scores.json", help="where the figures are written (default scores.json)")
    p.add_argument("--protocol", choices=("dstext", "bovtext", "artvideo"), default="dstext",
                   help="dstext: the XML protocol (default); bovtext / artvideo: the json protocols (score_json.py), where --gt "
                        "holds GT/<class>/<name>.json or GT/<name>.json and --results the jsons/<name>.json of the eval command")
    p.add_argument("--curve", action="store_true", help="artvideo only: only evaluate curved text (Straight objects are ignored)")
    p.add_argument("--det", action="store_true", help="dstext only: the detection protocol, precision / recall / hmean per frame "
                                                      "(score_det.py)")
    p.add_argument("--per-frame", action="store_true", help="--det only: also write per_sample, one entry per frame")
    return p


def main(argv=None):
    args = build_parser().parse_args(argv)
    if args.det or args.per_frame:
        return _main_det(args)
    if args.protocol != "dstext":
        from . import score_json
        return score_json.main(args)
    try:
        if args.curve:
            raise ScoreError("--curve belongs to --protocol artvideo")
        if not (0.0 < args.threshold < 1.0):
            raise ScoreError("--threshold must lie strictly between 0 and 1")
        res = score_method(args.gt, args.results, args.e2e, args.threshold, args.host_iou)
        with open(args.output, "w") as f:
            json.dump(res, f, indent=2, sort_keys=True)
    except ScoreError as e:
        sys.stderr.write("error: %s\n" % e)
        return 2
    except OSError as e:
        sys.stderr.write("error: %s\n" % e)
        return 2
    m = res["method"]
    print("method: MOTA %.4f  MOTP %.4f  IDF1 %.4f  MOTAN %.4f  MT %d  PT %d  ML %d" % (
        m["MOTA"], m["MOTP"], m["IDF1"], m["MOTAN"], m["MT"], m["PT"], m["ML"]))
    for k, s in res["per_sample"].items():
        print("Video_%s: MOTA %.4f  MOTP %.4f  IDF1 %.4f  FP %d  MS %d  SW %d" % (
            k, s["MOTA"], s["MOTP"], s["IDF1"], s["FP"], s["MS"], s["SW"]))
    return 0


def _main_det(args):
    from . import score_det
    try:
        if not args.det:
            raise ScoreError("--per-frame belongs to --det")
        if args.e2e or args.curve or args.protocol != "dstext":
            raise ScoreError("--det is the DSText detection protocol: it does not combine with --e2e, --curve or --protocol %s"
                             % args.protocol)
        if not (0.0 < args.threshold < 1.0):
            raise ScoreError("--threshold must lie strictly between 0 and 1")
        res = score_det.score_method(args.gt, args.results, args.threshold, args.host_iou, args.per_frame)
        with open(args.output, "w") as f:
            json.dump(res, f, indent=2, sort_keys=True)
    except (ScoreError, OSError) as e:
        sys.stderr.write("error: %s\n" % e)
        return 2
    score_det.print_scores(res)
    return 0


def host_mask_pairs(*args, **kwargs):
    """The mask measure of the json protocols on the host: `score_json.host_mask_pairs`, where it lives."""
    from . import score_json
    return score_json.host_mask_pairs(*args, **kwargs)


def device_mask_pairs(*args, **kwargs):
    """The mask measure of the json protocols through the kernels: `score_json.device_mask_pairs`."""
    from . import score_json
    return score_json.device_mask_pairs(*args, **kwargs)


if __name__ == "__main__":
    sys.exit(main())
