"""Score result jsons: the BOVText and ArTVideo protocols behind `python -m gomatching_amd.score --protocol ...`.

    python -m gomatching_amd.score --protocol bovtext  --gt GT --results OUT/jsons [--e2e] [--threshold 0.5] [--host-iou]
    python -m gomatching_amd.score --protocol artvideo --gt GT --results OUT/jsons [--e2e] [--curve] [--threshold 0.5] [--host-iou]

The figures are those of the reference's tools/Evaluation_Protocol_BOV_Text/{Task1_VideoTextTracking,Task2_VideoTextSpotting}/
evaluation.py and tools/Evaluation_Protocol_ArtVideo/{eval_trk,eval_e2e}.py (`--e2e` picks the second of each), which need
shapely, Levenshtein, cv2, pycocotools, pandas and a vendored motmetrics; here:

  * BOVText (GT/<class dir>/<name>.json against RES/<name>.json, {frame: [{"points": [8], "ID", "transcription" |
    "ID_transcription"}]}): the convex-hull quad IoU of `score.host_quad_pairs` / `ops.quad_pairs`, points truncated to int32.
  * ArTVideo (GT/<name>.json with COCO RLE masks against RES/<name>.json): the IoU of two pixel masks.  A result's mask is its
    "segmentation" (a list: the contours of one fillPoly call; a dict: an RLE), else the polygon of "points".  A mask is a
    box of rows [y0, y1) and of 32-pixel word columns [wx0, wx1) in absolute alignment plus its bit rows; all masks of a call
    share one uint32 buffer behind CSR word offsets.  `device_mask_pairs` fills them and counts the intersections in
    csrc/mask_pairs.hip (`ops.mask_fill_polygons`, `ops.mask_fill_rle`, `ops.mask_pairs`); `--host-iou` does the same integer
    arithmetic in numpy on the same representation (`host_mask_pairs`).  Both give the same bytes.
  * per frame as the scripts' `eval_frame`: ground truth splits into counted and ignored objects ("###" / "#1" transcriptions;
    with --curve the `Straight` objects), a hypothesis whose IoU with an ignored object is STRICTLY above the ignore
    threshold (BOVText 0.5, ArTVideo --threshold) leaves, a pair stays when its IoU is AT LEAST --threshold (the kernels keep
    values strictly above: the call is made with numpy.nextafter(t, 0.0), exact for doubles) and, with --e2e, when
    `cal_similarity` of the two transcriptions (the protocol's regular expression, then lower()) is at least 0.9.
    THE DISTANCE HANDED TO THE ACCUMULATOR IS THE IoU ITSELF, not 1 - IoU, as the scripts pass it: MOTP is a mean IoU and
    the assignment prefers the smaller IoU.  Frame ids are the `auto_id` numbers 0, 1, ..
  * every video's figures come from `score.MOTAccumulator.metrics()`, the OVERALL row from `overall()`, which restates
    `MetricsHost.compute_overall` (sums of the additive counts, the ratios from the sums, motp weighted by num_detections);
    pinned by tests/golden/score_overall.json, which the reference's vendored motmetrics produced.

UNPINNED (libraries that are not available to the tests; held to tests/mask_statement.py and tests/score_statement.py):
cv2.fillPoly (the rasterisation rule is the one in include/gomatching_hip.h; a difference could only sit in boundary pixels,
and OpenCV clips a line to the image before stepping it, which can move pixels of an edge whose end point lies outside the
image), pycocotools (RLE strings as `rleFrString` reads them), Levenshtein (plain two-row edit distance), shapely (hull IoU).

Deliberate differences: videos are keyed by base name (the BOVText scripts rebuild a class directory from the name, which
fails for names of other shapes); a video without a result file scores as one without hypotheses (the scripts stop there);
a frame named by the result but not by the ground truth is ignored as in the scripts; coordinates beyond +-2^20 (masks) or
2^24 (quads) and masks whose size is not the video's are errors.  Not built: XSD validation, the per-frame event dump and
the Excel summary.
"""
import json
import os
import sys
import zipfile

import numpy as np

from .score import MOTAccumulator, ScoreError, _GT_TEXT_STRIP, _quiet_divide, _split, device_quad_pairs, host_quad_pairs

S = 16                                   # fraction bits of a crossing position
IGNORE_IOU_BOVTEXT = 0.5
MAX_COORD = 1 << 20
MAX_WORDS = (256 << 20) // 4             # mask words of one device call
SKIP_NAME = "Cls1_Livestreaming_video40"
ADDITIVE = ("num_frames", "num_matches", "num_switches", "num_false_positives", "num_misses", "num_detections", "num_objects",
            "num_predictions", "num_unique_objects", "mostly_tracked", "partially_tracked", "mostly_lost", "idfp", "idfn", "idtp")


# ------------------------------------------------------------------------------------------ strings
def rle_from_string(s):
    """The compressed `counts` of a COCO RLE -> run lengths: 5 payload bits per character (the character minus 48), bit 0x20
    = more, sign extension when the last chunk has 0x10 set, and from the fourth count on counts[i-2] is added."""
    counts = []
    p, n = 0, len(s)
    while p < n:
        x, k, more = 0, 0, True
        while more:
            if p >= n:
                raise ScoreError("truncated RLE string")
            c = ord(s[p]) - 48
            if c < 0 or c > 63:
                raise ScoreError("bad character in an RLE string")
            x |= (c & 0x1f) << (5 * k)
            more = bool(c & 0x20)
            p += 1
            k += 1
            if not more and (c & 0x10):
                x |= -1 << (5 * k)
        if len(counts) > 2:
            x += counts[-2]
        counts.append(x)
    return counts


def levenshtein(a, b):
    """Edit distance, two-row dynamic programme."""
    if len(a) < len(b):
        a, b = b, a
    prev = list(range(len(b) + 1))
    for i, ca in enumerate(a, 1):
        cur = [i]
        for j, cb in enumerate(b, 1):
            cur.append(min(prev[j] + 1, cur[j - 1] + 1, prev[j - 1] + (ca != cb)))
        prev = cur
    return prev[len(b)]


def cal_similarity(a, b, memo=None):
    """The protocols' `cal_similarity`: 1.0 for two empty strings, 0.95 at edit distance 1, else 1 - distance / max(len)."""
    if a == "" and b == "":
        return 1.0
    if memo is None:
        dist = levenshtein(a, b)
    else:
        dist = memo.get((a, b))
        if dist is None:
            dist = memo[(a, b)] = levenshtein(a, b)
    if dist == 1:
        return 0.95
    return 1 - dist / max(len(a), len(b))


def clean_text(s):
    return _GT_TEXT_STRIP.sub("", str(s)).lower()


# ------------------------------------------------------------------------------------------ mask sets
class MaskSet:
    """N masks of one H x W image size, described but not rasterised: per mask either contours (CSR `mcoff` into contours,
    `coff` into `points` int32 [P,2]) or runs (CSR `roff` into `ends`, the cumulative run ends of a COCO RLE), its box
    `boxes` int32 [N,4] = (y0, y1, wx0, wx1) and the CSR word offsets `woff` int64 [N+1]."""

    def __init__(self, specs, H, W):
        """specs: per mask ("poly", [int array [n,2], ...]) or ("rle", run lengths)."""
        H, W = int(H), int(W)
        if H < 1 or W < 1 or H * W > 2 ** 31 - 1:
            raise ScoreError("image size %d x %d is not supported" % (H, W))
        self.H, self.W, self.N = H, W, len(specs)
        N = self.N
        boxes = np.zeros((N, 4), dtype=np.int32)
        mcoff, roff = np.zeros(N + 1, dtype=np.int64), np.zeros(N + 1, dtype=np.int64)
        points, clen, ends = [], [], []
        for k, (kind, data) in enumerate(specs):
            nc = nr = 0
            if kind == "poly":
                cs = [np.asarray(c, dtype=np.int64).reshape(-1, 2) for c in data]
                cs = [c for c in cs if len(c)]
                if cs:
                    allp = np.concatenate(cs)
                    if np.abs(allp).max() > MAX_COORD:
                        raise ScoreError("a polygon coordinate beyond +-2^20")
                    x0, y0 = max(int(allp[:, 0].min()), 0), max(int(allp[:, 1].min()), 0)
                    x1, y1 = min(int(allp[:, 0].max()), W - 1), min(int(allp[:, 1].max()), H - 1)
                    if x0 <= x1 and y0 <= y1:
                        boxes[k] = (y0, y1 + 1, x0 >> 5, (x1 >> 5) + 1)
                    points.extend(cs)
                    clen.extend(len(c) for c in cs)
                    nc = len(cs)
            elif kind == "rle":
                c = np.asarray(data, dtype=np.int64).reshape(-1)
                if len(c) == 0 or (c < 0).any() or int(c.sum()) != H * W:
                    raise ScoreError("the runs of an RLE mask do not add up to its %d x %d image" % (H, W))
                e = np.cumsum(c)
                start, stop = e[0:-1:2], e[1::2]
                live = stop > start
                start, stop = start[live], stop[live]
                if len(start):
                    xs, xe = start // H, (stop - 1) // H
                    one = xs == xe
                    ys, ye = np.where(one, start % H, 0), np.where(one, (stop - 1) % H, H - 1)
                    boxes[k] = (int(ys.min()), int(ye.max()) + 1, int(xs.min()) >> 5, (int(xe.max()) >> 5) + 1)
                ends.append(e)
                nr = len(e)
            else:
                raise ValueError(kind)
            mcoff[k + 1], roff[k + 1] = mcoff[k] + nc, roff[k] + nr
        self.boxes, self.mcoff, self.roff = boxes, mcoff, roff
        self.points = np.concatenate(points).astype(np.int32) if points else np.zeros((0, 2), dtype=np.int32)
        self.coff = np.concatenate([[0], np.cumsum(clen)]).astype(np.int64) if clen else np.zeros(1, dtype=np.int64)
        self.ends = np.concatenate(ends).astype(np.int32) if ends else np.zeros(0, dtype=np.int32)
        b = boxes.astype(np.int64)
        self.woff = np.zeros(N + 1, dtype=np.int64)
        self.woff[1:] = np.cumsum((b[:, 1] - b[:, 0]) * (b[:, 3] - b[:, 2]))

    def part(self, m0, m1):
        """Masks [m0, m1) as a set of their own (the CSR arrays re-based)."""
        out = MaskSet.__new__(MaskSet)
        out.H, out.W, out.N = self.H, self.W, m1 - m0
        out.boxes = self.boxes[m0:m1]
        c0, c1 = int(self.mcoff[m0]), int(self.mcoff[m1])
        out.mcoff = self.mcoff[m0:m1 + 1] - c0
        out.coff = self.coff[c0:c1 + 1] - self.coff[c0]
        out.points = self.points[int(self.coff[c0]):int(self.coff[c1])]
        r0, r1 = int(self.roff[m0]), int(self.roff[m1])
        out.roff = self.roff[m0:m1 + 1] - r0
        out.ends = self.ends[r0:r1]
        out.woff = self.woff[m0:m1 + 1] - self.woff[m0]
        return out

    def contours(self, k):
        return [self.points[int(self.coff[c]):int(self.coff[c + 1])] for c in range(int(self.mcoff[k]), int(self.mcoff[k + 1]))]


if hasattr(np, "bitwise_count"):
    def _popcount(a):
        return int(np.bitwise_count(a).sum(dtype=np.int64))
else:
    _POP8 = np.array([bin(i).count("1") for i in range(256)], dtype=np.int64)

    def _popcount(a):
        return int(_POP8[np.ascontiguousarray(a).view(np.uint8)].sum())


def _pack(img):
    """bool [R, 32 * NW] -> uint32 [R, NW], bit b of word w = pixel 32 * w + b."""
    return np.packbits(img, axis=1, bitorder="little").view("<u4").astype(np.uint32)


def fill_polygon_rows(contours, box, W, fill=True):
    """The rasterisation rule of include/gomatching_hip.h for one mask in closed form, as fill_polygon_kernel of
    csrc/mask_pairs.hip evaluates it: -> uint32 [y1 - y0, wx1 - wx0].
    Fill: a crossing c toggles the pixels x >= (c >> S) + 1 and sets pixel c >> S when its fraction is zero (the sort-free
    form).  Boundary: step k of a line sits at the minor offset (2 m k + M - 1) // (2 M), so an x-major edge covers on row j
    the steps ceil((2 M j - M + 1) / (2 m)) .. floor((2 M j + M) / (2 m)) and a y-major edge one pixel per row.
    fill=False leaves Fill out: Boundary alone, the outline `show` draws (outline_polygon_kernel of csrc/overlay.hip)."""
    y0, y1, wx0, wx1 = (int(v) for v in box)
    R, NW = y1 - y0, wx1 - wx0
    if R <= 0 or NW <= 0:
        return np.zeros((max(R, 0), max(NW, 0)), dtype=np.uint32)
    X0, WB = 32 * wx0, 32 * NW
    img = np.zeros((R, WB), dtype=bool)
    ys = np.arange(y0, y1, dtype=np.int64)[None, :]
    for c in contours:
        c = np.asarray(c, dtype=np.int64).reshape(-1, 2)
        if len(c) == 0:
            continue
        a = np.roll(c, 1, 0)
        xa, ya, xb, yb = a[:, 0], a[:, 1], c[:, 0], c[:, 1]
        # ---- fill
        top = ya < yb
        xt, yt, xo, yo = np.where(top, xa, xb), np.where(top, ya, yb), np.where(top, xb, xa), np.where(top, yb, ya)
        dy = yo - yt
        num = (xo - xt) << S
        dxq = np.sign(num) * (np.abs(num) // np.maximum(dy, 1))   # C division: toward zero
        act = (dy > 0)[:, None] & (yt[:, None] <= ys) & (ys < yo[:, None])
        pos = (xt[:, None] << S) + (ys - yt[:, None]) * dxq[:, None]
        e, r = np.nonzero(act) if fill else ((), ())
        if len(e):
            par = np.zeros((R, WB + 1), dtype=np.int64)
            np.add.at(par, (r, np.clip((pos[e, r] >> S) + 1 - X0, 0, WB)), 1)
            img |= (np.cumsum(par, axis=1)[:, :WB] & 1).astype(bool)
            exact = (pos[e, r] & ((1 << S) - 1)) == 0
            px = (pos[e, r] >> S) - X0
            ok = exact & (px >= 0) & (px < WB)
            img[r[ok], px[ok]] = True
        # ---- boundary: every edge left to right
        sw = xb < xa
        x0, yy0, x1, yy1 = np.where(sw, xb, xa), np.where(sw, yb, ya), np.where(sw, xa, xb), np.where(sw, ya, yb)
        dx, dyl = x1 - x0, yy1 - yy0
        ady, sy = np.abs(dyl), np.sign(dyl)
        M, m = np.maximum(dx, ady), np.minimum(dx, ady)
        ymaj = ady > dx
        j = (ys - yy0[:, None]) * np.where(sy == 0, 1, sy)[:, None]            # minor (x-major) or major (y-major) step of the row
        Mc, mc = M[:, None], m[:, None]
        # x-major
        on = ~ymaj[:, None] & (j >= 0) & (j <= mc)
        m1 = np.maximum(mc, 1)
        klo = np.where(mc == 0, 0, np.maximum(-((-(2 * Mc * j - Mc + 1)) // (2 * m1)), 0))
        khi = np.where(mc == 0, Mc, np.minimum((2 * Mc * j + Mc) // (2 * m1), Mc))
        lo, hi = x0[:, None] + klo - X0, x0[:, None] + khi - X0
        on &= (lo <= hi) & (hi >= 0) & (lo < WB)
        e, r = np.nonzero(on)
        if len(e):
            run = np.zeros((R, WB + 1), dtype=np.int64)
            np.add.at(run, (r, np.clip(lo[e, r], 0, WB)), 1)
            np.add.at(run, (r, np.clip(hi[e, r] + 1, 0, WB)), -1)
            img |= np.cumsum(run, axis=1)[:, :WB] > 0
        # y-major
        on = ymaj[:, None] & (j >= 0) & (j <= Mc)
        px = x0[:, None] + (2 * mc * j + Mc - 1) // (2 * np.maximum(Mc, 1)) - X0
        on &= (px >= 0) & (px < WB)
        e, r = np.nonzero(on)
        img[r, px[e, r]] = True
    img[:, max(W - X0, 0):] = False
    return _pack(img)


def fill_rle_rows(ends, box, H, W):
    """The bits of a COCO RLE inside a box: pixel (x, y) is set when an odd number of run ends lie at or below x * H + y."""
    y0, y1, wx0, wx1 = (int(v) for v in box)
    R, NW = y1 - y0, wx1 - wx0
    if R <= 0 or NW <= 0:
        return np.zeros((max(R, 0), max(NW, 0)), dtype=np.uint32)
    xs = np.arange(32 * wx0, 32 * wx1, dtype=np.int64)[None, :]
    p = xs * H + np.arange(y0, y1, dtype=np.int64)[:, None]
    img = (np.searchsorted(np.asarray(ends, dtype=np.int64), p, side="right") & 1).astype(bool) & (xs < W)
    return _pack(img)


def host_fill(ms):
    """MaskSet -> (list of uint32 [rows, words] per mask, areas int64 [N])."""
    rows, area = [], np.zeros(ms.N, dtype=np.int64)
    for k in range(ms.N):
        if ms.roff[k + 1] > ms.roff[k]:
            w = fill_rle_rows(ms.ends[int(ms.roff[k]):int(ms.roff[k + 1])], ms.boxes[k], ms.H, ms.W)
        else:
            w = fill_polygon_rows(ms.contours(k), ms.boxes[k], ms.W)
        rows.append(w)
        area[k] = _popcount(w)
    return rows, area


def host_mask_pairs(gt_set, det_set, gt_off, det_off, gt_key, det_key, threshold):
    """`ops.mask_pairs` on the host: -> (counts int32 [G], det int32 [K], value fp64 [K]).  The same integer counts, the
    same single fp64 division: bitwise the kernels' output."""
    G = gt_set.N
    counts = np.zeros(G, dtype=np.int32)
    det, val = [], []
    grows, garea = host_fill(gt_set)
    drows, darea = host_fill(det_set)
    gb, db = gt_set.boxes.astype(np.int64), det_set.boxes.astype(np.int64)
    gt_key, det_key = np.asarray(gt_key), np.asarray(det_key)
    for f in range(len(gt_off) - 1):
        g0, g1, d0, d1 = int(gt_off[f]), int(gt_off[f + 1]), int(det_off[f]), int(det_off[f + 1])
        if g1 == g0 or d1 == d0:
            continue
        A, B = gb[g0:g1, None, :], db[None, d0:d1, :]
        ya, yb = np.maximum(A[..., 0], B[..., 0]), np.minimum(A[..., 1], B[..., 1])
        xa, xb = np.maximum(A[..., 2], B[..., 2]), np.minimum(A[..., 3], B[..., 3])
        meet = (ya < yb) & (xa < xb) & (gt_key[g0:g1, None] == det_key[None, d0:d1])
        for a, b in zip(*np.nonzero(meet)):                       # ground truth ascending, then detection ascending
            g, d = g0 + int(a), d0 + int(b)
            y_0, y_1, x_0, x_1 = int(ya[a, b]), int(yb[a, b]), int(xa[a, b]), int(xb[a, b])
            wg = grows[g][y_0 - gb[g, 0]:y_1 - gb[g, 0], x_0 - gb[g, 2]:x_1 - gb[g, 2]]
            wd = drows[d][y_0 - db[d, 0]:y_1 - db[d, 0], x_0 - db[d, 2]:x_1 - db[d, 2]]
            inter = _popcount(wg & wd)
            if inter < 1:
                continue
            v = float(inter) / float(int(garea[g]) + int(darea[d]) - inter)
            if v > threshold:
                counts[g] += 1
                det.append(int(b))
                val.append(v)
    return counts, np.asarray(det, dtype=np.int32), np.asarray(val, dtype=np.float64)


def _frame_chunks(gt_set, det_set, gt_off, det_off, max_words):
    """Frame ranges [f0, f1) whose masks need at most `max_words` words (a single frame beyond it goes alone)."""
    F = len(gt_off) - 1
    words = (gt_set.woff[gt_off[1:]] - gt_set.woff[gt_off[:-1]]) + (det_set.woff[det_off[1:]] - det_set.woff[det_off[:-1]])
    out, f0, acc = [], 0, 0
    for f in range(F):
        if f > f0 and acc + int(words[f]) > max_words:
            out.append((f0, f))
            f0, acc = f, 0
        acc += int(words[f])
    out.append((f0, F))
    return out


def device_fill(ms, dev):
    """MaskSet -> (words uint32-as-int32 [nwords], area int32 [N], boxes, woff) on the device: one upload and one launch per
    kind of mask."""
    import torch
    from . import ops

    def up(a, dtype):
        return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(dev)
    nwords = int(ms.woff[-1])
    boxes, woff = up(ms.boxes, np.int32), up(ms.woff, np.int64)
    words = torch.empty((nwords,), dtype=torch.int32, device=dev)
    area = torch.zeros((ms.N,), dtype=torch.int32, device=dev)
    is_rle = ms.roff[1:] > ms.roff[:-1]
    n_rle = int(is_rle.sum())
    if n_rle:
        sel = None if n_rle == ms.N else up(np.nonzero(is_rle)[0], np.int32)
        ops.mask_fill_rle(up(ms.ends, np.int32), up(ms.roff, np.int32), boxes, woff, ms.H, ms.W, words, area, sel=sel)
    if n_rle < ms.N:
        sel = None if n_rle == 0 else up(np.nonzero(~is_rle)[0], np.int32)
        ops.mask_fill_polygons(up(ms.points, np.int32), up(ms.coff, np.int32), up(ms.mcoff, np.int32), boxes, woff, ms.H, ms.W,
                               words, area, sel=sel)
    return words, area, boxes, woff


def device_mask_pairs(gt_set, det_set, gt_off, det_off, gt_key, det_key, threshold, max_words=MAX_WORDS):
    """`host_mask_pairs` through the kernels: per chunk of frames (at most 256 MiB of mask words) one upload, the fill
    launches, the count and the emit launch, one copy back."""
    import torch
    from . import ops
    if not torch.cuda.is_available():
        raise ScoreError("no GPU: the mask measure runs in csrc/mask_pairs.hip (use --host-iou for the numpy path)")
    dev = torch.device("cuda", torch.cuda.current_device())
    gt_off, det_off = np.asarray(gt_off, dtype=np.int64), np.asarray(det_off, dtype=np.int64)
    gt_key, det_key = np.asarray(gt_key, dtype=np.int32), np.asarray(det_key, dtype=np.int32)
    counts, det, val = [], [], []
    for f0, f1 in _frame_chunks(gt_set, det_set, gt_off, det_off, max_words):
        g0, g1, d0, d1 = int(gt_off[f0]), int(gt_off[f1]), int(det_off[f0]), int(det_off[f1])
        if g1 == g0:
            continue
        goff, doff = gt_off[f0:f1 + 1] - g0, det_off[f0:f1 + 1] - d0
        pairs = int(((goff[1:] - goff[:-1]) * (doff[1:] - doff[:-1])).sum())
        if pairs > 2 ** 31 - 1:
            raise ScoreError("more than 2^31 - 1 (ground truth, detection) pairs in one call are not supported")
        gw, ga, gbx, gwo = device_fill(gt_set.part(g0, g1), dev)
        dw, da, dbx, dwo = device_fill(det_set.part(d0, d1), dev)

        def up(a):
            return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev)
        c, d, v = ops.mask_pairs(gw, gbx, gwo, ga, dw, dbx, dwo, da, up(goff), up(doff), up(gt_key[g0:g1]), up(det_key[d0:d1]),
                                 threshold, pairs=pairs)
        counts.append(c.cpu().numpy())
        det.append(d.cpu().numpy())
        val.append(v.cpu().numpy())
    if not counts:
        return np.zeros(gt_set.N, dtype=np.int32), np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.float64)
    return np.concatenate(counts), np.concatenate(det), np.concatenate(val)


# ------------------------------------------------------------------------------------------ readers
def load_jsons(path, depth):
    """Directory or .zip -> {base name without .json: bytes}.  depth 0: the entries of the directory itself; depth 1: those of
    its sub-directories (BOVText's class directories).  In an archive every .json entry counts, by base name."""
    out = {}

    def wanted(name):
        return name.endswith(".json") and ".ipynb_checkpoints" not in name and SKIP_NAME not in name
    if os.path.isdir(path):
        dirs = [path] if depth == 0 else [os.path.join(path, d) for d in sorted(os.listdir(path))
                                          if d != ".ipynb_checkpoints" and os.path.isdir(os.path.join(path, d))]
        for d in dirs:
            for name in sorted(os.listdir(d)):
                if wanted(name) and os.path.isfile(os.path.join(d, name)):
                    with open(os.path.join(d, name), "rb") as f:
                        out[name[:-5]] = f.read()
    elif os.path.isfile(path):
        try:
            archive = zipfile.ZipFile(path, mode="r", allowZip64=True)
        except (zipfile.BadZipFile, OSError):
            raise ScoreError("%r is neither a directory nor a ZIP archive" % path)
        with archive:
            for name in sorted(archive.namelist()):
                if wanted(name) and not name.endswith("/"):
                    out[os.path.basename(name)[:-5]] = archive.read(name)
    else:
        raise ScoreError("%r not found" % path)
    return out


def _parse(raw, what, kind):
    try:
        doc = json.loads(raw.decode("utf-8-sig"))
    except (ValueError, UnicodeDecodeError) as e:
        raise ScoreError("%s: not valid JSON (%s)" % (what, e))
    if not isinstance(doc, kind):
        raise ScoreError("%s: the top level is not a JSON %s" % (what, "object" if kind is dict else "array"))
    return doc


def _ints(values, what, limit):
    """Numbers -> Python ints truncated toward zero (the scripts' astype(np.int32))."""
    try:
        out = [int(float(v)) for v in values]
    except (TypeError, ValueError, OverflowError):
        raise ScoreError("%s: coordinates must be numbers" % what)
    if out and max(abs(v) for v in out) >= limit:
        raise ScoreError("%s: a coordinate of %d or more" % (what, limit))
    return out


def _quad(obj, what):
    pts = obj.get("points") if isinstance(obj, dict) else None
    if not isinstance(pts, list) or len(pts) != 8:
        raise ScoreError("%s: \"points\" must hold 8 numbers" % what)
    return _ints(pts, what, 1 << 24)


def _id(obj, key, what):
    try:
        return int(obj[key])
    except (KeyError, TypeError, ValueError):
        raise ScoreError("%s: missing or non-integer %r" % (what, key))


def _result_frames(raw, what):
    doc = _parse(raw, what, dict) if raw is not None else {}
    for k, v in doc.items():
        if not isinstance(v, list):
            raise ScoreError("%s: frame %s is not a list of objects" % (what, k))
    return doc


def _result_mask(obj, what):
    """A result object's mask: ("poly", contours) or ("rle", run lengths with the RLE's size)."""
    if not isinstance(obj, dict):
        raise ScoreError("%s: an object is not a JSON object" % what)
    seg = obj.get("segmentation")
    if isinstance(seg, dict):
        return _rle_spec(seg, what)
    if isinstance(seg, list):
        contours = []
        for c in seg:
            if not isinstance(c, list) or any(not isinstance(p, list) or len(p) != 2 for p in c):
                raise ScoreError("%s: \"segmentation\" must be a list of [[x, y], ...] contours" % what)
            contours.append(np.asarray(_ints([v for p in c for v in p], what, MAX_COORD + 1), dtype=np.int64).reshape(-1, 2))
        return ("poly", contours, None)
    if seg is not None:
        raise ScoreError("%s: \"segmentation\" is neither contours nor an RLE" % what)
    pts = obj.get("points")
    if not isinstance(pts, list) or len(pts) % 2:
        raise ScoreError("%s: \"points\" must hold x, y pairs" % what)
    return ("poly", [np.asarray(_ints(pts, what, MAX_COORD + 1), dtype=np.int64).reshape(-1, 2)], None)


def _rle_spec(seg, what):
    size, counts = seg.get("size"), seg.get("counts")
    if not isinstance(size, list) or len(size) != 2:
        raise ScoreError("%s: an RLE needs \"size\": [height, width]" % what)
    if isinstance(counts, str):
        counts = rle_from_string(counts)
    if not isinstance(counts, list) or any(not isinstance(c, int) for c in counts):
        raise ScoreError("%s: the \"counts\" of an RLE must be a string or a list of integers" % what)
    return ("rle", counts, (int(size[0]), int(size[1])))


# ------------------------------------------------------------------------------------------ one video
def _video_metrics(acc):
    m = acc.metrics()
    m["idfp"], m["idfn"] = acc._id_measures()
    m["idtp"] = m["num_objects"] - m["idfn"]
    return m


def overall(partials):
    """`MetricsHost.compute_overall` over the videos' metrics, in their order."""
    r = {k: sum(p[k] for p in partials) for k in ADDITIVE}
    det, nobj, npred = r["num_detections"], r["num_objects"], r["num_predictions"]
    r["mota"] = 1.0 - _quiet_divide(r["num_misses"] + r["num_switches"] + r["num_false_positives"], nobj)
    if det == 0:
        r["motp"] = 0.0
    else:
        res = 0
        for p in partials:
            res += p["motp"] * p["num_detections"]
        r["motp"] = _quiet_divide(res, det)
    r["precision"] = _quiet_divide(det, r["num_false_positives"] + det)
    r["recall"] = _quiet_divide(det, nobj)
    r["idp"] = _quiet_divide(r["idtp"], r["idtp"] + r["idfp"])
    r["idr"] = _quiet_divide(r["idtp"], r["idtp"] + r["idfn"])
    r["idf1"] = _quiet_divide(2 * r["idtp"], nobj + npred)
    return r


def _accumulate(counted, hyps, kept, e2e, memo):
    """counted: per frame [(id, text)], hyps: per frame [(id, text)], kept: per frame [(object, hypothesis, IoU)]."""
    acc = MOTAccumulator()
    for f in range(len(counted)):
        pairs = kept[f]
        if e2e:
            pairs = [(i, j, v) for i, j, v in pairs
                     if cal_similarity(clean_text(counted[f][i][1]), clean_text(hyps[f][j][1]), memo) >= 0.9]
        acc.update([o for o, _ in counted[f]], [h for h, _ in hyps[f]], pairs, f)
    return _video_metrics(acc)


def _off(per_frame):
    off = np.zeros(len(per_frame) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(x) for x in per_frame])
    return off


def _drop(hyps, counts, di, off):
    """Take the hypotheses named by an ignore pass out of their frames."""
    for f, hits in enumerate(_split(counts, di, np.zeros(len(di)), off)):
        drop = set(d for _, d, _ in hits)
        if drop:
            hyps[f] = [h for j, h in enumerate(hyps[f]) if j not in drop]


def score_bovtext(gt_raw, res_raw, e2e, threshold, host_iou, name, memo):
    key = "ID_transcription" if e2e else "transcription"
    gt = _parse(gt_raw, "ground truth of " + name, dict)
    res = _result_frames(res_raw, "result of " + name)
    F = len(gt)
    counted, ignored, hyps = [], [], []                          # per frame: (id, text, quad) / quad / (id, text, quad)
    for f in range(1, F + 1):
        what = "ground truth of %s, frame %d" % (name, f)
        objs = gt.get(str(f))
        if not isinstance(objs, list):
            raise ScoreError("%s: missing (frames must be numbered 1 .. %d)" % (what, F))
        cf, igf = [], []
        for o in objs:
            quad = _quad(o, what)
            if key not in o:
                raise ScoreError("%s: an object has no %r" % (what, key))
            if o[key] == "###" or o[key] == "#1":
                igf.append(quad)
            else:
                cf.append((_id(o, "ID", what), o[key], quad))
        what = "result of %s, frame %d" % (name, f)
        hf = [(_id(o, "ID", what), o.get("transcription", "error"), _quad(o, what)) for o in res.get(str(f), [])]
        counted.append(cf)
        ignored.append(igf)
        hyps.append(hf)
    pairs_fn = host_quad_pairs if host_iou else device_quad_pairs

    def run(objs, thr):
        gq = np.asarray([q for x in objs for q in x], dtype=np.int64).reshape(-1, 8)
        dq = np.asarray([h[2] for x in hyps for h in x], dtype=np.int64).reshape(-1, 8)
        if not len(gq) or not len(dq):
            return None
        return pairs_fn(gq, dq, _off(objs), _off(hyps), np.zeros(len(gq), dtype=np.int32), np.zeros(len(dq), dtype=np.int32), 0,
                        thr)
    r = run(ignored, IGNORE_IOU_BOVTEXT)
    if r is not None:
        _drop(hyps, r[0], r[1], _off(ignored))
    care = [[c[2] for c in x] for x in counted]
    r = run(care, float(np.nextafter(threshold, 0.0)))
    kept = _split(r[0], r[1], r[2], _off(care)) if r is not None else [[] for _ in range(F)]
    return _accumulate([[(c[0], c[1]) for c in x] for x in counted], [[(h[0], h[1]) for h in x] for x in hyps], kept, e2e, memo)


def score_artvideo(gt_raw, res_raw, e2e, curve, threshold, host_iou, name, memo):
    gt = _parse(gt_raw, "ground truth of " + name, dict)
    res = _result_frames(res_raw, "result of " + name)
    what = "ground truth of " + name
    frames, anns = gt.get("frame"), gt.get("annotations")
    if not isinstance(frames, list) or not frames or not isinstance(anns, list):
        raise ScoreError("%s: needs a non-empty \"frame\" list and an \"annotations\" list" % what)
    try:
        H, W = int(frames[0]["height"]), int(frames[0]["width"])
    except (KeyError, TypeError, ValueError):
        raise ScoreError("%s: the first frame has no integer height and width" % what)
    F = len(frames)
    counted, ignored, hyps = [[] for _ in range(F)], [[] for _ in range(F)], [[] for _ in range(F)]

    def sized(spec, what):
        if spec[2] is not None and spec[2] != (H, W):
            raise ScoreError("%s: a mask of size %s in a video of %d x %d" % (what, list(spec[2]), H, W))
        return spec[:2]
    for a in anns:
        if not isinstance(a, dict):
            raise ScoreError("%s: an annotation is not a JSON object" % what)
        f = _id(a, "frame_id", what)
        if not 1 <= f <= F:
            raise ScoreError("%s: frame_id %d outside 1 .. %d" % (what, f, F))
        for k in ("segmentation", "text_type", "Transcription"):
            if k not in a:
                raise ScoreError("%s: an annotation has no %r" % (what, k))
        if not isinstance(a["segmentation"], dict):
            raise ScoreError("%s: a ground-truth \"segmentation\" must be an RLE" % what)
        spec = sized(_rle_spec(a["segmentation"], what), what)
        text = a["Transcription"]
        ign = (e2e and (text == "###" or text == "#1")) or (curve and a["text_type"] == "Straight")
        if ign:
            ignored[f - 1].append(spec)
        else:
            counted[f - 1].append((_id(a, "obj_id", what), text, spec))
    for f in range(1, F + 1):
        what = "result of %s, frame %d" % (name, f)
        hyps[f - 1] = [(_id(o, "ID", what), o.get("transcription", "error") if isinstance(o, dict) else "", sized(_result_mask(o, what), what))
                       for o in res.get(str(f), [])]
    pairs_fn = host_mask_pairs if host_iou else device_mask_pairs

    def run(objs, thr):
        gs = [s for x in objs for s in x]
        ds = [h[2] for x in hyps for h in x]
        if not gs or not ds:
            return None
        return pairs_fn(MaskSet(gs, H, W), MaskSet(ds, H, W), _off(objs), _off(hyps), np.zeros(len(gs), dtype=np.int32),
                        np.zeros(len(ds), dtype=np.int32), thr)
    r = run(ignored, threshold)
    if r is not None:
        _drop(hyps, r[0], r[1], _off(ignored))
    care = [[c[2] for c in x] for x in counted]
    r = run(care, float(np.nextafter(threshold, 0.0)))
    kept = _split(r[0], r[1], r[2], _off(care)) if r is not None else [[] for _ in range(F)]
    return _accumulate([[(c[0], c[1]) for c in x] for x in counted], [[(h[0], h[1]) for h in x] for x in hyps], kept, e2e, memo)


def score_method(protocol, gt_path, res_path, e2e=False, curve=False, threshold=0.5, host_iou=False):
    """-> {"overall": {...}, "per_sample": {video: {...}}} with motmetrics' metric names."""
    if protocol not in ("bovtext", "artvideo"):
        raise ScoreError("unknown protocol %r" % protocol)
    if curve and protocol != "artvideo":
        raise ScoreError("--curve belongs to --protocol artvideo")
    gt = load_jsons(gt_path, 1 if protocol == "bovtext" else 0)
    if not gt:
        raise ScoreError("no ground-truth .json in %r" % gt_path)
    res = load_jsons(res_path, 0)
    memo = {}
    per_sample = {}
    for name in gt:
        if protocol == "bovtext":
            per_sample[name] = score_bovtext(gt[name], res.get(name), e2e, threshold, host_iou, name, memo)
        else:
            per_sample[name] = score_artvideo(gt[name], res.get(name), e2e, curve, threshold, host_iou, name, memo)
    return {"overall": overall(list(per_sample.values())), "per_sample": per_sample}


def main(args):
    """The command line of `score.main` for --protocol bovtext / artvideo."""
    try:
        if not (0.0 < args.threshold < 1.0):
            raise ScoreError("--threshold must lie strictly between 0 and 1")
        res = score_method(args.protocol, args.gt, args.results, args.e2e, args.curve, args.threshold, args.host_iou)
        with open(args.output, "w") as f:
            json.dump(res, f, indent=2, sort_keys=True)
    except ScoreError as e:
        sys.stderr.write("error: %s\n" % e)
        return 2
    except OSError as e:
        sys.stderr.write("error: %s\n" % e)
        return 2
    line = "%s: MOTA %.4f  MOTP %.4f  IDF1 %.4f  IDP %.4f  IDR %.4f  precision %.4f  recall %.4f  SW %d  FP %d  MS %d"
    for k, s in [("OVERALL", res["overall"])] + list(res["per_sample"].items()):
        print(line % (k, s["mota"], s["motp"], s["idf1"], s["idp"], s["idr"], s["precision"], s["recall"], s["num_switches"],
                      s["num_false_positives"], s["num_misses"]))
    return 0
