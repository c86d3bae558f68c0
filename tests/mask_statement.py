"""The mask measure of ArTVideo scoring, stated in plain Python / numpy integers (not collected: no test_ prefix).

What csrc/mask_pairs.hip, `score_json.host_mask_pairs` and the readers are held to:

  fill_contours     the project's statement of `cv2.fillPoly(img, contours, 1)` (lineType 8, shift 0) on an H x W image: the
                    union over the contours of Fill(contour) and Boundary(contour), step by step as written in
                    include/gomatching_hip.h -- the boundary by the error-stepped 8-connected line, the fill by the SORTED
                    PAIRED form (`form="paired"`) or by the sort-free count form (`form="count"`).  PARITY with OpenCV is
                    UNPINNED (cv2 is not available to the tests).
  rle_decode / rle_from_string / rle_to_string
                    COCO run-length masks: runs alternate 0 / 1 starting with 0 in column-major order; the compressed string
                    is the one `rleFrString` / `rleToString` of the COCO API read and write.  UNPINNED against pycocotools.
  levenshtein       the textbook full-matrix edit distance.  UNPINNED against the Levenshtein package.
  mask_pairs_statement
                    the kept (ground truth, detection) pairs of a video on boolean images, with the return convention of
                    score_statement.pairs_statement.
"""
import numpy as np

S = 16


def _cdiv(a, b):
    """C division of Python integers: truncation toward zero."""
    q = abs(a) // abs(b)
    return q if (a >= 0) == (b > 0) else -q


def line_pixels(x0, y0, x1, y1):
    """The 8-connected line between two integer points, both inclusive, as the rule steps it."""
    if x1 < x0:
        x0, y0, x1, y1 = x1, y1, x0, y0
    dx, dy = x1 - x0, y1 - y0
    ax, ay = abs(dx), abs(dy)
    sx = 1 if dx > 0 else 0
    sy = 1 if dy > 0 else (-1 if dy < 0 else 0)
    M, m = max(ax, ay), min(ax, ay)
    y_major = ay > ax
    err = M - 2 * m
    out = []
    x, y = x0, y0
    for _ in range(M + 1):
        out.append((x, y))
        if err < 0:
            x, y = x + sx, y + sy
            err += 2 * M - 2 * m
        else:
            if y_major:
                y += sy
            else:
                x += sx
            err -= 2 * m
    return out


def crossings(contour, y):
    """The positions X(y) of the edges active on scanline y, unsorted, in 2^-S pixel units."""
    out = []
    n = len(contour)
    for i in range(n):
        xa, ya = contour[i - 1]
        xb, yb = contour[i]
        if ya == yb:
            continue
        if ya < yb:
            xt, yt, xbot, ybot = xa, ya, xb, yb
        else:
            xt, yt, xbot, ybot = xb, yb, xa, ya
        if not (yt <= y < ybot):
            continue
        dxq = _cdiv((xbot - xt) << S, ybot - yt)
        out.append((xt << S) + (y - yt) * dxq)
    return out


def fill_contours(contours, H, W, form="paired"):
    """contours: a list of [[x, y], ...] integer vertex lists -> bool [H, W]."""
    img = np.zeros((H, W), dtype=bool)
    for contour in contours:
        contour = [(int(p[0]), int(p[1])) for p in contour]
        if not contour:
            continue
        for i in range(len(contour)):
            for x, y in line_pixels(*contour[i - 1], *contour[i]):
                if 0 <= x < W and 0 <= y < H:
                    img[y, x] = True
        ys = [p[1] for p in contour]
        for y in range(max(min(ys), 0), min(max(ys), H)):         # the lowest row max(ys) has no active edge
            cs = crossings(contour, y)
            if form == "paired":
                cs.sort()
                for k in range(0, len(cs) - 1, 2):
                    lo = -((-cs[k]) >> S)                         # ceil(c / 2^S)
                    hi = cs[k + 1] >> S                           # floor(c / 2^S)
                    lo, hi = max(lo, 0), min(hi, W - 1)
                    if lo <= hi:
                        img[y, lo:hi + 1] = True
            else:
                for x in range(W):
                    xp = x << S
                    a = sum(1 for c in cs if c < xp)
                    b = sum(1 for c in cs if c <= xp)
                    if b > a or (a & 1):
                        img[y, x] = True
    return img


# ------------------------------------------------------------------------------------------ COCO run-length masks
def rle_from_string(s):
    """The compressed `counts` string -> the list of run lengths (`rleFrString`: 5 payload bits per character, bit 0x20 =
    more, sign extension from bit 0x10 of the last chunk, and from the fourth count on the count two places back is added)."""
    if isinstance(s, bytes):
        s = s.decode("ascii")
    counts = []
    p = 0
    while p < len(s):
        x, k, more = 0, 0, True
        while more:
            c = ord(s[p]) - 48
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


def rle_to_string(counts):
    """The encoder of the same format (`rleToString`), for round trips."""
    out = []
    for i, x in enumerate(counts):
        x = int(x)
        if i > 2:
            x -= int(counts[i - 2])
        more = True
        while more:
            c = x & 0x1f
            x >>= 5
            more = (x != -1) if (c & 0x10) else (x != 0)
            if more:
                c |= 0x20
            out.append(chr(c + 48))
    return "".join(out)


def rle_encode(img):
    """bool [H, W] -> the list of run lengths (column-major, starting with a run of zeros that may be empty)."""
    flat = np.asarray(img, dtype=bool).T.reshape(-1)
    counts, cur, run = [], False, 0
    for v in flat.tolist():
        if v != cur:
            counts.append(run)
            cur, run = v, 0
        run += 1
    counts.append(run)
    return counts


def rle_decode(rle):
    """{"size": [H, W], "counts": list or string} -> bool [H, W]."""
    H, W = rle["size"]
    counts = rle["counts"]
    if isinstance(counts, (str, bytes)):
        counts = rle_from_string(counts)
    flat = np.zeros(H * W, dtype=bool)
    p, v = 0, False
    for c in counts:
        if v:
            flat[p:p + c] = True
        p += c
        v = not v
    return flat.reshape(W, H).T.copy()


# ------------------------------------------------------------------------------------------ strings
def levenshtein(a, b):
    """Edit distance (insert, delete, substitute, each 1) by the full (len(a)+1) x (len(b)+1) table."""
    d = [[0] * (len(b) + 1) for _ in range(len(a) + 1)]
    for i in range(len(a) + 1):
        d[i][0] = i
    for j in range(len(b) + 1):
        d[0][j] = j
    for i in range(1, len(a) + 1):
        for j in range(1, len(b) + 1):
            d[i][j] = min(d[i - 1][j] + 1, d[i][j - 1] + 1, d[i - 1][j - 1] + (a[i - 1] != b[j - 1]))
    return d[len(a)][len(b)]


def similarity(a, b):
    """`cal_similarity` of the protocols."""
    if a == "" and b == "":
        return 1.0
    dist = levenshtein(a, b)
    if dist == 1:
        return 0.95
    return 1 - dist / max(len(a), len(b))


# ------------------------------------------------------------------------------------------ pairs
def mask_pairs_statement(gt_imgs, det_imgs, gt_off, det_off, gt_key, det_key, threshold):
    """Boolean images -> (counts [G], kept [(g, detection index within the frame, value)] ordered by g, then detection,
    eligible [(g, j, value)] for EVERY pair of equal keys, kept or not): the convention of score_statement.pairs_statement.
    The value is 0.0 when fewer than one pixel is shared, else intersection / union of the pixel counts in one fp64
    division; a pair is kept when its value is strictly above `threshold`."""
    G = len(gt_imgs)
    counts, kept, eligible = np.zeros(G, dtype=np.int32), [], []
    for f in range(len(gt_off) - 1):
        for g in range(int(gt_off[f]), int(gt_off[f + 1])):
            for j in range(int(det_off[f + 1]) - int(det_off[f])):
                d = int(det_off[f]) + j
                if int(gt_key[g]) != int(det_key[d]):
                    continue
                inter = int(np.count_nonzero(gt_imgs[g] & det_imgs[d]))
                if inter < 1:
                    v = 0.0
                else:
                    v = float(inter) / float(int(np.count_nonzero(gt_imgs[g])) + int(np.count_nonzero(det_imgs[d])) - inter)
                eligible.append((g, j, v))
                if v > threshold:
                    counts[g] += 1
                    kept.append((g, j, v))
    return counts, kept, eligible


# ------------------------------------------------------------------------------------------ shared cases
HAND_CASES = [                                                    # (contours, H, W, the pixels (x, y) the rule gives)
    ([[(1, 1), (3, 1), (3, 3), (1, 3)]], 5, 5, {(x, y) for x in range(1, 4) for y in range(1, 4)}),
    ([[(0, 0), (4, 0), (0, 4)]], 5, 5, {(x, y) for x in range(5) for y in range(5) if x + y <= 4}),
    ([[(2, 3), (2, 3), (2, 3)]], 5, 5, {(2, 3)}),
    ([[(1, 2), (5, 2), (3, 2)]], 5, 7, {(x, 2) for x in range(1, 6)}),
    ([[(10, 10), (14, 10), (14, 14)]], 5, 5, set()),
]


def random_contours(n=200, H=64, W=96, seed=11):
    """Seeded contours of 3..50 vertices: star-shaped ones around a centre (simple), raw random vertex lists
    (self-intersecting), some with vertices up to 20 pixels outside the image, some with repeated vertices."""
    rng = np.random.RandomState(seed)
    out = []
    for k in range(n):
        nv = int(rng.randint(3, 51))
        lo = -20 if k % 3 == 0 else 0
        if k % 2 == 0:
            cx, cy = rng.randint(lo, W - lo), rng.randint(lo, H - lo)
            ang = np.sort(rng.uniform(0, 2 * np.pi, nv))
            rad = rng.uniform(2, 30, nv)
            pts = np.stack([cx + rad * np.cos(ang), cy + rad * np.sin(ang)], 1).astype(np.int64)
            pts[:, 0] = np.clip(pts[:, 0], lo, W - 1 - lo)
            pts[:, 1] = np.clip(pts[:, 1], lo, H - 1 - lo)
        else:
            pts = np.stack([rng.randint(lo, W - lo, nv), rng.randint(lo, H - lo, nv)], 1).astype(np.int64)
        if k % 7 == 0:
            pts[nv // 2] = pts[0]
        out.append(pts)
    return out
