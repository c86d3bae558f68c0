"""fp64 statements of the kernels that make discrete decisions -- proposal top-k (csrc/topk.hip), character argmax and detection
post-processing (csrc/detect.hip), proposal validity, the padded position table and the Bezier reference points
(csrc/elementwise.hip) -- with the error bounds of their float outputs, and the inputs and case tables that
tests/test_select_statement_cpu.py and tests/test_select_forms_gpu.py share (same generators, same seeds, same bits).  No test in
here, no GPU, no oracle import.

The statements are written for clarity and not after the kernels: a sort where the kernel ranks, a loop where it runs rounds.  Every
bound is derived from the kernels' operation count with U = 2^-24; nothing in a bound is measured and nothing is taken from a
kernel's output.  A decision (score against a threshold, IoU against nms_thr, the order of two scores) is *decided* when its margin
in fp64 exceeds the bound of the fp32 values it is taken on; the case tables hold only inputs all of whose decisions are decided,
except the kind `exact`, whose inputs are exactly representable and whose expected outputs are written out by hand."""
import numpy as np

U = 2.0 ** -24                                        # half an ulp of fp32: the relative error of one correctly rounded operation
EXPF = 4                                              # expf: 2 ulp = 4 U (the device library documents 1 ulp; numpy's is no worse)
RCP = 2                                               # 1 / x: 1 ulp = 2 U (a correctly rounded division is U; a hardware reciprocal 1 ulp)
SECOND = 1.0 + 2.0 ** -10                             # the products of two first-order terms, each below 2^-10 of a first-order one
ABS_TABLE = 2e-6                                      # Bezier points and position tables: the absolute bound tests/test_ops_gpu.py holds
CHUNK, MERGE_MAX, MAXQ = 4096, 8192, 1024             # csrc/topk.hip, csrc/detect.hip (the limits tests are written against them)


def _f32(x):
    return np.asarray(x, np.float32)


# ------------------------------------------------------------------------------------------ top-k
def topk64(logits, valid, c0, k):
    """logits [B, S]; valid [S] bool or None; c0: the logit of an invalid token -> (idx [B, k], rows [B, k]): invalid tokens take
    c0, tokens are ordered by value descending then index ascending, rows = b * S + idx.  (-0.0 == +0.0 here; the kernel orders
    their bit patterns, so a row that mixes them is compared on gathered values only.)"""
    v = np.array(logits, np.float64)
    B, S = v.shape
    if valid is not None:
        v[:, ~np.asarray(valid, bool)] = float(c0)
    idx = np.stack([np.lexsort((np.arange(S), -v[b]))[:k] for b in range(B)])
    return idx, np.arange(B)[:, None] * S + idx


def topk_values(logits, valid, c0, idx):
    v = np.array(logits, np.float64)
    if valid is not None:
        v[:, ~np.asarray(valid, bool)] = float(c0)
    return np.take_along_axis(v, np.asarray(idx, np.int64), 1)


class TopkCase:
    """One (B, S, k) with one value kind.  logits() [B, S] float32 (rows differ per b), valid() [S] bool or None, c0."""

    def __init__(self, B, S, k, kind):
        self.B, self.S, self.k, self.kind = B, S, k, kind
        self.id = "B%d-S%d-k%d-%s" % (B, S, k, kind)
        self.values_only = kind == "signed_zeros"
        self.c0 = {"invalid_flood_high": 50.0, "invalid_flood_low": -50.0}.get(kind, 0.37)

    def _rng(self):
        return np.random.default_rng([self.B, self.S, self.k, sum(map(ord, self.kind))])

    def logits(self):
        B, S, k, g = self.B, self.S, self.k, self._rng()
        x = g.standard_normal((B, S)).astype(np.float32)
        if self.kind == "signed_extremes":
            big, den = np.finfo(np.float32).max, np.float32(1e-45)
            pool = np.array([np.inf, -np.inf, big, -big, den, -den, 3 * den, -3 * den, np.float32(2 ** -126), -np.float32(2 ** -126),
                             -1.0, np.nextafter(np.float32(-1), np.float32(0)), np.nextafter(np.float32(-1), np.float32(-2)),
                             1.0, np.nextafter(np.float32(1), np.float32(2))], np.float32)
            at = g.permutation(S)[:min(S, len(pool))]
            for b in range(B):                        # distinct specials, so the row has no tie; their places differ per b
                x[b, np.roll(at, b)] = pool[:len(at)]
        elif self.kind == "signed_zeros":
            x[:, ::2] = np.float32(0.0)
            x[:, 1::2] = np.float32(-0.0)
            x[:, ::7] = -np.abs(x[:, ::7]) - 1
        elif self.kind == "all_equal":
            x[:] = np.arange(B, dtype=np.float32)[:, None] - 1      # -1, 0, 1, ...: one constant per row
        elif self.kind == "tie_across_chunk":
            x[:, CHUNK - 6:min(S, CHUNK + 6)] = np.float32(7.5)
        elif self.kind == "last_chunk_wins":
            x[:, (-(-S // CHUNK) - 1) * CHUNK:] += np.float32(100)
        return x

    def valid(self):
        S, g = self.S, np.random.default_rng([self.S, self.k, 5])
        if self.kind == "invalid_flood_high":
            return g.random(S) >= 0.9
        if self.kind == "invalid_flood_low":
            v = np.zeros(S, bool)
            v[g.permutation(S)[:self.k // 2]] = True
            return v
        if self.kind in ("randn", "signed_extremes"):
            return g.random(S) >= 0.2
        return None

    def expected(self):
        return topk64(self.logits(), self.valid(), self.c0, self.k)

    def by_hand(self):
        """The winners where the kind names them outright (None elsewhere), [B, k]."""
        B, S, k = self.B, self.S, self.k
        if self.kind == "all_equal":
            return np.tile(np.arange(k), (B, 1))
        if self.kind == "invalid_flood_high":
            inv = np.flatnonzero(~self.valid())
            return np.tile(inv[:k], (B, 1)) if len(inv) >= k else None
        if self.kind == "tie_across_chunk":
            t = np.arange(CHUNK - 6, min(S, CHUNK + 6))
            return np.tile(t[:k], (B, 1)) if k <= len(t) else None
        return None


TOPK_SHAPES = [(2, 1, 1), (2, 37, 37), (3, 4095, 100), (3, 4096, 4096), (3, 4097, 100), (2, 8192, 4096), (8, 8193, 100),
               (1, 27 * 4096, 300)]
TOPK_KINDS = ["randn", "signed_extremes", "signed_zeros", "all_equal", "tie_across_chunk", "last_chunk_wins", "invalid_flood_high",
              "invalid_flood_low"]
TOPK_CASES = [TopkCase(B, S, k, kind) for (B, S, k) in TOPK_SHAPES for kind in TOPK_KINDS
              if not (kind == "tie_across_chunk" and S <= CHUNK)]


# ------------------------------------------------------------------------------------------ argmax
def argmax_first(x):
    """x [rows, V] -> the index of the first maximum of every row; a constant row (all -inf too) gives 0.  Rows that hold a NaN
    have no statement: the reference leaves their result unspecified, the kernel only owes an index in [0, V)."""
    return np.argmax(np.asarray(x, np.float64), axis=1)


ARGMAX_V = [1, 2, 37, 38, 63, 64, 65, 129]
ARGMAX_ROWS = [1, 3, 5, 1025]
ARGMAX_KINDS = ["randn", "dup_max", "constant", "neg_inf", "nan"]


def argmax_input(V, rows, kind):
    g = np.random.default_rng([V, rows, sum(map(ord, kind))])
    x = g.standard_normal((rows, V)).astype(np.float32)
    r = np.arange(rows)
    if kind == "dup_max":
        top = np.float32(9)
        if V > 64:                                    # even rows: j and j + 64 (one lane, two passes); odd rows: a lower index that a
            j = r % (V - 64)                          # higher lane owns (lo, lane lo) against 64 + lane (lane < lo)
            lo = 1 + r % 63
            hi = np.minimum(64 + r % lo, V - 1)
            a, b = np.where(r % 2 == 0, j, lo), np.where(r % 2 == 0, j + 64, hi)
        else:
            a, b = r % V, (r * 7 + 3) % V
        x[r, a] = top
        x[r, b] = top
    elif kind == "constant":
        x[:] = (r % 5 - 2).astype(np.float32)[:, None]
    elif kind == "neg_inf":
        x[:] = -np.inf
        x[1::2, V // 2:] = -np.inf                    # (all rows are all -inf; odd rows keep the statement honest about V // 2)
    elif kind == "nan":
        x[g.random((rows, V)) < 0.3] = np.nan
        x[::3] = np.nan
    return x


# ------------------------------------------------------------------------------------------ validity, position table, Bezier
def level_starts(shapes):
    hw = np.asarray(shapes, np.int64).prod(1)
    return np.concatenate(([0], np.cumsum(hw)[:-1])), int(hw.sum())


def _grid32(shapes, vshapes):
    """The reference's proposal grid (deformable_transformer.py:113-124) in float32: per token ((col + 0.5) / valid_W,
    (row + 0.5) / valid_H); a single fp32 division is correctly rounded on both sides, so equality with the kernel is exact."""
    gx, gy = [], []
    for l, (H, W) in enumerate(shapes):
        Hv, Wv = (H, W) if vshapes is None else vshapes[l]
        r, c = np.divmod(np.arange(H * W), W)
        gx.append((c.astype(np.float32) + np.float32(0.5)) / np.float32(Wv))
        gy.append((r.astype(np.float32) + np.float32(0.5)) / np.float32(Hv))
    return np.concatenate(gx), np.concatenate(gy)


def proposal_valid_ref(shapes, vshapes=None):
    """[S] bool: both grid coordinates strictly inside (0.01, 0.99), compared in float32."""
    gx, gy = _grid32(shapes, vshapes)
    lo, hi = np.float32(0.01), np.float32(0.99)
    return (gx > lo) & (gx < hi) & (gy > lo) & (gy < hi)


def dim_t32():
    j = np.arange(128, dtype=np.float32)
    return (np.float32(10000) ** (2 * np.floor(j / 2) / np.float32(128))).astype(np.float32)


def enc_pos_valid64(dim_t, level_embed, H, W, Hv, Wv):
    """PositionalEncoding2D of a level whose valid region is [Hv, Wv] of a padded [H, W] (pos_encoding.py:62-82) plus the level
    embedding -> ([H * W, 256] float64, owned [H * W] bool).  Channels [0, 128) <- rows, [128, 256) <- columns; even channels sin,
    odd cos.  The cumulative sums stop at the valid extent, so the normaliser is Hv / Wv; tokens outside it are never read and
    have no statement (owned False)."""
    dt = np.asarray(dim_t, np.float64)
    r, c = np.divmod(np.arange(H * W), W)
    ay = ((r + 1 - 0.5) / (Hv + 1e-6) * 2 * np.pi)[:, None] / dt
    ax = ((c + 1 - 0.5) / (Wv + 1e-6) * 2 * np.pi)[:, None] / dt
    odd = (np.arange(128) % 2 == 1)
    tab = np.concatenate([np.where(odd, np.cos(ay), np.sin(ay)), np.where(odd, np.cos(ax), np.sin(ax))], 1)
    return tab + np.asarray(level_embed, np.float64), (r < Hv) & (c < Wv)


def bernstein(P):
    t = np.linspace(0.0, 1.0, P)
    return np.stack([(1 - t) ** 3, 3 * t * (1 - t) ** 2, 3 * t ** 2 * (1 - t), t ** 3], 1)


def bezier64(coord, idx, shapes, vshapes, bern):
    """coord [B, S, 8] float32, idx [B, nq] token indices, bern [P, 4] -> [B, nq, P, 2] float64: the selected tokens' four control
    points are sigmoid(coord + proposal logit), the proposal logit log(g / (1 - g)) of the token's grid position, +inf for an
    invalid token (so its control points are 1); the output is the Bernstein sum over the four (deformable_transformer.py:99-106,
    183-199)."""
    starts, S = level_starts(shapes)
    gx, gy = [], []
    for l, (H, W) in enumerate(shapes):
        Hv, Wv = (H, W) if vshapes is None else vshapes[l]
        r, c = np.divmod(np.arange(H * W), W)
        gx.append((c + 0.5) / Wv)
        gy.append((r + 0.5) / Hv)
    ok = proposal_valid_ref(shapes, vshapes)
    with np.errstate(divide="ignore", invalid="ignore"):
        g = np.stack([np.concatenate(gx), np.concatenate(gy)], 1)
        logit = np.where(ok[:, None], np.log(g / (1 - g)), np.inf)          # [S, 2]
    B, nq = idx.shape
    c = np.take_along_axis(np.asarray(coord, np.float64), np.asarray(idx, np.int64)[:, :, None], 1).reshape(B, nq, 4, 2)
    ctl = 1.0 / (1.0 + np.exp(-(c + logit[idx][:, :, None, :])))
    return np.einsum("pk,bqkc->bqpc", np.asarray(bern, np.float64), ctl)


# levels with H or W in {1, 12, 50, 150, 250}: at 50, 150 and 250 (i + 0.5) / W falls on 0.01 or 0.99
GEO_CASES = [
    ("unpadded", [(1, 250), (12, 50), (150, 12), (50, 1)], None),
    ("padded64", [(64, 64), (64, 12), (1, 64), (12, 64)], [(50, 50), (50, 12), (1, 50), (12, 50)]),
]


def geo_bezier_inputs(shapes, vshapes, B=2, nq=40, P=25):
    """(coord [B, S, 8] float32, idx [B, nq]): random distinct tokens, the first quarter replaced by invalid ones."""
    starts, S = level_starts(shapes)
    g = np.random.default_rng([S, nq, P])
    coord = g.standard_normal((B, S, 8)).astype(np.float32)
    inv = np.flatnonzero(~proposal_valid_ref(shapes, vshapes))
    idx = np.stack([g.permutation(S)[:nq] for _ in range(B)])
    idx[:, :nq // 4] = np.stack([g.permutation(inv)[:nq // 4] for _ in range(B)])
    return coord, idx


# ------------------------------------------------------------------------------------------ detection post-processing
def score64(logits):
    """logits [..., P] float32 -> (s, bound): s = sigmoid(mean) and the bound of the kernel's fp32 value,

        x   = fl(fl(sum_p l_p) / P)          a sequential sum of P terms: (P - 1) U sum|l_p|; the division: U |x|
        e   = expf(-x)                       relative error EXPF U + dx: the exponential turns an absolute error of its argument
                                             into a relative one of its value
        s   = 1 / fl(1 + e)                  the addition U, the reciprocal RCP U; e's error reaches s scaled by e / (1 + e) = 1 - s

        bound = s expm1((1 - s) (EXPF U + dx) + (1 + RCP) U),     dx = ((P - 1) sum|l_p| / P + |x|) U SECOND"""
    l = np.asarray(logits, np.float32).astype(np.float64)
    P = l.shape[-1]
    x = l.sum(-1) / P
    dx = ((P - 1) * np.abs(l).sum(-1) / P + np.abs(x)) * U * SECOND
    s = 1.0 / (1.0 + np.exp(-x))
    return s, s * np.expm1((1 - s) * (EXPF * U + dx) + (1 + RCP) * U)


def final_score64(cls, recls):
    """The query score and its bound: score64 of cls, with rescoring the larger of that and score64 of recls.  Where the two are
    closer than their bounds the kernel may take either, within the larger bound."""
    s, sb = score64(cls)
    if recls is None:
        return s, sb
    r, rb = score64(recls)
    return np.maximum(s, r), np.where(np.abs(s - r) <= sb + rb, np.maximum(sb, rb), np.where(s > r, sb, rb))


def boxes32(bd, img_h, img_w):
    """bd [..., P, 4] float32 normalised (x, y, x, y) -> ([..., 4] boxes, [..., P, 4] px points) float32: one fp32 multiply per
    coordinate, then min / max -- exact on both sides."""
    px = _f32(bd) * np.array([img_w, img_h, img_w, img_h], np.float32)
    xs, ys = px[..., 0::2], px[..., 1::2]
    lead = px.shape[:-2]
    box = np.stack([xs.reshape(lead + (-1,)).min(-1), ys.reshape(lead + (-1,)).min(-1), xs.reshape(lead + (-1,)).max(-1),
                    ys.reshape(lead + (-1,)).max(-1)], -1)
    return box, px


def iou64(a, b):
    """Boxes a [4], b [n, 4] float32 -> (iou, bound) float64 [n] of the kernel's inter / (iarea + area - inter):

        w, h         one subtraction of exact operands each: U
        inter, area  a product of two such differences: 3 U each
        union        fl(iarea + area) - inter with the product w h rounded first or contracted into an fma: either way within
                     U (4 (iarea + area) + 3 inter + union)
        iou          (d inter + iou d union) / (union - d union) + U iou

    A pair of zero-area boxes at one place gives 0 / 0 on both sides: NaN, which no threshold test passes (bound 0)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    w = np.maximum(0.0, np.minimum(a[2], b[:, 2]) - np.maximum(a[0], b[:, 0]))
    h = np.maximum(0.0, np.minimum(a[3], b[:, 3]) - np.maximum(a[1], b[:, 1]))
    inter = w * h
    ia, ar = (a[2] - a[0]) * (a[3] - a[1]), (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    union = ia + ar - inter
    du = U * (4 * (ia + ar) + 3 * inter + np.abs(union)) * SECOND
    with np.errstate(divide="ignore", invalid="ignore"):
        iou = inter / union
        bound = ((3 * U * inter * SECOND + iou * du) / (union - du) + U * iou) * SECOND
    return iou, np.where(np.isnan(iou), 0.0, bound)


def detect64(cls, recls, ctrl, bd, recs, hw, det_thr, nms_thr, asso_thr):
    """GoMatching.detection() + box NMS + the association head's foreground filter (gom_lstmatcher.py:579-629, 310-332,
    lstmatcher.py:271-282).  cls / recls [B, nq, P] float32 (recls may be None), ctrl [B, nq, P, 2], bd [B, nq, P, 4], recs
    [B, nq, P] int -> a dict:

        score = sigmoid(mean_p cls), with rescoring the larger of that and sigmoid(mean_p recls)          (fp64)
        selected: score > det_thr;  ranked by score descending, equal scores by query index (stable)
        greedy NMS in that order: a live box suppresses every later live box whose IoU with it is > nms_thr
        kept: the survivors with score > asso_thr, in rank order

    count [B], kept (a list of query index arrays), keep_idx (b * nq + q), scores / score_bound / boxes / ctrl / bd / recs of the
    kept; and the margins the decisions were taken with, each as (margin, bound) pairs in `margins`:
        thr    |score - det_thr| and |score - asso_thr| of every query
        nms    |IoU - nms_thr| of every pair greedy NMS evaluates
        order  |s_i - s_j| of every two selected queries with different logits, against bound_i + bound_j
    The thresholds are the float32 values the kernel receives."""
    cls = _f32(cls)
    B, nq, P = cls.shape
    det_thr, nms_thr, asso_thr = (float(np.float32(t)) for t in (det_thr, nms_thr, asso_thr))
    s, sb = final_score64(cls, recls)
    same = (cls[:, :, None] == cls[:, None]).all(-1)
    if recls is not None:
        same &= (_f32(recls)[:, :, None] == _f32(recls)[:, None]).all(-1)
    box, bd_px = boxes32(bd, hw[0], hw[1])
    ctrl_px = _f32(ctrl) * np.array([hw[1], hw[0]], np.float32)
    out = {"count": np.zeros(B, np.int64), "kept": [], "keep_idx": [], "scores": [], "score_bound": [], "boxes": [], "ctrl": [],
           "bd": [], "recs": [], "margins": {"thr": [], "nms": [], "order": []}}
    m = out["margins"]
    for b in range(B):
        m["thr"].append(np.stack([np.minimum(np.abs(s[b] - det_thr), np.abs(s[b] - asso_thr)), sb[b]], 1))
        sel = np.flatnonzero(s[b] > det_thr)
        gap = np.abs(s[b][sel][:, None] - s[b][sel][None])
        need = sb[b][sel][:, None] + sb[b][sel][None]
        pair = np.triu(~same[b][np.ix_(sel, sel)], 1)
        m["order"].append(np.stack([gap[pair], need[pair]], 1))
        order = sel[np.argsort(-s[b][sel], kind="stable")]
        dead = np.zeros(len(order), bool)
        for i in range(len(order)):
            if dead[i]:
                continue
            later = np.flatnonzero(~dead[i + 1:]) + i + 1
            iou, ib = iou64(box[b, order[i]], box[b, order[later]])
            dead[later[iou > nms_thr]] = True
            ok = ~np.isnan(iou)
            m["nms"].append(np.stack([np.abs(iou[ok] - nms_thr), ib[ok]], 1))
        kept = order[~dead]
        kept = kept[s[b][kept] > asso_thr]
        out["count"][b] = len(kept)
        out["kept"].append(kept)
        out["keep_idx"].append(b * nq + kept)
        out["scores"].append(s[b][kept])
        out["score_bound"].append(sb[b][kept])
        out["boxes"].append(box[b][kept])
        out["ctrl"].append(ctrl_px[b][kept].reshape(len(kept), P * 2))
        out["bd"].append(bd_px[b][kept])
        out["recs"].append(np.asarray(recs)[b][kept].astype(np.int64))
    for k in m:
        m[k] = np.concatenate(m[k]) if len(m[k]) else np.zeros((0, 2))
    return out


def undecided(margins):
    """{name: number of decisions whose margin does not exceed its bound}."""
    return {k: int((v[:, 0] <= v[:, 1]).sum()) for k, v in margins.items()}


def worst_margin_ratio(margins):
    """{name: the largest bound / margin}: below 1 everywhere when every decision is decided."""
    return {k: float((v[:, 1] / np.maximum(v[:, 0], 1e-300)).max()) if len(v) else 0.0 for k, v in margins.items()}


IMG_HW = (96, 128)
DETECT_SHAPES = [(1, 1, 1), (3, 60, 25), (2, 255, 25), (2, 256, 25), (2, 257, 25), (1, 1024, 25)]
DETECT_THR = {"det<asso": (0.3, 0.45), "det>asso": (0.45, 0.3)}
# The generator seed of a case: the first one, counted up from 0 by `python tests/select_statement.py` on the CPU, at which every
# decision of the case is decided (cases not listed are decided at seed 0).  tests/test_select_statement_cpu.py holds every case to
# zero undecided decisions.
SEEDS = {
    "random_clustered-B2-nq255-P25-re-det0.3-asso0.45-nms0.5-ld1": 1,
    "random_clustered-B2-nq257-P25-nore-det0.3-asso0.45-nms0.5-ld1": 3,
    "random_clustered-B1-nq1024-P25-re-det0.3-asso0.45-nms0.3-ld1": 25,
    "random_clustered-B1-nq1024-P25-re-det0.45-asso0.3-nms0.5-ld1": 1,
    "random_clustered-B1-nq1024-P25-nore-det0.3-asso0.45-nms0.3-ld1": 73,
}


class DetectCase:
    """One input set for gom_detect_post.  inputs() -> dict(cls [B, nq, P], recls or None, ctrl, bd, recs, V); thresholds and the
    image size are attributes; expected() = detect64 of them; `hand`: the expected kept queries per frame written out by hand."""

    def __init__(self, kind, B, nq, P, with_re, thr, nms_thr, ld_cls=1, hw=IMG_HW, seed=0, hand=None, tag=""):
        self.kind, self.B, self.nq, self.P, self.with_re, self.ld_cls, self.hw, self.seed = kind, B, nq, P, with_re, ld_cls, hw, seed
        self.det_thr, self.asso_thr = thr
        self.nms_thr, self.hand = nms_thr, hand
        self.id = "%s-B%d-nq%d-P%d-%s-det%g-asso%g-nms%g-ld%d%s" % (kind, B, nq, P, "re" if with_re else "nore", thr[0], thr[1],
                                                                     nms_thr, ld_cls, tag)
        self._in = self._exp = None

    def _random(self, g):
        B, nq, P = self.B, self.nq, self.P
        centers = g.random((B, nq, 1, 2)) * 0.8 + 0.1
        src = centers[:, 1::3]
        centers[:, 0::3][:, :src.shape[1]] = src[:, :centers[:, 0::3].shape[1]]          # overlapping centres
        ctrl = np.clip(centers + (g.random((B, nq, P, 2)) - 0.5) * 0.1, 0, 1)
        bd = np.clip(np.concatenate([ctrl - 0.02, ctrl + 0.02], -1), 0, 1) + g.random((B, nq, P, 4)) * 0.01
        cls = g.standard_normal((B, nq, P)) * 2 - 0.5
        re = g.standard_normal((B, nq, P)) * 2 - 1.0
        return cls, re, ctrl, bd

    def inputs(self):
        if self._in is not None:
            return self._in
        B, nq, P = self.B, self.nq, self.P
        g = np.random.default_rng([self.seed, B, nq, P, int(self.with_re)])
        if self.kind == "exact":
            cls, re, ctrl, bd = _exact_inputs(B, nq, P)
        else:
            cls, re, ctrl, bd = self._random(g)
            q = np.arange(nq)
            if self.kind == "all_selected":           # distinct scores far apart, every one above both thresholds
                lv = np.linspace(0.5, 6.0, nq)[g.permutation(nq)]
                cls = np.broadcast_to(lv[None, :, None], (B, nq, P)).copy()
                re = cls - 1.0
            elif self.kind == "none_selected":
                cls, re = cls * 0 - 20.0, re * 0 - 20.0
            elif self.kind == "one_selected":
                cls, re = cls * 0 - 20.0, re * 0 - 20.0
                cls[:, nq // 2] = 3.0
            elif self.kind == "score_ties":           # groups of three queries with identical logits; their boxes overlap in pairs
                cls = cls[:, q // 3 * 3]
                re = re[:, q // 3 * 3]
            if B > 1 and self.kind == "random_clustered":
                cls[0], re[0] = -20.0, -20.0          # an empty frame
        V = 38
        recs = g.integers(0, V, (B, nq, P))
        self._in = {"cls": _f32(cls), "recls": _f32(re) if self.with_re else None, "ctrl": _f32(ctrl), "bd": _f32(bd),
                    "recs": recs.astype(np.int32)}
        return self._in

    def expected_scores(self):
        i = self.inputs()
        return final_score64(i["cls"], i["recls"])

    def expected(self):
        if self._exp is None:
            i = self.inputs()
            self._exp = detect64(i["cls"], i["recls"], i["ctrl"], i["bd"], i["recs"], self.hw, self.det_thr, self.nms_thr,
                                 self.asso_thr)
        return self._exp


# `exact`: a 64 x 128 image, P = 2, both points of a query carry the query's box corners k / 128 (x) and k / 64 (y), so the pixel
# boxes are the integers below.  Frame 0 has zero logits everywhere; frame 1 holds, by query index:
_EXACT_BOXES = [
    (100, 5, 110, 8),     # 0  zero logits: 1 / (1 + exp(0)) = 0.5 exactly; not > 0.5
    (46, 10, 56, 20),     # 1  chain C  logit 1.0   B n C = 70 / 130, A n C = 40 / 160: kept, because B is dead when its turn comes
    (20, 0, 24, 3),       # 2  D        logit 2.0   IoU with query 7 = 12 / 16 = 3/4: suppressed
    (0, 0, 4, 4),         # 3  A1       logit 5.0
    (43, 10, 53, 20),     # 4  chain B  logit 1.5   A n B = 70 / 130 > 1/2: suppressed by query 8
    (70, 30, 70, 40),     # 5  Z1       logit 0.75  zero area
    (90, 40, 95, 45),     # 6           logit -2    not selected
    (20, 0, 24, 4),       # 7  C34      logit 2.5
    (40, 10, 50, 20),     # 8  chain A  logit 3.0
    (70, 30, 70, 40),     # 9  Z2       logit 0.5   the same zero-area box: 0 / 0, kept as in torchvision
    (0, 0, 4, 2),         # 10 B1       logit 4.0   IoU with query 3 = 8 / 16 = 1/2 exactly: not > 0.5, kept
    (100, 50, 110, 60),   # 11 R        logit -3, rescoring logit 2.25: selected only through the rescoring branch
]
_EXACT_LOGITS = [0.0, 1.0, 2.0, 5.0, 1.5, 0.75, -2.0, 2.5, 3.0, 0.5, 4.0, -3.0]
# by hand, frame 1 (frame 0 keeps nothing): rank order 3, 10, 8, 7, (11,) 2, 4, 1, 5, 9; NMS drops 4 and 2
EXACT_KEPT_RE = [[], [3, 10, 8, 7, 11, 1, 5, 9]]
EXACT_KEPT_NORE = [[], [3, 10, 8, 7, 1, 5, 9]]


def _exact_inputs(B, nq, P):
    assert (B, nq, P) == (2, 12, 2)
    box = np.array(_EXACT_BOXES, np.float64) / np.array([128, 64, 128, 64])
    bd = np.broadcast_to(box[None, :, None, :], (B, nq, P, 4)).copy()
    ctrl = bd[..., :2] * 0.5 + bd[..., 2:] * 0.5
    cls = np.zeros((B, nq, P))
    cls[1] = np.array(_EXACT_LOGITS)[:, None]
    re = np.full((B, nq, P), -10.0)
    re[0] = 0.0
    re[1, 0] = 0.0                                    # query 0 stays at exactly 0.5 through the rescoring maximum too
    re[1, 11] = 2.25
    return cls, re, ctrl, bd


def _detect_cases():
    cases = []
    for n, (B, nq, P) in enumerate(DETECT_SHAPES):
        for with_re in (True, False):
            for t, (name, thr) in enumerate(DETECT_THR.items()):
                ld = 3 if (B, nq) == (3, 60) else 1
                cases.append(DetectCase("random_clustered", B, nq, P, with_re, thr, (0.5, 0.3)[(n + t) % 2], ld))
    for with_re in (True, False):
        cases.append(DetectCase("all_selected", 1, 1024, 25, with_re, (0.3, 0.45), 0.5))
        cases.append(DetectCase("none_selected", 2, 257, 25, with_re, (0.45, 0.3), 0.5))
        cases.append(DetectCase("one_selected", 2, 257, 25, with_re, (0.3, 0.45), 0.5))
        cases.append(DetectCase("score_ties", 3, 60, 25, with_re, (0.3, 0.45), 0.3, ld_cls=3))
        cases.append(DetectCase("score_ties", 2, 257, 25, with_re, (0.45, 0.3), 0.5))
        hand = EXACT_KEPT_RE if with_re else EXACT_KEPT_NORE
        # det 0.5 puts query 0 (and frame 0) on the selection threshold, with asso 0.25 so that nothing else would stop it; det 0.25
        # selects it and puts it on the asso threshold.  Neither keeps it, so both variants have the same kept queries.
        cases.append(DetectCase("exact", 2, 12, 2, with_re, (0.5, 0.25), 0.5, hw=(64, 128), hand=hand, tag="-a"))
        cases.append(DetectCase("exact", 2, 12, 2, with_re, (0.25, 0.5), 0.5, hw=(64, 128), hand=hand, tag="-b"))
    for c in cases:
        c.seed = SEEDS.get(c.id, 0)
    return cases


DETECT_CASES = _detect_cases()


def first_decided_seed(case, limit=200):
    for seed in range(limit):
        c = DetectCase(case.kind, case.B, case.nq, case.P, case.with_re, (case.det_thr, case.asso_thr), case.nms_thr, case.ld_cls,
                       case.hw, seed)
        if not any(undecided(c.expected()["margins"]).values()):
            return seed
    raise RuntimeError("no decided seed below %d for %s" % (limit, case.id))


if __name__ == "__main__":
    for case in DETECT_CASES:
        if case.kind != "exact":
            seed = first_decided_seed(case)
            if seed:
                print('    "%s": %d,' % (case.id, seed))
