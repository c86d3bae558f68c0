"""fp64 statements of the tracker's association kernels (csrc/track.hip, track_score_one / asso_score_block / gather_match_item of
csrc/tracker_tasks.h) with element-wise error bounds, and the inputs and case tables that tests/test_asso_statement_cpu.py and
tests/test_asso_forms_gpu.py share (same generators, same seeds, same bits).  No test in here.

Every bound is derived from the kernels' operation count with U = 2^-24 (half an ulp of fp32, the relative error of one correctly
rounded operation); nothing in a bound is measured and nothing is taken from a kernel's output.  The helpers carry (value, error)
pairs: `_rnd(v, d)` is the error of an fp32 operation whose exact result is v and whose operands bring the absolute error d:
d + U (|v| + d)."""
import numpy as np
import torch

U = 2.0 ** -24
TINY = 2.0 ** -126                                    # fp32's smallest normal number: below it a result may be flushed or denormal
EXPF = 4                                              # expf: 2 ulp = 4 U (the device library documents 1 ulp; numpy's is no worse)
EPS32 = float(np.float32(1e-8))                       # the kernels' `+ 1e-8f`


def _rnd(v, d=0.0):
    return d + U * (np.abs(v) + d)


# ------------------------------------------------------------------------------------------ softmax with a background logit
def softmax_bg64(l, E=0.0):
    """l [..., n] float64, the logits of ONE frame segment (n >= 1); E: an absolute error every logit may carry (broadcastable to
    [..., 1]; 0 for logits read from memory) -> (a, bound) [..., n].

        m = max(0, max_j l_j),   a_j = exp(l_j - m) / (sum_j exp(l_j - m) + exp(-m))

        r_j   = (|l_j - m| + EXPF) U        relative error of expf(fl(l_j - m)): the argument is rounded once, |l_j - m| U, and the
                                            exponential turns an absolute error of its argument into a relative one of its value
        rbar  = sum_j a_j r_j + a_bg EXPF U the same errors seen through the normaliser: their a-weighted mean; the background's
                                            argument 0 - m is exact
        rel_j = r_j + rbar + (ceil(n / 64) + 8) U + 2 E
        bound = a_j expm1(rel_j) + 2^-126

    ceil(n / 64): the lane-strided partial sum of a lane (ceil(n / 64) terms).  8: six butterfly steps, the background term's
    addition, the division.  2 E: softmax-with-background is invariant under a common shift of its n + 1 logits, of which the
    background's is exact, so a logit error reaches a_j once directly and once through the normaliser.  expm1 instead of its
    argument keeps the bound valid where |l_j - m| U is not small.  2^-126: results below fp32's normal range."""
    n = l.shape[-1]
    m = np.maximum(l.max(-1, keepdims=True), 0.0)
    d = l - m
    e, bg = np.exp(d), np.exp(-m)
    Z = e.sum(-1, keepdims=True) + bg
    a = e / Z
    r = (np.abs(d) + EXPF) * U
    rbar = (a * r).sum(-1, keepdims=True) + bg / Z * EXPF * U
    rel = r + rbar + (-(-n // 64) + 8) * U + 2 * E
    return a, a * np.expm1(rel) + TINY


def activate64(logits, offs):
    """Statement of gom_asso_activate_f32.  logits [n_k, N] float32 (numpy), offs [T + 1] -> (exp, bound) float64 [n_k, N]: per row
    and frame segment [offs[t], offs[t + 1]) the softmax with an appended zero logit (softmax_bg64, E = 0).  An empty segment
    writes nothing; the columns no segment owns hold NaN in both."""
    l = np.asarray(logits, np.float32).astype(np.float64)
    exp = np.full(l.shape, np.nan)
    bound = np.full(l.shape, np.nan)
    for t in range(len(offs) - 1):
        lo, hi = int(offs[t]), int(offs[t + 1])
        if hi > lo:
            exp[:, lo:hi], bound[:, lo:hi] = softmax_bg64(l[:, lo:hi])
    return exp, bound


# ------------------------------------------------------------------------------------------ boxes: IoU and the centre gate
def _norm(b, img_w, img_h):
    """Boxes [..., 4] px -> normalised coordinates and their error: one division, one rounding each."""
    x = np.asarray(b, np.float32).astype(np.float64) / np.array([float(np.float32(img_w)), float(np.float32(img_h))] * 2)
    return x, _rnd(x)


def _diff(a1, d1, a0, d0):
    v = a1 - a0
    return v, _rnd(v, d1 + d0)


def _prod(a, da, b, db):
    v = a * b
    return v, _rnd(v, np.abs(a) * db + np.abs(b) * da + da * db)


def iou64(kb, lb, img_w, img_h):
    """IoU of boxes kb with lb (broadcast over leading dimensions) as track_score_one and short_term_pairs_kernel compute it, and
    its bound as a formula in the inputs:

        x = fl(px / img)                                   error |x| U per coordinate
        w_k = x1 - x0 (both boxes, both axes)              error dx1 + dx0 + U |w|: the cancellation keeps the coordinates' errors
        ww = max(min(kx1, lx1) - max(kx0, lx0), 0)         min, max and the clamp are 1-Lipschitz: max(dkx1, dlx1) + max(dkx0, dlx0)
                                                           + U |ww|
        inter = ww hh,  a1 = w_k h_k,  a2 = w_l h_l        |a| db + |b| da + da db + U |ab|
        union = (a1 + a2) - inter                          the three errors + U |a1 + a2| + U |union|
        iou = inter > 0 ? inter / union : 0                (d inter + iou d union) / (union - d union) + U iou

    The branch is covered: where one side sees inter > 0 and the other does not, inter <= d inter on the side that divides."""
    k, dk = _norm(kb, img_w, img_h)
    l, dl = _norm(lb, img_w, img_h)
    kw, dkw = _diff(k[..., 2], dk[..., 2], k[..., 0], dk[..., 0])
    kh, dkh = _diff(k[..., 3], dk[..., 3], k[..., 1], dk[..., 1])
    lw, dlw = _diff(l[..., 2], dl[..., 2], l[..., 0], dl[..., 0])
    lh, dlh = _diff(l[..., 3], dl[..., 3], l[..., 1], dl[..., 1])

    def overlap(a):
        raw = np.minimum(k[..., a + 2], l[..., a + 2]) - np.maximum(k[..., a], l[..., a])
        d = _rnd(raw, np.maximum(dk[..., a + 2], dl[..., a + 2]) + np.maximum(dk[..., a], dl[..., a]))
        return np.maximum(raw, 0.0), d
    ww, dww = overlap(0)
    hh, dhh = overlap(1)
    inter, di = _prod(ww, dww, hh, dhh)
    a1, d1 = _prod(kw, dkw, kh, dkh)
    a2, d2 = _prod(lw, dlw, lh, dlh)
    s12 = a1 + a2
    union = s12 - inter
    du = _rnd(union, _rnd(s12, d1 + d2) + di)
    assert bool((union - du > 0).all()), "a degenerate box pair: the IoU has no bound"
    iou = np.where(inter > 0, inter / np.where(union > 0, union, 1.0), 0.0)
    return iou, _rnd(iou, (di + iou * du) / (union - du))


def gate64(kb, nb, img_w, img_h, eps=EPS32):
    """dist = (dx^2 + dy^2) / (ks + 1e-8f) of query boxes kb [n_k, 1, 4] against candidates nb [1, Np, 4] with its propagated error
    [n_k, Np]: the centres (x0 + x1) / 2 (one rounding, the halving is exact), their difference, two squares and a sum for the
    numerator, the same for the query's size ks = w^2 + h^2, the sum with 1e-8f, the division."""
    k, dk = _norm(kb, img_w, img_h)
    n, dn = _norm(nb, img_w, img_h)

    def centre(x, d, a):
        s = x[..., a] + x[..., a + 2]
        return s / 2, _rnd(s, d[..., a] + d[..., a + 2]) / 2

    def sumsq(a, da, b, db):
        p, dp = _prod(a, da, a, da)
        q, dq = _prod(b, db, b, db)
        return p + q, _rnd(p + q, dp + dq)
    kcx, dkcx = centre(k, dk, 0)
    kcy, dkcy = centre(k, dk, 1)
    ncx, dncx = centre(n, dn, 0)
    ncy, dncy = centre(n, dn, 1)
    dx, ddx = _diff(kcx, dkcx, ncx, dncx)
    dy, ddy = _diff(kcy, dkcy, ncy, dncy)
    num, dnum = sumsq(dx, ddx, dy, ddy)
    kw, dkw = _diff(k[..., 2], dk[..., 2], k[..., 0], dk[..., 0])
    kh, dkh = _diff(k[..., 3], dk[..., 3], k[..., 1], dk[..., 1])
    ks, dks = sumsq(kw, dkw, kh, dkh)
    den = ks + eps
    dden = _rnd(den, dks)
    dist = num / den
    return dist, _rnd(dist, (dnum + dist * dden) / (den - dden))


def gate_fp32(boxes, k_inds, nonk, img_w, img_h, max_center_dist):
    """The reference's own fp32 torch expression of the gate on the CPU (as tests/test_ops_gpu.py states it) -> bool [n_k, Np]."""
    nb = torch.as_tensor(np.asarray(boxes, np.float32)).clone()
    nb[:, [0, 2]] /= float(img_w)
    nb[:, [1, 3]] /= float(img_h)
    kb, ob = nb[torch.as_tensor(k_inds).long()], nb[torch.as_tensor(nonk).long()]
    k_ct = (kb[:, :2] + kb[:, 2:]) / 2
    k_s = ((kb[:, 2:] - kb[:, :2]) ** 2).sum(1)
    n_ct = (ob[:, :2] + ob[:, 2:]) / 2
    dist = ((k_ct[:, None] - n_ct[None]) ** 2).sum(2) / (k_s[:, None] + 1e-8)
    return (dist < float(max_center_dist)).numpy()


def split_meta(meta, n_k, Np, M):
    """meta (int32) = nonk[Np] | col_of[Np] | last_idx[M] | k_inds[n_k], as track_score_one reads it."""
    meta = np.asarray(meta)
    assert meta.shape == (2 * Np + M + n_k,)
    return meta[:Np], meta[Np:2 * Np], meta[2 * Np:2 * Np + M], meta[2 * Np + M:]


def track_score64(act, meta, decay, boxes, img_w, img_h, with_iou, max_center_dist, Np, M, valid=None):
    """Statement of gom_track_score_f32.  act = (exp, bound) of activate64 [n_k, N]; decay [Np] float32 or None; boxes [N, 4] px
    -> (exp, bound, gate), exp and bound float64 [n_k, M]:

        sum[i, m] = sum over {j : col_of[j] = m} of act[i, nonk[j]] decay[j]
                    bound: the propagated activation bound, sum_j dact decay[j], plus (members + 1) U sum: one rounding for the
                    product and the sequential fp32 accumulation of `members` terms
        iou[i, m] = IoU(box k_inds[i], box nonk[last_idx[m]])                        (iou64's bound; with_iou only)
        s = max(sum, iou)                       |max(a, b) - max(a', b')| <= max(da, db)
        s = 0 unless some member j of m has dist(i, j) < max_center_dist             (only with max_center_dist > 0)

    The gate is the only discontinuity.  gate = {"dist", "err" [n_k, Np] (gate64), "margin" = |dist - max_center_dist|,
    "undecided" = margin <= err, "valid" [n_k, Np]}; a decided pair's decision is the same on every side, and where the gate
    zeroes a score the bound is 0: the kernel writes exactly 0.  `valid` [n_k, Np]: decisions given from outside (the `exact`
    box kind takes them from gate_fp32) instead of dist < max_center_dist."""
    a, da = act
    n_k = a.shape[0]
    nonk, col_of, last_idx, k_inds = split_meta(meta, n_k, Np, M)
    boxes = np.asarray(boxes, np.float32)
    onehot = (col_of[:, None] == np.arange(M)[None]).astype(np.float64)              # [Np, M]
    dec = np.ones(Np) if decay is None else np.asarray(decay, np.float32).astype(np.float64)
    s = (a[:, nonk] * dec) @ onehot
    ds = (da[:, nonk] * dec) @ onehot
    ds = ds + (onehot.sum(0) + 1) * U * (s + ds)
    if with_iou:
        iou, diou = iou64(boxes[k_inds][:, None], boxes[nonk[last_idx]][None], img_w, img_h)
        s, ds = np.maximum(s, iou), np.maximum(ds, diou)
    gate = None
    mcd = float(np.float32(max_center_dist))
    if mcd > 0:
        dist, err = gate64(boxes[k_inds][:, None], boxes[nonk][None], img_w, img_h)
        margin = np.abs(dist - mcd)
        gate = {"dist": dist, "err": err, "margin": margin, "undecided": margin <= err,
                "valid": (dist < mcd) if valid is None else np.asarray(valid, bool)}
        keep = (gate["valid"].astype(np.float64) @ onehot) > 0
        s, ds = np.where(keep, s, 0.0), np.where(keep, ds, 0.0)
    return s, ds, gate


# ------------------------------------------------------------------------------------------ short-term pairs
def short_term64(tgt, mem, pairs, row_pair, boxes, img_w, img_h, with_iou, s_floats):
    """Statement of gom_short_term_pairs_f32.  tgt [rows, d], mem [*, d], boxes [*, 4] float32; pairs int32 [P, 6] = (first memory
    row, n_prev, n_cur, first tgt row, first box row, S offset); row_pair [rows] -> (exp, bound) float64 [s_floats], packed as the
    kernel packs them (row i of a pair at S offset + i n_prev); NaN where no row writes.

        l_j = tgt_i . mem_j over the PREVIOUS frame's rows j < n_prev only,  a = softmax with background (softmax_bg64, E_i),
        S[i, j] = max(a_j, IoU(box b0 + n_prev + i, box b0 + j))                                         (iou64; with_iou only)

        E_i = (4 ceil(d / 256) + 6) U max_j sum_k |tgt_ik mem_jk|

    a lane's chain of 4 ceil(d / 256) fused multiply-adds plus six butterfly steps: the absolute error of a logit."""
    tgt, mem = np.asarray(tgt, np.float32).astype(np.float64), np.asarray(mem, np.float32).astype(np.float64)
    boxes = np.asarray(boxes, np.float32)
    pairs = np.asarray(pairs).reshape(-1, 6)
    d = tgt.shape[1]
    exp, bound = np.full(s_floats, np.nan), np.full(s_floats, np.nan)
    for w in range(tgt.shape[0]):
        m0, n_prev, _, t0, b0, s_off = (int(v) for v in pairs[int(row_pair[w])])
        i = w - t0
        if n_prev == 0:
            continue
        k = mem[m0:m0 + n_prev]
        E = (4 * -(-d // 256) + 6) * U * (np.abs(tgt[w])[None] * np.abs(k)).sum(1).max()
        a, da = softmax_bg64(k @ tgt[w], E)
        if with_iou:
            iou, diou = iou64(boxes[b0 + n_prev + i][None], boxes[b0:b0 + n_prev], img_w, img_h)
            a, da = np.maximum(a, iou), np.maximum(da, diou)
        o = s_off + i * n_prev
        exp[o:o + n_prev], bound[o:o + n_prev] = a, da
    return exp, bound


# ------------------------------------------------------------------------------------------ inputs: logits
LOGIT_KINDS = ("randn", "overflow", "negative", "peaked", "equal")


def _rng(*key):
    return np.random.default_rng([int(k) for k in key])


def asso_logits(kind, n_k, offs, seed):
    """[n_k, N] float32.  randn: x 3.  overflow: x 200, exp without the max subtraction overflows.  negative: every logit about
    -100, the background takes all the weight and the outputs underflow.  peaked: one column per row and segment holds about half
    the weight.  equal: every logit 0.75."""
    N = int(offs[-1])
    g = _rng(seed, LOGIT_KINDS.index(kind))
    x = g.standard_normal((n_k, N))
    if kind == "randn":
        x = 3 * x
    elif kind == "overflow":
        x = 200 * x
    elif kind == "negative":
        x = -100 + 0.25 * x
    elif kind == "equal":
        x = np.full((n_k, N), 0.75)
    else:
        x = 0.5 * x
        for t in range(len(offs) - 1):
            lo, hi = int(offs[t]), int(offs[t + 1])
            if hi - lo >= 2:
                j = lo + g.integers(0, hi - lo, n_k)
                x[np.arange(n_k), j] = -np.inf
                x[np.arange(n_k), j] = np.log(np.exp(x[:, lo:hi]).sum(1) + 1.0)
    return x.astype(np.float32)


# ------------------------------------------------------------------------------------------ inputs: boxes
BOX_KINDS = ("random", "exact")
RANDOM_IMAGE = (128.0, 96.0)                          # (img_w, img_h): not square
GRID = 64.0                                           # exact kind: coordinates k / 64 in [0, 16), image 1 x 1: 10 bits each, so the
                                                      # squares and products of differences (22 bits) and their sums are exact in fp32


def _random_box(g, kind):
    if kind == "exact":                               # x0 in [0, 4], sides in [0.5, 3]: k / 64; a query side of 0.5 and more absorbs 1e-8f
        x0, y0 = g.integers(0, 257, 2) / GRID
        w, h = g.integers(32, 193, 2) / GRID
    else:                                             # sides from 3 % of the coordinate
        x0, y0 = g.uniform(8, 0.75 * RANDOM_IMAGE[0]), g.uniform(8, 0.75 * RANDOM_IMAGE[1])
        w, h = x0 * g.uniform(0.03, 0.4), y0 * g.uniform(0.03, 0.4)
    return np.array([x0, y0, x0 + w, y0 + h])


def _jitter(g, box, kind):
    """The box moved by up to 40 % of its sides: an overlapping pair."""
    w, h = box[2] - box[0], box[3] - box[1]
    sx, sy = g.uniform(-0.4, 0.4) * w, g.uniform(-0.4, 0.4) * h
    if kind == "exact":
        sx, sy = np.round(sx * GRID) / GRID, np.round(sy * GRID) / GRID
        sx, sy = max(sx, -box[0]), max(sy, -box[1])
    return box + np.array([sx, sy, sx, sy])


def _touching(box):
    """The same box moved right by its width: shares an edge, IoU 0."""
    w = box[2] - box[0]
    return box + np.array([w, 0, w, 0])


def image_of(kind):
    return (1.0, 1.0) if kind == "exact" else RANDOM_IMAGE


# ------------------------------------------------------------------------------------------ cases: activate + track score
class AssoCase:
    """One match: T frame segments of lengths `segs`, the query frame `k` (n_k = segs[k] current detections), M tracks over the
    Np = N - n_k other detections.  Built once, seeded by the case's index.

    Tracks: track 0 has ONE member, j = 0 (for M >= 2); track 1 has a member in every non-empty history frame; every track has
    at least one member; the rest is drawn.  decay: distinct per-j values in [0.5, 1) or None.
    Planted boxes (with_gate = max_center_dist > 0), all relative to the current detections' boxes:
      j = 0 against query 0  (M >= 2; with one track j = 0 overlaps query 0 instead, or every score would be 0)
                             random: a box of twice the query's size, straight below it at dist = 1.5 max_center_dist -- invalid;
                                     valid under swapped image sides (dist x 0.33) and under the candidate's own size (dist / 4)
                             exact:  dist == max_center_dist exactly in fp32 (1 / 2 for 0.5, 25 / 0.5 for 50): invalid, `<` is strict
      last member of track 1 an overlapping copy of query 1 % n_k, its FIRST member far away
      last member of track 2 identical to query 0 (IoU exactly 1)
      last member of track 3 touching query 0 (IoU exactly 0 in the exact kind)
    Half of the other candidates overlap a query box, half are drawn freely (mostly disjoint)."""

    def __init__(self, index, name, segs, k, M, decay, with_iou, mcd, pad):
        self.index, self.id, self.segs, self.k, self.M = index, name, list(segs), k, M
        self.with_iou, self.mcd, self.pad = with_iou, float(mcd), pad
        self.T = len(segs)
        self.offs = np.concatenate([[0], np.cumsum(segs)]).astype(np.int32)
        self.N = int(self.offs[-1])
        self.lo, self.hi = int(self.offs[k]), int(self.offs[k + 1])
        self.n_k, self.Np = self.hi - self.lo, self.N - (self.hi - self.lo)
        self.ld = self.N + pad
        self.k_inds = np.arange(self.lo, self.hi)
        self.nonk = np.concatenate([np.arange(0, self.lo), np.arange(self.hi, self.N)]).astype(np.int64)
        g = _rng(1000 + index)
        Np = self.Np
        frame_of = np.searchsorted(self.offs, self.nonk, side="right") - 1
        col = np.full(Np, -1)
        if Np:
            assert 1 <= M <= Np
            if M == 1:
                col[:] = 0
            else:
                col[0] = 0
                for f in np.unique(frame_of):                                          # track 1: a member in every frame
                    free = np.nonzero((frame_of == f) & (col < 0))[0]
                    if len(free):
                        col[free[-1]] = 1
                if not (col == 1).any():
                    col[Np - 1] = 1
                free = g.permutation(np.nonzero(col < 0)[0])
                assert len(free) >= M - 2
                col[free[:M - 2]] = np.arange(2, M)
                col[free[M - 2:]] = g.integers(1, M, len(free) - (M - 2))
        self.col_of = col
        self.last_idx = np.array([np.nonzero(col == m)[0].max() if (col == m).any() else 0 for m in range(M)], np.int64)
        self.first_idx = np.array([np.nonzero(col == m)[0].min() if (col == m).any() else 0 for m in range(M)], np.int64)
        self.meta = np.concatenate([self.nonk, self.col_of, self.last_idx, self.k_inds]).astype(np.int32)
        self.decay = (0.5 + 0.5 * g.random(Np)).astype(np.float32) if decay else None
        self._boxes = {}

    def logits(self, kind):
        return asso_logits(kind, self.n_k, self.offs, 2000 + self.index)

    def gate_valid(self, box_kind):
        """The decisions the expected values use: None (the statement's own) for random boxes, gate_fp32's for exact ones."""
        if box_kind != "exact" or self.mcd <= 0 or self.Np == 0:
            return None
        img_w, img_h = image_of(box_kind)
        b = self.boxes(box_kind)
        v32 = gate_fp32(b, self.k_inds, self.nonk, img_w, img_h, self.mcd)
        # fp64 agrees with fp32 on every pair once the 1e-8 that fp32 absorbs is left out of the fp64 sum as well ...
        exact, _ = gate64(b[self.k_inds][:, None], b[self.nonk][None], img_w, img_h, eps=0.0)
        assert bool(((exact < self.mcd) == v32).all()), "exact boxes: fp32 and fp64 decide a gate pair differently"
        # ... and with it only the pairs planted at dist == max_center_dist change sides
        dist, _ = gate64(b[self.k_inds][:, None], b[self.nonk][None], img_w, img_h)
        assert bool((exact[(dist < self.mcd) != v32] == self.mcd).all())
        return v32

    def boxes(self, kind):
        """[N, 4] float32 px; for the random kind a candidate's box is drawn again until no gate pair is undecided."""
        if kind in self._boxes:
            return self._boxes[kind]
        g = _rng(3000 + self.index, BOX_KINDS.index(kind))
        img_w, img_h = image_of(kind)
        b = np.stack([_random_box(g, kind) for _ in range(self.N)])
        fixed = np.zeros(self.N, bool)
        fixed[self.k_inds] = True
        q = self.k_inds
        gated = self.mcd > 0
        if gated:                                                                      # query 0 and j = 0
            if kind == "exact":
                b[q[0]] = [1, 1, 2, 2] if self.mcd == 0.5 else [0.5, 0.5, 1, 1]
            else:
                s = np.sqrt(0.5 / self.mcd)
                b[q[0]] = [40, 30, 40 + 30 * s, 30 + 6 * s]
        if self.Np:
            def put(j, box):
                b[self.nonk[j]] = box
                fixed[self.nonk[j]] = True
            if gated and self.M == 1:                                                  # one track: a valid member, or every score is 0
                put(0, _jitter(g, b[q[0]], kind))
            elif gated:
                qb = b[q[0]]
                cx, cy = (qb[0] + qb[2]) / 2, (qb[1] + qb[3]) / 2
                if kind == "exact":
                    assert self.mcd in (0.5, 50.0)
                    cx, cy = (cx + 1, cy) if self.mcd == 0.5 else (cx + 3, cy + 4)
                    put(0, [cx - 0.5, cy - 0.5, cx + 0.5, cy + 0.5])
                else:
                    w, h = qb[2] - qb[0], qb[3] - qb[1]
                    ks = (w / img_w) ** 2 + (h / img_h) ** 2
                    cy = cy + img_h * np.sqrt(1.5 * self.mcd * ks)
                    put(0, [cx - w, cy - h, cx + w, cy + h])
            if self.M >= 2:
                put(self.last_idx[1], _jitter(g, b[q[1 % self.n_k]], kind))
                if self.first_idx[1] != self.last_idx[1] and self.first_idx[1] != 0:
                    far = b[q[1 % self.n_k]] + (np.array([4, 4, 4, 4]) if kind == "exact" else np.array([70, 50, 70, 50]))
                    put(self.first_idx[1], far)
            if self.M >= 3:
                put(self.last_idx[2], b[q[0]].copy())
            if self.M >= 4:
                put(self.last_idx[3], _touching(b[q[0]]))
            for j in range(self.Np):
                if not fixed[self.nonk[j]] and g.random() < 0.5:
                    b[self.nonk[j]] = _jitter(g, b[q[g.integers(0, self.n_k)]], kind)
        b = b.astype(np.float32)
        if kind == "random" and gated and self.Np:
            for _ in range(100):
                dist, err = gate64(b[self.k_inds][:, None], b[self.nonk][None], img_w, img_h)
                bad = np.nonzero((np.abs(dist - self.mcd) <= err).any(0))[0]
                if not len(bad):
                    break
                for j in bad:
                    assert not fixed[self.nonk[j]], "a planted box is undecided"
                    b[self.nonk[j]] = _random_box(g, kind).astype(np.float32)
        if kind == "exact":
            assert bool((b * GRID == np.round(b * GRID)).all()) and float(b.min()) >= 0 and float(b.max()) < 16
        self._boxes[kind] = b
        return b

    def expected(self, logit_kind, box_kind):
        """-> (act exp, act bound), (traj exp, traj bound, gate) of the case's inputs."""
        act = activate64(self.logits(logit_kind), self.offs)
        img_w, img_h = image_of(box_kind)
        return act, track_score64(act, self.meta, self.decay, self.boxes(box_kind), img_w, img_h, self.with_iou, self.mcd,
                                  self.Np, self.M, valid=self.gate_valid(box_kind))


def _asso_cases():
    # name, segment lengths, query frame, M, decay, with_iou, max_center_dist, ld - N
    rows = [
        ("T1-nohistory", [5], 0, 1, False, 0, 0.0, 0),               # N = n_k: the sum over no members is 0
        ("T2-one", [1, 1], 1, 1, True, 1, 0.5, 0),                   # one track with one member at j = 0
        ("T2-130", [130, 1], 1, 2, True, 1, 0.5, 0),
        ("T5-empty-first-middle", [0, 63, 0, 64, 4], 4, 2, True, 1, 50.0, 3),
        ("T5-empty-last-M255", [65, 130, 63, 3, 0], 3, 255, False, 1, 0.5, 0),
        ("T4-middle-M257", [130, 65, 5, 65], 2, 257, True, 1, 0.5, 5),          # nonk is not the identity; threads loop over tracks
        ("T9-middle-M256", [1, 63, 0, 64, 4, 65, 0, 1, 130], 4, 256, True, 1, 50.0, 1),   # waves loop over segments
        ("T9-last-nogate", [64, 1, 0, 63, 65, 1, 130, 0, 3], 8, 5, False, 0, 0.0, 0),
        ("T4-noiou-gate", [64, 0, 65, 4], 3, 4, True, 0, 0.5, 2),
    ]
    return [AssoCase(i, *r) for i, r in enumerate(rows)]


ASSO_CASES = _asso_cases()


# ------------------------------------------------------------------------------------------ cases: short-term pairs
class ShortCase:
    """One ragged launch: pairs (n_prev, n_cur); per pair the memory and box rows are prev | cur, the tgt rows follow pair by pair,
    S is packed [n_cur, n_prev] pair by pair (modeling/roi_heads.py builds the descriptors the same way).

    Inputs: channel 0 of tgt is 1 and channel 0 of a memory row its base logit; the other channels add N(0, sigma^2) to the logit.
    randn: base 0, sigma 3.  overflow: sigma 200.  negative: base -100, sigma 0.25.  peaked: sigma 0.5, one previous row per pair
    with base ln(1.13 n_prev + 1).  equal: sigma 0, base 0.75.  The current frame's own memory rows have base 0.
    Boxes: current detection 0 overlaps previous 0, 1 is identical to previous 1 % n_prev, 2 touches previous 2 % n_prev, the
    others overlap a drawn previous box; the previous boxes are drawn freely."""

    def __init__(self, index, name, d, pairs, with_iou):
        self.index, self.id, self.d, self.np_nc, self.with_iou = index, name, d, list(pairs), with_iou
        desc, row_pair, off, cur_off, s_off = [], [], 0, 0, 0
        for p, (n_prev, n_cur) in enumerate(pairs):
            desc.append([off, n_prev, n_cur, cur_off, off, s_off])
            row_pair += [p] * n_cur
            off, cur_off, s_off = off + n_prev + n_cur, cur_off + n_cur, s_off + n_prev * n_cur
        self.pairs = np.array(desc, np.int32)
        self.row_pair = np.array(row_pair, np.int32)
        self.mem_rows, self.rows, self.s_floats = off, cur_off, s_off
        self.max_prev = max(p[0] for p in pairs)

    def inputs(self, kind):
        g = _rng(4000 + self.index, LOGIT_KINDS.index(kind))
        sigma = {"randn": 3.0, "overflow": 200.0, "negative": 0.25, "peaked": 0.5, "equal": 0.0}[kind]
        tgt = g.standard_normal((self.rows, self.d)) * (sigma / np.sqrt(self.d - 1))
        mem = g.standard_normal((self.mem_rows, self.d))
        tgt[:, 0] = 1.0
        mem[:, 0] = 0.0
        for m0, n_prev, n_cur, _, _, _ in self.pairs:
            if kind == "negative":
                mem[m0:m0 + n_prev, 0] = -100.0
            elif kind == "equal":
                mem[m0:m0 + n_prev, 0] = 0.75
            elif kind == "peaked" and n_prev >= 2:
                mem[m0 + g.integers(0, n_prev), 0] = np.log(1.13 * n_prev + 1)
        return tgt.astype(np.float32), mem.astype(np.float32)

    def boxes(self, kind):
        g = _rng(5000 + self.index, BOX_KINDS.index(kind))
        b = np.stack([_random_box(g, kind) for _ in range(self.mem_rows)])
        for m0, n_prev, n_cur, _, _, _ in self.pairs:
            for i in range(n_cur):
                r = m0 + n_prev + i
                if i == 1:
                    b[r] = b[m0 + 1 % n_prev]
                elif i == 2:
                    b[r] = _touching(b[m0 + 2 % n_prev])
                else:
                    b[r] = _jitter(g, b[m0 + (0 if i == 0 else g.integers(0, n_prev))], kind)
        b = b.astype(np.float32)
        if kind == "exact":
            assert bool((b * GRID == np.round(b * GRID)).all()) and float(b.min()) >= 0 and float(b.max()) < 16
        return b

    def expected(self, logit_kind, box_kind):
        tgt, mem = self.inputs(logit_kind)
        img_w, img_h = image_of(box_kind)
        return short_term64(tgt, mem, self.pairs, self.row_pair, self.boxes(box_kind), img_w, img_h, self.with_iou, self.s_floats)


def _short_cases():
    # name, d, (n_prev, n_cur) per pair, with_iou.  9 and 13 rows are no multiple of the 4 rows of a workgroup; the last pair of d4
    # (rows 4..8) and the third of d256 (rows 9..11) straddle two workgroups.
    rows = [
        ("d4", 4, [(1, 1), (2, 3), (63, 5)], 1),
        ("d252", 252, [(64, 4), (65, 3), (128, 1)], 0),
        ("d256", 256, [(129, 5), (2, 4), (319, 3), (1, 1)], 1),
        ("d260", 260, [(320, 3), (65, 4), (64, 5)], 1),
        ("d1024", 1024, [(63, 1), (320, 4), (129, 5)], 0),
    ]
    return [ShortCase(i, *r) for i, r in enumerate(rows)]


SHORT_CASES = _short_cases()


# ------------------------------------------------------------------------------------------ cases: gathers
class GatherCase:
    """gom_gather_match_f32: rows [N] into a pool [R, ld_pool] (ld_pool > d) and projections [R, ld_proj] (ld_proj > 4 d: q | k | v of
    the encoder, then the decoder's query projection at column 3 d); repeated and non-monotone rows.  Exact: torch indexing."""

    def __init__(self, index, N, n_k, lo, d):
        self.index, self.N, self.n_k, self.lo, self.d = index, N, n_k, lo, d
        self.id = "N%d-nk%d-lo%d-d%d" % (N, n_k, lo, d)
        self.R, self.ld_pool, self.ld_proj = N + 3, d + 8, 4 * d + 12
        g = _rng(6000 + index)
        self.rows = g.integers(0, self.R, N).astype(np.int32)
        if N >= 5:
            self.rows[:5] = [4, 1, 1, self.R - 1, 0]                                   # repeated, non-monotone, first and last row

    def inputs(self):
        """pool and proj as flat float32 buffers [R ld]: the gap columns hold NaN."""
        g = _rng(6500 + self.index)
        pool = np.full((self.R, self.ld_pool), np.nan, np.float32)
        proj = np.full((self.R, self.ld_proj), np.nan, np.float32)
        pool[:, :self.d] = g.standard_normal((self.R, self.d))
        proj[:, :4 * self.d] = g.standard_normal((self.R, 4 * self.d))
        return pool, proj

    def expected(self, pool, proj):
        r, d = self.rows.astype(np.int64), self.d
        return pool[r, :d], proj[r, :3 * d], proj[r[self.lo:self.lo + self.n_k], 3 * d:4 * d]


def _gather_cases():
    rows = [(1, 1, 0, 4), (1, 0, 0, 1024), (5, 0, 5, 4), (5, 1, 4, 1024), (5, 5, 0, 4), (70, 1, 0, 4), (70, 1, 69, 1024), (70, 70, 0, 4),
            (70, 0, 0, 4), (70, 5, 65, 4)]
    return [GatherCase(i, *r) for i, r in enumerate(rows)]


GATHER_CASES = _gather_cases()
