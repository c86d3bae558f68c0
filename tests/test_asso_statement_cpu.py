"""CPU: the fp64 statements of tests/asso_statement.py (activate64, track_score64, short_term64 and their element-wise bounds) are the
yardstick of test_asso_forms_gpu.py.  On every input set of the GPU file (same generators, same seeds: the same bits) this file shows

  * the bounds are not vacuous: a numpy fp32 evaluation in the kernels' own order -- lane-strided partial sums, the xor butterfly,
    the sequential track sum, the lane's multiply-add chain -- lies within `bound` everywhere (worst ratio per form printed);
  * the bounds are not loose: the same fp32 evaluation with each planted mistake of the issue in it leaves the bound on at least one
    element, in every case and input kind in which the mistake exists at all;
  * no gate pair of the `random` boxes is undecided, and the `exact` boxes have the properties their name promises.

Which case can show a mistake is arithmetic, not choice, and is written next to each mistake: a softmax over the whole row needs two
non-empty segments; nonk mistakes need a query frame in the middle of the window; a gate mistake needs the gate; the activation
mistakes of the track score are looked for on the `randn` logits (the `negative` ones make every activation underflow and the
`overflow` ones make them one-hot, so a sum over them need not move)."""
import numpy as np
import pytest

from asso_statement import (ASSO_CASES, BOX_KINDS, GATHER_CASES, LOGIT_KINDS, SHORT_CASES, activate64, gate64, gate_fp32,
                            image_of, iou64, softmax_bg64, U)

f32 = np.float32
WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for k, v in sorted(WORST.items()):
        print("association fp32 emulation worst |emu-exp| / bound  %-14s %.4f" % (k, v))


def _outside(got, exp, bound):
    """Number of elements of `got` that are not within the bound of exp (NaN on one side only counts)."""
    got, own = np.asarray(got, np.float64), ~np.isnan(exp)
    bad = own & ~(np.abs(got - np.where(own, exp, 0)) <= np.where(own, bound, 0))
    return int(bad.sum()) + int((~own & ~np.isnan(got)).sum())


def _inside(form, got, exp, bound, what):
    assert _outside(got, exp, bound) == 0, "%s: the fp32 evaluation leaves the bound" % (what,)
    own = ~np.isnan(exp) & (bound > 0)
    if own.any():
        WORST[form] = max(WORST.get(form, 0.0), float((np.abs(np.asarray(got, np.float64) - exp)[own] / bound[own]).max()))


# ------------------------------------------------------------------------------------------ the kernels' order in numpy fp32
def _butterfly(v):
    """wave_sum: v [..., 64] -> [...]; v += v[lane ^ o] for o = 32 .. 1."""
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[..., lane ^ o]
    return v[..., 0]


def _lane_sum(e):
    """e [r, n] -> [r]: lane l adds its columns l, l + 64, ... in order, then the butterfly."""
    r, n = e.shape
    c = -(-n // 64)
    p = np.zeros((r, c * 64), e.dtype)
    p[:, :n] = e
    p = p.reshape(r, c, 64)
    acc = np.zeros((r, 64), e.dtype)
    for i in range(c):
        acc = acc + p[:, i]
    return _butterfly(acc)


def _softmax_bg32(x, mistake=None, extra=None):
    """x [r, n] fp32 -> the segment's activations as asso_activate_kernel computes them."""
    mx = np.maximum(x.max(1), f32(0))
    if extra is not None:
        mx = np.maximum(mx, extra.max(1))
    e = np.exp(x - mx[:, None])
    es = e[:, :64] if mistake == "first 64 columns only" else e
    if extra is not None:
        es = np.concatenate([es, np.exp(extra - mx[:, None])], 1)
    s = _lane_sum(es)
    if mistake != "no background":
        s = s + np.exp(f32(0) - mx)
    return e / s[:, None]


def emu_activate(logits, offs, mistake=None):
    L = np.asarray(logits, f32)
    out = np.full(L.shape, np.nan, f32)
    N = L.shape[1]
    segs = [(int(offs[t]), int(offs[t + 1])) for t in range(len(offs) - 1)]
    if mistake == "whole row":
        segs = [(segs[0][0], segs[-1][1])]
    for lo, hi in segs:
        if mistake == "end + 1":
            hi = min(hi + 1, N)
        elif mistake == "end - 1":
            hi -= 1
        if hi > lo:
            out[:, lo:hi] = _softmax_bg32(L[:, lo:hi], mistake)
    return out


def _iou32(kb, lb):
    """kb [n, 1, 4], lb [1, m, 4] normalised fp32 -> [n, m] as track_score_one computes it."""
    w = np.maximum(np.minimum(kb[..., 2], lb[..., 2]) - np.maximum(kb[..., 0], lb[..., 0]), f32(0))
    h = np.maximum(np.minimum(kb[..., 3], lb[..., 3]) - np.maximum(kb[..., 1], lb[..., 1]), f32(0))
    inter = w * h
    a1 = (kb[..., 2] - kb[..., 0]) * (kb[..., 3] - kb[..., 1])
    a2 = (lb[..., 2] - lb[..., 0]) * (lb[..., 3] - lb[..., 1])
    return np.where(inter > 0, inter / np.where(inter > 0, a1 + a2 - inter, f32(1)), f32(0)).astype(f32)


def emu_track(act, c, boxes, img_w, img_h, mistake=None):
    """track_score_one over all (i, m) in fp32: the members of a track are added in the order of j."""
    iw, ih = (f32(img_h), f32(img_w)) if mistake == "image sides swapped" else (f32(img_w), f32(img_h))
    nb = np.asarray(boxes, f32) / np.array([iw, ih, iw, ih], f32)
    kb = nb[c.k_inds]
    kcx, kcy = (kb[:, 0] + kb[:, 2]) / f32(2), (kb[:, 1] + kb[:, 3]) / f32(2)
    ks = (kb[:, 2] - kb[:, 0]) * (kb[:, 2] - kb[:, 0]) + (kb[:, 3] - kb[:, 1]) * (kb[:, 3] - kb[:, 1])
    s = np.zeros((c.n_k, c.M), f32)
    valid = np.zeros((c.n_k, c.M), bool)
    mcd = f32(c.mcd)
    for j in range(c.Np):
        m = c.col_of[j]
        a = act[:, j if mistake == "act[j]" else c.nonk[j]]
        if c.decay is not None and mistake != "decay ignored":
            a = a * c.decay[c.nonk[j] % c.Np if mistake == "decay[nonk[j]]" else j]
        s[:, m] = s[:, m] + a
        if mcd > 0:
            n = nb[c.nonk[j]]
            dx, dy = kcx - (n[0] + n[2]) / f32(2), kcy - (n[1] + n[3]) / f32(2)
            size = ks
            if mistake == "gate on the candidate's size":
                size = (n[2] - n[0]) * (n[2] - n[0]) + (n[3] - n[1]) * (n[3] - n[1])
            dist = (dx * dx + dy * dy) / (size + f32(1e-8))
            valid[:, m] |= (dist <= mcd) if mistake == "<= in the gate" else (dist < mcd)
    assert s.dtype == f32
    if c.with_iou:
        rows = c.nonk[c.last_idx]
        if mistake == "last_idx without nonk":
            rows = c.last_idx
        elif mistake == "first member's box":
            rows = c.nonk[c.first_idx]
        iou = _iou32(kb[:, None], nb[rows][None])
        s = s + iou if mistake == "sum with the IoU" else np.maximum(s, iou)
    if mcd > 0:
        s[~valid] = 0
    return s


def emu_short(c, tgt, mem, boxes, img_w, img_h, mistake=None):
    """short_term_pairs_kernel in fp32: a lane's chain of fused multiply-adds (through fp64: the product is exact there), the
    butterfly, the softmax over the lane-strided logits."""
    S = np.full(c.s_floats, np.nan, f32)
    nb = np.asarray(boxes, f32) / np.array([f32(img_w), f32(img_h)] * 2, f32)
    d = c.d
    steps = -(-d // 256)
    for w in range(c.rows):
        p = int(c.row_pair[w])
        m0, n_prev, n_cur, t0, b0, s_off = (int(v) for v in c.pairs[p])
        if mistake == "S offset of the next pair":
            s_off = int(c.pairs[(p + 1) % len(c.pairs)][5])
        i = w - t0
        n_log = n_prev + n_cur if mistake == "own rows in the softmax" else n_prev
        x = np.zeros(steps * 256, np.float64)
        x[:d] = tgt[w]
        y = np.zeros((n_log, steps * 256), np.float64)
        y[:, :d] = mem[m0:m0 + n_log]
        xs, ys = x.reshape(steps, 64, 4), y.reshape(n_log, steps, 64, 4)
        acc = np.zeros((n_log, 64), f32)
        for st in range(steps):
            for q in range(4):
                acc = (xs[st, :, q] * ys[:, st, :, q] + acc.astype(np.float64)).astype(f32)
        lg = _butterfly(acc)
        extra = lg[None, n_prev:] if n_log > n_prev else None
        lg = lg[None, :n_prev]
        if mistake == "second chunk dropped" and n_prev > 64:
            keep = np.r_[0:64, 128:n_prev] if n_prev > 128 else np.r_[0:64]
            a = np.full(n_prev, np.nan, f32)
            mx = np.maximum(lg.max(1), f32(0))
            e = np.exp(lg[:, keep] - mx[:, None])
            with np.errstate(invalid="ignore"):                                        # 0 / 0 where the dropped chunk held the maximum
                a[keep] = (e / (_lane_sum(e) + np.exp(f32(0) - mx))[:, None])[0]
        else:
            a = _softmax_bg32(lg, mistake, extra)[0]
        if c.with_iou:
            kb = nb[b0 + i if mistake == "query box at b0 + i" else b0 + n_prev + i]
            a = np.fmax(a, _iou32(kb[None, None], nb[b0:b0 + n_prev][None])[0]) if mistake != "second chunk dropped" else \
                np.where(np.isnan(a), a, np.maximum(a, _iou32(kb[None, None], nb[b0:b0 + n_prev][None])[0]))
        stride = n_cur if mistake == "row stride n_cur" else n_prev
        o = s_off + i * stride
        S[o:o + n_prev] = a[:max(0, min(n_prev, c.s_floats - o))]
    return S


# ------------------------------------------------------------------------------------------ hand-made pins of the statements
def test_activate_by_hand():
    l = np.array([[0.0, 0.0, 1.0, -2.0, 5.0]], f32)
    exp, bound = activate64(l, [0, 2, 2, 4, 4])                       # segments {0, 1}, {}, {2, 3}, {}: column 4 is nobody's
    assert np.allclose(exp[0, :2], 1 / 3, rtol=1e-15)
    e = np.exp([1.0, -2.0])
    assert np.allclose(exp[0, 2:4], e / (e.sum() + 1), rtol=1e-15)
    assert np.isnan(exp[0, 4]) and np.isnan(bound[0, 4])
    # equal logits 0, n = 2: r = EXPF U, rbar = EXPF U, ceil(2 / 64) + 8 = 9 -> 17 U
    assert np.allclose(bound[0, :2], np.expm1(17 * U) / 3 + 2.0 ** -126, rtol=1e-12)


def test_iou_and_gate_by_hand():
    k = np.array([[0, 0, 2, 2]], f32)
    iou, d = iou64(k[:, None], np.array([[[1, 1, 3, 3], [2, 0, 4, 2], [0, 0, 2, 2], [5, 5, 6, 6]]], f32), 1.0, 1.0)
    assert np.allclose(iou[0], [1 / 7, 0, 1, 0], rtol=1e-15)
    assert bool((d > 0).all()) and bool((d < 1e-5).all())
    dist, err = gate64(k[:, None], np.array([[[2, 0, 4, 2]]], f32), 1.0, 1.0, eps=0.0)
    assert dist[0, 0] == 0.5 and 0 < err[0, 0] < 1e-5                    # dx = 2, ks = 8


# ------------------------------------------------------------------------------------------ activate
def _segments(c):
    return [(int(c.offs[t]), int(c.offs[t + 1])) for t in range(c.T)]


# mistake -> (the logit kinds it is looked for in, the cases that can show it)
ACTIVATE_MISTAKES = {
    # the background weighs e^-m: nothing next to an overflowing logit
    "no background": (("randn", "negative", "peaked", "equal"), lambda c: True),
    "whole row": (("randn", "peaked", "equal"), lambda c: sum(hi > lo for lo, hi in _segments(c)) >= 2),
    # the column after a segment's end exists unless every later segment is empty
    "end + 1": (("randn", "peaked", "equal"), lambda c: any(lo < hi < c.N for lo, hi in _segments(c))),
    "end - 1": (LOGIT_KINDS, lambda c: True),
    # (on the `negative` logits the whole segment is nothing next to the background's weight)
    "first 64 columns only": (("randn", "peaked", "equal"), lambda c: any(hi - lo > 64 for lo, hi in _segments(c))),
}


@pytest.mark.parametrize("case", ASSO_CASES, ids=[c.id for c in ASSO_CASES])
def test_activate_bound(case):
    for kind in LOGIT_KINDS:
        l = case.logits(kind)
        exp, bound = activate64(l, case.offs)
        own = ~np.isnan(exp)
        assert bool(own.all()) and bool(np.isfinite(bound).all()) and bool((bound > 0).all())
        if kind == "overflow":
            assert float(l.max()) > 89                                                 # expf overflows without the subtraction
        if kind == "negative":
            assert float(exp.max()) < 2.0 ** -126                                      # every output underflows
        if kind == "peaked":
            for lo, hi in _segments(case):
                if hi - lo >= 2:
                    assert 0.4 < float(exp[:, lo:hi].max(1).min()) < 0.6
        _inside("activate", emu_activate(l, case.offs), exp, bound, "%s %s" % (case.id, kind))
        for name, (kinds, exists) in ACTIVATE_MISTAKES.items():
            if kind in kinds and exists(case):
                assert _outside(emu_activate(l, case.offs, name), exp, bound) > 0, "%s %s: '%s' stays inside the bound" % (
                    case.id, kind, name)


# ------------------------------------------------------------------------------------------ track score
def _middle(c):
    return bool((c.nonk != np.arange(c.Np)).any())


# mistake -> (box kinds, the cases that can show it); all on the `randn` logits
TRACK_MISTAKES = {
    # (T2-one is a single pair of overlapping boxes: its IoU hides the sum)
    "decay ignored": (BOX_KINDS, lambda c: c.decay is not None and c.Np > 1),
    "decay[nonk[j]]": (BOX_KINDS, lambda c: c.decay is not None and _middle(c)),
    "act[j]": (BOX_KINDS, _middle),
    "last_idx without nonk": (BOX_KINDS, lambda c: c.with_iou and _middle(c)),
    # (with M = 2 track 1 holds all detections but one: its sum is about the number of frames and no IoU reaches it)
    "first member's box": (BOX_KINDS, lambda c: c.with_iou and c.M >= 3 and c.first_idx[1] != c.last_idx[1]),
    "<= in the gate": (("exact",), lambda c: c.mcd > 0 and c.M >= 2),
    "gate on the candidate's size": (("random",), lambda c: c.mcd > 0 and c.M >= 2),
    "image sides swapped": (("random",), lambda c: c.mcd > 0 and c.M >= 2),
    "sum with the IoU": (BOX_KINDS, lambda c: c.with_iou and c.Np > 0),
}


@pytest.mark.parametrize("box_kind", BOX_KINDS)
@pytest.mark.parametrize("case", ASSO_CASES, ids=[c.id for c in ASSO_CASES])
def test_track_score_bound(case, box_kind):
    boxes = case.boxes(box_kind)
    img_w, img_h = image_of(box_kind)
    for kind in LOGIT_KINDS:
        (aexp, abound), (exp, bound, gate) = case.expected(kind, box_kind)
        assert exp.shape == (case.n_k, case.M) and bool(np.isfinite(exp).all()) and bool(np.isfinite(bound).all())
        act32 = emu_activate(case.logits(kind), case.offs)
        _inside("track score", emu_track(act32, case, boxes, img_w, img_h), exp, bound, "%s %s %s" % (case.id, kind, box_kind))
        if gate is not None and box_kind == "random":
            assert int(gate["undecided"].sum()) == 0
            assert exp[0, 0] == 0 or case.M == 1, "the planted pair (query 0, j = 0) is invalid"
        if kind != "randn":
            continue
        for name, (kinds, exists) in TRACK_MISTAKES.items():
            if box_kind in kinds and exists(case):
                assert _outside(emu_track(act32, case, boxes, img_w, img_h, name), exp, bound) > 0, \
                    "%s %s: '%s' stays inside the bound" % (case.id, box_kind, name)


@pytest.mark.parametrize("case", [c for c in ASSO_CASES if c.mcd > 0 and c.M >= 2], ids=lambda c: c.id)
def test_exact_boxes_are_exact(case):
    """The exact kind: fp32 and fp64 decide every gate pair alike except where the absorbed 1e-8 alone separates them -- the
    planted pair (query 0, j = 0), whose dist equals max_center_dist in fp32 and is therefore invalid; the IoU of the planted
    identical boxes is exactly 1, of the touching ones exactly 0, in fp32 as in fp64."""
    b = case.boxes("exact")
    v32 = gate_fp32(b, case.k_inds, case.nonk, 1.0, 1.0, case.mcd)
    dist, _ = gate64(b[case.k_inds][:, None], b[case.nonk][None], 1.0, 1.0)
    dist0, _ = gate64(b[case.k_inds][:, None], b[case.nonk][None], 1.0, 1.0, eps=0.0)
    assert bool(((dist0 < case.mcd) == v32).all()), "fp32 and fp64 differ by more than the absorbed 1e-8"
    differ = (dist < case.mcd) != v32
    assert bool(differ[0, 0]) and dist0[0, 0] == case.mcd and not v32[0, 0]
    assert bool((dist0[differ] == case.mcd).all())
    # every fp32 operation of the gate is exact: the fp32 distance times ks is the fp64 numerator
    kb = b[case.k_inds]
    assert float(((kb[:, 2:] - kb[:, :2]) ** 2).sum(1).min()) >= 0.5                  # ks + 1e-8f == ks
    if case.with_iou:
        nb = b.astype(f32)
        iou32 = _iou32(nb[case.k_inds][:, None], nb[case.nonk[case.last_idx]][None])
        iou, _ = iou64(b[case.k_inds][:, None], b[case.nonk[case.last_idx]][None], 1.0, 1.0)
        assert bool((np.abs(iou32 - iou) <= U * iou).all())                          # only the division rounds
        if case.M >= 3:
            assert iou32[0, 2] == 1.0 and iou[0, 2] == 1.0
        if case.M >= 4:
            assert iou32[0, 3] == 0.0 and iou[0, 3] == 0.0


def test_the_case_table_covers_the_issue():
    segs = {n for c in ASSO_CASES for i, n in enumerate(c.segs) if i != c.k}
    assert segs >= {0, 1, 63, 64, 65, 130}
    assert {c.T for c in ASSO_CASES} >= {1, 2, 4, 5, 9} and {c.n_k for c in ASSO_CASES} >= {1, 3, 4, 5}
    assert {c.M for c in ASSO_CASES} >= {1, 2, 255, 256, 257} and {c.mcd for c in ASSO_CASES} == {0.0, 0.5, 50.0}
    assert sum(_middle(c) for c in ASSO_CASES) >= 2
    assert any(c.segs[0] == 0 for c in ASSO_CASES) and any(c.segs[-1] == 0 for c in ASSO_CASES)
    assert any(0 in c.segs[1:-1] for c in ASSO_CASES) and any(c.pad for c in ASSO_CASES)
    assert any(c.decay is None for c in ASSO_CASES) and {c.with_iou for c in ASSO_CASES} == {0, 1}
    for c in ASSO_CASES:
        if c.M >= 2:
            assert (c.col_of == 0).sum() == 1 and c.col_of[0] == 0
            frames = np.searchsorted(c.offs, c.nonk, side="right") - 1
            assert set(frames[c.col_of == 1]) == set(frames[1:])              # (j = 0 is track 0's)
        if c.decay is not None:
            assert len(set(c.decay.tolist())) == c.Np
    assert {p[0] for c in SHORT_CASES for p in c.np_nc} >= {1, 2, 63, 64, 65, 128, 129, 319, 320}
    assert {p[1] for c in SHORT_CASES for p in c.np_nc} >= {1, 3, 4, 5} and {c.d for c in SHORT_CASES} == {4, 252, 256, 260, 1024}
    assert all(len(c.np_nc) >= 3 for c in SHORT_CASES) and any(c.rows % 4 for c in SHORT_CASES)
    assert {c.N for c in GATHER_CASES} == {1, 5, 70} and {c.d for c in GATHER_CASES} == {4, 1024}
    for c in GATHER_CASES:
        assert c.n_k in (0, 1, c.N - c.lo) and c.lo in (0, c.N - c.n_k)


# ------------------------------------------------------------------------------------------ short-term pairs
SHORT_MISTAKES = {
    "no background": (("randn", "negative", "peaked", "equal"), lambda c: True),
    "own rows in the softmax": (("randn", "peaked", "equal"), lambda c: True),
    "query box at b0 + i": (LOGIT_KINDS, lambda c: c.with_iou),
    "second chunk dropped": (LOGIT_KINDS, lambda c: c.max_prev > 64),
    "row stride n_cur": (LOGIT_KINDS, lambda c: any(n_cur > 1 and n_cur != n_prev for n_prev, n_cur in c.np_nc)),
    "S offset of the next pair": (LOGIT_KINDS, lambda c: True),
}


@pytest.mark.parametrize("box_kind", BOX_KINDS)
@pytest.mark.parametrize("case", SHORT_CASES, ids=[c.id for c in SHORT_CASES])
def test_short_term_bound(case, box_kind):
    boxes = case.boxes(box_kind)
    img_w, img_h = image_of(box_kind)
    for kind in LOGIT_KINDS:
        tgt, mem = case.inputs(kind)
        exp, bound = case.expected(kind, box_kind)
        assert not np.isnan(exp).any() and bool(np.isfinite(bound).all()) and bool((bound > 0).all())
        _inside("short term", emu_short(case, tgt, mem, boxes, img_w, img_h), exp, bound, "%s %s %s" % (case.id, kind, box_kind))
        for name, (kinds, exists) in SHORT_MISTAKES.items():
            if kind in kinds and exists(case):
                assert _outside(emu_short(case, tgt, mem, boxes, img_w, img_h, name), exp, bound) > 0, \
                    "%s %s %s: '%s' stays inside the bound" % (case.id, kind, box_kind, name)


def test_short_term_logits_are_the_kinds():
    for case in SHORT_CASES:
        for kind in LOGIT_KINDS:
            tgt, mem = case.inputs(kind)
            m0, n_prev = int(case.pairs[-1][0]), int(case.pairs[-1][1])
            l = mem[m0:m0 + n_prev].astype(np.float64) @ tgt[-1].astype(np.float64)
            a, _ = softmax_bg64(l)
            if kind == "overflow":
                assert float(np.abs(l).max()) > 89
            elif kind == "negative":
                assert float(l.max()) < -95 and float(a.max()) < 2.0 ** -126
            elif kind == "equal":
                assert bool((l == 0.75).all())
            elif kind == "peaked" and n_prev >= 2:
                assert 0.2 < float(a.max()) < 0.8


# ------------------------------------------------------------------------------------------ gathers
@pytest.mark.parametrize("case", GATHER_CASES, ids=[c.id for c in GATHER_CASES])
def test_gather_mistakes_are_visible(case):
    """The gathers are exact, so a mistake shows as soon as it moves one value: qdec from column 0 instead of 3 d, rows[r] instead of
    rows[lo + r]."""
    pool, proj = case.inputs()
    src, qkv, qdec = case.expected(pool, proj)
    assert np.isfinite(src).all() and np.isfinite(qkv).all() and np.isfinite(qdec).all()
    assert src.shape == (case.N, case.d) and qkv.shape == (case.N, 3 * case.d) and qdec.shape == (case.n_k, case.d)
    r = case.rows.astype(np.int64)
    if case.n_k:
        assert not np.array_equal(proj[r[case.lo:case.lo + case.n_k], :case.d], qdec)
        if case.lo and (r[:case.n_k] != r[case.lo:case.lo + case.n_k]).any():
            assert not np.array_equal(proj[r[:case.n_k], 3 * case.d:4 * case.d], qdec)
    if case.N >= 5:
        assert len(set(r.tolist())) < case.N and bool((np.diff(r) < 0).any())
