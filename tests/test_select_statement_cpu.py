"""CPU: the statements of tests/select_statement.py (topk64, argmax_first, proposal_valid_ref, enc_pos_valid64, bezier64, detect64 and
the score / IoU bounds) are the yardstick of test_select_forms_gpu.py.  On every case of the GPU file (same generators, same seeds:
the same bits) this file shows

  * the statements agree with oracle/gom_oracle.py wherever the oracle is defined;
  * the bounds are not vacuous: a numpy evaluation in the kernels' own order -- packed sort keys sorted per chunk and merged, the
    lane-strided argmax with its butterfly, the sequential fp32 score sum, the fp32 IoU with and without the fma contraction -- takes
    every decision the statement takes and stays within the score and IoU bounds (worst ratio printed);
  * no decision of a non-`exact` case is undecided;
  * the cases bite: the same evaluation with each planted mistake in it changes the result on at least one named case.  Which cases
    can show a mistake is arithmetic, not choice, and is written next to each mistake."""
import numpy as np
import pytest
import torch

import select_statement as S
from select_statement import (ARGMAX_KINDS, ARGMAX_ROWS, ARGMAX_V, CHUNK, DETECT_CASES, GEO_CASES, TOPK_CASES, U, argmax_first,
                              argmax_input, bezier64, boxes32, enc_pos_valid64, iou64, proposal_valid_ref, topk_values, undecided,
                              worst_margin_ratio)

f32 = np.float32
WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for k, v in sorted(WORST.items()):
        print("selection fp32 emulation worst ratio  %-22s %.4f" % (k, v))


def _worst(name, v):
    WORST[name] = max(WORST.get(name, 0.0), float(v))


# ------------------------------------------------------------------------------------------ top-k in the kernels' order
def _keys(v, idx, mistake):
    u = np.ascontiguousarray(v, f32).view(np.uint32).astype(np.uint64)
    neg = (u >> np.uint64(31)) == 1
    flipped = (u & np.uint64(0x7FFFFFFF)) if mistake == "neg_magnitude" else (~u & np.uint64(0xFFFFFFFF))
    u = np.where(neg, flipped, u | np.uint64(0x80000000))
    low = idx.astype(np.uint64) if mistake == "ties_high" else np.uint64(0xFFFFFFFF) - idx.astype(np.uint64)
    return (u << np.uint64(32)) | low


def topk_emul(logits, valid, c0, k, mistake=None):
    """topk_chunk_kernel + topk_merge_kernel: 64-bit keys (orderable float bits, ~index), a descending sort of every 4096-token
    chunk padded with zero keys, its first k keys as candidates, a descending sort of the candidates."""
    B, S = logits.shape
    chunks = -(-S // CHUNK)
    idx_out = np.zeros((B, k), np.int64)
    for b in range(B):
        cand = []
        for ch in range(chunks):
            s = np.arange(ch * CHUNK, min(S, (ch + 1) * CHUNK))
            v = logits[b, s].copy()
            keys = np.zeros(CHUNK, np.uint64)
            if mistake == "pad_real":                            # the tail's padding read as tokens of logit 0
                s = np.arange(ch * CHUNK, (ch + 1) * CHUNK)
                v = np.concatenate([v, np.zeros(len(s) - len(v), f32)])
            ok = np.ones(len(s), bool) if valid is None or mistake == "pad_real" else valid[s]
            if mistake == "pad_real" and valid is not None:
                ok[:min(S, (ch + 1) * CHUNK) - ch * CHUNK] = valid[ch * CHUNK:min(S, (ch + 1) * CHUNK)]
            v[~ok] = f32(c0)
            kk = _keys(v, (s - ch * CHUNK) if mistake == "chunk_local" else s, mistake)
            if mistake == "drop_invalid":
                kk[~ok] = 0
            keys[:len(kk)] = kk
            cand.append(np.sort(keys)[::-1][:k])
            if mistake == "merge_first":
                break
        low = np.sort(np.concatenate(cand))[::-1][:k] & np.uint64(0xFFFFFFFF)
        idx = low if mistake == "ties_high" else np.uint64(0xFFFFFFFF) - low
        idx_out[b] = idx.astype(np.uint32).view(np.int32)
    rows = idx_out + (0 if mistake == "rows_no_bS" else np.arange(B)[:, None] * S)
    return idx_out, rows


def _topk_same(case, got, exp):
    if case.values_only:
        return np.array_equal(topk_values(case.logits(), case.valid(), case.c0, np.clip(got[0], 0, case.S - 1)),
                              topk_values(case.logits(), case.valid(), case.c0, exp[0])) and np.array_equal(
            got[1] - got[0], exp[1] - exp[0]) and bool(((got[0] >= 0) & (got[0] < case.S)).all())
    return np.array_equal(got[0], exp[0]) and np.array_equal(got[1], exp[1])


@pytest.mark.parametrize("case", TOPK_CASES, ids=[c.id for c in TOPK_CASES])
def test_topk_emulation_and_hand(case):
    exp = case.expected()
    assert _topk_same(case, topk_emul(case.logits(), case.valid(), case.c0, case.k), exp), case.id
    for b in range(case.B):
        assert len(set(exp[0][b].tolist())) == case.k
    hand = case.by_hand()
    if hand is not None:
        assert np.array_equal(exp[0], hand)
    if case.kind == "invalid_flood_low":                         # the valid ones first by value, then the lowest invalid indices
        valid, nv = case.valid(), case.k // 2
        assert valid[exp[0][:, :nv]].all() and np.array_equal(exp[0][:, nv:], np.tile(np.flatnonzero(~valid)[:case.k - nv], (case.B, 1)))
    if case.kind == "last_chunk_wins":
        tail0 = (-(-case.S // CHUNK) - 1) * CHUNK
        n = min(case.k, case.S - tail0)
        assert (exp[0][:, :n] >= tail0).all()
    if case.B > 1 and case.S > 1 and case.kind == "randn":
        assert not np.array_equal(exp[0][0], exp[0][1]), "rows must differ per b"


def test_topk_agrees_with_torch_topk_on_tie_free_rows():
    seen = 0
    for case in TOPK_CASES:
        if case.kind not in ("randn", "signed_extremes", "last_chunk_wins"):
            continue
        l, v = case.logits(), case.valid()
        masked = torch.from_numpy(l.copy())
        if v is not None:
            masked[:, torch.from_numpy(~v)] = float(f32(case.c0))
        ref = torch.topk(masked, case.k, dim=1)[1].numpy()
        exp = case.expected()[0]
        for b in range(case.B):
            if len(np.unique(masked[b].numpy()[ref[b]])) == case.k:
                assert np.array_equal(ref[b], exp[b]), case.id
                seen += 1
    assert seen >= 10


# which cases can show it:
TOPK_MISTAKES = {
    "ties_high": "every case with a tie among or at the edge of the winners: all_equal, tie_across_chunk, the invalid floods",
    "chunk_local": "every S > 4096 whose winners are not all in chunk 0",
    "merge_first": "every S > 4096 whose winners are not all in chunk 0; last_chunk_wins outright",
    "drop_invalid": "a c0 that wins: invalid_flood_high, invalid_flood_low (k exceeds the valid tokens)",
    "neg_magnitude": "two negative winners: k == S (2, 37, 37), (3, 4096, 4096), signed_extremes with large k",
    "rows_no_bS": "every B > 1",
    "pad_real": "a chunk shorter than 4096 and a winner below 0: k == S at (2, 37, 37), all_equal's row of -1, invalid_flood_low",
}


@pytest.mark.parametrize("mistake", sorted(TOPK_MISTAKES))
def test_topk_planted_mistake_is_caught(mistake):
    caught = [c.id for c in TOPK_CASES if not c.values_only and c.S <= 8193
              and not _topk_same(c, topk_emul(c.logits(), c.valid(), c.c0, c.k, mistake), c.expected())]
    print("top-k %-14s caught by %d cases, e.g. %s" % (mistake, len(caught), caught[:3]))
    assert caught, mistake


# ------------------------------------------------------------------------------------------ argmax in the kernel's order
UNSET = 0x7FFFFFFF


def argmax_emul(x, mistake=None):
    """argmax_rows_kernel: lane l scans columns l, l + 64, ... with a strict >, then the xor butterfly takes the larger value and on
    equal values the lower index; a lane that saw nothing above -inf carries the unset index, which must not leave the kernel."""
    rows, V = x.shape
    best = np.full((rows, 64), -np.inf, f32)
    bi = np.full((rows, 64), UNSET, np.int64)
    for p in range(1 if mistake == "cols_ge_64_ignored" else -(-V // 64)):
        n = min(64, V - p * 64)
        v = x[:, p * 64:p * 64 + n]
        with np.errstate(invalid="ignore"):
            up = (v >= best[:, :n]) if mistake == "last_max" else (v > best[:, :n])
        best[:, :n] = np.where(up, v, best[:, :n])
        bi[:, :n] = np.where(up, p * 64 + np.arange(n), bi[:, :n])
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        ob, oi = best[:, lane ^ o], bi[:, lane ^ o]
        with np.errstate(invalid="ignore"):
            take = (ob > best) | ((ob == best) & ((oi > bi) if mistake == "last_max" else (oi < bi)))
        best, bi = np.where(take, ob, best), np.where(take, oi, bi)
    out = bi[:, 0]
    return out if mistake == "unset_leaks" else np.where(out == UNSET, 0, out)


def _argmax_cases():
    return [(V, rows, kind) for V in ARGMAX_V for rows in ARGMAX_ROWS for kind in ARGMAX_KINDS]


def test_argmax_emulation_matches_statement_and_torch():
    for V, rows, kind in _argmax_cases():
        x = argmax_input(V, rows, kind)
        got = argmax_emul(x)
        assert ((got >= 0) & (got < V)).all(), (V, rows, kind)
        if kind == "nan":
            clean = ~np.isnan(x).any(1)
            assert np.array_equal(got[clean], argmax_first(x[clean]))
            continue
        exp = argmax_first(x)
        assert np.array_equal(got, exp), (V, rows, kind)
        if kind in ("constant", "neg_inf"):
            assert (exp == 0).all()
        if kind == "randn":                                      # the oracle's text[b][sel].topk(1), defined on a tie-free row
            assert np.array_equal(torch.from_numpy(x).topk(1)[1][:, 0].numpy(), exp)


ARGMAX_MISTAKES = {
    "last_max": "dup_max and constant at every V >= 2",
    "cols_ge_64_ignored": "randn and dup_max at V in {65, 129}",
    "unset_leaks": "neg_inf at every V (and all-NaN rows)",
}


@pytest.mark.parametrize("mistake", sorted(ARGMAX_MISTAKES))
def test_argmax_planted_mistake_is_caught(mistake):
    caught = [(V, rows, kind) for V, rows, kind in _argmax_cases() if kind != "nan"
              and not np.array_equal(argmax_emul(argmax_input(V, rows, kind), mistake), argmax_first(argmax_input(V, rows, kind)))]
    print("argmax %-18s caught by %d cases, e.g. %s" % (mistake, len(caught), caught[:3]))
    assert caught, mistake


# ------------------------------------------------------------------------------------------ validity, position table, Bezier
def _oracle_props(shapes, vshapes):
    """oracle/gom_oracle.py deepsolo_forward, the proposal grid and its validity (lines "proposals"), for one image."""
    props = []
    for l, (H, W) in enumerate(shapes):
        Hv, Wv = (H, W) if vshapes is None else vshapes[l]
        gy, gx = torch.meshgrid(torch.linspace(0, H - 1, H), torch.linspace(0, W - 1, W), indexing="ij")
        grid = torch.cat([gx.unsqueeze(-1), gy.unsqueeze(-1)], -1)
        scale = torch.tensor([Wv, Hv]).view(1, 1, 2)
        props.append(((grid + 0.5) / scale).view(-1, 2))
    props = torch.cat(props, 0)
    return props, ((props > 0.01) & (props < 0.99)).all(-1)


def _valid_emul(shapes, vshapes, mistake=None):
    out = []
    for l, (H, W) in enumerate(shapes):
        Hn, Wn = (H, W) if (vshapes is None or mistake == "padded_extent") else vshapes[l]
        t = np.arange(H * W)
        x, y = ((t % W).astype(f32) + f32(0.5)) / f32(Wn), ((t // W).astype(f32) + f32(0.5)) / f32(Hn)
        lo, hi = f32(0.01), f32(0.99)
        out.append(((x >= lo) & (x <= hi) & (y >= lo) & (y <= hi)) if mistake == "ge" else ((x > lo) & (x < hi) & (y > lo) & (y < hi)))
    return np.concatenate(out)


@pytest.mark.parametrize("name,shapes,vshapes", GEO_CASES, ids=[g[0] for g in GEO_CASES])
def test_validity_statement(name, shapes, vshapes):
    ref = proposal_valid_ref(shapes, vshapes)
    assert np.array_equal(ref, _oracle_props(shapes, vshapes)[1].numpy())
    assert np.array_equal(ref, _valid_emul(shapes, vshapes))
    # the cases bite.  `>=`: (i + 0.5) / W == 0.01f needs W = 50 (i = 0) -- both geometries have it; the padded extent: only "padded64"
    assert not np.array_equal(ref, _valid_emul(shapes, vshapes, "ge")), "no coordinate falls on 0.01 or 0.99"
    if vshapes is not None:
        assert not np.array_equal(ref, _valid_emul(shapes, vshapes, "padded_extent"))
        starts, _ = S.level_starts(shapes)
        for l, (H, W) in enumerate(shapes):                      # every padded token is invalid
            r, c = np.divmod(np.arange(H * W), W)
            pad = (r >= vshapes[l][0]) | (c >= vshapes[l][1])
            assert not ref[starts[l]:starts[l] + H * W][pad].any()
    assert ref.any() and not ref.all()


@pytest.mark.parametrize("name,shapes,vshapes", GEO_CASES, ids=[g[0] for g in GEO_CASES])
def test_position_table_statement_vs_oracle(name, shapes, vshapes):
    from oracle import gom_oracle as O
    g = np.random.default_rng(3)
    lvl = g.standard_normal(256).astype(f32)
    worst = 0.0
    for l, (H, W) in enumerate(shapes):
        Hv, Wv = (H, W) if vshapes is None else vshapes[l]
        tab, own = enc_pos_valid64(S.dim_t32(), lvl, H, W, Hv, Wv)
        mask = torch.ones(1, H, W, dtype=torch.bool)
        mask[:, :Hv, :Wv] = False
        ref = (O.pos_encoding_2d(mask)[0].flatten(1).t() + torch.from_numpy(lvl)).double().numpy()
        assert own.sum() == Hv * Wv
        worst = max(worst, float(np.abs(ref - tab)[own].max()))
    _worst("pos table oracle/2e-6", worst / S.ABS_TABLE)
    assert worst <= S.ABS_TABLE
    assert np.allclose(S.dim_t32(), (10000 ** (2 * torch.div(torch.arange(128, dtype=torch.float32), 2, rounding_mode="trunc") / 128)).numpy(),
                       rtol=1e-6)


@pytest.mark.parametrize("name,shapes,vshapes", GEO_CASES, ids=[g[0] for g in GEO_CASES])
def test_bezier_statement_vs_oracle(name, shapes, vshapes):
    from oracle import gom_oracle as O
    coord, idx = S.geo_bezier_inputs(shapes, vshapes)
    bern = S.bernstein(25)
    assert float(np.abs(O.bernstein_matrix(25).double().numpy() - bern).max()) < 1e-7
    exp = bezier64(coord, idx, shapes, vshapes, bern)
    assert np.isfinite(exp).all()
    valid = proposal_valid_ref(shapes, vshapes)
    assert (~valid[idx]).any() and valid[idx].any(), "the index set holds valid and invalid tokens"
    assert np.allclose(exp[~valid[idx]], 1.0)                    # sigmoid(+inf) = 1 in all four control points; the Bernstein row sums to 1
    props, vref = _oracle_props(shapes, vshapes)
    lp = torch.log(props / (1 - props)).masked_fill(~vref[:, None], float("inf")).repeat(1, 4)
    unact = torch.from_numpy(coord) + lp[None]
    B, nq = idx.shape
    sel = torch.gather(unact, 1, torch.from_numpy(idx).unsqueeze(-1).repeat(1, 1, 8)).sigmoid()
    ref = torch.matmul(O.bernstein_matrix(25), sel.view(B, nq, 4, 2)).double().numpy()
    _worst("bezier oracle/2e-6", np.abs(ref - exp).max() / S.ABS_TABLE)
    assert np.abs(ref - exp).max() <= S.ABS_TABLE


# ------------------------------------------------------------------------------------------ detect_post in the kernel's order
def _score32(l):
    l = np.asarray(l, f32)
    s = np.zeros(l.shape[:-1], f32)
    for p in range(l.shape[-1]):
        s = s + l[..., p]
    with np.errstate(over="ignore"):
        return f32(1) / (f32(1) + np.exp(-(s / f32(l.shape[-1]))))


def _iou32(a, b, fma):
    w = np.maximum(f32(0), np.minimum(a[2], b[:, 2]) - np.maximum(a[0], b[:, 0]))
    h = np.maximum(f32(0), np.minimum(a[3], b[:, 3]) - np.maximum(a[1], b[:, 1]))
    inter = w * h
    ia, ar = (a[2] - a[0]) * (a[3] - a[1]), (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    # contracted: iarea + area - w * h with the product unrounded (fp64 holds the product of two fp32 exactly)
    union = ((ia + ar).astype(np.float64) - w.astype(np.float64) * h.astype(np.float64)).astype(f32) if fma else (ia + ar) - inter
    with np.errstate(divide="ignore", invalid="ignore"):
        return inter / union


def detect_emul(case, mistake=None, fma=False, track=False):
    """detect_post_kernel in numpy fp32 -> (count, kept, keep_idx) per frame; with `track` the worst |fp32 - fp64| / bound of the
    scores and of the IoUs it evaluates goes to WORST."""
    i = case.inputs()
    cls, re = i["cls"], None if mistake == "no_rescoring" else i["recls"]
    B, nq, P = cls.shape
    n = P - 1 if (mistake == "p_minus_1" and P > 1) else P
    sc = _score32(cls[..., :n])
    if re is not None:
        r = _score32(re[..., :n])
        sc = np.where(sc > r, sc, r)
    if track:
        s64, sb = case.expected_scores()
        _worst("score", (np.abs(sc.astype(np.float64) - s64) / sb).max())
    det, nms, asso = f32(case.det_thr), f32(case.nms_thr), f32(case.asso_thr)
    if mistake == "ctrl_boxes":
        px = i["ctrl"] * np.array([case.hw[1], case.hw[0]], f32)
        box = np.stack([px[..., 0].min(-1), px[..., 1].min(-1), px[..., 0].max(-1), px[..., 1].max(-1)], -1)
    else:
        box = boxes32(i["bd"], case.hw[0], case.hw[1])[0]
    count, kept_all, keep_idx = [], [], []
    for b in range(B):
        sel = (sc[b] >= det) if mistake == "ge_det" else (sc[b] > det)
        if mistake == "first_256":
            sel[256:] = False
        if mistake == "asso_first":
            sel &= sc[b] > asso
        q = np.flatnonzero(sel)
        order = q[np.lexsort((-q, -sc[b][q]))] if mistake == "unstable" else q[np.argsort(-sc[b][q], kind="stable")]
        dead = np.zeros(len(order), bool)
        for a in range(len(order)):
            if dead[a] and mistake != "dead_suppresses":
                continue
            later = np.flatnonzero(~dead[a + 1:]) + a + 1
            iou = _iou32(box[b, order[a]], box[b, order[later]], fma)
            with np.errstate(invalid="ignore"):
                dead[later[(iou >= nms) if mistake == "ge_nms" else (iou > nms)]] = True
            if track and len(later):
                i64, ib = iou64(box[b, order[a]], box[b, order[later]])
                ok = ~np.isnan(i64) & (ib > 0)
                assert np.array_equal(np.isnan(i64), np.isnan(iou))
                if ok.any():
                    _worst("iou fma" if fma else "iou", (np.abs(iou.astype(np.float64) - i64)[ok] / ib[ok]).max())
        kept = order[~dead]
        kept = kept[(sc[b][kept] >= asso) if mistake == "ge_asso" else (sc[b][kept] > asso)]
        count.append(len(kept))
        kept_all.append(kept)
        keep_idx.append(kept + (0 if mistake == "keep_no_b" else b * nq))
    return count, kept_all, keep_idx


def _same_decisions(case, got):
    e = case.expected()
    return (list(e["count"]) == list(got[0]) and all(np.array_equal(a, b) for a, b in zip(e["kept"], got[1]))
            and all(np.array_equal(a, b) for a, b in zip(e["keep_idx"], got[2])))


IDS = [c.id for c in DETECT_CASES]


@pytest.mark.parametrize("case", DETECT_CASES, ids=IDS)
def test_detect_emulation_inside_bounds_and_decided(case):
    e = case.expected()
    for fma in (False, True):
        assert _same_decisions(case, detect_emul(case, fma=fma, track=True)), "%s: the fp32 evaluation decides differently" % case.id
    if case.kind == "exact":
        assert [k.tolist() for k in e["kept"]] == case.hand
        assert e["keep_idx"][1].tolist() == [case.nq + q for q in case.hand[1]]
        return
    und = undecided(e["margins"])
    for k, v in worst_margin_ratio(e["margins"]).items():
        _worst("margin bound/margin " + k, v)
    assert und == {"thr": 0, "nms": 0, "order": 0}, "%s: undecided decisions %r" % (case.id, und)
    if case.kind == "all_selected":
        assert int(e["count"][0]) > 0 and len(e["margins"]["thr"]) == case.nq and (case.expected_scores()[0] > case.asso_thr).all()
    if case.kind == "none_selected":
        assert list(e["count"]) == [0] * case.B
    if case.kind == "one_selected":
        assert [k.tolist() for k in e["kept"]] == [[case.nq // 2]] * case.B
    if case.kind == "score_ties":                                # the lower index of an overlapping tied pair survives
        for kept in e["kept"]:
            assert len(kept) and not (set(kept.tolist()) & {q + 1 for q in kept.tolist() if q % 3 == 0})
    if case.kind == "random_clustered" and case.nq >= 60:
        assert int(e["count"].max()) >= 5 and (case.B == 1 or e["count"][0] == 0)


def test_exact_case_properties():
    """The `exact` inputs have what their name promises: integer boxes, a score of exactly 0.5, IoU of exactly 1/2 and 3/4, the
    chain, the identical zero-area boxes."""
    case = [c for c in DETECT_CASES if c.kind == "exact" and c.with_re][0]
    i = case.inputs()
    box = boxes32(i["bd"], 64, 128)[0][1]
    assert np.array_equal(box, np.array(S._EXACT_BOXES, f32))
    assert _score32(i["cls"])[1, 0] == f32(0.5) and _score32(i["recls"])[1, 0] == f32(0.5)
    iou = lambda a, b: float(_iou32(box[a], box[b:b + 1], False)[0])
    assert iou(3, 10) == 0.5 and iou(7, 2) == 0.75
    assert iou(8, 4) > 0.5 and iou(4, 1) > 0.5 and iou(8, 1) < 0.5
    assert np.isnan(iou(5, 9))
    s = _score32(i["cls"])[1]
    assert s[11] < 0.25 and _score32(i["recls"])[1, 11] > 0.5


def _oracle_detect(case):
    from oracle import gom_oracle as O
    from helpers import mini_cfg
    i = case.inputs()
    B, nq, P = i["cls"].shape
    cfg = mini_cfg("icdar15", nq=nq)
    cfg.VIDEO_TEST.NMS_THRESH = case.nms_thr
    cfg.MODEL.TRANSFORMER.INFERENCE_TH_TEST = case.det_thr
    V = 38
    text = torch.zeros(B, nq, P, V)
    text.scatter_(-1, torch.from_numpy(i["recs"].astype(np.int64)).unsqueeze(-1), 5.0)
    out = {"pred_logits": torch.from_numpy(i["cls"]).unsqueeze(-1), "pred_text_logits": text,
           "pred_ctrl_points": torch.from_numpy(i["ctrl"]), "pred_bd_points": torch.from_numpy(i["bd"]),
           "query_features": torch.arange(B * nq, dtype=torch.float32).view(B, nq, 1)}
    re = torch.from_numpy(i["recls"]).unsqueeze(-1) if i["recls"] is not None else None
    props = O.proposals_with_nms(cfg, O.detection(cfg, out, re, [case.hw] * B))
    return [p.select(p["objectness_logits"] > case.asso_thr) for p in props]


@pytest.mark.parametrize("case", DETECT_CASES, ids=IDS)
def test_detect_statement_agrees_with_oracle(case):
    e = case.expected()
    for b, p in enumerate(_oracle_detect(case)):
        n = len(p) if len(p.keys()) else 0
        assert n == e["count"][b], (case.id, b)
        if n == 0:
            continue
        assert np.array_equal(p["query_features"][:, 0].numpy().astype(np.int64), e["keep_idx"][b])
        assert np.array_equal(p["proposal_boxes"].numpy(), e["boxes"][b])
        assert np.array_equal(p["ctrl_points"].numpy(), e["ctrl"][b])
        assert np.array_equal(p["bd"].numpy(), e["bd"][b])
        assert np.array_equal(p["recs"].numpy(), e["recs"][b])
        assert (np.abs(p["scores"].double().numpy() - e["scores"][b]) <= 2 * e["score_bound"][b] + 2 * U).all()


# which cases can show it:
DETECT_MISTAKES = {
    "ge_det": "a score exactly on det_thr that asso_thr would let through: exact-a (det 0.5 > asso 0.25; query 0 and all of frame 0)",
    "ge_nms": "an IoU exactly on nms_thr: exact (queries 3 and 10)",
    "ge_asso": "a selected, unsuppressed score exactly on asso_thr: exact-b (det 0.25 selects the 0.5 of query 0)",
    "unstable": "equal scores on overlapping boxes: score_ties",
    "dead_suppresses": "a chain A > B > C: exact (queries 8, 4, 1); the clustered cases where one occurs",
    "no_rescoring": "every case with rescoring where it lifts a score over a threshold: exact (query 11), random_clustered",
    "p_minus_1": "every random case with P > 1 whose decisions move with one logit less; never P = 1",
    "ctrl_boxes": "every case with overlapping boxes: the ctrl boxes are smaller, so fewer pairs suppress",
    "first_256": "nq > 256 with a kept query past 255: nq 257 (one_selected sits at 128, so not that), 1024",
    "keep_no_b": "every B > 1 with a kept query in a frame b > 0",
}


@pytest.mark.parametrize("mistake", sorted(DETECT_MISTAKES))
def test_detect_planted_mistake_is_caught(mistake):
    caught = [c.id for c in DETECT_CASES if not _same_decisions(c, detect_emul(c, mistake))]
    print("detect_post %-16s caught by %d cases, e.g. %s" % (mistake, len(caught), caught[:3]))
    assert caught, mistake
    if mistake.startswith("ge_") or mistake == "dead_suppresses":
        assert any(c.startswith("exact") for c in caught)
    if mistake == "unstable":
        assert any(c.startswith("score_ties") for c in caught)
    if mistake == "first_256":
        assert all(("nq257" in c or "nq1024" in c) for c in caught)


def test_asso_filter_before_nms_is_the_same_function():
    """The issue lists "the asso filter applied before NMS" as a mistake.  It is none: a box is suppressed only by boxes of a higher
    (or equal, lower-index) score, so whatever the early filter removes (score <= asso_thr) could only have suppressed boxes whose
    score is <= asso_thr too, and those are removed either way.  No input can show a difference; this holds the emulation to that."""
    for c in DETECT_CASES:
        assert _same_decisions(c, detect_emul(c, "asso_first")), c.id
