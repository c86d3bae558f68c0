"""GPU: the kernels that make discrete decisions -- gom_topk_tokens (csrc/topk.hip), gom_argmax_rows_f32 and gom_detect_post
(csrc/detect.hip), gom_proposal_valid[_masked], gom_pos_encoding_2d[_valid]_f32 and gom_bezier_reference_points[_masked]
(csrc/elementwise.hip) -- against the statements of tests/select_statement.py on the cases and inputs of that file.
tests/test_select_statement_cpu.py shows on the same bits that the statements agree with the oracle, that every decision of every
case is decided, and that the cases catch the mistakes planted there.

Every call goes through the C entry points that `ops` uses, reads its operands from NaN-padded buffers (gap columns where ld > 1 or
ld > V, a row past the end) laid out as the `ops` wrappers lay them out, and writes into buffers prefilled with a sentinel bit pattern,
which every slot past count[b] and every element the op does not own must keep.  Indices, counts, keep_idx, recs, validity bytes,
boxes, ctrl and bd are compared exactly; scores, Bezier points and position tables within their bounds, and the worst
|got - exp| / bound per form is printed at the end (docs/LAB_NOTES.md keeps a record).  Each op's wrapper is called once for its own
contract: zeros in padded slots and the `small` layout."""
import numpy as np
import pytest
import torch

import select_statement as S
from select_statement import (ARGMAX_KINDS, ARGMAX_ROWS, ARGMAX_V, DETECT_CASES, GEO_CASES, TOPK_CASES, TOPK_SHAPES, argmax_first,
                              argmax_input, bezier64, enc_pos_valid64, proposal_valid_ref, topk_values)

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENTINEL = 0x7FC0DEAD                                 # a NaN with a payload: an element left unwritten is also not finite
SENTINEL64 = (SENTINEL << 32) | SENTINEL
PAD = 8
RATIOS = {}


def _ops():
    from gomatching_amd import ops
    return ops


def _sent_i32(n):
    return torch.full((n,), SENTINEL, dtype=torch.int32, device=DEV)


def _sent_f32(n):
    return _sent_i32(n).view(torch.float32)


def _is_sentinel(t):
    return bool((t.contiguous().view(torch.int32) == SENTINEL).all())


def _column0(x, ld):
    """x [n] float32 (numpy) -> a device buffer [n + 1, ld] full of NaN with x in column 0."""
    buf = torch.full((x.shape[0] + 1, ld), float("nan"))
    buf[:x.shape[0], 0] = torch.from_numpy(np.ascontiguousarray(x, np.float32))
    return buf.to(DEV)


def _flat_nan_padded(x):
    """x (numpy float32) -> a flat device buffer of x followed by PAD NaNs."""
    x = torch.from_numpy(np.ascontiguousarray(x, np.float32)).reshape(-1)
    return torch.cat([x, torch.full((PAD,), float("nan"))]).to(DEV)


def _ints(x, dtype=torch.int32):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dtype).to(DEV)


def _ratio(form, err, bound):
    err, bound = np.asarray(err, np.float64).reshape(-1), np.broadcast_to(np.asarray(bound, np.float64), np.shape(err)).reshape(-1)
    if err.size:
        RATIOS[form] = max(RATIOS.get(form, 0.0), float((err / bound).max()))


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for k, v in sorted(RATIOS.items()):
        print("selection worst |got-exp| / bound  %-22s %.4f" % (k, v))


# ------------------------------------------------------------------------------------------ top-k
def _topk_launch(case, ld, with_rows):
    """gom_topk_tokens with the buffers ops.topk_tokens passes (logits [B * S, ld] column 0, valid [S] bytes, one invalid logit, a
    workspace of gom_topk_workspace_bytes, idx and rows [B, k] int32) -> (rc, idx, rows) on the host; the slack is checked here."""
    ops = _ops()
    L = ops._L()
    B, Sn, k = case.B, case.S, case.k
    logits = _column0(case.logits().reshape(-1), ld)
    v = case.valid()
    valid = None if v is None else torch.cat([torch.from_numpy(v.astype(np.uint8)), torch.full((PAD,), 0xAB, dtype=torch.uint8)]).to(DEV)
    c0 = torch.tensor([case.c0, float("nan")], device=DEV) if v is not None else None
    nbytes = L.gom_topk_workspace_bytes(B, Sn, k)
    assert nbytes == 8 * B * -(-Sn // S.CHUNK) * k
    ws = _sent_i32(nbytes // 4 + PAD)
    idx, rows = _sent_i32(B * k + PAD), _sent_i32(B * k + PAD) if with_rows else None
    rc = L.gom_topk_tokens(ops._p(logits), ld, ops._p(valid), ops._p(c0), B, Sn, k, ops._p(ws), ops._p(idx), ops._p(rows), ops._stream())
    torch.cuda.synchronize()
    assert _is_sentinel(ws[nbytes // 4:]) and _is_sentinel(idx[B * k:]) and (rows is None or _is_sentinel(rows[B * k:])), \
        "%s: wrote past the end of an output" % case.id
    return rc, idx[:B * k].cpu().numpy().reshape(B, k), None if rows is None else rows[:B * k].cpu().numpy().reshape(B, k)


def _topk_check(case, idx, rows, what):
    exp_idx, exp_rows = case.expected()
    assert ((idx >= 0) & (idx < case.S)).all(), "%s: an index outside [0, S)" % what
    for b in range(case.B):
        assert len(set(idx[b].tolist())) == case.k, "%s: a token selected twice in row %d" % (what, b)
    if case.values_only:
        assert np.array_equal(topk_values(case.logits(), case.valid(), case.c0, idx),
                              topk_values(case.logits(), case.valid(), case.c0, exp_idx)), what
    else:
        assert np.array_equal(idx, exp_idx), "%s: %d of %d indices differ" % (what, int((idx != exp_idx).sum()), idx.size)
    if rows is not None:
        assert np.array_equal(rows, np.arange(case.B)[:, None] * case.S + idx), "%s: rows != b * S + idx" % what


@pytest.mark.parametrize("shape", TOPK_SHAPES, ids=["B%d-S%d-k%d" % s for s in TOPK_SHAPES])
def test_topk_tokens(shape):
    """Every value kind of the shape with (ld 1, rows) and (ld 3, no rows); randn also the other two combinations."""
    for case in [c for c in TOPK_CASES if (c.B, c.S, c.k) == shape]:
        forms = [(1, True), (3, False)] + ([(1, False), (3, True)] if case.kind == "randn" else [])
        for ld, with_rows in forms:
            what = "%s ld%d rows%d" % (case.id, ld, with_rows)
            rc, idx, rows = _topk_launch(case, ld, with_rows)
            assert rc == 0, what
            _topk_check(case, idx, rows, what)


def test_topk_wrapper_contract():
    """ops.topk_tokens: int32 [B, k] idx (and rows with with_rows), column 0 of a [B * S, ld] buffer by its stride."""
    ops = _ops()
    case = [c for c in TOPK_CASES if (c.B, c.S, c.k, c.kind) == (8, 8193, 100, "randn")][0]
    logits = _column0(case.logits().reshape(-1), 3)[:case.B * case.S]
    valid, c0 = _ints(case.valid().astype(np.uint8), torch.uint8), torch.tensor([case.c0], device=DEV)
    idx, rows = ops.topk_tokens(logits, case.B, case.S, case.k, valid=valid, invalid_logit=c0, with_rows=True)
    assert idx.dtype == rows.dtype == torch.int32 and tuple(idx.shape) == tuple(rows.shape) == (case.B, case.k)
    _topk_check(case, idx.cpu().numpy(), rows.cpu().numpy(), "wrapper")
    only = ops.topk_tokens(logits, case.B, case.S, case.k, valid=valid, invalid_logit=c0)
    assert torch.equal(only, idx)


def test_topk_limits():
    """k > S, k > 4096, chunks * k > 8192 return the library's argument error through ops.check and launch nothing; the largest
    accepted sizes are cases of test_topk_tokens."""
    ops = _ops()
    from gomatching_amd.lib import GomError
    L = ops._L()
    logits = torch.zeros(3 * 4096 + 8, device=DEV)
    for Sn, k in [(37, 38), (5000, 4097), (3 * 4096, 2731), (8193, 2731)]:
        ws, idx, rows = _sent_i32(3 * 8192 * 2), _sent_i32(8192), _sent_i32(8192)
        with pytest.raises(GomError, match="GOM_ERR_INVALID_ARG"):
            ops.check(L.gom_topk_tokens(ops._p(logits), 1, None, None, 1, Sn, k, ops._p(ws), ops._p(idx), ops._p(rows), ops._stream()),
                      "gom_topk_tokens")
        torch.cuda.synchronize()
        assert _is_sentinel(ws) and _is_sentinel(idx) and _is_sentinel(rows), "a refused call wrote to its output"


# ------------------------------------------------------------------------------------------ argmax
@pytest.mark.parametrize("V", ARGMAX_V)
def test_argmax_rows(V):
    """gom_argmax_rows_f32 at every row count, ld in {V, V + 3} (NaN in the gap columns and in a row past the end) and every kind:
    the first maximum, 0 for a constant or all -inf row, and for rows that hold NaN an index in [0, V)."""
    ops = _ops()
    L = ops._L()
    for rows in ARGMAX_ROWS:
        for ld in (V, V + 3):
            for kind in ARGMAX_KINDS:
                what = "V%d rows%d ld%d %s" % (V, rows, ld, kind)
                x = argmax_input(V, rows, kind)
                buf = torch.full((rows + 1, ld), float("nan"))
                buf[:rows, :V] = torch.from_numpy(x)
                buf = buf.to(DEV)
                out = _sent_i32(rows + PAD)
                assert L.gom_argmax_rows_f32(ops._p(buf), ld, V, rows, ops._p(out), ops._stream()) == 0, what
                got = out[:rows].cpu().numpy()
                assert _is_sentinel(out[rows:]), what + ": wrote past the end"
                assert ((got >= 0) & (got < V)).all(), "%s: an index outside [0, V): %r" % (what, got[(got < 0) | (got >= V)][:4])
                clean = ~np.isnan(x).any(1)
                assert np.array_equal(got[clean], argmax_first(x[clean])), what
                if kind == "randn" and ld > V:
                    assert torch.equal(ops.argmax_rows(buf[:rows, :V]).cpu(), out[:rows].cpu()), what + ": wrapper"


# ------------------------------------------------------------------------------------------ validity, position table, Bezier
def _geo_device(shapes, vshapes):
    starts, Sn = S.level_starts(shapes)
    vs = None if vshapes is None else _ints(np.asarray(vshapes, np.int64), torch.int64)
    return _ints(np.asarray(shapes, np.int64), torch.int64), _ints(starts.astype(np.int64), torch.int64), vs, Sn


@pytest.mark.parametrize("name,shapes,vshapes", GEO_CASES, ids=[g[0] for g in GEO_CASES])
def test_proposal_valid(name, shapes, vshapes):
    """gom_proposal_valid / gom_proposal_valid_masked: the bytes of the reference's float32 test, with extents on which
    (i + 0.5) / W falls on 0.01 and 0.99; a padded geometry is also run unmasked (its padded extents then count)."""
    ops = _ops()
    L = ops._L()
    ss, lsi, vs, Sn = _geo_device(shapes, vshapes)
    for masked in ([False] if vshapes is None else [True, False]):
        out = torch.full((Sn + PAD,), 0xAB, dtype=torch.uint8, device=DEV)
        if masked:
            rc = L.gom_proposal_valid_masked(ops._p(ss), ops._p(lsi), len(shapes), ops._p(vs), ops._p(out), Sn, ops._stream())
        else:
            rc = L.gom_proposal_valid(ops._p(ss), ops._p(lsi), len(shapes), ops._p(out), Sn, ops._stream())
        assert rc == 0
        exp = proposal_valid_ref(shapes, vshapes if masked else None)
        assert np.array_equal(out[:Sn].cpu().numpy(), exp.astype(np.uint8)), "%s masked=%d" % (name, masked)
        assert bool((out[Sn:] == 0xAB).all())
        assert torch.equal(ops.proposal_valid(ss, lsi, Sn, vs if masked else None), out[:Sn])


@pytest.mark.parametrize("name,shapes,vshapes", GEO_CASES, ids=[g[0] for g in GEO_CASES])
def test_pos_encoding_valid(name, shapes, vshapes):
    """ops.pos_encoding_into with valid_hw (gom_pos_encoding_2d_valid_f32) per level against enc_pos_valid64 on the valid tokens; an
    unpadded level gives the bits of gom_pos_encoding_2d_f32."""
    ops = _ops()
    dim_t = torch.from_numpy(S.dim_t32()).to(DEV)
    lvl = np.random.default_rng(3).standard_normal(256).astype(np.float32)
    lvl_d = torch.from_numpy(lvl).to(DEV)
    for l, (H, W) in enumerate(shapes):
        Hv, Wv = (H, W) if vshapes is None else vshapes[l]
        out = _sent_f32((H * W + 1) * 256)
        ops.pos_encoding_into(dim_t, lvl_d, out, H, W, valid_hw=(Hv, Wv))
        got = out[:H * W * 256].cpu().double().numpy().reshape(H * W, 256)
        assert _is_sentinel(out[H * W * 256:]) and np.isfinite(got).all()
        exp, own = enc_pos_valid64(S.dim_t32(), lvl, H, W, Hv, Wv)
        err = np.abs(got - exp)[own]
        _ratio("pos_encoding_valid", err, S.ABS_TABLE)
        assert (err <= S.ABS_TABLE).all(), "%s level %d: %.3e" % (name, l, err.max())
        if (Hv, Wv) == (H, W):
            plain = _sent_f32((H * W + 1) * 256)
            ops.pos_encoding_into(dim_t, lvl_d, plain, H, W)
            assert torch.equal(plain.view(torch.int32), out.view(torch.int32))


@pytest.mark.parametrize("name,shapes,vshapes", GEO_CASES, ids=[g[0] for g in GEO_CASES])
def test_bezier_reference_points(name, shapes, vshapes):
    """gom_bezier_reference_points[_masked] on an index set that holds invalid tokens: finite, within 2e-6 of bezier64, and the
    compact form (the selected tokens' rows) gives the bits of the full form."""
    ops = _ops()
    L = ops._L()
    P = 25
    bern = torch.from_numpy(S.bernstein(P).astype(np.float32)).to(DEV)
    bern64 = bern.cpu().double().numpy()
    ss, lsi, vs, Sn = _geo_device(shapes, vshapes)
    for use_v in ([None] if vshapes is None else [vshapes, None]):
        coord, idx = S.geo_bezier_inputs(shapes, use_v)
        B, nq = idx.shape
        assert (~proposal_valid_ref(shapes, use_v)[idx]).any()
        exp = bezier64(coord, idx, shapes, use_v, bern64)
        full = _flat_nan_padded(coord)
        sel = _flat_nan_padded(np.take_along_axis(coord, idx[:, :, None], 1))
        idx_d = _ints(idx.reshape(-1))
        outs = []
        for compact, src in ((0, full), (1, sel)):
            out = _sent_f32(B * nq * P * 2 + PAD)
            if use_v is None:
                rc = L.gom_bezier_reference_points(ops._p(src), ops._p(idx_d), ops._p(ss), ops._p(lsi), len(shapes), ops._p(bern),
                                                   ops._p(out), B, Sn, nq, P, compact, ops._stream())
            else:
                rc = L.gom_bezier_reference_points_masked(ops._p(src), ops._p(idx_d), ops._p(ss), ops._p(lsi), ops._p(vs), len(shapes),
                                                          ops._p(bern), ops._p(out), B, Sn, nq, P, compact, ops._stream())
            assert rc == 0
            got = out[:B * nq * P * 2].cpu().double().numpy().reshape(B, nq, P, 2)
            assert _is_sentinel(out[B * nq * P * 2:]) and np.isfinite(got).all(), name
            err = np.abs(got - exp)
            _ratio("bezier_reference_points", err, S.ABS_TABLE)
            assert (err <= S.ABS_TABLE).all(), "%s compact=%d: %.3e" % (name, compact, err.max())
            outs.append(out)
        assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32)), "%s: compact and full differ" % name
        w = ops.bezier_reference_points(sel[:B * nq * 8].view(B * nq, 8), idx_d.view(B, nq), ss, lsi, bern, B, Sn, nq, P, compact=True,
                                        vshapes=None if use_v is None else vs)
        assert tuple(w.shape) == (B, nq, P, 2) and torch.equal(w.reshape(-1), outs[1][:B * nq * P * 2])


# ------------------------------------------------------------------------------------------ detect_post
def _detect_device(case):
    i = case.inputs()
    n = case.B * case.nq * case.P
    return {"cls": _column0(i["cls"].reshape(-1), case.ld_cls),
            "recls": None if i["recls"] is None else _column0(i["recls"].reshape(-1), case.ld_cls),
            "ctrl": _flat_nan_padded(i["ctrl"]), "bd": _flat_nan_padded(i["bd"]),
            "recs": torch.cat([_ints(i["recs"].reshape(-1)), _sent_i32(PAD)]), "n": n}


def _detect_launch(case, dev, nq=None):
    """gom_detect_post with outputs laid out as ops.detect_post lays them out -- count | keep_idx | scores | boxes in one int32
    buffer, ctrl [B, nq, 2 P], bd [B, nq, P, 4], recs [B, nq, P] int64 -- each prefilled with the sentinel and PAD elements longer."""
    ops = _ops()
    B, nq, P = case.B, nq or case.nq, case.P
    small = _sent_i32(B * (1 + 6 * nq) + PAD)
    o1, o2, o3, o4 = B, B + B * nq, B + 2 * B * nq, B * (1 + 6 * nq)
    out = {"small": small, "ends": (o1, o2, o3, o4), "ctrl": _sent_f32(B * nq * P * 2 + PAD), "bd": _sent_f32(B * nq * P * 4 + PAD),
           "recs": torch.full((B * nq * P + PAD,), SENTINEL64, dtype=torch.int64, device=DEV)}
    re = dev["recls"]
    rc = ops._L().gom_detect_post(ops._p(dev["cls"]), case.ld_cls, ops._p(re), case.ld_cls if re is not None else 0, ops._p(dev["ctrl"]),
                                  ops._p(dev["bd"]), ops._p(dev["recs"]), B, nq, P, float(case.hw[0]), float(case.hw[1]),
                                  float(case.det_thr), float(case.nms_thr), float(case.asso_thr), ops._p(small), ops._p(small[o1:]),
                                  ops._p(small[o2:]), ops._p(small[o3:]), ops._p(out["ctrl"]), ops._p(out["bd"]), ops._p(out["recs"]),
                                  ops._stream())
    torch.cuda.synchronize()
    return rc, out


def _detect_check(case, e, count, keep_idx, scores, boxes, ctrl, bd, recs, empty, what):
    """Host arrays in the wrapper's shapes ([B], [B, nq], [B, nq], [B, nq, 4], [B, nq, 2 P], [B, nq, P, 4], [B, nq, P]); `empty(x)`:
    whether every element of x holds what an untouched slot holds."""
    assert count.tolist() == e["count"].tolist(), "%s: count %r, expected %r" % (what, count.tolist(), e["count"].tolist())
    for b in range(case.B):
        n = int(e["count"][b])
        assert np.array_equal(keep_idx[b, :n], e["keep_idx"][b]), "%s frame %d: keep_idx" % (what, b)
        err = np.abs(scores[b, :n].astype(np.float64) - e["scores"][b])
        assert np.isfinite(scores[b, :n]).all() and (err <= e["score_bound"][b]).all(), "%s frame %d: scores" % (what, b)
        _ratio("detect_post score", err, e["score_bound"][b])
        assert np.array_equal(_bits(boxes[b, :n]), _bits(e["boxes"][b])), "%s frame %d: boxes" % (what, b)
        assert np.array_equal(_bits(ctrl[b, :n]), _bits(e["ctrl"][b])), "%s frame %d: ctrl" % (what, b)
        assert np.array_equal(_bits(bd[b, :n]), _bits(e["bd"][b])), "%s frame %d: bd" % (what, b)
        assert np.array_equal(recs[b, :n], e["recs"][b]), "%s frame %d: recs" % (what, b)
        for name, x in (("keep_idx", keep_idx), ("scores", scores), ("boxes", boxes), ("ctrl", ctrl), ("bd", bd), ("recs", recs)):
            assert empty(x[b, n:]), "%s frame %d: %s written past count" % (what, b, name)


def _sentinel_np(x):
    x = np.ascontiguousarray(x)
    return bool((x.view(np.int32) == SENTINEL).all()) if x.size else True


@pytest.mark.parametrize("case", DETECT_CASES, ids=[c.id for c in DETECT_CASES])
def test_detect_post(case):
    B, nq, P = case.B, case.nq, case.P
    e = case.expected()
    rc, out = _detect_launch(case, _detect_device(case))
    assert rc == 0
    o1, o2, o3, o4 = out["ends"]
    small = out["small"].cpu()
    assert _is_sentinel(small[o4:]) and _is_sentinel(out["ctrl"][B * nq * P * 2:]) and _is_sentinel(out["bd"][B * nq * P * 4:]) \
        and _is_sentinel(out["recs"][B * nq * P:]), "%s: wrote past the end of an output" % case.id
    _detect_check(case, e, small[:o1].numpy(), small[o1:o2].numpy().reshape(B, nq), small[o2:o3].view(torch.float32).numpy().reshape(B, nq),
                  small[o3:o4].view(torch.float32).numpy().reshape(B, nq, 4), out["ctrl"][:B * nq * P * 2].cpu().numpy().reshape(B, nq, P * 2),
                  out["bd"][:B * nq * P * 4].cpu().numpy().reshape(B, nq, P, 4), out["recs"][:B * nq * P].cpu().numpy().reshape(B, nq, P),
                  _sentinel_np, case.id)
    if case.kind == "exact":
        assert [small[o1:o2].numpy().reshape(B, nq)[b, :len(h)].tolist() for b, h in enumerate(case.hand)] == \
            [[b * nq + q for q in h] for b, h in enumerate(case.hand)]


@pytest.mark.parametrize("case", [c for c in DETECT_CASES if (c.kind, c.nq) in (("random_clustered", 60), ("exact", 12))],
                         ids=lambda c: c.id)
def test_detect_post_wrapper_contract(case):
    """ops.detect_post: the `small` buffer is count | keep_idx | scores | boxes at small_layout and its views are views of it; padded
    slots of every output are zero; cls with ld_cls > 1 goes in by its stride."""
    ops = _ops()
    B, nq, P = case.B, case.nq, case.P
    dev = _detect_device(case)
    n = dev["n"]
    r = ops.detect_post(dev["cls"][:n], None if dev["recls"] is None else dev["recls"][:n], dev["ctrl"][:n * 2].view(B, nq, P, 2),
                        dev["bd"][:n * 4].view(B, nq, P, 4), dev["recs"][:n], B, nq, P, case.hw[0], case.hw[1], case.det_thr, case.nms_thr,
                        case.asso_thr)
    assert r["small_layout"] == (B, B + B * nq, B + 2 * B * nq) and r["small"].numel() == B * (1 + 6 * nq) and r["small"].dtype == torch.int32
    o1, o2, o3 = r["small_layout"]
    small = r["small"].cpu()
    assert torch.equal(small[:o1], r["count"].cpu()) and torch.equal(small[o1:o2], r["keep_idx"].cpu().reshape(-1))
    assert torch.equal(small[o2:o3], r["scores"].cpu().view(torch.int32).reshape(-1))
    assert torch.equal(small[o3:], r["boxes"].cpu().view(torch.int32).reshape(-1))
    assert r["recs"].dtype == torch.int64 and tuple(r["ctrl"].shape) == (B, nq, P * 2) and tuple(r["bd"].shape) == (B, nq, P, 4)
    _detect_check(case, case.expected(), r["count"].cpu().numpy(), r["keep_idx"].cpu().numpy(), r["scores"].cpu().numpy(),
                  r["boxes"].cpu().numpy(), r["ctrl"].cpu().numpy(), r["bd"].cpu().numpy(), r["recs"].cpu().numpy(),
                  lambda x: not np.ascontiguousarray(x).view(np.uint8).any(), case.id + " wrapper")


def test_detect_post_limits():
    """nq = 1024 is taken (a case of test_detect_post); nq = 1025 returns the library's argument error through ops.check and launches
    nothing."""
    ops = _ops()
    from gomatching_amd.lib import GomError
    case = S.DetectCase("none_selected", 1, 1025, 1, False, (0.3, 0.45), 0.5)
    rc, out = _detect_launch(case, _detect_device(case))
    with pytest.raises(GomError, match="GOM_ERR_INVALID_ARG"):
        ops.check(rc, "gom_detect_post")
    assert _is_sentinel(out["small"]) and _is_sentinel(out["ctrl"]) and _is_sentinel(out["bd"]) and _is_sentinel(out["recs"]), \
        "a refused call wrote to its output"
