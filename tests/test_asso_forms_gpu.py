"""GPU: the tracker's association kernels (csrc/track.hip; track_score_one, asso_score_block and gather_match_item of
csrc/tracker_tasks.h) against the fp64 statements of tests/asso_statement.py, element-wise within their derived bounds, on the
cases and inputs of that file -- tests/test_asso_statement_cpu.py shows on the same bits that the bounds hold an fp32 evaluation in
the kernels' order and do not hold the mistakes planted there.

Every call reads its operands from NaN-padded buffers (gap columns where ld > N, a row past the used part of every allocation) and
writes into a buffer prefilled with a sentinel bit pattern, which every element the op does not own must keep.  The only assertion
on accuracy is |got - exp| <= bound; the worst |got - exp| / bound per form is printed at the end (docs/LAB_NOTES.md keeps a
record)."""
import numpy as np
import pytest
import torch

from asso_statement import ASSO_CASES, BOX_KINDS, GATHER_CASES, LOGIT_KINDS, SHORT_CASES, AssoCase, image_of

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENTINEL = 0x7FC0DEAD                                 # a NaN with a payload: an element left unwritten is also not finite
RATIOS = {}


def _ops():
    from gomatching_amd import ops
    return ops


def _sentinel_buffer(*shape):
    return torch.full(shape, SENTINEL, dtype=torch.int32, device=DEV).view(torch.float32)


def _padded(x, ld=None):
    """x [r, n] (numpy float32) -> a device buffer [r + 1, ld] full of NaN with x in its corner."""
    x = np.atleast_2d(np.asarray(x, np.float32))
    buf = torch.full((x.shape[0] + 1, ld or x.shape[1]), float("nan"))
    buf[:x.shape[0], :x.shape[1]] = torch.from_numpy(x)
    return buf.to(DEV)


def _ints(x):
    return torch.from_numpy(np.ascontiguousarray(x, np.int32)).to(DEV)


def _check(out, exp, bound, form, what):
    """out: the whole output buffer; exp / bound: float64 arrays of its shape with NaN where the op owns nothing.  Owned elements
    are finite and within the bound, every other element keeps the sentinel's bits; the form's worst ratio is recorded."""
    out = out.detach().cpu().reshape(-1)
    exp, bound = torch.from_numpy(np.asarray(exp, np.float64)).reshape(-1), torch.from_numpy(np.asarray(bound, np.float64)).reshape(-1)
    assert out.numel() == exp.numel() == bound.numel()
    own = ~torch.isnan(exp)
    got = out[own].double()
    assert bool(torch.isfinite(got).all()), "%s: %d outputs are not finite" % (what, int((~torch.isfinite(got)).sum()))
    err, b = (got - exp[own]).abs(), bound[own]
    ok = err <= b
    if not bool(ok.all()):
        at = int((~ok).nonzero()[0])
        raise AssertionError("%s: %d elements out of bound, first at owned element %d: got %r exp %r bound %.3e" % (
            what, int((~ok).sum()), at, float(got[at]), float(exp[own][at]), float(b[at])))
    assert bool((out.view(torch.int32)[~own] == SENTINEL).all()), "%s: wrote outside its output block" % what
    pos = b > 0
    if bool(pos.any()):
        RATIOS[form] = max(RATIOS.get(form, 0.0), float((err[pos] / b[pos]).max()))


def _pad_to(a, shape):
    full = np.full(shape, np.nan)
    full[tuple(slice(0, n) for n in a.shape)] = a
    return full


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for k, v in sorted(RATIOS.items()):
        print("association worst |got-exp| / bound  %-22s %.4f" % (k, v))


# ------------------------------------------------------------------------------------------ activate, track score, one launch
def _asso_device(case, box_kind):
    img_w, img_h = image_of(box_kind)
    return {"offs": _ints(case.offs), "meta": _ints(case.meta), "boxes": _padded(case.boxes(box_kind)),
            "decay": None if case.decay is None else _padded(case.decay[None])[0], "img": (img_w, img_h)}


def _run_asso(case, dev, logits, expected):
    """The two launches and the one launch on one input set, each against the statement; the one launch gives the two launches'
    bits.  -> the one launch's scores [n_k, M] on the host."""
    ops = _ops()
    (aexp, abound), (texp, tbound, gate) = expected
    n_k, N, M, Np = case.n_k, case.N, case.M, case.Np
    lb = _padded(logits, case.ld)
    lv = lb[:n_k, :N]
    img_w, img_h = dev["img"]
    what = case.id
    # asso_activate: ld_out = N + 2, so the columns past N (an empty last segment ends there) are watched too
    act = _sentinel_buffer(n_k + 1, N + 2)
    ops.asso_activate(lv, dev["offs"], case.T, out=act[:n_k])
    _check(act, _pad_to(aexp, (n_k + 1, N + 2)), _pad_to(abound, (n_k + 1, N + 2)), "asso_activate", what + " activate")
    # track_score on the kernel's own activations (NaN sentinels in their gap columns)
    two = _sentinel_buffer(n_k * M + 8)
    ops.track_score(act[:n_k, :N], dev["meta"], dev["decay"], dev["boxes"], img_w, img_h, n_k, Np, M, case.with_iou, case.mcd, out=two)
    _check(two, _pad_to(texp.reshape(-1), (n_k * M + 8,)), _pad_to(tbound.reshape(-1), (n_k * M + 8,)), "track_score",
           what + " track score")
    one = _sentinel_buffer(n_k * M + 8)
    ops.asso_score(lv, dev["offs"], case.T, dev["meta"], dev["decay"], dev["boxes"], img_w, img_h, n_k, Np, M, case.with_iou,
                   case.mcd, out=one)
    _check(one, _pad_to(texp.reshape(-1), (n_k * M + 8,)), _pad_to(tbound.reshape(-1), (n_k * M + 8,)), "asso_score",
           what + " one launch")
    assert torch.equal(one.view(torch.int32), two.view(torch.int32)), "%s: %d scores of the one launch differ from the two launches" % (
        what, int((one.view(torch.int32) != two.view(torch.int32)).sum()))
    return one[:n_k * M].cpu().view(n_k, M)


@pytest.mark.parametrize("box_kind", BOX_KINDS)
@pytest.mark.parametrize("case", ASSO_CASES, ids=[c.id for c in ASSO_CASES])
def test_activate_track_score_and_one_launch(case, box_kind):
    """gom_asso_activate_f32, gom_track_score_f32 and gom_asso_score_f32 on every logit kind of the case.  Exact boxes: the planted
    pair with dist == max_center_dist is invalid and every other decision is the fp32 reference's -- a score is 0 exactly where the
    reference's gate closes (looked at on the randn logits, where no activation underflows)."""
    dev = _asso_device(case, box_kind)
    for kind in LOGIT_KINDS:
        expected = case.expected(kind, box_kind)
        got = _run_asso(case, dev, case.logits(kind), expected)
        texp, gate = expected[1][0], expected[1][2]
        if gate is not None and kind == "randn":
            assert torch.equal(got != 0, torch.from_numpy(texp != 0)), "%s %s: a gate decision differs" % (case.id, box_kind)
            if case.M >= 2:
                assert float(got[0, 0]) == 0.0


def test_one_launch_limits():
    """gom_asso_score_f32 takes N = 16 384 (a 64 KB LDS row; n_k = 2, M = 2, T = 3 with an empty segment) and is within the bound
    there, with the two launches' bits; N = 16 385 and ld < N are refused by return code and launch nothing."""
    ops = _ops()
    case = AssoCase(100, "N16384", [16382, 0, 2], 2, 2, True, 1, 0.5, 0)
    dev = _asso_device(case, "random")
    _run_asso(case, dev, case.logits("randn"), case.expected("randn", "random"))
    L = ops._L()
    out = _sentinel_buffer(16)
    big = torch.zeros((2, 16385), device=DEV)
    meta = torch.zeros((2 * 16383 + 2 + 2,), dtype=torch.int32, device=DEV)
    offs = _ints([0, 16383, 16385])

    def call(ld, Np, n_k):
        return L.gom_asso_score_f32(ops._p(big), ld, ops._p(offs), 2, ops._p(meta), None, ops._p(dev["boxes"]), 1.0, 1.0, n_k, Np, 2, 0,
                                    0.0, ops._p(out), ops._stream())
    assert call(16385, 16383, 2) == 1                                                  # N = 16 385
    assert call(16383, 16382, 2) == 1                                                  # ld < N = 16 384
    torch.cuda.synchronize()
    assert bool((out.view(torch.int32) == SENTINEL).all()), "a refused call wrote to its output"


# ------------------------------------------------------------------------------------------ short-term pairs
def _short_device(case, logit_kind, box_kind):
    tgt, mem = case.inputs(logit_kind)
    return {"tgt": _padded(tgt), "mem": _padded(mem), "boxes": _padded(case.boxes(box_kind)), "pairs": _ints(case.pairs.reshape(-1)),
            "row_pair": _ints(case.row_pair), "img": image_of(box_kind)}


def _short_launch(case, dev, tgt, pairs, row_pair, rows, max_prev, s_floats):
    S = _sentinel_buffer(s_floats + 5)
    _ops().short_term_pairs(tgt, dev["mem"], pairs, row_pair, dev["boxes"], dev["img"][0], dev["img"][1], case.with_iou, rows, max_prev,
                            s_floats, out=S)
    return S


@pytest.mark.parametrize("box_kind", BOX_KINDS)
@pytest.mark.parametrize("case", SHORT_CASES, ids=[c.id for c in SHORT_CASES])
def test_short_term_pairs(case, box_kind):
    """gom_short_term_pairs_f32 against short_term64 on every logit kind; then (randn) each pair launched alone gives the bits it has
    inside the ragged launch, and a row's result does not depend on the other rows of its launch (they are replaced by NaN)."""
    for kind in LOGIT_KINDS:
        dev = _short_device(case, kind, box_kind)
        exp, bound = case.expected(kind, box_kind)
        S = _short_launch(case, dev, dev["tgt"], dev["pairs"], dev["row_pair"], case.rows, case.max_prev, case.s_floats)
        _check(S, _pad_to(exp, (case.s_floats + 5,)), _pad_to(bound, (case.s_floats + 5,)), "short_term_pairs",
               "%s %s %s" % (case.id, kind, box_kind))
        if kind != "randn":
            continue
        bits = S.view(torch.int32)
        for m0, n_prev, n_cur, t0, b0, s_off in case.pairs.tolist():
            alone = _short_launch(case, dev, dev["tgt"][t0:], _ints([m0, n_prev, n_cur, 0, b0, 0]), _ints([0] * n_cur), n_cur, n_prev,
                                  n_cur * n_prev)
            assert torch.equal(alone.view(torch.int32)[:n_cur * n_prev], bits[s_off:s_off + n_cur * n_prev]), \
                "%s: pair at S offset %d alone differs from the ragged launch" % (case.id, s_off)
            assert bool((alone.view(torch.int32)[n_cur * n_prev:] == SENTINEL).all())
        for w in (0, case.rows // 2, case.rows - 1):
            tgt = torch.full_like(dev["tgt"], float("nan"))
            tgt[w] = dev["tgt"][w]
            lone = _short_launch(case, dev, tgt, dev["pairs"], dev["row_pair"], case.rows, case.max_prev, case.s_floats)
            m0, n_prev, n_cur, t0, b0, s_off = case.pairs[int(case.row_pair[w])].tolist()
            o = s_off + (w - t0) * n_prev
            assert torch.equal(lone.view(torch.int32)[o:o + n_prev], bits[o:o + n_prev]), "%s: row %d depends on other rows" % (case.id, w)


def test_short_term_limits():
    """max_prev = 320 is taken (the d260 and d1024 cases run it), 321 is refused by return code and launches nothing."""
    ops = _ops()
    case = [c for c in SHORT_CASES if c.max_prev == 320][0]
    dev = _short_device(case, "randn", "random")
    S = _sentinel_buffer(case.s_floats)

    def call(max_prev):
        return ops._L().gom_short_term_pairs_f32(ops._p(dev["tgt"]), ops._p(dev["mem"]), case.d, ops._p(dev["pairs"]),
                                                 ops._p(dev["row_pair"]), ops._p(dev["boxes"]), 1.0, 1.0, 0, case.rows, max_prev,
                                                 ops._p(S), ops._stream())
    assert call(321) == 1
    torch.cuda.synchronize()
    assert bool((S.view(torch.int32) == SENTINEL).all()), "a refused call wrote to its output"
    assert call(320) == 0
    torch.cuda.synchronize()
    assert bool(torch.isfinite(S).all())


# ------------------------------------------------------------------------------------------ gathers
def _gather_match(case, pool, proj, rows, N, lo, n_k, d, outs):
    ops = _ops()
    return ops._L().gom_gather_match_f32(ops._p(pool), case.ld_pool, ops._p(proj), case.ld_proj, ops._p(rows), N, lo, n_k, d,
                                         ops._p(outs[0]), ops._p(outs[1]), ops._p(outs[2]), ops._stream())


def _gather_buffers(case):
    return [_sentinel_buffer(case.N * case.d + 4), _sentinel_buffer(case.N * 3 * case.d + 4), _sentinel_buffer(case.n_k * case.d + 4)]


def _exact(out, want, what):
    out = out.cpu()
    n = want.size
    assert torch.equal(out[:n].view(torch.int32), torch.from_numpy(np.ascontiguousarray(want, np.float32)).reshape(-1).view(torch.int32)), what
    assert bool((out[n:].view(torch.int32) == SENTINEL).all()), what + ": wrote outside its output block"


@pytest.mark.parametrize("case", GATHER_CASES, ids=[c.id for c in GATHER_CASES])
def test_gathers_are_exact(case):
    """gom_gather_match_f32 (ld_pool > d, ld_proj > 4 d, NaN in the gap columns) and gom_gather_rows_f32 (dense rows): the bits of
    torch indexing, the sentinel everywhere else."""
    ops = _ops()
    pool, proj = case.inputs()
    src, qkv, qdec = case.expected(pool, proj)
    pool_d, proj_d, rows = torch.from_numpy(pool).to(DEV), torch.from_numpy(proj).to(DEV), _ints(case.rows)
    outs = _gather_buffers(case)
    assert _gather_match(case, pool_d, proj_d, rows, case.N, case.lo, case.n_k, case.d, outs) == 0
    for out, want, name in zip(outs, (src, qkv, qdec), ("src", "qkv", "qdec")):
        _exact(out, want, "%s %s" % (case.id, name))
    dense = torch.from_numpy(np.ascontiguousarray(pool[:, :case.d])).to(DEV)
    out = _sentinel_buffer(case.N * case.d + 4)
    assert ops._L().gom_gather_rows_f32(ops._p(dense), ops._p(rows), ops._p(out), case.N, case.d, ops._stream()) == 0
    _exact(out, src, "%s gather_rows" % case.id)


def test_gather_match_limits():
    """lo + n_k > N and a dim that 4 does not divide are refused by return code and launch nothing."""
    case = [c for c in GATHER_CASES if c.N == 5 and c.d == 4][0]
    pool, proj = case.inputs()
    pool_d, proj_d, rows = torch.from_numpy(pool).to(DEV), torch.from_numpy(proj).to(DEV), _ints(case.rows)
    outs = [_sentinel_buffer(256) for _ in range(3)]
    assert _gather_match(case, pool_d, proj_d, rows, 5, 4, 2, 4, outs) == 1
    assert _gather_match(case, pool_d, proj_d, rows, 5, 0, 1, 3, outs) == 1
    assert _gather_match(case, pool_d, proj_d, rows, 5, 0, 1, 6, outs) == 1
    torch.cuda.synchronize()
    for out in outs:
        assert bool((out.view(torch.int32) == SENTINEL).all()), "a refused call wrote to its output"
