"""GPU: every form of the six launches of a composite decoder layer (csrc/dec_attn.hip, dec_attn2.hip, dec_inter.hip, proj_ln.hip,
ffn_fused.hip, dec_tail.hip, dec_tail2.hip) against the float64 statements of tests/dec_statement.py, ELEMENTWISE within their
derived bounds, on the case tables and input kinds of that file -- tests/test_dec_statement_cpu.py shows on the same bits that the
bounds hold an fp32 emulation of the kernels' arithmetic and do not hold the planted mistakes (eps, the max subtraction, a
dropped or misplaced key, the sine embedding's layout ...).

Every input is a row-strided view (ld 256, 260 or 384) into a NaN-filled buffer with NaN rows in front and behind; every `out=` an
op accepts is such a view into a buffer prefilled with a NaN-payload sentinel, which everything outside the owned block must keep.
Outputs the ops allocate themselves (raw, mlp2_fused, proj_ln_dot, dec_tail's three) are checked for shape, finiteness and the
bound.  The range flag must stay down after every call.  The only assertion on accuracy is |got - exp| <= bound; the worst
|got - exp| / bound per form is printed at the end.

Not tested: form-1 dec_tail with proj_w and the output aliasing an input -- unreachable while ops.dec_tail allocates its outputs."""
import functools

import pytest
import torch

import dec_statement as S

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENTINEL = 0x7FC0DEAD                                 # a NaN with a payload: an element left unwritten is also not finite
RATIOS = {}
LDS = (256, 260, 384)
COL = {256: 0, 260: 4, 384: 64}                       # first column of the view inside its buffer: 16-byte aligned
FRONT, BACK = 2, 3


def _ops():
    from gomatching_amd import ops
    return ops


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for k, v in sorted(RATIOS.items()):
        print("decoder worst |got-exp| / bound  %-28s %.4f" % (k, v))


def _in(t, ld, extra=0):
    """t [rows, 256] as a view [rows + extra, 256] of a NaN-filled [FRONT + rows + extra + BACK, ld] device buffer (the extra rows NaN)."""
    rows = t.shape[0] + extra
    buf = torch.full((FRONT + rows + BACK, ld), float("nan"))
    buf[FRONT:FRONT + t.shape[0], COL[ld]:COL[ld] + 256] = t
    return buf.to(DEV)[FRONT:FRONT + rows, COL[ld]:COL[ld] + 256]


def _out(rows, ld):
    buf = torch.full((FRONT + rows + BACK, ld), SENTINEL, dtype=torch.int32, device=DEV).view(torch.float32)
    return buf, buf[FRONT:FRONT + rows, COL[ld]:COL[ld] + 256]


def _flag_down(what):
    try:
        _ops().check_range_flag(DEV)
    except Exception as e:                                               # noqa: BLE001 -- reported with the case's name
        raise AssertionError("%s: the range flag went up on clean data (%s)" % (what, e))


def _within(got, exp, bound, form, what):
    got = got.detach().cpu().double()
    assert tuple(got.shape) == tuple(exp.shape), "%s: shape %s, expected %s" % (what, tuple(got.shape), tuple(exp.shape))
    assert bool(torch.isfinite(got).all()), "%s: %d outputs are not finite" % (what, int((~torch.isfinite(got)).sum()))
    err = (got - exp).abs()
    ok = err <= bound
    if not bool(ok.all()):
        at = tuple(int(i) for i in (~ok).nonzero()[0])
        raise AssertionError("%s: %d elements out of bound, first at %s: got %r exp %r bound %.3e" % (
            what, int((~ok).sum()), at, float(got[at]), float(exp[at]), float(bound[at])))
    RATIOS[form] = max(RATIOS.get(form, 0.0), float((err / bound).max()) if err.numel() else 0.0)


def _owned(buf, view_rows, ld, order, exp, bound, form, what):
    """The first `view_rows` rows of the view inside sentinel buffer `buf` are the op's: row order[i] is exp[i].  Everything else
    in the buffer keeps the sentinel's bits."""
    host = buf.cpu()
    block = host[FRONT:FRONT + view_rows, COL[ld]:COL[ld] + 256]
    _within(block[order], exp, bound, form, what)
    keep = torch.ones(host.shape, dtype=torch.bool)
    keep[FRONT:FRONT + view_rows, COL[ld]:COL[ld] + 256][order] = False
    assert bool((host.view(torch.int32)[keep] == SENTINEL).all()), "%s: wrote outside its output block" % what
    return block


def _dev(*ts):
    return [None if t is None else t.to(DEV) for t in ts]


# ------------------------------------------------------------------------------------------ the attention blocks
@functools.lru_cache(maxsize=None)
def _block(kind, inter, raw, form):
    ops = _ops()
    w = S.block_weights(kind)
    d = {k: v.to(DEV) for k, v in w.items()}
    return ops.DecAttnBlock(d["in_w"], d["in_b"], d["out_w"], d["out_b"], d["gamma"], d["beta"], inter,
                            raw=(d["raw_w"], d["raw_b"]) if raw else None, form=form)


@functools.lru_cache(maxsize=None)
def _block_expect(layout, case, kind):
    """Inputs and expectation of one block case, computed once and shared by the forms (read-only)."""
    index = S.intra_index(*case) if layout == "intra" else S.inter_index(*case)
    extra = 3 if layout == "intra" else 0
    x, pos = S.block_inputs(kind, index.numel() + extra, index, layout == "intra", S.seed_of(*case), layout)
    w = S.block_weights(kind)
    return index, x, pos, S.self_attn_block64(x, pos, w, index)


def _same_rows(block, index, kind, what):
    if kind == "same":
        rows = block[index].view(torch.int32)                            # [n, G, 256]
        assert bool((rows == rows[:, :1]).all()), "%s: identical tokens of a group left with different bits" % what


@pytest.mark.parametrize("kind", S.BLOCK_KINDS)
@pytest.mark.parametrize("form", [1, 2])
def test_intra_forms(form, kind):
    ops = _ops()
    blk = _block(kind, False, False, form)
    for n, case in enumerate(S.INTRA_CASES):
        groups, G = case
        index, x, pos, (exp, bound) = _block_expect("intra", case, kind)
        rows = groups * G
        what = "intra form %d %s %s" % (form, case, kind)
        xd = _in(x[:rows], LDS[n % 3], extra=3)                          # x.shape[0] > rows: the launch stops at the groups
        pd = _in(pos[:rows], LDS[(n + 1) % 3], extra=3)
        buf, out = _out(rows + 3, LDS[(n + 2) % 3])
        ops.dec_attn(xd, blk, groups, G, pos=pd, out=out)
        _flag_down(what)
        block = _owned(buf, rows, LDS[(n + 2) % 3], index.reshape(-1), exp, bound, "intra form %d" % form, what)
        _same_rows(block, index, kind, what)


@pytest.mark.parametrize("kind", S.BLOCK_KINDS)
@pytest.mark.parametrize("form", [1, 2])
def test_inter_forms_with_and_without_raw(form, kind):
    ops = _ops()
    plain, with_raw = _block(kind, True, False, form), _block(kind, True, True, form)
    w = S.block_weights(kind)
    for n, case in enumerate(S.INTER_CASES):
        B, nq, P = case
        index, x, _, (exp, bound) = _block_expect("inter", case, kind)
        rows = index.numel()
        what = "inter form %d %s %s" % (form, case, kind)
        ldo = LDS[(n + 2) % 3]
        xd = _in(x, LDS[n % 3])
        buf, out = _out(rows, ldo)
        ops.dec_attn(xd, plain, B * P, nq, inner=P, out=out)
        _flag_down(what)
        block = _owned(buf, rows, ldo, index.reshape(-1), exp, bound, "inter form %d" % form, what)
        _same_rows(block, index, kind, what)
        qpos = S.rows_input("lowvar" if kind == "lowvar" else "randn", rows, 11)[1] * 0.7
        buf2, out2 = _out(rows, ldo)
        got, raw = ops.dec_attn(xd, with_raw, B * P, nq, inner=P, out=out2, raw_pos=_in(qpos, LDS[(n + 1) % 3]))
        _flag_down(what + " +raw")
        block2 = _owned(buf2, rows, ldo, index.reshape(-1), exp, bound, "inter+raw form %d (out)" % form, what + " +raw")
        assert torch.equal(block2.view(torch.int32), block.view(torch.int32)), "%s: out of the raw form is not the plain form's bits" % what
        order = torch.empty(rows, dtype=torch.long)
        order[index.reshape(-1)] = torch.arange(rows)
        rexp, rbound = S.raw64(exp[order], bound[order], qpos, w["raw_w"], w["raw_b"])      # rows in memory order
        assert tuple(raw.shape) == (rows, 384)
        _within(raw, rexp, rbound, "inter+raw form %d (raw)" % form, what + " raw")


@pytest.mark.parametrize("kind", S.BLOCK_KINDS)
def test_inter_heads_and_proj_ln(kind):
    """More than 128 queries per group: csrc/dec_inter.hip's head outputs, then the proj_ln launch.  The entry also accepts groups of
    at most 128 tokens (waves without a block): they must be right too."""
    ops = _ops()
    blk = _block(kind, True, False, 1)
    w = S.block_weights(kind)
    d = {k: v.to(DEV) for k, v in w.items()}
    pl = ops.ProjLN(ops.split_weight(d["out_w"], kind="f16x3"), d["out_b"], d["gamma"], d["beta"])
    for n, case in enumerate(S.HEADS_CASES):
        B, nq, P = case
        index, x, _, (exp, bound) = _block_expect("heads", case, kind)
        rows = index.numel()
        what = "inter heads %s %s" % (case, kind)
        ldh = LDS[(n + 1) % 3]
        xd = _in(x, LDS[n % 3])
        buf, heads = _out(rows, ldh)
        ops.dec_inter_heads(xd, blk, B * P, nq, inner=P, out=heads)
        _flag_down(what)
        hexp, hbound = S.heads64(x, None, w, index)
        _owned(buf, rows, ldh, index.reshape(-1), hexp, hbound, "inter heads", what)
        ldo = LDS[(n + 2) % 3]
        buf2, out = _out(rows, ldo)
        ops.proj_ln(heads, pl, xd, out=out)
        _flag_down(what + " proj_ln")
        block = _owned(buf2, rows, ldo, index.reshape(-1), exp, bound, "inter heads + proj_ln", what + " proj_ln")
        _same_rows(block, index, kind, what)


# ------------------------------------------------------------------------------------------ the row ops
@pytest.mark.parametrize("kind", S.LN_KINDS)
def test_proj_ln_forms(kind):
    ops = _ops()
    W, b, ga, be, cw, cb = S.ln_weights(kind)
    Wd, bd, gd, bed, cwd = _dev(W, b, ga, be, cw)
    blk = ops.ProjLN(ops.split_weight(Wd, kind="f16x3"), bd, gd, bed)
    for n, M in enumerate(S.PROJ_LN_M):
        x, R = S.rows_input(kind, M, S.seed_of(M, 1))
        what = "proj_ln M=%d %s" % (M, kind)
        xd, Rd, ldo = _in(x, LDS[n % 3]), _in(R, LDS[(n + 1) % 3]), LDS[(n + 2) % 3]
        buf, out = _out(M, ldo)
        ops.proj_ln(xd, blk, Rd, out=out)
        _flag_down(what)
        exp, bound = S.proj_ln64(x, W, b, R, ga, be)
        _owned(buf, M, ldo, torch.arange(M), exp, bound, "proj_ln R", what)
        if kind == "offset":                                             # the residual path's kind
            continue
        buf, out = _out(M, ldo)
        ops.proj_ln(xd, blk, None, out=out)
        _flag_down(what + " no R")
        exp, bound = S.proj_ln64(x, W, b, None, ga, be)
        _owned(buf, M, ldo, torch.arange(M), exp, bound, "proj_ln none", what + " no R")
        dot = ops.proj_ln_dot(xd, blk, cwd, cb)
        _flag_down(what + " dot")
        exp, bound = S.proj_ln_dot64(x, W, b, ga, be, cw, cb)
        _within(dot, exp, bound, "proj_ln_dot", what + " dot")


@pytest.mark.parametrize("kind", S.LN_KINDS)
def test_ffn_and_perceptron_forms(kind):
    ops = _ops()
    for Fh in S.FFN_F:
        ffn = S.ln_weights(kind, Fh)
        blk = ops.FusedFFN(*_dev(*ffn))
        for n, M in enumerate(S.FFN_M):
            x = S.ffn_case(kind, M)
            what = "ffn_fused_ln M=%d F=%d %s" % (M, Fh, kind)
            ldo = LDS[(n + 1) % 3]
            buf, out = _out(M, ldo)
            ops.ffn_fused_ln(_in(x, LDS[n % 3]), blk, out=out)
            _flag_down(what)
            exp, bound = S.ffn_ln64(x, *ffn)
            _owned(buf, M, ldo, torch.arange(M), exp, bound, "ffn_fused_ln", what)
    if kind == "offset":
        return
    w1, b1, w2, b2 = S.ln_weights(kind, 256)[:4]
    for relu_out in (False, True):
        blk = ops.FusedMLP2(*_dev(w1, b1, w2, b2), relu_out)
        for n, M in enumerate(S.FFN_M):
            x = S.rows_input(kind, M, S.seed_of(M, 2))[0]
            what = "mlp2_fused M=%d relu_out=%s %s" % (M, relu_out, kind)
            got = ops.mlp2_fused(_in(x, LDS[n % 3]), blk)
            _flag_down(what)
            exp, bound = S.mlp2_64(x, w1, b1, w2, b2, relu_out)
            _within(got, exp, bound, "mlp2_fused", what)


# ------------------------------------------------------------------------------------------ the tail
def _tail_blk(form, kind, Fh, with_proj, eps):
    ops = _ops()
    ffn, coord, qpos, proj = S.tail_weights(kind, Fh)
    pair = lambda p: tuple(_dev(*p))
    return ops.DecTail(pair(ffn), [pair(p) for p in coord], [pair(p) for p in qpos], S.dim_t128().to(DEV), eps=eps,
                       proj_w=pair(proj) if with_proj else None, **S.TAIL_FORMS[form])


@functools.lru_cache(maxsize=None)
def _tail_expect(kind, M, Fh, with_proj):
    ffn, coord, qpos, proj = S.tail_weights(kind, Fh)
    x, R, ref, eps = S.tail_case(kind, M, Fh, with_proj)
    kw = dict(proj=proj, residual=R) if with_proj else {}
    return x, R, ref, eps, S.tail64(x, ffn, coord, qpos, ref, S.dim_t128(), eps=eps, **kw)


@pytest.mark.parametrize("with_proj", [False, True], ids=["plain", "proj"])
@pytest.mark.parametrize("kind", S.TAIL_KINDS)
@pytest.mark.parametrize("form", list(S.TAIL_FORMS))
def test_dec_tail_forms(form, kind, with_proj):
    ops = _ops()
    name = "dec_tail %s%s" % (form, " +proj" if with_proj else "")
    for Fh in S.tail_F(form):
        blks = {1e-5: _tail_blk(form, kind, Fh, with_proj, 1e-5)}
        assert blks[1e-5].form == S.TAIL_FORMS[form]["form"]
        for n, M in enumerate(S.TAIL_M):
            x, R, ref, eps, exp = _tail_expect(kind, M, Fh, with_proj)
            if eps not in blks:
                blks[eps] = _tail_blk(form, kind, Fh, with_proj, eps)     # DecTail(..., eps=3e-5): a hard-coded 1e-5 shows
            xd = _in(x, LDS[n % 3])
            Rd = _in(R, LDS[(n + 1) % 3]) if with_proj else None
            for want in (True, False):
                what = "%s M=%d F=%d %s qpos=%s" % (name, M, Fh, kind, want)
                y, nref, qp = ops.dec_tail(xd, blks[eps], ref.to(DEV), want_qpos=want, residual=Rd)
                _flag_down(what)
                assert (qp is None) == (not want)
                _within(y, exp[0][0], exp[0][1], name + " (tgt)", what + " tgt")
                _within(nref, exp[1][0], exp[1][1], name + " (ref)", what + " ref")
                if want:
                    _within(qp, exp[2][0], exp[2][1], name + " (qpos)", what + " qpos")


# ------------------------------------------------------------------------------------------ refusals
def test_refusals():
    """Every check returns before any launch: GomError (or the op's own assertion), and the output keeps the sentinel."""
    ops = _ops()
    from gomatching_amd.lib import GomError
    intra, inter = _block("randn", False, False, 2), _block("randn", True, False, 2)
    intra1, inter1 = _block("randn", False, False, 1), _block("randn", True, False, 1)
    z = lambda rows, ld=256, col=0: torch.zeros((rows + 1, ld), device=DEV)[:rows, col:col + 256]

    def refused(call, rows, ld=256, col=0):
        buf = torch.full((rows + 1, ld), SENTINEL, dtype=torch.int32, device=DEV).view(torch.float32)
        with pytest.raises((GomError, AssertionError)):
            call(buf[:rows, col:col + 256])
        torch.cuda.synchronize()
        assert bool((buf.view(torch.int32) == SENTINEL).all()), "a refused call wrote to its output"

    for blk in (intra, intra1):                                          # intra with G = 33
        refused(lambda o: ops.dec_attn(z(66), blk, 2, 33, pos=z(66), out=o), 66)
    for blk in (inter, inter1):                                          # inter with G = 129 through dec_attn
        refused(lambda o: ops.dec_attn(z(258), blk, 2, 129, inner=1, out=o), 258)
    refused(lambda o: ops.dec_inter_heads(z(353), inter1, 1, 353, 1, out=o), 353)
    # a base pointer misaligned by 4 bytes (input, then output), and a leading dimension that is no multiple of 4
    for blk in (intra, intra1):
        refused(lambda o: ops.dec_attn(z(50, 260, 1), blk, 2, 25, pos=z(50), out=o), 50)
        refused(lambda o: ops.dec_attn(z(50), blk, 2, 25, pos=z(50), out=o), 50, 260, 1)
        refused(lambda o: ops.dec_attn(z(50, 258), blk, 2, 25, pos=z(50), out=o), 50)
        refused(lambda o: ops.dec_attn(z(50), blk, 2, 25, pos=z(50, 258), out=o), 50)
    for blk in (inter, inter1):
        refused(lambda o: ops.dec_attn(z(50, 260, 1), blk, 2, 25, inner=1, out=o), 50)
        refused(lambda o: ops.dec_attn(z(50), blk, 2, 25, inner=1, out=o), 50, 258, 0)
    refused(lambda o: ops.dec_inter_heads(z(300, 260, 1), inter1, 2, 150, 1, out=o), 300)
    refused(lambda o: ops.dec_inter_heads(z(300, 258), inter1, 2, 150, 1, out=o), 300)
    W, b, ga, be, _, _ = S.ln_weights("randn")
    Wd, bd, gd, bed = _dev(W, b, ga, be)
    pl = ops.ProjLN(ops.split_weight(Wd, kind="f16x3"), bd, gd, bed)
    refused(lambda o: ops.proj_ln(z(20, 260, 1), pl, z(20), out=o), 20)
    refused(lambda o: ops.proj_ln(z(20), pl, z(20, 258), out=o), 20)
    ffn = ops.FusedFFN(*_dev(*S.ln_weights("randn", 96)))
    refused(lambda o: ops.ffn_fused_ln(z(20, 260, 1), ffn, out=o), 20)
    refused(lambda o: ops.ffn_fused_ln(z(20, 258), ffn, out=o), 20)
    with pytest.raises((GomError, AssertionError)):                      # form 2 takes the hidden layer in chunks of 128
        _tail_blk("form2-4waves", "randn", 96, False, 1e-5)
    tail = _tail_blk("form1", "randn", 96, False, 1e-5)
    for bad in (z(20, 260, 1), z(20, 258)):
        with pytest.raises((GomError, AssertionError)):
            ops.dec_tail(bad, tail, torch.rand(20, 2, device=DEV))
    _flag_down("after the refusals")
    index, x, pos, (exp, bound) = _block_expect("intra", (5, 25), "randn")      # and the next valid call is as usual
    buf, out = _out(128, 256)
    ops.dec_attn(_in(x[:125], 256, extra=3), intra, 5, 25, pos=_in(pos[:125], 256, extra=3), out=out)
    _owned(buf, 125, 256, index.reshape(-1), exp, bound, "intra form 2", "after the refusals")
