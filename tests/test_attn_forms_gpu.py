"""GPU: every form of the softmax attention core (csrc/attn.hip; mha_tiny128_task of csrc/tracker_tasks.h) against the fp64
statement of tests/helpers.py (attention64), element-wise within its derived bound, on the inputs and views of
helpers.ATTN_CASES -- tests/test_attn_statement_cpu.py shows on the same bits that the bound holds an fp32 evaluation and
does not hold a dropped key, a swapped V row, a wrong scale, another head's K or swapped batch strides.

Forms behind ops.mha_core: mha_rows_kernel<32>, mha_core_kernel<32,32>, <32,8>, mha_tiny128_kernel, mha_core_kernel<128,32>,
<128,8>; ops.mha_core_segments runs <128,32> or <128,8> over per-block segment descriptors.  The form labels follow the
dispatch conditions of gom_mha_core_f32 as read from the source and only group the report: no test fails if a shape reaches
another kernel.  One kernel trace of this file (docs/LAB_NOTES.md) showed every kernel with the launch count the table gives.

Every call reads its operands from NaN-filled buffers (gap columns, rows past Lq / Lk inside the allocation) and writes into a
buffer prefilled with a sentinel bit pattern, which every element outside the [Lq, heads * hd] block of each batch must keep.
The only assertion on accuracy is |got - exp| <= bound; the worst |got - exp| / bound per form is printed at the end."""
import pytest
import torch

from helpers import (ATTN_CASES, ATTN_SEGMENT_KINDS, ATTN_SEGMENTS, attention64, attention64_views, attn_index, attn_inputs,
                     attn_pack, attn_segment_inputs)

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENTINEL = 0x7FC0DEAD                                 # a NaN with a payload: an element left unwritten is also not finite
RATIOS = {}


def _ops():
    from gomatching_amd import ops
    return ops


def _sentinel_buffer(n):
    return torch.full((n,), SENTINEL, dtype=torch.int32, device=DEV).view(torch.float32)


def _check(out, idx, exp, bound, form, what):
    """out: the flat output buffer; idx: the elements the op owns.  They are finite and within the bound, every other element
    keeps the sentinel's bits; the form's worst |got - exp| / bound is recorded."""
    out = out.cpu()
    got = out[idx].double()
    assert bool(torch.isfinite(got).all()), "%s: %d outputs are not finite" % (what, int((~torch.isfinite(got)).sum()))
    err = (got - exp).abs()
    ok = err <= bound
    if not bool(ok.all()):
        at = tuple(int(i) for i in (~ok).nonzero()[0])
        raise AssertionError("%s: %d elements out of bound, first at %s: got %r exp %r bound %.3e" % (
            what, int((~ok).sum()), at, float(got[at]), float(exp[at]), float(bound[at])))
    keep = torch.ones(out.numel(), dtype=torch.bool)
    keep[idx.reshape(-1)] = False
    assert bool((out.view(torch.int32)[keep] == SENTINEL).all()), "%s: wrote outside its output block" % what
    RATIOS[form] = max(RATIOS.get(form, 0.0), float((err / bound).max()) if err.numel() else 0.0)


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for k, v in sorted(RATIOS.items()):
        print("attention worst |got-exp| / bound  %-22s %.4f" % (k, v))


def _call(case, kind):
    """One ops.mha_core call on the case's views -> (flat output buffer, the output's element indices, exp, bound)."""
    q, k, v = case.inputs(kind)
    lay = case.layout()
    bufs = attn_pack(lay, q, k, v, case.outer, case.inner)
    w, st = lay["where"], lay["strides"]
    exp, bound = attention64_views(bufs[w["q"][0]], bufs[w["k"][0]], bufs[w["v"][0]], case.outer, case.inner, case.heads, case.hd,
                                   case.Lq, case.Lk, st, (w["q"][1], w["k"][1], w["v"][1]))
    dev = {n: b.to(DEV) for n, b in bufs.items()}
    out = _sentinel_buffer(lay["out_size"])
    _ops().mha_core(dev[w["q"][0]][w["q"][1]:], dev[w["k"][0]][w["k"][1]:], dev[w["v"][0]][w["v"][1]:], out, case.outer,
                    case.inner, case.heads, case.hd, case.Lq, case.Lk, st)
    idx = attn_index(0, st[9], st[10], st[11], case.outer, case.inner, case.heads, case.hd, case.Lq)
    return out, idx, exp, bound


@pytest.mark.parametrize("case", ATTN_CASES, ids=[c.id for c in ATTN_CASES])
def test_form_against_statement(case):
    """Each input kind of the case through ops.mha_core: finite, within the bound, nothing written outside the output block."""
    for kind in case.kinds:
        out, idx, exp, bound = _call(case, kind)
        _check(out, idx, exp, bound, case.form, "%s %s" % (case.id, kind))


# ------------------------------------------------------------------------------------------ segments
def _segment_rows(encoder):
    """First (query row, key row) of every segment of ATTN_SEGMENTS with sentinel / NaN rows between them.  Encoder layout: q and
    k from the same rows of one [R, 3 E] matrix; decoder layout: q [Rq, E] against k, v of [Rk, 2 E]."""
    rows, rq, rk = [], 1, 2
    for Lq, Lk in ATTN_SEGMENTS:
        if encoder:
            rows.append((rq, rq))
            rq += max(Lq, Lk) + 2
        else:
            rows.append((rq, rk))
            rq, rk = rq + Lq + 1, rk + Lk + 3
    return rows, rq + 1, (rq if encoder else rk) + 1


@pytest.mark.parametrize("kind", ATTN_SEGMENT_KINDS)
@pytest.mark.parametrize("encoder", [True, False], ids=["encoder", "decoder"])
def test_segments_against_statement(encoder, kind):
    """ops.mha_core_segments, one call over shared q / k / v / o matrices: max_Lq and max_Lk of the largest segment (<128,32>),
    then max_Lk = 833 (<128,8> serves the same segments).  Every segment within the bound; the rows of an empty query range, of a
    segment with NO keys (the kernel returns before it writes: that is the rule) and the rows between segments keep the sentinel."""
    ops = _ops()
    heads, hd = 2, 128
    E = heads * hd
    rows, Rq, Rk = _segment_rows(encoder)
    ld_q, ld_kv, col_k, col_v = (3 * E, 3 * E, E, 2 * E) if encoder else (E, 2 * E, 0, E)
    ld_o = E + 4
    kv = torch.full((Rk * ld_kv,), float("nan"))
    qb = kv if encoder else torch.full((Rq * ld_q,), float("nan"))
    want, desc = [], []
    for s, ((Lq, Lk), (q0, k0)) in enumerate(zip(ATTN_SEGMENTS, rows)):
        desc.append([q0, Lq, k0, Lk])
        if Lq == 0 or Lk == 0:
            continue
        q, k, v = attn_segment_inputs(kind, s)
        qb[attn_index(q0 * ld_q, 0, 0, ld_q, 1, 1, heads, hd, Lq).reshape(-1)] = q.reshape(-1)
        kv[attn_index(k0 * ld_kv + col_k, 0, 0, ld_kv, 1, 1, heads, hd, Lk).reshape(-1)] = k.reshape(-1)
        kv[attn_index(k0 * ld_kv + col_v, 0, 0, ld_kv, 1, 1, heads, hd, Lk).reshape(-1)] = v.reshape(-1)
        want.append((attn_index(q0 * ld_o, 0, 0, ld_o, 1, 1, heads, hd, Lq),) + attention64(q, k, v, hd))
    idx, exp, bound = (torch.cat([w[i] for w in want], 2) for i in range(3))
    kv_d = kv.to(DEV)
    q_d = kv_d if encoder else qb.to(DEV)
    seg = torch.tensor(desc, dtype=torch.int32, device=DEV)
    max_Lq, max_Lk = max(s[0] for s in ATTN_SEGMENTS), max(s[1] for s in ATTN_SEGMENTS)
    for form, mk in (("segments tile128x32", max_Lk), ("segments tile128x8", 833)):
        out = _sentinel_buffer(Rq * ld_o)
        ops.mha_core_segments(q_d, kv_d[col_k:], kv_d[col_v:], out, seg, len(desc), heads, hd, ld_q, ld_kv, ld_kv, ld_o, max_Lq, mk)
        _check(out, idx, exp, bound, form, "%s %s %s" % (form, "encoder" if encoder else "decoder", kind))


# ------------------------------------------------------------------------------------------ claimed bit-identities
def _tiny_and_tile(kind, Lq, Lk, heads=8):
    """The same problem through ops.mha_core (Lk <= 64: mha_tiny128_kernel) and as a one-segment ops.mha_core_segments call
    (always the tile kernel)."""
    ops = _ops()
    hd = 128
    E = heads * hd
    q, k, v = (x.transpose(1, 2).reshape(-1, E).to(DEV) for x in attn_inputs(kind, 1, heads, hd, Lq, Lk, 31 * Lq + Lk))
    a, b = torch.zeros(Lq, E, device=DEV), torch.zeros(Lq, E, device=DEV)
    ops.mha_core(q, k, v, a, 1, 1, heads, hd, Lq, Lk, [0, 0, E, 0, 0, E, 0, 0, E, 0, 0, E])
    seg = torch.tensor([[0, Lq, 0, Lk]], dtype=torch.int32, device=DEV)
    ops.mha_core_segments(q, k, v, b, seg, 1, heads, hd, E, E, E, E, Lq, Lk)
    return a, b


@pytest.mark.parametrize("kind", ["randn", "overflow"])
@pytest.mark.parametrize("Lq,Lk", [(9, 9), (53, 53), (5, 64)])
def test_tiny128_equals_the_tile_kernel_bit_for_bit(Lq, Lk, kind):
    """tracker_tasks.h: mha_tiny128_task is "the same arithmetic, value for value, as mha_core_kernel"."""
    a, b = _tiny_and_tile(kind, Lq, Lk)
    assert bool(torch.isfinite(a).all())
    assert torch.equal(a, b), "%d of %d elements differ, max %.3e" % (int((a != b).sum()), a.numel(), float((a - b).abs().max()))


def test_wave_count_switch_equals_tiny128_bit_for_bit():
    """129 batches x 8 heads x 64 rows = 66048 waves > 65536 take mha_core_kernel<128,32>; the first 8 batches alone take
    mha_tiny128_kernel: the same bits."""
    ops = _ops()
    case = [c for c in ATTN_CASES if c.outer == 129][0]
    lay = case.layout()
    q, k, v = case.inputs("randn")
    bufs = {n: b.to(DEV) for n, b in attn_pack(lay, q, k, v, case.outer, case.inner).items()}
    st = lay["strides"]
    outs = []
    for nb in (case.outer, 8):
        out = _sentinel_buffer(lay["out_size"])
        ops.mha_core(bufs["q"], bufs["k"], bufs["v"], out, nb, 1, case.heads, case.hd, case.Lq, case.Lk, st)
        outs.append(out[:8 * st[9]].view(torch.int32))
    assert torch.equal(outs[0], outs[1]), "%d elements differ" % int((outs[0] != outs[1]).sum())


# ------------------------------------------------------------------------------------------ refusals
def test_refusals():
    """Shapes beyond one workgroup's LDS, a head_dim that has no kernel, a q stride that is no multiple of 4 and an empty key
    range raise GomError and launch nothing; an empty query range or an empty batch returns: the output keeps its bits."""
    ops = _ops()
    from gomatching_amd.lib import GomError

    def call(hd, Lq, Lk, outer=1, q_ss=None, heads=2):
        E = heads * hd
        q_ss = E if q_ss is None else q_ss
        q = torch.zeros(max(outer, 1) * 4 * max(Lq, 1) * q_ss, device=DEV)         # batch stride 4 Lq q_ss: a multiple of 4
        k = torch.zeros(max(outer, 1) * max(Lk, 1) * E, device=DEV)
        out = _sentinel_buffer(max(outer, 1) * max(Lq, 1) * E)
        refused = None
        try:
            ops.mha_core(q, k, k.clone(), out, outer, 1, heads, hd, Lq, Lk, [4 * Lq * q_ss, 0, q_ss, Lk * E, 0, E, Lk * E, 0, E, Lq * E, 0, E])
        except GomError as e:
            refused = e
        torch.cuda.synchronize()
        assert bool((out.view(torch.int32) == SENTINEL).all()), "a refused or empty call wrote to its output"
        if refused is not None:
            raise refused

    for hd, Lq, Lk, kw in ((32, 3, 4801, {}), (128, 3, 3905, {}), (64, 5, 5, {}), (32, 5, 5, {"q_ss": 258}), (128, 5, 5, {"q_ss": 258}),
                           (32, 4, 0, {}), (128, 4, 0, {})):
        with pytest.raises(GomError):
            call(hd, Lq, Lk, **kw)
    for hd in (32, 128):
        call(hd, 0, 5)
        call(hd, 5, 5, outer=0)
    out, idx, exp, bound = _call(ATTN_CASES[1], "randn")                   # and the next valid call is as usual
    _check(out, idx, exp, bound, ATTN_CASES[1].form, "after the refusals")
