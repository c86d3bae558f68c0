"""GPU: the lean form of the decoder's row marking (csrc/dec_value_rows.hip: a flag is read before it is stored, a corner row's two
x-neighbours go as one 16-bit access) against the form before it (ops.DEC_VALUE_MARK_LEAN = False) and against the restatement of
tests/test_dec_value_rows_gpu.py: the same bytes, whatever the flags held before, and the same row list behind them."""
import numpy as np
import pytest
import torch

from test_dec_value_rows_gpu import _corner_rows, _geometry, _pixels

pytestmark = pytest.mark.gpu

DEV = "cuda"
LEVELS = ((13, 21), (7, 11), (4, 6), (2, 3))
B, LQ = 2, 75
SCALES = (1.0, 2.5, 40.0)                              # x 40: most samples outside their map


def _ops():
    from gomatching_amd import ops
    return ops


def _inputs(scale, seed):
    g = np.random.default_rng([seed, int(scale * 10)])
    Q = B * LQ
    raw = g.standard_normal((Q, 384)).astype(np.float32)
    raw[:, :256] *= np.float32(scale)
    ref = g.random((Q, 2)).astype(np.float32)
    ref[0::7, 0], ref[1::7, 1], ref[2::7, 0], ref[3::7, 1] = 0.0, 0.0, 1.0, 1.0      # reference points on the borders
    ref[4::14] = (1.0, 0.0)
    return raw, ref


def _want(raw, ref, lsi, S):
    """The restated flags [B * S] with the kernel's `row < S` guard (S may be smaller than the pyramid)."""
    rows, _ = _corner_rows(_pixels(raw, ref, LEVELS)[1], LEVELS, lsi)
    frame = np.broadcast_to((np.arange(raw.shape[0]) // LQ).reshape(-1, 1, 1, 1, 1), rows.shape)
    keep = rows < S
    flags = np.zeros((B * S,), np.uint8)
    flags[(frame * S + rows)[keep]] = 1
    return flags


def _mark(monkeypatch, lean, raw, ref, shapes, lsi, S, preset):
    ops = _ops()
    monkeypatch.setattr(ops, "DEC_VALUE_MARK_LEAN", lean)
    st = ops.DecValueRows(B * S, DEV)
    if preset is not None:
        st.flags[:B * S] = torch.from_numpy(preset).to(DEV)
    ops.dec_value_mark(raw, ref, shapes, lsi, B, LQ, S, st)
    return st


@pytest.mark.parametrize("short", [0, 5], ids=["whole_pyramid", "five_rows_short"])
@pytest.mark.parametrize("scale", SCALES)
def test_lean_marks_equal_the_plain_marks_and_the_restatement(monkeypatch, scale, short):
    ops = _ops()
    lsi_np, S_full = _geometry(LEVELS)
    S = S_full - short                                 # five rows short: the last level keeps one row, its neighbour is beyond S
    raw_np, ref_np = _inputs(scale, 3)
    want = _want(raw_np, ref_np, lsi_np, S)
    assert want.any() and (scale < 40 or not want.all())    # (x 2.5 marks every row of this small pyramid; x 40 leaves most unmarked)
    raw, ref = torch.from_numpy(raw_np).to(DEV), torch.from_numpy(ref_np).to(DEV)
    shapes = torch.tensor(LEVELS, dtype=torch.int64, device=DEV)
    lsi = torch.from_numpy(lsi_np).to(DEV)
    g = torch.Generator().manual_seed(int(scale * 10) + short)
    memory = torch.randn((B * S, 256), generator=g).to(DEV)
    with ops.gemm_mode("f16x3"):
        lin = ops.K256Linear(ops.prep_weight((torch.randn((256, 256), generator=g) * 0.06).to(DEV)), torch.randn((256,), generator=g).to(DEV))
    preset = (np.random.default_rng(short + 1).random(B * S) < 0.1).astype(np.uint8)
    for pre in (None, preset):
        exp = want if pre is None else want | pre
        st0 = _mark(monkeypatch, False, raw, ref, shapes, lsi, S, pre)
        st1 = _mark(monkeypatch, True, raw, ref, shapes, lsi, S, pre)
        assert torch.equal(st1.flags, st0.flags)
        got = st1.flags.cpu().numpy()
        assert np.array_equal(got[:B * S], exp), np.flatnonzero(got[:B * S] != exp)[:8]
        assert not got[B * S:].any()
        # the launches behind the marks: the same list and count, the listed rows projected, the flags zero again
        for st in (st0, st1):
            st.value.fill_(float("nan"))
            ops.dec_value_compact(st)
            ops.linear_rows(memory, lin, st)
        n0, n1 = int(st0.count.item()), int(st1.count.item())
        assert n0 == n1 == int(exp.sum())
        assert torch.equal(st1.rows[:n1], st0.rows[:n0])
        assert np.array_equal(st1.rows[:n1].cpu().numpy(), np.flatnonzero(exp))
        assert not bool(st0.flags.any()) and not bool(st1.flags.any())
        assert torch.equal(torch.isnan(st1.value), torch.isnan(st0.value))
        listed = torch.from_numpy(exp.astype(bool)).to(DEV)
        assert torch.equal(st1.value[listed], st0.value[listed]) and not bool(torch.isnan(st1.value[listed]).any())
