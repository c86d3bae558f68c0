"""GPU: the lean forms of the proposal top-k (csrc/topk.hip: the k-bounded chunk sort and the merge network sized by the candidates)
against the forms before them (ops.TOPK_LEAN = False) and against the statement of tests/select_statement.py.

The winners are fixed by the 64-bit key order, so the two forms must agree bit for bit (torch.equal) on every input, ties and signed
zeros included; against the fp64 statement the indices are compared exactly, and on rows that mix +0.0 and -0.0 (which the statement
holds equal and the kernel orders by bit pattern) the gathered values.  Shapes: one short chunk, one full chunk, a chunk border, four
chunks, and 8 and 9 chunks at k = 128: 1024 candidates exactly (the smallest merge network, full) and 1152 (the next network)."""
import numpy as np
import pytest
import torch

from select_statement import CHUNK, TopkCase, topk64, topk_values

pytestmark = pytest.mark.gpu

DEV = "cuda"
B = 2
SHAPES = [(100, 100), (4096, 100), (4097, 100), (12289, 100), (8 * 4096, 128), (8 * 4096 + 1, 128)]
KINDS = ["randn", "all_equal", "signed_zeros", "tie_across_chunk", "frame_valid"]
CASES = [(S, k, kind) for (S, k) in SHAPES for kind in KINDS if not (kind == "tie_across_chunk" and S <= CHUNK)]


def _ops():
    from gomatching_amd import ops
    return ops


def _inputs(S, k, kind):
    """(logits [B, S] float32, valid [S] bool or None, frame_valid [B, S] bool or None, c0)."""
    case = TopkCase(B, S, k, "randn" if kind == "frame_valid" else kind)
    x = case.logits()
    if kind == "tie_across_chunk":                    # duplicated maxima on both sides of the first chunk border
        assert (x[:, CHUNK - 6:CHUNK + 1] == x.max()).all()
    if kind == "frame_valid":
        g = np.random.default_rng([S, k, 9])
        fv = g.random((B, S)) >= 0.3
        fv[1, :S // 2] = False                        # frame 1: the invalid constant floods the winners (ties by index)
        return x, None, fv, 0.37
    return x, case.valid(), None, case.c0


def _expected(x, valid, fv, c0, k):
    if fv is None:
        return topk64(x, valid, c0, k)
    S = x.shape[1]
    idx = np.concatenate([topk64(x[b:b + 1], fv[b], c0, k)[0] for b in range(B)])
    return idx, np.arange(B)[:, None] * S + idx


def _values(x, valid, fv, c0, idx):
    if fv is None:
        return topk_values(x, valid, c0, idx)
    return np.concatenate([topk_values(x[b:b + 1], fv[b], c0, idx[b:b + 1]) for b in range(B)])


def _launch(monkeypatch, lean, x, valid, fv, c0, k, ld, with_rows):
    ops = _ops()
    monkeypatch.setattr(ops, "TOPK_LEAN", lean)
    S = x.shape[1]
    buf = torch.full((B * S + 1, ld), float("nan"))
    buf[:B * S, 0] = torch.from_numpy(x.reshape(-1))
    buf = buf.to(DEV)
    masked = valid is not None or fv is not None
    out = ops.topk_tokens(buf, B, S, k,
                          valid=None if valid is None else torch.from_numpy(valid.astype(np.uint8)).to(DEV),
                          invalid_logit=torch.tensor([c0], dtype=torch.float32, device=DEV) if masked else None,
                          with_rows=with_rows,
                          frame_valid=None if fv is None else torch.from_numpy(fv.astype(np.uint8)).contiguous().to(DEV))
    return out if with_rows else (out, None)


@pytest.mark.parametrize("S, k, kind", CASES, ids=["S%d-k%d-%s" % c for c in CASES])
def test_lean_forms_equal_the_full_sort_and_the_statement(monkeypatch, S, k, kind):
    x, valid, fv, c0 = _inputs(S, k, kind)
    exp_idx, exp_rows = _expected(x, valid, fv, c0, k)
    for ld, with_rows in ((1, True), (3, False), (3, True)):
        idx0, rows0 = _launch(monkeypatch, False, x, valid, fv, c0, k, ld, with_rows)
        idx1, rows1 = _launch(monkeypatch, True, x, valid, fv, c0, k, ld, with_rows)
        assert torch.equal(idx1, idx0), (ld, with_rows)
        assert (rows1 is None) == (not with_rows)
        if with_rows:
            assert torch.equal(rows1, rows0)
            assert np.array_equal(rows1.cpu().numpy(), np.arange(B)[:, None] * S + idx1.cpu().numpy())
        got = idx1.cpu().numpy().astype(np.int64)
        if kind == "signed_zeros":
            assert np.array_equal(_values(x, valid, fv, c0, got), _values(x, valid, fv, c0, exp_idx))
            assert all(len(set(r)) == k for r in got.tolist())
        else:
            assert np.array_equal(got, exp_idx), (ld, with_rows, np.flatnonzero((got != exp_idx).any(0))[:8])
            if with_rows:
                assert np.array_equal(rows1.cpu().numpy(), exp_rows)


def test_signed_zeros_rank_by_bit_pattern(monkeypatch):
    """+0.0 ranks above -0.0, ties to the lower index: the winners of a row of alternating zeros are the even tokens, in both forms."""
    S, k = 4097, 100
    x = np.zeros((B, S), np.float32)
    x[:, 1::2] = np.float32(-0.0)
    want = np.tile(np.arange(0, 2 * k, 2), (B, 1))
    for lean in (False, True):
        idx, _ = _launch(monkeypatch, lean, x, None, None, 0.0, k, 1, False)
        assert np.array_equal(idx.cpu().numpy(), want), lean
