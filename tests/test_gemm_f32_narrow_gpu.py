"""GPU: the exact-fp32 GEMM's 128-row tile for N <= 32 (csrc/gemm_conv.hip, dispatch_tile) against the 256-row tile
(ops.GEMM_NARROW_TILE = False) and against the fp64 statement of tests/conv_statement.py (a GEMM is its 1 x 1 convolution).

A row's k order does not depend on the tile height, so the two tiles must agree bit for bit (torch.equal) -- with and without bias,
ReLU, a residual and a row gather, at row counts around the 64-row wave patch, the 128- and 256-row tiles, and one of several tiles."""
import numpy as np
import pytest
import torch

from conv_statement import conv64, conv_bound

pytestmark = pytest.mark.gpu

DEV = "cuda"
K = 256
MS = [1, 63, 64, 65, 257, 800]
NS = [1, 4, 8, 32]
# (bias, relu, residual, a_rows)
EPILOGUES = {"plain": (False, False, False, False), "bias": (True, False, False, False), "bias_relu": (True, True, False, False),
             "residual": (False, False, True, False), "rows": (False, False, False, True), "all": (True, True, True, True)}


def _ops():
    from gomatching_amd import ops
    return ops


@pytest.fixture(scope="module")
def operands():
    g = torch.Generator().manual_seed(7)
    return {"A": torch.randn((1024, K), generator=g), "W": torch.randn((32, K), generator=g) * 0.1,
            "bias": torch.randn((32,), generator=g), "R": torch.randn((800, 32), generator=g),
            "perm": torch.randperm(1024, generator=g).to(torch.int32)}


@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("M", MS)
def test_narrow_tile_equals_the_256_row_tile_and_the_statement(monkeypatch, operands, M, N):
    ops = _ops()
    o = operands
    A, W = o["A"].to(DEV), o["W"][:N].contiguous().to(DEV)
    for name, (with_bias, relu, with_r, with_rows) in EPILOGUES.items():
        rows = o["perm"][:M].contiguous() if with_rows else None
        a_host = o["A"][rows.long()] if with_rows else o["A"][:M]
        bias = o["bias"][:N].contiguous() if with_bias else None
        R = o["R"][:M, :N].contiguous() if with_r else None
        kw = dict(bias=None if bias is None else bias.to(DEV), R=None if R is None else R.to(DEV), relu=relu)
        outs = []
        for narrow in (False, True):
            monkeypatch.setattr(ops, "GEMM_NARROW_TILE", narrow)
            out = torch.full((M + 1, N), float("nan"), device=DEV)
            if with_rows:
                ops.gemm(A, W, rows=rows.to(DEV), out=out, M=M, **kw)
            else:
                ops.gemm(A[:M], W, out=out, M=M, **kw)
            outs.append(out)
        assert torch.equal(outs[1][:M], outs[0][:M]), name
        assert bool(torch.isnan(outs[1][M]).all()), name                   # the row behind M stays unwritten
        x, w = a_host.numpy().reshape(1, M, 1, K), o["W"][:N].numpy().reshape(N, 1, 1, K)
        r = None if R is None else R.numpy().reshape(1, M, 1, N)
        b = None if bias is None else bias.numpy()
        exp = conv64(x, w, 1, 0, shift=b, R=r, relu=relu).reshape(M, N)
        bound = conv_bound(x, w, 1, 0, shift=b, R=r).reshape(M, N)
        err = np.abs(outs[1][:M].cpu().numpy().astype(np.float64) - exp)
        assert (err <= bound).all(), (name, float((err / bound).max()))
