"""GPU: ops.layernorm, ops.layernorm_any and ops.groupnorm32_into against the float64 statements of tests/norm_statement.py, at the
row counts and sizes where the kernels change path: rows that do not fill a workgroup (four rows each; eight on the 32-lane form of
layernorm_any), in-place output, constant rows (beta exactly), rows whose mean dwarfs their spread, GroupNorm across one, exactly one,
one-past-one and several 256-row statistics blocks, written at a token offset of a wider buffer whose other rows stay untouched.

tests/test_norm_statement_cpu.py shows that a one-pass variance and first-block-only statistics would leave these bounds."""
import numpy as np
import pytest
import torch

from norm_statement import (GN_B, GN_HW, GN_KINDS, LN_ANY_D, LN_ANY_ROWS, LN_D, LN_KINDS, LN_ROWS, gn_inputs, groupnorm64, layernorm64,
                            ln_inputs, ln_reference_error, moderate_bound)

pytestmark = pytest.mark.gpu
DEV = "cuda"
OFFSET = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for k, v in sorted(OFFSET.items()):
        print("layernorm offset rows, worst ratio to 2 x reference error + ulp  %-24s gpu %.3e, F.layer_norm fp32 on the CPU %.3e" % (k, v[1], v[2]))


def _d(a):
    return None if a is None else torch.from_numpy(np.array(a)).to(DEV)


def _check_ln(op, kind, got, x, r, ga, be, what):
    ref = layernorm64(x, ga, be, r)
    got = got.astype(np.float64)
    assert got.shape == ref.shape
    err = np.abs(got - ref)
    if kind == "moderate":
        ratio = float((err / moderate_bound(ref)).max())
        assert ratio <= 1.0, "%s: |gpu - fp64| = %.3f x (2e-5 + 1e-5 |ref|)" % (what, ratio)
    elif kind == "const":
        assert np.array_equal(got, np.broadcast_to(be.astype(np.float64), got.shape)), "%s: a constant row must give beta exactly" % what
    else:
        cpu_err, ulp = ln_reference_error(x, r, ga, be)
        gpu_err = float(err.max())
        print("%s: max|gpu - fp64| = %.3e, max|F.layer_norm fp32 on the CPU - fp64| = %.3e" % (what, gpu_err, cpu_err))
        key = "%s %s" % (op, kind)
        ratio = gpu_err / (2 * cpu_err + ulp)
        if ratio > OFFSET.get(key, (0.0,))[0]:
            OFFSET[key] = (ratio, gpu_err, cpu_err)
        assert gpu_err <= 2 * cpu_err + ulp, "%s: gpu %.3e, reference %.3e" % (what, gpu_err, cpu_err)


@pytest.mark.parametrize("residual", [False, True])
@pytest.mark.parametrize("rows", LN_ROWS)
@pytest.mark.parametrize("D", LN_D)
def test_layernorm(D, rows, residual):
    from gomatching_amd import ops
    for kind in LN_KINDS:
        x, r, ga, be = ln_inputs(kind, rows, D, residual)
        for inplace in (False, True):
            xd = _d(x)
            # a separate buffer with a sentinel row behind it: the kernel writes rows x D floats and nothing else
            buf = torch.full((rows + 1, D), -7.0, device=DEV)
            out = ops.layernorm(xd, _d(ga), _d(be), residual=_d(r), out=xd if inplace else buf[:rows])
            torch.cuda.synchronize()
            assert out.data_ptr() == (xd if inplace else buf).data_ptr()
            if not inplace:
                assert bool((buf[rows] == -7.0).all()) and torch.equal(xd.cpu(), torch.from_numpy(x))
            _check_ln("layernorm", kind, out.cpu().numpy(), x, r, ga, be,
                      "layernorm %s D %d rows %d residual %d inplace %d" % (kind, D, rows, residual, inplace))


@pytest.mark.parametrize("rows", LN_ANY_ROWS)
@pytest.mark.parametrize("D", LN_ANY_D)
def test_layernorm_any(D, rows):
    from gomatching_amd import ops
    for kind in LN_KINDS:
        x, _, ga, be = ln_inputs(kind, rows, D, False)
        out = ops.layernorm_any(_d(x), _d(ga), _d(be))
        torch.cuda.synchronize()
        _check_ln("layernorm_any", kind, out.cpu().numpy(), x, None, ga, be, "layernorm_any %s D %d rows %d" % (kind, D, rows))


@pytest.mark.parametrize("B", GN_B)
@pytest.mark.parametrize("HW", GN_HW)
def test_groupnorm32_into(HW, B):
    from gomatching_amd import ops
    kinds = GN_KINDS if (HW, B) == (600, 3) else GN_KINDS[:1]            # 50 + randn: one case, the largest
    for kind in kinds:
        x, ga, be = gn_inputs(kind, B, HW)
        ref = groupnorm64(x, ga, be)
        off, S = 5, HW + 11
        buf = torch.zeros(B, S, 256, device=DEV)
        ops.groupnorm32_into(_d(x), _d(ga), _d(be), buf[0, off:], S * 256)
        torch.cuda.synchronize()
        got = buf.cpu().numpy()
        assert not got[:, :off].any() and not got[:, off + HW:].any(), "rows outside the written range must stay zero"
        ratio = float((np.abs(got[:, off:off + HW].astype(np.float64) - ref) / moderate_bound(ref)).max())
        print("groupnorm %s B %d HW %d: worst |gpu - fp64| / (2e-5 + 1e-5 |ref|) = %.4f" % (kind, B, HW, ratio))
        assert ratio <= 1.0, (kind, B, HW, ratio)
