"""CPU: tests/norm_statement.py is the yardstick of test_norm_forms_gpu.py.  On the GPU file's own inputs this file shows

  * layernorm64 and groupnorm64 equal torch in float64;
  * the bounds are not vacuous: a numpy float32 evaluation in the kernels' own order (csrc/norm.hip: a lane's quads summed in sequence,
    the xor butterfly, the centred second pass; fp64 sums and the fp32 application for GroupNorm) stays inside them on every case, and
    gives beta exactly on the constant rows;
  * the cases bite: a one-pass E[x^2] - mean^2 variance in fp32 leaves the offset rows' bound, and GroupNorm statistics taken over the
    first 256 rows only leave the moderate bound as soon as HW > 256."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from norm_statement import (EPS, GN_B, GN_HW, GN_KINDS, LN_ANY_D, LN_ANY_ROWS, LN_D, LN_KINDS, LN_ROWS, gn_inputs, groupnorm64,
                            layernorm64, ln_inputs, ln_reference_error, moderate_bound)

f32 = np.float32


@pytest.mark.parametrize("D", LN_D + (96,))
@pytest.mark.parametrize("residual", [False, True])
def test_layernorm64_equals_torch_float64(D, residual):
    for kind in LN_KINDS:
        x, r, ga, be = ln_inputs(kind, 5, D, residual)
        v = torch.from_numpy(x).double() + (0 if r is None else torch.from_numpy(r).double())
        ref = F.layer_norm(v, (D,), torch.from_numpy(ga).double(), torch.from_numpy(be).double(), EPS).numpy()
        got = layernorm64(x, ga, be, r)
        assert np.abs(got - ref).max() <= 1e-9 * max(1.0, np.abs(ref).max()), kind      # (offset001: 1 / sqrt(var + eps) amplifies the last bits)


@pytest.mark.parametrize("HW", GN_HW)
def test_groupnorm64_equals_torch_float64(HW):
    for kind in GN_KINDS:
        x, ga, be = gn_inputs(kind, 3, HW)
        ref = F.group_norm(torch.from_numpy(x).double().permute(0, 2, 1), 32, torch.from_numpy(ga).double(), torch.from_numpy(be).double(), EPS)
        assert np.abs(groupnorm64(x, ga, be) - ref.permute(0, 2, 1).numpy()).max() <= 1e-10, kind


# ------------------------------------------------------------------------------------------ the kernels' order in numpy float32
def _butterfly(v):
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[:, lane ^ o]
    return v[:, :1]


def ln_emul32(x, r, gamma, beta, mistake=None):
    """layernorm_kernel<VEC>: lane l owns the quads (i * 64 + l) * 4, i < VEC; one fp32 rounding per operation."""
    rows, D = x.shape
    v = x if r is None else x + r
    q4 = v.reshape(rows, D // 256, 64, 4)
    s = np.zeros((rows, 64), f32)
    for i in range(D // 256):
        s = s + ((q4[:, i, :, 0] + q4[:, i, :, 1]) + (q4[:, i, :, 2] + q4[:, i, :, 3]))
    mean = _butterfly(s) * f32(1.0 / D)
    d4 = q4 if mistake == "one_pass" else (q4 - mean[:, :, None, None])
    q = np.zeros((rows, 64), f32)
    for i in range(D // 256):
        e = d4[:, i] * d4[:, i]
        q = q + ((e[..., 0] + e[..., 1]) + (e[..., 2] + e[..., 3]))
    var = _butterfly(q) * f32(1.0 / D)
    if mistake == "one_pass":
        var = np.maximum(var - mean * mean, f32(0))
    rstd = (1.0 / np.sqrt((var + f32(EPS)).astype(np.float64))).astype(f32)
    return (v - mean) * rstd * gamma + beta


LN_CASES = [(D, rows, residual) for D in LN_D for rows in LN_ROWS for residual in (False, True)]


@pytest.mark.parametrize("D,rows,residual", LN_CASES)
def test_two_pass_fp32_stays_inside_the_bounds(D, rows, residual):
    for kind in LN_KINDS:
        x, r, ga, be = ln_inputs(kind, rows, D, residual)
        got = ln_emul32(x, r, ga, be).astype(np.float64)
        ref = layernorm64(x, ga, be, r)
        err = np.abs(got - ref)
        if kind == "moderate":
            assert (err <= moderate_bound(ref)).all(), (kind, float((err / moderate_bound(ref)).max()))
        elif kind == "const":
            assert np.array_equal(got, np.broadcast_to(be.astype(np.float64), got.shape))
            assert np.abs(ref - be).max() <= 1e-12
        else:
            cpu_err, ulp = ln_reference_error(x, r, ga, be)
            print("layernorm %-9s D %4d rows %3d residual %d: two-pass fp32 %.3e, F.layer_norm fp32 %.3e" % (
                kind, D, rows, residual, err.max(), cpu_err))
            assert err.max() <= 2 * cpu_err + ulp, (kind, float(err.max()), cpu_err)


# named cases: offset1 and offset001 at D = 256, 130 rows (every D and row count shows it; the moderate kind never does: E[x^2] = 10
# against var = 9 loses a few ulp only)
@pytest.mark.parametrize("kind", ["offset1", "offset001"])
def test_one_pass_variance_leaves_the_offset_bound(kind):
    x, r, ga, be = ln_inputs(kind, 130, 256, False)
    ref = layernorm64(x, ga, be, r)
    cpu_err, ulp = ln_reference_error(x, r, ga, be)
    err = np.abs(ln_emul32(x, r, ga, be, "one_pass").astype(np.float64) - ref).max()
    print("layernorm one-pass %s: %.3e against 2 x %.3e + %.1e" % (kind, err, cpu_err, ulp))
    assert err > 2 * cpu_err + ulp
    x, r, ga, be = ln_inputs("moderate", 130, 256, False)
    ref = layernorm64(x, ga, be, r)
    assert (np.abs(ln_emul32(x, r, ga, be, "one_pass") - ref) <= moderate_bound(ref)).all()      # which is why the offset kinds exist


def ln_any_emul32(x, gamma, beta, shifted=True):
    """layernorm_any_kernel<LANES> (csrc/swin.hip): LANES = 32 for D <= 128, else 64; lane l owns the quads (l + LANES i) * 4 < D; the
    row is held relative to its first element (`shifted`; False: the raw row, as the kernel summed it before)."""
    rows, D = x.shape
    lanes = 32 if D <= 128 else 64
    nv = -(-D // (4 * lanes))
    v = np.zeros((rows, nv * lanes * 4), f32)
    v[:, :D] = x - x[:, :1] if shifted else x
    q4 = v.reshape(rows, nv, lanes, 4)

    def group_sum(t):
        lane, o = np.arange(lanes), lanes // 2
        while o:
            t, o = t + t[:, lane ^ o], o // 2
        return t[:, :1]

    s = np.zeros((rows, lanes), f32)
    for i in range(nv):
        s = s + (((q4[:, i, :, 0] + q4[:, i, :, 1]) + q4[:, i, :, 2]) + q4[:, i, :, 3])
    mean = group_sum(s) / f32(D)
    d = np.where(np.arange(nv * lanes * 4) < D, v - mean, f32(0)).reshape(rows, nv, lanes, 4)
    q = np.zeros((rows, lanes), f32)
    for i in range(nv):
        e = d[:, i] * d[:, i]
        q = q + (((e[..., 0] + e[..., 1]) + e[..., 2]) + e[..., 3])
    rstd = (1.0 / np.sqrt((group_sum(q) / f32(D) + f32(EPS)).astype(np.float64))).astype(f32)
    return (v[:, :D] - mean) * rstd * gamma + beta


def test_layernorm_any_holds_the_row_relative_to_its_first_element():
    """D = 96, 3 rows of 1000 + randn: the fp32 sum of the raw row (96 000, ulp 2^-7) loses the mean, and the result leaves twice the
    CPU reference's error -- the case with which tests/test_norm_forms_gpu.py found it.  The shifted row stays far inside on every
    case of the GPU file, and a constant row gives beta exactly."""
    x, _, ga, be = ln_inputs("offset1", 3, 96, False)
    ref = layernorm64(x, ga, be)
    cpu_err, ulp = ln_reference_error(x, None, ga, be)
    raw = np.abs(ln_any_emul32(x, ga, be, shifted=False).astype(np.float64) - ref).max()
    print("layernorm_any offset1 D 96 rows 3: raw sum %.3e against 2 x %.3e" % (raw, cpu_err))
    assert raw > 2 * cpu_err + ulp
    for D in LN_ANY_D:
        for rows in LN_ANY_ROWS:
            for kind in LN_KINDS:
                x, _, ga, be = ln_inputs(kind, rows, D, False)
                got = ln_any_emul32(x, ga, be).astype(np.float64)
                ref = layernorm64(x, ga, be)
                if kind == "const":
                    assert np.array_equal(got, np.broadcast_to(be.astype(np.float64), got.shape))
                elif kind == "moderate":
                    assert (np.abs(got - ref) <= moderate_bound(ref)).all()
                else:
                    cpu_err, ulp = ln_reference_error(x, None, ga, be)
                    assert np.abs(got - ref).max() <= 0.25 * (2 * cpu_err + ulp), (kind, D, rows)


def gn_emul(x, gamma, beta, mistake=None):
    """gn_stats_kernel + gn_apply_kernel: fp64 sum and sum of squares per (image, group), then fp32 (v - mu) * rstd * gamma + beta."""
    B, HW, C = x.shape
    rows = x[:, :256] if mistake == "first_256_rows" else x
    vg = rows.astype(np.float64).reshape(B, rows.shape[1], 32, 8)
    n = HW * 8.0
    mean = vg.sum((1, 3)) / n
    var = np.maximum((vg * vg).sum((1, 3)) / n - mean * mean, 0.0)
    mu = np.repeat(mean.astype(f32), 8, 1)[:, None]
    rstd = np.repeat((1.0 / np.sqrt(var + np.float64(f32(EPS)))).astype(f32), 8, 1)[:, None]
    return (x - mu) * rstd * gamma + beta


@pytest.mark.parametrize("HW", GN_HW)
@pytest.mark.parametrize("B", GN_B)
def test_groupnorm_fp64_stats_stay_inside_the_bound(B, HW):
    for kind in GN_KINDS:
        x, ga, be = gn_inputs(kind, B, HW)
        ref = groupnorm64(x, ga, be)
        ratio = (np.abs(gn_emul(x, ga, be).astype(np.float64) - ref) / moderate_bound(ref)).max()
        assert ratio <= 1.0, (kind, ratio)


# named cases: HW = 257 (one row past the first block) and HW = 600 (two blocks and a tail of 88), B = 3, moderate data; HW <= 256
# cannot show it
def test_groupnorm_stats_over_the_first_block_only_leave_the_bound():
    for HW in GN_HW:
        x, ga, be = gn_inputs("moderate", 3, HW)
        ref = groupnorm64(x, ga, be)
        ratio = (np.abs(gn_emul(x, ga, be, "first_256_rows").astype(np.float64) - ref) / moderate_bound(ref)).max()
        print("groupnorm first_256_rows HW %3d: worst |d| / bound = %.3g" % (HW, ratio))
        assert (ratio > 1.0) == (HW > 256), HW
