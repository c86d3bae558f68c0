"""CPU: the fp64 MSDA statement of tests/helpers.py (msda64, msda_locations32, msda_softmax64) is the yardstick of
test_msda_forms_gpu.py.  Here it is checked against the reference's own outputs (tests/golden/msda.npz: the reference's
`ms_deform_attn_core_pytorch` in fp32, oracle/gen_golden.py; tests/golden/msda_any.npz, oracle/gen_golden_msda_any.py) to
within those fixtures' own fp32 rounding, and its location / softmax / out-of-window rules are pinned on small cases."""
import numpy as np
import pytest
import torch

from helpers import golden, msda64, msda64_fused, msda_locations32, msda_softmax64, t

U = 2.0 ** -24
# fp32 roundings in one output of the fixtures: the bilinear blend of a sample (4 products, 3 sums, ~2 for the pixel
# coordinate through grid_sample's unnormalisation) and the sum over the levels' points -- at most 16 samples per head here
KAPPA_FIXTURE = 32


def _args(g, case):
    return [t(g[case + "_" + k]) for k in ("value", "shapes", "lsi", "loc", "w")]


@pytest.mark.parametrize("name,case", [("msda.npz", "enc"), ("msda.npz", "dec"), ("msda.npz", "oob"),
                                       ("msda_any.npz", "odd_f32"), ("msda_any.npz", "one_f32"), ("msda_any.npz", "ship_f32")])
def test_statement_reproduces_reference_outputs(name, case):
    """Element-wise: |statement - fixture| <= KAPPA_FIXTURE * 2^-24 * sum|w * v| (the same statement on |value|, |w|)."""
    g = golden(name)
    value, shapes, lsi, loc, w = _args(g, case)
    exp = t(g[case + "_out"]).double()
    got = msda64(value, shapes, lsi, loc, w)
    mag = msda64(value.abs(), shapes, lsi, loc, w.abs())
    err = (got - exp).abs()
    assert bool((err <= KAPPA_FIXTURE * U * mag).all()), (case, float(err.max()), float((err / (U * mag)).nan_to_num(0).max()))
    # and it is not vacuous: the fixtures do sample their maps
    assert float(exp.abs().max()) > 0.5


def test_statement_against_oracle_in_fp64():
    """oracle.gom_oracle.ms_deform_attn_forward called with fp32 locations and fp64 value / weights computes the same pixel
    coordinates; its corner weights are fp32 products there, so the two agree to fp32 rounding of those weights."""
    from oracle import gom_oracle as O
    g = golden("msda.npz")
    for case in ("enc", "dec", "oob"):
        value, shapes, lsi, loc, w = _args(g, case)
        a = msda64(value, shapes, lsi, loc, w)
        b = O.ms_deform_attn_forward(value.double(), shapes, lsi, loc, w.double())
        mag = msda64(value.abs(), shapes, lsi, loc, w.abs())
        assert bool(((a - b).abs() <= 4 * U * mag).all()), case


def test_statement_window_and_corners():
    """Hand-made samples on a 2 x 3 map (one head, one channel, one level, one point): pixel coordinates on the acceptance
    window's edges, exactly on a pixel, on the last row / column (one corner), outside, and NaN / inf (skipped)."""
    H, W = 2, 3
    vals = torch.arange(1.0, 7.0, dtype=torch.float64).view(1, H * W, 1, 1)          # v[y, x] = 1 + y * W + x
    shapes = torch.tensor([[H, W]])
    lsi = torch.tensor([0])

    def px(y, x):                                                                    # location of pixel coordinate (y, x)
        return [(x + 0.5) / W, (y + 0.5) / H]

    def v(y, x):
        return 1.0 + y * W + x if 0 <= y < H and 0 <= x < W else 0.0

    cases = [
        (px(0, 0), v(0, 0)), (px(1, 2), v(1, 2)),                                     # on a pixel
        (px(0.5, 1.5), 0.25 * (v(0, 1) + v(0, 2) + v(1, 1) + v(1, 2))),                 # centre of four
        (px(-0.5, 0), 0.5 * v(0, 0)), (px(0, -0.5), 0.5 * v(0, 0)),                    # half way to the padding
        (px(1.5, 2.5), 0.25 * v(1, 2)),                                                # past the last row and column: one corner
        ([(-1 + 0.5) / W, 0.25], 0.0), ([0.25, (H + 0.5) / H], 0.0),                    # w_im = -1, h_im = H: outside
        ([0.5, 7.0], 0.0), ([float("nan"), 0.5], 0.0), ([0.5, float("inf")], 0.0), ([-float("inf"), 0.5], 0.0),
    ]
    loc = torch.tensor([c[0] for c in cases], dtype=torch.float32).view(1, len(cases), 1, 1, 1, 2)
    w = torch.ones((1, len(cases), 1, 1, 1), dtype=torch.float64)
    out = msda64(vals, shapes, lsi, loc, w).view(-1)
    exp = torch.tensor([c[1] for c in cases], dtype=torch.float64)
    assert torch.allclose(out, exp, rtol=0, atol=1e-6), (out, exp)
    assert bool(torch.isfinite(out).all())


def test_fused_statement_locations_and_softmax():
    """msda_locations32 is IEEE fp32 (torch's CPU division and multiply are, too) and msda_softmax64 the float64 softmax;
    msda64_fused is msda64 on them."""
    rng = np.random.default_rng(3)
    shapes = [(7, 9), (4, 5), (2, 3), (1, 1)]
    Q = 6
    raw = rng.standard_normal((Q, 448)).astype(np.float32) * 3
    raw[:, 384:] = np.nan
    raw[0, 256:272] = 1e4 + rng.standard_normal(16).astype(np.float32)              # a missing max subtraction overflows
    ref = rng.random((Q, 2)).astype(np.float32)
    vr = np.array([[0.75, 0.5], [5 / 6, 2 / 3], [1.0, 0.5], [0.5, 1.0]], np.float32)
    off = torch.from_numpy(raw[:, :256]).view(Q, 8, 4, 4, 2)
    norm = torch.tensor([[w_, h] for h, w_ in shapes], dtype=torch.float32)
    for v in (None, vr):
        r = torch.from_numpy(ref)[:, None, None, None, :]
        if v is not None:
            r = r * torch.from_numpy(v)[None, None, :, None, :]
        want = (r + off / norm[None, None, :, None, :]).numpy()
        got = msda_locations32(raw, ref, shapes, v)
        assert got.dtype == np.float32 and np.array_equal(got, want)
    w, d = msda_softmax64(raw)
    assert np.isfinite(w).all() and np.allclose(w.reshape(Q, 8, 16).sum(-1), 1.0, rtol=0, atol=1e-15)
    assert (d <= 0).all() and np.allclose(w.reshape(Q, 8, 16), torch.softmax(torch.from_numpy(raw[:, 256:384]).double()
                                                                              .view(Q, 8, 16), -1).numpy(), rtol=1e-14, atol=0)
    ss = torch.tensor(shapes)
    lsi = torch.cat((ss.new_zeros(1), ss.prod(1).cumsum(0)[:-1]))
    S = int(ss.prod(1).sum())
    value = torch.from_numpy(rng.standard_normal((1, S, 8, 32)))
    fused = msda64_fused(value, ss, lsi, raw, ref, 1, Q, vr)
    direct = msda64(value, ss, lsi, torch.from_numpy(msda_locations32(raw, ref, shapes, vr)).view(1, Q, 8, 4, 4, 2),
                    torch.from_numpy(w).view(1, Q, 8, 4, 4)).view(Q, 256)
    assert torch.equal(fused, direct) and bool(torch.isfinite(fused).all())
