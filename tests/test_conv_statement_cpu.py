"""CPU: tests/conv_statement.py is the yardstick of test_conv_forms_gpu.py.  On every case of the GPU file (same generators, same
seeds: the same bits) this file shows

  * conv64 equals torch.nn.functional.conv2d in float64;
  * ops.conv_plan (host-only entry points of the built library) chooses the form each case declares, per back-end: the split-K cases
    are split, the ragged ones leave a shorter last slice, the patch cases reach the patch kernel;
  * the cases bite: a numpy evaluation in the tile kernel's own structure -- rows m decoded to (b, oh, ow), k to (kh, kw, c), 128-row
    M tiles, 32-wide k-tiles dealt to split-K slices, the epilogue -- agrees with conv64 as written, and with each planted mistake in it
    leaves conv_bound on a named case;
  * on the exact-integer inputs conv64 equals a float32 evaluation bit for bit, so the GPU file may ask every form for identical bits."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conv_statement import BK, BM, CASES, IDS, KINDS, PATCH_CASES, SPLITK_CASES, case, conv32, worst


def _cdiv(a, b):
    return -(-a // b)


# ------------------------------------------------------------------------------------------ the statement
@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_conv64_equals_torch_float64(c):
    i = c.inputs()
    t = lambda a: torch.from_numpy(np.asarray(a, np.float64))
    ref = F.conv2d(t(i["x"]).permute(0, 3, 1, 2), t(i["w"]).permute(0, 3, 1, 2), None, stride=c.stride, padding=c.pad)
    if i["scale"] is not None:
        ref = ref * t(i["scale"]).view(1, -1, 1, 1)
    if i["shift"] is not None:
        ref = ref + t(i["shift"]).view(1, -1, 1, 1)
    ref = ref.permute(0, 2, 3, 1)
    if i["R"] is not None:
        ref = ref + t(i["R"])
    if c.relu:
        ref = F.relu(ref)
    exp, bound = c.expected()
    assert exp.shape == tuple(ref.shape) == (c.B, c.OH, c.OW, c.Cout)
    d = np.abs(exp - ref.numpy()).max()
    assert d <= 1e-12 * max(1.0, np.abs(exp).max()), d
    assert (bound > 0).all()
    if c.relu:
        assert (exp == 0).any() and (exp > 0).any()          # the activation is on both of its branches
    small = np.abs(i["x"]) < 0.25
    assert 0.25 < small.mean() < 0.45 or i["x"].size < 64     # |x| < 0.25 in about a third of the entries


# ------------------------------------------------------------------------------------------ the forms
def _plan(c, kind, patch=True):
    from gomatching_amd import ops
    old = ops.CONV3_PATCH
    try:
        ops.CONV3_PATCH = patch
        return ops.conv_plan(c.rows, c.Cout, c.Cin, c.k, c.k, c.stride, c.pad, kind, residual=c.residual)
    finally:
        ops.CONV3_PATCH = old


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_conv_plan_chooses_the_declared_form(c):
    for kind in KINDS:
        assert _plan(c, kind) == c.forms[kind], (c.id, kind)
    nk = _cdiv(c.K, BK)
    if c.splits > 1:
        per = _cdiv(nk, c.splits)
        assert (per * c.splits != nk) == c.ragged, (nk, c.splits)
        assert 0 < nk - per * (c.splits - 1) <= per          # the last slice is not empty
    if c.patch:
        assert _plan(c, "f16x3", patch=False) == ("tile", 0)


def test_the_shapes_have_the_properties_they_are_there_for():
    by = {c.id: c for c in CASES}
    c = by["2x5x7-16to40-k3s1p1-bn_relu-R"]
    assert c.rows == 70 <= BM and c.OH * c.OW < c.rows and c.K == 144 and c.K % BK == 16 and c.Cout <= 64 and c.Cout % 4 == 0
    assert by["2x9x12-128to6-k3s2p1-bn_relu"].Cout % 4 and by["2x9x12-32to38-k3s1p1-bn-R"].Cout % 4
    c = by["3x9x11-32to38-k3s1p1-bias-R"]
    assert c.rows == 297 and _cdiv(c.rows, BM) == 3 and c.rows % BM and (c.OH * c.OW) % BM
    for cid in ("2x6x9-64to136-k3s2p1-none", "2x7x8-64to136-k3s2p1-none"):
        assert 128 < by[cid].Cout < 256 and by[cid].Cout % 128
    assert by["1x9x11-4to64-k7s2p3-bn_relu"].K == 196
    out = lambda o, n: o * 2 - 3 < 0 or o * 2 - 3 + 7 > n
    c = by["1x9x11-4to64-k7s2p3-bn_relu"]                    # (oh, ow) in {2} x {2, 3}: the window lies inside 9 x 11
    assert sum(not (out(oh, c.H) or out(ow, c.W)) for oh in range(c.OH) for ow in range(c.OW)) == 2
    c = by["1x7x11-4to64-k7s2p3-bn"]                         # every output touches padding: no 7 x 7 window fits inside 7 rows at pad 3
    assert all(out(oh, c.H) or out(ow, c.W) for oh in range(c.OH) for ow in range(c.OW))
    c = by["2x3x2-4to64-k7s2p3-bn_relu"]
    assert (c.OH, c.OW) == (2, 1) and c.H < c.k and c.W < c.k
    c = by["2x6x9-512to256-k3s2p1-bias"]
    assert c.splits == 9 and _cdiv(c.K, BK) == 9 * 16
    c = by["1x9x11-64to64-k7s2p3-bn_relu"]
    assert c.rows == 30 and _cdiv(c.K, BK) == 98 and c.splits == 6 and 98 - 5 * 17 == 13
    c = by["1x65x66-512to256-k3s1p1-bn_relu-R"]
    assert c.rows == 4290 and _cdiv(c.rows, BM) * 2 == 68 and c.splits == 7 and _cdiv(144, 7) == 21 and 144 - 6 * 21 == 18
    assert c.B * c.H * c.W * c.Cin * 4 < 9 * 2 ** 20
    assert len(SPLITK_CASES) == 3 and len(PATCH_CASES) == 8


# ------------------------------------------------------------------------------------------ the tile kernel's structure in numpy
def conv_emul(c, mistake=None):
    """The implicit GEMM of csrc/gemm_f16x3.hip in float64: row m -> (b, oh, ow), column k -> (kh, kw, c), taps outside the image read
    zero, the k-tiles past K read zero, split-K slices of cdiv(nk, splits) k-tiles summed in slice order, then the epilogue."""
    i = c.inputs()
    x, w = i["x"].astype(np.float64), i["w"].astype(np.float64)
    B, H, W, Cin, N, k, s, p = c.B, c.H, c.W, c.Cin, c.Cout, c.k, c.stride, c.pad
    OHd, OWd = c.OH, c.OW
    if mistake == "ceil_out":
        OHd, OWd = _cdiv(H + 2 * p - k, s) + 1, _cdiv(W + 2 * p - k, s) + 1
    M, K = c.rows, c.K
    nk = _cdiv(K, BK)
    Wm = np.zeros((N, nk * BK))
    Wm[:, :K] = w.reshape(N, K)
    kk = np.arange(nk * BK)
    ch, khw = kk % Cin, kk // Cin
    kh, kw = khw // k, khw % k
    if mistake == "kh_kw_swapped":
        kh, kw = kw, kh
    k_ok = kk < K
    if mistake == "k_tail_dropped" and K % BK:
        k_ok &= kk < (K // BK) * BK
    splits = max(1, c.splits)
    per = _cdiv(nk, splits)
    acc = np.zeros((M, N))
    for m0 in range(0, M, BM):
        m = np.arange(m0, min(M, m0 + BM))
        if mistake == "ow_oh_swapped":
            ow, t = m % OHd, m // OHd
            oh, b = t % OWd, t // OWd
        else:
            ow, t = m % OWd, m // OWd
            oh, b = t % OHd, t // OHd
        b = np.minimum(b, B - 1)
        if mistake == "tile_image0":
            b = np.where(b != b[0], 0, b)
        ih = (oh * s - p)[:, None] + kh[None]
        iw = (ow * (1 if mistake == "stride_one_axis" else s) - p)[:, None] + kw[None]
        inside = (ih >= 0) & (ih < H) & (iw >= 0) & (iw < W)
        ihc, iwc = np.clip(ih, 0, H - 1), np.clip(iw, 0, W - 1)
        if mistake == "pad_clamped":
            inside[:] = True
        A = np.where(inside & k_ok[None], x[b[:, None], ihc, iwc, ch[None]], 0.0)
        for sl in range(splits - (1 if mistake == "last_slice_dropped" else 0)):
            k0, k1 = sl * per * BK, min(nk, (sl + 1) * per) * BK
            acc[m] += A[:, k0:k1] @ Wm[:, k0:k1].T
    y = acc
    if i["scale"] is not None:
        y = y * i["scale"].astype(np.float64)
    if i["shift"] is not None:
        y = y + i["shift"].astype(np.float64)
    y = y.reshape(B, c.OH, c.OW, N)
    if i["R"] is not None:
        y = y + i["R"].astype(np.float64)
    if c.relu:
        y = np.maximum(y, 0)
    if mistake == "col_tail_skipped":
        y[..., (N // 4) * 4:] = 0.0
    return y


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_emulation_as_written_equals_the_statement(c):
    exp, bound = c.expected()
    r, at = worst(conv_emul(c), exp, bound)
    assert r <= 1e-6, (c.id, r, at)                          # float64 in another order: a millionth of the bound


# mistake -> (the case that catches it, why that case can)
MISTAKES = {
    # 2x5x7-16to40-k3s1p1-bn_relu-R: w[n, kh, kw] is not symmetric in (kh, kw), so every interior output moves
    "kh_kw_swapped": ("2x5x7-16to40-k3s1p1-bn_relu-R", "any k > 1 case: random weights are not symmetric in the taps"),
    # 2x5x7-16to40-k3s1p1-bn_relu-R: pad 1 on a 5 x 7 image, 20 of 35 outputs per image read padding
    "pad_clamped": ("2x5x7-16to40-k3s1p1-bn_relu-R", "any padded case: border outputs read the edge pixel instead of zero"),
    # 2x6x9-64to136-k3s2p1-none: H + 2p - k = 5 is odd, so the ceiling gives OH = 4 for 3 and every row past the first image row decodes wrong
    "ceil_out": ("2x6x9-64to136-k3s2p1-none", "stride 2 with (H + 2p - k) or (W + 2p - k) odd"),
    # 2x6x9-64to136-k3s2p1-none: OW = 5 > 1 at stride 2
    "stride_one_axis": ("2x6x9-64to136-k3s2p1-none", "stride 2 with OW > 1"),
    # 2x5x7-16to40-k3s1p1-bn_relu-R: OH = 5, OW = 7
    "ow_oh_swapped": ("2x5x7-16to40-k3s1p1-bn_relu-R", "OH != OW"),
    # 2x5x7-16to40-k3s1p1-bn_relu-R: K = 144 = 4 k-tiles + 16 (the tap (2, 2)); also 1x9x11-4to64-k7s2p3-bn_relu (K = 196 = 6 k-tiles + 4)
    "k_tail_dropped": ("2x5x7-16to40-k3s1p1-bn_relu-R", "K % 32 != 0"),
    # 1x9x11-64to64-k7s2p3-bn_relu: the sixth slice holds k-tiles 85 .. 97
    "last_slice_dropped": ("1x9x11-64to64-k7s2p3-bn_relu", "every split-K case"),
    # 2x5x7-16to40-k3s1p1-bn_relu-R: rows 35 .. 69 of the one M tile belong to image 1
    "tile_image0": ("2x5x7-16to40-k3s1p1-bn_relu-R", "B > 1 with an M tile that crosses an image boundary"),
    # 2x9x12-128to6-k3s2p1-bn_relu: columns 4 and 5
    "col_tail_skipped": ("2x9x12-128to6-k3s2p1-bn_relu", "Cout % 4 != 0"),
}


@pytest.mark.parametrize("mistake", sorted(MISTAKES))
def test_planted_mistake_leaves_the_bound_on_its_named_case(mistake):
    c = case(MISTAKES[mistake][0])
    exp, bound = c.expected()
    r, at = worst(conv_emul(c, mistake), exp, bound)
    also = []
    for o in CASES:                                          # which other small cases show it (printed, not asserted)
        if o is not c and o.rows * o.K <= 1 << 20 and worst(conv_emul(o, mistake), *o.expected())[0] > 1.0:
            also.append(o.id)
    print("conv %-18s %s: worst |d| / bound = %.3g at %s; also caught by %d cases, e.g. %s" % (mistake, c.id, r, at, len(also), also[:3]))
    assert r > 1.0, (mistake, c.id, r)
    if mistake == "k_tail_dropped":
        o = case("1x9x11-4to64-k7s2p3-bn_relu")
        assert worst(conv_emul(o, mistake), *o.expected())[0] > 1.0
    if mistake == "last_slice_dropped":
        assert all(worst(conv_emul(o, mistake), *o.expected())[0] > 1.0 for o in SPLITK_CASES if o.rows <= 1024)
    if mistake == "ceil_out":
        o = case("2x7x8-64to136-k3s2p1-none")                # W + 2p - k = 7
        assert worst(conv_emul(o, mistake), *o.expected())[0] > 1.0


# ------------------------------------------------------------------------------------------ exact-integer inputs
@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_exact_integer_inputs_are_exact_in_float32(c):
    i = c.inputs(exact=True)
    assert 6 * c.K < 2 ** 24
    for name in ("x", "w", "shift", "R"):
        if i[name] is not None:
            assert np.array_equal(i[name], np.round(i[name]))
    assert np.abs(i["x"]).max() <= 3 and np.abs(i["w"]).max() <= 2
    if i["scale"] is not None:
        assert set(np.unique(i["scale"]).tolist()) <= {0.5, 1.0, 2.0}
    exp, _ = c.expected(exact=True)
    got = conv32(i["x"], i["w"], c.stride, c.pad, i["scale"], i["shift"], i["R"], c.relu)
    assert got.dtype == np.float32 and np.array_equal(got.astype(np.float64), exp)
    assert np.array_equal(exp.astype(np.float32).astype(np.float64), exp) and np.abs(exp).max() < 2 ** 22
    if c.rows * c.Cout >= 64:
        assert len(np.unique(exp)) > 4                       # not a degenerate output
