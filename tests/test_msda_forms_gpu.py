"""GPU: every form of the MSDA sampling kernels (csrc/msda.hip) against the fp64 statement of tests/helpers.py, on inputs built
to sit where a bilinear gather goes wrong, plus the bit-identities the forms claim among themselves.

Forms: the 1:1 op (msda_fwd_kernel) and its strided entry; msda_prepare (ref_levels 1 and 4); the fused op with and without
valid ratios on the lane-distributed kernel (ops.MSDA_LANES on) and on msda_fused_kernel (off, or a batch stride >= 2^29
floats); the encoder's LDS-window kernels.

Bound, element-wise:  |got - exp| <= 2^-24 * (KAPPA * A + Sw) + Lip + TINY * max|v|,  where
  * A = the statement on |value| and |w| (sum |w * v| per output);
  * KAPPA = 128: one output accumulates 16 samples x 4 corners (64 fp32 sums) over fp32 corner weights (1 - l, two products,
    the attention weight: a few roundings per term) -- about 2 x 64 roundings of at most 2^-24 * A each;
  * Sw (fused forms only) = the statement on |value| and |w| * (|d| + 32), d = logit - max: the fp32 softmax -- expf(d) with d
    rounded (|d| ulps), the 16-term sum, the reciprocal and product (32 ulps);
  * Lip = 2 max|v| * sum_s |w_s| (dh_s + dw_s): dh, dw = the spread, in pixels, of the fp32 pixel coordinate over the ways a
    compiler may evaluate it (y * H - 0.5 with or without a fused multiply-add, ref * vr + q likewise, off / W correctly rounded or
    as the fused kernels' reciprocal plus one correction).  The bilinear blend is continuous (zero at the window's edge) with
    slope <= 2 max|v| per pixel.  On the exact-location inputs (offsets on the W / 4096 grid, reference points on the 2^-12 grid)
    every dh, dw is 0; only the ratios that are not short binary fractions (5/6, 2/3) and the arbitrary-offset case have any.
  * plus TINY * max|v|, TINY = 64 * 2^-126: weights (e^d for d < -87, their products with the corner weights) that leave fp32's
    normal range.  A corner that carries any weight fp32 can hold is far above it.
"""
import numpy as np
import pytest
import torch

from helpers import msda64, msda_locations32, msda_softmax64

pytestmark = pytest.mark.gpu

DEV = "cuda"
U = 2.0 ** -24
KAPPA = 128
SOFTMAX_ULPS = 32
TINY = 64 * 2.0 ** -126       # fp32's range: 64 weights below the smallest normal, flushed or rounded to a subnormal

BENCH = [(125, 223), (63, 112), (32, 56), (16, 28)]
ODD = [(37, 53), (19, 27), (10, 14), (5, 7)]
THIN = [(16, 32), (1, 64), (32, 1), (1, 1)]          # 1 x 1, 1 x W, H x 1; powers of two: every edge target is exact
VR = [(0.75, 0.5), (5 / 6, 2 / 3), (1.0, 0.5), (0.5, 1.0)]
F32 = np.float32


def _ops():
    from gomatching_amd import ops
    return ops


def _pyr(shapes):
    ss = torch.as_tensor(shapes, dtype=torch.long)
    lsi = torch.cat((ss.new_zeros((1,)), ss.prod(1).cumsum(0)[:-1]))
    return ss, lsi, int(ss.prod(1).sum())


def _targets(n):
    """Pixel coordinates where a gather goes wrong along an axis of n pixels: the window's edges -1 and n, the padding's
    half-pixel -0.5 and n - 0.5, the first and last pixel 0 and n - 1, integers, half-integers, just outside."""
    return np.array([-1.0, -0.5, 0.0, 0.5, 1.0, n - 1.5, n - 1.0, n - 0.5, float(n), -1.5, n + 0.5, n // 2, n // 2 + 0.5])


def _neighbours(x):
    """x and the fp32 values one ulp either side."""
    x = x.astype(F32)
    return np.stack([np.nextafter(x, F32(-np.inf)), x, np.nextafter(x, F32(np.inf))], -1)


# ------------------------------------------------------------------------------------------ inputs
def _logits(rng, Q):
    """Per (query, head), cycling: all equal; one dominant; spread over +-80; ~1e4 (overflows without the max subtraction)."""
    lg = np.zeros((Q, 8, 16), F32)
    kind = (np.arange(Q)[:, None] + np.arange(8)[None]) % 4
    lg[kind == 0] = 3.25
    dom = rng.standard_normal((Q, 8, 16)).astype(F32)
    dom[np.arange(Q)[:, None], np.arange(8)[None], rng.integers(0, 16, (Q, 8))] += 25.0
    lg[kind == 1] = dom[kind == 1]
    lg[kind == 2] = rng.uniform(-80, 80, (Q, 8, 16)).astype(F32)[kind == 2]
    lg[kind == 3] = (1e4 + rng.uniform(-6, 6, (Q, 8, 16))).astype(F32)[kind == 3]
    return lg.reshape(Q, 128)


def _fused_inputs(shapes, B, Lq, seed, vr=None, exact=True, fine=False):
    """raw [B*Lq, 384] (offsets | logits) and ref [B*Lq, 2] for the fused forms.

    exact: reference points on the 2^-12 grid, offsets fp32 multiples of (W_l or H_l) / 4096 -- off / W is exact for IEEE division
    and for the kernels' reciprocal + one correction, so kernel and statement see the same fp32 coordinates.  Otherwise
    arbitrary reals.  Half of the samples are a few pixels around the query, the rest aimed at the edges of their level: both
    axes on an edge target, one on an edge and the other outside the window, far outside (|loc| ~ 1e6), raw offsets of +-1e12.
    fine: every query's reference point is itself an edge target (or one fp32 ulp either side) of one level, whose samples then
    carry offset 0 -- the ulp neighbours of the window edges, reachable only through a full-precision reference point."""
    rng = np.random.default_rng(seed)
    Q = B * Lq
    H = np.array([h for h, _ in shapes], np.float64)
    W = np.array([w for _, w in shapes], np.float64)
    n_ax = np.stack([W, H], -1)                                           # [L, 2] (x, y) sizes
    if exact:
        ref = (rng.integers(-400, 4096 + 400, (Q, 2)) / 4096.0).astype(F32)
    else:
        ref = rng.uniform(-0.1, 1.1, (Q, 2)).astype(F32)
    vr_a = np.ones((4, 2), F32) if vr is None else np.asarray(vr, F32)
    if fine:
        lev = rng.integers(0, 4, Q)
        for ax in range(2):
            n = n_ax[lev, ax]
            tg = np.array([rng.choice(_targets(int(k))) for k in n])
            tg = _neighbours(tg)[np.arange(Q), rng.integers(0, 3, Q)].astype(np.float64)
            ref[:, ax] = ((tg + 0.5) / n / vr_a[lev, ax]).astype(F32)
    refv = (ref[:, None, :] * vr_a[None]).astype(np.float64)               # [Q, L, 2]
    shape = (Q, 8, 4, 4, 2)
    nn = np.broadcast_to(n_ax[None, None, :, None, :], shape)
    rv = np.broadcast_to(refv[:, None, :, None, :], shape)
    pix = rng.uniform(-6, 6, shape)                                       # a few pixels around the query
    kind = rng.integers(0, 10, shape[:4])
    tgt = np.empty(shape)
    for l in range(4):
        for ax in range(2):
            tl = _targets(int(n_ax[l, ax]))
            tgt[:, :, l, :, ax] = tl[rng.integers(0, len(tl), shape[:2] + (4,))]
    edge = (kind >= 5) & (kind <= 7)
    pix[edge] = (tgt + 0.5 - rv * nn)[edge]                               # both axes on an edge target
    half = kind == 8                                                      # one axis on an edge, the other outside the window
    out_ax = rng.integers(0, 2, shape[:4])
    for ax in range(2):
        sel = half & (out_ax == ax)
        far = np.where(rng.random(shape[:4]) < 0.5, -1.0 - rng.uniform(0, 3, shape[:4]), nn[..., ax] + rng.uniform(0, 3, shape[:4]))
        pix[..., ax][sel] = (far + 0.5 - rv[..., ax] * nn[..., ax])[sel]
        pix[..., 1 - ax][sel] = (tgt[..., 1 - ax] + 0.5 - rv[..., 1 - ax] * nn[..., 1 - ax])[sel]
    if exact:
        off = (np.round(pix * 4096.0 / nn) * nn / 4096.0).astype(F32)      # multiples of n / 4096: exact in fp32
    else:
        off = pix.astype(F32)
    farout = kind == 9
    big = np.where(rng.random(shape) < 0.5, 1e6 * nn, 1e12) * np.sign(rng.standard_normal(shape))   # |loc| ~ 1e6 | raw 1e12
    off[farout] = big.astype(F32)[farout]
    if fine:                                                              # the reference point's own level: offset 0
        off[np.arange(Q)[:, None], :, lev[:, None]] = 0.0
    raw = np.concatenate([off.reshape(Q, 256), _logits(rng, Q)], 1)
    assert np.isfinite(raw).all()
    return raw, ref


def _wide_value(value, ld, col, gap):
    """value [B,S,8,32] laid out as a column slice [S, 256] at `col` of a [S, ld] buffer per frame, frames `gap` floats apart
    (batch stride S*ld + gap > S*ld), NaN everywhere outside the slices -> (buffer, value2d of frame 0, batch stride)."""
    B, S = value.shape[:2]
    bs = S * ld + gap
    flat = torch.full(((B - 1) * bs + S * ld,), float("nan"), device=DEV)
    for b in range(B):
        flat[b * bs:b * bs + S * ld].view(S, ld)[:, col:col + 256] = value[b].reshape(S, 256).to(DEV)
    return flat, torch.as_strided(flat, (S, 256), (ld, 1), col), bs


def _raw_dev(raw, ld=448):
    """raw rows inside a wider buffer, NaN in the columns past 384."""
    buf = torch.full((raw.shape[0], ld), float("nan"), device=DEV)
    buf[:, :384] = torch.from_numpy(raw).to(DEV)
    return buf[:, :384]


# ------------------------------------------------------------------------------------------ bound
def _kdiv(o, n):
    """off / n as the fused kernels compute it: q = o * (1/n), r = fma(-q, n, o), q += r * (1/n)."""
    rn = F32(1.0) / F32(n)
    q = (o * rn).astype(F32)
    r = (o.astype(np.float64) - q.astype(np.float64) * float(n)).astype(F32)
    return (r.astype(np.float64) * float(rn) + q.astype(np.float64)).astype(F32)


def _spread(locs, shapes):
    """[..., L, P, 2] fp32 candidate locations (first = the statement's) -> per sample (dx + dy) in pixels over the candidates
    and over y * n - 0.5 with and without a fused multiply-add; 0 where every candidate is outside the window on one axis."""
    n_ax = np.array([[w, h] for h, w in shapes], np.float64)[:, None, :]  # [L, 1, 2]
    pix = []
    for c in locs:
        c64 = c.astype(np.float64)
        pix.append((((c * n_ax.astype(F32)).astype(F32) - F32(0.5)).astype(F32)).astype(np.float64))
        pix.append((c64 * n_ax - 0.5).astype(F32).astype(np.float64))
    pix = np.stack(pix)                                                   # [C, ..., L, P, 2]
    with np.errstate(invalid="ignore"):
        dev = np.abs(pix - pix[:1]).max(0)
        out = ((pix <= -1) | (pix >= n_ax) | np.isnan(pix)).all(0)       # [..., 2]
    dev = np.where(out.any(-1, keepdims=True), 0.0, dev)
    assert np.isfinite(dev).all()
    return dev.sum(-1)


def _bound(value, shapes, lsi, loc, w, spread=None, d=None):
    """(2^-24 (KAPPA A + Sw) + Lip + TINY max|v|, Lip + TINY max|v|), element-wise: [B, Lq, 256] float64."""
    va, wa = value.abs(), w.abs()
    b = KAPPA * U * msda64(va, shapes, lsi, loc, wa)
    slack = torch.full_like(b, TINY * float(va.max()))
    if d is not None:
        b += U * msda64(va, shapes, lsi, loc, wa * (torch.from_numpy(np.abs(d)).view(w.shape) + SOFTMAX_ULPS))
    if spread is not None:
        lip = 2 * float(va.max()) * (wa * torch.from_numpy(spread).view(w.shape)).sum((3, 4))      # [B, Lq, 8]
        slack += lip.repeat_interleave(32, -1)
    return b + slack, slack


RATIOS = {}


def _check(got, exp, mag, bound, slack, form):
    """Element-wise bound; records the form's worst (|got - exp| - Lip - TINY max|v|) / (2^-24 sum|w v|), printed at the end."""
    got = got.detach().cpu().double().reshape(exp.shape)
    bound = bound.reshape(exp.shape)
    err = (got - exp).abs()
    ok = err <= bound
    assert bool(ok.all()), "%s: %d elements out of bound, worst at %s: got %r exp %r bound %.3e" % (
        form, int((~ok).sum()), tuple(int(i) for i in np.unravel_index(int((~ok).view(-1).nonzero()[0]), tuple(exp.shape))),
        float(got.view(-1)[(~ok).view(-1)][0]), float(exp.view(-1)[(~ok).view(-1)][0]), float(bound.view(-1)[(~ok).view(-1)][0]))
    r = float(((err - slack.reshape(err.shape)).clamp(min=0) / (U * mag)).nan_to_num(0.0, posinf=0.0).max())
    RATIOS[form] = max(RATIOS.get(form, 0.0), r)


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for k, v in sorted(RATIOS.items()):
        print("msda worst |got-exp| / (2^-24 sum|w v|)  %-34s %.2f" % (k, v))


def _fused_statement(value, shapes, lsi, raw, ref, B, Lq, vr):
    """(exp, mag, bound) of the fused forms on these inputs."""
    loc = msda_locations32(raw, ref, shapes, vr)
    w, d = msda_softmax64(raw)
    Q = B * Lq
    # the other ways a compiler / the kernels may evaluate the location
    off = raw[:, :256].reshape(Q, 8, 4, 4, 2)
    qk = np.empty_like(off)
    for l, (h, w_) in enumerate(shapes):
        qk[:, :, l, :, 0] = _kdiv(off[:, :, l, :, 0], w_)
        qk[:, :, l, :, 1] = _kdiv(off[:, :, l, :, 1], h)
    q = off / np.array([[w_, h] for h, w_ in shapes], F32)[None, None, :, None, :]
    r = np.asarray(ref, F32).reshape(Q, 1, 1, 1, 2)
    va = np.ones((4, 2), F32) if vr is None else np.asarray(vr, F32)
    rsep = (r * va[None, None, :, None, :]).astype(F32)
    cands = [loc]
    for qq in (q, qk):
        cands.append((rsep + qq).astype(F32))
        cands.append((r.astype(np.float64) * va.astype(np.float64)[None, None, :, None, :] + qq.astype(np.float64)).astype(F32))
    spread = _spread(cands, shapes)
    loc_t = torch.from_numpy(loc).view(B, Lq, 8, 4, 4, 2)
    w_t = torch.from_numpy(w).view(B, Lq, 8, 4, 4)
    exp = msda64(value, shapes, lsi, loc_t, w_t)
    mag = msda64(value.abs(), shapes, lsi, loc_t, w_t)
    bound, slack = _bound(value, shapes, lsi, loc_t, w_t, spread, d)
    return exp.view(Q, 256), mag.view(Q, 256), (bound.view(Q, 256), slack.view(Q, 256)), spread


class _Lanes:
    """ops.MSDA_LANES set for the block, restored after."""

    def __init__(self, on):
        self.on = on

    def __enter__(self):
        self.ops = _ops()
        self.old = self.ops.MSDA_LANES
        self.ops.MSDA_LANES = self.on

    def __exit__(self, *a):
        self.ops.MSDA_LANES = self.old


# ------------------------------------------------------------------------------------------ 1:1 op
def _one_to_one_loc(shapes, B, Lq, seed):
    """loc [B,Lq,8,4,4,2] fp32: edge targets and their ulp neighbours on both axes, one axis outside, far outside (|loc| ~ 1e6),
    NaN / +-inf, and plain samples in the map; w [B,Lq,8,4,4] positive, spread over decades."""
    rng = np.random.default_rng(seed)
    shape = (B, Lq, 8, 4, 4, 2)
    loc = rng.uniform(-0.05, 1.05, shape)
    kind = rng.integers(0, 10, shape[:5])
    for l, (h, w_) in enumerate(shapes):
        for ax, n in ((0, w_), (1, h)):
            t = _neighbours(_targets(n)).reshape(-1).astype(np.float64)
            pick = t[rng.integers(0, len(t), shape[:2] + (8, 4))]
            sl = loc[:, :, :, l, :, ax]
            e = kind[:, :, :, l, :] <= 5
            sl[e] = ((pick + 0.5) / n)[e]
            o = (kind[:, :, :, l, :] == 6) & (rng.random(shape[:2] + (8, 4)) < 0.5)
            sl[o] = (rng.choice([-1.7, -1.0, n, n + 1.3], size=shape[:2] + (8, 4)) + 0.5)[o] / n
    far = kind == 7
    loc[far] = rng.choice([-1e6, 1e6, 3e5], size=far.shape + (2,))[far]
    loc = loc.astype(F32)
    bad = kind == 8
    special = np.array([np.nan, np.inf, -np.inf, 0.5], F32)
    loc[..., 0][bad] = special[rng.integers(0, 4, bad.shape)][bad]
    loc[..., 1][bad] = special[rng.integers(0, 3, bad.shape)][bad]
    w = (rng.random(shape[:5]) * 10.0 ** rng.integers(-3, 2, shape[:5])).astype(F32)
    return loc, w


@pytest.mark.parametrize("shapes,B,Lq", [(THIN, 1, 1), (THIN, 3, 11), (ODD, 1, 5), (BENCH, 1, 101), (BENCH, 3, 1)])
def test_one_to_one_op_and_strided_entry(shapes, B, Lq):
    """gom_ms_deform_attn_forward (msda_fwd_kernel) on the edge samples, and gom_ms_deform_attn_forward_strided on the same
    value read in place from a decoder-like [S, 1536] buffer at column 768 with NaN around it: the same bits."""
    ops = _ops()
    ss, lsi, S = _pyr(shapes)
    g = torch.Generator().manual_seed(S + B * 7 + Lq)
    value = torch.randn(B, S, 8, 32, generator=g)
    loc, w = _one_to_one_loc(shapes, B, Lq, S + Lq)
    loc_t, w_t = torch.from_numpy(loc), torch.from_numpy(w)
    out = ops.ms_deform_attn_forward(value.to(DEV), ss.to(DEV), lsi.to(DEV), loc_t.to(DEV), w_t.to(DEV))
    exp = msda64(value, ss, lsi, loc_t, w_t)
    mag = msda64(value.abs(), ss, lsi, loc_t, w_t.abs())
    spread = _spread([loc.reshape(B, Lq, 8, 4, 4, 2)], shapes)
    bound = _bound(value, ss, lsi, loc_t, w_t.double(), spread)
    _check(out, exp, mag, *bound, "1:1 op")
    flat, v2d, bs = _wide_value(value, 1536, 768, 4 * 37)
    st = ops.ms_deform_attn_forward_strided(v2d, bs, ss.to(DEV), lsi.to(DEV), loc_t.to(DEV), w_t.to(DEV), B, Lq)
    assert torch.equal(st, out.view(B * Lq, 256))
    _check(st, exp, mag, *bound, "strided 1:1 op")


# ------------------------------------------------------------------------------------------ prepare
@pytest.mark.parametrize("ref_levels", [1, 4])
def test_prepare_locations_bitexact_and_weights(ref_levels):
    """msda_prepare: locations equal numpy's IEEE fp32 arithmetic bit for bit (HIP's default fp32 division is correctly
    rounded); weights within (|logit - max| + 32) ulps of the float64 softmax (2^-126 absolute: fp32's normal range)."""
    ops = _ops()
    shapes = ODD
    ss, _, _ = _pyr(shapes)
    Q = 4 * 8 * 3 + 5
    raw, ref = _fused_inputs(shapes, 1, Q, 11, exact=False)
    rng = np.random.default_rng(12)
    refs = rng.uniform(-0.1, 1.1, (Q, ref_levels, 2)).astype(F32)
    refs[:, 0] = ref
    loc, w = ops.msda_prepare(_raw_dev(raw), torch.from_numpy(refs).to(DEV), ss.to(DEV), ref_levels=ref_levels)
    want = msda_locations32(raw, refs, shapes)
    got = loc.cpu().numpy()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), "%d locations differ" % int((got != want).sum())
    w64, d = msda_softmax64(raw)
    err = np.abs(w.cpu().numpy().astype(np.float64) - w64)
    assert (err <= (np.abs(d) + SOFTMAX_ULPS) * U * w64 + 2.0 ** -126).all(), float((err / (U * w64)).max())
    normal = w64 > 2.0 ** -100
    RATIOS["prepare w (ulps of w)"] = max(RATIOS.get("prepare w (ulps of w)", 0.0), float((err[normal] / (U * w64[normal])).max()))


# ------------------------------------------------------------------------------------------ fused forms
FUSED_CASES = [  # name, shapes, B, Lq, exact, fine, value layout (ld, col, gap)
    ("thin-ulp", THIN, 1, 5, True, True, (640, 384, 0)),
    ("thin", THIN, 3, 11, True, False, (640, 384, 64)),
    ("odd", ODD, 1, 33, True, False, (1536, 768, 4 * 101)),
    ("bench-1", BENCH, 1, 1, True, False, (640, 384, 0)),
    ("bench-3", BENCH, 3, 1, True, True, (640, 384, 16)),
    ("bench-101", BENCH, 1, 4 * 8 * 3 + 5, True, False, (640, 384, 32)),
    ("decoder", BENCH, 2, 100 * 25, True, False, (1536, 256, 4 * 7)),
    ("odd-real", ODD, 2, 37, False, False, (1536, 1280, 4)),
]


@pytest.mark.parametrize("case", FUSED_CASES, ids=[c[0] for c in FUSED_CASES])
@pytest.mark.parametrize("with_vr", [False, True], ids=["plain", "vr"])
def test_fused_forms_against_statement(case, with_vr):
    """ops.msda_fused with ops.MSDA_LANES on (msda_fused_lanes_kernel) and off (msda_fused_kernel), with and without valid ratios
    that differ per axis and level: each within the bound, and the two kernels bit-identical."""
    ops = _ops()
    name, shapes, B, Lq, exact, fine, (ld, col, gap) = case
    ss, lsi, S = _pyr(shapes)
    vr = VR if with_vr else None
    raw, ref = _fused_inputs(shapes, B, Lq, len(name) * 31 + B + Lq, vr=vr, exact=exact, fine=fine)
    g = torch.Generator().manual_seed(B * Lq + S)
    value = torch.randn(B, S, 8, 32, generator=g)
    exp, mag, bound, spread = _fused_statement(value, shapes, lsi, raw, ref, B, Lq, vr)
    if exact and not fine and not with_vr:
        assert not spread.any(), "exact inputs must give the kernels and the statement the same fp32 coordinates"
    flat, v2d, bs = _wide_value(value, ld, col, gap)
    raw_d, ref_d = _raw_dev(raw), torch.from_numpy(ref).to(DEV)
    vr_d = None if vr is None else torch.tensor(vr, dtype=torch.float32, device=DEV)
    outs = {}
    for lanes in (True, False):
        with _Lanes(lanes):
            outs[lanes] = ops.msda_fused(raw_d, ref_d, v2d, bs, ss.to(DEV), lsi.to(DEV), B, Lq, vr_d)
        _check(outs[lanes], exp, mag, *bound, "fused %s %s" % ("lanes" if lanes else "msda_fused_kernel", "vr" if vr else "plain"))
    assert torch.equal(outs[True], outs[False])


def test_fused_batch_stride_at_2p29_takes_the_gather_kernel():
    """A batch stride of 2^29 + 16 floats (the second frame 2 GB in): every fused entry takes msda_fused_kernel (64-bit
    addressing) and gives the lane kernel's bits on the same data at a small stride."""
    ops = _ops()
    shapes, B, Lq = ODD, 2, 45
    ss, lsi, S = _pyr(shapes)
    raw, ref = _fused_inputs(shapes, B, Lq, 99)
    g = torch.Generator().manual_seed(99)
    value = torch.randn(B, S, 8, 32, generator=g)
    exp, mag, bound, _ = _fused_statement(value, shapes, lsi, raw, ref, B, Lq, None)
    exp_vr, mag_vr, bound_vr, _ = _fused_statement(value, shapes, lsi, raw, ref, B, Lq, VR)
    raw_d, ref_d = _raw_dev(raw), torch.from_numpy(ref).to(DEV)
    vr_d = torch.tensor(VR, dtype=torch.float32, device=DEV)
    small_flat, small, small_bs = _wide_value(value, 256, 0, 64)
    with _Lanes(True):
        want = ops.msda_fused(raw_d, ref_d, small, small_bs, ss.to(DEV), lsi.to(DEV), B, Lq)
        want_vr = ops.msda_fused(raw_d, ref_d, small, small_bs, ss.to(DEV), lsi.to(DEV), B, Lq, vr_d)
        del small_flat, small
        big_bs = (1 << 29) + 16
        flat, v2d, bs = _wide_value(value, 256, 0, big_bs - S * 256)
        assert bs == big_bs
        got = ops.msda_fused(raw_d, ref_d, v2d, bs, ss.to(DEV), lsi.to(DEV), B, Lq)
        got_vr = ops.msda_fused(raw_d, ref_d, v2d, bs, ss.to(DEV), lsi.to(DEV), B, Lq, vr_d)
        torch.cuda.synchronize()
        del flat, v2d
        torch.cuda.empty_cache()
    assert torch.equal(got, want) and torch.equal(got_vr, want_vr)
    _check(got, exp, mag, *bound, "fused 2^29 stride plain")
    _check(got_vr, exp_vr, mag_vr, *bound_vr, "fused 2^29 stride vr")


def test_encoder_entry_at_2p29_falls_back_to_the_gather_kernel():
    """gom_msda_fused_forward_encoder with a batch stride >= 2^29 floats leaves the window kernels for msda_fused_kernel."""
    ops = _ops()
    shapes, B = [(9, 20), (5, 10), (3, 5), (2, 3)], 2
    ss, lsi, S = _pyr(shapes)
    g = torch.Generator().manual_seed(5)
    value = torch.randn(B, S, 8, 32, generator=g)
    raw = torch.randn(B * S, 384, generator=g)
    raw[:, :256] *= 3.0
    raw_d = raw.to(DEV)
    ref = ops.encoder_reference_points(ss.to(DEV), lsi.to(DEV), S).repeat(B, 1).contiguous()
    small_flat, small, small_bs = _wide_value(value, 256, 0, 0)
    with _Lanes(True):
        want = ops.msda_fused(raw_d, ref, small, small_bs, ss.to(DEV), lsi.to(DEV), B, S)
        flat, v2d, bs = _wide_value(value, 256, 0, (1 << 29) + 32 - S * 256)
        got = ops.msda_fused(raw_d, ref, v2d, bs, ss.to(DEV), lsi.to(DEV), B, S, encoder_hw0=shapes[0] + shapes[1])
        torch.cuda.synchronize()
        del flat, v2d
        torch.cuda.empty_cache()
    assert torch.equal(got, want)


# ------------------------------------------------------------------------------------------ encoder windows
R_HALO = 5                                            # gom_msda_fused_forward_encoder's R


@pytest.mark.parametrize("shapes", [ODD, [(21, 40), (11, 20), (6, 10), (3, 5)]])
def test_encoder_window_at_the_halo_edge(shapes):
    """The LDS-window kernels (level-0 tiles, and level-1 tiles) against the gather kernel on offsets of exactly R-1, R-0.5, R,
    R+0.5, R+1 pixels at every level, in every tile (edges of the map included), on maps that are not multiples of 8 x 16: the
    same bits.  With every |offset| <= R-1 no octet group leaves its window.  One run is also held to the statement."""
    ops = _ops()
    B = 2
    ss, lsi, S = _pyr(shapes)
    rng = np.random.default_rng(S)
    g = torch.Generator().manual_seed(S)
    value = torch.randn(B, S, 8, 32, generator=g)
    rv = torch.empty(B * S, 640)
    rv[:, 384:] = value.view(B * S, 256)
    R = float(R_HALO)
    ref = ops.encoder_reference_points(ss.to(DEV), lsi.to(DEV), S).repeat(B, 1).contiguous()
    hw01 = tuple(shapes[0]) + tuple(shapes[1])
    counter = torch.zeros((1,), dtype=torch.int32, device=DEV)
    old = ops.MSDA_WINDOW, ops.MSDA_WINDOW_L1
    try:
        ops.MSDA_WINDOW = True
        for steps, inside in (([0.0, R - 1, R - 0.5, R, R + 0.5, R + 1], False), ([0.0, 1.0, 2.5, R - 1], True)):
            mag = np.array(steps)[rng.integers(0, len(steps), (B * S, 128, 2))] * rng.choice([-1.0, 1.0], (B * S, 128, 2))
            rv[:, :256] = torch.from_numpy(mag.reshape(B * S, 256)).float()
            rv[:, 256:384] = torch.from_numpy(_logits(rng, B * S))
            d = rv.to(DEV)
            with _Lanes(True):
                plain = ops.msda_fused(d[:, :384], ref, d[:, 384:], S * 640, ss.to(DEV), lsi.to(DEV), B, S)
                for l1, hw in ((False, tuple(shapes[0])), (True, hw01)):
                    ops.MSDA_WINDOW_L1 = l1
                    win = ops.msda_fused(d[:, :384], ref, d[:, 384:], S * 640, ss.to(DEV), lsi.to(DEV), B, S, encoder_hw0=hw,
                                         fallback_counter=counter)
                    assert torch.equal(win, plain), (steps, l1, float((win - plain).abs().max()))
                    if inside:
                        assert int(counter.item()) == 0, "offsets within R-1 pixels must stay inside the windows"
                    else:
                        assert int(counter.item()) > 0
            if not inside:
                raw = rv[:, :384].numpy()
                exp, mag_, bound, _ = _fused_statement(value, shapes, lsi, raw, ref.cpu().numpy(), B, S, None)
                _check(win, exp, mag_, *bound, "encoder window")
    finally:
        ops.MSDA_WINDOW, ops.MSDA_WINDOW_L1 = old


# ------------------------------------------------------------------------------------------ padded-batch inputs
def _vshapes(shapes):
    return [(max(1, (h * 3 + 3) // 4), max(1, (w * 2 + 2) // 3)) for h, w in shapes]


@pytest.mark.parametrize("col0,ld", [(384, 640), (0, 1536)])
def test_zero_padded_tokens(col0, ld):
    """ops.zero_padded_tokens_ zeroes exactly the columns [col0, col0 + ncols) of the tokens outside their level's valid
    extent (ms_deform_attn.py:134-135: value.masked_fill(padding_mask, 0)), for the encoder's (384, 256) and the decoder's
    (0, full width) ranges, and leaves every other element as it was."""
    ops = _ops()
    shapes, B = ODD, 2
    ss, lsi, S = _pyr(shapes)
    vs = _vshapes(shapes)
    ncols = 256 if col0 == 384 else ld
    g = torch.Generator().manual_seed(ld)
    buf = torch.randn(B * S, ld, generator=g)
    mask = torch.zeros(S, dtype=torch.bool)                               # padding mask of one frame
    for l, ((h, w), (hv, wv)) in enumerate(zip(shapes, vs)):
        yy, xx = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
        mask[int(lsi[l]):int(lsi[l]) + h * w] = ((yy >= hv) | (xx >= wv)).reshape(-1)
    want = buf.clone()
    want[:, col0:col0 + ncols][mask.repeat(B)] = 0.0
    got = ops.zero_padded_tokens_(buf.to(DEV), col0, ncols, ss.to(DEV), lsi.to(DEV), torch.tensor(vs).to(DEV), B, S)
    assert torch.equal(got.cpu(), want)
    assert 0 < int(mask.sum()) < S


def test_encoder_reference_points_with_valid_ratios():
    """ops.encoder_reference_points(..., vshapes) x vr[l] (the fused kernels' HAS_VR scaling) against the oracle's
    encoder_reference_points(shapes, valid_ratios) (deformable_transformer.py:288-300): within one fp32 rounding."""
    from oracle import gom_oracle as O
    ops = _ops()
    shapes = ODD
    ss, lsi, S = _pyr(shapes)
    vs = _vshapes(shapes)
    vr = np.array([[F32(v[1]) / F32(s[1]), F32(v[0]) / F32(s[0])] for v, s in zip(vs, shapes)], F32)   # (Wv/W, Hv/H)
    ref = ops.encoder_reference_points(ss.to(DEV), lsi.to(DEV), S, torch.tensor(vs).to(DEV)).cpu()
    got = ref[:, None, :] * torch.from_numpy(vr)[None]                    # [S, L, 2]
    want = O.encoder_reference_points(shapes, torch.from_numpy(vr)[None])[0]
    assert got.shape == want.shape
    assert bool(((got - want).abs() <= 2 * U * want.abs()).all()), float((got - want).abs().max())


# ------------------------------------------------------------------------------------------ refusals
def test_fused_refusals():
    """A non-contiguous ref, raw at an offset that is not 16-byte aligned, and a raw row stride below 384 raise GomError from
    every fused entry (plain, valid ratios, encoder) and from msda_prepare where it applies, before anything is launched:
    the inputs are left as they were and the next valid call gives the usual result."""
    ops = _ops()
    from gomatching_amd.lib import GomError
    shapes, B = [(2, 3), (1, 2), (1, 1), (1, 1)], 2
    ss, lsi, S = _pyr(shapes)
    Lq = S                                                                # (an encoder call: query q = token q)
    raw, _ = _fused_inputs(shapes, B, Lq, 7)
    raw_buf = torch.zeros(B * Lq, 448, device=DEV)
    raw_buf[:, :384] = torch.from_numpy(raw).to(DEV)
    ref_d = ops.encoder_reference_points(ss.to(DEV), lsi.to(DEV), S).repeat(B, 1).contiguous()
    g = torch.Generator().manual_seed(7)
    value = torch.randn(B * S, 256, generator=g).to(DEV)
    vr_d = torch.tensor(VR, dtype=torch.float32, device=DEV)
    a = (ss.to(DEV), lsi.to(DEV), B, Lq)
    kws = ({}, {"valid_ratios": vr_d}, {"encoder_hw0": tuple(shapes[0])})
    good = [ops.msda_fused(raw_buf[:, :384], ref_d, value, S * 256, *a, **kw) for kw in kws]
    snap = raw_buf.clone(), value.clone(), ref_d.clone()
    ref_nc = torch.zeros(B * Lq, 3, device=DEV)
    ref_nc[:, :2] = ref_d
    low = torch.as_strided(raw_buf, (B * Lq, 384), (256, 1))             # row stride 256 < 384
    for kw in kws:
        with pytest.raises(GomError):
            ops.msda_fused(raw_buf[:, :384], ref_nc[:, :2], value, S * 256, *a, **kw)
        with pytest.raises(GomError):
            ops.msda_fused(raw_buf[:, 1:385], ref_d, value, S * 256, *a, **kw)
        with pytest.raises(GomError):
            ops.msda_fused(low, ref_d, value, S * 256, *a, **kw)
    with pytest.raises(GomError):
        ops.msda_prepare(raw_buf[:, :384], ref_nc[:, :2], ss.to(DEV))
    with pytest.raises(GomError):
        ops.msda_prepare(low, ref_d, ss.to(DEV))
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip((raw_buf, value, ref_d), snap))
    for kw, want in zip(kws, good):
        assert torch.equal(ops.msda_fused(raw_buf[:, :384], ref_d, value, S * 256, *a, **kw), want)
