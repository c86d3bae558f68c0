"""The float64 statement of the NHWC convolution every convolution form of the library computes, its componentwise error bound,
and the case table shared by tests/test_conv_statement_cpu.py (no GPU: the statement against torch float64, the declared forms
against ops.conv_plan, the planted mistakes) and tests/test_conv_forms_gpu.py (every case on every back-end).

    y[b, oh, ow, n] = act(scale[n] * sum_{kh, kw, c} x[b, oh*s - p + kh, ow*s - p + kw, c] * w[n, kh, kw, c] + shift[n] + R[b, oh, ow, n])

with zero padding, OH = (H + 2p - KH) // s + 1 (floor), likewise OW, and act = ReLU or the identity.

The bound is the project's f16x3 contract (tests/test_ops_gpu.py, test_gemm_split_epilogue_gather_and_extremes:
2e-6 (|A| |W|) + 1e-7 sum|W|) carried through the epilogue:

    2e-6 (|scale| conv64(|x|, |w|) + |shift| + |R|) + 1e-7 |scale| sum_k |w[n, k]|

per output element; ReLU is 1-Lipschitz, so it holds after the activation too.  The bf16x6 and fp32 back-ends are at least as accurate
and are held to the same bound."""
import functools

import numpy as np

BM, BK = 128, 32                                             # the tile kernel's M tile and k-tile (csrc/gemm_f16x3.hip)


def out_hw(H, W, k, stride, pad):
    return (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1


def _conv(x, w, stride, pad, scale, shift, R, relu, dtype):
    x, w = np.asarray(x, dtype), np.asarray(w, dtype)
    B, H, W, Cin = x.shape
    Cout, KH, KW, Cin2 = w.shape
    assert Cin == Cin2
    OH, OW = (H + 2 * pad - KH) // stride + 1, (W + 2 * pad - KW) // stride + 1
    assert OH > 0 and OW > 0
    xp = np.zeros((B, H + 2 * pad, W + 2 * pad, Cin), dtype)
    xp[:, pad:pad + H, pad:pad + W] = x
    y = np.zeros((B, OH, OW, Cout), dtype)
    for kh in range(KH):
        for kw in range(KW):
            tap = xp[:, kh:kh + (OH - 1) * stride + 1:stride, kw:kw + (OW - 1) * stride + 1:stride]      # [B, OH, OW, Cin]
            y += tap @ w[:, kh, kw].T
    if scale is not None:
        y = y * np.asarray(scale, dtype)
    if shift is not None:
        y = y + np.asarray(shift, dtype)
    if R is not None:
        y = y + np.asarray(R, dtype)
    return np.maximum(y, 0) if relu else y


def conv64(x, w_ohwi, stride, pad, scale=None, shift=None, R=None, relu=False):
    """x [B, H, W, Cin], w [Cout, KH, KW, Cin] -> [B, OH, OW, Cout] float64: one matrix product per (kh, kw) tap of the zero-padded input."""
    return _conv(x, w_ohwi, stride, pad, scale, shift, R, relu, np.float64)


def conv32(x, w_ohwi, stride, pad, scale=None, shift=None, R=None, relu=False):
    """The same loops with every operation rounded to float32 (the exact-integer cases: equal to conv64 bit for bit)."""
    return _conv(x, w_ohwi, stride, pad, scale, shift, R, relu, np.float32)


def conv_bound(x, w_ohwi, stride, pad, scale=None, shift=None, R=None):
    w = np.abs(np.asarray(w_ohwi, np.float64))
    Cout = w.shape[0]
    sc = np.ones(Cout) if scale is None else np.abs(np.asarray(scale, np.float64))
    b = sc * conv64(np.abs(np.asarray(x, np.float64)), w, stride, pad)
    if shift is not None:
        b = b + np.abs(np.asarray(shift, np.float64))
    if R is not None:
        b = b + np.abs(np.asarray(R, np.float64))
    return 2e-6 * b + 1e-7 * sc * w.reshape(Cout, -1).sum(1)


def maxpool64(y):
    """max_pool2d(3, stride 2, padding 1) of [B, H, W, C] float64 (padding never wins: -inf)."""
    B, H, W, C = y.shape
    PH, PW = (H + 2 - 3) // 2 + 1, (W + 2 - 3) // 2 + 1
    yp = np.full((B, H + 2, W + 2, C), -np.inf)
    yp[:, 1:1 + H, 1:1 + W] = y
    out = np.full((B, PH, PW, C), -np.inf)
    for kh in range(3):
        for kw in range(3):
            out = np.maximum(out, yp[:, kh:kh + (PH - 1) * 2 + 1:2, kw:kw + (PW - 1) * 2 + 1:2])
    return out


KINDS = ("f16x3", "bf16x6", "fp32")
# epilogue variants: which of scale / shift the call passes, and the activation
EPILOGUES = {"bn_relu": (True, True, True), "bn": (True, True, False), "bias": (False, True, False), "scale": (True, False, False),
             "relu": (False, False, True), "none": (False, False, False)}


class ConvCase:
    """One convolution call.  `forms`: what ops.conv_plan must return per back-end (with ops.CONV3_PATCH on, as shipped); `ragged`: the
    split-K slices do not divide the k-tiles (the last slice is shorter); `purpose`: the path of the kernel the shape is there for."""

    def __init__(self, purpose, B, H, W, Cin, Cout, k, stride, pad, residual=False, epilogue="bn", splits=0, ragged=False, patch=False):
        assert epilogue in EPILOGUES
        self.purpose, self.B, self.H, self.W, self.Cin, self.Cout = purpose, B, H, W, Cin, Cout
        self.k, self.stride, self.pad, self.residual, self.epilogue = k, stride, pad, residual, epilogue
        self.splits, self.ragged, self.patch = splits, ragged, patch
        self.kinds = ("f16x3",) if patch else KINDS
        self.forms = {"f16x3": ("patch", 0) if patch else ("tile", splits), "bf16x6": ("tile", splits), "fp32": ("fp32", 0)}
        self.OH, self.OW = out_hw(H, W, k, stride, pad)
        self.rows, self.K = B * self.OH * self.OW, k * k * Cin
        self.id = "%dx%dx%d-%dto%d-k%ds%dp%d-%s%s" % (B, H, W, Cin, Cout, k, stride, pad, epilogue, "-R" if residual else "")
        self.seed = 1000003 * B + 10007 * H + 101 * W + 13 * Cin + 7 * Cout + 3 * k + stride

    @property
    def relu(self):
        return EPILOGUES[self.epilogue][2]

    @functools.lru_cache(maxsize=None)
    def inputs(self, exact=False):
        """dict of float32 arrays: x, w, scale | None, shift | None, R | None.
          random  x = 1.5 randn with a quarter of the entries redrawn in (-0.25, 0.25) (|x| < 0.25 in about a third: the second plane's
                  absolute term matters), w rows = randn / sqrt(K) x logspace(-2, 1, Cout), scale in [0.5, 1.5), shift and R randn
          exact   x in {-3 .. 3}, w in {-2 .. 2}, scale in {0.5, 1, 2}, shift and R integers in {-3 .. 3}: every sum is an integer
                  (or a half) below 2^24, so any fp32 evaluation in any order is exact"""
        g = np.random.default_rng(self.seed + (500 if exact else 0))
        xs, ws = (self.B, self.H, self.W, self.Cin), (self.Cout, self.k, self.k, self.Cin)
        ys = (self.B, self.OH, self.OW, self.Cout)
        use_scale, use_shift, _ = EPILOGUES[self.epilogue]
        if exact:
            x, w = g.integers(-3, 4, xs), g.integers(-2, 3, ws)
            scale, shift, R = g.choice([0.5, 1.0, 2.0], self.Cout), g.integers(-3, 4, self.Cout), g.integers(-3, 4, ys)
        else:
            x = 1.5 * g.standard_normal(xs)
            small = g.random(xs) < 0.25
            x = np.where(small, 0.25 * (2 * g.random(xs) - 1), x)
            w = g.standard_normal(ws) / np.sqrt(self.K) * np.logspace(-2, 1, self.Cout).reshape(-1, 1, 1, 1)
            scale, shift, R = g.random(self.Cout) + 0.5, g.standard_normal(self.Cout), g.standard_normal(ys)
        f = lambda a, on: np.ascontiguousarray(a, np.float32) if on else None
        out = {"x": f(x, True), "w": f(w, True), "scale": f(scale, use_scale), "shift": f(shift, use_shift), "R": f(R, self.residual)}
        for v in out.values():
            if v is not None:
                v.setflags(write=False)
        return out

    @functools.lru_cache(maxsize=None)
    def expected(self, exact=False):
        """(conv64, conv_bound) of inputs(exact), computed once and shared (read-only)."""
        i = self.inputs(exact)
        y = conv64(i["x"], i["w"], self.stride, self.pad, i["scale"], i["shift"], i["R"], self.relu)
        b = conv_bound(i["x"], i["w"], self.stride, self.pad, i["scale"], i["shift"], i["R"])
        y.setflags(write=False)
        b.setflags(write=False)
        return y, b


def _cases():
    C = ConvCase
    tile = [
        C("3x3/1: one M tile spanning both images, K tail (144 = 4.5 k-tiles), BN = 64 with a column tail", 2, 5, 7, 16, 40, 3, 1, 1,
          residual=True, epilogue="bn_relu"),
        C("scalar epilogue (Cout % 4 != 0), one column group", 2, 9, 12, 128, 6, 3, 2, 1, epilogue="bn_relu"),
        C("scalar epilogue (Cout % 4 != 0) with residual", 2, 9, 12, 32, 38, 3, 1, 1, residual=True, epilogue="bn"),
        C("three M tiles with a row tail (297 rows)", 3, 9, 11, 32, 38, 3, 1, 1, residual=True, epilogue="bias"),
        C("3x3/2 at even x odd size, two column tiles with a tail", 2, 6, 9, 64, 136, 3, 2, 1, epilogue="none"),
        C("3x3/2 at odd x even size, two column tiles with a tail", 2, 7, 8, 64, 136, 3, 2, 1, epilogue="none"),
        C("1x1/2 shortcut form at odd sizes", 2, 5, 6, 32, 64, 1, 2, 0, epilogue="bn"),
        C("1x1/2 shortcut form on the one-pixel image", 1, 1, 1, 32, 64, 1, 2, 0, epilogue="scale"),
        C("7x7/2, K = 196 = 6 k-tiles + 4: border outputs and four whose window lies inside the image", 1, 9, 11, 4, 64, 7, 2, 3,
          epilogue="bn_relu"),
        C("7x7/2, every output touching padding (H = 7: no window fits)", 1, 7, 11, 4, 64, 7, 2, 3, epilogue="bn"),
        C("input smaller than the kernel (output 2 x 1)", 2, 3, 2, 4, 64, 7, 2, 3, epilogue="bn_relu"),
        C("H = 1", 1, 1, 9, 16, 64, 3, 1, 1, epilogue="bias"),
        C("W = 1", 1, 9, 1, 16, 64, 3, 2, 1, epilogue="relu"),
        C("split-K, exact slices (9 x 16 k-tiles)", 2, 6, 9, 512, 256, 3, 2, 1, epilogue="bias", splits=9),
        C("split-K, ragged last slice, small M (98 k-tiles: 6 slices of 17, the last 13)", 1, 9, 11, 64, 64, 7, 2, 3, epilogue="bn_relu",
          splits=6, ragged=True),
        C("split-K, ragged, many tiles, residual (68 tiles; 144 k-tiles: 7 slices of 21, the last 18)", 1, 65, 66, 512, 256, 3, 1, 1,
          residual=True, epilogue="bn_relu", splits=7, ragged=True),
        C("pointwise on the GEMM tile form", 2, 5, 7, 64, 136, 1, 1, 0, residual=True, epilogue="bn_relu"),
    ]
    patch = []
    for Cin in (64, 128):                                    # one and two resident 64-channel chunks
        for n, (B, H, W) in enumerate([(1, 1, 1), (1, 1, 33), (2, 9, 17), (1, 8, 16)]):      # 8 x 16 tile: below, past, one past, exactly
            patch.append(C("patch kernel at and around its 8 x 16 tile", B, H, W, Cin, 64, 3, 1, 1, patch=True,
                           epilogue=("bn_relu", "bn", "none", "bias")[(n + Cin // 64) % 4]))
    return tile + patch


CASES = _cases()
TILE_CASES = [c for c in CASES if not c.patch]
PATCH_CASES = [c for c in CASES if c.patch]
SPLITK_CASES = [c for c in CASES if c.splits > 1]
IDS = [c.id for c in CASES]
assert len(set(IDS)) == len(IDS)


def case(case_id):
    return CASES[IDS.index(case_id)]


def worst(got, exp, bound):
    """(largest |got - exp| / bound, its index) -- what a failing test prints."""
    r = np.abs(np.asarray(got, np.float64) - exp) / bound
    r = np.where(np.isnan(r), np.inf, r)
    at = np.unravel_index(int(r.argmax()), r.shape)
    return float(r[at]), tuple(int(v) for v in at)
