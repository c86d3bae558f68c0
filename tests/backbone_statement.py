"""The float64 statements of the Swin / ViTAEv2 backbone kernels (csrc/swin.hip, csrc/vitae.hip, csrc/attn_flash.hip, the GELU
epilogue of csrc/gemm_f16x3.hip), their element-wise error bounds, the input generators and the case tables shared by
tests/test_backbone_statement_cpu.py (no GPU: the statements against independent evaluations, fp32 / two-plane emulations inside
the bounds, the planted mistakes outside them) and tests/test_backbone_forms_gpu.py (every case through the ops entry points).
Torch on the CPU and numpy only; the same seeds give the same bits in both files.

Every statement is written from the reference model's definition (padding, roll, reshape, permute as the modules do:
swin_transformer.py PatchEmbed / SwinTransformerBlock / PatchMerging / WindowAttention, vitae_v2 ReductionCell / NormalCell /
window.py / token_transformer.py), never from a kernel's index arithmetic.

Bounds.  U = 2^-24 (half an fp32 ulp, relative).  Library functions are taken at the accuracy the OpenCL / HIP device-library
specification grants them: expf 3 ulp, erff 16 ulp, 1 ulp = 2 U relative.  The f16x3 contract is the project's
(tests/conv_statement.py): a product of K terms whose activation operand A is split into two fp16 planes as it is and whose weight
operand W is row-scaled first errs by at most 2e-6 (|A| |W|) + 1e-7 sum |W| (the second term: an activation below 2^-14 x 2^11
keeps an ABSOLUTE error of up to 2^-25 in its low plane).  Nothing in any bound was measured on a GPU."""
import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

from conv_statement import conv64, worst  # noqa: F401  (worst: what a failing test prints)
from helpers import ATTN_U, attn_inputs

U = ATTN_U
WS, WT = 7, 49
EXP_ULP, ERF_ULP = 3, 16                                     # specification accuracy of expf / erff in ulp
TINY = 2.0 ** -149                                           # one fp32 subnormal step: an output may be flushed or rounded there


def ceil_to(n, m):
    return -(-n // m) * m


def codes(shape, base=1):
    """A distinct exactly representable value per element: base + flat index, below 2^24."""
    n = int(np.prod(shape))
    assert base + n < 2 ** 24
    return (torch.arange(n, dtype=torch.float64) + base).float().reshape(shape)


def ro(*ts):
    for t in ts:
        if isinstance(t, np.ndarray):
            t.setflags(write=False)
    return ts if len(ts) > 1 else ts[0]


# =========================================================================================== data movement (bit-exact)
def swin_patchify_st(img):
    """PatchEmbed (swin_transformer.py:475-478 + the 4x4 / 4 projection's receptive field): [B,H,W,4] -> [B*Hp*Wp, 64], zero padding
    right / bottom to multiples of 4, a patch's 64 values in (kh, kw, c) order."""
    B, H, W, _ = img.shape
    x = F.pad(img.permute(0, 3, 1, 2), (0, (-W) % 4, 0, (-H) % 4))
    Hp, Wp = x.shape[2] // 4, x.shape[3] // 4
    return x.reshape(B, 4, Hp, 4, Wp, 4).permute(0, 2, 4, 3, 5, 1).reshape(B * Hp * Wp, 64)


def swin_window_gather_st(x, shift):
    """SwinTransformerBlock.forward :246-262: pad right / bottom to multiples of 7, roll by -shift, window partition.
    x [B,H,W,C] -> [B*nW*49, C]."""
    B, H, W, C = x.shape
    x = F.pad(x, (0, 0, 0, (-W) % WS, 0, (-H) % WS))
    Hp, Wp = x.shape[1], x.shape[2]
    if shift > 0:
        x = torch.roll(x, shifts=(-shift, -shift), dims=(1, 2))
    return x.view(B, Hp // WS, WS, Wp // WS, WS, C).permute(0, 1, 3, 2, 4, 5).reshape(-1, C)


def swin_window_scatter_add_st(win, shortcut, shift):
    """:264-279: window reverse, roll by +shift, crop, shortcut + x (one fp32 addition).  win [B*nW*49, C], shortcut [B,H,W,C]."""
    B, H, W, C = shortcut.shape
    Hp, Wp = ceil_to(H, WS), ceil_to(W, WS)
    x = win.view(B, Hp // WS, Wp // WS, WS, WS, C).permute(0, 1, 3, 2, 4, 5).reshape(B, Hp, Wp, C)
    if shift > 0:
        x = torch.roll(x, shifts=(shift, shift), dims=(1, 2))
    return shortcut + x[:, :H, :W]


def swin_patch_merge_st(x):
    """PatchMerging.forward :320-327: [B,H,W,C] -> [B*H2*W2, 4C]."""
    B, H, W, C = x.shape
    x = F.pad(x, (0, 0, 0, W % 2, 0, H % 2))
    x = torch.cat([x[:, 0::2, 0::2], x[:, 1::2, 0::2], x[:, 0::2, 1::2], x[:, 1::2, 1::2]], -1)
    return x.reshape(-1, 4 * C)


def vitae_pads(H, W):
    td, lr = (WS - H % WS) % WS, (WS - W % WS) % WS
    return td // 2, td - td // 2, lr // 2, lr - lr // 2        # top, bottom, left, right


def vitae_window_gather_st(x):
    """ReductionCell.py:147-156 / NormalCell.py:160-165: zero padding split top / bottom and left / right (the smaller half first),
    window partition.  x [B,H,W,C] -> [B*nW*49, C]."""
    B, H, W, C = x.shape
    top, bot, left, right = vitae_pads(H, W)
    x = F.pad(x.permute(0, 3, 1, 2), (left, right, top, bot)).permute(0, 2, 3, 1)
    Hp, Wp = x.shape[1], x.shape[2]
    return x.reshape(B, Hp // WS, WS, Wp // WS, WS, C).permute(0, 1, 3, 2, 4, 5).reshape(-1, C)


def vitae_window_crop_st(win, B, H, W, R1=None, R2=None):
    """Window reverse and crop; the sums are fp32 (win + R1) + R2.  win [B*nW*49, C] -> [B*H*W, C]."""
    C = win.shape[-1]
    top, bot, left, right = vitae_pads(H, W)
    Hp, Wp = H + top + bot, W + left + right
    y = win.view(B, Hp // WS, Wp // WS, WS, WS, C).permute(0, 1, 3, 2, 4, 5).reshape(B, Hp, Wp, C)
    y = y[:, top:top + H, left:left + W].reshape(B * H * W, C)
    if R1 is not None:
        y = y + R1
    if R2 is not None:
        y = y + R2
    return y


def im2col_st(x, k, stride, pad, dil, ldo):
    """The receptive fields of conv2d(kernel k, stride, padding pad, dilation dil) as rows in (kh, kw, c) order, zero beyond
    k*k*C: one strided slice of the zero-padded map per tap.  x [B,H,W,C] -> ([B*OH*OW, ldo], OH, OW)."""
    B, H, W, C = x.shape
    OH, OW = (H + 2 * pad - dil * (k - 1) - 1) // stride + 1, (W + 2 * pad - dil * (k - 1) - 1) // stride + 1
    xp = F.pad(x, (0, 0, pad, pad, pad, pad))
    out = torch.zeros(B, OH, OW, ldo, dtype=x.dtype)
    for kh in range(k):
        for kw in range(k):
            y0, x0 = kh * dil, kw * dil
            out[..., (kh * k + kw) * C:(kh * k + kw + 1) * C] = xp[:, y0:y0 + (OH - 1) * stride + 1:stride, x0:x0 + (OW - 1) * stride + 1:stride]
    return out.reshape(-1, ldo), OH, OW


class Move:
    def __init__(self, op, **kw):
        self.op = op
        self.__dict__.update(kw)
        self.id = op + "-" + "-".join("%s%s" % (k, "x".join(map(str, v)) if isinstance(v, tuple) else v) for k, v in kw.items())


def _thin_window_cases():
    """shift x (H, W) x B x C thinned to 39 cases: every (H, W) with every shift, B and C cycling so that every value of every axis
    occurs, then further combinations of the sizes where padding, wrap and shift interact."""
    out, n = [], 0
    hw = [(1, 1), (5, 3), (7, 7), (14, 7), (6, 8), (12, 17), (8, 50)]
    for i, (H, W) in enumerate(hw):
        for j, shift in enumerate((0, 1, 3, 6)):
            out.append(dict(H=H, W=W, shift=shift, B=(1, 3)[(i + j) % 2], C=(4, 96, 100)[n % 3]))
            n += 1
    for (H, W), shift, B, C in (((7, 7), 3, 3, 4), ((14, 7), 6, 1, 100), ((8, 50), 1, 3, 96), ((1, 1), 6, 3, 100), ((12, 17), 3, 3, 96),
                                ((12, 17), 0, 1, 100), ((5, 3), 1, 3, 4), ((6, 8), 6, 1, 96), ((12, 17), 6, 3, 4), ((6, 8), 3, 3, 100),
                                ((14, 7), 1, 3, 4), ((8, 50), 3, 1, 100), ((5, 3), 3, 1, 96), ((7, 7), 1, 1, 100)):
        if dict(H=H, W=W, shift=shift, B=B, C=C) not in out:
            out.append(dict(H=H, W=W, shift=shift, B=B, C=C))
    return out


VITAE_HW = [(1, 1), (7, 7), (8, 8), (13, 6), (12, 16), (24, 32)]
MOVE_CASES = (
    [Move("swin_patchify", B=B, H=H, W=W) for B, H, W in ((1, 1, 1), (2, 4, 4), (1, 5, 8), (3, 7, 3), (2, 10, 13))]
    + [Move("swin_window_gather", **c) for c in _thin_window_cases()]
    + [Move("swin_window_scatter_add", **c) for c in _thin_window_cases()]
    + [Move("swin_patch_merge", B=2, H=H, W=W, C=(8 if (H + W) % 2 else 100)) for H, W in ((1, 1), (2, 2), (3, 5), (6, 8), (12, 17))]
    + [Move("vitae_window_gather", B=(2 if n % 2 else 1), H=H, W=W, C=(64, 4, 128)[n % 3]) for n, (H, W) in enumerate(VITAE_HW)]
    + [Move("vitae_window_crop", B=(2 if n % 2 else 1), H=H, W=W, C=(64, 4, 128)[n % 3], add=add) for n, (H, W) in enumerate(VITAE_HW)
       for add in ("none", "R1", "R2", "both")]
    + [Move("im2col", B=2, H=H, W=W, C=C, k=k, s=s, d=d, ldo=ldo) for (C, k, s, dils, H, W) in ((4, 7, 4, (1, 2, 3, 4), 9, 14),
                                                                                           (64, 3, 2, (1, 2, 3), 5, 8))
       for d in dils for ldo in sorted({k * k * C, ceil_to(k * k * C, 32)})]
    + [Move("im2col", B=2, H=4, W=4, C=4, k=7, s=4, d=4, ldo=224),                    # dilated window (25) larger than the map
       Move("im2col", B=2, H=3, W=9, C=4, k=7, s=4, d=1, ldo=196),                    # OH == 1
       Move("im2col", B=1, H=2, W=5, C=64, k=3, s=2, d=3, ldo=576)]                    # OH == 1, every tap row but one in padding
    + [Move("transpose_into", rows=r, cols=c) for r, c in ((1, 1), (31, 33), (32, 32), (50, 64), (65, 128))])
MOVE_IDS = [c.id for c in MOVE_CASES]
assert len(set(MOVE_IDS)) == len(MOVE_IDS)


def im2col_pad(k, s, d):
    return math.ceil(((k - 1) * d + 1 - s) / 2)              # ReductionCell.py:27-34


@functools.lru_cache(maxsize=None)
def move_io(case_id):
    """(inputs dict of float32 CPU tensors, expected float32 tensor) of one movement case; every input element is a distinct code."""
    c = MOVE_CASES[MOVE_IDS.index(case_id)]
    if c.op == "swin_patchify":
        img = codes((c.B, c.H, c.W, 4))
        return {"img": img}, swin_patchify_st(img)
    if c.op == "swin_window_gather":
        x = codes((c.B, c.H, c.W, c.C))
        return {"x": x}, swin_window_gather_st(x, c.shift)
    if c.op == "swin_window_scatter_add":
        sc = codes((c.B, c.H, c.W, c.C), base=2 ** 22)
        Hp, Wp = ceil_to(c.H, WS), ceil_to(c.W, WS)
        win = codes((c.B * Hp * Wp, c.C))
        exp = swin_window_scatter_add_st(win, sc, c.shift)
        # the window rows of padded positions (where the gather of an all-ones map finds padding) hold NaN: they must not be read
        padded = swin_window_gather_st(torch.ones(c.B, c.H, c.W, 1), c.shift)[:, 0] == 0
        win = win.clone()
        win[padded] = float("nan")
        assert bool(torch.equal(exp, swin_window_scatter_add_st(torch.nan_to_num(win, nan=-7.0), sc, c.shift)))
        return {"win": win, "shortcut": sc}, exp
    if c.op == "swin_patch_merge":
        x = codes((c.B, c.H, c.W, c.C))
        return {"x": x}, swin_patch_merge_st(x)
    if c.op == "vitae_window_gather":
        x = codes((c.B, c.H, c.W, c.C))
        return {"x": x}, vitae_window_gather_st(x)
    if c.op == "vitae_window_crop":
        Hp, Wp = ceil_to(c.H, WS), ceil_to(c.W, WS)
        win = codes((c.B * Hp * Wp, c.C))
        n = c.B * c.H * c.W
        R1 = codes((n, c.C), base=2 ** 21) if c.add in ("R1", "both") else None
        R2 = codes((n, c.C), base=2 ** 22) if c.add in ("R2", "both") else None
        return {"win": win, "R1": R1, "R2": R2}, vitae_window_crop_st(win, c.B, c.H, c.W, R1, R2)
    if c.op == "im2col":
        x = codes((c.B, c.H, c.W, c.C))
        return {"x": x}, im2col_st(x, c.k, c.s, im2col_pad(c.k, c.s, c.d), c.d, c.ldo)[0]
    assert c.op == "transpose_into"
    wide = codes((c.rows, c.cols + 12))                       # the source is the column slice [4, 4 + cols) of this
    return {"wide": wide, "col0": 4}, wide[:, 4:4 + c.cols].t().contiguous()


def move_case(case_id):
    return MOVE_CASES[MOVE_IDS.index(case_id)]


# =========================================================================================== gelu_ / silu_
ACT_N = (4, 1020, 1024, 1028)                                 # 1028: one quad beyond a workgroup of 256 quads
ACT_SPECIALS = (0.0, 1e-30, 20.0, 88.0, 104.0, 1e4)


def act_inputs(n):
    """A dense grid over [-12, 12] with +-0, +-1e-30, +-20, +-88, +-104, +-1e4 at its front (n = 4: the first four of them)."""
    sp = [s * v for v in ACT_SPECIALS for s in (1.0, -1.0)]
    x = np.concatenate([np.array(sp[4:8] + sp[:4] + sp[8:]), np.linspace(-12.0, 12.0, max(n - len(sp), 0))])[:n]
    return ro(x.astype(np.float32))


def gelu64(x):
    """nn.GELU (exact): x Phi(x) = x erfc(-x / sqrt 2) / 2 in float64 (erfc: no cancellation in the left tail)."""
    x = torch.as_tensor(np.asarray(x, np.float64))
    return (0.5 * x * torch.special.erfc(-x / math.sqrt(2.0))).numpy()


def silu64(x):
    x = np.asarray(x, np.float64)
    with np.errstate(over="ignore"):
        return x / (1.0 + np.exp(-x))


def gelu_bound(x):
    """0.5f * x * (1.f + erff(x * 0.70710678f)).  t = x c: the constant's and the product's rounding move erf's argument by at most
    2 U |t|, and |t erf'(t)| <= 0.484, so erf moves by at most U; erff itself errs by ERF_ULP ulp <= 2 ERF_ULP U |erf| <= 2 ERF_ULP U.
    These are ABSOLUTE errors of 1 + erf (the cancellation for x < 0: 1 + erf may be as small as it likes), times |x| / 2.  The sum
    1 + e and the two products round once each: 3 U |y|, or 3 U (|x| U) where 1 + erf has fallen below U and the result is 0.
        bound = 3 U max(|y|, |x| U) + 0.5 |x| (2 ERF_ULP + 1) U + 2^-149"""
    x = np.asarray(x, np.float64)
    return 3 * U * np.maximum(np.abs(gelu64(x)), np.abs(x) * U) + 0.5 * np.abs(x) * (2 * ERF_ULP + 1) * U + TINY


def silu_bound(x, y=None):
    """v / (1.f + expf(-v)): expf EXP_ULP ulp = 2 EXP_ULP U relative on e / (1 + e) <= 1 of the result, the sum 1 U, the division
    2.5 ulp = 5 U where it is not correctly rounded: c = 2 EXP_ULP + 6 = 12.
        bound = c U max(|y|, |x| U) + 2^-149     (|x| U: expf(-v) overflowed or 1 + e lost it, the result is a signed zero)"""
    x = np.asarray(x, np.float64)
    y = silu64(x) if y is None else y
    return (2 * EXP_ULP + 6) * U * np.maximum(np.abs(y), np.abs(x) * U) + TINY


# =========================================================================================== grouped 3x3 convolution
class GConv:
    def __init__(self, Cin, Cout, groups, stride, H, W, scale, silu, R):
        self.Cin, self.Cout, self.groups, self.stride, self.H, self.W = Cin, Cout, groups, stride, H, W
        self.scale, self.silu, self.R, self.B = scale, silu, R, 2
        self.CG, self.cout_g = Cin // groups, Cout // groups
        self.OH, self.OW = (H - 1) // stride + 1, (W - 1) // stride + 1
        self.id = "cg%d-og%d-g%d-s%d-%dx%d-%s%s%s" % (self.CG, self.cout_g, groups, stride, H, W, "sc" if scale else "nosc",
                                                    "-silu" if silu else "", "-R" if R else "")
        self.seed = 7919 * Cin + 104729 * Cout + 31 * groups + 5 * stride + 1009 * H + 13 * W + 2 * scale + 4 * silu + 8 * R

    @functools.lru_cache(maxsize=None)
    def inputs(self):
        """x [B,H,W,Cin], w [Cout,3,3,CG] (group of output channel co = co // cout_g, nn.Conv2d's), scale | None, shift, R | None."""
        g = np.random.default_rng(self.seed)
        f = lambda a: ro(np.ascontiguousarray(a, np.float32))
        x = f(1.5 * g.standard_normal((self.B, self.H, self.W, self.Cin)))
        w = f(g.standard_normal((self.Cout, 3, 3, self.CG)) / np.sqrt(9 * self.CG) * np.logspace(-1, 1, self.Cout).reshape(-1, 1, 1, 1))
        return {"x": x, "w": w, "scale": f(g.random(self.Cout) + 0.5) if self.scale else None, "shift": f(g.standard_normal(self.Cout)),
                "R": f(g.standard_normal((self.B, self.OH, self.OW, self.Cout))) if self.R else None}

    @functools.lru_cache(maxsize=None)
    def expected(self):
        i = self.inputs()
        return ro(*grouped_conv64(i["x"], i["w"], i["scale"], i["shift"], i["R"], self.groups, self.stride, self.silu))


def grouped_conv64(x, w, scale, shift, R, groups, stride, silu):
    """act(conv * scale + shift) + R with nn.Conv2d(groups)'s channel rule: output channels [g cout_g, (g + 1) cout_g) see input
    channels [g CG, (g + 1) CG): conv_statement.conv64 per group.  -> (exp, bound) float64 [B,OH,OW,Cout].

    bound: a pure fmaf chain of n = 9 CG terms errs by n U conv(|x|, |w|); the scale, the shift (two roundings, or one fma) carry
    it to (n + 2) U (|scale| conv(|x|, |w|) + |shift|); SiLU's slope lies in [-0.1, 1.1] and its own evaluation adds silu_bound; the
    addition of R rounds once more."""
    x64, w64 = np.asarray(x, np.float64), np.asarray(w, np.float64)
    Cout, CG = w64.shape[0], w64.shape[3]
    cout_g = Cout // groups
    acc, mag = [], []
    for g in range(groups):
        xs, wg = x64[..., g * CG:(g + 1) * CG], w64[g * cout_g:(g + 1) * cout_g]
        acc.append(conv64(xs, wg, stride, 1))
        mag.append(conv64(np.abs(xs), np.abs(wg), stride, 1))
    acc, mag = np.concatenate(acc, -1), np.concatenate(mag, -1)
    sc = np.ones(Cout) if scale is None else np.asarray(scale, np.float64)
    sh = np.asarray(shift, np.float64)
    v = acc * sc + sh
    bound = 1.1 * (9 * CG + 2) * U * (np.abs(sc) * mag + np.abs(sh))
    y = v
    if silu:
        y = silu64(v)
        bound = bound + silu_bound(v, y)
    if R is not None:
        y = y + np.asarray(R, np.float64)
    return y, bound + U * np.abs(y) + TINY


def _gconv_cases():
    """(Cin, Cout, groups): CG 4 and 16 with cout_g 1, 4 and 16; both strides; every (H, W) with every CG and stride; the scale and
    the three activation / addend forms cycle.  Output counts B OH OW Cout: no multiple of 256 wherever the issue's sizes allow it
    (cout_g = 16 at 7 x 8 gives 112 x 16 k = 256 x 7 k for any group count; its other maps give 192 k and 960 k / 2) -- asserted below
    per (CG, stride): a count past one workgroup that is no multiple of 256."""
    chan = [(24, 6, 6), (24, 24, 6), (8, 32, 2), (48, 3, 3), (48, 12, 3), (32, 32, 2)]       # CG 4: og 1, 4, 16; CG 16: og 1, 4, 16
    forms = [(True, False), (False, True), (True, True)]                                       # (silu, R)
    out, n = [], 0
    for ci, (Cin, Cout, groups) in enumerate(chan):
        for stride in (1, 2):
            for hi, (H, W) in enumerate(((1, 1), (2, 3), (5, 3), (7, 8))):
                if (ci + hi + stride) % 2 and (H, W) not in ((7, 8),):     # thin: half of the small maps per channel triple and stride
                    continue
                silu, R = forms[n % 3]
                out.append(GConv(Cin, Cout, groups, stride, H, W, scale=bool((n // 3) % 2 == 0), silu=silu, R=R))
                n += 1
    return out


GCONV_CASES = _gconv_cases()
GCONV_IDS = [c.id for c in GCONV_CASES]
assert len(set(GCONV_IDS)) == len(GCONV_IDS)
for _cg in (4, 16):
    for _s in (1, 2):
        _n = [c.B * c.OH * c.OW * c.Cout for c in GCONV_CASES if c.CG == _cg and c.stride == _s]
        assert any(n > 256 and n % 256 for n in _n) and {c.cout_g for c in GCONV_CASES if c.CG == _cg} == {1, 4, 16}


# =========================================================================================== window attention
def window_attention64(q, k, v, hd, add=None):
    """helpers.attention64 with an additive logit term: q, k, v [..., 49, hd] float32, add [..., 49, 49] float32 (bias of the head +
    mask of the window, the sum of the two taken in float64) or None -> (exp, bound) float64.

        qs = fp32(q * fp32(1 / sqrt(hd))) widened;  s = qs k^T + add;  p = softmax(s);  exp = p v          all float64

    The logit of key j errs by e_ij = (hd + 5) U (sum_d |qs_id k_jd| + |add_ij|): the fmaf chain of hd terms and the pre-scale as in
    attention64, and the three additions that join the two half chains, the bias and the mask, each rounding a value no larger
    than sum |qs k| + |add|.  To first order p_j moves by p_j (e_j - sum_l p_l e_l): the error enters each weight once directly and
    once through the normaliser, weighted by the weights themselves -- so a key masked by -100 costs what its weight is, nothing.

        bound[i,d] = sum_j p_ij |v_jd| (e_ij + sum_l p_il e_il + (|s_ij - m_i| + 2 Lk + 16) U) + Lk 2^-126 max|v|

    (the remaining terms as attention64 states them)."""
    q, k, v = torch.as_tensor(q), torch.as_tensor(k), torch.as_tensor(v)
    assert q.dtype == k.dtype == v.dtype == torch.float32
    Lk = k.shape[-2]
    qs = (q * torch.tensor(1.0 / np.sqrt(hd), dtype=torch.float32)).double()
    k64, va = k.double(), v.double().abs()
    s = qs @ k64.transpose(-1, -2)
    mag = qs.abs() @ k64.abs().transpose(-1, -2)
    if add is not None:
        a64 = torch.as_tensor(add).double()
        s, mag = s + a64, mag + a64.abs()
    d = s - s.max(-1, keepdim=True).values
    e = torch.exp(d)
    p = e / e.sum(-1, keepdim=True)
    exp = p @ v.double()
    el = (hd + 5) * U * mag
    w = p * (el + (p * el).sum(-1, keepdim=True) + U * (d.abs() + 2 * Lk + 16))
    bound = w @ va + Lk * 2.0 ** -126 * va.amax((-1, -2), keepdim=True)
    return exp, bound


WIN_KINDS = ("randn", "peaked", "overflow", "same", "widev", "edge", "masked")


class WinCase:
    """One window-attention call: `images` x `nW` windows of 49 tokens, `heads` heads of `hd`.  Swin form (hd 32): bias [heads,49,49]
    always, mask [nW,49,49] for kind "masked"."""

    def __init__(self, form, images, nW, heads, hd):
        self.form, self.images, self.nW, self.heads, self.hd = form, images, nW, heads, hd
        self.windows, self.C = images * nW, heads * hd
        self.kinds = WIN_KINDS if form == "swin" else WIN_KINDS[:-1]
        self.id = "%s-i%d-w%d-h%d-hd%d" % (form, images, nW, heads, hd)

    @functools.lru_cache(maxsize=None)
    def inputs(self, kind):
        """-> (q, k, v [windows, heads, 49, hd], bias | None, mask | None)."""
        seed = 77 * WIN_KINDS.index(kind) + 1000 * self.windows + 10 * self.heads + self.hd
        q, k, v = attn_inputs("randn" if kind == "masked" else kind, self.windows, self.heads, self.hd, WT, WT, seed)
        if self.form != "swin":
            return q, k, v, None, None
        g = torch.Generator().manual_seed(seed + 5)
        bias = torch.randn(self.heads, WT, WT, generator=g) + torch.arange(self.heads).view(-1, 1, 1).float()      # distinct per head
        mask = None
        if kind == "masked":
            # window w of an image lets token i see the tokens of its own block of w + 1 consecutive tokens: window 0 leaves a row
            # only its own key, and no two windows of an image share a mask
            t = torch.arange(WT)
            mask = torch.stack([torch.where((t.view(-1, 1) // (w + 1)) == (t.view(1, -1) // (w + 1)), 0.0, -100.0) for w in range(self.nW)])
        return q, k, v, bias, mask

    def add(self, kind):
        """[windows, heads, 49, 49] float64 additive term, or None."""
        _, _, _, bias, mask = self.inputs(kind)
        if bias is None:
            return None
        a = bias.double().view(1, self.heads, WT, WT).expand(self.windows, -1, -1, -1)
        if mask is not None:
            a = a + mask.double().repeat(self.images, 1, 1).view(self.windows, 1, WT, WT)       # window b of an image: mask[b % nW]
        return a

    @functools.lru_cache(maxsize=None)
    def expected(self, kind):
        q, k, v, _, _ = self.inputs(kind)
        return window_attention64(q, k, v, self.hd, self.add(kind))

    def qkv(self, kind):
        """The packed [windows * 49, 3 C] rows the op reads: q | k | v, heads contiguous inside each."""
        q, k, v, _, _ = self.inputs(kind)
        return pack_qkv(q, k, v)


def pack_qkv(q, k, v):
    """[nb, heads, L, hd] x 3 -> [nb * L, 3 * heads * hd]."""
    nb, heads, L, hd = q.shape
    return torch.stack([t.permute(0, 2, 1, 3).reshape(nb * L, heads * hd) for t in (q, k, v)], 1).reshape(nb * L, 3 * heads * hd)


def unpack_out(out, nb, heads, L, hd):
    """[nb * L, heads * hd] -> [nb, heads, L, hd]."""
    return torch.as_tensor(out).reshape(nb, L, heads, hd).permute(0, 2, 1, 3)


WIN_CASES = ([WinCase("swin", i, w, h, 32) for i, w, h in ((1, 1, 1), (1, 1, 3), (1, 2, 3), (3, 1, 6), (1, 5, 3), (3, 2, 3), (2, 6, 12))]
             + [WinCase("vitae", 1, w, h, hd) for h, hd in ((1, 64), (2, 64), (4, 64), (1, 128), (2, 128)) for w in (1, 3)])
assert sorted({(c.windows * c.heads) % 4 for c in WIN_CASES if c.form == "swin"}) == [0, 1, 2, 3]


# =========================================================================================== softmax_rows_scaled_
SOFTMAX_KINDS = ("randn", "big", "const", "low")
SOFTMAX_CASES = [(rows, cols) for cols in (1, 255, 256, 257, 8191, 8192) for rows in (1, 3)]
SOFTMAX_SCALE = 0.088388346                                    # 128^-0.5 as a Python float: not a power of two


@functools.lru_cache(maxsize=None)
def softmax_inputs(rows, cols, kind):
    """randn x 3 | logits up to +-300 after the scale | one constant per row | randn with one entry per row 1e6 below the rest."""
    g = np.random.default_rng(100 * cols + 10 * rows + SOFTMAX_KINDS.index(kind))
    x = 3 * g.standard_normal((rows, cols))
    if kind == "big":
        x = g.uniform(-300, 300, (rows, cols)) / SOFTMAX_SCALE
    elif kind == "const":
        x = np.repeat(g.standard_normal((rows, 1)) * 50, cols, 1)
    elif kind == "low":
        x[np.arange(rows), g.integers(0, cols, rows)] = -1e6
    return ro(x.astype(np.float32))


def softmax64(x, scale):
    """softmax(x * scale) over rows, float64, with its bound.  scale is the fp32 value the kernel receives.  The fp32 product
    x * scale moves logit j by U |s_j| (enters p_j directly and through the normaliser, as in window_attention64); expf's argument
    rounds (|s_j - m| U); 64: the 32 sequential additions of a lane's terms, the wave butterfly, the four partial sums, expf, the
    reciprocal and the product.  -> (p, bound)."""
    s = np.asarray(x, np.float64) * float(np.float32(scale))
    d = s - s.max(1, keepdims=True)
    e = np.exp(d)
    p = e / e.sum(1, keepdims=True)
    el = U * np.abs(s)
    return p, p * (el + (p * el).sum(1, keepdims=True) + U * (np.abs(d) + 64)) + 2.0 ** -126


# =========================================================================================== flash attention / fallback path
FLASH_KINDS = ("randn", "peaked", "overflow", "same", "edge", "ties", "tiny", "widev4")
FLASH_KT = 64                                                  # keys per staged tile (csrc/attn_flash.hip)


def _ties(rng, shape, e_lo, e_hi):
    """Values exactly half-way between two fp16 numbers (tests/test_vitae_gpu.py, test_flash_attention_operands_on_rounding_ties)."""
    e = rng.integers(e_lo, e_hi, size=shape).astype(np.float64)
    ulp = 2.0 ** (e - 10)
    return ((2.0 ** e + rng.integers(0, 1024, size=shape) * ulp + 0.5 * ulp) * rng.choice([-1.0, 1.0], size=shape)).astype(np.float32)


class FlashCase:
    def __init__(self, N, heads, hd, B):
        self.N, self.heads, self.hd, self.B = N, heads, hd, B
        self.id = "n%d-h%dx%d-b%d" % (N, heads, hd, B)

    @functools.lru_cache(maxsize=None)
    def inputs(self, kind):
        """q, k, v [B, heads, N, hd] float32.  Beyond helpers.attn_inputs: `ties` (operands on fp16 rounding ties), `tiny`
        (randn x 1e-6: both fp16 planes subnormal), `widev4` (v x e^U(-4, 4))."""
        seed = 1000 * FLASH_KINDS.index(kind) + 7 * self.N + self.hd + 3 * self.heads + self.B
        shape = (self.B, self.heads, self.N, self.hd)
        if kind == "ties":
            rng = np.random.default_rng(seed)
            return tuple(torch.from_numpy(_ties(rng, shape, lo, hi)) for lo, hi in ((-4, -1), (-3, 1), (-6, 2)))
        q, k, v = attn_inputs(kind if kind in ("peaked", "overflow", "same", "edge") else "randn", self.B, self.heads, self.hd,
                              self.N, self.N, seed)
        if kind == "tiny":
            q, k, v = q * 1e-6, k * 1e-6, v * 1e-6
        elif kind == "widev4":
            v = v * torch.exp(torch.rand(shape, generator=torch.Generator().manual_seed(seed + 1)) * 8 - 4)
        return q, k, v

    @functools.lru_cache(maxsize=None)
    def expected(self, kind):
        return flash64(*self.inputs(kind), self.hd)


def flash64(q, k, v, hd):
    """s = (q k^T) * scale with scale = fp32(1 / sqrt(hd)) applied AFTER the product (token_transformer.py:33, NormalCell.py:52; the
    kernel and the GEMM pair order it so), p = softmax(s), exp = p v, float64.  q, k, v [..., N, hd] float32 -> (exp, bound).

    Bound.  Both products run on fp16 planes under the f16x3 contract.  In the first neither operand is row-scaled (the fused kernel
    splits q and k as they are; the GEMM pair scales k's rows, which only helps), so the contract's absolute term applies to both:
        E_ij = scale (2e-6 sum_d |q_id k_jd| + 1e-7 (sum_d |k_jd| + sum_d |q_id|)) + 2 U |s_ij|        (the last: the product with scale)
    is the absolute error of logit j.  As in window_attention64 it enters weight j once directly and once through the normaliser:
        sum_j p_ij |v_jd| (E_ij + sum_l p_il E_il).
    The second product multiplies the UNNORMALISED weights w_j = exp(s_j - m_running) <= 1 by v: relative part 2e-6 sum_j p_ij |v_jd|;
    a weight below 2^-14 keeps an absolute error of up to 2^-25 in its low plane, later multiplied by rescales alpha <= 1 and divided
    by the normaliser, which is at least 1 (the largest key's weight is 1): 1e-7 sum_j |v_jd|; v's own low plane keeps up to 2^-25 per
    element, weighted by p_j, which sum to 1: 1e-7.  (The GEMM pair splits the normalised p, the same absolute term, and row-scales
    v^T, which removes the last.)  The fp32 softmax between the products: expf's argument rounding |s_ij - m_i| U, the chain of
    rescales exp(m_old - m_new) over the T = ceil(N / 64) key tiles, whose arguments sum to at most dmax_i = max_j |s_ij - m_i| and
    which round l and O twice per tile, the sum of N weights and the fp32 accumulation of N products, expf / reciprocal / final
    product (16):
        U sum_j p_ij |v_jd| (|s_ij - m_i| + dmax_i + 2 N + 8 T + 16)
    Nothing here is fitted to a GPU result."""
    q, k, v = (torch.as_tensor(t) for t in (q, k, v))
    assert q.dtype == k.dtype == v.dtype == torch.float32
    N = k.shape[-2]
    scale = float(np.float32(1.0) / np.sqrt(np.float32(hd)))
    q64, k64, v64 = q.double(), k.double(), v.double()
    s = (q64 @ k64.transpose(-1, -2)) * scale
    d = s - s.max(-1, keepdim=True).values
    e = torch.exp(d)
    p = e / e.sum(-1, keepdim=True)
    exp = p @ v64
    va = v64.abs()
    E = scale * (2e-6 * (q64.abs() @ k64.abs().transpose(-1, -2))
                 + 1e-7 * (k64.abs().sum(-1).unsqueeze(-2) + q64.abs().sum(-1, keepdim=True))) + 2 * U * s.abs()
    T = -(-N // FLASH_KT)
    fp32 = U * (d.abs() + d.abs().amax(-1, keepdim=True) + 2 * N + 8 * T + 16)
    w = p * (E + (p * E).sum(-1, keepdim=True) + fp32 + 2e-6)
    bound = w @ va + 1e-7 * va.sum(-2, keepdim=True) + 1e-7
    return exp, bound


def _flash_cases():
    """N x (heads, hd) x B thinned to 40: every N for both head widths with one and two heads alternating, B = 2 on every other."""
    out = []
    for n, N in enumerate((1, 15, 63, 64, 65, 127, 128, 129, 200, 257)):
        for hd in (64, 128):
            for j in range(2):
                heads = 1 + (n + j) % 2
                out.append(FlashCase(N, heads, hd, 1 + (n + j + hd // 64) % 2))
    return out


FLASH_CASES = _flash_cases()
FLASH_IDS = [c.id for c in FLASH_CASES]
assert len(set(FLASH_IDS)) == len(FLASH_IDS)
assert {(c.heads, c.hd) for c in FLASH_CASES} == {(1, 64), (2, 64), (1, 128), (2, 128)} and {c.B for c in FLASH_CASES} == {1, 2}


# =========================================================================================== GELU epilogue of the f16x3 GEMM
class GeluGemm:
    """gelu(A [M,K] @ W [N,K]^T + bias).  `site`: the epilogue of csrc/gemm_f16x3.hip the case is expected to reach under f16x3, read
    from its dispatch -- "vector": (N | ldc) % 4 == 0; "scalar": otherwise; "splitk": splitk_reduce_kernel, which no ops entry point
    reaches with GELU today (gom_gemm_f32_f16x3_rp never slices K; ops.conv2d_nhwc passes ReLU or nothing), so the GPU file calls
    the library's 1x1 convolution entry with two K slices.  The labels only group the report.  `pad`: ldc - N of the column-slice
    call (ops.gemm(..., relu="gelu", out=buffer[:, col0:col0 + N]))."""

    def __init__(self, site, M, N, K, pad, note):
        self.site, self.M, self.N, self.K, self.pad, self.note = site, M, N, K, pad, note
        self.id = "%s-%dx%dx%d-pad%d" % (site, M, N, K, pad)

    @functools.lru_cache(maxsize=None)
    def inputs(self):
        g = np.random.default_rng(self.M * 1009 + self.N * 31 + self.K)
        f = lambda a: ro(np.ascontiguousarray(a, np.float32))
        A = 1.5 * g.standard_normal((self.M, self.K))
        A = np.where(g.random(A.shape) < 0.25, 0.25 * (2 * g.random(A.shape) - 1), A)        # low planes below fp16's normal range
        W = g.standard_normal((self.N, self.K)) / np.sqrt(self.K) * np.logspace(-1, 0.7, self.N).reshape(-1, 1)
        return f(A), f(W), f(g.standard_normal(self.N))

    @functools.lru_cache(maxsize=None)
    def expected(self):
        return ro(*gelu_gemm64(*self.inputs()))


def gelu_gemm64(A, W, bias):
    """-> (exp, bound).  bound = 1.13 (2e-6 (|A| |W|^T + |bias|) + 1e-7 sum_k |W|) + gelu_bound(v): the contract's pre-activation bound
    times GELU's largest slope (1.129 at x = sqrt 2) plus the evaluation of GELU at the pre-activation value."""
    A, W, b = (np.asarray(t, np.float64) for t in (A, W, bias))
    v = A @ W.T + b
    pre = 2e-6 * (np.abs(A) @ np.abs(W).T + np.abs(b)) + 1e-7 * np.abs(W).sum(1)
    return gelu64(v), 1.13 * pre + gelu_bound(v)


GELU_GEMM_CASES = [
    GeluGemm("vector", 130, 72, 36, 0, "two M tiles with a row tail, BN = 128 with a column tail, K tail (36 = 1 k-tile + 4)"),
    GeluGemm("vector", 130, 72, 36, 8, "the same into a column slice, ldc = N + 8"),
    GeluGemm("vector", 6, 8, 32, 4, "BN = 64 (N <= 64), one ragged tile, ldc = N + 4"),
    GeluGemm("scalar", 6, 70, 32, 0, "N % 4 = 2"),
    GeluGemm("scalar", 134, 66, 68, 5, "N % 4 = 2 and ldc % 4 = 3, two M tiles with a row tail"),
    GeluGemm("scalar", 6, 72, 32, 1, "N % 4 = 0 but ldc % 4 = 1"),
    GeluGemm("splitk", 6, 6, 64, 0, "two K slices of one k-tile each (1x1 convolution entry), N % 4 != 0"),
    GeluGemm("splitk", 133, 72, 128, 0, "two K slices of two k-tiles, two M tiles with a row tail"),
]
GELU_GEMM_IDS = [c.id for c in GELU_GEMM_CASES]
assert len(set(GELU_GEMM_IDS)) == len(GELU_GEMM_IDS)
