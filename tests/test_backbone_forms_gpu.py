"""GPU: every kernel of the Swin / ViTAEv2 backbones (csrc/swin.hip, csrc/vitae.hip, csrc/attn_flash.hip, the GELU epilogue of
csrc/gemm_f16x3.hip) against the float64 statements of tests/backbone_statement.py, element-wise within their derived bounds --
bit for bit for the data-movement kernels -- on every case of its tables.  tests/test_backbone_statement_cpu.py shows on the same
bits that each bound holds an fp32 / two-plane evaluation and does not hold the planted mistakes (a dropped key, `win / nW` for
the mask row, a missing alpha rescale, a swapped merge part, ...), and names the case that catches each.

Every operand is a view into a NaN-filled allocation: rows before and after it, and gap columns wherever the entry point takes a
leading dimension (the GEMM's A, the transpose's source, the softmax rows).  Every output lies in a buffer prefilled with the
NaN-payload sentinel 0x7FC0DEAD, and every element the op does not own must keep those bits: where the entry point takes its
output (ops.gemm's `out`, ops.transpose_into, the in-place gelu_ / silu_ / softmax_rows_scaled_) the test passes such a view;
the other entry points allocate their result with torch.empty, which the `guard` fixture replaces for the call by an allocator
that hands out the middle of a sentinel buffer -- an element the kernel leaves unwritten is then not finite, and a write before or
past the result is seen.  No case is skipped and no element is sampled.

The form labels follow the dispatch as read from the sources and only group the report printed at the end (worst |got - exp| /
bound per kernel form).  Measured once: 390 tests, 4.4 s on one MI355X (the largest tensors are 8192-column softmax rows and N = 257 attention)."""
import time

import numpy as np
import pytest
import torch

import backbone_statement as S

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENTINEL = 0x7FC0DEAD
RATIOS = {}
T0 = time.time()


def _ops():
    from gomatching_amd import ops
    return ops


def _gom_error():
    from gomatching_amd.lib import GomError
    return GomError


def _sentinel(n):
    return torch.full((n,), SENTINEL, dtype=torch.int32, device=DEV).view(torch.float32)


def _embed(t, pre=8, post=8):
    """`t` on the GPU as a contiguous view inside a NaN-filled allocation (8 floats before and after: 16-byte alignment kept)."""
    if t is None:
        return None
    t = torch.as_tensor(t)
    buf = torch.full((pre + t.numel() + post,), float("nan"), device=DEV)
    v = buf[pre:pre + t.numel()].view(t.shape)
    v.copy_(t)
    return v


def _embed_rows(t, gap=4):
    """A 2-D operand inside rows `gap` floats wider, with a NaN row before and after: a row-strided view."""
    t = torch.as_tensor(t)
    buf = torch.full((t.shape[0] + 2, t.shape[1] + gap), float("nan"), device=DEV)
    v = buf[1:1 + t.shape[0], :t.shape[1]]
    v.copy_(t)
    return v


def _untouched(flat, owned_idx, what):
    """Every element of the flat sentinel buffer outside `owned_idx` keeps the sentinel's bits."""
    keep = torch.ones(flat.numel(), dtype=torch.bool)
    keep[owned_idx.reshape(-1)] = False
    assert bool((flat.cpu().view(torch.int32)[keep] == SENTINEL).all()), "%s: wrote outside its output" % what


def _check(got, exp, bound, form, what):
    got = torch.as_tensor(got).detach().cpu().double().numpy()
    exp, bound = np.asarray(exp, np.float64), np.asarray(bound, np.float64)
    assert got.shape == exp.shape, (what, got.shape, exp.shape)
    assert np.isfinite(got).all(), "%s: %d outputs are not finite" % (what, int((~np.isfinite(got)).sum()))
    r, at = S.worst(got, exp, bound)
    RATIOS[form] = max(RATIOS.get(form, (0.0, "")), (r, what))
    assert r <= 1.0, "%s: |got - exp| / bound = %.3f at %s: got %r exp %r bound %.3e" % (what, r, at, got[at], exp[at], bound[at])


def _check_bits(got, exp, form, what):
    got = got.cpu().contiguous()
    assert tuple(got.shape) == tuple(exp.shape), (what, tuple(got.shape), tuple(exp.shape))
    assert bool(torch.equal(got.view(torch.int32), exp.contiguous().view(torch.int32))), "%s: %d elements differ" % (
        what, int((got != exp).sum()))
    RATIOS.setdefault(form, (0.0, "bit-equal"))


class _GuardedTorch:
    """Stands in for the `torch` name inside gomatching_amd.ops during one test: fp32 results are views into sentinel buffers with
    16 guard floats on either side; everything else is torch's own."""

    def __init__(self):
        self.buffers = []

    def __getattr__(self, name):
        return getattr(torch, name)

    def empty(self, *shape, dtype=None, device=None):
        shape = tuple(shape[0]) if len(shape) == 1 and not isinstance(shape[0], int) else tuple(shape)
        if dtype is not torch.float32:
            return torch.empty(shape, dtype=dtype, device=device)
        n = int(np.prod(shape))
        flat = _sentinel(16 + n + 16)
        self.buffers.append((flat, n))
        return flat[16:16 + n].view(shape)

    def empty_like(self, t):
        return self.empty(tuple(t.shape), dtype=t.dtype, device=t.device)

    def check(self):
        assert self.buffers, "the op allocated no result through torch.empty"
        for flat, n in self.buffers:
            _untouched(flat, 16 + torch.arange(n), "an allocated result of %d floats" % n)
        self.buffers = []


@pytest.fixture
def guard(monkeypatch):
    g = _GuardedTorch()
    monkeypatch.setattr(_ops(), "torch", g)
    yield g
    assert not g.buffers, "a test left allocated results unchecked"


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for k, v in sorted(RATIOS.items()):
        print("backbone worst |got-exp| / bound  %-40s %.4f  %s" % (k, v[0], v[1]))
    print("backbone forms file: %.1f s" % (time.time() - T0))


# =========================================================================================== data movement
@pytest.mark.parametrize("case_id", S.MOVE_IDS)
def test_movement_bit_exact(case_id, guard):
    ops, c = _ops(), S.move_case(case_id)
    io, exp = S.move_io(case_id)
    form = c.op
    if c.op == "swin_patchify":
        got, Hp, Wp = ops.swin_patchify(_embed(io["img"]))
        assert (Hp, Wp) == ((c.H + 3) // 4, (c.W + 3) // 4)
    elif c.op == "swin_window_gather":
        got = ops.swin_window_gather(_embed(io["x"].view(-1, c.C)), c.B, c.H, c.W, c.shift)
    elif c.op == "swin_window_scatter_add":
        got = ops.swin_window_scatter_add(_embed(io["win"]), _embed(io["shortcut"]), c.B, c.H, c.W, c.shift)
    elif c.op == "swin_patch_merge":
        got, H2, W2 = ops.swin_patch_merge(_embed(io["x"].view(-1, c.C)), c.B, c.H, c.W)
        assert (H2, W2) == ((c.H + 1) // 2, (c.W + 1) // 2)
    elif c.op == "vitae_window_gather":
        got = ops.vitae_window_gather(_embed(io["x"].view(-1, c.C)), c.B, c.H, c.W)
    elif c.op == "vitae_window_crop":
        got = ops.vitae_window_crop(_embed(io["win"]), c.B, c.H, c.W, R1=_embed(io["R1"]), R2=_embed(io["R2"]))
    elif c.op == "im2col":
        got, OH, OW = ops.im2col(_embed(io["x"]), c.k, c.k, c.s, S.im2col_pad(c.k, c.s, c.d), c.d, c.ldo)
        assert c.B * OH * OW == exp.shape[0]
    else:
        wide = _embed_rows(io["wide"], gap=0)
        ldo = c.rows + 3                                       # the output is wider than the source has rows
        flat = _sentinel(8 + c.cols * ldo + 8)
        out = flat[8:8 + c.cols * ldo].view(c.cols, ldo)
        ops.transpose_into(wide[:, io["col0"]:io["col0"] + c.cols], out)
        got = out[:, :c.rows]
        _untouched(flat, 8 + torch.arange(c.cols).view(-1, 1) * ldo + torch.arange(c.rows).view(1, -1), case_id)
    _check_bits(got.reshape(exp.shape) if got.numel() == exp.numel() else got, exp, form, case_id)
    if c.op != "transpose_into":
        guard.check()


# =========================================================================================== gelu_, silu_
@pytest.mark.parametrize("n", S.ACT_N)
@pytest.mark.parametrize("name", ["gelu_", "silu_"])
def test_activation_in_place(name, n):
    ops = _ops()
    x = S.act_inputs(n)
    flat = _sentinel(8 + n + 8)
    view = flat[8:8 + n]
    view.copy_(torch.from_numpy(np.array(x)))
    getattr(ops, name)(view)
    exp, bound = (S.gelu64(x), S.gelu_bound(x)) if name == "gelu_" else (S.silu64(x), S.silu_bound(x))
    _check(view, exp, bound, name, "%s n=%d" % (name, n))
    _untouched(flat, 8 + torch.arange(n), "%s n=%d" % (name, n))


# =========================================================================================== grouped convolution
@pytest.mark.parametrize("case_id", S.GCONV_IDS)
def test_grouped_conv(case_id, guard):
    ops = _ops()
    c = S.GCONV_CASES[S.GCONV_IDS.index(case_id)]
    i = c.inputs()
    exp, bound = c.expected()
    w = torch.from_numpy(np.array(i["w"])).permute(1, 2, 0, 3).contiguous()              # the op's layout [3, 3, Cout, CG]
    t = lambda a: None if a is None else _embed(torch.from_numpy(np.array(a)))
    got = ops.grouped_conv3x3(t(i["x"]), _embed(w), t(i["scale"]), t(i["shift"]), c.groups, stride=c.stride, silu=c.silu, R=t(i["R"]))
    _check(got, exp, bound, "grouped_conv3x3<%d>" % c.CG, case_id)
    guard.check()


# =========================================================================================== window attention
@pytest.mark.parametrize("case", S.WIN_CASES, ids=[c.id for c in S.WIN_CASES])
def test_window_attention(case, guard):
    ops = _ops()
    form = "window_attention_kernel" if case.form == "swin" else "window_attention_wide_kernel<%d>" % case.hd
    for kind in case.kinds:
        _, _, _, bias, mask = case.inputs(kind)
        exp, bound = case.expected(kind)
        qkv = _embed(case.qkv(kind))
        if case.form == "swin":
            out = ops.swin_window_attention(qkv, _embed(bias), _embed(mask), case.nW, case.heads)
        else:
            out = ops.vitae_window_attention(qkv, case.heads)
        assert tuple(out.shape) == (case.windows * 49, case.C)
        _check(S.unpack_out(out.cpu(), case.windows, case.heads, 49, case.hd), exp, bound, form, "%s %s" % (case.id, kind))
        guard.check()


# =========================================================================================== softmax rows
@pytest.mark.parametrize("rows,cols", S.SOFTMAX_CASES)
def test_softmax_rows_in_place(rows, cols):
    ops = _ops()
    ld = S.ceil_to(cols, 4) + 4
    for kind in S.SOFTMAX_KINDS:
        x = S.softmax_inputs(rows, cols, kind)
        flat = _sentinel((rows + 2) * ld)
        view = flat.view(rows + 2, ld)[1:1 + rows]
        view[:, :cols].copy_(torch.from_numpy(np.array(x)))
        ops.softmax_rows_scaled_(view, cols, S.SOFTMAX_SCALE)
        exp, bound = S.softmax64(x, np.float32(S.SOFTMAX_SCALE))
        what = "%dx%d %s" % (rows, cols, kind)
        _check(view[:, :cols], exp, bound, "softmax_rows_scaled_", what)
        _untouched(flat, ld + torch.arange(rows).view(-1, 1) * ld + torch.arange(cols).view(1, -1), what)


# =========================================================================================== flash attention and the GEMM pair
@pytest.mark.parametrize("case", S.FLASH_CASES, ids=S.FLASH_IDS)
def test_flash_attention(case, guard):
    ops = _ops()
    for kind in S.FLASH_KINDS:
        exp, bound = case.expected(kind)
        qkv = _embed(S.pack_qkv(*case.inputs(kind)))
        out = ops.flash_attention(qkv, case.B, case.N, case.heads)
        assert tuple(out.shape) == (case.B * case.N, case.heads * case.hd)
        _check(S.unpack_out(out.cpu(), case.B, case.heads, case.N, case.hd), exp, bound, "flash_attention_kernel<%d>" % case.hd,
               "%s %s" % (case.id, kind))
        guard.check()
    ops.check_range_flag(DEV)                                  # nothing in range raises the flag


@pytest.fixture(scope="module")
def vitae_net():
    from gomatching_amd.config import setup_cfg
    from gomatching_amd.modeling.vitae import ViTAEv2S
    from gomatching_amd.weights import synth_state_dict
    cfg = setup_cfg(builtin="icdar15")
    cfg.MODEL.BACKBONE.NAME = "build_vitaev2_backbone"
    net = ViTAEv2S(synth_state_dict(cfg, seed=3), torch.device(DEV))
    net.flash = False
    return net


@pytest.mark.parametrize("mode", ["f16x3", "bf16x6", "fp32"])
@pytest.mark.parametrize("case", S.FLASH_CASES, ids=S.FLASH_IDS)
def test_full_attention_gemm_pair(case, mode, vitae_net):
    """ViTAEv2S._full_attention with flash off: GEMM, softmax_rows_scaled_, transpose_into, GEMM over the zero-padded [N, ceil4(N)]
    scratch, on the flash cases under every contraction back-end, held to the flash bound."""
    ops = _ops()
    with ops.gemm_mode(mode):
        for kind in S.FLASH_KINDS:
            exp, bound = case.expected(kind)
            out = vitae_net._full_attention(_embed(S.pack_qkv(*case.inputs(kind))), case.B, case.N, case.heads)
            _check(S.unpack_out(out.cpu(), case.B, case.heads, case.N, case.hd), exp, bound, "fallback GEMM pair (%s)" % mode,
                   "%s %s" % (case.id, kind))
    ops.check_range_flag(DEV)


# =========================================================================================== GELU epilogue
def _splitk_gelu(ops, A, W, bias, c):
    """splitk_reduce_kernel with GELU: the library's convolution entry as a 1x1 convolution over M pixels with two K slices."""
    from gomatching_amd import lib
    pl = W.planes
    x = _embed(torch.from_numpy(np.array(A)))
    flat = _sentinel(8 + c.M * c.N + 8)
    y = flat[8:8 + c.M * c.N]
    nbytes = 4 * 2 * c.M * c.N
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=DEV)
    lib.check(lib.load().gom_conv2d_nhwc_f32_f16x3(ops._p(x), ops._p(pl), pl.stride(0), pl.stride(1), ops._p(W.inv_scale), None,
                                                   ops._p(bias), None, 2, ops._p(y), 1, c.M, 1, c.K, c.N, 1, 1, 1, 0, ops._p(ws), nbytes,
                                                   2, ops._p(ops.range_flag(DEV)), ops._stream()), "gom_conv2d_nhwc_f32_f16x3")
    _untouched(flat, 8 + torch.arange(c.M * c.N), c.id)
    return y.view(c.M, c.N)


@pytest.mark.parametrize("mode", ["f16x3", "bf16x6", "fp32"])
@pytest.mark.parametrize("case_id", S.GELU_GEMM_IDS)
def test_gelu_gemm(case_id, mode, guard):
    ops = _ops()
    c = S.GELU_GEMM_CASES[S.GELU_GEMM_IDS.index(case_id)]
    A, W, b = c.inputs()
    exp, bound = c.expected()
    Ad = _embed_rows(torch.from_numpy(np.array(A)))           # lda = K + 4
    Wd = torch.from_numpy(np.array(W)).to(DEV)
    bd = _embed(torch.from_numpy(np.array(b)))
    Wp = Wd if mode == "fp32" else ops.split_weight(Wd, kind=mode)
    if mode != "f16x3":                                        # GELU is the separate gelu_ pass over a contiguous result
        _check(ops.gemm_gelu(Ad, Wp, bias=bd), exp, bound, "gemm + gelu_ (%s)" % mode, case_id)
        guard.check()
        return
    form = "GELU epilogue: %s" % c.site
    if c.site == "splitk":
        _check(_splitk_gelu(ops, A, Wp, bd, c), exp, bound, form, case_id)
    elif c.pad == 0:
        _check(ops.gemm_gelu(Ad, Wp, bias=bd), exp, bound, form, case_id)
    else:
        ldc = c.N + c.pad                                      # a column slice of a wider buffer: ldc > N
        flat = _sentinel(8 + c.M * ldc + 8)
        out = flat.as_strided((c.M, c.N), (ldc, 1), 8)
        ops.gemm(Ad, Wp, bias=bd, relu="gelu", out=out)
        _check(out, exp, bound, form, case_id)
        _untouched(flat, 8 + torch.arange(c.M).view(-1, 1) * ldc + torch.arange(c.N).view(1, -1), case_id)
    guard.check()                                              # the result where the op allocated it, and the weight's row scales
    ops.check_range_flag(DEV)


# =========================================================================================== range contract, refusals
def test_range_flag_contract():
    """An operand beyond 65504 raises the flag (its fp16 plane is Inf: the result is Inf / NaN, nothing is addressed by it), the
    check raises GomError once and leaves the flag clear."""
    ops, GomError = _ops(), _gom_error()
    ops.check_range_flag(DEV)
    case = S.FLASH_CASES[S.FLASH_IDS.index("n65-h2x64-b1")] if "n65-h2x64-b1" in S.FLASH_IDS else S.FLASH_CASES[8]
    q, k, v = case.inputs("randn")
    k = k.clone()
    k[0, 0, case.N - 1, 3] = 7e4
    out = ops.flash_attention(_embed(S.pack_qkv(q, k, v)), case.B, case.N, case.heads)
    assert not bool(torch.isfinite(out).all())
    with pytest.raises(GomError):
        ops.check_range_flag(DEV)
    ops.check_range_flag(DEV)                                  # clear afterwards
    c = S.GELU_GEMM_CASES[0]
    A, W, b = c.inputs()
    A = np.array(A)
    A[c.M - 1, 5] = 7e4
    ops.gemm_gelu(_embed_rows(torch.from_numpy(A)), ops.split_weight(torch.from_numpy(np.array(W)).to(DEV), kind="f16x3"),
                  bias=torch.from_numpy(np.array(b)).to(DEV))
    with pytest.raises(GomError):
        ops.check_range_flag(DEV)
    ops.check_range_flag(DEV)


def test_abi_refusals():
    """Each call violates one precondition of the C ABI: GomError, nothing launched (the outputs the caller passed keep their bits)."""
    ops, GomError = _ops(), _gom_error()
    z = lambda *s: torch.zeros(s, device=DEV)
    with pytest.raises(GomError):                              # C % 4 != 0
        ops.swin_window_gather(z(49, 6), 1, 7, 7, 0)
    with pytest.raises(GomError):                              # shift 7
        ops.swin_window_gather(z(49, 8), 1, 7, 7, 7)
    with pytest.raises(GomError):                              # head width 32 for the ViTAE form
        ops.vitae_window_attention(z(49, 3 * 32), 1)
    with pytest.raises(GomError):                              # C != 32 heads for the Swin form
        ops.swin_window_attention(z(49, 3 * 64), z(1, 49, 49), None, 1, 1)
    with pytest.raises(GomError):                              # a qkv pointer offset by one float
        ops.vitae_window_attention(z(49 * 192 + 4)[1:1 + 49 * 192].view(49, 192), 1)
    with pytest.raises(GomError):                              # CG = 8
        ops.grouped_conv3x3(z(1, 2, 2, 16), z(3, 3, 4, 8), None, z(4), 2)
    flat = _sentinel(8200)
    with pytest.raises(GomError):                              # cols = 8193
        ops.softmax_rows_scaled_(flat.view(1, 8200), 8193, 1.0)
    assert bool((flat.cpu().view(torch.int32) == SENTINEL).all())
