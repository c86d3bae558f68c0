"""No GPU: the float64 statements of tests/backbone_statement.py against independent evaluations (torch float64 functional ops,
F.unfold, the window code of oracle/vitae_oracle.py and the mask of oracle/swin_oracle.py); on every case of every table an fp32
evaluation (numpy / torch float32 in the kernel's order of operations), or for the flash kernel and the GELU GEMM an emulation of the
two-plane fp16 split (tests/test_f16x3_cpu.py), stays inside the bound -- the worst error / bound per kernel is printed; and on the
same inputs every planted mistake leaves the bound, or the bit-exact comparison, in at least one case, which the test names.

tests/test_backbone_forms_gpu.py asserts the same bounds on the same bits, so a kernel carrying one of these mistakes fails there
on the case named here."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import backbone_statement as S
from test_f16x3_cpu import gemm_f16x3, split

f32, f64 = np.float32, np.float64
RATIOS = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for k, v in sorted(RATIOS.items()):
        print("backbone emulation worst |got-exp| / bound  %-34s %.4f" % (k, v))


def _ratio(name, got, exp, bound):
    got, exp, bound = (np.asarray(t, f64) for t in (got, exp, bound))
    assert np.isfinite(got).all(), name
    r = float((np.abs(got - exp) / bound).max())
    RATIOS[name] = max(RATIOS.get(name, 0.0), r)
    return r


def _outside(got, exp, bound):
    got = np.asarray(got, f64)
    return bool((~(np.abs(got - np.asarray(exp, f64)) <= np.asarray(bound, f64))).any())


def _caught(name, catching):
    assert catching, "planted mistake `%s` passes every case of its table" % name
    print("mistake %-28s caught by %d cases, first: %s" % (name, len(catching), catching[0]))


# =========================================================================================== data movement
def _win_src(H, W, shift, wrap_h=None, sign=1):
    """For every window row of the padded grid, the (y, x) of the token it shows, or -1: explicit coordinates, no roll / reshape."""
    Hp, Wp = S.ceil_to(H, 7), S.ceil_to(W, 7)
    src = np.full((Hp // 7, Wp // 7, 49, 2), -1)
    for wy in range(Hp // 7):
        for wx in range(Wp // 7):
            for t in range(49):
                y, x = (wy * 7 + t // 7 + sign * shift) % (wrap_h or Hp), (wx * 7 + t % 7 + sign * shift) % Wp
                if y < H and x < W:
                    src[wy, wx, t] = (y, x)
    return src.reshape(-1, 2)


def _gather_by_coords(x, src):
    B, H, W, C = x.shape
    out = torch.zeros(B, src.shape[0], C)
    ok = src[:, 0] >= 0
    out[:, ok] = x[:, src[ok, 0], src[ok, 1]]
    return out.reshape(-1, C)


def test_movement_statements_against_independent_evaluations():
    for c in S.MOVE_CASES:
        io, exp = S.move_io(c.id)
        if c.op == "swin_patchify":
            x = F.pad(io["img"].permute(0, 3, 1, 2), (0, (-c.W) % 4, 0, (-c.H) % 4))
            u = F.unfold(x, 4, stride=4)                                             # [B, (c, kh, kw), L]
            ind = u.view(c.B, 4, 4, 4, -1).permute(0, 4, 2, 3, 1).reshape(-1, 64)
        elif c.op == "swin_window_gather":
            ind = _gather_by_coords(io["x"], _win_src(c.H, c.W, c.shift))
        elif c.op == "swin_window_scatter_add":
            src = _win_src(c.H, c.W, c.shift)
            ind = io["shortcut"].clone()
            win = io["win"].view(c.B, -1, c.C)
            for r in np.nonzero(src[:, 0] >= 0)[0]:
                ind[:, src[r, 0], src[r, 1]] += win[:, r]
            assert not bool(torch.isnan(win[:, src[:, 0] >= 0]).any()) and bool(torch.isnan(win[:, src[:, 0] < 0]).all())
        elif c.op == "swin_patch_merge":
            x = F.pad(io["x"].permute(0, 3, 1, 2), (0, c.W % 2, 0, c.H % 2))
            u = F.unfold(x, 2, stride=2).view(c.B, c.C, 2, 2, -1)                    # [B, c, kh, kw, L]
            ind = u.permute(0, 4, 3, 2, 1).reshape(-1, 4 * c.C)                      # part = kh + 2 kw
        elif c.op in ("vitae_window_gather", "vitae_window_crop"):
            top, bot, left, right = S.vitae_pads(c.H, c.W)
            assert top <= bot <= top + 1 and left <= right <= left + 1 and (c.H + top + bot) % 7 == 0 and (c.W + left + right) % 7 == 0
            Hp, Wp = c.H + top + bot, c.W + left + right
            if c.op == "vitae_window_gather":
                full = torch.zeros(c.B, Hp, Wp, c.C)
                full[:, top:top + c.H, left:left + c.W] = io["x"]
                ind = torch.stack([full[b, wy * 7:wy * 7 + 7, wx * 7:wx * 7 + 7].reshape(49, c.C) for b in range(c.B)
                                   for wy in range(Hp // 7) for wx in range(Wp // 7)]).reshape(-1, c.C)
            else:
                full = torch.zeros(c.B, Hp, Wp, c.C)
                n = 0
                for b in range(c.B):
                    for wy in range(Hp // 7):
                        for wx in range(Wp // 7):
                            full[b, wy * 7:wy * 7 + 7, wx * 7:wx * 7 + 7] = io["win"][n * 49:(n + 1) * 49].view(7, 7, c.C)
                            n += 1
                ind = full[:, top:top + c.H, left:left + c.W].reshape(-1, c.C)
                for R in (io["R1"], io["R2"]):
                    ind = ind if R is None else ind + R
        elif c.op == "im2col":
            pad = S.im2col_pad(c.k, c.s, c.d)
            u = F.unfold(io["x"].permute(0, 3, 1, 2), c.k, dilation=c.d, padding=pad, stride=c.s)     # [B, (c, kh, kw), L]
            K = c.k * c.k * c.C
            ind = torch.zeros(u.shape[0] * u.shape[2], c.ldo)
            ind[:, :K] = u.view(c.B, c.C, c.k * c.k, -1).permute(0, 3, 2, 1).reshape(-1, K)
        else:
            ind = torch.tensor([[float(io["wide"][r, io["col0"] + cc]) for r in range(c.rows)] for cc in range(c.cols)])
        assert exp.dtype == torch.float32 and tuple(ind.shape) == tuple(exp.shape), c.id
        assert bool(torch.equal(ind, exp)), c.id


def test_vitae_window_statements_compose_to_the_oracle_window_attention():
    """oracle/vitae_oracle.py's _window_attention (pad, partition, attention, reverse, crop) with identity projections against
    crop(window_attention64(gather(x))) of the statements."""
    from oracle import vitae_oracle as O
    g = torch.Generator().manual_seed(5)
    for (H, W), heads, hd in (((13, 6), 1, 64), ((8, 8), 2, 64), ((1, 1), 1, 128)):
        C = heads * hd
        x = torch.randn(2, H, W, C, generator=g)
        eye = torch.eye(C, dtype=torch.float64)
        sd = {"a.qkv.weight": torch.cat([eye, eye, eye]), "a.proj.weight": eye}
        want = O._window_attention(x.double().view(2, H * W, C), H, W, sd, "a.", heads, C)
        win = S.vitae_window_gather_st(x)
        t = win.view(-1, 49, heads, hd).permute(0, 2, 1, 3)
        exp, _ = S.window_attention64(t, t, t, hd)
        got = S.vitae_window_crop_st(exp.permute(0, 2, 1, 3).reshape(-1, C), 2, H, W)
        assert float((got.view(2, H * W, C) - want).abs().max()) <= 1e-6        # the oracle pre-scales q in float64, the statement in fp32


def test_swin_window_statements_compose_to_the_oracle_block():
    """oracle/swin_oracle.py's _block (norm, pad, roll, partition, attention with the relative-position bias and the shift mask, reverse,
    roll back, crop, shortcut) with identity projections and a silent MLP against
    scatter_add(window_attention64(gather(norm(x)), add = bias[head] + mask[window % nW]), shortcut = x) of the statements."""
    from oracle import swin_oracle as O
    g = torch.Generator().manual_seed(9)
    for (H, W), heads, shift, B in (((12, 17), 3, 3, 2), ((5, 3), 1, 3, 1), ((8, 15), 2, 0, 2), ((14, 7), 1, 3, 3)):
        C = heads * 32
        x = torch.randn(B, H * W, C, generator=g, dtype=torch.float64)
        eye, one, zero = torch.eye(C, dtype=torch.float64), torch.ones(C, dtype=torch.float64), torch.zeros(C, dtype=torch.float64)
        table = torch.randn(169, heads, generator=g, dtype=torch.float64)
        sd = {"norm1.weight": one, "norm1.bias": zero, "attn.qkv.weight": torch.cat([eye, eye, eye]), "attn.qkv.bias": torch.zeros(3 * C, dtype=torch.float64),
              "attn.relative_position_bias_table": table, "attn.proj.weight": eye, "attn.proj.bias": zero, "norm2.weight": one,
              "norm2.bias": zero, "mlp.fc1.weight": eye, "mlp.fc1.bias": zero, "mlp.fc2.weight": torch.zeros(C, C, dtype=torch.float64),
              "mlp.fc2.bias": zero}
        mask = O.shift_mask(H, W).double()
        want = O._block(x, H, W, sd, "", heads, shift, mask)
        xn = F.layer_norm(x, (C,)).float().view(B, H, W, C)
        win = S.swin_window_gather_st(xn, shift)
        nW = win.shape[0] // 49 // B
        t = win.view(-1, 49, heads, 32).permute(0, 2, 1, 3)
        add = table[O.relative_position_index().view(-1)].view(49, 49, heads).permute(2, 0, 1).unsqueeze(0).expand(B * nW, -1, -1, -1)
        if shift > 0:
            add = add + mask.repeat(B, 1, 1).unsqueeze(1)
        exp, _ = S.window_attention64(t, t, t, 32, add)
        got = S.swin_window_scatter_add_st(exp.permute(0, 2, 1, 3).reshape(-1, C), x.view(B, H, W, C), shift)
        assert float((got.view(B, H * W, C) - want).abs().max()) <= 2e-6, (H, W, shift)      # norm(x) rounded to fp32 for the statement


MOVE_MISTAKES = {
    "shift sign reversed": ("swin_window_gather", lambda c, io: _gather_by_coords(io["x"], _win_src(c.H, c.W, c.shift, sign=-1))),
    "wrap by H instead of Hp": ("swin_window_gather", lambda c, io: _gather_by_coords(io["x"], _win_src(c.H, c.W, c.shift, wrap_h=c.H))),
    "top = ceil(td / 2)": ("vitae_window_gather", lambda c, io: _vitae_gather_top_ceil(io["x"])),
    "merge parts (1,0) and (0,1) swapped": ("swin_patch_merge", lambda c, io: _merge_swapped(io["x"])),
    "patchify (kw, kh) swapped": ("swin_patchify", lambda c, io: _patchify_swapped(io["img"])),
    "im2col ignoring dilation": ("im2col", lambda c, io: _im2col_no_dilation(c, io["x"])),
    "transpose reading with ld = cols": ("transpose_into", lambda c, io: io["wide"].reshape(-1)[
        (io["col0"] + torch.arange(c.rows).view(1, -1) * c.cols + torch.arange(c.cols).view(-1, 1)) % io["wide"].numel()]),
}


def _vitae_gather_top_ceil(x):
    B, H, W, C = x.shape
    top, bot, left, right = S.vitae_pads(H, W)
    xp = F.pad(x.permute(0, 3, 1, 2), (left, right, bot, top)).permute(0, 2, 3, 1)
    return xp.reshape(B, xp.shape[1] // 7, 7, xp.shape[2] // 7, 7, C).permute(0, 1, 3, 2, 4, 5).reshape(-1, C)


def _merge_swapped(x):
    x = F.pad(x, (0, 0, 0, x.shape[2] % 2, 0, x.shape[1] % 2))
    return torch.cat([x[:, 0::2, 0::2], x[:, 0::2, 1::2], x[:, 1::2, 0::2], x[:, 1::2, 1::2]], -1).reshape(-1, 4 * x.shape[-1])


def _patchify_swapped(img):
    B, H, W, _ = img.shape
    x = F.pad(img.permute(0, 3, 1, 2), (0, (-W) % 4, 0, (-H) % 4))
    Hp, Wp = x.shape[2] // 4, x.shape[3] // 4
    return x.reshape(B, 4, Hp, 4, Wp, 4).permute(0, 2, 4, 5, 3, 1).reshape(B * Hp * Wp, 64)


def _im2col_no_dilation(c, x):
    out = S.im2col_st(x, c.k, c.s, S.im2col_pad(c.k, c.s, c.d), 1, c.ldo)[0]
    want = S.move_io(c.id)[1]
    return out[:want.shape[0]] if out.shape[0] >= want.shape[0] else F.pad(out, (0, 0, 0, want.shape[0] - out.shape[0]))


@pytest.mark.parametrize("name", list(MOVE_MISTAKES))
def test_movement_mistake_breaks_bit_equality(name):
    op, wrong = MOVE_MISTAKES[name]
    catching = []
    for c in S.MOVE_CASES:
        if c.op != op:
            continue
        io, exp = S.move_io(c.id)
        got = wrong(c, io)
        if tuple(got.shape) != tuple(exp.shape) or not bool(torch.equal(got, exp)):
            catching.append(c.id)
    _caught(name, catching)


# =========================================================================================== gelu_, silu_
def _gelu32(x):
    x = torch.from_numpy(np.array(x, f32))
    return (torch.tensor(0.5) * x * (1.0 + torch.erf(x * torch.tensor(0.70710678118654752440, dtype=torch.float32)))).numpy()


def _silu32(x):
    x = np.asarray(x, f32)
    with np.errstate(over="ignore"):
        return x / (f32(1) + np.exp(-x))


def test_activation_statements_and_fp32_evaluations():
    for n in S.ACT_N:
        x = S.act_inputs(n)
        assert x.shape == (n,)
        x64 = torch.from_numpy(x.astype(f64))
        y = S.gelu64(x)
        ind = F.gelu(x64).numpy()                                  # 0.5 x (1 + erf): cancels in the left tail, hence the absolute term
        assert (np.abs(y - ind) <= 1e-15 * np.abs(x) + 1e-300).all()
        assert all(abs(y[i] - 0.5 * float(x[i]) * math.erfc(-float(x[i]) / math.sqrt(2))) <= 1e-15 * abs(y[i]) for i in range(0, n, 7))
        assert (np.abs(S.silu64(x) - F.silu(x64).numpy()) <= 1e-15 * np.abs(x)).all()
        assert _ratio("gelu_", _gelu32(x), y, S.gelu_bound(x)) <= 1.0
        assert _ratio("silu_", _silu32(x), S.silu64(x), S.silu_bound(x)) <= 1.0
    x = S.act_inputs(1028)
    tanh = 0.5 * x.astype(f64) * (1 + np.tanh(math.sqrt(2 / math.pi) * (x.astype(f64) + 0.044715 * x.astype(f64) ** 3)))
    assert _outside(tanh, S.gelu64(x), S.gelu_bound(x))
    print("mistake the tanh approximation (gelu_)  caught at n = 1028: %d elements" % int((np.abs(tanh - S.gelu64(x)) > S.gelu_bound(x)).sum()))


# =========================================================================================== grouped convolution
def _gconv_direct(i, c, dtype, mistake=None):
    """The convolution tap by tap, one fused multiply-add chain per output in `dtype`, reading the weights in the op's layout
    [3][3][Cout][CG]; `mistake` plants one of the three index mistakes."""
    x, w = np.asarray(i["x"], dtype), np.asarray(i["w"], dtype)
    wk = np.ascontiguousarray(w.transpose(1, 2, 0, 3)).reshape(-1)           # [3][3][Cout][CG] flat
    B, H, W, Cin = x.shape
    Cout, CG, s = c.Cout, c.CG, c.stride
    co = np.arange(Cout)
    grp = co // (CG if mistake == "group" else c.cout_g)
    tap_stride = CG if mistake == "tap" else Cout * CG
    org = 0 if (mistake == "origin" and s == 2) else 1
    acc = np.zeros((B, c.OH, c.OW, Cout), dtype)
    for kh in range(3):
        for kw in range(3):
            for oy in range(c.OH):
                iy = oy * s - org + kh
                if iy < 0 or iy >= H:
                    continue
                for ox in range(c.OW):
                    ix = ox * s - org + kw
                    if ix < 0 or ix >= W:
                        continue
                    for cc in range(CG):
                        ch = (grp * CG + cc) % Cin
                        wv = wk[(co * CG + (kh * 3 + kw) * tap_stride + cc) % wk.size]
                        acc[:, oy, ox, :] = acc[:, oy, ox, :] + x[:, iy, ix, ch] * wv
    v = acc * (dtype(1) if i["scale"] is None else np.asarray(i["scale"], dtype)) + np.asarray(i["shift"], dtype)
    if c.silu:
        v = (v / (dtype(1) + np.exp(-v))).astype(dtype)
    return v if i["R"] is None else v + np.asarray(i["R"], dtype)


def test_grouped_conv_statement_fp32_and_mistakes():
    catching = {"group": [], "tap": [], "origin": []}
    for c in S.GCONV_CASES:
        i = c.inputs()
        exp, bound = c.expected()
        xt = torch.from_numpy(i["x"].astype(f64)).permute(0, 3, 1, 2)
        wt = torch.from_numpy(i["w"].astype(f64)).permute(0, 3, 1, 2)
        ind = F.conv2d(xt, wt, None, c.stride, 1, 1, c.groups)
        if i["scale"] is not None:
            ind = ind * torch.from_numpy(i["scale"].astype(f64)).view(1, -1, 1, 1)
        ind = ind + torch.from_numpy(i["shift"].astype(f64)).view(1, -1, 1, 1)
        ind = F.silu(ind) if c.silu else ind
        ind = ind.permute(0, 2, 3, 1).numpy() + (0 if i["R"] is None else i["R"].astype(f64))
        assert np.abs(ind - exp).max() <= 1e-12 * max(1.0, np.abs(exp).max()), c.id
        assert np.abs(_gconv_direct(i, c, f64) - exp).max() <= 1e-12 * max(1.0, np.abs(exp).max()), c.id
        assert _ratio("grouped_conv3x3<%d>" % c.CG, _gconv_direct(i, c, f32), exp, bound) <= 1.0, c.id
        for m in catching:
            if _outside(_gconv_direct(i, c, f32, m), exp, bound):
                catching[m].append(c.id)
    _caught("group index co // CG", catching["group"])
    _caught("tap stride CG", catching["tap"])
    _caught("stride-2 origin off by one", catching["origin"])


# =========================================================================================== window attention
def _window_attention32(c, kind, mistake=None):
    q, k, v, bias, mask = (None if t is None else t.numpy() for t in c.inputs(kind))
    hd = c.hd
    scale = f32(1.0 / hd) if mistake == "scale 1/hd" else f32(1.0) / np.sqrt(f32(hd))
    s = (q * scale) @ k.transpose(0, 1, 3, 2)
    if bias is not None:
        b = np.roll(bias, -1, 0) if mistake == "bias of head h+1" else bias
        b = b * scale if mistake == "scale on the bias" else b
        s = s + b[None]
        if mask is not None:
            win = np.arange(c.windows)
            s = s + mask[(win // c.nW) % c.nW if mistake == "mask of window win // nW" else win % c.nW][:, None]
    if mistake == "last key dropped":
        s, v = s[..., :-1], v[:, :, :-1]
    if mistake == "V row swapped":
        v = v.copy()
        v[:, :, [0, 48]] = v[:, :, [48, 0]]
    e = np.exp(s - s.max(-1, keepdims=True))
    return (e @ v) * (f32(1) / e.sum(-1, keepdims=True, dtype=f32))


WIN_MISTAKES = ("last key dropped", "scale 1/hd", "scale on the bias", "bias of head h+1", "mask of window win // nW", "V row swapped")


def test_window_attention_statement_fp32_and_mistakes():
    from oracle import swin_oracle
    assert tuple(swin_oracle.shift_mask(8, 15).shape) == (6, 49, 49)          # the op's mask: [windows of an image, 49, 49] of 0 / -100
    catching = {m: [] for m in WIN_MISTAKES}
    for c in S.WIN_CASES:
        for kind in c.kinds:
            q, k, v, bias, mask = c.inputs(kind)
            exp, bound = c.expected(kind)
            s = (q * torch.tensor(1.0 / np.sqrt(c.hd), dtype=torch.float32)).double() @ k.double().transpose(-1, -2)   # the fp32 pre-scale
            if bias is not None:
                s = s + bias.double()[None]
            if mask is not None:
                s = (s.view(c.images, c.nW, c.heads, 49, 49) + mask.double().unsqueeze(1).unsqueeze(0)).view(-1, c.heads, 49, 49)   # :64
                assert bool((mask[0] == 0).sum(-1).eq(1).all())                # window 0: a row sees only its own key
            ind = s.softmax(-1) @ v.double()
            assert float((ind - exp).abs().max()) <= 1e-12 * max(1.0, float(exp.abs().max())), (c.id, kind)
            name = "window_attention_kernel" if c.form == "swin" else "window_attention_wide_kernel<%d>" % c.hd
            assert _ratio(name, _window_attention32(c, kind), exp, bound) <= 1.0, (c.id, kind)
            for m in WIN_MISTAKES:
                if (c.form == "swin" or m in ("last key dropped", "scale 1/hd", "V row swapped")) and \
                        _outside(_window_attention32(c, kind, m), exp, bound):
                    catching[m].append("%s %s" % (c.id, kind))
    for m in WIN_MISTAKES:
        _caught(m, catching[m])
        for form in ("swin", "vitae"):
            if form == "swin" or m in ("last key dropped", "scale 1/hd", "V row swapped"):
                assert any(x.startswith(form) for x in catching[m]), (m, form)


# =========================================================================================== softmax rows
def test_softmax_rows_statement_and_fp32():
    scale = f32(S.SOFTMAX_SCALE)
    for rows, cols in S.SOFTMAX_CASES:
        for kind in S.SOFTMAX_KINDS:
            x = S.softmax_inputs(rows, cols, kind)
            p, bound = S.softmax64(x, scale)
            ind = torch.softmax(torch.from_numpy(x.astype(f64)) * float(scale), -1).numpy()
            assert np.abs(ind - p).max() <= 1e-14
            s = x * scale
            e = np.exp(s - s.max(1, keepdims=True))
            got = e * (f32(1) / e.sum(1, keepdims=True, dtype=f32))
            assert _ratio("softmax_rows_scaled_", got, p, bound) <= 1.0, (rows, cols, kind)
            assert kind != "big" or cols == 1 or np.abs(s).max() > 250
    x = S.softmax_inputs(3, 257, "big")                                             # a planted mistake: no max subtraction
    with np.errstate(over="ignore", invalid="ignore"):
        e = np.exp(x * scale)
        assert _outside(np.nan_to_num(e / e.sum(1, keepdims=True), nan=9.0), *S.softmax64(x, scale))


# =========================================================================================== flash attention
def _mm(a, b):
    return a.astype(f64) @ np.swapaxes(b.astype(f64), -1, -2)


def flash_emulate(q, k, v, hd, mistake=None):
    """csrc/attn_flash.hip in numpy: q, k, v split into two fp16 planes as they are, exact plane products with wide accumulation
    rounded to fp32 per key tile, fp32 online softmax over tiles of 64 keys, the unnormalised weights split again for the second
    product.  q, k, v [..., N, hd] float32 arrays."""
    N = q.shape[-2]
    low = mistake != "low planes dropped"
    scale = f32(1.0 / hd) if mistake == "scale 1/hd" else f32(1.0) / np.sqrt(f32(hd))
    q0, q1 = split(q)
    m = np.full(q.shape[:-1] + (1,), -np.inf, f32)
    l = np.zeros_like(m)
    O = np.zeros(q.shape, f32)
    for kt in range(0, N, S.FLASH_KT):
        kk, vv = k[..., kt:kt + S.FLASH_KT, :], v[..., kt:kt + S.FLASH_KT, :]
        n = kk.shape[-2]
        if mistake == "key >= N with logit 0" and n < S.FLASH_KT:
            z = np.zeros(kk.shape[:-2] + (S.FLASH_KT - n, hd), f32)
            kk, vv = np.concatenate([kk, z], -2), np.concatenate([vv, z], -2)
        k0, k1 = split(kk)
        s = _mm(q0, k0) + ((_mm(q0, k1) + _mm(q1, k0)) if low else 0.0)
        s = s.astype(f32) * scale
        if mistake == "last key dropped" and kt + n == N:
            s[..., n - 1] = -np.inf
        with np.errstate(invalid="ignore"):
            m_new = np.maximum(m, s.max(-1, keepdims=True))
            alpha = np.exp(m - m_new)
            w = np.exp(s - m_new)
        l = l * alpha + w.sum(-1, keepdims=True, dtype=f32)
        if mistake != "no alpha rescale":
            O = O * alpha
        w0, w1 = split(w)
        v0, v1 = split(vv)
        t = lambda a, b: a.astype(f64) @ b.astype(f64)
        O = (O + (t(w0, v0) + ((t(w0, v1) + t(w1, v0)) if low else 0.0))).astype(f32)
        m = m_new
    return O * (f32(1) / l)


FLASH_MISTAKES = ("last key dropped", "key >= N with logit 0", "no alpha rescale", "low planes dropped", "scale 1/hd")


def _fallback_emulate(q, k, v, hd):
    """The GEMM pair: s = f16x3(q, row-scaled k), fp32 softmax of s * scale, f16x3(p, row-scaled v^T)."""
    out = np.zeros(q.shape, f32)
    scale = f32(1.0) / np.sqrt(f32(hd))
    for ix in np.ndindex(q.shape[:-2]):
        s = gemm_f16x3(q[ix], k[ix]).astype(f32) * scale
        e = np.exp(s - s.max(1, keepdims=True))
        p = e * (f32(1) / e.sum(1, keepdims=True, dtype=f32))
        out[ix] = gemm_f16x3(p, np.ascontiguousarray(v[ix].T)).astype(f32)
    return out


def test_flash_statement_emulations_and_mistakes():
    catching = {m: [] for m in FLASH_MISTAKES}
    for c in S.FLASH_CASES:
        for kind in S.FLASH_KINDS:
            q, k, v = c.inputs(kind)
            exp, bound = c.expected(kind)
            ind = ((q.double() @ k.double().transpose(-1, -2)) * float(np.float32(1.0) / np.sqrt(np.float32(c.hd)))).softmax(-1) @ v.double()
            assert float((ind - exp).abs().max()) <= 1e-12 * max(1.0, float(exp.abs().max())), (c.id, kind)
            qn, kn, vn = q.numpy(), k.numpy(), v.numpy()
            assert np.abs(qn).max() < 65504 and np.abs(kn).max() < 65504 and np.abs(vn).max() < 65504
            assert _ratio("flash_attention_kernel<%d>" % c.hd, flash_emulate(qn, kn, vn, c.hd), exp, bound) <= 1.0, (c.id, kind)
            assert _ratio("fallback GEMM pair (f16x3)", _fallback_emulate(qn, kn, vn, c.hd), exp, bound) <= 1.0, (c.id, kind)
            if kind == "tiny":
                assert float(np.abs(split(qn)[0].astype(f32)).max()) < 2.0 ** -14       # the high plane itself is subnormal
            for mname in FLASH_MISTAKES:
                if _outside(flash_emulate(qn, kn, vn, c.hd, mname), exp, bound):
                    catching[mname].append("%s %s" % (c.id, kind))
    for mname in FLASH_MISTAKES:
        _caught(mname, catching[mname])
        assert {x.split("-")[1].split("x")[1] for x in catching[mname]} == {"64", "128"}, mname       # on both head widths


# =========================================================================================== GELU GEMM
def test_gelu_gemm_statement_emulation_and_mistakes():
    catching = {"tanh": [], "before bias": []}
    assert {c.site for c in S.GELU_GEMM_CASES} == {"vector", "scalar", "splitk"}
    for c in S.GELU_GEMM_CASES:
        A, W, b = c.inputs()
        exp, bound = c.expected()
        ind = F.gelu(F.linear(*(torch.from_numpy(t.astype(f64)) for t in (A, W, b)))).numpy()
        assert np.abs(ind - exp).max() <= 1e-12 * max(1.0, np.abs(exp).max())
        pre = (gemm_f16x3(A, W).astype(f32) + b).astype(f32)
        assert _ratio("GELU epilogue (f16x3 emulation)", _gelu32(pre), exp, bound) <= 1.0, c.id
        pre32 = (A @ W.T + b).astype(f32)
        assert _ratio("gemm + gelu_ (fp32)", _gelu32(pre32), exp, bound) <= 1.0, c.id
        p64 = pre.astype(f64)
        if _outside(0.5 * p64 * (1 + np.tanh(math.sqrt(2 / math.pi) * (p64 + 0.044715 * p64 ** 3))), exp, bound):
            catching["tanh"].append(c.id)
        if _outside(_gelu32((pre - b).astype(f32)) + b, exp, bound):
            catching["before bias"].append(c.id)
    _caught("the tanh approximation", catching["tanh"])
    _caught("GELU applied before the bias", catching["before bias"])
    assert all(len(v) == len(S.GELU_GEMM_CASES) for v in catching.values())              # every site would notice
