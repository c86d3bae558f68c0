"""GPU: the launch-profile records of gomatching_amd.ops (`set_gemm_profile`): every instrumented op called once at the smallest
shape its own test file uses, half of the calls inside `profile_scope("decoder_layer")`.  bench.py reads the records by position and
by label prefix and DESIGN.md §5's roofline fractions hang on their FLOP and byte figures, so the (flops, bytes, label, scope) of
every record is held to a literal table with `==`: the figures are integer-valued floats.  The table was recorded from the commit
before the launch bracket became one helper (`ops._timed`), by this file's own call list: run as a program, this file prints the
rows of whatever ops.py is checked out (profiles/ops_bracket_ab.log keeps that run's output)."""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
MINI = [(9, 20), (5, 10), (3, 5), (2, 3)]                        # tests/test_msda_forms_gpu.py's mini pyramid


def _calls(ops):
    """[(name, thunk)]: blocks and inputs are prepared here, the thunks only launch."""
    g = torch.Generator().manual_seed(11)
    r = lambda *s: torch.randn(s, generator=g).to(DEV)
    w = lambda n, k: r(n, k) / k ** 0.5
    f16 = lambda t: ops.split_weight(t, kind="f16x3")
    calls = []
    add = lambda name, fn: calls.append((name, fn))

    # decoder self-attention blocks (tests/test_dec_attn_gpu.py): intra 4 x 25; inter (B, nq, P) = (3, 7, 2); heads (2, 129, 3)
    att = lambda inter, **kw: ops.DecAttnBlock(w(768, 256), r(768) * 0.1, w(256, 256), r(256) * 0.1, r(256) * 0.1 + 1, r(256) * 0.1,
                                               inter, **kw)
    intra, inter, inter_raw = att(False), att(True), att(True, raw=(w(384, 256), r(384) * 0.1))
    x100, p100, x42, p42, x774 = r(100, 256), r(100, 256), r(42, 256), r(42, 256), r(774, 256)
    add("dec_attn intra", lambda: ops.dec_attn(x100, intra, 4, 25, pos=p100))
    add("dec_attn inter", lambda: ops.dec_attn(x42, inter, 6, 7, inner=2))
    add("dec_attn inter raw", lambda: ops.dec_attn(x42, inter_raw, 6, 7, inner=2, raw_pos=p42))
    add("dec_inter_heads", lambda: ops.dec_inter_heads(x774, inter, 6, 129, 3))

    # decoder tail (tests/test_dec_tail_gpu.py): F = 128, M = 129 = one workgroup of either form (80 / 128 rows) and a partial one
    M = 129
    ffn_w = (w(128, 256), r(128) * 0.1, w(256, 128), r(256) * 0.1, r(256) * 0.1 + 1, r(256) * 0.1)
    coord = [(w(256, 256), r(256) * 0.1), (w(256, 256), r(256) * 0.1), (w(2, 256), r(2) * 0.1)]
    qpos = [(w(256, 256), r(256) * 0.1), (w(256, 256), r(256) * 0.1)]
    dim_t = 10000.0 ** (2 * torch.div(torch.arange(128, dtype=torch.float32), 2, rounding_mode="trunc") / 128).to(DEV)
    proj_w = (w(256, 256), r(256) * 0.1, r(256) * 0.1 + 1, r(256) * 0.1)
    xt, rt, ref = r(M, 256), r(M, 256), torch.rand((M, 2), generator=g).to(DEV)
    for form in (2, 1):                                           # explicit: the table must not depend on the GOM_DEC_TAIL2* switches
        plain = ops.DecTail(ffn_w, coord, qpos, dim_t, form=form, waves=8)
        proj = ops.DecTail(ffn_w, coord, qpos, dim_t, proj_w=proj_w, form=form, waves=8)
        for want in (True, False):
            add("dec_tail form %s qpos %s" % (form, want), lambda b=plain, q=want: ops.dec_tail(xt, b, ref, want_qpos=q))
            add("dec_tail form %s qpos %s proj" % (form, want), lambda b=proj, q=want: ops.dec_tail(xt, b, ref, want_qpos=q, residual=rt))

    # projection + LayerNorm (tests/test_proj_ln_gpu.py: M = 31)
    pln = ops.ProjLN(f16(w(256, 256)), r(256) * 0.1, r(256) * 0.1 + 1, r(256) * 0.1)
    x31, r31, cw = r(31, 256), r(31, 256), r(256) * 0.1
    add("proj_ln R", lambda: ops.proj_ln(x31, pln, r31))
    add("proj_ln", lambda: ops.proj_ln(x31, pln, None))
    add("proj_ln_dot", lambda: ops.proj_ln_dot(x31, pln, cw, -1.25))

    # fused FFN and two-layer perceptron (tests/test_ffn_gpu.py): M = 129 = one 128-row tile and a remainder
    ffn = ops.FusedFFN(w(64, 256), r(64) * 0.1, w(256, 64), r(256) * 0.1, r(256) * 0.1 + 1, r(256) * 0.1)
    mlp = ops.FusedMLP2(w(256, 256), r(256) * 0.1, w(256, 256), r(256) * 0.1, True)
    x129 = r(129, 256)
    add("ffn_fused_ln", lambda: ops.ffn_fused_ln(x129, ffn))
    add("mlp2_fused", lambda: ops.mlp2_fused(x129, mlp))

    # row-resident K = 256 GEMM (tests/test_gemm_k256_gpu.py: (M, N, period) = (129, 64, 32))
    lin = ops.K256Linear(f16(w(64, 256)), r(64))
    a2, rp = r(129, 256), r(32, 32)
    add("linear", lambda: ops.linear(x129, lin, groups=1))
    add("linear A2", lambda: ops.linear(x129, lin, A2=a2, groups=1))
    add("linear r_period", lambda: ops.linear(x129, lin, R=rp, r_cols=32, r_period=32, groups=1))

    # ops.gemm: the exact-fp32 tile kernel records for N > 64 under GEMM_MODE "fp32" only; split weights through _gemm_split
    a33, w65, w64, r65 = r(33, 64), w(65, 64), w(64, 64), r(33, 65)

    def fp32(wt):
        with ops.gemm_mode("fp32"):
            return ops.gemm(a33, wt)
    add("gemm fp32 N=65", lambda: fp32(w65))
    add("gemm fp32 N=64 (no record)", lambda: fp32(w64))
    add("gemm fp32 N=65 in f16x3 mode (no record)", lambda: ops.gemm(a33, w65))
    s65, b65 = f16(w65), ops.split_weight(w65, kind="bf16x6")
    add("gemm f16x3", lambda: ops.gemm(a33, s65))
    add("gemm f16x3 R", lambda: ops.gemm(a33, s65, R=r65))
    add("gemm bf16x6", lambda: ops.gemm(a33, b65, R=r65))

    # convolutions: patch (tests/test_conv3x3_patch_gpu.py (1, 8, 16, 128, 128)), pw_k256 (switch forced on), pointwise, 3x3 / 2
    conv_w = lambda co, kh, ci: ops.split_weight(w(co, kh * kh * ci), conv_shape=(co, kh, kh, ci), kind="f16x3")
    w_patch, w_k256, w_pw, w_s2 = conv_w(128, 3, 128), conv_w(512, 1, 256), conv_w(256, 1, 64), conv_w(128, 3, 64)
    xp, xk, xw, rw_, rk = r(1, 8, 16, 128), r(1, 8, 16, 256), r(2, 13, 21, 64), r(2, 13, 21, 256), r(1, 8, 16, 512)
    sc, sh = r(512) * 0.1 + 1, r(512) * 0.1

    def pw_k256(R):
        old = ops.PW_K256, ops.PW_K256_MIN_ROWS
        ops.PW_K256, ops.PW_K256_MIN_ROWS = True, 0
        try:
            return ops.conv2d_nhwc(xk, w_k256, scale=sc, shift=sh, R=R, relu=True)
        finally:
            ops.PW_K256, ops.PW_K256_MIN_ROWS = old
    add("conv patch", lambda: ops.conv2d_nhwc(xp, w_patch, relu=True, stride=1, pad=1))
    add("conv pw_k256", lambda: pw_k256(None))
    add("conv pw_k256 R", lambda: pw_k256(rk))
    add("conv pointwise", lambda: ops.conv2d_nhwc(xw, w_pw, relu=True))
    add("conv pointwise R", lambda: ops.conv2d_nhwc(xw, w_pw, R=rw_, relu=True))
    add("conv 3x3 stride 2 (no record)", lambda: ops.conv2d_nhwc(xw, w_s2, stride=2, pad=1))

    # fused bottlenecks (tests/test_bneck_gpu.py (64, 64, (13, 21)) and the csrc/bneck2.hip form (256, 256, (1, 1)), B = 2;
    # tests/test_bneck_shortcut_gpu.py (64, 64, 64, 1, (13, 21)))
    def bneck(k1, mp, ks=0):
        c4 = 4 * k1
        s3, s1 = conv_w(c4, 1, k1), conv_w(mp, 1, c4)
        short = (conv_w(c4, 1, ks), r(c4) * 0.1 + 1, r(c4) * 0.1, 1) if ks else None
        return ops.BneckFused(s3, r(c4) * 0.1 + 1, r(c4) * 0.1, s1, r(mp) * 0.1 + 1, r(mp) * 0.1, shortcut=short)
    b64, b256, bsc = bneck(64, 64), bneck(256, 256), bneck(64, 64, ks=64)
    a64, a256, src = r(2, 13, 21, 64).abs(), r(2, 1, 1, 256).abs(), r(2, 13, 21, 64).abs()
    r256, r1024 = r(2, 13, 21, 256), r(2, 1, 1, 1024)
    add("bneck_fused", lambda: ops.bneck_fused(a64, b64, r256))
    add("bneck_fused wide", lambda: ops.bneck_fused(a256, b256, r1024))
    add("bneck_fused shortcut", lambda: ops.bneck_fused(a64, bsc, src))

    # fused MSDA at the mini geometry, B = 2: a decoder call (50 queries), one with valid ratios, an encoder call (every token)
    ss = torch.as_tensor(MINI, dtype=torch.long)
    lsi = torch.cat((ss.new_zeros((1,)), ss.prod(1).cumsum(0)[:-1]))
    B, S, Lq = 2, int(ss.prod(1).sum()), 50
    ss, lsi = ss.to(DEV), lsi.to(DEV)
    value = r(B * S, 256)
    raw_d, ref_d, raw_e = r(B * Lq, 384), torch.rand((B * Lq, 2), generator=g).to(DEV), r(B * S, 384)
    ref_e = ops.encoder_reference_points(ss, lsi, S).repeat(B, 1).contiguous()
    vr = torch.tensor([[0.75, 0.5], [5 / 6, 2 / 3], [1.0, 0.5], [0.5, 1.0]], device=DEV)
    add("msda decoder", lambda: ops.msda_fused(raw_d, ref_d, value, S * 256, ss, lsi, B, Lq))
    add("msda decoder vr", lambda: ops.msda_fused(raw_d, ref_d, value, S * 256, ss, lsi, B, Lq, vr))
    add("msda encoder", lambda: ops.msda_fused(raw_e, ref_e, value, S * 256, ss, lsi, B, S, encoder_hw0=MINI[0] + MINI[1]))
    return calls


def run_calls(ops, collector):
    """Every call once with `collector` installed (None: none), odd-numbered ones inside profile_scope("decoder_layer")."""
    calls = _calls(ops)
    ops.set_gemm_profile(collector)
    try:
        for i, (_, fn) in enumerate(calls):
            if i % 2:
                with ops.profile_scope("decoder_layer"):
                    fn()
            else:
                fn()
    finally:
        ops.set_gemm_profile(None)
    torch.cuda.synchronize()
    ops.check_range_flag(torch.device(DEV, torch.cuda.current_device()))
    return len(calls)


# (flops, bytes, label, scope) in call order, as recorded by the parent of the commit that introduced ops._timed
TABLE = [
    (54988800.0, 1486848.0, 'decattn:intra:4x25', ''),
    (22321152.0, 1265664.0, 'decattn:inter:6x7', 'decoder_layer'),
    (30578688.0, 1815552.0, 'decattn:inter+raw:6x7', ''),
    (406591488.0, 2469888.0, 'decattn:inter-heads:6x129', 'decoder_layer'),
    (84673536.0, 1707008.0, 'dectail:129x128+qpos', ''),
    (101581824.0, 1969152.0, 'dectail:129x128+qpos', 'decoder_layer'),
    (50856960.0, 1574912.0, 'dectail:129x128', ''),
    (67765248.0, 1837056.0, 'dectail:129x128', 'decoder_layer'),
    (84673536.0, 1727488.0, 'dectail:129x128+qpos', ''),
    (101581824.0, 1993728.0, 'dectail:129x128+qpos', 'decoder_layer'),
    (50856960.0, 1595392.0, 'dectail:129x128', ''),
    (67765248.0, 1861632.0, 'dectail:129x128', 'decoder_layer'),
    (4063232.0, 357376.0, 'projln:31x256x256', ''),
    (4063232.0, 325632.0, 'projln:31x256x256', 'decoder_layer'),
    (4079104.0, 294012.0, 'projdot:31x256x257', ''),
    (8454144.0, 397312.0, 'ffn129x256x64', 'decoder_layer'),
    (33816576.0, 796672.0, 'ffn-mlp2:129x256x256', ''),
    (4227072.0, 232704.0, 'k256:129x64x256', 'decoder_layer'),
    (4227072.0, 364800.0, 'k256:129x64x256', ''),
    (4227072.0, 236800.0, 'k256:129x64x256', 'decoder_layer'),
    (274560.0, 33668.0, '33x65x64', ''),
    (274560.0, 33668.0, '33x65x64', 'decoder_layer'),
    (274560.0, 42248.0, '33x65x64', ''),
    (274560.0, 50568.0, '33x65x64', 'decoder_layer'),
    (37748736.0, 720896.0, 'conv3:128x128x1152', ''),
    (33554432.0, 917504.0, 'pwk256:128x512x256', 'decoder_layer'),
    (33554432.0, 1179648.0, 'pwk256:128x512x256', ''),
    (17891328.0, 764416.0, 'pw:546x256x64', 'decoder_layer'),
    (17891328.0, 1323520.0, 'pw:546x256x64', ''),
    (35782656.0, 1537024.0, 'bneck:546x64x256x64', ''),
    (2097152.0, 2150400.0, 'bneck:2x256x1024x256', 'decoder_layer'),
    (53673984.0, 1183232.0, 'bneck:546x64x256x64+sc64/1', ''),
    (3276800.0, 770048.0, 'msda:2x50', 'decoder_layer'),
    (3276800.0, 770048.0, 'msda:2x50', ''),
    (16449536.0, 1799168.0, 'msda:2x251', 'decoder_layer'),
]


def test_records_equal_the_table():
    from gomatching_amd import ops
    got = []
    n = run_calls(ops, got)
    assert n - len(got) == 3                                      # the three calls whose condition is false record nothing
    assert all(len(rec) == 6 for rec in got)
    assert [tuple(rec[2:]) for rec in got] == TABLE
    for e0, e1 in (rec[:2] for rec in got):
        assert e0 is not e1 and e0.elapsed_time(e1) >= 0


def test_no_collector_no_records(monkeypatch):
    from gomatching_amd import ops
    made, earlier = [], []
    ops.set_gemm_profile(earlier)                                 # a collector that was installed and taken away again
    ops.set_gemm_profile(None)
    monkeypatch.setattr(torch.cuda, "Event", lambda *a, **k: made.append(1))
    run_calls(ops, None)
    assert ops._gemm_profile is None and earlier == [] and made == []     # off: not even an event is created


if __name__ == "__main__":                                        # the rows of TABLE, as the checked-out ops.py records them
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from gomatching_amd import ops as _ops
    _got = []
    print("calls", run_calls(_ops, _got), "records", len(_got))
    for _rec in _got:
        print("    (%r, %r, %r, %r)," % tuple(_rec[2:]))
