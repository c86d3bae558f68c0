"""GPU: the shortcut form of the fused bottleneck launch (csrc/bneck_fused.hip, KS > 0) -- a stage's first block with its 1x1
projection shortcut computed inside the launch from the block's input -- against the launches it replaces (shortcut, conv3 +
residual, the next conv1 on the tile kernel) and a float64 statement.

Built forms (k1, mp, ks, stride): res2.0 = (64, 64, 64, 1).  The stride-2 res3.0 form (128, 128, 256, 2) did not beat its two launches
by more than their run-to-run difference and is not built (docs/LAB_NOTES.md), so it has no cases here."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"

# (k1, mp, ks, stride, SOURCE size of the block's input)
FORMS = [(64, 64, 64, 1, (13, 21)), (64, 64, 64, 1, (125, 223))]


def _case(k1, mp, ks, stride, hw, B, seed):
    from gomatching_amd import ops
    g = torch.Generator().manual_seed(seed)
    c4 = 4 * k1
    Hs, Ws = hw
    H, W = (Hs - 1) // stride + 1, (Ws - 1) // stride + 1
    t = {"B": B, "H": H, "W": W, "c4": c4}
    t["a"] = torch.randn(B, H, W, k1, generator=g).abs().to(DEV)                 # conv2's output is behind a ReLU
    t["S"] = torch.randn(B, Hs, Ws, ks, generator=g).abs().to(DEV)               # the block's input: behind a ReLU too
    t["w3"] = (torch.randn(c4, 1, 1, k1, generator=g) / k1 ** 0.5 * torch.logspace(-1, 1, c4).view(-1, 1, 1, 1)).to(DEV)
    t["ws"] = (torch.randn(c4, 1, 1, ks, generator=g) / ks ** 0.5 * torch.logspace(-1, 1, c4).view(-1, 1, 1, 1)).to(DEV)
    t["w1"] = (torch.randn(mp, 1, 1, c4, generator=g) / c4 ** 0.5).to(DEV)
    t["sc3"], t["sh3"] = (torch.rand(c4, generator=g) + 0.5).to(DEV), torch.randn(c4, generator=g).to(DEV) * 0.2
    t["scs"], t["shs"] = (torch.rand(c4, generator=g) + 0.5).to(DEV), torch.randn(c4, generator=g).to(DEV) * 0.2
    t["sc1"], t["sh1"] = (torch.rand(mp, generator=g) + 0.5).to(DEV), torch.randn(mp, generator=g).to(DEV) * 0.2
    t["s3"] = ops.split_weight(t["w3"].reshape(c4, k1), conv_shape=tuple(t["w3"].shape), kind="f16x3")
    t["ss"] = ops.split_weight(t["ws"].reshape(c4, ks), conv_shape=tuple(t["ws"].shape), kind="f16x3")
    t["s1"] = ops.split_weight(t["w1"].reshape(mp, c4), conv_shape=tuple(t["w1"].shape), kind="f16x3")
    t["blk"] = ops.BneckFused(t["s3"], t["sc3"], t["sh3"], t["s1"], t["sc1"], t["sh1"],
                              shortcut=(t["ss"], t["scs"], t["shs"], stride))
    return t


def _launches(t, stride):
    """The path the form replaces: shortcut launch, conv3 + residual, the next block's conv1 (tile kernel)."""
    from gomatching_amd import ops
    R = ops.conv2d_nhwc(t["S"], t["ss"], scale=t["scs"], shift=t["shs"], stride=stride)
    X0 = ops.conv2d_nhwc(t["a"], t["s3"], scale=t["sc3"], shift=t["sh3"], R=R, relu=True)
    Y0 = ops.conv2d_nhwc(X0, t["s1"], scale=t["sc1"], shift=t["sh1"], relu=True)
    return X0, Y0


@pytest.mark.parametrize("k1,mp,ks,stride,hw", FORMS)
def test_shortcut_form_equals_the_launches_and_the_fp64_statement(k1, mp, ks, stride, hw):
    from gomatching_amd import ops
    t = _case(k1, mp, ks, stride, hw, B=2, seed=k1 + mp + ks + hw[0])            # B = 2: 128-pixel workgroups straddle the frames
    c4 = t["c4"]
    assert t["blk"].ks == ks and t["blk"].stride == stride
    X0, Y0 = _launches(t, stride)
    X, Y1 = ops.bneck_fused(t["a"], t["blk"], t["S"])
    ops.check_range_flag(torch.device(DEV, torch.cuda.current_device()))
    assert X.shape == X0.shape and Y1.shape == Y0.shape
    dx, dy = float((X - X0).abs().max()), float((Y1 - Y0).abs().max())
    print("vs the launches: max|dX| = %.3e (max|X0| %.3e), max|dY1| = %.3e (max|Y0| %.3e)"
          % (dx, float(X0.abs().max()), dy, float(Y0.abs().max())))
    # the same products in the same order; the epilogue's fma contraction may differ in the last bit
    assert dx <= 2e-6 * float(X0.abs().max())
    assert dy <= 1e-5 * float(Y0.abs().max()) + 1e-6
    # float64 statement; the bound is the error of the launches themselves against it x 1.5 (the fma-contraction difference is
    # below one ulp per value)
    d = lambda v: v.double().cpu()
    Ssub = d(t["S"])[:, ::stride, ::stride].reshape(-1, ks)
    r = (Ssub @ d(t["ws"]).view(c4, ks).t()) * d(t["scs"]) + d(t["shs"])
    xr = torch.relu((d(t["a"]).view(-1, k1) @ d(t["w3"]).view(c4, k1).t()) * d(t["sc3"]) + d(t["sh3"]) + r)
    yr = torch.relu((xr @ d(t["w1"]).view(mp, c4).t()) * d(t["sc1"]) + d(t["sh1"]))
    ex0, ey0 = float((d(X0).view(-1, c4) - xr).abs().max()), float((d(Y0).view(-1, mp) - yr).abs().max())
    ex, ey = float((d(X).view(-1, c4) - xr).abs().max()), float((d(Y1).view(-1, mp) - yr).abs().max())
    print("vs fp64: X launches %.3e fused %.3e (max %.3e); Y1 launches %.3e fused %.3e (max %.3e)"
          % (ex0, ex, float(xr.abs().max()), ey0, ey, float(yr.abs().max())))
    assert ex <= 1.5 * ex0
    assert ey <= 1.5 * ey0


def test_shortcut_operand_raises_the_range_flag():
    from gomatching_amd import ops
    dev = torch.device(DEV, torch.cuda.current_device())
    k1, c4, mp, ks = 64, 256, 64, 64
    s3 = ops.split_weight(torch.ones(c4, k1, device=DEV) / k1, conv_shape=(c4, 1, 1, k1), kind="f16x3")
    ss = ops.split_weight(torch.ones(c4, ks, device=DEV) / ks, conv_shape=(c4, 1, 1, ks), kind="f16x3")
    s1 = ops.split_weight(torch.ones(mp, c4, device=DEV) / c4, conv_shape=(mp, 1, 1, c4), kind="f16x3")
    one3, z3, one1, z1 = torch.ones(c4, device=DEV), torch.zeros(c4, device=DEV), torch.ones(mp, device=DEV), torch.zeros(mp, device=DEV)
    blk = ops.BneckFused(s3, one3, z3, s1, one1, z1, shortcut=(ss, one3, z3, 1))
    a, S = torch.ones(1, 9, 17, k1, device=DEV), torch.ones(1, 9, 17, ks, device=DEV)
    ops.check_range_flag(dev)
    ops.bneck_fused(a, blk, S)
    ops.check_range_flag(dev)
    S2 = S.clone()
    S2[0, 3, 3, 5] = 7e4                                     # the shortcut's operand beyond fp16
    ops.bneck_fused(a, blk, S2)
    with pytest.raises(Exception, match="fp16's range"):
        ops.check_range_flag(dev)
    a2 = a.clone()
    a2[0, 8, 16, 63] = 7e4                                   # conv3's operand, in the partial last tile
    ops.bneck_fused(a2, blk, S)
    with pytest.raises(Exception, match="fp16's range"):
        ops.check_range_flag(dev)


@pytest.mark.parametrize("k1,mp,ks,stride,hw", FORMS[:1])
def test_frame_bits_do_not_depend_on_the_step(k1, mp, ks, stride, hw):
    from gomatching_amd import ops
    t = _case(k1, mp, ks, stride, hw, B=3, seed=11)
    assert (t["H"] * t["W"]) % 128 != 0
    X3, Y3 = ops.bneck_fused(t["a"], t["blk"], t["S"])
    X1, Y1 = ops.bneck_fused(t["a"][:1].contiguous(), t["blk"], t["S"][:1].contiguous())
    ops.check_range_flag(torch.device(DEV, torch.cuda.current_device()))
    assert torch.equal(X3[:1], X1) and torch.equal(Y3[:1], Y1)


@pytest.mark.parametrize("size", [(1000, 1778), (97, 161)])
def test_backbone_switch(size):
    """ResNet50 with the shortcut inside the fused launch and as a launch of its own: res3 / res4 / res5 within the bound
    tests/test_bneck_gpu.py uses for another summation order (1e-5 x max of the map)."""
    from gomatching_amd import ops
    from gomatching_amd.modeling.backbone import ResNet50
    from gomatching_amd.weights import synth_state_dict
    from helpers import mini_cfg
    sd = synth_state_dict(mini_cfg(), seed=0)
    g = torch.Generator().manual_seed(size[0])
    x = torch.randn((1, size[0], size[1], 4), generator=g).to(DEV)
    x[..., 3] = 0.0
    outs, forms = [], []
    before = ops.BNECK_SHORTCUT
    try:
        for on in (True, False):
            ops.BNECK_SHORTCUT = on
            net = ResNet50(sd, DEV)
            forms.append(sorted(p for p, b in net.fused.items() if b.ks))
            outs.append(net.forward(x))
    finally:
        ops.BNECK_SHORTCUT = before
    ops.check_range_flag(torch.device(DEV, torch.cuda.current_device()))
    assert forms == [["res2.0."], []]
    for k in ("res3", "res4", "res5"):
        d, m = float((outs[0][k] - outs[1][k]).abs().max()), float(outs[1][k].abs().max())
        print("%s: max|d| = %.3e, max = %.3e" % (k, d, m))
        assert m > 0 and d <= 1e-5 * m, k
