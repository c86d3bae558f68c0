"""GPU: every convolution form of the library against the float64 statement of tests/conv_statement.py.

  * every case of the table on the f16x3, bf16x6 and fp32 back-ends (csrc/gemm_f16x3.hip, gemm_bf16x6.hip, gemm_conv.hip; the patch
    cases on csrc/conv3x3_patch.hip): |y - conv64| <= conv_bound componentwise, the form ops.conv_plan reports is the declared one, and
    the f16x3 range flag stays down;
  * exact-integer inputs (x in {-3 .. 3}, w in {-2 .. 2}, power-of-two scales, integer shift and residual): small integers are exact in
    both fp16 planes, in bf16 and in the fp32 accumulator, and an fp16 re-split of an integer (or half-integer) intermediate below 2^22
    is exact too, so every form -- the tile kernel on all back-ends, the patch kernel, the fused stem (csrc/stem_pool.hip), the fused
    bottleneck pairs (csrc/bneck_fused.hip, csrc/bneck2.hip) and the shortcut form -- must give the statement's bits;
  * an operand beyond fp16's range in the ragged split-K case raises the device flag through splitk_reduce_kernel, and the next clean
    call does not;
  * a split-K convolution run twice gives identical bits (the slices are summed in slice order).

tests/test_conv_statement_cpu.py shows that the table's shapes catch the addressing mistakes this kernel could make."""
import numpy as np
import pytest
import torch

from conv_statement import CASES, SPLITK_CASES, case, conv64, maxpool64, worst

pytestmark = pytest.mark.gpu
DEV = "cuda"
RATIOS = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for k, v in sorted(RATIOS.items()):
        print("conv worst |y - conv64| / bound  %-8s %.4f  (%s)" % (k, v[0], v[1]))


def _dev():
    return torch.device(DEV, torch.cuda.current_device())


def _d(a):
    return None if a is None else torch.from_numpy(np.array(a)).to(DEV)


def _weight(ops, w, kind):
    wd = _d(w)
    if kind == "fp32":
        return wd
    return ops.split_weight(wd.reshape(wd.shape[0], -1), conv_shape=tuple(wd.shape), kind=kind)


def _run(ops, c, kind, exact=False, x=None):
    """One call of ops.conv2d_nhwc on case c with the patch switch as shipped (on) -> (y on the host, the plan the call took)."""
    i = c.inputs(exact)
    old = ops.CONV3_PATCH
    try:
        ops.CONV3_PATCH = True
        plan = ops.conv_plan(c.rows, c.Cout, c.Cin, c.k, c.k, c.stride, c.pad, kind, residual=c.residual)
        y = ops.conv2d_nhwc(_d(i["x"]) if x is None else x, _weight(ops, i["w"], kind), scale=_d(i["scale"]), shift=_d(i["shift"]),
                            R=_d(i["R"]), relu=c.relu, stride=c.stride, pad=c.pad)
    finally:
        ops.CONV3_PATCH = old
    torch.cuda.synchronize()
    return y.cpu().numpy(), plan


PAIRS = [(c, kind) for c in CASES for kind in c.kinds]


@pytest.mark.parametrize("c,kind", PAIRS, ids=["%s-%s" % (c.id, kind) for c, kind in PAIRS])
def test_case_within_the_bound_on_the_declared_form(c, kind):
    from gomatching_amd import ops
    ops.check_range_flag(_dev())
    exp, bound = c.expected()
    y, plan = _run(ops, c, kind)
    assert plan == c.forms[kind], (c.id, kind, plan)
    assert y.shape == exp.shape
    r, at = worst(y, exp, bound)
    print("%s %s %s: worst |y - conv64| / bound = %.4f at (b, oh, ow, n) = %s" % (c.id, kind, plan, r, at))
    if r > RATIOS.get(kind, (0.0, ""))[0]:
        RATIOS[kind] = (r, c.id)
    assert r <= 1.0, "%s %s: |y - conv64| = %.4f x bound at (b, oh, ow, n) = %s: got %r, statement %r" % (
        c.id, kind, r, at, float(y[at]), float(exp[at]))
    if kind == "f16x3":
        ops.check_range_flag(_dev())


def _same_bits(got, exp, what):
    got = np.asarray(got, np.float64)
    assert got.shape == exp.shape, (what, got.shape, exp.shape)
    bad = got != exp
    if bad.any():
        at = tuple(int(v[0]) for v in np.nonzero(bad))
        raise AssertionError("%s: %d of %d values differ from the statement, first at %s: got %r, statement %r"
                             % (what, int(bad.sum()), bad.size, at, float(got[at]), float(exp[at])))


@pytest.mark.parametrize("c,kind", PAIRS, ids=["%s-%s" % (c.id, kind) for c, kind in PAIRS])
def test_exact_integer_inputs_give_the_statement_bits(c, kind):
    from gomatching_amd import ops
    ops.check_range_flag(_dev())
    y, plan = _run(ops, c, kind, exact=True)
    assert plan == c.forms[kind]
    _same_bits(y, c.expected(exact=True)[0], "%s %s %s" % (c.id, kind, plan))
    ops.check_range_flag(_dev())


def _ints(g, lo, hi, shape):
    return g.integers(lo, hi + 1, shape).astype(np.float32)


@pytest.mark.parametrize("B,H,W", [(3, 9, 11), (1, 7, 30)])
def test_stem_conv_pool_exact(B, H, W):
    """conv 7x7 / 2 / 3 + scale + shift + ReLU + max-pool 3x3 / 2 / 1 as one launch: the maximum is exact, so integers stay exact."""
    from gomatching_amd import ops
    g = np.random.default_rng(100 * H + W)
    x = _ints(g, -3, 3, (B, H, W, 4))
    x[..., 3] = 0.0                                          # the padded fourth channel
    w = _ints(g, -2, 2, (64, 7, 7, 4))
    sc, sh = g.choice([0.5, 1.0, 2.0], 64).astype(np.float32), _ints(g, -3, 3, 64)
    sw = _weight(ops, w, "f16x3")
    ops.check_range_flag(_dev())
    for scale, shift in ((sc, sh), (None, None)):
        exp = maxpool64(conv64(x, w, 2, 3, scale, shift, relu=True))
        got = ops.stem_conv_pool(_d(x), sw, scale=_d(scale), shift=_d(shift))
        torch.cuda.synchronize()
        _same_bits(got.cpu().numpy(), exp, "stem %s" % ((B, H, W),))
        assert len(np.unique(exp)) > 4
    ops.check_range_flag(_dev())


def _bneck_tensors(g, k1, mp, B, H, W):
    c4 = 4 * k1
    t = {"a": _ints(g, -3, 3, (B, H, W, k1)), "w3": _ints(g, -2, 2, (c4, 1, 1, k1)), "w1": _ints(g, -2, 2, (mp, 1, 1, c4)),
         "sc3": g.choice([0.5, 1.0, 2.0], c4).astype(np.float32), "sh3": _ints(g, -3, 3, c4),
         "sc1": g.choice([0.5, 1.0, 2.0], mp).astype(np.float32), "sh1": _ints(g, -3, 3, mp)}
    return t


@pytest.mark.parametrize("k1,mp,hw", [(64, 64, (1, 1)), (64, 64, (5, 7)), (256, 256, (1, 1)), (256, 256, (5, 7))])
def test_bneck_fused_exact(k1, mp, hw):
    """conv3 + BN + residual + ReLU fused with the next conv1 + BN + ReLU: X is an integer or a half below 2^12 (|X| <= 2 (6 k1) + 6),
    its fp16 re-split is exact, and |Y1| <= 2 (2 c4 max|X|) + 3 < 2^24 (k1 = 256: 12.6 M), so both outputs are the statement's bits."""
    from gomatching_amd import ops
    g = np.random.default_rng(k1 + 10 * hw[0] + hw[1])
    B, (H, W), c4 = 2, hw, 4 * k1
    t = _bneck_tensors(g, k1, mp, B, H, W)
    R = _ints(g, -3, 3, (B, H, W, c4))
    xr = conv64(t["a"], t["w3"], 1, 0, t["sc3"], t["sh3"], R, relu=True)
    yr = conv64(xr, t["w1"], 1, 0, t["sc1"], t["sh1"], relu=True)
    assert np.abs(xr).max() < 2 ** 12 and np.abs(yr).max() < 2 ** 24 and np.array_equal(yr, yr.astype(np.float32).astype(np.float64))
    blk = ops.BneckFused(_weight(ops, t["w3"], "f16x3"), _d(t["sc3"]), _d(t["sh3"]), _weight(ops, t["w1"], "f16x3"), _d(t["sc1"]), _d(t["sh1"]))
    assert bool(blk.v2) == (k1 == 256) and not blk.ks        # both kernel files: bneck_fused.hip (64) and bneck2.hip (256)
    ops.check_range_flag(_dev())
    X, Y1 = ops.bneck_fused(_d(t["a"]), blk, _d(R))
    torch.cuda.synchronize()
    ops.check_range_flag(_dev())
    _same_bits(X.cpu().numpy(), xr, "bneck %d X" % k1)
    _same_bits(Y1.cpu().numpy(), yr, "bneck %d Y1" % k1)


def test_bneck_shortcut_form_exact():
    """The shortcut form as tests/test_bneck_shortcut_gpu.py builds it (res2.0: k1 = mp = ks = 64, stride 1) at its smallest size there."""
    from gomatching_amd import ops
    g = np.random.default_rng(77)
    k1, mp, ks, stride, (H, W), B = 64, 64, 64, 1, (13, 21), 2
    c4 = 4 * k1
    t = _bneck_tensors(g, k1, mp, B, H, W)
    S, ws = _ints(g, -3, 3, (B, H, W, ks)), _ints(g, -2, 2, (c4, 1, 1, ks))
    scs, shs = g.choice([0.5, 1.0, 2.0], c4).astype(np.float32), _ints(g, -3, 3, c4)
    r = conv64(S, ws, stride, 0, scs, shs)
    xr = conv64(t["a"], t["w3"], 1, 0, t["sc3"], t["sh3"], r, relu=True)
    yr = conv64(xr, t["w1"], 1, 0, t["sc1"], t["sh1"], relu=True)
    assert np.abs(xr).max() < 2 ** 12 and np.abs(yr).max() < 2 ** 24
    blk = ops.BneckFused(_weight(ops, t["w3"], "f16x3"), _d(t["sc3"]), _d(t["sh3"]), _weight(ops, t["w1"], "f16x3"), _d(t["sc1"]), _d(t["sh1"]),
                         shortcut=(_weight(ops, ws, "f16x3"), _d(scs), _d(shs), stride))
    assert blk.ks == ks and blk.stride == stride
    ops.check_range_flag(_dev())
    X, Y1 = ops.bneck_fused(_d(t["a"]), blk, _d(S))
    torch.cuda.synchronize()
    ops.check_range_flag(_dev())
    _same_bits(X.cpu().numpy(), xr, "shortcut form X")
    _same_bits(Y1.cpu().numpy(), yr, "shortcut form Y1")


def test_split_k_reducer_raises_the_range_flag():
    """One operand of 7e4 in the ragged split-K case: its slice's partial sums are not finite and splitk_reduce_kernel raises the device
    flag (never a silent wrong result); the next clean call leaves it down."""
    from gomatching_amd import ops
    c = case("1x9x11-64to64-k7s2p3-bn_relu")
    assert c.ragged and c.forms["f16x3"] == ("tile", 6)
    ops.check_range_flag(_dev())
    x = _d(c.inputs()["x"])
    x[0, 4, 5, 7] = 7e4
    _, plan = _run(ops, c, "f16x3", x=x)
    assert plan == ("tile", 6)
    with pytest.raises(Exception, match="fp16's range"):
        ops.check_range_flag(_dev())
    y, _ = _run(ops, c, "f16x3")
    ops.check_range_flag(_dev())                             # cleared by the raise, and not raised again
    assert worst(y, *c.expected())[0] <= 1.0


@pytest.mark.parametrize("c", SPLITK_CASES, ids=[c.id for c in SPLITK_CASES])
@pytest.mark.parametrize("kind", ["f16x3", "bf16x6"])
def test_split_k_twice_gives_identical_bits(c, kind):
    from gomatching_amd import ops
    a, plan = _run(ops, c, kind)
    b, _ = _run(ops, c, kind)
    assert plan[1] > 1
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
