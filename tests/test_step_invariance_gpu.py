"""Step invariance: a frame's results are bit-identical whatever shares its detector step.  The kernel choices that
depend on a launch's row count -- the convolutions' split-K count and patch kernel (`ops.conv_plan`), the decoder tail's form
(`ops.tail_form2_wins`) -- are made for the model's planned step (`ops.step_plan`, entered by GoMatching._detect_core) and not for the
call's B.  Every case below straddles a switch of the unplanned rule (asserted in the test, from the rule itself), so none can pass
because all its step sizes happened to make the same choice."""
import math

import pytest
import torch
import torch.nn.functional as F

DEV = "cuda"
PLAN = 8                                                     # GoMatching's default frames_per_step, the bench workload's step
P = 25                                                       # control points per query


def _out(h, w, k, s, p):
    return (h + 2 * p - k) // s + 1, (w + 2 * p - k) // s + 1


def _r50_convs(H, W):
    """(name, Cin, Cout, k, stride, pad, OH, OW) of every convolution of the R-50 backbone (modeling/backbone.py: stride on conv2 and
    the shortcut) and of input_proj[3] (3x3 / 2 on res5) for one H x W frame."""
    h, w = _out(H, W, 7, 2, 3)
    convs = [("stem.conv1", 4, 64, 7, 2, 3, h, w)]
    h, w = _out(h, w, 3, 2, 1)                               # max pool
    cin = 64
    for stage, nblk, first, mid in (("res2", 3, 1, 64), ("res3", 4, 2, 128), ("res4", 6, 2, 256), ("res5", 3, 2, 512)):
        for i in range(nblk):
            s = first if i == 0 else 1
            oh, ow = _out(h, w, 3, s, 1)
            if i == 0:
                convs.append(("%s.0.shortcut" % stage, cin, 4 * mid, 1, s, 0, oh, ow))
            convs.append(("%s.%d.conv1" % (stage, i), cin, mid, 1, 1, 0, h, w))
            convs.append(("%s.%d.conv2" % (stage, i), mid, mid, 3, s, 1, oh, ow))
            convs.append(("%s.%d.conv3" % (stage, i), mid, 4 * mid, 1, 1, 0, oh, ow))
            h, w, cin = oh, ow, 4 * mid
    oh, ow = _out(h, w, 3, 2, 1)
    convs.append(("input_proj.3", 2048, 256, 3, 2, 1, oh, ow))
    return convs


def _old_conv_choice(ops, rows, Cin, Cout, k, s, p, kind, residual=False):
    """The unplanned rule, worked out from the library's split count for the call's own rows: (kernel, splits)."""
    splits = ops._L().gom_conv_bf16x6_splits(rows, Cout, k * k * Cin)
    if kind == "f16x3" and ops.CONV3_PATCH and k == 3 and s == 1 and p == 1 and not residual and splits <= 1 \
            and ops._L().gom_conv3x3_patch_supported(Cin, Cout):
        return "patch", 0
    return "tile", splits


# ------------------------------------------------------------------------------------------ the decisions (no GPU)
# default (ICDAR15, 100 queries) and BOVText's landscape frames: 1000x1778; BOVText's portrait ones: 1778x1000; DSText: 1280x2276,
# 300 queries
GEOMETRIES = [((1000, 1778), 100), ((1778, 1000), 100), ((1280, 2276), 300)]


@pytest.mark.parametrize("kind", ["f16x3", "bf16x6"])
@pytest.mark.parametrize("hw,nq", GEOMETRIES)
def test_conv_plan_makes_one_choice_for_every_step_size(hw, nq, kind):
    from gomatching_amd import ops
    straddles = 0
    for name, cin, cout, k, s, p, oh, ow in _r50_convs(*hw):
        res = name.endswith("conv3")
        old = {_old_conv_choice(ops, B * oh * ow, cin, cout, k, s, p, kind, res) for B in range(1, PLAN + 1)}
        straddles += len(old) > 1
        assert ops.conv_plan(oh * ow, cout, cin, k, k, s, p, kind, residual=res) == \
            _old_conv_choice(ops, oh * ow, cin, cout, k, s, p, kind, res), name          # no plan: the call's own rows, as before
        with ops.step_plan(PLAN):
            got = {ops.conv_plan(ops.plan_rows(B, oh * ow), cout, cin, k, k, s, p, kind, residual=res) for B in range(1, 2 * PLAN + 1)}
        assert got == {_old_conv_choice(ops, PLAN * oh * ow, cin, cout, k, s, p, kind, res)}, name    # a full step's choice
        assert ops.conv_plan(oh * ow, cout, cin, k, k, s, p, "fp32") == ("fp32", 0)
    assert straddles >= 4                                    # res5 conv1 / conv2 and input_proj[3] switch with B at these sizes
    assert ops.STEP_FRAMES is None


@pytest.mark.parametrize("hw,nq", GEOMETRIES)
def test_tail_form_makes_one_choice_for_every_step_size(hw, nq):
    from gomatching_amd import ops
    with ops.step_plan(PLAN):
        got = {ops.tail_form2_wins(ops.plan_rows(B, nq * P)) for B in range(1, 2 * PLAN + 1)}
    assert got == {ops.tail_form2_wins(PLAN * nq * P)}
    # the unplanned rule switches: nq = 300 inside one step of 8 (B = 1, 2, 5 form 2), nq = 100 from B = 9 on
    assert len({ops.tail_form2_wins(B * nq * P) for B in range(1, 2 * PLAN + 1)}) == 2
    assert ops.plan_rows(3, nq * P) == 3 * nq * P            # no plan: the call's own rows


def test_step_plan_nests_and_restores():
    from gomatching_amd import ops
    assert ops.STEP_FRAMES is None
    with ops.step_plan(8):
        assert ops.plan_rows(3, 10) == 80
        with ops.step_plan(2):
            assert ops.plan_rows(5, 10) == 20
        assert ops.STEP_FRAMES == 8
        with pytest.raises(RuntimeError):
            with ops.step_plan(1):
                raise RuntimeError("step failed")
        assert ops.STEP_FRAMES == 8
    assert ops.STEP_FRAMES is None


# ------------------------------------------------------------------------------------------ convolutions
# the real workload's layers at 1000x1778 (per-frame input geometry): (name, Cin, Cout, k, stride, pad, H, W, relu)
CONV_CASES = [("input_proj.3", 2048, 256, 3, 2, 1, 32, 56, False), ("res5.conv2", 512, 512, 3, 1, 1, 32, 56, True),
              ("res5.0.conv2", 512, 512, 3, 2, 1, 63, 112, True), ("res5.conv1", 2048, 512, 1, 1, 0, 32, 56, True),
              ("res4.conv2", 256, 256, 3, 1, 1, 63, 112, True)]
SUBSETS = (1, 2, 5, 7)
_REF64 = {}


def _close(a, b, atol, rtol, msg):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    err = (a - b).abs()
    assert bool((err <= atol + rtol * b.abs()).all()), "%s max|d|=%.3e (tol %.1e + %.1e |ref|)" % (msg, float(err.max()), atol, rtol)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["f16x3", "bf16x6"])
@pytest.mark.parametrize("case", CONV_CASES, ids=[c[0] for c in CONV_CASES])
def test_conv_frames_are_bit_identical_across_step_sizes(case, kind):
    from gomatching_amd import ops
    name, cin, cout, k, s, p, H, W, relu = case
    oh, ow = _out(H, W, k, s, p)
    old = [_old_conv_choice(ops, B * oh * ow, cin, cout, k, s, p, kind) for B in SUBSETS + (PLAN,)]
    assert len(set(old)) > 1, "case %s no longer straddles a switch of the unplanned rule: %s" % (name, old)
    g = torch.Generator().manual_seed(cin + cout + k + s)
    x = torch.randn(PLAN, H, W, cin, generator=g)
    w = torch.randn(cout, k, k, cin, generator=g) / math.sqrt(cin * k * k)
    sc = torch.rand(cout, generator=g) + 0.5 if relu else None
    sh = torch.randn(cout, generator=g)
    dv = lambda t: None if t is None else t.to(DEV)
    xd = dv(x)
    sw = ops.split_weight(dv(w).reshape(cout, -1), conv_shape=tuple(w.shape), kind=kind)
    run = lambda a, b: ops.conv2d_nhwc(xd[a:b].contiguous(), sw, scale=dv(sc), shift=dv(sh), relu=relu, stride=s, pad=p)
    with ops.step_plan(PLAN):
        full = run(0, PLAN)
        parts = {B: run(0, B) for B in SUBSETS}
    torch.cuda.synchronize()
    ops.check_range_flag(DEV)
    for B, y in parts.items():
        for f in range(B):
            assert torch.equal(y[f], full[f]), "%s %s: frame %d of a %d-frame step differs from the %d-frame step" % (name, kind, f, B, PLAN)
    # against float64 at the tolerances of test_ops_gpu.py::test_conv_nhwc: the planned launches and, for B = 1, the unplanned one
    # (the split-K forms the direct op call takes at these real map sizes)
    ref = _REF64.get(name)
    if ref is None:                                          # the same frames and weights for both back-ends
        ref = F.conv2d(x[:2].permute(0, 3, 1, 2).double(), w.permute(0, 3, 1, 2).double(), stride=s, padding=p)
        ref = ref * (sc.double().view(1, -1, 1, 1) if sc is not None else 1.0) + sh.double().view(1, -1, 1, 1)
        ref = _REF64[name] = (F.relu(ref) if relu else ref).permute(0, 2, 3, 1)
    _close(parts[1], ref[:1], 3e-5, 1e-5, "%s %s planned B=1" % (name, kind))
    _close(parts[2], ref, 3e-5, 1e-5, "%s %s planned B=2" % (name, kind))
    _close(run(0, 1), ref[:1], 3e-5, 1e-5, "%s %s unplanned B=1 (%s)" % (name, kind, old[0]))


# ------------------------------------------------------------------------------------------ decoder tail
def _tail_weights(F_, seed):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(s, generator=g)
    ffn = (r(F_, 256) * 0.05, r(F_) * 0.1, r(256, F_) * 0.05, r(256) * 0.1, 1.0 + 0.2 * r(256), 0.1 * r(256))
    coord = [(r(256, 256) / 16, r(256) * 0.1), (r(256, 256) / 16, r(256) * 0.1), (r(2, 256) / 16, r(2) * 0.1)]
    qpos = [(r(256, 256) / 16, r(256) * 0.1), (r(256, 256) / 16, r(256) * 0.1)]
    proj = (r(256, 256) / 16, r(256) * 0.1, 1.0 + 0.2 * r(256), 0.1 * r(256))
    dim_t = torch.arange(128, dtype=torch.float32)
    dim_t = 10000.0 ** (2 * torch.div(dim_t, 2, rounding_mode="trunc") / 128)
    return ffn, coord, qpos, proj, dim_t


# (queries, planned frames, step sizes): nq = 100 switches form at B = 9 (a plan of 13, and a plan of 8 with longer steps),
# nq = 300 inside one step of 8
TAIL_CASES = [(100, 13, (1, 8, 9, 13)), (100, 8, (8, 9, 13)), (300, 8, (1, 2, 3, 5, 8))]


@pytest.mark.gpu
@pytest.mark.parametrize("proj", [False, True])
@pytest.mark.parametrize("nq,plan,steps", TAIL_CASES)
def test_dec_tail_block_frames_are_bit_identical_across_step_sizes(nq, plan, steps, proj):
    """Through `dec_tail_block` (the block the decoder builds, with both forms) and `dec_tail(..., frames=B)` as the decoder calls it."""
    from gomatching_amd import ops
    rows = nq * P
    assert len({ops.tail_form2_wins(B * rows) for B in steps}) == 2, "the unplanned rule no longer switches inside %s" % (steps,)
    ffn, coord, qpos, pw, dim_t = _tail_weights(1024, seed=nq + plan)
    dv = lambda t: t.to(DEV)
    args = (tuple(dv(v) for v in ffn), [(dv(w), dv(b)) for w, b in coord], [(dv(w), dv(b)) for w, b in qpos], dv(dim_t))
    pwd = tuple(dv(v) for v in pw) if proj else None
    blk = ops.dec_tail_block(*args, proj_w=pwd)
    assert blk is not None and blk.form == 2 and blk.alt is not None and blk.alt.form == 1 and (blk.proj is not None) == proj
    Bmax = max(steps)
    g = torch.Generator().manual_seed(rows + Bmax)
    x, samp = dv(torch.randn((Bmax * rows, 256), generator=g)), dv(torch.randn((Bmax * rows, 256), generator=g))
    ref = dv(torch.rand((Bmax * rows, 2), generator=g))

    def run(b, B, **kw):                                    # the first B frames
        e = B * rows
        if proj:
            return ops.dec_tail(samp[:e], b, ref[:e], residual=x[:e], **kw)
        return ops.dec_tail(x[:e], b, ref[:e], **kw)

    want_form = 2 if ops.tail_form2_wins(plan * rows) else 1
    direct = ops.DecTail(*args, proj_w=pwd, form=want_form)
    with ops.step_plan(plan):
        outs = {B: run(blk, B, frames=B) for B in steps}
    torch.cuda.synchronize()
    ops.check_range_flag(DEV)
    for B in steps:
        pinned = run(direct, B)                              # the plan's form, launched directly: pins which form ran
        for u, v in zip(outs[B], pinned):
            assert torch.equal(u, v), "B=%d: not the plan's form %d" % (B, want_form)
        for u, v in zip(outs[B], outs[Bmax]):
            assert torch.equal(u, v[:B * rows]), "B=%d: a frame's rows differ from the %d-frame step's" % (B, Bmax)


# ------------------------------------------------------------------------------------------ the model
def _time_cost():
    return {k: 0.0 for k in ("pre_process", "backbone", "detector", "rescore", "tracker", "short_match",
                             "long_match", "post_process", "total_time")}


FIELDS = ("scores", "bd", "ctrl_points", "recs", "reid_features")


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["f16x3", "bf16x6"])
def test_model_frames_are_bit_identical_across_step_sizes(mode):
    """6 frames of 640x1138 at 300 queries in one step against the same frames alone: the unplanned rules pick other split counts,
    the patch kernel and the other tail form between these step sizes; under the model's plan every field is bit-identical."""
    from gomatching_amd import ops
    from gomatching_amd.config import setup_cfg
    from gomatching_amd.modeling import GoMatching
    from gomatching_amd.synth import make_clip
    from gomatching_amd.weights import synth_state_dict
    H, W, nq, n = 640, 1138, 300, 6
    diff = [name for name, cin, cout, k, s, p, oh, ow in _r50_convs(H, W)
            if len({_old_conv_choice(ops, B * oh * ow, cin, cout, k, s, p, mode, name.endswith("conv3")) for B in (1, n)}) > 1]
    assert diff, "no convolution switches between steps of 1 and %d frames at %dx%d" % (n, H, W)
    if mode == "f16x3":
        assert ops.tail_form2_wins(nq * P) != ops.tail_form2_wins(n * nq * P)
    cfg = setup_cfg(builtin="icdar15")
    cfg.MODEL.DEVICE = DEV
    cfg.MODEL.TRANSFORMER.NUM_QUERIES = nq
    sd = synth_state_dict(cfg, seed=3, cls_bias={"detection_transformer.ctrl_point_class.0.bias": 0.0})
    clip = make_clip(n, H, W, clip_id=9)
    inputs = [{"image": torch.as_tensor(f.astype("float32").transpose(2, 0, 1))} for f in clip]
    with ops.gemm_mode(mode):
        model = GoMatching(cfg, sd, device=DEV)
        assert model.frames_per_step == PLAN
        grab = lambda insts: [{k: getattr(r, k).clone() for k in FIELDS} for r in insts]
        whole = grab(model.inference(inputs, _time_cost()))
        alone = {f: grab(model.inference(inputs[f:f + 1], _time_cost()))[0] for f in (0, 4)}
    for f, one in alone.items():
        assert len(one["scores"]) > 0
        for k in FIELDS:
            assert torch.equal(whole[f][k], one[k]), "%s: frame %d's %s differs between a %d-frame step and a 1-frame step" % (
                mode, f, k, n)
