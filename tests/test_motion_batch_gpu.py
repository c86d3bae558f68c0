"""Motion clips as ONE padded batch with per-frame valid extents.

Kernel level: every per-frame launch on B frames equals, word for word, the B calls of the existing single-extent op on that
frame alone (B = 1, that frame's vshapes / valid ratios / scale / size).  The existing ops are held to fp64 statements by the
edge tests (test_select_forms_gpu, test_msda_forms_gpu, test_ops_gpu), so bit equality with them is the whole criterion.

Model level: `detect_for_training(whole_batch=True)` against the grouped call of the same model and against the CPU oracle on
the padded batch with per-frame masks; `forward_losses`, a video clip under the flag, and the train command line."""
import json
import os

import numpy as np
import pytest
import torch

from clip_data_fixture import AUG_OPTS
from helpers import mini_cfg
from image_motion_fixture import write_stills

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# (padded size, frame sizes): the smallest pyramids that cross a 256-thread block (S = 193 / 219) and mix a full frame with
# padded ones; (8, 8) leaves Hv = Wv = 1 on the coarse levels
SETS = [((96, 96), [(96, 96), (84, 96), (96, 96), (60, 80), (8, 8)]),
        ((72, 136), [(72, 136), (33, 136), (72, 41)])]
SET_IDS = ["96x96", "72x136"]


def _ops():
    from gomatching_amd import ops
    return ops


def _bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def _same(a, b, what):
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape)
    assert torch.equal(_bits(a), _bits(b)), "%s: %d words differ" % (what, int((_bits(a) != _bits(b)).sum()))


class Pyramid:
    """Device descriptors of a shape set: shapes / lsi, per-frame vshapes [B,L,2] and valid ratios [B,L,2] as the model forms them."""

    def __init__(self, padded, sizes):
        from gomatching_amd.modeling.deepsolo import DeepSolo
        self.shapes = DeepSolo.level_shapes(*padded)
        self.sizes, self.B = sizes, len(sizes)
        ss = torch.as_tensor(self.shapes, dtype=torch.long)
        lsi = torch.cat((ss.new_zeros((1,)), ss.prod(1).cumsum(0)[:-1]))
        self.S = int(ss.prod(1).sum())
        self.ss, self.lsi = ss.to(DEV), lsi.to(DEV)
        self.fv = DeepSolo.valid_shapes_frames(self.shapes, sizes)
        self.vs = torch.as_tensor(self.fv, dtype=torch.long).to(DEV)
        vr = np.array([[[np.float32(v[1]) / np.float32(s[1]), np.float32(v[0]) / np.float32(s[0])] for v, s in zip(f, self.shapes)]
                       for f in self.fv], np.float32)
        self.vr_host = vr
        self.vr = torch.from_numpy(vr).to(DEV)
        self.full = [b for b, hw in enumerate(sizes) if tuple(hw) == tuple(padded)]
        assert self.full and len(self.full) < self.B


@pytest.fixture(scope="module", params=SETS, ids=SET_IDS)
def pyr(request):
    return Pyramid(*request.param)


def _dim_t():
    d = torch.arange(128, dtype=torch.float32)
    return (10000.0 ** (2 * torch.div(d, 2, rounding_mode="trunc") / 128)).to(DEV)


# ------------------------------------------------------------------------------------------------- kernel level
def test_geometry_tables_in_one_launch(pyr):
    ops = _ops()
    g = torch.Generator().manual_seed(pyr.S)
    dim_t, level_embed = _dim_t(), torch.randn(4, 256, generator=g).to(DEV)
    lvl_pos, ref, valid = ops.padded_geometry(dim_t, level_embed, pyr.ss, pyr.lsi, pyr.vs, pyr.B, pyr.S)
    assert tuple(lvl_pos.shape) == (pyr.B, pyr.S, 256) and tuple(ref.shape) == (pyr.B, pyr.S, 2) and tuple(valid.shape) == (pyr.B, pyr.S)
    lsi = [int(v) for v in pyr.lsi.cpu()]

    def pos_table(vshapes):
        out = torch.empty((pyr.S, 256), dtype=torch.float32, device=DEV)
        for l, (H, W) in enumerate(pyr.shapes):
            ops.pos_encoding_into(dim_t, level_embed[l], out[lsi[l]:], H, W, None if vshapes is None else vshapes[l])
        return out

    assert int(valid.sum()) > 0 and int((valid == 0).sum()) > 0
    for b in range(pyr.B):
        vs_b = pyr.vs[b].contiguous()
        _same(lvl_pos[b], pos_table(pyr.fv[b]), "lvl_pos of frame %d" % b)
        _same(ref[b], ops.encoder_reference_points(pyr.ss, pyr.lsi, pyr.S, vs_b), "enc_ref of frame %d" % b)
        _same(valid[b], ops.proposal_valid(pyr.ss, pyr.lsi, pyr.S, vs_b), "validity of frame %d" % b)
    for b in pyr.full:                                            # the frame that fills the padded size: the UNMASKED ops
        _same(lvl_pos[b], pos_table(None), "lvl_pos of full frame %d, unmasked" % b)
        _same(ref[b], ops.encoder_reference_points(pyr.ss, pyr.lsi, pyr.S), "enc_ref of full frame %d, unmasked" % b)
        _same(valid[b], ops.proposal_valid(pyr.ss, pyr.lsi, pyr.S), "validity of full frame %d, unmasked" % b)


@pytest.mark.parametrize("ld,col0,ncols", [(640, 384, 256), (1536, 0, 1536), (260, 4, 4)])
def test_zero_fill_with_frame_extents(pyr, ld, col0, ncols):
    ops = _ops()
    g = torch.Generator().manual_seed(ld + pyr.S)
    buf = (torch.rand(pyr.B * pyr.S, ld, generator=g) + 0.5).to(DEV)             # NaN-free, no zero
    got = ops.zero_padded_tokens_frames_(buf.clone(), col0, ncols, pyr.ss, pyr.lsi, pyr.vs, pyr.B, pyr.S)
    want = buf.clone()
    for b in range(pyr.B):
        ops.zero_padded_tokens_(want[b * pyr.S:(b + 1) * pyr.S], col0, ncols, pyr.ss, pyr.lsi, pyr.vs[b].contiguous(), 1, pyr.S)
    _same(got, want, "zero fill")
    touched = got != buf
    assert bool(touched.any()) and not bool(touched[:, :col0].any()) and not bool(touched[:, col0 + ncols:].any())
    for b in pyr.full:
        assert not bool(touched[b * pyr.S:(b + 1) * pyr.S].any())


@pytest.mark.parametrize("k", [1, 20, 100])
def test_topk_with_frame_validity_and_ties_across_the_boundary(pyr, k):
    ops = _ops()
    g = torch.Generator().manual_seed(k + pyr.S)
    # logits on a grid of eight values: exact ties everywhere; invalid tokens take 0.75, a grid value, so that they tie with valid ones
    logits = (torch.randint(0, 8, (pyr.B * pyr.S, 3), generator=g).float() / 4.0).to(DEV)
    invalid_logit = torch.tensor([0.75], device=DEV)
    valid = torch.stack([ops.proposal_valid(pyr.ss, pyr.lsi, pyr.S, pyr.vs[b].contiguous()) for b in range(pyr.B)])
    idx, rows = ops.topk_tokens(logits, pyr.B, pyr.S, k, invalid_logit=invalid_logit, with_rows=True, frame_valid=valid)
    among_invalid = 0
    for b in range(pyr.B):
        i1, r1 = ops.topk_tokens(logits[b * pyr.S:(b + 1) * pyr.S], 1, pyr.S, k, valid=valid[b].contiguous(),
                                 invalid_logit=invalid_logit, with_rows=True)
        _same(idx[b:b + 1], i1, "top-k of frame %d" % b)
        _same(rows[b:b + 1], r1 + b * pyr.S, "top-k rows of frame %d" % b)
        among_invalid += int((valid[b][idx[b].long()] == 0).sum())
    if k == 100:
        assert among_invalid > 0                                  # the substituted logit does compete
    same_for_all = ops.topk_tokens(logits, pyr.B, pyr.S, k, valid=valid[0].contiguous(), invalid_logit=invalid_logit)
    _same(same_for_all, ops.topk_tokens(logits, pyr.B, pyr.S, k, invalid_logit=invalid_logit,
                                        frame_valid=valid[0:1].expand(pyr.B, -1).contiguous()), "one row for the batch")


@pytest.mark.parametrize("compact", [True, False])
def test_bezier_reference_points_with_frame_extents(pyr, compact):
    ops = _ops()
    nq, P = 23, 25
    g = torch.Generator().manual_seed(nq + pyr.S)
    topk = torch.randint(0, pyr.S, (pyr.B, nq), generator=g).int()
    topk[:, 0], topk[:, 1] = 0, pyr.S - 1
    topk = topk.to(DEV)
    coord = torch.randn(pyr.B * (nq if compact else pyr.S), 8, generator=g).to(DEV)
    ts = torch.linspace(0, 1, P)
    bern = torch.stack([(1 - ts) ** 3, 3 * ts * (1 - ts) ** 2, 3 * ts ** 2 * (1 - ts), ts ** 3], 1).contiguous().to(DEV)
    got = ops.bezier_reference_points(coord, topk, pyr.ss, pyr.lsi, bern, pyr.B, pyr.S, nq, P, compact=compact, frame_vshapes=pyr.vs)
    n = nq if compact else pyr.S
    for b in range(pyr.B):
        args = (coord[b * n:(b + 1) * n], topk[b:b + 1].contiguous(), pyr.ss, pyr.lsi, bern, 1, pyr.S, nq, P)
        _same(got[b:b + 1], ops.bezier_reference_points(*args, compact=compact, vshapes=pyr.vs[b].contiguous()), "frame %d" % b)
        if b in pyr.full:
            _same(got[b:b + 1], ops.bezier_reference_points(*args, compact=compact), "full frame %d, unmasked" % b)


def test_scale_xy_and_ref_update_with_frame_scales(pyr):
    ops = _ops()
    ppf = 7 * 25                                                  # points per frame: no multiple of the 4 points of a block
    Q = pyr.B * ppf
    g = torch.Generator().manual_seed(Q)
    scales = pyr.vr[:, 0].contiguous()                            # level 0's (Wv/W, Hv/H) per frame, as the decoder passes them
    x = torch.randn(Q, 2, generator=g).to(DEV)
    got = ops.scale_xy_frames_(x.clone(), scales)
    for b in range(pyr.B):
        sx, sy = (float(v) for v in pyr.vr_host[b, 0])
        _same(got[b * ppf:(b + 1) * ppf], ops.scale_xy_(x[b * ppf:(b + 1) * ppf].clone(), sx, sy), "scale_xy of frame %d" % b)
    h = torch.randn(Q, 256, generator=g).to(DEV)
    last = ((torch.randn(2, 256, generator=g) * 0.05).to(DEV), torch.randn(2, generator=g).to(DEV))
    ref = torch.rand(Q, 2, generator=g).to(DEV)
    ref[0, 0], ref[1, 1] = 0.0, 1.0                                # the clamps of inverse_sigmoid
    dim_t = _dim_t()
    new_ref, pos = ops.ref_update(h, last, ref, dim_t, frame_scales=scales)
    only_ref, none = ops.ref_update(h, last, ref, dim_t, frame_scales=scales, want_pos=False)
    assert none is None
    _same(only_ref, new_ref, "ref_update without the embedding")
    for b in range(pyr.B):
        sl = slice(b * ppf, (b + 1) * ppf)
        r1, p1 = ops.ref_update(h[sl], last, ref[sl].contiguous(), dim_t, scale=tuple(float(v) for v in pyr.vr_host[b, 0]))
        _same(new_ref[sl], r1, "refined points of frame %d" % b)
        _same(pos[sl], p1, "point embedding of frame %d" % b)
    for b in pyr.full:
        sl = slice(b * ppf, (b + 1) * ppf)
        _same(pos[sl], ops.ref_update(h[sl], last, ref[sl].contiguous(), dim_t)[1], "point embedding of full frame %d, unscaled" % b)


def test_detect_post_with_frame_sizes(pyr):
    ops = _ops()
    nq, P = 37, 25
    B = pyr.B
    g = torch.Generator().manual_seed(nq + pyr.S)
    n = B * nq * P
    cls = (torch.randn(B * nq, 1, 1, generator=g) * 1.5 + torch.randn(B * nq, P, 1, generator=g) * 0.3).reshape(n, 1).to(DEV)
    recls = (torch.randn(B * nq, 1, 1, generator=g) * 1.5 + torch.randn(B * nq, P, 1, generator=g) * 0.3).reshape(n, 1).to(DEV)
    centre = torch.rand(B * nq, 1, 2, generator=g) * 0.8 + 0.1
    ctrl = (centre + torch.randn(B * nq, P, 2, generator=g) * 0.04).clamp(0, 1).reshape(n, 2).contiguous().to(DEV)
    bd = (centre.repeat(1, 1, 2) + torch.randn(B * nq, P, 4, generator=g) * 0.04).clamp(0, 1).reshape(n, 4).contiguous().to(DEV)
    recs = torch.randint(0, 37, (n,), generator=g).int().to(DEV)
    sizes = torch.tensor(pyr.sizes, dtype=torch.float32).to(DEV)
    thr = (0.4, 0.3, 0.45)
    got = ops.detect_post(cls, recls, ctrl, bd, recs, B, nq, P, None, None, *thr, frame_sizes=sizes)
    counts = got["count"].cpu().tolist()
    assert 0 < min(counts) and max(counts) < nq, counts           # the thresholds and the NMS both drop some and keep some
    for b in range(B):
        sl = slice(b * nq * P, (b + 1) * nq * P)
        one = ops.detect_post(cls[sl], recls[sl], ctrl[sl], bd[sl], recs[sl], 1, nq, P, pyr.sizes[b][0], pyr.sizes[b][1], *thr)
        assert int(one["count"][0]) == counts[b]
        keep = one["keep_idx"].clone()
        keep[0, :counts[b]] += b * nq
        _same(got["keep_idx"][b:b + 1], keep, "keep_idx of frame %d" % b)
        for k in ("scores", "boxes", "ctrl", "bd", "recs"):
            _same(got[k][b:b + 1], one[k], "%s of frame %d" % (k, b))


def _msda_inputs(pyr, Lq, ref, seed):
    """raw [B*Lq, 384]: offsets (pixels of the sampled level) of five kinds -- zero (the sample sits on its reference point), a few
    pixels, across the frame's valid extent, far outside the map, sub-pixel -- and logits over a wide range."""
    g = torch.Generator().manual_seed(seed)
    Q = pyr.B * Lq
    off = torch.randn(Q, 8, 4, 4, 2, generator=g) * 3.0
    kind = torch.randint(0, 5, (Q, 8, 4, 4, 1), generator=g)
    span = torch.tensor([[w, h] for h, w in pyr.shapes], dtype=torch.float32).view(1, 1, 4, 1, 2)
    sign = torch.randint(0, 2, off.shape, generator=g).float() * 2 - 1
    off = torch.where(kind == 0, torch.zeros_like(off), off)
    off = torch.where(kind == 2, sign * span * torch.rand(off.shape, generator=g), off)
    off = torch.where(kind == 3, sign * (span + 50.0), off)
    off = torch.where(kind == 4, torch.rand(off.shape, generator=g) - 0.5, off)
    raw = torch.cat([off.reshape(Q, 256), torch.randn(Q, 128, generator=g) * 3.0], 1).contiguous()
    return raw.to(DEV), ref.reshape(Q, 2).contiguous().to(DEV)


class _Lanes:
    """ops.MSDA_LANES set for the block, restored after (the switch of tests/test_msda_forms_gpu.py)."""

    def __init__(self, on):
        self.on = on

    def __enter__(self):
        self.ops = _ops()
        self.old = self.ops.MSDA_LANES
        self.ops.MSDA_LANES = self.on

    def __exit__(self, *a):
        self.ops.MSDA_LANES = self.old


@pytest.mark.parametrize("kind", ["encoder", "decoder"])
def test_msda_with_frame_valid_ratios(pyr, kind):
    ops = _ops()
    B, S = pyr.B, pyr.S
    g = torch.Generator().manual_seed(S + len(kind))
    if kind == "encoder":                                         # Lq = S, the tokens' own (masked) positions, value at column 384 of 640
        Lq, ld, col = S, 640, 384
        ref = torch.stack([ops.encoder_reference_points(pyr.ss, pyr.lsi, S, pyr.vs[b].contiguous()) for b in range(B)]).cpu()
    else:                                                         # Lq = 7 queries x 25 points, value = one slice of the [., 1536] buffer
        Lq, ld, col = 7 * 25, 1536, 256
        ref = torch.rand(B, Lq, 2, generator=g) * 1.2 - 0.1
        for b in range(B):                                        # ... some exactly on the last valid pixel of level 0, and past it
            Hv, Wv = pyr.fv[b][0]
            ref[b, 0] = torch.tensor([(Wv - 0.5) / Wv, (Hv - 0.5) / Hv])
            ref[b, 1] = torch.tensor([(Wv + 0.5) / Wv, (Hv + 0.5) / Hv])
            ref[b, 2] = torch.tensor([1.0, 1.0])
    raw, ref = _msda_inputs(pyr, Lq, ref, S + Lq)
    value = torch.randn(B * S, ld, generator=g).to(DEV)
    v2d = value[:, col:col + 256]
    outs = {}
    for lanes in (True, False):
        with _Lanes(lanes):
            got = ops.msda_fused(raw, ref, v2d, S * ld, pyr.ss, pyr.lsi, B, Lq, frame_valid_ratios=pyr.vr)
            for b in range(B):
                one = ops.msda_fused(raw[b * Lq:(b + 1) * Lq], ref[b * Lq:(b + 1) * Lq], v2d[b * S:(b + 1) * S], S * ld, pyr.ss, pyr.lsi,
                                     1, Lq, pyr.vr[b].contiguous())
                _same(got[b * Lq:(b + 1) * Lq], one, "%s, lanes %s, frame %d" % (kind, lanes, b))
            for b in pyr.full:                                    # ratio 1.0 through the same kernel: the unpadded kernel's bits
                plain = ops.msda_fused(raw[b * Lq:(b + 1) * Lq], ref[b * Lq:(b + 1) * Lq], v2d[b * S:(b + 1) * S], S * ld, pyr.ss,
                                       pyr.lsi, 1, Lq)
                _same(got[b * Lq:(b + 1) * Lq], plain, "%s, lanes %s, full frame %d against the unpadded kernel" % (kind, lanes, b))
            # the existing entry with ONE table equals the new entry fed that table B times
            table = pyr.vr[B - 1].contiguous()
            _same(ops.msda_fused(raw, ref, v2d, S * ld, pyr.ss, pyr.lsi, B, Lq, table),
                  ops.msda_fused(raw, ref, v2d, S * ld, pyr.ss, pyr.lsi, B, Lq, frame_valid_ratios=table[None].expand(B, -1, -1).contiguous()),
                  "%s, lanes %s, one table repeated" % (kind, lanes))
            outs[lanes] = got
    _same(outs[True], outs[False], "the two launch forms")
    assert bool(torch.isfinite(outs[True]).all()) and float(outs[True].abs().max()) > 0


def test_wrappers_refuse_descriptors_of_another_batch_size(pyr):
    ops = _ops()
    from gomatching_amd.lib import GomError
    B, S = pyr.B, pyr.S
    short_vs, short_vr = pyr.vs[:B - 1].contiguous(), pyr.vr[:B - 1].contiguous()
    buf = torch.ones(B * S, 256, device=DEV)
    with pytest.raises(GomError, match="frame_vshapes"):
        ops.zero_padded_tokens_frames_(buf, 0, 256, pyr.ss, pyr.lsi, short_vs, B, S)
    with pytest.raises(GomError, match="frame_vshapes"):
        ops.padded_geometry(_dim_t(), torch.zeros(4, 256, device=DEV), pyr.ss, pyr.lsi, short_vs, B, S)
    with pytest.raises(GomError, match="frame_valid_ratios"):
        ops.msda_fused(torch.zeros(B * 4, 384, device=DEV), torch.zeros(B * 4, 2, device=DEV), buf, S * 256, pyr.ss, pyr.lsi, B, 4,
                       frame_valid_ratios=short_vr)
    with pytest.raises(GomError, match="frame_valid"):
        ops.topk_tokens(buf, B, S, 4, frame_valid=torch.ones(B - 1, S, dtype=torch.uint8, device=DEV))
    with pytest.raises(GomError, match="frame_vshapes"):
        ops.bezier_reference_points(torch.zeros(B * 4, 8, device=DEV), torch.zeros(B, 4, dtype=torch.int32, device=DEV), pyr.ss, pyr.lsi,
                                    torch.zeros(25, 4, device=DEV), B, S, 4, 25, compact=True, frame_vshapes=short_vs)
    with pytest.raises(GomError, match="frame_sizes"):
        z = torch.zeros(B * 4 * 25, 4, device=DEV)
        ops.detect_post(z[:, :1], None, z[:, :2].contiguous(), z, torch.zeros(B * 100, dtype=torch.int32, device=DEV), B, 4, 25, None,
                        None, 0.5, 0.5, 0.5, frame_sizes=torch.ones(B - 1, 2, device=DEV))
    with pytest.raises(GomError, match="frame_scales"):
        ops.scale_xy_frames_(torch.zeros(B * 10, 2, device=DEV), torch.ones(B + 1, 2, device=DEV))
    assert bool((buf == 1).all())                                 # nothing was launched


# -------------------------------------------------------------------------------------------------- model level
def _train_cfg():
    from gomatching_amd.config import merge_from_list
    cfg = mini_cfg("icdar15", device="cuda")
    merge_from_list(cfg, list(AUG_OPTS) + ["INPUT.VIDEO.TRAIN_LEN", "4"])
    cfg.MODEL.ASSO_HEAD.DROPOUT = 0.0
    return cfg


# the hand-made step of tests/test_image_motion_gpu.py: four frames of one 96x128 source on the 96x96 motion target
HAND = [(96, 128, 0, 16, 1.0), (84, 112, 0, 8, 0.875), (96, 128, 0, 24, 1.0), (60, 80, 0, 0, 0.625)]
SIZES = [(96, 96), (84, 96), (96, 96), (60, 80)]


@pytest.fixture(scope="module")
def step(tmp_path_factory):
    """-> {cfg, sd, model, dev_clip, host_clip, grouped, whole, taps}: the hand-built motion step, its grouped detector result and
    its whole-batch one (each computed once and left unchanged)."""
    from gomatching_amd import data, training
    from gomatching_amd.modeling import GoMatching
    from gomatching_amd.synth import TRAINING_CLS_BIAS
    from gomatching_amd.weights import synth_state_dict
    cfg = _train_cfg()
    json_file, image_root = write_stills(str(tmp_path_factory.mktemp("still")))
    video = data.get_video_dataset_dicts([data.load_video_json(json_file, image_root)], gen_inst_id=True)[0]
    plan = data.MotionPlan(HAND)
    clips = [data.GoMDatasetMapper(cfg, True, device_ingest=d, image_motion=True).map_clip(video["images"] * 4, plan) for d in (True, False)]
    assert [fr["crop"][2:] for fr in clips[0]] == SIZES
    sd = synth_state_dict(cfg, seed=7, cls_bias=TRAINING_CLS_BIAS)
    model = GoMatching(cfg, sd, device=DEV)
    gtaps, wtaps = [], []
    grouped = training.detect_for_training(model, model.trainable_parameters(), clips[0], taps=gtaps)
    whole = training.detect_for_training(model, model.trainable_parameters(), clips[0], taps=wtaps, whole_batch=True)
    yield {"cfg": cfg, "sd": sd, "model": model, "dev_clip": clips[0], "host_clip": clips[1], "grouped": grouped, "whole": whole,
           "gtaps": gtaps, "wtaps": wtaps}
    model.close()


def test_whole_batch_detector_against_the_grouped_one(step):
    T = step["cfg"].MODEL.TRANSFORMER
    nq = T.NUM_QUERIES
    g, w = step["grouped"], step["whole"]
    assert len(g["groups"]) == 3 and len(step["gtaps"]) == 3                       # the grouped path is what it was
    assert w["groups"] == [((96, 96), [0, 1, 2, 3])] and len(step["wtaps"]) == 1
    assert w["sizes"] == g["sizes"] == SIZES and w["padded_hw"] == g["padded_hw"] == (96, 96)
    geo = step["wtaps"][0]["geo"]
    assert geo["frames"] and tuple(geo["vr0"].shape) == (4, 2) and not geo["pos_periodic"] and tuple(geo["pos_w"][0].shape) == (4 * geo["S"], 384)
    g_topk = torch.empty((4, nq), dtype=torch.long)
    for (hw, members), tp in zip(g["groups"], step["gtaps"]):
        g_topk[members] = tp["topk"].view(len(members), nq).cpu().long()
    w_topk = step["wtaps"][0]["topk"].view(4, nq).cpu().long()
    tol = 2e-4
    worst, equal = {}, True
    for t in range(4):
        assert sorted(w_topk[t].tolist()) == sorted(g_topk[t].tolist()), t           # the same top-k SET
        a, b = g["frames"][t], w["frames"][t]
        assert tuple(b["image_size"]) == tuple(a["image_size"]) == SIZES[t]
        ra, rb = a["keep_rows"].cpu(), b["keep_rows"].cpu()
        assert sorted(ra.tolist()) == sorted(rb.tolist()) and len(ra) > 0, t
        oa, ob = torch.argsort(ra), torch.argsort(rb)
        d = {"query_features": (g["query_features"][t] - w["query_features"][t]).abs().max(),
             "pred_ctrl_points": (g["pred_ctrl_points"][t] - w["pred_ctrl_points"][t]).abs().max(),
             "objectness_logits": (a["objectness_logits"].cpu()[oa] - b["objectness_logits"].cpu()[ob]).abs().max(),
             "kept query_features": (a["query_features"].cpu()[oa] - b["query_features"].cpu()[ob]).abs().max(),
             "proposal_boxes / max(size)": (a["proposal_boxes"].cpu()[oa] - b["proposal_boxes"].cpu()[ob]).abs().max() / max(SIZES[t])}
        for k, v in d.items():
            worst[k] = max(worst.get(k, 0.0), float(v))
            assert float(v) <= tol, (t, k, float(v))
        equal = equal and torch.equal(w_topk[t], g_topk[t]) and torch.equal(_bits(g["query_features"][t]), _bits(w["query_features"][t])) \
            and torch.equal(_bits(g["pred_ctrl_points"][t]), _bits(w["pred_ctrl_points"][t]))
    print("whole batch against grouped, maxima over the four frames: %s; bit-equal: %s"
          % (", ".join("%s %.3g" % kv for kv in worst.items()), equal))


def _scores(out, re):
    s = out["pred_logits"].mean(-2).sigmoid().max(-1)[0]
    r = re.mean(-2).sigmoid().max(-1)[0]
    return torch.where(s > r, s, r)


def test_whole_batch_detector_against_the_oracle(step):
    """`test_grouped_training_detector_against_the_oracle` on the whole-batch result: the CPU oracle on the padded batch with
    per-frame masks, the same tolerance, the same allowance for near-tie top-k reordering (same winners)."""
    from gomatching_amd import training
    from oracle import gom_oracle as O
    from oracle import train_oracle as TO
    cfg, sd, model, dev_clip, host_clip = (step[k] for k in ("cfg", "sd", "model", "dev_clip", "host_clip"))
    ocfg = mini_cfg("icdar15")
    ocfg.MODEL.TRANSFORMER.INFERENCE_TH_TEST = model.test_score_threshold
    T = cfg.MODEL.TRANSFORMER
    nq = T.NUM_QUERIES
    det = step["whole"]
    native_topk = step["wtaps"][0]["topk"].view(4, nq).cpu().long()
    osd = {k: torch.as_tensor(v).float() for k, v in sd.items()}
    mean, std = torch.tensor(ocfg.MODEL.PIXEL_MEAN).view(3, 1, 1), torch.tensor(ocfg.MODEL.PIXEL_STD).view(3, 1, 1)
    x = torch.zeros((4, 3, 96, 96))
    for t, fr in enumerate(host_clip):
        oh, ow = SIZES[t]
        x[t, :, :oh, :ow] = (fr["image"].float() - mean) / std
    with torch.no_grad():
        feats = O.resnet50(x, osd)
        feats = [feats[k] for k in ("res3", "res4", "res5")]
        masks = O.mask_out_padding([f.shape for f in feats], SIZES)
        pos = [O.pos_encoding_2d(m, T.HIDDEN_DIM // 2, T.TEMPERATURE) for m in masks]
        otaps = {}
        out = O.deepsolo_forward(osd, ocfg, feats, masks, pos, taps=otaps)
        moved = [t for t in range(4) if not torch.equal(otaps["topk"][t], native_topk[t])]
        print("frames whose top-k order parts from the oracle's: %d of 4 %s" % (len(moved), moved))
        if moved:
            for t in moved:                                      # near-ties only: the same WINNERS, in another order
                assert sorted(otaps["topk"][t].tolist()) == sorted(native_topk[t].tolist()), t
            out = O.deepsolo_forward(osd, ocfg, feats, masks, pos, topk_override=native_topk)
        re = O.linear(out["query_features"], osd, "roi_heads.rescoring_head")
        odet = O.detection(ocfg, out, re, SIZES)
    tol = 2e-4
    for t in range(4):
        nat, ref = det["frames"][t], odet[t]
        pts = ref["bd"].reshape(len(ref), -1, 2)
        ref_boxes = torch.cat([pts[:, :, 0].min(-1)[0][:, None], pts[:, :, 1].min(-1)[0][:, None],
                               pts[:, :, 0].max(-1)[0][:, None], pts[:, :, 1].max(-1)[0][:, None]], -1)
        rows = nat["keep_rows"].cpu()
        sel = (_scores(out, re)[t] > ocfg.MODEL.TRANSFORMER.INFERENCE_TH_TEST).nonzero().flatten()
        assert sorted(rows.tolist()) == sel.tolist() and len(sel) > 0, (t, rows.tolist(), sel.tolist())
        order = torch.argsort(rows)
        assert tuple(nat["image_size"]) == SIZES[t]
        d_box = float((nat["proposal_boxes"].cpu()[order] - ref_boxes).abs().max())
        d_sc = float((nat["objectness_logits"].cpu()[order] - ref["scores"]).abs().max())
        d_qf = float((nat["query_features"].cpu()[order] - ref["query_features"]).abs().max())
        d_all = float((det["query_features"][t].cpu() - out["query_features"][t]).abs().max())
        d_pts = float((det["pred_ctrl_points"][t].cpu() - out["pred_ctrl_points"][t]).abs().max())
        print("frame %d %s: %d proposals, max|d| boxes %.3g px, scores %.3g, query features %.3g (all queries %.3g), ctrl points %.3g"
              % (t, SIZES[t], len(sel), d_box, d_sc, d_qf, d_all, d_pts))
        assert d_sc <= tol and d_qf <= tol and d_all <= tol and d_pts <= tol
        assert d_box <= tol * max(SIZES[t])
    frames = [{k: (v.cpu() if hasattr(v, "cpu") else v) for k, v in f.items() if k != "keep_rows"} for f in det["frames"]]
    targets = [{"image_size": SIZES[t], "gt_boxes": fr["instances"]["gt_boxes"], "gt_instance_ids": fr["instances"]["gt_instance_ids"]}
               for t, fr in enumerate(dev_clip)]
    with torch.no_grad():
        want = TO.asso_losses(osd, ocfg, frames, targets)
    got = training.asso_losses(model.trainable_parameters(), cfg, det["frames"], targets)
    for k in ("loss_long_asso", "loss_short_asso"):
        print(k, float(got[k].detach()), float(want[k]))
        assert abs(float(got[k].detach()) - float(want[k])) <= 1e-4 * max(1.0, abs(float(want[k]))), k


def test_forward_losses_under_whole_batch(step):
    from gomatching_amd import training
    model, dev_clip, host_clip = step["model"], step["dev_clip"], step["host_clip"]
    tr = model.detection_transformer
    training.forward_losses(model, [{k: v for k, v in dev_clip[0].items() if k != "motion"}] * 2)      # a video step: cached, as always
    before = dict(tr._geom)
    assert len(before) >= 1
    grouped = training.forward_losses(model, dev_clip)
    losses = [training.forward_losses(model, c, motion_whole_batch=True) for c in (dev_clip, host_clip)]
    assert set(losses[0]) == set(losses[1]) == set(grouped) >= {"loss_long_asso", "loss_short_asso", "loss_res"}
    for k in losses[0]:
        a, b = losses[0][k].detach().cpu(), losses[1][k].detach().cpu()
        print(k, "whole", float(a), "host ingest", float(b), "grouped", float(grouped[k].detach()))
        assert torch.isfinite(a).all() and a.view(torch.int32).equal(b.view(torch.int32)), k
    after = tr._geom
    assert not tr._geom_transient and len(after) == len(before) and all(after[k] is before[k] for k in before)
    # the model attribute the Trainer and the META_ARCH wrapper set is what None reads
    model.motion_whole_batch = True
    try:
        again = training.forward_losses(model, dev_clip)
    finally:
        model.motion_whole_batch = False
    for k in again:
        assert again[k].detach().cpu().view(torch.int32).equal(losses[0][k].detach().cpu().view(torch.int32)), k


def test_a_video_clip_is_untouched_by_the_flag(step):
    from gomatching_amd import training
    model, dev_clip = step["model"], step["dev_clip"]
    video = [{k: v for k, v in dev_clip[0].items() if k != "motion"}] * 3
    params = model.trainable_parameters()
    a = training.detect_for_training(model, params, video)
    b = training.detect_for_training(model, params, video, whole_batch=True)
    assert a["groups"] == b["groups"] and len(b["groups"]) == 1 and a["sizes"] == b["sizes"] and a["padded_hw"] == b["padded_hw"]
    _same(a["query_features"], b["query_features"], "query features")
    _same(a["pred_ctrl_points"], b["pred_ctrl_points"], "ctrl points")
    for fa, fb in zip(a["frames"], b["frames"]):
        assert fa["image_size"] == fb["image_size"]
        for k in ("proposal_boxes", "objectness_logits", "query_features", "keep_rows"):
            _same(fa[k], fb[k], k)


def test_frames_with_an_empty_level_and_exclusive_arguments_are_refused(step):
    tr = step["model"].detection_transformer
    shapes = tr.level_shapes(96, 96)
    with pytest.raises(ValueError, match="a level has no valid token"):
        tr.geometry_frames(shapes, [(96, 96), (0, 96)])
    feats = [torch.zeros((2, h, w, 8), device=DEV) for h, w in shapes[:3]]
    with pytest.raises(ValueError, match="exclusive"):
        tr.forward(feats, image_hw=(96, 96), image_sizes=[(96, 96), (84, 96)])
    with pytest.raises(ValueError, match="2 frames"):
        tr.forward(feats, image_sizes=[(96, 96)])


# -------------------------------------------------------------------------------------------------- the CLI
def _weights(tmp_path):
    from gomatching_amd.solver import save_checkpoint
    from gomatching_amd.synth import TRAINING_CLS_BIAS
    from gomatching_amd.weights import synth_state_dict
    return save_checkpoint(os.path.join(str(tmp_path), "deepsolo.pth"), synth_state_dict(_train_cfg(), seed=7, cls_bias=TRAINING_CLS_BIAS))


def _argv(dataset, weights, out, iters, extra=()):
    return ["--builtin", "icdar15", "--json", dataset[0], "--image-root", dataset[1], "--seed", "21", "--image-motion",
            "--motion-batch", "whole"] + list(extra) + \
           ["--opts", "MODEL.WEIGHTS", weights, "OUTPUT_DIR", out, "MODEL.TRANSFORMER.NUM_QUERIES", "12", "MODEL.ASSO_HEAD.DROPOUT", "0.0",
            "SOLVER.TRAIN_ITER", str(iters), "SOLVER.WARMUP_ITERS", "0", "DATALOADER.NUM_WORKERS", "2", "INPUT.VIDEO.TRAIN_LEN", "4"] + AUG_OPTS


def test_train_main_with_motion_batch_whole_trains_and_resumes_to_the_same_bits(tmp_path, monkeypatch):
    from gomatching_amd import eval as gom_eval
    from gomatching_amd import train, training
    dataset = write_stills(os.path.join(str(tmp_path), "ds"), num_videos=1, num_stills=2)       # videos and stills: the existing CLI test's
    weights = _weights(tmp_path)
    seen = []
    real = training.detect_for_training

    def spy(*a, **kw):
        det = real(*a, **kw)
        seen.append((bool(kw.get("whole_batch")), len(det["groups"]), len(set(det["sizes"]))))
        return det

    monkeypatch.setattr(training, "detect_for_training", spy)
    out = os.path.join(str(tmp_path), "run")
    assert train.main(_argv(dataset, weights, out, 6)) == 0
    assert len(seen) == 6 and all(s[0] and s[1] == 1 for s in seen)                  # the flag arrived; one group per step
    assert any(s[2] > 1 for s in seen) and any(s[2] == 1 for s in seen)              # stills (several sizes) and videos (one)
    final = gom_eval.load_weights(os.path.join(out, "model_final.pth"))
    start = gom_eval.load_weights(weights)
    assert not torch.equal(final["roi_heads.asso_head.fc1.weight"], torch.as_tensor(start["roi_heads.asso_head.fc1.weight"]))
    with open(os.path.join(out, "metrics.json")) as f:
        lines = [json.loads(line) for line in f]
    assert len(lines) == 1 and lines[0]["iteration"] == 6
    assert {"loss_long_asso", "loss_short_asso", "loss_res", "total_loss"} <= set(lines[0]) and all(np.isfinite(v) for v in lines[0].values())
    out2 = os.path.join(str(tmp_path), "run2")
    assert train.main(_argv(dataset, weights, out2, 4)) == 0
    assert os.path.isfile(os.path.join(out2, "last_checkpoint"))
    assert train.main(_argv(dataset, weights, out2, 6, extra=["--resume"])) == 0
    resumed = gom_eval.load_weights(os.path.join(out2, "model_final.pth"))
    for k, v in final.items():
        if k.startswith("roi_heads."):
            assert v.dtype == resumed[k].dtype and torch.equal(v.view(torch.int32), resumed[k].view(torch.int32)), k
