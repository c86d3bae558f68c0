"""Training from still images on the GPU: `gom_ingest_motion_u8_hwc3_to_nhwc4` (one source image, T windows of T resizes,
zero-padded, one launch) against Pillow bit for bit; the model's fourth input kind and the grouped training detector against
the host path and the CPU oracle; the geometry cache; `python -m gomatching_amd.train --image-motion` end to end."""
import json
import os

import numpy as np
import pytest
import torch
from PIL import Image

from clip_data_fixture import AUG_OPTS
from helpers import mini_cfg
from image_motion_fixture import write_stills

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MEAN, STD = [123.675, 116.28, 103.53], [58.395, 57.12, 57.375]
NAN = float("nan")


def _source(h, w, seed=0):
    img = np.random.default_rng(1000 * h + w + seed).integers(0, 256, size=(h, w, 3), dtype=np.uint8)
    img[::2] = 255                                               # every other row saturated
    return img


def _pillow(img, scaled, window):
    y0, x0, oh, ow = window
    return np.asarray(Image.fromarray(img).resize((scaled[1], scaled[0]), Image.BILINEAR))[y0:y0 + oh, x0:x0 + ow]


def _guarded(T, PH, PW, guard=1024):
    """A [T,PH,PW,4] view in the middle of a NaN-filled allocation -> (view, head guard, tail guard)."""
    n = T * PH * PW * 4
    big = torch.full((n + 2 * guard,), NAN, dtype=torch.float32, device=DEV)
    return big[guard:guard + n].view(T, PH, PW, 4), big[:guard], big[guard + n:]


# (SH, SW), (y0, x0, OH, OW): up-scale touching the right and bottom edges and filling the padded size; down-scale with many
# taps, mostly padding; identity resize; 1x1 at the last pixel
FOUR = [((74, 106), (31, 45, 43, 61)), ((7, 10), (0, 0, 7, 10)), ((37, 53), (5, 7, 32, 40)), ((61, 87), (60, 86, 1, 1))]


@pytest.mark.parametrize("flip", [False, True])
def test_ingest_motion_equals_pillow_and_writes_its_own_padding(flip):
    from gomatching_amd import ops
    img = _source(37, 53)
    out, head, tail = _guarded(4, 43, 61)
    got = ops.ingest_motion(torch.as_tensor(img).to(DEV), FOUR, MEAN, STD, flip, out=out)
    assert got.data_ptr() == out.data_ptr()
    torch.cuda.synchronize()
    assert bool(torch.isnan(head).all()) and bool(torch.isnan(tail).all())
    res = out.cpu().numpy()
    bits = res.view(np.int32)
    perm = [2, 1, 0] if flip else [0, 1, 2]
    for t, (scaled, window) in enumerate(FOUR):
        oh, ow = window[2:]
        want = (_pillow(img, scaled, window)[..., perm].astype(np.float32) - np.asarray(MEAN, np.float32)) / np.asarray(STD, np.float32)
        assert np.array_equal(res[t, :oh, :ow, :3], want), t
        assert not bits[t, :, :, 3].any(), t                                     # +0.0: all bits clear
        assert not bits[t, oh:].any() and not bits[t, :, ow:].any(), t
    assert (FOUR[0][1][2:]) == (43, 61)                                          # frame A has no zero region but channel 3


def test_ingest_motion_degenerate_shapes():
    from gomatching_amd import ops
    img = _source(45, 80)
    src = torch.as_tensor(img).to(DEV)
    whole = ((61, 109), (0, 0, 61, 109))
    one = ops.ingest_motion(src, [whole], MEAN, STD, False)                      # T = 1, the whole resized image
    assert tuple(one.shape) == (1, 61, 109, 4)
    assert torch.equal(one.view(torch.int32), ops.ingest_crop(src[None], whole[0], whole[1], MEAN, STD, False).view(torch.int32))
    desc = ((61, 109), (17, 23, 32, 40))
    many = ops.ingest_motion(src[None], [desc] * 16, MEAN, STD, True)            # T = 16 of one descriptor; [1,H,W,3] is taken too
    ref = ops.ingest_crop(src[None].expand(16, -1, -1, -1).contiguous(), desc[0], desc[1], MEAN, STD, True)
    assert tuple(many.shape) == (16, 32, 40, 4) and torch.equal(many.view(torch.int32), ref.view(torch.int32))
    small = [((61, 109), (3, 5, 12, 17)), ((20, 30), (8, 13, 12, 9)), ((45, 80), (0, 0, 5, 17))]      # PH * PW = 204 < 256
    out, head, tail = _guarded(3, 12, 17)
    ops.ingest_motion(src, small, MEAN, STD, False, out=out)
    torch.cuda.synchronize()
    assert bool(torch.isnan(head).all()) and bool(torch.isnan(tail).all())
    for t, (scaled, window) in enumerate(small):
        oh, ow = window[2:]
        ref = ops.ingest_crop(src[None], scaled, window, MEAN, STD, False)[0]
        assert torch.equal(out[t, :oh, :ow].view(torch.int32), ref.view(torch.int32)), t
        assert not out[t, oh:].view(torch.int32).any() and not out[t, :, ow:].view(torch.int32).any(), t
    with pytest.raises(ValueError, match="1..16 frames"):
        ops.ingest_motion(src, [desc] * 17, MEAN, STD, False)
    with pytest.raises(ValueError, match="out must be"):
        ops.ingest_motion(src, small, MEAN, STD, False, out=torch.empty((3, 12, 18, 4), device=DEV))


# ------------------------------------------------------------------------------- the model's fourth input kind
def _train_cfg():
    from gomatching_amd.config import merge_from_list
    cfg = mini_cfg("icdar15", device="cuda")
    merge_from_list(cfg, list(AUG_OPTS) + ["INPUT.VIDEO.TRAIN_LEN", "4"])
    cfg.MODEL.ASSO_HEAD.DROPOUT = 0.0
    return cfg


# four hand-built frames of one 96x128 source on the 96x96 motion target, (scaled_h, scaled_w, offset_y, offset_x, img_scale):
# frames 0 and 2 share the size 96x96 and are not adjacent, frames 1 and 3 are 84x96 and 60x80
HAND = [(96, 128, 0, 16, 1.0), (84, 112, 0, 8, 0.875), (96, 128, 0, 24, 1.0), (60, 80, 0, 0, 0.625)]
SIZES = [(96, 96), (84, 96), (96, 96), (60, 80)]


@pytest.fixture(scope="module")
def step(tmp_path_factory):
    """-> (cfg, state dict, model, device-ingest clip, host-ingest clip) of the hand-built motion step."""
    from gomatching_amd import data
    from gomatching_amd.modeling import GoMatching
    from gomatching_amd.synth import TRAINING_CLS_BIAS
    from gomatching_amd.weights import synth_state_dict
    cfg = _train_cfg()
    json_file, image_root = write_stills(str(tmp_path_factory.mktemp("still")))
    video = data.get_video_dataset_dicts([data.load_video_json(json_file, image_root)], gen_inst_id=True)[0]
    plan = data.MotionPlan(HAND)
    clips = [data.GoMDatasetMapper(cfg, True, device_ingest=d, image_motion=True).map_clip(video["images"] * 4, plan) for d in (True, False)]
    assert [fr["crop"][2:] for fr in clips[0]] == SIZES and [tuple(fr["image"].shape[1:]) for fr in clips[1]] == SIZES
    assert all(len(fr["instances"]["gt_instance_ids"]) == 2 for c in clips for fr in c)
    sd = synth_state_dict(cfg, seed=7, cls_bias=TRAINING_CLS_BIAS)
    model = GoMatching(cfg, sd, device=DEV)
    yield cfg, sd, model, clips[0], clips[1]
    model.close()


def test_device_and_host_motion_clips_give_the_same_input_and_loss_bits(step):
    from gomatching_amd import training
    from gomatching_amd.predictor import new_time_cost
    cfg, sd, model, dev_clip, host_clip = step
    x, hw = model.preprocess_image(dev_clip)
    y, hw_host = model.preprocess_image(host_clip)
    assert tuple(hw) == tuple(hw_host) == (96, 96) and tuple(x.shape) == (4, 96, 96, 4)
    assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    for t, (oh, ow) in enumerate(SIZES):
        assert not x[t, oh:].view(torch.int32).any() and not x[t, :, ow:].view(torch.int32).any() and x[t, :oh, :ow, :3].abs().sum() > 0
    resident = dev_clip[0]["frame_u8"].to(DEV)
    on_device = [dict(fr, frame_u8=resident) for fr in dev_clip]                 # the image already resident
    assert torch.equal(model.preprocess_image(on_device)[0], x)
    losses = [training.forward_losses(model, c) for c in (dev_clip, host_clip)]
    assert set(losses[0]) == set(losses[1]) >= {"loss_long_asso", "loss_short_asso", "loss_res"}
    for k in losses[0]:
        a, b = losses[0][k].detach().cpu(), losses[1][k].detach().cpu()
        print(k, float(a), float(b))
        assert torch.isfinite(a).all() and a.view(torch.int32).equal(b.view(torch.int32)), k
    # unflagged, the same frames are what they always were: frames that do not share a crop
    plain = [{k: v for k, v in fr.items() if k != "motion"} for fr in dev_clip]
    with pytest.raises(ValueError, match="must share"):
        model.preprocess_image(plain)
    with pytest.raises(ValueError, match="must share"):
        model.preprocess_image([{k: v for k, v in fr.items() if k != "motion"} for fr in host_clip])
    # two images in one motion step, and motion frames at inference
    other = [dict(fr) for fr in dev_clip]
    other[2]["frame_u8"] = dev_clip[2]["frame_u8"].clone()
    with pytest.raises(ValueError, match="ONE frame_u8"):
        model.preprocess_image(other)
    for clip in (dev_clip, host_clip):
        with pytest.raises(ValueError, match="training input"):
            model.inference(clip, new_time_cost())


def test_grouped_training_detector_against_the_oracle(step):
    """The step's detector part, frame by frame, against the CPU oracle run on the padded batch with per-frame masks
    (`mask_out_padding`), and the association losses of the oracle on the native proposals with their own `image_size`."""
    from gomatching_amd import training
    from oracle import gom_oracle as O
    from oracle import train_oracle as TO
    cfg, sd, model, dev_clip, host_clip = step
    ocfg = mini_cfg("icdar15")
    ocfg.MODEL.TRANSFORMER.INFERENCE_TH_TEST = model.test_score_threshold
    T = cfg.MODEL.TRANSFORMER
    nq, P = T.NUM_QUERIES, T.NUM_POINTS
    taps = []
    det = training.detect_for_training(model, model.trainable_parameters(), dev_clip, taps=taps)
    assert [g[0] for g in det["groups"]] == [(96, 96), (84, 96), (60, 80)] and [g[1] for g in det["groups"]] == [[0, 2], [1], [3]]
    assert det["sizes"] == SIZES and det["padded_hw"] == (96, 96) and len(taps) == 3
    native_topk = torch.empty((4, nq), dtype=torch.long)
    for (hw, members), tp in zip(det["groups"], taps):
        native_topk[members] = tp["topk"].view(len(members), nq).cpu().long()

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
        pts = ref["bd"].reshape(len(ref), -1, 2)                  # training proposals: no NMS, the boxes of gom_lstmatcher.py:310-318
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
        assert d_box <= tol * max(SIZES[t])                       # normalised points within tol, scaled to pixels
    # the association losses of the oracle on the NATIVE proposals, every frame under its own image_size
    frames = [{k: (v.cpu() if hasattr(v, "cpu") else v) for k, v in f.items() if k != "keep_rows"} for f in det["frames"]]
    targets = [{"image_size": SIZES[t], "gt_boxes": fr["instances"]["gt_boxes"], "gt_instance_ids": fr["instances"]["gt_instance_ids"]}
               for t, fr in enumerate(dev_clip)]
    with torch.no_grad():
        want = TO.asso_losses(osd, ocfg, frames, targets)
    got = training.asso_losses(model.trainable_parameters(), cfg, det["frames"], targets)
    for k in ("loss_long_asso", "loss_short_asso"):
        print(k, float(got[k].detach()), float(want[k]))
        assert abs(float(got[k].detach()) - float(want[k])) <= 1e-4 * max(1.0, abs(float(want[k]))), k


def _scores(out, re):
    s = out["pred_logits"].mean(-2).sigmoid().max(-1)[0]
    r = re.mean(-2).sigmoid().max(-1)[0]
    return torch.where(s > r, s, r)


def test_motion_steps_leave_the_geometry_cache_as_it_was(step):
    from gomatching_amd import data, training
    cfg, sd, model, dev_clip, host_clip = step
    training.forward_losses(model, [{k: v for k, v in dev_clip[0].items() if k != "motion"}] * 2)      # a video step: cached, as always
    before = dict(model.detection_transformer._geom)
    assert len(before) >= 1
    mapper = data.GoMDatasetMapper(cfg, True, device_ingest=True, image_motion=True)
    record = {k: dev_clip[0][k] for k in ("file_name", "height", "width", "image_id", "video_id")}
    record["annotations"] = []
    seen = set()
    for k in range(6):                                           # six steps, pairwise different sizes
        plan = data.MotionPlan([(96 - 4 * k, 128, 0, 10, 1.0), (87 - 4 * k, 112, 0, 0, 0.875)])
        clip = mapper.map_clip([record] * 2, plan)
        det = training.detect_for_training(model, model.trainable_parameters(), clip)
        seen.update(det["sizes"])
        assert not model.detection_transformer._geom_transient
    assert len(seen) == 12
    after = model.detection_transformer._geom
    assert len(after) == len(before) and all(after[k] is before[k] for k in before)


# -------------------------------------------------------------------------------------------------- the CLI
def _weights(tmp_path):
    from gomatching_amd.solver import save_checkpoint
    from gomatching_amd.synth import TRAINING_CLS_BIAS
    from gomatching_amd.weights import synth_state_dict
    return save_checkpoint(os.path.join(str(tmp_path), "deepsolo.pth"), synth_state_dict(_train_cfg(), seed=7, cls_bias=TRAINING_CLS_BIAS))


def _argv(dataset, weights, out, iters, extra=()):
    return ["--builtin", "icdar15", "--json", dataset[0], "--image-root", dataset[1], "--seed", "21", "--image-motion"] + list(extra) + \
           ["--opts", "MODEL.WEIGHTS", weights, "OUTPUT_DIR", out, "MODEL.TRANSFORMER.NUM_QUERIES", "12", "MODEL.ASSO_HEAD.DROPOUT", "0.0",
            "SOLVER.TRAIN_ITER", str(iters), "SOLVER.WARMUP_ITERS", "0", "DATALOADER.NUM_WORKERS", "2", "INPUT.VIDEO.TRAIN_LEN", "4"] + AUG_OPTS


def test_train_main_with_image_motion_trains_on_videos_and_stills_and_resumes_to_the_same_bits(tmp_path):
    from gomatching_amd import data
    from gomatching_amd import eval as gom_eval
    from gomatching_amd import train
    dataset = write_stills(os.path.join(str(tmp_path), "ds"), num_videos=1, num_stills=2)
    weights = _weights(tmp_path)
    cfg = _train_cfg()
    with data.build_vts_train_loader(cfg, data.GoMDatasetMapper(cfg, True, image_motion=True), 21,
                                     dataset_dicts=data.load_video_json(*dataset)) as ld:
        kinds = [isinstance(ld.plan(i)[2], data.MotionPlan) for i in range(6)]
    assert any(kinds[:4]) and not all(kinds[:4]) and any(kinds[4:])              # both kinds before the break, a still after it
    out = os.path.join(str(tmp_path), "run")
    assert train.main(_argv(dataset, weights, out, 6)) == 0
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
