"""The training augmentation on the GPU: `gom_resize_crop_bilinear_u8_hwc3` / `gom_ingest_crop_u8_hwc3_to_nhwc4` (one launch
per clip, csrc/ingest.hip) against Pillow's resize followed by the slice -- bit-exact, integer work -- the model's third
input kind against the host path through `training.forward_losses`, and `python -m gomatching_amd.train` end to end."""
import json
import os

import numpy as np
import pytest
import torch
from PIL import Image

from clip_data_fixture import AUG_OPTS, write_dataset
from helpers import mini_cfg

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MEAN, STD = [123.675, 116.28, 103.53], [58.395, 57.12, 57.375]

# (source h, w), (SH, SW), (y0, x0, OH, OW)
CASES = {
    "upscale 2, window touching the right and bottom edges": ((37, 53), (74, 106), (31, 45, 43, 61)),
    "downscale ~10 (21 taps), whole image": ((72, 128), (7, 12), (0, 0, 7, 12)),
    "1x1 at the last pixel": ((45, 80), (61, 109), (60, 108, 1, 1)),
    "32x40 at an odd offset": ((45, 80), (61, 109), (17, 23, 32, 40)),
    "more than one block per frame, window in the middle": ((45, 80), (61, 109), (1, 3, 59, 101)),
}


def _frames(src):
    g = np.random.default_rng(src[0] * 1000 + src[1])
    frames = g.integers(0, 256, size=(3,) + src + (3,), dtype=np.uint8)
    frames[1, ::2] = 255                                          # three distinct frames, one of them saturating
    return frames


def _pillow(frames, scaled, window):
    y0, x0, oh, ow = window
    return np.stack([np.asarray(Image.fromarray(f).resize((scaled[1], scaled[0]), Image.BILINEAR))[y0:y0 + oh, x0:x0 + ow] for f in frames])


@pytest.mark.parametrize("name", list(CASES))
def test_resize_crop_u8_equals_pillow_resize_then_slice(name):
    from gomatching_amd import ops
    src, scaled, window = CASES[name]
    frames = _frames(src)
    want = _pillow(frames, scaled, window)
    assert want.shape == (3,) + window[2:] + (3,)
    dev = torch.as_tensor(frames).to(DEV)
    out = ops.resize_crop_u8(dev, scaled, window).cpu().numpy()
    flipped = ops.resize_crop_u8(dev, scaled, window, flip=True).cpu().numpy()
    assert out.dtype == np.uint8 and np.array_equal(out, want)
    assert np.array_equal(flipped, want[..., ::-1])


def test_whole_window_equals_resize_u8():
    from gomatching_amd import ops
    frames = torch.as_tensor(_frames((45, 80))).to(DEV)
    for flip in (False, True):
        assert torch.equal(ops.resize_crop_u8(frames, (61, 109), (0, 0, 61, 109), flip=flip), ops.resize_u8(frames, 61, 109, flip=flip))


@pytest.mark.parametrize("name", list(CASES))
@pytest.mark.parametrize("flip", [False, True])
def test_ingest_crop_equals_the_two_fp32_operations_on_the_pillow_crop(name, flip):
    from gomatching_amd import ops
    src, scaled, window = CASES[name]
    frames = _frames(src)
    crop = _pillow(frames, scaled, window)
    perm = [2, 1, 0] if flip else [0, 1, 2]
    want = (crop[..., perm].astype(np.float32) - np.asarray(MEAN, np.float32)) / np.asarray(STD, np.float32)
    out = ops.ingest_crop(torch.as_tensor(frames).to(DEV), scaled, window, MEAN, STD, flip).cpu().numpy()
    assert out.dtype == np.float32 and out.shape == (3,) + window[2:] + (4,)
    assert np.array_equal(out[..., :3], want)
    assert not out[..., 3].any()
    if window == (0, 0) + scaled:
        assert np.array_equal(out, ops.ingest(torch.as_tensor(frames).to(DEV), scaled[0], scaled[1], MEAN, STD, flip).cpu().numpy())


def test_crop_tables_are_bounded_and_leave_the_resize_cache_alone():
    from gomatching_amd import ops
    frames = torch.as_tensor(_frames((45, 80))).to(DEV)
    before = dict(ops._resample_tables)
    first = ops.resize_crop_u8(frames, (50, 90), (1, 1, 8, 8)).cpu()
    for k in range(2 * ops.CROP_TABLES_MAX):                     # a new size every clip, as random scales give
        ops.resize_crop_u8(frames, (51 + k, 91 + k), (1, 1, 8, 8))
    assert len(ops._crop_tables) <= ops.CROP_TABLES_MAX and dict(ops._resample_tables) == before
    assert torch.equal(ops.resize_crop_u8(frames, (50, 90), (1, 1, 8, 8)).cpu(), first)       # evicted and rebuilt: the same bits


# ------------------------------------------------------------------------------- the model's third input kind
def _train_cfg():
    from gomatching_amd.config import merge_from_list
    cfg = mini_cfg("icdar15", device="cuda")
    merge_from_list(cfg, AUG_OPTS)
    cfg.MODEL.ASSO_HEAD.DROPOUT = 0.0
    return cfg


@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    return write_dataset(str(tmp_path_factory.mktemp("clipdata")), num_videos=2)


def test_device_ingest_and_host_ingest_give_the_same_loss_bits(dataset):
    """One clip (4 frames of 96x128, scaled by 1.5 to 144x192, a 96x128 window -- the size the trainer tests run the detector
    at) mapped twice from the same draws: `frame_u8` + `resize_hw` + `crop` through the model's single launch, and the
    reference's `image` from Pillow on the host."""
    from gomatching_amd import data, training
    from gomatching_amd.modeling import GoMatching
    from gomatching_amd.synth import TRAINING_CLS_BIAS
    from gomatching_amd.weights import synth_state_dict
    cfg = _train_cfg()
    videos = data.get_video_dataset_dicts([data.load_video_json(*dataset)])
    clips = [data.GoMDatasetMapper(cfg, True, device_ingest=d)(videos[0], np.random.default_rng(5)) for d in (True, False)]
    assert len(clips[0]) == 4 and "frame_u8" in clips[0][0] and "image" in clips[1][0]
    model = GoMatching(cfg, synth_state_dict(cfg, seed=7, cls_bias=TRAINING_CLS_BIAS), device=DEV)
    x, hw = model.preprocess_image(clips[0])
    y, hw_host = model.preprocess_image(clips[1])
    assert tuple(hw) == tuple(hw_host) == (96, 128) and tuple(x.shape) == (4, 96, 128, 4)
    assert torch.equal(x, y)
    on_device = [dict(fr, frame_u8=fr["frame_u8"].to(DEV)) for fr in clips[0]]                 # frames already resident
    assert torch.equal(model.preprocess_image(on_device)[0], x)
    losses = [training.forward_losses(model, c) for c in clips]
    assert set(losses[0]) == set(losses[1]) >= {"loss_long_asso", "loss_short_asso", "loss_res"}
    for k in losses[0]:
        a, b = losses[0][k].detach().cpu(), losses[1][k].detach().cpu()
        print(k, float(a), float(b))
        assert torch.isfinite(a).all() and a.view(torch.int32).equal(b.view(torch.int32)), k
    mixed = [dict(clips[0][0])] + [dict(fr, crop=(0, 0, 96, 128)) for fr in clips[0][1:]]
    if tuple(clips[0][0]["crop"]) != (0, 0, 96, 128):
        with pytest.raises(ValueError, match="must share"):
            model.preprocess_image(mixed)
    model.close()


# -------------------------------------------------------------------------------------------------- the CLI
def _weights(tmp_path):
    from gomatching_amd.solver import save_checkpoint
    from gomatching_amd.synth import TRAINING_CLS_BIAS
    from gomatching_amd.weights import synth_state_dict
    return save_checkpoint(os.path.join(str(tmp_path), "deepsolo.pth"), synth_state_dict(_train_cfg(), seed=7, cls_bias=TRAINING_CLS_BIAS))


def _argv(dataset, weights, out, iters, extra=()):
    return ["--builtin", "icdar15", "--json", dataset[0], "--image-root", dataset[1], "--seed", "21"] + list(extra) + \
           ["--opts", "MODEL.WEIGHTS", weights, "OUTPUT_DIR", out, "MODEL.TRANSFORMER.NUM_QUERIES", "12", "MODEL.ASSO_HEAD.DROPOUT", "0.0",
            "SOLVER.TRAIN_ITER", str(iters), "SOLVER.WARMUP_ITERS", "0", "DATALOADER.NUM_WORKERS", "2"] + AUG_OPTS


def test_train_main_trains_writes_and_resumes_to_the_same_bits(dataset, tmp_path):
    from gomatching_amd import eval as gom_eval
    from gomatching_amd import train
    weights = _weights(tmp_path)
    out = os.path.join(str(tmp_path), "run")
    assert train.main(_argv(dataset, weights, out, 3)) == 0
    final = gom_eval.load_weights(os.path.join(out, "model_final.pth"))
    start = gom_eval.load_weights(weights)
    assert set(final) >= set(start)
    assert not torch.equal(final["roi_heads.asso_head.fc1.weight"], torch.as_tensor(start["roi_heads.asso_head.fc1.weight"]))
    ck = torch.load(os.path.join(out, "model_final.pth"), map_location="cpu")
    assert ck["data_seed"] == 21 and ck["iteration"] == 2
    with open(os.path.join(out, "metrics.json")) as f:
        lines = [json.loads(line) for line in f]
    assert len(lines) == 1 and lines[0]["iteration"] == 3
    m = lines[0]
    assert {"loss_long_asso", "loss_short_asso", "loss_res", "total_loss", "lr", "grad_norm", "data_time", "time", "iteration"} <= set(m)
    assert all(np.isfinite(v) for v in m.values())

    # TRAIN_ITER 2, then --resume to 3: the head of the uninterrupted run, bit for bit (dropout is 0: any difference is the data's)
    out2 = os.path.join(str(tmp_path), "run2")
    assert train.main(_argv(dataset, weights, out2, 2)) == 0
    two = gom_eval.load_weights(os.path.join(out2, "model_final.pth"))
    assert not torch.equal(two["roi_heads.asso_head.fc1.weight"], final["roi_heads.asso_head.fc1.weight"])
    argv = _argv(dataset, weights, out2, 3, extra=["--resume"])
    argv[argv.index("--seed") + 1] = "999"                        # the checkpoint's data seed wins
    assert train.main(argv) == 0
    resumed = gom_eval.load_weights(os.path.join(out2, "model_final.pth"))
    assert torch.load(os.path.join(out2, "model_final.pth"), map_location="cpu")["data_seed"] == 21
    for k, v in final.items():
        if k.startswith("roi_heads."):
            assert v.dtype == resumed[k].dtype and torch.equal(v.view(torch.int32), resumed[k].view(torch.int32)), k
