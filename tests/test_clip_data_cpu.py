"""The training data pipeline on the host (gomatching_amd/data.py, train.py's argument handling, the new ABI entry points'
argument checks): the augmentation against what the reference's own classes computed (tests/golden/clip_aug.npz,
tools/gen_golden_clip_aug.py), everything else against statements written out here."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch
from PIL import Image

from clip_data_fixture import AUG_OPTS, box_bezier, training_boxes, write_dataset
from helpers import GOLDEN, mini_cfg


@pytest.fixture(scope="module")
def aug():
    return np.load(os.path.join(GOLDEN, "clip_aug.npz"))


def _draws(case):
    """The three draws `get_transform` makes after numpy.random.seed(k)."""
    lo, hi, k = case[5], case[6], int(case[7])
    rs = np.random.RandomState(k)
    return rs.uniform(lo, hi), rs.uniform(0, 1), rs.uniform(0, 1)


def _params(case):
    from gomatching_amd import data
    h, w, size, th, tw = (int(v) for v in case[:5])
    target = (size, size) if th < 0 and tw < 0 else (th, tw)
    return data.resize_crop_params(h, w, target, *_draws(case)), target


# ------------------------------------------------------------------------------------------- augmentation
def test_fixture_covers_the_crop_regimes(aug):
    ints = aug["ints"]
    sh, sw, th, tw = ints[:, 0], ints[:, 1], ints[:, 4], ints[:, 5]
    assert len(ints) >= 40
    assert ((sh <= th) & (sw <= tw)).any() and ((sh > th) & (sw > tw)).any() and ((sh > th) != (sw > tw)).any()
    assert (th != tw).any() and (aug["cases"][:, 0] % 2 == 1).any()
    assert (aug["cases"][:, 5] == 0.1).any() and (aug["cases"][:, 6] == 2.0).any()


def test_resize_crop_params_equal_the_reference_transform(aug):
    from gomatching_amd import data
    for case, ints, scale, coords in zip(aug["cases"], aug["ints"], aug["img_scale"], aug["coords"]):
        params, target = _params(case)
        assert tuple(params[:4]) == tuple(int(v) for v in ints[:4]), case
        assert all(isinstance(v, int) for v in params[:4])
        assert params[4] == scale, case                                          # the same float64, not a close one
        assert target == (int(ints[4]), int(ints[5]))
        got = data.apply_coords(aug["points"], params)
        assert got.dtype == np.float64 and np.array_equal(got, coords), case
        y0, x0, oh, ow = data.crop_window(params, target)
        assert 0 <= y0 and 0 <= x0 and y0 + oh <= params[0] and x0 + ow <= params[1] and oh <= target[0] and ow <= target[1]
        assert oh == min(params[0], target[0]) or y0 + oh == params[0]


def test_host_apply_image_equals_the_reference_arrays(aug):
    from gomatching_amd import data
    for i in range(4):
        case = aug["cases"][int(aug["image_%d_case" % i])]
        params, target = _params(case)
        got = data.apply_image(aug["image_%d" % i], params, target)
        assert got.dtype == np.uint8 and np.array_equal(got, aug["image_%d_out" % i]), i


# ------------------------------------------------------------------------------------------------ dataset
def _write_json(tmp_path, images, annotations):
    path = os.path.join(str(tmp_path), "d.json")
    with open(path, "w") as f:
        json.dump({"images": images, "annotations": annotations, "categories": [{"id": 5, "name": "other"}, {"id": 3, "name": "text"}]}, f)
    return path


def _bezier64(pts):
    """Float64 statement of the 25-point evaluation: B(u) = sum_k C(3,k) (1-u)^(3-k) u^k P_k for the top and the bottom curve."""
    p = np.asarray(pts, np.float64).reshape(2, 4, 2)
    u = np.linspace(0.0, 1.0, 25)[:, None]
    curve = lambda c: (1 - u) ** 3 * c[0] + 3 * u * (1 - u) ** 2 * c[1] + 3 * u ** 2 * (1 - u) * c[2] + u ** 3 * c[3]
    top, bottom = curve(p[0]), curve(p[1])
    return top, bottom


def test_load_video_json(tmp_path):
    from gomatching_amd import data
    curved = [0, 10, 10, 0, 20, 0, 30, 10, 30, 20, 20, 12, 10, 12, 0, 20]
    straight = box_bezier([4, 6, 34, 16])
    images = [{"id": 12, "file_name": "b/2.jpg", "height": 48, "width": 64, "video_id": 2},
              {"id": 11, "file_name": "b/1.jpg", "height": 48, "width": 64, "video_id": 2},
              {"id": 3, "file_name": "a/1.jpg", "height": 48, "width": 64, "video_id": 1},
              {"id": 40, "file_name": "single.jpg", "height": 48, "width": 64}]
    anns = [{"id": 1, "image_id": 11, "category_id": 3, "iscrowd": 0, "bbox": [1, 2, 3, 4], "instance_id": 70, "transcription": "###",
             "bezier_pts": curved},
            {"id": 2, "image_id": 3, "category_id": 5, "iscrowd": 1, "bbox": [5, 6, 7, 8], "instance_id": 0,
             "transcription": "ABCDEFGHIJKLMNOPQRSTUVWXYZ0123456789", "bezier_pts": straight},
            {"id": 3, "image_id": 11, "category_id": 3, "iscrowd": 0, "bbox": [1, 2, 3, 4], "instance_id": -1, "transcription": "a-Z é9",
             "poly": [0, 0, 10, 0, 10, 5, 0, 5]},
            {"id": 4, "image_id": 12, "category_id": 3, "iscrowd": 0, "bbox": [1, 2, 3, 4], "instance_id": 20, "transcription": "x!",
             "text_category": "nonalphanumeric", "bezier_pts": straight},
            {"id": 5, "image_id": 12, "category_id": 3, "iscrowd": 0, "bbox": [1, 2, 3, 4], "instance_id": 70, "bezier_pts": straight}]
    recs = data.load_video_json(_write_json(tmp_path, images, anns), "/images")
    assert [r["image_id"] for r in recs] == [3, 11, 12, 40]
    assert recs[1]["file_name"] == os.path.join("/images", "b/1.jpg") and (recs[1]["height"], recs[1]["width"]) == (48, 64)
    assert [r["video_id"] for r in recs] == [1, 2, 2, -1]
    a_crowd, (a1, a3), (a4, a5) = recs[0]["annotations"][0], recs[1]["annotations"], recs[2]["annotations"]
    assert recs[3]["annotations"] == []
    # instance ids: sorted positives {20, 70} -> 1, 2; 0 and -1 -> 0
    assert (a1["instance_id"], a_crowd["instance_id"], a3["instance_id"], a4["instance_id"], a5["instance_id"]) == (2, 0, 0, 1, 2)
    assert a_crowd["iscrowd"] == 1 and a1["iscrowd"] == 0
    assert (a1["category_id"], a_crowd["category_id"]) == (0, 1) and a1["bbox"] == [1, 2, 3, 4]      # sorted category ids 3, 5 -> 0, 1
    # texts
    pad = [37] * 24
    assert a1["texts"].dtype == np.int32 and a1["texts"].tolist() == [36] + pad                        # '###'
    assert a_crowd["texts"].tolist() == list(range(25))                                                 # cut at 25 characters, lower-cased
    assert a3["texts"].tolist() == [0, 36, 25, 36, 36, 35] + [37] * 19                                   # '-', ' ', 'é' are outside the table
    assert a4["texts"].tolist() == [36] + pad and a5["texts"].tolist() == [36] + pad                    # nonalphanumeric; no transcription
    # points
    top, bottom = _bezier64(curved)
    assert a1["boundary"].shape == (50, 2) and a1["polyline"].shape == (25, 2) and a1["beziers"].shape == (4, 2)
    # boundary interleaves: point i of the top curve, then the point of the bottom curve under it (the bottom curve runs backwards)
    np.testing.assert_allclose(a1["boundary"][0::2], top, rtol=0, atol=1e-12)
    np.testing.assert_allclose(a1["boundary"][1::2], bottom[::-1], rtol=0, atol=1e-12)
    np.testing.assert_allclose(a1["polyline"], (top + bottom[::-1]) / 2, rtol=0, atol=1e-12)
    c = np.asarray(curved, np.float64).reshape(8, 2)
    np.testing.assert_array_equal(a1["beziers"], (c[:4] + c[4:][::-1]) / 2)
    # a straight-edged Bezier with evenly spaced control points gives evenly spaced points
    np.testing.assert_allclose(a4["polyline"], np.stack([np.linspace(4, 34, 25), np.full(25, 11.0)], -1), rtol=0, atol=1e-12)
    np.testing.assert_allclose(a4["boundary"][0::2], np.stack([np.linspace(4, 34, 25), np.full(25, 6.0)], -1), rtol=0, atol=1e-12)
    np.testing.assert_allclose(a4["boundary"][1::2], np.stack([np.linspace(4, 34, 25), np.full(25, 16.0)], -1), rtol=0, atol=1e-12)
    # poly only: loads, without the point fields
    assert not {"beziers", "boundary", "polyline"} & set(a3)
    # grouping
    videos = data.get_video_dataset_dicts([recs], gen_inst_id=False)
    assert [(v["video_id"], [im["image_id"] for im in v["images"]], v["dataset_source"]) for v in videos] == \
        [(1, [3], 0), (2, [11, 12], 0), (1000001, [40], 0)]
    videos = data.get_video_dataset_dicts([data.load_video_json(_write_json(tmp_path, images, anns), "r")], gen_inst_id=True)
    assert [a["instance_id"] for a in videos[1]["images"][0]["annotations"]] == [2, 1000002]              # the crowd one of video 1 took 1000001


def test_poly_only_annotation_fails_at_mapping_time_under_with_resr(tmp_path):
    from gomatching_amd import data
    Image.fromarray(np.zeros((48, 64, 3), np.uint8)).save(os.path.join(str(tmp_path), "1.png"))
    images = [{"id": i, "file_name": "1.png", "height": 48, "width": 64, "video_id": 1} for i in (1, 2)]
    anns = [{"id": 77, "image_id": i, "category_id": 3, "iscrowd": 0, "bbox": [1, 2, 30, 20], "instance_id": 5, "transcription": "a",
             "poly": [0, 0, 10, 0, 10, 5, 0, 5]} for i in (1, 2)]
    videos = data.get_video_dataset_dicts([data.load_video_json(_write_json(tmp_path, images, anns), str(tmp_path))])
    cfg = mini_cfg("icdar15")
    assert cfg.MODEL.ROI_HEADS.WITH_RESR
    with pytest.raises(ValueError, match=r"(?s)annotation 77.*bezier_pts.*precomputed"):
        data.GoMDatasetMapper(cfg, True, device_ingest=False)(videos[0], np.random.default_rng(0))
    cfg.MODEL.ROI_HEADS.WITH_RESR = False
    clip = data.GoMDatasetMapper(cfg, True, device_ingest=False)(videos[0], np.random.default_rng(0))
    assert len(clip) == 2 and "polyline" not in clip[0]["instances"] and len(clip[0]["instances"]["gt_boxes"]) == 1


# ----------------------------------------------------------------------------------------------- sampling
def _video(n, h=720, w=1280):
    return {"video_id": 9, "images": [{"height": h, "width": w, "image_id": i, "annotations": []} for i in range(n)]}


def test_sample_clip_counts_and_order():
    from gomatching_amd import data
    # no dynamic scale, SAMPLE_RANGE 2: TRAIN_LEN frames, sorted, unique, from [st, st + 2 * TRAIN_LEN)
    seen_gap = False
    for seed in range(50):
        rng = np.random.default_rng(seed)
        inds, params = data.sample_clip(_video(100), rng, 6, (1280, 1280), (0.1, 2.0), 2.0, False, True)
        assert len(inds) == 6 and inds == sorted(set(inds)) and inds[0] >= 0 and inds[-1] < 100
        assert inds[-1] - inds[0] < 12 and inds[0] <= 94
        seen_gap |= inds[-1] - inds[0] > 5
        assert len(params) == 5
    assert seen_gap
    # SAMPLE_RANGE 1: the contiguous slice
    inds, _ = data.sample_clip(_video(100), np.random.default_rng(1), 6, (1280, 1280), (1.0, 1.0), 1.0, False, True)
    assert inds == list(range(inds[0], inds[0] + 6))
    # a short video: every frame
    inds, _ = data.sample_clip(_video(4), np.random.default_rng(1), 6, (1280, 1280), (1.0, 1.0), 2.0, True, True)
    assert inds == [0, 1, 2, 3]
    # dynamic scale at scale exactly 0.5: 1280x720 -> 640x360, auged 640, max_frames = int(6 * (1280/640)^2) = 24 > 6:
    # the length is drawn from [6, 24], capped at 12; the window [st, st + 2 * n) is cut by the video's end
    lengths = set()
    for seed in range(60):
        inds, params = data.sample_clip(_video(100), np.random.default_rng(seed), 6, (1280, 1280), (0.5, 0.5), 2.0, True, True)
        assert params[:2] == (360, 640) and 6 <= len(inds) <= 12 and inds == sorted(set(inds))
        lengths.add(len(inds))
    assert 12 in lengths and min(lengths) < 12
    # dynamic scale at scale 1: 1280x720 -> auged 1280, max_frames = 6: no lengthening
    for seed in range(10):
        inds, _ = data.sample_clip(_video(100), np.random.default_rng(seed), 6, (1280, 1280), (1.0, 1.0), 2.0, True, True)
        assert len(inds) == 6
    # scale 2: max_frames = int(6 / 4) = 1 <= TRAIN_LEN: still TRAIN_LEN frames
    inds, _ = data.sample_clip(_video(100), np.random.default_rng(3), 6, (1280, 1280), (2.0, 2.0), 2.0, True, True)
    assert len(inds) == 6
    # a 7-frame video at scale 0.5: never more frames than the video has
    for seed in range(10):
        inds, _ = data.sample_clip(_video(7), np.random.default_rng(seed), 6, (1280, 1280), (0.5, 0.5), 2.0, True, True)
        assert 6 <= len(inds) <= 7 and inds[-1] < 7


def test_gen_image_motion_on_a_one_image_video_raises():
    from gomatching_amd import data
    with pytest.raises(NotImplementedError, match="video 9"):
        data.sample_clip(_video(1), np.random.default_rng(0), 6, (640, 640), (0.1, 2.0), 2.0, True, True)
    inds, _ = data.sample_clip(_video(1), np.random.default_rng(0), 6, (640, 640), (0.1, 2.0), 2.0, True, False)
    assert inds == [0]


# ------------------------------------------------------------------------------------------------- mapper
def _mapper_cfg(clamp, opts=()):
    cfg = mini_cfg("icdar15")
    from gomatching_amd.config import merge_from_list
    merge_from_list(cfg, list(AUG_OPTS) + ["INPUT.NOT_CLAMP_BOX", "false" if clamp else "true"] + list(opts))
    return cfg


def test_mapper_on_the_host(tmp_path):
    from gomatching_amd import data
    json_file, image_root = write_dataset(str(tmp_path))
    videos = data.get_video_dataset_dicts([data.load_video_json(json_file, image_root)])
    assert len(videos) == 1 and len(videos[0]["images"]) == 4
    clips = {}
    for clamp in (True, False):
        mapper = data.GoMDatasetMapper(_mapper_cfg(clamp), True, device_ingest=False)
        clips[clamp] = mapper(videos[0], np.random.default_rng(5))
    _, params = data.GoMDatasetMapper(_mapper_cfg(True), True).plan(videos[0], np.random.default_rng(5))
    assert params[:2] == (144, 192) and params[4] == 1.5 and 0 <= params[2] <= 48 and 0 <= params[3] <= 64
    oy, ox = params[2], params[3]
    assert oy > 0 and ox > 0                                                     # this seed crops in both axes
    for clamp in (True, False):
        assert len(clips[clamp]) == 4
        for t, fr in enumerate(clips[clamp]):
            assert fr["image"].dtype == torch.uint8 and tuple(fr["image"].shape) == (3, 96, 128)
            src = np.asarray(Image.open(fr["file_name"]).convert("RGB"))
            want = np.asarray(Image.fromarray(src).resize((192, 144), Image.BILINEAR))[oy:oy + 96, ox:ox + 128]
            assert np.array_equal(fr["image"].numpy().transpose(1, 2, 0), want)
            assert (fr["height"], fr["width"], fr["video_id"], fr["image_id"]) == (96, 128, 1, t + 1)
            inst = fr["instances"]
            want_boxes, want_ids, want_poly = [], [], []
            for b, iid in zip(training_boxes(t), (2, 1)):                        # instance ids 107, 103 -> 2, 1
                x = np.array([b[0] * 1.5 - ox, b[1] * 1.5 - oy, b[2] * 1.5 - ox, b[3] * 1.5 - oy])
                if clamp:
                    x = np.minimum(np.maximum(x, 0), [128, 96, 128, 96])
                if x[2] - x[0] > 1e-5 and x[3] - x[1] > 1e-5:
                    want_boxes.append(x)
                    want_ids.append(iid)
                    want_poly.append(np.stack([np.linspace(b[0], b[2], 25) * 1.5 - ox, np.full(25, (b[1] + b[3]) / 2 * 1.5 - oy)], -1))
            assert inst["gt_boxes"].dtype == torch.float32 and inst["gt_instance_ids"].tolist() == want_ids
            assert torch.equal(inst["gt_boxes"], torch.as_tensor(np.array(want_boxes).reshape(-1, 4), dtype=torch.float32))
            assert inst["gt_classes"].tolist() == [0] * len(want_ids) and tuple(inst["texts"].shape) == (len(want_ids), 25)
            assert tuple(inst["polyline"].shape) == (len(want_ids), 50) and tuple(inst["boundary"].shape) == (len(want_ids), 100)
            assert tuple(inst["beziers"].shape) == (len(want_ids), 8)
            np.testing.assert_allclose(inst["polyline"].numpy().reshape(-1, 25, 2), np.array(want_poly).reshape(-1, 25, 2),
                                       rtol=0, atol=2e-5)
    # unclamped boxes may leave the crop; clamped ones never do
    allb = torch.cat([fr["instances"]["gt_boxes"] for fr in clips[True]])
    assert float(allb.min()) >= 0 and float(allb[:, 2].max()) <= 128 and float(allb[:, 3].max()) <= 96


def test_mapper_filters_a_box_the_crop_empties_and_drops_crowds(tmp_path):
    from gomatching_amd import data
    json_file, image_root = write_dataset(str(tmp_path))
    with open(json_file) as f:
        d = json.load(f)
    # a box in the far corner of every frame: under a 1.5x scale it lies outside every 96x128 window whose offset is small, and
    # clamping then leaves it no width; plus a crowd annotation that must never come through
    for im in d["images"]:
        d["annotations"].append({"id": 900 + im["id"], "image_id": im["id"], "category_id": 1, "iscrowd": 0, "bbox": [124, 92, 4, 4],
                                 "instance_id": 55, "transcription": "far", "bezier_pts": box_bezier([124, 92, 128, 96])})
        d["annotations"].append({"id": 950 + im["id"], "image_id": im["id"], "category_id": 1, "iscrowd": 1, "bbox": [0, 0, 128, 96],
                                 "instance_id": 56, "transcription": "crowd", "bezier_pts": box_bezier([0, 0, 128, 96])})
    with open(json_file, "w") as f:
        json.dump(d, f)
    videos = data.get_video_dataset_dicts([data.load_video_json(json_file, image_root)])
    _, params = data.GoMDatasetMapper(_mapper_cfg(True), True).plan(videos[0], np.random.default_rng(5))
    oy, ox = params[2], params[3]
    # the far box becomes [186 - ox, 138 - oy, 192 - ox, 144 - oy]: at or beyond the window's right edge for ox <= 58, beyond
    # its lower edge for oy <= 42, so clamping leaves it no area; this seed's offsets do that
    assert ox <= 58 or oy <= 42
    for clamp in (True, False):
        clip = data.GoMDatasetMapper(_mapper_cfg(clamp), True, device_ingest=False)(videos[0], np.random.default_rng(5))
        for t, fr in enumerate(clip):
            ids = fr["instances"]["gt_instance_ids"].tolist()                    # ids 55, 56, 103, 107 -> 1, 2, 3, 4: 56 is the crowd
            assert 2 not in ids
            if not clamp:
                assert ids == [4, 3, 1]                                          # nothing is emptied without the clamp
            else:
                want = []
                for b, iid in zip(training_boxes(t), (4, 3)):
                    x = np.minimum(np.maximum(np.array(b) * 1.5 - [ox, oy, ox, oy], 0), [128, 96, 128, 96])
                    if x[2] - x[0] > 1e-5 and x[3] - x[1] > 1e-5:
                        want.append(iid)
                assert ids == want and 1 not in ids
            assert len(fr["instances"]["gt_boxes"]) == len(fr["instances"]["texts"]) == len(fr["instances"]["polyline"]) == len(ids)


def test_mapper_device_ingest_hands_over_the_frame_and_the_numbers(tmp_path):
    from gomatching_amd import data
    json_file, image_root = write_dataset(str(tmp_path))
    videos = data.get_video_dataset_dicts([data.load_video_json(json_file, image_root)])
    clip = data.GoMDatasetMapper(_mapper_cfg(False), True, device_ingest=True)(videos[0], np.random.default_rng(5))
    host = data.GoMDatasetMapper(_mapper_cfg(False), True, device_ingest=False)(videos[0], np.random.default_rng(5))
    for fr, h in zip(clip, host):
        assert "image" not in fr and fr["frame_u8"].dtype == torch.uint8 and tuple(fr["frame_u8"].shape) == (96, 128, 3)
        assert fr["resize_hw"] == (144, 192) and fr["crop"][2:] == (96, 128) and fr["flip_channels"] is False
        assert torch.equal(fr["instances"]["gt_boxes"], h["instances"]["gt_boxes"])
        assert np.array_equal(fr["frame_u8"].numpy(), np.asarray(Image.open(fr["file_name"]).convert("RGB")))


def test_mapper_refusals(tmp_path):
    from gomatching_amd import data
    cfg = _mapper_cfg(True, ["INPUT.CUSTOM_AUG", "ResizeShortestEdge"])
    with pytest.raises(NotImplementedError, match="ResizeShortestEdge"):
        data.GoMDatasetMapper(cfg, True)
    json_file, image_root = write_dataset(str(tmp_path))
    recs = data.load_video_json(json_file, image_root)
    recs[1]["height"] = 97                                                       # one frame of another size
    with pytest.raises(ValueError, match="video 1"):
        data.GoMDatasetMapper(_mapper_cfg(True), True).plan(data.get_video_dataset_dicts([recs])[0], np.random.default_rng(0))
    recs = data.load_video_json(json_file, image_root)
    for r in recs:
        r["height"] = 90                                                         # the json disagrees with the decoded frames
    with pytest.raises(ValueError, match="Mismatched image shape"):
        data.GoMDatasetMapper(_mapper_cfg(True), True)(data.get_video_dataset_dicts([recs])[0], np.random.default_rng(0))


def test_data_defaults_are_the_references_and_leave_the_config_alone():
    from gomatching_amd import data
    from gomatching_amd.config import get_cfg
    cfg = get_cfg()
    before = json.dumps(cfg, sort_keys=True)
    D = data.data_cfg(cfg)
    assert json.dumps(cfg, sort_keys=True) == before and "CUSTOM_AUG" not in cfg.INPUT
    I = D.INPUT
    assert (I.CUSTOM_AUG, I.TRAIN_SIZE, I.TRAIN_H, I.TRAIN_W, tuple(I.SCALE_RANGE), I.NOT_CLAMP_BOX) == ("", 640, -1, -1, (0.1, 2.0), False)
    assert (I.VIDEO.SAMPLE_RANGE, I.VIDEO.DYNAMIC_SCALE, I.VIDEO.GEN_IMAGE_MOTION, I.VIDEO.TRAIN_LEN) == (2.0, True, True, 8)
    assert (D.DATALOADER.SAMPLER_TRAIN, D.DATALOADER.NUM_WORKERS) == ("TrainingSampler", 4)
    want = {"icdar15": "icdar15_train", "pp_icdar15": "icdar15_train", "dstext": "dstext_train", "pp_dstext": "dstext_train",
            "artvideo": "artvideo_train", "pp_artvideo": "artvideo_train", "bovtext": "bov_train", "pp_bovtext": "bov_train"}
    for name, split in want.items():
        c = mini_cfg(name)
        I = data.data_cfg(c).INPUT
        assert (I.CUSTOM_AUG, I.TRAIN_SIZE, I.NOT_CLAMP_BOX, I.VIDEO.TRAIN_LEN) == ("EfficientDetResizeCrop", 1280, True, 6), name
        assert tuple(I.SCALE_RANGE) == ((0.5, 2.0) if "dstext" in name else (0.1, 2.0)), name
        assert list(c.DATASETS.TRAIN) == [split] and data.resolve_split(split)[0].startswith("datasets/")
        m = data.GoMDatasetMapper(c, True)
        assert m.target_size == (1280, 1280) and m.not_clamp_box and m.train_len == 6
    c = mini_cfg("icdar15")
    c.INPUT.SCALE_RANGE = "(0.5, 2.0)"                                           # the reference's yaml spelling, a string under safe_load
    assert data.GoMDatasetMapper(c, True).scale == (0.5, 2.0)


# ------------------------------------------------------------------------------------------------- loader
def _loader(tmp_path, workers=4, num_videos=6, **kw):
    from gomatching_amd import data
    root = os.path.join(str(tmp_path), "ds")
    if not os.path.isdir(root):
        write_dataset(root, num_videos=num_videos, num_frames=9, height=24, width=32)
    cfg = _mapper_cfg(True, ["INPUT.TRAIN_H", "24", "INPUT.TRAIN_W", "32", "INPUT.SCALE_RANGE", "[0.5, 2.0]",
                             "INPUT.VIDEO.TRAIN_LEN", "3", "DATALOADER.NUM_WORKERS", str(workers)])
    recs = data.load_video_json(os.path.join(root, "train.json"), os.path.join(root, "frame"))
    return data.build_vts_train_loader(cfg, data.GoMDatasetMapper(cfg, True, device_ingest=False), dataset_dicts=recs, **kw)


def _plan_key(plan):
    v, records, params = plan
    return v, tuple(r["image_id"] for r in records), params


def _clip_key(clip):
    return [(fr["image_id"], fr["image"].numpy().tobytes(), fr["instances"]["gt_boxes"].numpy().tobytes()) for fr in clip]


def test_loader_clip_is_a_pure_function_of_seed_iteration_and_rank(tmp_path):
    a = _loader(tmp_path, workers=1, seed=11)
    b = _loader(tmp_path, workers=4, seed=11)
    assert (a.num_workers, b.num_workers) == (1, 4) and _loader(tmp_path, workers=64, seed=1).num_workers == 16
    with a, b:
        clips_a = [next(a) for _ in range(9)]
        clips_b = [next(b) for _ in range(9)]
    for i in range(9):
        assert _clip_key(clips_a[i]) == _clip_key(clips_b[i]), i                 # 1 thread and 4 threads
        assert [fr["image_id"] for fr in clips_a[i]] == list(_plan_key(a.plan(i))[1])
    assert a.iteration == 9 and len({_plan_key(a.plan(i)) for i in range(9)}) > 1
    with _loader(tmp_path, seed=11, start_iter=5) as c:                          # a resumed run
        assert c.iteration == 5
        for i in range(5, 9):
            assert _plan_key(c.plan(i)) == _plan_key(a.plan(i))
            assert _clip_key(next(c)) == _clip_key(clips_a[i]), i
    assert [_plan_key(_loader(tmp_path, seed=12).plan(i)) for i in range(9)] != [_plan_key(a.plan(i)) for i in range(9)]
    # every epoch visits every video once, and the epochs' orders differ
    order = [a.video_index(i) for i in range(18)]
    assert sorted(order[:6]) == sorted(order[6:12]) == sorted(order[12:]) == list(range(6))
    assert len({tuple(order[:6]), tuple(order[6:12]), tuple(order[12:])}) > 1


def test_loader_ranks_take_disjoint_positions_that_cover_an_epoch_once(tmp_path):
    from gomatching_amd import data
    root = os.path.join(str(tmp_path), "ds")
    write_dataset(root, num_videos=6, num_frames=4, height=24, width=32)
    cfg = _mapper_cfg(True, ["SOLVER.IMS_PER_BATCH", "2"])
    recs = data.load_video_json(os.path.join(root, "train.json"), os.path.join(root, "frame"))
    mapper = data.GoMDatasetMapper(cfg, True)
    ranks = [data.build_vts_train_loader(cfg, mapper, 3, rank=r, world_size=2, dataset_dicts=recs) for r in (0, 1)]
    single = data.build_vts_train_loader(_mapper_cfg(True), mapper, 3, dataset_dicts=recs)
    pos = [[ld.position(i) for i in range(3)] for ld in ranks]
    assert pos == [[0, 2, 4], [1, 3, 5]]
    vids = [[ld.video_index(i) for i in range(3)] for ld in ranks]
    assert not set(vids[0]) & set(vids[1]) and sorted(vids[0] + vids[1]) == list(range(6))
    assert [single.video_index(p) for p in range(6)] == [vids[p % 2][p // 2] for p in range(6)]          # the same stream, dealt out
    # the draws of one iteration differ between ranks
    assert ranks[0].plan(0)[2] != ranks[1].plan(0)[2]
    with pytest.raises(AssertionError):
        data.build_vts_train_loader(_mapper_cfg(True), mapper, 3, rank=0, world_size=2, dataset_dicts=recs)   # IMS_PER_BATCH 1 // 2 = 0


def test_loader_refusals(tmp_path):
    from gomatching_amd import data
    cfg = _mapper_cfg(True, [])
    mapper = data.GoMDatasetMapper(cfg, True)
    cfg.DATALOADER = {"SAMPLER_TRAIN": "MultiDatasetSampler"}
    with pytest.raises(NotImplementedError, match="MultiDatasetSampler"):
        data.build_vts_train_loader(cfg, mapper, 0, dataset_dicts=[{}])
    cfg = _mapper_cfg(True, [])
    cfg.DATASETS.TRAIN = ["icdar15_train", "dstext_train"]
    with pytest.raises(NotImplementedError, match="one training dataset"):
        data.build_vts_train_loader(cfg, mapper, 0)


def test_loader_refuses_at_construction_what_the_sampler_would_refuse_mid_run(tmp_path):
    from gomatching_amd import data
    json_file, image_root = write_dataset(str(tmp_path), num_videos=3)
    cfg = _mapper_cfg(True)
    mapper = data.GoMDatasetMapper(cfg, True)
    recs = data.load_video_json(json_file, image_root)
    lonely = [r for r in recs if r["video_id"] != 3] + [r for r in recs if r["video_id"] == 3][:1]       # video 3 keeps one image
    with pytest.raises(NotImplementedError, match="video 3 has one image"):
        data.build_vts_train_loader(cfg, mapper, 0, dataset_dicts=lonely)
    off = _mapper_cfg(True, ["INPUT.VIDEO.GEN_IMAGE_MOTION", "false"])
    with data.build_vts_train_loader(off, data.GoMDatasetMapper(off, True), 0, dataset_dicts=lonely) as ld:
        assert {len(ld.plan(i)[1]) for i in range(6)} == {1, 4}
    recs[5]["width"] = 130                                                       # video 2, frame 2
    with pytest.raises(ValueError, match="video 2"):
        data.build_vts_train_loader(cfg, mapper, 0, dataset_dicts=recs)
    a, b = data.new_data_seed(), data.new_data_seed()
    assert 0 <= a < 2 ** 63 and 0 <= b < 2 ** 63 and a != b


# ---------------------------------------------------------------------------------------------------- ABI
def test_crop_entry_points_reject_bad_windows_without_a_gpu():
    """As test_abi.py's argument test: the checks run before any HIP call, so nonsense comes back as GOM_ERR_INVALID_ARG."""
    from gomatching_amd import lib
    L = lib.load()
    INVALID = 1
    p = ctypes.c_void_p(0x1000)                                   # non-null, never dereferenced
    m = (ctypes.c_float * 3)(1, 2, 3)

    def u8(src=p, dst=p, xb=p, B=1, H=8, W=8, SH=16, SW=16, y0=0, x0=0, OH=16, OW=16, ks=3):
        return L.gom_resize_crop_bilinear_u8_hwc3(src, B, H, W, xb, p, ks, p, p, ks, dst, SH, SW, y0, x0, OH, OW, 0, None)

    def f32(src=p, dst=p, mean=m, std=m, SH=16, SW=16, y0=0, x0=0, OH=16, OW=16):
        return L.gom_ingest_crop_u8_hwc3_to_nhwc4(src, 1, 8, 8, p, p, 3, p, p, 3, mean, std, dst, SH, SW, y0, x0, OH, OW, 0, None)

    for bad in (dict(x0=-1), dict(y0=-1), dict(x0=1), dict(y0=1), dict(x0=8, OW=9), dict(y0=15, OH=2), dict(OH=17), dict(OW=17),
                dict(OH=0), dict(OW=0), dict(OH=-4), dict(SH=0), dict(SW=-1), dict(x0=2 ** 31 - 1, OW=2), dict(y0=2 ** 31 - 1, OH=2)):
        assert u8(**bad) == INVALID, bad
        assert f32(**bad) == INVALID, bad
    for bad in (dict(src=None), dict(dst=None), dict(xb=None), dict(B=0), dict(H=0), dict(W=-1), dict(ks=0)):
        assert u8(**bad) == INVALID, bad
    for bad in (dict(src=None), dict(dst=None), dict(mean=None), dict(std=None)):
        assert f32(**bad) == INVALID, bad
    assert {"gom_resize_crop_bilinear_u8_hwc3", "gom_ingest_crop_u8_hwc3_to_nhwc4"} <= set(lib.SIGNATURES)


def test_crop_ops_check_the_window_and_the_frames_before_any_launch():
    from gomatching_amd import ops
    frames = torch.zeros((1, 8, 8, 3), dtype=torch.uint8)
    for window in ((0, 1, 16, 16), (-1, 0, 4, 4), (0, 0, 0, 4), (13, 0, 4, 4)):
        with pytest.raises(ValueError, match="not inside"):
            ops.resize_crop_u8(frames, (16, 16), window)
        with pytest.raises(ValueError, match="not inside"):
            ops.ingest_crop(frames, (16, 16), window, [0, 0, 0], [1, 1, 1], False)
    with pytest.raises(ValueError, match="CUDA"):
        ops.resize_crop_u8(frames, (16, 16), (0, 0, 16, 16))                     # host frames: no CPU path exists


def test_checkpoint_keeps_the_data_seed_only_when_given(tmp_path):
    from gomatching_amd.solver import save_checkpoint
    a = save_checkpoint(os.path.join(str(tmp_path), "a.pth"), {"w": torch.zeros(2)}, None, 4)
    b = save_checkpoint(os.path.join(str(tmp_path), "b.pth"), {"w": torch.zeros(2)}, None, 4, data_seed=99)
    assert set(torch.load(a)) == {"model", "optimizer", "iteration"}
    assert torch.load(b)["data_seed"] == 99


# ---------------------------------------------------------------------------------------------------- CLI
def test_train_main_argument_errors_return_2(tmp_path, capsys):
    from gomatching_amd import train
    json_file, image_root = write_dataset(str(tmp_path))
    weights = os.path.join(str(tmp_path), "w.pth")
    torch.save({"model": {}}, weights)
    data_args = ["--json", json_file, "--image-root", image_root]
    with open(json_file) as f:
        d = json.load(f)
    d["images"].append(dict(d["images"][0], id=9999, video_id=77))               # a video of one image
    lonely = os.path.join(str(tmp_path), "lonely.json")
    with open(lonely, "w") as f:
        json.dump(d, f)
    ok_opts = ["--opts", "MODEL.WEIGHTS", weights, "OUTPUT_DIR", os.path.join(str(tmp_path), "out")]
    cases = {
        "neither config source": data_args + ok_opts,
        "both config sources": ["--builtin", "icdar15", "--config-file", "x.yaml"] + data_args + ok_opts,
        "missing config file": ["--config-file", os.path.join(str(tmp_path), "no.yaml")] + data_args + ok_opts,
        "odd --opts": ["--builtin", "icdar15"] + data_args + ok_opts + ["SOLVER.TRAIN_ITER"],
        "--json without --image-root": ["--builtin", "icdar15", "--json", json_file] + ok_opts,
        "missing json": ["--builtin", "icdar15", "--json", json_file + ".no", "--image-root", image_root] + ok_opts,
        "split table json absent": ["--builtin", "icdar15"] + ok_opts,
        "unknown split": ["--builtin", "icdar15"] + ok_opts + ["DATASETS.TRAIN", "[nowhere_train]"],
        "two datasets": ["--builtin", "icdar15"] + ok_opts + ["DATASETS.TRAIN", "[icdar15_train, dstext_train]"],
        "missing weights": ["--builtin", "icdar15"] + data_args + ["--opts", "MODEL.WEIGHTS", weights + ".no"],
        "no weights": ["--builtin", "icdar15"] + data_args,
        "unsupported sampler": ["--builtin", "icdar15"] + data_args + ok_opts + ["DATALOADER.SAMPLER_TRAIN", "MultiDatasetSampler"],
        "unsupported augmentation": ["--builtin", "icdar15"] + data_args + ok_opts + ["INPUT.CUSTOM_AUG", "ResizeShortestEdge"],
        "a one-image video under GEN_IMAGE_MOTION": ["--builtin", "icdar15", "--json", lonely, "--image-root", image_root] + ok_opts,
        "resume without a checkpoint": ["--builtin", "icdar15", "--resume"] + data_args + ok_opts,
    }
    for what, argv in cases.items():
        assert train.main(argv) == 2, what
        err = capsys.readouterr().err
        assert err.startswith("error: ") and err.count("\n") == 1, (what, err)
    assert not os.path.exists(os.path.join(str(tmp_path), "out"))
