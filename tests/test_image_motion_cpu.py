"""Training from still images, the host half: `data.motion_clip_params` against what the reference's own lines compute
(tests/golden/clip_motion.npz, tools/gen_golden_clip_motion.py), the mapper's and the loader's motion clips, the argument
checks of `gom_ingest_motion_u8_hwc3_to_nhwc4`, and `train --image-motion` up to the GPU's doorstep.  No GPU."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch
from PIL import Image

from clip_data_fixture import AUG_OPTS, box_bezier, training_boxes
from helpers import GOLDEN, mini_cfg
from image_motion_fixture import write_stills

# the issue's seven cases: (source h, w, size, TRAIN_LEN)
SEVEN = [(96, 128, 96, 4), (128, 96, 96, 4), (720, 1280, 1280, 6), (3000, 4000, 1280, 6), (37, 53, 48, 4), (64, 64, 64, 4),
         (40, 300, 64, 5)]


class LegacyDraws:
    """`uniform` from numpy's global state, which the golden's generator seeded: the draws the reference's transform made."""

    @staticmethod
    def uniform(lo, hi):
        return np.random.uniform(lo, hi)


class Replay:
    def __init__(self, draws):
        self.draws = list(draws)

    def uniform(self, lo, hi):
        return lo + (hi - lo) * self.draws.pop(0)


def restated(h, w, size, n, u, div):
    """The rule written out (issue, part 1) for six unit draws `u`, with the integer division handed in -> (st, ed, frames)."""
    from gomatching_amd import data
    lo, hi = 0.8, 1.2
    st = data.resize_crop_params(h, w, (size, size), lo + (hi - lo) * u[0], u[1], u[2])
    oh, ow = data.crop_window(st, (size, size))[2:]
    ed = data.resize_crop_params(oh, ow, (size, size), lo + (hi - lo) * u[3], u[4], u[5])
    frames = []
    for x in range(n):
        s = st[4] + (ed[4] - st[4]) * x / (n - 1)
        frames.append((int(h * s), int(w * s), st[2] + div((ed[2] - st[2]) * x, n - 1), st[3] + div((ed[3] - st[3]) * x, n - 1), s))
    return st, ed, frames


def floor_div(a, b):
    return a // b


def trunc_div(a, b):
    return int(a / b)


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "clip_motion.npz"))


def test_motion_clip_params_equal_the_reference_lines(gold):
    from gomatching_amd import data
    assert data.MOTION_SCALE_RANGE == (0.8, 1.2)
    shapes, mixed = set(), 0
    for case, ints, scales, target in zip(gold["cases"], gold["ints"], gold["img_scale"], gold["target"]):
        h, w, size, th, tw, n, k = (int(v) for v in case)
        msize = size if th < 0 and tw < 0 else th
        assert tuple(target) == (msize, msize)                                   # square, whatever TRAIN_H / TRAIN_W are
        np.random.seed(k)
        plan = data.motion_clip_params(h, w, msize, n, LegacyDraws)
        assert isinstance(plan, data.MotionPlan) and len(plan) == n
        for x, p in enumerate(plan):
            assert all(type(v) is int for v in p[:4]) and type(p[4]) is float
            assert list(p[:4]) == [int(v) for v in ints[x]], (case, x)
            assert np.float64(p[4]).tobytes() == np.float64(scales[x]).tobytes(), (case, x)
        shapes.add((h, w, size, th, tw, n))
        mixed += len({data.crop_window(p, (msize, msize))[2:] for p in plan}) > 1
    assert {s[:2] + s[5:] for s in shapes} >= {(c[0], c[1], c[3]) for c in SEVEN} and any(s[3] != s[4] for s in shapes)
    assert mixed > len(gold["cases"]) // 2                                       # mixed sizes are the normal case


def test_first_frame_is_st_last_offsets_are_eds_and_the_division_floors():
    from gomatching_amd import data
    g = np.random.default_rng(3)
    bites = 0
    for h, w, size, n in SEVEN:
        for _ in range(200):
            u = [float(v) for v in g.uniform(0, 1, 6)]
            st, ed, frames = restated(h, w, size, n, u, floor_div)
            plan = data.motion_clip_params(h, w, size, n, Replay(u))
            assert list(plan) == frames
            assert plan[0] == st                                                 # exactly, img_scale included
            assert plan[-1][2:4] == ed[2:4]
            if ed[2] < st[2] or ed[3] < st[3]:
                other = restated(h, w, size, n, u, trunc_div)[2]
                bites += other != frames
    assert bites > 0                      # some clip moves backwards by a distance n - 1 does not divide: truncation would differ


def test_a_non_square_target_still_gives_a_square_motion_target_and_train_len_1_is_refused():
    from gomatching_amd import data
    from gomatching_amd.config import merge_from_list
    cfg = mini_cfg("icdar15")
    merge_from_list(cfg, list(AUG_OPTS) + ["INPUT.VIDEO.TRAIN_LEN", "4"])
    m = data.GoMDatasetMapper(cfg, True, image_motion=True)
    assert m.target_size == (96, 128) and m.motion_size == 96 and m.image_motion
    video = {"video_id": 7, "images": [{"height": 96, "width": 128, "file_name": "x.png", "image_id": 1, "video_id": 7}]}
    records, plan = m.plan(video, np.random.default_rng(0))
    assert len(records) == 4 and all(r is video["images"][0] for r in records) and isinstance(plan, data.MotionPlan)
    for p in plan:
        y0, x0, oh, ow = data.crop_window(p, (96, 96))
        assert 0 < oh <= 96 and 0 < ow <= 96
    assert not data.GoMDatasetMapper(cfg, True).image_motion                     # opt-in
    merge_from_list(cfg, ["INPUT.VIDEO.TRAIN_LEN", "1"])
    with pytest.raises(ValueError, match="INPUT.VIDEO.TRAIN_LEN"):
        data.GoMDatasetMapper(cfg, True, image_motion=True)
    data.GoMDatasetMapper(cfg, True)                                             # without the flag nothing changes
    with pytest.raises(ValueError, match="train_len"):
        data.motion_clip_params(96, 128, 96, 1, np.random.default_rng(0))


@pytest.mark.parametrize("case", SEVEN, ids=lambda c: "%dx%d_%d_%d" % c)
def test_every_window_is_non_empty_and_inside_its_resized_image(case):
    from gomatching_amd import data
    h, w, size, n = case
    g = np.random.default_rng(h * 7 + w)
    mixed = 0
    for _ in range(2000):
        plan = data.motion_clip_params(h, w, size, n, g)
        sizes = set()
        for p in plan:
            y0, x0, oh, ow = data.crop_window(p, (size, size))
            assert oh > 0 and ow > 0 and y0 >= 0 and x0 >= 0 and y0 + oh <= p[0] and x0 + ow <= p[1], (case, p)
            assert oh <= size and ow <= size
            sizes.add((oh, ow))
        mixed += len(sizes) > 1
    assert mixed >= 0.7 * 2000, mixed


# ------------------------------------------------------------------------------------------------- mapper
def _cfg(opts=()):
    from gomatching_amd.config import merge_from_list
    cfg = mini_cfg("icdar15")
    merge_from_list(cfg, list(AUG_OPTS) + ["INPUT.NOT_CLAMP_BOX", "false", "INPUT.VIDEO.TRAIN_LEN", "4"] + list(opts))
    return cfg


SEED = 5


def _still_video(tmp_path):
    from gomatching_amd import data
    json_file, image_root = write_stills(str(tmp_path))
    videos = data.get_video_dataset_dicts([data.load_video_json(json_file, image_root)], gen_inst_id=True)
    assert len(videos) == 1 and len(videos[0]["images"]) == 1 and videos[0]["video_id"] == data.FIRST_GENERATED_ID
    return videos[0]


def test_mapper_on_the_host_makes_a_clip_of_one_still(tmp_path, monkeypatch):
    from gomatching_amd import data
    video = _still_video(tmp_path)
    reads = []
    real = data.read_image
    monkeypatch.setattr(data, "read_image", lambda path, fmt: (reads.append(path), real(path, fmt))[1])
    mapper = data.GoMDatasetMapper(_cfg(), True, device_ingest=False, image_motion=True)
    clip = mapper(video, np.random.default_rng(SEED))
    assert len(reads) == 1                                                       # decoded once per clip
    _, plan = mapper.plan(video, np.random.default_rng(SEED))
    assert len(clip) == 4 == len(plan)
    src = np.asarray(Image.open(video["images"][0]["file_name"]).convert("RGB"))
    assert mapper.image_format == "RGB"
    sizes = []
    for fr, p in zip(clip, plan):
        y0, x0, oh, ow = data.crop_window(p, (96, 96))
        sizes.append((oh, ow))
        assert fr["motion"] is True and "frame_u8" not in fr
        want = np.asarray(Image.fromarray(np.ascontiguousarray(src)).resize((p[1], p[0]), Image.BILINEAR))[y0:y0 + oh, x0:x0 + ow]
        assert fr["image"].dtype == torch.uint8 and tuple(fr["image"].shape) == (3, oh, ow)
        assert np.array_equal(fr["image"].numpy().transpose(1, 2, 0), want)
        assert (fr["image_id"], fr["video_id"], fr["height"], fr["width"]) == (9001, -1, 96, 128)
        inst = fr["instances"]
        want_boxes, want_fields, kept = [], {"beziers": [], "polyline": [], "boundary": []}, []
        for j, b in enumerate(training_boxes(0)):
            x = np.minimum(data.apply_box(b, p).clip(min=0), [ow, oh, ow, oh])
            if x[2] - x[0] > 1e-5 and x[3] - x[1] > 1e-5:
                kept.append(j)
                want_boxes.append(x)
                for key, val in data.bezier_fields(box_bezier(b)).items():
                    want_fields[key].append(data.apply_coords(val, p).reshape(-1))
        assert torch.equal(inst["gt_boxes"], torch.as_tensor(np.array(want_boxes).reshape(-1, 4), dtype=torch.float32))
        for key, width in (("beziers", 8), ("polyline", 50), ("boundary", 100)):
            assert torch.equal(inst[key], torch.as_tensor(np.array(want_fields[key]).reshape(-1, width), dtype=torch.float32)), key
        assert inst["gt_instance_ids"].tolist() == [data.FIRST_GENERATED_ID + j for j in kept]
    assert len(set(sizes)) >= 2, sizes                                           # this seed's frames differ in size
    ids = [fr["instances"]["gt_instance_ids"].tolist() for fr in clip]
    assert all(i == ids[0] for i in ids) and len(ids[0]) == 2 and min(ids[0]) >= data.FIRST_GENERATED_ID


def test_mapper_device_ingest_dicts_share_one_frame_and_carry_their_own_numbers(tmp_path):
    from gomatching_amd import data
    video = _still_video(tmp_path)
    clip = data.GoMDatasetMapper(_cfg(), True, device_ingest=True, image_motion=True)(video, np.random.default_rng(SEED))
    host = data.GoMDatasetMapper(_cfg(), True, device_ingest=False, image_motion=True)(video, np.random.default_rng(SEED))
    _, plan = data.GoMDatasetMapper(_cfg(), True, image_motion=True).plan(video, np.random.default_rng(SEED))
    assert len(clip) == 4
    for fr, h, p in zip(clip, host, plan):
        assert fr["frame_u8"] is clip[0]["frame_u8"] and "image" not in fr and fr["motion"] is True
        assert fr["frame_u8"].dtype == torch.uint8 and tuple(fr["frame_u8"].shape) == (96, 128, 3)
        assert fr["resize_hw"] == (p[0], p[1]) and fr["crop"] == data.crop_window(p, (96, 96)) and fr["flip_channels"] is False
        assert tuple(h["image"].shape[1:]) == fr["crop"][2:]
        assert torch.equal(fr["instances"]["gt_boxes"], h["instances"]["gt_boxes"])
    assert len({fr["crop"] for fr in clip}) > 1 and len({fr["resize_hw"] for fr in clip}) > 1
    # a video of several images goes through the code it always went through
    multi = {"video_id": 3, "images": [dict(video["images"][0], image_id=k) for k in (1, 2, 3, 4, 5)]}
    a = data.GoMDatasetMapper(_cfg(), True, image_motion=True)
    b = data.GoMDatasetMapper(_cfg(), True)
    pa, pb = a.plan(multi, np.random.default_rng(2)), b.plan(multi, np.random.default_rng(2))
    assert pa == pb and not isinstance(pa[1], data.MotionPlan)
    assert all("motion" not in fr for fr in a(multi, np.random.default_rng(2)))
    with pytest.raises(NotImplementedError, match="one image"):
        b.plan(video, np.random.default_rng(0))                                  # the default mapper refuses as before


def test_a_window_outside_its_resized_image_raises_naming_the_video(tmp_path, monkeypatch):
    from gomatching_amd import data
    video = _still_video(tmp_path)
    bad = data.MotionPlan([(72, 96, 0, 0, 0.75), (72, 96, 80, 0, 0.75), (72, 96, 0, 0, 0.75), (72, 96, 0, 0, 0.75)])
    monkeypatch.setattr(data, "motion_clip_params", lambda *a: bad)
    with pytest.raises(ValueError, match="video %d: frame 1" % data.FIRST_GENERATED_ID):
        data.GoMDatasetMapper(_cfg(), True, image_motion=True).plan(video, np.random.default_rng(0))


# ------------------------------------------------------------------------------------------------- loader
def _loader(tmp_path, workers=4, image_motion=True, **kw):
    from gomatching_amd import data
    root = os.path.join(str(tmp_path), "ds")
    if not os.path.isdir(root):
        write_stills(root, num_videos=2, num_stills=1, height=24, width=32, num_frames=9)
    cfg = _cfg(["INPUT.TRAIN_H", "24", "INPUT.TRAIN_W", "32", "INPUT.SCALE_RANGE", "[0.5, 2.0]", "INPUT.VIDEO.TRAIN_LEN", "3",
                "DATALOADER.NUM_WORKERS", str(workers)])
    recs = data.load_video_json(os.path.join(root, "train.json"), os.path.join(root, "frame"))
    mapper = data.GoMDatasetMapper(cfg, True, device_ingest=False, image_motion=image_motion)
    return data.build_vts_train_loader(cfg, mapper, dataset_dicts=recs, **kw)


def _clip_key(clip):
    return [(fr["image_id"], bool(fr.get("motion")), tuple(fr["image"].shape), fr["image"].numpy().tobytes(),
             fr["instances"]["gt_boxes"].numpy().tobytes(), tuple(fr["instances"]["gt_instance_ids"].tolist())) for fr in clip]


def test_loader_mixes_videos_and_stills_and_stays_a_pure_function_of_its_key(tmp_path):
    from gomatching_amd import data
    with pytest.raises(NotImplementedError, match="has one image"):
        _loader(tmp_path, image_motion=False, seed=11)
    a, b = _loader(tmp_path, workers=1, seed=11), _loader(tmp_path, workers=4, seed=11)
    with a, b:
        clips_a = [next(a) for _ in range(9)]
        clips_b = [next(b) for _ in range(9)]
    stills = 0
    for i in range(9):
        assert _clip_key(clips_a[i]) == _clip_key(clips_b[i]), i                 # 1 thread and 4 threads
        if clips_a[i][0].get("motion"):
            stills += 1
            assert len(clips_a[i]) == 3 and {fr["image_id"] for fr in clips_a[i]} == {9001}
            assert isinstance(a.plan(i)[2], data.MotionPlan)
            assert all(fr["instances"]["gt_instance_ids"].tolist() == clips_a[i][0]["instances"]["gt_instance_ids"].tolist()
                       and min(fr["instances"]["gt_instance_ids"].tolist(), default=data.FIRST_GENERATED_ID) >= data.FIRST_GENERATED_ID
                       for fr in clips_a[i])
        else:
            assert all("motion" not in fr for fr in clips_a[i]) and len({fr["image_id"] for fr in clips_a[i]}) == len(clips_a[i])
    assert stills == 3                                                           # one of three videos, three epochs
    with _loader(tmp_path, seed=11, start_iter=4) as c:                          # a resumed run
        for i in range(4, 9):
            assert _clip_key(next(c)) == _clip_key(clips_a[i]), i
    with _loader(tmp_path, seed=12) as d:
        assert [_clip_key(next(d)) for _ in range(3)] != [_clip_key(x) for x in clips_a[:3]]


# ---------------------------------------------------------------------------------------------------- ABI
def test_motion_entry_point_rejects_bad_descriptors_without_a_gpu():
    """As test_abi.py's argument test: every check runs before any HIP call, so nonsense comes back as GOM_ERR_INVALID_ARG.
    Every call below is invalid: a valid one would launch on whatever GPU is present, with these made-up pointers."""
    from gomatching_amd import lib, ops
    L = lib.load()
    INVALID = 1
    p = ctypes.c_void_p(0x1000)                                   # non-null, never dereferenced
    m = (ctypes.c_float * 3)(1, 2, 3)
    assert L.gom_resample_ksize_bilinear(8, 16) == 3 and L.gom_resample_ksize_bilinear(8, 4) == 5
    WORDS = 160                                                   # two tables of 8 -> 16: bounds 32 + kk 48 each
    good = dict(SH=16, SW=16, y0=0, x0=0, OH=16, OW=16, xks=3, yks=3, xb=0, xk=32, yb=80, yk=112)
    order = ("SH", "SW", "y0", "x0", "OH", "OW", "xks", "yks", "xb", "xk", "yb", "yk")
    assert len(order) == 12

    def call(T=1, src=p, tables=p, frames=True, mean=m, std=m, dst=p, H=8, W=8, PH=16, PW=16, words=WORDS, last=None, **over):
        rows = [[dict(good, **(over if (last is None or t == T - 1) else {}))[k] for k in order] for t in range(max(T, 1))]
        desc = (ctypes.c_int * (12 * len(rows)))(*[v for r in rows for v in r])
        return L.gom_ingest_motion_u8_hwc3_to_nhwc4(src, H, W, tables, words, desc if frames else None, T, mean, std, dst, PH, PW,
                                                    0, None)

    for bad in (dict(src=None), dict(tables=None), dict(frames=False), dict(mean=None), dict(std=None), dict(dst=None),
                dict(T=0), dict(T=-1), dict(T=17), dict(H=0), dict(W=-1), dict(PH=0), dict(PW=-3), dict(words=0),
                # a window outside its resized image ...
                dict(x0=-1), dict(y0=-1), dict(x0=1), dict(y0=1), dict(OH=17, PH=32), dict(OW=17, PW=32), dict(OH=0), dict(OW=-2),
                dict(SH=0), dict(SW=-1), dict(x0=2 ** 31 - 1, OW=2), dict(y0=15, OH=2),
                # ... or outside the padded frame
                dict(PH=15), dict(PW=15),
                # a tap count that is not gom_resample_ksize_bilinear's
                dict(xks=5), dict(yks=1), dict(xks=0), dict(SH=4, OH=4), dict(SW=4, OW=4),
                # a table that does not lie inside the buffer
                dict(xb=-1), dict(xk=-4), dict(yb=-1), dict(yk=-1), dict(xb=WORDS - 31), dict(xk=WORDS - 47), dict(yb=WORDS),
                dict(yk=113), dict(yk=2 ** 31 - 1), dict(words=159),
                # the LAST of several frames is checked as the first is
                dict(T=4, last=True, x0=1), dict(T=16, last=True, yk=113), dict(T=3, last=True, xks=5)):
        assert call(**bad) == INVALID, bad
    assert "gom_ingest_motion_u8_hwc3_to_nhwc4" in lib.SIGNATURES and ops.INGEST_MOTION_MAX_FRAMES == 16
    # the host half of the op: one buffer, descriptors that pass the checks above, shared tables stored once
    tables, desc, padded = ops.motion_tables(8, 8, [((16, 16), (0, 0, 16, 16)), ((16, 12), (3, 2, 5, 7)), ((16, 16), (15, 15, 1, 1))])
    assert tables.dtype == torch.int32 and tables.dim() == 1 and desc.dtype == torch.int32 and tuple(desc.shape) == (3, 12)
    assert padded == (16, 16) and desc[0].tolist() == [16, 16, 0, 0, 16, 16, 3, 3, 0, 32, 0, 32]      # 8 -> 16 serves both axes
    assert tables.numel() == 80 + 12 * 5 and desc[2].tolist()[6:] == desc[0].tolist()[6:]
    assert desc[1].tolist() == [16, 12, 3, 2, 5, 7, 3, 3, 80, 104, 0, 32]
    with pytest.raises(ValueError, match="1..16 frames"):
        ops.motion_tables(8, 8, [((16, 16), (0, 0, 16, 16))] * 17)
    with pytest.raises(ValueError, match="1..16 frames"):
        ops.motion_tables(8, 8, [])
    with pytest.raises(ValueError, match="not inside"):
        ops.motion_tables(8, 8, [((16, 16), (0, 1, 16, 16))])
    with pytest.raises(ValueError, match="CUDA uint8"):
        ops.ingest_motion(torch.zeros((8, 8, 3), dtype=torch.uint8), [((16, 16), (0, 0, 16, 16))], [0, 0, 0], [1, 1, 1], False)


# ---------------------------------------------------------------------------------------------------- CLI
def test_train_main_with_image_motion_gets_past_the_refusal_of_stills(tmp_path, capsys, monkeypatch):
    from gomatching_amd import eval as gom_eval
    from gomatching_amd import train
    json_file, image_root = write_stills(str(tmp_path), num_videos=1, num_stills=2)
    weights = os.path.join(str(tmp_path), "w.pth")
    torch.save({"model": {}}, weights)
    argv = ["--builtin", "icdar15", "--json", json_file, "--image-root", image_root, "--opts", "MODEL.WEIGHTS", weights,
            "OUTPUT_DIR", os.path.join(str(tmp_path), "out")]
    assert train.main(argv) == 2                                                 # as today
    assert "has one image" in capsys.readouterr().err

    class Reached(Exception):
        pass

    def stop(path):                                                              # the first thing `main` does once the data is accepted
        raise Reached(path)

    monkeypatch.setattr(gom_eval, "load_weights", stop)
    for extra in (["--image-motion"], ["--image-motion", "--host-ingest"]):
        with pytest.raises(Reached):
            train.main(argv[:6] + extra + argv[6:])
    assert train.main(argv[:6] + ["--image-motion"] + argv[6:] + ["INPUT.VIDEO.TRAIN_LEN", "1"]) == 2
    assert "TRAIN_LEN" in capsys.readouterr().err
    assert train.main(argv) == 2                                                 # the flag, not the patch, opened the door
    assert not os.path.exists(os.path.join(str(tmp_path), "out"))
