"""CPU: `python -m gomatching_amd.prepare` -- the converters against the files the REFERENCE's own scripts wrote for the same raw
tree (tests/golden/prepare_raw/, tools/gen_golden_prepare.py), the error exits, and the end to end the command exists for: a
converted ICDAR15 tree that `GoMDatasetMapper` maps under MODEL.ROI_HEADS.WITH_RESR."""
import ctypes
import json
import os

import numpy as np
import pytest

import prepare_fixture as F
from helpers import mini_cfg
from gomatching_amd import data, prepare


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    return F.build_tree(str(tmp_path_factory.mktemp("prepare_raw")))


@pytest.mark.parametrize("name", ["icdar15", "dstext", "bovtext"])
def test_converter_writes_the_references_bytes(tree, name):
    """`--no-bezier` with the video order the reference's script saw: byte-identical."""
    doc = prepare.CONVERTERS[name](*tree[name], video_order=F.video_order()[name])
    assert prepare.dumps(doc).encode("utf-8") == F.reference_json(name)


@pytest.mark.parametrize("name", ["dstext", "bovtext"])
def test_command_no_bezier_is_the_references_file_where_sorted_order_is_its_order(tree, name, tmp_path):
    assert F.video_order()[name] == sorted(F.video_order()[name])
    out = str(tmp_path / "train.json")
    assert prepare.main([name, "--annotations", tree[name][0], "--frames", tree[name][1], "--output", out, "--no-bezier"]) == 0
    with open(out, "rb") as f:
        assert f.read() == F.reference_json(name)


def test_sorted_order_renumbers_as_documented(tree, tmp_path):
    """The ICDAR15 script took Video_5_2_0 first; the command takes the videos sorted, Video_18_3_1 first.  Ids are then
    numbered in that order, and nothing else changes."""
    order = F.video_order()["icdar15"]
    assert order != sorted(order)
    out = str(tmp_path / "train.json")
    assert prepare.main(["icdar15", "--annotations", tree["icdar15"][0], "--frames", tree["icdar15"][1], "--output", out,
                         "--no-bezier"]) == 0
    with open(out, encoding="utf-8") as f:
        got = json.load(f)
    ref = json.loads(F.reference_json("icdar15").decode("utf-8"))
    assert [v["file_name"] for v in got["videos"]] == sorted(v["file_name"] for v in ref["videos"])
    assert [v["id"] for v in got["videos"]] == [1, 2]
    assert [im["id"] for im in got["images"]] == list(range(1, len(ref["images"]) + 1))
    assert [a["id"] for a in got["annotations"]] == list(range(1, len(ref["annotations"]) + 1))
    assert got["categories"] == ref["categories"]

    def keyed(doc):
        video = {v["id"]: v["file_name"] for v in doc["videos"]}
        image = {im["id"]: im for im in doc["images"]}
        images = {im["file_name"]: (im["height"], im["width"], im["frame_id"], video[im["video_id"]],
                                    image.get(im["prev_image_id"], {}).get("file_name"), image.get(im["next_image_id"], {}).get("file_name"))
                  for im in doc["images"]}
        anns = sorted((image[a["image_id"]]["file_name"], a["instance_id"], json.dumps({k: v for k, v in a.items() if k not in ("id", "image_id")},
                                                                                  sort_keys=True)) for a in doc["annotations"])
        return images, anns
    assert keyed(got) == keyed(ref)
    first = [im for im in got["images"] if im["video_id"] == 1]
    assert first[0]["prev_image_id"] == -1 and first[-1]["next_image_id"] == -1 and first[0]["file_name"] == "Video_18_3_1/1.jpg"


def test_reference_fixture_covers_the_branches():
    """What the raw tree was built to exercise shows in the reference's own output."""
    ic = json.loads(F.reference_json("icdar15").decode("utf-8"))
    ds = json.loads(F.reference_json("dstext").decode("utf-8"))
    bov = json.loads(F.reference_json("bovtext").decode("utf-8"))
    image = {im["id"]: im for im in ic["images"]}
    late = [(image[a["image_id"]]["frame_id"], a["instance_id"]) for a in ic["annotations"]
            if image[a["image_id"]]["file_name"].startswith("Video_18_3_1/")]
    assert (133, 65007) in late and (134, 65007) not in late and (135, 65001) in late and (136, 65001) not in late and (137, 65002) in late
    assert {a["text_category"] for a in ic["annotations"]} == {"alphanumeric", "nonalphanumeric", "other"}
    first = [a for a in ic["annotations"] if image[a["image_id"]]["file_name"] == "Video_5_2_0/1.jpg"]
    assert [a["instance_id"] for a in first] == [1001, 1002, 1003]                   # the repeated 1001 is skipped
    assert any(min(min(p) for p in a["poly"]) < 0 for a in ic["annotations"])
    assert [a["instance_id"] for a in ds["annotations"][:3]] == [7, 7, 9]             # "7" and "07" differ as strings
    assert {a["anno_type"] for a in bov["annotations"]} == {"line"}
    assert bov["annotations"][1]["poly"][0] == [-3, 0]                               # -3.9, -0.5 truncated toward zero


# ------------------------------------------------------------------------------------------------- error exits
def _run(capsys, argv):
    status = prepare.main(argv)
    return status, capsys.readouterr().err


def test_error_exits_name_the_file(tree, tmp_path, capsys):
    import shutil
    ann, frames = tree["icdar15"]
    out = str(tmp_path / "train.json")
    status, err = _run(capsys, ["icdar15", "--annotations", str(tmp_path / "nowhere"), "--frames", frames, "--output", out, "--no-bezier"])
    assert status == 2 and "nowhere" in err
    status, err = _run(capsys, ["dstext", "--annotations", tree["dstext"][0], "--frames", str(tmp_path / "noframes"), "--output", out])
    assert status == 2 and "noframes" in err
    # a video without 1.jpg
    broken = str(tmp_path / "frames_a")
    shutil.copytree(frames, broken)
    os.remove(os.path.join(broken, "Video_5_2_0", "1.jpg"))
    status, err = _run(capsys, ["icdar15", "--annotations", ann, "--frames", broken, "--output", out, "--no-bezier"])
    assert status == 2 and os.path.join("Video_5_2_0", "1.jpg") in err
    # a frame-count mismatch: the reference's `assert num_images == len(Frames)`
    broken = str(tmp_path / "frames_b")
    shutil.copytree(frames, broken)
    os.remove(os.path.join(broken, "Video_5_2_0", "3.jpg"))
    status, err = _run(capsys, ["icdar15", "--annotations", ann, "--frames", broken, "--output", out, "--no-bezier"])
    assert status == 2 and "Video_5_2_0_GT.xml" in err and "Video_5_2_0 " in err and "2 frames" in err and "3 in" in err
    broken = str(tmp_path / "frames_c")
    shutil.copytree(tree["dstext"][1], broken)
    os.remove(os.path.join(broken, "Driving", "Video_44_6_4", "2.jpg"))
    status, err = _run(capsys, ["dstext", "--annotations", tree["dstext"][0], "--frames", broken, "--output", out, "--no-bezier"])
    assert status == 2 and "Video_44_6_4" in err
    assert not os.path.exists(out)
    # a bad point count: the reference's ValueError('Error Num of points'), with the annotation's id
    doc = json.loads(F.reference_json("dstext").decode("utf-8"))
    doc["annotations"][2]["poly"] = doc["annotations"][2]["poly"] + [[1, 2]]
    bad = str(tmp_path / "five_points.json")
    with open(bad, "w", encoding="utf-8") as f:
        f.write(prepare.dumps(doc))
    status, err = _run(capsys, ["bezier", "--json", bad, "--output", out, "--host-bezier"])
    assert status == 2 and "five_points.json" in err and "Error Num of points" in err and "annotation %d" % doc["annotations"][2]["id"] in err
    status, err = _run(capsys, ["bezier", "--json", str(tmp_path / "missing.json"), "--output", out, "--host-bezier"])
    assert status == 2 and "missing.json" in err
    assert not os.path.exists(out)


def test_device_path_is_refused_without_a_gpu_instead_of_falling_back(tmp_path, capsys):
    import torch
    src, out = str(tmp_path / "ref.json"), str(tmp_path / "out.json")
    with open(src, "wb") as f:
        f.write(F.reference_json("dstext"))
    status, err = _run(capsys, ["bezier", "--json", src, "--output", out])
    if torch.cuda.is_available():
        assert status == 0 and os.path.exists(out)
    else:
        assert status == 1 and "--host-bezier" in err and not os.path.exists(out)


def test_abi_rejects_bad_arguments_without_a_gpu():
    from gomatching_amd import lib
    L = lib.load()
    p, odd = ctypes.c_void_p(0x1000), ctypes.c_void_p(0x1004)
    assert L.gom_quad_bezier_i32(p, p, -1, p, None) == 1
    assert L.gom_quad_bezier_i32(None, p, 4, p, None) == 1
    assert L.gom_quad_bezier_i32(p, None, 4, p, None) == 1
    assert L.gom_quad_bezier_i32(p, p, 4, None, None) == 1
    assert L.gom_quad_bezier_i32(odd, p, 4, p, None) == 1                            # a quad is read as two 16-byte words
    assert L.gom_quad_bezier_i32(p, odd, 4, p, None) == 1
    assert L.gom_quad_bezier_i32(p, p, 4, odd, None) == 1
    assert L.gom_quad_bezier_i32(None, None, 0, None, None) == 0                     # n == 0: GOM_OK, nothing launched


# ------------------------------------------------------------------------------------------------- bezier_pts
def test_bezier_pts_sits_after_poly_and_is_ints_for_quads_floats_for_14gons(tmp_path):
    doc = json.loads(F.reference_json("bovtext").decode("utf-8"))
    curve = [[10 + 15 * k, 50 + (k - 3) ** 2] for k in range(7)] + [[100 - 15 * k, 75 + (3 - k) ** 2] for k in range(7)]
    doc["annotations"][0]["poly"] = curve
    already = [1.0 * v for v in range(16)]
    doc["annotations"][1] = dict(doc["annotations"][1], bezier_pts=already)
    src, out = str(tmp_path / "in.json"), str(tmp_path / "out.json")
    with open(src, "w", encoding="utf-8") as f:
        f.write(prepare.dumps(doc))
    assert prepare.main(["bezier", "--json", src, "--output", out, "--host-bezier"]) == 0
    with open(out, encoding="utf-8") as f:
        got = json.load(f)
    size = {im["id"]: (im["height"], im["width"]) for im in got["images"]}
    import prepare_statement as S
    for k, a in enumerate(got["annotations"]):
        keys = list(a)
        assert len(a["bezier_pts"]) == 16
        if k == 1:
            assert a["bezier_pts"] == already                                          # left alone
            continue
        assert keys[keys.index("poly") + 1] == "bezier_pts", keys
        if k == 0:
            assert all(isinstance(v, float) for v in a["bezier_pts"]) and a["bezier_pts"] == prepare.fit_14gon(curve)
        else:
            assert all(isinstance(v, int) for v in a["bezier_pts"])
            assert a["bezier_pts"] == S.quad_bezier(np.array(a["poly"]).reshape(-1), *size[a["image_id"]])
        assert {kk: v for kk, v in a.items() if kk != "bezier_pts"} == doc["annotations"][k]
    # a json whose annotations all carry the field goes through byte for byte, whatever its formatting
    compact = str(tmp_path / "compact.json")
    with open(compact, "w", encoding="utf-8") as f:
        json.dump(got, f, ensure_ascii=True, separators=(",", ":"))
    again = str(tmp_path / "again.json")
    assert prepare.main(["bezier", "--json", compact, "--output", again]) == 0        # no device is needed for a copy
    with open(compact, "rb") as f, open(again, "rb") as g:
        assert f.read() == g.read()


# ------------------------------------------------------------------------------------------------- the end to end
def test_converted_icdar15_tree_maps_under_with_resr(tree, tmp_path):
    """What fails without this command: the headline config has WITH_RESR, the converters' json has `poly` only, and the mapper
    then raises "`bezier_pts` must be precomputed in the json"."""
    cfg = mini_cfg("icdar15")
    assert cfg.MODEL.ROI_HEADS.WITH_RESR
    ann, frames = tree["icdar15"]
    out = str(tmp_path / "train.json")
    assert prepare.main(["icdar15", "--annotations", ann, "--frames", frames, "--output", out, "--host-bezier"]) == 0
    with open(out, encoding="utf-8") as f:
        doc = json.load(f)
    assert all(len(a["bezier_pts"]) == 16 for a in doc["annotations"])
    by_image = {}
    for a in doc["annotations"]:
        by_image.setdefault(a["image_id"], []).append(a)
    videos = data.get_video_dataset_dicts([data.load_video_json(out, frames)])
    video = [v for v in videos if os.path.basename(os.path.dirname(v["images"][0]["file_name"])) == "Video_5_2_0"][0]
    mapper = data.GoMDatasetMapper(cfg, True, device_ingest=False)
    records, params = mapper.plan(video, np.random.default_rng(3))
    clip = [mapper.map_frame(r, params) for r in records]
    assert len(clip) == 3
    total = 0
    for rec, fr in zip(records, clip):
        inst = fr["instances"]
        n = inst["gt_boxes"].shape[0]
        total += n
        fields = {"polyline": (25, 2), "boundary": (50, 2), "beziers": (4, 2)}
        want = [data.bezier_fields(a["bezier_pts"]) for a in by_image[rec["image_id"]]]
        for key, shape in fields.items():
            got = inst[key].reshape((n,) + shape).numpy()
            assert got.shape == (n,) + shape and np.isfinite(got).all()
            rows = [data.apply_coords(w[key], params).astype(np.float32) for w in want]
            k = 0
            for g in got:                                        # the kept instances are a subsequence of the record's annotations
                while k < len(rows) and not np.array_equal(rows[k], g):
                    k += 1
                assert k < len(rows), (key, rec["file_name"])
                k += 1
    assert total >= 3
    # the same json without the field is what the mapper refuses
    plain = str(tmp_path / "plain.json")
    assert prepare.main(["icdar15", "--annotations", ann, "--frames", frames, "--output", plain, "--no-bezier"]) == 0
    video = [v for v in data.get_video_dataset_dicts([data.load_video_json(plain, frames)])
             if os.path.basename(os.path.dirname(v["images"][0]["file_name"])) == "Video_5_2_0"][0]
    with pytest.raises(ValueError, match="must be precomputed"):
        mapper(video, np.random.default_rng(3))
