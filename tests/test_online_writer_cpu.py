"""`results.VideoResultWriter` writes, frame by frame, the bytes `results.write_video_results` writes for the whole annotation;
until `close()` nothing under preds/ looks like a finished video."""
import os

import pytest

from gomatching_amd import eval as E
from gomatching_amd import results

TEXTS = ["plain", "a&b", "<tag>", "x>y", 'say "hi"', "it's", "& < > \" '", "中文文本", "テキスト mixed", "",
         " lead", "tab\tin", "back\\slash"]


def _row(k, text, fields):
    pts = [10 + k, 20, 110 + k, 22, 108 + k, 60, 8 + k, 58]
    row = pts + [k * 7 + 1 + (1 << 33) * (k % 2), text]
    if fields == 11:
        row.append([[[pts[0], pts[1]], [pts[2], pts[3]], [pts[4], pts[5]], [pts[6], pts[7]], [-3, 0]]])
    return row


def _annotation(frames):
    """Frame i (0-based) -> rows; an empty frame, rows of 10 and of 11 fields, every text of TEXTS."""
    out = []
    for i in range(frames):
        if i % 7 == 3:
            out.append([])
            continue
        n = 1 + i % 4
        out.append([_row(i * 5 + j, TEXTS[(i + 3 * j) % len(TEXTS)], 10 if (i + j) % 3 == 0 else 11) for j in range(n)])
    return out


def _read(path):
    with open(path, "rb") as f:
        return f.read()


@pytest.mark.parametrize("frames", [1, 4, 250])
@pytest.mark.parametrize("data_type,video,xml_stem", [("ICDAR15", "Video_35_2_3", "video_35"), ("DSText", "Cls9_vid", "Cls9_vid")])
def test_incremental_files_equal_the_whole_annotation_files(tmp_path, frames, data_type, video, xml_stem):
    rows = _annotation(frames)
    if frames == 1:
        rows = [[_row(j, t, 11 - j % 2) for j, t in enumerate(TEXTS)]]
    whole, inc = tmp_path / "whole", tmp_path / "inc"
    os.makedirs(str(whole))
    results.write_video_results({str(i + 1): r for i, r in enumerate(rows)}, str(whole / "v.json"), str(whole / "v.xml"))
    w = results.VideoResultWriter(video, data_type, str(inc))
    for i, r in enumerate(rows):
        w.add(i, r)
        assert not [f for f in os.listdir(str(inc / "preds")) if f.startswith("res_")]
        assert not os.listdir(str(inc / "jsons"))
        assert xml_stem not in E.written_videos(str(inc / "preds"))
    json_path, xml_path = w.close()
    assert json_path == str(inc / "jsons" / (video + ".json")) and xml_path == str(inc / "preds" / ("res_%s.xml" % xml_stem))
    assert _read(xml_path) == _read(str(whole / "v.xml"))
    assert _read(json_path) == _read(str(whole / "v.json"))
    assert E.written_videos(str(inc / "preds")) == {xml_stem}
    assert not os.path.exists(str(inc / ".partial"))
    assert w.close() == (json_path, xml_path)
    results.write_track_transcriptions(str(inc / "preds"))             # parses what the writer left
    assert os.path.isfile(str(inc / "preds" / ("res_%s.txt" % xml_stem)))


def test_empty_frames_only_and_order(tmp_path):
    whole, inc = tmp_path / "whole", tmp_path / "inc"
    os.makedirs(str(whole))
    results.write_video_results({"1": [], "2": []}, str(whole / "v.json"), str(whole / "v.xml"))
    w = results.VideoResultWriter("v", "OTHER", str(inc))
    w.add(0, [])
    with pytest.raises(ValueError):
        w.add(2, [])
    w.add(1, [])
    json_path, xml_path = w.close()
    assert _read(xml_path) == _read(str(whole / "v.xml")) and _read(json_path) == _read(str(whole / "v.json"))
    with pytest.raises(ValueError):
        w.add(2, [])


def test_abort_leaves_nothing_that_looks_like_a_result(tmp_path):
    w = results.VideoResultWriter("v", "OTHER", str(tmp_path))
    w.add(0, [_row(0, "x", 11)])
    w.abort()
    assert E.written_videos(str(tmp_path / "preds")) == set()
    assert not os.listdir(str(tmp_path / "jsons")) and not os.listdir(str(tmp_path / ".partial"))
