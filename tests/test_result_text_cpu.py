"""CPU: the result text rule and its host side -- the plain-Python statement against the reference writers' fixture and against
`results.write_video_results` on the GPU test's case list, `results.finish_points` against `finish_rows`, the per-character
byte tables against json and minidom themselves, `VideoResultWriter.add_text`, and the two refusals of `eval --device-write`
that need no GPU."""
import json
import os
import pickle
import random
import subprocess
import sys
from xml.dom.minidom import Document

import numpy as np
import pytest

import result_text_cases as rc
import result_text_statement as st

from gomatching_amd import lib, results
from gomatching_amd.predictor import TextDecoder

GOLD = os.path.join(os.path.dirname(__file__), "golden", "results_writer.json")


def test_statement_is_pinned_by_the_reference_writers():
    with open(GOLD, encoding="utf-8") as f:
        gold = json.load(f)
    seen = set()
    for name, ann in gold["videos"].items():
        assert list(ann.keys()) == [str(i + 1) for i in range(len(ann))]
        frames = [ann[str(i + 1)] for i in range(len(ann))]
        assert st.video_json(frames) == gold["json"][name], name
        assert st.video_xml(frames) == gold["xml"][name], name
        for rows in frames:
            seen.add("empty frame" if not rows else "")
            for row in rows:
                seen.add(len(row))
                seen.add(row[9])
    assert {'q"uote', "<tag>", "a&b", "中文", "", "empty frame", 10, 11} <= seen    # what the fixture is said to carry


def test_constants_are_the_headers():
    assert rc.SCAN_BLOCK == lib.CONSTANTS["GOM_RT_SCAN_BLOCK"] and rc.WORDS == lib.CONSTANTS["GOM_RESULT_ROWS_WORDS"]
    assert results.TEXT_ENTRY_BYTES == lib.CONSTANTS["GOM_RT_ENTRY_BYTES"]
    for name in ("POLY_I32", "POLY_F32", "RECS", "EMIT", "NHULL", "HULL_MASK", "EDGE", "TRACK_ID"):
        assert getattr(results, "_RR_" + name) == lib.CONSTANTS["GOM_RR_" + name]


@pytest.mark.parametrize("case", rc.cases(), ids=lambda c: c.name)
def test_statement_equals_write_video_results(case, tmp_path):
    assert rc.statement_text(case) == rc.writer_text(case, tmp_path)


def test_empty_frames_on_the_host_follow_the_statement():
    for first, count in ((0, 0), (0, 3), (8, 2), (998, 3)):
        js = "".join(st.frame_json(f, []) for f in range(first, first + count)).encode()
        xs = "".join(st.frame_xml(f, []) for f in range(first, first + count)).encode()
        assert results.host_text_of_empty_frames(first, count) == (js, xs)


def test_finish_points_are_finish_rows_points():
    rng = np.random.RandomState(5)
    n = 300
    words = np.zeros((n, 234), dtype=np.int32)
    P = rng.uniform(-20, 900, size=(n, 50, 2)).astype(np.float32)
    P[:40] = (P[:40, :1] + rng.uniform(0, 6, size=(40, 50, 2))).astype(np.float32)          # small ones: the extent filter drops some
    P[40:44] = P[40:44, :1]                                                                # a single distinct point
    words[:, 0:100] = P.reshape(n, 100).astype(np.int32)
    words[:, 100:200] = P.reshape(n, 100).view(np.int32)
    for k in range(n):                                                                     # the kernel's part, by the host's own functions
        hull = results._convex_hull(P[k].astype(np.float64))
        idx = [int(np.nonzero((P[k].astype(np.float64) == np.array(h)).all(1))[0][0]) for h in hull]
        words[k, 226] = len(hull)
        m = sum(1 << i for i in idx)
        words[k, 227:229] = np.array([m], dtype=np.uint64).view(np.int32)
        words[k, 229:231] = (idx[0], idx[1 % len(idx)]) if len(hull) >= 2 else (-1, -1)
    words[:, 200:225] = rng.randint(0, 40, size=(n, 25))
    words[:, 225] = rng.randint(0, 1 << 25, size=n)
    words[:, 232] = np.arange(n)
    decoder = TextDecoder(37)
    words[:, 200:225] = np.minimum(words[:, 200:225], 35)
    for min_extent in (5, 40):
        pts, keep = results.finish_points(words, min_extent)
        rows = results.finish_rows(words, decoder, min_extent)
        assert pts.dtype == np.int64 and pts.shape == (n, 8) and keep.dtype == bool and 0 < keep.sum() < n
        for k in range(n):
            assert (rows[k] is not None) == bool(keep[k])
            if keep[k]:
                assert rows[k][:8] == pts[k].tolist()
    pts, keep = results.finish_points(words[:0])
    assert pts.shape == (0, 8) and keep.shape == (0,) and results.finish_rows(words[:0], decoder) == []


def _minidom_value(s):
    e = Document().createElement("a")
    e.setAttribute("v", s)
    x = e.toxml()
    return x[len('<a v="'):-len('"/>')]


def _table_text(tab, ids):
    return b"".join(bytes(tab[i, 1:1 + tab[i, 0]]) for i in ids)


def test_text_tables_are_the_libraries_own_escapes(tmp_path):
    custom = str(tmp_path / "dict.pkl")
    with open(custom, "wb") as f:
        pickle.dump([ord(c) for c in rc.CUSTOM], f)
    assert {'"', "\\", "&", "<", ">", "'", "\x7f"} <= set(rc.CUSTOM)
    assert {1, 2, 3, 4} == {len(c.encode("utf-8")) for c in rc.CUSTOM}
    rnd = random.Random(11)
    for decoder in (TextDecoder(37), TextDecoder(96), TextDecoder(len(rc.CUSTOM) + 1, custom)):
        jt, xt = results.text_tables(decoder)
        n = decoder.voc_size - 1
        assert jt.shape == xt.shape == (n, 8) and jt.dtype == xt.dtype == np.uint8
        assert jt[:, 0].max() <= 7 and xt[:, 0].max() <= 7 and jt[:, 0].min() >= 1
        for i, ch in enumerate(decoder.labels):
            assert _table_text(jt, [i]).decode("utf-8") == st.json_char(ch)          # and the statement's escapes are the same
            assert _table_text(xt, [i]).decode("utf-8") == st.xml_char(ch)
        for _ in range(200):                                                          # both libraries escape per character
            ids = [rnd.randrange(n) for _ in range(rnd.randrange(0, 26))]
            s = "".join(decoder.labels[i] for i in ids)
            assert _table_text(jt, ids) == json.dumps(s, ensure_ascii=False)[1:-1].encode("utf-8")
            assert _table_text(xt, ids) == _minidom_value(s).encode("utf-8")
    with pytest.raises(ValueError):
        results.text_tables(rc.Labels(["a", "\ud800"]))                               # no UTF-8 form


def _whole(case, tmp_path, name):
    out = tmp_path / name
    frames = case.frames()
    (out / "jsons").mkdir(parents=True)
    (out / "preds").mkdir()
    results.write_video_results({str(f + 1): rows for f, rows in enumerate(frames)}, str(out / "jsons" / "v.json"),
                                str(out / "preds" / "res_v.xml"))
    return (out / "jsons" / "v.json").read_bytes(), (out / "preds" / "res_v.xml").read_bytes()


@pytest.mark.parametrize("cuts", ((3,), (2, 4), (0, 6)))
def test_add_text_in_pieces_gives_the_files_of_one_write(cuts, tmp_path):
    case = {c.name: c for c in rc.cases()}["six-frames"]
    want = _whole(case, tmp_path, "whole")
    w = results.VideoResultWriter("v", "OTHER", str(tmp_path / "pieces"))
    edges = [0] + list(cuts) + [6]
    for a, b in zip(edges[:-1], edges[1:]):
        js, xs = rc.statement_text(case.part(a, b))
        w.add_text(a, b - a, js, xs)
        assert not os.path.exists(w.json_path) and not os.path.exists(w.xml_path)       # under .partial/ until close()
    assert w.frames == 6
    jp, xp = w.close()
    assert (open(jp, "rb").read(), open(xp, "rb").read()) == want
    assert not os.path.exists(str(tmp_path / "pieces" / ".partial"))


def test_add_text_without_frames_is_the_empty_video(tmp_path):
    w = results.VideoResultWriter("v", "OTHER", str(tmp_path / "a"))
    w.add_text(0, 0, b"", b"")
    jp, xp = w.close()
    assert open(jp, "rb").read() == b"{}" and open(xp, "rb").read() == b'<?xml version="1.0" ?>\n'
    assert (st.video_json([]), st.video_xml([])) == ("{}", '<?xml version="1.0" ?>\n')


def test_add_text_order_mixing_and_abort(tmp_path):
    case = {c.name: c for c in rc.cases()}["six-frames"]
    js, xs = rc.statement_text(case.part(0, 3))
    w = results.VideoResultWriter("v", "OTHER", str(tmp_path / "o"))
    with pytest.raises(ValueError, match="in order"):
        w.add_text(3, 3, *rc.statement_text(case.part(3, 6)))
    w.add_text(0, 3, js, xs)
    with pytest.raises(ValueError, match="in order"):
        w.add_text(0, 3, js, xs)
    with pytest.raises(ValueError, match="not both"):
        w.add(3, [])
    w.abort()
    left = [os.path.join(d, f) for d, _, fs in os.walk(str(tmp_path / "o")) for f in fs]
    assert left == []
    with pytest.raises(ValueError, match="closed"):
        w.add_text(3, 3, js, xs)
    w2 = results.VideoResultWriter("v", "OTHER", str(tmp_path / "m"))
    w2.add(0, [])
    with pytest.raises(ValueError, match="not both"):
        w2.add_text(1, 2, b"x", b"y")
    w2.abort()


def _eval(tmp_path, *flags, env=None):
    (tmp_path / "in").mkdir(exist_ok=True)
    return subprocess.run([sys.executable, "-m", "gomatching_amd.eval", "--builtin", "icdar15", "--input", str(tmp_path / "in"),
                           "--output", str(tmp_path / "out")] + list(flags), capture_output=True, text=True, env=env)


def test_device_write_does_not_go_with_host_rows(tmp_path):
    r = _eval(tmp_path, "--device-write", "--host-rows")
    assert r.returncode == 2 and "--device-write" in r.stderr and "--host-rows" in r.stderr
    assert not (tmp_path / "out").exists()


def test_device_write_without_a_gpu_is_an_error_not_a_fallback(tmp_path):
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1")      # the child sees no device, wherever it runs
    r = _eval(tmp_path, "--device-write", env=env)
    assert r.returncode == 1 and "--device-write needs a GPU" in r.stderr
    assert not (tmp_path / "out").exists()
