"""Result rows without a GPU: the host finishing of the device row path (`results.finish_rows`), fed by the plain-Python
statement of the kernel (result_rows_statement.py), against `results.frame_lines`; the CPU fallback of `clip_lines`; and
the listing / naming / argument handling of `python -m gomatching_amd.eval`.

Comparison (b) of the two the feature keeps apart: statement + finishing must give the rows of `frame_lines`, except
instances the host itself decides by rounding (`near_tie`: its two smallest distinct edge areas within a relative 1e-12),
of which at most 0.1 % of a family may be left out.  Measured: 0 rows differing in 26 600, none left out."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import result_rows_statement as S
from gomatching_amd import results as R
from gomatching_amd.predictor import TextDecoder, boundary_to_polygon
from gomatching_amd.structures import Instances

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _instances(bd, recs, ids):
    inst = Instances((720, 1280))
    inst.bd = torch.as_tensor(np.asarray(bd, dtype=np.float32))
    inst.recs = torch.as_tensor(np.asarray(recs, dtype=np.int64))
    inst.track_ids = torch.as_tensor(np.asarray(ids, dtype=np.int64))
    return inst


@pytest.mark.parametrize("name", list(S.FAMILY_COUNTS))
def test_statement_and_finishing_equal_frame_lines(name):
    bd = S.family(name)
    n = len(bd)
    recs = S.random_recs(n, 37, seed=n)
    ids = np.arange(n, dtype=np.int64) * 7 + 1
    dec = TextDecoder(37)
    # min_extent = 0 keeps every instance (extents are >= 0), so rows align with instances on both sides
    want = R.frame_lines(_instances(bd, recs, ids), dec, min_extent=0)
    got = R.finish_rows(S.statement_words(bd, recs, 37, ids), dec, min_extent=0)
    assert len(want) == len(got) == n
    differ = [k for k in range(n) if got[k] != want[k]]
    near = [k for k in differ if S.near_tie(boundary_to_polygon(bd[k]))]
    print("%-6s instances %5d  rows differing %d  of them near-ties left out %d" % (name, n, len(differ), len(near)))
    assert len(near) <= n // 1000                                       # the cap: 0.1 % of the family
    assert differ == near, "rows differ where the host's areas are not within rounding: %s" % (
        [k for k in differ if k not in near][:5],)
    for k in (0, n // 2, n - 1):                                        # the rows carry python ints, str and nested lists
        r = got[k]
        assert all(type(v) is int for v in r[:9]) and type(r[9]) is str and np.asarray(r[10]).shape == (1, 50, 2)


def test_extent_filter_and_empty_frame():
    dec = TextDecoder(37)
    t = np.linspace(0, 1, 25)

    def box(w, h):
        xs = 10 + t * w
        return np.stack([xs, np.full(25, 20.0), xs, np.full(25, 20.0 + h)], 1).astype(np.float32)

    bd = np.stack([box(4, 50), box(5, 50), box(50, 4), box(50, 5), box(0, 0), box(40, 0)])
    recs = S.random_recs(len(bd), 37, seed=1)
    ids = np.arange(len(bd), dtype=np.int64) + 3
    want = R.frame_lines(_instances(bd, recs, ids), dec)
    got = R.finish_rows(S.statement_words(bd, recs, 37, ids), dec)
    assert [r is not None for r in got] == [False, True, False, True, False, False]
    assert [r for r in got if r is not None] == want and [r[8] for r in want] == [4, 6]
    assert R.finish_rows(np.zeros((0, S.WORDS), np.int32), dec) == []
    empty = _instances(np.zeros((0, 25, 4)), np.zeros((0, 25)), np.zeros((0,)))
    assert R.clip_lines([{"instances": empty}, {"instances": empty}], dec) == [[], []]


@pytest.mark.parametrize("voc", [37, 5462])
def test_emit_mask_equals_text_decoder(voc, tmp_path):
    dec = S.decoder_for(voc, tmp_path)
    n = 400
    recs = S.random_recs(n, voc, seed=voc)
    bd = S.family("axis", 1).repeat(n, 0) + np.float32(30)              # one kept box for every row of recs
    bd[:, :, 3] += 30
    bd[:, :, 0::2] += (np.linspace(0, 1, 25) * 30).astype(np.float32)[None, :, None]
    rows = R.finish_rows(S.statement_words(bd, recs, voc, np.zeros(n, np.int64)), dec, min_extent=0)
    assert [r[9] for r in rows] == [dec.decode(r) for r in recs]
    assert rows[1][9] == "" and len(rows[2][9]) == 1                    # all-blank row, all-equal row
    for r in recs[:50]:
        mask = S.emit_mask(r.tolist(), voc)
        assert "".join(dec._table[r[[c for c in range(25) if mask >> c & 1]]]) == dec.decode(r)


def _clip(frames=4):
    dec = TextDecoder(37)
    out, rng = [], np.random.default_rng(9)
    for f in range(frames):
        n = [5, 0, 12, 1][f % 4]
        bd = S.family("smooth", 40)[rng.permutation(40)[:n]] if n else np.zeros((0, 25, 4), np.float32)
        out.append({"instances": _instances(bd, S.random_recs(n, 37, seed=f), rng.integers(1, 99, n))})
    return out, dec


def test_clip_lines_cpu_fallback_equals_frame_lines():
    results, dec = _clip()
    want = [R.frame_lines(r["instances"], dec) for r in results]
    assert R.clip_lines(results, dec) == want
    assert sum(len(w) for w in want) > 0 and want[1] == []


def test_write_video_device_rows_writes_the_same_bytes(tmp_path):
    results, dec = _clip()
    a, b = tmp_path / "a", tmp_path / "b"
    ann_a = R.write_video(results, "Video_5_1_2", "ICDAR15", str(a), dec)
    ann_b = R.write_video(results, "Video_5_1_2", "ICDAR15", str(b), dec, device_rows=True)
    assert ann_a == ann_b
    for rel in ("preds/res_video_5.xml", "jsons/Video_5_1_2.json"):
        assert (a / rel).read_bytes() == (b / rel).read_bytes() and (a / rel).stat().st_size > 0


# ------------------------------------------------------------------------------------------------ command line
def _tree(root, videos, frames=("10.jpg", "2.jpg", "1.jpg")):
    for v in videos:
        os.makedirs(os.path.join(root, v))
        for f in frames:
            open(os.path.join(root, v, f), "wb").close()


def test_list_videos_and_frame_paths(tmp_path):
    from gomatching_amd import eval as E
    ic = str(tmp_path / "ICDAR15" / "test")
    _tree(ic, ["Video_5_1_2", "Video_17_3_1"])
    dt, vids = E.list_videos(ic)
    assert dt == "ICDAR15" and [n for n, _ in vids] == ["Video_17_3_1", "Video_5_1_2"]
    assert [os.path.basename(p) for p in E.frame_paths(vids[0][1])] == ["1.jpg", "2.jpg", "10.jpg"]
    assert [R.result_names(n, dt)[0] for n, _ in vids] == ["video_17", "video_5"]
    # resume: the XML stem decides, not the raw video name
    preds = tmp_path / "out" / "preds"
    preds.mkdir(parents=True)
    (preds / "res_video_5.xml").write_text("<Frames/>")
    (preds / "res_video_5.txt").write_text("")
    assert E.written_videos(str(preds)) == {"video_5"}
    assert [n for n, _ in E.list_videos(ic, done=E.written_videos(str(preds)))[1]] == ["Video_17_3_1"]
    assert E.written_videos(str(tmp_path / "nowhere")) == set()
    # DSText / BOVText: video directories one level deeper; the damaged BOVText video is skipped
    bov = str(tmp_path / "BOVText" / "frames")
    _tree(bov, ["Cls1_Livestreaming/Cls1_Livestreaming_video40", "Cls1_Livestreaming/Cls1_Livestreaming_video41",
                "Cls2_Cartoon/Cls2_Cartoon_video1"])
    dt, vids = E.list_videos(bov)
    assert dt == "BOVText" and [n for n, _ in vids] == ["Cls1_Livestreaming_video41", "Cls2_Cartoon_video1"]
    assert all(os.path.isdir(d) for _, d in vids)
    ds = str(tmp_path / "DSText_frames")
    _tree(ds, ["Activity/Video_1", "Game/Video_2"])
    assert E.list_videos(ds)[0] == "DSText" and [n for n, _ in E.list_videos(ds)[1]] == ["Video_1", "Video_2"]
    other = str(tmp_path / "clips")
    _tree(other, ["a", "b"])
    assert E.list_videos(other, done={"a"}) == ("OTHER", [("b", os.path.join(other, "b"))])


def test_parser_options():
    from gomatching_amd import eval as E
    p = E.get_parser()
    a = p.parse_args(["--builtin", "icdar15", "--input", "in", "--output", "out", "--opts", "MODEL.WEIGHTS", "w.pth",
                      "INPUT.MIN_SIZE_TEST", "128"])
    assert a.opts == ["MODEL.WEIGHTS", "w.pth", "INPUT.MIN_SIZE_TEST", "128"] and a.builtin == "icdar15"
    assert a.frames_per_step == 8 and not a.host_ingest and not a.host_rows and a.config_file is None
    a = p.parse_args(["--config-file", "f.yaml", "--input", "i", "--output", "o", "--host-rows", "--host-ingest",
                      "--frames-per-step", "4"])
    assert a.opts == [] and a.host_rows and a.host_ingest and a.frames_per_step == 4 and a.config_file == "f.yaml"
    text = "".join(p.format_help().split())
    assert "--cpu" in text and "--webcam" in text and "--show" in text      # named as absent
    for flag in ("--cpu", "--webcam", "--show"):
        with pytest.raises(SystemExit):
            p.parse_args(["--builtin", "icdar15", "--input", "i", "--output", "o", flag])


def test_missing_weights_exit_status_2(tmp_path):
    (tmp_path / "in").mkdir()
    base = [sys.executable, "-m", "gomatching_amd.eval", "--builtin", "icdar15", "--input", str(tmp_path / "in"),
            "--output", str(tmp_path / "out")]
    for extra in ([], ["--opts", "MODEL.WEIGHTS", str(tmp_path / "absent.pth")], ["--opts", "MODEL.WEIGHTS", ""]):
        r = subprocess.run(base + extra, cwd=ROOT, capture_output=True, text=True, timeout=300)
        assert r.returncode == 2, (r.returncode, r.stderr[-500:])
        assert "MODEL.WEIGHTS" in r.stderr and "Traceback" not in r.stderr
        assert not (tmp_path / "out").exists()                          # nothing was written, nothing touched the GPU
