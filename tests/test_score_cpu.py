"""Scoring on the CPU: the float64 statement of the pair geometry on hand cases, `score.host_quad_pairs` against it, the
accumulator and metrics against what the reference's motmetrics gave (tests/golden/score_mot.json, written by
tools/gen_golden_score.py), the readers, the command line with --host-iou, the error exits and the entry points' argument
checks."""
import ctypes
import json
import math
import os

import numpy as np
import pytest

import score_statement as S

UNIT = (0, 0, 1, 0, 1, 1, 0, 1)


# ------------------------------------------------------------------------------------------ the statement, by hand
def test_statement_identical_and_disjoint_quads():
    q = (3, 4, 40, 6, 38, 30, 5, 28)
    assert S.pair_value(q, q, 0) == 1.0 and S.pair_value(q, q, 1) == 1.0
    far = tuple(v + 100 for v in q)
    assert S.pair_value(q, far, 0) == 0.0 and S.pair_value(q, far, 1) == 0.0
    touching = (1, 0, 2, 0, 2, 1, 1, 1)                          # shares an edge with the unit square: no area in common
    assert S.pair_value(UNIT, touching, 0) == 0.0


def test_statement_half_covered_rectangle():
    wide = (0, 0, 2, 0, 2, 1, 0, 1)
    assert S.pair_value(wide, UNIT, 0) == 0.5 and S.pair_value(UNIT, wide, 0) == 0.5
    assert S.pair_value(wide, UNIT, 1) == 1.0                    # the detection (unit square) lies inside the ground truth
    assert S.pair_value(UNIT, wide, 1) == 0.5


def test_statement_takes_the_hull_of_a_bow_tie():
    bow = (0, 0, 4, 4, 4, 0, 0, 4)                               # hull: the square 0..4
    other = (2, 2, 6, 2, 6, 6, 2, 6)
    assert S.hull(bow) == [(0, 0), (4, 0), (4, 4), (0, 4)]
    assert abs(S.pair_value(bow, other, 0) - 1 / 7) < 1e-15 and abs(S.pair_value(other, bow, 0) - 1 / 7) < 1e-15
    for order in ((0, 0, 4, 0, 4, 4, 0, 4), (0, 4, 4, 4, 4, 0, 0, 0), (4, 4, 0, 0, 0, 4, 4, 0)):
        assert S.pair_value(order, other, 0) == S.pair_value(bow, other, 0)


def test_statement_degenerate_quads_have_no_area():
    line = (0, 0, 1, 1, 2, 2, 3, 3)
    assert S.pair_value(line, UNIT, 0) == 0.0 and S.pair_value(UNIT, line, 0) == 0.0
    assert S.pair_value(UNIT, line, 1) == 0.0 and S.pair_value(line, line, 0) == 0.0
    point = (5, 5, 5, 5, 5, 5, 5, 5)
    assert S.pair_value(point, point, 0) == 0.0
    triangle = (0, 0, 4, 0, 4, 0, 0, 4)                          # a repeated point: the triangle remains
    assert S.hull(triangle) == [(0, 0), (4, 0), (0, 4)]
    assert S.pair_value(triangle, triangle, 0) == 1.0
    inner = (0, 0, 4, 0, 1, 1, 0, 4)                             # a point inside the triangle of the other three
    assert S.hull(inner) == [(0, 0), (4, 0), (0, 4)]


# ------------------------------------------------------------------------------------------ the host path = the statement
def _edge_quads():
    rng = np.random.RandomState(3)
    quads = [UNIT, (0, 0, 2, 0, 2, 1, 0, 1), (0, 0, 4, 4, 4, 0, 0, 4), (2, 2, 6, 2, 6, 6, 2, 6), (0, 0, 1, 1, 2, 2, 3, 3),
             (5, 5, 5, 5, 5, 5, 5, 5), (0, 0, 4, 0, 4, 0, 0, 4), (0, 0, 4, 0, 1, 1, 0, 4), (0, 0, 4, 0, 2, 0, 0, 4),
             (1, 0, 2, 0, 2, 1, 1, 1), (0, 0, 8191, 0, 8191, 8191, 0, 8191), (3, 0, 6, 3, 3, 6, 0, 3)]
    quads += [tuple(rng.randint(0, 12, size=8)) for _ in range(28)]         # small coordinates: many ties and collinear points
    return np.asarray(quads, dtype=np.int32)


@pytest.mark.parametrize("measure", [0, 1])
def test_host_path_equals_the_statement_on_edge_cases(measure):
    from gomatching_amd import score
    q = _edge_quads()
    n = len(q)
    off = np.asarray([0, n], dtype=np.int32)
    key = np.zeros(n, dtype=np.int32)
    counts, det, val = score.host_quad_pairs(q, q, off, off, key, key, measure, 1e-9)
    want_counts, kept, _ = S.pairs_statement(q, q, off, off, key, key, measure, 1e-9)
    assert counts.tolist() == want_counts.tolist()
    assert det.tolist() == [j for _, j, _ in kept]
    np.testing.assert_allclose(val, [v for _, _, v in kept], rtol=0, atol=1e-12)


def test_host_path_equals_the_statement_on_the_fixture():
    from gomatching_amd import score
    v = S.fixture_video()
    rng = np.random.RandomState(5)
    gk = rng.randint(0, 3, size=len(v["gt_quads"])).astype(np.int32)
    dk = rng.randint(0, 4, size=len(v["det_quads"])).astype(np.int32)   # key 3 exists on the detection side only
    for measure, keys in ((0, (gk * 0, dk * 0)), (1, (gk * 0, dk * 0)), (0, (gk, dk))):
        counts, det, val = score.host_quad_pairs(v["gt_quads"], v["det_quads"], v["gt_off"], v["det_off"], *keys, measure, 0.5)
        want_counts, kept, _ = S.pairs_statement(v["gt_quads"], v["det_quads"], v["gt_off"], v["det_off"], *keys, measure, 0.5)
        assert counts.tolist() == want_counts.tolist() and det.tolist() == [j for _, j, _ in kept]
        np.testing.assert_allclose(val, [x for _, _, x in kept], rtol=0, atol=1e-12)
        assert len(kept) > 10


# ------------------------------------------------------------------------------------------ accumulator and metrics
def _golden(golden_dir):
    with open(os.path.join(golden_dir, "score_mot.json")) as f:
        return json.load(f)


def test_golden_sequences_cover_the_required_situations(golden_dir):
    seqs = {s["name"]: s for s in _golden(golden_dir)["sequences"]}
    assert any(s["expected"]["num_switches"] > 0 for s in seqs.values())
    assert any(not fr["oids"] and fr["hids"] for s in seqs.values() for fr in s["frames"])       # a frame with no ground truth
    assert any(fr["oids"] and not fr["hids"] for s in seqs.values() for fr in s["frames"])       # a frame with no hypotheses
    assert any(all(not fr["hids"] for fr in s["frames"]) for s in seqs.values())                 # a video with none at all
    assert any(len(fr["hids"]) > len(fr["oids"]) > 0 for s in seqs.values() for fr in s["frames"])
    lost = seqs["lost_and_refound"]["frames"]                    # object 1: matched, then unmatched for frames, then matched
    assert lost[0]["pairs"] and not lost[2]["pairs"] and lost[5]["pairs"]


def test_accumulator_and_metrics_equal_the_reference(golden_dir):
    from gomatching_amd import score
    doc = _golden(golden_dir)
    for seq in doc["sequences"]:
        acc = score.MOTAccumulator()
        for fr in seq["frames"]:
            acc.update(fr["oids"], fr["hids"], [tuple(p) for p in fr["pairs"]], fr["frameid"])
        got = acc.metrics()
        for name in doc["metrics"]:
            want = seq["expected"][name]
            if isinstance(want, int):
                assert isinstance(got[name], int) and got[name] == want, (seq["name"], name, got[name], want)
            elif math.isnan(want):
                assert math.isnan(got[name]), (seq["name"], name, got[name])
            else:
                assert abs(got[name] - want) <= 1e-12, (seq["name"], name, got[name], want)


def test_max_switch_time_turns_a_late_switch_into_a_match():
    from gomatching_amd import score
    frames = [(1, [1], [10], [(0, 0, 0.1)]), (2, [1], [], []), (9, [1], [11], [(0, 0, 0.1)])]
    for limit, switches in ((float("inf"), 1), (7, 1), (6, 0)):
        acc = score.MOTAccumulator(max_switch_time=limit)
        for f in frames:
            acc.update(f[1], f[2], f[3], f[0])
        assert acc.metrics()["num_switches"] == switches


# ------------------------------------------------------------------------------------------ readers
def test_readers_on_the_writers_files_directory_and_zip(tmp_path):
    from gomatching_amd import score
    gt_dir, res_dir = S.write_tree(str(tmp_path / "d"))
    gt_zip, res_zip = S.write_tree(str(tmp_path / "z"), zipped=True)
    for gt, res in ((gt_dir, res_dir), (gt_zip, res_zip)):
        assert sorted(score.load_source(gt, score.GT_XML)) == ["1_1_1", "2_1_1"]
        assert sorted(score.load_source(gt, score.GT_TXT)) == ["1_1_1", "2_1_1"]
        xml = score.load_source(res, score.DET_XML)
        txt = score.load_source(res, score.DET_TXT)
        assert sorted(xml) == ["1_1_1"] and sorted(txt) == ["1_1_1"]
        frames = score.read_frames(xml["1_1_1"], "res")
        assert [fid for fid, _ in frames] == ["1", "2", "3", "4"]
        assert frames[1][1][0] == ("10", "hello", [15, 10, 55, 10, 55, 30, 15, 30])
        assert [oid for oid, _, _ in frames[1][1]] == ["10", "12", "13", "14"]
        assert score.read_transcriptions(txt["1_1_1"], "txt") == {"10": "hello", "11": "hello", "12": "x", "13": "abc", "14": "stray"}
        gtf = score.read_frames(score.load_source(gt, score.GT_XML)["1_1_1"], "gt")
        assert gtf[3][1][3] == ("4", "zz", [300, 300, 320, 300, 320, 320, 300, 320])
    assert score.load_source(gt_dir, score.GT_XML) == score.load_source(gt_zip, score.GT_XML)


def test_readers_reject_what_the_protocol_rejects():
    from gomatching_amd import score
    dup = b'<Frames><frame ID="1"><object ID="3" Transcription="a">' + b'<Point x="1" y="1"/>' * 4 + b"</object>" \
          b'<object ID="3" Transcription="b">' + b'<Point x="1" y="1"/>' * 4 + b"</object></frame></Frames>"
    with pytest.raises(score.ScoreError, match="[Dd]uplicated object ID"):
        score.read_frames(dup, "x")
    with pytest.raises(score.ScoreError, match="four points"):
        score.read_frames(b'<Frames><frame ID="1"><object ID="3"><Point x="1" y="1"/></object></frame></Frames>', "x")
    with pytest.raises(score.ScoreError):
        score.read_frames(b"<Frames><frame ID=", "x")
    with pytest.raises(score.ScoreError):
        score.read_transcriptions(b'"1","a"\n2,b\n', "x")
    neg = b'<Frames><frame ID="1"><object ID="3" Transcription="a"><Point x="-4" y="2"/>' + b'<Point x="1" y="-1"/>' * 3 + \
          b"</object></frame></Frames>"
    assert score.read_frames(neg, "x")[0][1][0][2] == [0, 2, 1, 0, 1, 0, 1, 0]          # max(0, .)
    assert score.read_transcriptions(b'\xef\xbb\xbf"1","a,"b""\r\n\r\n"2",""\n', "x") == {"1": 'a,"b"', "2": ""}


# ------------------------------------------------------------------------------------------ the command line
def _check(sample, expected):
    for k, want in expected.items():
        if isinstance(want, int):
            assert sample[k] == want, (k, sample[k], want)
        else:
            assert abs(sample[k] - want) <= 1e-12, (k, sample[k], want)


@pytest.mark.parametrize("zipped", [False, True])
def test_command_line_tracking_with_host_iou(tmp_path, capsys, zipped):
    from gomatching_amd import score
    gt, res = S.write_tree(str(tmp_path / "t"), zipped=zipped)
    out = str(tmp_path / "scores.json")
    assert score.main(["--gt", gt, "--results", res, "--host-iou", "--output", out]) == 0
    doc = json.load(open(out))
    assert sorted(doc["per_sample"]) == ["1_1_1", "2_1_1"]
    for k, exp in S.TRACKING_EXPECTED.items():
        _check(doc["per_sample"][k], exp)
    assert doc["per_sample"]["1_1_1"]["DC_GT"] == 4 and doc["per_sample"]["1_1_1"]["DC_DT"] == 4
    e = S.TRACKING_EXPECTED["1_1_1"]
    _check(doc["method"], {"MOTA": e["MOTA"] / 2, "MOTP": e["MOTP"] / 2, "IDF1": e["IDF1"] / 2, "MOTAN": e["MOTAN"] / 2,
                           "MT": 1, "PT": 1, "ML": 1})
    printed = capsys.readouterr().out.splitlines()
    assert printed[0].startswith("method: MOTA") and len(printed) == 3 and printed[1].startswith("Video_1_1_1:")


def test_command_line_end_to_end_with_host_iou(tmp_path):
    from gomatching_amd import score
    gt, res = S.write_tree(str(tmp_path / "a"))
    out = str(tmp_path / "a.json")
    assert score.main(["--gt", gt, "--results", res, "--e2e", "--host-iou", "--output", out]) == 0
    doc = json.load(open(out))
    for k, exp in S.TRACKING_EXPECTED.items():                   # every transcription agrees: the tracking figures
        _check(doc["per_sample"][k], exp)
    gt, res = S.write_tree(str(tmp_path / "b"), wrong_text=True)
    out = str(tmp_path / "b.json")
    assert score.main(["--gt", gt, "--results", res, "--e2e", "--host-iou", "--output", out]) == 0
    _check(json.load(open(out))["per_sample"]["1_1_1"], S.E2E_WRONG_TEXT_EXPECTED)
    # a detection without a transcription line is skipped: without track 13's line, object 3 is missed as with a wrong text
    # (its detections no longer count as false positives)
    txt = os.path.join(res, "res_Video_1_1_1.txt")
    lines = [l for l in open(txt).read().splitlines(True) if not l.startswith('"13"')]
    open(txt, "w").writelines(lines)
    assert score.main(["--gt", gt, "--results", res, "--e2e", "--host-iou", "--output", out]) == 0
    s = json.load(open(out))["per_sample"]["1_1_1"]
    assert (s["MA"], s["SW"], s["MS"], s["FP"], s["PR"]) == (3, 1, 5, 1, 5)
    # a ground-truth object without a transcription line is "don't care": object 3 leaves, and track 13 with it
    gt2, res2 = S.write_tree(str(tmp_path / "c"))
    gtxt = os.path.join(gt2, "Video_1_1_1_GT.txt")
    kept_lines = [l for l in open(gtxt).read().splitlines(True) if not l.startswith('"3"')]
    open(gtxt, "w").writelines(kept_lines)
    assert score.main(["--gt", gt2, "--results", res2, "--e2e", "--host-iou", "--output", out]) == 0
    s = json.load(open(out))["per_sample"]["1_1_1"]
    assert (s["MA"], s["SW"], s["MS"], s["FP"], s["OB"], s["DC_GT"]) == (3, 1, 1, 1, 5, 8)


def test_command_line_error_exits(tmp_path, capsys):
    from gomatching_amd import score
    gt, res = S.write_tree(str(tmp_path / "t"))
    out = str(tmp_path / "s.json")

    def fails(argv, word):
        assert score.main(argv) == 2
        err = capsys.readouterr().err
        assert err.startswith("error: ") and word in err, err
        assert not os.path.exists(out)
    fails(["--gt", str(tmp_path / "missing"), "--results", res, "--host-iou", "--output", out], "not found")
    fails(["--gt", gt, "--results", str(tmp_path / "missing.zip"), "--host-iou", "--output", out], "not found")
    fails(["--gt", gt, "--results", res, "--host-iou", "--threshold", "1.5", "--output", out], "--threshold")
    empty = tmp_path / "empty"
    empty.mkdir()
    fails(["--gt", str(empty), "--results", res, "--host-iou", "--output", out], "GT.xml")
    notzip = tmp_path / "not.zip"
    notzip.write_bytes(b"plain text")
    fails(["--gt", gt, "--results", str(notzip), "--host-iou", "--output", out], "ZIP")
    extra = os.path.join(res, "res_Video_9_9_9.xml")             # a result for a video the ground truth does not have
    open(extra, "w").write(open(os.path.join(res, "res_Video_1_1_1.xml")).read())
    fails(["--gt", gt, "--results", res, "--host-iou", "--output", out], "not present in GT")
    os.remove(extra)
    os.remove(os.path.join(res, "res_Video_1_1_1.txt"))
    fails(["--gt", gt, "--results", res, "--e2e", "--host-iou", "--output", out], "text file")
    with pytest.raises(SystemExit) as e:                         # argparse's own exit for a missing required option
        score.main(["--gt", gt])
    assert e.value.code == 2


# ------------------------------------------------------------------------------------------ the entry points' checks
def test_score_entry_points_reject_bad_arguments_without_a_gpu():
    """Argument checks run before any HIP call (the pattern of test_entry_points_reject_bad_arguments_without_a_gpu)."""
    from gomatching_amd import lib
    L = lib.load()
    INVALID, OK = 1, 0
    p = ctypes.c_void_p(0x1000)                                   # non-null, aligned, never dereferenced

    def count(gq=p, dq=p, go=p, do=p, gk=p, dk=p, G=4, D=6, F=2, pairs=12, measure=0, thr=0.5, counts=p):
        return L.gom_quad_pairs_count_f64(gq, dq, go, do, gk, dk, G, D, F, pairs, measure, thr, counts, None)

    def emit(gq=p, dq=p, go=p, do=p, gk=p, dk=p, G=4, D=6, F=2, pairs=12, measure=0, thr=0.5, scan=p, total=3, od=p, ov=p):
        return L.gom_quad_pairs_emit_f64(gq, dq, go, do, gk, dk, G, D, F, pairs, measure, thr, scan, total, od, ov, None)
    for fn, none_kept in ((count, {}), (emit, {"total": 0})):
        for name in ("gq", "dq", "go", "do", "gk", "dk"):
            assert fn(**{name: None}) == INVALID, name
        assert fn(G=-1) == INVALID and fn(D=-1) == INVALID and fn(F=-1) == INVALID
        assert fn(F=0) == INVALID                                 # objects without a frame
        assert fn(measure=2) == INVALID and fn(measure=-1) == INVALID
        for thr in (0.0, 1.0, -0.5, 1.5, float("nan")):
            assert fn(thr=thr) == INVALID, thr
        assert fn(pairs=-1) == INVALID and fn(pairs=25) == INVALID              # more than G * D
        assert fn(G=70000, D=70000, pairs=2 ** 31) == INVALID                   # does not fit int32
        assert fn(G=0, D=0, F=0, pairs=0, **none_kept) == OK                    # nothing to do, nothing launched
        assert fn(G=0, D=6, F=2, pairs=0, **none_kept) == OK
    assert count(counts=None) == INVALID
    assert emit(scan=None) == INVALID and emit(od=None) == INVALID and emit(ov=None) == INVALID
    assert emit(total=-1) == INVALID and emit(total=13) == INVALID              # more than pairs
    assert emit(total=0, scan=None, od=None, ov=None) == OK                     # nothing kept: no launch
