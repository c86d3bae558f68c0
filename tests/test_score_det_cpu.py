"""The detection protocol of scoring on the CPU (no GPU needed): the host path (`score_det.py`, numpy float64) against the
reference's own figures (tests/golden/score_det.json, written by tools/gen_golden_score_det.py) and against the plain
statement of the rule (det_statement.py); the command line's refusals; the C entry's argument checks."""
import ctypes
import json
import os
import shutil

import numpy as np
import pytest

import det_statement as DS
import score_statement as S


@pytest.fixture(scope="module")
def golden_dir():
    return os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _raw(golden_dir):
    return os.path.join(golden_dir, "score_det_raw", "gt"), os.path.join(golden_dir, "score_det_raw", "res")


# ------------------------------------------------------------------------------------------ against the reference's figures
def test_fixture_covers_the_required_situations(golden_dir):
    """Conditions on the recorded file alone: the situations the fixture was written for did occur in the reference's run."""
    doc = json.load(open(os.path.join(golden_dir, "score_det.json")))
    ps = doc["per_sample"]
    assert doc["frames"] == {"Video_1_1_1": 4, "Video_2_1_1": 2} and len(ps) == 6
    f = ps["res_Video_1_1_1_1.txt"]          # two objects pass detection 0, the first takes it; detection 1 passes a care
    assert f["pairs"] == [{"gt": 0, "det": 0}] and f["gtDontCare"] == [2] and f["detDontCare"] == [1]   # object but is covered
    assert ps["res_Video_1_1_1_2.txt"]["recall"] == 1.0 and ps["res_Video_1_1_1_2.txt"]["precision"] == 0.0   # no ground truth
    assert ps["res_Video_1_1_1_3.txt"]["pairs"] == [] and ps["res_Video_1_1_1_3.txt"]["recall"] == 0.0         # no detections
    assert doc["dropped"]["gt"]["Video_1_1_1"] == [[2, 1]] and doc["dropped"]["det"]["Video_2_1_1"] == [[1, 0]]
    f = ps["res_Video_2_1_1_1.txt"]          # IoU exactly 0.5: no pair for object 0; overlap exactly 0.5: detection 1 stays
    assert f["pairs"] == [{"gt": 3, "det": 3}] and f["detDontCare"] == [] and f["gtDontCare"] == [1]
    assert ps["res_Video_2_1_1_2.txt"]["pairs"][0] == {"gt": 0, "det": 0}                                     # the two diamonds


def test_host_path_equals_the_reference(golden_dir, tmp_path):
    from gomatching_amd import score, score_det
    doc = json.load(open(os.path.join(golden_dir, "score_det.json")))
    gt, res = _raw(golden_dir)
    out = str(tmp_path / "scores.json")
    assert score.main(["--det", "--gt", gt, "--results", res, "--host-iou", "--per-frame", "--output", out]) == 0
    got = json.load(open(out))
    assert sorted(got["per_sample"]) == sorted(doc["per_sample"])
    for name, want in doc["per_sample"].items():
        have = got["per_sample"][name]
        assert sorted(have) == ["detDontCare", "gtDontCare", "hmean", "pairs", "precision", "recall"]
        for k in ("pairs", "gtDontCare", "detDontCare"):
            assert have[k] == want[k], (name, k, have[k], want[k])
        for k in ("precision", "recall", "hmean"):
            assert abs(have[k] - want[k]) <= 1e-12, (name, k, have[k], want[k])
    for k in ("precision", "recall", "hmean"):
        assert abs(got["method"][k] - doc["method"][k]) <= 1e-12, (k, got["method"][k], doc["method"][k])
    assert got["method"]["AP"] == 0 and doc["method"]["AP"] == 0
    assert (got["method"]["matched"], got["method"]["gt_care"], got["method"]["det_care"]) == (4, 10, 11)
    assert got["method"]["nonconvex_gt"] == 0 and got["method"]["nonconvex_det"] == 0
    assert sorted(got["per_video"]) == ["1_1_1", "2_1_1"]
    # the drop lists, by (frame position, object position)
    for v in doc["videos"]:
        key = v[len("Video_"):]
        raw_gt = open(os.path.join(gt, v + "_GT.xml"), "rb").read()
        raw_res = open(os.path.join(res, "res_%s.xml" % v), "rb").read()
        assert [list(x) for x in score_det.read_quads(raw_gt, v, True)[1]] == doc["dropped"]["gt"][v]
        assert [list(x) for x in score_det.read_quads(raw_res, v, False)[1]] == doc["dropped"]["det"][v]
        assert got["per_video"][key]["invalid_gt"] == len(doc["dropped"]["gt"][v])
        assert got["per_video"][key]["invalid_det"] == len(doc["dropped"]["det"][v])
    # without --per-frame: the same figures, no per_sample
    assert score.main(["--det", "--gt", gt, "--results", res, "--host-iou", "--output", out]) == 0
    lean = json.load(open(out))
    assert sorted(lean) == ["method", "per_video"] and lean["method"] == got["method"] and lean["per_video"] == got["per_video"]


def test_printed_lines(golden_dir, tmp_path, capsys):
    from gomatching_amd import score
    gt, res = _raw(golden_dir)
    assert score.main(["--det", "--gt", gt, "--results", res, "--host-iou", "--output", str(tmp_path / "s.json")]) == 0
    lines = capsys.readouterr().out.splitlines()
    assert len(lines) == 3 and lines[0].startswith("method: precision 0.3636  recall 0.4000  hmean 0.3810  matched 4  care GT 10")
    assert lines[1].startswith("Video_1_1_1: ") and lines[2].startswith("Video_2_1_1: ")


def test_a_video_without_results_and_nonconvex_counts(golden_dir, tmp_path):
    from gomatching_amd import score
    gt, res = _raw(golden_dir)
    res2 = tmp_path / "res"
    res2.mkdir()
    shutil.copy(os.path.join(res, "res_Video_1_1_1.xml"), str(res2))
    out = str(tmp_path / "s.json")
    assert score.main(["--det", "--gt", gt, "--results", str(res2), "--host-iou", "--output", out]) == 0
    doc = json.load(open(out))
    v = doc["per_video"]["2_1_1"]
    assert (v["matched"], v["gt_care"], v["det_care"], v["precision"], v["recall"]) == (0, 5, 0, 0.0, 0.0)
    assert doc["method"]["gt_care"] == 10 and doc["method"]["det_care"] == 3
    # an ordered quad that is not convex (an arrow head) is counted, and scored through its hull
    gt3 = tmp_path / "gt"
    gt3.mkdir()
    (gt3 / "Video_7_1_1_GT.xml").write_text(S._gt_xml([(1, [(1, "dart", [0, 0, 40, 20, 0, 40, 10, 20])])]))
    (tmp_path / "empty").mkdir()
    assert score.main(["--det", "--gt", str(gt3), "--results", str(tmp_path / "empty"), "--host-iou", "--output", out]) == 0
    assert json.load(open(out))["method"]["nonconvex_gt"] == 1


# ------------------------------------------------------------------------------------------ against the statement
def test_host_path_equals_the_statement_on_random_frames():
    """320 seeded frames (rotated rectangles, near-duplicate objects and detections, don't-care regions with detections inside
    them, strays): every frame's det_care, match and counts must be the statement's.  First a condition on the inputs alone:
    no pair the rule looks at lies within 1e-6 of its threshold, so that the two float64 evaluations (the statement's true
    hulls, the host path's four-slot hulls) cannot differ in a decision."""
    from gomatching_amd import score_det
    v = DS.random_video(20241019, 320)
    want_care, want_match, want_stats, closest = DS.video_statement(v["gt_quads"], v["det_quads"], v["gt_off"], v["det_off"],
                                                                    v["gt_care"])
    print("%d frames, %d objects (%d don't care), %d detections; closest to a threshold %.3g; matched %d, dropped detections %d"
          % (len(v["gt_off"]) - 1, len(v["gt_quads"]), int((v["gt_care"] == 0).sum()), len(v["det_quads"]), closest,
             int(want_stats[:, 0].sum()), int((want_care == 0).sum())))
    assert closest > 1e-6
    assert int((v["gt_care"] == 0).sum()) >= 100 and int((want_care == 0).sum()) >= 100 and int(want_stats[:, 0].sum()) >= 300
    # objects that lost their first passing detection to an earlier object, and took another one or none: the greedy part
    det_care, match, stats = score_det.host_quad_det_match(v["gt_quads"], v["det_quads"], v["gt_off"], v["det_off"], v["gt_care"])
    assert det_care.dtype == np.int32 and match.dtype == np.int32 and stats.dtype == np.int32
    for f in range(len(v["gt_off"]) - 1):
        g0, g1, d0, d1 = v["gt_off"][f], v["gt_off"][f + 1], v["det_off"][f], v["det_off"][f + 1]
        assert det_care[d0:d1].tolist() == want_care[d0:d1].tolist(), f
        assert match[g0:g1].tolist() == want_match[g0:g1].tolist(), f
        assert stats[f].tolist() == want_stats[f].tolist(), f


def test_host_path_equals_the_statement_on_the_edge_video():
    """The GPU tests' video (det_statement.edge_video), which holds pairs at exactly 0.5: integer rectangles, exact in both."""
    from gomatching_amd import score_det
    v, notes = DS.edge_video()
    want = DS.video_statement(v["gt_quads"], v["det_quads"], v["gt_off"], v["det_off"], v["gt_care"])
    got = score_det.host_quad_det_match(v["gt_quads"], v["det_quads"], v["gt_off"], v["det_off"], v["gt_care"])
    for a, b in zip(got, want[:3]):
        assert a.tolist() == b.tolist()
    go, do = v["gt_off"], v["det_off"]
    m = lambda f: got[1][go[f]:go[f + 1]].tolist()
    assert got[2][0].tolist() == [0, 0, 0] and got[2][1].tolist() == [0, 0, 2] and got[2][2].tolist() == [0, 1, 0]
    assert m(3) == [0] and m(4) == [64] and m(5) == [3, 64]
    assert len(m(6)) == 130 and max(m(6)) >= 64
    assert m(7) == [2, -1] and got[0][do[7]:do[8]].tolist() == [0, 0, 1]
    assert m(8) == [-1, -1, 2] and got[0][do[8]:do[9]].tolist() == [1, 1, 1]      # exactly 0.5 counts on neither side
    assert m(9) == [-1, 2, -1, -1]


def test_order_points_and_validity():
    from gomatching_amd import score_det
    rect = [(10, 10), (50, 10), (50, 30), (10, 30)]
    assert score_det.order_points(rect) == [(10, 30), (10, 10), (50, 10), (50, 30)]
    assert score_det.clockwise_valid(score_det.order_points(rect))
    # a tie in x: the two middle points keep their file order, which decides who is "left"
    assert score_det.order_points([(0, 100), (50, 0), (50, 200), (100, 100)]) == [(0, 100), (50, 0), (100, 100), (50, 200)]
    assert score_det.order_points([(50, 200), (0, 100), (100, 100), (50, 0)]) == [(50, 200), (0, 100), (50, 0), (100, 100)]
    bad = score_det.order_points([(0, 0), (3, 1), (13, 50), (10, 49)])
    assert bad == [(3, 1), (0, 0), (10, 49), (13, 50)] and not score_det.clockwise_valid(bad)


def test_the_kernel_path_refuses_a_frame_past_its_limit():
    """The per-frame limit of the matching kernel is checked on the host before anything is launched, naming video and frame
    (no GPU needed: the refusal comes before the matching function is called)."""
    from gomatching_amd import score_det
    from gomatching_amd.score import ScoreError
    obj = '<object ID="1" Transcription="a"><Point x="0" y="0"/><Point x="9" y="0"/><Point x="9" y="9"/><Point x="0" y="9"/></object>'
    gt = ("<Frames><frame ID=\"1\">%s</frame><frame ID=\"2\">%s</frame></Frames>" % (obj, obj)).encode()
    res = ("<Frames><frame ID=\"1\">%s</frame><frame ID=\"2\">%s</frame></Frames>" % (obj, obj * 4097)).encode()

    def never(*args):
        raise AssertionError("the matching function was called")
    with pytest.raises(ScoreError) as e:
        score_det.score_video(gt, res, match_fn=never, name="Video_5_1_1")
    assert "Video_5_1_1" in str(e.value) and "frame 2" in str(e.value) and "4097" in str(e.value)
    assert score_det.MAX_FRAME_DETECTIONS == 4096 >= 1024
    sums, _ = score_det.score_video(gt, res)                      # the numpy path has no such limit
    assert (sums["matched"], sums["gt_care"], sums["det_care"]) == (2, 2, 4098)


# ------------------------------------------------------------------------------------------ the command line's refusals
def test_command_line_refusals(golden_dir, tmp_path, capsys):
    from gomatching_amd import score
    gt, res = _raw(golden_dir)
    out = str(tmp_path / "s.json")

    def fails(argv, word):
        assert score.main(argv) == 2
        captured = capsys.readouterr()
        assert captured.err.startswith("error: ") and captured.err.count("\n") == 1 and word in captured.err, captured.err
        assert captured.out == "" and not os.path.exists(out)
    base = ["--det", "--gt", gt, "--results", res, "--host-iou", "--output", out]
    fails(base + ["--e2e"], "--e2e")
    fails(base + ["--protocol", "bovtext"], "bovtext")
    fails(base + ["--protocol", "artvideo", "--curve"], "--curve")
    fails(["--gt", gt, "--results", res, "--host-iou", "--output", out, "--per-frame"], "--per-frame")
    fails(base + ["--threshold", "1.0"], "--threshold")
    # a five-point object
    bad_gt = tmp_path / "gt5"
    shutil.copytree(gt, str(bad_gt))
    p = bad_gt / "Video_1_1_1_GT.xml"
    p.write_text(p.read_text().replace('<Point x="10" y="10"/>', '<Point x="10" y="10"/>\n      <Point x="11" y="10"/>', 1))
    fails(["--det", "--gt", str(bad_gt), "--results", res, "--host-iou", "--output", out], "not four")
    # a result with more frames than its ground truth
    bad_res = tmp_path / "res5"
    shutil.copytree(res, str(bad_res))
    p = bad_res / "res_Video_2_1_1.xml"
    p.write_text(p.read_text().replace("</Frames>", '  <frame ID="3">\n  </frame>\n</Frames>'))
    fails(["--det", "--gt", gt, "--results", str(bad_res), "--host-iou", "--output", out], "frames")
    # a coordinate of 2^24 or more after the shift
    big = tmp_path / "gtbig"
    shutil.copytree(gt, str(big))
    p = big / "Video_2_1_1_GT.xml"
    p.write_text(p.read_text().replace('<Point x="10" y="40"/>', '<Point x="16777186" y="40"/>', 1))
    assert 'x="16777186"' in p.read_text()
    fails(["--det", "--gt", str(big), "--results", res, "--host-iou", "--output", out], "2^24")


def test_without_det_the_command_writes_what_it_wrote(tmp_path, capsys):
    """The tracking protocol's scores.json for score_statement's tree, byte for byte: tests/golden/score_cli_tracking.json is
    the file the command wrote before the detection protocol existed."""
    from gomatching_amd import score
    gt, res = S.write_tree(str(tmp_path / "t"))
    out = str(tmp_path / "scores.json")
    assert score.main(["--gt", gt, "--results", res, "--host-iou", "--output", out]) == 0
    printed = capsys.readouterr().out
    text = open(out).read()
    assert text == open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "score_cli_tracking.json")).read()
    want = json.loads(text)
    assert sorted(want) == ["method", "per_sample"] and sorted(want["method"]) == ["IDF1", "ML", "MOTA", "MOTAN", "MOTP", "MT", "PT"]
    m = want["method"]
    assert printed.splitlines()[0] == "method: MOTA %.4f  MOTP %.4f  IDF1 %.4f  MOTAN %.4f  MT %d  PT %d  ML %d" % (
        m["MOTA"], m["MOTP"], m["IDF1"], m["MOTAN"], m["MT"], m["PT"], m["ML"])
    assert abs(m["MOTA"] - S.TRACKING_EXPECTED["1_1_1"]["MOTA"] / 2) <= 1e-12
    args = score.build_parser().parse_args(["--gt", gt, "--results", res])
    assert args.det is False and args.per_frame is False


# ------------------------------------------------------------------------------------------ the entry point's checks
def test_det_match_entry_rejects_bad_arguments_without_a_gpu():
    """Argument checks run before any HIP call (the pattern of test_score_entry_points_reject_bad_arguments_without_a_gpu)."""
    from gomatching_amd import lib
    L = lib.load()
    INVALID, OK = 1, 0
    p = ctypes.c_void_p(0x1000)                                   # non-null, aligned, never dereferenced

    def call(gq=p, dq=p, go=p, do=p, gc=p, G=4, D=6, F=2, iou=0.5, area=0.5, dc=p, m=p, st=p):
        return L.gom_quad_det_match_f64(gq, dq, go, do, gc, G, D, F, iou, area, dc, m, st, None)
    for name in ("gq", "dq", "go", "do", "gc", "dc", "m", "st"):
        assert call(**{name: None}) == INVALID, name
    assert call(G=-1) == INVALID and call(D=-1) == INVALID and call(F=-1) == INVALID
    assert call(F=0) == INVALID                                   # objects without a frame
    for thr in (0.0, 1.0, -0.5, 1.5, float("nan")):
        assert call(iou=thr) == INVALID and call(area=thr) == INVALID, thr
    assert call(G=0, D=0, F=0) == OK                              # nothing to do, nothing launched
    assert call(G=0, D=0, F=0, gq=None, dq=None, go=None, do=None, gc=None, dc=None, m=None, st=None) == OK
    assert "gom_quad_det_match_f64" in lib.SIGNATURES
