"""CPU: the json protocols of scoring (gomatching_amd/score_json.py) with the host path -- the OVERALL row against what the
reference's motmetrics gave (tests/golden/score_overall.json, written by tools/gen_golden_score_overall.py), the four protocol
variants and --curve on hand-made videos whose figures follow from the protocols' rules, the unchanged default protocol, the
error exits, the new entry points' argument checks and `host_mask_pairs` against the statement."""
import ctypes
import json
import math
import os

import numpy as np
import pytest

import mask_statement as ms
import score_json_cases as cases
import score_statement as S


def _same(got, want, what):
    if isinstance(want, int) and not isinstance(want, bool):
        assert got == want, (what, got, want)
    elif math.isnan(want):
        assert math.isnan(got), (what, got)
    else:
        assert abs(got - want) <= 1e-12, (what, got, want)


def test_overall_row_equals_the_reference(golden_dir):
    from gomatching_amd import score, score_json
    doc = json.load(open(os.path.join(golden_dir, "score_overall.json")))
    seqs = {s["name"]: s["frames"] for s in json.load(open(os.path.join(golden_dir, "score_mot.json")))["sequences"]}
    assert len(doc["groups"]) >= 3 and any("no_hypotheses" in g["names"] and len(g["names"]) > 1 for g in doc["groups"])
    for group in doc["groups"]:
        partials = []
        for name, row in zip(group["names"], group["rows"]):
            acc = score.MOTAccumulator()
            for fr in seqs[name]:
                acc.update(fr["oids"], fr["hids"], fr["pairs"], fr["frameid"])
            m = score_json._video_metrics(acc)
            for k in doc["metrics"]:
                _same(m[k], row[k], (name, k))
            partials.append(m)
        got = score_json.overall(partials)
        for k in doc["metrics"]:
            _same(got[k], group["overall"][k], (group["names"], k))


def _run(tmp_path, protocol, e2e, curve, write, extra=()):
    from gomatching_amd import score
    gt, res = write(str(tmp_path / "tree"))
    out = str(tmp_path / "scores.json")
    argv = ["--protocol", protocol, "--gt", gt, "--results", res, "--host-iou", "--output", out] + list(extra)
    argv += (["--e2e"] if e2e else []) + (["--curve"] if curve else [])
    assert score.main(argv) == 0
    return json.load(open(out))


@pytest.mark.parametrize("protocol,e2e,curve", sorted(cases.EXPECTED))
def test_protocol_variants_on_hand_made_videos(tmp_path, capsys, protocol, e2e, curve):
    write = cases.write_bovtext if protocol == "bovtext" else cases.write_artvideo
    doc = _run(tmp_path, protocol, e2e, curve, write)
    first, second = ("Cls2_Cartoon_video1", "Cls3_Sports_video2") if protocol == "bovtext" else ("video_1", "video_2")
    assert sorted(doc["per_sample"]) == [first, second]           # (video40 and the checkpoints directory are left out)
    want = cases.EXPECTED[(protocol, e2e, curve)]
    for k, v in want.items():
        _same(doc["per_sample"][first][k], v, k)
    for k, v in cases.NO_RESULT.items():                          # the video without a result file: every object missed
        _same(doc["per_sample"][second][k], v, k)
    o = doc["overall"]
    for k in ("num_frames", "num_matches", "num_false_positives", "num_misses", "num_objects"):
        assert o[k] == want[k] + cases.NO_RESULT[k], k
    _same(o["mota"], 1 - (o["num_false_positives"] + o["num_misses"]) / o["num_objects"], "mota")
    _same(o["motp"], want["motp"], "motp")                        # weighted by the detections: the second video has none
    printed = capsys.readouterr().out.splitlines()
    assert len(printed) == 3 and printed[0].startswith("OVERALL: MOTA %.4f  MOTP %.4f  IDF1" % (o["mota"], o["motp"]))
    assert "SW 0  FP %d  MS %d" % (o["num_false_positives"], o["num_misses"]) in printed[0]


def test_threshold_is_inclusive_for_pairs_and_exclusive_for_ignored(tmp_path):
    """At --threshold 0.5 hypothesis 10 (IoU exactly 0.5 with A) pairs and 12 (exactly 0.5 with the ignored C) stays; the
    next double above 0.5 turns the pair away, and ArTVideo's ignore test, which uses the same threshold, with it."""
    up = repr(float(np.nextafter(0.5, 1.0)))
    doc = _run(tmp_path / "a", "artvideo", True, False, cases.write_artvideo, ["--threshold", up])
    s = doc["per_sample"]["video_1"]
    assert (s["num_matches"], s["num_false_positives"], s["num_misses"]) == (1, 3, 4)
    doc = _run(tmp_path / "b", "bovtext", False, False, cases.write_bovtext, ["--threshold", up])
    s = doc["per_sample"]["Cls2_Cartoon_video1"]                  # (BOVText's ignore threshold stays 0.5)
    assert (s["num_matches"], s["num_false_positives"], s["num_misses"]) == (2, 2, 3)


def test_zipped_sources_give_the_same_file(tmp_path):
    import zipfile
    from gomatching_amd import score
    gt, res = cases.write_artvideo(str(tmp_path / "t"))
    out1, out2 = str(tmp_path / "a.json"), str(tmp_path / "b.json")
    assert score.main(["--protocol", "artvideo", "--gt", gt, "--results", res, "--host-iou", "--e2e", "--output", out1]) == 0
    for d in (gt, res):
        with zipfile.ZipFile(d + ".zip", "w") as z:
            for name in os.listdir(d):
                z.write(os.path.join(d, name), name)
    assert score.main(["--protocol", "artvideo", "--gt", gt + ".zip", "--results", res + ".zip", "--host-iou", "--e2e",
                       "--output", out2]) == 0
    assert open(out1, "rb").read() == open(out2, "rb").read()


def test_default_protocol_is_unchanged(tmp_path, capsys):
    from gomatching_amd import score
    gt, res = S.write_tree(str(tmp_path / "t"))
    out1, out2 = str(tmp_path / "a.json"), str(tmp_path / "b.json")
    assert score.main(["--gt", gt, "--results", res, "--host-iou", "--e2e", "--output", out1]) == 0
    first = capsys.readouterr().out
    assert score.main(["--protocol", "dstext", "--gt", gt, "--results", res, "--host-iou", "--e2e", "--output", out2]) == 0
    assert capsys.readouterr().out == first and first.startswith("method: MOTA")
    assert open(out1, "rb").read() == open(out2, "rb").read()
    assert sorted(json.load(open(out1))) == ["method", "per_sample"]


def test_reader_errors_exit_with_status_2(tmp_path, capsys):
    from gomatching_amd import score
    out = str(tmp_path / "s.json")

    def fails(argv, word):
        assert score.main(argv + ["--host-iou", "--output", out]) == 2
        err = capsys.readouterr().err
        assert err.startswith("error: ") and word in err, err
        assert not os.path.exists(out)
    gt, res = cases.write_artvideo(str(tmp_path / "art"))
    art = ["--protocol", "artvideo", "--gt", gt, "--results", res]
    fails(["--protocol", "artvideo", "--gt", str(tmp_path / "missing"), "--results", res], "not found")
    empty = tmp_path / "empty"
    empty.mkdir()
    fails(["--protocol", "artvideo", "--gt", str(empty), "--results", res], "no ground-truth")
    fails(art + ["--threshold", "0"], "--threshold")
    path = os.path.join(res, "video_1.json")
    good = open(path).read()
    open(path, "w").write(good[:-20])
    fails(art, "not valid JSON")
    doc = json.loads(good)
    doc["1"][0]["points"] = [1, 2, 3]
    open(path, "w").write(json.dumps(doc))
    fails(art, "x, y pairs")
    doc = json.loads(good)
    doc["2"][1]["segmentation"]["size"] = [cases.H + 1, cases.W]
    open(path, "w").write(json.dumps(doc))
    fails(art, "a mask of size")
    doc = json.loads(good)
    doc["2"][1]["segmentation"]["counts"] = [5, 5]
    open(path, "w").write(json.dumps(doc))
    fails(art, "do not add up")
    doc = json.loads(good)
    doc["1"][1]["segmentation"][0][0][0] = 2 ** 21
    open(path, "w").write(json.dumps(doc))
    fails(art, "coordinate")
    open(path, "w").write(good)
    gpath = os.path.join(gt, "video_1.json")
    gdoc = json.load(open(gpath))
    gdoc["annotations"][0]["frame_id"] = 4
    open(gpath, "w").write(json.dumps(gdoc))
    fails(art, "frame_id 4 outside")
    bgt, bres = cases.write_bovtext(str(tmp_path / "bov"))
    bov = ["--protocol", "bovtext", "--gt", bgt, "--results", bres]
    fails(bov + ["--curve"], "--curve")
    fails(["--gt", bgt, "--results", bres, "--curve"], "--curve")
    path = os.path.join(bres, "Cls2_Cartoon_video1.json")
    doc = json.load(open(path))
    doc["1"][0]["points"] = doc["1"][0]["points"][:6]
    open(path, "w").write(json.dumps(doc))
    fails(bov, "8 numbers")
    gpath = os.path.join(bgt, "Cls2_Cartoon", "Cls2_Cartoon_video1.json")
    gdoc = json.load(open(gpath))
    del gdoc["2"]
    open(gpath, "w").write(json.dumps(gdoc))
    fails(bov, "frame")


def test_host_mask_pairs_equals_the_statement():
    from gomatching_amd import score, score_json as sj
    Hh, Ww = 64, 96
    rng = np.random.RandomState(4)
    conts = ms.random_contours(36, Hh, Ww, seed=31)
    det_specs = [("poly", [c]) for c in conts[:20]] + [("poly", [conts[20], conts[21]])]
    det_specs.append(("rle", ms.rle_encode(ms.fill_contours([conts[22]], Hh, Ww))))
    det_specs.append(("poly", []))                                 # a mask without a contour: empty
    gt_imgs = [ms.fill_contours([c], Hh, Ww) for c in conts[23:35]]
    gt_imgs += [np.zeros((Hh, Ww), dtype=bool), ms.fill_contours([conts[15]], Hh, Ww)]        # empty; identical to detection 15
    gt_specs = [("rle", ms.rle_encode(g)) for g in gt_imgs]
    det_imgs = [ms.fill_contours(s[1], Hh, Ww) if s[0] == "poly" else ms.rle_decode({"size": [Hh, Ww], "counts": s[1]})
                for s in det_specs]
    gt_off, det_off = [0, 5, 5, 9, 14], [0, 8, 12, 12, 23]        # a frame without ground truth, one without detections
    gt_key = rng.randint(0, 2, len(gt_specs)).astype(np.int32)
    det_key = rng.randint(0, 2, len(det_specs)).astype(np.int32)
    gt_key[-1] = det_key[15] = 0
    gs, ds = sj.MaskSet(gt_specs, Hh, Ww), sj.MaskSet(det_specs, Hh, Ww)
    seen = 0
    for thr in (0.05, 0.3, float(np.nextafter(0.5, 0.0))):
        counts, det, val = sj.host_mask_pairs(gs, ds, gt_off, det_off, gt_key, det_key, thr)
        wc, kept, eligible = ms.mask_pairs_statement(gt_imgs, det_imgs, gt_off, det_off, gt_key, det_key, thr)
        assert counts.dtype == np.int32 and det.dtype == np.int32 and val.dtype == np.float64
        assert np.array_equal(counts, wc)
        assert det.tolist() == [j for _, j, _ in kept]
        assert val.tobytes() == np.asarray([v for _, _, v in kept], dtype=np.float64).tobytes()
        again = score.host_mask_pairs(gs, ds, gt_off, det_off, gt_key, det_key, thr)                # the name under `score`
        assert all(a.tobytes() == b.tobytes() for a, b in zip((counts, det, val), again))
        seen += len(kept)
    assert seen > 10 and any(v == 1.0 for _, _, v in eligible) and any(v == 0.0 for _, _, v in eligible)
    # chunks by frames (the 256 MiB rule, here with a tiny limit) cut only between frames and cover them all
    chunks = sj._frame_chunks(gs, ds, np.asarray(gt_off), np.asarray(det_off), 300)
    assert len(chunks) > 1 and chunks[0][0] == 0 and chunks[-1][1] == 4 and all(a[1] == b[0] for a, b in zip(chunks, chunks[1:]))


def test_mask_entry_points_reject_bad_arguments_without_a_gpu():
    """Argument checks run before any HIP call (the pattern of test_score_entry_points_reject_bad_arguments_without_a_gpu)."""
    from gomatching_amd import lib
    L = lib.load()
    INVALID, OK = 1, 0
    p = ctypes.c_void_p(0x1000)                                   # non-null, aligned, never dereferenced

    def poly(pts=p, P=8, co=p, C=2, mc=p, bx=p, wo=p, N=2, nwords=10, sel=None, M=2, H=40, W=80, words=p, area=p):
        return L.gom_mask_fill_polygons_u32(pts, P, co, C, mc, bx, wo, N, nwords, sel, M, H, W, words, area, None)

    def rle(ends=p, R=6, ro=p, bx=p, wo=p, N=2, nwords=10, sel=None, M=2, H=40, W=80, words=p, area=p):
        return L.gom_mask_fill_rle_u32(ends, R, ro, bx, wo, N, nwords, sel, M, H, W, words, area, None)
    for fn in (poly, rle):
        for name in ("bx", "wo", "words", "area"):
            assert fn(**{name: None}) == INVALID, name
        assert fn(N=-1) == INVALID and fn(nwords=-1) == INVALID and fn(M=-1) == INVALID
        assert fn(H=0) == INVALID and fn(W=0) == INVALID and fn(H=65536, W=32768) == INVALID       # H * W does not fit int32
        assert fn(M=1) == INVALID                                 # without sel every mask is filled
        assert fn(sel=p, M=3) == INVALID                          # more selected masks than masks
        assert fn(sel=p, M=0) == OK and fn(N=0, M=0, nwords=0) == OK                               # nothing to do, nothing launched
        assert fn(bx=ctypes.c_void_p(0x1004)) == INVALID          # a box is read as one 16-byte word
    assert poly(pts=None) == INVALID and poly(co=None) == INVALID and poly(mc=None) == INVALID
    assert poly(P=-1) == INVALID and poly(C=-1) == INVALID
    assert rle(ends=None) == INVALID and rle(ro=None) == INVALID and rle(R=-1) == INVALID

    names = ("gw", "gb", "go", "ga", "dw", "db", "do", "da", "gf", "df", "gk", "dk")

    def count(G=4, D=6, F=2, gn=10, dn=10, pairs=12, thr=0.5, counts=p, **kw):
        a = {n: kw.get(n, p) for n in names}
        return L.gom_mask_pairs_count_f64(a["gw"], a["gb"], a["go"], a["ga"], gn, a["dw"], a["db"], a["do"], a["da"], dn, a["gf"],
                                          a["df"], a["gk"], a["dk"], G, D, F, pairs, thr, counts, None)

    def emit(G=4, D=6, F=2, gn=10, dn=10, pairs=12, thr=0.5, scan=p, total=3, od=p, ov=p, **kw):
        a = {n: kw.get(n, p) for n in names}
        return L.gom_mask_pairs_emit_f64(a["gw"], a["gb"], a["go"], a["ga"], gn, a["dw"], a["db"], a["do"], a["da"], dn, a["gf"],
                                         a["df"], a["gk"], a["dk"], G, D, F, pairs, thr, scan, total, od, ov, None)
    for fn, none_kept in ((count, {}), (emit, {"total": 0})):
        for name in names:
            assert fn(**{name: None}) == INVALID, name
        assert fn(G=-1) == INVALID and fn(D=-1) == INVALID and fn(F=-1) == INVALID and fn(gn=-1) == INVALID and fn(dn=-1) == INVALID
        assert fn(F=0) == INVALID                                 # masks without a frame
        assert fn(gb=ctypes.c_void_p(0x1004)) == INVALID and fn(db=ctypes.c_void_p(0x1008)) == INVALID     # box alignment
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
