"""`gom_quad_det_match_f64` on the GPU: det_care, match and frame_stats must equal the host path's (`score_det.
host_quad_det_match`, numpy float64, itself held to the plain statement and to the reference's figures by
test_score_det_cpu.py) EXACTLY, on every frame of one call built from the smallest shapes at which the kernel can go wrong
(det_statement.edge_video: 70 frames, more than the waves of a workgroup; frames without ground truth, without detections and
without both; 1 x 1; D = 65 with the only passing detection at index 64; index 64 winning after an earlier object took index
3; G = 130; first candidates that are don't-care detections; IoU and overlap of exactly 0.5; zero-area quads on both sides;
60 seeded random frames).  No tolerance anywhere: the outputs are integers."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import det_statement as DS

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = -77
_cache = {}


def _video():
    if "video" not in _cache:
        from gomatching_amd import score_det
        v, notes = DS.edge_video()
        host = score_det.host_quad_det_match(v["gt_quads"], v["det_quads"], v["gt_off"], v["det_off"], v["gt_care"])
        _cache["video"] = (v, notes, host)
    return _cache["video"]


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(DEV)


def _run(v, frames=None):
    """The op on the frames [a, b) of `v` (all by default) -> numpy (det_care, match, frame_stats)."""
    from gomatching_amd import ops
    a, b = frames or (0, len(v["gt_off"]) - 1)
    g0, g1, d0, d1 = v["gt_off"][a], v["gt_off"][b], v["det_off"][a], v["det_off"][b]
    out = ops.quad_det_match(_t(v["gt_quads"][g0:g1]), _t(v["det_quads"][d0:d1]), _t(v["gt_off"][a:b + 1] - g0),
                             _t(v["det_off"][a:b + 1] - d0), _t(v["gt_care"][g0:g1]))
    assert all(t.dtype == torch.int32 for t in out)
    return tuple(t.cpu().numpy() for t in out)


def test_every_frame_equals_the_host_path():
    v, notes, host = _video()
    got = _run(v)
    go, do = v["gt_off"], v["det_off"]
    assert got[0].shape == host[0].shape and got[1].shape == host[1].shape and got[2].shape == (70, 3)
    for f in range(70):
        what = (f, notes.get(f, "random"))
        assert got[0][do[f]:do[f + 1]].tolist() == host[0][do[f]:do[f + 1]].tolist(), what
        assert got[1][go[f]:go[f + 1]].tolist() == host[1][go[f]:go[f + 1]].tolist(), what
        assert got[2][f].tolist() == host[2][f].tolist(), what
    m = lambda f: got[1][go[f]:go[f + 1]].tolist()
    assert m(4) == [64] and m(5) == [3, 64] and m(7) == [2, -1] and m(8) == [-1, -1, 2] and m(9) == [-1, 2, -1, -1]
    assert got[2][0].tolist() == [0, 0, 0] and got[2][3].tolist() == [1, 1, 1]
    print("matched %d of %d care objects, %d of %d detections stay" % (got[2][:, 0].sum(), got[2][:, 1].sum(), got[2][:, 2].sum(),
                                                                      len(got[0])))


def test_two_runs_and_two_halves_give_the_same():
    v, _, host = _video()
    a, b = _run(v), _run(v)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()
    first, second = _run(v, (0, 33)), _run(v, (33, 70))            # an odd split: the frames land on other waves and workgroups
    for k in range(3):
        assert np.concatenate([first[k], second[k]]).tobytes() == a[k].tobytes()


def test_match_equals_a_greedy_sweep_over_quad_pairs():
    """The same geometry bits through both kernels: the pairs `ops.quad_pairs` keeps, swept greedily on the host."""
    from gomatching_amd import score_det
    v, _, host = _video()
    got = _run(v)
    comp = score_det.composed_quad_det_match(v["gt_quads"], v["det_quads"], v["gt_off"], v["det_off"], v["gt_care"])
    for x, y in zip(got, comp):
        assert x.tobytes() == y.tobytes()


def test_words_beyond_the_sizes_keep_the_sentinel():
    from gomatching_amd.ops import _L, _p, _stream, check
    v, _, host = _video()
    G, D, F = len(v["gt_quads"]), len(v["det_quads"]), len(v["gt_off"]) - 1
    slack = 257
    det_care = torch.full((D + slack,), SENTINEL, dtype=torch.int32, device=DEV)
    match = torch.full((G + slack,), SENTINEL, dtype=torch.int32, device=DEV)
    stats = torch.full((F * 3 + slack,), SENTINEL, dtype=torch.int32, device=DEV)
    t = [_t(v[k]) for k in ("gt_quads", "det_quads", "gt_off", "det_off", "gt_care")]
    with torch.cuda.device(DEV):
        check(_L().gom_quad_det_match_f64(*[_p(x) for x in t], G, D, F, 0.5, 0.5, _p(det_care), _p(match), _p(stats), _stream()))
    torch.cuda.synchronize()
    assert det_care[:D].cpu().numpy().tolist() == host[0].tolist() and bool((det_care[D:] == SENTINEL).all())
    assert match[:G].cpu().numpy().tolist() == host[1].tolist() and bool((match[G:] == SENTINEL).all())
    assert stats[:F * 3].cpu().numpy().tolist() == host[2].reshape(-1).tolist() and bool((stats[F * 3:] == SENTINEL).all())


def test_nothing_to_do_and_argument_checks():
    from gomatching_amd import ops
    e = lambda *shape: torch.zeros(shape, dtype=torch.int32, device=DEV)
    dc, m, st = ops.quad_det_match(e(0, 8), e(0, 8), e(1), e(1), e(0))                                 # F = 0
    assert dc.numel() == 0 and m.numel() == 0 and tuple(st.shape) == (0, 3)
    dc, m, st = ops.quad_det_match(e(0, 8), e(0, 8), e(4), e(4), e(0))                                 # three empty frames
    assert st.cpu().tolist() == [[0, 0, 0]] * 3
    quads = torch.tensor([[0, 0, 9, 0, 9, 9, 0, 9]] * 2, dtype=torch.int32, device=DEV)
    with pytest.raises(ValueError):
        ops.quad_det_match(quads.cpu(), quads, e(2), e(2), e(2))
    with pytest.raises(ValueError):
        ops.quad_det_match(quads, quads, e(2), e(3), e(2))
    with pytest.raises(ValueError):
        ops.quad_det_match(quads, quads, e(2), e(2), e(2), max_det=5000)
    from gomatching_amd.lib import GomError
    with pytest.raises(GomError):
        ops.quad_det_match(quads, quads, e(2), e(2), e(2), iou_thr=1.0)


def test_command_line_through_the_kernel_equals_host_iou(tmp_path):
    from gomatching_amd import score
    raw = os.path.join(ROOT, "tests", "golden", "score_det_raw")
    gt, res = os.path.join(raw, "gt"), os.path.join(raw, "res")
    dev, host = str(tmp_path / "device.json"), str(tmp_path / "host.json")
    r = subprocess.run([sys.executable, "-m", "gomatching_amd.score", "--det", "--gt", gt, "--results", res, "--per-frame",
                        "--output", dev], cwd=ROOT, capture_output=True, text=True, timeout=300)   # a child, as a user starts it
    assert r.returncode == 0, r.stderr
    assert r.stdout.startswith("method: precision 0.3636  recall 0.4000  hmean 0.3810")
    assert score.main(["--det", "--gt", gt, "--results", res, "--per-frame", "--host-iou", "--output", host]) == 0
    assert open(dev, "rb").read() == open(host, "rb").read()
    doc = json.load(open(dev))
    assert doc["per_sample"]["res_Video_2_1_1_2.txt"]["pairs"] == [{"gt": 0, "det": 0}, {"gt": 2, "det": 2}]
