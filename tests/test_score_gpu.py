"""`gom_quad_pairs_count_f64` / `gom_quad_pairs_emit_f64` on the GPU against the float64 statement (score_statement.py), and
the scoring command line through the kernels against its --host-iou path.

Every comparison first asserts, on the statement alone, that no eligible pair's value lies within 1e-6 of the threshold: a
condition on the inputs, so it cannot hide a kernel error.  Under it the kept (ground truth, detection) lists must be
identical, in order, and the values within 1e-9: coordinates are at most 2^13 and areas at most 2^26, a clip runs about a
hundred fp64 operations, so 1e-9 is three orders above that rounding."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import score_statement as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_cache = {}


def _run(v, gk, dk, measure, thr):
    from gomatching_amd import ops
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(DEV)
    counts, det, val = ops.quad_pairs(t(v["gt_quads"]), t(v["det_quads"]), t(v["gt_off"]), t(v["det_off"]), t(gk), t(dk), measure, thr)
    assert counts.dtype == torch.int32 and det.dtype == torch.int32 and val.dtype == torch.float64
    return counts.cpu().numpy(), det.cpu().numpy(), val.cpu().numpy()


def _compare(tag, v, gk, dk, measure, thr):
    key = (tag, measure, thr)
    if key not in _cache:
        _cache[key] = S.pairs_statement(v["gt_quads"], v["det_quads"], v["gt_off"], v["det_off"], gk, dk, measure, thr)
    want_counts, kept, eligible = _cache[key]
    margin = min([abs(x - thr) for _, _, x in eligible] or [1.0])
    print("%s measure %d: %d eligible pairs, %d kept, closest to the threshold %.3g" % (tag, measure, len(eligible), len(kept), margin))
    assert margin > 1e-6, "the inputs hold a pair within 1e-6 of the threshold"
    counts, det, val = _run(v, gk, dk, measure, thr)
    assert int(counts.sum()) == len(det) == len(val)
    assert counts.tolist() == want_counts.tolist()
    assert det.tolist() == [j for _, j, _ in kept]
    err = float(np.abs(val - np.asarray([x for _, _, x in kept], dtype=np.float64)).max()) if len(kept) else 0.0
    print("%s measure %d: max |value - statement| = %.3g" % (tag, measure, err))
    assert err <= 1e-9
    return counts, det, val, kept


def _fixture():
    if "fixture" not in _cache:
        v = S.fixture_video()
        rng = np.random.RandomState(11)
        # keys 0..2 on the ground truth, 0..3 on the detections (3 on one side only); mostly equal so that pairs remain
        gk = (rng.rand(len(v["gt_quads"])) < 0.25).astype(np.int32) * rng.randint(1, 3, size=len(v["gt_quads"])).astype(np.int32)
        dk = (rng.rand(len(v["det_quads"])) < 0.25).astype(np.int32) * rng.randint(1, 4, size=len(v["det_quads"])).astype(np.int32)
        _cache["fixture"] = (v, gk, dk)
    return _cache["fixture"]


@pytest.mark.parametrize("measure", [0, 1])
def test_fixture_pairs_equal_the_statement(measure):
    v, gk, dk = _fixture()
    zg, zd = np.zeros_like(gk), np.zeros_like(dk)
    _, _, _, kept = _compare("fixture", v, zg, zd, measure, 0.5)
    assert len(kept) >= 40


def test_fixture_pairs_with_keys_equal_the_statement():
    v, gk, dk = _fixture()
    assert set(gk.tolist()) == {0, 1, 2} and set(dk.tolist()) == {0, 1, 2, 3}
    _, _, _, kept = _compare("fixture-keys", v, gk, dk, 0, 0.5)
    _, all_kept, _ = S.pairs_statement(v["gt_quads"], v["det_quads"], v["gt_off"], v["det_off"], gk * 0, dk * 0, 0, 0.5)
    assert 10 <= len(kept) < len(all_kept)                      # the keys removed pairs and left pairs


def _edge_video():
    """Frames that reach the lane and wave edges: 63, 64, 65 and 130 detections against 3 ground-truth objects, a frame
    without ground truth, one without detections, G = 1 with D = 1, degenerate quads on either side, the last frame empty."""
    rng = np.random.RandomState(23)
    gt, det, goff, doff = [], [], [0], [0]

    def rect(x, y, w, h):
        return np.array([x, y, x + w, y, x + w, y + h, x, y + h], dtype=np.int64)

    def close():
        goff.append(len(gt))
        doff.append(len(det))
    for nd in (63, 64, 65, 130):
        boxes = [rect(20, 20, 60, 40), rect(200, 30, 50, 50), rect(100, 200, 80, 30)]
        gt += boxes
        for j in range(nd):                                       # every detection near one of the three, in turn
            det.append(np.maximum(boxes[j % 3] + rng.randint(-7, 8, size=8), 0))
        close()
    det += [rect(5, 5, 20, 20)] * 5                               # no ground truth
    close()
    gt += [rect(5, 5, 20, 20), rect(50, 50, 20, 20)]              # no detections
    close()
    gt.append(rect(10, 10, 30, 30))                               # G = 1, D = 1
    det.append(rect(12, 11, 30, 30))
    close()
    gt += [np.array([0, 0, 10, 10, 20, 20, 30, 30]), rect(40, 40, 20, 20), np.array([0, 0, 40, 40, 40, 0, 0, 40])]
    det += [rect(0, 0, 30, 30), np.array([45, 45, 45, 45, 45, 45, 45, 45]), np.array([40, 40, 60, 60, 60, 40, 40, 60]),
            np.array([40, 40, 60, 40, 60, 40, 40, 60]), rect(2, 2, 36, 36)]
    close()
    close()                                                      # the last frame is empty
    i32 = lambda a, shape: np.asarray(a, dtype=np.int32).reshape(shape)
    return {"gt_quads": i32(gt, (-1, 8)), "det_quads": i32(det, (-1, 8)), "gt_off": i32(goff, (-1,)), "det_off": i32(doff, (-1,))}


@pytest.mark.parametrize("measure", [0, 1])
def test_lane_and_wave_edges(measure):
    v = _edge_video()
    zg, zd = np.zeros(len(v["gt_quads"]), dtype=np.int32), np.zeros(len(v["det_quads"]), dtype=np.int32)
    counts, det, _, _ = _compare("edges", v, zg, zd, measure, 0.3)
    assert counts[9:12].min() >= 40 and det.max() >= 128          # the 130-detection frame keeps pairs past two wavefronts
    go = v["gt_off"]
    assert counts[go[5]:go[6]].tolist() == [0, 0]                 # the frame without detections
    assert counts[go[6]] == 1                                     # G = 1, D = 1
    assert counts[go[7]] == 0                                     # the collinear ground-truth quad pairs with nothing


def test_nothing_to_do():
    from gomatching_amd import ops
    e = lambda *shape: torch.zeros(shape, dtype=torch.int32, device=DEV)
    counts, det, val = ops.quad_pairs(e(0, 8), e(0, 8), e(1), e(1), e(0), e(0), 0, 0.5)           # F = 0
    assert counts.numel() == 0 and det.numel() == 0 and val.numel() == 0
    counts, det, val = ops.quad_pairs(e(0, 8), e(3, 8), e(3), torch.tensor([0, 1, 3], dtype=torch.int32, device=DEV), e(0), e(3), 0, 0.5)
    assert counts.numel() == 0 and det.numel() == 0
    quads = torch.tensor([[0, 0, 9, 0, 9, 9, 0, 9]] * 2, dtype=torch.int32, device=DEV)
    counts, det, val = ops.quad_pairs(quads, e(0, 8), torch.tensor([0, 1, 2], dtype=torch.int32, device=DEV), e(3), e(2), e(0), 1, 0.5)
    assert counts.tolist() == [0, 0] and det.numel() == 0
    from gomatching_amd.lib import GomError
    with pytest.raises(GomError):
        ops.quad_pairs(quads, quads, e(2), e(2), e(2), e(2), 2, 0.5)                                # measure outside {0, 1}
    with pytest.raises(ValueError):
        ops.quad_pairs(quads.cpu(), quads, e(2), e(2), e(2), e(2), 0, 0.5)
    with pytest.raises(ValueError):
        ops.quad_pairs(quads.to(torch.int64), quads, e(2), e(2), e(2), e(2), 0, 0.5)


def test_two_runs_are_bitwise_equal():
    v, gk, dk = _fixture()
    e = _edge_video()
    ze = (np.zeros(len(e["gt_quads"]), dtype=np.int32), np.zeros(len(e["det_quads"]), dtype=np.int32))
    for video, keys, thr in ((v, (gk, dk), 0.5), (e, ze, 0.3)):
        a, b = _run(video, *keys, 0, thr), _run(video, *keys, 0, thr)
        for x, y in zip(a, b):
            assert x.tobytes() == y.tobytes()


def test_command_line_through_the_kernels_equals_host_iou(tmp_path):
    from gomatching_amd import score
    gt, res = S.write_tree(str(tmp_path / "t"))
    out = {k: str(tmp_path / (k + ".json")) for k in ("device", "host", "e2e_device", "e2e_host")}
    r = subprocess.run([sys.executable, "-m", "gomatching_amd.score", "--gt", gt, "--results", res, "--output", out["device"]],
                       cwd=ROOT, capture_output=True, text=True, timeout=300)           # a child process, as a user starts it
    assert r.returncode == 0, r.stderr
    assert r.stdout.startswith("method: MOTA")
    assert score.main(["--gt", gt, "--results", res, "--host-iou", "--output", out["host"]]) == 0
    assert score.main(["--gt", gt, "--results", res, "--e2e", "--output", out["e2e_device"]]) == 0
    assert score.main(["--gt", gt, "--results", res, "--e2e", "--host-iou", "--output", out["e2e_host"]]) == 0
    docs = {k: json.load(open(p)) for k, p in out.items()}
    assert docs["device"] == docs["host"]
    assert docs["e2e_device"] == docs["e2e_host"]
    for k, exp in S.TRACKING_EXPECTED.items():
        for name, want in exp.items():
            assert abs(docs["device"]["per_sample"][k][name] - want) <= 1e-12
