"""`gom_result_rows_i32` on the GPU.  Comparison (a) of the two the feature keeps apart: every output word of the kernel equals
the plain-Python fp64 statement (result_rows_statement.py) -- exact, no exceptions: with unfused, once-rounded fp64 on the
device a differing word is a kernel bug or a contraction the compiler slipped in, never noise.  Then `clip_lines` on the
CUDA results of a tracked clip against `frame_lines` frame by frame (comparison (b) on network outputs: instances the
host itself decides by rounding are reported and left out, at most 0.1 % of them)."""
import ctypes

import numpy as np
import pytest
import torch

import result_rows_statement as S
from helpers import mini_cfg

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_geometry = {}


def _inputs(n):
    if n not in _geometry:
        bd = S.mixed(n)
        _geometry[n] = (bd, S.geometry_words(bd))
    return _geometry[n]


@pytest.mark.parametrize("voc", [37, 5462])
@pytest.mark.parametrize("n", [0, 1, 7, 100, 30000])
def test_kernel_words_equal_the_statement(n, voc):
    from gomatching_amd import ops
    bd, geo = _inputs(n)
    recs = S.random_recs(n, voc, seed=n + voc)
    ids = (np.arange(n, dtype=np.int64) * 3 + 1) | (np.int64(1) << 40) * (np.arange(n, dtype=np.int64) % 2)
    want = S.text_words(geo, recs, voc, ids)
    got = ops.result_rows(torch.as_tensor(bd).to(DEV), torch.as_tensor(recs).to(DEV), voc,
                          torch.as_tensor(ids).to(DEV)).cpu().numpy()
    assert got.shape == (n, S.WORDS) and got.dtype == np.int32
    bad = np.argwhere(got != want)
    print("n %d voc %d: words differing %d of %d" % (n, voc, len(bad), want.size))
    assert len(bad) == 0, "first differing (instance, word): %s got %s want %s" % (
        bad[:5].tolist(), [int(got[i, j]) for i, j in bad[:5]], [int(want[i, j]) for i, j in bad[:5]])
    if n:                                                   # without ids the id words are zero, the rest unchanged
        no_ids = ops.result_rows(torch.as_tensor(bd).to(DEV), torch.as_tensor(recs).to(DEV), voc).cpu().numpy()
        assert np.array_equal(no_ids[:, :S.TRACK_ID], want[:, :S.TRACK_ID]) and not no_ids[:, S.TRACK_ID:].any()


@pytest.mark.parametrize("name", list(S.FAMILY_COUNTS))
def test_kernel_words_equal_the_statement_per_family(name):
    from gomatching_amd import ops
    bd = S.family(name, 300 if name in ("smooth", "axis", "noisy") else 100)
    n = len(bd)
    recs = S.random_recs(n, 37, seed=5)
    ids = np.arange(n, dtype=np.int64)
    want = S.statement_words(bd, recs, 37, ids)
    got = ops.result_rows(torch.as_tensor(bd).to(DEV), torch.as_tensor(recs).to(DEV), 37,
                          torch.as_tensor(ids).to(DEV)).cpu().numpy()
    bad = np.argwhere(got != want)
    print("%s: words differing %d of %d" % (name, len(bad), want.size))
    assert len(bad) == 0, bad[:5].tolist()


def test_clip_lines_equals_frame_lines_on_a_tracked_clip():
    from gomatching_amd import results
    from gomatching_amd.modeling import GoMatching
    from gomatching_amd.predictor import GoMBatchPredictor, TextDecoder, boundary_to_polygon, new_time_cost
    from gomatching_amd.synth import make_clip
    from gomatching_amd.weights import synth_state_dict
    cfg = mini_cfg("icdar15", device=DEV)
    cfg.INPUT.MIN_SIZE_TEST, cfg.INPUT.MAX_SIZE_TEST = 128, 256
    sd = synth_state_dict(cfg, seed=7, cls_bias={"detection_transformer.ctrl_point_class.0.bias": 0.5})
    model = GoMatching(cfg, sd, device=DEV, frames_per_step=4)
    spotter = GoMBatchPredictor(cfg, model, device_ingest=True)
    frames = [np.ascontiguousarray(f[:, :, ::-1]) for f in make_clip(7, 72, 128, clip_id=3)]
    preds, _ = results.spot_video(spotter, frames, new_time_cost())
    dec = TextDecoder(cfg.MODEL.TRANSFORMER.VOC_SIZE)
    assert all(r["instances"].bd.is_cuda for r in preds if len(r["instances"]))
    # min_extent = 0 keeps every instance, so rows align with instances and a near-tie can be attributed to one
    want = [results.frame_lines(r["instances"], dec, min_extent=0) for r in preds]
    got = results.clip_lines(preds, dec, min_extent=0)
    total = sum(len(r["instances"]) for r in preds)
    differ, near = 0, 0
    for r, w, g in zip(preds, want, got):
        assert len(w) == len(g) == len(r["instances"])
        bd = r["instances"].bd.cpu().numpy().reshape(-1, 25, 4)
        for k, (a, b) in enumerate(zip(w, g)):
            if a != b:
                differ += 1
                near += bool(S.near_tie(boundary_to_polygon(bd[k])))
    print("tracked clip: instances %d, rows differing %d, of them near-ties left out %d" % (total, differ, near))
    assert near <= total // 1000 and differ == near
    kept = results.clip_lines(preds, dec)                    # and with the filter the writers use
    assert sum(len(rows) for rows in kept) > 0
    if differ == 0:
        assert kept == [results.frame_lines(r["instances"], dec) for r in preds]


def test_entry_point_rejects_bad_arguments_without_launching():
    from gomatching_amd import lib, ops
    L = lib.load()
    INVALID = 1
    p = ctypes.c_void_p(0x1000)                              # non-null, never dereferenced
    W = S.WORDS
    assert L.gom_result_rows_i32(p, p, p, -1, 37, p, W, None) == INVALID          # n < 0
    assert L.gom_result_rows_i32(p, p, p, 4, 1, p, W, None) == INVALID           # voc_size < 2
    assert L.gom_result_rows_i32(p, p, p, 4, 37, p, W - 1, None) == INVALID      # short ld
    assert L.gom_result_rows_i32(None, p, p, 4, 37, p, W, None) == INVALID
    assert L.gom_result_rows_i32(p, None, p, 4, 37, p, W, None) == INVALID
    assert L.gom_result_rows_i32(p, p, p, 4, 37, None, W, None) == INVALID
    assert L.gom_result_rows_i32(p, p, None, 0, 37, p, W, None) == 0             # n == 0: GOM_OK, nothing launched
    assert ops.RESULT_ROWS_WORDS == W
    bd = torch.zeros(3, 25, 4, device=DEV)
    with pytest.raises(ValueError):
        ops.result_rows(bd.cpu(), torch.zeros(3, 25, dtype=torch.int64), 37)
    with pytest.raises(ValueError):
        ops.result_rows(bd, torch.zeros(3, 25, dtype=torch.int32, device=DEV), 37)
    with pytest.raises(ValueError):
        ops.result_rows(bd[:, :24], torch.zeros(3, 25, dtype=torch.int64, device=DEV), 37)
    with pytest.raises(lib.GomError):
        ops.result_rows(bd, torch.zeros(3, 25, dtype=torch.int64, device=DEV), 1)
