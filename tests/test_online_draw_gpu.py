"""GPU: pictures from an online session.  `OnlineSpotter(draw=True)` at 2 frames per step over a 48-frame synthetic clip of
72 x 128 frames -- longer than the session's ring of 29 frames, so the pixel ring wraps -- with pushes of 2 and of 8 frames and
with `device_text` off and on: the concatenated `take_drawn()` frames equal `show.draw_clip` of the same frames and the offline
rows, byte for byte; what `push` / `close()` return equals what a session without `draw` returns; every `take_drawn()` covers
exactly the frames the same call returned; a frame of another size raises before the push runs anything; and the device
memory the session holds is the same after frame 30 and after the last frame."""
import gc

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
OPTS = ["MODEL.TRANSFORMER.NUM_QUERIES", "12", "INPUT.MIN_SIZE_TEST", "128", "INPUT.MAX_SIZE_TEST", "256", "MODEL.DEVICE", DEV]
FRAMES, H, W, STEP = 48, 72, 128, 2
_built = {}


def _time_cost():
    from gomatching_amd.predictor import new_time_cost
    return new_time_cost()


def _case():
    """Model, clip, the offline rows and the offline pictures, computed once and left unchanged."""
    if not _built:
        from gomatching_amd import results, show
        from gomatching_amd.config import setup_cfg
        from gomatching_amd.modeling import GoMatching
        from gomatching_amd.predictor import GoMBatchPredictor, TextDecoder
        from gomatching_amd.synth import make_clip
        from gomatching_amd.weights import synth_state_dict
        cfg = setup_cfg(builtin="icdar15", opts=OPTS)
        sd = synth_state_dict(cfg, seed=7, cls_bias={"detection_transformer.ctrl_point_class.0.bias": 0.5})
        model = GoMatching(cfg, sd, device=DEV, frames_per_step=STEP)
        dec = TextDecoder(cfg.MODEL.TRANSFORMER.VOC_SIZE, cfg.MODEL.TRANSFORMER.CUSTOM_DICT)
        frames = [np.ascontiguousarray(f[:, :, ::-1]) for f in make_clip(FRAMES, H, W, clip_id=3)]     # BGR, as read_frame yields
        preds, _ = results.spot_video(GoMBatchPredictor(cfg, model, device_ingest=True), frames, _time_cost())
        rows = results.clip_lines(preds, dec)
        want = show.draw_clip(frames, rows, cfg.MODEL.TRANSFORMER.VOC_SIZE)
        _built.update(cfg=cfg, model=model, dec=dec, frames=frames, rows=rows, want=want)
    return _built


def _held(base):
    gc.collect()
    torch.cuda.synchronize()
    return torch.cuda.memory_allocated() - base


def _stream(case, push, device_text, draw, resident):
    """One session over the clip -> (items of push / close, [(first, frames)] drawn, memory held after frame 30 and after the
    last frame, the session).  resident: the frames go in as CUDA tensors, as `eval.decode_frames` hands them over."""
    from gomatching_amd.online import OnlineSpotter
    frames = case["frames"]
    gc.collect()
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    s = OnlineSpotter(case["cfg"], case["model"], case["dec"], device_ingest=True, device_text=device_text,
                      draw=True if draw else None)
    items, drawn, held = [], [], {}

    def took(out):
        items.extend(out)
        got = s.take_drawn() if draw else []
        if draw:                                                          # exactly the frames the same call returned
            a = [(i[0], i[0] + i[1]) for i in out] if device_text else [(f, f + 1) for f, _ in out]
            covered = [f for first, t in got for f in range(first, first + t.shape[0])]
            assert covered == [f for lo, hi in a for f in range(lo, hi)]
            assert s.take_drawn() == []
        drawn.extend((first, t.cpu().numpy()) for first, t in got)

    for f0 in range(0, len(frames), push):
        part = frames[f0:f0 + push]
        if resident:
            part = [torch.from_numpy(f).to(DEV) for f in part]
        took(s.push(part))
        del part
        if "30" not in held and f0 + push >= 30:
            held["30"] = _held(base)
    held["last"] = _held(base)
    took(s.close())
    return items, drawn, held, s


@pytest.mark.parametrize("device_text", [False, True])
@pytest.mark.parametrize("push", [2, 8])
def test_online_pictures_equal_offline_pictures(push, device_text):
    case = _case()
    frames, rows, want = case["frames"], case["rows"], case["want"]
    assert sum(len(r) for r in rows) > 0 and (want != np.stack(frames)).any()       # not a comparison of undrawn frames
    plain_items, _, plain_held, plain = _stream(case, push, device_text, draw=False, resident=True)
    items, drawn, held, s = _stream(case, push, device_text, draw=True, resident=(push == 8))
    assert plain.ring_px is None and plain.take_drawn() == []
    assert s.cap_frames == 29 < FRAMES and tuple(s.ring_px.shape) == (29, H, W, 3)   # the pixel ring wrapped
    # rows / text: those of a session without `draw`, and (rows) the offline ones
    assert items == plain_items
    if not device_text:
        assert [f for f, _ in items] == list(range(FRAMES))
        for f, r in items:
            assert r == rows[f], "frame %d" % f
    # pictures
    assert [first for first, _ in drawn] == sorted(first for first, _ in drawn)
    got = np.concatenate([t for _, t in drawn])
    assert got.shape == want.shape
    for f in range(FRAMES):
        assert np.array_equal(got[f], want[f]), "frame %d: the online picture differs from show.draw_clip's" % f
    # memory: flat from frame 30 to the end, and drawing adds the same amount at both points
    print("push %d, device_text %s: held after frame 30 / the last frame: %d / %d bytes with draw, %d / %d without; ring_px %d"
          % (push, device_text, held["30"], held["last"], plain_held["30"], plain_held["last"], s.ring_px.numel()))
    assert held["last"] - plain_held["last"] == held["30"] - plain_held["30"]
    assert held["last"] == held["30"]


def test_a_frame_of_another_size_is_refused_before_the_push_runs():
    from gomatching_amd.online import OnlineSpotter
    from gomatching_amd.show import ShowError
    case = _case()
    frames = case["frames"]
    s = OnlineSpotter(case["cfg"], case["model"], case["dec"], device_ingest=True, draw=True)
    out = s.push(frames[:2])
    seen, tracked = s.frames_seen, len(s.instances)
    with pytest.raises(ShowError, match="share one size"):
        s.push([frames[2], np.ascontiguousarray(frames[3][:, :100])])
    assert (s.frames_seen, len(s.instances), len(s._buffer)) == (seen, tracked, 0)   # nothing was taken in, nothing ran
    out += s.push(frames[2:4]) + s.close()                                # the session goes on
    assert [f for f, _ in out] == [0, 1, 2, 3]
    got = np.concatenate([t.cpu().numpy() for _, t in s.take_drawn()])
    assert got.shape == (4, H, W, 3)
    with pytest.raises(ValueError, match="device_ingest"):
        OnlineSpotter(case["cfg"], case["model"], case["dec"], device_ingest=False, draw=True)
