"""The online session (gomatching_amd/online.py) against the offline path on the GPU: every frame's rows (ids, points, text,
segmentation) equal what `batch_inference` in 100-frame batches, `_remove_short_track`, `batch_postprocess` and `clip_lines`
give once the whole video is in -- (a) with detection stubbed out on a 130-frame trace, at several step sizes and with pushes
of uneven size, (b) with the real detector on a spliced clip, through the library and through `eval --online`."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from PIL import Image

from helpers import mini_cfg

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NET_HW, SRC_HW = (96, 128), (144, 192)                              # network input and source frame of the stubbed trace
PUSHES = [1, 5, 2, 11, 3, 8, 17, 4, 9, 6, 13, 7, 10, 12, 22]        # 130 frames in pushes of uneven size
_built = {}


def _time_cost():
    from gomatching_amd.predictor import new_time_cost
    return new_time_cost()


def _trace(frames, dim, seed):
    """Per frame (reid [n, dim], boxes [n, 4], bd [n, 25, 4], recs [n, 25], scores [n]): six lasting objects that drop out
    for 1..4 frames and come back, objects that live for 1..3 frames only, and entirely empty frames."""
    g = np.random.default_rng(seed)

    def obj():
        return {"f": g.standard_normal(dim).astype(np.float32), "xy": g.uniform(10, 90, 2), "v": g.uniform(-0.3, 0.3, 2)}
    lasting = [dict(obj(), off=0, born=int(b)) for b in (0, 0, 0, 0, 9, 33)]
    brief = []
    out = []
    for t in range(frames):
        if t % 9 == 4:
            brief.append(dict(obj(), left=int(g.integers(1, 4))))
        feats, boxes = [], []
        empty = t % 37 == 20
        for k, o in enumerate(lasting):
            o["xy"] = np.clip(o["xy"] + o["v"], 2, 100)
            if t < o["born"]:
                continue
            if o["off"] == 0 and t % 11 == (3 * k) % 11 and t > o["born"] + 6:
                o["off"] = 1 + (t // 11 + k) % 4                     # a drop-out of 1..4 frames
            if o["off"] > 0:
                o["off"] -= 1
                continue
            if not empty:
                feats.append(o["f"] + 0.1 * g.standard_normal(dim).astype(np.float32))
                boxes.append([o["xy"][0], o["xy"][1], o["xy"][0] + 14, o["xy"][1] + 8])
        for o in brief:
            if o["left"] > 0 and not empty:
                o["left"] -= 1
                feats.append(o["f"] + 0.1 * g.standard_normal(dim).astype(np.float32))
                boxes.append([o["xy"][0], o["xy"][1], o["xy"][0] + 14, o["xy"][1] + 8])
        n = len(feats)
        x0 = g.uniform(0, 100, (n, 1)).astype(np.float32)
        y0 = g.uniform(0, 70, (n, 1)).astype(np.float32)
        xs = x0 + np.linspace(0, 1, 25, dtype=np.float32)[None, :] * g.uniform(8, 28, (n, 1)).astype(np.float32)
        wob = g.uniform(-1, 1, (n, 25)).astype(np.float32)
        bd = np.stack([xs, y0 + wob, xs, y0 + wob + g.uniform(6, 20, (n, 1)).astype(np.float32)], -1).astype(np.float32)
        recs = g.integers(0, 37, (n, 25)).astype(np.int64)
        recs[g.random((n, 25)) < 0.3] = 36
        out.append((np.asarray(feats, np.float32).reshape(n, dim), np.asarray(boxes, np.float32).reshape(n, 4), bd, recs,
                    g.uniform(0.3, 1, n).astype(np.float32)))
    return out


def _instances(trace):
    from gomatching_amd.structures import Instances, Boxes
    dets = []
    for f, b, bd, recs, sc in trace:
        inst = Instances(NET_HW)
        inst.reid_features = torch.from_numpy(f).to(DEV)
        inst.pred_boxes = Boxes(torch.from_numpy(b).to(DEV))
        inst.scores = torch.from_numpy(sc).to(DEV)
        inst.bd = torch.from_numpy(bd).to(DEV)
        inst.recs = torch.from_numpy(recs).to(DEV)
        dets.append(inst)
    return dets


def _stub(model, dets):
    it = iter(dets)
    model.detect_launch = lambda batched_inputs, time_cost: list(batched_inputs)       # detection stubbed out, as in
    model.detect_finish = lambda h, time_cost: [next(it) for _ in h]                    # test_model_gpu's tracker tests


def _gap_and_removed(ids_before, ids_after):
    """-> (ids removed as short, kept ids that are missing from two or more consecutive frames between two sightings)."""
    before, after = set(np.concatenate(ids_before).tolist()), set(np.concatenate(ids_after).tolist())
    seen, revived = {}, set()
    for t, ids in enumerate(ids_after):
        for i in ids.tolist():
            if i in seen and t - seen[i] >= 3:
                revived.add(i)
            seen[i] = t
    return before - after, revived


def _stub_case(builtin):
    """Model, trace and the offline rows of one config, computed once and left unchanged."""
    if builtin not in _built:
        from gomatching_amd import results
        from gomatching_amd.modeling import GoMatching
        from gomatching_amd.predictor import TextDecoder
        from gomatching_amd.weights import synth_state_dict
        cfg = mini_cfg(builtin, device=DEV)
        model = GoMatching(cfg, synth_state_dict(cfg, seed=7), device=DEV)
        dec = TextDecoder(cfg.MODEL.TRANSFORMER.VOC_SIZE, cfg.MODEL.TRANSFORMER.CUSTOM_DICT)
        assert dec.voc_size == 37
        trace = _trace(130, model.roi_heads.feature_dim, seed=5)
        _stub(model, _instances(trace))
        insts, id_count = model.batch_inference([{} for _ in range(100)], 0, 0, [], _time_cost())
        insts, id_count = model.batch_inference([{} for _ in range(30)], 1, id_count, insts, _time_cost())
        ids_before = [model._host(x)["ids"].copy() for x in insts]
        if model.min_track_len > 0:
            insts = model._remove_short_track(insts)
        ids_after = [model._host(x)["ids"].copy() for x in insts]
        res = model.batch_postprocess(insts, [SRC_HW] * len(insts))
        rows = results.clip_lines(res, dec)
        _built[builtin] = (cfg, model, dec, trace, rows, ids_before, ids_after, int(id_count))
    return _built[builtin]


@pytest.mark.parametrize("builtin", ["icdar15", "pp_dstext"])
def test_offline_result_of_the_trace_has_short_and_revived_tracks(builtin):
    cfg, model, dec, trace, rows, ids_before, ids_after, _ = _stub_case(builtin)
    removed, revived = _gap_and_removed(ids_before, ids_after)
    print("%s: tracks %d, removed as short %d, kept across a gap of >= 2 frames %d, rows %d, empty frames %d" % (
        builtin, len(set(np.concatenate(ids_before).tolist())), len(removed), len(revived), sum(len(r) for r in rows),
        sum(1 for t in trace if len(t[0]) == 0)))
    assert len(removed) >= 1 and len(revived) >= 1
    assert sum(len(r) for r in rows) > 300 and any(len(t[0]) == 0 for t in trace)
    assert any(r[9] for fr in rows for r in fr)                        # texts are not all empty


@pytest.mark.parametrize("fps", [1, 3, 8])
@pytest.mark.parametrize("builtin", ["icdar15", "pp_dstext"])
def test_online_rows_equal_offline_rows_on_a_stubbed_trace(builtin, fps):
    from gomatching_amd.online import OnlineSpotter
    cfg, model, dec, trace, want, _, _, want_count = _stub_case(builtin)
    old = model.frames_per_step
    model.frames_per_step = fps
    try:
        _stub(model, _instances(trace))
        s = OnlineSpotter(cfg, model, dec)
        L, M = model.test_len, model.min_track_len
        D, R = max(M - 1, 0) * max(L - 1, 1), max(L - 1, 1)
        assert s.latency_bound == D and s.cap_frames == D + R + 2 * fps
        assert tuple(s.ring_bd.shape) == (s.cap_frames * cfg.MODEL.TRANSFORMER.NUM_QUERIES, 25, 4)
        ring_ptrs = (s.ring_bd.data_ptr(), s.ring_recs.data_ptr())
        live_seen = []
        on_step = s._on_step

        def counting(dets, first):                                    # the list as the tracker leaves it, then as the session does
            on_step(dets, first)
            live_seen.append(sum(x is not None for x in s.instances))
        s._on_step = counting
        got, worst, fed = [], 0, 0
        assert sum(PUSHES) == 130
        for n in PUSHES:
            out = s.push_inputs([{"height": SRC_HW[0], "width": SRC_HW[1]} for _ in range(n)])
            fed += n
            tracked = fed // fps * fps                                # whole steps only
            for f, _ in out:
                worst = max(worst, tracked - 1 - f)                  # as the caller sees it: the push's own frames included
            got.extend(out)
            assert s.frames_seen == fed and s.pending == fed - len(got)
            assert len(got) >= tracked - D                            # whatever was tracked D frames ago has left
        launches_before_close = s.gather_launches
        got.extend(s.close())
        assert s.close() == [] and s.pending == 0
        assert [f for f, _ in got] == list(range(130))
        for f, rows in got:
            assert rows == want[f], "frame %d: online rows differ from offline rows" % f
        assert int(s.id_count) == want_count
        print("%s fps %d: largest wait %d (settler %d, bound %d), live instances peak %d (limit %d), ring high water %d of %d, "
              "gather launches %d for %d pushes" % (builtin, fps, worst, s.max_wait, D, max(live_seen), D + R + 2 * fps,
                                                    s.ring_high_water, s.cap_frames, s.gather_launches, len(PUSHES)))
        assert s.max_wait <= s.latency_bound and worst <= s.latency_bound + max(PUSHES) - 1
        if M > 1:
            assert s.max_wait > 0 and s.settler.rows_dropped > 0
        assert max(live_seen) <= D + R + 2 * fps and s.max_live_instances <= D + R + 2 * fps
        assert s.ring_high_water <= s.cap_frames                      # (an overflow raises)
        assert launches_before_close <= len(PUSHES)                   # one launch per push at most: these pushes fit the ring
        assert (s.ring_bd.data_ptr(), s.ring_recs.data_ptr()) == ring_ptrs
    finally:
        model.frames_per_step = old


# ------------------------------------------------------------------------------------------------ (b) the real detector
OPTS = ["MODEL.TRANSFORMER.NUM_QUERIES", "100", "INPUT.MIN_SIZE_TEST", "320", "INPUT.MAX_SIZE_TEST", "480",
        "MODEL.DEVICE", DEV]
SPLICE = (8, 3, 13)                                                  # frames of clip A, of clip B, of clip A again
CLIP_A, CLIP_B = 3, 11


def _spliced_clip():
    from gomatching_amd.synth import make_clip
    a = make_clip(SPLICE[0] + SPLICE[2], 320, 480, clip_id=CLIP_A)
    b = make_clip(SPLICE[1], 320, 480, clip_id=CLIP_B)
    frames = list(a[:SPLICE[0]]) + list(b) + list(a[SPLICE[0]:])
    return [np.ascontiguousarray(f[:, :, ::-1]) for f in frames]        # BGR, as eval.read_frame yields


def _real_case(tmp_path_factory):
    if "real" not in _built:
        from gomatching_amd.config import setup_cfg
        from gomatching_amd.modeling import GoMatching
        from gomatching_amd.predictor import TextDecoder
        from gomatching_amd.weights import synth_state_dict
        weights = str(tmp_path_factory.mktemp("online_weights") / "weights.pth")
        cfg = setup_cfg(builtin="icdar15", opts=OPTS + ["MODEL.WEIGHTS", weights])
        sd = synth_state_dict(cfg, seed=7, cls_bias={"detection_transformer.ctrl_point_class.0.bias": 0.5})
        torch.save(sd, weights)
        model = GoMatching(cfg, sd, device=DEV, frames_per_step=8)
        dec = TextDecoder(cfg.MODEL.TRANSFORMER.VOC_SIZE, cfg.MODEL.TRANSFORMER.CUSTOM_DICT)
        _built["real"] = (cfg, model, dec, weights, _spliced_clip())
    return _built["real"]


def test_online_rows_equal_spot_video_rows_with_the_real_detector(tmp_path_factory):
    from gomatching_amd import results
    from gomatching_amd.online import OnlineSpotter
    from gomatching_amd.predictor import GoMBatchPredictor
    cfg, model, dec, _, frames = _real_case(tmp_path_factory)
    assert len(frames) == 24
    spotter = GoMBatchPredictor(cfg, model, device_ingest=True)
    # ids before removal: the same tracking, without the last batch's post-processing
    inputs, hw = spotter.prepare_device(frames)
    raw, _ = spotter.run_prepared(inputs, hw, [], 0, 0, False, _time_cost())
    ids_before = [model._host(x)["ids"].copy() for x in raw]
    preds, _ = results.spot_video(spotter, frames, _time_cost())
    ids_after = [model._host(r["instances"])["ids"].copy() for r in preds]
    want = results.clip_lines(preds, dec)
    removed, revived = _gap_and_removed(ids_before, ids_after)
    print("real detector: instances %d, tracks %d, removed as short %d, kept across a gap of >= 2 frames %d, rows %d" % (
        sum(len(i) for i in ids_before), len(set(np.concatenate(ids_before).tolist())), len(removed), len(revived),
        sum(len(r) for r in want)))
    assert len(removed) >= 1 and len(revived) >= 1
    s = OnlineSpotter(cfg, model, dec, device_ingest=True)
    got = []
    for a, b in ((0, 8), (8, 11), (11, 24)):                          # one step, a part of a step, the rest
        got.extend(s.push(frames[a:b]))
    got.extend(s.close())
    assert [f for f, _ in got] == list(range(24))
    for f, rows in got:
        assert rows == want[f], "frame %d" % f
    assert sum(len(r) for _, r in got) > 0 and s.max_wait <= s.latency_bound


def _files(out_dir):
    found = {}
    for sub in ("preds", "jsons"):
        for f in sorted(os.listdir(os.path.join(out_dir, sub))):
            with open(os.path.join(out_dir, sub, f), "rb") as fp:
                found[sub + "/" + f] = fp.read()
    return found


def test_eval_online_writes_the_files_of_a_plain_run(tmp_path, tmp_path_factory):
    from gomatching_amd import eval as E
    cfg, model, dec, weights, frames = _real_case(tmp_path_factory)
    data = tmp_path / "ICDAR15_frames" / "Video_7_1_1"
    data.mkdir(parents=True)
    for i, bgr in enumerate(frames):
        Image.fromarray(np.ascontiguousarray(bgr[:, :, ::-1])).save(str(data / ("%d.png" % (i + 1))))
    base = ["--builtin", "icdar15", "--input", str(tmp_path / "ICDAR15_frames")]
    opts = ["--opts"] + OPTS + ["MODEL.WEIGHTS", weights]
    outs = {}
    for name, extra in (("plain", []), ("online", ["--online", "--push", "8"])):
        outs[name] = str(tmp_path / name)
        r = subprocess.run([sys.executable, "-m", "gomatching_amd.eval"] + base + ["--output", outs[name]] + extra + opts,
                           cwd=ROOT, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, "%s: exit status %d\n%s\n%s" % (name, r.returncode, r.stdout[-2000:], r.stderr[-4000:])
        assert r.stdout.count("processing ") == 1 and "total_time" in r.stdout
        if name == "online":
            assert "online: largest wait" in r.stdout
    plain, online = _files(outs["plain"]), _files(outs["online"])
    assert sorted(plain) == sorted(online) == ["jsons/Video_7_1_1.json", "preds/res_video_7.txt", "preds/res_video_7.xml"]
    for f in plain:
        assert plain[f] == online[f], "eval --online and plain eval differ in %s" % f
    assert b"<object" in plain["preds/res_video_7.xml"]               # not a comparison of empty files
    assert not os.path.exists(os.path.join(outs["online"], ".partial"))
    # flags that do not go with --online: status 2 before anything is built (in-process: no model, no GPU work)
    for bad in (["--online", "--show"], ["--online", "--host-rows"]):
        assert E.main(base + ["--output", str(tmp_path / "refused")] + bad + opts) == 2
    assert not os.path.exists(str(tmp_path / "refused"))
