"""`python -m gomatching_amd.eval --show` and `python -m gomatching_amd.show` end to end on the GPU: the small ICDAR15-named
PNG tree of test_eval_cli_gpu.py (one video crosses the 100-frame chunk) with synthetic weights; every command is a fresh
child process, one at a time.  --show must write a picture per frame, leave the XML / JSON / TXT files byte-identical to a
run without it, and the pictures must be `show.draw_clip(host=True)` of the written json's rows; the stand-alone command, on
the GPU and with --host-draw, must write the same pixels again."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from PIL import Image

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPTS = ["MODEL.TRANSFORMER.NUM_QUERIES", "12", "INPUT.MIN_SIZE_TEST", "128", "INPUT.MAX_SIZE_TEST", "256",
        "MODEL.DEVICE", "cuda:0"]
VIDEOS = {"Video_5_1_2": (7, 3), "Video_17_3_1": (103, 4)}              # name -> (frames, clip id)


def _run(module, args):
    """One child at a time, no retry; a non-zero status fails the test."""
    r = subprocess.run([sys.executable, "-m", module] + args, cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, "exit status %d\n%s\n%s" % (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    return r.stdout


def _files(out_dir):
    found = {}
    for sub in ("preds", "jsons"):
        for f in sorted(os.listdir(os.path.join(out_dir, sub))):
            with open(os.path.join(out_dir, sub, f), "rb") as fp:
                found[sub + "/" + f] = fp.read()
    return found


def _pictures(out_dir):
    """{video/file: BGR pixels} of results/."""
    from gomatching_amd import eval as E
    found = {}
    for video in sorted(os.listdir(os.path.join(out_dir, "results"))):
        for f in os.listdir(os.path.join(out_dir, "results", video)):
            found[video + "/" + f] = E.read_frame(os.path.join(out_dir, "results", video, f))
    return found


def test_show_draws_every_frame_and_changes_no_result_file(tmp_path):
    from gomatching_amd import show
    from gomatching_amd.config import setup_cfg
    from gomatching_amd.synth import make_clip
    from gomatching_amd.weights import synth_state_dict
    data = tmp_path / "ICDAR15_frames"
    clips = {}
    for name, (count, clip_id) in VIDEOS.items():
        (data / name).mkdir(parents=True)
        clips[name] = [np.ascontiguousarray(f[:, :, ::-1]) for f in make_clip(count, 72, 128, clip_id=clip_id)]   # BGR
        for i, bgr in enumerate(clips[name]):
            Image.fromarray(np.ascontiguousarray(bgr[:, :, ::-1])).save(str(data / name / ("%d.png" % (i + 1))))
    weights = str(tmp_path / "weights.pth")
    cfg = setup_cfg(builtin="icdar15", opts=OPTS + ["MODEL.WEIGHTS", weights])
    torch.save(synth_state_dict(cfg, seed=7, cls_bias={"detection_transformer.ctrl_point_class.0.bias": 0.5}), weights)
    base = ["--builtin", "icdar15", "--input", str(data)]
    opts = ["--opts"] + OPTS + ["MODEL.WEIGHTS", weights]

    out_show, out_plain = str(tmp_path / "out_show"), str(tmp_path / "out_plain")
    _run("gomatching_amd.eval", base + ["--output", out_show, "--show"] + opts)
    _run("gomatching_amd.eval", base + ["--output", out_plain] + opts)
    shown, plain = _files(out_show), _files(out_plain)
    assert sorted(shown) == sorted(plain) and len(shown) == 6
    for f in shown:
        assert shown[f] == plain[f], "--show changed %s" % f
    assert not os.path.exists(os.path.join(out_plain, "results"))

    # a picture per frame, equal to the host path applied to the written json's rows
    pics = _pictures(out_show)
    assert sorted(pics) == sorted("%s/%d.png" % (n, i + 1) for n, (c, _) in VIDEOS.items() for i in range(c))
    voc = cfg.MODEL.TRANSFORMER.VOC_SIZE
    changed = 0
    for name, (count, _) in VIDEOS.items():
        annotation = show.rows_of_json(json.loads(shown["jsons/%s.json" % name].decode("utf-8")))
        rows = [annotation[str(i + 1)] for i in range(count)]
        want = np.concatenate([show.draw_clip(clips[name][f0:f0 + 100], rows[f0:f0 + 100], voc, host=True)
                               for f0 in range(0, count, 100)])
        for i in range(count):
            assert np.array_equal(pics["%s/%d.png" % (name, i + 1)], want[i]), (name, i)
            changed += int((want[i] != clips[name][i]).any())
    assert changed >= 1                                                   # not a comparison of untouched frames

    # the stand-alone command on that output, on the GPU and on the host: the same pixels again
    for extra in ([], ["--host-draw"]):
        again = str(tmp_path / ("again" + "_".join(extra)))
        _run("gomatching_amd.show", ["--input", str(data), "--results", out_show, "--output", again, "--builtin", "icdar15"] + extra)
        redone = _pictures(again)
        assert sorted(redone) == sorted(pics)
        for f in pics:
            assert np.array_equal(redone[f], pics[f]), (extra, f)
