"""GPU: `python -m gomatching_amd.eval --device-write --device-vote` on the tiny synthetic tree of
tests/test_eval_device_write_gpu.py: all nine files byte-identical to a run without the flags, offline and with
`--online --push 8`; the log counts three txt files voted on the GPU and none by the host; after one txt and another video's
XML and JSON are deleted a resumed run restores them, one video on the GPU and the others' txt by the host route;
`--device-vote` without `--device-write` ends with status 2 before anything is created."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from PIL import Image

from test_eval_cli_gpu import OPTS, ROOT, _files, _run
from test_eval_device_write_gpu import VIDEOS

pytestmark = pytest.mark.gpu


def _counts(log):
    line = [l for l in log.splitlines() if l.startswith("track transcriptions:")]
    assert len(line) == 1, log[-2000:]
    words = line[0].split()
    return int(words[2]), int(words[words.index("GPU,") + 1])


def test_device_vote_writes_the_same_files(tmp_path):
    from gomatching_amd.config import setup_cfg
    from gomatching_amd.synth import make_clip
    from gomatching_amd.weights import synth_state_dict
    data = tmp_path / "ICDAR15_frames"
    for name, (count, clip_id) in VIDEOS.items():
        (data / name).mkdir(parents=True)
        for i, rgb in enumerate(make_clip(count, 72, 128, clip_id=clip_id)):
            Image.fromarray(np.ascontiguousarray(rgb)).save(str(data / name / ("%d.png" % (i + 1))))
    weights = str(tmp_path / "weights.pth")
    cfg = setup_cfg(builtin="icdar15", opts=OPTS + ["MODEL.WEIGHTS", weights])
    torch.save(synth_state_dict(cfg, seed=7, cls_bias={"detection_transformer.ctrl_point_class.0.bias": 0.5}), weights)
    base = ["--builtin", "icdar15", "--input", str(data)]
    opts = ["--opts"] + OPTS + ["MODEL.WEIGHTS", weights]

    r = subprocess.run([sys.executable, "-m", "gomatching_amd.eval"] + base + ["--output", str(tmp_path / "no"), "--device-vote"] + opts,
                       cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 2 and "--device-write" in r.stderr and not os.path.exists(str(tmp_path / "no"))

    out_plain, out_dev, out_online = str(tmp_path / "plain"), str(tmp_path / "dev"), str(tmp_path / "online")
    log = _run(base + ["--output", out_plain] + opts)
    assert "track transcriptions:" not in log
    assert _counts(_run(base + ["--output", out_dev, "--device-write", "--device-vote"] + opts)) == (3, 0)
    assert _counts(_run(base + ["--output", out_online, "--device-write", "--device-vote", "--online", "--push", "8"] + opts)) == (3, 0)
    plain, dev, online = _files(out_plain), _files(out_dev), _files(out_online)
    assert sorted(plain) == sorted(dev) == sorted(online) and len(plain) == 9
    for f in plain:
        assert dev[f] == plain[f], "--device-vote changed %s" % f
        assert online[f] == plain[f], "--device-vote --online changed %s" % f
    assert plain["preds/res_video_17.txt"].count(b"\n") >= 1           # a vote took place: at least one track has a line
    for out in (out_dev, out_online):
        assert not os.path.exists(os.path.join(out, ".partial"))

    # a resumed run: video_5 lost its txt (its XML stays: the host route), video_17 lost its XML and JSON (spotted again: the GPU)
    os.remove(os.path.join(out_dev, "preds", "res_video_5.txt"))
    os.remove(os.path.join(out_dev, "preds", "res_video_17.xml"))
    os.remove(os.path.join(out_dev, "jsons", "Video_17_3_1.json"))
    with open(os.path.join(out_dev, "preds", "res_video_17.txt"), "wb") as f:
        f.write(b"stale")
    log = _run(base + ["--output", out_dev, "--device-write", "--device-vote"] + opts)
    assert log.count("processing ") == 1 and _counts(log) == (1, 2)
    assert _files(out_dev) == plain and not os.path.exists(os.path.join(out_dev, ".partial"))
