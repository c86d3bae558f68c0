"""GPU: `python -m gomatching_amd.eval --device-write` on a tiny synthetic tree: preds/*.xml, preds/*.txt and jsons/*.json
byte-identical to a run without the flag, offline and with `--online --push 8` (three pushes for the longest video); a
three-frame video, whose tracks are all shorter than MIN_TRACK_LEN, gives frames without rows beside the frames with rows;
`--device-write --host-rows` ends with status 2 before anything is built."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from PIL import Image

from test_eval_cli_gpu import OPTS, ROOT, _files, _run

pytestmark = pytest.mark.gpu
VIDEOS = {"Video_5_1_2": (7, 3), "Video_9_2_1": (3, 5), "Video_17_3_1": (19, 4)}     # name -> (frames, clip id)


def test_device_write_writes_the_same_files(tmp_path):
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

    r = subprocess.run([sys.executable, "-m", "gomatching_amd.eval"] + base + ["--output", str(tmp_path / "no"), "--device-write",
                                                                               "--host-rows"] + opts,
                       cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 2 and "--host-rows" in r.stderr and not os.path.exists(str(tmp_path / "no"))

    out_plain, out_dev, out_online = str(tmp_path / "plain"), str(tmp_path / "dev"), str(tmp_path / "online")
    _run(base + ["--output", out_plain] + opts)
    log = _run(base + ["--output", out_dev, "--device-write"] + opts)
    assert "building rows and writing files" in log
    log = _run(base + ["--output", out_online, "--device-write", "--online", "--push", "8"] + opts)
    assert "building rows and writing files" in log and "gather launches" in log
    out_show = str(tmp_path / "show")                                           # the row lists are still built, for the drawing
    _run(base + ["--output", out_show, "--device-write", "--show"] + opts)
    assert _files(out_show) == _files(out_plain)
    assert sorted(os.listdir(os.path.join(out_show, "results"))) == sorted(VIDEOS)
    assert len(os.listdir(os.path.join(out_show, "results", "Video_17_3_1"))) == 19
    plain, dev, online = _files(out_plain), _files(out_dev), _files(out_online)
    assert sorted(plain) == sorted(dev) == sorted(online) and len(plain) == 9
    for f in plain:
        assert dev[f] == plain[f], "--device-write changed %s" % f
        assert online[f] == plain[f], "--device-write --online changed %s" % f
    for out in (out_dev, out_online):
        assert not os.path.exists(os.path.join(out, ".partial"))
    rows = {name: [len(v) for v in json.loads(plain["jsons/%s.json" % name]).values()] for name in VIDEOS}
    assert [len(v) for v in rows.values()] == [7, 3, 19]
    assert rows["Video_9_2_1"] == [0, 0, 0] and min(rows["Video_17_3_1"]) >= 1  # frames without rows, and frames with rows
