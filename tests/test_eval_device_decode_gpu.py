"""GPU: `python -m gomatching_amd.eval --device-decode` on a tiny synthetic tree of JPEG frames: preds/ and jsons/ byte-identical
to a run without the flag, offline and with `--online --push 8`; a .png frame and a progressive .jpg among the frames take the
per-file Pillow route (the run prints the counts); `--device-decode --host-ingest` ends with status 2 before anything is built."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch
from PIL import Image

from test_eval_cli_gpu import OPTS, ROOT, _files, _run

pytestmark = pytest.mark.gpu
VIDEOS = {"Video_5_1_2": (7, 3), "Video_17_3_1": (19, 4)}               # name -> (frames, clip id)


def _routes(log):
    m = re.search(r"device decode:\s+(\d+)\s+files decoded on the GPU; through Pillow:\s+(\d+)\s+with another extension,\s+(\d+)\s+"
                  r"refused by the parser,\s+(\d+)\s+with a status word set", log)
    assert m, log[-2000:]
    return tuple(int(v) for v in m.groups())


def test_device_decode_writes_the_same_files(tmp_path):
    from gomatching_amd import eval as E
    from gomatching_amd import jpeg
    from gomatching_amd.config import setup_cfg
    from gomatching_amd.synth import make_clip
    from gomatching_amd.weights import synth_state_dict
    data = tmp_path / "ICDAR15_frames"
    for name, (count, clip_id) in VIDEOS.items():
        (data / name).mkdir(parents=True)
        for i, rgb in enumerate(make_clip(count, 72, 128, clip_id=clip_id)):
            im = Image.fromarray(np.ascontiguousarray(rgb))
            if name == "Video_17_3_1" and i == 4:
                im.save(str(data / name / "5.png"))
            elif name == "Video_17_3_1" and i == 9:
                im.save(str(data / name / "10.jpg"), quality=90, progressive=True)
            else:
                im.save(str(data / name / ("%d.jpg" % (i + 1))), quality=90)
    sample = open(str(data / "Video_5_1_2" / "1.jpg"), "rb").read()
    info = jpeg.parse(sample)
    assert (info.H, info.W, info.hs, info.vs) == (72, 128, 2, 2)                 # 4:2:0, 4.5 MCU rows
    assert isinstance(jpeg.parse(open(str(data / "Video_17_3_1" / "10.jpg"), "rb").read()), jpeg.Refusal)
    frames = E.decode_frames([str(data / "Video_5_1_2" / "1.jpg")], [sample], {k: 0 for k in E.DECODE_ROUTES}, torch.device("cuda:0"))
    assert np.array_equal(frames[0].cpu().numpy(), E.read_frame(str(data / "Video_5_1_2" / "1.jpg")))

    weights = str(tmp_path / "weights.pth")
    cfg = setup_cfg(builtin="icdar15", opts=OPTS + ["MODEL.WEIGHTS", weights])
    torch.save(synth_state_dict(cfg, seed=7, cls_bias={"detection_transformer.ctrl_point_class.0.bias": 0.5}), weights)
    base = ["--builtin", "icdar15", "--input", str(data)]
    opts = ["--opts"] + OPTS + ["MODEL.WEIGHTS", weights]

    r = subprocess.run([sys.executable, "-m", "gomatching_amd.eval"] + base + ["--output", str(tmp_path / "no"), "--device-decode",
                                                                               "--host-ingest"] + opts,
                       cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 2 and "--host-ingest" in r.stderr and not os.path.exists(str(tmp_path / "no"))

    out_plain, out_dev, out_online = str(tmp_path / "plain"), str(tmp_path / "dev"), str(tmp_path / "online")
    log = _run(base + ["--output", out_plain] + opts)
    assert "device decode" not in log
    assert _routes(_run(base + ["--output", out_dev, "--device-decode"] + opts)) == (24, 1, 1, 0)
    assert _routes(_run(base + ["--output", out_online, "--device-decode", "--online", "--push", "8"] + opts)) == (24, 1, 1, 0)
    plain, dev, online = _files(out_plain), _files(out_dev), _files(out_online)
    assert sorted(plain) == sorted(dev) == sorted(online) and len(plain) == 6
    for f in plain:
        assert dev[f] == plain[f], "--device-decode changed %s" % f
        assert online[f] == plain[f], "--device-decode --online changed %s" % f
    import xml.etree.ElementTree as ET
    assert sum(len(fr) for fr in ET.fromstring(plain["preds/res_video_17.xml"])) >= 1      # not a comparison of empty output
