"""GPU: pictures drawn from frames that were decoded on the GPU, through the command lines.  A tiny synthetic tree of two videos
(7 and 27 frames of 72 x 128, a .png frame and a progressive .jpg among them, as tests/test_eval_device_decode_gpu.py builds
them) goes through

    (a)  eval --show                                    (b)  eval --show --device-decode
    (c)  eval --online --push 8 --show --device-decode  (a'), (c')  (a) and (c) with --device-encode
    (d)  show --device-decode over (a)'s output, into a fresh directory

results/, preds/ and jsons/ of (a), (b) and (c) are byte-identical, (a') equals (c'), (d)'s pictures are (a)'s; at least one
picture is not its undrawn source frame; (b) and (c) print the drawing's own route line with the Pillow routes counted, and the
spotting line of (b) reads what it reads without --show."""
import os
import re

import numpy as np
import pytest
import torch
from PIL import Image

from test_eval_cli_gpu import OPTS

pytestmark = pytest.mark.gpu
VIDEOS = {"Video_5_1_2": (7, 3), "Video_17_3_1": (27, 4)}               # name -> (frames, clip id)
ROUTES = (32, 1, 1, 0)                                                   # 34 files: one .png, one the parser refuses


def _tree_files(out_dir, subs=("results", "preds", "jsons")):
    found = {}
    for sub in subs:
        for root, _, files in os.walk(os.path.join(out_dir, sub)):
            for f in files:
                path = os.path.join(root, f)
                with open(path, "rb") as fp:
                    found[os.path.relpath(path, out_dir)] = fp.read()
    return found


def _counts(log, head):
    m = re.search(head + r":\s+(\d+)\s+files decoded on the GPU[^;]*; through Pillow:\s+(\d+)\s+with another extension,\s+(\d+)\s+"
                  r"refused by the parser,\s+(\d+)\s+with a status word set", log)
    assert m, log[-2000:]
    return tuple(int(v) for v in m.groups())


def test_pictures_from_frames_decoded_on_the_gpu(tmp_path, capsys):
    from gomatching_amd import eval as E
    from gomatching_amd import show
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
    weights = str(tmp_path / "weights.pth")
    cfg = setup_cfg(builtin="icdar15", opts=OPTS + ["MODEL.WEIGHTS", weights])
    torch.save(synth_state_dict(cfg, seed=7, cls_bias={"detection_transformer.ctrl_point_class.0.bias": 0.5}), weights)
    opts = ["--opts"] + OPTS + ["MODEL.WEIGHTS", weights]

    def run(name, extra):
        out = str(tmp_path / name)
        capsys.readouterr()
        assert E.main(["--builtin", "icdar15", "--input", str(data), "--output", out, "--show"] + extra + opts) == 0
        return out, capsys.readouterr().out

    online = ["--online", "--push", "8", "--device-decode"]
    out_a, log_a = run("a", [])
    out_b, log_b = run("b", ["--device-decode"])
    out_c, log_c = run("c", online)
    out_a2, _ = run("a2", ["--device-encode"])
    out_c2, _ = run("c2", online + ["--device-encode"])

    a, b, c = _tree_files(out_a), _tree_files(out_b), _tree_files(out_c)
    pictures = sorted(f for f in a if f.startswith("results"))
    assert len(pictures) == 34 and len(a) == 34 + 6 and sorted(a) == sorted(b) == sorted(c)
    for f in sorted(a):
        assert b[f] == a[f], "--show --device-decode changed %s" % f
        assert c[f] == a[f], "--online --show --device-decode changed %s" % f
    a2, c2 = _tree_files(out_a2), _tree_files(out_c2)
    assert sorted(a2) == sorted(c2) == sorted(a)
    for f in sorted(a2):
        assert c2[f] == a2[f], "--online --show --device-decode --device-encode changed %s" % f
    assert any(a2[f] != a[f] for f in pictures)                          # (the project's encoder writes other bytes than Pillow's)

    # (d) the show command, from (a)'s result files
    drawn = str(tmp_path / "d")
    capsys.readouterr()
    assert show.main(["--input", str(data), "--results", out_a, "--output", drawn, "--device-decode"]) == 0
    log_d = capsys.readouterr().out
    d = _tree_files(drawn, subs=("results",))
    assert sorted(d) == pictures
    for f in pictures:
        assert d[f] == a[f], "show --device-decode changed %s" % f
    assert show.main(["--input", str(data), "--results", out_a, "--output", str(tmp_path / "d2"), "--device-decode",
                      "--device-encode", "--decode-walk", "chunks"]) == 0
    d2 = _tree_files(str(tmp_path / "d2"), subs=("results",))
    assert all(d2[f] == a2[f] for f in pictures)

    # not a comparison of undrawn files: some picture is not what the writer makes of its source frame
    differs = 0
    for f in pictures:
        src = os.path.join(str(data), os.path.relpath(f, "results"))
        plain = str(tmp_path / ("undrawn" + os.path.splitext(f)[1]))
        show.write_frame(E.read_frame(src), plain)
        with open(plain, "rb") as fp:
            differs += fp.read() != a[f]
    assert differs >= 1

    # the route lines
    assert "device decode" not in log_a and "drawing decode" not in log_a
    assert _counts(log_b, "device decode") == ROUTES                     # the spotting decode alone, as without --show
    assert _counts(log_b, "drawing decode") == ROUTES                    # the second decode, made for drawing, counted apart
    assert _counts(log_c, "device decode") == ROUTES
    assert _counts(log_c, "drawing decode") == ROUTES and "once, for spotting and drawing" in log_c
    assert _counts(log_d, "drawing decode") == ROUTES
