"""`python -m gomatching_amd.eval` end to end on the GPU: two videos of PNG frames (one crosses the 100-frame chunk) and a
weights file in a temporary ICDAR15-named tree; the command runs as a fresh child process, once with its defaults
(device ingest, device rows) and once with --host-rows --host-ingest.  Every XML / JSON / TXT file must be byte-identical
between the two runs and to what the library's host path writes in-process; a second invocation resumes and processes
nothing."""
import os
import subprocess
import sys
import xml.etree.ElementTree as ET

import numpy as np
import pytest
import torch
from PIL import Image

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPTS = ["MODEL.TRANSFORMER.NUM_QUERIES", "12", "INPUT.MIN_SIZE_TEST", "128", "INPUT.MAX_SIZE_TEST", "256",
        "MODEL.DEVICE", "cuda:0"]
VIDEOS = {"Video_5_1_2": (7, 3), "Video_17_3_1": (103, 4)}              # name -> (frames, clip id)


def _run(args):
    """One child at a time, no retry; a non-zero status fails the test."""
    r = subprocess.run([sys.executable, "-m", "gomatching_amd.eval"] + args, cwd=ROOT, capture_output=True, text=True,
                       timeout=900)
    assert r.returncode == 0, "exit status %d\n%s\n%s" % (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    return r.stdout


def _files(out_dir):
    found = {}
    for sub in ("preds", "jsons"):
        for f in sorted(os.listdir(os.path.join(out_dir, sub))):
            with open(os.path.join(out_dir, sub, f), "rb") as fp:
                found[sub + "/" + f] = fp.read()
    return found


def test_command_line_writes_the_library_host_path_files(tmp_path):
    from gomatching_amd import eval as E
    from gomatching_amd import results
    from gomatching_amd.config import setup_cfg
    from gomatching_amd.modeling import GoMatching
    from gomatching_amd.predictor import GoMBatchPredictor, TextDecoder, new_time_cost
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
    sd = synth_state_dict(cfg, seed=7, cls_bias={"detection_transformer.ctrl_point_class.0.bias": 0.5})
    torch.save(sd, weights)
    base = ["--builtin", "icdar15", "--input", str(data)]
    opts = ["--opts"] + OPTS + ["MODEL.WEIGHTS", weights]

    out_dev, out_host, out_lib = str(tmp_path / "out_dev"), str(tmp_path / "out_host"), str(tmp_path / "out_lib")
    log = _run(base + ["--output", out_dev] + opts)
    assert log.count("processing ") == 2 and "per_img_time" in log and "total_time" in log
    _run(base + ["--output", out_host, "--host-rows", "--host-ingest"] + opts)

    # the library's host path in-process: same listing order, one model across the videos, as the command does
    model = GoMatching(cfg, E.load_weights(weights), frames_per_step=8)
    spotter = GoMBatchPredictor(cfg, model, device_ingest=False)
    dec = TextDecoder(cfg.MODEL.TRANSFORMER.VOC_SIZE)
    data_type, videos = E.list_videos(str(data))
    assert data_type == "ICDAR15" and sorted(n for n, _ in videos) == sorted(VIDEOS)
    for name, video_dir in videos:
        frames = [E.read_frame(p) for p in E.frame_paths(video_dir)]
        assert len(frames) == len(clips[name]) and all(np.array_equal(a, b) for a, b in zip(frames, clips[name]))
        preds, _ = results.spot_video(spotter, frames, new_time_cost())
        results.write_video(preds, name, data_type, out_lib, dec)
    results.write_track_transcriptions(os.path.join(out_lib, "preds"))

    dev, host, lib_files = _files(out_dev), _files(out_host), _files(out_lib)
    expected = sorted(["preds/res_video_5.xml", "preds/res_video_5.txt", "preds/res_video_17.xml", "preds/res_video_17.txt",
                       "jsons/Video_5_1_2.json", "jsons/Video_17_3_1.json"])
    assert sorted(dev) == sorted(host) == sorted(lib_files) == expected
    for f in expected:
        assert dev[f] == host[f], "device and host paths of the command differ in %s" % f
        assert dev[f] == lib_files[f], "the command and the library's host path differ in %s" % f
    for stem in ("video_5", "video_17"):                                 # not a comparison of empty output
        root = ET.fromstring(dev["preds/res_%s.xml" % stem])
        assert sum(len(fr) for fr in root) >= 1, stem
    assert os.path.isfile(os.path.join(out_dev, "gom_icdar15.yaml"))    # the config travels with the results

    # resume: both XML files exist, nothing is processed, nothing changes
    log = _run(base + ["--output", out_dev] + opts)
    assert log.count("processing ") == 0
    assert _files(out_dev) == dev
