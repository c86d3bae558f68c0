"""GPU: `python -m gomatching_amd.eval --device-write --device-vote --lexicon L --device-lexicon` on the tiny synthetic tree of
tests/test_eval_device_write_gpu.py.  The lexicon and its pair list are made from a plain run's own transcriptions (a third of
the distinct strings verbatim with a display form that differs, a third with one edit, a third left out); the reference is the
host step, `lexicon.correct_results(host=True)`, on the plain run's files, and it must have changed, unaccepted and dropped
rows.  OUT/lexicon/** is byte-equal to the reference and OUT/{jsons,preds}/** to the plain run, offline, with `--online --push 8`
and with per-video lexicons and `--lexicon-unmatched drop`; no .partial directory is left in either root; the log counts
three videos corrected on the GPU and none by the host; a resumed run restores what was deleted, one video on the GPU and the
others by the host; the flag without its three companions ends with status 2 and creates nothing."""
import json
import os
import shutil
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
    line = [l for l in log.splitlines() if l.startswith("device lexicon:")]
    assert len(line) == 1, log[-2000:]
    words = line[0].split()
    return int(words[2]), int(words[words.index("by") - 1])


def _one_edit(word, k):
    """`word` at edit distance 1: a substitution, a deletion or an insertion, by turns."""
    kind = (k // 3) % 3
    if kind == 0:
        return ("z" if word[0] != "z" else "y") + word[1:]
    return word[1:] if kind == 1 and len(word) > 1 else word[:1] + "q" + word[1:]


def _all_files(out_dir):
    found = _files(out_dir)
    found.update({"lexicon/" + k: v for k, v in _files(os.path.join(out_dir, "lexicon")).items()})
    return found


def test_device_lexicon_writes_the_host_steps_files(tmp_path):
    from gomatching_amd import lexicon
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
    flags = ["--device-write", "--device-vote", "--device-lexicon"]

    # ---- the flag without its three companions: status 2, nothing created
    lex_file, pair_file, lex_dir = str(tmp_path / "lexicon.txt"), str(tmp_path / "pairs.txt"), tmp_path / "lexicons"
    open(lex_file, "w").write("word\n")
    for args in (flags, ["--device-write", "--device-lexicon", "--lexicon", lex_file], ["--device-lexicon", "--lexicon", lex_file]):
        r = subprocess.run([sys.executable, "-m", "gomatching_amd.eval"] + base + ["--output", str(tmp_path / "no")] + args + opts,
                           cwd=ROOT, capture_output=True, text=True, timeout=300)
        assert r.returncode == 2 and "--device-lexicon" in r.stderr and not os.path.exists(str(tmp_path / "no")), r.stderr[-2000:]

    # ---- a plain run, and a lexicon made of its own transcriptions
    out_plain = str(tmp_path / "plain")
    _run(base + ["--output", out_plain] + opts)
    plain = _files(out_plain)
    texts = sorted({row["transcription"] for name in VIDEOS for rows in json.loads(plain["jsons/%s.json" % name]).values()
                    for row in rows if row["transcription"].strip()})
    assert len(texts) >= 3, texts
    words = [t for k, t in enumerate(texts) if k % 3 == 0] + [_one_edit(t, k) for k, t in enumerate(texts) if k % 3 == 1]
    with open(lex_file, "w", encoding="utf-8") as f:
        f.write("".join(w + "\n" for w in words))
    with open(pair_file, "w", encoding="utf-8") as f:
        f.write("".join("%s <%s> & co\n" % (w.upper(), w.capitalize()) for w in words))
    lex_dir.mkdir()
    for name in VIDEOS:
        shutil.copy(lex_file, str(lex_dir / (name + ".txt")))
        shutil.copy(pair_file, str(lex_dir / (name + ".pairs.txt")))

    # ---- the reference: the host step on the plain run's files; it must have something to compare
    ref_keep, ref_drop = str(tmp_path / "ref_keep"), str(tmp_path / "ref_drop")
    figures = lexicon.correct_results(out_plain, ref_keep, lex_file, pair_file, 1, "keep", host=True)
    assert figures["changed"] >= 1 and figures["dropped"] == 0, figures
    figures = lexicon.correct_results(out_plain, ref_drop, str(lex_dir), None, 1, "drop", host=True)
    assert figures["changed"] >= 1 and 1 <= figures["dropped"] < figures["rows"], figures     # unaccepted rows, and accepted ones
    want_keep = dict(plain, **{"lexicon/" + k: v for k, v in _files(ref_keep).items()})
    want_drop = dict(plain, **{"lexicon/" + k: v for k, v in _files(ref_drop).items()})
    assert len(want_keep) == len(want_drop) == 18 and want_keep != want_drop

    # ---- the device path: offline, online, per-video lexicons with drop
    out_dev, out_online, out_drop = str(tmp_path / "dev"), str(tmp_path / "online"), str(tmp_path / "drop")
    lex = ["--lexicon", lex_file, "--lexicon-pairs", pair_file]
    assert _counts(_run(base + ["--output", out_dev] + flags + lex + opts)) == (3, 0)
    assert _counts(_run(base + ["--output", out_online] + flags + lex + ["--online", "--push", "8"] + opts)) == (3, 0)
    assert _counts(_run(base + ["--output", out_drop] + flags + ["--lexicon", str(lex_dir), "--lexicon-unmatched", "drop"] + opts)) == (3, 0)
    for out, want in ((out_dev, want_keep), (out_online, want_keep), (out_drop, want_drop)):
        got = _all_files(out)
        assert sorted(got) == sorted(want)
        for f in want:
            assert got[f] == want[f], "%s differs in %s" % (f, out)
        assert not os.path.exists(os.path.join(out, ".partial")) and not os.path.exists(os.path.join(out, "lexicon", ".partial"))

    # ---- a resumed run: video_5 lost its corrected files (the host route), video_17 its original XML and JSON (spotted again: the GPU)
    for f in ("lexicon/jsons/Video_5_1_2.json", "lexicon/preds/res_video_5.xml", "lexicon/preds/res_video_5.txt",
              "preds/res_video_17.xml", "jsons/Video_17_3_1.json"):
        os.remove(os.path.join(out_dev, f))
    with open(os.path.join(out_dev, "lexicon", "preds", "res_video_17.txt"), "wb") as f:
        f.write(b"stale")
    log = _run(base + ["--output", out_dev] + flags + lex + opts)
    assert log.count("processing ") == 1 and _counts(log) == (1, 2)
    assert _all_files(out_dev) == want_keep
    assert not os.path.exists(os.path.join(out_dev, ".partial")) and not os.path.exists(os.path.join(out_dev, "lexicon", ".partial"))


def test_a_display_form_above_the_limit_ends_with_status_2_before_anything_is_built(tmp_path):
    """The command itself: a 176-byte display form (no weights file is even looked for: the check comes first)."""
    data = tmp_path / "ICDAR15_frames" / "Video_5_1_2"
    data.mkdir(parents=True)
    Image.fromarray(np.zeros((72, 128, 3), dtype=np.uint8)).save(str(data / "1.png"))
    lex_file, pair_file = str(tmp_path / "lexicon.txt"), str(tmp_path / "pairs.txt")
    open(lex_file, "w").write("fine\nwide\n")
    open(pair_file, "w").write("FINE Fine\nWIDE %s\n" % ("\\" * 88))
    out = str(tmp_path / "out")
    r = subprocess.run([sys.executable, "-m", "gomatching_amd.eval", "--builtin", "icdar15", "--input", str(tmp_path / "ICDAR15_frames"),
                        "--output", out, "--device-write", "--device-vote", "--device-lexicon", "--lexicon", lex_file,
                        "--lexicon-pairs", pair_file, "--opts", "MODEL.WEIGHTS", str(tmp_path / "none.pth")],
                       cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 2 and not os.path.exists(out), (r.returncode, r.stderr[-2000:])
    errors = [l for l in r.stderr.splitlines() if l.startswith("error: ")]      # (a driver may print lines of its own in front)
    assert len(errors) == 1 and errors[0].startswith("error: lexicon: ") and "Traceback" not in r.stderr
    assert lex_file in r.stderr and "'wide'" in r.stderr and "176 bytes in the JSON file" in r.stderr
