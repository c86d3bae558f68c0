"""GPU: `python -m gomatching_amd.show --device-read` writes the bytes `show` writes without the flag -- plain, with
--device-decode --device-encode, and on a results directory where one video's json is an indent=2 dump, which the parser refuses
and json.load reads -- and keeps the exit statuses of the errors."""
import json
import os
import random

import numpy as np
import pytest
from PIL import Image

import result_parse_cases as rc

pytestmark = pytest.mark.gpu
VIDEOS = ("Video_7_1_1", "Video_8_1_1")


def _annotation(seed, frames=5):
    """Rows from the parser's cases: transcriptions with escapes and Chinese, contours of 0, 1, 2 and 50 points, polygons across
    the edges of a 64 x 48 frame, an empty frame."""
    rng = random.Random(seed)
    a = {}
    for f in range(frames):
        a[str(f + 1)] = [] if f == 2 else [
            rc.obj(rng, n, rng.randint(-3, 600), rc.TEXTS[rng.randrange(len(rc.TEXTS))], -10, 70)
            for n in (50, rng.choice((0, 1, 2)), rng.randint(3, 9))]
    return a


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    root = tmp_path_factory.mktemp("device_read")
    rng = np.random.RandomState(5)
    for v in VIDEOS:
        d = root / "ICDAR15_frames" / v
        d.mkdir(parents=True)
        for i in range(5):
            Image.fromarray(rng.randint(0, 256, (48, 64, 3)).astype(np.uint8)).save(str(d / ("%d.jpg" % (i + 1))), quality=90)
    return root, str(root / "ICDAR15_frames")


def _results(root, name, texts):
    out = root / name / "jsons"
    out.mkdir(parents=True)
    for v, t in zip(VIDEOS, texts):
        (out / (v + ".json")).write_bytes(t)
    return str(root / name)


def _files(directory):
    got = {}
    for base, _, names in os.walk(os.path.join(directory, "results")):
        for n in names:
            with open(os.path.join(base, n), "rb") as fp:
                got[os.path.relpath(os.path.join(base, n), directory)] = fp.read()
    return got


def _same_pictures(root, data, results, flags, tag, capsys):
    from gomatching_amd import show
    a, b = str(root / (tag + "_plain")), str(root / (tag + "_read"))
    assert show.main(["--input", data, "--results", results, "--output", a] + flags) == 0
    capsys.readouterr()
    assert show.main(["--input", data, "--results", results, "--output", b, "--device-read"] + flags) == 0
    out = capsys.readouterr().out
    fa, fb = _files(a), _files(b)
    assert len(fa) == 5 * len(VIDEOS) and sorted(fa) == sorted(fb)
    for k in fa:
        assert fa[k] == fb[k], k
    return out


def test_device_read_writes_the_same_pictures(tree, capsys):
    root, data = tree
    results = _results(root, "canonical", [rc.dumps(_annotation(1)), rc.dumps(_annotation(2))])
    out = _same_pictures(root, data, results, [], "plain", capsys)
    assert "result files: 2 read on the GPU, 0 through json.load" in out
    out = _same_pictures(root, data, results, ["--device-decode", "--device-encode"], "resident", capsys)
    assert "result files: 2 read on the GPU, 0 through json.load" in out


def test_a_refused_file_goes_through_json_load(tree, capsys):
    root, data = tree
    results = _results(root, "mixed", [rc.dumps(_annotation(1)), rc.dumps(_annotation(2), indent=2)])
    out = _same_pictures(root, data, results, [], "mixed", capsys)
    assert "result files: 1 read on the GPU, 1 through json.load (refused by the parser -- " in out


def test_exit_statuses(tree, capsys):
    from gomatching_amd import show
    root, data = tree
    good = rc.dumps(_annotation(1))
    drawn = str(root / "never")
    base = ["--input", data, "--output", drawn, "--device-read"]
    assert show.main(base + ["--results", _results(root, "s0", [good, good]), "--host-draw"]) == 2
    assert "--host-draw" in capsys.readouterr().err
    assert not os.path.exists(drawn)
    assert show.main(base + ["--results", _results(root, "s1", [rc.dumps(_annotation(1, frames=4)), good])]) == 2
    assert "video Video_7_1_1: 5 frames but results for 4" in capsys.readouterr().err
    bare = _annotation(3)
    del bare["2"][0]["segmentation"]
    assert show.main(base + ["--results", _results(root, "s2", [good, rc.dumps(bare)])]) == 2
    assert "video Video_8_1_1: result rows without a segmentation cannot be drawn" in capsys.readouterr().err
    os.remove(os.path.join(str(root / "s2"), "jsons", VIDEOS[1] + ".json"))
    assert show.main(base + ["--results", str(root / "s2")]) == 2
    err = capsys.readouterr().err
    assert "video Video_8_1_1: result file" in err and "not found" in err
