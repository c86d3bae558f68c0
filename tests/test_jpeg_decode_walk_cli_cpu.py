"""CPU: the choice of the JPEG decoder's entropy walk -- `eval --decode-walk` as a dependent flag, `jpeg.decode_device`'s
argument check, and `jpeg.resolve_walk`, the pure function behind walk="auto"."""
import subprocess
import sys

import numpy as np
import pytest

import jpeg_decode_families as fam

from gomatching_amd import jpeg


def test_decode_walk_needs_device_decode(tmp_path):
    (tmp_path / "in").mkdir()
    r = subprocess.run([sys.executable, "-m", "gomatching_amd.eval", "--builtin", "icdar15", "--input", str(tmp_path / "in"),
                        "--output", str(tmp_path / "out"), "--decode-walk", "chunks"], capture_output=True, text=True)
    assert r.returncode == 2 and "--decode-walk goes with --device-decode" in r.stderr
    assert not (tmp_path / "out").exists()


def test_eval_parser_takes_the_three_walks():
    from gomatching_amd import eval as E
    base = ["--builtin", "icdar15", "--input", "in", "--output", "out", "--device-decode"]
    assert E.get_parser().parse_args(base).decode_walk is None                   # (main makes it "auto")
    for walk in ("auto", "segments", "chunks"):
        assert E.get_parser().parse_args(base + ["--decode-walk", walk]).decode_walk == walk
    with pytest.raises(SystemExit):
        E.get_parser().parse_args(base + ["--decode-walk", "bogus"])


def test_an_unknown_walk_is_a_value_error():
    files = dict(fam.families())["own-70x37"]
    with pytest.raises(ValueError, match="bogus"):
        jpeg.decode_device(files, walk="bogus")                                  # before the GPU is asked for
    with pytest.raises(ValueError, match="bogus"):
        jpeg.resolve_walk("bogus", jpeg.plan(files))
    with pytest.raises(ValueError, match="chunk_bytes"):
        jpeg.decode_device(files, walk="segments", chunk_bytes=64)               # as ops.jpeg_decode: not dropped in silence


def test_auto_resolves_by_the_mean_segment_length():
    own = jpeg.plan(dict(fam.families())["own-70x37"])                           # a restart interval per MCU row: short segments
    assert own.desc.shape[0] > 1 and jpeg.resolve_walk("auto", own) == "segments"
    big = jpeg.plan((fam.pillow_file(fam.content("noise", 320, 240, 21), 2, 95),))
    assert big.desc.shape[0] == 1 and len(big.data) == 89997 > jpeg.AUTO_SEGMENT_BYTES
    assert jpeg.resolve_walk("auto", big) == "chunks"
    for walk in ("segments", "chunks"):
        assert jpeg.resolve_walk(walk, own) == walk and jpeg.resolve_walk(walk, big) == walk
    # the threshold itself: a plan whose one segment is exactly that long, and one byte shorter
    edge = jpeg.plan(dict(fam.families())["size-16x16-2"])
    edge.desc = np.array([[0, jpeg.AUTO_SEGMENT_BYTES, jpeg.AUTO_SEGMENT_BYTES, 0, 1, 0, 0, 0]], dtype=np.int64)
    assert jpeg.resolve_walk("auto", edge) == "chunks"
    edge.desc[0, 1] -= 1
    assert jpeg.resolve_walk("auto", edge) == "segments"
    assert jpeg.CHUNK_BYTES in (64, 128, 256, 512, 1024) and jpeg.AUTO_SEGMENT_BYTES > jpeg.CHUNK_BYTES
