"""GPU: csrc/jpeg.hip against `jpeg.encode_host` byte for byte, offsets included, on the cases of tests/jpeg_statement.py (which
the CPU test holds to the plain-Python statement) and at 48 x 1296, where one restart interval is 486 blocks -- two rounds of
the entropy kernel's 256 lanes; reproducibility; the refusal above the stated width; and `show --device-encode` against
`show --host-encode` on a tiny tree."""
import io
import json
import os

import numpy as np
import pytest
import torch
from PIL import Image

import jpeg_statement as js

from gomatching_amd import jpeg

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _device(frames, quality, bgr):
    from gomatching_amd import ops
    payload, offsets = ops.jpeg_encode(torch.tensor(np.asarray(frames), device=DEV), quality, bgr)
    assert payload.is_cuda and payload.dtype == torch.uint8 and not offsets.is_cuda and offsets.dtype == torch.int64
    return payload.cpu().numpy(), offsets.numpy()


@pytest.mark.parametrize("name", sorted(js.CASES))
def test_kernels_equal_the_host_path(name):
    frames, quality, bgr, want = js.case(name)
    payload, offsets = _device(frames, quality, bgr)
    h_payload, h_offsets = jpeg.encode_host(frames, quality, bgr)
    assert np.array_equal(offsets, h_offsets), (offsets, h_offsets)
    assert np.array_equal(payload, h_payload)
    assert tuple(jpeg.files(payload, offsets, frames.shape[1], frames.shape[2], quality)) == want     # and so the statement


@pytest.mark.parametrize("quality", [95, 100])
def test_wide_interval_equals_the_host_path_and_repeats(quality):
    """48 x 1296: 81 MCUs, 486 blocks per interval; at q = 100 of noise also many words per interval (several rounds of the
    word loop).  Two calls on the same input give the same bytes."""
    frames = np.random.RandomState(21).randint(0, 256, (2, 48, 1296, 3)).astype(np.uint8)
    payload, offsets = _device(frames, quality, True)
    h_payload, h_offsets = jpeg.encode_host(frames, quality, True)
    assert np.array_equal(offsets, h_offsets) and np.array_equal(payload, h_payload)
    again, again_off = _device(frames, quality, True)
    assert np.array_equal(again_off, offsets) and np.array_equal(again, payload)
    im = Image.open(io.BytesIO(jpeg.files(payload, offsets, 48, 1296, quality)[1]))
    im.load()
    assert im.size == (1296, 48)


def test_encode_device_takes_host_arrays_and_resident_tensors():
    frames, quality, bgr, want = js.case("three_frames")
    for src in (frames, torch.tensor(np.asarray(frames), device=DEV)):
        payload, offsets = jpeg.encode_device(src, quality, bgr)
        assert isinstance(payload, np.ndarray) and payload.dtype == np.uint8 and offsets.dtype == np.int64
        assert tuple(jpeg.files(payload, offsets, frames.shape[1], frames.shape[2], quality)) == want


def test_too_wide_is_refused_without_a_launch():
    from gomatching_amd import lib, ops
    frames = torch.zeros((1, 16, ops.JPEG_MAX_WIDTH + 1, 3), dtype=torch.uint8, device=DEV)
    with pytest.raises(lib.GomError, match="GOM_ERR_UNSUPPORTED"):
        ops.jpeg_encode(frames, 95, True)
    ws = torch.zeros((1 << 20,), dtype=torch.uint8, device=DEV)
    off = torch.full((2,), -7, dtype=torch.int64, device=DEV)
    rc = lib.load().gom_jpeg_encode_scan_u8(frames.data_ptr(), 1, 16, ops.JPEG_MAX_WIDTH + 1, 1, 95, ws.data_ptr(), ws.shape[0],
                                            off.data_ptr(), None)
    torch.cuda.synchronize()
    assert rc == 2 and off.tolist() == [-7, -7] and not ws.any()                 # nothing ran
    empty_payload, empty_off = ops.jpeg_encode(frames[:0], 95, True)
    assert empty_payload.numel() == 0 and empty_off.tolist() == [0]
    with pytest.raises(ValueError):
        ops.jpeg_encode(frames[:, :, :16], 0, True)


def test_show_device_encode_writes_the_files_of_host_encode(tmp_path):
    """One video of 1.jpg, 2.png, 3.jpeg with an instance on the first frame: the same bytes from --device-encode and from
    --host-encode --host-draw, the PNG as a run without either flag writes it, and Pillow decodes the JPEG files."""
    from gomatching_amd import show
    data = tmp_path / "ICDAR15_frames" / "Video_9_1_1"
    data.mkdir(parents=True)
    rng = np.random.RandomState(3)
    for i, ext in enumerate(("jpg", "png", "jpeg")):
        Image.fromarray(rng.randint(0, 256, (40, 64, 3)).astype(np.uint8)).save(str(data / ("%d.%s" % (i + 1, ext))))
    out = tmp_path / "out"
    (out / "jsons").mkdir(parents=True)
    obj = {"points": [5, 5, 50, 5, 50, 30, 5, 30], "ID": 4, "transcription": "abc",
           "segmentation": [[[5, 5], [50, 5], [50, 30], [5, 30]]]}
    with open(str(out / "jsons" / "Video_9_1_1.json"), "w") as fp:
        json.dump({str(i + 1): ([obj] if i == 0 else []) for i in range(3)}, fp)
    base = ["--input", str(tmp_path / "ICDAR15_frames"), "--results", str(out), "--voc-size", "37"]
    runs = {"device": ["--device-encode"], "host": ["--host-encode", "--host-draw"], "plain": []}
    for name, extra in runs.items():
        assert show.main(base + ["--output", str(tmp_path / name)] + extra) == 0

    def read(run, f):
        with open(str(tmp_path / run / "results" / "Video_9_1_1" / f), "rb") as fp:
            return fp.read()
    for f in ("1.jpg", "3.jpeg"):
        assert read("device", f) == read("host", f) and read("device", f) != read("plain", f)
        with Image.open(str(tmp_path / "device" / "results" / "Video_9_1_1" / f)) as im:
            im.load()
            assert im.size == (64, 40)
    assert read("device", "2.png") == read("plain", "2.png") == read("host", "2.png")
    assert sorted(os.listdir(str(tmp_path / "device" / "results" / "Video_9_1_1"))) == ["1.jpg", "2.png", "3.jpeg"]
