"""GPU: the chunked entropy walk (`ops.jpeg_decode(..., walk="chunks")`, csrc/jpeg_decode.hip + csrc/jpeg_decode_chunks.h)
against `jpeg.decode_host` byte for byte, status words included: the families of tests/jpeg_decode_families.py at chunk sizes 16
(the ones that stress it: many spans, many passes, many tiny segments, less than a chunk), 64 and 256; two larger files; the
damaged streams (route `serial`, the serial walk's status words); reproducibility, seg_info included; the segment walk's pixels;
refused chunk sizes before any launch."""
import functools

import numpy as np
import pytest
import torch

import jpeg_decode_families as fam

from gomatching_amd import jpeg

pytestmark = pytest.mark.gpu
FAMILIES = dict(fam.families())
DAMAGED = dict(fam.damaged())
AT_16 = ("size-1296x48-0", "size-48x1296-2", "size-1x1-L", "flat-33x47-2", "rst-blocks-33x47-2", "rst-rows-48x1296-1",
         "q100-noise-33x47-0", "optimize-70x37-2", "own-70x37", "three-files-70x37-420")
LARGER = {"noise-320x240": lambda: (fam.pillow_file(fam.content("noise", 320, 240, 21), 2, 95),),
          "gradient-640x360": lambda: (fam.pillow_file(fam.content("gradient", 640, 360, 21), 2, 95),)}


@functools.lru_cache(maxsize=None)
def _files(name):
    return FAMILIES[name] if name in FAMILIES else LARGER[name]()


@functools.lru_cache(maxsize=None)
def _host(name, bgr=True):
    """(pixels, status) of jpeg.decode_host, computed once per case and left unchanged."""
    out, status = jpeg.decode_host(_files(name), bgr=bgr, return_status=True)
    out.setflags(write=False)
    return out, status


def _device(files, bgr=True, chunk=None, walk="chunks"):
    from gomatching_amd import ops
    if walk == "segments":
        out, status = ops.jpeg_decode(jpeg.plan(files), bgr)
        return out.cpu().numpy(), status.cpu().numpy(), None
    out, status, info = ops.jpeg_decode(jpeg.plan(files), bgr, walk="chunks", chunk_bytes=chunk, return_info=True)
    assert out.is_cuda and out.dtype == torch.uint8 and status.dtype == torch.int32
    assert info.is_cuda and info.dtype == torch.int32 and info.shape == (jpeg.plan(files).desc.shape[0], 2)
    return out.cpu().numpy(), status.cpu().numpy(), info.cpu().numpy()


def _check_clean(name, chunk):
    want, want_status = _host(name)
    got, status, info = _device(_files(name), True, chunk)
    assert list(status) == list(want_status) == [0] * len(_files(name))
    assert got.shape == want.shape and int((got != want).sum()) == 0
    assert (info[:, 0] == 0).all(), info[:, 0]                                   # every clean segment is the chunk walk's
    assert info[:, 1].min() >= 0 and info[:, 1].max() <= 256
    return info


@pytest.mark.parametrize("name", AT_16)
def test_chunks_of_16_equal_the_host_path(name):
    info = _check_clean(name, 16)
    if name == "q100-noise-33x47-0":
        assert info[:, 1].max() > 64                                             # (the slow case: it settles over many passes)


@pytest.mark.parametrize("chunk", (64, 256))
@pytest.mark.parametrize("name", sorted(FAMILIES))
def test_chunks_equal_the_host_path(name, chunk):
    _check_clean(name, chunk)


@pytest.mark.parametrize("chunk", (256, None))
@pytest.mark.parametrize("name", sorted(LARGER))
def test_larger_files_equal_the_host_path(name, chunk):
    _check_clean(name, chunk)


def test_both_channel_orders():
    name = "size-33x47-2"
    for bgr in (True, False):
        want, _ = _host(name, bgr)
        got, status, _ = _device(_files(name), bgr, 64)
        assert list(status) == [0] and int((got != want).sum()) == 0
    assert np.array_equal(got[0], fam.pillow_pixels(_files(name)[0]))            # and so Pillow (R G B)


def test_damaged_streams_go_to_the_serial_walk():
    for chunk in (16, 256):
        for name, data in sorted(DAMAGED.items()):
            _, want = jpeg.decode_host([data], return_status=True)
            _, status, info = _device([data], True, chunk)
            assert want[0] != 0 and list(status) == list(want), (name, chunk, status, want)
            assert (info[:, 0] == 1).any(), (name, chunk, info)
    files = [FAMILIES["size-33x47-2"][0], DAMAGED["cut-50%"], FAMILIES["q50-noise-33x47-420"][0]]
    want, want_status = jpeg.decode_host(files, return_status=True)
    got, status, info = _device(files, True, 64)
    assert list(status) == list(want_status) and status[0] == 0 and status[1] != 0 and status[2] == 0
    assert list(info[:, 0]) == [0, 1, 0]
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[2], want[2])


def test_two_calls_give_the_same_bytes_and_info():
    files = FAMILIES["three-files-70x37-420"]
    a, sa, ia = _device(files, True, 64)
    b, sb, ib = _device(files, True, 64)
    assert np.array_equal(a, b) and np.array_equal(sa, sb) and np.array_equal(ia, ib)
    dev = jpeg.decode_device(files, bgr=True, walk="chunks", chunk_bytes=64)
    assert dev.is_cuda and np.array_equal(dev.cpu().numpy(), a)


def test_chunks_equal_segments():
    files = FAMILIES["rst-rows-70x37-2"]
    a, sa, _ = _device(files, True, None)
    b, sb, _ = _device(files, True, walk="segments")
    assert np.array_equal(a, b) and np.array_equal(sa, sb)
    auto, status = jpeg.decode_device(files, return_status=True, walk="auto")
    assert np.array_equal(auto.cpu().numpy(), a) and list(status) == list(sa)


def test_eval_decode_frames_counts_the_routes():
    from gomatching_amd import eval as E
    blobs = [FAMILIES["size-33x47-2"][0], FAMILIES["q50-noise-33x47-420"][0]]       # short segments: auto takes the segment walk
    want = jpeg.decode_host(blobs, bgr=True)
    for walk in ("chunks", "segments", "auto"):
        counts = {k: 0 for k in E.DECODE_ROUTES}
        frames = E.decode_frames(["a.jpg", "b.jpg"], blobs, counts, torch.device("cuda:0"), walk)
        assert np.array_equal(frames[0].cpu().numpy(), want[0]) and np.array_equal(frames[1].cpu().numpy(), want[1])
        assert (counts["device"], counts["flagged"]) == (2, 0)
        assert (counts["chunks"], counts["serial"]) == ((2, 0) if walk == "chunks" else (0, 2)), (walk, counts)


@pytest.mark.parametrize("chunk", (24, 8, 8192))
def test_refused_chunk_bytes_raise_before_any_launch(chunk):
    from gomatching_amd import ops
    with pytest.raises(ValueError, match="power of two"):
        ops.jpeg_decode(jpeg.plan(FAMILIES["size-16x16-2"]), True, walk="chunks", chunk_bytes=chunk)
    with pytest.raises(ValueError, match="power of two"):
        jpeg.decode_device(FAMILIES["size-16x16-2"], walk="chunks", chunk_bytes=chunk)
