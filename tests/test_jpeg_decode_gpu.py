"""GPU: csrc/jpeg_decode.hip against `jpeg.decode_host` byte for byte, status words included, on every family of
tests/jpeg_decode_families.py (which the CPU test holds to the plain-Python statement and to Pillow); the damaged streams (the
host check has walked them under sanitizers first); reproducibility; refusals before any launch."""
import numpy as np
import pytest
import torch

import jpeg_decode_families as fam

from gomatching_amd import jpeg

pytestmark = pytest.mark.gpu
FAMILIES = dict(fam.families())
DAMAGED = dict(fam.damaged())


def _device(files, bgr):
    from gomatching_amd import ops
    out, status = ops.jpeg_decode(jpeg.plan(files), bgr)
    assert out.is_cuda and out.dtype == torch.uint8 and status.is_cuda and status.dtype == torch.int32
    return out.cpu().numpy(), status.cpu().numpy()


@pytest.mark.parametrize("name", sorted(FAMILIES))
def test_kernels_equal_the_host_path(name):
    files = FAMILIES[name]
    for bgr in (True, False):
        want, want_status = jpeg.decode_host(files, bgr=bgr, return_status=True)
        got, status = _device(files, bgr)
        assert list(status) == list(want_status) == [0] * len(files)
        assert got.shape == want.shape and int((got != want).sum()) == 0
    assert np.array_equal(got[0], fam.pillow_pixels(files[0]))                  # and so Pillow (R G B)


def test_damaged_streams_give_the_host_status_words():
    for name, data in sorted(DAMAGED.items()):
        _, want = jpeg.decode_host([data], return_status=True)
        _, status = _device([data], True)
        assert want[0] != 0 and list(status) == list(want), (name, status, want)
    files = [FAMILIES["size-33x47-2"][0], DAMAGED["cut-50%"], FAMILIES["q50-noise-33x47-420"][0]]
    want, want_status = jpeg.decode_host(files, return_status=True)
    got, status = _device(files, True)
    assert list(status) == list(want_status) and status[0] == 0 and status[1] != 0 and status[2] == 0
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[2], want[2])


def test_two_calls_give_the_same_bytes():
    files = FAMILIES["three-files-70x37-420"]
    a, sa = _device(files, True)
    b, sb = _device(files, True)
    assert np.array_equal(a, b) and np.array_equal(sa, sb)
    dev = jpeg.decode_device(files, bgr=True)
    assert dev.is_cuda and np.array_equal(dev.cpu().numpy(), a)


def test_refused_geometry_raises_before_any_launch():
    from gomatching_amd import lib, ops
    L = lib.load()
    assert L.gom_jpeg_decode_workspace_bytes(1, 16, 16, 3, 2, 2) == 256 * 3 + 256 * 2
    assert L.gom_jpeg_decode_workspace_bytes(1, 16, 4097, 3, 2, 2) == -1        # too wide
    assert L.gom_jpeg_decode_workspace_bytes(1, 16, 16, 3, 1, 2) == -1          # 4:4:0
    assert L.gom_jpeg_decode_workspace_bytes(1, 16, 16, 4, 1, 1) == -1          # four components
    p = jpeg.plan(FAMILIES["size-16x16-2"])
    p.hs, p.vs = 4, 1
    with pytest.raises(lib.GomError, match="GOM_ERR_UNSUPPORTED"):
        ops.jpeg_decode(p, True)
