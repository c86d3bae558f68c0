"""CPU: the JPEG decoding rule of include/gomatching_hip.h (`gom_jpeg_decode_*`).  `jpeg.decode_host` against the plain-Python
statement byte for byte, and both against Pillow's `Image.open(..).convert("RGB")` with 0 differing bytes on every family of
tests/jpeg_decode_families.py (the bound is derived, not measured: all three are the same integer rule); the parser's
refusals; the status words of the damaged streams."""
import numpy as np
import pytest

import jpeg_decode_families as fam
import jpeg_decode_statement as stmt

from gomatching_amd import jpeg

FAMILIES = dict(fam.families())


def test_every_family_is_accepted():
    """A refusal would send the file to Pillow and hide a failure: none is refused, and the list covers what it claims."""
    assert len(FAMILIES) == len(fam.families()) >= 80
    samplings = set()
    for name, files in fam.families():
        for data in files:
            info = jpeg.parse(data)
            assert isinstance(info, jpeg.JpegInfo), (name, info)
            samplings.add((info.ncomp, info.hs, info.vs))
    assert samplings == {(1, 1, 1), (3, 1, 1), (3, 2, 1), (3, 2, 2)}
    assert any(jpeg.parse(f[0]).restart for _, f in fam.families())
    custom = jpeg.parse(FAMILIES["optimize-70x37-2"][0]).huff
    assert list(custom[(1, 0)][0]) != jpeg.HUFF["ac_lum"][0]           # Pillow's optimize=True: not the Annex K table


@pytest.mark.parametrize("name", sorted(FAMILIES))
def test_host_path_equals_pillow_and_the_statement(name):
    files = FAMILIES[name]
    rgb, status = jpeg.decode_host(files, bgr=False, return_status=True)
    bgr = jpeg.decode_host(files, bgr=True)
    assert rgb.dtype == np.uint8 and list(status) == [0] * len(files)
    assert np.array_equal(bgr, rgb[..., ::-1])
    for f, data in enumerate(files):
        want = fam.pillow_pixels(data)
        assert rgb[f].shape == want.shape
        assert int((rgb[f] != want).sum()) == 0, "%s file %d: %d bytes differ from Pillow" % (name, f, int((rgb[f] != want).sum()))
        assert np.array_equal(np.array(stmt.decode(data, bgr=False), dtype=np.uint8), rgb[f])
    assert np.array_equal(np.array(stmt.decode(files[0], bgr=True), dtype=np.uint8), bgr[0])


def test_datasets_form_is_decoded_not_refused():
    """4:2:0 colour without restart markers at sizes that are no multiple of 16: what the datasets are."""
    for name in ("size-17x17-2", "size-33x47-2", "size-70x37-2", "q50-noise-33x47-420"):
        info = jpeg.parse(FAMILIES[name][0])
        assert (info.ncomp, info.hs, info.vs, info.restart) == (3, 2, 2, 0) and len(info.seg_start) == 1


def test_parse_reports_the_file():
    data = FAMILIES["rst-rows-70x37-2"][0]
    info = jpeg.parse(data)
    assert (info.H, info.W, info.ncomp, info.hs, info.vs) == (37, 70, 3, 2, 2)
    assert info.restart == 5 and info.mcus == 15 and len(info.seg_start) == len(info.seg_end) == 3
    assert info.quant.shape == (3, 64) and data[info.scan[1]:info.scan[1] + 2] == b"\xff\xd9"
    for s in range(2):                                      # a segment ends where its RSTn stands
        assert data[info.seg_end[s]:info.seg_end[s] + 2] == bytes([0xFF, 0xD0 + s]) and info.seg_start[s + 1] == info.seg_end[s] + 2
    own = jpeg.parse(FAMILIES["own-70x37"][0])
    assert own.restart == 5 and len(own.seg_start) == 3 and np.array_equal(own.quant[0], jpeg.quant_tables(95)[0])
    p = jpeg.plan(FAMILIES["three-files-70x37-420"])
    assert p.F == 3 and p.sets.shape == (3, jpeg.SET_WORDS) and p.desc.shape == (3, jpeg.DESC_WORDS) and list(p.seg_off) == [0, 1, 2, 3]
    assert len({len(f) for f in FAMILIES["three-files-70x37-420"]}) == 3


@pytest.mark.parametrize("name, data, word", fam.refused(), ids=[r[0] for r in fam.refused()])
def test_refusals_name_their_reason(name, data, word):
    r = jpeg.parse(data)
    assert isinstance(r, jpeg.Refusal) and word in r.reason, r
    with pytest.raises(ValueError, match="refused"):
        jpeg.decode_host([data])


def test_mixed_geometry_is_an_error():
    with pytest.raises(ValueError, match="group the files"):
        jpeg.decode_host([FAMILIES["size-8x8-2"][0], FAMILIES["size-16x16-2"][0]])


DAMAGED = dict(fam.damaged())


@pytest.mark.parametrize("name", sorted(DAMAGED))
def test_damaged_streams_set_the_status_word(name):
    data = DAMAGED[name]
    assert isinstance(jpeg.parse(data), jpeg.JpegInfo)
    pixels, status = jpeg.decode_host([data], return_status=True)      # raises nothing
    assert status.shape == (1,) and status[0] != 0
    want = {"cut": jpeg.STATUS_PAST_END, "wrong-rst": jpeg.STATUS_RST, "missing-rst": jpeg.STATUS_LEFT_OVER,
            "index-past-63": jpeg.STATUS_INDEX, "zrl-past-63": jpeg.STATUS_INDEX}
    for prefix, code in want.items():
        if name.startswith(prefix):
            assert status[0] == code


def test_a_damaged_file_flags_only_itself():
    files = [FAMILIES["size-33x47-2"][0], DAMAGED["cut-50%"], FAMILIES["q50-noise-33x47-420"][0]]
    pixels, status = jpeg.decode_host(files, bgr=False, return_status=True)
    assert status[0] == 0 and status[1] != 0 and status[2] == 0
    assert np.array_equal(pixels[0], fam.pillow_pixels(files[0])) and np.array_equal(pixels[2], fam.pillow_pixels(files[2]))
