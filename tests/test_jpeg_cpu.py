"""CPU: the JPEG rule of include/gomatching_hip.h.  `jpeg.encode_host` (numpy, vectorised over blocks) against the plain-Python
statement byte for byte; the files against Pillow (they decode; size, mode, sampling and quantisation tables are those of
Pillow's own files; the Huffman tables are the ones Pillow writes); fidelity against Pillow's encoder; the command line."""
import ctypes
import io
import json
import os

import numpy as np
import pytest
from PIL import Image

import jpeg_statement as js
import overlay_statement as ovs

from gomatching_amd import jpeg

NAMES = sorted(js.CASES)


def _host_files(frames, quality, bgr):
    payload, offsets = jpeg.encode_host(frames, quality, bgr)
    assert payload.dtype == np.uint8 and offsets.dtype == np.int64 and offsets[0] == 0 and offsets[-1] == len(payload)
    return jpeg.files(payload, offsets, frames.shape[1], frames.shape[2], quality)


def _segments(data):
    """[(marker, body)] of a file up to and including SOS, and the offset of the entropy-coded data."""
    out, i = [], 2
    assert data[:2] == b"\xff\xd8"
    while True:
        assert data[i] == 0xFF
        marker, size = data[i + 1], data[i + 2] * 256 + data[i + 3]
        out.append((marker, data[i + 4:i + 2 + size]))
        i += 2 + size
        if marker == 0xDA:
            return out, i


def _pillow_file(rgb, quality):
    buf = io.BytesIO()
    Image.fromarray(rgb).save(buf, format="JPEG", quality=quality)
    return buf.getvalue()


def _rgb(frame, bgr):
    return np.ascontiguousarray(frame[:, :, ::-1]) if bgr else np.ascontiguousarray(frame)


# ------------------------------------------------------------------------------------------ tables
def test_tables_are_the_stated_ones():
    assert list(jpeg.ZIGZAG) == js.zigzag()
    assert jpeg.DCT_T.tolist() == js.dct_table()
    assert list(jpeg.Q_LUM) == js.Q_LUM and list(jpeg.Q_CHR) == js.Q_CHR
    assert list(jpeg.quant_tables(95)[0][:8]) == [2, 1, 1, 2, 2, 4, 5, 6]
    for q in (0, 101):
        with pytest.raises(ValueError):
            jpeg.quant_tables(q)


def test_huffman_tables_are_the_ones_pillow_writes():
    """The four Annex K tables: the DHT segments of Pillow's own (not optimised) file hold the same BITS and HUFFVAL."""
    segs, _ = _segments(_pillow_file(np.zeros((8, 8, 3), dtype=np.uint8), 95))
    body = b"".join(b for m, b in segs if m == 0xC4)
    found, i = {}, 0
    while i < len(body):
        n = sum(body[i + 1:i + 17])
        found[body[i]] = (list(body[i + 1:i + 17]), list(body[i + 17:i + 17 + n]))
        i += 17 + n
    assert found == {0x00: jpeg.HUFF["dc_lum"], 0x10: jpeg.HUFF["ac_lum"], 0x01: jpeg.HUFF["dc_chr"], 0x11: jpeg.HUFF["ac_chr"]}


# ------------------------------------------------------------------------------------------ twin against statement
@pytest.mark.parametrize("name", NAMES)
def test_host_path_equals_the_statement(name):
    frames, quality, bgr, want = js.case(name)
    got = _host_files(frames, quality, bgr)
    assert len(got) == len(want) == frames.shape[0]
    for f in range(len(want)):
        assert got[f] == want[f], (name, f, len(got[f]), len(want[f]))


def test_the_cases_hold_what_they_are_for():
    """Each edge the list names is really there."""
    def data_of(name):
        frames, quality, bgr, want = js.case(name)
        _, start = _segments(want[0])
        return frames, jpeg.coefficients(frames, quality, bgr), want[0][start:-2]

    _, co, data = data_of("flat")
    assert not co[..., 1:].any() and len(set(co[0, 0, :, 0, 0])) == 1              # EOB only, zero DC differences behind the first
    _, co, _ = data_of("checker_q100")
    assert np.abs(co[..., 1:]).max() >= 512                                        # category 10
    _, co, _ = data_of("zrl")
    nz0, nz1 = np.nonzero(co[0, 0, 0, 0])[0], np.nonzero(co[0, 0, 0, 1])[0]
    assert np.diff(nz0).max() > 16 and list(nz1) == [63]                           # one ZRL; three ZRLs and no EOB
    assert js.search_ff(js.FF_SEED + 1) == js.FF_SEED                              # the seed is what the search finds
    _, _, data = data_of("ff")
    assert data.count(b"\xff\x00") >= 3 and b"\xff\x00\xff\xd0" in data            # one of them last in its interval
    frames, _, data = data_of("nine_rows")
    assert frames.shape[1] > 9 * 16 and b"\xff\xd7" in data and data.count(b"\xff\xd0") == 2    # RST7, then RST0 again
    assert js.case("three_frames")[0].shape[0] == 3 and js.case("1x1")[0].shape[1:3] == (1, 1)
    assert {js.CASES[n][1] for n in NAMES} >= {1, 50, 95, 100} and {js.CASES[n][2] for n in NAMES} == {True, False}
    for name in ("17x23", "33x47"):
        H, W = js.case(name)[0].shape[1:3]
        assert H % 16 and W % 16


# ------------------------------------------------------------------------------------------ Pillow
@pytest.mark.parametrize("name", NAMES)
def test_pillow_decodes_the_files_and_agrees_on_their_layout(name):
    frames, quality, bgr, want = js.case(name)
    for f, data in enumerate(want):
        ours = Image.open(io.BytesIO(data))
        ours.load()                                                                # a full decode
        theirs = Image.open(io.BytesIO(_pillow_file(_rgb(frames[f], bgr), quality)))
        assert ours.size == theirs.size == (frames.shape[2], frames.shape[1]) and ours.mode == theirs.mode == "RGB"
        assert ours.layer == theirs.layer == [(1, 2, 2, 0), (2, 1, 1, 1), (3, 1, 1, 1)]
        assert {k: list(v) for k, v in ours.quantization.items()} == {k: list(v) for k, v in theirs.quantization.items()}
        assert not ours.info.get("progressive") and ours.info.get("jfif_version") == (1, 1)


@pytest.mark.parametrize("quality", [1, 25, 50, 75, 95, 100])
def test_quantisation_tables_equal_pillows(quality):
    theirs = Image.open(io.BytesIO(_pillow_file(np.zeros((8, 8, 3), dtype=np.uint8), quality))).quantization
    lum, chr_ = jpeg.quant_tables(quality)
    ours = Image.open(io.BytesIO(jpeg.header(8, 8, quality))).quantization
    assert list(theirs[0]) == list(ours[0]) and list(theirs[1]) == list(ours[1])
    assert list(lum) == list(theirs[0]) and list(chr_) == list(theirs[1])           # natural order, as Pillow reports


# ------------------------------------------------------------------------------------------ fidelity
def _fidelity_inputs():
    yy, xx = np.mgrid[0:48, 0:64]
    grad = np.stack([xx * 4, yy * 5, (xx + yy) * 2], axis=-1).astype(np.uint8)
    grad[10:14, 5:50] = (255, 0, 0)
    grad[20:40, 30:33] = (0, 255, 255)
    grad[5:44:6, 52:62] = (255, 255, 255)
    from gomatching_amd import show
    frames, instances, labels, _ = ovs.case("main")
    drawn = show.compose_host(frames, ovs.scene_of(frames, instances, labels))[2]
    noise = np.random.RandomState(11).randint(0, 256, (47, 33, 3)).astype(np.uint8)
    return [("gradient+strokes 64x48", grad), ("drawn frame 70x37", drawn), ("noise 33x47", noise)]


def _psnr(a, b):
    mse = np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2)
    return 10.0 * np.log10(255.0 ** 2 / mse)


# The margin, fixed after measuring here (the twin gives the device's bytes): the worst shortfall against Pillow over the
# three inputs and q = 50, 95, 100 is 0.015 dB (noise at q = 50), rounded up to the next 0.05 dB.  PSNR against the source in
# dB, ours / Pillow's, and file bytes, ours / Pillow's (ours carry the restart markers; sizes are not a gate):
#   gradient+strokes 64x48   q= 50   24.555 / 24.543   1040 / 1032
#   gradient+strokes 64x48   q= 95   27.641 / 27.583   2055 / 2017
#   gradient+strokes 64x48   q=100   27.773 / 27.771   3151 / 3171
#   drawn frame 70x37        q= 50   15.493 / 15.467   1867 / 1727
#   drawn frame 70x37        q= 95   17.090 / 17.076   4255 / 4001
#   drawn frame 70x37        q=100   17.102 / 17.100   6671 / 6409
#   noise 33x47              q= 50   11.870 / 11.885   1432 / 1360
#   noise 33x47              q= 95   12.814 / 12.814   2761 / 2634
#   noise 33x47              q=100   12.821 / 12.824   4024 / 3938
FIDELITY_BOUND_DB = 0.05


def test_fidelity_against_pillows_encoder(capsys):
    """Both files decoded by Pillow, PSNR against the source.  The margin exists only because two correct DCT roundings differ
    by a quantisation step on near-ties; a shortfall above 0.5 dB anywhere would be a defect."""
    worst = 0.0
    with capsys.disabled():
        for name, img in _fidelity_inputs():
            for q in (50, 95, 100):
                ours = _host_files(img[None], q, False)[0]
                theirs = _pillow_file(img, q)
                p_ours = _psnr(np.asarray(Image.open(io.BytesIO(ours)).convert("RGB")), img)
                p_theirs = _psnr(np.asarray(Image.open(io.BytesIO(theirs)).convert("RGB")), img)
                print("fidelity %-24s q=%3d  psnr %.3f / %.3f dB  bytes %d / %d" % (name, q, p_ours, p_theirs, len(ours), len(theirs)))
                worst = max(worst, p_theirs - p_ours)
    assert FIDELITY_BOUND_DB <= 0.5
    assert worst <= FIDELITY_BOUND_DB, worst


# ------------------------------------------------------------------------------------------ the boundary
def test_entry_points_refuse_without_a_gpu():
    """Argument checks run before any HIP call: a width above the stated limit is GOM_ERR_UNSUPPORTED without a launch."""
    from gomatching_amd import lib, ops
    L = lib.load()
    OK, INVALID, UNSUPPORTED = 0, 1, 2
    p, odd = ctypes.c_void_p(0x1000), ctypes.c_void_p(0x1002)                  # never dereferenced
    big = 1 << 40
    assert ops.JPEG_MAX_WIDTH == jpeg.MAX_WIDTH == 4096 and ops.JPEG_MAX_HEIGHT == jpeg.MAX_HEIGHT == 65535

    def scan(frames=p, F=1, H=16, W=16, bgr=1, quality=95, ws=p, ws_bytes=big, off=p):
        return L.gom_jpeg_encode_scan_u8(frames, F, H, W, bgr, quality, ws, ws_bytes, off, None)
    assert scan(W=4097) == UNSUPPORTED and scan(H=65536) == UNSUPPORTED
    assert scan(frames=None) == INVALID and scan(ws=None) == INVALID and scan(off=None) == INVALID
    assert scan(F=-1) == INVALID and scan(H=0) == INVALID and scan(W=0) == INVALID
    assert scan(quality=0) == INVALID and scan(quality=101) == INVALID and scan(bgr=2) == INVALID
    assert scan(ws_bytes=100) == INVALID and scan(ws=odd) == INVALID
    assert scan(F=0) == OK                                                     # no frames: no launch
    assert L.gom_jpeg_workspace_bytes(1, 16, 4097) == -1 and L.gom_jpeg_workspace_bytes(1, 0, 16) == -1
    one = L.gom_jpeg_workspace_bytes(1, 16, 16)
    assert one >= 6 * (128 + 208 + 416) and L.gom_jpeg_workspace_bytes(3, 16, 16) <= 3 * one

    def pack(ws=p, ws_bytes=big, F=1, H=16, W=16, total=8, payload=p, payload_bytes=8):
        return L.gom_jpeg_encode_pack_u8(ws, ws_bytes, F, H, W, total, payload, payload_bytes, None)
    assert pack(W=4097) == UNSUPPORTED
    assert pack(ws=None) == INVALID and pack(payload=None) == INVALID and pack(payload=odd) == INVALID
    assert pack(total=-1) == INVALID and pack(total=9, payload_bytes=9) == INVALID and pack(total=1 << 30, payload_bytes=1 << 30) == INVALID
    assert pack(total=0, payload_bytes=0, payload=None) == OK                  # nothing to pack: no launch

    with pytest.raises(ValueError):
        jpeg.header(16, 4097, 95)
    with pytest.raises(ValueError):
        jpeg.encode_host(np.zeros((1, 8, 4097, 3), dtype=np.uint8), 95, True)


# ------------------------------------------------------------------------------------------ command line
def _tree(tmp_path):
    """One video of three frames: 1.jpg, 2.png, 3.jpeg (40 x 64), an instance on the first."""
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
    return str(tmp_path / "ICDAR15_frames"), str(out)


def _read(path):
    with open(path, "rb") as fp:
        return fp.read()


def test_command_line_host_encode(tmp_path):
    from gomatching_amd import eval as E
    from gomatching_amd import show
    data, out = _tree(tmp_path)
    plain, coded = str(tmp_path / "plain"), str(tmp_path / "coded")
    base = ["--input", data, "--results", out, "--host-draw", "--voc-size", "37"]
    assert show.main(base + ["--output", plain]) == 0
    assert show.main(base + ["--output", coded, "--host-encode", "--jpeg-quality", "90"]) == 0
    paths = E.frame_paths(os.path.join(data, "Video_9_1_1"))
    with open(os.path.join(out, "jsons", "Video_9_1_1.json")) as fp:
        annotation = show.rows_of_json(json.load(fp))
    drawn = show.draw_clip([E.read_frame(p) for p in paths], [annotation[str(i + 1)] for i in range(3)], 37, host=True)
    want = jpeg.files(*jpeg.encode_host(drawn[[0, 2]], 90, True), 40, 64, 90)
    for name, expect in (("1.jpg", want[0]), ("3.jpeg", want[1])):
        got = _read(os.path.join(coded, "results", "Video_9_1_1", name))
        assert got == expect and got != _read(os.path.join(plain, "results", "Video_9_1_1", name))
        im = Image.open(io.BytesIO(got))
        im.load()
        assert im.size == (64, 40) and list(im.quantization[0]) == list(Image.open(io.BytesIO(_pillow_file(
            np.zeros((8, 8, 3), dtype=np.uint8), 90))).quantization[0])
    # the PNG source goes through Pillow as before, byte for byte
    assert _read(os.path.join(coded, "results", "Video_9_1_1", "2.png")) == _read(os.path.join(plain, "results", "Video_9_1_1", "2.png"))
    # the drawing is in the decoded picture: close to the drawn frame, far from the source
    got = E.read_frame(os.path.join(coded, "results", "Video_9_1_1", "1.jpg"))
    assert _psnr(got, drawn[0]) > _psnr(got, E.read_frame(paths[0])) + 3


@pytest.mark.parametrize("extra,status,word", [
    (["--device-encode", "--host-draw"], 2, "--host-draw"),
    (["--device-encode", "--host-encode"], 2, "at most one"),
    (["--host-draw", "--jpeg-quality", "80"], 2, "--jpeg-quality"),
    (["--host-draw", "--host-encode", "--jpeg-quality", "0"], 2, "1 .. 100"),
])
def test_command_line_refusals(tmp_path, capsys, extra, status, word):
    from gomatching_amd import show
    data, out = _tree(tmp_path)
    assert show.main(["--input", data, "--results", out] + extra) == status
    assert word in capsys.readouterr().err
    assert not os.path.exists(os.path.join(out, "results"))


def test_device_encode_without_a_gpu_exits_1(tmp_path, capsys, monkeypatch):
    import torch
    from gomatching_amd import show
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    data, out = _tree(tmp_path)
    assert show.main(["--input", data, "--results", out, "--device-encode"]) == 1
    assert "GPU" in capsys.readouterr().err
    assert not os.path.exists(os.path.join(out, "results"))


def test_eval_takes_the_encode_flags_only_with_show(capsys):
    from gomatching_amd import eval as E
    args = ["--builtin", "icdar15", "--input", ".", "--output", "unused"]
    assert E.main(args + ["--host-encode"]) == 2 and "--show" in capsys.readouterr().err
    assert E.main(args + ["--show", "--device-encode", "--host-draw"]) == 2 and "--host-draw" in capsys.readouterr().err
    assert not os.path.exists("unused")
