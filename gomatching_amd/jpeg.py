"""Baseline JPEG encoding of drawn frames: THE RULE of include/gomatching_hip.h (`gom_jpeg_encode_*`) in numpy integers, the
file header, and the device path through csrc/jpeg.hip.

    header(H, W, quality)                  -> bytes   SOI, APP0 JFIF 1.01, two DQT, SOF0, four DHT, DRI, SOS
    encode_host(frames, quality, bgr)      -> (payload u8 [n], offsets int64 [F+1])   the rule in numpy, vectorised over blocks
    encode_device(frames, quality, bgr)    -> the same pair through `ops.jpeg_encode` (frames: a CUDA tensor or a host array)
    files(payload, offsets, H, W, quality) -> list[bytes]   header + a frame's entropy-coded data + EOI

The payload of a frame is its entropy-coded segment alone: the restart intervals (one MCU row each) one after the other, each
padded with 1-bits to a byte, 0x00 after every 0xFF, RSTn between two intervals.  `encode_host` and the kernels agree byte for
byte by construction (integers only); tests/jpeg_statement.py states the same rule per block and per bit in plain Python.
Baseline sequential DCT, 8 bits, Y Cb Cr at 4:2:0, the Annex K quantisation tables scaled by the usual quality rule and the
four Annex K Huffman tables -- what Pillow's `save(quality=q)` writes, plus the restart markers.  No byte parity with libjpeg
is claimed: its DCT rounds differently (tests/test_jpeg_cpu.py measures the difference in PSNR).

The second half of the module DECODES baseline files (`gom_jpeg_decode_*`, csrc/jpeg_decode.hip; `eval --device-decode`):

    parse(data)                            -> JpegInfo | Refusal   header, tables, restart segments; what is refused and why
    plan(files)                            -> DecodePlan           what one decode call uploads
    decode_host(files, bgr)                -> u8 [F,H,W,3]         the rule in numpy, the entropy walk in plain Python
    decode_device(files, bgr)              -> CUDA u8 [F,H,W,3]    the same through `ops.jpeg_decode`

There the rule IS libjpeg's arithmetic, and the pixels are byte-equal to Pillow's (tests/test_jpeg_decode_cpu.py).
"""
import numpy as np

from .lib import CONSTANTS as _ABI

MAX_WIDTH = _ABI["GOM_JPEG_MAX_WIDTH"]
# The chunked entropy walk (THE RULE of `gom_jpeg_decode_entropy_chunks_i16`): the default chunk and the mean segment length from
# which walk="auto" takes it, both measured (profiles/jpeg_decode_chunks_bench.log) and stated in include/gomatching_hip.h.
CHUNK_BYTES = _ABI["GOM_JPEG_DECODE_CHUNK_BYTES"]
AUTO_SEGMENT_BYTES = _ABI["GOM_JPEG_DECODE_AUTO_SEGMENT_BYTES"]
WALKS = ("auto", "segments", "chunks")
MAX_HEIGHT = 65535                                         # SOF0 holds 16 bits

# natural index of the k-th coefficient in zigzag order
ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21,
                   28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61,
                   54, 47, 55, 62, 63], dtype=np.int64)
# Annex K.1 / K.2, natural order
Q_LUM = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51,
                  87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120,
                  101, 72, 92, 95, 98, 112, 100, 103, 99], dtype=np.int64)
Q_CHR = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99,
                  99, 99, 99] + [99] * 32, dtype=np.int64)
# DCT_T[u][x] = round(8192 a(u) cos((2 x + 1) u pi / 16)), a(0) = sqrt(1/8), a(u) = 1/2
DCT_T = np.array([[2896, 2896, 2896, 2896, 2896, 2896, 2896, 2896],
                  [4017, 3406, 2276, 799, -799, -2276, -3406, -4017],
                  [3784, 1567, -1567, -3784, -3784, -1567, 1567, 3784],
                  [3406, -799, -4017, -2276, 2276, 4017, 799, -3406],
                  [2896, -2896, -2896, 2896, 2896, -2896, -2896, 2896],
                  [2276, -4017, 799, 3406, -3406, -799, 4017, -2276],
                  [1567, -3784, 3784, -1567, -1567, 3784, -3784, 1567],
                  [799, -2276, 3406, -4017, 4017, -3406, 2276, -799]], dtype=np.int64)
# Annex K.3 - K.6: (BITS, HUFFVAL) of the DC luminance, DC chrominance, AC luminance and AC chrominance tables
_AC_LUM_VALS = [
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91,
    0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a,
    0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53,
    0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79,
    0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5,
    0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9,
    0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2,
    0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa]
_AC_CHR_VALS = [
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14,
    0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17,
    0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a,
    0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78,
    0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3,
    0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7,
    0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2,
    0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa]
HUFF = {
    "dc_lum": ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12))),
    "dc_chr": ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(12))),
    "ac_lum": ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d], _AC_LUM_VALS),
    "ac_chr": ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77], _AC_CHR_VALS),
}


def quant_tables(quality):
    """(luminance, chrominance) int64 [64] in natural order: base * scale, scale = 5000 // q below 50 and 200 - 2 q from 50,
    (v + 50) // 100, clamped to 1 .. 255."""
    q = int(quality)
    if not 1 <= q <= 100:
        raise ValueError("quality must lie in 1 .. 100, not %r" % (quality,))
    scale = 5000 // q if q < 50 else 200 - 2 * q
    return tuple(np.clip((t * scale + 50) // 100, 1, 255) for t in (Q_LUM, Q_CHR))


def _code_table(bits, vals):
    """Annex C: (code, length) per symbol, int64 [256] each (length 0 = no code)."""
    code = np.zeros(256, dtype=np.int64)
    size = np.zeros(256, dtype=np.int64)
    c, k = 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            code[vals[k]], size[vals[k]] = c, length
            c += 1
            k += 1
        c <<= 1
    return code, size


_CODES = {name: _code_table(*t) for name, t in HUFF.items()}


def _u16(v):
    return bytes([(int(v) >> 8) & 255, int(v) & 255])


def check_size(H, W):
    H, W = int(H), int(W)
    if H < 1 or W < 1 or H > MAX_HEIGHT or W > MAX_WIDTH:
        raise ValueError("%d x %d (W x H) cannot be encoded: the width must lie in 1 .. %d and the height in 1 .. %d"
                         % (W, H, MAX_WIDTH, MAX_HEIGHT))
    return H, W


def header(H, W, quality):
    """Everything in front of the entropy-coded data; it depends only on H, W and quality."""
    H, W = check_size(H, W)
    lum, chr_ = quant_tables(quality)
    out = [b"\xff\xd8", b"\xff\xe0" + _u16(16) + b"JFIF\x00\x01\x01\x00" + _u16(1) + _u16(1) + b"\x00\x00"]
    for i, t in enumerate((lum, chr_)):
        out.append(b"\xff\xdb" + _u16(67) + bytes([i]) + bytes(int(v) for v in t[ZIGZAG]))
    out.append(b"\xff\xc0" + _u16(17) + b"\x08" + _u16(H) + _u16(W) + b"\x03" + b"\x01\x22\x00" + b"\x02\x11\x01" + b"\x03\x11\x01")
    for tc, name in ((0x00, "dc_lum"), (0x10, "ac_lum"), (0x01, "dc_chr"), (0x11, "ac_chr")):
        bits, vals = HUFF[name]
        out.append(b"\xff\xc4" + _u16(19 + len(vals)) + bytes([tc]) + bytes(bits) + bytes(vals))
    out.append(b"\xff\xdd" + _u16(4) + _u16((W + 15) // 16))
    out.append(b"\xff\xda" + _u16(12) + b"\x03" + b"\x01\x00" + b"\x02\x11" + b"\x03\x11" + b"\x00\x3f\x00")
    return b"".join(out)


def coefficients(frames, quality, bgr):
    """u8 [F,H,W,3] -> int64 [F, MH, MW, 6, 64]: the quantised coefficients of every MCU's blocks Y00 Y01 Y10 Y11 Cb Cr in
    zigzag order (colour, padding, 2x2 mean, DCT and quantisation of the rule)."""
    fr = np.asarray(frames)
    if fr.dtype != np.uint8 or fr.ndim != 4 or fr.shape[3] != 3:
        raise ValueError("frames must be u8 [F,H,W,3]")
    F, H, W, _ = fr.shape
    check_size(H, W)
    lum, chr_ = quant_tables(quality)
    MH, MW = (H + 15) // 16, (W + 15) // 16
    ys, xs = np.minimum(np.arange(16 * MH), H - 1), np.minimum(np.arange(16 * MW), W - 1)
    px = fr[:, ys][:, :, xs].astype(np.int64)
    r, g, b = (px[..., 2], px[..., 1], px[..., 0]) if bgr else (px[..., 0], px[..., 1], px[..., 2])
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    cb = (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16
    cr = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16

    def mean4(c):
        return (c[:, 0::2, 0::2] + c[:, 0::2, 1::2] + c[:, 1::2, 0::2] + c[:, 1::2, 1::2] + 2) >> 2

    yb = (y - 128).reshape(F, MH, 2, 8, MW, 2, 8).transpose(0, 1, 4, 2, 5, 3, 6).reshape(F, MH, MW, 4, 8, 8)
    cbb, crb = ((mean4(c) - 128).reshape(F, MH, 8, MW, 8).transpose(0, 1, 3, 2, 4)[:, :, :, None] for c in (cb, cr))
    s = np.concatenate([yb, cbb, crb], axis=3)                              # [F, MH, MW, 6, y, x]
    t = (np.einsum("ux,...yx->...yu", DCT_T, s) + 128) >> 8                 # rows
    f = (np.einsum("vy,...yu->...vu", DCT_T, t) + (1 << 17)) >> 18          # columns
    f = f.reshape(F, MH, MW, 6, 64)
    q = np.stack([lum] * 4 + [chr_] * 2)                                    # [6, 64]
    k = (np.abs(f) + (q >> 1)) // q
    k[..., 1:] = np.minimum(k[..., 1:], 1023)
    return (np.sign(f) * k)[..., ZIGZAG]


def _category(a):
    """Bits needed for a magnitude (0 for 0)."""
    a = np.asarray(a, dtype=np.int64)
    return sum((a >= (1 << k)).astype(np.int64) for k in range(11))


def _tokens(co):
    """Coefficients int64 [B, 6, 64] of a run of MCUs (one restart interval per leading index is the caller's business) ->
    (value, length) int64 [B, 6, 64, 5]: slot 3 of coefficient 0 = the DC code and amplitude, slots 0-2 of a non-zero AC
    coefficient = its ZRLs, slot 3 = its code and amplitude, slot 4 of coefficient 63 = EOB.  DC differences are the
    caller's: co[..., 0] holds them already."""
    B = co.shape[0]
    val = np.zeros((B, 6, 64, 5), dtype=np.int64)
    ln = np.zeros((B, 6, 64, 5), dtype=np.int64)
    is_chr = np.array([0, 0, 0, 0, 1, 1], dtype=np.int64)[None, :, None]
    cat = _category(np.abs(co))
    amp = np.where(co < 0, co - 1, co) & ((1 << cat) - 1)
    # DC
    dcode = np.where(is_chr[..., 0] == 1, _CODES["dc_chr"][0][cat[..., 0]], _CODES["dc_lum"][0][cat[..., 0]])
    dsize = np.where(is_chr[..., 0] == 1, _CODES["dc_chr"][1][cat[..., 0]], _CODES["dc_lum"][1][cat[..., 0]])
    val[..., 0, 3] = (dcode << cat[..., 0]) | amp[..., 0]
    ln[..., 0, 3] = dsize + cat[..., 0]
    # AC: the run of zeros in front of every non-zero coefficient
    idx = np.arange(64, dtype=np.int64)
    nz = co != 0
    nz[..., 0] = True                                                       # the DC position ends no run but starts the count
    last = np.maximum.accumulate(np.where(nz, idx, 0), axis=-1)
    prev = np.concatenate([np.zeros_like(last[..., :1]), last[..., :-1]], axis=-1)
    run = idx - prev - 1
    ac = nz.copy()
    ac[..., 0] = False
    sym = ((run & 15) << 4) | cat
    for name, sel in (("ac_lum", is_chr == 0), ("ac_chr", is_chr == 1)):
        code, size = _CODES[name]
        m = ac & sel
        val[..., 3] = np.where(m, (code[sym & 255] << cat) | amp, val[..., 3])
        ln[..., 3] = np.where(m, size[sym & 255] + cat, ln[..., 3])
        for z in range(3):
            mz = m & ((run >> 4) > z)
            val[..., z] = np.where(mz, code[0xF0], val[..., z])
            ln[..., z] = np.where(mz, size[0xF0], ln[..., z])
        eob = (last[..., 63] < 63) & sel[..., 0]
        val[..., 63, 4] = np.where(eob, code[0x00], val[..., 63, 4])
        ln[..., 63, 4] = np.where(eob, size[0x00], ln[..., 63, 4])
    return val, ln


def _frame_intervals(co):
    """The coefficients int64 [MH, MW, 6, 64] of one frame -> its MH restart intervals as u8 arrays: padded with 1-bits to a
    byte, 0x00 after every 0xFF, without markers."""
    MH, MW = co.shape[:2]
    co = co.copy()
    dc = co[..., 0]                                                          # [MH, MW, 6]
    order = dc[:, :, :4].reshape(MH, MW * 4)                                 # luminance in coding order
    dc[:, :, :4] = (order - np.concatenate([np.zeros((MH, 1), dtype=np.int64), order[:, :-1]], axis=1)).reshape(MH, MW, 4)
    for c in (4, 5):                                                         # a chrominance block follows its MCU's predecessor
        col = dc[:, :, c].copy()
        dc[:, 1:, c] = col[:, 1:] - col[:, :-1]
    val, ln = _tokens(co.reshape(MH * MW, 6, 64))
    val, ln = val.reshape(MH, -1), ln.reshape(MH, -1)
    out = []
    for r in range(MH):
        keep = ln[r] > 0
        v, n = val[r][keep], ln[r][keep]
        total = int(n.sum())
        pad = -total % 8
        if pad:
            v, n = np.append(v, (1 << pad) - 1), np.append(n, pad)
        k = np.arange(26, dtype=np.int64)[None, :]
        bits = ((v[:, None] >> np.maximum(n[:, None] - 1 - k, 0)) & 1).astype(np.uint8)
        data = np.packbits(bits[k < n[:, None]])
        ff = data == 255
        stuffed = np.repeat(data, 1 + ff.astype(np.int64))
        pos = np.cumsum(1 + ff.astype(np.int64)) - 1                        # where each byte's last copy landed
        stuffed[pos[ff]] = 0
        out.append(stuffed)
    return out


def encode_host(frames, quality=95, bgr=True):
    """The rule in numpy: u8 [F,H,W,3] -> (payload u8 [offsets[F]], offsets int64 [F+1]); frame f's entropy-coded data is
    payload[offsets[f]:offsets[f+1]] -- the bytes `ops.jpeg_encode` returns."""
    fr = np.asarray(frames)
    if fr.ndim != 4 or fr.shape[3] != 3 or fr.dtype != np.uint8:
        raise ValueError("frames must be u8 [F,H,W,3]")
    parts, offsets = [], [0]
    for f in range(fr.shape[0]):
        co = coefficients(fr[f:f + 1], quality, bgr)[0]
        rows = _frame_intervals(co)
        size = 0
        for r, data in enumerate(rows):
            parts.append(data)
            size += len(data)
            if r + 1 < len(rows):
                parts.append(np.array([0xFF, 0xD0 + (r & 7)], dtype=np.uint8))
                size += 2
        offsets.append(offsets[-1] + size)
    payload = np.concatenate(parts) if parts else np.zeros(0, dtype=np.uint8)
    return payload.astype(np.uint8), np.asarray(offsets, dtype=np.int64)


def encode_device(frames, quality=95, bgr=True):
    """`encode_host` through csrc/jpeg.hip: frames = a CUDA u8 tensor [F,H,W,3] (resident drawn frames) or a host array (one
    upload).  What comes back: the F + 1 offsets and one copy of exactly offsets[F] bytes."""
    import torch
    from . import ops
    if not torch.cuda.is_available():
        raise RuntimeError("no GPU: the encoder runs in csrc/jpeg.hip (encode_host is the numpy path)")
    if not isinstance(frames, torch.Tensor):
        host = np.ascontiguousarray(frames, dtype=np.uint8)
        host = host if host.flags.writeable else host.copy()             # (torch refuses to wrap read-only memory quietly)
        frames = torch.from_numpy(host).to(torch.device("cuda", torch.cuda.current_device()))
    payload, offsets = ops.jpeg_encode(frames, quality, bgr)
    return payload.cpu().numpy(), offsets.numpy()


def files(payload, offsets, H, W, quality=95):
    """-> one complete JPEG file per frame: header + its data + EOI."""
    head = header(H, W, quality)
    raw = np.asarray(payload, dtype=np.uint8).tobytes()
    return [head + raw[int(offsets[f]):int(offsets[f + 1])] + b"\xff\xd9" for f in range(len(offsets) - 1)]


# ---- decoding (THE RULE of `gom_jpeg_decode_*` in include/gomatching_hip.h; kernels: csrc/jpeg_decode.hip) -------------------
#     parse(data)                      -> JpegInfo | Refusal   the header, the tables and the restart segments of one file
#     decode_host(files, bgr)          -> u8 [F,H,W,3]         the rule in numpy; the entropy walk in plain Python
#     decode_device(files, bgr)        -> CUDA u8 [F,H,W,3]    the same through `ops.jpeg_decode`
# Pixels are byte-equal to Pillow's `Image.open(p).convert("RGB")` (libjpeg-turbo: islow IDCT, fancy upsampling) for every
# file `parse` accepts and whose status word is 0 (tests/test_jpeg_decode_cpu.py); everything else goes to Pillow.
STATUS_OK, STATUS_PAST_END, STATUS_BAD_CODE, STATUS_INDEX, STATUS_RST, STATUS_LEFT_OVER = 0, 1, 2, 3, 4, 5
DESC_WORDS = _ABI["GOM_JPEG_DECODE_DESC_WORDS"]            # int64 per segment: start, end, limit, first MCU, MCUs, frame, set, RSTn
SET_WORDS = _ABI["GOM_JPEG_DECODE_SET_WORDS"]              # int32 per table set
_HT_WORDS = 548                                            # one Huffman table: look[256], maxcode[18], valoff[18], huffval[256]
_SET_COMP = 4 * _HT_WORDS                                  # then dc table of component 0..3, ac table of component 0..3
_SET_QUANT = _SET_COMP + 8                                 # then the quantisation table of component 0..2, natural order
_SAMPLINGS = ((1, 1), (2, 1), (2, 2))
# jidctint.c: FIX(0.298631336) .. FIX(3.072711026) at CONST_BITS = 13
_F0298, _F0390, _F0541, _F0765, _F0899, _F1175 = 2446, 3196, 4433, 6270, 7373, 9633
_F1501, _F1847, _F1961, _F2053, _F2562, _F3072 = 12299, 15137, 16069, 16819, 20995, 25172


class Refusal:
    """What `parse` returns for a file the decoder does not take: Pillow reads it."""

    def __init__(self, reason):
        self.reason = reason

    def __repr__(self):
        return "Refusal(%r)" % (self.reason,)


class JpegInfo:
    """The header of an accepted file.  H, W; ncomp 1 or 3; (hs, vs) the luminance sampling; quant int32 [ncomp,64] in natural
    order; huff = {(class, id): (bits, vals)}; comp_dc / comp_ac = the table ids of every component; restart = MCUs per
    restart interval (0: none); scan = (first, end) byte range of the entropy-coded segment; seg_start / seg_end int64 = the
    byte range of every restart segment found in it (markers excluded)."""
    __slots__ = ("H", "W", "ncomp", "hs", "vs", "quant", "huff", "comp_dc", "comp_ac", "restart", "scan", "seg_start", "seg_end")

    @property
    def mcus(self):
        return ((self.H + 8 * self.vs - 1) // (8 * self.vs)) * ((self.W + 8 * self.hs - 1) // (8 * self.hs))

    @property
    def key(self):
        return (self.H, self.W, self.ncomp, self.hs, self.vs)


class _Short(Exception):
    pass


def parse(data):
    """One file's bytes -> JpegInfo, or Refusal(reason) for anything outside the accepted set of the rule."""
    try:
        return _parse(bytes(data))
    except _Short:
        return Refusal("truncated header")


def _parse(data):
    n = len(data)

    def need(a, b):
        if b > n:
            raise _Short()
        return data[a:b]

    if need(0, 2) != b"\xff\xd8":
        return Refusal("not a JPEG file (no SOI)")
    pos = 2
    info = JpegInfo()
    quant, huff = {}, {}
    frame = None
    jfif, adobe = False, None
    info.restart = 0
    while True:
        if need(pos, pos + 1)[0] != 0xFF:
            return Refusal("marker expected at byte %d" % pos)
        while need(pos + 1, pos + 2)[0] == 0xFF:           # fill bytes
            pos += 1
        m = data[pos + 1]
        pos += 2
        if m == 0xD8 or 0xD0 <= m <= 0xD7 or m == 0x01:
            continue
        if m == 0xD9:
            return Refusal("no scan before EOI")
        ln = int.from_bytes(need(pos, pos + 2), "big")
        if ln < 2:
            return Refusal("segment length below 2")
        seg = need(pos + 2, pos + ln)
        pos += ln
        if m == 0xC0:
            if frame is not None:
                return Refusal("two frame headers")
            if len(seg) < 6 or len(seg) != 6 + 3 * seg[5]:
                return Refusal("malformed SOF0")
            if seg[0] != 8:
                return Refusal("%d-bit samples" % seg[0])
            frame = (int.from_bytes(seg[1:3], "big"), int.from_bytes(seg[3:5], "big"),
                     [(seg[6 + 3 * i], seg[7 + 3 * i] >> 4, seg[7 + 3 * i] & 15, seg[8 + 3 * i]) for i in range(seg[5])])
        elif m in (0xC1, 0xC2, 0xC3, 0xC5, 0xC6, 0xC7, 0xC9, 0xCA, 0xCB, 0xCD, 0xCE, 0xCF, 0xCC):
            return Refusal({0xC1: "extended sequential coding", 0xC2: "progressive coding"}.get(
                m, "arithmetic coding" if m >= 0xC9 else "lossless or hierarchical coding"))
        elif m == 0xC4:
            p = 0
            while p < len(seg):
                if p + 17 > len(seg):
                    return Refusal("malformed DHT")
                tc, th = seg[p] >> 4, seg[p] & 15
                bits = list(seg[p + 1:p + 17])
                cnt = sum(bits)
                if tc > 1 or th > 1 or cnt > 256 or p + 17 + cnt > len(seg):
                    return Refusal("malformed DHT (class %d, id %d, %d codes)" % (tc, th, cnt))
                vals = list(seg[p + 17:p + 17 + cnt])
                code = 0
                for length in range(1, 17):                # Annex C: the codes of a length must fit that length
                    code = (code + bits[length - 1]) << 1
                    if code > (1 << (length + 1)):
                        return Refusal("malformed DHT (over-subscribed code)")
                if tc == 0 and any(v > 11 for v in vals):
                    return Refusal("malformed DHT (DC category above 11)")
                huff[(tc, th)] = (bits, vals)
                p += 17 + cnt
        elif m == 0xDB:
            p = 0
            while p < len(seg):
                if seg[p] >> 4:
                    return Refusal("16-bit quantisation table")
                if (seg[p] & 15) > 3 or p + 65 > len(seg):
                    return Refusal("malformed DQT")
                t = np.zeros(64, dtype=np.int32)
                t[ZIGZAG] = np.frombuffer(seg[p + 1:p + 65], dtype=np.uint8)
                quant[seg[p] & 15] = t
                p += 65
        elif m == 0xDD:
            if len(seg) != 2:
                return Refusal("malformed DRI")
            info.restart = int.from_bytes(seg, "big")
        elif m == 0xE0:
            jfif = jfif or seg[:5] == b"JFIF\x00"
        elif m == 0xEE:
            if seg[:5] == b"Adobe" and len(seg) >= 12:
                adobe = seg[11]
        elif m == 0xDC:
            return Refusal("DNL")
        elif m == 0xDA:
            break
        # every other segment (APPn, COM) is skipped
    if frame is None:
        return Refusal("scan without a frame header")
    H, W, comps = frame
    if H == 0:
        return Refusal("DNL (height 0 in the frame header)")
    if W < 1 or W > MAX_WIDTH:
        return Refusal("width %d outside 1 .. %d" % (W, MAX_WIDTH))
    if len(comps) not in (1, 3):
        return Refusal("%d components (CMYK / YCCK)" % len(comps))
    if len(comps) == 3:
        if adobe is not None and adobe != 1:
            return Refusal("Adobe transform %d" % adobe)
        if not jfif and adobe is None and [c[0] for c in comps] != [1, 2, 3]:
            return Refusal("three components that are not Y Cb Cr")
        if (comps[0][1], comps[0][2]) not in _SAMPLINGS or any((c[1], c[2]) != (1, 1) for c in comps[1:]):
            return Refusal("sampling " + " ".join("%dx%d" % (c[1], c[2]) for c in comps))
    elif (comps[0][1], comps[0][2]) != (1, 1):
        return Refusal("sampling %dx%d of a single component" % (comps[0][1], comps[0][2]))
    if len(seg) < 1 or len(seg) != 4 + 2 * seg[0]:
        return Refusal("malformed SOS")
    if seg[0] != len(comps):
        return Refusal("several scans")
    if tuple(seg[-3:]) != (0, 63, 0):
        return Refusal("a scan that is not Ss 0, Se 63, Ah Al 0")
    info.comp_dc, info.comp_ac = [], []
    for i, c in enumerate(comps):
        if seg[1 + 2 * i] != c[0]:
            return Refusal("scan components out of order")
        td, ta = seg[2 + 2 * i] >> 4, seg[2 + 2 * i] & 15
        if (0, td) not in huff or (1, ta) not in huff or c[3] not in quant:
            return Refusal("a missing table")
        info.comp_dc.append(td)
        info.comp_ac.append(ta)
    info.H, info.W, info.ncomp, info.hs, info.vs = H, W, len(comps), comps[0][1], comps[0][2]
    info.quant = np.stack([quant[c[3]] for c in comps])
    info.huff = huff
    # the entropy-coded segment ends at the first marker that is neither a stuffed 0xFF nor RSTn
    a = np.frombuffer(data, dtype=np.uint8)[pos:]
    ff = np.flatnonzero(a[:-1] == 0xFF) if len(a) > 1 else np.zeros(0, dtype=np.int64)
    nxt = a[ff + 1]
    other = ff[(nxt != 0) & ((nxt < 0xD0) | (nxt > 0xD7)) & (nxt != 0xFF)]
    end = int(other[0]) if len(other) else len(a)
    if len(other) and a[end + 1] != 0xD9:
        return Refusal("DNL" if a[end + 1] == 0xDC else "several scans")
    rst = ff[(nxt >= 0xD0) & (nxt <= 0xD7) & (ff < end)]
    info.scan = (pos, pos + end)
    info.seg_start = np.concatenate([[0], rst + 2]).astype(np.int64) + pos
    info.seg_end = np.concatenate([rst, [end]]).astype(np.int64) + pos
    return info


def _huff_words(bits, vals):
    """A Huffman table for the walk: look[c] = length << 8 | symbol for the 8-bit prefixes c of codes of at most 8 bits (0: a
    longer code or none); maxcode[l] = the largest code of length l or -1 (maxcode[17] ends every search); valoff[l] = the
    index of the length's first symbol minus its first code."""
    out = np.zeros(_HT_WORDS, dtype=np.int32)
    look, maxcode, valoff, huffval = out[:256], out[256:274], out[274:292], out[292:]
    maxcode[:] = -1
    huffval[:len(vals)] = vals
    code, k = 0, 0
    for length in range(1, 17):
        nl = bits[length - 1]
        if nl:
            valoff[length] = k - code
            for i in range(nl):
                if length <= 8:
                    look[(code + i) << (8 - length):(code + i + 1) << (8 - length)] = (length << 8) | vals[k + i]
            code += nl
            k += nl
            maxcode[length] = code - 1
        code <<= 1
    return out


def _table_set(info):
    out = np.zeros(SET_WORDS, dtype=np.int32)
    for t, key in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
        out[t * _HT_WORDS:(t + 1) * _HT_WORDS] = _huff_words(*info.huff[key]) if key in info.huff else _huff_words([0] * 16, [])
    out[_SET_COMP:_SET_COMP + info.ncomp] = info.comp_dc
    out[_SET_COMP + 4:_SET_COMP + 4 + info.ncomp] = [2 + t for t in info.comp_ac]
    out[_SET_QUANT:_SET_QUANT + 64 * info.ncomp] = info.quant.reshape(-1)
    return out


class DecodePlan:
    """What one decode call uploads: `data` u8 the files' entropy bytes, packed; `desc` int64 [nseg, DESC_WORDS]; `seg_off` int32
    [F+1] the segments of every frame; `sets` int32 [nsets, SET_WORDS] the distinct table sets; `frame_set` int32 [F]; and the
    geometry (H, W, ncomp, hs, vs) all files share."""
    __slots__ = ("data", "desc", "seg_off", "sets", "frame_set", "H", "W", "ncomp", "hs", "vs", "F")


def plan(files, infos=None):
    """Files (bytes) of one geometry -> DecodePlan.  A file `parse` refuses, or one of another geometry, is a ValueError: the
    caller sends refused files to Pillow and groups the rest by `JpegInfo.key`."""
    infos = [parse(f) for f in files] if infos is None else list(infos)
    for i, inf in enumerate(infos):
        if isinstance(inf, Refusal):
            raise ValueError("file %d is refused: %s" % (i, inf.reason))
        if inf.key != infos[0].key:
            raise ValueError("file %d is %r, file 0 is %r (H, W, components, sampling): group the files first" % (i, inf.key, infos[0].key))
    p = DecodePlan()
    p.F = len(infos)
    if p.F:
        p.H, p.W, p.ncomp, p.hs, p.vs = infos[0].key
    parts, desc, seg_off, sets, frame_set, at = [], [], [0], {}, [], 0
    for f, (raw, inf) in enumerate(zip(files, infos)):
        a, b = inf.scan
        parts.append(np.frombuffer(raw, dtype=np.uint8)[a:b])
        words = _table_set(inf)
        frame_set.append(sets.setdefault(words.tobytes(), len(sets)))
        total = inf.mcus
        ri = inf.restart if inf.restart else total
        nseg = (total + ri - 1) // ri
        found = len(inf.seg_start)
        for s in range(nseg):                               # a segment the scan for RSTn did not find is empty, at the end
            s0, s1 = (int(inf.seg_start[s]), int(inf.seg_end[s])) if s < found else (b, b)
            desc.append([at + s0 - a, at + s1 - a, at + b - a, s * ri, min(ri, total - s * ri), f, frame_set[-1],
                         0xD0 + (s & 7) if s + 1 < nseg else 0])
        seg_off.append(len(desc))
        at += b - a
    p.data = np.concatenate(parts) if parts else np.zeros(0, dtype=np.uint8)
    p.desc = np.asarray(desc, dtype=np.int64).reshape(-1, DESC_WORDS)
    p.seg_off = np.asarray(seg_off, dtype=np.int32)
    by_index = sorted(sets.items(), key=lambda kv: kv[1])
    p.sets = np.stack([np.frombuffer(k, dtype=np.int32) for k, _ in by_index]) if by_index else np.zeros((0, SET_WORDS), np.int32)
    p.frame_set = np.asarray(frame_set, dtype=np.int32)
    return p


def geometry(H, W, ncomp, hs, vs):
    """-> (MH, MW, [(block rows, block columns) per component], [first block of every component], blocks per frame)."""
    MH, MW = (H + 8 * vs - 1) // (8 * vs), (W + 8 * hs - 1) // (8 * hs)
    grids = [(MH * vs, MW * hs)] + [(MH, MW)] * (ncomp - 1)
    first = [0]
    for g in grids:
        first.append(first[-1] + g[0] * g[1])
    return MH, MW, grids, first[:-1], first[-1]


def _walk_segment(data, d, tabs, geo, ncomp, hs, vs, coef):
    """csrc/jpeg_decode_core.h `gom_jd_walk_segment` in plain Python: the same reads, the same checks, the same status.
    coef int16 [blocks, 64] of the segment's frame."""
    MH, MW, grids, first, _ = geo
    n = len(data)
    start = min(max(int(d[0]), 0), n)
    end = min(max(int(d[1]), start), n)
    limit = min(max(int(d[2]), end), n)
    pos, acc, nbits, fake = start, 0, 0, 0
    status = STATUS_OK
    pred = [0, 0, 0]
    total = MH * MW
    m0, cnt = int(d[3]), int(d[4])

    def fill():
        nonlocal pos, acc, nbits, fake
        while nbits <= 24:
            b = 0
            if pos < end and not (data[pos] == 0xFF and not (pos + 1 < end and data[pos + 1] == 0)):
                b = int(data[pos])
                pos += 2 if b == 0xFF else 1
            else:
                fake += 8
            acc = ((acc << 8) | b) & 0xFFFFFFFFFFFFFFFF
            nbits += 8

    def take(k):
        nonlocal nbits, status
        v = (acc >> (nbits - k)) & ((1 << k) - 1)
        nbits -= k
        if nbits < fake and status == STATUS_OK:
            status = STATUS_PAST_END
        return v

    def symbol(t):
        nonlocal status
        fill()
        base = t * _HT_WORDS
        e = int(tabs[base + ((acc >> (nbits - 8)) & 255)])
        if e:
            take(e >> 8)
            return e & 255
        for length in range(9, 17):
            code = (acc >> (nbits - length)) & ((1 << length) - 1)
            if code <= int(tabs[base + 256 + length]):
                take(length)
                return int(tabs[base + 292 + ((code + int(tabs[base + 274 + length])) & 255)])
        if status == STATUS_OK:
            status = STATUS_BAD_CODE
        return 0

    def receive(s):
        if s == 0:
            return 0
        fill()
        v = take(s)
        return v if v >> (s - 1) else v - (1 << s) + 1

    if m0 < 0 or cnt < 0 or m0 + cnt > total:
        return STATUS_PAST_END
    for m in range(m0, m0 + cnt):
        my, mx = divmod(m, MW)
        for c in range(ncomp):
            h, v = (hs, vs) if c == 0 else (1, 1)
            for by in range(v):
                for bx in range(h):
                    if status != STATUS_OK:
                        continue                            # (the block stays zero)
                    blk = first[c] + (my * v + by) * grids[c][1] + mx * h + bx
                    s = symbol(int(tabs[_SET_COMP + c]))
                    if status == STATUS_OK and s > 11:
                        status = STATUS_BAD_CODE
                    diff = receive(s) if status == STATUS_OK else 0
                    if status != STATUS_OK:
                        continue
                    pred[c] += diff
                    coef[blk, 0] = ((pred[c] + 32768) & 65535) - 32768
                    k = 1
                    while k < 64 and status == STATUS_OK:
                        rs = symbol(int(tabs[_SET_COMP + 4 + c]))
                        if status != STATUS_OK:
                            break
                        r, s = rs >> 4, rs & 15
                        if s:
                            k += r
                            if k > 63:
                                status = STATUS_INDEX
                                break
                            val = receive(s)
                            if status != STATUS_OK:
                                break
                            coef[blk, ZIGZAG[k]] = val
                            k += 1
                        elif r == 15:
                            k += 16
                            if k > 63:
                                status = STATUS_INDEX
                        else:
                            break
    if status != STATUS_OK:
        return status
    rst = int(d[7])
    if nbits - fake >= 8 or pos < end:                      # whole bytes the walk never needed (those read ahead included)
        return STATUS_LEFT_OVER
    if rst:
        if not (end + 2 <= limit and data[end] == 0xFF and data[end + 1] == rst):
            return STATUS_RST
    elif end != limit:
        return STATUS_RST
    return STATUS_OK


def _idct_1d(d, shift):
    """jidctint.c's one-dimensional pass over eight int64 arrays: (even part, odd part, butterflies) descaled by `shift`."""
    z1 = (d[2] + d[6]) * _F0541
    t2 = z1 - d[6] * _F1847
    t3 = z1 + d[2] * _F0765
    t0 = (d[0] + d[4]) << 13
    t1 = (d[0] - d[4]) << 13
    e0, e3, e1, e2 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    o0, o1, o2, o3 = d[7], d[5], d[3], d[1]
    z1, z2, z3, z4 = o0 + o3, o1 + o2, o0 + o2, o1 + o3
    z5 = (z3 + z4) * _F1175
    o0, o1, o2, o3 = o0 * _F0298, o1 * _F2053, o2 * _F3072, o3 * _F1501
    z1, z2, z3, z4 = -z1 * _F0899, -z2 * _F2562, -z3 * _F1961 + z5, -z4 * _F0390 + z5
    o0, o1, o2, o3 = o0 + z1 + z3, o1 + z2 + z4, o2 + z2 + z3, o3 + z1 + z4
    r = 1 << (shift - 1)
    return [(e0 + o3 + r) >> shift, (e1 + o2 + r) >> shift, (e2 + o1 + r) >> shift, (e3 + o0 + r) >> shift,
            (e3 - o0 + r) >> shift, (e2 - o1 + r) >> shift, (e1 - o2 + r) >> shift, (e0 - o3 + r) >> shift]


def idct_blocks(coef, q):
    """int16 [N,64] natural order, q int [64] -> u8 [N,8,8]: dequantise, columns (descale 11), rows (descale 18), + 128, clamp."""
    d = (coef.astype(np.int64) * np.asarray(q, dtype=np.int64)[None]).reshape(-1, 8, 8)
    ws = np.stack(_idct_1d([d[:, r, :] for r in range(8)], 11), axis=1)          # [N, row, col]
    out = np.stack(_idct_1d([ws[:, :, c] for c in range(8)], 18), axis=2)
    return np.clip(out + 128, 0, 255).astype(np.uint8)


def planes_of(coef, quant, geo, H, W, ncomp, hs, vs):
    """The coefficients of one frame -> its component planes u8, each the size of its padded block grid."""
    _, _, grids, first, _ = geo
    out = []
    for c in range(ncomp):
        bh, bw = grids[c]
        px = idct_blocks(coef[first[c]:first[c] + bh * bw], quant[c])
        out.append(px.reshape(bh, bw, 8, 8).transpose(0, 2, 1, 3).reshape(bh * 8, bw * 8))
    return out


def _upsample(c, H, W, hs, vs):
    """jdsample.c: a chrominance plane (padded grid) -> int64 [H, W].  Fancy (triangle) when the component is more than two
    samples wide, else replication; the neighbour that a picture edge lacks is the nearest sample of the ch x cw real ones."""
    ch, cw = (H + vs - 1) // vs, (W + hs - 1) // hs
    c = c[:ch, :cw].astype(np.int64)
    if hs == 1:
        return c[:H, :W]
    x = np.arange(W)
    cx = x >> 1
    if cw <= 2:
        return c[(np.arange(H) >> 1) if vs == 2 else np.arange(H)][:, cx]
    side = np.where(x & 1, np.minimum(cx + 1, cw - 1), np.maximum(cx - 1, 0))
    if vs == 1:
        return (3 * c[:, cx] + c[:, side] + np.where(x & 1, 2, 1)[None]) >> 2
    y = np.arange(H)
    cy = y >> 1
    near = np.where(y & 1, np.minimum(cy + 1, ch - 1), np.maximum(cy - 1, 0))
    col = 3 * c[cy] + c[near]                                                # [H, cw]
    return (3 * col[:, cx] + col[:, side] + np.where(x & 1, 7, 8)[None]) >> 4


def pixels_of(planes, H, W, ncomp, hs, vs, bgr):
    """Component planes -> u8 [H,W,3]: upsampling and jdcolor.c's 16-bit fixed-point Y Cb Cr -> R G B."""
    y = planes[0][:H, :W].astype(np.int64)
    if ncomp == 1:
        return np.repeat(y.astype(np.uint8)[:, :, None], 3, axis=2)
    cb, cr = (_upsample(p, H, W, hs, vs) - 128 for p in planes[1:])
    r = y + ((91881 * cr + 32768) >> 16)
    g = y + ((-22554 * cb - 46802 * cr + 32768) >> 16)
    b = y + ((116130 * cb + 32768) >> 16)
    return np.clip(np.stack([b, g, r] if bgr else [r, g, b], axis=2), 0, 255).astype(np.uint8)


def decode_host(files, bgr=True, return_status=False, return_coefficients=False):
    """The rule in numpy (the entropy walk in plain Python): files (bytes) of one geometry -> u8 [F,H,W,3], B G R or R G B.
    return_status: also int32 [F], the per-frame status word (0 = clean; the pixels of a flagged frame are whatever the walk
    left and Pillow reads that file).  A refused file is a ValueError."""
    p = plan(files)
    if p.F == 0:
        raise ValueError("no files")
    geo = geometry(p.H, p.W, p.ncomp, p.hs, p.vs)
    out = np.zeros((p.F, p.H, p.W, 3), dtype=np.uint8)
    status = np.zeros(p.F, dtype=np.int32)
    coefs = np.zeros((p.F, geo[4], 64), dtype=np.int16)
    for f in range(p.F):
        tabs = p.sets[p.frame_set[f]]
        for s in range(p.seg_off[f], p.seg_off[f + 1]):
            st = _walk_segment(p.data, p.desc[s], tabs, geo, p.ncomp, p.hs, p.vs, coefs[f])
            if st and not status[f]:
                status[f] = st
        quant = tabs[_SET_QUANT:_SET_QUANT + 64 * p.ncomp].reshape(p.ncomp, 64)
        out[f] = pixels_of(planes_of(coefs[f], quant, geo, p.H, p.W, p.ncomp, p.hs, p.vs), p.H, p.W, p.ncomp, p.hs, p.vs, bgr)
    res = (out,) + ((status,) if return_status else ()) + ((coefs,) if return_coefficients else ())
    return res if len(res) > 1 else out


def resolve_walk(walk, plan):
    """The entropy walk of one decode call: "segments" and "chunks" stand; "auto" gives "chunks" when the plan's segments are
    at least AUTO_SEGMENT_BYTES long in the mean (files without restart markers: one segment each), else "segments".  Pure."""
    if walk not in WALKS:
        raise ValueError("walk must be one of %s, not %r" % (", ".join(WALKS), walk))
    if walk != "auto":
        return walk
    nseg = int(plan.desc.shape[0])
    mean = float((plan.desc[:, 1] - plan.desc[:, 0]).sum()) / nseg if nseg else 0.0
    return "chunks" if mean >= AUTO_SEGMENT_BYTES else "segments"


def decode_device(files, bgr=True, return_status=False, walk="segments", chunk_bytes=None):
    """`decode_host` through csrc/jpeg_decode.hip: three uploads (bytes, descriptors, table sets), the pixels stay on the
    device.  -> CUDA u8 [F,H,W,3] (and the status words as a host int32 array).  walk: "segments", "chunks" (with
    `chunk_bytes`, None = CHUNK_BYTES) or "auto" (`resolve_walk`): `ops.jpeg_decode`'s, the same pixels either way."""
    if walk not in WALKS:
        raise ValueError("walk must be one of %s, not %r" % (", ".join(WALKS), walk))
    if walk == "segments" and chunk_bytes is not None:
        raise ValueError("chunk_bytes belongs to walk=\"chunks\" (or \"auto\", where it counts when the chunk walk is taken)")
    import torch
    from . import ops
    if not torch.cuda.is_available():
        raise RuntimeError("no GPU: the decoder runs in csrc/jpeg_decode.hip (decode_host is the numpy path)")
    p = plan(files)
    walk = resolve_walk(walk, p)
    out, status = ops.jpeg_decode(p, bgr, walk=walk, chunk_bytes=chunk_bytes if walk == "chunks" else None)
    return (out, status.cpu().numpy()) if return_status else out
