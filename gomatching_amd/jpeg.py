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
"""
import numpy as np

from .lib import CONSTANTS as _ABI

MAX_WIDTH = _ABI["GOM_JPEG_MAX_WIDTH"]
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
