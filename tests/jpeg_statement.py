"""Baseline JPEG encoding of a frame, stated per pixel, per block and per bit in plain Python integers (not collected: no
test_ prefix).

What csrc/jpeg.hip and `jpeg.encode_host` are held to, byte for byte -- the rule of `gom_jpeg_encode_*` in
include/gomatching_hip.h:

  ycc              JFIF's full-range matrix in 16-bit fixed point
  mcu_blocks       the 16 x 16 pixels of an MCU (last column and row replicated) -> Y00 Y01 Y10 Y11 Cb Cr, level-shifted;
                   chrominance = the mean of each 2 x 2 block, (a + b + c + d + 2) >> 2
  fdct             rows then columns on the integer table T (built here from its definition, round(8192 a(u) cos(..)), and
                   compared with the printed one by the test), (s + 128) >> 8 then (s + 2^17) >> 18, floor shifts
  quantise         sign(f) ((|f| + (q >> 1)) // q), AC clamped to +-1023; tables: Annex K scaled by the quality rule
  BitWriter        codes most significant bit first, 1-bits to the byte at the end of an interval, 0x00 after 0xFF
  encode_statement the file: header, per MCU row one restart interval (predictors reset), RSTn between them, EOI

and the cases the CPU and the GPU tests share.
"""
import functools
import math

import numpy as np

Q_LUM = [16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
         18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112,
         100, 103, 99]
Q_CHR = [17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99] \
    + [99] * 32


def zigzag():
    """Natural indices in zigzag order, walked: up-right on even diagonals, down-left on odd ones."""
    out = []
    for d in range(15):
        cells = [(y, d - y) for y in range(8) if 0 <= d - y < 8]                # (row, column), row ascending
        out += [8 * y + x for y, x in (cells if d % 2 else cells[::-1])]
    return out


def dct_table():
    """T[u][x] = round(8192 a(u) cos((2 x + 1) u pi / 16)) -- floating point makes the TABLE, never a coefficient."""
    return [[int(round(8192 * (math.sqrt(0.125) if u == 0 else 0.5) * math.cos((2 * x + 1) * u * math.pi / 16))) for x in range(8)]
            for u in range(8)]


def quant_table(base, quality):
    scale = 5000 // quality if quality < 50 else 200 - 2 * quality
    return [min(max((b * scale + 50) // 100, 1), 255) for b in base]


def ycc(r, g, b):
    return ((19595 * r + 38470 * g + 7471 * b + 32768) >> 16,
            (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16,
            (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16)


def mcu_blocks(frame, my, mx, bgr):
    """-> six lists of 64 level-shifted samples (row-major)."""
    H, W = len(frame), len(frame[0])
    Y = [[0] * 16 for _ in range(16)]
    Cb = [[0] * 16 for _ in range(16)]
    Cr = [[0] * 16 for _ in range(16)]
    for y in range(16):
        for x in range(16):
            p = frame[min(16 * my + y, H - 1)][min(16 * mx + x, W - 1)]
            r, g, b = (p[2], p[1], p[0]) if bgr else (p[0], p[1], p[2])
            Y[y][x], Cb[y][x], Cr[y][x] = ycc(int(r), int(g), int(b))
    blocks = [[Y[8 * by + y][8 * bx + x] - 128 for y in range(8) for x in range(8)] for by in range(2) for bx in range(2)]
    for C in (Cb, Cr):
        blocks.append([((C[2 * y][2 * x] + C[2 * y][2 * x + 1] + C[2 * y + 1][2 * x] + C[2 * y + 1][2 * x + 1] + 2) >> 2) - 128
                       for y in range(8) for x in range(8)])
    return blocks


def fdct(s, T):
    t = [[(sum(T[u][x] * s[8 * y + x] for x in range(8)) + 128) >> 8 for u in range(8)] for y in range(8)]
    return [(sum(T[v][y] * t[y][u] for y in range(8)) + (1 << 17)) >> 18 for v in range(8) for u in range(8)]


def quantise(f, q):
    out = []
    for i in range(64):
        k = (abs(f[i]) + (q[i] >> 1)) // q[i]
        if i > 0:
            k = min(k, 1023)
        out.append(-k if f[i] < 0 else k)
    return out


def huff_codes(bits, vals):
    """Annex C -> {symbol: (code, length)}."""
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[vals[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return out


class BitWriter:
    def __init__(self):
        self.bits = []

    def put(self, value, n):
        for k in range(n - 1, -1, -1):
            self.bits.append((value >> k) & 1)

    def interval(self):
        """The bits written so far as the bytes of a finished interval."""
        bits = self.bits + [1] * (-len(self.bits) % 8)
        out = bytearray()
        for i in range(0, len(bits), 8):
            byte = 0
            for b in bits[i:i + 8]:
                byte = 2 * byte + b
            out.append(byte)
            if byte == 0xFF:
                out.append(0)
        return bytes(out)


def _amplitude(w, v):
    """-> the category of v; its low bits (v, or v - 1 when negative) are written."""
    cat = abs(v).bit_length()
    return cat, (v if v >= 0 else v - 1) & ((1 << cat) - 1)


def encode_block(w, zz, pred, dc_codes, ac_codes):
    cat, amp = _amplitude(w, zz[0] - pred)
    w.put(*dc_codes[cat])
    w.put(amp, cat)
    run = 0
    for k in range(1, 64):
        if zz[k] == 0:
            run += 1
            continue
        while run > 15:
            w.put(*ac_codes[0xF0])
            run -= 16
        cat, amp = _amplitude(w, zz[k])
        w.put(*ac_codes[(run << 4) | cat])
        w.put(amp, cat)
        run = 0
    if run > 0:
        w.put(*ac_codes[0x00])


def header_statement(H, W, quality, huff):
    def u16(v):
        return bytes([v >> 8, v & 255])
    zz = zigzag()
    out = b"\xff\xd8" + b"\xff\xe0" + u16(16) + b"JFIF\x00" + bytes([1, 1, 0]) + u16(1) + u16(1) + bytes([0, 0])
    for i, base in enumerate((Q_LUM, Q_CHR)):
        q = quant_table(base, quality)
        out += b"\xff\xdb" + u16(67) + bytes([i]) + bytes(q[n] for n in zz)
    out += b"\xff\xc0" + u16(17) + bytes([8]) + u16(H) + u16(W) + bytes([3, 1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1])
    for tc, name in ((0x00, "dc_lum"), (0x10, "ac_lum"), (0x01, "dc_chr"), (0x11, "ac_chr")):
        bits, vals = huff[name]
        out += b"\xff\xc4" + u16(19 + len(vals)) + bytes([tc]) + bytes(bits) + bytes(vals)
    out += b"\xff\xdd" + u16(4) + u16((W + 15) // 16)
    out += b"\xff\xda" + u16(12) + bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0])
    return out


def encode_statement(frame, quality, bgr):
    """One frame u8 [H,W,3] -> the bytes of its file.  The Huffman tables (BITS, HUFFVAL) are data: `jpeg.HUFF`, checked
    against the tables of Pillow's own files by the test."""
    from gomatching_amd import jpeg
    frame = np.asarray(frame, dtype=np.uint8).tolist()
    H, W = len(frame), len(frame[0])
    MH, MW = (H + 15) // 16, (W + 15) // 16
    T, zz = dct_table(), zigzag()
    ql, qc = quant_table(Q_LUM, quality), quant_table(Q_CHR, quality)
    codes = {name: huff_codes(*t) for name, t in jpeg.HUFF.items()}
    out = header_statement(H, W, quality, jpeg.HUFF)
    for my in range(MH):
        w = BitWriter()
        pred = [0, 0, 0]
        for mx in range(MW):
            for b, s in enumerate(mcu_blocks(frame, my, mx, bgr)):
                comp = 0 if b < 4 else b - 3
                q = quantise(fdct(s, T), ql if comp == 0 else qc)
                z = [q[n] for n in zz]
                encode_block(w, z, pred[comp], codes["dc_lum" if comp == 0 else "dc_chr"], codes["ac_lum" if comp == 0 else "ac_chr"])
                pred[comp] = z[0]
        out += w.interval()
        if my + 1 < MH:
            out += bytes([0xFF, 0xD0 + (my & 7)])
    return out + b"\xff\xd9"


# ------------------------------------------------------------------------------------------ shared cases
def _noise(H, W, seed, F=None):
    rng = np.random.RandomState(seed)
    return rng.randint(0, 256, ((F or 1), H, W, 3)).astype(np.uint8)


def _flat():
    return np.full((1, 16, 32, 3), (200, 30, 90), dtype=np.uint8)


def _checker():
    """A one-pixel checkerboard of black and white: the largest coefficient sits last in zigzag order (long codes, top
    categories at q = 100)."""
    yy, xx = np.mgrid[0:16, 0:16]
    return np.repeat((((yy + xx) & 1) * 255).astype(np.uint8)[None, :, :, None], 3, axis=3)


def _zrl():
    """Grey 8 x 16: the left block is the horizontal basis function of frequency 7 (its coefficient is number 28 in zigzag
    order, behind a run of more than 15 zeros: one ZRL), the right block the basis function (7, 7) (coefficient 63 behind a
    run of 62 zeros: three ZRLs and no EOB).  The test checks those runs on the coefficients."""
    c7 = [math.cos((2 * x + 1) * 7 * math.pi / 16) for x in range(8)]
    img = np.full((1, 8, 16, 3), 128, dtype=np.uint8)
    for y in range(8):
        for x in range(8):
            img[0, y, x] = 128 + int(round(100 * c7[x]))
            img[0, y, 8 + x] = 128 + int(round(120 * c7[x] * c7[y]))
    return img


FF_SEED = 10                                                              # what `search_ff` returns


def _ff():
    """Noise whose entropy data holds several 0xFF bytes, one of them the last byte of the first restart interval (found by
    `search_ff`, a search over seeds with the numpy path)."""
    return _noise(32, 16, FF_SEED)


def search_ff(limit=100000):
    """The first seed whose 16 x 32 noise, at q = 100 in B, G, R order, ends its first interval on a 0xFF byte and holds at
    least three 0xFF bytes."""
    from gomatching_amd import jpeg
    for seed in range(limit):
        payload, _ = jpeg.encode_host(_noise(32, 16, seed), 100, True)
        data = payload.tobytes()
        if b"\xff\x00\xff\xd0" in data and data.count(b"\xff\x00") >= 3:
            return seed
    raise RuntimeError("no seed found")


# name -> (frames u8 [F,H,W,3] maker, quality, bgr)
CASES = {
    "8x8": (lambda: _noise(8, 8, 1), 95, True),
    "16x16": (lambda: _noise(16, 16, 2), 95, True),
    "17x23": (lambda: _noise(23, 17, 3), 95, True),
    "33x47": (lambda: _noise(47, 33, 4), 95, True),
    "1x1": (lambda: _noise(1, 1, 5), 95, True),
    "flat": (_flat, 95, True),
    "checker_q100": (_checker, 100, True),
    "zrl": (_zrl, 90, True),
    "ff": (_ff, 100, True),
    "nine_rows": (lambda: _noise(9 * 16 + 3, 16, 6), 50, True),
    "three_frames": (lambda: _noise(20, 24, 7, F=3), 95, True),
    "q1": (lambda: _noise(16, 32, 8), 1, True),
    "q50": (lambda: _noise(16, 32, 8), 50, True),
    "q100": (lambda: _noise(16, 32, 8), 100, True),
    "rgb": (lambda: _noise(23, 17, 3), 95, False),
}


@functools.lru_cache(maxsize=None)
def case(name):
    """-> (frames, quality, bgr, the statement's files: one `bytes` per frame), computed once and shared (never modified)."""
    make, quality, bgr = CASES[name]
    frames = make()
    want = tuple(encode_statement(f, quality, bgr) for f in frames)
    frames.setflags(write=False)
    return frames, quality, bgr, want
