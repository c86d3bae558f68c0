"""THE RULE of `gom_jpeg_decode_*` (include/gomatching_hip.h) stated per bit and per sample in plain Python: no numpy in the
arithmetic, no table-driven shortcuts, nothing shared with gomatching_amd/jpeg.py.  `decode(data, bgr)` -> nested lists
[H][W][3] of a clean file of the accepted set; anything else is an AssertionError.  tests/test_jpeg_decode_cpu.py holds
`jpeg.decode_host` to it byte for byte."""

ZIGZAG = [0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42,
          49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63]


def _u16(d, p):
    return (d[p] << 8) | d[p + 1]


def _header(d):
    assert d[0] == 0xFF and d[1] == 0xD8
    p = 2
    quant, codes, ri = {}, {}, 0
    while True:
        assert d[p] == 0xFF
        m = d[p + 1]
        n = _u16(d, p + 2)
        seg = d[p + 4:p + 2 + n]
        p += 2 + n
        if m == 0xDB:
            q = 0
            while q < len(seg):
                assert seg[q] >> 4 == 0
                quant[seg[q] & 15] = list(seg[q + 1:q + 65])                    # zigzag order
                q += 65
        elif m == 0xC0:
            assert seg[0] == 8
            H, W = _u16(seg, 1), _u16(seg, 3)
            comps = [(seg[6 + 3 * i], seg[7 + 3 * i] >> 4, seg[7 + 3 * i] & 15, seg[8 + 3 * i]) for i in range(seg[5])]
        elif m == 0xC4:
            q = 0
            while q < len(seg):
                counts = seg[q + 1:q + 17]
                table, code, k = {}, 0, q + 17
                for length in range(1, 17):
                    for _ in range(counts[length - 1]):
                        table[(length, code)] = seg[k]
                        code += 1
                        k += 1
                    code <<= 1
                codes[(seg[q] >> 4, seg[q] & 15)] = table
                q = k
        elif m == 0xDD:
            ri = _u16(seg, 0)
        elif m == 0xDA:
            assert seg[0] == len(comps)
            tabs = [(seg[2 + 2 * i] >> 4, seg[2 + 2 * i] & 15) for i in range(seg[0])]
            return H, W, comps, quant, codes, ri, tabs, p
        else:
            assert 0xE0 <= m <= 0xFE, "marker %02x" % m


class _Bits:
    def __init__(self, d, p):
        self.d, self.p, self.bit = d, p, 0

    def one(self):
        byte = self.d[self.p]
        assert not (byte == 0xFF and self.d[self.p + 1] != 0), "a marker inside the data"
        v = (byte >> (7 - self.bit)) & 1
        self.bit += 1
        if self.bit == 8:
            self.bit = 0
            self.p += 2 if byte == 0xFF else 1
        return v

    def many(self, n):
        v = 0
        for _ in range(n):
            v = (v << 1) | self.one()
        return v

    def symbol(self, table):
        code = 0
        for length in range(1, 17):
            code = (code << 1) | self.one()
            if (length, code) in table:
                return table[(length, code)]
        raise AssertionError("no code")

    def amplitude(self, s):
        if s == 0:
            return 0
        v = self.many(s)
        return v if v >= (1 << (s - 1)) else v - (1 << s) + 1

    def restart(self, n):
        if self.bit:                                                            # the padding of the last byte
            self.p += 2 if self.d[self.p] == 0xFF else 1
            self.bit = 0
        assert self.d[self.p] == 0xFF and self.d[self.p + 1] == 0xD0 + (n & 7), "RST%d expected" % (n & 7)
        self.p += 2


def _pass(d, n):
    z1 = (d[2] + d[6]) * 4433
    t2 = z1 - d[6] * 15137
    t3 = z1 + d[2] * 6270
    t0 = (d[0] + d[4]) << 13
    t1 = (d[0] - d[4]) << 13
    e0, e3, e1, e2 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    o0, o1, o2, o3 = d[7], d[5], d[3], d[1]
    z1, z2, z3, z4 = o0 + o3, o1 + o2, o0 + o2, o1 + o3
    z5 = (z3 + z4) * 9633
    o0, o1, o2, o3 = o0 * 2446, o1 * 16819, o2 * 25172, o3 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z5 - z3 * 16069, z5 - z4 * 3196
    o0, o1, o2, o3 = o0 + z1 + z3, o1 + z2 + z4, o2 + z2 + z3, o3 + z1 + z4
    return [(v + (1 << (n - 1))) >> n for v in (e0 + o3, e1 + o2, e2 + o1, e3 + o0, e3 - o0, e2 - o1, e1 - o2, e0 - o3)]


def _idct(block):
    """64 dequantised coefficients in natural order -> 64 samples."""
    ws = [0] * 64
    for c in range(8):
        col = _pass([block[8 * r + c] for r in range(8)], 11)
        for r in range(8):
            ws[8 * r + c] = col[r]
    out = []
    for r in range(8):
        out.extend(min(max(v + 128, 0), 255) for v in _pass(ws[8 * r:8 * r + 8], 18))
    return out


def _chroma(plane, y, x, hs, vs, ch, cw):
    """The upsampled value over pixel (y, x) of a plane with ch x cw real samples."""
    if hs == 1:
        return plane[y][x]
    cy = y >> 1 if vs == 2 else y
    cx = x >> 1
    if cw <= 2:
        return plane[cy][cx]
    side = min(cx + 1, cw - 1) if x & 1 else max(cx - 1, 0)
    if vs == 1:
        return (3 * plane[cy][cx] + plane[cy][side] + (2 if x & 1 else 1)) >> 2
    near = min(cy + 1, ch - 1) if y & 1 else max(cy - 1, 0)
    this = 3 * plane[cy][cx] + plane[near][cx]
    other = 3 * plane[cy][side] + plane[near][side]
    return (3 * this + other + (7 if x & 1 else 8)) >> 4


def decode(data, bgr=False):
    d = bytes(data)
    H, W, comps, quant, codes, ri, tabs, p = _header(d)
    hs, vs = comps[0][1], comps[0][2]
    assert len(comps) in (1, 3) and all((c[1], c[2]) == (1, 1) for c in comps[1:])
    MW, MH = -(-W // (8 * hs)), -(-H // (8 * vs))
    planes = [[[0] * (8 * MW * (hs if i == 0 else 1)) for _ in range(8 * MH * (vs if i == 0 else 1))] for i in range(len(comps))]
    bits = _Bits(d, p)
    pred = [0] * len(comps)
    for m in range(MH * MW):
        if ri and m and m % ri == 0:
            bits.restart(m // ri - 1)
            pred = [0] * len(comps)
        my, mx = divmod(m, MW)
        for i, comp in enumerate(comps):
            h, v = (hs, vs) if i == 0 else (1, 1)
            q = quant[comp[3]]
            for by in range(v):
                for bx in range(h):
                    co = [0] * 64
                    pred[i] += bits.amplitude(bits.symbol(codes[(0, tabs[i][0])]))
                    co[0] = pred[i] * q[0]
                    k = 1
                    while k < 64:
                        rs = bits.symbol(codes[(1, tabs[i][1])])
                        r, s = rs >> 4, rs & 15
                        if s == 0:
                            if r != 15:
                                break
                            k += 16
                            continue
                        k += r
                        assert k <= 63
                        co[ZIGZAG[k]] = bits.amplitude(s) * q[k]
                        k += 1
                    px = _idct(co)
                    for yy in range(8):
                        row = planes[i][(my * v + by) * 8 + yy]
                        x0 = (mx * h + bx) * 8
                        row[x0:x0 + 8] = px[8 * yy:8 * yy + 8]
    ch, cw = -(-H // vs), -(-W // hs)
    out = []
    for y in range(H):
        row = []
        for x in range(W):
            Y = planes[0][y][x]
            if len(comps) == 1:
                row.append([Y, Y, Y])
                continue
            cb = _chroma(planes[1], y, x, hs, vs, ch, cw) - 128
            cr = _chroma(planes[2], y, x, hs, vs, ch, cw) - 128
            rgb = [Y + ((91881 * cr + 32768) >> 16), Y + ((-22554 * cb - 46802 * cr + 32768) >> 16), Y + ((116130 * cb + 32768) >> 16)]
            rgb = [min(max(v, 0), 255) for v in rgb]
            row.append(rgb[::-1] if bgr else rgb)
        out.append(row)
    return out
