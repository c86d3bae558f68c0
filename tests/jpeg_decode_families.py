"""The input families of the JPEG decoder's tests (CPU, host check and GPU share them): small files made with Pillow and
with this project's `jpeg.encode_host` from seeded arrays, and the fixed list of damaged streams.  No test lives here."""
import functools
import io

import numpy as np
from PIL import Image

SIZES = ((1, 1), (8, 8), (16, 16), (17, 17), (33, 47), (70, 37), (48, 1296), (1296, 48))        # (W, H)
MODES = (0, 1, 2, "L")                                                              # Pillow's `subsampling`, or mode "L"
# Seeds of the single flipped bits.  A flip inside a coefficient's amplitude bits leaves a valid stream with other pixels, which
# no decoder can notice; the seeds kept here land in a code word, so that the stream stops making sense before it ends.
FLIP_SEEDS = (100, 101, 103, 105, 112)


def content(kind, W, H, seed=0):
    """u8 [H,W,3] R G B."""
    rng = np.random.RandomState(1000 + seed)
    y, x = np.mgrid[0:H, 0:W]
    if kind == "flat":
        img = np.empty((H, W, 3), dtype=np.uint8)
        img[:] = (200, 30, 90)
    elif kind == "gradient":                                                        # a gradient with text-like strokes on it
        img = np.stack([(x * 255) // max(W - 1, 1), (y * 255) // max(H - 1, 1), ((x + y) * 255) // max(W + H - 2, 1)], axis=2).astype(np.uint8)
        for _ in range(max(2, (W * H) // 400)):
            x0, y0 = rng.randint(0, W), rng.randint(0, H)
            img[y0:y0 + rng.randint(1, 4), x0:x0 + rng.randint(2, 12)] = rng.randint(0, 256, size=3)
    elif kind == "checker":
        img = (((x + y) & 1) * 255).astype(np.uint8)[:, :, None].repeat(3, axis=2)
        img[:, :, 1] = 255 - img[:, :, 1]
    elif kind == "noise":
        img = rng.randint(0, 256, size=(H, W, 3)).astype(np.uint8)
    else:
        raise ValueError(kind)
    return img


def pillow_file(img, mode, quality=95, **kw):
    buf = io.BytesIO()
    if mode == "L":
        Image.fromarray(img).convert("L").save(buf, "JPEG", quality=quality, **kw)
    else:
        Image.fromarray(img).save(buf, "JPEG", quality=quality, subsampling=mode, **kw)
    return buf.getvalue()


def own_file(img, quality=95):
    """A round trip through this project's encoder: 4:2:0 with a restart interval per MCU row."""
    from gomatching_amd import jpeg
    H, W = img.shape[:2]
    payload, offsets = jpeg.encode_host(img[None], quality, bgr=False)
    return jpeg.files(payload, offsets, H, W, quality)[0]


def pillow_pixels(data):
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


@functools.lru_cache(maxsize=None)
def families():
    """-> tuple of (name, (file bytes, ...)): every entry is one decode call (its files share a geometry)."""
    out = []
    for W, H in SIZES:
        for mode in MODES:
            out.append(("size-%dx%d-%s" % (W, H, mode), (pillow_file(content("gradient", W, H), mode),)))
    for W, H in ((33, 47), (70, 37)):
        for q in (1, 50, 100):
            for kind in ("noise", "gradient"):
                out.append(("q%d-%s-%dx%d-420" % (q, kind, W, H), (pillow_file(content(kind, W, H, q), 2, q),)))
    for q in (1, 100):
        for mode in (0, 1, "L"):
            out.append(("q%d-noise-33x47-%s" % (q, mode), (pillow_file(content("noise", 33, 47, q), mode, q),)))
    for kind in ("flat", "checker", "noise"):
        for mode in MODES:
            out.append(("%s-33x47-%s" % (kind, mode), (pillow_file(content(kind, 33, 47), mode),)))
    for mode in MODES:
        out.append(("optimize-70x37-%s" % mode, (pillow_file(content("noise", 70, 37, 3), mode, 90, optimize=True),)))
        out.append(("rst-rows-70x37-%s" % mode, (pillow_file(content("gradient", 70, 37, 4), mode, restart_marker_rows=1),)))
        out.append(("rst-rows-48x1296-%s" % mode, (pillow_file(content("gradient", 48, 1296, 5), mode, 75, restart_marker_rows=1),)))
        out.append(("rst-blocks-33x47-%s" % mode, (pillow_file(content("noise", 33, 47, 6), mode, restart_marker_blocks=3),)))
    for W, H in ((1, 1), (16, 16), (33, 47), (70, 37)):
        out.append(("own-%dx%d" % (W, H), (own_file(content("gradient", W, H, 7)),)))
    out.append(("own-noise-q100-33x47", (own_file(content("noise", 33, 47, 8), 100),)))
    out.append(("three-files-70x37-420", (pillow_file(content("noise", 70, 37, 9), 2, 100, optimize=True),
                                          pillow_file(content("flat", 70, 37), 2, 30),
                                          pillow_file(content("gradient", 70, 37, 10), 2, 95, optimize=True))))
    return tuple(out)


def refused():
    """-> [(name, file bytes, a word its reason must hold)]."""
    img = content("gradient", 33, 47)
    buf = io.BytesIO()
    Image.fromarray(img).save(buf, "JPEG", progressive=True)
    prog = buf.getvalue()
    buf = io.BytesIO()
    Image.fromarray(img).convert("CMYK").save(buf, "JPEG")
    cmyk = buf.getvalue()
    base = pillow_file(img, 2)
    return [("progressive", prog, "progressive"), ("cmyk", cmyk, "components"), ("cut-header", base[:150], "truncated")]


def _scan_start(data):
    from gomatching_amd import jpeg
    return jpeg.parse(data).scan


def _bit_writer():
    bits = []

    def put(value, length):
        bits.extend((value >> (length - 1 - i)) & 1 for i in range(length))

    def done():
        while len(bits) % 8:
            bits.append(1)
        raw = np.packbits(np.array(bits, dtype=np.uint8)).tobytes()
        return raw.replace(b"\xff", b"\xff\x00")

    return put, done


def _codes(bits, vals):
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[vals[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return out


@functools.lru_cache(maxsize=None)
def damaged():
    """-> tuple of (name, file bytes): each must parse, give a non-zero status word and raise nothing."""
    from gomatching_amd import jpeg
    out = []
    base = pillow_file(content("noise", 33, 47, 11), 2, 90)
    a, b = _scan_start(base)
    for frac in (0.25, 0.5, 0.9):
        cut = a + int((b - a) * frac)
        out.append(("cut-%d%%" % int(frac * 100), base[:cut] + b"\xff\xd9"))
    out.append(("cut-no-eoi", base[:a + (b - a) // 3]))
    for seed in FLIP_SEEDS:
        rng = np.random.RandomState(seed)
        pos = a + int(rng.randint(0, (b - a) * 3 // 4))
        raw = bytearray(base)
        raw[pos] ^= 1 << int(rng.randint(0, 8))
        out.append(("flip-%d" % seed, bytes(raw)))
    rst = pillow_file(content("gradient", 70, 37, 4), 2, restart_marker_rows=1)
    at = rst.index(b"\xff\xd1", _scan_start(rst)[0])
    out.append(("wrong-rst", rst[:at + 1] + b"\xd3" + rst[at + 2:]))
    out.append(("missing-rst", rst[:at] + rst[at + 2:]))
    # a run that pushes the coefficient index past 63: DC category 0, then four times (run 15, size 1)
    gray = pillow_file(content("flat", 8, 8), "L")
    info = jpeg.parse(gray)
    dc, ac = _codes(*info.huff[(0, info.comp_dc[0])]), _codes(*info.huff[(1, info.comp_ac[0])])
    put, done = _bit_writer()
    put(*dc[0])
    for _ in range(4):
        put(*ac[0xF1])
        put(1, 1)
    put(*ac[0x00])
    out.append(("index-past-63", gray[:info.scan[0]] + done() + b"\xff\xd9"))
    put, done = _bit_writer()
    put(*dc[0])
    for _ in range(4):
        put(*ac[0xF0])
    put(*ac[0x00])
    out.append(("zrl-past-63", gray[:info.scan[0]] + done() + b"\xff\xd9"))
    return tuple(out)
