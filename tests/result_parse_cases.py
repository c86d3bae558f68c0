"""Inputs for the result parser's tests: clean families, built with json.dumps itself, which the rule MUST accept, and a damaged
corpus of bytes it may not read differently from json.loads.  Seeded; a case is (name, bytes)."""
import json
import os
import random
import struct

from gomatching_amd.lib import CONSTANTS as C

HERE = os.path.dirname(os.path.abspath(__file__))
BLOCK_BYTES, BLOCK = C["GOM_RP_BLOCK_BYTES"], C["GOM_RP_BLOCK"]
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1
TEXTS = ["", 'a"b\\c', "\u0001", "line\nfeed\ttab", "\u007f", "中文字幕", "ABCDEFGHIJKLMNOPQRSTUVWXY", "hello"]


def dumps(a, **kw):
    kw.setdefault("indent", 4)
    kw.setdefault("ensure_ascii", False)
    return json.dumps(a, **kw).encode("utf-8")


def obj(rng, n=4, track=None, text="text", lo=-40, hi=90, seg=True):
    o = {"points": [rng.randint(lo, hi) for _ in range(8)], "ID": rng.randint(0, 900) if track is None else track,
         "transcription": text}
    if seg:
        o["segmentation"] = [[[rng.randint(lo, hi), rng.randint(lo, hi)] for _ in range(n)]]
    return o


def base_annotation(seed=3):
    """Three frames, the middle one empty; contours of 50, 3 and 5 points."""
    rng = random.Random(seed)
    return {"1": [obj(rng, 50, 7, "first"), obj(rng, 3, 8, "second")], "2": [], "3": [obj(rng, 5, 7, "third")]}


def long_annotation():
    """More than a tile of block counts (GOM_RP_BLOCK blocks of GOM_RP_BLOCK_BYTES bytes) and more than a tile of line blocks."""
    rng = random.Random(11)
    a, f = {}, 0
    rows = 0                                                   # (a row of 50 points: 218 lines, more than 5000 bytes)
    while rows * 5000 < BLOCK * BLOCK_BYTES + 3 * BLOCK_BYTES or rows * 218 < BLOCK * BLOCK + 2 * BLOCK:
        f += 1
        rows = sum(len(v) for v in a.values())
        a[str(f)] = [obj(rng, 50, rng.randint(0, 40), TEXTS[rng.randrange(len(TEXTS))], 0, 1900) for _ in range(rng.randint(0, 9))]
    return a


def clean_annotations():
    rng = random.Random(5)
    out = [("no frames", {}), ("three frames", base_annotation()), ("one empty frame", {"1": []}),
           ("empty frames", {"1": [], "2": [], "3": []}),
           ("without segmentation", {"1": [obj(rng, seg=False), obj(rng, 4)], "2": [obj(rng, seg=False)]}),
           ("contour sizes", {"1": [obj(rng, n) for n in (0, 1, 2, 49, 50)], "2": [obj(rng, 0)], "3": [obj(rng, 1), obj(rng, 0)]}),
           ("negative", {"1": [obj(rng, 6, lo=-5000, hi=-1)]}),
           ("int32 limits", {"1": [obj(rng, 4, lo=I32_MIN, hi=I32_MIN), obj(rng, 3, lo=I32_MAX, hi=I32_MAX),
                                   {"points": [I32_MIN, I32_MAX, 0, -1, 1, 10, -10, 2147483646], "ID": -2 ** 63, "transcription": "x",
                                    "segmentation": [[[I32_MAX, I32_MIN], [0, 0], [-1, 1]]]}]}),
           ("ids", {"1": [obj(rng, 3, 0), obj(rng, 3, -1), obj(rng, 3, 2 ** 40), obj(rng, 3, 2 ** 63 - 1), obj(rng, 3, -499)]}),
           ("transcriptions", {str(i + 1): [obj(rng, 3, i, t), obj(rng, 0, i + 50, t, seg=i % 2 == 0)] for i, t in enumerate(TEXTS)})]
    return out


def golden_texts():
    with open(os.path.join(HERE, "golden", "results_writer.json"), "r", encoding="utf-8") as fp:
        g = json.load(fp)
    return [("golden " + k, v.encode("utf-8")) for k, v in sorted(g.get("json", {}).items())]


_CLEAN = None


def clean_cases():
    """[(name, bytes)]: every one MUST be accepted.  Built once and shared."""
    global _CLEAN
    if _CLEAN is None:
        _CLEAN = [(n, dumps(a)) for n, a in clean_annotations()] + [("long", dumps(long_annotation()))] + golden_texts()
    return _CLEAN


def _line_kinds(text):
    """One line index per kind of line of the base text: the kinds are the lines' bytes with digits folded."""
    kinds = {}
    for i, ln in enumerate(text.split(b"\n")):
        k = bytes(48 if 48 <= c <= 57 else c for c in ln)
        while b"00" in k:
            k = k.replace(b"00", b"0")
        kinds.setdefault(k, i)
    return sorted(kinds.values())


def _with_token(tok, where="points"):
    a = base_annotation()
    mark = 123456789
    if where == "points":
        a["1"][0]["points"][3] = mark
    elif where == "seg":
        a["1"][0]["segmentation"][0][7][1] = mark
    else:
        a["1"][0]["ID"] = mark
    return dumps(a).replace(str(mark).encode(), tok)


def damaged_cases():
    """[(name, bytes)]: bytes near the accepted ones."""
    rng = random.Random(17)
    base = dumps(base_annotation())
    lines = base.split(b"\n")
    join = b"\n".join
    out = []
    kinds = _line_kinds(base)
    starts = [0]
    for ln in lines:
        starts.append(starts[-1] + len(ln) + 1)
    for i in kinds:                                            # a substitution and a truncation inside every kind of line
        at = starts[i] + rng.randrange(len(lines[i]))
        for c in (0x20, 0x0A, 0x22, 0x31, 0x2C, 0x5B, 0x7D):
            if base[at] != c:
                out.append(("substitute %#x at line %d" % (c, i), base[:at] + bytes([c]) + base[at + 1:]))
        out.append(("truncated in line %d" % i, base[:at]))
        out.append(("delete line %d" % i, join(lines[:i] + lines[i + 1:])))
        out.append(("duplicate line %d" % i, join(lines[:i + 1] + lines[i:])))
    for _ in range(40):                                        # seeded substitutions anywhere
        at = rng.randrange(len(base))
        c = rng.choice(b' \n",:[]{}0123456789-\\ax\r\t')
        if base[at] != c:
            out.append(("substitute %#x at byte %d" % (c, at), base[:at] + bytes([c]) + base[at + 1:]))
    for _ in range(12):
        i, j = rng.sample(range(len(lines)), 2)
        sw = list(lines)
        sw[i], sw[j] = sw[j], sw[i]
        if sw != lines:
            out.append(("swap lines %d and %d" % (i, j), join(sw)))
    out.append(("crlf", base.replace(b"\n", b"\r\n")))
    out.append(("tab indent", base.replace(b"\n        {", b"\n\t{", 1)))
    out.append(("tab indent of a value", base.replace(b"\n" + b" " * 16, b"\n" + b" " * 12 + b"\t", 1)))
    out.append(("indent 2", dumps(base_annotation(), indent=2)))
    out.append(("no indent", dumps(base_annotation(), indent=None)))
    chinese = {"1": [obj(random.Random(2), 3, 1, "中文")]}
    out.append(("ensure_ascii", dumps(chinese, ensure_ascii=True)))
    for tok in (b"1.5", b"1e3", b"01", b"-0", b"12345678901234567890", b"2147483648", b"-2147483649", b"+1", b"1 ", b"true",
                b"null", b"0x10", b"--1", b"-", b"1-1"):
        for where in ("points", "seg"):
            out.append(("token %s in %s" % (tok.decode(), where), _with_token(tok, where)))
    for tok in (b"9223372036854775808", b"-9223372036854775809", b"1.0", b"007", b'"7"'):
        out.append(("token %s as ID" % tok.decode(), _with_token(tok, "id")))
    a = base_annotation()
    out.append(("keys 1 3", dumps({"1": a["1"], "3": a["3"]})))
    out.append(("keys from 0", dumps({"0": a["1"], "1": a["2"], "2": a["3"]})))
    out.append(("keys 1 2 2", dumps(a).replace(b'"3": [', b'"2": [')))
    out.append(("key 01", dumps(a).replace(b'"1": [', b'"01": [')))
    o = a["1"][0]
    out.append(("ID first", dumps({"1": [{"ID": o["ID"], "points": o["points"], "transcription": "t"}]})))
    out.append(("extra key", dumps({"1": [dict(o, score=1)]})))
    out.append(("extra key in front", dumps({"1": [dict([("score", 1)] + list(o.items()))]})))
    out.append(("no transcription", dumps({"1": [{"points": o["points"], "ID": 1, "segmentation": o["segmentation"]}]})))
    out.append(("no transcription, no segmentation", dumps({"1": [{"points": o["points"], "ID": 1}]})))
    for n in (0, 7, 9, 11, 12):
        for seg in (True, False):
            d = {"points": list(range(n)), "ID": 1, "transcription": "t"}
            if seg:
                d["segmentation"] = [[[1, 2]] * 3]
            out.append(("%d points%s" % (n, ", segmentation" if seg else ""), dumps({"1": [d, obj(rng)]})))
    out.append(("two contours", dumps({"1": [dict(o, segmentation=[[[1, 2], [3, 4]], [[5, 6], [7, 8]]])]})))
    out.append(("no contour", dumps({"1": [dict(o, segmentation=[])]})))
    out.append(("a point of three", dumps({"1": [dict(o, segmentation=[[[1, 2, 3], [4, 5, 6]]])]})))
    out.append(("a point of one", dumps({"1": [dict(o, segmentation=[[[1], [2], [3], [4]]])]})))
    out.append(("trailing newline", base + b"\n"))
    out.append(("leading newline", b"\n" + base))
    out.append(("a list", dumps([a["1"]])))
    out.append(("frame is an object", dumps({"1": {"points": [1]}})))
    out.append(("frame is a number", dumps({"1": 5, "2": []})))
    out.append(("nested braces", b"{\n}"))
    out.append(("one byte", b"{"))
    out.append(("spaces", b"{ }"))
    out.append(("escaped quote at the end", base.replace(b'"first",', b'"first\\",')))
    out.append(("quote inside", base.replace(b'"first",', b'"fi"rst",')))
    out.append(("escape json.dumps does not write", base.replace(b'"first",', b'"f\\u0069rst",')))
    out.append(("an escape json.loads refuses", base.replace(b'"first",', b'"f\\xrst",')))
    out.append(("raw control byte", base.replace(b'"first",', b'"f\x01rst",')))
    out.append(("bytes that are not UTF-8", base.replace(b'"first",', b'"f\xff\xferst",')))
    out.append(("a lone surrogate", base.replace(b'"first",', b'"f\\ud800rst",')))
    out.append(("long line", base.replace(b'"first",', b'"' + b"w" * (C["GOM_RP_MAX_LINE"] + 1) + b'",')))
    out.append(("transcription is a number", base.replace(b'"first",', b'5,')))
    out.append(("comma after the last row", base.replace(b"        }\n    ],", b"        },\n    ],", 1)))
    out.append(("no comma between frames", base.replace(b"    ],\n", b"    ]\n", 1)))
    out.append(("comma after the last frame", base[:-2] + b",\n}"))
    return out


def dump(path, cases):
    """The cases as tools/result_parse_hostcheck.cpp reads them: int64 count; per case int64 size and the bytes."""
    with open(path, "wb") as fp:
        fp.write(struct.pack("<q", len(cases)))
        for _, data in cases:
            fp.write(struct.pack("<q", len(data)))
            fp.write(data)
