"""The rule of `gom_result_parse_*` (include/gomatching_hip.h) in plain Python, line by line: bytes -> (status, arrays).

Nothing here is shared with the kernels or with csrc/result_parse_core.h; the constants are the header's.  `reserialise` gives
the text back from the arrays, through json.dumps itself: the property every test leans on is
    status != 0   or   reserialise(data, arrays) == data.
"""
import json
import re

import numpy as np

from gomatching_amd.lib import CONSTANTS as C

BAD_PLACE, BAD_INT, BAD_KEY, BAD_POINTS = C["GOM_RP_BAD_PLACE"], C["GOM_RP_BAD_INT"], C["GOM_RP_BAD_KEY"], C["GOM_RP_BAD_POINTS"]
BAD_LINE, BAD_ENDS, BAD_SIZE, BAD_STRING = C["GOM_RP_BAD_LINE"], C["GOM_RP_BAD_ENDS"], C["GOM_RP_BAD_SIZE"], C["GOM_RP_BAD_STRING"]
MAX_LINE, MAX_SIZE = C["GOM_RP_MAX_LINE"], C["GOM_RP_MAX_SIZE"]
I32 = (-2 ** 31, 2 ** 31 - 1)
I64 = (-2 ** 63, 2 ** 63 - 1)
CAUSES = {BAD_PLACE: "a line that does not fit its place", BAD_INT: "an integer that is not canonical or out of range",
          BAD_KEY: "a frame key that is not the next number", BAD_POINTS: "a wrong count of points",
          BAD_LINE: "an unterminated or over-long line", BAD_ENDS: "a file that does not end as the writer ends it",
          BAD_SIZE: "a size the call does not take", BAD_STRING: "a transcription json.dumps writes differently"}


def integer(tok, lo, hi):
    """An integer token -> (status, value)."""
    if not tok or chr(tok[0]) not in "-0123456789" or any(chr(c) not in "-+.eE0123456789" for c in tok):
        return BAD_PLACE, 0
    if not re.fullmatch(rb"-?(0|[1-9][0-9]*)", tok) or tok == b"-0" or len(tok.lstrip(b"-")) > 19:
        return BAD_INT, 0
    v = int(tok)
    return (0, v) if lo <= v <= hi else (BAD_INT, 0)


def int_line(line, indent, key, comma, lo, hi):
    head = b" " * indent + key
    if len(line) < len(head) + 1 + comma or not line.startswith(head) or (comma and not line.endswith(b",")):
        return BAD_PLACE, 0
    return integer(line[len(head):len(line) - comma], lo, hi)


def string_line(line):
    """-> (status, offset of the span in the line, its length, whether a comma follows)."""
    head = b" " * 12 + b'"transcription": "'
    if len(line) < len(head) + 1 or not line.startswith(head):
        return BAD_PLACE, 0, 0, False
    i = len(head)
    while i < len(line):
        if line[i] == 0x5C:
            i += 2
        elif line[i] == 0x22:
            break
        else:
            i += 1
    if i >= len(line):
        return BAD_LINE, 0, 0, False
    rest = line[i + 1:]
    if rest not in (b"", b","):
        return BAD_PLACE, 0, 0, False
    return 0, len(head), i - len(head), rest == b","


def key_line(line):
    """-> (status, key, the [] form, comma)."""
    if len(line) < 5 or not line.startswith(b'    "'):
        return BAD_PLACE, 0, False, False
    comma = line.endswith(b",")
    body = line[:-1] if comma else line
    empty = body.endswith(b"]")
    body = body[:-1] if empty else body
    if len(body) - 5 < 5 or not body.endswith(b'": ['):
        return BAD_PLACE, 0, empty, comma
    st, key = integer(body[5:-4], 1, 2 ** 31 - 2)
    return (BAD_KEY if st == BAD_INT else st), key, empty, comma


def points_of(nl):
    return (nl - 18) // 4 if nl >= 22 and (nl - 18) % 4 == 0 else 0


def is_line(line, indent, lit, comma=False):
    return line == b" " * indent + lit + (b"," if comma else b"")


def parse(data):
    """-> (status, arrays or None).  arrays: frame_rows, ids, pts, has_seg, t_off, t_len, poly_off, poly_xy (numpy, the dtypes of
    the header) and the totals L, F, N, P."""
    data = bytes(data)
    size = len(data)
    if size < 1 or size > MAX_SIZE - 1:
        return BAD_SIZE, None
    lines = data.split(b"\n")
    L = len(lines)
    start = [0]
    for ln in lines:
        start.append(start[-1] + len(ln) + 1)
    empty = dict(L=L, F=0, N=0, P=0, frame_rows=np.zeros(1, np.int32), ids=np.zeros(0, np.int64), pts=np.zeros((0, 8), np.int32),
                 has_seg=np.zeros(0, np.uint8), t_off=np.zeros(0, np.int64), t_len=np.zeros(0, np.int32),
                 poly_off=np.zeros(1, np.int32), poly_xy=np.zeros((0, 2), np.int32))
    # ---- stage 1
    if L == 1:
        return (0, empty) if data == b"{}" else (BAD_ENDS, None)
    if not (size >= 3 and data.startswith(b"{\n") and data.endswith(b"\n}")):
        return BAD_ENDS, None
    # ---- stage 2
    status = 0
    marks = []                                                 # (line, is an object line)
    for i, ln in enumerate(lines):
        if len(ln) > MAX_LINE:
            status |= BAD_LINE
        if ln == b" " * 8 + b"{":
            marks.append((i, True))
        elif len(ln) >= 5 and ln.startswith(b'    "'):
            marks.append((i, False))
    N = sum(1 for _, o in marks if o)
    F = len(marks) - N
    if F == 0:
        status |= BAD_PLACE
    if status:
        return status, None
    marks.append((L - 1, False))
    obj_mark = [k for k, (_, o) in enumerate(marks[:-1]) if o]
    frame_mark = [k for k, (_, o) in enumerate(marks[:-1]) if not o]
    frame_rows = [sum(1 for k in obj_mark if k < fm) for fm in frame_mark] + [N]
    # ---- stage 3
    ids, pts, has_seg = np.zeros(N, np.int64), np.zeros((N, 8), np.int32), np.zeros(N, np.uint8)
    t_off, t_len, poly_off = np.zeros(N, np.int64), np.zeros(N, np.int32), np.zeros(N + 1, np.int32)
    spans = []
    for o, k in enumerate(obj_mark):
        s, e = marks[k][0], marks[k + 1][0]
        next_obj = marks[k + 1][1]
        nl = max(e - s - (0 if next_obj else 1), 0)
        spans.append((s, nl, next_obj))
        poly_off[o + 1] = poly_off[o] + points_of(nl)
    P = int(poly_off[N])
    poly_xy = np.zeros((P, 2), np.int32)
    for o, (s, nl, next_obj) in enumerate(spans):
        closers = [j for j in range(2, min(nl, 64)) if is_line(lines[s + j], 12, b"]", True)]
        if not closers:
            status |= BAD_PLACE
            continue
        if closers[0] != 10:
            status |= BAD_POINTS
            continue
        if not (nl in (14, 17) or (nl >= 22 and (nl - 18) % 4 == 0)):
            status |= BAD_PLACE
            continue
        n = points_of(nl)
        ob = lines[s:s + nl]
        ok = is_line(ob[0], 8, b"{") and is_line(ob[1], 12, b'"points": [') and is_line(ob[10], 12, b"]", True) and \
            is_line(ob[nl - 1], 8, b"}", next_obj)
        for j in range(2, 10):
            st, v = int_line(ob[j], 16, b"", j < 9, *I32)
            status |= st
            pts[o, j - 2] = v
        st, v = int_line(ob[11], 12, b'"ID": ', True, *I64)
        status |= st
        ids[o] = v
        st, off, ln, comma = string_line(ob[12])
        status |= st
        if st == 0:
            if comma != (nl > 14):
                status |= BAD_PLACE
            t_off[o], t_len[o], has_seg[o] = start[s + 12] + off, ln, nl > 14
        if nl > 14:
            ok = ok and is_line(ob[13], 12, b'"segmentation": [') and is_line(ob[nl - 2], 12, b"]")
            if nl == 17:
                ok = ok and is_line(ob[14], 16, b"[]")
            else:
                ok = ok and is_line(ob[14], 16, b"[") and is_line(ob[nl - 3], 16, b"]")
                for p in range(n):
                    q = ob[15 + 4 * p:19 + 4 * p]
                    ok = ok and is_line(q[0], 20, b"[") and is_line(q[3], 20, b"]", p < n - 1)
                    for c in (0, 1):
                        st, v = int_line(q[1 + c], 24, b"", c == 0, *I32)
                        status |= st
                        poly_xy[poly_off[o] + p, c] = v
        if not ok:
            status |= BAD_PLACE
    for f, k in enumerate(frame_mark):
        kl, e = marks[k][0], marks[k + 1][0]
        x = marks[frame_mark[f + 1]][0] if f + 1 < F else L - 1
        r0, r1, last = frame_rows[f], frame_rows[f + 1], f == F - 1
        if f == 0 and (kl != 1 or r0 != 0):
            status |= BAD_PLACE
        st, key, emp, comma = key_line(lines[kl])
        if st:
            status |= st
            continue
        if key != f + 1:
            status |= BAD_KEY
        if r1 <= r0:
            if not emp or e != kl + 1 or comma != (not last):
                status |= BAD_PLACE
        elif emp or comma or e != kl + 1 or not is_line(lines[x - 1], 4, b"]", not last):
            status |= BAD_PLACE
    if status:
        return status, None
    # ---- the host's part: every transcription decodes, and json.dumps writes it back as it stands
    for o in range(N):
        span = data[int(t_off[o]):int(t_off[o]) + int(t_len[o])]
        try:
            text = json.loads(b'"' + span + b'"')
            back = json.dumps(text, ensure_ascii=False).encode("utf-8")
        except (ValueError, UnicodeError):
            return BAD_STRING, None
        if back != b'"' + span + b'"':
            return BAD_STRING, None
    return 0, dict(L=L, F=F, N=N, P=P, frame_rows=np.asarray(frame_rows, np.int32), ids=ids, pts=pts, has_seg=has_seg, t_off=t_off,
                   t_len=t_len, poly_off=poly_off, poly_xy=poly_xy)


def annotation(data, a):
    """The arrays of an accepted file -> {frame: [{"points": .., "ID": .., "transcription": .., ["segmentation": ..]}]}."""
    out = {}
    for f in range(a["F"]):
        objs = []
        for o in range(int(a["frame_rows"][f]), int(a["frame_rows"][f + 1])):
            span = data[int(a["t_off"][o]):int(a["t_off"][o]) + int(a["t_len"][o])]
            obj = {"points": [int(v) for v in a["pts"][o]], "ID": int(a["ids"][o]), "transcription": json.loads(b'"' + span + b'"')}
            if a["has_seg"][o]:
                obj["segmentation"] = [[[int(x), int(y)] for x, y in a["poly_xy"][int(a["poly_off"][o]):int(a["poly_off"][o + 1])]]]
            objs.append(obj)
        out[str(f + 1)] = objs
    return out


def reserialise(data, a):
    return json.dumps(annotation(data, a), ensure_ascii=False, indent=4).encode("utf-8")
