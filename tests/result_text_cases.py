"""The case list of the result text tests, shared by the CPU statement test, the host check under sanitizers and the GPU test:
hand-made `ops.result_rows` words (50-point polygons, class ids, emit masks, track ids), rectangle points, keep flags and
frame offsets -- the smallest inputs at which the count / scan / emit trio can go wrong.  numpy only."""
import os

import numpy as np

from gomatching_amd import results
from gomatching_amd.predictor import CTLABELS_37, CTLABELS_96

WORDS = 234
SCAN_BLOCK = 256                                                  # GOM_RT_SCAN_BLOCK (asserted against the header by the tests)
I32_EDGE = (0, -1, 9, 10, -10, 99999, 2 ** 31 - 1, -2 ** 31)
ID_EDGE = (0, 2 ** 63 - 1, -2 ** 63)
# a custom dictionary: every escape of either writer, U+007F, and 2-, 3- and 4-byte code points
CUSTOM = ['"', "\\", "&", "<", ">", "'", "\x7f", "é", "中", "\U0001f600", "文", "a", "/", "€"]


class Labels:
    """What `results.text_tables` and the row builder need of a TextDecoder."""

    def __init__(self, labels):
        self.labels = list(labels)
        self.voc_size = len(self.labels) + 1
        self._table = np.asarray(self.labels, dtype=object)


DECODERS = {"37": Labels(CTLABELS_37), "96": Labels(CTLABELS_96), "custom": Labels(CUSTOM)}


class Case:
    def __init__(self, name, voc, counts, first_frame=0, seed=0):
        self.name, self.voc, self.first_frame = name, voc, first_frame
        self.decoder = DECODERS[voc]
        self.frame_rows = np.concatenate(([0], np.cumsum(counts))).astype(np.int32)
        n = int(self.frame_rows[-1])
        rng = np.random.RandomState(seed)
        ntab = len(self.decoder.labels)
        self.words = np.zeros((n, WORDS), dtype=np.int32)
        self.words[:, :100] = rng.randint(-50, 2000, size=(n, 100))
        self.words[:, 100:200] = self.words[:, :100].astype(np.float32).view(np.int32)
        recs = rng.randint(0, ntab + 3, size=(n, 25))            # ids from ntab on are blanks
        for r in range(n):
            self.set_text(r, recs[r])
            self.set_id(r, int(rng.randint(0, 5000)))
        self.pts = rng.randint(-20, 3000, size=(n, 8)).astype(np.int64)
        self.keep = np.ones((n,), dtype=np.uint8)

    # ---- the words of one row
    def set_text(self, r, recs, emit=None):
        """Class ids of row r; `emit` None: the CTC collapse's own mask (TextDecoder.decode), else the given bit mask."""
        recs = np.asarray(recs, dtype=np.int64)
        ntab = len(self.decoder.labels)
        if emit is None:
            char = recs < ntab
            prev_char = np.concatenate(([False], char[:-1]))
            prev = np.concatenate(([-1], recs[:-1]))
            emit = int(sum(1 << c for c in range(25) if char[c] and (not prev_char[c] or recs[c] != prev[c])))
        self.words[r, 200:225] = recs
        self.words[r, 225] = np.uint32(emit).astype(np.int32)

    def set_id(self, r, track_id):
        self.words[r, 232:234] = np.array([track_id], dtype=np.int64).view(np.int32)

    def track_id(self, r):
        return int(self.words[r, 232:234].copy().view(np.int64)[0])

    def text(self, r):
        emit = int(np.uint32(self.words[r, 225]))
        return "".join(self.decoder.labels[self.words[r, 200 + c]] for c in range(25) if (emit >> c) & 1)

    # ---- what the writers take
    def frames(self):
        """Per frame of the call, the kept rows in `frame_lines`' form."""
        out = []
        for f in range(len(self.frame_rows) - 1):
            rows = []
            for r in range(self.frame_rows[f], self.frame_rows[f + 1]):
                if self.keep[r]:
                    seg = [self.words[r, :100].reshape(50, 2).tolist()]
                    rows.append([int(v) for v in self.pts[r]] + [self.track_id(r), self.text(r), seg])
            out.append(rows)
        return out

    def part(self, f0, f1):
        """The call that covers frames f0 .. f1 - 1 of this one."""
        c = Case.__new__(Case)
        c.name, c.voc, c.decoder = "%s[%d:%d]" % (self.name, f0, f1), self.voc, self.decoder
        r0, r1 = int(self.frame_rows[f0]), int(self.frame_rows[f1])
        c.first_frame = self.first_frame + f0
        c.frame_rows = (self.frame_rows[f0:f1 + 1] - r0).astype(np.int32)
        c.words, c.pts, c.keep = self.words[r0:r1].copy(), self.pts[r0:r1].copy(), self.keep[r0:r1].copy()
        return c


def writer_text(case, tmp_dir):
    """(json bytes, xml bytes) of the call as `results.write_video_results` writes its frames: the files of the annotation
    {first_frame + 1: .., ..} without header and footer, with the ",\\n" the rule puts in front of every frame but frame 0."""
    frames = case.frames()
    if not frames:
        return b"", b""
    annotation = {str(case.first_frame + f + 1): rows for f, rows in enumerate(frames)}
    jp, xp = os.path.join(str(tmp_dir), "w.json"), os.path.join(str(tmp_dir), "w.xml")
    results.write_video_results(annotation, jp, xp)
    js, xs = open(jp, "rb").read(), open(xp, "rb").read()
    head, foot = b'<?xml version="1.0" ?>\n<Frames>\n', b"</Frames>\n"
    assert js.startswith(b"{\n") and js.endswith(b"\n}") and xs.startswith(head) and xs.endswith(foot)
    return (b",\n" if case.first_frame else b"") + js[2:-2], xs[len(head):-len(foot)]


def statement_text(case):
    import result_text_statement as st
    frames = case.frames()
    js = "".join(st.frame_json(case.first_frame + f, rows) for f, rows in enumerate(frames))
    xs = "".join(st.frame_xml(case.first_frame + f, rows) for f, rows in enumerate(frames))
    return js.encode("utf-8"), xs.encode("utf-8")


def cases():
    out = []
    out.append(Case("one", "37", [1], seed=1))
    out.append(Case("empty-frames", "37", [0, 1, 0, 0, 2, 0], seed=2))       # first, two in a row in the middle, last
    out.append(Case("only-empty-frames", "37", [0, 0], seed=3))
    c = Case("dropped", "96", [3, 3, 3, 2, 1, 2], seed=4)                      # first / middle / last of a frame, a whole frame,
    c.keep[[0, 4, 8, 9, 10, 13]] = 0                                          # and the last row of the call
    out.append(c)
    c = Case("dropped-first-frame", "96", [2, 1], seed=5)
    c.keep[[0, 1]] = 0
    out.append(c)
    out.append(Case("65-rows", "37", [65], seed=6))
    c = Case("scan-blocks", "37", [SCAN_BLOCK - 1, 3, SCAN_BLOCK - 1], seed=7)  # 2 * block + 1 rows over 3 frames
    assert len(c.keep) == 2 * SCAN_BLOCK + 1
    c.keep[[0, SCAN_BLOCK - 1, SCAN_BLOCK, 2 * SCAN_BLOCK]] = 0
    out.append(c)
    c = Case("integers", "37", [len(I32_EDGE), len(ID_EDGE)], seed=8)
    for r, v in enumerate(I32_EDGE):
        c.words[r, :100] = np.roll(np.array(I32_EDGE * 13, dtype=np.int64)[:100], r).astype(np.int32)
        c.pts[r] = np.roll(np.array(I32_EDGE, dtype=np.int64), r)
    for k, v in enumerate(ID_EDGE):
        c.set_id(len(I32_EDGE) + k, v)
        c.pts[len(I32_EDGE) + k] = [v, -v if v > -2 ** 63 else v, 0, 5, 2 ** 31, -2 ** 31 - 1, 10 ** 18, -10 ** 18]
    out.append(c)
    c = Case("transcriptions-96", "96", [4], seed=9)
    quote = CTLABELS_96.index('"')
    c.set_text(0, [95] * 25)                                                  # empty: blanks only
    c.set_text(1, [quote] * 25, emit=(1 << 25) - 1)                           # 25 emitted '"' (the mask written directly)
    a, b = CTLABELS_96.index("a"), CTLABELS_96.index("&")
    c.set_text(2, [a, a, 95, a, 95, 95, b, b, a, 96, a, 95, b] + [95] * 12)   # blank-separated repeats, the collapse's own mask
    c.set_text(3, ([CTLABELS_96.index(ch) for ch in "<a h='x'>\\&\"q\"</a>~ `|{}"] + [95] * 25)[:25])
    out.append(c)
    c = Case("transcriptions-custom", "custom", [3, 1], seed=10)
    c.set_text(0, [CUSTOM.index("中")] * 25, emit=(1 << 25) - 1)          # 25 three-byte characters
    c.set_text(1, [CUSTOM.index("\U0001f600"), len(CUSTOM), CUSTOM.index("\U0001f600")] + [len(CUSTOM)] * 22)
    c.set_text(2, list(range(len(CUSTOM))) + [len(CUSTOM)] * (25 - len(CUSTOM)))
    c.set_text(3, [len(CUSTOM) + 1] * 25)
    out.append(c)
    for first in (8, 98, 998):                                                # keys 9, 10 / 99, 100, 101 / 999, 1000, 1001
        out.append(Case("first-frame-%d" % first, "37", [1, 2, 0][:2 if first == 8 else 3], first_frame=first, seed=11 + first))
    out.append(Case("six-frames", "96", [2, 0, 1, 3, 0, 2], seed=12))         # the split test: [0:3] + [3:6] == [0:6]
    return out


def dump(path, case_list):
    """The calls as tools/result_text_hostcheck.cpp reads them: little-endian, a count, then per call n, F, first_frame, ntab,
    words, pts, keep, frame_rows, json table, xml table."""
    import struct
    with open(path, "wb") as f:
        f.write(struct.pack("<q", len(case_list)))
        for c in case_list:
            jt, xt = results.text_tables(c.decoder)
            f.write(struct.pack("<4q", c.words.shape[0], len(c.frame_rows) - 1, c.first_frame, jt.shape[0]))
            f.write(np.ascontiguousarray(c.words, dtype="<i4").tobytes())
            f.write(np.ascontiguousarray(c.pts, dtype="<i8").tobytes())
            f.write(np.ascontiguousarray(c.keep, dtype=np.uint8).tobytes())
            f.write(np.ascontiguousarray(c.frame_rows, dtype="<i4").tobytes())
            f.write(jt.tobytes())
            f.write(xt.tobytes())
