"""The case list of the track vote tests, shared by the CPU statement test, the host check under sanitizers and the GPU test:
hand-made videos of `ops.result_rows` words (class ids, emit masks, track ids), keep flags and frame offsets -- the smallest
inputs at which the records / vote / scan / emit kernels can go wrong.  A case is one video; all of them together are about
three thousand rows.  numpy only."""
import struct

import numpy as np

from gomatching_amd import results
from gomatching_amd.predictor import CTLABELS_37, CTLABELS_96

WORDS = 234
RECORD_WORDS, BLOCK = 28, 256                                     # GOM_TV_RECORD_WORDS, GOM_TV_BLOCK (asserted by the ABI test)
# a custom dictionary: every escape of the XML writer, 2-, 3- and 4-byte code points, and "a" twice (two ids, one entry)
CUSTOM = ['"', "\\", "&", "<", ">", "'", "\x7f", "é", "中", "\U0001f600", "文", "a", "/", "€", "a", "b"]


class Labels:
    """What `results.txt_table` / `text_tables` need of a TextDecoder."""

    def __init__(self, labels):
        self.labels = list(labels)
        self.voc_size = len(self.labels) + 1


DECODERS = {"37": Labels(CTLABELS_37), "96": Labels(CTLABELS_96), "custom": Labels(CUSTOM)}


class Case:
    """One video.  `add(frame, track id, text)` in any order; `build()` puts the rows in file order."""

    def __init__(self, name, voc, frames=None):
        self.name, self.voc, self.decoder = name, voc, DECODERS[voc]
        self._rows, self._frames = [], frames

    def add(self, frame, tid, text="", keep=1, recs=None, emit=None):
        """text: characters of the dictionary, each emitted (the first id of a repeated label); or recs (25 ids) with the emit
        mask given directly."""
        if recs is None:
            blank = len(self.decoder.labels)
            recs = [self.decoder.labels.index(ch) for ch in text] + [blank] * (25 - len(text))
            emit = (1 << len(text)) - 1
        assert len(recs) == 25 and 0 <= emit < 1 << 25
        self._rows.append((int(frame), int(tid), [int(v) for v in recs], int(emit), int(keep)))
        return self

    def build(self):
        order = sorted(range(len(self._rows)), key=lambda k: self._rows[k][0])       # stable: row order within a frame stays
        rows = [self._rows[k] for k in order]
        n = len(rows)
        F = self._frames if self._frames is not None else (max(r[0] for r in rows) + 1 if rows else 0)
        self.words = np.zeros((n, WORDS), dtype=np.int32)
        self.keep = np.zeros((n,), dtype=np.uint8)
        counts = np.zeros((F,), dtype=np.int64)
        for r, (frame, tid, recs, emit, keep) in enumerate(rows):
            self.words[r, 200:225] = recs
            self.words[r, 225] = emit
            self.words[r, 232:234] = np.array([tid], dtype=np.int64).view(np.int32)
            self.keep[r] = keep
            counts[frame] += 1
        self.frame_rows = np.concatenate(([0], np.cumsum(counts))).astype(np.int64)
        return self

    def track_id(self, r):
        return int(self.words[r, 232:234].copy().view(np.int64)[0])

    def text(self, r):
        emit = int(self.words[r, 225])
        return "".join(self.decoder.labels[self.words[r, 200 + c]] for c in range(25) if (emit >> c) & 1)

    def annotation(self):
        """The video as `results.write_video_results` takes it: {frame key: the kept rows in `frame_lines`' form}."""
        out = {}
        for f in range(len(self.frame_rows) - 1):
            out[str(f + 1)] = [[0, 0, 9, 0, 9, 9, 0, 9, self.track_id(r), self.text(r), [[[0, 0], [9, 9]]]]
                               for r in range(self.frame_rows[f], self.frame_rows[f + 1]) if self.keep[r]]
        return out

    def table(self):
        return results.txt_table(self.decoder)

    def statement(self):
        import track_vote_statement as st
        return st.statement(self.words, self.keep, self.table())


def _distinct(i):
    """A text of letters that no other i shares (and that is not "win")."""
    return "q" + "".join("abcdefghij"[int(d)] for d in str(i))


def cases():
    out = []
    out.append(Case("tie-2-2", "37").add(0, 5, "b").add(1, 5, "a").add(2, 5, "a").add(3, 5, "b"))   # the first seen wins: "b"
    out.append(Case("tie-3", "37").add(0, 1, "x").add(0, 2, "k").add(1, 1, "y").add(2, 1, "z"))
    out.append(Case("3-against-2", "37").add(0, 3, "a").add(1, 3, "b").add(2, 3, "b").add(3, 3, "a").add(4, 3, "b"))
    out.append(Case("single-rows", "96").add(0, 4, "Exit").add(0, 8, "~").add(2, 6, "a b").add(5, 1, "").add(5, 0, '"&<'))
    c = Case("dropped-track", "37", frames=4)                     # track 7 has no kept row: no line; the last frame is empty
    c.add(0, 7, "gone", keep=0).add(1, 7, "gone", keep=0).add(0, 2, "stay").add(2, 2, "stay", keep=0).add(2, 2, "sta")
    out.append(c)
    c = Case("id-order", "37")                                    # integer order, not string order; the high word; a negative id
    for k, tid in enumerate((2, 10, 9, 0, 2 ** 31 + 5, 2 ** 40 + 1, -3, 2 ** 63 - 1, -2 ** 63)):
        c.add(0, tid, "t%d" % k).add(1, tid, "t%d" % k)
    out.append(c)
    out.append(Case("empty-text", "37").add(0, 1, "").add(1, 1, "a").add(2, 1, "").add(0, 2, "a").add(1, 2, "").add(2, 2, "a"))
    c = Case("long-entries", "custom")                            # 25 characters of 3 and of 4 bytes: 75 and 100 bytes
    c.add(0, 1, "中" * 25).add(1, 1, "中" * 24 + "文").add(2, 1, "中" * 25)
    c.add(0, 2, "\U0001f600" * 24).add(1, 2, "\U0001f600" * 25).add(2, 2, "\U0001f600" * 24 + "a").add(3, 2, "\U0001f600" * 25)
    c.add(0, 3, "".join(CUSTOM[:14]))                             # every entry once, the escapes included
    out.append(c)
    c = Case("last-character", "37")                              # 25 characters that differ in the last one only
    c.add(0, 1, "a" * 24 + "b").add(1, 1, "a" * 24 + "c").add(2, 1, "a" * 24 + "c")
    out.append(c)
    c = Case("prefix", "37")                                      # one text a prefix of the other: a tie, then a majority
    c.add(0, 1, "abc").add(1, 1, "ab").add(0, 2, "ab").add(1, 2, "abc").add(2, 2, "abc").add(0, 3, "abcd").add(1, 3, "abc")
    c.add(2, 3, "abc").add(3, 3, "abcd").add(4, 3, "abcd")
    out.append(c)
    c = Case("same-text-other-recs", "37")                        # "ab" from three different recs rows, against "ba" twice
    a, b, blank = CTLABELS_37.index("a"), CTLABELS_37.index("b"), 36
    c.add(0, 1, recs=[b, a] + [blank] * 23, emit=0b11).add(1, 1, recs=[a, a, b, b] + [blank] * 21, emit=0b0101)
    c.add(2, 1, recs=[b, a] + [blank] * 23, emit=0b11).add(3, 1, recs=[blank, a, blank, b] + [blank] * 21, emit=0b1010)
    c.add(4, 1, recs=[a, b, b] + [37] * 22, emit=0b011)
    out.append(c)
    c = Case("shared-entry", "custom")                            # ids 11 and 14 are both "a": counted together, 3 against 2
    blank = len(CUSTOM)
    c.add(0, 1, "b").add(1, 1, recs=[11] + [blank] * 24, emit=1).add(2, 1, "b").add(3, 1, recs=[14] + [blank] * 24, emit=1)
    c.add(4, 1, recs=[14] + [blank] * 24, emit=1)
    out.append(c)
    c = Case("tiles", "37")                                       # the winner's first row in the last, partial tile of its track
    for tid, L in enumerate((64, 65, BLOCK, BLOCK + 1, 600)):
        for i in range(L):
            c.add(i, tid, "win" if i >= L - 3 else _distinct(i // 2 if i < 8 else i))      # pairs at the front: counts of 2
    out.append(c)
    c = Case("300-tracks", "37")                                  # more tracks than one scan block; ids in no order
    ids = np.random.RandomState(3).permutation(300) * 7 + 1
    for k, tid in enumerate(ids):
        c.add(0, tid, _distinct(k)).add(1, tid, _distinct(k + 1)).add(2, tid, _distinct(k + 1))
    out.append(c)
    out.append(Case("two-rows-one-frame", "37").add(0, 4, "a").add(0, 4, "b").add(1, 4, "b").add(1, 9, "c").add(1, 9, "c"))
    out.append(Case("no-kept-rows", "37", frames=3).add(0, 1, "a", keep=0).add(2, 2, "b", keep=0))
    out.append(Case("no-rows", "37", frames=2))
    return [c.build() for c in out]


def dump(path, case_list):
    """The videos as tools/track_vote_hostcheck.cpp reads them: little-endian, a count, then per video n, ntab, words, keep and
    the txt table."""
    with open(path, "wb") as f:
        f.write(struct.pack("<q", len(case_list)))
        for c in case_list:
            tab = c.table()
            f.write(struct.pack("<2q", c.words.shape[0], tab.shape[0]))
            f.write(np.ascontiguousarray(c.words, dtype="<i4").tobytes())
            f.write(np.ascontiguousarray(c.keep, dtype=np.uint8).tobytes())
            f.write(tab.tobytes())
