"""Lexicon correction of transcriptions: every recognised word is snapped to the nearest word of a vocabulary.

    python -m gomatching_amd.lexicon --results RES --lexicon FILE|DIR [--pairs FILE] [--max-dist N]
            [--unmatched keep|drop] [--output DIR] [--host-match]
    python -m gomatching_amd.eval ... --lexicon FILE|DIR [--lexicon-pairs FILE] [--lexicon-max-dist N]
            [--lexicon-unmatched keep|drop]

The rule is the reference's `find_match_word` (third_party/adet/evaluation/text_evaluation_all.py:249-264, accepted at :332,
lexicon and pair-list parsing at :193-215) and is stated once, in include/gomatching_hip.h ("Lexicon correction"): both sides
upper-cased with `str.upper` and taken as code points, at most 64 of them; the Levenshtein distance without transposition; the
LOWEST index at the smallest distance; (-1, 100) for an empty lexicon; accepted when the distance is at most `max_dist`
(default 1, the reference's `< 1.5`); an accepted transcription becomes the display form `pairs[norm(word)]`.

The command reads RES/jsons/<video>.json (every field of a row: points, ID, transcription, segmentation), rewrites the
transcriptions and writes OUT/jsons/<video>.json and OUT/preds/res_<stem>.xml through `results.write_video_results` and
OUT/preds/res_<stem>.txt through `results.write_track_transcriptions` -- so the track vote is taken over the CORRECTED words.
OUT defaults to RES/lexicon; the originals are never touched.  `--lexicon DIR` means per-video lexicons DIR/<video>.txt with
optional DIR/<video>.pairs.txt: every video is a segment of its own.  Either way the distinct (segment, normalised string)
pairs of the WHOLE result set go up in ONE upload, are matched by ONE `gom_lexicon_match_u32` launch (csrc/lexicon.hip) and
come back in ONE copy; `--host-match` runs `host_match`, the same rule in numpy vectorised over a segment's words, and
writes the same bytes.

`eval --device-lexicon` does not go through the files at all: `DeviceLexicon` (the words, the decoder's table of upper-cased
code points and the three display tables of a Lexicon, uploaded once) and `RowCorrection` are what `results.rows_text` takes to
correct a call's rows where they lie on the GPU (csrc/lexicon_rows.hip; the rule is in include/gomatching_hip.h,
`gom_lexicon_rows_*`), and `correct_results(skip=)` leaves the videos corrected that way alone.  The bytes are the same.

Deliberate differences: the correction applies per instance and the track vote is retaken (the reference has no tracks at
that point); unmatched detections are kept by default, `--unmatched drop` removes their rows as the reference's `*_full` files
do; strong lexicons are per video, not per image; blank lexicon lines are skipped (the reference would look up '').
UNPINNED: the arithmetic of the `editdistance` library, which is plain Levenshtein; everything else is pinned by
tests/golden/lexicon_match.json, which the reference's own functions wrote.

Exit status 2, with a message: a missing directory or file, an unreadable json, a video without its lexicon or without its
XML under RES/preds, a lexicon line or a transcription above the length limit, a word missing from the pair list.  Without
a GPU and without `--host-match` the command refuses (status 1): the numpy path is a choice, not a fall-back.
"""
import argparse
import json
import os
import sys

import numpy as np

from . import results as _results
from .lib import CONSTANTS as _ABI

MAX_LEN = _ABI["GOM_LEXICON_MAX_LEN"]
NO_MATCH_DIST = _ABI["GOM_LEXICON_NO_MATCH_DIST"]


class LexiconError(Exception):
    """An input the command cannot use; the message names it.  Exit status 2."""


class NoDeviceError(Exception):
    """The device path was asked for and there is no GPU.  Exit status 1: there is no quiet fall-back to numpy."""


def norm(s):
    return s.upper()


# ------------------------------------------------------------------------------------------------- lexicons
class Lexicon:
    """`words`: the stripped non-blank lines in file order; `normal`: their normal forms; `pairs`: normal form -> display."""

    def __init__(self, words, pairs, path="<lexicon>"):
        self.words, self.pairs, self.path = list(words), pairs, path
        self.normal = [norm(w) for w in self.words]

    def __len__(self):
        return len(self.words)

    def display(self, index):
        return self.pairs[self.normal[index]]


def _lines(path):
    try:
        with open(path, "r", encoding="utf-8") as f:
            return f.readlines()
    except (OSError, UnicodeDecodeError) as e:
        raise LexiconError("%s: cannot be read as text (%s)" % (path, e))


def load_lexicon(path, pairs=None):
    """The lexicon file `path` and the pair-list file `pairs` (or None) -> Lexicon, by the rule of include/gomatching_hip.h."""
    words, where = [], []
    for k, line in enumerate(_lines(path)):
        line = line.strip()
        if not line:
            continue
        if len(norm(line)) > MAX_LEN:
            raise LexiconError("%s: line %d has %d code points after upper-casing; at most %d are matched"
                               % (path, k + 1, len(norm(line)), MAX_LEN))
        words.append(line)
        where.append(k + 1)
    table = {}
    if pairs is not None:
        for line in _lines(pairs):
            line = line.strip()
            key = line.split(" ")[0].upper()
            table[key] = line[len(key) + 1:]
    else:
        for w in words:
            table[norm(w)] = w
    for w, k in zip(words, where):
        if norm(w) not in table:
            raise LexiconError("%s: line %d: the word %r has no entry in the pair list %s" % (path, k, w, pairs))
    return Lexicon(words, table, path)


# ------------------------------------------------------------------------------------------------- CSR marshalling
def pack(strings):
    """Strings -> (code points int32 [n], offsets int32 [len + 1]); a string is its sequence of Unicode code points."""
    lens = np.fromiter((len(s) for s in strings), dtype=np.int64, count=len(strings))
    off = np.zeros(len(strings) + 1, dtype=np.int64)
    np.cumsum(lens, out=off[1:])
    if off[-1] > 2 ** 31 - 1:
        raise LexiconError("more than 2^31 - 1 code points in one call")
    chars = np.frombuffer("".join(strings).encode("utf-32-le", "surrogatepass"), dtype="<i4").astype(np.int32)
    return chars, off.astype(np.int32)


def _check_csr(q_chars, q_off, q_seg, w_chars, w_off, seg_off):
    arrs = [np.ascontiguousarray(a, dtype=np.int32).reshape(-1) for a in (q_chars, q_off, q_seg, w_chars, w_off, seg_off)]
    q_chars, q_off, q_seg, w_chars, w_off, seg_off = arrs
    S, W, n_seg = q_seg.size, w_off.size - 1, seg_off.size - 1
    if q_off.size != S + 1 or W < 0 or n_seg < 0:
        raise ValueError("q_off must be [S+1] for q_seg [S], w_off [W+1] and seg_off [n_seg+1]")
    for off, total, name in ((q_off, q_chars.size, "q_off"), (w_off, w_chars.size, "w_off"), (seg_off, W, "seg_off")):
        if off[0] != 0 or off[-1] != total or (np.diff(off) < 0).any():
            raise ValueError("%s is not a CSR offset array over its %d entries" % (name, total))
    if S and (n_seg == 0 or q_seg.min() < 0 or q_seg.max() >= n_seg):
        raise ValueError("q_seg names a segment outside [0, %d)" % n_seg)
    max_len = max(int(np.diff(q_off).max()) if S else 0, int(np.diff(w_off).max()) if W else 0)
    if max_len > MAX_LEN:
        raise ValueError("a query or a word of %d code points: at most %d are matched" % (max_len, MAX_LEN))
    return arrs, max_len


# ------------------------------------------------------------------------------------------------- the rule, on the host
def segment_matrix(w_chars, w_off, first, last):
    """The words first .. last - 1 as a padded matrix: (code points int32 [n, L] with -1 behind a word's end, lengths [n])."""
    lens = (w_off[first + 1:last + 1] - w_off[first:last]).astype(np.int64)
    n, L = lens.size, int(lens.max()) if lens.size else 0
    mat = np.full((n, L), -1, dtype=np.int32)
    col = np.arange(L)[None, :]
    inside = col < lens[:, None]
    mat[inside] = w_chars[w_off[first]:w_off[last]]
    return mat, lens


def distances(q, mat, lens):
    """Levenshtein distances of the query `q` (code points [m]) and every word of `segment_matrix`'s pair: int32 [n].  The
    two-row programme over the query's characters, vectorised over the words; within a row the insertions' dependency along
    the word, cur[j] = min(best[j], cur[j-1] + 1), is the running minimum of best[k] - k, plus j."""
    n, L = mat.shape
    ramp = np.arange(L + 1, dtype=np.int16)[None, :]                  # (every value is at most 2 * MAX_LEN: int16 rows)
    prev = np.repeat(ramp, n, axis=0)
    for i, c in enumerate(np.asarray(q).tolist()):
        cur = np.empty_like(prev)
        cur[:, 0] = i + 1
        np.minimum(prev[:, :-1] + (mat != c), prev[:, 1:] + np.int16(1), out=cur[:, 1:])
        cur -= ramp
        np.minimum.accumulate(cur, axis=1, out=cur)
        cur += ramp
        prev = cur
    return prev[np.arange(n), lens].astype(np.int32)


def host_match(q_chars, q_off, q_seg, w_chars, w_off, seg_off):
    """The rule of `gom_lexicon_match_u32` in numpy, on the kernel's own arguments as numpy arrays -> (index int32 [S],
    dist int32 [S]): per query the lowest index at the smallest distance within its segment, (-1, 100) for an empty one."""
    (q_chars, q_off, q_seg, w_chars, w_off, seg_off), _ = _check_csr(q_chars, q_off, q_seg, w_chars, w_off, seg_off)
    S = q_seg.size
    index = np.full(S, -1, dtype=np.int32)
    dist = np.full(S, NO_MATCH_DIST, dtype=np.int32)
    for g in np.unique(q_seg).tolist():
        first, last = int(seg_off[g]), int(seg_off[g + 1])
        if last == first:
            continue
        mat, lens = segment_matrix(w_chars, w_off, first, last)
        for s in np.nonzero(q_seg == g)[0].tolist():
            d = distances(q_chars[q_off[s]:q_off[s + 1]], mat, lens)
            k = int(np.argmin(d))                                   # the first occurrence of the minimum
            index[s], dist[s] = k, d[k]
    return index, dist


def device_match(q_chars, q_off, q_seg, w_chars, w_off, seg_off):
    """The same through `ops.lexicon_match`: the six arrays go up as ONE buffer, one launch, both results come back in ONE
    copy.  numpy in, numpy out."""
    arrs, max_len = _check_csr(q_chars, q_off, q_seg, w_chars, w_off, seg_off)
    import torch
    if not torch.cuda.is_available():
        raise NoDeviceError("no GPU: transcriptions are matched by gom_lexicon_match_u32; pass --host-match for the numpy path")
    from . import ops
    S = arrs[2].size
    packed = torch.from_numpy(np.concatenate(arrs)).cuda()
    views, o = [], 0
    for a in arrs:
        views.append(packed[o:o + a.size])
        o += a.size
    out = torch.empty((2, S), dtype=torch.int32, device=packed.device)
    ops.lexicon_match(*views, max_len=max_len, out=out)
    both = out.cpu().numpy()
    return both[0].copy(), both[1].copy()


def match_strings(items, lexicons, host=False):
    """items: [(segment, normalised string)], lexicons: [Lexicon] by segment -> (index [n], dist [n]) in ONE match call."""
    q_chars, q_off = pack([s for _, s in items])
    q_seg = np.asarray([g for g, _ in items], dtype=np.int32).reshape(-1)
    w_chars, w_off = pack([w for lex in lexicons for w in lex.normal])
    seg_off = np.zeros(len(lexicons) + 1, dtype=np.int32)
    np.cumsum([len(lex) for lex in lexicons], out=seg_off[1:])
    return (host_match if host else device_match)(q_chars, q_off, q_seg, w_chars, w_off, seg_off)


# ------------------------------------------------------------------------------------------------- rows on the device
NORM_WORDS = _ABI["GOM_LR_NORM_WORDS"]
DISPLAY_TEXT_MAX = 25 * (_ABI["GOM_RT_ENTRY_BYTES"] - 1)         # a JSON or XML display form: no longer than 25 table entries
DISPLAY_TXT_MAX = 4 * _ABI["GOM_TV_TEXT_WORDS"]                   # a txt display form: what a vote record holds


def norm_table(decoder):
    """The per-vocabulary table of the device queries (include/gomatching_hip.h, `gom_lexicon_rows_*`), int32 [voc_size - 1, 4]:
    a count and the code points of label.upper().  `str.upper` works character by character (tests/test_lexicon_rows_cpu.py), so
    the query of a row is its characters' entries, one after another.  A label that is not one character, or whose upper-case
    form has more than 3 code points, is a ValueError naming the entry."""
    labels = list(decoder.labels)
    tab = np.zeros((len(labels), NORM_WORDS), dtype=np.int32)
    for i, ch in enumerate(labels):
        up = norm(ch)
        if len(ch) != 1 or len(up) > NORM_WORDS - 1:
            raise ValueError("dictionary entry %d (%r) is upper-cased to %d code points, a norm-table entry holds %d"
                             % (i, ch, len(up), NORM_WORDS - 1))
        tab[i, 0] = len(up)
        tab[i, 1:1 + len(up)] = [ord(c) for c in up]
    return tab


def txt_form(text):
    """`text` as `results.write_track_transcriptions` reads it back from the XML minidom wrote it into (the round trip of
    `results.txt_table`, over a whole string)."""
    import xml.etree.ElementTree as ET
    parser = ET.XMLParser(encoding="utf-8")
    parser.feed(('<a v="%s"/>' % _results._xml_attribute(text)).encode("utf-8"))
    return parser.close().attrib["v"]


def display_tables(lex, shortcut=True):
    """The three display tables of a Lexicon, each (bytes uint8 [>= 1], offsets int32 [W + 1], bytes in use): entry i is the
    display form of word i as the JSON writer, the XML writer and the txt reader have it, over the whole form.  A form above
    its stream's limit, or one a writer cannot take, is a LexiconError naming the file and the word.
    The libraries are asked once per distinct character whether all three leave it as it is (they work character by character:
    `results.text_tables`, `results.txt_table`); a form of such characters alone is its own UTF-8 bytes in all three tables, any
    other form goes through the libraries whole.  shortcut=False sends every form through the libraries whole: the same tables
    (tests/test_lexicon_rows_cpu.py compares the two)."""
    forms = [[], [], []]
    plain = {}

    def is_plain(ch):
        if ch not in plain:
            try:
                ch.encode("utf-8")
                plain[ch] = json.dumps(ch, ensure_ascii=False)[1:-1] == ch and _results._xml_attribute(ch) == ch and txt_form(ch) == ch
            except Exception:
                plain[ch] = False
        return plain[ch]

    for i in range(len(lex)):
        d = str(lex.display(i))
        try:
            if shortcut and all(is_plain(ch) for ch in d):
                data = [d.encode("utf-8")] * 3
            else:
                texts = (json.dumps(d, ensure_ascii=False)[1:-1], _results._xml_attribute(d), txt_form(d))
                data = [t.encode("utf-8") for t in texts]
        except Exception as e:                                   # (the XML parser's own error type, UnicodeEncodeError, ...)
            raise LexiconError("%s: word %d (%r): the display form %r cannot be written (%s)" % (lex.path, i + 1, lex.words[i], d, e))
        for b, limit, name in zip(data, (DISPLAY_TEXT_MAX, DISPLAY_TEXT_MAX, DISPLAY_TXT_MAX), ("JSON", "XML", "txt")):
            if len(b) > limit:
                raise LexiconError("%s: word %d (%r): the display form %r is %d bytes in the %s file, the device path takes at "
                                   "most %d (run without --device-lexicon)" % (lex.path, i + 1, lex.words[i], d, len(b), name, limit))
        for k in range(3):
            forms[k].append(data[k])
    out = []
    for items in forms:
        off = np.zeros(len(items) + 1, dtype=np.int64)
        np.cumsum([len(b) for b in items], out=off[1:])
        if off[-1] > 2 ** 31 - 1:
            raise LexiconError("%s: more than 2^31 - 1 bytes of display forms" % lex.path)
        data = np.frombuffer(b"".join(items) or b"\0", dtype=np.uint8).copy()
        out.append((data, off.astype(np.int32), int(off[-1])))
    return out


def checked_display_tables(lex):
    """`display_tables(lex)`, built once per Lexicon and kept on it: the host check of the device path's limits (a command
    runs it for every lexicon it needs before it builds or uploads anything) and what `DeviceLexicon` uploads."""
    if "_display_tables" not in lex.__dict__:
        lex.__dict__["_display_tables"] = display_tables(lex)
    return lex.__dict__["_display_tables"]


class DeviceLexicon:
    """One Lexicon on one device, for `results.rows_text(lexicon=...)`: the words' code points (CSR, one segment), the three
    display tables and the decoder's norm table, uploaded once.  `DeviceLexicon.of` caches per (lexicon, decoder, device); the
    limits of the display forms are checked here, before any upload."""

    def __init__(self, lex, decoder, device):
        import torch
        if not torch.cuda.is_available():
            raise NoDeviceError("no GPU: rows are corrected by csrc/lexicon_rows.hip")
        self.lexicon, self.decoder, self.device = lex, decoder, device
        tables = checked_display_tables(lex)                     # (raises before anything is uploaded)
        norm_tab = norm_table(decoder)
        w_chars, w_off = pack(lex.normal)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
        self.W = len(lex)
        self.w_chars, self.w_off = up(w_chars), up(w_off)
        self.seg_off = up(np.asarray([0, self.W], dtype=np.int32))
        self.norm_tab = up(norm_tab)
        self.json_disp, self.xml_disp, self.txt_disp = [(up(d), up(o), nb) for d, o, nb in tables]

    @classmethod
    def of(cls, lex, decoder, device):
        cache = lex.__dict__.setdefault("_device", {})
        key = (tuple(decoder.labels), str(device))               # (the vocabulary itself: an id may be reused)
        if key not in cache:
            cache[key] = cls(lex, decoder, device)
        return cache[key]


class RowCorrection:
    """What `results.rows_text` needs to correct a call's rows: a DeviceLexicon, the acceptance (`max_dist`, `unmatched`), the
    `results.TrackVote` of the corrected words, and where the rows come from (for the error that names video and frame).  The
    figures of the device path add up in `rows` (kept rows in), `accepted` and `dropped`."""

    def __init__(self, device_lexicon, max_dist=1, unmatched="keep", vote=None, video="<video>"):
        if unmatched not in ("keep", "drop"):
            raise ValueError("unmatched must be 'keep' or 'drop', not %r" % (unmatched,))
        if max_dist < 0:
            raise ValueError("max_dist must not be negative")
        self.lexicon, self.max_dist, self.unmatched, self.vote, self.video = device_lexicon, int(max_dist), unmatched, vote, video
        self.rows = self.accepted = self.dropped = 0


# ------------------------------------------------------------------------------------------------- annotations
def correct_annotations(annotations, lexicons, max_dist=1, unmatched="keep", host=False):
    """annotations {video: {frame: [rows]}} (rows as `results.write_video_results` takes them), lexicons {video: Lexicon} or
    one Lexicon for all -> ({video: corrected annotation}, figures).  The distinct (lexicon, norm(transcription)) pairs of
    ALL videos are matched once and mapped back; the inputs are not modified."""
    if unmatched not in ("keep", "drop"):
        raise ValueError("unmatched must be 'keep' or 'drop', not %r" % (unmatched,))
    segs, seg_of, items, slot = [], {}, [], {}
    for video, annotation in annotations.items():
        lex = lexicons if isinstance(lexicons, Lexicon) else lexicons[video]
        if id(lex) not in seg_of:
            seg_of[id(lex)] = len(segs)
            segs.append(lex)
        g = seg_of[id(lex)]
        for frame, rows in annotation.items():
            for row in rows:
                q = norm(str(row[9]))
                if len(q) > MAX_LEN:
                    raise LexiconError("video %s, frame %s: a transcription of %d code points after upper-casing; at most %d "
                                       "are matched" % (video, frame, len(q), MAX_LEN))
                if (g, q) not in slot:
                    slot[(g, q)] = len(items)
                    items.append((g, q))
    if items:
        index, dist = match_strings(items, segs, host=host)
        index, dist = index.tolist(), dist.tolist()
    out, rows_in, changed, dropped = {}, 0, 0, 0
    for video, annotation in annotations.items():
        lex = lexicons if isinstance(lexicons, Lexicon) else lexicons[video]
        g = seg_of[id(lex)]
        fixed = {}
        for frame, rows in annotation.items():
            fixed[frame] = []
            for row in rows:
                rows_in += 1
                k = slot[(g, norm(str(row[9])))]
                if index[k] >= 0 and dist[k] <= max_dist:
                    word = lex.display(index[k])
                    changed += word != row[9]
                    fixed[frame].append(list(row[:9]) + [word] + list(row[10:]))
                elif unmatched == "keep":
                    fixed[frame].append(list(row))
                else:
                    dropped += 1
        out[video] = fixed
    return out, {"videos": len(out), "rows": rows_in, "distinct": len(items), "changed": changed, "dropped": dropped}


def correct_annotation(annotation, lexicon, max_dist=1, unmatched="keep", host=False, video="<annotation>"):
    """One video's {frame: [rows]} -> the corrected {frame: [rows]}."""
    return correct_annotations({video: annotation}, lexicon, max_dist, unmatched, host)[0][video]


# ------------------------------------------------------------------------------------------------- result directories
def read_annotation(json_path):
    """RES/jsons/<video>.json -> {frame: [rows]} as `results.write_video_results` takes it."""
    try:
        with open(json_path, "r", encoding="utf-8") as f:
            doc = json.load(f)
        annotation = {}
        for frame, recs in doc.items():
            annotation[frame] = [list(r["points"][:8]) + [r["ID"], r["transcription"]] +
                                 ([r["segmentation"]] if "segmentation" in r else []) for r in recs]
            if any(len(row) < 10 for row in annotation[frame]):
                raise ValueError("a row with fewer than 8 point coordinates")
    except (OSError, ValueError, KeyError, TypeError, AttributeError) as e:
        raise LexiconError("%s: cannot be read as a result json (%s: %s)" % (json_path, type(e).__name__, e))
    return annotation


def xml_stem(video, xml_dir):
    """The stem the video's XML was written under: `results.result_names` without a data type or with ICDAR15's."""
    stems = [_results.result_names(video, None)[0]]
    if len(video.split("_")) > 1:
        stems.append(_results.result_names(video, "ICDAR15")[0])
    for stem in stems:
        if os.path.isfile(os.path.join(xml_dir, "res_%s.xml" % stem)):
            return stem
    raise LexiconError("%s: video %s has no res_%s.xml there" % (xml_dir, video, " / res_".join(stems)))


def load_lexicons(lexicon, pairs, videos):
    """`--lexicon FILE [--pairs FILE]` -> one Lexicon; `--lexicon DIR` -> {video: Lexicon} from DIR/<video>.txt and the
    optional DIR/<video>.pairs.txt."""
    if os.path.isdir(lexicon):
        if pairs is not None:
            raise LexiconError("--pairs goes with a lexicon FILE; a lexicon directory holds <video>.pairs.txt files")
        out = {}
        for video in videos:
            path, ppath = os.path.join(lexicon, video + ".txt"), os.path.join(lexicon, video + ".pairs.txt")
            if not os.path.isfile(path):
                raise LexiconError("%s: video %s has no lexicon there (%s.txt)" % (lexicon, video, video))
            out[video] = load_lexicon(path, ppath if os.path.isfile(ppath) else None)
        return out
    if not os.path.isfile(lexicon):
        raise LexiconError("%s: no such lexicon file or directory" % lexicon)
    if pairs is not None and not os.path.isfile(pairs):
        raise LexiconError("%s: no such pair-list file" % pairs)
    return load_lexicon(lexicon, pairs)


def correct_results(results_dir, out_dir=None, lexicon=None, pairs=None, max_dist=1, unmatched="keep", host=False, skip=()):
    """RES/jsons/*.json -> OUT/jsons, OUT/preds (xml and txt) with corrected transcriptions; -> the figures of
    `correct_annotations`.  One match call for the whole directory.  `skip`: videos (the json stems) that are left alone -- those
    whose corrected files, the txt included, the device path wrote already (`results.rows_text(lexicon=)`); their files are
    neither read nor written, and the figures do not count them."""
    json_dir, xml_dir = os.path.join(results_dir, "jsons"), os.path.join(results_dir, "preds")
    for d in (results_dir, json_dir, xml_dir):
        if not os.path.isdir(d):
            raise LexiconError("%s: no such directory" % d)
    if out_dir is None:
        out_dir = os.path.join(results_dir, "lexicon")
    skip = frozenset(skip)
    videos = sorted(f[:-len(".json")] for f in os.listdir(json_dir) if f.endswith(".json"))
    stems = {v: xml_stem(v, xml_dir) for v in videos}
    skipped_xml = ["res_%s.xml" % stems[v] for v in videos if v in skip]
    videos = [v for v in videos if v not in skip]
    lexicons = load_lexicons(lexicon, pairs, videos)
    annotations = {v: read_annotation(os.path.join(json_dir, v + ".json")) for v in videos}
    fixed, figures = correct_annotations(annotations, lexicons, max_dist, unmatched, host)
    out_json, out_xml = os.path.join(out_dir, "jsons"), os.path.join(out_dir, "preds")
    os.makedirs(out_json, exist_ok=True)
    os.makedirs(out_xml, exist_ok=True)
    for v in videos:
        _results.write_video_results(fixed[v], os.path.join(out_json, v + ".json"), os.path.join(out_xml, "res_%s.xml" % stems[v]))
    _results.write_track_transcriptions(out_xml, skip=skipped_xml)
    figures["output"] = out_dir
    return figures


# ------------------------------------------------------------------------------------------------- command line
def _parser():
    ap = argparse.ArgumentParser(prog="python -m gomatching_amd.lexicon", description=__doc__.split("\n\n")[0])
    ap.add_argument("--results", required=True, metavar="RES", help="a result directory: RES/jsons/<video>.json, RES/preds/res_*.xml")
    ap.add_argument("--lexicon", required=True, metavar="FILE|DIR",
                    help="a vocabulary file (one word per line), or a directory of per-video <video>.txt [+ <video>.pairs.txt]")
    ap.add_argument("--pairs", default=None, metavar="FILE", help="pair list: `KEY display form` per line (default: the lexicon's lines)")
    ap.add_argument("--max-dist", type=int, default=1, metavar="N", help="accept a word at an edit distance of at most N (default 1)")
    ap.add_argument("--unmatched", choices=("keep", "drop"), default="keep",
                    help="a transcription without an accepted word is kept unchanged (default) or its row removed")
    ap.add_argument("--output", default=None, metavar="DIR", help="default RES/lexicon")
    ap.add_argument("--host-match", action="store_true", help="match in numpy instead of on the GPU (the same bytes)")
    return ap


def main(argv=None):
    args = _parser().parse_args(argv)
    try:
        if args.max_dist < 0:
            raise LexiconError("--max-dist must not be negative")
        figures = correct_results(args.results, args.output, args.lexicon, args.pairs, args.max_dist, args.unmatched,
                                  host=args.host_match)
    except LexiconError as e:
        sys.stderr.write("lexicon: %s\n" % e)
        return 2
    except NoDeviceError as e:
        sys.stderr.write("lexicon: %s\n" % e)
        return 1
    print("lexicon: %(videos)d videos, %(rows)d rows, %(distinct)d distinct strings matched, %(changed)d changed, "
          "%(dropped)d dropped -> %(output)s" % figures)
    return 0


if __name__ == "__main__":
    sys.exit(main())
