"""The case list of the tests of the lexicon correction of rows, shared by the CPU statement test, the host check under
sanitizers and the GPU test: calls of tests/result_text_cases.py with a lexicon, an acceptance and an `unmatched` mode each, plus
rows made for the lexicon path -- and the two references every test compares with: the plain-Python statement
(tests/lexicon_rows_statement.py) and the bytes of the host path (`lexicon.correct_annotation(host=True)` ->
`results.write_video_results` -> `results.write_track_transcriptions`).  numpy only."""
import json
import os
import struct

import numpy as np

import lexicon_rows_statement as lrs
import result_text_cases as rc
from gomatching_amd import lexicon, results
from gomatching_amd.predictor import CTLABELS_96

UPPER = ["ß", "ﬃ", "ΐ"]                                           # str.upper gives 2, 3 and 3 code points
rc.DECODERS.setdefault("lex", rc.Labels(rc.CUSTOM + UPPER + list("xyz")))


def lex_of(words, pairs=None):
    """A Lexicon of `words`; pairs: {word: display form} (default: the word itself), keyed by the word as written."""
    table = {lexicon.norm(w): w for w in words}
    for w, d in (pairs or {}).items():
        table[lexicon.norm(w)] = d
    return lexicon.Lexicon(words, table, "<case>")


def set_str(case, r, text):
    """Row r emits exactly the characters of `text` (the emit mask written directly, blanks behind)."""
    labels = case.decoder.labels
    ids = [labels.index(ch) for ch in text]
    assert len(ids) <= 25
    case.set_text(r, ids + [len(labels)] * (25 - len(ids)), emit=(1 << len(ids)) - 1)


class LexCase:
    def __init__(self, name, case, lex, max_dist=1, unmatched="keep"):
        self.name, self.case, self.lex, self.max_dist, self.unmatched = name, case, lex, max_dist, unmatched

    def part(self, f0, f1):
        return LexCase("%s[%d:%d]" % (self.name, f0, f1), self.case.part(f0, f1), self.lex, self.max_dist, self.unmatched)


def words_of(case, k, seed, limit=24):
    """A lexicon from the call's own transcriptions (the first `limit` distinct ones: the plain-Python match is slow): every
    k-th text verbatim, every k-th + 1 with one edit, the rest left out; display forms differ from the words (a suffix), so
    that a correction shows."""
    texts = sorted({case.text(r) for r in range(len(case.keep)) if case.text(r) and len(lexicon.norm(case.text(r))) < 60})[:limit]
    rng = np.random.RandomState(seed)
    words = []
    for i, t in enumerate(texts):
        if i % k == 0:
            words.append(t)
        elif i % k == 1:
            j = int(rng.randint(0, len(t)))
            words.append(t[:j] + t[j + 1:] if len(t) > 1 else t + t)
    words = [w for w in words if w.strip() == w and w]
    return lex_of(words, {w: w + "~" for w in words})


def cases():
    out = []
    by_name = {c.name: c for c in rc.cases()}
    for name, k, md, un in (("one", 1, 1, "keep"), ("empty-frames", 2, 1, "drop"), ("dropped", 3, 1, "keep"),
                            ("dropped-first-frame", 1, 0, "drop"), ("65-rows", 3, 1, "keep"), ("scan-blocks", 3, 1, "drop"),
                            ("transcriptions-96", 2, 3, "keep"), ("transcriptions-custom", 2, 1, "keep"),
                            ("first-frame-998", 2, 1, "drop"), ("six-frames", 2, 1, "drop")):
        out.append(LexCase(name, by_name[name], words_of(by_name[name], k, len(out)), md, un))
    out.append(LexCase("only-empty-frames", by_name["only-empty-frames"], lex_of(["a"]), 1, "drop"))
    # ---- no emitted character: the empty query is accepted only if a word of length <= max_dist exists
    c = rc.Case("empty-query", "96", [2, 1], seed=40)
    c.set_text(0, [95] * 25)
    c.set_text(2, [95] * 25)
    out.append(LexCase("empty-query-short-word", c, lex_of(["longword", "b", "c"], {"b": "B!"}), 1, "drop"))
    out.append(LexCase("empty-query-no-short-word", c, lex_of(["longword", "bc"]), 1, "drop"))
    # ---- 25 emitted characters; 21 x U+FB03 (63 code points)
    c = rc.Case("long-rows", "lex", [2, 1], seed=41)
    set_str(c, 0, "xyz" * 8 + "x")
    set_str(c, 1, "ﬃ" * 21)
    set_str(c, 2, "ßΐ" + "x" * 3)
    out.append(LexCase("long-rows", c, lex_of(["xyz" * 8 + "y", "FFI" * 21, "ssΐxxx"], {"FFI" * 21: "ffi"}), 1, "keep"))
    # ---- keep == 0 first, last and as a whole frame; an empty lexicon; one word; ties; max_dist 0, 1, 3
    c = by_name["dropped"]
    out.append(LexCase("empty-lexicon-keep", c, lex_of([]), 1, "keep"))
    out.append(LexCase("empty-lexicon-drop", c, lex_of([]), 3, "drop"))
    c = rc.Case("dist", "96", [3, 2], seed=42)
    for r, t in enumerate(("cat", "cot", "dog", "cart", "c")):
        set_str(c, r, t)
    out.append(LexCase("one-word", c, lex_of(["cat"], {"cat": "Cat"}), 1, "drop"))
    for md in (0, 1, 3):
        # "cot" is at distance 1 of "cat" and of "cut" and "cog": the lowest index wins
        out.append(LexCase("ties-dist-%d" % md, c, lex_of(["cut", "cat", "cog", "dig"], {"cut": "CUT", "cat": "CAT", "cog": "COG"}),
                           md, "drop" if md != 1 else "keep"))
    # ---- display forms: every escape, 2-, 3- and 4-byte code points, the empty one, the limits, two words with one form
    c = rc.Case("display", "96", [4, 5], seed=43)
    forms = ['"\\&<>\'', "a\tb\nc", "é中\U0001f600€", "", "\\" * 87 + "a", "<" * 43 + "abc", "a" * 100, "same", "same"]
    words = ["w" + chr(ord("a") + i) * 3 for i in range(len(forms))]
    for r in range(9):
        set_str(c, r, words[r])
    c.set_id(7, 77)
    c.set_id(8, 77)                                                 # two words, one display form, one track
    out.append(LexCase("display-forms", c, lex_of(words, dict(zip(words, forms))), 0, "keep"))
    # ---- an unaccepted row whose own text equals another row's display form, in one track: they vote together
    c = rc.Case("vote-together", "96", [1, 1, 1], seed=44)
    for r, t in enumerate(("dog", "zzzzzz", "cat")):
        set_str(c, r, t)
        c.set_id(r, 5)
    out.append(LexCase("vote-together", c, lex_of(["cat"], {"cat": "zzzzzz"}), 1, "keep"))
    return out


def bad_id_case():
    c = rc.Case("bad-id", "37", [2, 1], seed=45)
    c.set_text(1, [3, 40, 5] + [36] * 22, emit=0b111)               # id 40 is outside the 36-entry table, and emitted
    return LexCase("bad-id", c, lex_of(["a"]), 1, "keep")


def too_long_case():
    c = rc.Case("too-long", "lex", [1, 2], seed=46)
    set_str(c, 2, "ﬃ" * 22)                                          # 66 code points, in the call's last row
    return LexCase("too-long", c, lex_of(["FFI"]), 1, "keep")


# ---------------------------------------------------------------------------------------------------- the tables
def norm_tab(decoder):
    return lexicon.norm_table(decoder)


def forms(lex):
    """(json forms, xml forms, txt forms) per word: strings, strings, bytes -- from the libraries, as `lexicon.display_tables`."""
    d = [str(lex.display(i)) for i in range(len(lex))]
    return ([json.dumps(t, ensure_ascii=False)[1:-1] for t in d], [results._xml_attribute(t) for t in d],
            [lexicon.txt_form(t).encode("utf-8") for t in d])


# ---------------------------------------------------------------------------------------------------- the references
def statement_bytes(lc):
    """-> (json bytes, xml bytes, txt bytes, (ov, keep_out, totals)) of the call by tests/lexicon_rows_statement.py."""
    if getattr(lc, "_statement", None) is not None:              # (computed once, shared among the tests, left unchanged)
        return lc._statement
    c = lc.case
    _, ov, keep_out, totals = lrs.apply(c.words, c.keep, norm_tab(c.decoder).tolist(), lc.lex.normal, lc.max_dist,
                                        lc.unmatched == "drop")
    jf, xf, tf = forms(lc.lex)
    kept = rc.Case.__new__(rc.Case)
    kept.__dict__.update(c.__dict__)
    kept.keep = np.asarray(keep_out, dtype=np.uint8)
    frame_ov = [[ov[r] for r in range(c.frame_rows[f], c.frame_rows[f + 1]) if keep_out[r]] for f in range(len(c.frame_rows) - 1)]
    js, xs = lrs.corrected_text(kept.frames(), c.first_frame, frame_ov, jf, xf)
    txt = lrs.corrected_vote(c.words, keep_out, ov, results.txt_table(c.decoder), tf)
    lc._statement = js.encode("utf-8"), xs.encode("utf-8"), txt, (ov, keep_out, totals)
    return lc._statement


def host_bytes(lc, tmp_dir):
    """-> (json bytes, xml bytes, txt bytes) of the call as the host path writes them: `correct_annotation(host=True)` on the
    call's annotation, `write_video_results`, `write_track_transcriptions`; header and footer cut off as `rc.writer_text` does."""
    c = lc.case
    frames = c.frames()
    if not frames:
        return b"", b"", b""
    annotation = {str(c.first_frame + f + 1): rows for f, rows in enumerate(frames)}
    fixed = lexicon.correct_annotation(annotation, lc.lex, lc.max_dist, lc.unmatched, host=True)
    d = os.path.join(str(tmp_dir), "host-%s" % abs(hash(lc.name)))
    os.makedirs(os.path.join(d, "preds"), exist_ok=True)
    jp, xp = os.path.join(d, "w.json"), os.path.join(d, "preds", "res_w.xml")
    results.write_video_results(fixed, jp, xp)
    results.write_track_transcriptions(os.path.join(d, "preds"))
    js, xs = open(jp, "rb").read(), open(xp, "rb").read()
    txt = open(os.path.join(d, "preds", "res_w.txt"), "rb").read()
    head, foot = b'<?xml version="1.0" ?>\n<Frames>\n', b"</Frames>\n"
    assert js.startswith(b"{\n") and js.endswith(b"\n}") and xs.startswith(head) and xs.endswith(foot)
    return (b",\n" if c.first_frame else b"") + js[2:-2], xs[len(head):-len(foot)], txt


# ---------------------------------------------------------------------------------------------------- the host check's dump
def dump(path, case_list):
    """The calls as tools/lexicon_rows_hostcheck.cpp reads them: little-endian, a count, then per call n, F, first_frame, ntab,
    W, max_dist, drop and the byte sizes of the three display tables; words, pts, keep, frame_rows, json / xml / txt tables, the
    norm table, ov (the statement's: the match is not the host check's business), then per display table its offsets and bytes."""
    with open(path, "wb") as f:
        f.write(struct.pack("<q", len(case_list)))
        for lc in case_list:
            c = lc.case
            jt, xt = results.text_tables(c.decoder)
            tt = results.txt_table(c.decoder)
            tables = lexicon.display_tables(lc.lex)
            ov = statement_bytes(lc)[3][0]
            f.write(struct.pack("<10q", c.words.shape[0], len(c.frame_rows) - 1, c.first_frame, jt.shape[0], len(lc.lex),
                                lc.max_dist, 1 if lc.unmatched == "drop" else 0, *[t[2] for t in tables]))
            f.write(np.ascontiguousarray(c.words, dtype="<i4").tobytes())
            f.write(np.ascontiguousarray(c.pts, dtype="<i8").tobytes())
            f.write(np.ascontiguousarray(c.keep, dtype=np.uint8).tobytes())
            f.write(np.ascontiguousarray(c.frame_rows, dtype="<i4").tobytes())
            f.write(jt.tobytes() + xt.tobytes() + tt.tobytes())
            f.write(np.ascontiguousarray(norm_tab(c.decoder), dtype="<i4").tobytes())
            f.write(np.asarray(ov, dtype="<i4").tobytes())
            for data, off, nbytes in tables:
                f.write(np.ascontiguousarray(off, dtype="<i4").tobytes())
                f.write(data[:nbytes].tobytes())
