"""CPU: the rule of the lexicon correction of rows (include/gomatching_hip.h, `gom_lexicon_rows_*`).  `str.upper` works
character by character on every shipped vocabulary, so a row's query is its characters' norm-table entries; the statement's
query is `lexicon.norm` of the row's text; the statement's corrected bytes are those of the host path
(`lexicon.correct_annotation(host=True)` -> `results.write_video_results` -> `write_track_transcriptions`); and the three
limits are refused on the host: a 176-byte JSON or XML display form, a 101-byte txt form, a 65-code-point query."""
import os
import re

import numpy as np
import pytest

import lexicon_rows_cases as lc
import lexicon_rows_statement as lrs
import result_text_cases as rc
from gomatching_amd import lexicon
from gomatching_amd.predictor import CTLABELS_37, CTLABELS_96

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VOCABULARIES = {"37": CTLABELS_37, "96": CTLABELS_96, "custom+": rc.CUSTOM + lc.UPPER}


@pytest.fixture(scope="module")
def case_list():
    return lc.cases()


def test_constants_are_the_headers():
    text = open(os.path.join(ROOT, "include", "gomatching_hip.h")).read()
    value = lambda name: int(re.search(r"#define %s (-?\d+)" % name, text).group(1))
    assert value("GOM_LR_NORM_WORDS") == lrs.NORM_WORDS == lexicon.NORM_WORDS
    assert value("GOM_LEXICON_MAX_LEN") == lrs.MAX_LEN == lexicon.MAX_LEN
    assert lexicon.DISPLAY_TEXT_MAX == 25 * (value("GOM_RT_ENTRY_BYTES") - 1) == 175
    assert lexicon.DISPLAY_TXT_MAX == 4 * value("GOM_TV_TEXT_WORDS") == 100
    assert (value("GOM_RR_RECS"), value("GOM_RR_EMIT")) == (lrs.RECS, lrs.EMIT)


@pytest.mark.parametrize("voc", sorted(VOCABULARIES))
def test_upper_works_character_by_character(voc):
    labels = VOCABULARIES[voc]
    tab = lexicon.norm_table(rc.Labels(labels))
    assert tab.shape == (len(labels), 4) and tab.dtype == np.int32
    for i, ch in enumerate(labels):
        assert tab[i].tolist() == lrs.norm_entry(ch) and 0 <= tab[i, 0] <= 3
        for other in labels:                                      # no context: a pair upper-cases to its halves
            assert (ch + other).upper() == ch.upper() + other.upper()
    rng = np.random.RandomState(len(labels))
    for _ in range(50):
        s = "".join(labels[k] for k in rng.randint(0, len(labels), size=25))
        assert s.upper() == "".join(c.upper() for c in s)
    if voc == "custom+":
        assert [int(tab[labels.index(c), 0]) for c in lc.UPPER] == [2, 3, 3]
    with pytest.raises(ValueError):
        lexicon.norm_table(rc.Labels(["ab"]))


def test_query_is_norm_of_the_text(case_list):
    seen = 0
    for c in case_list + [lc.bad_id_case()]:
        tab = lc.norm_tab(c.case.decoder).tolist()
        for r in range(len(c.case.keep)):
            q = lrs.query(c.case.words[r], c.case.keep[r], tab)
            if c.name == "bad-id" and r == 1:
                assert q == []
                continue
            assert q == ([ord(ch) for ch in lexicon.norm(c.case.text(r))] if c.case.keep[r] else []), (c.name, r)
            seen += 1
    assert seen > 2 * rc.SCAN_BLOCK + 1                           # (the scan-blocks call alone has that many rows)


def test_statement_writes_the_host_paths_bytes(case_list, tmp_path):
    changed = unaccepted = dropped = 0
    for c in case_list:
        js, xs, txt, (ov, keep_out, totals) = lc.statement_bytes(c)
        hj, hx, ht = lc.host_bytes(c, tmp_path)
        assert js == hj, c.name
        assert xs == hx, c.name
        assert txt == ht, c.name
        assert totals[0] == int(c.case.keep.sum()) and totals[1] == sum(o >= 0 for o in ov)
        assert totals[2] == int(c.case.keep.sum()) - sum(keep_out)
        changed += totals[1]
        unaccepted += totals[0] - totals[1]
        dropped += totals[2]
    assert changed >= 10 and unaccepted >= 10 and dropped >= 10    # (the comparison does not pass emptily)


def test_split_call_is_the_whole_call(case_list):
    whole = [c for c in case_list if c.name == "six-frames"][0]
    a, b = lc.statement_bytes(whole.part(0, 3)), lc.statement_bytes(whole.part(3, 6))
    w = lc.statement_bytes(whole)
    assert a[0] + b[0] == w[0] and a[1] + b[1] == w[1]


def test_the_three_limits_are_refused():
    ok = lc.lex_of(["aa", "bb", "cc"], {"aa": "\\" * 87 + "a", "bb": "<" * 43 + "abc", "cc": "a" * 100})
    tables = lexicon.display_tables(ok)
    assert [int(t[1][1] - t[1][0]) for t in tables] == [175, 88, 88] and int(tables[1][1][2] - tables[1][1][1]) == 175
    assert int(tables[2][1][3] - tables[2][1][2]) == 100
    for form, stream in (("\\" * 88, "JSON"), ("<" * 44, "XML"), ("a" * 101, "txt")):
        with pytest.raises(lexicon.LexiconError) as e:
            lexicon.display_tables(lc.lex_of(["ok", "word"], {"word": form}))
        assert "<case>" in str(e.value) and "'word'" in str(e.value) and stream in str(e.value)
    long = lc.too_long_case()
    with pytest.raises(lrs.TooLong) as e:
        lc.statement_bytes(long)
    assert e.value.row == 2
    with pytest.raises(lexicon.LexiconError):
        lc.host_bytes(long, "/nonexistent")
    passes = [c for c in lc.cases() if c.name == "long-rows"][0]      # 63 code points pass
    assert len(lrs.query(passes.case.words[1], 1, lc.norm_tab(passes.case.decoder).tolist())) == 63


def test_correct_results_skips_what_the_device_path_wrote(tmp_path):
    """`correct_results(skip=)`: a skipped video's files are neither read nor written, the others are corrected as ever."""
    from gomatching_amd import results
    res = tmp_path / "res"
    for d in ("jsons", "preds"):
        (res / d).mkdir(parents=True)
    row = [0, 0, 9, 0, 9, 9, 0, 9, 1, "cot"]
    for v in ("va", "vb"):
        results.write_video_results({"1": [row]}, str(res / "jsons" / (v + ".json")), str(res / "preds" / ("res_%s.xml" % v)))
    lex = tmp_path / "lex.txt"
    lex.write_text("cat\n")
    out = res / "lexicon"
    (out / "preds").mkdir(parents=True)
    (out / "preds" / "res_va.xml").write_text("not xml: the host must not parse this")
    figures = lexicon.correct_results(str(res), None, str(lex), host=True, skip=["va"])
    assert figures["videos"] == 1 and figures["rows"] == 1 and figures["changed"] == 1
    assert sorted(os.listdir(str(out / "preds"))) == ["res_va.xml", "res_vb.txt", "res_vb.xml"]
    assert os.listdir(str(out / "jsons")) == ["vb.json"] and (out / "preds" / "res_vb.txt").read_text() == '"1","cat"\n'


def test_entries_refuse_bad_arguments_without_a_gpu():
    """GOM_ERR_INVALID_ARG before any HIP call; n == 0 is GOM_OK without a launch (no compute, no device)."""
    import ctypes as C
    from gomatching_amd import lib
    L = lib.load()
    p, ld = C.c_void_p(0x1000), lib.CONSTANTS["GOM_RESULT_ROWS_WORDS"]

    def queries(n=2, ld=ld, ntab=36, q_cap=128, words=p, keep=p, tab=p, q_len=p, q_off=p, st=p, chars=p):
        return L.gom_lexicon_rows_queries_u32(words, ld, keep, n, tab, ntab, q_len, q_off, st, chars, q_cap, None)

    def apply(n=2, W=3, max_dist=1, drop=0, keep=p, q_len=p, st=p, index=p, dist=p, ov=p, keep_out=p, totals=p):
        return L.gom_lexicon_rows_apply_i32(keep, q_len, st, index, dist, n, W, max_dist, drop, ov, keep_out, totals, None)

    def count(ov=p, keep_out=p, jd=p, jo=p, jn=4, xd=p, xo=p, xn=4, W=2, n=1):
        return L.gom_result_text_count_scan_ov(p, ld, p, p, n, p, 1, 0, p, p, 36, ov, keep_out, jd, jo, jn, xd, xo, xn, W, p, p, p, p, p, None)

    def emit(ov=p, keep_out=p, jd=p, jo=p, jn=4, xd=p, xo=p, xn=4, W=2, cap=8):
        return L.gom_result_text_emit_ov(p, ld, p, p, 1, p, 1, 0, p, p, 36, ov, keep_out, jd, jo, jn, xd, xo, xn, W, p, p, p, p, p, cap, p, cap,
                                         None)

    def records(ov=p, keep_out=p, disp=p, off=p, nbytes=4, W=2, n=1):
        return L.gom_track_vote_records_ov_i32(p, ld, p, n, p, 36, ov, keep_out, disp, off, nbytes, W, p, None)

    assert queries(n=0) == 0 and apply(n=0) == 0
    for rc in (queries(n=-1), queries(n=2 ** 25, q_cap=2 ** 31), queries(ld=ld - 1), queries(ntab=0), queries(q_cap=127), queries(words=None),
               queries(keep=None), queries(tab=None), queries(q_len=None), queries(q_off=None), queries(st=None), queries(chars=None),
               apply(n=-1), apply(W=-1), apply(max_dist=-1), apply(drop=2), apply(keep=None), apply(q_len=None), apply(st=None),
               apply(index=None), apply(dist=None), apply(ov=None), apply(keep_out=None), apply(totals=None),
               count(ov=None), count(keep_out=None), count(jd=None), count(jo=None), count(jn=-1), count(xd=None), count(xo=None),
               count(xn=-1), count(W=-1), count(n=0),
               emit(ov=None), emit(keep_out=None), emit(jd=None), emit(xo=None), emit(W=-1), emit(cap=-1),
               records(ov=None), records(keep_out=None), records(disp=None), records(off=None), records(nbytes=-1), records(W=-1),
               records(n=0)):
        assert rc == 1                                        # GOM_ERR_INVALID_ARG


def test_the_shortcut_for_plain_forms_gives_the_whole_form_tables():
    """`display_tables` takes a form of characters that all three libraries leave alone as its own bytes; the tables are those of
    every form sent through the libraries whole."""
    rng = np.random.RandomState(5)
    alphabet = list("abcXYZ019 _-.,;:!?()[]{}/@#$%^*+=~`|") + ['"', "\\", "&", "<", ">", "'", "\t", "\x7f", "é", "ß", "中", "\U0001f600", "€"]
    forms = ["".join(alphabet[k] for k in rng.randint(0, len(alphabet), size=rng.randint(0, 20))) for _ in range(300)]
    forms += ["plain", "", "a b", " lead", "trail ", "a\tb", "a  b", "x" * 100]
    words = ["w%d" % i for i in range(len(forms))]
    lex = lc.lex_of(words, dict(zip(words, forms)))
    fast, whole = lexicon.display_tables(lex), lexicon.display_tables(lex, shortcut=False)
    assert any(f and all(ch in "abcXYZ019 _-.,;:!?()[]{}/@#$%^*+=~`|" for ch in f) for f in forms)      # some forms took the shortcut
    for (a, ao, an), (b, bo, bn) in zip(fast, whole):
        assert an == bn and ao.tolist() == bo.tolist() and a.tobytes() == b.tobytes()
    assert lexicon.checked_display_tables(lex) is lexicon.checked_display_tables(lex)                  # built once per Lexicon


def test_the_command_checks_the_limits_before_it_builds_anything(tmp_path):
    """`eval.device_lexicons`, what `--device-lexicon` runs before a model is built or a directory created: a 176-byte display
    form is a LexiconError naming the pair list's lexicon and the word, for one lexicon file and for per-video lexicons."""
    from gomatching_amd import eval as E
    data = tmp_path / "frames"
    for v in ("va", "vb"):
        (data / v).mkdir(parents=True)
        (data / v / "1.png").write_bytes(b"")
    lex, pairs = tmp_path / "lexicon.txt", tmp_path / "pairs.txt"
    lex.write_text("fine\nwide\n")
    pairs.write_text("FINE Fine\nWIDE %s\n" % ("<" * 44))               # 176 bytes as an XML attribute value
    with pytest.raises(lexicon.LexiconError) as e:
        E.device_lexicons(str(lex), str(pairs), str(data))
    assert str(lex) in str(e.value) and "'wide'" in str(e.value) and "176 bytes in the XML file" in str(e.value)
    pairs.write_text("FINE Fine\nWIDE %s\n" % ("<" * 43 + "abc"))        # 175: taken
    got = E.device_lexicons(str(lex), str(pairs), str(data))
    assert isinstance(got, lexicon.Lexicon) and "_display_tables" in got.__dict__
    per_video = tmp_path / "lexicons"
    per_video.mkdir()
    (per_video / "va.txt").write_text("fine\n")
    (per_video / "vb.txt").write_text("long\n")
    (per_video / "vb.pairs.txt").write_text("LONG %s\n" % ("a" * 101))
    with pytest.raises(lexicon.LexiconError) as e:
        E.device_lexicons(str(per_video), None, str(data))
    assert "vb.txt" in str(e.value) and "101 bytes in the txt file" in str(e.value)
    assert sorted(E.device_lexicons(str(per_video), None, str(data), done=["vb"])) == ["va"]     # a finished video needs none
    (per_video / "va.txt").unlink()
    with pytest.raises(lexicon.LexiconError):
        E.device_lexicons(str(per_video), None, str(data), done=["vb"])


def test_main_turns_a_lexicon_error_into_status_2(monkeypatch, capsys):
    """Whatever part of the run raises `LexiconError` (the device path does inside the video loop), the command ends with
    status 2 and the message."""
    from gomatching_amd import eval as E

    def run(argv):
        raise lexicon.LexiconError("video V, frame 3: a transcription of more than 64 code points")
    monkeypatch.setattr(E, "run", run)
    assert E.main([]) == 2
    assert capsys.readouterr().err == "error: lexicon: video V, frame 3: a transcription of more than 64 code points\n"
