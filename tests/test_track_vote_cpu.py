"""CPU: the plain-Python statement of the track vote (tests/track_vote_statement.py) against the host writer it restates --
`results.write_track_transcriptions` over files `results.write_video_results` wrote -- on every shared case, and against the
reference's own getid_text output (tests/golden/results_writer.json); `results.txt_table` against the XML round trip of whole
strings; `write_track_transcriptions(skip=)`."""
import json
import os

import numpy as np
import pytest

import track_vote_cases as tc
import track_vote_statement as st
from gomatching_amd import results

GOLD = os.path.join(os.path.dirname(__file__), "golden", "results_writer.json")
CASES = tc.cases()


def _host_txt(annotation, tmp_path, stem="v"):
    preds = tmp_path / "preds"
    preds.mkdir(exist_ok=True)
    results.write_video_results(annotation, str(tmp_path / (stem + ".json")), str(preds / ("res_%s.xml" % stem)))
    results.write_track_transcriptions(str(preds))
    return (preds / ("res_%s.txt" % stem)).read_bytes()


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_statement_is_the_host_writers_file(case, tmp_path):
    text, winners = case.statement()
    assert text == _host_txt(case.annotation(), tmp_path), case.name
    assert [w[0] for w in winners] == sorted(set(case.track_id(r) for r in range(len(case.keep)) if case.keep[r]))
    for tid, pos, count in winners:                              # the winner is a kept row of its track, the first with its text
        assert case.keep[pos] and case.track_id(pos) == tid
        same = [r for r in range(len(case.keep)) if case.keep[r] and case.track_id(r) == tid and
                case.text(r) == case.text(pos)]
        assert same[0] == pos and len(same) == count


def test_the_cases_cover_what_they_name():
    by = {c.name: c for c in CASES}
    assert sum(len(c.keep) for c in CASES) <= 4000
    assert by["tie-2-2"].statement()[0] == b'"5","b"\n'
    assert by["tie-3"].statement()[0] == b'"1","x"\n"2","k"\n'
    assert by["3-against-2"].statement() == (b'"3","b"\n', [(3, 1, 3)])
    assert by["dropped-track"].statement()[0] == b'"2","stay"\n'
    assert [w[0] for w in by["id-order"].statement()[1]] == [-2 ** 63, -3, 0, 2, 9, 10, 2 ** 31 + 5, 2 ** 40 + 1, 2 ** 63 - 1]
    assert by["empty-text"].statement()[0] == b'"1",""\n"2","a"\n'
    lines = by["long-entries"].statement()[0].split(b"\n")
    assert len(lines[0]) == 6 + 75 and len(lines[1]) == 6 + 100 and lines[1].endswith("\U0001f600".encode("utf-8") + b'"')
    assert by["last-character"].statement()[0] == b'"1","' + b"a" * 24 + b'c"\n'
    assert by["prefix"].statement()[0] == b'"1","abc"\n"2","abc"\n"3","abcd"\n'
    assert by["same-text-other-recs"].statement() == (b'"1","ab"\n', [(1, 1, 3)])
    assert by["shared-entry"].statement() == (b'"1","a"\n', [(1, 1, 3)])
    tiles = by["tiles"].statement()[1]
    frame_of = lambda c, r: int(np.searchsorted(c.frame_rows, r, side="right")) - 1
    assert [(frame_of(by["tiles"], p), n) for _, p, n in tiles] == [(L - 3, 3) for L in (64, 65, 256, 257, 600)]
    assert len(by["300-tracks"].statement()[1]) == 300 > tc.BLOCK
    assert by["two-rows-one-frame"].statement() == (b'"4","b"\n"9","c"\n', [(4, 1, 2), (9, 3, 2)])
    assert by["no-kept-rows"].statement() == (b"", []) and by["no-rows"].statement() == (b"", [])


def test_statement_is_the_references_getid_text():
    with open(GOLD, encoding="utf-8") as f:
        gold = json.load(f)
    assert gold["videos"]
    for name, ann in gold["videos"].items():
        voters = [(row[8], row[9].encode("utf-8"), k) for k, row in
                  enumerate(row for frame in ann for row in ann[frame])]
        assert st.vote(voters)[0] == gold["txt"][name].encode("utf-8"), name


def test_a_bad_id_is_refused_by_the_statement():
    c = tc.Case("bad", "37").add(0, 1, recs=[36] * 25, emit=1).build()
    with pytest.raises(st.BadId):
        c.statement()
    c = tc.Case("bad-but-dropped", "37").add(0, 1, recs=[-1] * 25, emit=1, keep=0).add(0, 1, recs=[99] * 25, emit=0).build()
    assert c.statement()[0] == b'"1",""\n'


@pytest.mark.parametrize("voc", ["37", "96", "custom"])
def test_txt_table_round_trips_whole_strings(voc, tmp_path):
    """A transcription goes through minidom and the parser as a whole; its bytes are its characters' entries, one after another."""
    decoder = tc.DECODERS[voc]
    tab = results.txt_table(decoder)
    assert tab.shape == (len(decoder.labels), 8) and tab.dtype == np.uint8 and int(tab[:, 0].max()) <= 4
    rng = np.random.RandomState(11)
    strings = [[int(i) for i in rng.randint(0, len(decoder.labels), size=rng.randint(0, 26))] for _ in range(60)]
    strings.append(list(range(len(decoder.labels)))[:25])
    strings.append(list(range(len(decoder.labels)))[-25:])
    ann = {"1": [[0, 0, 9, 0, 9, 9, 0, 9, k, "".join(decoder.labels[i] for i in ids)] for k, ids in enumerate(strings)]}
    got = _host_txt(ann, tmp_path)
    want = b"".join(b'"%d","' % k + b"".join(tab[i, 1:1 + tab[i, 0]].tobytes() for i in ids) + b'"\n' for k, ids in enumerate(strings))
    assert got == want


def test_txt_table_refuses_what_does_not_survive():
    with pytest.raises(ValueError, match="entry 1"):
        results.txt_table(tc.Labels(["a", "\x01"]))               # no XML 1.0 character: the parser refuses it
    with pytest.raises(ValueError, match="entry 0"):
        results.txt_table(tc.Labels(["\ud800"]))                  # a lone surrogate: no UTF-8 encoding


def test_skip_is_honoured_and_the_default_is_unchanged(tmp_path):
    preds = tmp_path / "preds"
    preds.mkdir()
    for stem in ("a", "b", "c"):
        ann = {"1": [[0, 0, 9, 0, 9, 9, 0, 9, 1, stem]]}
        results.write_video_results(ann, str(tmp_path / (stem + ".json")), str(preds / ("res_%s.xml" % stem)))
    (preds / "res_b.txt").write_bytes(b"kept as it is")
    (preds / "res_c.xml").write_text("not XML at all")          # a skipped file is not even parsed
    results.write_track_transcriptions(str(preds), skip=("res_b.xml", "res_c.xml", "res_missing.xml"))
    assert (preds / "res_a.txt").read_bytes() == b'"1","a"\n'
    assert (preds / "res_b.txt").read_bytes() == b"kept as it is" and not (preds / "res_c.txt").exists()
    (preds / "res_c.xml").unlink()
    results.write_track_transcriptions(str(preds))               # the default: every XML, as ever
    assert (preds / "res_b.txt").read_bytes() == b'"1","b"\n' and sorted(os.listdir(str(preds))) == [
        "res_a.txt", "res_a.xml", "res_b.txt", "res_b.xml"]
