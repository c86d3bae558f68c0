"""GPU: the lexicon correction of rows (csrc/lexicon_rows.hip and the `_ov` entries of csrc/result_text.hip and
csrc/track_vote.hip) against the plain-Python statement (tests/lexicon_rows_statement.py) and against the bytes of the host path
(`lexicon.correct_annotation(host=True)` -> `results.write_video_results` -> `write_track_transcriptions`), on the case list of
tests/lexicon_rows_cases.py: one row, 65 rows, one row more than two scan blocks with kept flags cleared at the tile edges, a
row without characters, 25 characters, 63 and 66 code points, an id outside the table, dropped rows in every position, an
empty and a one-word lexicon, ties, max_dist 0 / 1 / 3, keep and drop, display forms with every escape and UTF-8 length, the
empty one and the two limits, two words with one form, an unaccepted row that votes with an accepted one, a split call; and
with no override the `_ov` entries give the bytes of the entries without it."""
import numpy as np
import pytest
import torch

import lexicon_rows_cases as lc
import lexicon_rows_statement as lrs
import result_text_cases as rc

from gomatching_amd import lexicon, lib, ops, results

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASES = lc.cases()


def _up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _device_lexicon(case):
    return lexicon.DeviceLexicon(case.lex, case.case.decoder, torch.device(DEV))


def _run(case, part=None):
    """The device path of `results.corrected_text` on a case -> (json, xml, txt bytes, queries, ov, keep_out, totals)."""
    c = case.case
    dl = _device_lexicon(case)
    words, pts, keep = _up(c.words), _up(c.pts), _up(c.keep)
    n = len(c.keep)
    q_chars, q_off, q_len, q_status = ops.lexicon_rows_queries(words, keep, dl.norm_tab)
    index, dist = ops.lexicon_match(q_chars, q_off, torch.zeros((n,), dtype=torch.int32, device=DEV), dl.w_chars, dl.w_off,
                                    dl.seg_off, max_len=64)
    ov, keep_out, totals = ops.lexicon_rows_apply(keep, q_len, q_status, index, dist, dl.W, case.max_dist, case.unmatched == "drop")
    js, xs, _, _ = ops.result_text(words, pts, keep, c.frame_rows, c.first_frame,
                                   tuple(_up(t) for t in results.text_tables(c.decoder)),
                                   ov=(ov, keep_out, dl.json_disp, dl.xml_disp))
    rec = ops.track_vote_records(words, keep, _up(results.txt_table(c.decoder)), ov=(ov, keep_out, dl.txt_disp))
    txt = ops.track_vote(rec)[0].cpu().numpy().tobytes() if n else b""
    off = q_off.cpu().numpy()
    chars = q_chars.cpu().numpy()
    queries = [chars[off[r]:off[r + 1]].tolist() for r in range(n)]
    return (js.cpu().numpy().tobytes(), xs.cpu().numpy().tobytes(), txt, queries, ov.cpu().numpy().tolist(),
            keep_out.cpu().numpy().tolist(), totals.cpu().numpy().tolist(), index.cpu().numpy().tolist(), dist.cpu().numpy().tolist())


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_corrected_bytes_are_the_statements_and_the_hosts(case, tmp_path):
    c = case.case
    if len(c.keep) == 0:                                       # frames without rows: no launch, the host text of empty frames
        want = lc.statement_bytes(case)
        assert results.host_text_of_empty_frames(c.first_frame, len(c.frame_rows) - 1) == want[:2] == lc.host_bytes(case, tmp_path)[:2]
        return
    js, xs, txt, queries, ov, keep_out, totals, index, dist = _run(case)
    want_js, want_xs, want_txt, (want_ov, want_keep, want_totals) = lc.statement_bytes(case)
    tab = lc.norm_tab(c.decoder).tolist()
    assert queries == [lrs.query(c.words[r], c.keep[r], tab) for r in range(len(c.keep))]
    assert ov == want_ov and keep_out == want_keep
    assert totals == list(want_totals) + [0, -1]
    assert js == want_js and xs == want_xs and txt == want_txt
    assert (js, xs, txt) == lc.host_bytes(case, tmp_path)
    assert _run(case)[:3] == (js, xs, txt)                     # bitwise reproducible


def test_what_the_cases_are_there_for():
    """The figures the rule names, read off the device results of the cases made for them."""
    by = {c.name: c for c in CASES}
    r = _run(by["empty-lexicon-drop"])
    assert set(r[7]) == {-1} and set(r[8]) == {100} and r[6][1] == 0 and not any(r[5])
    frames = len(by["empty-lexicon-drop"].case.frame_rows) - 1
    assert r[0].count(b": []") == frames and r[1].count(b"/>\n") == frames and r[2] == b""
    r = _run(by["empty-query-short-word"])
    assert r[3][0] == [] and r[4][0] == 1 and r[4][2] == 1     # the empty query takes the FIRST word of length 1
    r = _run(by["empty-query-no-short-word"])
    assert r[4][0] == -1 and r[5][0] == 0
    r = _run(by["long-rows"])
    assert [len(q) for q in r[3]] == [25, 63, 8] and r[4] == [0, 1, 2]
    for md, want in ((0, [1, -1, -1, -1, -1]), (1, [1, 0, 2, 1, -1]), (3, [1, 0, 2, 1, 0])):
        r = _run(by["ties-dist-%d" % md])
        assert r[4] == want, md                               # "cot": cut, cat and cog at distance 1; "dog": cog and dig -- the lowest index wins
    r = _run(by["display-forms"])
    assert r[4] == list(range(9)) and b'"transcription": "",' in r[0] and b'Transcription="">' in r[1]
    assert b'"77","same"\n' in r[2] and b'","' + b"a" * 100 + b'"\n' in r[2]
    r = _run(by["vote-together"])
    assert r[4] == [-1, -1, 0] and r[2] == b'"5","zzzzzz"\n'   # the unaccepted "zzzzzz" and the accepted "cat" -> "zzzzzz" agree


def test_a_query_above_the_limit_sets_the_status_and_the_row():
    case = lc.too_long_case()
    c = case.case
    dl = _device_lexicon(case)
    words, keep = _up(c.words), _up(c.keep)
    q_chars, q_off, q_len, q_status = ops.lexicon_rows_queries(words, keep, dl.norm_tab)
    assert q_status.tolist() == [lib.CONSTANTS["GOM_LR_TOO_LONG"], 2] and q_len.tolist()[2] == lib.CONSTANTS["GOM_LR_LEN_LONG"]
    off = q_off.tolist()
    assert off[3] == off[2] and off[3] <= q_chars.shape[0]     # the row owns nothing: nothing was written for it
    fix = lexicon.RowCorrection(dl, 1, "keep", None, video="Video_7")
    pts = _up(c.pts)
    with pytest.raises(lexicon.LexiconError) as e:
        results.corrected_text(words, pts, keep, c.frame_rows, 40, c.decoder, fix)
    assert "Video_7" in str(e.value) and "frame 42" in str(e.value)


def test_an_id_outside_the_table_is_never_an_index():
    case = lc.bad_id_case()
    c = case.case
    dl = _device_lexicon(case)
    words, keep = _up(c.words), _up(c.keep)
    q_chars, q_off, q_len, q_status = ops.lexicon_rows_queries(words, keep, dl.norm_tab)
    assert q_len.tolist()[1] == 0 and q_status.tolist() == [0, -1]
    n = len(c.keep)
    index, dist = ops.lexicon_match(q_chars, q_off, torch.zeros((n,), dtype=torch.int32, device=DEV), dl.w_chars, dl.w_off,
                                    dl.seg_off, max_len=64)
    ov, keep_out, _ = ops.lexicon_rows_apply(keep, q_len, q_status, index, dist, dl.W, 1, False)
    with pytest.raises(lib.GomError):
        ops.result_text(words, _up(c.pts), keep, c.frame_rows, 0, tuple(_up(t) for t in results.text_tables(c.decoder)),
                        ov=(ov, keep_out, dl.json_disp, dl.xml_disp))
    rec = ops.track_vote_records(words, keep, _up(results.txt_table(c.decoder)), ov=(ov, keep_out, dl.txt_disp))
    assert rec[1, lib.CONSTANTS["GOM_TV_LEN"]].item() == lib.CONSTANTS["GOM_TV_LEN_BAD"]


@pytest.mark.parametrize("name", ["dropped", "scan-blocks", "transcriptions-custom", "first-frame-998"])
def test_without_an_override_the_ov_entries_give_the_plain_bytes(name):
    case = {c.name: c for c in CASES}[name]
    c = case.case
    dl = _device_lexicon(case)
    words, pts, keep = _up(c.words), _up(c.pts), _up(c.keep)
    tables = tuple(_up(t) for t in results.text_tables(c.decoder))
    ov = torch.full((len(c.keep),), -1, dtype=torch.int32, device=DEV)
    plain = ops.result_text(words, pts, keep, c.frame_rows, c.first_frame, tables)
    with_ov = ops.result_text(words, pts, keep, c.frame_rows, c.first_frame, tables, ov=(ov, keep.clone(), dl.json_disp, dl.xml_disp))
    for a, b in zip(plain, with_ov):
        assert torch.equal(a, b)
    tt = _up(results.txt_table(c.decoder))
    assert torch.equal(ops.track_vote_records(words, keep, tt), ops.track_vote_records(words, keep, tt, ov=(ov, keep.clone(), dl.txt_disp)))


def test_two_calls_are_one_call_cut_in_two():
    case = {c.name: c for c in CASES}["first-frame-998"]
    whole = _run(case)
    F = len(case.case.frame_rows) - 1
    a, b = _run(case.part(0, 1)), _run(case.part(1, F))
    assert a[0] + b[0] == whole[0] and a[1] + b[1] == whole[1]
    six = {c.name: c for c in CASES}["six-frames"]
    six = lc.LexCase("six-frames@998", rc.Case.part(six.case, 0, 6), six.lex, six.max_dist, six.unmatched)
    six.case.first_frame = 998
    whole = _run(six)
    a, b = _run(six.part(0, 3)), _run(six.part(3, 6))
    assert a[0] + b[0] == whole[0] and a[1] + b[1] == whole[1] and whole[:3] == lc.statement_bytes(six)[:3]
    assert b[0].startswith(b',\n    "1002": ')


def test_rows_text_returns_both_pairs(tmp_path):
    """`results.rows_text(lexicon=)`: the original pair as without it, the corrected pair beside it, the figures added up, the
    corrected vote in the correction's own TrackVote."""
    case = {c.name: c for c in CASES}["ties-dist-1"]
    c = case.case
    words = _up(c.words)
    fix = lexicon.RowCorrection(lexicon.DeviceLexicon.of(case.lex, c.decoder, torch.device(DEV)), case.max_dist, case.unmatched,
                                results.TrackVote(c.decoder))
    with np.errstate(invalid="ignore"):                        # (hand-made words: no hull, so no rectangle worth the name)
        plain = results.rows_text(words, c.frame_rows, c.first_frame, c.decoder, min_extent=-10 ** 9)
        both = results.rows_text(words, c.frame_rows, c.first_frame, c.decoder, min_extent=-10 ** 9, lexicon=fix)
    assert len(both) == 4 and both[:2] == plain and both[2:] != plain
    assert (fix.rows, fix.accepted, fix.dropped) == (5, 4, 0) and fix.vote.rows == 5
    assert lexicon.DeviceLexicon.of(case.lex, c.decoder, torch.device(DEV)) is fix.lexicon       # cached per (lexicon, device)
    same, other = rc.Labels(list(c.decoder.labels)), rc.Labels(list(c.decoder.labels)[::-1])      # keyed by the vocabulary, not the object
    assert lexicon.DeviceLexicon.of(case.lex, same, torch.device(DEV)) is fix.lexicon
    assert lexicon.DeviceLexicon.of(case.lex, other, torch.device(DEV)) is not fix.lexicon
