"""GPU: `ops.result_text` (csrc/result_text.hip) against the bytes `results.write_video_results` writes, on the smallest cases
that can break the count / scan / emit trio (tests/result_text_cases.py: empty frames and dropped rows in every position, 65
rows in a frame, one row more than two scan blocks, the edges of int32 and int64, every escape and UTF-8 length, first frames
that change the key's digit count), words that come out of `ops.result_rows` itself, a video split into two calls, an id
outside the table, a cap below the totals, and two runs of one call."""
import numpy as np
import pytest
import torch

import result_text_cases as rc
import result_text_statement as st

from gomatching_amd import lib, ops, results
from gomatching_amd.predictor import TextDecoder

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _tables(decoder):
    return tuple(torch.from_numpy(t).to(DEV) for t in results.text_tables(decoder))


def _run(case):
    out = ops.result_text(torch.from_numpy(case.words).to(DEV), torch.from_numpy(case.pts).to(DEV),
                          torch.from_numpy(case.keep).to(DEV), case.frame_rows, case.first_frame, _tables(case.decoder))
    js, xs, joff, xoff = (t.cpu().numpy() for t in out)
    assert js.dtype == xs.dtype == np.uint8 and joff.dtype == xoff.dtype == np.int64
    return js.tobytes(), xs.tobytes(), joff.tolist(), xoff.tolist()


@pytest.mark.parametrize("case", rc.cases(), ids=lambda c: c.name)
def test_text_is_the_writers(case, tmp_path):
    want_js, want_xs = rc.writer_text(case, tmp_path)
    js, xs, joff, xoff = _run(case)
    assert len(js) == len(want_js) and len(xs) == len(want_xs)
    assert js == want_js and xs == want_xs
    frames = case.frames()                                     # the frame offsets cut the streams where the statement does
    assert len(joff) == len(xoff) == len(frames) + 1 and joff[0] == xoff[0] == 0
    for f, rows in enumerate(frames):
        assert js[joff[f]:joff[f + 1]] == st.frame_json(case.first_frame + f, rows).encode("utf-8"), f
        assert xs[xoff[f]:xoff[f + 1]] == st.frame_xml(case.first_frame + f, rows).encode("utf-8"), f
    assert _run(case)[:2] == (js, xs)                          # bitwise reproducible


def test_no_rows_and_no_frames_need_no_launch():
    tabs = _tables(rc.DECODERS["37"])
    empty = (torch.zeros((0, 234), dtype=torch.int32, device=DEV), torch.zeros((0, 8), dtype=torch.int64, device=DEV),
             torch.zeros((0,), dtype=torch.uint8, device=DEV))
    js, xs, joff, xoff = ops.result_text(*empty, np.zeros((1,), np.int32), 0, tabs)                 # F == 0
    assert js.numel() == xs.numel() == 0 and js.dtype == torch.uint8 and joff.tolist() == xoff.tolist() == [0]
    js, xs, joff, xoff = ops.result_text(*empty, np.zeros((4,), np.int32), 8, tabs)                 # n == 0, three frames
    want_js = "".join(st.frame_json(f, []) for f in (8, 9, 10)).encode()
    want_xs = "".join(st.frame_xml(f, []) for f in (8, 9, 10)).encode()
    assert js.cpu().numpy().tobytes() == want_js and xs.cpu().numpy().tobytes() == want_xs
    assert joff.tolist()[-1] == len(want_js) and xoff.tolist()[-1] == len(want_xs) and len(joff) == 4


def test_bad_frame_rows_are_refused_on_the_host():
    case = rc.cases()[0]
    args = (torch.from_numpy(case.words).to(DEV), torch.from_numpy(case.pts).to(DEV), torch.from_numpy(case.keep).to(DEV))
    for bad in ([0, 2], [1, 1], [0, 1, 0, 1], [0]):
        with pytest.raises(ValueError):
            ops.result_text(*args, np.array(bad, np.int32), 0, _tables(case.decoder))


def test_two_calls_are_one_call_cut_in_two():
    case = {c.name: c for c in rc.cases()}["six-frames"]
    whole = _run(case)
    a, b = _run(case.part(0, 3)), _run(case.part(3, 6))
    assert a[0] + b[0] == whole[0] and a[1] + b[1] == whole[1]
    assert b[0].startswith(b',\n    "4": ')                 # the ",\n" depends on the absolute frame index alone


def test_words_of_result_rows(tmp_path):
    """The words as the rows kernel leaves them: integer polygons from crafted boundaries (every value fp32 holds exactly), its own
    CTC mask over blank-separated repeats, and the edges of the id."""
    decoder = TextDecoder(96)
    n = 6
    rng = np.random.RandomState(3)
    bd = rng.uniform(-30, 1500, size=(n, 25, 4)).astype(np.float32)
    bd[0].reshape(-1)[:8] = [0, -1, 9, 10, -10, 99999, -0.5, 0.99]
    bd[1] = np.float32(16777216.0)                                                                   # one distinct point
    recs = rng.randint(0, 99, size=(n, 25)).astype(np.int64)
    a, q = decoder.labels.index("a"), decoder.labels.index('"')
    recs[2] = [a, a, 95, a, a, 96, q, q, 95, q] + [95] * 15                                          # -> aa""
    recs[3] = 95                                                                                     # -> empty
    recs[4] = [q, a] * 12 + [q]                                                                      # 25 emitted, 13 escapes
    ids = np.array([0, 2 ** 63 - 1, -2 ** 63, 7, -1, 12345678901234], dtype=np.int64)
    words_d = ops.result_rows(torch.from_numpy(bd).to(DEV), torch.from_numpy(recs).to(DEV), decoder.voc_size, torch.from_numpy(ids).to(DEV))
    case = rc.Case("rows", "96", [2, 0, 4], first_frame=98, seed=1)
    case.words = words_d.cpu().numpy()
    case.pts, keep = results.finish_points(case.words, 5)
    case.keep = keep.astype(np.uint8)
    assert [case.text(r) for r in range(n)] == [decoder.decode(recs[r]) for r in range(n)]
    assert case.text(2) == 'aa""' and case.text(3) == "" and len(case.text(4)) == 25
    assert [case.track_id(r) for r in range(n)] == ids.tolist()
    out = ops.result_text(words_d, torch.from_numpy(case.pts).to(DEV), torch.from_numpy(case.keep).to(DEV), case.frame_rows, 98,
                          _tables(decoder))
    want = rc.writer_text(case, tmp_path)
    assert (out[0].cpu().numpy().tobytes(), out[1].cpu().numpy().tobytes()) == want
    # the host rows of the same words are the rows that text was written from
    rows = results.finish_rows(case.words, decoder, 5)
    assert [r for fr in case.frames() for r in fr] == [r for r in rows if r is not None] and not keep[1] and keep.sum() == n - 1


def _launch(case, json_cap_cut, pad=64):
    """The two entry points by hand, with text buffers `pad` bytes longer than the totals, filled with 0xAA, and caps
    `json_cap_cut` bytes below them."""
    dev = torch.device(DEV)
    words, pts, keep = (torch.from_numpy(x).to(dev) for x in (case.words, case.pts, case.keep))
    jt, xt = _tables(case.decoder)
    n, F = case.words.shape[0], len(case.frame_rows) - 1
    fr = torch.from_numpy(case.frame_rows).to(dev)
    row_len = torch.empty((2, n), dtype=torch.int32, device=dev)
    row_off = torch.empty((2, n + 1), dtype=torch.int64, device=dev)
    row_kept = torch.empty((n + 1,), dtype=torch.int32, device=dev)
    frame_off = torch.empty((2, F + 1), dtype=torch.int64, device=dev)
    totals = torch.empty((4,), dtype=torch.int64, device=dev)
    p = ops._p
    common = (p(words), 234, p(pts), p(keep), n, p(fr), F, case.first_frame, p(jt), p(xt), jt.shape[0])
    ops._call("gom_result_text_count_scan", *common, p(row_len), p(row_off), p(row_kept), p(frame_off), p(totals), ops._stream())
    tj, tx, status, _ = totals.tolist()
    js = torch.full((tj + pad,), 0xAA, dtype=torch.uint8, device=dev)
    xs = torch.full((tx + pad,), 0xAA, dtype=torch.uint8, device=dev)
    ops._call("gom_result_text_emit", *common, p(row_len), p(row_off), p(row_kept), p(frame_off), p(js), tj - json_cap_cut, p(xs),
              tx - json_cap_cut, ops._stream())
    return js.cpu().numpy(), xs.cpu().numpy(), tj, tx, status, row_len.cpu().numpy()


def test_nothing_is_stored_at_or_past_the_cap(tmp_path):
    case = {c.name: c for c in rc.cases()}["dropped"]
    want_js, want_xs = rc.writer_text(case, tmp_path)
    js, xs, tj, tx, status, _ = _launch(case, 0)
    assert (tj, tx, status) == (len(want_js), len(want_xs), 0)
    assert js[:tj].tobytes() == want_js and xs[:tx].tobytes() == want_xs
    assert (js[tj:] == 0xAA).all() and (xs[tx:] == 0xAA).all()                 # not one byte behind the totals
    js, xs, tj, tx, status, _ = _launch(case, 5)                               # caps five bytes short: what does not fit is left out
    assert (js[tj - 5:] == 0xAA).all() and (xs[tx - 5:] == 0xAA).all()
    first_frame_end = len(st.frame_json(0, case.frames()[0]))
    assert js[:first_frame_end].tobytes() == want_js[:first_frame_end]         # and what fits is still right


def test_an_id_outside_the_table_sets_the_status_and_raises():
    case = rc.Case("bad-id", "37", [2, 2], seed=21)
    for r, bad in ((1, 36), (2, -1)):                                          # one past the table; a negative id
        c = rc.Case("bad-id", "37", [2, 2], seed=21)
        c.words[r, 200 + 3] = bad
        c.words[r, 225] |= 1 << 3                                              # its emit bit set, written into the words directly
        with pytest.raises(lib.GomError, match="outside"):
            _run(c)
        js, xs, tj, tx, status, row_len = _launch(c, 0)
        assert status == lib.CONSTANTS["GOM_RT_BAD_ID"] and row_len[0, r] == -1 and row_len[1, r] == -1
        c.keep[r] = 0                                                          # the streams leave the row out, as if it were dropped
        want_js, want_xs = rc.statement_text(c)
        assert js[:tj].tobytes() == want_js and xs[:tx].tobytes() == want_xs
    c = rc.Case("huge-id", "37", [1], seed=22)
    c.words[0, 200] = 2 ** 31 - 1
    c.words[0, 225] = 1
    with pytest.raises(lib.GomError, match="outside"):
        _run(c)
    assert _run(case)[0]                                                       # the device is fine afterwards
