"""GPU: `ops.track_vote_records` / `ops.track_vote` and `results.TrackVote` (csrc/track_vote.hip) against the plain-Python
statement (tests/track_vote_statement.py) on the shared cases (tests/track_vote_cases.py: ties, dropped tracks, integer order
of the ids and the high word, the empty text, 100-byte texts, texts that differ in the last byte, ids that share an entry,
tracks around the block size with the winner in the last tile, more tracks than a scan block, two rows of a track in a frame):
the records against a derivation from the words, the bytes, winners and counts, the same video cut into calls three ways, an
id outside the table, and two runs of one vote."""
import numpy as np
import pytest
import torch

import track_vote_cases as tc
import track_vote_statement as st

from gomatching_amd import lib, ops, results

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASES = tc.cases()


def _table(case):
    return torch.from_numpy(case.table()).to(DEV)


def _records(case, r0=0, r1=None):
    r1 = len(case.keep) if r1 is None else r1
    return ops.track_vote_records(torch.from_numpy(case.words[r0:r1]).to(DEV), torch.from_numpy(case.keep[r0:r1]).to(DEV),
                                  _table(case))


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_records_are_the_words(case):
    n = len(case.keep)
    rec = _records(case)
    assert rec.dtype == torch.int32 and tuple(rec.shape) == (n, tc.RECORD_WORDS)
    rec = rec.cpu().numpy()
    table = case.table()
    for r in range(n):
        assert rec[r, 0:2].copy().view(np.int64)[0] == st.track_id(case.words[r])
        text = st.row_text(case.words[r], table) if case.keep[r] else b""
        assert rec[r, 2] == (len(text) if case.keep[r] else -1), (case.name, r)
        assert rec[r, 3:].astype("<i4").tobytes() == text + b"\0" * (100 - len(text)), (case.name, r)


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_vote_is_the_statement(case):
    want_text, want_winners = case.statement()
    rec = _records(case)
    text, ids, pos, count = ops.track_vote(rec)
    assert text.dtype == torch.uint8 and ids.dtype == torch.int64 and pos.dtype == count.dtype == torch.int32
    assert text.cpu().numpy().tobytes() == want_text, case.name
    assert list(zip(ids.tolist(), pos.tolist(), count.tolist())) == want_winners, case.name
    again = ops.track_vote(rec)                                 # bitwise reproducible
    assert again[0].cpu().numpy().tobytes() == want_text and again[2].tolist() == pos.tolist()


@pytest.mark.parametrize("name", ["tiles", "300-tracks", "two-rows-one-frame", "dropped-track", "no-rows"])
def test_the_cut_into_calls_does_not_matter(name):
    case = {c.name: c for c in CASES}[name]
    want = case.statement()[0]
    F = len(case.frame_rows) - 1
    cuts = {"one call": [0, F], "a call per frame": list(range(F + 1)), "uneven": sorted({0, F // 7, F // 7 + 1, (2 * F) // 3, F})}
    table = tc.Labels(case.decoder.labels)                      # (a decoder of its own: the table cache is per decoder)
    for how, cut in cuts.items():
        vote = results.TrackVote(table)
        for f0, f1 in zip(cut[:-1], cut[1:]):
            r0, r1 = int(case.frame_rows[f0]), int(case.frame_rows[f1])
            vote.add(torch.from_numpy(case.words[r0:r1]).to(DEV), torch.from_numpy(case.keep[r0:r1]).to(DEV))
        assert vote.rows == len(case.keep)
        assert vote.finish() == want, (name, how)
        with pytest.raises(ValueError):
            vote.finish()
    if len(case.keep):
        assert list(table.__dict__["_txt_table"]) == [DEV]      # uploaded once per decoder and device


def test_a_bad_id_raises():
    case = tc.Case("bad", "37").add(0, 1, "ok").add(1, 1, recs=[36] + [0] * 24, emit=1).add(2, 1, "ok").build()
    rec = _records(case)
    assert rec[:, 2].tolist() == [2, lib.CONSTANTS["GOM_TV_LEN_BAD"], 2] and rec[1, 3:].abs().sum().item() == 0
    with pytest.raises(lib.GomError, match="outside the table"):
        ops.track_vote(rec)
    case = tc.Case("bad-but-dropped", "37").add(0, 1, "ok").add(1, 1, recs=[-5] + [0] * 24, emit=1, keep=0).build()
    assert ops.track_vote(_records(case))[0].cpu().numpy().tobytes() == b'"1","ok"\n'


def test_wrong_tensors_are_refused_on_the_host():
    case = CASES[0]
    rec = _records(case)
    for bad in (rec.cpu(), rec.to(torch.int64), rec[:, :27], rec[:, :27].contiguous(), rec.t()):
        with pytest.raises(ValueError):
            ops.track_vote(bad)
    words, keep = torch.from_numpy(case.words).to(DEV), torch.from_numpy(case.keep).to(DEV)
    for args in ((words[:, :200], keep, _table(case)), (words, keep[:-1], _table(case)), (words, keep, _table(case)[:, :4]),
                 (words, keep.to(torch.int32), _table(case))):
        with pytest.raises(ValueError):
            ops.track_vote_records(*args)
