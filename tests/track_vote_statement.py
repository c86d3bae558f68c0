"""The rule of the track vote (include/gomatching_hip.h, `gom_track_vote_*`) in plain Python: which rows vote, a row's text,
the vote and the lines of preds/res_<video>.txt.  No XML, no numpy, no sorting by anything but the integer id: lists, bytes
and integers only."""

RECS, EMIT, TRACK_ID = 200, 225, 232                            # GOM_RR_RECS, GOM_RR_EMIT, GOM_RR_TRACK_ID
ENTRY_BYTES, ENTRY_MAX = 8, 4                                   # GOM_RT_ENTRY_BYTES, GOM_TV_ENTRY_MAX


class BadId(Exception):
    """An emitted character id outside the table."""


def track_id(row):
    """The int64 in the two id words of a row, low word first."""
    lo, hi = int(row[TRACK_ID]) & 0xFFFFFFFF, int(row[TRACK_ID + 1]) & 0xFFFFFFFF
    v = lo | (hi << 32)
    return v - (1 << 64) if v >= (1 << 63) else v


def row_text(row, table):
    """The text bytes of one row: for every emitted character, in order, the bytes of its table entry.  `table`: a sequence of
    entries of ENTRY_BYTES integers, a length byte and the bytes."""
    emit, out = int(row[EMIT]) & 0xFFFFFFFF, []
    for c in range(25):
        if not (emit >> c) & 1:
            continue
        i = int(row[RECS + c])
        if i < 0 or i >= len(table):
            raise BadId("row emits id %d, the table has %d entries" % (i, len(table)))
        entry = [int(b) for b in table[i]]
        out.extend(entry[1:1 + min(entry[0], ENTRY_MAX)])
    return bytes(out)


def integer(v):
    """Plain decimal, '-' in front of a negative value, digit by digit."""
    v = int(v)
    m, digits = abs(v), ""
    while True:
        digits = "0123456789"[m % 10] + digits
        m //= 10
        if m == 0:
            break
    return ("-" if v < 0 else "") + digits


def vote(voters):
    """voters: [(track id, text bytes, position)] of the voting rows in file order -> (the file's bytes, [(track id, the winner's
    position, its count)] in line order).  The winner of a track is the first of its rows whose text has the greatest count
    among the track's rows; lines go by ascending integer id."""
    tracks = {}
    for tid, text, pos in voters:
        tracks.setdefault(int(tid), []).append((text, pos))
    out, winners = b"", []
    for tid in sorted(tracks):
        rows = tracks[tid]
        best = None
        for text, pos in rows:
            count = 0
            for other, _ in rows:
                if other == text:
                    count += 1
            if best is None or count > best[2]:                 # strictly greater: the first row with the greatest count stays
                best = (text, pos, count)
        out += b'"' + integer(tid).encode("ascii") + b'","' + best[0] + b'"\n'
        winners.append((tid, best[1], best[2]))
    return out, winners


def statement(words, keep, table):
    """Rows of a video in file order (words: the result-row words of every row, keep: its flag) -> `vote`'s pair, positions
    being row indices.  A kept row with a bad id raises BadId."""
    voters = []
    for r in range(len(words)):
        if keep[r]:
            voters.append((track_id(words[r]), row_text(words[r], table), r))
    return vote(voters)
