"""The rule of the lexicon correction of rows (include/gomatching_hip.h, `gom_lexicon_rows_*`) in plain Python: a row's query
through the norm table, the match (tests/lexicon_statement.py), the apply step, and the corrected text of the three files --
the result text statement and the track vote statement with the transcription piece taken from a display form.  Lists, strings,
bytes and integers only; the display forms come in as the caller escaped them."""
import lexicon_statement as ls
import result_text_statement as rts
import track_vote_statement as tvs

RECS, EMIT = 200, 225                                           # GOM_RR_RECS, GOM_RR_EMIT
MAX_LEN = 64                                                    # GOM_LEXICON_MAX_LEN
NORM_WORDS = 4                                                  # GOM_LR_NORM_WORDS


class TooLong(Exception):
    """A kept row whose query has more than MAX_LEN code points; .row is its index."""

    def __init__(self, row):
        Exception.__init__(self, "row %d" % row)
        self.row = row


def norm_entry(label):
    """One norm-table entry: a count and the code points of label.upper(), padded to NORM_WORDS integers."""
    up = [ord(c) for c in label.upper()]
    assert len(up) <= NORM_WORDS - 1
    return [len(up)] + up + [0] * (NORM_WORDS - 1 - len(up))


def query(row, keep, norm_tab):
    """The code points of one row's query.  A row that is not kept, or that emits an id outside the table, has the empty one."""
    if not keep:
        return []
    emit = int(row[EMIT]) & 0xFFFFFFFF
    ids = [int(row[RECS + c]) for c in range(25) if (emit >> c) & 1]
    if any(i < 0 or i >= len(norm_tab) for i in ids):
        return []
    out = []
    for i in ids:
        entry = [int(v) for v in norm_tab[i]]
        out.extend(entry[1:1 + min(entry[0], NORM_WORDS - 1)])
    return out


def apply(words, keep, norm_tab, lex_words, max_dist, drop):
    """Rows of a call and the lexicon's normalised words (strings or lists of code points) -> (queries, ov, keep_out, totals):
    totals = {kept rows in, accepted, dropped}.  Raises TooLong for the first kept row above the limit."""
    lex_words = [[ord(c) for c in w] if isinstance(w, str) else list(w) for w in lex_words]
    queries, ov, keep_out, kept, accepted, dropped = [], [], [], 0, 0, 0
    for r in range(len(words)):
        q = query(words[r], keep[r], norm_tab)
        if len(q) > MAX_LEN:
            raise TooLong(r)
        queries.append(q)
        index, dist = ls.match(q, lex_words)
        ok = bool(keep[r]) and index >= 0 and dist <= max_dist
        out = bool(keep[r]) and (ok or not drop)
        ov.append(index if ok else -1)
        keep_out.append(1 if out else 0)
        kept += 1 if keep[r] else 0
        accepted += 1 if ok else 0
        dropped += 1 if keep[r] and not out else 0
    return queries, ov, keep_out, (kept, accepted, dropped)


def _row(row, text):
    return list(row[:9]) + [text] + list(row[10:])


def corrected_text(frames, first_frame, frame_ov, json_forms, xml_forms):
    """frames: per frame the rows that are still kept (`frame_lines`' form, the transcription being the row's own text);
    frame_ov: per frame, per such row, the override (-1 or a word's index); json_forms / xml_forms: the display forms per word as
    STRINGS already escaped for their stream -> (json str, xml str) of the call between the files' header and footer."""
    js, xs = "", ""
    for f, (rows, ovs) in enumerate(zip(frames, frame_ov)):
        # a display form goes in as it is: the pieces around the transcription are the statement's, the piece itself is not escaped again
        jrows = [rts.row_json(_row(r, "@@OV@@")).replace("@@OV@@", json_forms[o]) if o >= 0 else rts.row_json(r) for r, o in zip(rows, ovs)]
        xrows = [rts.row_xml(_row(r, "@@OV@@")).replace("@@OV@@", xml_forms[o]) if o >= 0 else rts.row_xml(r) for r, o in zip(rows, ovs)]
        head = (",\n" if first_frame + f else "") + '    "' + rts.integer(first_frame + f + 1) + '": '
        js += head + ("[]" if not rows else "[\n" + ",\n".join(jrows) + "\n    ]")
        tag = '  <frame ID="' + rts.integer(first_frame + f + 1)
        xs += tag + '"/>\n' if not rows else tag + '">\n' + "".join(xrows) + "  </frame>\n"
    return js, xs


def corrected_vote(words, keep_out, ov, txt_table, txt_forms):
    """The vote over the corrected words: a row with ov >= 0 votes with txt_forms[ov] (bytes), any other kept row with its own
    text through the txt table -> the bytes of the corrected preds/res_<video>.txt."""
    voters = []
    for r in range(len(words)):
        if keep_out[r]:
            text = bytes(txt_forms[ov[r]]) if ov[r] >= 0 else tvs.row_text(words[r], txt_table)
            voters.append((tvs.track_id(words[r]), text, r))
    return tvs.vote(voters)[0]
