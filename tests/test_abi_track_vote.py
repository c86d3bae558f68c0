"""CPU: the track vote entry points are bound from include/gomatching_hip.h as the header states them, their constants reach
Python from there, and they refuse bad arguments before any HIP call (no compute, no device)."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _args(name):
    text = open(os.path.join(ROOT, "include", "gomatching_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^()]*)\)\s*;" % name, text)
    assert m, name
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_signatures_are_the_headers():
    from gomatching_amd import lib
    P, I, L = C.c_void_p, C.c_int, C.c_long
    assert _args("gom_track_vote_records_i32") == ["const int32_t* words", "int ld", "const uint8_t* keep", "int n",
                                                   "const uint8_t* txt_tab", "int ntab", "int32_t* records", "void* stream"]
    assert _args("gom_track_vote_count_scan") == ["const int32_t* records", "long m", "const int32_t* order", "long nv",
                                                  "const int32_t* seg", "int T", "int32_t* winner", "int64_t* line_off",
                                                  "int64_t* totals", "void* stream"]
    assert _args("gom_track_vote_emit") == ["const int32_t* records", "long m", "const int32_t* winner", "const int64_t* line_off",
                                            "int T", "uint8_t* out", "long cap", "void* stream"]
    assert lib.SIGNATURES["gom_track_vote_records_i32"] == (I, [P, I, P, I, P, I, P, P])
    assert lib.SIGNATURES["gom_track_vote_count_scan"] == (I, [P, L, P, L, P, I, P, P, P, P])
    assert lib.SIGNATURES["gom_track_vote_emit"] == (I, [P, L, P, P, I, P, L, P])
    loaded = lib.load()
    for name in ("gom_track_vote_records_i32", "gom_track_vote_count_scan", "gom_track_vote_emit"):
        assert hasattr(loaded, name)


def test_constants_come_from_the_header():
    import track_vote_cases as tc
    import track_vote_statement as st
    from gomatching_amd import lib, ops, results
    K = lib.CONSTANTS
    assert ops.TRACK_VOTE_RECORD_WORDS == tc.RECORD_WORDS == K["GOM_TV_RECORD_WORDS"] == 28
    assert K["GOM_TV_LEN"] == 2 and K["GOM_TV_TEXT"] == 3 and K["GOM_TV_TEXT"] + K["GOM_TV_TEXT_WORDS"] == K["GOM_TV_RECORD_WORDS"]
    assert ops.TRACK_VOTE_ENTRY_MAX == results.TXT_ENTRY_MAX == st.ENTRY_MAX == K["GOM_TV_ENTRY_MAX"] == 4
    assert 25 * K["GOM_TV_ENTRY_MAX"] == 4 * K["GOM_TV_TEXT_WORDS"]          # the longest text fills the record
    assert K["GOM_TV_ENTRY_MAX"] < K["GOM_RT_ENTRY_BYTES"] == st.ENTRY_BYTES
    assert K["GOM_TV_LEN_DROPPED"] == -1 and K["GOM_TV_LEN_BAD"] == -2
    block = ops.TRACK_VOTE_BLOCK
    assert block == tc.BLOCK == K["GOM_TV_BLOCK"] and block % 64 == 0 and 64 <= block <= 1024
    assert K["GOM_TV_STATUS"] < K["GOM_TV_TOTALS"] and K["GOM_TV_BAD_ID"] != 0 and K["GOM_TV_BAD_ORDER"] & K["GOM_TV_BAD_ID"] == 0
    assert (st.RECS, st.EMIT, st.TRACK_ID) == (K["GOM_RR_RECS"], K["GOM_RR_EMIT"], K["GOM_RR_TRACK_ID"])


def test_bad_arguments_are_refused_without_a_gpu():
    from gomatching_amd import lib
    L = lib.load()
    p = C.c_void_p(0x1000)                                    # non-null, never dereferenced
    ld = lib.CONSTANTS["GOM_RESULT_ROWS_WORDS"]

    def records(n=1, ld=ld, ntab=36, words=p, keep=p, tab=p, out=p):
        return L.gom_track_vote_records_i32(words, ld, keep, n, tab, ntab, out, None)

    def count(m=4, nv=3, T=2, records=p, order=p, seg=p, winner=p, off=p, totals=p):
        return L.gom_track_vote_count_scan(records, m, order, nv, seg, T, winner, off, totals, None)

    def emit(m=4, T=2, cap=10, records=p, winner=p, off=p, out=p):
        return L.gom_track_vote_emit(records, m, winner, off, T, out, cap, None)

    for rc in (records(n=0), records(n=-1), records(ld=ld - 1), records(ntab=0), records(words=None), records(keep=None),
               records(tab=None), records(out=None),
               count(m=0), count(m=2 ** 31), count(nv=0), count(nv=5), count(T=0), count(T=4), count(records=None),
               count(order=None), count(seg=None), count(winner=None), count(off=None), count(totals=None),
               emit(m=0), emit(m=2 ** 31), emit(T=0), emit(cap=-1), emit(records=None), emit(winner=None), emit(off=None),
               emit(out=None)):
        assert rc == 1                                        # GOM_ERR_INVALID_ARG
