"""CPU: the result text entry points are bound from include/gomatching_hip.h as the header states them, their constants reach
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
    count, emit = _args("gom_result_text_count_scan"), _args("gom_result_text_emit")
    inputs = ["const int32_t* words", "int ld", "const int64_t* pts", "const uint8_t* keep", "int n", "const int32_t* frame_rows",
              "int F", "long first_frame", "const uint8_t* json_tab", "const uint8_t* xml_tab", "int ntab"]
    assert count == inputs + ["int32_t* row_len", "int64_t* row_off", "int32_t* row_kept", "int64_t* frame_off", "int64_t* totals",
                              "void* stream"]
    assert emit == inputs + ["const int32_t* row_len", "const int64_t* row_off", "const int32_t* row_kept",
                             "const int64_t* frame_off", "uint8_t* json", "long json_cap", "uint8_t* xml", "long xml_cap", "void* stream"]
    common = [P, I, P, P, I, P, I, L, P, P, I]
    assert lib.SIGNATURES["gom_result_text_count_scan"] == (I, common + [P, P, P, P, P, P])
    assert lib.SIGNATURES["gom_result_text_emit"] == (I, common + [P, P, P, P, P, L, P, L, P])
    loaded = lib.load()
    assert hasattr(loaded, "gom_result_text_count_scan") and hasattr(loaded, "gom_result_text_emit")


def test_constants_come_from_the_header():
    from gomatching_amd import lib, ops, results
    assert ops.RESULT_TEXT_ENTRY_BYTES == results.TEXT_ENTRY_BYTES == lib.CONSTANTS["GOM_RT_ENTRY_BYTES"] == 8
    block = ops.RESULT_TEXT_SCAN_BLOCK
    assert block == lib.CONSTANTS["GOM_RT_SCAN_BLOCK"] and block % 64 == 0 and 64 <= block <= 1024
    assert lib.CONSTANTS["GOM_RT_STATUS"] < lib.CONSTANTS["GOM_RT_TOTALS"] and lib.CONSTANTS["GOM_RT_BAD_ID"] != 0


def test_bad_arguments_are_refused_without_a_gpu():
    from gomatching_amd import lib
    L = lib.load()
    p = C.c_void_p(0x1000)                                    # non-null, never dereferenced
    ld = lib.CONSTANTS["GOM_RESULT_ROWS_WORDS"]

    def count(n=1, F=1, ld=ld, first=0, ntab=36, words=p, totals=p):
        return L.gom_result_text_count_scan(words, ld, p, p, n, p, F, first, p, p, ntab, p, p, p, p, totals, None)

    def emit(n=1, F=1, first=0, json_cap=10, xml_cap=10, json=p):
        return L.gom_result_text_emit(p, ld, p, p, n, p, F, first, p, p, 36, p, p, p, p, json, json_cap, p, xml_cap, None)

    for rc in (count(n=0), count(F=0), count(n=-1), count(ld=ld - 1), count(first=-1), count(first=2 ** 31 - 2), count(ntab=0),
               count(words=None), count(totals=None), emit(n=0), emit(F=0), emit(json_cap=-1), emit(xml_cap=-1), emit(json=None),
               emit(first=-1)):
        assert rc == 1                                        # GOM_ERR_INVALID_ARG
