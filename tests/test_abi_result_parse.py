"""CPU: the result parse entry points are bound from include/gomatching_hip.h as the header states them, their constants reach
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
    assert _args("gom_result_parse_lines") == ["const uint8_t* data", "long size", "int32_t* blk", "int nblk", "int64_t* totals",
                                               "void* stream"]
    assert _args("gom_result_parse_marks") == ["const uint8_t* data", "long size", "const int32_t* blk", "int nblk", "long L",
                                               "int32_t* line_start", "int32_t* mblk", "int32_t* sblk", "int nmblk",
                                               "int64_t* totals", "void* stream"]
    assert _args("gom_result_parse_emit") == [
        "const uint8_t* data", "long size", "const int32_t* line_start", "long L", "const int32_t* mblk", "int nmblk", "int F",
        "int N", "int32_t* mark_line", "int32_t* obj_mark", "int32_t* frame_mark", "int32_t* frame_rows", "int32_t* poly_off",
        "int64_t* ids", "int32_t* pts", "uint8_t* has_seg", "int64_t* t_off", "int32_t* t_len", "int32_t* poly_xy", "long cap_p",
        "int32_t* unit_status", "int64_t* totals", "void* stream"]
    assert lib.SIGNATURES["gom_result_parse_lines"] == (I, [P, L, P, I, P, P])
    assert lib.SIGNATURES["gom_result_parse_marks"] == (I, [P, L, P, I, L, P, P, P, I, P, P])
    assert lib.SIGNATURES["gom_result_parse_emit"] == (I, [P, L, P, L, P, I, I, I] + [P] * 11 + [L, P, P, P])
    loaded = lib.load()
    for name in ("gom_result_parse_lines", "gom_result_parse_marks", "gom_result_parse_emit"):
        assert hasattr(loaded, name)


def test_constants_come_from_the_header():
    from gomatching_amd import lib, ops
    K = lib.CONSTANTS
    bits = [K["GOM_RP_BAD_" + n] for n in ("PLACE", "INT", "KEY", "POINTS", "LINE", "ENDS", "SIZE", "STRING", "CAP")]
    assert all(b > 0 and b & (b - 1) == 0 for b in bits) and len(set(bits)) == len(bits)      # one bit per cause
    assert K["GOM_RP_BLOCK"] % 64 == 0 and 64 <= K["GOM_RP_BLOCK"] <= 1024
    assert K["GOM_RP_BLOCK_BYTES"] == K["GOM_RP_BLOCK"] * K["GOM_RP_THREAD_BYTES"] and K["GOM_RP_THREAD_BYTES"] == 16
    assert ops.RESULT_PARSE_MAX_SIZE == K["GOM_RP_MAX_SIZE"] == 2 ** 31 - 2 and ops.RESULT_PARSE_BAD_SIZE == K["GOM_RP_BAD_SIZE"]
    slots = [K["GOM_RP_" + n] for n in ("L", "F", "N", "P", "STATUS", "STATUS_LINES", "STATUS_MARKS")]
    assert sorted(slots) == list(range(7)) and K["GOM_RP_TOTALS"] >= 7


def test_bad_arguments_are_refused_without_a_gpu():
    from gomatching_amd import lib
    L = lib.load()
    p = C.c_void_p(0x1000)                                    # non-null, never dereferenced
    B = lib.CONSTANTS["GOM_RP_BLOCK_BYTES"]

    def lines(data=p, size=100, blk=p, nblk=1, totals=p):
        return L.gom_result_parse_lines(data, size, blk, nblk, totals, None)

    def marks(data=p, size=100, nblk=1, Ln=10, line_start=p, nmblk=1, totals=p):
        return L.gom_result_parse_marks(data, size, p, nblk, Ln, line_start, p, p, nmblk, totals, None)

    def emit(data=p, size=100, Ln=10, nmblk=1, F=1, N=1, ids=p, cap_p=2, totals=p):
        return L.gom_result_parse_emit(data, size, p, Ln, p, nmblk, F, N, p, p, p, p, p, ids, p, p, p, p, p, cap_p, p, totals, None)

    for rc in (lines(data=None), lines(blk=None), lines(totals=None), lines(size=0), lines(size=-1), lines(nblk=2), lines(nblk=0),
               lines(size=2 ** 31 - 1, nblk=(2 ** 31 - 1 + B - 1) // B), lines(size=2 ** 31, nblk=2 ** 31 // B),
               lines(size=2 ** 40, nblk=1),
               marks(data=None), marks(size=0), marks(size=2 ** 31 - 1, nblk=(2 ** 31 - 1 + B - 1) // B), marks(Ln=1), marks(Ln=0),
               marks(Ln=-5), marks(Ln=102), marks(nmblk=2), marks(line_start=None), marks(totals=None), marks(nblk=3),
               emit(data=None), emit(size=0), emit(size=2 ** 31 - 1), emit(Ln=1), emit(Ln=102), emit(nmblk=0), emit(F=0), emit(N=-1),
               emit(F=6, N=5), emit(ids=None), emit(cap_p=-1), emit(totals=None)):
        assert rc == 1                                        # GOM_ERR_INVALID_ARG


def test_the_wrapper_refuses_sizes_without_a_launch():
    """A file of 0 bytes is refused with GOM_RP_BAD_SIZE on the host (as one of 2^31 - 1 bytes or more is: the same comparison)."""
    from gomatching_amd import lib, results
    rows = results.parse_json_device(b"", "cpu")
    assert rows.status == lib.CONSTANTS["GOM_RP_BAD_SIZE"] and rows.causes() == ["size"]


def test_scene_polygons_is_bound_and_refuses_bad_arguments():
    from gomatching_amd import lib, ops, show
    P, I = C.c_void_p, C.c_int
    assert lib.SIGNATURES["gom_scene_polygons_i32"] == (I, [P, I, P, P, I, P, I, I, I, I, I, P, I, P, I, P, P, P, P, P, P, I, P, P])
    assert ops.SCENE_PALETTE == lib.CONSTANTS["GOM_SP_PALETTE"] == show.PALETTE_SIZE == len(show.INK)
    assert lib.CONSTANTS["GOM_SP_MAX_COORD"] == 2 ** 20 and lib.CONSTANTS["GOM_SP_BLOCK"] % 64 == 0
    L = lib.load()
    p = C.c_void_p(0x1000)                                    # non-null, 16-byte aligned, never dereferenced

    def scene(frame_rows=p, F=4, N=6, Pn=9, f0=1, f1=3, H=48, W=64, n_cont=2, n_inst=3, boxes=p, xy=p, status=p):
        return L.gom_scene_polygons_i32(frame_rows, F, p, p, N, xy, Pn, f0, f1, H, W, p, 1, p, n_cont, p, boxes, p, p, p, p, n_inst,
                                        status, None)

    for rc in (scene(frame_rows=None), scene(status=None), scene(F=0), scene(N=-1), scene(Pn=-1), scene(f0=-1), scene(f0=3),
               scene(f1=5), scene(H=0), scene(W=0), scene(H=65536, W=65536), scene(n_cont=4), scene(n_cont=-1), scene(n_inst=-1),
               scene(boxes=C.c_void_p(0x1008)), scene(xy=C.c_void_p(0x1004))):
        assert rc == 1                                        # GOM_ERR_INVALID_ARG
