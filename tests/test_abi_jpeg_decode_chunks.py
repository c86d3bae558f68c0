"""CPU: the chunked entropy walk's entry point is bound from include/gomatching_hip.h as the header states it, its constants
reach Python from there, and it refuses a bad chunk size before any HIP call (no compute, no device)."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _args(name):
    text = open(os.path.join(ROOT, "include", "gomatching_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^()]*)\)\s*;" % name, text)
    assert m, name
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_signature_is_the_headers():
    from gomatching_amd import lib
    P, I, L = C.c_void_p, C.c_int, C.c_long
    serial = _args("gom_jpeg_decode_entropy_i16")
    chunks = _args("gom_jpeg_decode_entropy_chunks_i16")
    assert chunks == serial[:-1] + ["int chunk_bytes", "int32_t* seg_info", "void* stream"]     # the serial entry's, and two more
    assert lib.SIGNATURES["gom_jpeg_decode_entropy_i16"] == (I, [P, L, P, I, P, P, I, I, I, I, I, I, I, P, L, P, P, P])
    assert lib.SIGNATURES["gom_jpeg_decode_entropy_chunks_i16"] == (I, [P, L, P, I, P, P, I, I, I, I, I, I, I, P, L, P, P, I, P, P])
    assert hasattr(lib.load(), "gom_jpeg_decode_entropy_chunks_i16")


def test_constants_come_from_the_header():
    from gomatching_amd import jpeg, lib, ops
    assert jpeg.CHUNK_BYTES == ops.JPEG_DECODE_CHUNK_BYTES == lib.CONSTANTS["GOM_JPEG_DECODE_CHUNK_BYTES"]
    assert jpeg.AUTO_SEGMENT_BYTES == lib.CONSTANTS["GOM_JPEG_DECODE_AUTO_SEGMENT_BYTES"]
    c = jpeg.CHUNK_BYTES
    assert 16 <= c <= 4096 and c & (c - 1) == 0


@pytest.mark.parametrize("chunk", (24, 8, 8192, 0, -256))
def test_a_bad_chunk_size_is_refused_without_a_gpu(chunk):
    from gomatching_amd import lib
    L = lib.load()
    p = C.c_void_p(0x1000)                                    # non-null, 256-byte aligned, never dereferenced
    call = lambda cb, info=p: L.gom_jpeg_decode_entropy_chunks_i16(p, 4, p, 1, p, p, 1, 1, 16, 16, 3, 2, 2, p, 1 << 20, p, p, cb, info, None)
    assert call(chunk) == 1                                   # GOM_ERR_INVALID_ARG
    assert call(256, None) == 1                               # a null seg_info
    assert L.gom_jpeg_decode_entropy_chunks_i16(p, 4, p, 1, p, p, 1, 1, 16, 4097, 3, 2, 2, p, 1 << 20, p, p, 256, p, None) == 2   # too wide
