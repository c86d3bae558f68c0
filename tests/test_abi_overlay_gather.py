"""CPU: `gom_overlay_compose_gather_u8` is bound from include/gomatching_hip.h as the header states it, and its launcher
refuses bad arguments before any HIP call (no compute, no device)."""
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


def test_signature_is_the_headers():
    from gomatching_amd import lib
    P, I, L = C.c_void_p, C.c_int, C.c_long
    dense, gather = _args("gom_overlay_compose_u8"), _args("gom_overlay_compose_gather_u8")
    assert gather[:7] == ["const uint8_t* ring", "int cap", "const int32_t* slots", "uint8_t* out", "int F", "int H", "int W"]
    assert dense[:5] == ["const uint8_t* frames", "uint8_t* out", "int F", "int H", "int W"]
    assert gather[7:] == dense[5:] and gather[7] == "const uint32_t* face_words" and gather[-1] == "void* stream"
    assert lib.SIGNATURES["gom_overlay_compose_gather_u8"] == (
        I, [P, I, P, P, I, I, I, P, P, P, P, I, L, P, P, P, P, P, P, I, P, P, P, I, L, I, I, P])
    assert lib.SIGNATURES["gom_overlay_compose_gather_u8"][1][7:] == lib.SIGNATURES["gom_overlay_compose_u8"][1][5:]
    assert hasattr(lib.load(), "gom_overlay_compose_gather_u8")


def test_the_header_states_the_rule():
    text = " ".join(open(os.path.join(ROOT, "include", "gomatching_hip.h")).read().replace(" *", " ").split())
    assert "out[f] is word for word what gom_overlay_compose_u8 writes for frames[f] = ring[slots[f]]" in text


def test_bad_arguments_are_refused_without_a_gpu():
    from gomatching_amd import lib
    L = lib.load()
    OK, INVALID = 0, 1
    H, W, cap = 8, 8, 5
    ring = 0x100000                                           # non-null, never dereferenced
    p, odd = C.c_void_p(0x1000), C.c_void_p(0x1004)
    past = ring + cap * H * W * 3                             # the first byte after the ring

    def gather(ring=ring, cap=cap, slots=p, out=past, F=2, H=H, W=W, boxes=p, N=1, nwords=4, Lb=1, G=1, gwords=4, a_face=128,
               a_box=204, inst_off=p):
        v = lambda a: a if a is None or isinstance(a, C.c_void_p) else C.c_void_p(a)
        return L.gom_overlay_compose_gather_u8(v(ring), cap, slots, v(out), F, H, W, p, p, boxes, p, N, nwords, inst_off, p, p, p,
                                               p, p, Lb, p, p, p, G, gwords, a_face, a_box, None)
    assert gather(cap=0) == INVALID and gather(cap=-1) == INVALID
    assert gather(F=-1) == INVALID
    assert gather(ring=None) == INVALID and gather(out=None) == INVALID
    assert gather(slots=None) == INVALID                                  # ... with F > 0
    assert gather(slots=None, F=0) == OK                                  # no frames: no launch, no table needed
    assert gather(out=ring) == INVALID                                    # `out` inside [ring, ring + cap * H * W * 3)
    assert gather(out=ring + 1) == INVALID and gather(out=past - 1) == INVALID
    assert gather(out=ring - 1) == INVALID                                # ... or reaching into it from below
    assert gather(a_face=256) == INVALID and gather(a_box=-1) == INVALID
    # the dense entry's checks
    assert gather(inst_off=None) == INVALID and gather(boxes=None) == INVALID and gather(boxes=odd) == INVALID
    assert gather(N=-1) == INVALID and gather(Lb=-1) == INVALID and gather(nwords=-1) == INVALID
    assert gather(H=0) == INVALID and gather(W=0) == INVALID and gather(H=65536, W=32768) == INVALID
    assert gather(G=0) == INVALID                                         # labels without an atlas
    assert gather(F=0) == OK
