"""CPU: the dropout mask stream of the training path as a contract ("Dropout"): the generator against the
published Philox4x32-10 known-answer vectors, the stream's first bits, its keep rate and the independence of the streams that
differ in site, iteration, rank or seed (tests/dropout_statement.py); `DropoutState`'s site numbering; the argument checks of
the library's dropout entry points (no GPU needed: they run before any HIP call)."""
import math

import numpy as np
import pytest

import dropout_statement as D


def _hex(words):
    return " ".join("%08x" % int(w[0]) for w in words)


def test_philox_known_answer_vectors():
    assert (D.M0, D.M1, D.W0, D.W1) == (0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85)
    assert _hex(D.philox4x32_10((0, 0, 0, 0), (0, 0))) == "6627e8d5 e169c58d bc57ac4c 9b00dbd8"
    ones = 0xFFFFFFFF
    assert _hex(D.philox4x32_10((ones,) * 4, (ones, ones))) == "408f276d 41c83b0e a20bc7c6 6d5451fd"
    assert _hex(D.philox4x32_10((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0))) == \
        "d16cfe09 94fdcceb 5001e420 24126ea1"


def test_first_keep_bits_of_the_stream():
    bits = lambda p: "".join("1" if k else "0" for k in D.keep_mask(7, 0, 0, 0, 16, p))
    assert bits(0.1) == "1110111100111111"
    assert bits(0.5) == "1100010100110000"
    # a prefix of a longer stream is the shorter stream; element e uses word e & 3 of group e >> 2
    assert np.array_equal(D.keep_mask(7, 0, 0, 0, 4099, 0.1)[:16], D.keep_mask(7, 0, 0, 0, 16, 0.1))
    assert D.threshold(0.5) == 1 << 31 and D.threshold(0.0) == 0 and D.keep_mask(3, 1, 2, 0, 9, 0.0).all()


N = 1 << 20
STREAMS = [((7, 0, 0, 0), 0.1), ((7, 0, 0, 0), 0.5), ((7, 1, 0, 0), 0.1), ((7, 0, 1, 0), 0.1), ((7, 0, 0, 1), 0.1), ((8, 0, 0, 0), 0.1)]


@pytest.fixture(scope="module")
def masks():
    return {(s, p): D.keep_mask(*s, N, p) for s, p in STREAMS}


def test_keep_rate_within_four_sigma(masks):
    for (s, p), m in masks.items():
        sigma = math.sqrt(p * (1 - p) / N)
        off = (m.mean() - (1 - p)) / sigma
        print("stream %s p %.1f: keep rate %.6f, %+.2f sigma" % (s, p, m.mean(), off))
        assert abs(off) <= 4.0, (s, p, off)


def test_site_iteration_rank_and_seed_each_change_the_mask(masks):
    base = masks[((7, 0, 0, 0), 0.1)]
    for s in ((7, 1, 0, 0), (7, 0, 1, 0), (7, 0, 0, 1), (8, 0, 0, 0)):
        agree = float((masks[(s, 0.1)] == base).mean())
        print("stream %s agrees with (7, 0, 0, 0) on %.4f of positions (independent masks: 0.82)" % (s, agree))
        assert abs(agree - 0.82) <= 0.004, (s, agree)


def test_dropout_state_numbers_sites_consecutively_and_restarts_per_forward():
    from gomatching_amd.training import DropoutState
    st = DropoutState(0.1, seed=(1 << 40) + 5, iteration=3, rank=2)
    assert [st.next_site() for _ in range(4)] == [0, 1, 2, 3] and st.site == 4
    assert st.next_stream() == (0.1, (1 << 40) + 5, 4, 3, 2)
    st.begin_forward(9)
    assert st.site == 0 and st.iteration == 9 and st.next_site() == 0 and st.next_site() == 1
    assert st.active and not DropoutState(0.0, 1).active
    for bad in (-0.1, 1.0, 1.5, float("nan")):
        with pytest.raises(ValueError):
            DropoutState(bad, 1)


def test_dropout_entry_points_reject_bad_arguments_without_a_gpu():
    import ctypes
    import __graft_entry__ as entry
    entry.build()
    from gomatching_amd import lib, ops
    L = lib.load()
    INVALID = 1
    p = ctypes.c_void_p(0x1000)
    q = ctypes.c_void_p(0x2000)
    ok = ops.dropout_args(0.1, 7, 0, 0, 0)
    assert ok[4] == D.threshold(0.1) and np.float32(ok[5]) == D.scale_f32(0.1)
    st = lambda pp: ops.dropout_args(pp, 7, 0, 0, 0)
    for pp in (-0.25, 1.0, 1.5):                                   # p outside [0, 1), through the pair the host passes
        assert L.gom_dropout_f32(p, 8, None, 0, q, 8, 2, 8, *st(pp), None) == INVALID, pp
        assert L.gom_softmax_dropout_rows_f32(p, q, 2, 8, 8, 1.0, 0, *st(pp), None) == INVALID, pp
        assert L.gom_softmax_dropout_rows_backward_f32(p, p, q, 2, 8, 8, 1.0, 0, *st(pp), None) == INVALID, pp
    assert L.gom_dropout_f32(p, 8, None, 0, q, 8, 2, 8, 7, 0, 0, 0, D.threshold(0.1), 2.0, None) == INVALID     # scale of another p
    assert L.gom_dropout_f32(p, 8, None, 0, q, 8, 2, 8, 7, 0, 0, 0, D.threshold(0.1), float("nan"), None) == INVALID
    assert L.gom_dropout_f32(None, 8, None, 0, q, 8, 2, 8, *ok, None) == INVALID                                # null x
    assert L.gom_dropout_f32(p, 8, None, 0, None, 8, 2, 8, *ok, None) == INVALID                                # null y
    assert L.gom_dropout_f32(p, 8, None, 0, q, 8, -1, 8, *ok, None) == INVALID                                  # negative size
    assert L.gom_dropout_f32(p, 8, None, 0, q, 8, 2, -8, *ok, None) == INVALID
    assert L.gom_dropout_f32(p, 4, None, 0, q, 8, 2, 8, *ok, None) == INVALID                                   # ld < cols
    assert L.gom_dropout_f32(p, 8, q, 4, q, 8, 2, 8, *ok, None) == INVALID                                      # residual's ld < cols
    assert L.gom_dropout_f32(p, 1 << 33, None, 0, q, 1 << 33, 4, 1 << 33, *ok, None) == INVALID                # e >> 2 beyond 2^32
    assert L.gom_dropout_f32(p, 8, None, 0, q, 8, 0, 8, *ok, None) == 0                                         # nothing to do
    assert L.gom_relu_backward_scaled_f32(None, p, q, 4, 1.5, None) == INVALID
    assert L.gom_relu_backward_scaled_f32(p, p, q, -1, 1.5, None) == INVALID
    assert L.gom_relu_backward_scaled_f32(p, p, q, 4, 0.5, None) == INVALID                                     # 1 / (1 - p) >= 1
    assert L.gom_softmax_dropout_rows_f32(None, q, 2, 8, 8, 1.0, 0, *ok, None) == INVALID
    assert L.gom_softmax_dropout_rows_f32(p, p, 2, 8, 8, 1.0, 0, *ok, None) == INVALID                          # P~ over P
    assert L.gom_softmax_dropout_rows_f32(p, q, 2, 9000, 9000, 1.0, 0, *ok, None) == INVALID                    # > 8192 columns
    assert L.gom_softmax_dropout_rows_f32(p, q, 2, 8, 4, 1.0, 0, *ok, None) == INVALID                          # ld < cols
    assert L.gom_softmax_dropout_rows_f32(p, q, -1, 8, 8, 1.0, 0, *ok, None) == INVALID
    assert L.gom_softmax_dropout_rows_f32(p, q, 2, 8, 8, 1.0, -4, *ok, None) == INVALID                         # negative first element
    assert L.gom_softmax_dropout_rows_f32(p, q, 2, 8, 8, 1.0, 1 << 34, *ok, None) == INVALID
    assert L.gom_softmax_dropout_rows_backward_f32(p, None, q, 2, 8, 8, 1.0, 0, *ok, None) == INVALID
    assert L.gom_softmax_dropout_rows_backward_f32(p, p, q, 2, 8, 4, 1.0, 0, *ok, None) == INVALID
    assert L.gom_softmax_dropout_rows_backward_f32(p, p, q, -2, 8, 8, 1.0, 0, *ok, None) == INVALID
