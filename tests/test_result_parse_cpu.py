"""CPU: the rule of the result parser as tests/result_parse_statement.py states it -- on every clean and damaged case either a
nonzero status or the input back, byte for byte, from json.dumps of what was parsed; every clean case accepted -- the host side of
`results.ParsedRows`, and `show.label_anchors` bit for bit against `show.label_anchor`."""
import json
import random

import numpy as np
import pytest

import result_parse_cases as rc
import result_parse_statement as rps
from gomatching_amd import results, show


@pytest.fixture(scope="module")
def parsed():
    """(name, bytes, status, arrays) of every case, the statement run once."""
    return [(n, d) + rps.parse(d) for n, d in rc.clean_cases() + rc.damaged_cases()]


def test_clean_families_are_accepted():
    names = [n for n, _ in rc.clean_cases()]
    assert any(n.startswith("golden") for n in names) and "long" in names
    for n, d in rc.clean_cases():
        st, a = rps.parse(d)
        assert st == 0, (n, st)
        assert a["F"] == len(json.loads(d))
    size = dict(rc.clean_cases())["long"]
    assert len(size) > rc.BLOCK * rc.BLOCK_BYTES + 2 * rc.BLOCK_BYTES and size.count(b"\n") > rc.BLOCK * rc.BLOCK


def test_status_zero_means_the_text_comes_back(parsed):
    refused = 0
    for name, data, st, a in parsed:
        if st:
            refused += 1
            continue
        assert rps.reserialise(data, a) == data, name
    assert refused > 300                                       # the damaged corpus is damaged


def test_what_json_loads_refuses_is_never_accepted(parsed):
    for name, data, st, a in parsed:
        try:
            doc = json.loads(data.decode("utf-8"))
        except (ValueError, UnicodeError):
            assert st != 0, name
            continue
        if st == 0:
            assert rps.annotation(data, a) == doc, name


def test_the_causes_are_told_apart(parsed):
    by = {n: st for n, _, st, _ in parsed}
    assert by["token 1.5 in points"] == by["token 01 in seg"] == by["token -0 in points"] == rps.BAD_INT
    assert by["token 12345678901234567890 in seg"] == by["token 2147483648 in points"] == rps.BAD_INT
    assert by["token true in points"] == by["tab indent"] == by["extra key"] == rps.BAD_PLACE
    assert by["keys 1 3"] == by["keys from 0"] == by["key 01"] == rps.BAD_KEY
    assert by["7 points"] == by["9 points, segmentation"] == rps.BAD_POINTS
    assert by["trailing newline"] == by["no indent"] == by["one byte"] == rps.BAD_ENDS
    assert by["long line"] == by["escaped quote at the end"] == rps.BAD_LINE
    assert by["escape json.dumps does not write"] == by["ensure_ascii"] == by["raw control byte"] == rps.BAD_STRING
    assert by["two contours"] & rps.BAD_PLACE and by["crlf"] == rps.BAD_ENDS and by["indent 2"] & rps.BAD_PLACE
    assert rps.parse(b"")[0] == rps.BAD_SIZE


def _rows(data, a):
    host = [a[k] for k in ("frame_rows", "ids", "t_off", "t_len", "has_seg", "poly_off", "poly_xy")]
    return results.ParsedRows(0, None, host, results.decode_spans(data, a["t_off"], a["t_len"]), pts=a["pts"])


def test_to_annotation_is_rows_of_json():
    for name, data in rc.clean_cases():
        st, a = rps.parse(data)
        assert st == 0
        assert _rows(data, a).to_annotation() == show.rows_of_json(json.loads(data)), name


def test_decode_spans_refuses_what_the_statement_refuses(parsed):
    for name, data, st, a in parsed:
        if st == rps.BAD_STRING:
            # the device side of such a file is clean: find the spans with the statement's own line functions
            spans = [ln for ln in data.split(b"\n") if ln.startswith(b" " * 12 + b'"transcription": "')]
            offs = [(data.index(ln) + 30, rps.string_line(ln)[2]) for ln in spans]
            assert results.decode_spans(data, np.asarray([o for o, _ in offs]), np.asarray([n for _, n in offs])) is None, name


def _polygons():
    rng = random.Random(23)
    polys = [[], [[3, 4]], [[0, 0], [10, 7]], [[5, 5]] * 6, [[0, 0], [0, 0], [4, 4], [4, 4]],
             [[0, 0], [1, 0], [2, 0], [2, 1], [1, 1], [0, 1]],                    # a half-integer centre line
             [[0, 0], [3, 0], [3, 3], [0, 3], [1, 1]], [[-7, 2], [9, -3], [4, 4]]]
    for n in (3, 5, 7, 16, 17, 49, 50, 50, 50, 51, 99, 100, 257):
        for _ in range(6):
            polys.append([[rng.randint(-300, 2000), rng.randint(-300, 1200)] for _ in range(n)])
    for _ in range(40):                                        # zero-length segments among the others
        p = [[rng.randint(0, 30), rng.randint(0, 30)] for _ in range(25)]
        polys.append(p + p[::-1])
    for name, data in rc.clean_cases():
        if name != "long":
            for objs in json.loads(data).values():
                polys.extend(o["segmentation"][0] for o in objs if "segmentation" in o)
    return polys


def test_label_anchors_is_label_anchor_bit_for_bit():
    polys = _polygons()
    off = np.concatenate([[0], np.cumsum([len(p) for p in polys])])
    xy = np.asarray([q for p in polys for q in p], dtype=np.int64).reshape(-1, 2)
    got = show.label_anchors(xy, off)
    want = np.asarray([show.label_anchor(np.asarray(p, dtype=np.int64).reshape(-1, 2)) for p in polys], dtype=np.int64)
    assert got.dtype == np.int64 and np.array_equal(got, want)
    assert show.label_anchors(np.zeros((0, 2), np.int32), np.zeros(1, np.int32)).shape == (0, 2)
