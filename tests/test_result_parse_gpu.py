"""GPU: csrc/result_parse.hip against tests/result_parse_statement.py on every clean and damaged case -- the status word always,
every output word where it is 0 (a refused file's outputs are unspecified) -- and the same bits from two calls."""
import json

import numpy as np
import pytest
import torch

import result_parse_cases as rc
import result_parse_statement as rps
from gomatching_amd import ops, results, show

pytestmark = pytest.mark.gpu
NAMES = ("frame_rows", "ids", "pts", "has_seg", "t_off", "t_len", "poly_off", "poly_xy")


@pytest.fixture(scope="module")
def cases():
    """(name, bytes, the statement's status and arrays), the statement run once."""
    return [(n, d) + rps.parse(d) for n, d in rc.clean_cases() + rc.damaged_cases()]


def _device(data):
    return torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()


def test_kernels_equal_the_statement_on_every_case(cases):
    accepted = 0
    for name, data, st, a in cases:
        if not data:
            continue                                           # (no bytes: the wrapper's refusal, tested below)
        status, rows = ops.result_parse(_device(data))
        # the strings are the host's to decode: the kernels accept a file whose only fault is one of them
        assert status == (0 if st == rps.BAD_STRING else st), (name, status, st)
        if st:
            continue
        accepted += 1
        assert (rows["L"], rows["F"], rows["N"], rows["P"]) == (a["L"], a["F"], a["N"], a["P"]), name
        for k in NAMES:
            got = rows[k].cpu().numpy()
            assert got.dtype == a[k].dtype and got.shape == a[k].shape and np.array_equal(got, a[k]), (name, k)
    assert accepted >= len(rc.clean_cases())


def test_an_unaligned_file_reads_the_same():
    """The byte path of the line kernels: the file at an odd address."""
    name, data = rc.clean_cases()[1]
    st, a = rps.parse(data)
    buf = torch.zeros(len(data) + 3, dtype=torch.uint8, device="cuda")
    buf[3:] = _device(data)
    status, rows = ops.result_parse(buf[3:])
    assert status == 0
    for k in NAMES:
        assert np.array_equal(rows[k].cpu().numpy(), a[k]), k


def test_two_calls_give_the_same_bits():
    data = dict(rc.clean_cases())["long"]
    d = _device(data)
    s1, r1 = ops.result_parse(d)
    s2, r2 = ops.result_parse(d)
    assert s1 == s2 == 0
    for k in NAMES:
        assert torch.equal(r1[k], r2[k]), k


def test_parse_json_device_gives_the_annotation(cases):
    dev = torch.device("cuda", torch.cuda.current_device())
    for name, data, st, a in cases:
        parsed = results.parse_json_device(data, dev)
        assert parsed.status == st, (name, parsed.status, st)
        if st == 0:
            assert parsed.to_annotation() == show.rows_of_json(json.loads(data)), name
        else:
            assert parsed.causes(), name
