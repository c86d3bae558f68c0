"""CPU: tools/result_parse_hostcheck.cpp -- csrc/result_parse_core.h, the per-line functions the parse kernels call, compiled
with the host compiler under AddressSanitizer and UndefinedBehaviorSanitizer as a stand-alone program, over every clean and
damaged case.  No sanitizer report, the status and the arrays of the statement, and with every output one element too short a
refusal by the bounds check (not a report).  Nothing here is loaded into Python."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import result_parse_cases as rc
import result_parse_statement as rps
from gomatching_amd.lib import CONSTANTS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler on the path")
    tmp = tmp_path_factory.mktemp("result_parse_hostcheck")
    exe = str(tmp / "result_parse_hostcheck")
    # the sanitizer runtimes linked into the program (clang's default; g++ is told to): it runs as it is, wherever it is started
    static = ["-static-libasan", "-static-libubsan"] if os.path.basename(cxx).startswith("g++") else []
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all"] + static + [os.path.join(ROOT, "tools", "result_parse_hostcheck.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    cases = rc.clean_cases() + rc.damaged_cases()
    dump = str(tmp / "cases.bin")
    rc.dump(dump, cases)
    return exe, dump, cases, [rps.parse(d) for _, d in cases], tmp


def _arrays(blob, F, N, P):
    out, at = {}, 0
    for name, dtype, shape in (("frame_rows", "<i4", (F + 1,)), ("ids", "<i8", (N,)), ("pts", "<i4", (N, 8)), ("has_seg", "u1", (N,)),
                               ("t_off", "<i8", (N,)), ("t_len", "<i4", (N,)), ("poly_off", "<i4", (N + 1,)),
                               ("poly_xy", "<i4", (P, 2))):
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        out[name] = np.frombuffer(blob[at:at + n], dtype=dtype).reshape(shape)
        at += n
    assert at == len(blob)
    return out


def test_shared_core_under_sanitizers(program):
    exe, dump, cases, stated, tmp = program
    out = tmp / "exact"
    out.mkdir()
    r = subprocess.run([exe, dump, str(out)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr[-2000:])
    lines = r.stdout.splitlines()
    assert len(lines) == len(cases)
    for i, ((name, data), (st, a), line) in enumerate(zip(cases, stated, lines)):
        words = line.split()
        assert words[:2] == ["case", "%d:" % i], line
        status, L, F, N, P = (int(words[k]) for k in (3, 5, 7, 9, 11))
        # the strings are the host's to decode: the core accepts a file whose only fault is one of them
        assert status == (0 if st == rps.BAD_STRING else st), (name, line)
        if st == 0:
            assert (L, F, N, P) == (a["L"], a["F"], a["N"], a["P"]), (name, line)
            if L > 1:
                got = _arrays((out / ("case_%d.bin" % i)).read_bytes(), F, N, P)
                for k, v in got.items():
                    assert np.array_equal(v, a[k]), (name, k)


def test_outputs_one_element_short_are_refused_not_overrun(program):
    exe, dump, cases, stated, tmp = program
    out = tmp / "short"
    out.mkdir()
    r = subprocess.run([exe, dump, str(out), "1"], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr[-2000:])
    lines = r.stdout.splitlines()
    assert len(lines) == len(cases)
    for (name, data), (st, a), line in zip(cases, stated, lines):
        status = int(line.split()[3])
        if st == 0 and a["N"] > 0:
            assert status == CONSTANTS["GOM_RP_BAD_CAP"], (name, line)
        elif st == 0:
            assert status == 0, (name, line)
    rowless = ["case_%d.bin" % i for i, (st, a) in enumerate(stated) if st == 0 and a["N"] == 0 and a["L"] > 1]
    assert sorted(os.listdir(str(out))) == sorted(rowless)   # nothing else was complete enough to write
