"""CPU: tools/track_vote_hostcheck.cpp -- csrc/track_vote_core.h, the functions the track vote kernels build records, compare
them and format lines with, compiled with the host compiler under AddressSanitizer and UndefinedBehaviorSanitizer as a
stand-alone program, over the shared case list.  No sanitizer report, the bytes of the statement, and with a buffer one byte
too short a refusal by the bounds check (not a report).  Nothing here is loaded into Python."""
import os
import shutil
import subprocess

import pytest

import track_vote_cases as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler on the path")
    tmp = tmp_path_factory.mktemp("track_vote_hostcheck")
    exe = str(tmp / "track_vote_hostcheck")
    # the sanitizer runtimes linked into the program (clang's default; g++ is told to): it runs as it is, wherever it is started
    static = ["-static-libasan", "-static-libubsan"] if os.path.basename(cxx).startswith("g++") else []
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all"] + static + [os.path.join(ROOT, "tools", "track_vote_hostcheck.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    cases = tc.cases()
    dump = str(tmp / "videos.bin")
    tc.dump(dump, cases)
    return exe, dump, cases, tmp


def test_shared_core_under_sanitizers(program):
    exe, dump, cases, tmp = program
    out = tmp / "exact"
    out.mkdir()
    r = subprocess.run([exe, dump, str(out)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr[-2000:])
    lines = r.stdout.splitlines()
    assert len(lines) == len(cases)
    for i, (case, line) in enumerate(zip(cases, lines)):
        text, winners = case.statement()
        assert line == "video %d: bytes %d tracks %d status 0" % (i, len(text), len(winners)), (case.name, line)
        assert (out / ("video_%d.txt" % i)).read_bytes() == text, case.name


def test_a_buffer_one_byte_short_is_refused_not_overrun(program):
    exe, dump, cases, tmp = program
    out = tmp / "short"
    out.mkdir()
    r = subprocess.run([exe, dump, str(out), "1"], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr[-2000:])
    lines = r.stdout.splitlines()
    assert len(lines) == len(cases)
    written = []
    for i, (case, line) in enumerate(zip(cases, lines)):
        text, _ = case.statement()
        if text:
            assert line == "video %d: refused %d > %d" % (i, len(text), len(text) - 1), (case.name, line)
        else:                                                    # a video without lines needs no byte: nothing to refuse
            assert line == "video %d: bytes 0 tracks 0 status 0" % i, (case.name, line)
            written.append("video_%d.txt" % i)
    assert sorted(os.listdir(str(out))) == sorted(written) and len(written) == 2
