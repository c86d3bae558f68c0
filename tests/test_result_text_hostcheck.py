"""CPU: tools/result_text_hostcheck.cpp -- csrc/result_text_core.h, the functions the result text kernels count and emit with,
compiled with the host compiler under AddressSanitizer and UndefinedBehaviorSanitizer as a stand-alone program, over the GPU
test's case list.  No sanitizer report, the bytes of the statement, and with buffers one byte too short a refusal by the bounds
check (not a report).  Nothing here is loaded into Python."""
import os
import shutil
import subprocess

import pytest

import result_text_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler on the path")
    tmp = tmp_path_factory.mktemp("result_text_hostcheck")
    exe = str(tmp / "result_text_hostcheck")
    # the sanitizer runtimes linked into the program (clang's default; g++ is told to): it runs as it is, wherever it is started
    static = ["-static-libasan", "-static-libubsan"] if os.path.basename(cxx).startswith("g++") else []
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all"] + static + [os.path.join(ROOT, "tools", "result_text_hostcheck.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    cases = rc.cases()
    dump = str(tmp / "calls.bin")
    rc.dump(dump, cases)
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
        js, xs = rc.statement_text(case)
        assert line == "call %d: json %d xml %d status 0" % (i, len(js), len(xs)), (case.name, line)
        assert (out / ("call_%d.json" % i)).read_bytes() == js, case.name
        assert (out / ("call_%d.xml" % i)).read_bytes() == xs, case.name


def test_a_buffer_one_byte_short_is_refused_not_overrun(program):
    exe, dump, cases, tmp = program
    out = tmp / "short"
    out.mkdir()
    r = subprocess.run([exe, dump, str(out), "1"], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr[-2000:])
    lines = r.stdout.splitlines()
    assert len(lines) == len(cases)
    for i, (case, line) in enumerate(zip(cases, lines)):
        js, xs = rc.statement_text(case)
        assert line == "call %d: refused json %d > %d xml %d > %d" % (i, len(js), len(js) - 1, len(xs), len(xs) - 1), (case.name, line)
    assert os.listdir(str(out)) == []
