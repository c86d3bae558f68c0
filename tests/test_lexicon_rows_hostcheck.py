"""CPU: tools/lexicon_rows_hostcheck.cpp -- csrc/lexicon_rows_core.h and the override forms of result_text_core.h and
track_vote_core.h, the functions the kernels of the lexicon correction of rows count and emit with, compiled with the host compiler
under AddressSanitizer and UndefinedBehaviorSanitizer as a stand-alone program, over the GPU test's case list.  No sanitizer
report, the queries, bytes and records of the statement, and with buffers one element too short a refusal by the bounds check (not
a report).  Nothing here is loaded into Python."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import lexicon_rows_cases as lc
import lexicon_rows_statement as lrs
import track_vote_statement as tvs
from gomatching_amd import results

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler on the path")
    tmp = tmp_path_factory.mktemp("lexicon_rows_hostcheck")
    exe = str(tmp / "lexicon_rows_hostcheck")
    # the sanitizer runtimes linked into the program (clang's default; g++ is told to): it runs as it is, wherever it is started
    static = ["-static-libasan", "-static-libubsan"] if os.path.basename(cxx).startswith("g++") else []
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all"] + static + [os.path.join(ROOT, "tools", "lexicon_rows_hostcheck.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    cases = lc.cases()
    dump = str(tmp / "calls.bin")
    lc.dump(dump, cases)
    return exe, dump, cases, tmp


def _queries(case):
    c = case.case
    tab = lc.norm_tab(c.decoder).tolist()
    return [q for r in range(len(c.keep)) for q in lrs.query(c.words[r], c.keep[r], tab)]


def test_shared_core_under_sanitizers(program):
    exe, dump, cases, tmp = program
    out = tmp / "exact"
    out.mkdir()
    r = subprocess.run([exe, dump, str(out)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr[-2000:])
    lines = r.stdout.splitlines()
    assert len(lines) == len(cases)
    for i, (case, line) in enumerate(zip(cases, lines)):
        js, xs, _, (ov, keep_out, _) = lc.statement_bytes(case)
        q = _queries(case)
        assert line == "call %d: q %d json %d xml %d" % (i, len(q), len(js), len(xs)), (case.name, line)
        assert np.frombuffer((out / ("call_%d.q" % i)).read_bytes(), dtype="<u4").tolist() == q, case.name
        assert (out / ("call_%d.json" % i)).read_bytes() == js, case.name
        assert (out / ("call_%d.xml" % i)).read_bytes() == xs, case.name
        rec = np.frombuffer((out / ("call_%d.rec" % i)).read_bytes(), dtype="<i4").reshape(-1, 28)
        table, forms = results.txt_table(case.case.decoder), lc.forms(case.lex)[2]
        for k in range(rec.shape[0]):
            if not keep_out[k]:
                assert rec[k, 2] == -1 and not rec[k, 3:].any(), (case.name, k)
                continue
            text = forms[ov[k]] if ov[k] >= 0 else tvs.row_text(case.case.words[k], table)
            assert rec[k, 2] == len(text) and rec[k, 3:].tobytes() == text + b"\0" * (100 - len(text)), (case.name, k)
            assert tvs.track_id(case.case.words[k]) == int(rec[k, :2].copy().view("<i8")[0])


def test_buffers_one_element_short_are_refused_not_overrun(program):
    exe, dump, cases, tmp = program
    out = tmp / "short"
    out.mkdir()
    r = subprocess.run([exe, dump, str(out), "1"], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr[-2000:])
    lines = r.stdout.splitlines()
    assert len(lines) == len(cases)
    for i, (case, line) in enumerate(zip(cases, lines)):
        js, xs, _, _ = lc.statement_bytes(case)
        q = len(_queries(case))
        assert line == "call %d: refused q %d > %d json %d > %d xml %d > %d" % (i, q, max(q - 1, 0), len(js), len(js) - 1, len(xs),
                                                                                  len(xs) - 1), (case.name, line)
    assert os.listdir(str(out)) == []
