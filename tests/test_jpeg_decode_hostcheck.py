"""CPU: tools/jpeg_decode_hostcheck.cpp -- csrc/jpeg_decode_core.h, the walk the kernel runs, compiled with the host compiler
under AddressSanitizer and UndefinedBehaviorSanitizer as a stand-alone program, over the clean families and the damaged
streams.  No sanitizer report, the status words of `jpeg.decode_host`, and its coefficients (by checksum)."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import jpeg_decode_families as fam

from gomatching_amd import jpeg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _checksum(coefs):
    h = 1469598103934665603
    for v in coefs.reshape(-1).astype(np.uint16).tolist():
        h = ((h ^ v) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


def _dump(path, calls):
    with open(path, "wb") as f:
        f.write(struct.pack("<q", len(calls)))
        for files in calls:
            p = jpeg.plan(files)
            f.write(struct.pack("<9q", p.F, p.H, p.W, p.ncomp, p.hs, p.vs, len(p.data), p.desc.shape[0], p.sets.shape[0]))
            f.write(p.data.tobytes())
            f.write(np.ascontiguousarray(p.desc, dtype="<i8").tobytes())
            f.write(np.ascontiguousarray(p.seg_off, dtype="<i4").tobytes())
            f.write(np.ascontiguousarray(p.sets, dtype="<i4").tobytes())


def test_shared_walk_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler on the path")
    exe = str(tmp_path / "jpeg_decode_hostcheck")
    # the sanitizer runtimes linked into the program (clang's default; g++ is told to): it runs as it is, wherever it is started
    static = ["-static-libasan", "-static-libubsan"] if os.path.basename(cxx).startswith("g++") else []
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all"] + static + [os.path.join(ROOT, "tools", "jpeg_decode_hostcheck.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    calls = [files for _, files in fam.families()] + [(data,) for _, data in fam.damaged()]
    calls.append((dict(fam.families())["size-33x47-2"][0], dict(fam.damaged())["cut-50%"]))
    dump = str(tmp_path / "calls.bin")
    _dump(dump, calls)
    r = subprocess.run([exe, dump], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr[-2000:])
    lines = r.stdout.splitlines()
    assert len(lines) == len(calls)
    n_damaged = 0
    for i, (files, line) in enumerate(zip(calls, lines)):
        _, status, coefs = jpeg.decode_host(files, return_status=True, return_coefficients=True)
        assert line == "call %d: status %s checksum %d" % (i, " ".join(str(int(s)) for s in status), _checksum(coefs)), (i, line)
        n_damaged += int(status[0] != 0)
    assert n_damaged == len(fam.damaged())
