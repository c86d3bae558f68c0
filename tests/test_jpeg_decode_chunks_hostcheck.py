"""CPU: tools/jpeg_decode_chunks_hostcheck.cpp -- csrc/jpeg_decode_chunks.h, the chunked walk the kernel runs, compiled with the
host compiler under AddressSanitizer and UndefinedBehaviorSanitizer as a stand-alone program, at chunk sizes 16, 64 and 256, over
the clean families, the damaged streams, a mixed call and two larger files (the noise one is two spans of 256 chunks).  No
sanitizer report; the status words and coefficients (by checksum) of `jpeg.decode_host`; every segment of a clean file finished
by the chunk walk, the failing segment of every damaged stream left to the serial walk; one checksum at all three sizes."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import jpeg_decode_families as fam

from gomatching_amd import jpeg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHUNKS = (16, 64, 256)


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


def _failing_segments(files):
    """-> per segment of the call: True where the serial walk's status word is not 0 (jpeg.decode_host's walk, per segment)."""
    p = jpeg.plan(files)
    geo = jpeg.geometry(p.H, p.W, p.ncomp, p.hs, p.vs)
    out = []
    for f in range(p.F):
        coef = np.zeros((geo[4], 64), dtype=np.int16)
        for s in range(p.seg_off[f], p.seg_off[f + 1]):
            out.append(jpeg._walk_segment(p.data, p.desc[s], p.sets[p.frame_set[f]], geo, p.ncomp, p.hs, p.vs, coef) != 0)
    return out


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler on the path")
    exe = str(tmp_path_factory.mktemp("chunks_hostcheck") / "jpeg_decode_chunks_hostcheck")
    # the sanitizer runtimes linked into the program (clang's default; g++ is told to): it runs as it is, wherever it is started
    static = ["-static-libasan", "-static-libubsan"] if os.path.basename(cxx).startswith("g++") else []
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all"] + static + [os.path.join(ROOT, "tools", "jpeg_decode_chunks_hostcheck.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def test_chunked_walk_under_sanitizers(program, tmp_path):
    clean = [files for _, files in fam.families()]
    clean.append((fam.pillow_file(fam.content("noise", 320, 240, 21), 2, 95),))
    clean.append((fam.pillow_file(fam.content("gradient", 640, 360, 21), 2, 95),))
    damaged = [(data,) for _, data in fam.damaged()]
    mixed = (dict(fam.families())["size-33x47-2"][0], dict(fam.damaged())["cut-50%"])
    calls = clean + damaged + [mixed]
    assert len(jpeg.plan(clean[-2]).data) == 89997
    dump = str(tmp_path / "calls.bin")
    _dump(dump, calls)
    want = []
    for files in calls:
        _, status, coefs = jpeg.decode_host(files, return_status=True, return_coefficients=True)
        want.append((" ".join(str(int(s)) for s in status), _checksum(coefs), _failing_segments(files)))
    assert all(not any(w[2]) for w in want[:len(clean)]) and all(any(w[2]) for w in want[len(clean):])
    sums = {}
    for chunk in CHUNKS:
        r = subprocess.run([program, dump, str(chunk)], capture_output=True, text=True)
        assert r.returncode == 0 and r.stderr == "", (chunk, r.returncode, r.stderr[-2000:])
        lines = r.stdout.splitlines()
        assert len(lines) == len(calls)
        for i, (line, (status, checksum, failing)) in enumerate(zip(lines, want)):
            head, _, tail = line.partition(" routes ")
            assert head == "call %d: status %s checksum %d" % (i, status, checksum), (chunk, i, line)
            routes, _, passes = tail.partition(" passes ")
            routes = [int(r) for r in routes.split()]
            assert len(routes) == len(failing) and 0 <= int(passes) <= 256
            if i < len(clean):
                assert routes == [0] * len(routes), (chunk, i, line)                # a condition: the settling is exact
            for r, bad in zip(routes, failing):
                assert r == 1 or not bad, (chunk, i, line)                          # a failing segment is the serial walk's
        sums[chunk] = [line.partition(" routes ")[0] for line in lines]
    assert sums[16] == sums[64] == sums[256]
