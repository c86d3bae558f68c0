"""GPU: `gom_lexicon_match_u32` (csrc/lexicon.hip) through `ops.lexicon_match` against the plain-Python statement
(lexicon_statement.py), every int32 word equal, at the shapes where the kernel can go wrong: the lane, wave, workgroup and
stride boundaries of the segment size (256 threads stride over the words), lengths 0 / 1 / 63 / 64 and the 32 | 33 switch
between the 32- and 64-bit recurrence, code points on either side of the 256-entry mask table, the best word planted at the
boundaries and planted TWICE (the reduction's tie-break), several segments in one call.  Then the command as a fresh child
process on the CPU test's tree, device output against `--host-match` output byte for byte."""
import functools
import os
import random
import subprocess
import sys

import numpy as np
import pytest
import torch

import lexicon_fixture as F
import lexicon_statement as S
from gomatching_amd import lexicon, lib, ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALPHABET = "ABCDEFGH"


def _device(args, **kw):
    index, dist = ops.lexicon_match(*[torch.tensor(a, dtype=torch.int32, device=DEV) for a in args], **kw)
    assert index.dtype == torch.int32 and dist.dtype == torch.int32
    return index.cpu().tolist(), dist.cpu().tolist()


def _word(rng, lo, hi, alphabet=ALPHABET):
    return "".join(rng.choice(alphabet) for _ in range(rng.randint(lo, hi)))


@functools.lru_cache(maxsize=None)
def _far_words(q, n=1025):
    """n seeded words that are all more than 2 edits away from q (made once per query string)."""
    rng = random.Random(len(q))
    words = []
    while len(words) < n:
        w = _word(rng, 8, 13)
        if S.levenshtein(q, w) > 2:
            words.append(w)
    return tuple(words)


def _check(queries, segments):
    args = F.csr(queries, segments)
    got, want = _device(args), S.match_csr(*args)
    assert got == (want[0], want[1])
    return want


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257, 1025])
def test_segment_sizes_at_lane_wave_workgroup_and_stride_edges(n):
    rng = random.Random(100 + n)
    words = [_word(rng, 3, 9) for _ in range(n)]
    queries = [(0, _word(rng, 2, 10)) for _ in range(6)] + ([(0, words[-1])] if n else []) + [(0, "")]
    index, dist = _check(queries, [words])
    if n == 0:
        assert set(index) == {-1} and set(dist) == {100}


@pytest.mark.parametrize("lq", [0, 1, 31, 32, 33, 63, 64])
def test_query_and_word_lengths(lq):
    rng = random.Random(200 + lq)
    words = []
    for lw in (0, 1, 31, 32, 33, 63, 64):
        words += [_word(rng, lw, lw, "AB") for _ in range(3)]
    words += [_word(rng, 0, 64, "AB") for _ in range(45 - len(words))]
    rng.shuffle(words)
    q = _word(rng, lq, lq, "AB")
    near = [(0, w[:lq].ljust(lq, "A")) for w in words[:2]]            # queries close to a word, so small distances occur too
    _check([(0, q), (0, q[::-1])] + near, [words])


@pytest.mark.parametrize("at", [0, 63, 64, 255, 256, 1024])
@pytest.mark.parametrize("d", [0, 1])
def test_unique_best_word_planted_at_a_boundary(at, d):
    q = "ABCDEFGHABCD"
    words = list(_far_words(q))
    words[at] = q if d == 0 else q[:5] + q[6:]
    (index,), (dist,) = _check([(0, q)], [words])
    assert (index, dist) == (at, d)


@pytest.mark.parametrize("first,second", [(3, 40), (3, 70), (3, 200), (3, 259), (3, 300), (255, 256), (63, 64), (700, 1023)])
def test_the_same_best_word_twice_returns_the_lower_index(first, second):
    """Two copies in different lanes of a wave, in different waves, in different stride iterations of the same lane (3, 259)
    and of different lanes: the reduction must break the tie towards the lower index."""
    q = "ABCDEFGHABCD"
    words = _far_words(q)
    for d, word in ((0, q), (1, q[:-1] + "A"), (2, "HG" + q[2:])):
        ws = list(words)
        ws[first] = ws[second] = word
        (index,), (dist,) = _check([(0, q)], [ws])
        assert (index, dist) == (first, d)


def test_four_segments_in_one_call_indices_segment_relative():
    rng = random.Random(5)
    segments = [[], [_word(rng, 4, 8)], [_word(rng, 4, 8) for _ in range(65)], [_word(rng, 3, 9) for _ in range(1025)]]
    queries = []
    for g in (3, 0, 2, 1, 3, 2, 0, 1, 3, 3, 2):
        queries.append((g, _word(rng, 3, 9)))
    queries += [(3, segments[3][1024]), (2, segments[2][64]), (1, segments[1][0]), (3, segments[2][0])]
    index, dist = _check(queries, segments)
    assert index[1] == -1 and dist[1] == 100 and (index[11], dist[11]) == (segments[3].index(segments[3][1024]), 0)
    assert (index[12], dist[12]) == (segments[2].index(segments[2][64]), 0) and (index[13], dist[13]) == (0, 0)


def test_code_points_on_both_sides_of_the_mask_table():
    rng = random.Random(6)
    alphabet = ["A", "\xff", "Ā", "中", "文", "\U0001F600"]             # 255 | 256, BMP, astral
    words = [[ord(c) for c in _word(rng, 0, 10, alphabet)] for _ in range(400)]
    queries = [(0, [ord(c) for c in _word(rng, n, n, alphabet)]) for n in (0, 1, 5, 9, 33, 40)] + [(0, words[399]), (0, words[17][:-1])]
    _check(queries, [words])


def test_s_0_returns_empty_tensors_and_invalid_arguments_are_refused():
    args = F.csr([], [["AB", "CD"]])
    assert _device(args) == ([], [])
    assert _device(F.csr([], [])) == ([], [])
    with pytest.raises(ValueError, match="at most 64"):
        _device(F.csr([(0, "A" * 65)], [["A"]]))
    with pytest.raises(ValueError, match="at most 64"):
        _device(F.csr([(0, "A")], [["A"]]), max_len=65)
    with pytest.raises(ValueError, match="without a lexicon segment"):
        _device(([65], [0, 1], [0], [], [0], [0]))
    with pytest.raises(ValueError):
        ops.lexicon_match(*[torch.zeros(2, dtype=torch.int32) for _ in range(6)])                  # not on the GPU
    L = lib.load()
    t = torch.zeros(8, dtype=torch.int32, device=DEV)
    p = ops._p(t)
    assert L.gom_lexicon_match_u32(p, 1, p, p, 1, p, 1, p, 1, p, 1, 65, p, p, None) == 1           # no launch: the error code
    assert L.gom_lexicon_match_u32(p, 1, p, None, 1, p, 1, p, 1, p, 1, 64, p, p, None) == 1
    assert L.gom_lexicon_match_u32(p, 1, p, p, -1, p, 1, p, 1, p, 1, 64, p, p, None) == 1
    torch.cuda.synchronize()


def test_host_and_device_paths_agree_through_the_library():
    rng = random.Random(7)
    lexicons = [lexicon.Lexicon(ws, F.pairs_of(ws)) for ws in ([_word(rng, 2, 9) for _ in range(300)], [_word(rng, 2, 9) for _ in range(40)])]
    items = [(rng.randrange(2), _word(rng, 0, 10)) for _ in range(50)]
    h, d = lexicon.match_strings(items, lexicons, host=True), lexicon.match_strings(items, lexicons)
    assert np.array_equal(h[0], d[0]) and np.array_equal(h[1], d[1]) and d[0].dtype == np.int32


@pytest.mark.parametrize("form", ["file", "directory", "drop"])
def test_command_device_and_host_write_the_same_trees(tmp_path, form):
    tree = F.build(str(tmp_path / "tree"))
    extra = {"file": ["--lexicon", tree["lexicon"]], "directory": ["--lexicon", tree["lexdir"]],
             "drop": ["--lexicon", tree["lexicon"], "--unmatched", "drop", "--max-dist", "2"]}[form]
    outs = []
    for flag in ([], ["--host-match"]):
        out = str(tmp_path / ("out" + str(len(flag))))
        r = subprocess.run([sys.executable, "-m", "gomatching_amd.lexicon", "--results", tree["res"], "--output", out] + extra + flag,
                           cwd=ROOT, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        outs.append(F.tree_bytes(out))
    assert outs[0] == outs[1] and len(outs[0]) == 6


def test_eval_lexicon_flag_writes_what_the_command_writes_resumed_runs_included(tmp_path):
    """`eval --lexicon` on one small synthetic video: OUT/lexicon is the tree the stand-alone command's numpy path writes from
    OUT, the three files of OUT itself are there as always; a second, resumed run (nothing left to spot) with other
    lexicon options rewrites OUT/lexicon from the videos already written."""
    from PIL import Image
    from gomatching_amd.config import setup_cfg
    from gomatching_amd.synth import make_clip
    from gomatching_amd.weights import synth_state_dict
    opts = ["MODEL.TRANSFORMER.NUM_QUERIES", "12", "INPUT.MIN_SIZE_TEST", "128", "INPUT.MAX_SIZE_TEST", "256", "MODEL.DEVICE", "cuda:0"]
    data = tmp_path / "ICDAR15_frames"
    (data / "Video_5_1_2").mkdir(parents=True)
    for i, rgb in enumerate(make_clip(7, 72, 128, clip_id=3)):
        Image.fromarray(np.ascontiguousarray(rgb)).save(str(data / "Video_5_1_2" / ("%d.png" % (i + 1))))
    weights = str(tmp_path / "weights.pth")
    cfg = setup_cfg(builtin="icdar15", opts=opts + ["MODEL.WEIGHTS", weights])
    torch.save(synth_state_dict(cfg, seed=7, cls_bias={"detection_transformer.ctrl_point_class.0.bias": 0.5}), weights)
    vocab = F._write_lines(str(tmp_path / "vocab.txt"), ["a", "Bc", "DEF", "ghij", "klmnop", "0", "12"])
    out = str(tmp_path / "out")
    base = [sys.executable, "-m", "gomatching_amd.eval", "--builtin", "icdar15", "--input", str(data), "--output", out, "--lexicon", vocab]
    tail = ["--opts"] + opts + ["MODEL.WEIGHTS", weights]
    for extra, same in ((["--lexicon-max-dist", "64"], ["--max-dist", "64"]),
                        (["--lexicon-max-dist", "2", "--lexicon-unmatched", "drop"], ["--max-dist", "2", "--unmatched", "drop"])):
        r = subprocess.run(base + extra + tail, cwd=ROOT, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, "exit status %d\n%s\n%s" % (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
        assert "lexicon: " in r.stdout
        assert {"jsons/Video_5_1_2.json", "preds/res_video_5.txt", "preds/res_video_5.xml"} <= set(F.tree_bytes(out, skip=("lexicon",)))
        want = str(tmp_path / ("want%d" % len(extra)))
        assert lexicon.main(["--results", out, "--lexicon", vocab, "--output", want, "--host-match"] + same) == 0
        got = F.tree_bytes(os.path.join(out, "lexicon"))
        assert got == F.tree_bytes(want) and sorted(got) == ["jsons/Video_5_1_2.json", "preds/res_video_5.txt", "preds/res_video_5.xml"]
    rows = [r for rows in lexicon.read_annotation(os.path.join(out, "jsons", "Video_5_1_2.json")).values() for r in rows]
    assert rows, "the synthetic video must have rows for the flag to act on"
