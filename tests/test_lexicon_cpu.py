"""CPU: the lexicon match (gomatching_amd/lexicon.py) -- `host_match` and the loaders against the plain-Python statement
(lexicon_statement.py), index and distance equal, family by family; the reference's own `find_match_word` and pair-list parsing
through tests/golden/lexicon_match.json (tools/gen_golden_lexicon.py); and the command on a hand-made result tree with
`--host-match`: expected files byte for byte, keep / drop, the directory form, the exits."""
import ctypes
import json
import os
import random

import numpy as np
import pytest

import lexicon_fixture as F
import lexicon_statement as S
from gomatching_amd import lexicon

A64, B64 = "A" * 64, "AB" * 32
ASTRAL = "\U0001F600"


def _both(queries, segments):
    args = F.csr(queries, segments)
    index, dist = lexicon.host_match(*args)
    assert index.dtype == np.int32 and dist.dtype == np.int32
    want = S.match_csr(*args)
    assert (index.tolist(), dist.tolist()) == want, (queries, segments)
    return want


def _one(q, words):
    (i,), (d,) = _both([(0, q)], [words])
    return i, d


def test_empty_query_empty_word_empty_segment():
    assert _one("", ["AB", "A", "", "B"]) == (2, 0)
    assert _one("", ["AB", "A", "B"]) == (1, 1)
    assert _one("ABC", ["", "ABCD"]) == (1, 1)
    assert _one("ABC", []) == (-1, 100)
    assert _one("", []) == (-1, 100)
    assert _both([], [["A"]]) == ([], [])


def test_equal_strings_and_lengths_1_and_64():
    assert _one("HELLO", ["WORLD", "HELLO"]) == (1, 0)
    assert _one("A", ["B", "A", "AA"]) == (1, 0)
    assert _one("A", ["B"]) == (0, 1)
    assert _one(A64, [B64, A64]) == (1, 0)
    assert _one(A64, [B64]) == (0, 32)
    assert _one("A", [B64, A64]) == (0, 63)
    assert _one(B64, ["A", "B"]) == (0, 63)
    assert _one(A64[:63], [A64, B64]) == (0, 1)


def test_length_65_is_refused(tmp_path):
    with pytest.raises(ValueError, match="at most 64"):
        lexicon.host_match(*F.csr([(0, "A" * 65)], [["A"]]))
    with pytest.raises(ValueError, match="at most 64"):
        lexicon.host_match(*F.csr([(0, "A")], [["A" * 65]]))
    path = str(tmp_path / "long.txt")
    with open(path, "w", encoding="utf-8") as f:
        f.write("fine\n\n" + "ß" * 33 + "\n")                        # 33 code points, 66 after upper-casing; line 3
    with pytest.raises(lexicon.LexiconError, match=r"long\.txt: line 3 "):
        lexicon.load_lexicon(path)
    lex = lexicon.Lexicon(["A"], {"A": "A"})
    with pytest.raises(lexicon.LexiconError, match="video V9, frame 4:"):
        lexicon.correct_annotation({"4": [F._row(0, 1, "ß" * 33)]}, lex, host=True, video="V9")
    assert lexicon.correct_annotation({"4": [F._row(0, 1, "ß" * 32)]}, lex, host=True) == {"4": [F._row(0, 1, "ß" * 32)]}


@pytest.mark.parametrize("pos", [0, 4, 8])
def test_distance_1_insert_delete_substitute_at_first_middle_last(pos):
    base = "ABCDEFGHA"
    far = ["HHHHHHHHH", "GGGG"]
    for q in (base[:pos] + "H" + base[pos:], base[:pos] + base[pos + 1:], base[:pos] + "D" * (base[pos] != "D") + base[pos + 1:]):
        assert _one(q, far + [base]) == (2, 1), q
    assert _one(base + "H", far + [base]) == (2, 1)                   # an insert behind the last position


def test_transposition_reads_2_and_aaaa_against_aaa():
    assert _one("AB", ["BA"]) == (0, 2)
    assert _one("ABCD", ["ABDC"]) == (0, 2)
    assert _one("AAAA", ["AAA"]) == (0, 1)
    assert _one("AAA", ["AAAA"]) == (0, 1)


def test_query_longer_than_every_word():
    assert _one("ABCDEFGH", ["AB", "H", "ABC", ""]) == (2, 5)


def test_ties_go_to_the_lower_index_and_the_last_word_can_win():
    assert _one("CAT", ["DOG", "CAT", "CAT"]) == (1, 0)               # a duplicated word
    assert _one("CAT", ["CAR", "BAT", "CAT" "S"]) == (0, 1)           # different words at the same distance
    assert _one("CAT", ["DOG", "BIRD", "FISH", "CAT"]) == (3, 0)      # the best word is the last of the segment


def test_segments_are_independent_and_indices_segment_relative():
    segs = [["DOG", "CAT"], [], ["BIRD", "FISH", "CAT"], ["CAT"]]
    want = _both([(2, "CAT"), (0, "CAT"), (1, "CAT"), (3, "CAT"), (2, "FIST")], segs)
    assert want == ([2, 1, -1, 0, 1], [0, 0, 100, 0, 1])


def test_random_pairs_over_a_small_alphabet():
    rng = random.Random(5)
    word = lambda lo, hi: "".join(rng.choice("ABCDEFGH") for _ in range(rng.randint(lo, hi)))
    segs = [[word(0, 12) for _ in range(rng.randint(0, 40))] for _ in range(5)]
    _both([(rng.randrange(5), word(0, 14)) for _ in range(60)], segs)


def test_upper_can_lengthen_and_code_points_beyond_ascii():
    assert S.norm("ß") == "SS" and len(S.norm("ŉ")) == 2
    words = ["straße", "ŉ", "中文字", "中文", ASTRAL + "a", "x" + ASTRAL]
    lex = lexicon.Lexicon(words, F.pairs_of(words))
    qs = ["STRASSE", "strase", "ŉ", "中文", "中字", ASTRAL + "A", ASTRAL, "X"]
    items = [(0, S.norm(q)) for q in qs]
    index, dist = lexicon.match_strings(items, [lex], host=True)
    want = [S.match(S.norm(q), [S.norm(w) for w in words]) for q in qs]
    assert list(zip(index.tolist(), dist.tolist())) == want
    assert want[0] == (0, 0) and want[2] == (1, 0) and want[3] == (3, 0) and want[5] == (4, 0) and want[6][1] == 1
    chars, off = lexicon.pack([S.norm(q) for q in qs])                # an astral code point is ONE entry
    assert chars.tolist() == [c for q in qs for c in F.codes(S.norm(q))] and off.tolist()[-1] == len(chars)
    assert int(chars.max()) == 0x1F600


def test_pair_list_later_line_wins_display_with_spaces_missing_word_refused(tmp_path):
    lex_path = F._write_lines(str(tmp_path / "lex.txt"), F.DIR_WORDS["clipB"])
    pair_path = F._write_lines(str(tmp_path / "pairs.txt"), F.DIR_PAIRS["clipB"])
    lex = lexicon.load_lexicon(lex_path, pair_path)
    assert lex.pairs == F.pairs_of(F.DIR_WORDS["clipB"], F.DIR_PAIRS["clipB"])
    assert [lex.display(i) for i in range(3)] == ["way out", "Straße", " New  York City"]
    short = F._write_lines(str(tmp_path / "short.txt"), F.DIR_PAIRS["clipB"][:2])
    with pytest.raises(lexicon.LexiconError, match=r"lex\.txt: line 3: the word 'newyork' has no entry"):
        lexicon.load_lexicon(lex_path, short)
    plain = lexicon.load_lexicon(F._write_lines(str(tmp_path / "dup.txt"), ["Hello", "", "hello", "HELLO "]))
    assert plain.words == ["Hello", "hello", "HELLO"] and plain.pairs == {"HELLO": "HELLO"}    # blank skipped, duplicates kept


def test_golden_reference_find_match_word(golden_dir, tmp_path):
    """The reference's own functions wrote the fixture: normalisation, scan order, tie rule, initial values, pair parsing and
    the acceptance bound are pinned; the `editdistance` library's arithmetic (plain Levenshtein) is not."""
    with open(os.path.join(golden_dir, "lexicon_match.json"), encoding="utf-8") as f:
        doc = json.load(f)
    assert len(doc["cases"]) >= 4
    for k, case in enumerate(doc["cases"]):
        lex_path = str(tmp_path / ("lex%d.txt" % k))
        with open(lex_path, "w", encoding="utf-8") as f:
            f.write(case["lexicon_text"])
        pair_path = None
        if case["pairs_text"] is not None:
            pair_path = str(tmp_path / ("pairs%d.txt" % k))
            with open(pair_path, "w", encoding="utf-8") as f:
                f.write(case["pairs_text"])
        lex = lexicon.load_lexicon(lex_path, pair_path)
        assert lex.words == case["lexicon"] and lex.pairs == case["pairs"]
        index, dist = lexicon.match_strings([(0, lexicon.norm(q)) for q in case["queries"]], [lex], host=True)
        for q, i, d, (word, ref_d, accepted) in zip(case["queries"], index.tolist(), dist.tolist(), case["expect"]):
            assert (lex.display(i) if i >= 0 else "", d) == (word, ref_d), (k, q)
            assert (d <= 1) == accepted, (k, q)                        # the default max_dist against the reference's `< 1.5`
            got = lexicon.correct_annotation({"1": [F._row(0, 1, q)]}, lex, unmatched="drop", host=True)["1"]
            assert [r[9] for r in got] == ([word] if accepted else []), (k, q)


def test_abi_rejects_bad_arguments_without_a_gpu():
    from gomatching_amd import lib
    L = lib.load()
    p = ctypes.c_void_p(0x1000)
    ok = [p, 8, p, p, 2, p, 8, p, 3, p, 1, 64, p, p, None]

    def call(**change):
        a = list(ok)
        for k, v in change.items():
            a[int(k[1:])] = v
        return L.gom_lexicon_match_u32(*a)
    for k in (0, 2, 3, 5, 7, 9, 12, 13):                               # each pointer of a non-empty array
        assert call(**{"a%d" % k: None}) == 1, k
    for k in (1, 4, 6, 8, 10, 11):                                     # each size negative
        assert call(**{"a%d" % k: -1}) == 1, k
    assert call(a11=65) == 1                                           # a length above the limit
    assert call(a10=0, a9=None) == 1                                   # queries without a segment
    assert call(a1=2 ** 31) == 1 and call(a6=2 ** 31) == 1
    assert L.gom_lexicon_match_u32(None, 0, None, None, 0, None, 0, None, 0, None, 0, 0, None, None, None) == 0   # S == 0
    assert L.gom_lexicon_match_u32(None, 0, None, None, 0, p, 8, p, 3, p, 1, 64, None, None, None) == 0


# ------------------------------------------------------------------------------------------------- the command
@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    return F.build(str(tmp_path_factory.mktemp("lexicon")))


def _run(capsys, argv):
    status = lexicon.main(argv)
    return status, capsys.readouterr().err


def _expected_tree(root, fixed):
    return F.tree_bytes(F.write_tree(root, fixed))


def test_command_host_match_writes_the_expected_files_and_leaves_res_alone(tree, tmp_path, capsys):
    before = F.tree_bytes(tree["res"], skip=("lexicon",))
    status, err = _run(capsys, ["--results", tree["res"], "--lexicon", tree["lexicon"], "--host-match"])
    assert status == 0, err
    vocab = {v: (F.SHARED_WORDS, None) for v in F.VIDEOS}
    fixed = F.expected(F.annotations(), vocab)
    got = F.tree_bytes(os.path.join(tree["res"], "lexicon"))           # OUT defaults to RES/lexicon
    assert got == _expected_tree(str(tmp_path / "want"), fixed)
    assert sorted(got) == sorted(os.path.join(d, n) for d, n in (
        [("jsons", v + ".json") for v in F.VIDEOS] + [("preds", "res_%s.%s" % (F.STEMS[v], e)) for v in F.VIDEOS for e in ("xml", "txt")]))
    assert F.tree_bytes(tree["res"], skip=("lexicon",)) == before
    # what the tree was made to show: 'hello' is the later line, so its display form wins; the vote of track 7 changes
    assert fixed["Video_35_2_3"]["1"][0][9] == "hello" and fixed["Video_35_2_3"]["4"][2][9] == "WORLD"
    assert fixed["Video_35_2_3"]["2"][2][9] == "straße" and fixed["clipB"]["2"][1][9] == "straße"
    assert fixed["Video_35_2_3"]["1"][2][9] == "zzzzzz" and fixed["clipB"]["2"][2][9] == "中文"          # kept
    assert b'"7","HELO"' in before[os.path.join("preds", "res_video_35.txt")]
    txt = got[os.path.join("preds", "res_video_35.txt")].decode()
    assert '"7","hello"\n' in txt and '"8","exit"\n' in txt


def test_keep_with_a_lexicon_that_matches_nothing_reproduces_the_input(tree, tmp_path, capsys):
    out = str(tmp_path / "out")
    status, err = _run(capsys, ["--results", tree["res"], "--lexicon", tree["nothing"], "--output", out, "--host-match"])
    assert status == 0, err
    assert F.tree_bytes(out) == F.tree_bytes(tree["res"], skip=("lexicon",))


def test_drop_removes_exactly_the_unmatched_rows(tree, tmp_path, capsys):
    out = str(tmp_path / "out")
    status, err = _run(capsys, ["--results", tree["res"], "--lexicon", tree["lexicon"], "--unmatched", "drop", "--max-dist", "0",
                                "--output", out, "--host-match"])
    assert status == 0, err
    vocab = {v: (F.SHARED_WORDS, None) for v in F.VIDEOS}
    fixed = F.expected(F.annotations(), vocab, max_dist=0, unmatched="drop")
    assert F.tree_bytes(out) == _expected_tree(str(tmp_path / "want"), fixed)
    kept = {v: {fr: [r[8] for r in rows] for fr, rows in a.items()} for v, a in fixed.items()}
    assert kept == {"Video_35_2_3": {"1": [8], "2": [11], "3": [], "4": [7, 9]}, "clipB": {"1": [2], "2": [2]}}


def test_directory_form_picks_each_videos_own_file(tree, tmp_path, capsys):
    out = str(tmp_path / "out")
    status, err = _run(capsys, ["--results", tree["res"], "--lexicon", tree["lexdir"], "--output", out, "--host-match"])
    assert status == 0, err
    vocab = {v: (F.DIR_WORDS[v], F.DIR_PAIRS.get(v)) for v in F.VIDEOS}
    fixed = F.expected(F.annotations(), vocab)
    assert F.tree_bytes(out) == _expected_tree(str(tmp_path / "want"), fixed)
    assert [r[9] for r in fixed["Video_35_2_3"]["1"]] == ["HELP", "EXIT", "zzzzzz"]                # 'exit' is clipB's word only
    assert [r[9] for r in fixed["clipB"]["1"]] == [" New  York City", "Straße", "Hallo"]


def test_status_1_without_a_gpu_and_without_the_flag(tree, tmp_path, capsys, monkeypatch):
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    out = str(tmp_path / "out")
    status, err = _run(capsys, ["--results", tree["res"], "--lexicon", tree["lexicon"], "--output", out])
    assert status == 1 and "--host-match" in err and not os.path.exists(out)


def test_status_2_exits(tree, tmp_path, capsys):
    out = str(tmp_path / "out")
    base = ["--output", out, "--host-match"]
    status, err = _run(capsys, ["--results", str(tmp_path / "absent"), "--lexicon", tree["lexicon"]] + base)
    assert status == 2 and "absent" in err
    status, err = _run(capsys, ["--results", tree["res"], "--lexicon", str(tmp_path / "absent.txt")] + base)
    assert status == 2 and "absent.txt" in err
    # a video without its lexicon in the directory form
    lexdir = str(tmp_path / "strong")
    os.makedirs(lexdir)
    F._write_lines(os.path.join(lexdir, "clipB.txt"), ["exit"])
    status, err = _run(capsys, ["--results", tree["res"], "--lexicon", lexdir] + base)
    assert status == 2 and "Video_35_2_3" in err
    # an unreadable json, then a video whose XML is under neither stem
    res = F.write_tree(str(tmp_path / "res"), F.annotations())
    os.remove(os.path.join(res, "preds", "res_clipB.xml"))
    status, err = _run(capsys, ["--results", res, "--lexicon", tree["lexicon"]] + base)
    assert status == 2 and "clipB" in err
    res2 = F.write_tree(str(tmp_path / "res2"), F.annotations())
    with open(os.path.join(res2, "jsons", "clipB.json"), "w") as f:
        f.write("{\"1\": [{\"points\": [1, 2]}]")
    status, err = _run(capsys, ["--results", res2, "--lexicon", tree["lexicon"]] + base)
    assert status == 2 and "clipB.json" in err
    assert not os.path.exists(out)


def test_eval_refuses_lexicon_arguments_it_cannot_use_before_building_anything(tmp_path, capsys):
    from gomatching_amd import eval as E
    data = tmp_path / "frames"
    data.mkdir()
    base = ["--builtin", "icdar15", "--input", str(data), "--output", str(tmp_path / "out")]
    assert E.main(base + ["--lexicon", str(tmp_path / "absent.txt")]) == 2
    assert "absent.txt" in capsys.readouterr().err
    vocab = F._write_lines(str(tmp_path / "vocab.txt"), ["word"])
    assert E.main(base + ["--lexicon", vocab, "--lexicon-pairs", str(tmp_path / "absent.pairs")]) == 2
    assert E.main(base + ["--lexicon", vocab, "--lexicon-max-dist", "-1"]) == 2
    assert E.main(base + ["--lexicon-unmatched", "drop"]) == 2                                     # goes with --lexicon
    assert "go with --lexicon" in capsys.readouterr().err
    assert not os.path.exists(str(tmp_path / "out"))
    args = E.get_parser(drawing=True).parse_args(base)                                              # the defaults: nothing is asked for
    assert (args.lexicon, args.lexicon_pairs, args.lexicon_max_dist, args.lexicon_unmatched) == (None, None, 1, "keep")
