"""Writes tests/golden/lexicon_match.json: what the REFERENCE's lexicon rule gives for small vocabularies and queries.  CPU
only; needs the reference tree (oracle/ref_shim.py names its place).

The rule sits inside `TextEvaluator.sort_detection` (third_party/adet/evaluation/text_evaluation_all.py), which cannot be
imported (Detectron2, shapely, editdistance) and reads fixed dataset paths, so the pieces that hold it are cut out of the
reference file's TEXT at generation time, compiled and executed unmodified -- nothing of that text is written here:

  * `find_match_word`, the nested function (normalisation, scan order, strict `<`, initial values, the display lookup);
  * the "ic15" generic block: pair-list parsing, then the lexicon's lines;
  * the "ctw1500" block: the lexicon's lines with `pairs[line.upper()] = line`;
  * the acceptance condition of the `if match_dist<...:` line, evaluated as an expression.

Stand-ins: `open` hands the block the case's text, and `editdistance.eval` -- the library is not installed -- is the plain
Levenshtein distance of tests/lexicon_statement.py.  That library's own arithmetic is therefore the one thing this file does
NOT pin.  The fixture holds strings and integers only.

    python tools/gen_golden_lexicon.py
"""
import io
import json
import os
import sys
import textwrap
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import lexicon_statement as S  # noqa: E402
from oracle import ref_shim  # noqa: E402

ASTRAL = "\U0001F600"
# (lexicon lines, pair-list lines or None, queries)
CASES = [
    (["Hello", "WORLD", "straße", "exit", "Ab", "hello", "Exit"], None,
     ["HELO", "hello", "EXIT", "exis", "zzzzzz", "", "STRASSE", "strase", "world", "wrld", "A", "ab", "ba", "AAAA", "Helloo", "xit"]),
    (["exit", "STRASSE", "newyork", "CAT", "CAR", "BAT", "CAT", "ŉ", "中文字", "中文", ASTRAL + "a"],
     ["EXIT Way Out", "STRASSE Straße", "NEWYORK  New  York City", "EXIT way out", "CAT cat one", "CAR car", "BAT  bat",
      "ʼN ŉ", "中文字 中文字", "中文 中文", ASTRAL + "A smile a", "UNUSED never looked up", "  CAT cat two  "],
     ["NEW YORK", "NEW YORC", "EXIT", "cat", "cot", "ct", "BA", "ŉ", "中文", "中字", "文", ASTRAL, ASTRAL + "ab", "STRAßE", "rat"]),
    ([], None, ["", "ANY"]),
    (["A" * 64, "AB" * 32, "B"], None, ["A" * 64, "A" * 63, "AB" * 32, "B" * 64, "A", ""]),
    (["AAA", "AAAA", "AB", "BA"], ["AAA three", "AAAA four", "AB ab", "BA ba"], ["AAAA", "AAA", "AA", "AB", "BA", "ABA", "B", "AAAAA"]),
]


def cut(lines, after, stop):
    """The lines behind the first one that contains `after` up to (not including) the next one whose text starts with `stop`,
    dedented."""
    a = next(i for i, ln in enumerate(lines) if after in ln) + 1
    b = next(i for i in range(a + 1, len(lines)) if lines[i].strip().startswith(stop))
    return textwrap.dedent("".join(lines[a:b])), a + 1, b


def main():
    path = os.path.join(ref_shim.REF_ROOT, "third_party", "adet", "evaluation", "text_evaluation_all.py")
    if not os.path.isfile(path):
        raise SystemExit("reference file not present at %s" % path)
    with open(path) as f:
        lines = f.readlines()
    a = next(i for i, ln in enumerate(lines) if ln.strip().startswith("def find_match_word("))
    b = next(i for i in range(a + 1, len(lines)) if lines[i].strip().startswith("for i in files:"))
    fmw_src = textwrap.dedent("".join(lines[a:b]))
    generic_src, a1, b1 = cut(lines, "GenericVocabulary_pair_list.txt", "if self.lexicon_type==2:")
    plain_src, a2, b2 = cut(lines, "ctw1500/weak_voc_pair_list.txt", 'elif "ic15"')
    accept_line = next(ln for ln in lines if ln.strip().startswith("if match_dist<"))
    print("executing %s lines %d-%d, %d-%d, %d-%d and the condition %r" % (os.path.basename(path), a + 1, b, a1, b1, a2, b2,
                                                                          accept_line.strip()))
    ns = {"editdistance": types.SimpleNamespace(eval=S.levenshtein)}
    exec(compile(fmw_src, path, "exec"), ns)
    find_match_word = ns["find_match_word"]
    accept = compile(accept_line.strip()[len("if "):-1], path, "eval")
    generic, plain = compile(generic_src, path, "exec"), compile(plain_src, path, "exec")

    cases = []
    for words, pair_lines, queries in CASES:
        lexicon_text = "".join(w + "\n" for w in words)
        pairs_text = None if pair_lines is None else "".join(p + "\n" for p in pair_lines)
        env = {"open": lambda name, mode="r": io.StringIO(lexicon_text), "lexicon_path": "lexicon"}
        if pairs_text is not None:
            env["pair_list"] = io.StringIO(pairs_text)
        exec(generic if pairs_text is not None else plain, env)
        lexicon, pairs = env["lexicon"], env["pairs"]
        expect = []
        for q in queries:
            word, dist = find_match_word(q, pairs, lexicon)
            expect.append([word, int(dist), bool(eval(accept, {"match_dist": dist}))])
        cases.append({"lexicon_text": lexicon_text, "pairs_text": pairs_text, "lexicon": lexicon, "pairs": pairs, "queries": queries,
                      "expect": expect})
    dst = os.path.join(ROOT, "tests", "golden", "lexicon_match.json")
    with open(dst, "w", encoding="utf-8") as f:
        f.write(json.dumps({"cases": cases}, ensure_ascii=False, indent=1) + "\n")
    n = sum(len(c["queries"]) for c in cases)
    print("wrote %s: %d cases, %d queries (%d accepted), %d bytes" % (
        dst, len(cases), n, sum(e[2] for c in cases for e in c["expect"]), os.path.getsize(dst)))


if __name__ == "__main__":
    main()
