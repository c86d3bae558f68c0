"""Shared by tests/test_lexicon_cpu.py and tests/test_lexicon_gpu.py: CSR marshalling in plain Python, and a hand-made result
tree (two videos, a few frames, rows with and without `segmentation`, a track whose vote changes after correction) with the
output the rule asks for, worked out with tests/lexicon_statement.py alone."""
import os

import lexicon_statement as S
from gomatching_amd import results

VIDEOS = ("Video_35_2_3", "clipB")                       # the first is written under ICDAR15's stem, res_video_35.xml
STEMS = {"Video_35_2_3": "video_35", "clipB": "clipB"}
SHARED_WORDS = ["Hello", "WORLD", "straße", "exit", "Ab", "hello"]          # 'hello' after 'Hello': the later line's display wins
NOTHING_WORDS = ["qqqqqqqqqqqqqqqqqqqqqqqq", "jjjjjjjjjjjjjjjjjjjjjjjjjjjjjj"]
DIR_WORDS = {"Video_35_2_3": ["HELP", "WORD"], "clipB": ["exit", "STRASSE", "newyork"]}
# later line wins; a display value with spaces (everything behind the key's one separator, a second space included)
DIR_PAIRS = {"clipB": ["EXIT Way Out", "STRASSE Straße", "NEWYORK  New  York City", "EXIT way out"]}


def codes(s):
    return [ord(c) for c in s]


def csr(queries, segments):
    """queries: [(segment, string or list of code points)], segments: [[word, ...]] -> the kernel's six arrays as lists."""
    q_chars, q_off, q_seg = [], [0], []
    for g, q in queries:
        q_chars += codes(q) if isinstance(q, str) else list(q)
        q_off.append(len(q_chars))
        q_seg.append(g)
    w_chars, w_off, seg_off = [], [0], [0]
    for words in segments:
        for w in words:
            w_chars += codes(w) if isinstance(w, str) else list(w)
            w_off.append(len(w_chars))
        seg_off.append(len(w_off) - 1)
    return q_chars, q_off, q_seg, w_chars, w_off, seg_off


def _quad(k):
    return [10 + k, 20, 60 + k, 20, 60 + k, 40, 10 + k, 40]


def _row(k, track, text, seg=True):
    row = _quad(k) + [track, text]
    if seg:
        row.append([[[10 + k, 20], [60 + k, 20], [60 + k, 40], [10 + k, 40]]])
    return row


def annotations():
    a = {"1": [_row(0, 7, "HELO"), _row(1, 8, "EXIT", seg=False), _row(2, 9, "zzzzzz")],
         "2": [_row(0, 7, "HELO"), _row(1, 8, "EXIS"), _row(3, 11, "STRASSE", seg=False)],
         "3": [],
         "4": [_row(0, 7, "HELLO", seg=False), _row(1, 8, "EXIU"), _row(2, 9, "world"), _row(4, 12, "")]}
    b = {"1": [_row(5, 1, "NEW YORK"), _row(6, 2, "strasse"), _row(7, 3, "Hallo")],
         "2": [_row(5, 1, "NEW YORC"), _row(6, 2, "STRAßE", seg=False), _row(8, 4, "中文")]}
    return {"Video_35_2_3": a, "clipB": b}


def write_tree(root, anns):
    """anns {video: annotation} -> root/jsons, root/preds (xml + txt) as the eval command leaves them."""
    os.makedirs(os.path.join(root, "jsons"), exist_ok=True)
    os.makedirs(os.path.join(root, "preds"), exist_ok=True)
    for v, ann in anns.items():
        results.write_video_results(ann, os.path.join(root, "jsons", v + ".json"), os.path.join(root, "preds", "res_%s.xml" % STEMS[v]))
    results.write_track_transcriptions(os.path.join(root, "preds"))
    return root


def _write_lines(path, lines):
    with open(path, "w", encoding="utf-8") as f:
        f.write("".join(l + "\n" for l in lines))
    return path


def build(root):
    """-> {"res", "lexicon", "nothing", "lexdir"}: a result tree and its vocabularies under `root`."""
    res = write_tree(os.path.join(root, "res"), annotations())
    lexdir = os.path.join(root, "strong")
    os.makedirs(lexdir)
    for v, words in DIR_WORDS.items():
        _write_lines(os.path.join(lexdir, v + ".txt"), words)
    for v, lines in DIR_PAIRS.items():
        _write_lines(os.path.join(lexdir, v + ".pairs.txt"), lines)
    return {"res": res, "lexdir": lexdir,
            "lexicon": _write_lines(os.path.join(root, "shared.txt"), ["", "  Hello ", "WORLD"] + SHARED_WORDS[2:] + [" "]),
            "nothing": _write_lines(os.path.join(root, "nothing.txt"), NOTHING_WORDS)}


def pairs_of(words, pair_lines=None):
    """The display map by the rule, in plain Python."""
    table = {}
    if pair_lines is None:
        for w in words:
            table[S.norm(w)] = w
    else:
        for line in pair_lines:
            line = line.strip()
            key = line.split(" ")[0].upper()
            table[key] = line[len(key) + 1:]
    return table


def expected(anns, vocab, max_dist=1, unmatched="keep"):
    """vocab {video: (words, pair lines or None)} -> the corrected {video: annotation}, by the statement."""
    out = {}
    for v, ann in anns.items():
        words, pair_lines = vocab[v]
        table = pairs_of(words, pair_lines)
        normal = [S.norm(w) for w in words]
        out[v] = {}
        for frame, rows in ann.items():
            out[v][frame] = []
            for row in rows:
                i, d = S.match(S.norm(row[9]), normal)
                if i >= 0 and d <= max_dist:
                    out[v][frame].append(row[:9] + [table[normal[i]]] + row[10:])
                elif unmatched == "keep":
                    out[v][frame].append(row)
    return out


def tree_bytes(root, skip=()):
    """{path relative to root: bytes} of every file under root, directories named in `skip` left out."""
    out = {}
    for dirpath, dirs, files in os.walk(root):
        dirs[:] = [d for d in dirs if d not in skip]
        for f in files:
            p = os.path.join(dirpath, f)
            with open(p, "rb") as fh:
                out[os.path.relpath(p, root)] = fh.read()
    return out
