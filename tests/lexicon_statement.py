"""THE RULE of the lexicon match (include/gomatching_hip.h, "Lexicon correction") as plain Python: the two-row dynamic
programme per pair and the strict-`<` scan in file order.  Strings are sequences of code points (Python str or lists of
ints).  Nothing else is trusted: the kernel and the numpy path are held to this, word for word."""

NO_MATCH = (-1, 100)


def norm(s):
    return s.upper()


def levenshtein(a, b):
    """Unit insert, delete and substitute; no transposition."""
    prev = list(range(len(b) + 1))
    for i in range(1, len(a) + 1):
        cur = [i] + [0] * len(b)
        for j in range(1, len(b) + 1):
            cur[j] = min(prev[j] + 1, cur[j - 1] + 1, prev[j - 1] + (a[i - 1] != b[j - 1]))
        prev = cur
    return prev[len(b)]


def match(q, words):
    """-> (index, distance): the LOWEST index at the smallest distance; (-1, 100) for no words."""
    best_i, best_d = NO_MATCH
    for i, w in enumerate(words):
        d = levenshtein(q, w)
        if d < best_d:
            best_i, best_d = i, d
    return best_i, best_d


def match_csr(q_chars, q_off, q_seg, w_chars, w_off, seg_off):
    """`match` on the kernel's own arguments (lists or arrays of ints) -> ([index], [dist])."""
    q_chars, q_off, q_seg, w_chars, w_off, seg_off = [[int(v) for v in a] for a in (q_chars, q_off, q_seg, w_chars, w_off, seg_off)]
    index, dist = [], []
    for s, g in enumerate(q_seg):
        words = [w_chars[w_off[i]:w_off[i + 1]] for i in range(seg_off[g], seg_off[g + 1])]
        i, d = match(q_chars[q_off[s]:q_off[s + 1]], words)
        index.append(i)
        dist.append(d)
    return index, dist
