"""Plain statements of what `gom_result_rows_i32` computes, and the input families its tests run on (shared by
test_result_rows_cpu.py and test_result_rows_gpu.py; no test in here).

`search` is the fp64 statement of the kernel's edge search: the hull of `results._convex_hull`, then Python floats and
`math.sqrt`, one rounding per operation, first minimum winning.  It differs from `results.min_area_rect` in one place,
sqrt(ex*ex + ey*ey) for np.hypot, which can only change the chosen edge where two DIFFERENT areas are within rounding of
each other (`near_tie`)."""
import math
import pickle

import numpy as np

from gomatching_amd import results as R
from gomatching_amd.predictor import boundary_to_polygon

WORDS = 234
POLY_I32, POLY_F32, RECS, EMIT, NHULL, HULL_MASK, EDGE, TRACK_ID = 0, 100, 200, 225, 226, 227, 229, 232


def search(points):
    """-> (hull, index of the chosen hull edge or -1, [area per non-degenerate edge])."""
    hull = R._convex_hull(np.asarray(points, dtype=np.float64).reshape(-1, 2))
    n = len(hull)
    if n < 2:
        return hull, -1, None
    best, bi, areas = None, -1, []
    for i in range(n):
        ex, ey = hull[(i + 1) % n][0] - hull[i][0], hull[(i + 1) % n][1] - hull[i][1]
        norm = math.sqrt(ex * ex + ey * ey)
        if norm == 0:
            continue
        ux, uy = ex / norm, ey / norm
        pu = [p[0] * ux + p[1] * uy for p in hull]
        pv = [-p[0] * uy + p[1] * ux for p in hull]
        a = (max(pu) - min(pu)) * (max(pv) - min(pv))
        areas.append(a)
        if best is None or a < best:
            best, bi = a, i
    return hull, bi, areas


def host_areas(points):
    """The edge areas `results.min_area_rect` itself compares (np.hypot, numpy arithmetic)."""
    hull = np.asarray(R._convex_hull(np.asarray(points, dtype=np.float64).reshape(-1, 2)), dtype=np.float64)
    areas, n = [], len(hull)
    if n < 2:
        return areas
    for i in range(n):
        e = hull[(i + 1) % n] - hull[i]
        norm = np.hypot(e[0], e[1])
        if norm == 0:
            continue
        ux, uy = e / norm
        pu = hull[:, 0] * ux + hull[:, 1] * uy
        pv = -hull[:, 0] * uy + hull[:, 1] * ux
        areas.append(float((pu.max() - pu.min()) * (pv.max() - pv.min())))
    return areas


def near_tie(points, rel=1e-12):
    """True iff the host's two smallest DISTINCT edge areas differ by a relative `rel` or less: the host itself decides such an
    instance by rounding.  Exact ties (equal areas) are not near-ties."""
    s = sorted(set(host_areas(points)))
    if len(s) < 2:
        return False
    return (s[1] - s[0]) <= rel * abs(s[1])


def emit_mask(rec, voc_size):
    """Bit c set iff character c is emitted (TextDecoder.decode's collapse), as a plain loop."""
    m = 0
    for c, v in enumerate(rec):
        is_char = v < voc_size - 1
        if is_char and (c == 0 or not (rec[c - 1] < voc_size - 1) or rec[c - 1] != v):
            m |= 1 << c
    return m


def geometry_words(bd):
    """The geometry words of every instance: bd [n,25,4] float32 -> int32 [n, WORDS] with recs / emit / id words left 0."""
    bd = np.asarray(bd, dtype=np.float32).reshape(-1, 25, 4)
    out = np.zeros((len(bd), WORDS), dtype=np.int32)
    for k, b in enumerate(bd):
        poly = boundary_to_polygon(b)                                   # [50,2] float32
        out[k, POLY_I32:POLY_I32 + 100] = poly.astype(int).reshape(100)
        out[k, POLY_F32:POLY_F32 + 100] = np.ascontiguousarray(poly).view(np.int32).reshape(100)
        hull, bi, _ = search(poly)
        pts = [(float(x), float(y)) for x, y in poly.astype(np.float64)]
        idx = [pts.index(h) for h in hull]                              # first occurrence of a repeated point
        mask = 0
        for i in idx:
            mask |= 1 << i
        out[k, NHULL] = len(hull)
        out[k, HULL_MASK:HULL_MASK + 2] = np.array([mask & 0xFFFFFFFF, mask >> 32], dtype=np.uint32).view(np.int32)
        out[k, EDGE:EDGE + 2] = (idx[bi], idx[(bi + 1) % len(idx)]) if bi >= 0 else (-1, -1)
    return out


def text_words(out, recs, voc_size, ids):
    """Fill the recs / emit / track-id words of `out` (a copy is returned)."""
    out = out.copy()
    recs = np.asarray(recs, dtype=np.int64).reshape(-1, 25)
    out[:, RECS:RECS + 25] = recs.astype(np.int32)
    out[:, EMIT] = [emit_mask(r, voc_size) for r in recs.tolist()]
    out[:, TRACK_ID:TRACK_ID + 2] = np.ascontiguousarray(np.asarray(ids, dtype=np.int64)).view(np.int32).reshape(-1, 2)
    return out


def statement_words(bd, recs, voc_size, ids):
    return text_words(geometry_words(bd), recs, voc_size, ids)


# ------------------------------------------------------------------------------------------------ input families
_T = np.linspace(0, 1, 25)
FAMILY_COUNTS = {"smooth": 20000, "axis": 3000, "noisy": 3000, "line": 500, "point": 100}


def _smooth(rng):
    cx, cy = rng.uniform(0, 1900), rng.uniform(0, 1000)
    L, hg, a = rng.uniform(3, 300), rng.uniform(2, 60), rng.uniform(-2, 2)
    xs = cx + (_T - .5) * L
    bend = rng.uniform(0, 10) * np.sin(_T * rng.uniform(0, 6) + a)
    top = np.stack([xs, cy - hg / 2 + bend + a * (xs - cx)], 1)
    bot = np.stack([xs, cy + hg / 2 + bend + a * (xs - cx)], 1)
    return np.hstack([top, bot]).astype(np.float32)


def _axis(rng):
    x0, y0 = rng.integers(0, 1000, 2)
    w, h = rng.integers(0, 200, 2)
    xs = x0 + _T * w
    return np.stack([xs, np.full(25, y0), xs, np.full(25, y0 + h)], 1).astype(np.float32)


def _noisy(rng):
    return rng.uniform(0, 500, (25, 4)).astype(np.float32)


def _line(rng):
    xs = rng.uniform(0, 500) + _T * rng.uniform(0, 100)
    return np.stack([xs, 2 * xs, xs, 2 * xs], 1).astype(np.float32)


def _point(rng):
    return np.full((25, 4), rng.uniform(0, 100), np.float32)


_GEN = {"smooth": _smooth, "axis": _axis, "noisy": _noisy, "line": _line, "point": _point}
_SEED = {"smooth": 11, "axis": 12, "noisy": 13, "line": 14, "point": 15}


def family(name, count=None):
    """[count,25,4] float32 boundaries of one family (text-like smooth strips, axis-aligned boxes including zero width or
    height, random point sets, collinear points, one repeated point); fixed seed."""
    rng = np.random.default_rng(_SEED[name])
    count = FAMILY_COUNTS[name] if count is None else count
    return np.stack([_GEN[name](rng) for _ in range(count)]) if count else np.zeros((0, 25, 4), np.float32)


def mixed(n):
    """n boundaries drawn from the five families in turn."""
    names = list(_GEN)
    per = {m: family(m, (n + len(names) - 1 - i) // len(names)) for i, m in enumerate(names)}
    out = np.zeros((n, 25, 4), np.float32)
    for i, m in enumerate(names):
        out[i::len(names)] = per[m]
    return out


def random_recs(n, voc_size, seed):
    """[n,25] int64 class ids with runs, blanks, and (when n allows) an all-blank and an all-equal row."""
    rng = np.random.default_rng(seed)
    recs = rng.integers(0, voc_size, (n, 25))
    blank = rng.random((n, 25)) < 0.4
    recs[blank] = voc_size - 1
    run = rng.random((n, 25)) < 0.3
    for c in range(1, 25):
        recs[:, c] = np.where(run[:, c], recs[:, c - 1], recs[:, c])
    if n > 2:
        recs[1] = voc_size - 1
        recs[2] = min(3, voc_size - 2)
    return recs.astype(np.int64)


def decoder_for(voc_size, tmp_path):
    """TextDecoder for 37 / 96, or for a custom dictionary of voc_size - 1 code points written under tmp_path."""
    from gomatching_amd.predictor import TextDecoder
    if voc_size in (37, 96):
        return TextDecoder(voc_size)
    path = str(tmp_path / ("dict_%d.pkl" % voc_size))
    with open(path, "wb") as fp:
        pickle.dump([0x4E00 + i for i in range(voc_size - 1)], fp)
    return TextDecoder(voc_size, path)
