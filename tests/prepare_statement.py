"""Plain statement of what `gom_quad_bezier_i32` and `prepare.quad_bezier_host` compute, one annotation at a time, and the
input families their tests and the benchmark run on (shared by test_prepare_statement_cpu.py, test_prepare_gpu.py and
tools/prepare_bench.py; no test in here).

The rule is the one written out in include/gomatching_hip.h ("Quad -> Bezier control points"): Python ints for everything
that is an integer (they do not overflow), Python floats and `math.sqrt` for the rest, one rounding per operation, no numpy
broadcasting.  `quad_bezier` is the whole rule; `hull`, `min_rect_corners`, `tight_rect`, `orient` and `bezier_of_rect` are its
steps, so that the steps the reference's own helpers pin (`get_tight_rect`, `cpt_bezier_pts`) can be compared on their own."""
import math

import numpy as np


def hull(points):
    """Monotone chain with `cross <= 0` popping over the distinct points, as `results._convex_hull`; integer crosses."""
    pts = sorted(set((int(x), int(y)) for x, y in points))
    if len(pts) <= 2:
        return pts

    def cross(o, a, b):
        return (a[0] - o[0]) * (b[1] - o[1]) - (a[1] - o[1]) * (b[0] - o[0])

    lower, upper = [], []
    for p in pts:
        while len(lower) >= 2 and cross(lower[-2], lower[-1], p) <= 0:
            lower.pop()
        lower.append(p)
    for p in reversed(pts):
        while len(upper) >= 2 and cross(upper[-2], upper[-1], p) <= 0:
            upper.pop()
        upper.append(p)
    return lower[:-1] + upper[:-1]


def min_rect_corners(h):
    """Hull -> the four corners of its minimum-area rectangle, truncated toward zero: [(x, y)] * 4."""
    n = len(h)
    if n == 1:
        return [h[0]] * 4
    best = None
    for i in range(n):
        ex, ey = float(h[(i + 1) % n][0] - h[i][0]), float(h[(i + 1) % n][1] - h[i][1])
        norm = math.sqrt(ex * ex + ey * ey)
        if norm == 0:
            continue
        ux, uy = ex / norm, ey / norm
        for j, (x, y) in enumerate(h):
            x, y = float(x), float(y)
            pu = x * ux + y * uy
            pv = y * ux - x * uy
            if j == 0:
                umin = umax = pu
                vmin = vmax = pv
            else:
                if pu > umax:
                    umax = pu
                if pu < umin:
                    umin = pu
                if pv > vmax:
                    vmax = pv
                if pv < vmin:
                    vmin = pv
        area = (umax - umin) * (vmax - vmin)
        if best is None or area < best[0]:
            best = (area, ux, uy, umin, umax, vmin, vmax)
    _, ux, uy, umin, umax, vmin, vmax = best
    return [(int(u * ux - v * uy), int(u * uy + v * ux)) for u, v in ((umin, vmin), (umax, vmin), (umax, vmax), (umin, vmax))]


def tight_rect(corners, H, W):
    """`get_tight_rect` with start 0 and scale 1: [(x, y)] * 4."""
    ps = sorted(corners, key=lambda p: p[0])                    # stable
    if ps[1][1] > ps[0][1]:
        p1, p4 = ps[0], ps[1]
    else:
        p1, p4 = ps[1], ps[0]
    if ps[3][1] > ps[2][1]:
        p2, p3 = ps[2], ps[3]
    else:
        p2, p3 = ps[3], ps[2]
    return [(min(max(x, 1), W - 1), min(max(y, 1), H - 1)) for x, y in (p1, p2, p3, p4)]


def orient(rect):
    s = 0
    for i in range(4):
        (x0, y0), (x1, y1) = rect[i], rect[(i + 1) % 4]
        s += x0 * y1 - x1 * y0
    return rect[::-1] if s < 0 else rect


def bezier_of_rect(rect):
    """`cpt_bezier_pts`: 16 ints."""
    len2 = [(rect[(i + 1) % 4][0] - rect[i][0]) ** 2 + (rect[(i + 1) % 4][1] - rect[i][1]) ** 2 for i in range(4)]
    order = sorted(range(4), key=lambda i: -len2[i])            # stable: ties go to the lower index
    out = []
    for i in order[:2]:
        p1, p2 = rect[i], rect[(i + 1) % 4]
        out += [p1[0], p1[1]]
        for k in (1, 2):
            t = k / 3
            out += [int((1 - t) * p1[0] + t * p2[0]), int((1 - t) * p1[1] + t * p2[1])]
        out += [p2[0], p2[1]]
    return out


def quad_bezier(quad, H, W):
    """quad: 8 ints (x1, y1, .., x4, y4) -> 16 ints."""
    pts = [(int(quad[2 * i]), int(quad[2 * i + 1])) for i in range(4)]
    return bezier_of_rect(orient(tight_rect(min_rect_corners(hull(pts)), int(H), int(W))))


def quad_bezier_all(quads, hw):
    quads = np.asarray(quads).reshape(-1, 8)
    return np.array([quad_bezier(q, h, w) for q, (h, w) in zip(quads.tolist(), np.asarray(hw).tolist())],
                    dtype=np.int32).reshape(-1, 16)


# ------------------------------------------------------------------------------------------------- input families
FAMILIES = ("strips", "axis_boxes", "convex", "concave", "self_intersecting", "three_collinear", "all_collinear",
            "repeated_point", "single_point", "partly_outside", "up_to_4096")
SIZES = np.array([[720, 1280], [1080, 1920], [480, 640], [97, 131], [361, 203], [2160, 4096], [4096, 4096], [2, 2]], dtype=np.int32)


def _rot_rect(rng, m, cx, cy, length, height, ang):
    ca, sa = np.cos(ang), np.sin(ang)
    local = np.array([[-1, -1], [1, -1], [1, 1], [-1, 1]], dtype=np.float64)          # [4,2]
    dx = local[None, :, 0] * length[:, None] / 2
    dy = local[None, :, 1] * height[:, None] / 2
    x = cx[:, None] + dx * ca[:, None] - dy * sa[:, None]
    y = cy[:, None] + dx * sa[:, None] + dy * ca[:, None]
    return np.rint(np.stack([x, y], axis=2)).astype(np.int64)


def _family(name, rng, m):
    """-> int64 [m,4,2]; coordinates meant for images of about 1280 x 720 unless the family says otherwise."""
    u = rng.uniform
    if name == "strips":
        return _rot_rect(rng, m, u(50, 1200, m), u(50, 650, m), u(20, 300, m), u(4, 40, m), u(-np.pi, np.pi, m))
    if name == "axis_boxes":
        x0, y0 = rng.integers(1, 1000, m), rng.integers(1, 600, m)
        w, h = rng.integers(0, 200, m), rng.integers(0, 80, m)
        w[::7] = 0
        h[3::7] = 0
        return np.stack([np.stack([x0, y0], 1), np.stack([x0 + w, y0], 1), np.stack([x0 + w, y0 + h], 1), np.stack([x0, y0 + h], 1)], 1)
    if name in ("convex", "self_intersecting"):
        ang = np.sort(u(0, 2 * np.pi, (m, 4)), axis=1)
        cx, cy, rx, ry = u(100, 1100, m), u(100, 600, m), u(5, 120, m), u(5, 90, m)
        q = np.rint(np.stack([cx[:, None] + rx[:, None] * np.cos(ang), cy[:, None] + ry[:, None] * np.sin(ang)], 2)).astype(np.int64)
        if name == "self_intersecting":
            q = q[:, [0, 2, 1, 3]]
        return q
    if name == "concave":
        tri = rng.integers(10, 700, (m, 3, 2))
        wts = rng.dirichlet([2, 2, 2], m)                                              # a point inside the triangle
        inner = np.rint((tri * wts[:, :, None]).sum(1)).astype(np.int64)
        q = np.concatenate([tri, inner[:, None]], 1)
        return q[:, [0, 1, 3, 2]]
    if name in ("three_collinear", "all_collinear"):
        base = rng.integers(10, 600, (m, 1, 2))
        step = rng.integers(-6, 7, (m, 1, 2))
        step[(step == 0).all(2)] = 1
        k = rng.integers(-8, 9, (m, 4, 1))
        q = base + k * step
        if name == "three_collinear":
            q[:, 3] = rng.integers(10, 600, (m, 2))
        return np.take_along_axis(q, rng.permuted(np.tile(np.arange(4), (m, 1)), axis=1)[:, :, None], 1)
    if name == "repeated_point":
        q = rng.integers(5, 700, (m, 4, 2))
        a, b = rng.integers(0, 4, m), rng.integers(0, 4, m)
        q[np.arange(m), a] = q[np.arange(m), b]
        return q
    if name == "single_point":
        return np.repeat(rng.integers(-5, 1400, (m, 1, 2)), 4, axis=1)
    if name == "partly_outside":
        return _rot_rect(rng, m, u(-60, 1340, m), u(-60, 780, m), u(20, 400, m), u(4, 120, m), u(-np.pi, np.pi, m))
    if name == "up_to_4096":
        q = rng.integers(0, 4097, (m, 4, 2))
        q[::5] = _rot_rect(rng, len(q[::5]), u(200, 3900, len(q[::5])), u(200, 3900, len(q[::5])), u(100, 1500, len(q[::5])),
                           u(10, 200, len(q[::5])), u(-np.pi, np.pi, len(q[::5])))
        return q
    raise KeyError(name)


def mixed_batch(n, seed=0x9E2A):
    """-> (quads int32 [n,8], hw int32 [n,2], family index int64 [n]): the families above in equal shares, shuffled, with a
    per-quad image size from SIZES (the family's usual size three times in four, any of SIZES otherwise)."""
    rng = np.random.Generator(np.random.Philox(key=seed))
    fam = np.arange(n) % len(FAMILIES)
    quads = np.zeros((n, 4, 2), dtype=np.int64)
    for f, name in enumerate(FAMILIES):
        idx = np.nonzero(fam == f)[0]
        quads[idx] = _family(name, rng, len(idx))
    usual = np.where(fam == FAMILIES.index("up_to_4096"), 6, 0)
    size = np.where(rng.random(n) < 0.75, usual, rng.integers(0, len(SIZES), n))
    perm = rng.permutation(n)
    return quads.reshape(n, 8).astype(np.int32)[perm], SIZES[size][perm], fam[perm]


BATCH = 20000
_batch = []


def reference_batch():
    """The mixed batch of the CPU and GPU tests with the statement's 16 words per quad; computed once per process (about a
    second) and handed out read-only."""
    if not _batch:
        quads, hw, fam = mixed_batch(BATCH)
        ref = quad_bezier_all(quads, hw)
        for a in (quads, hw, fam, ref):
            a.setflags(write=False)
        _batch.append((quads, hw, fam, ref))
    return _batch[0]
