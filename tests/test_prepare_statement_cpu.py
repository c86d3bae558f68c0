"""CPU: the quad -> Bezier rule of the prepare command (include/gomatching_hip.h, "Quad -> Bezier control points").

  * the plain-Python statement (prepare_statement.py) against what the REFERENCE's own `get_tight_rect` and `cpt_bezier_pts`
    returned (tests/golden/prepare_geometry.json, tools/gen_golden_prepare.py): integers equal;
  * `prepare.fit_14gon` against the reference's `polygon_to_bezier_pts`, within 64 * eps * cond * max|coordinate| -- the
    forward-error bound of a least-squares solve with the recorded condition number of the reference's own Bernstein matrix,
    not a tuned number;
  * `prepare.quad_bezier_host` (numpy, vectorised over the annotations) against the statement, every word, on the families of
    the GPU test;
  * four hand-checked quads with their 16 integers written out.
The hull and rectangle steps (cv2.minAreaRect / boxPoints in the reference) and the orientation at zero area have no
reference fixture: they are UNPINNED and only the statement holds them."""
import json
import os

import numpy as np
import pytest

import prepare_statement as S
from helpers import GOLDEN
from gomatching_amd import prepare


@pytest.fixture(scope="module")
def geometry():
    with open(os.path.join(GOLDEN, "prepare_geometry.json")) as f:
        return json.load(f)


def test_tight_rect_is_the_references_get_tight_rect(geometry):
    cases = geometry["get_tight_rect"]
    assert len(cases) >= 100
    ties = 0
    for c in cases:
        corners = [tuple(p) for p in c["corners"]]
        got = S.tight_rect(corners, c["H"], c["W"])
        assert [v for p in got for v in p] == c["out"], c
        ties += len(set(p[0] for p in corners)) < 4
    assert ties >= 30                                            # x-ties, where only the stable sort decides


def test_bezier_of_rect_is_the_references_cpt_bezier_pts(geometry):
    cases = geometry["cpt_bezier_pts"]
    assert len(cases) >= 100
    equal_edges = 0
    for c in cases:
        rect = [tuple(p) for p in c["rect"]]
        assert S.bezier_of_rect(rect) == c["out"], c
        len2 = [(rect[(i + 1) % 4][0] - rect[i][0]) ** 2 + (rect[(i + 1) % 4][1] - rect[i][1]) ** 2 for i in range(4)]
        equal_edges += len(set(len2)) < 4
    assert equal_edges >= 60


def test_fit_14gon_is_the_references_polygon_to_bezier_pts(geometry):
    cases = geometry["polygon_to_bezier_pts"]
    assert len(cases) >= 30
    eps = np.finfo(np.float64).eps
    worst = 0.0
    for c in cases:
        got = np.array(prepare.fit_14gon(c["poly"]))
        ref = np.array(c["out"])
        assert got.shape == ref.shape == (16,)
        big = float(np.abs(c["poly"]).max())
        for side in range(2):
            bound = 64 * eps * c["cond"][side] * big
            err = float(np.abs(got[8 * side:8 * side + 8] - ref[8 * side:8 * side + 8]).max())
            worst = max(worst, err / bound)
            assert err <= bound, (c["poly"], side, err, bound)
        # end control points are the first and last data points of each side
        p = np.array(c["poly"], dtype=np.float64).reshape(14, 2)
        assert got[0:2].tolist() == p[0].tolist() and got[6:8].tolist() == p[6].tolist()
        assert got[8:10].tolist() == p[7].tolist() and got[14:16].tolist() == p[13].tolist()
    print("largest error / bound: %.3g" % worst)


def test_host_path_equals_the_statement_word_for_word():
    quads, hw, fam, ref = S.reference_batch()
    got = prepare.quad_bezier_host(quads, hw)
    assert got.dtype == np.int32 and got.shape == ref.shape == (S.BATCH, 16)
    bad = np.nonzero((got != ref).any(1))[0]
    assert bad.size == 0, [(S.FAMILIES[fam[b]], quads[b].tolist(), hw[b].tolist(), ref[b].tolist(), got[b].tolist()) for b in bad[:3]]
    counts = np.bincount(fam, minlength=len(S.FAMILIES))
    print({name: int(c) for name, c in zip(S.FAMILIES, counts)})
    assert (counts >= S.BATCH // len(S.FAMILIES)).all()
    sizes = np.bincount([len(S.hull(np.array(q).reshape(4, 2))) for q in quads[:4000].tolist()], minlength=5)
    assert (sizes[1:] > 0).all(), sizes                          # hulls of 1, 2, 3 and 4 points all occur
    assert len(set(map(tuple, hw.tolist()))) == len(S.SIZES)     # per-quad H, W differ within the batch
    for n in (0, 1, 63, 64, 65, 257):
        assert np.array_equal(prepare.quad_bezier_host(quads[:n], hw[:n]), ref[:n]), n


HAND = [
    # an axis-aligned rectangle 100 x 30: the corners are exact, the long edges are the top (left to right) and the bottom (right to
    # left); thirds of 10 -> 110 are 43.33 and 76.67, truncated
    ("axis-aligned rectangle", [10, 20, 110, 20, 110, 50, 10, 50], (720, 1280),
     [10, 20, 43, 20, 76, 20, 110, 20, 110, 50, 76, 50, 43, 50, 10, 50]),
    # a square on its tip, corners (100,50) (150,100) (100,150) (50,100).  The hull starts at (50,100) and its first edge is
    # (50,-50)/70.71..: the corners come back through an irrational unit vector, and fp64 lands a hair under 100, 50 and 150 for
    # some of them, which truncation turns into 99, 49 and 149 -- this is what the rule says, not what a calipers library would.
    # All edges are equal: edges 0 and 1 are taken.
    ("45-degree square", [100, 50, 150, 100, 100, 150, 50, 100], (720, 1280),
     [99, 49, 115, 65, 132, 82, 149, 99, 149, 99, 132, 115, 115, 132, 99, 149]),
    # the whole top strip of a 1280 x 720 image: x is clamped to [1, 1279], y to [1, 719]; thirds of 1 -> 1279 are 427 and 853
    ("quad on the image border", [0, 0, 1279, 0, 1279, 30, 0, 30], (720, 1280),
     [1, 1, 427, 1, 853, 1, 1279, 1, 1279, 30, 853, 30, 427, 30, 1, 30]),
    # one point four times: a one-point hull, four equal corners, every control point is the point
    ("single repeated point", [7, 9, 7, 9, 7, 9, 7, 9], (720, 1280), [7, 9] * 8),
]


@pytest.mark.parametrize("name,quad,hw,want", HAND, ids=[h[0] for h in HAND])
def test_hand_checked_quads(name, quad, hw, want):
    assert S.quad_bezier(quad, *hw) == want
    assert prepare.quad_bezier_host(np.array([quad]), np.array([hw])).tolist() == [want]
