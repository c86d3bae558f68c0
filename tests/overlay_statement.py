"""Drawing tracked text on frames, stated per pixel in plain Python / numpy integers (not collected: no test_ prefix).

What csrc/overlay.hip and `show.compose_host` are held to, byte for byte -- the rule of `gom_overlay_compose_u8` in
include/gomatching_hip.h, built on `mask_statement.line_pixels` and `mask_statement.fill_contours`, imported unchanged:

  outline_contours   Boundary(contour) alone, unioned over the contours: the error-stepped 8-connected lines
  compose_statement  for every pixel: the frame's instances IN ORDER (outline bit -> the colour, else face bit -> blend at
                     a_face), then the frame's labels IN ORDER (glyph bit -> the label's colour, else blend with white at a_box)
  blend              (p (255 - a) + c a + 127) // 255

and the seeded cases the CPU and the GPU test share.
"""
import functools

import numpy as np

import mask_statement as ms

A_FACE, A_BOX = 128, 204


def blend(p, c, a):
    return (int(p) * (255 - a) + int(c) * a + 127) // 255


def outline_contours(contours, H, W):
    """contours: a list of [[x, y], ...] integer vertex lists -> bool [H, W], Boundary alone."""
    img = np.zeros((H, W), dtype=bool)
    for contour in contours:
        contour = [(int(p[0]), int(p[1])) for p in contour]
        for i in range(len(contour)):
            for x, y in ms.line_pixels(*contour[i - 1], *contour[i]):
                if 0 <= x < W and 0 <= y < H:
                    img[y, x] = True
    return img


def compose_statement(frames, instances, labels, a_face=A_FACE, a_box=A_BOX):
    """frames u8 [F,H,W,3]; instances: per frame a list of (contours, (c0, c1, c2)); labels: per frame a list of
    (x0, y0, bool [h, w] bitmap, (c0, c1, c2)) -> u8 [F,H,W,3]."""
    frames = np.asarray(frames, dtype=np.uint8)
    F, H, W, _ = frames.shape
    out = frames.copy()
    for f in range(F):
        faces = [ms.fill_contours(c, H, W) for c, _ in instances[f]]
        lines = [outline_contours(c, H, W) for c, _ in instances[f]]
        for y in range(H):
            for x in range(W):
                v = [int(t) for t in frames[f, y, x]]
                for k, (_, rgb) in enumerate(instances[f]):
                    if lines[k][y, x]:
                        v = [int(t) for t in rgb]
                    elif faces[k][y, x]:
                        v = [blend(v[i], rgb[i], a_face) for i in range(3)]
                for x0, y0, bits, rgb in labels[f]:
                    h, w = bits.shape
                    if x0 <= x < x0 + w and y0 <= y < y0 + h:
                        if bits[y - y0, x - x0]:
                            v = [int(t) for t in rgb]
                        else:
                            v = [blend(v[i], 255, a_box) for i in range(3)]
                out[f, y, x] = v
    return out


# ------------------------------------------------------------------------------------------ shared cases
def _colors(rng, n):
    return [tuple(int(v) for v in rng.randint(0, 256, 3)) for _ in range(n)]


def _label(rng, x0, y0, w, h):
    return (x0, y0, rng.rand(h, w) < 0.5, tuple(int(v) for v in rng.randint(0, 256, 3)))


def main_case():
    """F = 3 frames of 37 x 70: three word columns with a partial last one, rows of 210 bytes and frames of 7770 bytes (no
    multiples of 4).  Frame 0 empty, frame 1 one instance, frame 2 seventy heavily overlapping instances (more than one
    64-wide culling round) and the labels: inside, across each image side, outside, of size 0, 33 and 70 wide, two
    overlapping."""
    H, W = 37, 70
    rng = np.random.RandomState(5)
    frames = rng.randint(0, 256, (3, H, W, 3)).astype(np.uint8)
    contours = ms.random_contours(71, H, W, seed=23)
    colors = _colors(rng, 71)
    instances = [[], [([contours[0]], colors[0])], [([c], col) for c, col in zip(contours[1:], colors[1:])]]
    labels = [[], [_label(rng, 30, 12, 17, 7)],
              [_label(rng, 10, 5, 20, 8),                                # inside
               _label(rng, -7, 10, 20, 6), _label(rng, 20, -4, 12, 9), _label(rng, 60, 15, 20, 7), _label(rng, 30, 33, 15, 8),
               _label(rng, 100, 100, 9, 9), _label(rng, -50, -50, 9, 9),  # outside
               _label(rng, 40, 20, 0, 0),                                # size 0
               _label(rng, 2, 20, 33, 5), _label(rng, 0, 26, 70, 6), _label(rng, -3, 1, 70, 3),
               _label(rng, 12, 7, 18, 9), _label(rng, 15, 9, 18, 9)]]    # overlapping each other (and the first)
    return frames, instances, labels


def small_case(H, W, seed):
    """Two frames with a handful of instances and two labels each."""
    rng = np.random.RandomState(seed)
    frames = rng.randint(0, 256, (2, H, W, 3)).astype(np.uint8)
    contours = ms.random_contours(9, H, W, seed=seed + 1)
    colors = _colors(rng, 9)
    instances = [[([c], col) for c, col in zip(contours[:5], colors[:5])], [([c], col) for c, col in zip(contours[5:], colors[5:])]]
    labels = [[_label(rng, 1, 1, 9, 3), _label(rng, W - 5, H - 2, 9, 4)], [_label(rng, -2, 2, W + 4, 2), _label(rng, 3, 0, 6, H)]]
    return frames, instances, labels


SMALL = ((16, 32, 41), (5, 33, 43))                                      # exactly one word column; one word column and a pixel


@functools.lru_cache(maxsize=None)
def case(name):
    """-> (frames, instances, labels, the statement's output), computed once and shared (never modified)."""
    frames, instances, labels = main_case() if name == "main" else small_case(*SMALL[int(name)])
    want = compose_statement(frames, instances, labels)
    frames.setflags(write=False)
    want.setflags(write=False)
    return frames, instances, labels, want


def scene_of(frames, instances, labels):
    """A case as the `show.Scene` the host path and the kernels take (one contour per instance)."""
    from gomatching_amd import show
    atlas = show.Atlas()
    lab = [[(x0, y0, atlas.add(bits), rgb) for x0, y0, bits, rgb in fr] for fr in labels]
    polys = [[np.asarray(c[0], dtype=np.int64) for c, _ in fr] for fr in instances]
    colors = [[rgb for _, rgb in fr] for fr in instances]
    return show.Scene(polys, colors, lab, atlas.arrays(), frames.shape[1], frames.shape[2])
