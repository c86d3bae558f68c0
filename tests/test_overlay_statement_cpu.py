"""CPU: drawing tracked text on frames without a GPU -- hand-worked pixels of the statement (tests/overlay_statement.py), the
numpy path of `gomatching_amd.show` against the statement byte for byte on the seeded cases of the GPU test, the host
helpers (colours, label text, font size, label anchor, atlas packing), the argument checks of the two entry points and the
errors of the command line."""
import ctypes
import json
import os

import numpy as np
import pytest
from PIL import Image

import overlay_statement as ov

TRIANGLE = [(1, 1), (6, 1), (1, 6)]
TRI_LINE = {(x, 1) for x in range(1, 7)} | {(1, y) for y in range(1, 7)} | {(x, 7 - x) for x in range(1, 7)}
TRI_FACE = {(x, y) for x in range(2, 6) for y in range(2, 6) if x + y <= 6}        # strictly inside


def _pixels(img):
    return {(int(x), int(y)) for y, x in zip(*np.nonzero(img))}


def _host(frames, instances, labels, **kw):
    from gomatching_amd import show
    return show.compose_host(frames, ov.scene_of(np.asarray(frames), instances, labels), **kw)


def test_blend_hand_values():
    from gomatching_amd import show
    for p, c, a, want in ((0, 255, 128, 128), (255, 0, 128, 127), (10, 200, 204, 162), (7, 99, 0, 7), (7, 99, 255, 99)):
        assert ov.blend(p, c, a) == want
        assert int(show._blend(np.int32(p), np.int32(c), a)) == want


def test_triangle_outline_face_and_blended_values():
    import mask_statement as ms
    assert _pixels(ov.outline_contours([TRIANGLE], 8, 8)) == TRI_LINE
    assert _pixels(ms.fill_contours([TRIANGLE], 8, 8)) == TRI_LINE | TRI_FACE
    for back, col, face_value in ((0, 255, 128), (255, 0, 127)):
        frames = np.full((1, 8, 8, 3), back, dtype=np.uint8)
        inst = [[([TRIANGLE], (col, col, col))]]
        for got in (ov.compose_statement(frames, inst, [[]]), _host(frames, inst, [[]])):
            for y in range(8):
                for x in range(8):
                    want = col if (x, y) in TRI_LINE else (face_value if (x, y) in TRI_FACE else back)
                    assert got[0, y, x].tolist() == [want] * 3, (x, y)
    frames = np.full((1, 8, 8, 3), 10, dtype=np.uint8)
    got = ov.compose_statement(frames, [[([TRIANGLE], (200, 200, 200))]], [[]], a_face=204)
    assert got[0, 3, 3].tolist() == [162] * 3 and got[0, 7, 7].tolist() == [10] * 3
    assert np.array_equal(got, _host(frames, [[([TRIANGLE], (200, 200, 200))]], [[]], a_face=204))


def test_instance_order_matters():
    a = ([[(0, 0), (5, 0), (5, 5), (0, 5)]], (250, 10, 10))
    b = ([[(3, 3), (7, 3), (7, 7), (3, 7)]], (10, 10, 250))
    frames = np.full((1, 8, 8, 3), 100, dtype=np.uint8)
    ab, ba = ov.compose_statement(frames, [[a, b]], [[]]), ov.compose_statement(frames, [[b, a]], [[]])
    assert not np.array_equal(ab, ba)
    assert ab[0, 3, 4].tolist() == [10, 10, 250]                          # b's outline over a's face
    assert ba[0, 4, 5].tolist() == [250, 10, 10]                          # a's outline over b's face
    assert ba[0, 3, 4].tolist() == [ov.blend(10, 250, 128), 10, ov.blend(250, 10, 128)]       # a's face over b's outline
    x = ov.blend(100, 250, 128)                                                               # (4, 4): both faces
    assert ab[0, 4, 4].tolist() == [ov.blend(x, 10, 128), ov.blend(ov.blend(100, 10, 128), 10, 128), ov.blend(ov.blend(100, 10, 128), 250, 128)]
    assert np.array_equal(ab, _host(frames, [[a, b]], [[]])) and np.array_equal(ba, _host(frames, [[b, a]], [[]]))


def test_label_over_polygon_wins():
    square = ([[(0, 0), (7, 0), (7, 7), (0, 7)]], (0, 200, 0))
    bits = np.zeros((3, 4), dtype=bool)
    bits[1, 1:3] = True
    frames = np.zeros((1, 8, 8, 3), dtype=np.uint8)
    got = ov.compose_statement(frames, [[square]], [[(2, 2, bits, (9, 8, 7))]])
    face = [0, ov.blend(0, 200, 128), 0]
    assert got[0, 3, 3].tolist() == [9, 8, 7] and got[0, 3, 4].tolist() == [9, 8, 7]            # glyph bits
    assert got[0, 2, 2].tolist() == [ov.blend(v, 255, 204) for v in face]                       # the label's box over the face
    assert got[0, 5, 5].tolist() == face and got[0, 0, 0].tolist() == [0, 200, 0]
    assert np.array_equal(got, _host(frames, [[square]], [[(2, 2, bits, (9, 8, 7))]]))


@pytest.mark.parametrize("x0,y0,inside", [(-2, 3, (slice(3, 6), slice(0, 2))), (6, 3, (slice(3, 6), slice(6, 8))),
                                          (2, -1, (slice(0, 2), slice(2, 6))), (2, 6, (slice(6, 8), slice(2, 6)))])
def test_label_clipped_at_each_image_side(x0, y0, inside):
    bits = np.ones((3, 4), dtype=bool)
    frames = np.full((1, 8, 8, 3), 50, dtype=np.uint8)
    got = ov.compose_statement(frames, [[]], [[(x0, y0, bits, (1, 2, 3))]])
    want = frames.copy()
    want[0][inside] = (1, 2, 3)
    assert np.array_equal(got, want)
    assert np.array_equal(got, _host(frames, [[]], [[(x0, y0, bits, (1, 2, 3))]]))


@pytest.mark.parametrize("name", ["main", "0", "1"])
def test_host_path_equals_the_statement(name):
    frames, instances, labels, want = ov.case(name)
    got = _host(frames, instances, labels)
    assert got.dtype == np.uint8 and np.array_equal(got, want)
    if name == "main":
        assert np.array_equal(got[0], frames[0]) and (got[1] != frames[1]).any() and (got[2] != frames[2]).any()


def test_host_helpers():
    from gomatching_amd import show
    colors = [show.track_color(i) for i in range(1200)]
    assert all(len(c) == 3 and all(isinstance(v, int) and 0 <= v <= 255 for v in c) for c in colors)
    assert colors[:500] == colors[500:1000] and show.track_color(7) == show.track_color(507) == show.track_color(7)
    assert len(set(colors[:500])) > 400                                   # a palette, not one colour
    assert show.track_color(0) == (255, 115, 115)                         # hsv (0, 0.55, 1.0)
    assert show.text_color((0, 0, 0)) == (204, 51, 51)                    # all raised to 0.2, the first maximum to 0.8
    assert show.text_color((10, 20, 30)) == (204, 51, 51)
    assert show.text_color((10, 20, 90)) == (51, 51, 204)
    assert show.text_color((255, 128, 0)) == (255, 128, 51)
    assert show.text_color((100, 230, 100)) == (100, 230, 100)
    assert show.label_text(3, "hello", 37) == "(3)HELLO" and show.label_text(3, "hello", 96) == "(3)hello"
    assert show.label_text(12, "", 37) == "(12)"
    assert show.font_px(720, 1280) == 13 and show.font_px(72, 128) == 10 and show.font_px(1080, 1920) == 20
    # a straight strip: 25 points along y = 0 from x = 0 to 96, back along y = 10 -> centre line y = 5, midpoint x = 48
    top = np.stack([np.linspace(0, 96, 25), np.zeros(25)], 1)
    strip = np.concatenate([top, top[::-1] + [0, 10]])
    assert show.label_anchor(strip) == (48, 5)
    assert show.label_anchor([[0, 0], [10, 0], [10, 4], [0, 4]]) == (5, 2)
    assert show.label_anchor([[0, 0], [3, 0], [3, 9], [0, 9]]) == (1, 4)          # (1.5, 4.5) truncated
    assert show.label_anchor([[4, 4], [4, 4], [4, 4]]) == (4, 4)                  # no length: the first point
    # an L-shaped centre line: (0,0) -> (10,0) -> (10,30): half of 40 lies 10 down the second leg
    assert show.label_anchor([[0, 0], [10, 0], [10, 30], [10, 30], [10, 0], [0, 0]]) == (10, 10)


def test_atlas_packing_equals_pillow():
    from PIL import ImageFont
    from gomatching_amd import show
    atlas = show.Atlas()
    texts = ["(1)A", "(23)A MUCH LONGER LABEL THAN SIXTY-FOUR PIXELS", "(1)A"]
    idx = [atlas.index(t, 13) for t in texts]
    assert idx[0] == idx[2] != idx[1] and len(atlas.wh) == 2             # cached by (string, px)
    assert atlas.index("(1)A", 10) == 2                                   # another size is another bitmap
    wh, woff, words = atlas.arrays()
    assert wh.dtype == np.int32 and woff.dtype == np.int64 and words.dtype == np.uint32 and woff[-1] == len(words)
    font = ImageFont.load_default(13)
    for i, t in ((0, texts[0]), (1, texts[1])):
        mask = font.getmask(t, mode="1")
        w, h = mask.size
        ref = np.zeros((h + 2, w + 2), dtype=bool)                        # one pixel of padding on every side
        ref[1:-1, 1:-1] = np.asarray(Image.frombytes("L", (w, h), bytes(mask))) != 0
        assert tuple(wh[i]) == (w + 2, h + 2) and ref.any()
        rw = (w + 2 + 31) // 32
        mine = words[woff[i]:woff[i + 1]].reshape(h + 2, rw)
        for y in range(h + 2):
            for x in range(32 * rw):
                assert bool(mine[y, x // 32] >> np.uint32(x % 32) & np.uint32(1)) == (x < w + 2 and bool(ref[y, x])), (i, x, y)
    assert wh[1][0] > 64
    sub = atlas.arrays([1])
    assert np.array_equal(sub[0], wh[1:2]) and np.array_equal(sub[2], words[woff[1]:woff[2]])


def test_entry_points_reject_bad_arguments_without_a_gpu():
    from gomatching_amd import lib
    L = lib.load()
    OK, INVALID = 0, 1
    p, odd = ctypes.c_void_p(0x1000), ctypes.c_void_p(0x1004)             # never dereferenced

    def compose(frames=p, out=p, F=1, H=8, W=8, boxes=p, N=1, nwords=4, Lb=1, G=1, gwords=4, a_face=128, a_box=204, inst_off=p):
        return L.gom_overlay_compose_u8(frames, out, F, H, W, p, p, boxes, p, N, nwords, inst_off, p, p, p, p, p, Lb, p, p, p, G,
                                        gwords, a_face, a_box, None)
    assert compose(frames=None) == INVALID and compose(out=None) == INVALID and compose(inst_off=None) == INVALID
    assert compose(boxes=None) == INVALID
    assert compose(F=-1) == INVALID and compose(N=-1) == INVALID and compose(Lb=-1) == INVALID and compose(nwords=-1) == INVALID
    assert compose(H=0) == INVALID and compose(W=0) == INVALID and compose(H=65536, W=32768) == INVALID
    assert compose(a_face=256) == INVALID and compose(a_box=-1) == INVALID
    assert compose(boxes=odd) == INVALID
    assert compose(G=0) == INVALID                                        # labels without an atlas
    assert compose(F=0) == OK                                             # no frames: no launch
    assert compose(N=0, Lb=0) == OK                                       # nothing to draw in place: no launch

    def outline(boxes=p, N=2, M=2, sel=None, H=8, W=8, points=p, nwords=4, words=p):
        return L.gom_mask_outline_polygons_u32(points, 6, p, 2, p, boxes, p, N, nwords, sel, M, H, W, words, None)
    assert outline(boxes=None) == INVALID and outline(points=None) == INVALID and outline(words=None) == INVALID
    assert outline(M=1) == INVALID and outline(sel=p, M=3) == INVALID     # M != N without sel, M > N with it
    assert outline(boxes=odd) == INVALID and outline(H=0) == INVALID and outline(H=65536, W=32768) == INVALID
    assert outline(nwords=-1) == INVALID
    assert outline(sel=p, M=0) == OK                                      # nothing selected: no launch


# ------------------------------------------------------------------------------------------ command line
def _tree(tmp_path, frames=2, json_frames=2, segmentation=True):
    data = tmp_path / "ICDAR15_frames" / "Video_9_1_1"
    data.mkdir(parents=True)
    rng = np.random.RandomState(3)
    for i in range(frames):
        Image.fromarray(rng.randint(0, 256, (40, 64, 3)).astype(np.uint8)).save(str(data / ("%d.png" % (i + 1))))
    out = tmp_path / "out"
    (out / "jsons").mkdir(parents=True)
    obj = {"points": [5, 5, 50, 5, 50, 30, 5, 30], "ID": 4, "transcription": "abc"}
    if segmentation:
        obj["segmentation"] = [[[5, 5], [50, 5], [50, 30], [5, 30]]]
    if json_frames is not None:
        tracks = {str(i + 1): ([obj] if i == 0 else []) for i in range(json_frames)}
        with open(str(out / "jsons" / "Video_9_1_1.json"), "w") as fp:
            json.dump(tracks, fp)
    return str(tmp_path / "ICDAR15_frames"), str(out)


@pytest.mark.parametrize("kw,word", [({"json_frames": None}, "not found"), ({"json_frames": 3}, "2 frames but results for 3"),
                                     ({"segmentation": False}, "segmentation")])
def test_command_line_errors_exit_2_and_name_the_video(tmp_path, capsys, kw, word):
    from gomatching_amd import show
    data, out = _tree(tmp_path, **kw)
    assert show.main(["--input", data, "--results", out, "--host-draw"]) == 2
    err = capsys.readouterr().err
    assert "Video_9_1_1" in err and word in err
    assert not os.path.exists(os.path.join(out, "results", "Video_9_1_1", "1.png"))


def test_command_line_host_draw_writes_the_library_pixels(tmp_path):
    from gomatching_amd import eval as E
    from gomatching_amd import show
    data, out = _tree(tmp_path)
    assert show.main(["--input", data, "--results", out, "--host-draw", "--voc-size", "37"]) == 0
    with open(os.path.join(out, "jsons", "Video_9_1_1.json")) as fp:
        annotation = show.rows_of_json(json.load(fp))
    paths = E.frame_paths(os.path.join(data, "Video_9_1_1"))
    frames = [E.read_frame(p) for p in paths]
    want = show.draw_clip(frames, [annotation["1"], annotation["2"]], 37, host=True)
    for i, p in enumerate(paths):
        got = E.read_frame(os.path.join(out, "results", "Video_9_1_1", os.path.basename(p)))
        assert np.array_equal(got, want[i])
    assert (want[0] != frames[0]).any() and np.array_equal(want[1], frames[1])
