"""GPU: `ops.scene_polygons` (csrc/scene_polygons.hip) over rows the parser left on the device against the arrays of the `Scene`
that `show._scene_of_rows` builds on the host for the same rows: points, coff, mcoff, boxes, woff, inst_off, inst_rgb -- and the
label arrays `ParsedScenes` adds on the host.  Polygons partly and wholly outside the image, empty contours, both channel orders,
a middle range of a longer video."""
import json
import random

import numpy as np
import pytest
import torch

import result_parse_cases as rc
from gomatching_amd import results, show

pytestmark = pytest.mark.gpu
SIZES = ((48, 64), (47, 33))                                   # H, W: 64 x 48 and 33 x 47


def _longer_video():
    """Seven frames: polygons inside, across every edge, wholly outside on every side, empty contours, an empty frame, a
    contour that is one point, negative ids."""
    rng = random.Random(31)
    poly = lambda n, x0, x1, y0, y1: [[rng.randint(x0, x1), rng.randint(y0, y1)] for _ in range(n)]
    o = lambda seg, track: {"points": [1, 2, 3, 4, 5, 6, 7, 8], "ID": track, "transcription": "t%d" % (track % 7),
                            "segmentation": [seg]}
    return {"1": [o(poly(50, 2, 60, 2, 44), 3), o(poly(6, -20, 20, -20, 20), -1)],
            "2": [o(poly(5, 40, 120, 30, 90), 499), o([], 7), o(poly(4, -90, -10, 5, 40), 500)],
            "3": [],
            "4": [o(poly(8, 70, 200, 0, 40), 12), o(poly(8, 0, 60, 50, 300), -501), o(poly(3, 0, 63, -40, -1), 2 ** 40)],
            "5": [o([], 1), o([], 2)],
            "6": [o([[31, 20]], 5), o([[32, 0], [32, 47]], 6), o(poly(50, -1000, 1000, -1000, 1000), 8)],
            "7": [o(poly(7, 0, 32, 0, 46), 3)]}


TILE_EDGE_EMPTY = (255, 256, 511, 512)                         # chunk positions on both sides of the scan's tile edges


def _tile_edge_video():
    """Three frames of 255, 3 and 255 tiny polygons: the chunk 0..3 has 2 * 256 + 1 instances, three tiles of the scan kernel's
    block with a carry between them.  The instances at the chunk positions TILE_EDGE_EMPTY have an empty contour, so the kept
    count and the word offset cross both tile edges with a zero on each side."""
    rng = random.Random(47)
    objects = []
    for k in range(2 * 256 + 1):
        x, y = rng.randint(0, 60), rng.randint(0, 44)
        seg = [] if k in TILE_EDGE_EMPTY else [[x, y], [x + 3, y + 1], [x + 1, y + 3]]
        objects.append({"points": [1, 2, 3, 4, 5, 6, 7, 8], "ID": k % 255, "transcription": "t%d" % (k % 7),
                        "segmentation": [seg]})
    return {"1": objects[:255], "2": objects[255:258], "3": objects[258:]}


def _families():
    skip = ("int32 limits", "long")                           # coordinates beyond 2^20 (tested below); size
    fams = [(n, json.loads(d)) for n, d in rc.clean_cases() if n not in skip]
    for _, a in fams:                                          # a row without a segmentation is not drawn: the others are
        for f in a:
            a[f] = [o for o in a[f] if "segmentation" in o]
    assert sum(len(v) for _, a in fams for v in a.values()) > 60
    return fams + [("longer video", _longer_video())]


def _compare(annotation, f0, f1, H, W, bgr, dev):
    parsed = results.parse_json_device(rc.dumps(annotation), dev)
    assert parsed.status == 0
    rows = show.rows_of_json(annotation)
    want = show._scene_of_rows([rows[str(f + 1)] for f in range(f0, f1)], 37, show.Atlas(), H, W, bgr)
    dims, (arr, face, line, area) = show.ParsedScenes(parsed, 37, show.Atlas(), bgr).chunk(f0, f1, H, W, dev)
    got = [t.cpu().numpy() for t in arr]
    ms = want.mset
    assert (dims.F, dims.H, dims.W) == (want.F, H, W)
    stated = [ms.points.astype(np.int32).reshape(-1, 2), ms.coff.astype(np.int32), ms.mcoff.astype(np.int32),
              ms.boxes.astype(np.int32).reshape(-1, 4), ms.woff.astype(np.int64), want.inst_off, want.inst_rgb.reshape(-1, 3),
              want.label_off, want.label_pos, want.label_glyph, want.label_rgb, want.glyph_wh.astype(np.int32),
              want.glyph_woff.astype(np.int64), want.glyph_words.astype(np.uint32).view(np.int32)]
    names = ("points", "coff", "mcoff", "boxes", "woff", "inst_off", "inst_rgb", "label_off", "label_pos", "label_glyph",
             "label_rgb", "glyph_wh", "glyph_woff", "glyph_words")
    for name, g, w in zip(names, got, stated):
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), (name, f0, f1, H, W, bgr)
    assert face.shape[0] == line.shape[0] == int(ms.woff[-1]) and area.shape[0] == ms.N


@pytest.mark.parametrize("H,W", SIZES)
def test_scene_of_parsed_rows_is_the_hosts_scene(H, W):
    dev = torch.device("cuda", torch.cuda.current_device())
    for i, (name, annotation) in enumerate(_families()):
        F = len(annotation)
        if F == 0:
            continue
        _compare(annotation, 0, F, H, W, bool(i % 2), dev)


@pytest.mark.parametrize("bgr", (True, False))
def test_a_middle_frame_range_of_a_longer_video(bgr):
    dev = torch.device("cuda", torch.cuda.current_device())
    video = _longer_video()
    for f0, f1 in ((1, 4), (2, 3), (4, 5), (3, 7), (0, 7), (6, 7)):
        for H, W in SIZES:
            _compare(video, f0, f1, H, W, bgr, dev)


def test_a_chunk_longer_than_the_scan_block_crosses_its_tile_edges():
    dev = torch.device("cuda", torch.cuda.current_device())
    video = _tile_edge_video()
    assert [len(video[f]) for f in ("1", "2", "3")] == [255, 3, 255]
    flat = [o for f in ("1", "2", "3") for o in video[f]]
    assert [k for k, o in enumerate(flat) if o["segmentation"] == [[]]] == list(TILE_EDGE_EMPTY)
    for f0, f1 in ((0, 3), (1, 3)):
        _compare(video, f0, f1, 48, 64, False, dev)


def test_a_coordinate_beyond_the_limit_raises():
    dev = torch.device("cuda", torch.cuda.current_device())
    for bad in (2 ** 20 + 1, -2 ** 20 - 1):
        video = _longer_video()
        video["4"][1]["segmentation"][0][2][1] = bad
        parsed = results.parse_json_device(rc.dumps(video), dev)
        assert parsed.status == 0
        scenes = show.ParsedScenes(parsed, 37, show.Atlas())
        with pytest.raises(show.ShowError, match="a polygon coordinate beyond"):
            scenes.chunk(3, 4, 48, 64, dev)
        scenes.chunk(0, 3, 48, 64, dev)                        # (the frames without it are drawn)
        rows = show.rows_of_json(video)
        with pytest.raises(show.ShowError, match="a polygon coordinate beyond"):
            show._scene_of_rows([rows["4"]], 37, show.Atlas(), 48, 64, True)
    video = _longer_video()
    video["4"][1]["segmentation"][0][2][1] = 2 ** 20           # the limit itself is drawn
    _compare(video, 3, 4, 48, 64, True, dev)
