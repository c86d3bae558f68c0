"""GPU: the mask kernels of scoring (csrc/mask_pairs.hip) against tests/mask_statement.py, bit for bit -- the two fill kernels
against `fill_contours` / `rle_decode` (hand cases, seeded contours, boxes on word boundaries, one-word and very wide masks),
the count / emit pair against `mask_pairs_statement` (every detection count around the wave size, empty frames, disjoint
boxes, keys, a value exactly at the threshold), and the command line through the kernels against --host-iou."""
import functools
import os

import numpy as np
import pytest
import torch

import mask_statement as ms
import score_json_cases as cases

pytestmark = pytest.mark.gpu

H, W = 64, 96


@functools.lru_cache(maxsize=None)
def _reference():
    """The seeded contours and their statement images, computed once and shared (never modified)."""
    contours = ms.random_contours(200, H, W)
    imgs = [ms.fill_contours([c], H, W) for c in contours]
    for i in imgs:
        i.setflags(write=False)
    return contours, imgs


def _images(words, area, mset):
    """The device buffers of a filled set -> (bool [N, H, W], areas)."""
    words = words.cpu().numpy().view(np.uint32)
    out = np.zeros((mset.N, mset.H, 32 * ((mset.W + 31) // 32)), dtype=bool)
    for k in range(mset.N):
        y0, y1, wx0, wx1 = (int(v) for v in mset.boxes[k])
        if y1 > y0 and wx1 > wx0:
            w = words[int(mset.woff[k]):int(mset.woff[k + 1])].reshape(y1 - y0, wx1 - wx0)
            out[k, y0:y1, 32 * wx0:32 * wx1] = np.unpackbits(w.view(np.uint8), axis=1, bitorder="little").astype(bool)
    assert not out[:, :, mset.W:].any()
    return out[:, :, :mset.W], area.cpu().numpy()


def _fill(specs, h, w):
    from gomatching_amd import score_json as sj
    mset = sj.MaskSet(specs, h, w)
    words, area, _, _ = sj.device_fill(mset, torch.device("cuda", torch.cuda.current_device()))
    return _images(words, area, mset)


def _check_fill(specs, h, w, want):
    got, area = _fill(specs, h, w)
    for k, img in enumerate(want):
        assert np.array_equal(got[k], img), k
        assert int(area[k]) == int(img.sum()), k


def test_fill_polygons_hand_cases():
    for contours, h, w, pixels in ms.HAND_CASES:
        want = np.zeros((h, w), dtype=bool)
        for x, y in pixels:
            want[y, x] = True
        _check_fill([("poly", [np.asarray(c) for c in contours])], h, w, [want])


def test_fill_polygons_random_contours():
    contours, imgs = _reference()
    specs = [("poly", [c]) for c in contours]
    want = list(imgs)
    specs += [("poly", [contours[0], contours[1], contours[2]]), ("poly", [])]     # a union of three; a mask without contours
    want += [imgs[0] | imgs[1] | imgs[2], np.zeros((H, W), dtype=bool)]
    _check_fill(specs, H, W, want)


def test_fill_rle_random_masks_and_mixed_sets():
    contours, imgs = _reference()
    rng = np.random.RandomState(2)
    masks = [imgs[k] for k in range(0, 60, 3)] + [np.zeros((H, W), dtype=bool), np.ones((H, W), dtype=bool), rng.rand(H, W) < 0.5]
    _check_fill([("rle", ms.rle_encode(m)) for m in masks], H, W, masks)
    # both kinds in one set: one launch of each kernel over its own masks
    specs, want = [], []
    for k in range(12):
        if k % 3 == 1:
            specs.append(("rle", ms.rle_encode(imgs[k])))
        else:
            specs.append(("poly", [contours[k]]))
        want.append(imgs[k])
    _check_fill(specs, H, W, want)


@pytest.mark.parametrize("w", [70, 96])
def test_fill_boxes_on_word_boundaries(w):
    h = 6
    edges = [0, 31, 32, 33, 63, 64, w - 1]
    specs, want = [], []
    for x0 in edges:
        for x1 in edges:
            if x1 < x0:
                continue
            img = np.zeros((h, w), dtype=bool)
            img[1:4, x0:x1 + 1] = True
            specs.append(("poly", [np.asarray([[x0, 1], [x1, 1], [x1, 3], [x0, 3]])]))
            specs.append(("rle", ms.rle_encode(img)))
            want += [img, img]
    assert np.array_equal(ms.fill_contours(specs[2][1], h, w), want[2])           # (the rectangles are what the rule gives)
    _check_fill(specs, h, w, want)
    # a slanted polygon that leaves the image on the right: the last word is cut at W - 1
    c = np.asarray([[w - 30, 0], [w + 15, 2], [w - 3, 5], [w - 40, 4]])
    _check_fill([("poly", [c])], h, w, [ms.fill_contours([c], h, w)])


@pytest.mark.parametrize("h", [3, 6])
def test_fill_one_word_and_very_wide_masks(h):
    """2100 pixels are 66 words: with 3 rows a mask has more words than a wave has lanes (the pair kernel's stride wraps),
    with 6 rows more than a fill block has threads."""
    w = 2100
    wide = np.asarray([[3, 0], [2090, 1], [2099, h - 1], [40, h - 1]])
    thin = np.asarray([[70, 0], [75, h - 1], [68, 1]])                              # inside word 2
    imgs = [ms.fill_contours([wide], h, w), ms.fill_contours([thin], h, w)]
    specs = [("poly", [wide]), ("poly", [thin]), ("rle", ms.rle_encode(imgs[0])), ("rle", ms.rle_encode(imgs[1]))]
    from gomatching_amd import score_json as sj
    mset = sj.MaskSet(specs, h, w)
    assert mset.boxes[0].tolist() == [0, h, 0, 66] and mset.boxes[1].tolist()[2:] == [2, 3]
    _check_fill(specs, h, w, imgs + imgs)
    # and the pairs of the wide masks: every word of 66 x h takes part
    gs, ds = sj.MaskSet(specs[2:], h, w), sj.MaskSet(specs[:2], h, w)
    got = sj.device_mask_pairs(gs, ds, [0, 2], [0, 2], [0, 0], [0, 0], 0.001)
    wc, kept, _ = ms.mask_pairs_statement(imgs, imgs, [0, 2], [0, 2], [0, 0], [0, 0], 0.001)
    _same_pairs(got, wc, kept)
    assert [v for _, _, v in kept if v == 1.0] == [1.0, 1.0]


def _same_pairs(got, counts, kept):
    assert got[0].dtype == np.int32 and got[1].dtype == np.int32 and got[2].dtype == np.float64
    assert np.array_equal(got[0], counts)
    assert got[1].tolist() == [j for _, j, _ in kept]
    assert got[2].tobytes() == np.asarray([v for _, _, v in kept], dtype=np.float64).tobytes()


@functools.lru_cache(maxsize=None)
def _pairs_video():
    """Frames with 0, 1, 63, 64, 65 and 130 detections against 3 ground-truth masks each, a frame with detections and no
    ground truth, and a frame of hand cases: a pair at exactly 0.5, disjoint boxes, no shared pixel inside boxes that meet."""
    contours, imgs = _reference()
    rng = np.random.RandomState(17)
    gt_specs, gt_imgs, det_specs, det_imgs, gt_off, det_off = [], [], [], [], [0], [0]
    k = 0
    for nd in (0, 1, 63, 64, 65, 130):
        for _ in range(3):
            g = int(rng.randint(0, 200))
            gt_specs.append(("rle", ms.rle_encode(imgs[g])))
            gt_imgs.append(imgs[g])
        for _ in range(nd):
            det_specs.append(("rle", ms.rle_encode(imgs[k % 200])) if k % 11 == 5 else ("poly", [contours[k % 200]]))
            det_imgs.append(imgs[k % 200])
            k += 1
        gt_off.append(len(gt_specs))
        det_off.append(len(det_specs))
    for _ in range(4):                                             # detections without ground truth
        det_specs.append(("poly", [contours[k % 200]]))
        det_imgs.append(imgs[k % 200])
        k += 1
    gt_off.append(len(gt_specs))
    det_off.append(len(det_specs))
    hand_gt = [[(0, 0), (29, 0), (29, 9), (0, 9)], [(0, 20), (20, 20), (0, 40)]]
    hand_det = [[(0, 0), (14, 0), (14, 9), (0, 9)],               # half of the first: IoU exactly 0.5
                [(40, 50), (60, 50), (60, 60), (40, 60)],         # boxes disjoint from both
                [(30, 50), (30, 32), (12, 50)]]                   # its box meets the triangle's, its pixels do not
    for c in hand_gt:
        gt_specs.append(("rle", ms.rle_encode(ms.fill_contours([c], H, W))))
        gt_imgs.append(ms.fill_contours([c], H, W))
    for c in hand_det:
        det_specs.append(("poly", [np.asarray(c)]))
        det_imgs.append(ms.fill_contours([c], H, W))
    gt_off.append(len(gt_specs))
    det_off.append(len(det_specs))
    gt_key = rng.randint(0, 2, len(gt_specs)).astype(np.int32)
    det_key = rng.randint(0, 2, len(det_specs)).astype(np.int32)
    gt_key[-2:] = 1
    det_key[-3:] = 1
    return gt_specs, gt_imgs, det_specs, det_imgs, gt_off, det_off, gt_key, det_key


@pytest.mark.parametrize("thr", [0.1, float(np.nextafter(0.5, 0.0)), 0.5])
def test_pairs_equal_the_statement(thr):
    from gomatching_amd import score_json as sj
    gt_specs, gt_imgs, det_specs, det_imgs, gt_off, det_off, gt_key, det_key = _pairs_video()
    gs, ds = sj.MaskSet(gt_specs, H, W), sj.MaskSet(det_specs, H, W)
    counts, kept, eligible = ms.mask_pairs_statement(gt_imgs, det_imgs, gt_off, det_off, gt_key, det_key, thr)
    got = sj.device_mask_pairs(gs, ds, gt_off, det_off, gt_key, det_key, thr)
    _same_pairs(got, counts, kept)
    again = sj.device_mask_pairs(gs, ds, gt_off, det_off, gt_key, det_key, thr)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, again))           # two runs, the same bytes
    host = sj.host_mask_pairs(gs, ds, gt_off, det_off, gt_key, det_key, thr)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, host))
    chunked = sj.device_mask_pairs(gs, ds, gt_off, det_off, gt_key, det_key, thr, max_words=500)     # cut into frame ranges
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, chunked))
    # the hand frame: the pair at exactly 0.5 is kept below 0.5 and not at 0.5; the other two detections never pair
    G = len(gt_specs)
    hand = [(g, j, v) for g, j, v in eligible if g >= G - 2]
    assert (G - 2, 0, 0.5) in hand and all(v == 0.0 for g, j, v in hand if j > 0)
    assert ((G - 2, 0, 0.5) in kept) == (thr < 0.5)
    # (the video exercises what it is meant to: half of the 3 x 323 + 6 pairs have equal keys, and a low threshold keeps many)
    assert len(eligible) > 400 and any(int(gt_key[g]) != 0 for g, _, _ in kept) and (thr > 0.2 or len(kept) > 100)
    assert counts[:3].sum() == 0                                   # the frame without detections


def test_pairs_without_ground_truth():
    from gomatching_amd import ops, score_json as sj
    contours, _ = _reference()
    dev = torch.device("cuda", torch.cuda.current_device())
    ds = sj.MaskSet([("poly", [contours[0]]), ("poly", [contours[1]])], H, W)
    gs = sj.MaskSet([], H, W)
    dw, da, dbx, dwo = sj.device_fill(ds, dev)
    gw, ga, gbx, gwo = sj.device_fill(gs, dev)
    i32 = lambda a: torch.tensor(a, dtype=torch.int32, device=dev)
    counts, det, val = ops.mask_pairs(gw, gbx, gwo, ga, dw, dbx, dwo, da, i32([0, 0]), i32([0, 2]), i32([]), i32([0, 0]), 0.5)
    assert counts.numel() == 0 and det.numel() == 0 and val.numel() == 0
    got = sj.device_mask_pairs(gs, ds, [0, 0], [0, 2], [], [0, 0], 0.5)
    assert len(got[0]) == 0 and len(got[1]) == 0 and len(got[2]) == 0


@pytest.mark.parametrize("protocol", ["bovtext", "artvideo"])
@pytest.mark.parametrize("e2e", [False, True])
def test_command_line_through_the_kernels_equals_host_iou(tmp_path, protocol, e2e):
    from gomatching_amd import score
    write = cases.write_bovtext if protocol == "bovtext" else cases.write_artvideo
    gt, res = write(str(tmp_path / "t"))
    a, b = str(tmp_path / "a.json"), str(tmp_path / "b.json")
    argv = ["--protocol", protocol, "--gt", gt, "--results", res] + (["--e2e"] if e2e else [])
    assert score.main(argv + ["--output", a]) == 0
    assert score.main(argv + ["--host-iou", "--output", b]) == 0
    assert open(a, "rb").read() == open(b, "rb").read()
    assert os.path.getsize(a) > 200
