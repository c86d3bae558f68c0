"""GPU: the kernels of drawing (csrc/overlay.hip) against tests/overlay_statement.py, bit for bit -- the compositor on the
seeded cases (unaligned rows and frames, an empty frame, 70 overlapping instances in one frame, labels inside, across every
image side, outside, empty, 33 and 70 pixels wide, overlapping), in place and out of place, twice; the outline kernel against
Boundary alone, with and without `sel`; and `show.draw_clip` on the device against its host path across uneven chunks."""
import functools

import numpy as np
import pytest
import torch

import mask_statement as ms
import overlay_statement as ov

pytestmark = pytest.mark.gpu


def _dev():
    return torch.device("cuda", torch.cuda.current_device())


def _compose(frames, scene, in_place):
    """The three launches over one case -> (drawn frames, the device's copy of the input frames)."""
    from gomatching_amd import show
    fr = torch.from_numpy(np.array(frames)).to(_dev())
    keep = fr.clone()
    out = fr if in_place else torch.full_like(fr, 7)
    got = show.launch(fr, scene, show.device_arrays(scene, _dev()), out=out)
    assert got is out
    return got.cpu().numpy(), fr.cpu().numpy(), keep.cpu().numpy()


def test_compose_main_case():
    frames, instances, labels, want = ov.case("main")
    scene = ov.scene_of(frames, instances, labels)
    assert scene.F == 3 and (scene.inst_off == [0, 0, 1, 71]).all() and (3 * scene.W) % 4 and (scene.H * scene.W * 3) % 4
    got, src, keep = _compose(frames, scene, in_place=False)
    assert np.array_equal(got, want)
    assert np.array_equal(src, keep)                                      # out of place: the input is left alone
    assert np.array_equal(got[0], frames[0])                              # no instance, no label: byte-identical
    assert (got[1] != frames[1]).any() and (got[2] != frames[2]).any()
    inp, _, _ = _compose(frames, scene, in_place=True)
    assert np.array_equal(inp, got)
    again, _, _ = _compose(frames, scene, in_place=False)
    assert again.tobytes() == got.tobytes()


@pytest.mark.parametrize("name", ["0", "1"])
def test_compose_small_sizes(name):
    frames, instances, labels, want = ov.case(name)
    scene = ov.scene_of(frames, instances, labels)
    for in_place in (False, True):
        got, _, _ = _compose(frames, scene, in_place)
        assert np.array_equal(got, want), in_place


def test_compose_nothing_to_draw_copies():
    frames = ov.case("0")[0]
    scene = ov.scene_of(frames, [[], []], [[], []])
    got, _, _ = _compose(frames, scene, in_place=False)
    assert np.array_equal(got, frames)


@functools.lru_cache(maxsize=None)
def _outlines():
    """The 200 seeded contours of the fill tests and the statement's Boundary of each, computed once."""
    H, W = 64, 96
    contours = ms.random_contours(200, H, W)
    return H, W, contours, [ov.outline_contours([c], H, W) for c in contours]


def _unpack(words, mset):
    out = np.zeros((mset.N, mset.H, 32 * ((mset.W + 31) // 32)), dtype=bool)
    for k in range(mset.N):
        y0, y1, wx0, wx1 = (int(v) for v in mset.boxes[k])
        if y1 > y0 and wx1 > wx0:
            w = words[int(mset.woff[k]):int(mset.woff[k + 1])].reshape(y1 - y0, wx1 - wx0)
            out[k, y0:y1, 32 * wx0:32 * wx1] = np.unpackbits(w.view(np.uint8), axis=1, bitorder="little").astype(bool)
    assert not out[:, :, mset.W:].any()
    return out[:, :, :mset.W]


def test_outline_kernel_equals_boundary_alone():
    from gomatching_amd import ops, score_json as sj
    H, W, contours, want = _outlines()
    mset = sj.MaskSet([("poly", [c]) for c in contours] + [("poly", [contours[0], contours[1]]), ("poly", [])], H, W)
    want = want + [want[0] | want[1], np.zeros((H, W), dtype=bool)]

    def up(a, dtype):
        return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(_dev())
    args = (up(mset.points, np.int32), up(mset.coff, np.int32), up(mset.mcoff, np.int32), up(mset.boxes, np.int32),
            up(mset.woff, np.int64), H, W)
    nwords = int(mset.woff[-1])
    words = torch.full((nwords,), 0x5A5A5A5A, dtype=torch.int32, device=_dev())
    ops.mask_outline_polygons(*args, words)
    got = _unpack(words.cpu().numpy().view(np.uint32), mset)
    for k, img in enumerate(want):
        assert np.array_equal(got[k], img), k
    assert any((ms.fill_contours([c], H, W) != w).any() for c, w in zip(contours[:10], want))   # Boundary is not Fill u Boundary
    # with sel: the unselected masks' words are untouched
    chosen = np.arange(0, mset.N, 3)
    words2 = torch.full((nwords,), 0x5A5A5A5A, dtype=torch.int32, device=_dev())
    ops.mask_outline_polygons(*args, words2, sel=up(chosen, np.int32))
    w1, w2 = words.cpu().numpy(), words2.cpu().numpy()
    for k in range(mset.N):
        a, b = int(mset.woff[k]), int(mset.woff[k + 1])
        if k in chosen:
            assert np.array_equal(w2[a:b], w1[a:b]), k
        else:
            assert (w2[a:b] == 0x5A5A5A5A).all(), k


def test_draw_clip_device_equals_host_across_uneven_chunks():
    from gomatching_amd import show
    H, W, F = 45, 83, 12
    rng = np.random.RandomState(9)
    frames = rng.randint(0, 256, (F, H, W, 3)).astype(np.uint8)
    rows = []
    for f in range(F):
        fr = []
        for k in range(f % 4):                                            # frames without rows among them
            x, y = int(rng.randint(-5, W - 20)), int(rng.randint(-5, H - 10))
            top = [[x + 2 * i, y + (i % 3)] for i in range(25)]
            poly = top + [[px, py + 9] for px, py in reversed(top)]
            fr.append([0] * 8 + [3 * f + k, "word%d" % k, [poly]])
        rows.append(fr)
    host = show.draw_clip(frames, rows, 37, host=True, chunk=5)
    dev = show.draw_clip(frames, rows, 37, host=False, chunk=5)
    assert host.shape == frames.shape and np.array_equal(dev, host)
    assert np.array_equal(host, show.draw_clip(frames, rows, 37, host=True))      # chunking does not change the pixels
    assert np.array_equal(host[0], frames[0]) and (host[1] != frames[1]).any()
