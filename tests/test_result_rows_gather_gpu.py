"""`gom_result_rows_gather_i32` on the GPU: every word equals the composition the offline path runs -- `index_select` of the
ring rows, `scale_xy_` per scale group, `result_rows` -- for permuted and repeated ring rows, scale pairs mixed within one
launch, and coordinates at which a fused or double-rounded multiply would show in the truncated polygon."""
import ctypes

import numpy as np
import pytest
import torch

import result_rows_statement as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CAP, VOC = 257, 37
SCALES = [(1.0, 1.0), (1280 / 1778, 720 / 1000), (0.5, 2.0)]
_cache = {}


def _beside_integers(scale, count, rng):
    """fp32 values x with fl32(x * scale) exactly one ulp below or above an integer (as many as a search of the neighbours of
    k / scale finds; with scale 1 or a power of two every k yields both)."""
    s = np.float32(scale)
    out = []
    for k in rng.integers(-900, 1900, 4 * count).tolist():
        if k == 0:
            continue
        kf = np.float32(k)
        lo, hi = np.nextafter(kf, np.float32(-np.inf)), np.nextafter(kf, np.float32(np.inf))
        x = np.float32(kf / s)
        cands = [x]
        for _ in range(6):
            cands = [np.nextafter(cands[0], np.float32(-np.inf))] + cands + [np.nextafter(cands[-1], np.float32(np.inf))]
        for c in cands:
            p = np.float32(c) * s
            if p == lo or p == hi:
                out.append(np.float32(c))
        if len(out) >= count:
            break
    return np.asarray(out[:count], np.float32)


def _ring():
    """bd [CAP,25,4] f32, recs [CAP,25] int64 and the scale group of every ring row (row r is scaled by SCALES[r % 3])."""
    if "ring" not in _cache:
        rng = np.random.default_rng(77)
        bd = S.mixed(CAP).copy()
        bd[5:40] -= 300.0                                              # negative coordinates (truncation toward zero)
        bd[40:60] = np.round(bd[40:60])                                # exactly integral
        near = 0
        for r in range(60, 160):                                       # x * sx / y * sy one ulp either side of an integer
            sx, sy = SCALES[r % 3]
            xs, ys = _beside_integers(sx, 50, rng), _beside_integers(sy, 50, rng)
            near += len(xs) + len(ys)
            flat_x = bd[r][:, 0::2].copy().reshape(-1)
            flat_y = bd[r][:, 1::2].copy().reshape(-1)
            flat_x[:len(xs)], flat_y[:len(ys)] = xs, ys
            bd[r][:, 0::2], bd[r][:, 1::2] = flat_x.reshape(25, 2), flat_y.reshape(25, 2)
        assert near > 5000
        recs = S.random_recs(CAP, VOC, seed=9)
        recs[3] = VOC - 1                                              # all blank
        recs[4, ::2] = VOC - 1                                         # ids at voc_size - 1 between characters
        recs[6] = 5                                                    # one repeated character
        _cache["ring"] = (bd.astype(np.float32), recs.astype(np.int64))
    return _cache["ring"]


def _picks(n):
    """Ring rows of a launch of n: permuted, with repeats, row 0 and row CAP - 1 included as soon as n allows."""
    rng = np.random.default_rng(1000 + n)
    rows = rng.permutation(CAP)[:n].astype(np.int64)
    if n >= 3:
        rows[0], rows[1], rows[2] = CAP - 1, 0, CAP - 1               # both ends; a row twice
    elif n == 1:
        rows[0] = CAP - 1
    if n >= 100:
        rows[50:70] = rows[20:40]                                      # more repeats
        rows[70:100] = rng.integers(60, 160, 30)                       # the rows built beside the integers
    ids = (np.arange(n, dtype=np.int64) * 5 + 1) + (np.int64(1) << 33) * (np.arange(n, dtype=np.int64) % 3) \
        + (np.int64(1) << 40) * (np.arange(n, dtype=np.int64) % 2)
    return rows, ids


def _composition(bd_d, recs_d, rows, ids, groups):
    """What the offline path runs: select the rows, scale each scale group in place, one `result_rows` launch."""
    from gomatching_amd import ops
    idx = torch.as_tensor(rows).to(DEV)
    bd = bd_d.index_select(0, idx).contiguous()
    for g, (sx, sy) in enumerate(SCALES):
        sel = torch.as_tensor(np.nonzero(groups == g)[0]).to(DEV)
        if len(sel):
            bd[sel] = ops.scale_xy_(bd.index_select(0, sel).contiguous(), sx, sy)
    return ops.result_rows(bd, recs_d.index_select(0, idx).contiguous(), VOC, torch.as_tensor(ids).to(DEV))


@pytest.mark.parametrize("n", [0, 1, 3, 4, 5, 130])
def test_gather_words_equal_the_offline_composition(n):
    from gomatching_amd import ops
    bd, recs = _ring()
    bd_d, recs_d = torch.as_tensor(bd).to(DEV), torch.as_tensor(recs).to(DEV)
    rows, ids = _picks(n)
    groups = rows % 3
    sx = np.asarray([SCALES[g][0] for g in groups], np.float64)
    sy = np.asarray([SCALES[g][1] for g in groups], np.float64)
    desc = ops.result_rows_desc(rows, ids, sx, sy)
    assert desc.shape == (n, 6) and desc.dtype == np.int32 and not desc[:, 5].any()
    got = ops.result_rows_gather(bd_d, recs_d, desc, VOC)
    assert tuple(got.shape) == (n, S.WORDS) and got.dtype == torch.int32
    want = _composition(bd_d, recs_d, rows, ids, groups)
    bad = (got != want).nonzero().cpu().numpy()
    print("n %d: words differing %d of %d; scale groups used %s" % (n, len(bad), want.numel(), sorted(set(groups.tolist()))))
    assert torch.equal(got, want), "first differing (instance, word): %s" % bad[:5].tolist()
    if n >= 100:
        assert len(set(groups.tolist())) == 3                          # the three scale pairs share the launch
        assert len(set(rows.tolist())) < n and 0 in rows and CAP - 1 in rows
        w = got.cpu().numpy()
        assert (w[:, S.TRACK_ID + 1] != 0).any()                       # ids above 2^32 arrive whole
        assert np.array_equal(w[:, S.TRACK_ID:S.TRACK_ID + 2].copy().view(np.int64).reshape(-1), ids)
        # the scaled polygon, not the ring's: a row scaled by (0.5, 2) differs from its unscaled words
        plain = ops.result_rows(bd_d.index_select(0, torch.as_tensor(rows).to(DEV)).contiguous(),
                                recs_d.index_select(0, torch.as_tensor(rows).to(DEV)).contiguous(), VOC).cpu().numpy()
        assert (w[groups == 2, :100] != plain[groups == 2, :100]).any()
        assert np.array_equal(w[groups == 0, :S.TRACK_ID], plain[groups == 0, :S.TRACK_ID])    # (1, 1) changes nothing
    # the model's pinned staging as the upload path gives the same words
    if n == 5:
        staged = []

        def upload(arr):
            staged.append(arr.shape)
            return torch.from_numpy(arr).to(DEV)
        assert torch.equal(ops.result_rows_gather(bd_d, recs_d, desc, VOC, upload=upload), want) and staged == [(5, 6)]


def test_refusals():
    from gomatching_amd import lib, ops
    L = lib.load()
    INVALID = 1
    p = ctypes.c_void_p(0x1000)                                        # non-null, never dereferenced
    W = S.WORDS
    assert L.gom_result_rows_gather_i32(p, p, 8, p, -1, 37, p, W, None) == INVALID          # n < 0
    assert L.gom_result_rows_gather_i32(p, p, 0, p, 4, 37, p, W, None) == INVALID           # cap < 1 with n > 0
    assert L.gom_result_rows_gather_i32(p, p, 8, p, 4, 37, p, W - 1, None) == INVALID       # short ld
    assert L.gom_result_rows_gather_i32(p, p, 8, p, 0, 37, p, W - 1, None) == INVALID       # ... also without work
    assert L.gom_result_rows_gather_i32(None, p, 8, p, 4, 37, p, W, None) == INVALID
    assert L.gom_result_rows_gather_i32(p, None, 8, p, 4, 37, p, W, None) == INVALID
    assert L.gom_result_rows_gather_i32(p, p, 8, None, 4, 37, p, W, None) == INVALID
    assert L.gom_result_rows_gather_i32(p, p, 8, p, 4, 37, None, W, None) == INVALID
    assert L.gom_result_rows_gather_i32(None, None, 0, None, 0, 37, None, W, None) == 0     # n == 0: GOM_OK, nothing launched
    bd = torch.zeros(CAP, 25, 4, device=DEV)
    recs = torch.zeros(CAP, 25, dtype=torch.int64, device=DEV)
    ok = ops.result_rows_desc([0, CAP - 1], [1, 2], 1.0, 1.0)
    assert tuple(ops.result_rows_gather(bd, recs, ok, 37).shape) == (2, W)
    for bad_row in (CAP, -1, 1 << 20):
        with pytest.raises(ValueError):
            ops.result_rows_gather(bd, recs, ops.result_rows_desc([0, bad_row], [1, 2], 1.0, 1.0), 37)
    with pytest.raises(ValueError):
        ops.result_rows_gather(bd, recs, ok.astype(np.int64), 37)
    with pytest.raises(ValueError):
        ops.result_rows_gather(bd, recs, ok[:, :5], 37)
    with pytest.raises(ValueError):
        ops.result_rows_gather(bd, recs.to(torch.int32), ok, 37)
    with pytest.raises(ValueError):
        ops.result_rows_gather(bd.cpu(), recs.cpu(), ok, 37)
