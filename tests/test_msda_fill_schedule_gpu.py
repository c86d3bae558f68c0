"""GPU: the two fill schedules of the encoder's LDS-window kernel (csrc/msda.hip, bit 2 of gom_msda_set_window).

The overlapped schedule requests a tile's first window in front of the owner part and the other windows in pairs that share the
workgroup's buffer, so a level's lines may be read from a REGION of the buffer while another region is being filled.  What can go
wrong is a read of lines that have not landed (the previous call's bytes, or a neighbour level's) and a region plan that lets two
live windows touch.  The arithmetic of a sample is untouched, so every comparison is `torch.equal`:
  * the window path under the overlapped schedule, under the one-fill-at-a-time schedule and the lane-distributed kernel give the
    same bits, with and without level-1 tiles, for offsets inside the halo, far outside it and outside the map;
  * two calls with different value maps at one shape, on grids of more than two workgroups per CU, each match the lane kernel;
  * the region plan (host replay of the kernel's own function, nothing launched): 8-line aligned, inside the buffer, disjoint
    where live together, and the windows of the old schedule wherever those fit their regions.
"""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
R = 5                                                     # the kernel's halo, pixels
TY, TX = 8, 16                                            # tiles of both kinds
MIXED = [(27, 53), (14, 27), (7, 14), (4, 7)]             # an interior tile with a full halo, partial last tiles, 2 x 2 level-1 tiles
SMALL = [(9, 17), (5, 9), (3, 5), (2, 3)]                 # every window clipped on every side
LONG = [(40, 140), (20, 70), (10, 35), (5, 18)]           # long rows: L1 + L2 nearest its bound
PLAN_ONLY = [[(125, 223), (63, 112), (32, 56), (16, 28)], [(160, 285), (80, 143), (40, 72), (20, 36)],
             [(223, 125), (112, 63), (56, 32), (28, 16)], [(121, 211), (61, 106), (31, 53), (16, 27)]]


def _ops():
    from gomatching_amd import ops
    return ops


def _pyr(shapes):
    ss = torch.as_tensor(shapes, dtype=torch.long)
    lsi = torch.cat((ss.new_zeros((1,)), ss.prod(1).cumsum(0)[:-1]))
    return ss, lsi, int(ss.prod(1).sum())


def _groups(shapes, B, l1):
    return B * 8 * sum(-(-h // TY) * -(-w // TX) * (TY * TX // 8) for h, w in shapes[:2 if l1 else 1])


class _Switches:
    """ops' three window switches, restored on exit."""

    def __enter__(self):
        ops = _ops()
        self.saved = (ops.MSDA_WINDOW, ops.MSDA_WINDOW_L1, ops.MSDA_WINDOW_OVERLAP)
        ops.MSDA_WINDOW = True
        return ops

    def __exit__(self, *exc):
        ops = _ops()
        ops.MSDA_WINDOW, ops.MSDA_WINDOW_L1, ops.MSDA_WINDOW_OVERLAP = self.saved


def _window_call(ops, raw, ref, value, shapes, ss, lsi, B, S, l1, overlap, counter):
    ops.MSDA_WINDOW_L1, ops.MSDA_WINDOW_OVERLAP = l1, overlap
    hw = tuple(shapes[0]) + (tuple(shapes[1]) if l1 else ())
    out = ops.msda_fused(raw, ref, value, S * 640, ss, lsi, B, S, encoder_hw0=hw, fallback_counter=counter)
    return out, int(counter.item())


@pytest.mark.parametrize("scale", [1.0, 2.5, 40.0])
@pytest.mark.parametrize("shapes", [MIXED, SMALL, LONG], ids=["mixed", "small", "long"])
def test_fill_schedules_are_bit_identical(shapes, scale):
    B = 2
    ss, lsi, S = _pyr(shapes)
    g = torch.Generator().manual_seed(int(scale * 10) + S)
    wide = torch.randn(B * S, 640, generator=g).to(DEV)
    raw = torch.randn(B * S, 384, generator=g)
    raw[:, :256] *= scale                                             # offsets in pixels of the sampled level
    if scale == 1.0:
        # an offset below the halo cannot leave a window: floor(x + off) lies within R pixels of floor(x), its second corner R + 1
        # (a handful of the ~10^6 normal draws exceed 5)
        raw[:, :256].clamp_(-(R - 0.01), R - 0.01)
    raw = raw.to(DEV)
    ssd, lsid = ss.to(DEV), lsi.to(DEV)
    counter = torch.zeros((1,), dtype=torch.int32, device=DEV)
    with _Switches() as ops:
        ref = ops.encoder_reference_points(ssd, lsid, S).repeat(B, 1).contiguous()
        lanes = ops.msda_fused(raw, ref, wide[:, 384:], S * 640, ssd, lsid, B, S)      # encoder_hw0=None: the lane-distributed kernel
        assert bool(torch.isfinite(lanes).all())
        for l1 in (True, False):
            new, slow_new = _window_call(ops, raw, ref, wide[:, 384:], shapes, ssd, lsid, B, S, l1, True, counter)
            old, slow_old = _window_call(ops, raw, ref, wide[:, 384:], shapes, ssd, lsid, B, S, l1, False, counter)
            print("l1 %s scale %g: fallback groups new %d old %d of %d" % (l1, scale, slow_new, slow_old, _groups(shapes, B, l1)))
            assert torch.equal(new, lanes), ("overlapped", l1, float((new - lanes).abs().max()))
            assert torch.equal(old, lanes), ("one at a time", l1, float((old - lanes).abs().max()))
            assert torch.equal(new, old)
            groups = _groups(shapes, B, l1)
            assert 0 <= slow_new <= groups and 0 <= slow_old <= groups
            if scale == 1.0:
                assert slow_new == 0 and slow_old == 0, "offsets inside the halo: no group may fall back"
            if scale == 2.5:
                assert slow_new > 0 and slow_old > 0, "offsets of several halos: groups must take the global path"


def test_no_stale_window_between_calls():
    """Value map A, then value map B at the same shape, on 1024 + 256 workgroups (more than two per CU, so regions are reused by
    later workgroups of a launch as well): a region read before its fill landed shows the other map's bytes, or another level's."""
    B = 8
    ss, lsi, S = _pyr(MIXED)
    g = torch.Generator().manual_seed(7)
    raw = torch.randn(B * S, 384, generator=g).to(DEV)
    maps = [torch.randn(B * S, 640, generator=g).to(DEV), (100.0 + torch.randn(B * S, 640, generator=g)).to(DEV)]
    ssd, lsid = ss.to(DEV), lsi.to(DEV)
    counter = torch.zeros((1,), dtype=torch.int32, device=DEV)
    with _Switches() as ops:
        ref = ops.encoder_reference_points(ssd, lsid, S).repeat(B, 1).contiguous()
        lanes = [ops.msda_fused(raw, ref, w[:, 384:], S * 640, ssd, lsid, B, S) for w in maps]
        assert not torch.equal(lanes[0], lanes[1])
        for overlap in (True, False):
            for rnd in range(2):
                for w, want in zip(maps, lanes):
                    got, _ = _window_call(ops, raw, ref, w[:, 384:], MIXED, ssd, lsid, B, S, True, overlap, counter)
                    assert torch.equal(got, want), (overlap, rnd, float((got - want).abs().max()))


def _r8(n):
    return (n + 7) & ~7


@pytest.mark.parametrize("shapes", [MIXED, SMALL, LONG] + PLAN_ONLY, ids=lambda s: "%dx%d" % tuple(s[0]))
def test_region_plan(shapes):
    """Host replay (gom_msda_window_plan) of every tile of both kinds under both schedules."""
    from gomatching_amd import lib
    L = lib.load()
    ss, lsi, S = _pyr(shapes)
    ref = _ops().encoder_reference_points(ss.to(DEV), lsi.to(DEV), S).cpu().numpy()
    shp = ss.numpy().astype(np.int64)
    plan, cap = (ctypes.c_int * 12)(), ctypes.c_int()
    largest = np.zeros((2, 4), int)

    def replay(kind, q_first, q_last, schedule):
        a, z = np.ascontiguousarray(ref[q_first]), np.ascontiguousarray(ref[q_last])
        rc = L.gom_msda_window_plan(shp.ctypes.data_as(ctypes.c_void_p), kind, a.ctypes.data_as(ctypes.c_void_p),
                                    z.ctypes.data_as(ctypes.c_void_p), schedule, plan, ctypes.byref(cap))
        assert rc == 0
        return np.array(list(plan)).reshape(4, 3)                     # per level: first line, width, rows

    for kind in (0, 1):
        Hq, Wq = shapes[kind]
        live_pairs = [(1, 2), (2, 3)] if kind == 0 else [(2, 3)]      # windows that are in the buffer at the same time
        for ty in range(-(-Hq // TY)):
            for tx in range(-(-Wq // TX)):
                y1, x1 = min(ty * TY + TY, Hq) - 1, min(tx * TX + TX, Wq) - 1
                qa, qz = int(lsi[kind]) + ty * TY * Wq + tx * TX, int(lsi[kind]) + y1 * Wq + x1
                old, new = replay(kind, qa, qz, 0), replay(kind, qa, qz, 1)
                CAP = cap.value
                assert CAP == 576
                lines_old, lines_new = old[:, 1] * old[:, 2], new[:, 1] * new[:, 2]
                largest[kind] = np.maximum(largest[kind], lines_old)
                assert (old[:, 0] == 0).all() and (lines_old <= CAP).all()
                for lev in range(kind, 4):
                    start, n = int(new[lev, 0]), int(lines_new[lev])
                    assert start % 8 == 0 and n >= 1 and start + _r8(n) <= CAP, (kind, ty, tx, lev, new)   # fills write groups of 8
                    assert new[lev, 1] <= old[lev, 1] and new[lev, 2] <= old[lev, 2]
                for a, b in live_pairs:
                    ra = (int(new[a, 0]), int(new[a, 0]) + _r8(int(lines_new[a])))
                    rb = (int(new[b, 0]), int(new[b, 0]) + _r8(int(lines_new[b])))
                    assert ra[1] <= rb[0] or rb[1] <= ra[0], (kind, ty, tx, a, b, new)
                # wherever the old windows fit the regions, the new ones are the old ones
                first = 1 if kind == 0 else 2
                fits = lines_old[first] <= CAP - 8 and _r8(int(lines_old[first])) + _r8(int(lines_old[first + 1])) <= CAP
                if kind == 0:
                    fits = fits and _r8(int(lines_old[3])) <= _r8(int(lines_old[1]))
                if fits:
                    assert (new[kind:, 1:] == old[kind:, 1:]).all(), (kind, ty, tx, old, new)
                assert fits, "the pairs fit on every pyramid of this list: L1 + L2 and L2 + L3 stay below 544 lines"
    print("largest windows, lines per level: level-0 tiles %s, level-1 tiles %s" % (largest[0].tolist(), largest[1, 1:].tolist()))
