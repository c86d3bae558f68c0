"""GPU: the four-lane layout of the encoder's LDS-window kernel (csrc/msda.hip, bit 3 of gom_msda_set_window).

Four lanes serve a (query, head) pair with 8 channels each instead of eight lanes with 4; the owner's values reach the other
lanes by DPP inside the quad, a wave takes 16 pairs per iteration and decides the fallback per half-wave (an octet of 8 tile
queries, as before).  The arithmetic of a sample is untouched, so every comparison is `torch.equal`:
  * the new layout, the 8-lane layout and the lane-distributed kernel give the same bits, with and without level-1 tiles, under
    both fill schedules, for offsets inside the halo, offsets that leave it for some octets and offsets outside the map -- and
    the two layouts count the same fallback octets;
  * the mixed case holds an iteration with one octet that must fall back next to one that cannot (shown on the host from the
    offsets), so the half-wave path is exercised;
  * tiles whose iterations have fewer than 16 live queries write nothing but their own rows (sentinel-filled output with guards);
  * two calls with different value maps at one shape on more than 512 workgroups each match the lane kernel (stale LDS).
"""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
R = 5                                                     # the kernel's halo, pixels
TY, TX = 8, 16                                            # tiles of both kinds
MIXED = [(27, 53), (14, 27), (7, 14), (4, 7)]             # an interior tile with a full halo, partial last tiles, 2 x 2 level-1 tiles
SMALL = [(9, 17), (5, 9), (3, 5), (2, 3)]                 # every window clipped on every side; last tiles one column wide
LONG = [(40, 140), (20, 70), (10, 35), (5, 18)]           # long rows
HEAD = 3                                                  # the head the mixed iteration is planted in
# The planted iteration of the x 2.5 case, per pyramid: a level-0 tile (ty, tx), the tile row jy that one wave iteration covers (16
# queries), the tile column jx of the query that gets one level-0 sample far outside the tile's window but inside the map, and
# that sample's x offset in pixels.  SMALL: tile (0, 1) is one column wide, so lanes jx >= 1 repeat the tile's first query (the
# kernel clamps dead lanes to it): octet 0 of row 1 holds query (1, 16), octet 1 only repeats of query (0, 16).
PLANT = {"mixed": (0, 0, 0, 12, 30.0), "long": (0, 0, 0, 12, 30.0), "small": (0, 1, 1, 0, -10.0)}
PYRAMIDS = {"mixed": MIXED, "small": SMALL, "long": LONG}


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
    """ops' four window switches, restored on exit."""

    def __enter__(self):
        ops = _ops()
        self.saved = (ops.MSDA_WINDOW, ops.MSDA_WINDOW_L1, ops.MSDA_WINDOW_OVERLAP, ops.MSDA_WINDOW_LANES4)
        ops.MSDA_WINDOW = True
        return ops

    def __exit__(self, *exc):
        ops = _ops()
        ops.MSDA_WINDOW, ops.MSDA_WINDOW_L1, ops.MSDA_WINDOW_OVERLAP, ops.MSDA_WINDOW_LANES4 = self.saved


def _window_call(ops, raw, ref, value, shapes, ss, lsi, B, S, l1, overlap, lanes4, counter):
    ops.MSDA_WINDOW_L1, ops.MSDA_WINDOW_OVERLAP, ops.MSDA_WINDOW_LANES4 = l1, overlap, lanes4
    hw = tuple(shapes[0]) + (tuple(shapes[1]) if l1 else ())
    out = ops.msda_fused(raw, ref, value, S * 640, ss, lsi, B, S, encoder_hw0=hw, fallback_counter=counter)
    return out, int(counter.item())


def _lane_query(shapes, ty, tx, jy, jx):
    """Level-0 pixel (y, x) that lane (jy, jx) of tile (ty, tx) computes: its own where live, the tile's first query where not."""
    H, W = shapes[0]
    y, x = ty * TY + jy, tx * TX + jx
    return (y, x) if y <= min(ty * TY + TY, H) - 1 and x <= min(tx * TX + TX, W) - 1 else (ty * TY, tx * TX)


def _plant(raw, shapes, name, B, S):
    """Make one iteration of head HEAD mixed in every frame: every query of the row gets offsets inside the halo (it cannot fall
    back), then one query gets a level-0 sample that must."""
    ty, tx, jy, jx_slow, off_x = PLANT[name]
    W = shapes[0][1]
    rows = sorted({_lane_query(shapes, ty, tx, jy, jx) for jx in range(TX)})
    for b in range(B):
        for (y, x) in rows:
            raw[b * S + y * W + x, HEAD * 32:HEAD * 32 + 32].clamp_(-(R - 0.01), R - 0.01)
        y, x = _lane_query(shapes, ty, tx, jy, jx_slow)
        raw[b * S + y * W + x, HEAD * 32 + 0] = off_x                 # sample 0 (level 0, point 0): x offset
        raw[b * S + y * W + x, HEAD * 32 + 1] = 0.25                  # ... and y


def _octet_states(raw, shapes, name, b, S):
    """('fast' | 'slow' | None) x 2 for the planted iteration's octets, by sufficient conditions on the offsets alone:
    fast: every offset of every lane's query is below the halo (floor(x + off) stays within R pixels, the second corner R + 1);
    slow: a level-0 sample of a lane's query lies inside the map and, with a pixel to spare, outside the tile's level-0 window
          [x0 - R, x1 + R + 1] (level-0 queries project onto level 0 as themselves; 19 x 27 lines fit the buffer unshrunk)."""
    ty, tx, jy, _, _ = PLANT[name]
    H, W = shapes[0]
    x0, x1 = tx * TX, min(tx * TX + TX, W) - 1
    states = []
    for octet in range(2):
        fast, slow = True, False
        for jx in range(octet * 8, octet * 8 + 8):
            y, x = _lane_query(shapes, ty, tx, jy, jx)
            off = raw[b * S + y * W + x, HEAD * 32:HEAD * 32 + 32].double()
            fast = fast and bool((off.abs() <= R - 0.01).all())
            for p in range(4):                                        # level 0's samples: w_im = x + off_x, h_im = y + off_y
                w_im, h_im = x + float(off[2 * p]), y + float(off[2 * p + 1])
                inside = 1.0 <= w_im <= W - 2.0 and 0.0 <= h_im <= H - 2.0
                left, right = math.floor(w_im) + 1 < x0 - R - 1, math.floor(w_im) > x1 + R + 2
                slow = slow or (inside and (left or right))
        states.append("fast" if fast else "slow" if slow else None)
    return states


@pytest.mark.parametrize("scale", [1.0, 2.5, 40.0])
@pytest.mark.parametrize("name", ["mixed", "small", "long"])
def test_lane_layouts_are_bit_identical(name, scale):
    shapes = PYRAMIDS[name]
    B = 2
    ss, lsi, S = _pyr(shapes)
    g = torch.Generator().manual_seed(int(scale * 10) + S)
    wide = torch.randn(B * S, 640, generator=g).to(DEV)
    raw = torch.randn(B * S, 384, generator=g)
    raw[:, :256] *= scale                                             # offsets in pixels of the sampled level
    if scale == 1.0:
        raw[:, :256].clamp_(-(R - 0.01), R - 0.01)                    # below the halo: no sample can leave a window
    if scale == 2.5:
        _plant(raw, shapes, name, B, S)
        for b in range(B):
            states = _octet_states(raw, shapes, name, b, S)
            assert sorted(states) == ["fast", "slow"], (name, b, states)   # exactly one slow octet in that iteration
    raw = raw.to(DEV)
    ssd, lsid = ss.to(DEV), lsi.to(DEV)
    counter = torch.zeros((1,), dtype=torch.int32, device=DEV)
    with _Switches() as ops:
        ref = ops.encoder_reference_points(ssd, lsid, S).repeat(B, 1).contiguous()
        lanes = ops.msda_fused(raw, ref, wide[:, 384:], S * 640, ssd, lsid, B, S)      # encoder_hw0=None: the lane-distributed kernel
        assert bool(torch.isfinite(lanes).all())
        for l1 in (True, False):
            for overlap in (True, False):
                new, slow_new = _window_call(ops, raw, ref, wide[:, 384:], shapes, ssd, lsid, B, S, l1, overlap, True, counter)
                old, slow_old = _window_call(ops, raw, ref, wide[:, 384:], shapes, ssd, lsid, B, S, l1, overlap, False, counter)
                groups = _groups(shapes, B, l1)
                print("%s l1 %s overlap %s scale %g: fallback octets four-lane %d eight-lane %d of %d"
                      % (name, l1, overlap, scale, slow_new, slow_old, groups))
                assert torch.equal(new, lanes), ("four lanes", l1, overlap, float((new - lanes).abs().max()))
                assert torch.equal(old, lanes), ("eight lanes", l1, overlap, float((old - lanes).abs().max()))
                assert torch.equal(new, old)
                assert slow_new == slow_old and 0 <= slow_new <= groups
                if scale == 1.0:
                    assert slow_new == 0, "offsets inside the halo: no octet may fall back"
                if scale == 2.5:
                    assert 0 < slow_new < groups, "mixed: some octets take the global path, some do not"


@pytest.mark.parametrize("name", ["mixed", "small"])
def test_dead_lanes_write_nothing(name):
    """Last tiles of 5 (mixed) and 1 (small) live columns: most lanes of their iterations have no query.  The output buffer is
    filled with a sentinel and guarded on both sides: every row of the call equals the lane kernel's, the guards are untouched."""
    shapes = PYRAMIDS[name]
    B, GUARD = 2, 64
    ss, lsi, S = _pyr(shapes)
    g = torch.Generator().manual_seed(11 + S)
    wide = torch.randn(B * S, 640, generator=g).to(DEV)
    raw = torch.randn(B * S, 384, generator=g)
    raw[:, :256] *= 2.5                                               # fast and slow octets alike
    raw = raw.to(DEV)
    ssd, lsid = ss.to(DEV), lsi.to(DEV)
    value = wide[:, 384:]
    with _Switches() as ops:
        from gomatching_amd import lib
        L = lib.load()
        ref = ops.encoder_reference_points(ssd, lsid, S).repeat(B, 1).contiguous()
        lanes = ops.msda_fused(raw, ref, value, S * 640, ssd, lsid, B, S)
        for l1 in (True, False):
            for overlap in (True, False):
                ops.MSDA_WINDOW_L1, ops.MSDA_WINDOW_OVERLAP, ops.MSDA_WINDOW_LANES4 = l1, overlap, True
                hw = tuple(shapes[0]) + (tuple(shapes[1]) if l1 else ())
                ops.msda_fused(raw, ref, value, S * 640, ssd, lsid, B, S, encoder_hw0=hw)      # (sets the library's mask)
                buf = torch.full((B * S + 2 * GUARD, 256), -777.0, dtype=torch.float32, device=DEV)
                out = buf[GUARD:GUARD + B * S]
                h1, w1 = shapes[1] if l1 else (0, 0)
                rc = L.gom_msda_fused_forward_encoder(ops._p(raw), raw.stride(0), ops._p(ref), ops._p(value), S * 640, value.stride(0),
                                                      ops._p(ssd), ops._p(lsid), ops._p(out), B, S, shapes[0][0], shapes[0][1], h1, w1,
                                                      ops._stream())
                assert rc == 0
                torch.cuda.synchronize()
                assert torch.equal(out, lanes), (l1, overlap, float((out - lanes).abs().max()))
                assert bool((buf[:GUARD] == -777.0).all()) and bool((buf[GUARD + B * S:] == -777.0).all())


def test_no_stale_window_between_calls():
    """Value map A, then value map B at the same shape, on 1024 + 256 workgroups (more than two per CU): a region read before its
    fill landed shows the other map's bytes, or another level's."""
    B = 8
    ss, lsi, S = _pyr(MIXED)
    g = torch.Generator().manual_seed(7)
    raw = torch.randn(B * S, 384, generator=g).to(DEV)
    maps = [torch.randn(B * S, 640, generator=g).to(DEV), (100.0 + torch.randn(B * S, 640, generator=g)).to(DEV)]
    ssd, lsid = ss.to(DEV), lsi.to(DEV)
    counter = torch.zeros((1,), dtype=torch.int32, device=DEV)
    assert B * 8 * -(-MIXED[0][0] // TY) * -(-MIXED[0][1] // TX) > 512
    with _Switches() as ops:
        ref = ops.encoder_reference_points(ssd, lsid, S).repeat(B, 1).contiguous()
        lanes = [ops.msda_fused(raw, ref, w[:, 384:], S * 640, ssd, lsid, B, S) for w in maps]
        assert not torch.equal(lanes[0], lanes[1])
        for overlap in (True, False):
            for rnd in range(2):
                for w, want in zip(maps, lanes):
                    got, _ = _window_call(ops, raw, ref, w[:, 384:], MIXED, ssd, lsid, B, S, True, overlap, True, counter)
                    assert torch.equal(got, want), (overlap, rnd, float((got - want).abs().max()))
