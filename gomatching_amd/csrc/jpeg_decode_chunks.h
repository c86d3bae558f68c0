// The chunked entropy walk of the JPEG decoder (THE RULE: include/gomatching_hip.h, `gom_jpeg_decode_entropy_chunks_i16`), on top
// of the reader and the Huffman lookup of jpeg_decode_core.h and, like it, written once for the device (csrc/jpeg_decode.hip) and
// for the host (tools/jpeg_decode_chunks_hostcheck.cpp).  A segment is cut into chunks; a lane walks a chunk from a walk state
// (GomJcPoint) and reports the state at which the next chunk begins.  Equal entry states give equal walks: everything below is a
// function of the entry state and the bytes alone.
// Like the core it walks bytes nobody vouches for, and here from positions that are guesses: every read is bounded by the
// segment's end, every table index masked, every block index checked before the store, and every loop consumes at least one bit
// per turn or ends.
#pragma once
#include "jpeg_decode_core.h"

#define GOM_JC_MIN_CHUNK 16
#define GOM_JC_MAX_CHUNK 4096
#define GOM_JC_MAX_LANES 256                                  // chunks of a span, and so the bound of the settling loop
#define GOM_JC_STAGE_BYTES 65536                              // of a span, staged in LDS
#define GOM_JC_CHUNK_OK(cb) ((cb) >= GOM_JC_MIN_CHUNK && (cb) <= GOM_JC_MAX_CHUNK && ((cb) & ((cb) - 1)) == 0)
#define GOM_JC_LANES(cb) (GOM_JC_STAGE_BYTES / (cb) < GOM_JC_MAX_LANES ? GOM_JC_STAGE_BYTES / (cb) : GOM_JC_MAX_LANES)

// The walk state at a symbol boundary: the stuffed byte that holds the next unread bit and the bits of it already read, the
// block slot within the MCU, the zigzag index (0: the block's DC symbol comes next).
struct GomJcPoint {
    long byte;
    int bit, slot, k;
};

GOM_JD_FN bool gom_jc_same(const GomJcPoint& a, const GomJcPoint& b) {
    return a.byte == b.byte && a.bit == b.bit && a.slot == b.slot && a.k == b.k;
}

// What does not change over a segment's walk.  start / end are clamped as gom_jd_open clamps them.
struct GomJcSeg {
    const uint8_t* p;
    long nbytes, start, end, base;                            // base: start rounded down to 4, where chunk 0 begins
    const int32_t* set;
    int nslots, lum;                                          // blocks of an MCU; luminance blocks of an MCU (hs vs)
    long blocks;                                              // cnt MCUs' blocks
};

// false: a descriptor whose MCUs do not fit the frame (the serial walk answers it with status 1)
GOM_JD_FN bool gom_jc_segment(GomJcSeg& sg, const uint8_t* p, long nbytes, const GomJdDesc& d, const int32_t* set, const GomJdGeom& g) {
    sg.p = p;
    sg.nbytes = nbytes;
    sg.start = gom_jd_clampl(d.start, 0, nbytes);
    sg.end = gom_jd_clampl(d.end, sg.start, nbytes);
    sg.base = sg.start & ~3L;
    sg.set = set;
    sg.lum = g.ncomp == 3 ? g.hs * g.vs : 1;
    sg.nslots = g.ncomp == 3 ? sg.lum + 2 : 1;
    const long total = (long)g.MH * g.MW;
    if (d.m0 < 0 || d.cnt < 1 || d.m0 > total || d.cnt > total - d.m0) return false;
    sg.blocks = d.cnt * sg.nslots;
    return true;
}

GOM_JD_FN long gom_jc_chunks(const GomJcSeg& sg, int chunk_bytes) { return (sg.end - sg.base + chunk_bytes - 1) / chunk_bytes; }

// the frame's block of the segment's `ordinal`-th block (as gom_jd_walk_segment computes it), or -1
GOM_JD_FN long gom_jc_block_index(const GomJdGeom& g, const GomJcSeg& sg, long m0, long ordinal) {
    if (ordinal < 0 || ordinal >= sg.blocks) return -1;       // (so that 32 bits hold everything below: gom_jd_geometry's sizes)
    const unsigned o = (unsigned)ordinal, ns = (unsigned)sg.nslots;
    const unsigned m = (unsigned)m0 + o / ns;
    const int slot = (int)(o % ns);
    const int my = (int)(m / (unsigned)g.MW), mx = (int)(m % (unsigned)g.MW);
    const int c = slot < sg.lum ? 0 : slot - sg.lum + 1;
    const int h = c == 0 ? g.hs : 1, v = c == 0 ? g.vs : 1;
    const int by = c == 0 ? slot / g.hs : 0, bx = c == 0 ? slot % g.hs : 0;
    const long first = c == 0 ? g.first[0] : (c == 1 ? g.first[1] : g.first[2]);
    const int bw = c == 0 ? g.bw[0] : (c == 1 ? g.bw[1] : g.bw[2]);
    const long bi = first + (long)(my * v + by) * bw + (mx * h + bx);
    return (bi >= 0 && bi < g.nblk) ? bi : -1;
}

// A reader at a point.  `win` mirrors bytes [win_lo, win_hi) as in GomJdState.
GOM_JD_FN void gom_jc_seek(GomJdState& s, const GomJcSeg& sg, const uint8_t* win, long win_lo, long win_hi, const GomJcPoint& at) {
    gom_jd_open(s, sg.p, sg.nbytes, gom_jd_clampl(at.byte, sg.start, sg.end), sg.end);
    s.win = win;
    s.win_lo = win_lo;
    s.win_hi = win_hi;
    gom_jd_fill(s);
    if (at.bit & 7) gom_jd_take(s, at.bit & 7);
    s.status = GOM_JD_OK;
}

// no data bit is left unread (zeros behind the data may be)
GOM_JD_FN bool gom_jc_dry(const GomJdState& s) { return s.fake > 0 && s.n <= s.fake; }

// The reader's place as (byte, bit): the unread data bits are stepped back over, whole stuffed bytes at a time (0xFF 0x00 is one).
// A dry reader stands at the segment's end.
GOM_JD_FN void gom_jc_where(const GomJdState& s, const GomJcSeg& sg, long& byte, int& bit) {
    if (gom_jc_dry(s)) {
        byte = sg.end;
        bit = 0;
        return;
    }
    const int q = s.n - s.fake;                               // 0 .. 32
    long at = s.pos;
    for (int i = (q + 7) >> 3; i > 0 && at > sg.start; --i)
        at -= (at - 2 >= sg.start && gom_jd_byte(s, at - 1) == 0u && gom_jd_byte(s, at - 2) == 0xFFu) ? 2 : 1;
    byte = at;
    bit = (8 - (q & 7)) & 7;
}

// The guess a lane starts from: the chunk's first bit (a 0x00 behind the previous chunk's 0xFF is skipped), slot 0, index 0.
GOM_JD_FN GomJcPoint gom_jc_guess(const GomJcSeg& sg, long chunk_start) {
    GomJcPoint at;
    at.byte = gom_jd_clampl(chunk_start, sg.start, sg.end);
    if (at.byte > sg.start && at.byte < sg.end && sg.p[at.byte] == 0u && sg.p[at.byte - 1] == 0xFFu) at.byte += 1;
    at.bit = at.slot = at.k = 0;
    return at;
}

// What a chunk's walk yields for the scans: the blocks that begin in it and the sums of their DC differences (mod 2^32).
struct GomJcTotals {
    int blocks;
    uint32_t dc0, dc1, dc2;                                   // (scalars: they stay in registers)
};

// What the write walk needs beyond the entry state.
struct GomJcWrite {
    long ordinal;                                             // of the first block that begins in the chunk
    uint32_t pred0, pred1, pred2;                             // the DC predictors in front of it
    long m0;
    long limit;                                               // the descriptor's, for gom_jd_close
    int rst;
    int16_t* out;                                             // the frame's coefficients (zero where the walk stores nothing)
};

// A chunk's walk from `at` to the first symbol boundary at or behind `stop`.
//   WRITE false (cold walk, settling): -> exit, tot.  An invalid code costs one bit, a DC category is taken mod 16, an index above
//     63 ends the block: a fixed rule, since the guess is discarded unless it was the truth (and then none of the three happens
//     in a clean stream).
//   WRITE true (the entry is the truth): the blocks that begin in the chunk are stored at their places, the last one to its end
//     behind `stop`; the tail of a block that began earlier is read as above and belongs to the lane that began it.  Anything but
//     GOM_JD_OK inside an owned block comes back in `status`; the lane that ends the segment's last block sets `closed` to
//     gom_jd_close's answer.
template <bool WRITE>
GOM_JD_FN void gom_jc_walk(const GomJcSeg& sg, const GomJdGeom& g, const uint8_t* win, long win_lo, long win_hi, const GomJcPoint& at,
                           long stop, GomJcPoint& exit, GomJcTotals& tot, GomJcWrite& w, int& status, int& closed) {
    const unsigned char* zz = gom_jd_zigzag();
    GomJdState s;
    gom_jc_seek(s, sg, win, win_lo, win_hi, at);
    int slot = (at.slot >= 0 && at.slot < sg.nslots) ? at.slot : 0, k = at.k & 63;
    tot.blocks = 0;
    tot.dc0 = tot.dc1 = tot.dc2 = 0;
    exit = at;
    bool own = false, reached = false;                        // reached: the place is at or behind `stop` (it only moves on)
    long bi = -1;
    for (;;) {
        // the place is at most pos less the unread data bytes (a stuffed byte is one or two): below `stop`, no need to look
        if (!reached && (s.pos - ((s.n - s.fake + 7) >> 3) >= stop || gom_jc_dry(s))) {
            gom_jc_where(s, sg, exit.byte, exit.bit);
            reached = exit.byte >= stop;
        }
        if (reached && !(WRITE && own)) break;
        const int c = slot < sg.lum ? 0 : slot - sg.lum + 1;
        bool done = false;                                    // the block ends with this symbol
        if (k == 0) {
            if (WRITE) {
                if (w.ordinal >= sg.blocks) break;
                own = true;
                bi = gom_jc_block_index(g, sg, w.m0, w.ordinal);
            }
            int size = gom_jd_symbol(s, sg.set, sg.set[GOM_JD_SET_COMP + c]);
            if (WRITE) {
                if (s.status == GOM_JD_OK && (size > 11 || bi < 0)) s.status = GOM_JD_BAD_CODE;
                if (s.status != GOM_JD_OK) break;
            } else if (s.status == GOM_JD_BAD_CODE) {
                gom_jd_take(s, 1);
            }
            const int diff = gom_jd_receive(s, size & 15);
            if (WRITE) {
                if (s.status != GOM_JD_OK) break;
                w.pred0 += c == 0 ? (uint32_t)diff : 0u;
                w.pred1 += c == 1 ? (uint32_t)diff : 0u;
                w.pred2 += c == 2 ? (uint32_t)diff : 0u;
                const uint32_t dc = c == 0 ? w.pred0 : (c == 1 ? w.pred1 : w.pred2);
                w.out[bi * 64] = (int16_t)((int)((dc + 32768u) & 65535u) - 32768);
            } else {
                tot.blocks += 1;
                tot.dc0 += c == 0 ? (uint32_t)diff : 0u;
                tot.dc1 += c == 1 ? (uint32_t)diff : 0u;
                tot.dc2 += c == 2 ? (uint32_t)diff : 0u;
            }
            k = 1;
        } else {
            const bool strict = WRITE && own;
            const int rs = gom_jd_symbol(s, sg.set, sg.set[GOM_JD_SET_COMP + 4 + c]);
            if (strict) {
                if (s.status != GOM_JD_OK) break;
            } else if (s.status == GOM_JD_BAD_CODE) {
                gom_jd_take(s, 1);
            }
            const int r = rs >> 4, sz = rs & 15;
            if (sz) {
                k += r;
                if (k > 63) {
                    if (strict) {
                        s.status = GOM_JD_INDEX;
                        break;
                    }
                    done = true;
                } else {
                    const int val = gom_jd_receive(s, sz);
                    if (strict) {
                        if (s.status != GOM_JD_OK) break;
                        w.out[bi * 64 + zz[k]] = (int16_t)val;
                    }
                    done = ++k > 63;
                }
            } else if (r == 15) {
                k += 16;
                if (k > 63) {
                    if (strict) {
                        s.status = GOM_JD_INDEX;
                        break;
                    }
                    done = true;
                }
            } else {
                done = true;
            }
        }
        if (!(WRITE && own)) s.status = GOM_JD_OK;            // a guess's trouble is nobody's
        if (done) {
            slot = slot + 1 == sg.nslots ? 0 : slot + 1;
            k = 0;
            if (WRITE && own) {
                own = false;
                w.ordinal += 1;
                if (w.ordinal == sg.blocks) {
                    closed = gom_jd_close(s, sg.nbytes, w.limit, w.rst);
                    break;
                }
            }
        }
    }
    exit.slot = slot;
    exit.k = k;
    if (WRITE && s.status != GOM_JD_OK) status = s.status;
}
