// The entropy walk of the JPEG decoder (THE RULE: include/gomatching_hip.h, `gom_jpeg_decode_*`), written once for the device
// (csrc/jpeg_decode.hip) and for the host (tools/jpeg_decode_hostcheck.cpp, built with the host compiler and sanitizers): the
// bit reader, the Huffman lookup, one block's coefficients, a segment's loop over its MCUs and the checks behind it.
// It walks bytes nobody vouches for.  Every read of the data is bounded by the segment's end, which is clamped into the buffer;
// every table index is masked or checked; every coefficient index is checked before the store; a block's index is computed from
// an MCU number that was checked against the frame.  It needs nothing but <stdint.h>.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define GOM_JD_FN __host__ __device__ __forceinline__
#else
#define GOM_JD_FN static inline
#endif

#define GOM_JD_OK 0
#define GOM_JD_PAST_END 1
#define GOM_JD_BAD_CODE 2
#define GOM_JD_INDEX 3
#define GOM_JD_RST 4
#define GOM_JD_LEFT_OVER 5

#define GOM_JD_HT_WORDS 548                                   // look[256], maxcode[18], valoff[18], huffval[256]
#define GOM_JD_SET_COMP (4 * GOM_JD_HT_WORDS)                 // dc table of component 0..3, ac table of component 0..3
#define GOM_JD_SET_QUANT (GOM_JD_SET_COMP + 8)                // quantisers [3][64], natural order
#define GOM_JD_SET_WORDS (GOM_JD_SET_QUANT + 192)
#define GOM_JD_DESC_WORDS 8

struct GomJdGeom {
    int ncomp, hs, vs, MH, MW;
    int bw[3];                                                // block columns of a component's grid
    long first[3];                                            // a component's first block within the frame
    long nblk;                                                // blocks of a frame
};

// false: outside the accepted set (or sizes the index types do not hold)
GOM_JD_FN bool gom_jd_geometry(int H, int W, int ncomp, int hs, int vs, GomJdGeom& g) {
    if (H < 1 || W < 1 || H > 65535 || W > 65535) return false;
    if (!(ncomp == 1 || ncomp == 3)) return false;
    if (!((hs == 1 && vs == 1) || (ncomp == 3 && hs == 2 && (vs == 1 || vs == 2)))) return false;
    g.ncomp = ncomp;
    g.hs = hs;
    g.vs = vs;
    g.MH = (H + 8 * vs - 1) / (8 * vs);
    g.MW = (W + 8 * hs - 1) / (8 * hs);
    long at = 0;
    for (int c = 0; c < 3; ++c) {
        const int h = c == 0 ? hs : 1, v = c == 0 ? vs : 1;
        g.bw[c] = g.MW * h;
        g.first[c] = at;
        if (c < ncomp) at += (long)g.MH * v * g.MW * h;
    }
    g.nblk = at;
    return true;
}

// natural index of the k-th coefficient in zigzag order (a copy per address space)
#define GOM_JD_ZIGZAG                                                                                                           \
    {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,  7,  14, 21, 28, \
     35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63}
static const unsigned char gom_jd_zz_host[64] = GOM_JD_ZIGZAG;
#if defined(__HIPCC__)
static __constant__ unsigned char gom_jd_zz_device[64] = GOM_JD_ZIGZAG;
#endif
GOM_JD_FN const unsigned char* gom_jd_zigzag() {
#if defined(__HIP_DEVICE_COMPILE__)
    return gom_jd_zz_device;
#else
    return gom_jd_zz_host;
#endif
}

// A segment's reader.  `win` (optional) mirrors bytes [win_lo, win_hi) of `p` in faster memory; a read outside it goes to `p`.
struct GomJdState {
    const uint8_t* p;
    const uint8_t* win;
    long win_lo, win_hi;
    long pos, end;
    uint32_t acc;                                             // the low `n` bits are unread, the oldest on top
    int n, fake;                                              // fake: how many of them (the lowest) are zeros behind the data
    int status;
    int dc;                                                   // the DC predictor of the component being walked
};

GOM_JD_FN long gom_jd_clampl(long v, long lo, long hi) { return v < lo ? lo : (v > hi ? hi : v); }

GOM_JD_FN void gom_jd_open(GomJdState& s, const uint8_t* p, long nbytes, long start, long end) {
    s.p = p;
    s.win = nullptr;
    s.win_lo = s.win_hi = 0;
    s.pos = gom_jd_clampl(start, 0, nbytes);
    s.end = gom_jd_clampl(end, s.pos, nbytes);
    s.acc = 0;
    s.n = s.fake = 0;
    s.status = GOM_JD_OK;
    s.dc = 0;
}

GOM_JD_FN unsigned gom_jd_byte(const GomJdState& s, long at) {    // at < s.end, the caller's check
    return (at >= s.win_lo && at < s.win_hi) ? s.win[at - s.win_lo] : s.p[at];
}

// at least 25 unread bits
GOM_JD_FN void gom_jd_fill(GomJdState& s) {
    while (s.n <= 24) {
        unsigned b = 0;
        bool real = false;
        if (s.pos < s.end) {
            b = gom_jd_byte(s, s.pos);
            if (b != 0xFFu) {
                real = true;
                s.pos += 1;
            } else if (s.pos + 1 < s.end && gom_jd_byte(s, s.pos + 1) == 0u) {
                real = true;
                s.pos += 2;
            }
        }
        if (!real) {
            b = 0;
            s.fake += 8;
        }
        s.acc = (s.acc << 8) | b;
        s.n += 8;
    }
}

// k in 1 .. 16 of the unread bits, after a fill
GOM_JD_FN unsigned gom_jd_take(GomJdState& s, int k) {
    const unsigned v = (s.acc >> (s.n - k)) & ((1u << k) - 1u);
    s.n -= k;
    if (s.n < s.fake && s.status == GOM_JD_OK) s.status = GOM_JD_PAST_END;
    return v;
}

// the next symbol of table t (0 .. 3) of a table set; 0 with a status when no code matches
GOM_JD_FN int gom_jd_symbol(GomJdState& s, const int32_t* set, int t) {
    const int32_t* tab = set + (t & 3) * GOM_JD_HT_WORDS;
    gom_jd_fill(s);
    const int e = tab[(s.acc >> (s.n - 8)) & 255u];
    const int len8 = (e >> 8) & 15;
    if (len8 >= 1 && len8 <= 8) {
        gom_jd_take(s, len8);
        return e & 255;
    }
    for (int len = 9; len <= 16; ++len) {
        const int code = (int)((s.acc >> (s.n - len)) & ((1u << len) - 1u));
        if (code <= tab[256 + len]) {
            gom_jd_take(s, len);
            return tab[292 + ((code + tab[274 + len]) & 255)] & 255;
        }
    }
    if (s.status == GOM_JD_OK) s.status = GOM_JD_BAD_CODE;
    return 0;
}

GOM_JD_FN int gom_jd_receive(GomJdState& s, int size) {        // size in 0 .. 15
    if (size == 0) return 0;
    gom_jd_fill(s);
    const int v = (int)gom_jd_take(s, size);
    return (v >> (size - 1)) ? v : v - (1 << size) + 1;
}

// One block of component c (its DC predictor in s.dc) into blk[64] (natural order, zero on entry).  Stops at the first thing
// wrong; s.status says what.
GOM_JD_FN void gom_jd_block(GomJdState& s, const int32_t* set, int c, int16_t* blk) {
    const unsigned char* zz = gom_jd_zigzag();
    const int size = gom_jd_symbol(s, set, set[GOM_JD_SET_COMP + c]);
    if (s.status != GOM_JD_OK) return;
    if (size > 11) {
        s.status = GOM_JD_BAD_CODE;
        return;
    }
    const int diff = gom_jd_receive(s, size);
    if (s.status != GOM_JD_OK) return;
    s.dc += diff;
    blk[0] = (int16_t)(((s.dc + 32768) & 65535) - 32768);
    int k = 1;
    while (k < 64) {
        const int rs = gom_jd_symbol(s, set, set[GOM_JD_SET_COMP + 4 + c]);
        if (s.status != GOM_JD_OK) return;
        const int r = rs >> 4, sz = rs & 15;
        if (sz) {
            k += r;
            if (k > 63) {
                s.status = GOM_JD_INDEX;
                return;
            }
            const int val = gom_jd_receive(s, sz);
            if (s.status != GOM_JD_OK) return;
            blk[zz[k]] = (int16_t)val;
            ++k;
        } else if (r == 15) {
            k += 16;
            if (k > 63) {
                s.status = GOM_JD_INDEX;
                return;
            }
        } else {
            return;
        }
    }
}

// behind a segment that was walked cleanly: whole bytes left over, then the marker that must follow (rst = its second byte, or 0
// for the frame's last segment, which must end where the frame's bytes end: `limit`)
GOM_JD_FN int gom_jd_close(const GomJdState& s, long nbytes, long limit, int rst) {
    if (s.status != GOM_JD_OK) return s.status;
    if (s.n - s.fake >= 8 || s.pos < s.end) return GOM_JD_LEFT_OVER;
    limit = gom_jd_clampl(limit, s.end, nbytes);
    if (rst) {
        if (!(s.end + 2 <= limit && s.p[s.end] == 0xFFu && s.p[s.end + 1] == (unsigned)(rst & 255))) return GOM_JD_RST;
    } else if (s.end != limit) {
        return GOM_JD_RST;
    }
    return GOM_JD_OK;
}

// A segment's descriptor, words {start, end, limit, first MCU, MCUs, frame, table set, RSTn} (scalars: they stay in registers)
struct GomJdDesc {
    long start, end, limit, m0, cnt, frame, set;
    int rst;
};

GOM_JD_FN GomJdDesc gom_jd_desc(const int64_t* w) {
    GomJdDesc d;
    d.start = (long)w[0];
    d.end = (long)w[1];
    d.limit = (long)w[2];
    d.m0 = (long)w[3];
    d.cnt = (long)w[4];
    d.frame = (long)w[5];
    d.set = (long)w[6];
    d.rst = (int)w[7];
    return d;
}

// A segment.  `leader` walks the bits; every caller runs the same loop: begin(state) before a block (blk must be zero behind
// it), emit(block index within the frame) behind it.  On the host there is one caller and it leads.  -> the segment's status
// (the leader's).
template <typename Begin, typename Emit>
GOM_JD_FN int gom_jd_walk_segment(const uint8_t* p, long nbytes, const GomJdDesc& d, const int32_t* set, const GomJdGeom& g,
                                  bool leader, int16_t* blk, Begin begin, Emit emit) {
    GomJdState s;
    gom_jd_open(s, p, nbytes, d.start, d.end);
    const long total = (long)g.MH * g.MW;
    int pred0 = 0, pred1 = 0, pred2 = 0;                      // the DC predictors (scalars: everything stays in registers)
    if (d.m0 < 0 || d.cnt < 0 || d.m0 > total || d.cnt > total - d.m0) return GOM_JD_PAST_END;
    for (long m = d.m0; m < d.m0 + d.cnt; ++m) {
        const int my = (int)(m / g.MW), mx = (int)(m % g.MW);
        for (int c = 0; c < g.ncomp; ++c) {
            const int h = c == 0 ? g.hs : 1, v = c == 0 ? g.vs : 1;
            const long first = c == 0 ? g.first[0] : (c == 1 ? g.first[1] : g.first[2]);
            const int bw = c == 0 ? g.bw[0] : (c == 1 ? g.bw[1] : g.bw[2]);
            for (int by = 0; by < v; ++by)
                for (int bx = 0; bx < h; ++bx) {
                    begin(s);
                    s.dc = c == 0 ? pred0 : (c == 1 ? pred1 : pred2);
                    if (leader && s.status == GOM_JD_OK) gom_jd_block(s, set, c, blk);
                    pred0 = c == 0 ? s.dc : pred0;
                    pred1 = c == 1 ? s.dc : pred1;
                    pred2 = c == 2 ? s.dc : pred2;
                    const long bi = first + (long)(my * v + by) * bw + (mx * h + bx);
                    if (bi >= 0 && bi < g.nblk) emit(bi);
                }
        }
    }
    return gom_jd_close(s, nbytes, d.limit, d.rst);
}
