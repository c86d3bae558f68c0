// The reading of result text (THE RULE: include/gomatching_hip.h, `gom_result_parse_*`), written once for the device
// (csrc/result_parse.hip) and for the host (tools/result_parse_hostcheck.cpp, built with the host compiler and sanitizers): a
// line's bounds, the marks, the canonical integer, the string span, an object's line against its template, a frame's wrapper
// lines.  The bytes are untrusted: every read of `data` goes through `rp_at`, which compares the index with the file's size, and
// every store through an `rp_store_*`, which compares the index with the array's length.  No local arrays, no recursion.
#pragma once
#include <stdint.h>

#include "../../include/gomatching_hip.h"

#if defined(__HIPCC__)
#define GOM_RP_FN __host__ __device__ __forceinline__
#else
#define GOM_RP_FN static inline
#endif

// The file and its lines.
struct GomRpText {
    const unsigned char* data;
    long size;
    const int32_t* line_start;                                 // [L + 1]
    long L;
};

// Where the rows go, with the arrays' lengths in elements.
struct GomRpRows {
    int64_t* ids;
    int32_t* pts;
    unsigned char* has_seg;
    int64_t* t_off;
    int32_t* t_len;
    long cap_n;
    int32_t* poly_xy;
    long cap_p;
};

GOM_RP_FN int rp_at(const GomRpText& t, long i) { return i >= 0 && i < t.size ? (int)t.data[i] : -1; }

// line i = bytes [a, b): clamped into the file, empty for an index outside [0, L)
GOM_RP_FN void rp_line(const GomRpText& t, long i, long& a, long& b) {
    a = b = 0;
    if (i < 0 || i >= t.L) return;
    a = t.line_start[i];
    b = (long)t.line_start[i + 1] - 1;
    if (a < 0) a = 0;
    if (b > t.size) b = t.size;
    if (b < a) b = a;
}

// [a, b) is `indent` spaces, then the bytes of `lit`, then a comma iff `comma`
GOM_RP_FN bool rp_is(const GomRpText& t, long a, long b, int indent, const char* lit, bool comma) {
    int n = 0;
    while (lit[n]) ++n;
    if (b - a != (long)indent + n + (comma ? 1 : 0)) return false;
    for (int i = 0; i < indent; ++i)
        if (rp_at(t, a + i) != ' ') return false;
    for (int i = 0; i < n; ++i)
        if (rp_at(t, a + indent + i) != (unsigned char)lit[i]) return false;
    return !comma || rp_at(t, b - 1) == ',';
}

GOM_RP_FN bool rp_is_object_line(const GomRpText& t, long a, long b) { return rp_is(t, a, b, 8, "{", false); }

GOM_RP_FN bool rp_is_key_line(const GomRpText& t, long a, long b) {
    if (b - a < 5) return false;
    for (int i = 0; i < 4; ++i)
        if (rp_at(t, a + i) != ' ') return false;
    return rp_at(t, a + 4) == '"';
}

// the integer token [a, b) with lo <= value <= hi -> 0 and v, GOM_RP_BAD_PLACE (no number at all) or GOM_RP_BAD_INT
GOM_RP_FN int rp_int(const GomRpText& t, long a, long b, int64_t lo, int64_t hi, int64_t& v) {
    v = 0;
    if (b <= a) return GOM_RP_BAD_PLACE;
    for (long i = a; i < b; ++i) {
        const int c = rp_at(t, i);
        const bool num = (c >= '0' && c <= '9') || c == '-';
        if (!(num || (i > a && (c == '+' || c == '.' || c == 'e' || c == 'E')))) return GOM_RP_BAD_PLACE;
    }
    const bool neg = rp_at(t, a) == '-';
    const long d = a + (neg ? 1 : 0);
    if (d >= b || b - d > 19) return GOM_RP_BAD_INT;
    uint64_t m = 0;
    for (long i = d; i < b; ++i) {
        const int c = rp_at(t, i);
        if (c < '0' || c > '9') return GOM_RP_BAD_INT;
        m = m * 10 + (uint64_t)(c - '0');
    }
    if (rp_at(t, d) == '0' && (b - d > 1 || neg)) return GOM_RP_BAD_INT;
    const uint64_t top = neg ? (uint64_t)0 - (uint64_t)lo : (uint64_t)hi;
    if ((neg && lo >= 0) || (!neg && hi < 0) || m > top) return GOM_RP_BAD_INT;
    v = neg ? (int64_t)((uint64_t)0 - m) : (int64_t)m;
    return 0;
}

// [a, b) is `indent` spaces, `key`, an integer in [lo, hi], a comma iff `comma`
GOM_RP_FN int rp_int_line(const GomRpText& t, long a, long b, int indent, const char* key, bool comma, int64_t lo, int64_t hi,
                          int64_t& v) {
    int n = 0;
    while (key[n]) ++n;
    v = 0;
    if (b - a < (long)indent + n + 1 + (comma ? 1 : 0)) return GOM_RP_BAD_PLACE;
    for (int i = 0; i < indent; ++i)
        if (rp_at(t, a + i) != ' ') return GOM_RP_BAD_PLACE;
    for (int i = 0; i < n; ++i)
        if (rp_at(t, a + indent + i) != (unsigned char)key[i]) return GOM_RP_BAD_PLACE;
    if (comma && rp_at(t, b - 1) != ',') return GOM_RP_BAD_PLACE;
    return rp_int(t, a + indent + n, b - (comma ? 1 : 0), lo, hi, v);
}

// the transcription line: -> 0 with the span [off, off + len) and whether a comma follows the closing quote
GOM_RP_FN int rp_string_line(const GomRpText& t, long a, long b, long& off, int& len, bool& comma) {
    const char* key = "\"transcription\": \"";
    off = 0, len = 0, comma = false;
    if (b - a < 12 + 18 + 1) return GOM_RP_BAD_PLACE;
    for (int i = 0; i < 12; ++i)
        if (rp_at(t, a + i) != ' ') return GOM_RP_BAD_PLACE;
    for (int i = 0; i < 18; ++i)
        if (rp_at(t, a + 12 + i) != (unsigned char)key[i]) return GOM_RP_BAD_PLACE;
    const long p = a + 30;
    long i = p;
    while (i < b) {
        const int c = rp_at(t, i);
        if (c == '\\') {
            i += 2;
        } else if (c == '"') {
            break;
        } else {
            ++i;
        }
    }
    if (i >= b) return GOM_RP_BAD_LINE;
    if (b - i == 2 && rp_at(t, i + 1) == ',') comma = true;
    else if (b - i != 1) return GOM_RP_BAD_PLACE;
    off = p;
    len = (int)(i - p);
    return 0;
}

// the key line of a frame: -> 0 with the key, the form (`empty`: []) and the comma; GOM_RP_BAD_PLACE; GOM_RP_BAD_KEY
GOM_RP_FN int rp_key_line(const GomRpText& t, long a, long b, int64_t& key, bool& empty, bool& comma) {
    key = 0, empty = false, comma = false;
    if (!rp_is_key_line(t, a, b)) return GOM_RP_BAD_PLACE;
    long e = b;
    if (rp_at(t, e - 1) == ',') {
        comma = true;
        --e;
    }
    if (rp_at(t, e - 1) == ']') {
        empty = true;
        --e;
    }
    // `": [` in front of e, after at least one byte of key
    if (e - (a + 5) < 5 || rp_at(t, e - 4) != '"' || rp_at(t, e - 3) != ':' || rp_at(t, e - 2) != ' ' || rp_at(t, e - 1) != '[')
        return GOM_RP_BAD_PLACE;
    const int s = rp_int(t, a + 5, e - 4, 1, 2147483646L, key);
    return s == GOM_RP_BAD_INT ? GOM_RP_BAD_KEY : s;
}

// n of an object of nl lines (0 for a length no template has)
GOM_RP_FN int rp_points_of(long nl) { return nl >= 22 && ((nl - 18) & 3) == 0 ? (int)((nl - 18) >> 2) : 0; }

GOM_RP_FN bool rp_template_len(long nl) { return nl == 14 || nl == 17 || (nl >= 22 && ((nl - 18) & 3) == 0); }

GOM_RP_FN bool rp_is_points_closer(const GomRpText& t, long line) {
    long a, b;
    rp_line(t, line, a, b);
    return rp_is(t, a, b, 12, "]", true);
}

GOM_RP_FN int rp_store_i32(int32_t* p, long cap, long i, int64_t v) {
    if (i < 0 || i >= cap) return GOM_RP_BAD_CAP;
    p[i] = (int32_t)v;
    return 0;
}

// line j of object o (nl lines from line s, nl a template's length, its points from poly_off[o] = poff) against its template;
// the value on it is stored.  next_obj: the mark after the object is an object line.  -> status bits
GOM_RP_FN int rp_object_line(const GomRpText& t, long s, long nl, bool next_obj, long j, long o, long poff,
                             const GomRpRows& r) {
    long a, b;
    rp_line(t, s + j, a, b);
    const int n = rp_points_of(nl);
    const int64_t lo32 = -2147483647L - 1, hi32 = 2147483647L;
    int64_t v;
    if (j == 0) return rp_is(t, a, b, 8, "{", false) ? 0 : GOM_RP_BAD_PLACE;
    if (j == 1) return rp_is(t, a, b, 12, "\"points\": [", false) ? 0 : GOM_RP_BAD_PLACE;
    if (j <= 9) {
        const int st = rp_int_line(t, a, b, 16, "", j < 9, lo32, hi32, v);
        return st ? st : rp_store_i32(r.pts, r.cap_n * 8, o * 8 + (j - 2), v);
    }
    if (j == 10) return rp_is(t, a, b, 12, "]", true) ? 0 : GOM_RP_BAD_PLACE;
    if (j == 11) {
        const int st = rp_int_line(t, a, b, 12, "\"ID\": ", true, -9223372036854775807L - 1, 9223372036854775807L, v);
        if (st) return st;
        if (o < 0 || o >= r.cap_n) return GOM_RP_BAD_CAP;
        r.ids[o] = v;
        return 0;
    }
    if (j == 12) {
        long off;
        int len;
        bool comma;
        const int st = rp_string_line(t, a, b, off, len, comma);
        if (st) return st;
        if (comma != (nl > 14)) return GOM_RP_BAD_PLACE;
        if (o < 0 || o >= r.cap_n) return GOM_RP_BAD_CAP;
        r.t_off[o] = off;
        r.t_len[o] = len;
        r.has_seg[o] = nl > 14 ? 1 : 0;
        return 0;
    }
    if (j == nl - 1) return rp_is(t, a, b, 8, "}", next_obj) ? 0 : GOM_RP_BAD_PLACE;
    if (j == 13) return rp_is(t, a, b, 12, "\"segmentation\": [", false) ? 0 : GOM_RP_BAD_PLACE;
    if (j == nl - 2) return rp_is(t, a, b, 12, "]", false) ? 0 : GOM_RP_BAD_PLACE;
    if (nl == 17) return rp_is(t, a, b, 16, "[]", false) ? 0 : GOM_RP_BAD_PLACE;          // (j == 14)
    if (j == 14) return rp_is(t, a, b, 16, "[", false) ? 0 : GOM_RP_BAD_PLACE;
    if (j == nl - 3) return rp_is(t, a, b, 16, "]", false) ? 0 : GOM_RP_BAD_PLACE;
    const long q = j - 15, p = q >> 2;
    const int part = (int)(q & 3);
    if (part == 0) return rp_is(t, a, b, 20, "[", false) ? 0 : GOM_RP_BAD_PLACE;
    if (part == 3) return rp_is(t, a, b, 20, "]", p < n - 1) ? 0 : GOM_RP_BAD_PLACE;
    const int st = rp_int_line(t, a, b, 24, "", part == 1, lo32, hi32, v);
    return st ? st : rp_store_i32(r.poly_xy, r.cap_p * 2, (poff + p) * 2 + (part - 1), v);
}

// what is checked of an object before its lines: j10 = the offset of the first <12>], among 2 .. min(nl, 64) - 1, or -1
GOM_RP_FN int rp_object_shape(long nl, int j10) {
    if (j10 < 0) return GOM_RP_BAD_PLACE;
    if (j10 != 10) return GOM_RP_BAD_POINTS;
    return rp_template_len(nl) ? 0 : GOM_RP_BAD_PLACE;
}

// The marks, as the emit call lays them out.
struct GomRpMarks {
    const int32_t* mark_line;                                  // [N + F + 1], the last entry = L - 1
    const int32_t* obj_mark;                                   // [N]
    const int32_t* frame_mark;                                 // [F]
    const int32_t* frame_rows;                                 // [F + 1]
    long N, F;
};

GOM_RP_FN long rp_clampl(long v, long lo, long hi) { return v < lo ? lo : (v > hi ? hi : v); }

// object o -> its first line, its line count and whether an object line follows it
GOM_RP_FN void rp_object_span(const GomRpMarks& m, long L, long o, long& s, long& nl, bool& next_obj) {
    const long M = m.N + m.F, k = rp_clampl(m.obj_mark[o], 0, M - 1);
    s = rp_clampl(m.mark_line[k], 0, L - 1);
    const long e = rp_clampl(m.mark_line[k + 1], 0, L - 1);
    next_obj = o + 1 < m.N && m.obj_mark[o + 1] == k + 1;
    nl = e - s - (next_obj ? 0 : 1);
    if (nl < 0) nl = 0;
}

// the wrapper lines of frame f -> status bits
GOM_RP_FN int rp_frame(const GomRpText& t, const GomRpMarks& m, long f) {
    const long M = m.N + m.F, k = rp_clampl(m.frame_mark[f], 0, M - 1);
    const long kl = m.mark_line[k], e = m.mark_line[k + 1];
    const long x = f + 1 < m.F ? m.mark_line[rp_clampl(m.frame_mark[f + 1], 0, M)] : m.mark_line[M];
    const long r0 = m.frame_rows[f], r1 = m.frame_rows[f + 1];
    const bool last = f == m.F - 1;
    int st = 0;
    if (f == 0 && (kl != 1 || r0 != 0)) st |= GOM_RP_BAD_PLACE;
    long a, b;
    rp_line(t, kl, a, b);
    int64_t key;
    bool empty, comma;
    const int ks = rp_key_line(t, a, b, key, empty, comma);
    if (ks) return st | ks;
    if (key != f + 1) st |= GOM_RP_BAD_KEY;
    if (r1 <= r0) {
        if (!empty || e != kl + 1 || comma != !last) st |= GOM_RP_BAD_PLACE;
    } else {
        rp_line(t, x - 1, a, b);
        if (empty || comma || e != kl + 1 || !rp_is(t, a, b, 4, "]", !last)) st |= GOM_RP_BAD_PLACE;
    }
    return st;
}

// stage 1 of the rule -> status; L as counted
GOM_RP_FN int rp_ends(const unsigned char* data, long size, long L) {
    if (L == 1) return size == 2 && data[0] == '{' && data[1] == '}' ? 0 : GOM_RP_BAD_ENDS;
    return size >= 3 && data[0] == '{' && data[1] == '\n' && data[size - 2] == '\n' && data[size - 1] == '}' ? 0 : GOM_RP_BAD_ENDS;
}
