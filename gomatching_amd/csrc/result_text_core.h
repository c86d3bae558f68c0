// The formatting of result text (THE RULE: include/gomatching_hip.h, `gom_result_text_*`), written once for the device
// (csrc/result_text.hip) and for the host (tools/result_text_hostcheck.cpp, built with the host compiler and sanitizers): the
// bounded writer, the digit count and the integer print, the pieces of a row and of a frame's wrappers, a row's length and a
// row's emit into a bounded buffer.
// One function both counts and writes: a writer without a buffer only advances, so a length is by construction the length of
// what the same call writes.  Every byte goes through `rt_put`, which compares the index with the writer's cap before the store;
// a table index is checked before the read (`rt_entry`).  No local arrays: digits are stored back to front at their final place.
#pragma once
#include <stdint.h>

#include "../../include/gomatching_hip.h"

#if defined(__HIPCC__)
#define GOM_RT_FN __host__ __device__ __forceinline__
#else
#define GOM_RT_FN static inline
#endif

#define GOM_RT_JSON_PIECES 63                                  // opener, 8 points, id, transcription, ring opener, 50 pairs, closer
#define GOM_RT_XML_PIECES 8                                    // object + id, transcription, end of the tag, 4 points, closer
#define GOM_RT_STAGE_BYTES 6656                                // a row's JSON (at most 6593 bytes with its separator) + 15 of shift

// A bounded writer: byte `pos` is stored iff buf && pos < cap; pos advances either way.
struct GomRtOut {
    unsigned char* buf;
    long cap;
    long pos;
};

// One row's operands.
struct GomRtRow {
    const int32_t* words;                                      // GOM_RESULT_ROWS_WORDS words
    const int64_t* pts;                                        // 8
    const unsigned char* json_tab;                             // [ntab][GOM_RT_ENTRY_BYTES]
    const unsigned char* xml_tab;
    int ntab;
    // a lexicon override (`gom_result_text_*_ov`): with a non-null pointer the transcription piece is these bytes as they are, the
    // row's display form for that stream; null (what `GomRtRow{words, pts, json_tab, xml_tab, ntab}` leaves): the tables, as ever
    const unsigned char* json_ov;
    int json_ov_len;
    const unsigned char* xml_ov;
    int xml_ov_len;
};

GOM_RT_FN void rt_put(GomRtOut& o, unsigned char c) {
    if (o.buf && o.pos >= 0 && o.pos < o.cap) o.buf[o.pos] = c;
    ++o.pos;
}

GOM_RT_FN void rt_spaces(GomRtOut& o, int k) {
    for (int i = 0; i < k; ++i) rt_put(o, ' ');
}

GOM_RT_FN void rt_str(GomRtOut& o, const char* s) {
    for (; *s; ++s) rt_put(o, (unsigned char)*s);
}

GOM_RT_FN int rt_digits_u64(uint64_t m) {
    int d = 1;
    while (m >= 10) {
        m /= 10;
        ++d;
    }
    return d;
}

GOM_RT_FN int rt_digits_u32(uint32_t m) {
    int d = 1;
    while (m >= 10) {
        m /= 10;
        ++d;
    }
    return d;
}

// plain decimal, '-' for a negative value; the magnitude is taken in unsigned arithmetic, so INT64_MIN is no special case
GOM_RT_FN void rt_i64(GomRtOut& o, int64_t v) {
    uint64_t m = v < 0 ? (uint64_t)0 - (uint64_t)v : (uint64_t)v;
    if (v < 0) rt_put(o, '-');
    const int d = rt_digits_u64(m);
    for (int i = d - 1; i >= 0; --i) {
        const long at = o.pos + i;
        if (o.buf && at >= 0 && at < o.cap) o.buf[at] = (unsigned char)('0' + (int)(m % 10));
        m /= 10;
    }
    o.pos += d;
}

GOM_RT_FN void rt_i32(GomRtOut& o, int32_t v) {
    uint32_t m = v < 0 ? (uint32_t)0 - (uint32_t)v : (uint32_t)v;
    if (v < 0) rt_put(o, '-');
    const int d = rt_digits_u32(m);
    for (int i = d - 1; i >= 0; --i) {
        const long at = o.pos + i;
        if (o.buf && at >= 0 && at < o.cap) o.buf[at] = (unsigned char)('0' + (int)(m % 10));
        m /= 10;
    }
    o.pos += d;
}

GOM_RT_FN int64_t rt_track_id(const GomRtRow& r) {
    const uint64_t lo = (uint32_t)r.words[GOM_RR_TRACK_ID], hi = (uint32_t)r.words[GOM_RR_TRACK_ID + 1];
    return (int64_t)(lo | (hi << 32));
}

// true: an emitted character id of the row lies outside the table
GOM_RT_FN bool rt_char_bad(const GomRtRow& r, int c) {
    if (!(((uint32_t)r.words[GOM_RR_EMIT] >> c) & 1u)) return false;
    const int32_t id = r.words[GOM_RR_RECS + c];
    return id < 0 || id >= r.ntab;
}

GOM_RT_FN bool rt_row_bad(const GomRtRow& r) {
    bool bad = false;
    for (int c = 0; c < 25; ++c) bad = bad || rt_char_bad(r, c);
    return bad;
}

// the emitted characters through a table; an id outside the table contributes nothing (and the row is flagged elsewhere)
GOM_RT_FN void rt_transcription(GomRtOut& o, const GomRtRow& r, const unsigned char* tab) {
    const uint32_t emit = (uint32_t)r.words[GOM_RR_EMIT];
    for (int c = 0; c < 25; ++c) {
        if (!((emit >> c) & 1u)) continue;
        const int32_t id = r.words[GOM_RR_RECS + c];
        if (id < 0 || id >= r.ntab) continue;
        const unsigned char* e = tab + (long)id * GOM_RT_ENTRY_BYTES;
        int len = e[0];
        if (len > GOM_RT_ENTRY_BYTES - 1) len = GOM_RT_ENTRY_BYTES - 1;
        for (int i = 0; i < len; ++i) rt_put(o, e[1 + i]);
    }
}

// an override's bytes: a display form of the lexicon, escaped on the host, at most 25 * (GOM_RT_ENTRY_BYTES - 1) of them
GOM_RT_FN void rt_override(GomRtOut& o, const unsigned char* b, int len) {
    if (len > 25 * (GOM_RT_ENTRY_BYTES - 1)) len = 25 * (GOM_RT_ENTRY_BYTES - 1);
    for (int i = 0; i < len; ++i) rt_put(o, b[i]);
}

// ---- JSON: piece s of a row, in stream order.  `sep`: the row is not the first kept row of its frame.
GOM_RT_FN void rt_json_piece(GomRtOut& o, const GomRtRow& r, int s, bool sep) {
    if (s == 0) {
        if (sep) rt_str(o, ",\n");
        rt_spaces(o, 8);
        rt_str(o, "{\n");
        rt_spaces(o, 12);
        rt_str(o, "\"points\": [\n");
    } else if (s <= 8) {
        rt_spaces(o, 16);
        rt_i64(o, r.pts[s - 1]);
        rt_str(o, s < 8 ? ",\n" : "\n");
    } else if (s == 9) {
        rt_spaces(o, 12);
        rt_str(o, "],\n");
        rt_spaces(o, 12);
        rt_str(o, "\"ID\": ");
        rt_i64(o, rt_track_id(r));
        rt_str(o, ",\n");
        rt_spaces(o, 12);
        rt_str(o, "\"transcription\": \"");
    } else if (s == 10) {
        if (r.json_ov) rt_override(o, r.json_ov, r.json_ov_len);
        else rt_transcription(o, r, r.json_tab);
    } else if (s == 11) {
        rt_str(o, "\",\n");
        rt_spaces(o, 12);
        rt_str(o, "\"segmentation\": [\n");
        rt_spaces(o, 16);
        rt_str(o, "[\n");
    } else if (s < 12 + 50) {
        const int p = s - 12;
        rt_spaces(o, 20);
        rt_str(o, "[\n");
        rt_spaces(o, 24);
        rt_i32(o, r.words[GOM_RR_POLY_I32 + 2 * p]);
        rt_str(o, ",\n");
        rt_spaces(o, 24);
        rt_i32(o, r.words[GOM_RR_POLY_I32 + 2 * p + 1]);
        rt_put(o, '\n');
        rt_spaces(o, 20);
        rt_str(o, p < 49 ? "],\n" : "]");
    } else if (s == 62) {
        rt_put(o, '\n');
        rt_spaces(o, 16);
        rt_str(o, "]\n");
        rt_spaces(o, 12);
        rt_str(o, "]\n");
        rt_spaces(o, 8);
        rt_put(o, '}');
    }
}

// ---- XML: piece s of an object, in stream order
GOM_RT_FN void rt_xml_piece(GomRtOut& o, const GomRtRow& r, int s) {
    if (s == 0) {
        rt_spaces(o, 4);
        rt_str(o, "<object ID=\"");
        rt_i64(o, rt_track_id(r));
        rt_str(o, "\" Transcription=\"");
    } else if (s == 1) {
        if (r.xml_ov) rt_override(o, r.xml_ov, r.xml_ov_len);
        else rt_transcription(o, r, r.xml_tab);
    } else if (s == 2) {
        rt_str(o, "\">\n");
    } else if (s < 7) {
        const int i = s - 3;
        rt_spaces(o, 6);
        rt_str(o, "<Point x=\"");
        rt_i64(o, r.pts[2 * i]);
        rt_str(o, "\" y=\"");
        rt_i64(o, r.pts[2 * i + 1]);
        rt_str(o, "\"/>\n");
    } else if (s == 7) {
        rt_spaces(o, 4);
        rt_str(o, "</object>\n");
    }
}

// ---- frame wrappers; `frame` is the absolute 0-based index, `kept` the frame's kept rows
GOM_RT_FN void rt_json_frame_head(GomRtOut& o, long frame, int kept) {
    if (frame > 0) rt_str(o, ",\n");
    rt_spaces(o, 4);
    rt_put(o, '"');
    rt_i64(o, (int64_t)frame + 1);
    rt_str(o, kept > 0 ? "\": [\n" : "\": []");
}

GOM_RT_FN void rt_json_frame_tail(GomRtOut& o, int kept) {
    if (kept > 0) {
        rt_put(o, '\n');
        rt_spaces(o, 4);
        rt_put(o, ']');
    }
}

GOM_RT_FN void rt_xml_frame_head(GomRtOut& o, long frame, int kept) {
    rt_spaces(o, 2);
    rt_str(o, "<frame ID=\"");
    rt_i64(o, (int64_t)frame + 1);
    rt_str(o, kept > 0 ? "\">\n" : "\"/>\n");
}

GOM_RT_FN void rt_xml_frame_tail(GomRtOut& o, int kept) {
    if (kept > 0) {
        rt_spaces(o, 2);
        rt_str(o, "</frame>\n");
    }
}

// a frame's whole length in a stream: wrappers, its rows' bytes and the separators between its kept rows
GOM_RT_FN long rt_json_frame_len(long frame, int kept, long row_bytes) {
    GomRtOut o = {nullptr, 0, 0};
    rt_json_frame_head(o, frame, kept);
    rt_json_frame_tail(o, kept);
    return o.pos + row_bytes + (kept > 1 ? 2L * (kept - 1) : 0L);
}

GOM_RT_FN long rt_xml_frame_len(long frame, int kept, long row_bytes) {
    GomRtOut o = {nullptr, 0, 0};
    rt_xml_frame_head(o, frame, kept);
    rt_xml_frame_tail(o, kept);
    return o.pos + row_bytes;
}

// ---- a whole row, piece after piece (the host's form; the kernel gives a lane a piece): the row's length without a buffer,
// the row's bytes with one.  -> the length; bytes at or past `cap` were not written.
GOM_RT_FN long rt_json_row(const GomRtRow& r, bool sep, unsigned char* buf, long cap) {
    GomRtOut o = {buf, cap, 0};
    for (int s = 0; s < GOM_RT_JSON_PIECES; ++s) rt_json_piece(o, r, s, sep);
    return o.pos;
}

GOM_RT_FN long rt_xml_row(const GomRtRow& r, unsigned char* buf, long cap) {
    GomRtOut o = {buf, cap, 0};
    for (int s = 0; s < GOM_RT_XML_PIECES; ++s) rt_xml_piece(o, r, s);
    return o.pos;
}
