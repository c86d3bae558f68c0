// Lexicon correction of rows (THE RULE: include/gomatching_hip.h, `gom_lexicon_rows_*`), written once for the device
// (csrc/lexicon_rows.hip, and the `_ov` forms of csrc/result_text.hip and csrc/track_vote.hip) and for the host
// (tools/lexicon_rows_hostcheck.cpp, built with the host compiler and sanitizers): a row's query through the norm table, the
// acceptance of a match, and the display form an accepted row takes its text from.
// One function both counts and writes a query: without a buffer it only advances, so a length is by construction the length of
// what the same call writes.  Every store compares the index with the cap first; a table index is checked before the read.
#pragma once
#include <stdint.h>

#include "../../include/gomatching_hip.h"

#if defined(__HIPCC__)
#define GOM_LR_FN __host__ __device__ __forceinline__
#else
#define GOM_LR_FN static inline
#endif

// the query of one row: code point k is stored at out[k] iff out && k < cap -> the number of code points (at most 75).  A row that
// is not kept, or that has an emitted id outside the table, has the empty query: no id is used as an index unchecked.
GOM_LR_FN int lr_query(const int32_t* row, bool keep, const uint32_t* tab, int ntab, uint32_t* out, long cap) {
    if (!keep) return 0;
    const uint32_t emit = (uint32_t)row[GOM_RR_EMIT];
    for (int c = 0; c < 25; ++c) {
        const int32_t id = row[GOM_RR_RECS + c];
        if (((emit >> c) & 1u) && (id < 0 || id >= ntab)) return 0;
    }
    int len = 0;
    for (int c = 0; c < 25; ++c) {
        if (!((emit >> c) & 1u)) continue;
        const uint32_t* e = tab + (long)row[GOM_RR_RECS + c] * GOM_LR_NORM_WORDS;
        int k = (int)e[0];
        if (k < 0 || k > GOM_LR_NORM_WORDS - 1) k = GOM_LR_NORM_WORDS - 1;
        for (int i = 0; i < k; ++i) {
            if (out && len < cap) out[len] = e[1 + i];
            ++len;
        }
    }
    return len;
}

// the length word of a row: GOM_LR_LEN_LONG for a query above the limit (it is matched as the empty query and flagged)
GOM_LR_FN int lr_query_len(const int32_t* row, bool keep, const uint32_t* tab, int ntab) {
    const int len = lr_query(row, keep, tab, ntab, nullptr, 0);
    return len > GOM_LEXICON_MAX_LEN ? GOM_LR_LEN_LONG : len;
}

// the apply step of one row -> ov: the accepted word's index within its lexicon, or -1
GOM_LR_FN int lr_accept(bool keep, int q_len, int index, int dist, int W, int max_dist) {
    return keep && q_len >= 0 && index >= 0 && index < W && dist <= max_dist ? index : -1;
}

// entry `i` of a display table (bytes + int32 off[W + 1], `nbytes` bytes in all): -> its length, clamped to `limit` and to the
// table, and its first byte in `at`; an index or an offset outside the table gives the empty form at byte 0
GOM_LR_FN int lr_display(const int32_t* off, int W, long nbytes, int i, int limit, long& at) {
    at = 0;
    if (i < 0 || i >= W) return 0;
    const long b = off[i], e = off[i + 1];
    if (b < 0 || e < b || e > nbytes) return 0;
    at = b;
    return e - b > limit ? limit : (int)(e - b);
}
