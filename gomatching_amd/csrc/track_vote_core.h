// The track vote (THE RULE: include/gomatching_hip.h, `gom_track_vote_*`), written once for the device (csrc/track_vote.hip) and
// for the host (tools/track_vote_hostcheck.cpp, built with the host compiler and sanitizers): a row's record (the text build),
// the record compare, the vote key and the line formatter.
// A record's words are written once each, in order, through `tv_store`, which compares the index with the record's size before
// the store; a table index is checked before the read.  A line is a pure function of the winner's record, byte by byte
// (`tv_line_byte`): the kernel gives a lane a byte, the host walks them into a bounded buffer (`tv_line`).
#pragma once
#include <stdint.h>

#include "../../include/gomatching_hip.h"

#if defined(__HIPCC__)
#define GOM_TV_FN __host__ __device__ __forceinline__
#define GOM_TV_UNROLL _Pragma("unroll")
#else
#define GOM_TV_FN static inline
#define GOM_TV_UNROLL
#endif

#define GOM_TV_KEY_WORDS (GOM_TV_RECORD_WORDS - GOM_TV_LEN)   // what two records are compared by: the length, then the text

GOM_TV_FN void tv_store(int32_t* rec, int at, int32_t v) {
    if (at >= 0 && at < GOM_TV_RECORD_WORDS) rec[at] = v;
}

// ---- the record of one row.  `row`: the GOM_RESULT_ROWS_WORDS words of the row; `rec`: GOM_TV_RECORD_WORDS words, all written.
// `ovb` non-null (`gom_track_vote_records_ov_i32`): the text is the `ovlen` bytes there, the txt display form of the word a lexicon
// put in the row's place, instead of the table's entries; the flags (dropped, bad id) are the row's own either way.
GOM_TV_FN void tv_record_ov(const int32_t* row, bool keep, const unsigned char* tab, int ntab, const unsigned char* ovb, int ovlen,
                            int32_t* rec) {
    tv_store(rec, 0, row[GOM_RR_TRACK_ID]);
    tv_store(rec, 1, row[GOM_RR_TRACK_ID + 1]);
    const uint32_t emit = (uint32_t)row[GOM_RR_EMIT];
    bool bad = false;
    for (int c = 0; c < 25; ++c) {
        const int32_t id = row[GOM_RR_RECS + c];
        bad = bad || (((emit >> c) & 1u) && (id < 0 || id >= ntab));
    }
    int len = 0, word_at = GOM_TV_TEXT;                        // bytes so far; the next text word to store
    uint32_t word = 0;
    if (keep && !bad && ovb) {
        if (ovlen > 4 * GOM_TV_TEXT_WORDS) ovlen = 4 * GOM_TV_TEXT_WORDS;
        for (int i = 0; i < ovlen; ++i) {
            word |= (uint32_t)ovb[i] << (8 * (len & 3));
            ++len;
            if ((len & 3) == 0) {
                tv_store(rec, word_at++, (int32_t)word);
                word = 0;
            }
        }
    } else if (keep && !bad) {
        for (int c = 0; c < 25; ++c) {
            if (!((emit >> c) & 1u)) continue;
            const unsigned char* e = tab + (long)row[GOM_RR_RECS + c] * GOM_RT_ENTRY_BYTES;
            int n = e[0];
            if (n > GOM_TV_ENTRY_MAX) n = GOM_TV_ENTRY_MAX;
            for (int i = 0; i < n; ++i) {
                word |= (uint32_t)e[1 + i] << (8 * (len & 3));
                ++len;
                if ((len & 3) == 0) {
                    tv_store(rec, word_at++, (int32_t)word);
                    word = 0;
                }
            }
        }
    }
    tv_store(rec, GOM_TV_LEN, !keep ? GOM_TV_LEN_DROPPED : (bad ? GOM_TV_LEN_BAD : len));
    if (len & 3) tv_store(rec, word_at++, (int32_t)word);
    for (; word_at < GOM_TV_RECORD_WORDS; ++word_at) tv_store(rec, word_at, 0);
}

GOM_TV_FN void tv_record(const int32_t* row, bool keep, const unsigned char* tab, int ntab, int32_t* rec) {
    tv_record_ov(row, keep, tab, ntab, nullptr, 0, rec);
}

GOM_TV_FN int64_t tv_track_id(const int32_t* rec) {
    const uint64_t lo = (uint32_t)rec[0], hi = (uint32_t)rec[1];
    return (int64_t)(lo | (hi << 32));
}

// ---- the compare.  A lane (or the host's loop) holds one record's key and meets the others where they lie.
struct GomTvKey {
    int32_t w[GOM_TV_KEY_WORDS];                               // (indexed by constants only: the loops below unroll)
};

GOM_TV_FN GomTvKey tv_key_load(const int32_t* rec) {
    GomTvKey k;
    GOM_TV_UNROLL
    for (int i = 0; i < GOM_TV_KEY_WORDS; ++i) k.w[i] = rec[GOM_TV_LEN + i];
    return k;
}

// true: the record at `rec` votes and has the key's text -- the length word and every text word.  Without a branch: the 26 words
// of `rec` are then ONE batch of loads; with an exit per word they were 26 loads, each waited for (docs/LAB_NOTES.md).
GOM_TV_FN bool tv_same(const GomTvKey& k, const int32_t* rec) {
    uint32_t diff = 0;
    GOM_TV_UNROLL
    for (int i = 0; i < GOM_TV_KEY_WORDS; ++i) diff |= (uint32_t)rec[GOM_TV_LEN + i] ^ (uint32_t)k.w[i];
    return diff == 0 && k.w[0] >= 0;
}

// the greatest key wins: the greatest count, then the smallest place in the track.  0 is below every voting row's key.
GOM_TV_FN unsigned long long tv_vote_key(uint32_t count, uint32_t place) {
    return ((unsigned long long)count << 32) | (unsigned long long)(0xFFFFFFFFu - place);
}

// ---- the line of a track:  "I","W"\n
GOM_TV_FN int tv_digits_u64(uint64_t m) {
    int d = 1;
    while (m >= 10) {
        m /= 10;
        ++d;
    }
    return d;
}

GOM_TV_FN int tv_text_len(const int32_t* rec) {
    const int len = rec[GOM_TV_LEN];
    return len < 0 ? 0 : (len > 4 * GOM_TV_TEXT_WORDS ? 4 * GOM_TV_TEXT_WORDS : len);
}

GOM_TV_FN int tv_line_len(const int32_t* rec) {
    const int64_t id = tv_track_id(rec);
    const uint64_t mag = id < 0 ? (uint64_t)0 - (uint64_t)id : (uint64_t)id;
    return 1 + (id < 0 ? 1 : 0) + tv_digits_u64(mag) + 3 + tv_text_len(rec) + 2;
}

// byte k of the line, 0 <= k < tv_line_len(rec)
GOM_TV_FN unsigned char tv_line_byte(const int32_t* rec, int k) {
    const int64_t id = tv_track_id(rec);
    uint64_t mag = id < 0 ? (uint64_t)0 - (uint64_t)id : (uint64_t)id;
    const int neg = id < 0 ? 1 : 0, d = tv_digits_u64(mag), len = tv_text_len(rec);
    const int text_at = 1 + neg + d + 3;
    if (k == 0) return '"';
    if (neg && k == 1) return '-';
    if (k < 1 + neg + d) {
        for (int i = 1 + neg + d - 1 - k; i > 0; --i) mag /= 10;
        return (unsigned char)('0' + (int)(mag % 10));
    }
    if (k < text_at) return k == text_at - 2 ? ',' : '"';
    if (k < text_at + len) {
        const int b = k - text_at;
        return (unsigned char)(((uint32_t)rec[GOM_TV_TEXT + (b >> 2)] >> (8 * (b & 3))) & 0xFFu);
    }
    return k == text_at + len ? '"' : '\n';
}

// the whole line into a bounded buffer (the host's form) -> the line's length; bytes at or past `cap` were not written
GOM_TV_FN long tv_line(const int32_t* rec, unsigned char* buf, long cap) {
    const int n = tv_line_len(rec);
    for (int k = 0; k < n; ++k)
        if (buf && k < cap) buf[k] = tv_line_byte(rec, k);
    return n;
}
