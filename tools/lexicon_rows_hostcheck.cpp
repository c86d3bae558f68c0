// The lexicon correction of rows (gomatching_amd/csrc/lexicon_rows_core.h and the override forms of result_text_core.h and
// track_vote_core.h) on the host, for a run under the host compiler's sanitizers: the same functions the kernels call -- the
// queries counted, then written; the rows with their overrides counted, then emitted into bounded buffers; the vote records --
// over dumped calls.
//
//   lexicon_rows_hostcheck DUMP OUTDIR [SHORT]
//
// DUMP (written by tests/lexicon_rows_cases.py), all little-endian:
//   int64  ncalls
//   per call: int64 n, F, first_frame, ntab, W, max_dist, drop, json_dbytes, xml_dbytes, txt_dbytes
//             int32 words[n][234]; int64 pts[n][8]; u8 keep[n]; int32 frame_rows[F+1]; u8 json_tab, xml_tab, txt_tab [ntab][8];
//             uint32 norm_tab[ntab][4]; int32 ov[n] (the match is another program's business: csrc/lexicon.hip);
//             per display table (json, xml, txt): int32 off[W+1]; u8 bytes[dbytes]
// Every array is copied into an allocation of exactly its size; the queries are written into an allocation of exactly the
// counted code points minus SHORT, the two streams into allocations of exactly the counted totals minus SHORT bytes (default 0),
// so that a read or a write one element outside any of them is the sanitizer's to report.  With SHORT > 0 every writer must
// refuse: the bounds checks drop what does not fit and the needed length comes back larger than the buffer.
// Output: OUTDIR/call_I.q (the queries' code points, uint32, row after row), call_I.json, call_I.xml (the corrected streams
// between the files' header and footer), call_I.rec (the vote records, int32 [n][28]) and one line per call,
// "call I: q Q json J xml X" or "call I: refused q Q > A json J > B xml X > C".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../gomatching_amd/csrc/lexicon_rows_core.h"
#include "../gomatching_amd/csrc/result_text_core.h"
#include "../gomatching_amd/csrc/track_vote_core.h"

static bool read_exact(FILE* f, void* dst, size_t n) { return n == 0 || fread(dst, 1, n, f) == n; }

template <typename T>
static T* exact(FILE* f, size_t count, bool& ok) {
    T* p = (T*)malloc(count ? count * sizeof(T) : 1);
    ok = ok && p && read_exact(f, p, count * sizeof(T));
    return p;
}

struct Table {
    int32_t* off;
    uint8_t* bytes;
    int64_t nbytes;
};

struct Call {
    int64_t n, F, first, ntab, W, max_dist, drop;
    int32_t* words;
    int64_t* pts;
    uint8_t* keep;
    int32_t* frame_rows;
    uint8_t *jt, *xt, *tt;
    uint32_t* norm;
    int32_t* ov;
    Table disp[3];
    const int32_t* words_of(int64_t r) const { return words + r * GOM_RESULT_ROWS_WORDS; }
    int accepted(int64_t r) const {                            // the apply step on the dumped match: index = ov, distance 0
        return lr_accept(keep[r] != 0, lr_query_len(words_of(r), keep[r] != 0, norm, (int)ntab), ov[r], 0, (int)W, (int)max_dist);
    }
    bool keep_out(int64_t r) const { return keep[r] && (!drop || accepted(r) >= 0); }
    GomRtRow row(int64_t r) const {
        GomRtRow row = {words_of(r), pts + r * 8, jt, xt, (int)ntab, nullptr, 0, nullptr, 0};
        const int i = accepted(r);
        if (i >= 0) {
            long at;
            row.json_ov_len = lr_display(disp[0].off, (int)W, disp[0].nbytes, i, 25 * (GOM_RT_ENTRY_BYTES - 1), at);
            row.json_ov = disp[0].bytes + at;
            row.xml_ov_len = lr_display(disp[1].off, (int)W, disp[1].nbytes, i, 25 * (GOM_RT_ENTRY_BYTES - 1), at);
            row.xml_ov = disp[1].bytes + at;
        }
        return row;
    }
    bool kept(int64_t r) const { return keep_out(r) && !rt_row_bad(row(r)); }
};

// the queries of a call through one bounded buffer; a null buffer counts -> the code points needed
static long queries(const Call& c, uint32_t* buf, long cap) {
    long pos = 0;
    for (int64_t r = 0; r < c.n; ++r) {
        const int len = lr_query_len(c.words_of(r), c.keep[r] != 0, c.norm, (int)c.ntab);
        if (len <= 0) continue;
        const int w = lr_query(c.words_of(r), c.keep[r] != 0, c.norm, (int)c.ntab, buf ? buf + (pos < cap ? pos : cap) : nullptr,
                               buf && pos < cap ? cap - pos : 0);
        if (w != len) {
            fprintf(stderr, "row %lld: counted %d code points, wrote %d\n", (long long)r, len, w);
            exit(3);
        }
        pos += len;
    }
    return pos;
}

// both streams of a call through one bounded writer each; a null buffer counts
static void run(const Call& c, GomRtOut& js, GomRtOut& xs) {
    for (int64_t f = 0; f < c.F; ++f) {
        const int64_t s = c.frame_rows[f], e = c.frame_rows[f + 1];
        int kept = 0;
        for (int64_t r = s; r < e; ++r) kept += c.kept(r) ? 1 : 0;
        rt_json_frame_head(js, c.first + f, kept);
        rt_xml_frame_head(xs, c.first + f, kept);
        int before = 0;
        for (int64_t r = s; r < e; ++r) {
            if (!c.kept(r)) continue;
            const GomRtRow row = c.row(r);
            const long lj = rt_json_row(row, before > 0, nullptr, 0), lx = rt_xml_row(row, nullptr, 0);
            const long wj = rt_json_row(row, before > 0, js.buf ? js.buf + js.pos : nullptr, js.buf ? js.cap - js.pos : 0);
            const long wx = rt_xml_row(row, xs.buf ? xs.buf + xs.pos : nullptr, xs.buf ? xs.cap - xs.pos : 0);
            if (wj != lj || wx != lx) {
                fprintf(stderr, "row %lld: counted %ld / %ld bytes, emitted %ld / %ld\n", (long long)r, lj, lx, wj, wx);
                exit(3);
            }
            js.pos += lj;
            xs.pos += lx;
            ++before;
        }
        rt_json_frame_tail(js, kept);
        rt_xml_frame_tail(xs, kept);
    }
}

static bool write_file(const std::string& path, const void* p, size_t n) {
    FILE* f = fopen(path.c_str(), "wb");
    if (!f) return false;
    const bool ok = n == 0 || fwrite(p, 1, n, f) == n;
    return fclose(f) == 0 && ok;
}

int main(int argc, char** argv) {
    if (argc != 3 && argc != 4) {
        fprintf(stderr, "usage: %s DUMP OUTDIR [SHORT]\n", argv[0]);
        return 2;
    }
    const long shorter = argc == 4 ? atol(argv[3]) : 0;
    FILE* f = fopen(argv[1], "rb");
    if (!f) {
        fprintf(stderr, "cannot open %s\n", argv[1]);
        return 2;
    }
    int64_t ncalls = 0;
    if (!read_exact(f, &ncalls, 8) || ncalls < 0 || shorter < 0) return 2;
    for (int64_t call = 0; call < ncalls; ++call) {
        int64_t h[10];
        if (!read_exact(f, h, sizeof h)) return 2;
        Call c;
        c.n = h[0], c.F = h[1], c.first = h[2], c.ntab = h[3], c.W = h[4], c.max_dist = h[5], c.drop = h[6];
        if (c.n < 0 || c.F < 0 || c.first < 0 || c.ntab < 1 || c.ntab > (1 << 20) || c.W < 0 || c.W > (1 << 24) || c.max_dist < 0 ||
            (c.drop != 0 && c.drop != 1) || h[7] < 0 || h[8] < 0 || h[9] < 0) {
            fprintf(stderr, "call %lld: a header the entries refuse\n", (long long)call);
            return 2;
        }
        bool ok = true;
        c.words = exact<int32_t>(f, (size_t)c.n * GOM_RESULT_ROWS_WORDS, ok);
        c.pts = exact<int64_t>(f, (size_t)c.n * 8, ok);
        c.keep = exact<uint8_t>(f, (size_t)c.n, ok);
        c.frame_rows = exact<int32_t>(f, (size_t)c.F + 1, ok);
        c.jt = exact<uint8_t>(f, (size_t)c.ntab * GOM_RT_ENTRY_BYTES, ok);
        c.xt = exact<uint8_t>(f, (size_t)c.ntab * GOM_RT_ENTRY_BYTES, ok);
        c.tt = exact<uint8_t>(f, (size_t)c.ntab * GOM_RT_ENTRY_BYTES, ok);
        c.norm = exact<uint32_t>(f, (size_t)c.ntab * GOM_LR_NORM_WORDS, ok);
        c.ov = exact<int32_t>(f, (size_t)c.n, ok);
        for (int k = 0; k < 3; ++k) {
            c.disp[k].nbytes = h[7 + k];
            c.disp[k].off = exact<int32_t>(f, (size_t)c.W + 1, ok);
            c.disp[k].bytes = exact<uint8_t>(f, (size_t)c.disp[k].nbytes, ok);
        }
        if (!ok) return 2;
        for (int64_t i = 0; i <= c.F; ++i)                     // (the wrapper's check of the offsets)
            if (c.frame_rows[i] < 0 || c.frame_rows[i] > c.n || (i && c.frame_rows[i] < c.frame_rows[i - 1]) ||
                (i == 0 && c.frame_rows[0] != 0) || (i == c.F && c.frame_rows[i] != c.n)) {
                fprintf(stderr, "call %lld: frame_rows are no offsets over %lld rows\n", (long long)call, (long long)c.n);
                return 2;
            }
        // ---- the queries: count, then write
        const long nq = queries(c, nullptr, 0);
        const long aq = nq > shorter ? nq - shorter : 0;
        uint32_t* bq = (uint32_t*)malloc(aq ? (size_t)aq * 4 : 1);
        if (!bq) return 2;
        if (queries(c, bq, aq) != nq) return 3;
        // ---- the two streams: count, then emit
        GomRtOut cj = {nullptr, 0, 0}, cx = {nullptr, 0, 0};
        run(c, cj, cx);
        const long aj = cj.pos > shorter ? cj.pos - shorter : 0, ax = cx.pos > shorter ? cx.pos - shorter : 0;
        unsigned char* bj = (unsigned char*)malloc(aj ? (size_t)aj : 1);
        unsigned char* bx = (unsigned char*)malloc(ax ? (size_t)ax : 1);
        if (!bj || !bx) return 2;
        GomRtOut ej = {bj, aj, 0}, ex = {bx, ax, 0};
        run(c, ej, ex);
        if (ej.pos != cj.pos || ex.pos != cx.pos) {
            fprintf(stderr, "call %lld: counted %ld / %ld bytes, emitted %ld / %ld\n", (long long)call, cj.pos, cx.pos, ej.pos, ex.pos);
            return 3;
        }
        // ---- the vote records, every word through tv_store
        int32_t* rec = (int32_t*)malloc(c.n ? (size_t)c.n * GOM_TV_RECORD_WORDS * 4 : 1);
        if (!rec) return 2;
        for (int64_t r = 0; r < c.n; ++r) {
            const int i = c.accepted(r);
            long at = 0;
            const int len = i >= 0 ? lr_display(c.disp[2].off, (int)c.W, c.disp[2].nbytes, i, 4 * GOM_TV_TEXT_WORDS, at) : 0;
            tv_record_ov(c.words_of(r), c.keep_out(r), c.tt, (int)c.ntab, i >= 0 ? c.disp[2].bytes + at : nullptr, len,
                         rec + r * GOM_TV_RECORD_WORDS);
        }
        if (nq > aq || ej.pos > aj || ex.pos > ax) {
            printf("call %lld: refused q %ld > %ld json %ld > %ld xml %ld > %ld\n", (long long)call, nq, aq, ej.pos, aj, ex.pos, ax);
        } else {
            const std::string stem = std::string(argv[2]) + "/call_" + std::to_string((long long)call);
            if (!write_file(stem + ".q", bq, (size_t)aq * 4) || !write_file(stem + ".json", bj, (size_t)aj) ||
                !write_file(stem + ".xml", bx, (size_t)ax) || !write_file(stem + ".rec", rec, (size_t)c.n * GOM_TV_RECORD_WORDS * 4)) {
                fprintf(stderr, "cannot write %s.*\n", stem.c_str());
                return 2;
            }
            printf("call %lld: q %ld json %ld xml %ld\n", (long long)call, aq, aj, ax);
        }
        free(bq);
        free(bj);
        free(bx);
        free(rec);
        free(c.words);
        free(c.pts);
        free(c.keep);
        free(c.frame_rows);
        free(c.jt);
        free(c.xt);
        free(c.tt);
        free(c.norm);
        free(c.ov);
        for (int k = 0; k < 3; ++k) {
            free(c.disp[k].off);
            free(c.disp[k].bytes);
        }
    }
    fclose(f);
    return 0;
}
