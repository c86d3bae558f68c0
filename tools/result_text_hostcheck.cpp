// The result text formatter (gomatching_amd/csrc/result_text_core.h) on the host, for a run under the host compiler's
// sanitizers: the same functions the kernels call -- count, then emit into a bounded buffer -- over dumped calls.
//
//   result_text_hostcheck DUMP OUTDIR [SHORT]
//
// DUMP (written by tests/result_text_cases.py), all little-endian:
//   int64  ncalls
//   per call: int64 n, F, first_frame, ntab
//             int32 words[n][234]; int64 pts[n][8]; u8 keep[n]; int32 frame_rows[F+1]; u8 json_tab[ntab][8]; u8 xml_tab[ntab][8]
// Every array is copied into an allocation of exactly its size, and the two streams are emitted into allocations of exactly the
// counted totals minus SHORT bytes (default 0), so that a read or a write one byte outside any of them is the sanitizer's to
// report.  With SHORT > 0 the emit must refuse: the writer's bounds check drops what does not fit and the needed length comes
// back larger than the buffer.
// Output: OUTDIR/call_I.json and call_I.xml (the streams of call I: what stands between the files' header and footer), and one
// line per call, "call I: json J xml X status S" or "call I: refused json J > A xml X > B".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../gomatching_amd/csrc/result_text_core.h"

static bool read_exact(FILE* f, void* dst, size_t n) { return n == 0 || fread(dst, 1, n, f) == n; }

template <typename T>
static T* exact(FILE* f, size_t count, bool& ok) {
    T* p = (T*)malloc(count ? count * sizeof(T) : 1);
    ok = ok && p && read_exact(f, p, count * sizeof(T));
    return p;
}

struct Call {
    int64_t n, F, first, ntab;
    int32_t* words;
    int64_t* pts;
    uint8_t* keep;
    int32_t* frame_rows;
    uint8_t *jt, *xt;
    GomRtRow row(int64_t r) const { return GomRtRow{words + r * GOM_RESULT_ROWS_WORDS, pts + r * 8, jt, xt, (int)ntab}; }
    bool kept(int64_t r) const { return keep[r] && !rt_row_bad(row(r)); }
};

// both streams of a call through one bounded writer each; a null buffer counts
static void run(const Call& c, GomRtOut& js, GomRtOut& xs, int& status) {
    for (int64_t f = 0; f < c.F; ++f) {
        const int64_t s = c.frame_rows[f], e = c.frame_rows[f + 1];
        int kept = 0;
        for (int64_t r = s; r < e; ++r) {
            kept += c.kept(r) ? 1 : 0;
            if (c.keep[r] && rt_row_bad(c.row(r))) status = GOM_RT_BAD_ID;
        }
        rt_json_frame_head(js, c.first + f, kept);
        rt_xml_frame_head(xs, c.first + f, kept);
        int before = 0;
        for (int64_t r = s; r < e; ++r) {
            if (!c.kept(r)) continue;
            const GomRtRow row = c.row(r);
            // the row's length, then the row into what is left of the buffer: the kernel's order of events
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

static bool write_file(const std::string& path, const unsigned char* p, long n) {
    FILE* f = fopen(path.c_str(), "wb");
    if (!f) return false;
    const bool ok = n == 0 || fwrite(p, 1, (size_t)n, f) == (size_t)n;
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
        int64_t h[4];
        if (!read_exact(f, h, sizeof h)) return 2;
        Call c;
        c.n = h[0], c.F = h[1], c.first = h[2], c.ntab = h[3];
        if (c.n < 0 || c.F < 0 || c.first < 0 || c.ntab < 1 || c.ntab > (1 << 20)) {
            fprintf(stderr, "call %lld: a header the formatter refuses\n", (long long)call);
            return 2;
        }
        bool ok = true;
        c.words = exact<int32_t>(f, (size_t)c.n * GOM_RESULT_ROWS_WORDS, ok);
        c.pts = exact<int64_t>(f, (size_t)c.n * 8, ok);
        c.keep = exact<uint8_t>(f, (size_t)c.n, ok);
        c.frame_rows = exact<int32_t>(f, (size_t)c.F + 1, ok);
        c.jt = exact<uint8_t>(f, (size_t)c.ntab * GOM_RT_ENTRY_BYTES, ok);
        c.xt = exact<uint8_t>(f, (size_t)c.ntab * GOM_RT_ENTRY_BYTES, ok);
        if (!ok) return 2;
        for (int64_t i = 0; i <= c.F; ++i)                     // (the wrapper's check of the offsets)
            if (c.frame_rows[i] < 0 || c.frame_rows[i] > c.n || (i && c.frame_rows[i] < c.frame_rows[i - 1]) ||
                (i == 0 && c.frame_rows[0] != 0) || (i == c.F && c.frame_rows[i] != c.n)) {
                fprintf(stderr, "call %lld: frame_rows are no offsets over %lld rows\n", (long long)call, (long long)c.n);
                return 2;
            }
        int status = 0;
        GomRtOut cj = {nullptr, 0, 0}, cx = {nullptr, 0, 0};
        run(c, cj, cx, status);                                 // count
        const long aj = cj.pos > shorter ? cj.pos - shorter : 0, ax = cx.pos > shorter ? cx.pos - shorter : 0;
        unsigned char* bj = (unsigned char*)malloc(aj ? (size_t)aj : 1);
        unsigned char* bx = (unsigned char*)malloc(ax ? (size_t)ax : 1);
        if (!bj || !bx) return 2;
        GomRtOut ej = {bj, aj, 0}, ex = {bx, ax, 0};
        run(c, ej, ex, status);                                 // emit
        if (ej.pos != cj.pos || ex.pos != cx.pos) {
            fprintf(stderr, "call %lld: counted %ld / %ld bytes, emitted %ld / %ld\n", (long long)call, cj.pos, cx.pos, ej.pos, ex.pos);
            return 3;
        }
        if (ej.pos > aj || ex.pos > ax) {
            printf("call %lld: refused json %ld > %ld xml %ld > %ld\n", (long long)call, ej.pos, aj, ex.pos, ax);
        } else {
            const std::string stem = std::string(argv[2]) + "/call_" + std::to_string((long long)call);
            if (!write_file(stem + ".json", bj, aj) || !write_file(stem + ".xml", bx, ax)) {
                fprintf(stderr, "cannot write %s.*\n", stem.c_str());
                return 2;
            }
            printf("call %lld: json %ld xml %ld status %d\n", (long long)call, aj, ax, status);
        }
        free(bj);
        free(bx);
        free(c.words);
        free(c.pts);
        free(c.keep);
        free(c.frame_rows);
        free(c.jt);
        free(c.xt);
    }
    fclose(f);
    return 0;
}
