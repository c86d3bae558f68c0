// The reading of result text (gomatching_amd/csrc/result_parse_core.h) on the host, for a run under the host compiler's
// sanitizers: the same per-line functions the kernels call -- the marks, the spans, every object line against its template, every
// frame's wrapper lines -- over dumped files, the stages of the rule one after another as the three calls run them.
//
//   result_parse_hostcheck DUMP OUTDIR [SHORT]
//
// DUMP (written by tests/result_parse_cases.py), little-endian: int64 ncases; per case int64 size and the bytes.
// Every array is an allocation of exactly its size: the file, line_start [L + 1], the marks, and the outputs -- the per-object
// arrays of N - SHORT elements, poly_xy of P - SHORT points (default 0) -- so that a read or a write one element outside any of
// them is the sanitizer's to report.  With SHORT > 0 the bounds checks must drop what does not fit and say GOM_RP_BAD_CAP.
// Output: one line per case, "case I: status S L l F f N n P p", and for status 0 OUTDIR/case_I.bin: frame_rows int32 [F + 1],
// ids int64 [N], pts int32 [N][8], has_seg u8 [N], t_off int64 [N], t_len int32 [N], poly_off int32 [N + 1], poly_xy int32 [P][2].
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "../gomatching_amd/csrc/result_parse_core.h"

template <typename T>
static T* alloc(long count) {
    T* p = (T*)malloc(count > 0 ? (size_t)count * sizeof(T) : 1);
    if (!p) exit(2);
    return p;
}

template <typename T>
static bool put(FILE* f, const T* p, long count) {
    return count <= 0 || fwrite(p, sizeof(T), (size_t)count, f) == (size_t)count;
}

int main(int argc, char** argv) {
    if (argc != 3 && argc != 4) {
        fprintf(stderr, "usage: %s DUMP OUTDIR [SHORT]\n", argv[0]);
        return 2;
    }
    const long shorter = argc == 4 ? atol(argv[3]) : 0;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    int64_t ncases = 0;
    if (fread(&ncases, 8, 1, f) != 1 || ncases < 0 || shorter < 0) return 2;
    for (int64_t c = 0; c < ncases; ++c) {
        int64_t size = 0;
        if (fread(&size, 8, 1, f) != 1 || size < 0) return 2;
        if (size < 1 || size > GOM_RP_MAX_SIZE - 1) {          // (the wrapper's refusal: nothing is launched; a dump holds no bytes)
            printf("case %lld: status %d L 0 F 0 N 0 P 0\n", (long long)c, GOM_RP_BAD_SIZE);
            if (size > 0) return 2;
            continue;
        }
        unsigned char* data = alloc<unsigned char>(size);
        if (fread(data, 1, (size_t)size, f) != (size_t)size) return 2;
        // ---- lines
        long L = 1;
        for (long i = 0; i < size; ++i) L += data[i] == '\n';
        int status = rp_ends(data, size, L);
        long F = 0, N = 0, P = 0;
        if (status == 0 && L >= 2) {
            int32_t* line_start = alloc<int32_t>(L + 1);
            long q = 0;
            line_start[0] = 0;
            for (long i = 0; i < size; ++i)
                if (data[i] == '\n') line_start[++q] = (int32_t)(i + 1);
            line_start[L] = (int32_t)(size + 1);
            const GomRpText t = {data, size, line_start, L};
            // ---- marks
            for (long i = 0; i < L; ++i) {
                long a, b;
                rp_line(t, i, a, b);
                N += rp_is_object_line(t, a, b);
                F += rp_is_key_line(t, a, b);
                if ((long)line_start[i + 1] - 1 - line_start[i] > GOM_RP_MAX_LINE) status |= GOM_RP_BAD_LINE;
            }
            if (F == 0) status |= GOM_RP_BAD_PLACE;
            if (status == 0) {
                int32_t* mark_line = alloc<int32_t>(N + F + 1);
                int32_t* obj_mark = alloc<int32_t>(N);
                int32_t* frame_mark = alloc<int32_t>(F);
                int32_t* frame_rows = alloc<int32_t>(F + 1);
                long oi = 0, ki = 0;
                for (long i = 0; i < L; ++i) {
                    long a, b;
                    rp_line(t, i, a, b);
                    if (rp_is_object_line(t, a, b)) {
                        mark_line[oi + ki] = (int32_t)i;
                        obj_mark[oi] = (int32_t)(oi + ki);
                        ++oi;
                    } else if (rp_is_key_line(t, a, b)) {
                        mark_line[oi + ki] = (int32_t)i;
                        frame_mark[ki] = (int32_t)(oi + ki);
                        frame_rows[ki] = (int32_t)oi;
                        ++ki;
                    }
                }
                mark_line[N + F] = (int32_t)(L - 1);
                frame_rows[F] = (int32_t)N;
                const GomRpMarks m = {mark_line, obj_mark, frame_mark, frame_rows, N, F};
                // ---- the scan of n
                int32_t* poly_off = alloc<int32_t>(N + 1);
                poly_off[0] = 0;
                for (long o = 0; o < N; ++o) {
                    long s, nl;
                    bool next_obj;
                    rp_object_span(m, L, o, s, nl, next_obj);
                    poly_off[o + 1] = poly_off[o] + rp_points_of(nl);
                }
                P = poly_off[N];
                // ---- objects and frames
                const long cap_n = N > shorter ? N - shorter : 0, cap_p = P > shorter ? P - shorter : 0;
                const GomRpRows r = {alloc<int64_t>(cap_n),   alloc<int32_t>(cap_n * 8), alloc<unsigned char>(cap_n), alloc<int64_t>(cap_n),
                                     alloc<int32_t>(cap_n), cap_n,                     alloc<int32_t>(cap_p * 2),   cap_p};
                for (long o = 0; o < N; ++o) {
                    long s, nl;
                    bool next_obj;
                    rp_object_span(m, L, o, s, nl, next_obj);
                    int j10 = -1;
                    for (long j = 2; j < nl && j < 64 && j10 < 0; ++j)
                        if (rp_is_points_closer(t, s + j)) j10 = (int)j;
                    const int shape = rp_object_shape(nl, j10);
                    status |= shape;
                    if (shape) continue;
                    for (long j = 0; j < nl; ++j) status |= rp_object_line(t, s, nl, next_obj, j, o, poly_off[o], r);
                }
                for (long k = 0; k < F; ++k) status |= rp_frame(t, m, k);
                if (status == 0) {
                    const std::string path = std::string(argv[2]) + "/case_" + std::to_string((long long)c) + ".bin";
                    FILE* g = fopen(path.c_str(), "wb");
                    if (!g || !put(g, frame_rows, F + 1) || !put(g, r.ids, N) || !put(g, r.pts, N * 8) || !put(g, r.has_seg, N) ||
                        !put(g, r.t_off, N) || !put(g, r.t_len, N) || !put(g, poly_off, N + 1) || !put(g, r.poly_xy, P * 2) ||
                        fclose(g) != 0) {
                        fprintf(stderr, "cannot write %s\n", path.c_str());
                        return 2;
                    }
                }
                free(r.ids);
                free(r.pts);
                free(r.has_seg);
                free(r.t_off);
                free(r.t_len);
                free(r.poly_xy);
                free(poly_off);
                free(mark_line);
                free(obj_mark);
                free(frame_mark);
                free(frame_rows);
            }
            free(line_start);
        }
        printf("case %lld: status %d L %ld F %ld N %ld P %ld\n", (long long)c, status, L, F, N, P);
        free(data);
    }
    fclose(f);
    return 0;
}
