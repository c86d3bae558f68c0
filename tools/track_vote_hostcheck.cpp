// The track vote's shared core (gomatching_amd/csrc/track_vote_core.h) on the host, for a run under the host compiler's
// sanitizers: the same functions the kernels call -- a row's record, the record compare, the vote key, the line formatter --
// over dumped videos.
//
//   track_vote_hostcheck DUMP OUTDIR [SHORT]
//
// DUMP (written by tests/track_vote_cases.py), all little-endian:
//   int64  nvideos
//   per video: int64 n, ntab;  int32 words[n][234]; u8 keep[n]; u8 txt_tab[ntab][8]
// Every array is copied into an allocation of exactly its size, the records go into an allocation of exactly n * 28 words and
// the lines into one of exactly the counted bytes minus SHORT (default 0), so that a read or a write one byte outside any of
// them is the sanitizer's to report.  With SHORT > 0 the emit must refuse: the formatter's bounds check drops what does not
// fit and the needed length comes back larger than the buffer.
// The ordering the Python wrapper does with a stable sort is a std::stable_sort here; the vote is the kernel's: every row of a
// track against every row of the track, the greatest key wins.
// Output: OUTDIR/video_I.txt, and one line per video, "video I: bytes B tracks T status S" or "video I: refused B > A".
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../gomatching_amd/csrc/track_vote_core.h"

static bool read_exact(FILE* f, void* dst, size_t n) { return n == 0 || fread(dst, 1, n, f) == n; }

template <typename T>
static T* exact(FILE* f, size_t count, bool& ok) {
    T* p = (T*)malloc(count ? count * sizeof(T) : 1);
    ok = ok && p && read_exact(f, p, count * sizeof(T));
    return p;
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
    int64_t nvideos = 0;
    if (!read_exact(f, &nvideos, 8) || nvideos < 0 || shorter < 0) return 2;
    for (int64_t video = 0; video < nvideos; ++video) {
        int64_t h[2];
        if (!read_exact(f, h, sizeof h)) return 2;
        const int64_t n = h[0], ntab = h[1];
        if (n < 0 || n > (1 << 24) || ntab < 1 || ntab > (1 << 20)) {
            fprintf(stderr, "video %lld: a header the vote refuses\n", (long long)video);
            return 2;
        }
        bool ok = true;
        int32_t* words = exact<int32_t>(f, (size_t)n * GOM_RESULT_ROWS_WORDS, ok);
        uint8_t* keep = exact<uint8_t>(f, (size_t)n, ok);
        uint8_t* tab = exact<uint8_t>(f, (size_t)ntab * GOM_RT_ENTRY_BYTES, ok);
        if (!ok) return 2;
        // ---- records
        int32_t* records = (int32_t*)malloc(n ? (size_t)n * GOM_TV_RECORD_WORDS * sizeof(int32_t) : 1);
        if (!records) return 2;
        for (int64_t r = 0; r < n; ++r)
            tv_record(words + r * GOM_RESULT_ROWS_WORDS, keep[r] != 0, tab, (int)ntab, records + r * GOM_TV_RECORD_WORDS);
        // ---- the ordering: the voters by (track id, log position)
        std::vector<int32_t> order;
        for (int64_t r = 0; r < n; ++r)
            if (records[r * GOM_TV_RECORD_WORDS + GOM_TV_LEN] != GOM_TV_LEN_DROPPED) order.push_back((int32_t)r);
        std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) {
            return tv_track_id(records + (long)a * GOM_TV_RECORD_WORDS) < tv_track_id(records + (long)b * GOM_TV_RECORD_WORDS);
        });
        std::vector<long> seg(1, 0);
        for (size_t i = 1; i <= order.size(); ++i)
            if (i == order.size() || tv_track_id(records + (long)order[i] * GOM_TV_RECORD_WORDS) !=
                                         tv_track_id(records + (long)order[i - 1] * GOM_TV_RECORD_WORDS))
                seg.push_back((long)i);
        const size_t T = seg.size() - 1;
        // ---- the vote
        int status = 0;
        long total = 0;
        std::vector<long> winner(T, -1), line_off(T + 1, 0);
        for (size_t t = 0; t < T; ++t) {
            const long s = seg[t], L = seg[t + 1] - seg[t];
            unsigned long long best = 0;
            for (long i = 0; i < L; ++i) {
                const GomTvKey key = tv_key_load(records + (long)order[s + i] * GOM_TV_RECORD_WORDS);
                if (key.w[0] == GOM_TV_LEN_BAD) status |= GOM_TV_BAD_ID;
                if (key.w[0] < 0) continue;
                uint32_t count = 0;
                for (long j = 0; j < L; ++j) count += tv_same(key, records + (long)order[s + j] * GOM_TV_RECORD_WORDS) ? 1u : 0u;
                const unsigned long long k = tv_vote_key(count, (uint32_t)i);
                best = k > best ? k : best;
            }
            line_off[t] = total;
            if (best != 0) {
                winner[t] = order[s + (long)(0xFFFFFFFFu - (uint32_t)(best & 0xFFFFFFFFull))];
                total += tv_line_len(records + winner[t] * GOM_TV_RECORD_WORDS);
            }
        }
        line_off[T] = total;
        // ---- the lines, into exactly the counted bytes (minus SHORT)
        const long cap = total > shorter ? total - shorter : 0;
        unsigned char* out = (unsigned char*)malloc(cap ? (size_t)cap : 1);
        if (!out) return 2;
        long need = 0;
        for (size_t t = 0; t < T; ++t) {
            if (winner[t] < 0) continue;
            const long at = line_off[t], room = cap - at;
            const long len = tv_line(records + winner[t] * GOM_TV_RECORD_WORDS, room > 0 ? out + at : nullptr, room > 0 ? room : 0);
            if (len != line_off[t + 1] - at) {
                fprintf(stderr, "video %lld track %zu: counted %ld bytes, emitted %ld\n", (long long)video, t, line_off[t + 1] - at, len);
                return 3;
            }
            need = at + len;
        }
        if (need > cap) {
            printf("video %lld: refused %ld > %ld\n", (long long)video, need, cap);
        } else {
            if (status == 0) {
                const std::string path = std::string(argv[2]) + "/video_" + std::to_string((long long)video) + ".txt";
                FILE* o = fopen(path.c_str(), "wb");
                const bool wrote = o && (cap == 0 || fwrite(out, 1, (size_t)cap, o) == (size_t)cap);
                if (!o || fclose(o) != 0 || !wrote) {
                    fprintf(stderr, "cannot write %s\n", path.c_str());
                    return 2;
                }
            }
            printf("video %lld: bytes %ld tracks %zu status %d\n", (long long)video, cap, T, status);
        }
        free(out);
        free(records);
        free(words);
        free(keep);
        free(tab);
    }
    fclose(f);
    return 0;
}
