// The JPEG decoder's entropy walk (gomatching_amd/csrc/jpeg_decode_core.h) on the host, for a run under the host compiler's
// sanitizers: the same functions the kernel calls, over the same uploads, before a GPU sees damaged bytes.
//
//   jpeg_decode_hostcheck DUMP
//
// DUMP (written by tests/test_jpeg_decode_hostcheck.py from jpeg.plan), all little-endian:
//   int64  ncalls
//   per call: int64 F, H, W, ncomp, hs, vs, nbytes, nseg, nsets
//             u8 data[nbytes]; int64 desc[nseg][8]; int32 seg_off[F+1]; int32 sets[nsets][2392]
// Every array is copied into an allocation of exactly its size, so that a read one byte outside it is the sanitizer's to report.
// Output: one line per call, "call I: status s0 s1 ... checksum C" (frame status words; a checksum of the coefficients).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../gomatching_amd/csrc/jpeg_decode_core.h"

static bool read_exact(FILE* f, void* dst, size_t n) { return n == 0 || fread(dst, 1, n, f) == n; }

int main(int argc, char** argv) {
    if (argc != 2) {
        fprintf(stderr, "usage: %s DUMP\n", argv[0]);
        return 2;
    }
    FILE* f = fopen(argv[1], "rb");
    if (!f) {
        fprintf(stderr, "cannot open %s\n", argv[1]);
        return 2;
    }
    int64_t ncalls = 0;
    if (!read_exact(f, &ncalls, 8) || ncalls < 0) return 2;
    for (int64_t call = 0; call < ncalls; ++call) {
        int64_t h[9];
        if (!read_exact(f, h, sizeof h)) return 2;
        const int64_t F = h[0], nbytes = h[6], nseg = h[7], nsets = h[8];
        GomJdGeom g;
        if (F < 1 || nbytes < 0 || nseg < 0 || nsets < 1 || !gom_jd_geometry((int)h[1], (int)h[2], (int)h[3], (int)h[4], (int)h[5], g)) {
            fprintf(stderr, "call %lld: a header the decoder refuses\n", (long long)call);
            return 2;
        }
        uint8_t* data = (uint8_t*)malloc((size_t)nbytes ? (size_t)nbytes : 1);
        int64_t* desc = (int64_t*)malloc((size_t)(nseg ? nseg : 1) * GOM_JD_DESC_WORDS * 8);
        int32_t* seg_off = (int32_t*)malloc((size_t)(F + 1) * 4);
        int32_t* sets = (int32_t*)malloc((size_t)nsets * GOM_JD_SET_WORDS * 4);
        if (!read_exact(f, data, (size_t)nbytes) || !read_exact(f, desc, (size_t)nseg * GOM_JD_DESC_WORDS * 8) ||
            !read_exact(f, seg_off, (size_t)(F + 1) * 4) || !read_exact(f, sets, (size_t)nsets * GOM_JD_SET_WORDS * 4))
            return 2;
        std::vector<int16_t> coef((size_t)F * g.nblk * 64, (int16_t)0);
        std::vector<int> seg_status((size_t)nseg, 0);
        for (int64_t s = 0; s < nseg; ++s) {
            const GomJdDesc d = gom_jd_desc(desc + s * GOM_JD_DESC_WORDS);
            if (d.frame < 0 || d.frame >= F || d.set < 0 || d.set >= nsets) {  // as the kernel
                seg_status[s] = GOM_JD_PAST_END;
                continue;
            }
            int16_t blk[64];
            int16_t* out = coef.data() + d.frame * g.nblk * 64;
            auto begin = [&](GomJdState&) { memset(blk, 0, sizeof blk); };
            auto emit = [&](long bi) { memcpy(out + bi * 64, blk, sizeof blk); };
            seg_status[s] = gom_jd_walk_segment(data, (long)nbytes, d, sets + d.set * GOM_JD_SET_WORDS, g, true, blk, begin, emit);
        }
        printf("call %lld: status", (long long)call);
        for (int64_t fr = 0; fr < F; ++fr) {
            int a = seg_off[fr], b = seg_off[fr + 1];
            a = a < 0 ? 0 : (a > nseg ? (int)nseg : a);
            b = b < a ? a : (b > nseg ? (int)nseg : b);
            int st = 0;
            for (int s = a; s < b && st == 0; ++s) st = seg_status[s];
            printf(" %d", st);
        }
        uint64_t sum = 1469598103934665603ull;                               // FNV-1a over the coefficients
        for (int16_t v : coef) {
            sum = (sum ^ (uint16_t)v) * 1099511628211ull;
        }
        printf(" checksum %llu\n", (unsigned long long)sum);
        free(data);
        free(desc);
        free(seg_off);
        free(sets);
    }
    fclose(f);
    return 0;
}
