// The JPEG decoder's chunked entropy walk (gomatching_amd/csrc/jpeg_decode_chunks.h) on the host, for a run under the host
// compiler's sanitizers: the functions the kernel calls, over the same uploads, with a span's lanes run one after another --
// sub-steps (a) .. (e) of the rule in include/gomatching_hip.h and the same bounded settling loop.  A segment the chunk walk
// marks goes through gom_jd_walk_segment, as the serial kernel does behind the chunk launch.
//
//   jpeg_decode_chunks_hostcheck DUMP CHUNK_BYTES
//
// DUMP: the format of tools/jpeg_decode_hostcheck.cpp (written from jpeg.plan), all little-endian:
//   int64  ncalls
//   per call: int64 F, H, W, ncomp, hs, vs, nbytes, nseg, nsets
//             u8 data[nbytes]; int64 desc[nseg][8]; int32 seg_off[F+1]; int32 sets[nsets][2392]
// Every array is copied into an allocation of exactly its size, so that a read one byte outside it is the sanitizer's to report.
// Output: one line per call, "call I: status s0 s1 ... checksum C routes r0 r1 ... passes P" (frame status words; a checksum of
// the coefficients; per segment 0 = chunks, 1 = serial; the largest pass count of the call).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../gomatching_amd/csrc/jpeg_decode_chunks.h"

static bool read_exact(FILE* f, void* dst, size_t n) { return n == 0 || fread(dst, 1, n, f) == n; }

// -> route (0: the chunk walk finished the segment; 1: it marked it); passes = the most settling passes of a span
static int chunk_walk(const uint8_t* data, long nbytes, const GomJdDesc& d, const int32_t* set, const GomJdGeom& g, int chunk_bytes,
                      int16_t* out, int& passes) {
    passes = 0;
    GomJcSeg sg;
    if (!gom_jc_segment(sg, data, nbytes, d, set, g)) return 1;
    for (long o = 0; o < sg.blocks; ++o) {                                       // the zeros in front
        const long bi = gom_jc_block_index(g, sg, d.m0, o);
        if (bi >= 0) memset(out + bi * 64, 0, 128);
    }
    const int lanes = GOM_JC_LANES(chunk_bytes);
    const long nchunks = gom_jc_chunks(sg, chunk_bytes);
    GomJcPoint truth = {sg.start, 0, 0, 0};
    long carry_blocks = 0;
    uint32_t carry_dc0 = 0, carry_dc1 = 0, carry_dc2 = 0;
    int status = GOM_JD_OK, closed = -1;
    std::vector<GomJcPoint> entry(lanes), exit(lanes), next(lanes);
    std::vector<GomJcTotals> tot(lanes);
    GomJcWrite none = {};
    int unused = 0;
    for (long c0 = 0; c0 < nchunks && carry_blocks < sg.blocks && status == GOM_JD_OK; c0 += lanes) {
        const int act = nchunks - c0 < lanes ? (int)(nchunks - c0) : lanes;
        auto stop_of = [&](int t) {
            const long e = sg.base + (c0 + t + 1) * chunk_bytes;
            return e < sg.end ? e : sg.end;
        };
        for (int t = 0; t < act; ++t) {                                          // (a) the cold walk
            entry[t] = t == 0 ? truth : gom_jc_guess(sg, sg.base + (c0 + t) * chunk_bytes);
            gom_jc_walk<false>(sg, g, nullptr, 0, 0, entry[t], stop_of(t), exit[t], tot[t], none, unused, unused);
        }
        int p = 0;
        for (int pass = 0; pass < GOM_JC_MAX_LANES; ++pass) {                    // (b) settling: every lane reads, then the changed walk
            bool any = false;
            for (int t = 0; t < act; ++t) {
                next[t] = t == 0 ? entry[0] : exit[t - 1];
                any = any || !gom_jc_same(next[t], entry[t]);
            }
            if (!any) break;
            ++p;
            for (int t = 0; t < act; ++t)
                if (!gom_jc_same(next[t], entry[t])) {
                    entry[t] = next[t];
                    gom_jc_walk<false>(sg, g, nullptr, 0, 0, entry[t], stop_of(t), exit[t], tot[t], none, unused, unused);
                }
        }
        passes = p > passes ? p : passes;
        for (int t = 0; t < act; ++t) {                                          // (c), (d) the exclusive scans; (e) the write walk
            GomJcWrite w;
            w.ordinal = carry_blocks;
            w.pred0 = carry_dc0;
            w.pred1 = carry_dc1;
            w.pred2 = carry_dc2;
            w.m0 = d.m0;
            w.limit = d.limit;
            w.rst = d.rst;
            w.out = out;
            GomJcPoint e;
            GomJcTotals x;
            gom_jc_walk<true>(sg, g, nullptr, 0, 0, entry[t], stop_of(t), e, x, w, status, closed);
            carry_blocks += tot[t].blocks;
            carry_dc0 += tot[t].dc0;
            carry_dc1 += tot[t].dc1;
            carry_dc2 += tot[t].dc2;
        }
        truth = exit[act - 1];
    }
    return (status == GOM_JD_OK && closed == GOM_JD_OK) ? 0 : 1;
}

int main(int argc, char** argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: %s DUMP CHUNK_BYTES\n", argv[0]);
        return 2;
    }
    const int chunk_bytes = atoi(argv[2]);
    if (!GOM_JC_CHUNK_OK(chunk_bytes)) {
        fprintf(stderr, "CHUNK_BYTES must be a power of two in %d .. %d\n", GOM_JC_MIN_CHUNK, GOM_JC_MAX_CHUNK);
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
        std::vector<int16_t> coef((size_t)F * g.nblk * 64, (int16_t)-1);         // (-1: what the walk does not write must be cleared)
        std::vector<int> seg_status((size_t)nseg, 0), route((size_t)nseg, 1);
        int most = 0;
        for (int64_t s = 0; s < nseg; ++s) {
            const GomJdDesc d = gom_jd_desc(desc + s * GOM_JD_DESC_WORDS);
            if (d.frame < 0 || d.frame >= F || d.set < 0 || d.set >= nsets) {    // as the kernels
                seg_status[s] = GOM_JD_PAST_END;
                continue;
            }
            int16_t* out = coef.data() + d.frame * g.nblk * 64;
            int passes = 0;
            route[s] = chunk_walk(data, (long)nbytes, d, sets + d.set * GOM_JD_SET_WORDS, g, chunk_bytes, out, passes);
            most = passes > most ? passes : most;
            if (route[s] == 0) continue;
            int16_t blk[64];
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
        uint64_t sum = 1469598103934665603ull;                                   // FNV-1a over the coefficients
        for (int16_t v : coef) sum = (sum ^ (uint16_t)v) * 1099511628211ull;
        printf(" checksum %llu routes", (unsigned long long)sum);
        for (int64_t s = 0; s < nseg; ++s) printf(" %d", route[s]);
        printf(" passes %d\n", most);
        free(data);
        free(desc);
        free(seg_off);
        free(sets);
    }
    fclose(f);
    return 0;
}
