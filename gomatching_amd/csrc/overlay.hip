// Drawing tracked text on frames: what the reference's visualizer does with one matplotlib patch and one text
// artist per instance per frame, as an outline pass over the bit-row masks of csrc/mask_pairs.hip and one compositor launch
// per clip.  Contract and the integer rule: include/gomatching_hip.h; the statement the kernels are held to bit for bit:
// tests/overlay_statement.py.
//
// outline_polygon_kernel: fill_polygon_kernel of csrc/mask_pairs.hip without Fill -- one block per mask, a thread OWNS a word
// and ORs the closed form of Boundary (mask_rule.h) over the edges of the mask's contours.  Plain stores, no area.
//
// compose_kernel: one wave64 per 256-pixel row segment (eight absolute 32-pixel word columns of one row of one frame), a lane
// per 4 pixels -- 12 bytes of the frame, 4 bits of ONE mask word -- grid-strided over the segments.  The wave culls the
// frame's instances 64 per round -- lane j tests instance j's box against the segment -- and walks the ballot from its
// lowest bit, which keeps instance order; the box, the word offset and the colour of a candidate are wave-uniform loads and
// its words one load per 8 lanes.  Labels follow the same way, after all instances.  No LDS, no barrier, no atomics: a pixel
// is read once and written once by its own lane, so `out` may be `frames`, and the result does not depend on the launch
// geometry.  Rows are 3 W bytes and start at any byte alignment: a lane moves its 12 bytes as three dwords where they are
// 4-byte aligned (lanes are 12 bytes apart, so a wave's lanes agree) and byte by byte otherwise and at the ragged end of a row.
// compose_gather_kernel is the same body with one other source address: frame f is read from slot slots[f] of a ring of frames
// (the online session's pending frames, online.py) and written to a dense `out` -- one launch whatever the ring's wrap, and no
// index_select pass over F H W 3 bytes first.  The slot is clamped into the ring; the `wide` test stays per address.
// Offsets, boxes, positions and atlas indices are device data the host cannot vouch for: every index made from them is clamped
// or tested against its buffer.
#include "common.h"
#include "mask_rule.h"

#define OV_FILL_THREADS 256
#define OV_WAVES 4
#define OV_MAX_BLOCKS 8192
#define OV_PX 4                                                        // pixels of a lane: 12 bytes, 4 bits of one mask word
#define OV_SEG (64 * OV_PX)                                            // pixels of a wave: a row segment of 8 word columns

namespace {

__global__ __launch_bounds__(OV_FILL_THREADS) void outline_polygon_kernel(
    const int* __restrict__ points, int P, const int* __restrict__ contour_off, int C, const int* __restrict__ mask_coff,
    const int* __restrict__ boxes, const long long* __restrict__ word_off, int N, long long nwords, const int* __restrict__ sel,
    int H, int W, unsigned* __restrict__ words) {
    int k = sel ? sel[blockIdx.x] : (int)blockIdx.x;
    k = clampi(k, 0, N - 1);
    const Box bx = load_box(boxes, k, H, W);
    const int NW = bx.wx1 - bx.wx0;
    const long long base = word_off[k];
    long long n = (long long)(bx.y1 - bx.y0) * NW;
    if (base < 0 || base > nwords) n = 0;
    else if (n > nwords - base) n = nwords - base;
    const int c0 = clampi(mask_coff[k], 0, C), c1 = clampi(mask_coff[k + 1], c0, C);

    for (long long i = threadIdx.x; i < n; i += OV_FILL_THREADS) {
        const int y = bx.y0 + (int)(i / NW);
        const long long px0 = 32LL * (bx.wx0 + (int)(i % NW));        // the word's first pixel
        unsigned word = 0u;
        for (int c = c0; c < c1; ++c) {
            const int p0 = clampi(contour_off[c], 0, P), p1 = clampi(contour_off[c + 1], p0, P);
            if (p1 == p0) continue;
            long long xa = points[2 * (long long)(p1 - 1)], ya = points[2 * (long long)(p1 - 1) + 1];
            for (int p = p0; p < p1; ++p) {
                const long long xb = points[2 * (long long)p], yb = points[2 * (long long)p + 1];
                word |= boundary_bits(xa, ya, xb, yb, y, px0);
                xa = xb;
                ya = yb;
            }
        }
        word &= bit_range(0, (long long)W - 1 - px0);                 // pixels of the image only
        words[base + i] = word;
    }
}

// blend(p, c, a) = (p (255 - a) + c a + 127) / 255
__device__ __forceinline__ int blend(int p, int c, int a) { return (p * (255 - a) + c * a + 127) / 255; }

// The body of both compose kernels.  GATHER = false: frame f is read from frames[f] (the dense entry, `out` may be `frames`).
// GATHER = true: `frames` is a ring of `cap` frames and frame f is read from ring[slots[f]], the slot clamped into the ring;
// `out` is dense and never the ring, so every live pixel is written.  Only the source address differs.
template <bool GATHER>
__device__ __forceinline__ void compose_body(
    const unsigned char* frames, int cap, const int* __restrict__ slots, unsigned char* out, int F, int H, int W,
    const unsigned* __restrict__ face_words, const unsigned* __restrict__ outline_words, const int* __restrict__ boxes,
    const long long* __restrict__ word_off, int N,
    long long nwords, const int* __restrict__ inst_off, const unsigned char* __restrict__ inst_rgb,
    const int* __restrict__ label_off, const int* __restrict__ label_pos, const int* __restrict__ label_glyph,
    const unsigned char* __restrict__ label_rgb, int L, const int* __restrict__ glyph_wh,
    const long long* __restrict__ glyph_woff, const unsigned* __restrict__ glyph_words, int G, long long glyph_nwords,
    int a_face, int a_box) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int CG = (W + OV_SEG - 1) / OV_SEG;                          // segments of a row
    const long long tasks = (long long)F * H * CG;
    for (long long t = (long long)blockIdx.x * OV_WAVES + w; t < tasks; t += (long long)gridDim.x * OV_WAVES) {
        const int cg = (int)(t % CG);
        const int y = (int)((t / CG) % H);
        const int f = (int)(t / ((long long)CG * H));
        const int x = OV_SEG * cg + OV_PX * lane;                      // the lane's first pixel: OV_PX pixels of ONE word
        const int wx = x >> 5, bit = x & 31;
        const int wlo = (OV_SEG >> 5) * cg, whi = wlo + (OV_SEG >> 5); // the segment's word columns
        const int live = clampi(W - x, 0, OV_PX);
        const long long pix = 3 * (((long long)f * H + y) * W + x);
        const long long spix = GATHER ? 3 * (((long long)clampi(slots[f], 0, cap - 1) * H + y) * W + x) : pix;   // the source
        // 12 bytes as three dwords where they are 4-byte aligned (every lane of a wave, or none: lanes are 12 bytes apart)
        const bool wide = live == OV_PX && (((uintptr_t)(frames + spix) | (uintptr_t)(out + pix)) & 3) == 0;
        int v[OV_PX][3];
        if (wide) {
            const unsigned* src = reinterpret_cast<const unsigned*>(frames + spix);
            const unsigned d[3] = {src[0], src[1], src[2]};
#pragma unroll
            for (int i = 0; i < 3 * OV_PX; ++i) v[i / 3][i % 3] = d[i >> 2] >> (8 * (i & 3)) & 255u;
        } else {
#pragma unroll
            for (int i = 0; i < 3 * OV_PX; ++i) v[i / 3][i % 3] = i < 3 * live ? frames[spix + i] : 0;
        }
        bool touched = false;

        // ---- instances, in order
        const int i0 = clampi(inst_off[f], 0, N), i1 = clampi(inst_off[f + 1], i0, N);
        for (int base = i0; base < i1; base += 64) {
            bool cand = false;
            if (base + lane < i1) {
                const Box bx = load_box(boxes, base + lane, H, W);
                cand = bx.y0 <= y && y < bx.y1 && bx.wx0 < whi && wlo < bx.wx1;
            }
            unsigned long long todo = __ballot(cand);
            while (todo) {                                             // wave-uniform: one candidate after the other
                const int k = base + __ffsll((long long)todo) - 1;
                todo &= todo - 1;
                const Box bx = load_box(boxes, k, H, W);
                const long long wbase = word_off[k];
                const long long i = (long long)(y - bx.y0) * (bx.wx1 - bx.wx0) + (wx - bx.wx0);
                // the words the fill kernels gave this mask: the box's, cut back to the buffer
                if (wx >= bx.wx0 && wx < bx.wx1 && wbase >= 0 && wbase <= nwords && i < nwords - wbase) {
                    const unsigned mo = outline_words[wbase + i] >> bit, mf = face_words[wbase + i] >> bit;
                    if ((mo | mf) & ((1u << OV_PX) - 1)) {
                        const int c[3] = {inst_rgb[3 * (long long)k], inst_rgb[3 * (long long)k + 1], inst_rgb[3 * (long long)k + 2]};
#pragma unroll
                        for (int j = 0; j < OV_PX; ++j) {
                            const bool o = mo >> j & 1u, fc = mf >> j & 1u;
#pragma unroll
                            for (int ch = 0; ch < 3; ++ch) v[j][ch] = o ? c[ch] : (fc ? blend(v[j][ch], c[ch], a_face) : v[j][ch]);
                        }
                        touched = true;
                    }
                }
            }
        }

        // ---- labels, in order, above every instance
        const int l0 = clampi(label_off[f], 0, L), l1 = clampi(label_off[f + 1], l0, L);
        for (int base = l0; base < l1; base += 64) {
            bool cand = false;
            if (base + lane < l1) {
                const int k = base + lane;
                const int gi = clampi(label_glyph[k], 0, G - 1);
                const long long x0 = label_pos[2 * (long long)k], y0 = label_pos[2 * (long long)k + 1];
                const long long gw = glyph_wh[2 * (long long)gi], gh = glyph_wh[2 * (long long)gi + 1];
                cand = y0 <= y && y < y0 + gh && x0 < (long long)OV_SEG * (cg + 1) && (long long)OV_SEG * cg < x0 + gw;
            }
            unsigned long long todo = __ballot(cand);
            while (todo) {
                const int k = base + __ffsll((long long)todo) - 1;
                todo &= todo - 1;
                const int gi = clampi(label_glyph[k], 0, G - 1);
                const long long x0 = label_pos[2 * (long long)k], y0 = label_pos[2 * (long long)k + 1];
                const long long gw = glyph_wh[2 * (long long)gi];
                const long long ly = y - y0;                           // 0 <= ly < gh: the candidate test
                if (x + OV_PX > x0 && x < x0 + gw) {
                    const long long gbase = glyph_woff[gi];
                    const int c[3] = {label_rgb[3 * (long long)k], label_rgb[3 * (long long)k + 1], label_rgb[3 * (long long)k + 2]};
#pragma unroll
                    for (int j = 0; j < OV_PX; ++j) {
                        const long long lx = x + j - x0;
                        if (lx < 0 || lx >= gw) continue;
                        const long long i = ly * ((gw + 31) >> 5) + (lx >> 5);
                        unsigned on = 0u;
                        if (gbase >= 0 && gbase <= glyph_nwords && i < glyph_nwords - gbase) on = glyph_words[gbase + i] >> (lx & 31) & 1u;
#pragma unroll
                        for (int ch = 0; ch < 3; ++ch) v[j][ch] = on ? c[ch] : blend(v[j][ch], 255, a_box);
                    }
                    touched = true;
                }
            }
        }

        if (live > 0 && (GATHER || touched || out != frames)) {
            if (wide) {
                unsigned d[3] = {0u, 0u, 0u};
#pragma unroll
                for (int i = 0; i < 3 * OV_PX; ++i) d[i >> 2] |= (unsigned)v[i / 3][i % 3] << (8 * (i & 3));
                unsigned* dst = reinterpret_cast<unsigned*>(out + pix);
                dst[0] = d[0];
                dst[1] = d[1];
                dst[2] = d[2];
            } else {
#pragma unroll
                for (int i = 0; i < 3 * OV_PX; ++i)
                    if (i < 3 * live) out[pix + i] = (unsigned char)v[i / 3][i % 3];
            }
        }
    }
}

#define OV_COMPOSE_PARAMS                                                                                                        \
    int F, int H, int W, const unsigned *__restrict__ face_words, const unsigned *__restrict__ outline_words,                    \
        const int *__restrict__ boxes, const long long *__restrict__ word_off, int N, long long nwords,                          \
        const int *__restrict__ inst_off, const unsigned char *__restrict__ inst_rgb, const int *__restrict__ label_off,         \
        const int *__restrict__ label_pos, const int *__restrict__ label_glyph, const unsigned char *__restrict__ label_rgb,     \
        int L, const int *__restrict__ glyph_wh, const long long *__restrict__ glyph_woff,                                       \
        const unsigned *__restrict__ glyph_words, int G, long long glyph_nwords, int a_face, int a_box
#define OV_COMPOSE_ARGS                                                                                                          \
    F, H, W, face_words, outline_words, boxes, word_off, N, nwords, inst_off, inst_rgb, label_off, label_pos, label_glyph,       \
        label_rgb, L, glyph_wh, glyph_woff, glyph_words, G, glyph_nwords, a_face, a_box

__global__ __launch_bounds__(64 * OV_WAVES) void compose_kernel(const unsigned char* frames, unsigned char* out,
                                                                OV_COMPOSE_PARAMS) {
    compose_body<false>(frames, 0, nullptr, out, OV_COMPOSE_ARGS);
}

__global__ __launch_bounds__(64 * OV_WAVES) void compose_gather_kernel(const unsigned char* ring, int cap,
                                                                       const int* __restrict__ slots, unsigned char* out,
                                                                       OV_COMPOSE_PARAMS) {
    compose_body<true>(ring, cap, slots, out, OV_COMPOSE_ARGS);
}

}  // namespace

extern "C" int gom_mask_outline_polygons_u32(const int32_t* points, int P, const int32_t* contour_off, int C,
                                             const int32_t* mask_coff, const int32_t* boxes, const int64_t* word_off, int N,
                                             long nwords, const int32_t* sel, int M, int H, int W, uint32_t* words,
                                             void* stream) {
    GOM_CHECK_ARG(N >= 0 && M >= 0 && nwords >= 0 && P >= 0 && C >= 0);
    GOM_CHECK_ARG(H >= 1 && W >= 1 && (long)H * (long)W <= 2147483647L);
    GOM_CHECK_ARG(sel ? M <= N : M == N);
    if (N > 0) GOM_CHECK_ARG(boxes && word_off && contour_off && mask_coff);
    GOM_CHECK_ARG(((uintptr_t)boxes & 15) == 0);                       // a box is read as one 16-byte word
    if (nwords > 0) GOM_CHECK_ARG(words);
    if (P > 0) GOM_CHECK_ARG(points);
    if (M == 0) return GOM_OK;
    hipLaunchKernelGGL(outline_polygon_kernel, dim3((unsigned)M), dim3(OV_FILL_THREADS), 0, (hipStream_t)stream, points, P,
                       contour_off, C, mask_coff, boxes, (const long long*)word_off, N, (long long)nwords, sel, H, W,
                       (unsigned*)words);
    return gom_launch_status();
}

extern "C" int gom_overlay_compose_u8(const uint8_t* frames, uint8_t* out, int F, int H, int W, const uint32_t* face_words,
                                      const uint32_t* outline_words, const int32_t* boxes, const int64_t* word_off, int N,
                                      long nwords, const int32_t* inst_off, const uint8_t* inst_rgb, const int32_t* label_off,
                                      const int32_t* label_pos, const int32_t* label_glyph, const uint8_t* label_rgb, int L,
                                      const int32_t* glyph_wh, const int64_t* glyph_woff, const uint32_t* glyph_words, int G,
                                      long glyph_nwords, int a_face, int a_box, void* stream) {
    GOM_CHECK_ARG(F >= 0 && N >= 0 && L >= 0 && G >= 0 && nwords >= 0 && glyph_nwords >= 0);
    GOM_CHECK_ARG(H >= 1 && W >= 1 && (long)H * (long)W <= 2147483647L);
    GOM_CHECK_ARG(a_face >= 0 && a_face <= 255 && a_box >= 0 && a_box <= 255);
    GOM_CHECK_ARG(((uintptr_t)boxes & 15) == 0);                       // a box is read as one 16-byte word
    if (F == 0) return GOM_OK;
    GOM_CHECK_ARG(frames && out && inst_off && label_off);
    if (N > 0) GOM_CHECK_ARG(boxes && word_off && inst_rgb);
    if (N > 0 && nwords > 0) GOM_CHECK_ARG(face_words && outline_words);
    if (L > 0) GOM_CHECK_ARG(G > 0 && label_pos && label_glyph && label_rgb);
    if (G > 0) GOM_CHECK_ARG(glyph_wh && glyph_woff);
    if (glyph_nwords > 0) GOM_CHECK_ARG(glyph_words);
    if (N == 0 && L == 0 && out == frames) return GOM_OK;              // nothing to draw, nothing to copy
    const long waves = (long)F * (long)H * (long)((W + OV_SEG - 1) / OV_SEG);
    const long blocks = (waves + OV_WAVES - 1) / OV_WAVES;
    hipLaunchKernelGGL(compose_kernel, dim3((unsigned)(blocks < OV_MAX_BLOCKS ? blocks : OV_MAX_BLOCKS)), dim3(64 * OV_WAVES), 0,
                       (hipStream_t)stream, frames, out, F, H, W, (const unsigned*)face_words, (const unsigned*)outline_words,
                       boxes, (const long long*)word_off, N, (long long)nwords, inst_off, inst_rgb, label_off, label_pos,
                       label_glyph, label_rgb, L, glyph_wh, (const long long*)glyph_woff, (const unsigned*)glyph_words, G,
                       (long long)glyph_nwords, a_face, a_box);
    return gom_launch_status();
}

extern "C" int gom_overlay_compose_gather_u8(const uint8_t* ring, int cap, const int32_t* slots, uint8_t* out, int F, int H, int W,
                                             const uint32_t* face_words, const uint32_t* outline_words, const int32_t* boxes,
                                             const int64_t* word_off, int N, long nwords, const int32_t* inst_off,
                                             const uint8_t* inst_rgb, const int32_t* label_off, const int32_t* label_pos,
                                             const int32_t* label_glyph, const uint8_t* label_rgb, int L, const int32_t* glyph_wh,
                                             const int64_t* glyph_woff, const uint32_t* glyph_words, int G, long glyph_nwords,
                                             int a_face, int a_box, void* stream) {
    GOM_CHECK_ARG(F >= 0 && N >= 0 && L >= 0 && G >= 0 && nwords >= 0 && glyph_nwords >= 0 && cap >= 1);
    GOM_CHECK_ARG(H >= 1 && W >= 1 && (long)H * (long)W <= 2147483647L);
    GOM_CHECK_ARG(a_face >= 0 && a_face <= 255 && a_box >= 0 && a_box <= 255);
    GOM_CHECK_ARG(((uintptr_t)boxes & 15) == 0);                       // a box is read as one 16-byte word
    if (F == 0) return GOM_OK;
    GOM_CHECK_ARG(ring && slots && out && inst_off && label_off);
    {                                                                  // the ring is only read: `out` lies wholly outside it
        const uintptr_t frame = 3u * (uintptr_t)H * (uintptr_t)W;
        const uintptr_t r0 = (uintptr_t)ring, r1 = r0 + (uintptr_t)cap * frame, o0 = (uintptr_t)out, o1 = o0 + (uintptr_t)F * frame;
        GOM_CHECK_ARG(o1 <= r0 || r1 <= o0);
    }
    if (N > 0) GOM_CHECK_ARG(boxes && word_off && inst_rgb);
    if (N > 0 && nwords > 0) GOM_CHECK_ARG(face_words && outline_words);
    if (L > 0) GOM_CHECK_ARG(G > 0 && label_pos && label_glyph && label_rgb);
    if (G > 0) GOM_CHECK_ARG(glyph_wh && glyph_woff);
    if (glyph_nwords > 0) GOM_CHECK_ARG(glyph_words);
    const long waves = (long)F * (long)H * (long)((W + OV_SEG - 1) / OV_SEG);
    const long blocks = (waves + OV_WAVES - 1) / OV_WAVES;
    hipLaunchKernelGGL(compose_gather_kernel, dim3((unsigned)(blocks < OV_MAX_BLOCKS ? blocks : OV_MAX_BLOCKS)),
                       dim3(64 * OV_WAVES), 0, (hipStream_t)stream, ring, cap, slots, out, F, H, W, (const unsigned*)face_words,
                       (const unsigned*)outline_words, boxes, (const long long*)word_off, N, (long long)nwords, inst_off, inst_rgb,
                       label_off, label_pos, label_glyph, label_rgb, L, glyph_wh, (const long long*)glyph_woff,
                       (const unsigned*)glyph_words, G, (long long)glyph_nwords, a_face, a_box);
    return gom_launch_status();
}
