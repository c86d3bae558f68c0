// Scoring on the pixel grid: the mask IoU of the ArTVideo protocol -- what its script computes by drawing every
// result polygon with cv2.fillPoly at image size, decoding every ground-truth RLE and ANDing two full-frame images per
// (ground truth, result) pair in a Python double loop.  Contract and the rasterisation rule: include/gomatching_hip.h; the
// statement the kernels are held to bit for bit: tests/mask_statement.py.
//
// A mask is a box (rows [y0, y1), 32-pixel word columns [wx0, wx1) in ABSOLUTE alignment: bit b of word wx is pixel
// 32 * wx + b) and its bit rows, all masks of a call in one uint32 buffer behind CSR word offsets; two masks are ANDed without
// shifts.
//
// fill_polygon_kernel / fill_rle_kernel: one block per mask, a thread OWNS a word (plain store, no atomics) and evaluates the
// rule in closed form for its 32 pixels, so nothing is stepped and nothing is sorted:
//   * fill: a crossing c = X(y) of an active edge toggles the pixels x >= (c >> 16) + 1 and sets the pixel c >> 16 when its
//     fraction is zero -- the sort-free form "b > a or a odd" as two bit masks per edge, per contour, ORed over the contours;
//   * boundary: step k of the error-stepped line sits at the minor offset (2 m k + M - 1) / (2 M) (the error stays in
//     [-2m, 2M - 2m), which fixes the number of minor steps taken), so an x-major edge covers on its row j the steps
//     ceil((2 M j - M + 1) / (2 m)) .. floor((2 M j + M) / (2 m)) -- a bit range -- and a y-major edge one pixel per row;
//   * RLE: pixel (x, y) is set when an odd number of cumulative run ends are <= x * H + y (a binary search per pixel).
// The loops over contours, edges and runs are uniform across the block; the popcount of the mask is a shuffle + LDS reduction.
// Coordinates are expected within +-2^20 (the 64-bit products then stay below 2^60); whatever they are, only the mask's own
// words are written.
//
// mask_pairs_kernel: one wave64 per ground-truth mask, as quad_pairs_kernel of score.hip: 64 detections of the frame are
// tested per round (equal key, boxes that meet), the ballot of the candidates is walked bit by bit, all lanes stride over
// the words of the box intersection with popc(a & b), a shuffle reduction gives the count to every lane, and the kept
// count / write position are wave-uniform scalars: no atomics, output independent of the launch geometry.  Offsets, boxes,
// scan and areas are device data the host cannot vouch for: every index made from them is clamped.
#include "common.h"
#include "mask_rule.h"
#include "wave_block.h"

#define MK_FILL_THREADS 256
#define MK_WAVES 4
#define MK_S 16

namespace {

__global__ __launch_bounds__(MK_FILL_THREADS) void fill_polygon_kernel(
    const int* __restrict__ points, int P, const int* __restrict__ contour_off, int C, const int* __restrict__ mask_coff,
    const int* __restrict__ boxes, const long long* __restrict__ word_off, int N, long long nwords, const int* __restrict__ sel,
    int H, int W, unsigned* __restrict__ words, int* __restrict__ area) {
    __shared__ int red[MK_FILL_THREADS / 64];
    int k = sel ? sel[blockIdx.x] : (int)blockIdx.x;
    k = clampi(k, 0, N - 1);
    const Box bx = load_box(boxes, k, H, W);
    const int NW = bx.wx1 - bx.wx0;
    const long long base = word_off[k];
    long long n = (long long)(bx.y1 - bx.y0) * NW;
    if (base < 0 || base > nwords) n = 0;
    else if (n > nwords - base) n = nwords - base;
    const int c0 = clampi(mask_coff[k], 0, C), c1 = clampi(mask_coff[k + 1], c0, C);

    int pop = 0;
    for (long long i = threadIdx.x; i < n; i += MK_FILL_THREADS) {
        const int y = bx.y0 + (int)(i / NW);
        const long long px0 = 32LL * (bx.wx0 + (int)(i % NW));        // the word's first pixel
        unsigned word = 0u;
        for (int c = c0; c < c1; ++c) {
            const int p0 = clampi(contour_off[c], 0, P), p1 = clampi(contour_off[c + 1], p0, P);
            if (p1 == p0) continue;
            unsigned parity = 0u, set = 0u;
            long long xa = points[2 * (long long)(p1 - 1)], ya = points[2 * (long long)(p1 - 1) + 1];
            for (int p = p0; p < p1; ++p) {
                const long long xb = points[2 * (long long)p], yb = points[2 * (long long)p + 1];
                // ---- fill: the edge is active on min(ya, yb) <= y < max(ya, yb)
                if (ya != yb) {
                    const bool a_top = ya < yb;
                    const long long xt = a_top ? xa : xb, yt = a_top ? ya : yb, xo = a_top ? xb : xa, yo = a_top ? yb : ya;
                    if (yt <= y && y < yo) {
                        const long long dxq = ((xo - xt) * (1LL << MK_S)) / (yo - yt);          // truncates toward zero
                        const long long pos = xt * (1LL << MK_S) + (y - yt) * dxq;
                        const long long fl = pos >> MK_S;                                        // floor
                        const long long t = fl + 1 - px0;                                        // toggles bits >= t
                        parity ^= t <= 0 ? 0xffffffffu : (t > 31 ? 0u : (0xffffffffu << (int)t));
                        if ((pos & ((1LL << MK_S) - 1)) == 0) set |= bit_range(fl - px0, fl - px0);
                    }
                }
                set |= boundary_bits(xa, ya, xb, yb, y, px0);
                xa = xb;
                ya = yb;
            }
            word |= parity | set;
        }
        word &= bit_range(0, (long long)W - 1 - px0);                 // pixels of the image only
        words[base + i] = word;
        pop += __popc(word);
    }
    const int total = wb_block_reduce<MK_FILL_THREADS, WbSum>(pop, red);   // (in thread 0)
    if (threadIdx.x == 0) area[k] = total;
}

__global__ __launch_bounds__(MK_FILL_THREADS) void fill_rle_kernel(
    const int* __restrict__ ends, int R, const int* __restrict__ run_off, const int* __restrict__ boxes,
    const long long* __restrict__ word_off, int N, long long nwords, const int* __restrict__ sel, int H, int W,
    unsigned* __restrict__ words, int* __restrict__ area) {
    __shared__ int red[MK_FILL_THREADS / 64];
    int k = sel ? sel[blockIdx.x] : (int)blockIdx.x;
    k = clampi(k, 0, N - 1);
    const Box bx = load_box(boxes, k, H, W);
    const int NW = bx.wx1 - bx.wx0;
    const long long base = word_off[k];
    long long n = (long long)(bx.y1 - bx.y0) * NW;
    if (base < 0 || base > nwords) n = 0;
    else if (n > nwords - base) n = nwords - base;
    const int r0 = clampi(run_off[k], 0, R), r1 = clampi(run_off[k + 1], r0, R);

    int pop = 0;
    for (long long i = threadIdx.x; i < n; i += MK_FILL_THREADS) {
        const int y = bx.y0 + (int)(i / NW);
        const int px0 = 32 * (bx.wx0 + (int)(i % NW));
        unsigned word = 0u;
        for (int b = 0; b < 32; ++b) {
            const int x = px0 + b;
            if (x >= W) break;
            const long long pix = (long long)x * H + y;
            int lo = r0, hi = r1;                                     // the number of ends <= pix, within [r0, r1)
            while (lo < hi) {
                const int mid = lo + ((hi - lo) >> 1);
                if ((long long)ends[mid] <= pix) lo = mid + 1;
                else hi = mid;
            }
            word |= (unsigned)((lo - r0) & 1) << b;
        }
        words[base + i] = word;
        pop += __popc(word);
    }
    const int total = wb_block_reduce<MK_FILL_THREADS, WbSum>(pop, red);   // (in thread 0)
    if (threadIdx.x == 0) area[k] = total;
}

template <bool EMIT>
__global__ __launch_bounds__(64 * MK_WAVES) void mask_pairs_kernel(
    const unsigned* __restrict__ gt_words, const int* __restrict__ gt_boxes, const long long* __restrict__ gt_woff,
    const int* __restrict__ gt_area, long long gt_nwords, const unsigned* __restrict__ det_words,
    const int* __restrict__ det_boxes, const long long* __restrict__ det_woff, const int* __restrict__ det_area,
    long long det_nwords, const int* __restrict__ gt_off, const int* __restrict__ det_off, const int* __restrict__ gt_key,
    const int* __restrict__ det_key, int G, int D, int F, double threshold, int* __restrict__ counts,
    const long long* __restrict__ scan, long long total, int* __restrict__ out_det, double* __restrict__ out_val) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const long long gl = (long long)blockIdx.x * MK_WAVES + w;
    if (gl >= G) return;                                               // no barrier below
    const int g = (int)gl;

    int lo = 0, hi = F - 1;                                            // the mask's frame: the largest f with gt_off[f] <= g
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (gt_off[mid] <= g) lo = mid;
        else hi = mid - 1;
    }
    int d0 = det_off[lo], d1 = det_off[lo + 1];
    d0 = d0 < 0 ? 0 : (d0 > D ? D : d0);
    d1 = d1 < d0 ? d0 : (d1 > D ? D : d1);
    const int nd = d1 - d0;

    const int4 gb = *reinterpret_cast<const int4*>(gt_boxes + 4 * (long long)g);         // y0, y1, wx0, wx1
    const int gnw = gb.w - gb.z;
    const long long gbase = gt_woff[g];
    const long long ag = gt_area[g];
    const int kg = gt_key[g];

    long long pos = EMIT ? scan[g] : 0;
    int kept = 0;
    for (int base = 0; base < nd; base += 64) {
        const int j = base + lane;
        bool cand = false;
        if (j < nd && det_key[d0 + j] == kg) {
            const int4 db = *reinterpret_cast<const int4*>(det_boxes + 4 * (long long)(d0 + j));
            cand = max(gb.x, db.x) < min(gb.y, db.y) && max(gb.z, db.z) < min(gb.w, db.w);
        }
        unsigned long long todo = __ballot(cand);
        while (todo) {                                                 // wave-uniform: one candidate after the other
            const int bit = __ffsll((long long)todo) - 1;
            todo &= todo - 1;
            const int jj = base + bit, d = d0 + jj;
            const int4 db = *reinterpret_cast<const int4*>(det_boxes + 4 * (long long)d);
            const int y0 = max(gb.x, db.x), y1 = min(gb.y, db.y), x0 = max(gb.z, db.z), x1 = min(gb.w, db.w);
            const int nw = x1 - x0, dnw = db.w - db.z;
            const long long dbase = det_woff[d];
            long long n = gt_nwords > 0 && det_nwords > 0 ? (long long)(y1 - y0) * nw : 0;
            n = n > gt_nwords ? gt_nwords : n;                         // an intersection has no more words than either set
            n = n > det_nwords ? det_nwords : n;
            int inter = 0;
            for (long long i = lane; i < n; i += 64) {
                const int r = (int)(i / nw), c = (int)(i % nw);
                const long long gi = clampl(gbase + (long long)(y0 + r - gb.x) * gnw + (x0 + c - gb.z), 0, gt_nwords - 1);
                const long long di = clampl(dbase + (long long)(y0 + r - db.x) * dnw + (x0 + c - db.z), 0, det_nwords - 1);
                inter += __popc(gt_words[gi] & det_words[di]);
            }
            inter = wb_wave_reduce<WbSum>(inter);
            double v = 0.0;
            if (inter >= 1) {
                const long long uni = ag + (long long)det_area[d] - inter;
                if (uni > 0) v = (double)inter / (double)uni;
            }
            if (v > threshold) {
                if (EMIT) {
                    if (lane == 0 && pos >= 0 && pos < total) {
                        out_det[pos] = jj;
                        out_val[pos] = v;
                    }
                    ++pos;
                } else {
                    ++kept;
                }
            }
        }
    }
    if (!EMIT && lane == 0) counts[g] = kept;
}

int check_fill(const void* boxes, const void* word_off, int N, long nwords, const void* sel, int M, int H, int W,
               const void* words, const void* area) {
    GOM_CHECK_ARG(N >= 0 && M >= 0 && nwords >= 0);
    GOM_CHECK_ARG(H >= 1 && W >= 1 && (long)H * (long)W <= 2147483647L);
    GOM_CHECK_ARG(sel ? M <= N : M == N);
    if (N > 0) GOM_CHECK_ARG(boxes && word_off && area);
    GOM_CHECK_ARG(((uintptr_t)boxes & 15) == 0);                       // a box is read as one 16-byte word
    if (nwords > 0) GOM_CHECK_ARG(words);
    return GOM_OK;
}

int check_pairs(const void* gt_words, const void* gt_boxes, const void* gt_woff, const void* gt_area, long gt_nwords,
                const void* det_words, const void* det_boxes, const void* det_woff, const void* det_area, long det_nwords,
                const void* gt_off, const void* det_off, const void* gt_key, const void* det_key, int G, int D, int F,
                long pairs, double threshold) {
    GOM_CHECK_ARG(G >= 0 && D >= 0 && F >= 0 && gt_nwords >= 0 && det_nwords >= 0);
    GOM_CHECK_ARG(F > 0 || (G == 0 && D == 0));
    GOM_CHECK_ARG(threshold > 0.0 && threshold < 1.0);                 // (a NaN fails both)
    GOM_CHECK_ARG(pairs >= 0 && pairs <= 2147483647L && pairs <= (long)G * (long)D);
    if (F > 0) GOM_CHECK_ARG(gt_off && det_off);
    if (G > 0) GOM_CHECK_ARG(gt_boxes && gt_woff && gt_area && gt_key);
    if (D > 0) GOM_CHECK_ARG(det_boxes && det_woff && det_area && det_key);
    GOM_CHECK_ARG(((uintptr_t)gt_boxes & 15) == 0 && ((uintptr_t)det_boxes & 15) == 0);
    if (gt_nwords > 0) GOM_CHECK_ARG(gt_words);
    if (det_nwords > 0) GOM_CHECK_ARG(det_words);
    return GOM_OK;
}

}  // namespace

extern "C" int gom_mask_fill_polygons_u32(const int32_t* points, int P, const int32_t* contour_off, int C,
                                          const int32_t* mask_coff, const int32_t* boxes, const int64_t* word_off, int N,
                                          long nwords, const int32_t* sel, int M, int H, int W, uint32_t* words,
                                          int32_t* area, void* stream) {
    const int rc = check_fill(boxes, word_off, N, nwords, sel, M, H, W, words, area);
    if (rc != GOM_OK) return rc;
    GOM_CHECK_ARG(P >= 0 && C >= 0);
    if (N > 0) GOM_CHECK_ARG(contour_off && mask_coff);
    if (P > 0) GOM_CHECK_ARG(points);
    if (M == 0) return GOM_OK;
    hipLaunchKernelGGL(fill_polygon_kernel, dim3((unsigned)M), dim3(MK_FILL_THREADS), 0, (hipStream_t)stream, points, P,
                       contour_off, C, mask_coff, boxes, (const long long*)word_off, N, (long long)nwords, sel, H, W,
                       (unsigned*)words, (int*)area);
    return gom_launch_status();
}

extern "C" int gom_mask_fill_rle_u32(const int32_t* ends, int R, const int32_t* run_off, const int32_t* boxes,
                                     const int64_t* word_off, int N, long nwords, const int32_t* sel, int M, int H, int W,
                                     uint32_t* words, int32_t* area, void* stream) {
    const int rc = check_fill(boxes, word_off, N, nwords, sel, M, H, W, words, area);
    if (rc != GOM_OK) return rc;
    GOM_CHECK_ARG(R >= 0);
    if (N > 0) GOM_CHECK_ARG(run_off);
    if (R > 0) GOM_CHECK_ARG(ends);
    if (M == 0) return GOM_OK;
    hipLaunchKernelGGL(fill_rle_kernel, dim3((unsigned)M), dim3(MK_FILL_THREADS), 0, (hipStream_t)stream, ends, R, run_off,
                       boxes, (const long long*)word_off, N, (long long)nwords, sel, H, W, (unsigned*)words, (int*)area);
    return gom_launch_status();
}

extern "C" int gom_mask_pairs_count_f64(const uint32_t* gt_words, const int32_t* gt_boxes, const int64_t* gt_woff,
                                        const int32_t* gt_area, long gt_nwords, const uint32_t* det_words,
                                        const int32_t* det_boxes, const int64_t* det_woff, const int32_t* det_area,
                                        long det_nwords, const int32_t* gt_off, const int32_t* det_off,
                                        const int32_t* gt_key, const int32_t* det_key, int G, int D, int F, long pairs,
                                        double threshold, int32_t* counts, void* stream) {
    const int rc = check_pairs(gt_words, gt_boxes, gt_woff, gt_area, gt_nwords, det_words, det_boxes, det_woff, det_area,
                               det_nwords, gt_off, det_off, gt_key, det_key, G, D, F, pairs, threshold);
    if (rc != GOM_OK) return rc;
    if (G == 0) return GOM_OK;
    GOM_CHECK_ARG(counts);
    hipLaunchKernelGGL(mask_pairs_kernel<false>, dim3((unsigned)cdiv((long)G, (long)MK_WAVES)), dim3(64 * MK_WAVES), 0,
                       (hipStream_t)stream, (const unsigned*)gt_words, gt_boxes, (const long long*)gt_woff, gt_area,
                       (long long)gt_nwords, (const unsigned*)det_words, det_boxes, (const long long*)det_woff, det_area,
                       (long long)det_nwords, gt_off, det_off, gt_key, det_key, G, D, F, threshold, (int*)counts,
                       (const long long*)nullptr, 0LL, (int*)nullptr, (double*)nullptr);
    return gom_launch_status();
}

extern "C" int gom_mask_pairs_emit_f64(const uint32_t* gt_words, const int32_t* gt_boxes, const int64_t* gt_woff,
                                       const int32_t* gt_area, long gt_nwords, const uint32_t* det_words,
                                       const int32_t* det_boxes, const int64_t* det_woff, const int32_t* det_area,
                                       long det_nwords, const int32_t* gt_off, const int32_t* det_off,
                                       const int32_t* gt_key, const int32_t* det_key, int G, int D, int F, long pairs,
                                       double threshold, const int64_t* scan, long total, int32_t* out_det,
                                       double* out_val, void* stream) {
    const int rc = check_pairs(gt_words, gt_boxes, gt_woff, gt_area, gt_nwords, det_words, det_boxes, det_woff, det_area,
                               det_nwords, gt_off, det_off, gt_key, det_key, G, D, F, pairs, threshold);
    if (rc != GOM_OK) return rc;
    GOM_CHECK_ARG(total >= 0 && total <= pairs);
    if (G == 0 || total == 0) return GOM_OK;
    GOM_CHECK_ARG(scan && out_det && out_val);
    hipLaunchKernelGGL(mask_pairs_kernel<true>, dim3((unsigned)cdiv((long)G, (long)MK_WAVES)), dim3(64 * MK_WAVES), 0,
                       (hipStream_t)stream, (const unsigned*)gt_words, gt_boxes, (const long long*)gt_woff, gt_area,
                       (long long)gt_nwords, (const unsigned*)det_words, det_boxes, (const long long*)det_woff, det_area,
                       (long long)det_nwords, gt_off, det_off, gt_key, det_key, G, D, F, threshold, (int*)nullptr,
                       (const long long*)scan, (long long)total, (int*)out_det, (double*)out_val);
    return gom_launch_status();
}
