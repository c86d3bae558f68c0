// The scene of parsed rows: what show.Scene / score_json.MaskSet build on the host for a chunk of frames, made from the arrays the
// result parser left on the device (THE RULE: include/gomatching_hip.h, `gom_scene_polygons_i32`).
//
//   boxes : a lane per instance of the chunk walks the instance's points (50 of them in a result file): the extent, clamped to the
//           frame and cut to 32-pixel words as MaskSet does it, the colour of the track, and a status word.
//   scan  : ONE block of GOM_SP_BLOCK threads, tiles of the block with a carry: the kept contours before every instance (mcoff) and
//           the words before it (woff, int64), coff at the places mcoff names, inst_off, and the OR of the status words.
//
// No atomics, no scratch, one writer per output word.  The offsets are data: every one is clamped into its array before it is used
// as an index, and every store index is compared with the length the caller gave.
#include "common.h"
#include "wave_block.h"

namespace {

__device__ __forceinline__ int sp_clamp(long v, long lo, long hi) { return (int)(v < lo ? lo : (v > hi ? hi : v)); }

struct SpIn {
    const int32_t* frame_rows;
    const int64_t* ids;
    const int32_t* poly_off;
    const int32_t* poly_xy;
    int F, N, P, f0, f1, H, W;
};

// the chunk's first row, its rows, and its first point
__device__ __forceinline__ void sp_chunk(const SpIn& in, int& i0, int& count, int& p0) {
    i0 = sp_clamp(in.frame_rows[in.f0], 0, in.N);
    const int i1 = sp_clamp(in.frame_rows[in.f1], i0, in.N);
    count = i1 - i0;
    p0 = sp_clamp(in.poly_off[i0], 0, in.P);
}

// the points of row i: [a, b) inside [0, P)
__device__ __forceinline__ void sp_points(const SpIn& in, int i, int& a, int& b) {
    a = sp_clamp(in.poly_off[i], 0, in.P);
    b = sp_clamp(in.poly_off[i + 1], a, in.P);
}

__global__ __launch_bounds__(GOM_SP_BLOCK) void scene_boxes_kernel(SpIn in, const unsigned char* __restrict__ palette, int bgr,
                                                                   int32_t* __restrict__ boxes,
                                                                   unsigned char* __restrict__ inst_rgb,
                                                                   int32_t* __restrict__ inst_status, int n_inst) {
    const long k = (long)blockIdx.x * GOM_SP_BLOCK + threadIdx.x;
    int i0, count, p0;
    sp_chunk(in, i0, count, p0);
    if (k >= n_inst) return;
    int st = 0, y0 = 0, y1 = 0, wx0 = 0, wx1 = 0;
    int r = 0, g = 0, b = 0;
    if (k < count) {
        const int i = i0 + (int)k;
        int a, e;
        sp_points(in, i, a, e);
        int xmin = 2147483647, xmax = -2147483647 - 1, ymin = 2147483647, ymax = -2147483647 - 1;
        for (int p = a; p < e; ++p) {
            const int2 v = *reinterpret_cast<const int2*>(in.poly_xy + 2L * p);
            xmin = min(xmin, v.x), xmax = max(xmax, v.x), ymin = min(ymin, v.y), ymax = max(ymax, v.y);
        }
        if (e > a) {
            if (xmin < -GOM_SP_MAX_COORD || ymin < -GOM_SP_MAX_COORD || xmax > GOM_SP_MAX_COORD || ymax > GOM_SP_MAX_COORD)
                st = GOM_SP_BAD_COORD;
            const int x0 = max(xmin, 0), x1 = min(xmax, in.W - 1), ya = max(ymin, 0), yb = min(ymax, in.H - 1);
            if (x0 <= x1 && ya <= yb) y0 = ya, y1 = yb + 1, wx0 = x0 >> 5, wx1 = (x1 >> 5) + 1;
        }
        long m = in.ids[i] % GOM_SP_PALETTE;
        if (m < 0) m += GOM_SP_PALETTE;
        r = palette[3 * m], g = palette[3 * m + 1], b = palette[3 * m + 2];
    } else {
        st = GOM_SP_BAD_SHAPE;
    }
    *reinterpret_cast<int4*>(boxes + 4 * k) = make_int4(y0, y1, wx0, wx1);
    inst_rgb[3 * k] = (unsigned char)(bgr ? b : r);
    inst_rgb[3 * k + 1] = (unsigned char)g;
    inst_rgb[3 * k + 2] = (unsigned char)(bgr ? r : b);
    inst_status[k] = st;
}

__global__ __launch_bounds__(GOM_SP_BLOCK) void scene_scan_kernel(SpIn in, const int32_t* __restrict__ boxes,
                                                                  const int32_t* __restrict__ inst_status, int n_inst,
                                                                  int32_t* __restrict__ coff, int n_cont,
                                                                  int32_t* __restrict__ mcoff, int64_t* __restrict__ woff,
                                                                  int32_t* __restrict__ inst_off, int32_t* __restrict__ status) {
    __shared__ int wc[GOM_SP_BLOCK / 64];
    __shared__ long long ww[GOM_SP_BLOCK / 64];
    __shared__ int ws[GOM_SP_BLOCK / 64];
    int i0, count, p0;
    sp_chunk(in, i0, count, p0);
    int cc = 0, st = count == n_inst ? 0 : GOM_SP_BAD_SHAPE;
    long long cw = 0;
    for (long base = 0; base < n_inst; base += GOM_SP_BLOCK) {
        const long k = base + threadIdx.x;
        int kept = 0, a = 0;
        long long words = 0;
        if (k < n_inst) {
            const int4 bx = *reinterpret_cast<const int4*>(boxes + 4 * k);
            words = (long long)(bx.y - bx.x) * (bx.w - bx.z);
            st |= inst_status[k];
            if (k < count) {
                int e;
                sp_points(in, i0 + (int)k, a, e);
                kept = e > a ? 1 : 0;
            }
        }
        const int c = wb_block_excl_scan_carry<GOM_SP_BLOCK>(kept, wc, cc);
        const long long w = wb_block_excl_scan_carry<GOM_SP_BLOCK>(words, ww, cw);
        if (k < n_inst) {
            mcoff[k] = c;
            woff[k] = w;
            if (kept) {
                if (c < n_cont) coff[c] = a - p0;
                else st |= GOM_SP_BAD_SHAPE;
            }
        }
    }
    for (long j = threadIdx.x; j <= in.f1 - in.f0; j += GOM_SP_BLOCK)
        inst_off[j] = sp_clamp((long)in.frame_rows[in.f0 + j] - i0, 0, n_inst);
    int all = wb_block_reduce<GOM_SP_BLOCK, WbOr>(st, ws);
    if (threadIdx.x == 0) {
        if (cc != n_cont) all |= GOM_SP_BAD_SHAPE;
        mcoff[n_inst] = cc;
        woff[n_inst] = cw;
        int a, e = p0;
        if (count > 0) sp_points(in, i0 + count - 1, a, e);
        coff[n_cont] = e - p0;
        status[0] = all;
    }
}

}  // namespace

extern "C" int gom_scene_polygons_i32(const int32_t* frame_rows, int F, const int64_t* ids, const int32_t* poly_off, int N,
                                      const int32_t* poly_xy, int P, int f0, int f1, int H, int W, const uint8_t* palette, int bgr,
                                      int32_t* coff, int n_cont, int32_t* mcoff, int32_t* boxes, int64_t* woff, int32_t* inst_off,
                                      uint8_t* inst_rgb, int32_t* inst_status, int n_inst, int32_t* status, void* stream) {
    GOM_CHECK_ARG(frame_rows && ids && poly_off && poly_xy && palette && coff && mcoff && boxes && woff && inst_off && inst_rgb &&
                  inst_status && status);
    GOM_CHECK_ARG(F >= 1 && N >= 0 && P >= 0 && f0 >= 0 && f0 < f1 && f1 <= F && n_inst >= 0 && n_cont >= 0 && n_cont <= n_inst);
    GOM_CHECK_ARG(H >= 1 && W >= 1 && (long)H * W <= 2147483647L);
    GOM_CHECK_ARG((reinterpret_cast<uintptr_t>(boxes) & 15) == 0 && (reinterpret_cast<uintptr_t>(poly_xy) & 7) == 0);
    const SpIn in = {frame_rows, ids, poly_off, poly_xy, F, N, P, f0, f1, H, W};
    if (n_inst > 0)
        hipLaunchKernelGGL(scene_boxes_kernel, dim3((unsigned)cdiv((long)n_inst, (long)GOM_SP_BLOCK)), dim3(GOM_SP_BLOCK), 0,
                           (hipStream_t)stream, in, palette, bgr, boxes, inst_rgb, inst_status, n_inst);
    hipLaunchKernelGGL(scene_scan_kernel, dim3(1), dim3(GOM_SP_BLOCK), 0, (hipStream_t)stream, in, (const int32_t*)boxes,
                       (const int32_t*)inst_status, n_inst, coff, n_cont, mcoff, woff, inst_off, status);
    return gom_launch_status();
}
