// Baseline JPEG decoding of source frames: file bytes go up, u8 [F,H,W,3] stays in HBM.  Contract and THE RULE:
// include/gomatching_hip.h (`gom_jpeg_decode_*`); the walks shared with the host checks: jpeg_decode_core.h, jpeg_decode_chunks.h; the numpy twin:
// gomatching_amd/jpeg.py (decode_host); the per-bit statement: tests/jpeg_decode_statement.py.  Integers only, no atomics, no
// scratch, one writer per output byte, nothing depends on launch order.
//
// Four launches over one workspace in HBM (gom_jpeg_decode_workspace_bytes: coefficients, then planes):
//   jpeg_decode_entropy_kernel  a wavefront per restart segment (a 64-thread workgroup, so that segments spread over the CUs).
//                               The segment's table set (9.3 KiB) is copied to LDS once.  Per block: the 64 lanes zero the
//                               block's LDS row, lane 0 walks the bits (gom_jd_block) and drops the coefficients at their natural
//                               positions, the 64 lanes store the row: 128 contiguous bytes.  The bytes lane 0 reads come from a
//                               2 KiB LDS window of the segment that the wave refills (32-bit loads) between two blocks once
//                               less than 1 KiB of it lies ahead -- a block's code is at most ~0.5 KiB, so the walk stays inside
//                               it; a read outside it goes to HBM.  A walk that stops leaves the remaining blocks zero.
//   jpeg_decode_chunks_kernel   gom_jpeg_decode_entropy_chunks_i16 only, in front of the kernel above (which then skips the
//                               segments this one finished): a 256-thread workgroup per segment, a lane per chunk of its bytes;
//                               cold walk, settling, scans, write walk per span of chunks (jpeg_decode_chunks.h; below).
//   jpeg_decode_status_kernel   a thread per frame: the status of its first segment that is not clean.
//   jpeg_decode_idct_kernel     eight lanes per block: lane c dequantises and transforms column c (strided 16-bit loads), the
//                               block's 8 x 8 intermediate goes through LDS (rows padded to 9 words), lane r transforms row r,
//                               clamps and stores its eight samples as one 8-byte row of the component's plane.
//   jpeg_decode_colour_kernel   a thread per four consecutive pixels of the output (12 bytes = three aligned words): luminance
//                               sample, the two upsampled chrominance samples, the colour matrix, clamp.
#include "common.h"
#include "jpeg_decode_core.h"
#include "jpeg_decode_chunks.h"
#include "wave_block.h"

#define JD_WIN_BYTES 2048
#define JC_THREADS GOM_JC_MAX_LANES
#define JD_IDCT_THREADS 256
#define JD_COLOUR_THREADS 256

namespace {

struct JdLayout {
    GomJdGeom g;
    long coef, planes, total;                                           // byte offsets, 256-aligned, and the size
};

inline long jd_align(long v) { return (v + 255) / 256 * 256; }

// GOM_OK, or why not
inline int jd_layout(int F, int H, int W, int ncomp, int hs, int vs, JdLayout& L) {
    if (F < 0 || H < 1 || W < 1) return GOM_ERR_INVALID_ARG;
    if (W > GOM_JPEG_MAX_WIDTH || H > GOM_JPEG_MAX_HEIGHT || !gom_jd_geometry(H, W, ncomp, hs, vs, L.g)) return GOM_ERR_UNSUPPORTED;
    const long blocks = (long)F * L.g.nblk;
    if (blocks > (1L << 40) / 192) return GOM_ERR_UNSUPPORTED;
    L.coef = 0;
    L.planes = jd_align(blocks * 128);
    L.total = jd_align(L.planes + blocks * 64);
    return GOM_OK;
}

// ---- launch 1: the entropy walk, a wavefront per restart segment ----------------------------------------------------------------
__global__ __launch_bounds__(64) void jpeg_decode_entropy_kernel(const uint8_t* __restrict__ bytes, long nbytes,
                                                                 const int64_t* __restrict__ desc, const int32_t* __restrict__ sets,
                                                                 int nsets, int F, GomJdGeom g, int16_t* __restrict__ coef,
                                                                 int32_t* __restrict__ seg_status,
                                                                 const int32_t* __restrict__ seg_info) {
    __shared__ int32_t s_set[GOM_JD_SET_WORDS];
    __shared__ uint32_t s_win[JD_WIN_BYTES / 4];
    __shared__ int16_t s_blk[64];
    __shared__ long s_pos;
    const int lane = threadIdx.x;
    const long seg = blockIdx.x;
    if (seg_info && seg_info[2 * seg] == 0) return;                     // the chunk walk finished this segment
    const GomJdDesc d = gom_jd_desc(desc + seg * GOM_JD_DESC_WORDS);
    if (d.frame < 0 || d.frame >= F || d.set < 0 || d.set >= nsets) {  // a descriptor that names no frame or no table set
        if (lane == 0) seg_status[seg] = GOM_JD_PAST_END;
        return;
    }
    for (int i = lane; i < GOM_JD_SET_WORDS; i += 64) s_set[i] = sets[d.set * GOM_JD_SET_WORDS + i];
    __syncthreads();
    int16_t* out = coef + d.frame * g.nblk * 64;

    auto begin = [=](GomJdState& s) __attribute__((always_inline)) {
        if (lane == 0) s_pos = s.pos;
        s_blk[lane] = 0;
        __syncthreads();
        const long pos = s_pos;                                         // the same in every lane from here
        if (pos < s.end && s.win_hi < s.end && pos + JD_WIN_BYTES / 2 > s.win_hi) {
            const long lo = pos & ~3L;                                  // `bytes` is 4-byte aligned
            for (int i = lane; i < JD_WIN_BYTES / 4; i += 64) {
                const long at = lo + 4L * i;
                uint32_t w = 0;
                if (at + 4 <= nbytes) {
                    w = *reinterpret_cast<const uint32_t*>(bytes + at);
                } else {
                    for (int b = 0; b < 4; ++b)
                        if (at + b < nbytes) w |= (uint32_t)bytes[at + b] << (8 * b);
                }
                s_win[i] = w;
            }
            s.win = reinterpret_cast<const uint8_t*>(s_win);
            s.win_lo = lo;
            s.win_hi = lo + JD_WIN_BYTES < nbytes ? lo + JD_WIN_BYTES : nbytes;
            __syncthreads();
        }
    };
    auto emit = [=](long bi) __attribute__((always_inline)) {
        __syncthreads();
        out[bi * 64 + lane] = s_blk[lane];                              // (the lane zeroes the same word in the next begin)
    };
    const int status = gom_jd_walk_segment(bytes, nbytes, d, s_set, g, lane == 0, s_blk, begin, emit);
    if (lane == 0) seg_status[seg] = status;
}

// ---- launch 1c: the chunked entropy walk, a workgroup per segment, a lane per chunk (jpeg_decode_chunks.h) -----------------------
// A span is `lanes` chunks; its bytes are staged in LDS, chunk t at word t (chunk_bytes / 4 + 1): the odd stride spreads the
// lanes' byte reads, which advance at about the same pace, over the banks.  A lane's window is its own chunk; what it reads beyond
// it (the end of a symbol, the end of a block it began) comes from HBM.  Exit states travel through LDS; a lane whose entry did not
// change does not walk again, and a wave of such lanes skips the pass.
__device__ __forceinline__ int jc_pack(const GomJcPoint& a) { return a.bit | (a.slot << 3) | (a.k << 6); }

__global__ __launch_bounds__(JC_THREADS) void jpeg_decode_chunks_kernel(const uint8_t* __restrict__ bytes, long nbytes,
                                                                        const int64_t* __restrict__ desc, const int32_t* __restrict__ sets,
                                                                        int nsets, int F, GomJdGeom g, int16_t* __restrict__ coef,
                                                                        int32_t* __restrict__ seg_status, int32_t* __restrict__ seg_info,
                                                                        int chunk_bytes, int lanes) {
    __shared__ int32_t s_set[GOM_JD_SET_WORDS];
    __shared__ uint32_t s_stage[GOM_JC_STAGE_BYTES / 4 + GOM_JC_MAX_LANES];
    __shared__ long s_exit_byte[GOM_JC_MAX_LANES];
    __shared__ int s_exit_w[GOM_JC_MAX_LANES];
    __shared__ uint32_t s_wave[JC_THREADS / 64][4];
    __shared__ int s_bad, s_closed;
    const int tid = threadIdx.x;
    const long seg = blockIdx.x;
    const GomJdDesc d = gom_jd_desc(desc + seg * GOM_JD_DESC_WORDS);
    GomJcSeg sg;
    if (d.frame < 0 || d.frame >= F || d.set < 0 || d.set >= nsets || !gom_jc_segment(sg, bytes, nbytes, d, s_set, g)) {
        if (tid == 0) {                                                 // the serial walk says what is wrong with it
            seg_info[2 * seg] = 1;
            seg_info[2 * seg + 1] = 0;
        }
        return;
    }
    for (int i = tid; i < GOM_JD_SET_WORDS; i += JC_THREADS) s_set[i] = sets[d.set * GOM_JD_SET_WORDS + i];
    if (tid == 0) {
        s_bad = 0;
        s_closed = -1;
    }
    __syncthreads();
    const int row = chunk_bytes / 4 + 1, shift = 31 - __clz(chunk_bytes / 4);
    const long nchunks = gom_jc_chunks(sg, chunk_bytes);
    GomJcPoint truth = {sg.start, 0, 0, 0};
    long carry_blocks = 0;
    uint32_t carry_dc0 = 0, carry_dc1 = 0, carry_dc2 = 0;
    int passes = 0;
    bool bad = false;
    for (long c0 = 0; c0 < nchunks && carry_blocks < sg.blocks && !bad; c0 += lanes) {
        const int act = nchunks - c0 < lanes ? (int)(nchunks - c0) : lanes;
        const long span = sg.base + c0 * chunk_bytes;
        for (int w = tid; w < act << shift; w += JC_THREADS) {          // staging: coalesced 32-bit loads (`bytes` is 4-byte aligned)
            const long at = span + 4L * w;
            if (at >= sg.end) break;
            uint32_t v = 0;
            if (at + 4 <= nbytes) {
                v = *reinterpret_cast<const uint32_t*>(bytes + at);
            } else {
                for (int b = 0; b < 4; ++b)
                    if (at + b < nbytes) v |= (uint32_t)bytes[at + b] << (8 * b);
            }
            s_stage[(w >> shift) * row + (w & ((1 << shift) - 1))] = v;
        }
        __syncthreads();
        const bool active = tid < act;
        const long lo = span + (long)tid * chunk_bytes;
        const long stop = lo + chunk_bytes < sg.end ? lo + chunk_bytes : sg.end;
        const uint8_t* win = reinterpret_cast<const uint8_t*>(s_stage + (active ? tid : 0) * row);
        GomJcPoint entry = truth, exit = truth;
        GomJcTotals tot = {0, 0u, 0u, 0u};
        GomJcWrite w;
        int status = GOM_JD_OK, closed = -1;
        if (active) {                                                   // (a) the cold walk
            if (tid > 0) entry = gom_jc_guess(sg, lo);
            gom_jc_walk<false>(sg, g, win, lo, lo + chunk_bytes, entry, stop, exit, tot, w, status, closed);
            s_exit_byte[tid] = exit.byte;
            s_exit_w[tid] = jc_pack(exit);
        }
        __syncthreads();
        int p = 0;
        for (int pass = 0; pass < GOM_JC_MAX_LANES; ++pass) {           // (b) settling: after pass p the first p + 1 chunks are exact
            GomJcPoint nx = entry;
            if (active && tid > 0) {
                const int ew = s_exit_w[tid - 1];
                nx.byte = s_exit_byte[tid - 1];
                nx.bit = ew & 7;
                nx.slot = (ew >> 3) & 7;
                nx.k = ew >> 6;
            }
            const bool changed = !gom_jc_same(nx, entry);
            if (!__syncthreads_or(changed)) break;                      // (every lane has read before any lane writes)
            ++p;
            if (changed) {
                entry = nx;
                gom_jc_walk<false>(sg, g, win, lo, lo + chunk_bytes, entry, stop, exit, tot, w, status, closed);
                s_exit_byte[tid] = exit.byte;
                s_exit_w[tid] = jc_pack(exit);
            }
            __syncthreads();
        }
        passes = p > passes ? p : passes;
        {                                                               // the next span's true entry
            const int ew = s_exit_w[act - 1];
            truth.byte = s_exit_byte[act - 1];
            truth.bit = ew & 7;
            truth.slot = (ew >> 3) & 7;
            truth.k = ew >> 6;
        }
        // (c), (d) exclusive scans of the blocks begun and the DC sums: within the wave by the shared scan (wave_block.h), across the
        // waves through LDS, the four values behind ONE barrier (which is why this is not four block scans)
        uint32_t inc[4] = {active ? (uint32_t)tot.blocks : 0u, active ? tot.dc0 : 0u, active ? tot.dc1 : 0u, active ? tot.dc2 : 0u};
        const uint32_t own[4] = {inc[0], inc[1], inc[2], inc[3]};
        const int wl = tid & 63, wv = tid >> 6;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            inc[q] = wb_wave_incl_scan<uint32_t>(inc[q]);
            if (wl == 63) s_wave[wv][q] = inc[q];
        }
        __syncthreads();
        uint32_t before[4], all[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            before[q] = inc[q] - own[q];
            all[q] = 0;
#pragma unroll
            for (int v = 0; v < JC_THREADS / 64; ++v) {
                const uint32_t t = s_wave[v][q];
                if (v < wv) before[q] += t;
                all[q] += t;
            }
        }
        if (active) {                                                   // (e) the write walk, from the truth
            w.ordinal = carry_blocks + before[0];
            w.pred0 = carry_dc0 + before[1];
            w.pred1 = carry_dc1 + before[2];
            w.pred2 = carry_dc2 + before[3];
            w.m0 = d.m0;
            w.limit = d.limit;
            w.rst = d.rst;
            w.out = coef + d.frame * g.nblk * 64;
            GomJcPoint e;
            GomJcTotals x;
            gom_jc_walk<true>(sg, g, win, lo, lo + chunk_bytes, entry, stop, e, x, w, status, closed);
            if (status != GOM_JD_OK) s_bad = 1;
            if (closed != -1) s_closed = closed;                        // (one lane ends the last block)
        }
        carry_blocks += all[0];
        carry_dc0 += all[1];
        carry_dc1 += all[2];
        carry_dc2 += all[3];
        __syncthreads();                                                // the stage, the exit words and s_wave are free again
        bad = s_bad != 0;
    }
    if (tid == 0) {
        const int route = (!bad && s_closed == GOM_JD_OK) ? 0 : 1;
        seg_info[2 * seg] = route;
        seg_info[2 * seg + 1] = passes;
        if (route == 0) seg_status[seg] = GOM_JD_OK;
    }
}

// ---- launch 2: segment status words -> frame status words ------------------------------------------------------------------------
__global__ __launch_bounds__(64) void jpeg_decode_status_kernel(const int32_t* __restrict__ seg_status, const int32_t* __restrict__ seg_off,
                                                                int nseg, int F, int32_t* __restrict__ frame_status) {
    const int f = blockIdx.x * 64 + threadIdx.x;
    if (f >= F) return;
    const int a = min(max(seg_off[f], 0), nseg), b = min(max(seg_off[f + 1], a), nseg);
    int st = GOM_JD_OK;
    for (int s = a; s < b && st == GOM_JD_OK; ++s) st = seg_status[s];
    frame_status[f] = st;
}

// ---- launch 3: dequantise, inverse DCT, range limit ---------------------------------------------------------------------------------
// jidctint.c's pass over d[0..7]; out = (x + 2^(SHIFT-1)) >> SHIFT
template <int SHIFT>
__device__ __forceinline__ void jd_idct_pass(const int (&d)[8], int (&o)[8]) {
    int z1 = (d[2] + d[6]) * 4433;
    const int t2 = z1 - d[6] * 15137, t3 = z1 + d[2] * 6270;
    const int t0 = (d[0] + d[4]) * 8192, t1 = (d[0] - d[4]) * 8192;
    const int e0 = t0 + t3, e3 = t0 - t3, e1 = t1 + t2, e2 = t1 - t2;
    int o0 = d[7], o1 = d[5], o2 = d[3], o3 = d[1];
    z1 = o0 + o3;
    int z2 = o1 + o2, z3 = o0 + o2, z4 = o1 + o3;
    const int z5 = (z3 + z4) * 9633;
    o0 *= 2446;
    o1 *= 16819;
    o2 *= 25172;
    o3 *= 12299;
    z1 *= -7373;
    z2 *= -20995;
    z3 = z5 - z3 * 16069;
    z4 = z5 - z4 * 3196;
    o0 += z1 + z3;
    o1 += z2 + z4;
    o2 += z2 + z3;
    o3 += z1 + z4;
    constexpr int R = 1 << (SHIFT - 1);
    o[0] = (e0 + o3 + R) >> SHIFT;
    o[7] = (e0 - o3 + R) >> SHIFT;
    o[1] = (e1 + o2 + R) >> SHIFT;
    o[6] = (e1 - o2 + R) >> SHIFT;
    o[2] = (e2 + o1 + R) >> SHIFT;
    o[5] = (e2 - o1 + R) >> SHIFT;
    o[3] = (e3 + o0 + R) >> SHIFT;
    o[4] = (e3 - o0 + R) >> SHIFT;
}

__global__ __launch_bounds__(JD_IDCT_THREADS) void jpeg_decode_idct_kernel(const int16_t* __restrict__ coef, const int32_t* __restrict__ sets,
                                                                           int nsets, const int32_t* __restrict__ frame_set, long blocks,
                                                                           GomJdGeom g, uint8_t* __restrict__ planes) {
    __shared__ int s_ws[JD_IDCT_THREADS / 8][72];
    const int tid = threadIdx.x, slot = tid >> 3, l = tid & 7;
    const long b = (long)blockIdx.x * (JD_IDCT_THREADS / 8) + slot;
    const bool live = b < blocks;
    const long bc = live ? b : blocks - 1;                              // a spare slot repeats the last block and stores nothing
    const long frame = bc / g.nblk, local = bc % g.nblk;
    const int c = (g.ncomp == 3 && local >= g.first[2]) ? 2 : ((g.ncomp == 3 && local >= g.first[1]) ? 1 : 0);
    const int set = min(max(frame_set[frame], 0), nsets - 1);
    const int32_t* q = sets + (long)set * GOM_JD_SET_WORDS + GOM_JD_SET_QUANT + 64 * c;
    const int16_t* src = coef + bc * 64;
    int d[8], o[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) d[r] = (int)src[r * 8 + l] * q[r * 8 + l];
    jd_idct_pass<11>(d, o);
#pragma unroll
    for (int r = 0; r < 8; ++r) s_ws[slot][r * 9 + l] = o[r];
    __syncthreads();
#pragma unroll
    for (int x = 0; x < 8; ++x) d[x] = s_ws[slot][l * 9 + x];
    jd_idct_pass<18>(d, o);
    uint32_t w0 = 0, w1 = 0;
#pragma unroll
    for (int x = 0; x < 4; ++x) {
        w0 |= (uint32_t)min(max(o[x] + 128, 0), 255) << (8 * x);
        w1 |= (uint32_t)min(max(o[x + 4] + 128, 0), 255) << (8 * x);
    }
    if (live) {
        const long lb = local - g.first[c];
        const long by = lb / g.bw[c], bx = lb % g.bw[c];
        uint8_t* dst = planes + frame * g.nblk * 64 + g.first[c] * 64 + ((by * 8 + l) * g.bw[c] + bx) * 8;
        *reinterpret_cast<uint2*>(dst) = make_uint2(w0, w1);
    }
}

// ---- launch 4: upsampling and colour -----------------------------------------------------------------------------------------------
__global__ __launch_bounds__(JD_COLOUR_THREADS) void jpeg_decode_colour_kernel(const uint8_t* __restrict__ planes, GomJdGeom g, int H, int W,
                                                                               long pixels, int bgr, uint8_t* __restrict__ out) {
    const long t = (long)blockIdx.x * JD_COLOUR_THREADS + threadIdx.x;
    const long p0 = 4 * t;
    if (p0 >= pixels) return;
    const long HW = (long)H * W;
    long f = p0 / HW;
    int rem = (int)(p0 % HW);
    int y = rem / W, x = rem % W;
    const int ch = (H + g.vs - 1) / g.vs, cw = (W + g.hs - 1) / g.hs;   // real chrominance samples
    const int w0 = g.bw[0] * 8, w1 = g.bw[1] * 8;
    uint8_t px[12];
    const int n = pixels - p0 < 4 ? (int)(pixels - p0) : 4;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        int r = 0, gg = 0, b = 0;
        if (j < n) {
            const uint8_t* base = planes + f * g.nblk * 64;
            const int Y = base[(long)y * w0 + x];
            if (g.ncomp == 1) {
                r = gg = b = Y;
            } else {
                const uint8_t* pb = base + g.first[1] * 64;
                const uint8_t* pr = base + g.first[2] * 64;
                int cb, cr;
                if (g.hs == 1) {
                    cb = pb[(long)y * w1 + x];
                    cr = pr[(long)y * w1 + x];
                } else {
                    const int cy = g.vs == 2 ? y >> 1 : y, cx = x >> 1;
                    if (cw <= 2) {
                        cb = pb[(long)cy * w1 + cx];
                        cr = pr[(long)cy * w1 + cx];
                    } else {
                        const int side = (x & 1) ? min(cx + 1, cw - 1) : max(cx - 1, 0);
                        if (g.vs == 1) {
                            const int k = (x & 1) ? 2 : 1;
                            cb = (3 * pb[(long)cy * w1 + cx] + pb[(long)cy * w1 + side] + k) >> 2;
                            cr = (3 * pr[(long)cy * w1 + cx] + pr[(long)cy * w1 + side] + k) >> 2;
                        } else {
                            const int near = (y & 1) ? min(cy + 1, ch - 1) : max(cy - 1, 0);
                            const int k = (x & 1) ? 7 : 8;
                            const long a = (long)cy * w1, e = (long)near * w1;
                            cb = (3 * (3 * pb[a + cx] + pb[e + cx]) + 3 * pb[a + side] + pb[e + side] + k) >> 4;
                            cr = (3 * (3 * pr[a + cx] + pr[e + cx]) + 3 * pr[a + side] + pr[e + side] + k) >> 4;
                        }
                    }
                }
                cb -= 128;
                cr -= 128;
                r = min(max(Y + ((91881 * cr + 32768) >> 16), 0), 255);
                gg = min(max(Y + ((-22554 * cb - 46802 * cr + 32768) >> 16), 0), 255);
                b = min(max(Y + ((116130 * cb + 32768) >> 16), 0), 255);
            }
            if (++x == W) {
                x = 0;
                if (++y == H) {
                    y = 0;
                    ++f;
                }
            }
        }
        px[3 * j] = (uint8_t)(bgr ? b : r);
        px[3 * j + 1] = (uint8_t)gg;
        px[3 * j + 2] = (uint8_t)(bgr ? r : b);
    }
    uint8_t* dst = out + 3 * p0;
    if (n == 4) {
        uint32_t* d32 = reinterpret_cast<uint32_t*>(dst);
#pragma unroll
        for (int k = 0; k < 3; ++k)
            d32[k] = (uint32_t)px[4 * k] | ((uint32_t)px[4 * k + 1] << 8) | ((uint32_t)px[4 * k + 2] << 16) | ((uint32_t)px[4 * k + 3] << 24);
    } else {
        for (int k = 0; k < 3 * n; ++k) dst[k] = px[k];
    }
}

}  // namespace

extern "C" long gom_jpeg_decode_workspace_bytes(int F, int H, int W, int ncomp, int hs, int vs) {
    JdLayout L;
    return jd_layout(F, H, W, ncomp, hs, vs, L) == GOM_OK ? L.total : -1;
}

extern "C" int gom_jpeg_decode_entropy_i16(const uint8_t* bytes, long nbytes, const int64_t* desc, int nseg, const int32_t* seg_off,
                                           const int32_t* sets, int nsets, int F, int H, int W, int ncomp, int hs, int vs,
                                           void* workspace, long workspace_bytes, int32_t* seg_status, int32_t* frame_status,
                                           void* stream) {
    JdLayout L;
    const int rc = jd_layout(F, H, W, ncomp, hs, vs, L);
    if (rc != GOM_OK) return rc;
    GOM_CHECK_ARG(nbytes >= 0 && nseg >= 0 && nsets >= 0);
    if (F == 0) return GOM_OK;
    GOM_CHECK_ARG(bytes && desc && seg_off && sets && nsets >= 1 && workspace && seg_status && frame_status);
    GOM_CHECK_ARG(((uintptr_t)bytes & 3) == 0 && workspace_bytes >= L.total && ((uintptr_t)workspace & 255) == 0);
    unsigned char* ws = (unsigned char*)workspace;
    if (nseg > 0)
        hipLaunchKernelGGL(jpeg_decode_entropy_kernel, dim3((unsigned)nseg), dim3(64), 0, (hipStream_t)stream, bytes, nbytes, desc, sets,
                           nsets, F, L.g, (int16_t*)(ws + L.coef), seg_status, (const int32_t*)nullptr);
    hipLaunchKernelGGL(jpeg_decode_status_kernel, dim3((unsigned)((F + 63) / 64)), dim3(64), 0, (hipStream_t)stream, seg_status, seg_off,
                       nseg, F, frame_status);
    return gom_launch_status();
}

extern "C" int gom_jpeg_decode_entropy_chunks_i16(const uint8_t* bytes, long nbytes, const int64_t* desc, int nseg, const int32_t* seg_off,
                                                  const int32_t* sets, int nsets, int F, int H, int W, int ncomp, int hs, int vs,
                                                  void* workspace, long workspace_bytes, int32_t* seg_status, int32_t* frame_status,
                                                  int chunk_bytes, int32_t* seg_info, void* stream) {
    JdLayout L;
    const int rc = jd_layout(F, H, W, ncomp, hs, vs, L);
    if (rc != GOM_OK) return rc;
    GOM_CHECK_ARG(nbytes >= 0 && nseg >= 0 && nsets >= 0 && GOM_JC_CHUNK_OK(chunk_bytes));
    if (F == 0) return GOM_OK;
    GOM_CHECK_ARG(bytes && desc && seg_off && sets && nsets >= 1 && workspace && seg_status && frame_status && (seg_info || nseg == 0));
    GOM_CHECK_ARG(((uintptr_t)bytes & 3) == 0 && workspace_bytes >= L.total && ((uintptr_t)workspace & 255) == 0);
    unsigned char* ws = (unsigned char*)workspace;
    if (nseg > 0) {
        // the zeros in front: what a clean walk does not store is zero (a marked segment's blocks are all stored again below)
        const hipError_t e = hipMemsetAsync(ws + L.coef, 0, (size_t)F * L.g.nblk * 128, (hipStream_t)stream);
        if (e != hipSuccess) return GOM_ERR_HIP_BASE + (int)e;
        hipLaunchKernelGGL(jpeg_decode_chunks_kernel, dim3((unsigned)nseg), dim3(JC_THREADS), 0, (hipStream_t)stream, bytes, nbytes, desc,
                           sets, nsets, F, L.g, (int16_t*)(ws + L.coef), seg_status, seg_info, chunk_bytes, GOM_JC_LANES(chunk_bytes));
        hipLaunchKernelGGL(jpeg_decode_entropy_kernel, dim3((unsigned)nseg), dim3(64), 0, (hipStream_t)stream, bytes, nbytes, desc, sets,
                           nsets, F, L.g, (int16_t*)(ws + L.coef), seg_status, (const int32_t*)seg_info);
    }
    hipLaunchKernelGGL(jpeg_decode_status_kernel, dim3((unsigned)((F + 63) / 64)), dim3(64), 0, (hipStream_t)stream, seg_status, seg_off,
                       nseg, F, frame_status);
    return gom_launch_status();
}

extern "C" int gom_jpeg_decode_pixels_u8(const int32_t* sets, int nsets, const int32_t* frame_set, int F, int H, int W, int ncomp,
                                         int hs, int vs, int bgr, void* workspace, long workspace_bytes, uint8_t* out, void* stream) {
    JdLayout L;
    const int rc = jd_layout(F, H, W, ncomp, hs, vs, L);
    if (rc != GOM_OK) return rc;
    GOM_CHECK_ARG(bgr == 0 || bgr == 1);
    if (F == 0) return GOM_OK;
    GOM_CHECK_ARG(sets && nsets >= 1 && frame_set && workspace && out);
    GOM_CHECK_ARG(((uintptr_t)out & 3) == 0 && workspace_bytes >= L.total && ((uintptr_t)workspace & 255) == 0);
    unsigned char* ws = (unsigned char*)workspace;
    const long blocks = (long)F * L.g.nblk, pixels = (long)F * H * W;
    const long per = JD_IDCT_THREADS / 8;
    hipLaunchKernelGGL(jpeg_decode_idct_kernel, dim3((unsigned)((blocks + per - 1) / per)), dim3(JD_IDCT_THREADS), 0, (hipStream_t)stream,
                       (const int16_t*)(ws + L.coef), sets, nsets, frame_set, blocks, L.g, ws + L.planes);
    const long threads = (pixels + 3) / 4;
    hipLaunchKernelGGL(jpeg_decode_colour_kernel, dim3((unsigned)((threads + JD_COLOUR_THREADS - 1) / JD_COLOUR_THREADS)),
                       dim3(JD_COLOUR_THREADS), 0, (hipStream_t)stream, (const uint8_t*)(ws + L.planes), L.g, H, W, pixels, bgr, out);
    return gom_launch_status();
}
