// Result parse: the rows of jsons/<video>.json, read from the file's bytes where they lie on the device (THE RULE:
// include/gomatching_hip.h, `gom_result_parse_*`; the per-line functions: result_parse_core.h, shared with the host).
//
//   lines : count -- a thread per GOM_RP_THREAD_BYTES bytes counts the 0x0A bytes (a zero-byte test on 32-bit words), a block per
//           GOM_RP_BLOCK_BYTES; scan -- ONE block scans the block counts in place and tests the file's ends; emit (in the marks
//           call) -- the same tiling, a block scan places every line's start.
//   marks : count -- a lane per line flags object lines, key lines and long lines; scan -- ONE block; emit (in the emit call) --
//           the same tiling: every mark's line, every object's and frame's place among the marks, frame_rows.
//   emit  : ONE block scans the objects' point counts (a function of their line counts) -> poly_off; then a wave64 per object,
//           its lanes striding over the object's lines, each line held against its template and its value stored, and a wave64
//           per frame for the wrapper lines; the status words go to one word per unit and ONE block folds them.
//
// No atomics, no scratch (the four words a thread holds are indexed by unrolled constants: registers), one writer per output
// word.  Reads of the file go through rp_at (index < size), and a vector load only where all of its 16 bytes lie inside the
// file; every store index is compared with its array's length.
#include "common.h"
#include "result_parse_core.h"
#include "wave_block.h"

namespace {

// (the block scans and reductions: wave_block.h; wsum / the slots: GOM_RP_BLOCK / 64 ints)

// a bit 7 per byte of w that equals 0x0A (exact: no carry crosses a byte)
__device__ __forceinline__ uint32_t newline_bits(uint32_t w) {
    const uint32_t x = w ^ 0x0A0A0A0Au;
    const uint32_t t = (x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu;
    return ~(t | x | 0x7F7F7F7Fu);
}

// the 16 bytes of thread `t` as four words (little-endian byte order), zero where the file has ended
__device__ __forceinline__ uint4 load16(const unsigned char* __restrict__ data, long size, long base, bool aligned) {
    uint4 v = make_uint4(0, 0, 0, 0);
    if (base + GOM_RP_THREAD_BYTES <= size && aligned) {
        v = *reinterpret_cast<const uint4*>(data + base);
    } else {
        uint32_t w[4] = {0, 0, 0, 0};
#pragma unroll
        for (int i = 0; i < GOM_RP_THREAD_BYTES; ++i)
            if (base + i < size) w[i >> 2] |= (uint32_t)data[base + i] << (8 * (i & 3));
        v = make_uint4(w[0], w[1], w[2], w[3]);
    }
    return v;
}

__device__ __forceinline__ int count16(const uint4& v) {
    return __popc(newline_bits(v.x)) + __popc(newline_bits(v.y)) + __popc(newline_bits(v.z)) + __popc(newline_bits(v.w));
}

__global__ __launch_bounds__(GOM_RP_BLOCK) void rp_lines_count_kernel(const unsigned char* __restrict__ data, long size,
                                                                      bool aligned, int32_t* __restrict__ blk) {
    __shared__ int wsum[GOM_RP_BLOCK / 64];
    const long base = ((long)blockIdx.x * GOM_RP_BLOCK + threadIdx.x) * GOM_RP_THREAD_BYTES;
    const int c = base < size ? count16(load16(data, size, base, aligned)) : 0;
    const int s = wb_block_reduce<GOM_RP_BLOCK, WbSum>(c, wsum);
    if (threadIdx.x == 0) blk[blockIdx.x] = s;
}

// in-place exclusive scan of a[0 .. n) by the one block, tiles of the block with a carry -> the sum
__device__ __forceinline__ int scan_in_place(int32_t* a, int n, int* wsum) {
    int carry = 0;
    for (long base = 0; base < n; base += GOM_RP_BLOCK) {
        const long i = base + threadIdx.x;
        const int v = i < n ? a[i] : 0;
        const int ex = wb_block_excl_scan_carry<GOM_RP_BLOCK>(v, wsum, carry);
        if (i < n) a[i] = ex;
    }
    return carry;
}

__global__ __launch_bounds__(GOM_RP_BLOCK) void rp_lines_scan_kernel(const unsigned char* __restrict__ data, long size,
                                                                     int32_t* __restrict__ blk, int nblk,
                                                                     int64_t* __restrict__ totals) {
    __shared__ int wsum[GOM_RP_BLOCK / 64];
    const int newlines = scan_in_place(blk, nblk, wsum);
    if (threadIdx.x == 0) {
        const long L = (long)newlines + 1;
        totals[GOM_RP_L] = L;
        totals[GOM_RP_STATUS_LINES] = rp_ends(data, size, L);
    }
}

__global__ __launch_bounds__(GOM_RP_BLOCK) void rp_lines_emit_kernel(const unsigned char* __restrict__ data, long size,
                                                                     bool aligned, const int32_t* __restrict__ blk, long L,
                                                                     int32_t* __restrict__ line_start) {
    __shared__ int wsum[GOM_RP_BLOCK / 64];
    const long base = ((long)blockIdx.x * GOM_RP_BLOCK + threadIdx.x) * GOM_RP_THREAD_BYTES;
    uint4 v = make_uint4(0, 0, 0, 0);
    if (base < size) v = load16(data, size, base, aligned);
    int total;
    long q = (long)blk[blockIdx.x] + wb_block_excl_scan<GOM_RP_BLOCK>(count16(v), wsum, total);     // newlines before this thread's bytes
    const uint32_t bits[4] = {newline_bits(v.x), newline_bits(v.y), newline_bits(v.z), newline_bits(v.w)};
#pragma unroll
    for (int i = 0; i < GOM_RP_THREAD_BYTES; ++i) {
        if (bits[i >> 2] & (0x80u << (8 * (i & 3)))) {
            ++q;                                               // newline number q - 1 opens line q
            if (q >= 1 && q < L) line_start[q] = (int32_t)(base + i + 1);
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        line_start[0] = 0;
        line_start[L] = (int32_t)(size + 1);
    }
}

// flags of line i: bit 0 an object line, bit 1 a key line, bit 2 a long line
__device__ __forceinline__ int line_flags(const GomRpText& t, long i) {
    if (i >= t.L) return 0;
    long a, b;
    rp_line(t, i, a, b);
    const long raw = (long)t.line_start[i + 1] - 1 - t.line_start[i];
    return (rp_is_object_line(t, a, b) ? 1 : 0) | (rp_is_key_line(t, a, b) ? 2 : 0) | (raw > GOM_RP_MAX_LINE ? 4 : 0);
}

__global__ __launch_bounds__(GOM_RP_BLOCK) void rp_marks_count_kernel(GomRpText t, int32_t* __restrict__ mblk,
                                                                      int32_t* __restrict__ sblk, int nmblk) {
    __shared__ int wo[GOM_RP_BLOCK / 64], wk[GOM_RP_BLOCK / 64], ws[GOM_RP_BLOCK / 64];
    const int fl = line_flags(t, (long)blockIdx.x * GOM_RP_BLOCK + threadIdx.x);
    wb_block_stage<WbSum>(fl & 1, wo);
    wb_block_stage<WbSum>((fl >> 1) & 1, wk);
    wb_block_stage<WbOr>(fl & 4, ws);
    __syncthreads();
    if (threadIdx.x == 0) {
        mblk[blockIdx.x] = wb_block_fold<GOM_RP_BLOCK, WbSum>(wo);
        mblk[(long)nmblk + blockIdx.x] = wb_block_fold<GOM_RP_BLOCK, WbSum>(wk);
        sblk[blockIdx.x] = wb_block_fold<GOM_RP_BLOCK, WbOr>(ws) ? GOM_RP_BAD_LINE : 0;
    }
}

__global__ __launch_bounds__(GOM_RP_BLOCK) void rp_marks_scan_kernel(int32_t* __restrict__ mblk,
                                                                     const int32_t* __restrict__ sblk, int nmblk,
                                                                     int64_t* __restrict__ totals) {
    __shared__ int wsum[GOM_RP_BLOCK / 64];
    __shared__ int ws[GOM_RP_BLOCK / 64];
    const int N = scan_in_place(mblk, nmblk, wsum);
    const int F = scan_in_place(mblk + nmblk, nmblk, wsum);
    int st = 0;
    for (long i = threadIdx.x; i < nmblk; i += GOM_RP_BLOCK) st |= sblk[i];
    int all = wb_block_reduce<GOM_RP_BLOCK, WbOr>(st, ws);
    if (threadIdx.x == 0) {
        if (F == 0) all |= GOM_RP_BAD_PLACE;
        totals[GOM_RP_N] = N;
        totals[GOM_RP_F] = F;
        totals[GOM_RP_STATUS_MARKS] = all;
    }
}

__global__ __launch_bounds__(GOM_RP_BLOCK) void rp_marks_emit_kernel(GomRpText t, const int32_t* __restrict__ mblk, int nmblk,
                                                                     int N, int F, int32_t* __restrict__ mark_line,
                                                                     int32_t* __restrict__ obj_mark,
                                                                     int32_t* __restrict__ frame_mark,
                                                                     int32_t* __restrict__ frame_rows) {
    __shared__ int wsum[GOM_RP_BLOCK / 64];
    const long i = (long)blockIdx.x * GOM_RP_BLOCK + threadIdx.x;
    const int fl = line_flags(t, i);
    int total;
    const long oi = (long)mblk[blockIdx.x] + wb_block_excl_scan<GOM_RP_BLOCK>(fl & 1, wsum, total);
    const long ki = (long)mblk[(long)nmblk + blockIdx.x] + wb_block_excl_scan<GOM_RP_BLOCK>((fl >> 1) & 1, wsum, total);
    const long m = oi + ki, M = (long)N + F;
    if ((fl & 1) && oi >= 0 && oi < N && m < M) {
        mark_line[m] = (int32_t)i;
        obj_mark[oi] = (int32_t)m;
    } else if ((fl & 2) && ki >= 0 && ki < F && m < M) {       // (a line is never both)
        mark_line[m] = (int32_t)i;
        frame_mark[ki] = (int32_t)m;
        frame_rows[ki] = (int32_t)(oi < N ? oi : N);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        mark_line[M] = (int32_t)(t.L - 1);
        frame_rows[F] = N;
    }
}

__global__ __launch_bounds__(GOM_RP_BLOCK) void rp_poly_scan_kernel(GomRpMarks m, long L, int32_t* __restrict__ poly_off,
                                                                    int64_t* __restrict__ totals) {
    __shared__ int wsum[GOM_RP_BLOCK / 64];
    int carry = 0;
    for (long base = 0; base < m.N; base += GOM_RP_BLOCK) {
        const long o = base + threadIdx.x;
        int n = 0;
        if (o < m.N) {
            long s, nl;
            bool next_obj;
            rp_object_span(m, L, o, s, nl, next_obj);
            n = rp_points_of(nl);
        }
        const int ex = wb_block_excl_scan_carry<GOM_RP_BLOCK>(n, wsum, carry);
        if (o < m.N) poly_off[o] = ex;
    }
    if (threadIdx.x == 0) {
        poly_off[m.N] = carry;
        totals[GOM_RP_P] = carry;
    }
}

#define RP_WAVES 4

__global__ __launch_bounds__(64 * RP_WAVES) void rp_emit_kernel(GomRpText t, GomRpMarks m, const int32_t* __restrict__ poly_off,
                                                                GomRpRows r, int32_t* __restrict__ unit_status) {
    const int lane = threadIdx.x & 63;
    const long unit = (long)blockIdx.x * RP_WAVES + (threadIdx.x >> 6);
    if (unit >= m.N + m.F) return;                             // (whole waves leave; nothing below needs the block)
    int st = 0;
    if (unit < m.N) {
        long s, nl;
        bool next_obj;
        rp_object_span(m, t.L, unit, s, nl, next_obj);
        const bool closer = lane >= 2 && lane < nl && rp_is_points_closer(t, s + lane);
        const unsigned long long found = __ballot(closer);
        const int j10 = found ? __ffsll((long long)found) - 1 : -1;
        st = rp_object_shape(nl, j10);
        if (st == 0) {
            const long poff = poly_off[unit];
            for (long j = lane; j < nl; j += 64) st |= rp_object_line(t, s, nl, next_obj, j, unit, poff, r);
        }
        st = wb_wave_reduce<WbOr>(st);
    } else if (lane == 0) {
        st = rp_frame(t, m, unit - m.N);
    }
    if (lane == 0) unit_status[unit] = st;
}

__global__ __launch_bounds__(GOM_RP_BLOCK) void rp_fold_kernel(const int32_t* __restrict__ unit_status, long units,
                                                               int64_t* __restrict__ totals) {
    __shared__ int ws[GOM_RP_BLOCK / 64];
    int st = 0;
    for (long i = threadIdx.x; i < units; i += GOM_RP_BLOCK) st |= unit_status[i];
    const int all = wb_block_reduce<GOM_RP_BLOCK, WbOr>(st, ws);
    if (threadIdx.x == 0) {
        totals[GOM_RP_STATUS] = (int64_t)all | totals[GOM_RP_STATUS_LINES] | totals[GOM_RP_STATUS_MARKS];
    }
}

bool rp_file_ok(const void* data, long size, int nblk) {
    return data && size >= 1 && size <= GOM_RP_MAX_SIZE - 1 && nblk == (int)((size + GOM_RP_BLOCK_BYTES - 1) / GOM_RP_BLOCK_BYTES);
}

bool rp_lines_ok(long size, long L, int nmblk) {
    return L >= 2 && L <= size + 1 && nmblk == (int)((L + GOM_RP_BLOCK - 1) / GOM_RP_BLOCK);
}

}  // namespace

extern "C" int gom_result_parse_lines(const uint8_t* data, long size, int32_t* blk, int nblk, int64_t* totals, void* stream) {
    GOM_CHECK_ARG(rp_file_ok(data, size, nblk) && blk && totals);
    const bool aligned = (reinterpret_cast<uintptr_t>(data) & 15) == 0;
    hipLaunchKernelGGL(rp_lines_count_kernel, dim3((unsigned)nblk), dim3(GOM_RP_BLOCK), 0, (hipStream_t)stream, data, size,
                       aligned, blk);
    hipLaunchKernelGGL(rp_lines_scan_kernel, dim3(1), dim3(GOM_RP_BLOCK), 0, (hipStream_t)stream, data, size, blk, nblk, totals);
    return gom_launch_status();
}

extern "C" int gom_result_parse_marks(const uint8_t* data, long size, const int32_t* blk, int nblk, long L, int32_t* line_start,
                                      int32_t* mblk, int32_t* sblk, int nmblk, int64_t* totals, void* stream) {
    GOM_CHECK_ARG(rp_file_ok(data, size, nblk) && blk && rp_lines_ok(size, L, nmblk) && line_start && mblk && sblk && totals);
    const bool aligned = (reinterpret_cast<uintptr_t>(data) & 15) == 0;
    const GomRpText t = {data, size, line_start, L};
    hipLaunchKernelGGL(rp_lines_emit_kernel, dim3((unsigned)nblk), dim3(GOM_RP_BLOCK), 0, (hipStream_t)stream, data, size, aligned,
                       blk, L, line_start);
    hipLaunchKernelGGL(rp_marks_count_kernel, dim3((unsigned)nmblk), dim3(GOM_RP_BLOCK), 0, (hipStream_t)stream, t, mblk, sblk,
                       nmblk);
    hipLaunchKernelGGL(rp_marks_scan_kernel, dim3(1), dim3(GOM_RP_BLOCK), 0, (hipStream_t)stream, mblk, (const int32_t*)sblk,
                       nmblk, totals);
    return gom_launch_status();
}

extern "C" int gom_result_parse_emit(const uint8_t* data, long size, const int32_t* line_start, long L, const int32_t* mblk,
                                     int nmblk, int F, int N, int32_t* mark_line, int32_t* obj_mark, int32_t* frame_mark,
                                     int32_t* frame_rows, int32_t* poly_off, int64_t* ids, int32_t* pts, uint8_t* has_seg,
                                     int64_t* t_off, int32_t* t_len, int32_t* poly_xy, long cap_p, int32_t* unit_status,
                                     int64_t* totals, void* stream) {
    GOM_CHECK_ARG(data && size >= 1 && size <= GOM_RP_MAX_SIZE - 1 && line_start && mblk && rp_lines_ok(size, L, nmblk));
    GOM_CHECK_ARG(F >= 1 && N >= 0 && (long)F + N <= L && cap_p >= 0);
    GOM_CHECK_ARG(mark_line && obj_mark && frame_mark && frame_rows && poly_off && ids && pts && has_seg && t_off && t_len &&
                  poly_xy && unit_status && totals);
    const GomRpText t = {data, size, line_start, L};
    const GomRpMarks m = {mark_line, obj_mark, frame_mark, frame_rows, N, F};
    const GomRpRows r = {ids, pts, has_seg, t_off, t_len, N, poly_xy, cap_p};
    const long units = (long)N + F;
    hipLaunchKernelGGL(rp_marks_emit_kernel, dim3((unsigned)nmblk), dim3(GOM_RP_BLOCK), 0, (hipStream_t)stream, t, mblk, nmblk, N, F,
                       mark_line, obj_mark, frame_mark, frame_rows);
    hipLaunchKernelGGL(rp_poly_scan_kernel, dim3(1), dim3(GOM_RP_BLOCK), 0, (hipStream_t)stream, m, L, poly_off, totals);
    hipLaunchKernelGGL(rp_emit_kernel, dim3((unsigned)cdiv(units, (long)RP_WAVES)), dim3(64 * RP_WAVES), 0, (hipStream_t)stream, t, m,
                       (const int32_t*)poly_off, r, unit_status);
    hipLaunchKernelGGL(rp_fold_kernel, dim3(1), dim3(GOM_RP_BLOCK), 0, (hipStream_t)stream, (const int32_t*)unit_status, units,
                       totals);
    return gom_launch_status();
}
