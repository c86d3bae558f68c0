// Which rows of the encoder memory a decoder layer's deformable cross attention reads: mark, then compact.
//
// The decoder's value projection (deepsolo.py `decoder`) used to run for every encoder token and all six layers in one launch
// (M = frames x tokens, N = 1536).  A layer's sampling reads, from its 256 columns, the rows around frames x queries x points
// reference points: 8-9 % of the rows on the bench clip.  These two launches name them, and the row-list form of the K = 256 GEMM
// (gemm_k256.hip) projects only those:
//
//   mark     one wave per query, the owner mapping of msda_fused_lanes_kernel (lane (head m, k) owns samples 2k and 2k + 1 of level
//            k >> 1): flags[frame * S + row] = 1 for the four corners of both samples, by msda_corners() -- the function that kernel
//            takes its load addresses from (msda_corners.h), so a weight-0 load (a clamped corner, a sample outside the map) is marked
//            like any other.  Plain byte stores of the same value from whoever gets there: no atomics, no order.
//   compact  flags -> the ascending list of marked rows and their count.  One launch, no atomics, no cross-workgroup hand-off:
//            workgroup j owns bytes [4096 j, 4096 (j + 1)) and counts the marks in front of its tile itself (the bytes are in L2:
//            the whole array is 0.3 MB at the bench shape, and the longest count, the last workgroup's, reads it once).  The list is
//            the same for any grid order.  The last workgroup writes the count.
//
// The flags are NOT cleared here (other workgroups are still counting them): the GEMM's row-list form clears the flag of every row
// it projects, which leaves the array zero for the next layer's marks.
#include "common.h"
#include "msda_corners.h"
#include "wave_block.h"

namespace {

constexpr int HEADS = 8, LEVELS = 4, POINTS = 4, LP = LEVELS * POINTS;
constexpr int CBLOCK = 256, CTILE = CBLOCK * 16;             // compaction: 16 flag bytes per thread

__global__ __launch_bounds__(256) void dec_value_mark_kernel(const float* __restrict__ raw, int ld_raw, const float* __restrict__ ref,
                                                             const int64_t* __restrict__ shapes, const int64_t* __restrict__ lsi,
                                                             int B, int Lq, int S, unsigned char* __restrict__ flags) {
    const long q_global = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (q_global >= (long)B * Lq) return;
    const int lane = threadIdx.x & 63;
    const int m = lane >> 3, k = lane & 7;
    const int b = (int)(q_global / Lq);
    const int l = k >> 1;
    const f32x4 off = *reinterpret_cast<const f32x4*>(raw + (size_t)q_global * ld_raw + m * (LP * 2) + 4 * k);
    const float rx = ref[q_global * 2], ry = ref[q_global * 2 + 1];
    const int H = (int)shapes[2 * l], W = (int)shapes[2 * l + 1];
    const float Hf = (float)H, Wf = (float)W;
    const float rW = 1.f / Wf, rH = 1.f / Hf;
    const unsigned lvl = (unsigned)lsi[l];
    unsigned char* fb = flags + (size_t)b * S;
    auto mark = [&](int y, int x) {
        const unsigned row = lvl + (unsigned)(y * W + x);
        if (row < (unsigned)S) fb[row] = 1;                  // (a pyramid that does not fit its S marks nothing out of bounds)
    };
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const MsdaCorners c = msda_corners(off[2 * t], off[2 * t + 1], rx, ry, H, W, Hf, Wf, rW, rH);
        mark(c.yc0, c.xc0);
        mark(c.yc0, c.xc1);
        mark(c.yc1, c.xc0);
        mark(c.yc1, c.xc1);
    }
}

// The lean form: the same bytes, fewer stores.  On the bench clip 10.2 M corner stores land on ~26 000 distinct rows, so a corner's
// flag is read first and stored only where it is still 0 (a flag only goes 0 -> 1 inside the launch, so a stale 0 costs a store of
// the same 1 and nothing else); and the two x-neighbours of a sample's corner row, adjacent bytes, go as one 16-bit access (alignment
// 1: the address is any byte).  The four reads of a lane's two samples are issued in front of its stores.
__global__ __launch_bounds__(256) void dec_value_mark_lean_kernel(const float* __restrict__ raw, int ld_raw, const float* __restrict__ ref,
                                                                  const int64_t* __restrict__ shapes, const int64_t* __restrict__ lsi,
                                                                  int B, int Lq, int S, unsigned char* flags) {
    const long q_global = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (q_global >= (long)B * Lq) return;
    const int lane = threadIdx.x & 63;
    const int m = lane >> 3, k = lane & 7;
    const int b = (int)(q_global / Lq);
    const int l = k >> 1;
    const f32x4 off = *reinterpret_cast<const f32x4*>(raw + (size_t)q_global * ld_raw + m * (LP * 2) + 4 * k);
    const float rx = ref[q_global * 2], ry = ref[q_global * 2 + 1];
    const int H = (int)shapes[2 * l], W = (int)shapes[2 * l + 1];
    const float Hf = (float)H, Wf = (float)W;
    const float rW = 1.f / Wf, rH = 1.f / Hf;
    const unsigned lvl = (unsigned)lsi[l];
    unsigned char* fb = flags + (size_t)b * S;
    // corner row i: bytes row[i] and, where the sample has a second column on it, row[i] + 1.  form 0: nothing (the second corner
    // row is the first, or the byte is beyond S), 1: one byte, 2: the pair
    unsigned row[4];
    int form[4];
    unsigned have[4];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const MsdaCorners c = msda_corners(off[2 * t], off[2 * t + 1], rx, ry, H, W, Hf, Wf, rW, rH);
        const bool two = c.xc1 != c.xc0;                     // xc1 is xc0 or xc0 + 1
#pragma unroll
        for (int y = 0; y < 2; ++y) {
            const unsigned r = lvl + (unsigned)((y ? c.yc1 : c.yc0) * W + c.xc0);
            const bool skip = y == 1 && c.yc1 == c.yc0;
            row[2 * t + y] = r;
            form[2 * t + y] = skip || r >= (unsigned)S ? 0 : (two && r + 1 < (unsigned)S ? 2 : 1);
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        have[i] = 0x0101u;
        if (form[i] == 2) {
            unsigned short v;
            __builtin_memcpy(&v, fb + row[i], 2);
            have[i] = v;
        } else if (form[i] == 1) {
            have[i] = 0x0100u | fb[row[i]];
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        if (have[i] == 0x0101u) continue;
        if (form[i] == 2) {
            const unsigned short v = 0x0101u;
            __builtin_memcpy(fb + row[i], &v, 2);
        } else {
            fb[row[i]] = 1;
        }
    }
}

__device__ __forceinline__ int marks_of(const uint4 v) {     // a flag byte is 0 or 1
    return __popc(v.x & 0x01010101u) + __popc(v.y & 0x01010101u) + __popc(v.z & 0x01010101u) + __popc(v.w & 0x01010101u);
}

// flags: cdiv(n, 4096) * 4096 bytes, zero behind n
__global__ __launch_bounds__(CBLOCK) void dec_value_compact_kernel(const unsigned char* __restrict__ flags, int n, int* __restrict__ rows,
                                                                  int* __restrict__ count) {
    __shared__ int wsum[CBLOCK / 64];
    const int tid = threadIdx.x, j = blockIdx.x;
    const uint4* f4 = reinterpret_cast<const uint4*>(flags);
    int before = 0;
#pragma unroll 8
    for (int i = tid; i < j * CBLOCK; i += CBLOCK) before += marks_of(f4[i]);
    int base;
    wb_block_excl_scan<CBLOCK, int>(before, wsum, base);     // base = the marks in front of this tile, in every thread
    const uint4 mine = f4[j * CBLOCK + tid];
    int total;
    int pos = base + wb_block_excl_scan<CBLOCK, int>(marks_of(mine), wsum, total);
    const unsigned w[4] = {mine.x, mine.y, mine.z, mine.w};
    const int first = j * CTILE + tid * 16;
#pragma unroll
    for (int i = 0; i < 16; ++i)
        if (((w[i >> 2] >> (8 * (i & 3))) & 1u) && first + i < n) rows[pos++] = first + i;
    if (j == (int)gridDim.x - 1 && tid == 0) *count = base + total;
}

}  // namespace

static int g_mark_lean = 1;

extern "C" int gom_dec_value_set_lean_mark(int on) {
    g_mark_lean = on ? 1 : 0;
    return GOM_OK;
}

extern "C" long gom_dec_value_flag_bytes(int n) { return n < 0 ? -1 : (long)cdiv(n, CTILE) * CTILE; }

extern "C" int gom_dec_value_mark(const float* raw, int ld_raw, const float* ref, const int64_t* spatial_shapes,
                                  const int64_t* level_start_index, int batch, int num_query, int rows_per_frame,
                                  unsigned char* flags, void* stream) {
    GOM_CHECK_ARG(raw && ref && spatial_shapes && level_start_index && flags);
    GOM_CHECK_ARG(batch > 0 && num_query > 0 && rows_per_frame > 0 && ld_raw >= HEADS * LP * 3 && (ld_raw % 4) == 0);
    GOM_CHECK_ARG(((uintptr_t)raw % 16) == 0 && (long)batch * rows_per_frame < (1L << 31));
    const long nq = (long)batch * num_query;
    if (g_mark_lean) {
        hipLaunchKernelGGL(dec_value_mark_lean_kernel, dim3((unsigned)cdiv(nq, 4)), dim3(256), 0, (hipStream_t)stream, raw, ld_raw, ref,
                           spatial_shapes, level_start_index, batch, num_query, rows_per_frame, flags);
        return gom_launch_status();
    }
    hipLaunchKernelGGL(dec_value_mark_kernel,dim3((unsigned)cdiv(nq, 4)), dim3(256), 0, (hipStream_t)stream, raw, ld_raw, ref,
                       spatial_shapes, level_start_index, batch, num_query, rows_per_frame, flags);
    return gom_launch_status();
}

extern "C" int gom_dec_value_compact(const unsigned char* flags, int n, int* rows, int* count, void* stream) {
    GOM_CHECK_ARG(flags && rows && count && n > 0 && ((uintptr_t)flags % 16) == 0);
    hipLaunchKernelGGL(dec_value_compact_kernel, dim3((unsigned)cdiv(n, CTILE)), dim3(CBLOCK), 0, (hipStream_t)stream, flags, n, rows,
                       count);
    return gom_launch_status();
}
