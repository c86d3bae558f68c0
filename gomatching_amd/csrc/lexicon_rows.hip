// Lexicon correction of rows on the device: the glue between the rows `result_rows` left, the match kernel of csrc/lexicon.hip and
// the `_ov` forms of the result text and the track vote (THE RULE: include/gomatching_hip.h, `gom_lexicon_rows_*`; the query, the
// acceptance and the display lookup: lexicon_rows_core.h, shared with the host).
//
//   queries : the offsets are a result, so count / scan / emit as result_text.hip does it.
//             count : a lane per row: the query's length through the norm table (0 for a row that is not kept or has an id outside
//                     the table, GOM_LR_LEN_LONG above the limit).
//             scan  : ONE block of GOM_LR_BLOCK threads walks the rows in tiles of the block: exclusive int32 scan of the lengths
//                     with a carry between tiles -> q_off; the status word and the first row above the limit -> q_status.
//             emit  : a lane per row writes the row's code points at its offset: one writer per word.
//   apply   : ONE block strides over the rows: ov and keep_out per row, the four counts through a block reduction -> totals.
//
// No atomics, no scratch, plain stores.  Every id is checked before it indexes the norm table; every query store against the row's
// counted extent and the cap; a match index against the lexicon's size.
#include "common.h"
#include "lexicon_rows_core.h"
#include "wave_block.h"

namespace {

__global__ __launch_bounds__(GOM_LR_BLOCK) void lexicon_rows_count_kernel(const int32_t* __restrict__ words, int ld,
                                                                          const unsigned char* __restrict__ keep, int n,
                                                                          const uint32_t* __restrict__ tab, int ntab,
                                                                          int32_t* __restrict__ q_len) {
    const long r = (long)blockIdx.x * GOM_LR_BLOCK + threadIdx.x;
    if (r >= n) return;
    q_len[r] = lr_query_len(words + r * (long)ld, keep[r] != 0, tab, ntab);
}

__global__ __launch_bounds__(GOM_LR_BLOCK) void lexicon_rows_scan_kernel(const int32_t* __restrict__ q_len, int n,
                                                                         int32_t* __restrict__ q_off,
                                                                         int32_t* __restrict__ q_status) {
    __shared__ int wsum[GOM_LR_BLOCK / 64];
    __shared__ int wlong[GOM_LR_BLOCK / 64];
    const int t = threadIdx.x;
    int carry = 0, first_long = 0x7FFFFFFF;                   // (n <= GOM_LR_MAX_ROWS: the sum of the lengths fits an int)
    for (long base = 0; base < n; base += GOM_LR_BLOCK) {
        const long r = base + t;
        int len = 0;
        if (r < n) {
            len = q_len[r];
            if (len < 0 || len > GOM_LEXICON_MAX_LEN) {     // above the limit (or not a length at all): flagged, matched as empty
                if ((int)r < first_long) first_long = (int)r;
                len = 0;
            }
        }
        const int at = wb_block_excl_scan_carry<GOM_LR_BLOCK>(len, wsum, carry);
        if (r < n) q_off[r] = at;
    }
    const int m = wb_block_reduce<GOM_LR_BLOCK, WbMin>(first_long, wlong);
    if (t == 0) {
        q_off[n] = carry;
        q_status[0] = m != 0x7FFFFFFF ? GOM_LR_TOO_LONG : 0;
        q_status[1] = m != 0x7FFFFFFF ? m : -1;
    }
}

__global__ __launch_bounds__(GOM_LR_BLOCK) void lexicon_rows_emit_kernel(const int32_t* __restrict__ words, int ld,
                                                                         const unsigned char* __restrict__ keep, int n,
                                                                         const uint32_t* __restrict__ tab, int ntab,
                                                                         const int32_t* __restrict__ q_len,
                                                                         const int32_t* __restrict__ q_off,
                                                                         uint32_t* __restrict__ q_chars, long q_cap) {
    const long r = (long)blockIdx.x * GOM_LR_BLOCK + threadIdx.x;
    if (r >= n) return;
    const int len = q_len[r];
    const long at = q_off[r], next = q_off[r + 1];
    // a row whose extent is not the one the scan left for its length, or that leaves the buffer, is not written
    if (len <= 0 || len > GOM_LEXICON_MAX_LEN || at < 0 || next - at != len || next > q_cap) return;
    lr_query(words + r * (long)ld, keep[r] != 0, tab, ntab, q_chars + at, len);
}

__global__ __launch_bounds__(GOM_LR_BLOCK) void lexicon_rows_apply_kernel(const unsigned char* __restrict__ keep,
                                                                          const int32_t* __restrict__ q_len,
                                                                          const int32_t* __restrict__ q_status,
                                                                          const int32_t* __restrict__ best_index,
                                                                          const int32_t* __restrict__ best_dist, int n, int W,
                                                                          int max_dist, int drop, int32_t* __restrict__ ov,
                                                                          unsigned char* __restrict__ keep_out,
                                                                          int64_t* __restrict__ totals) {
    __shared__ int sums[3][GOM_LR_BLOCK / 64];
    const int t = threadIdx.x;
    int kept = 0, accepted = 0, dropped = 0;                  // (n < 2^25 rows: an int holds a thread's and the block's counts)
    for (long r = t; r < n; r += GOM_LR_BLOCK) {
        const bool k = keep[r] != 0;
        const int i = lr_accept(k, q_len[r], best_index[r], best_dist[r], W, max_dist);
        const bool out = k && (!drop || i >= 0);
        ov[r] = i;
        keep_out[r] = out ? 1 : 0;
        kept += k ? 1 : 0;
        accepted += i >= 0 ? 1 : 0;
        dropped += k && !out ? 1 : 0;
    }
    wb_block_stage<WbSum>(kept, sums[0]);
    wb_block_stage<WbSum>(accepted, sums[1]);
    wb_block_stage<WbSum>(dropped, sums[2]);
    __syncthreads();
    if (t == 0) {
        totals[GOM_LR_KEPT] = wb_block_fold<GOM_LR_BLOCK, WbSum>(sums[0]);
        totals[GOM_LR_ACCEPTED] = wb_block_fold<GOM_LR_BLOCK, WbSum>(sums[1]);
        totals[GOM_LR_DROPPED] = wb_block_fold<GOM_LR_BLOCK, WbSum>(sums[2]);
        totals[GOM_LR_STATUS] = q_status[0];
        totals[GOM_LR_FIRST_LONG] = q_status[1];
    }
}

}  // namespace

extern "C" int gom_lexicon_rows_queries_u32(const int32_t* words, int ld, const uint8_t* keep, int n, const uint32_t* norm_tab,
                                            int ntab, int32_t* q_len, int32_t* q_off, int32_t* q_status, uint32_t* q_chars,
                                            long q_cap, void* stream) {
    GOM_CHECK_ARG(n >= 0 && n <= GOM_LR_MAX_ROWS && ld >= GOM_RESULT_ROWS_WORDS && ntab >= 1 && q_cap >= 0);
    if (n == 0) return GOM_OK;
    GOM_CHECK_ARG(words && keep && norm_tab && q_len && q_off && q_status && q_chars);
    GOM_CHECK_ARG(q_cap >= (long)n * GOM_LEXICON_MAX_LEN);
    const unsigned blocks = (unsigned)cdiv((long)n, (long)GOM_LR_BLOCK);
    hipLaunchKernelGGL(lexicon_rows_count_kernel, dim3(blocks), dim3(GOM_LR_BLOCK), 0, (hipStream_t)stream, words, ld, keep, n,
                       norm_tab, ntab, q_len);
    hipLaunchKernelGGL(lexicon_rows_scan_kernel, dim3(1), dim3(GOM_LR_BLOCK), 0, (hipStream_t)stream, (const int32_t*)q_len, n,
                       q_off, q_status);
    hipLaunchKernelGGL(lexicon_rows_emit_kernel, dim3(blocks), dim3(GOM_LR_BLOCK), 0, (hipStream_t)stream, words, ld, keep, n,
                       norm_tab, ntab, (const int32_t*)q_len, (const int32_t*)q_off, q_chars, q_cap);
    return gom_launch_status();
}

extern "C" int gom_lexicon_rows_apply_i32(const uint8_t* keep, const int32_t* q_len, const int32_t* q_status,
                                          const int32_t* best_index, const int32_t* best_dist, int n, int W, int max_dist,
                                          int drop, int32_t* ov, uint8_t* keep_out, int64_t* totals, void* stream) {
    GOM_CHECK_ARG(n >= 0 && n <= GOM_LR_MAX_ROWS && W >= 0 && max_dist >= 0 && (drop == 0 || drop == 1));
    if (n == 0) return GOM_OK;
    GOM_CHECK_ARG(keep && q_len && q_status && best_index && best_dist && ov && keep_out && totals);
    hipLaunchKernelGGL(lexicon_rows_apply_kernel, dim3(1), dim3(GOM_LR_BLOCK), 0, (hipStream_t)stream, keep, q_len, q_status,
                       best_index, best_dist, n, W, max_dist, drop, ov, keep_out, totals);
    return gom_launch_status();
}
