// Track vote: the bytes of preds/res_<video>.txt, one line per track with its majority transcription, from the rows where
// `result_rows` left them (THE RULE: include/gomatching_hip.h, `gom_track_vote_*`; the text build, the compare and the line
// formatter: track_vote_core.h, shared with the host).
//
//   records : one lane per row: the row's record (track id, text length, 25 zero-padded words of text bytes).
//   vote    : one workgroup per track.  A lane holds the key of its own record in registers (26 words) and walks the track's
//             records j = 0 .. L - 1; every lane reads the same j, so the read is one broadcast load of a record that streams from
//             L2 (a long track does not fit LDS); the compare has no branch, so that a record's 26 words are one batch of loads, and
//             the position of record j + 1 is read while record j is compared.  The winner is the wave, then LDS, maximum of
//             count << 32 | (0xFFFFFFFF - place); tracks longer than the block go tile by tile.
//   scan    : ONE block: exclusive int64 scans of the line lengths in tiles of the block, the status words or-ed -> totals.
//   emit    : one wave64 per track, a lane per byte of the line.
//
// No atomics, no scratch, one writer per output word and byte.  Every position read from `order` / `winner` is checked against
// the log before it is used as an index, every output byte against the line's extent and the cap.
#include "common.h"
#include "track_vote_core.h"
#include "lexicon_rows_core.h"
#include "wave_block.h"

#define TV_WAVES (GOM_TV_BLOCK / 64)

namespace {

__global__ __launch_bounds__(GOM_TV_BLOCK) void track_vote_records_kernel(const int32_t* __restrict__ words, int ld,
                                                                          const unsigned char* __restrict__ keep, int n,
                                                                          const unsigned char* __restrict__ tab, int ntab,
                                                                          int32_t* __restrict__ records) {
    const long r = (long)blockIdx.x * GOM_TV_BLOCK + threadIdx.x;
    if (r >= n) return;
    tv_record(words + r * (long)ld, keep[r] != 0, tab, ntab, records + r * GOM_TV_RECORD_WORDS);
}

// the `_ov` form: a row with ov[r] >= 0 takes its text from the txt display table of the lexicon's W words (an index or an offset
// outside the table gives the empty text); keep_out is what the apply step left of keep
__global__ __launch_bounds__(GOM_TV_BLOCK) void track_vote_records_ov_kernel(
    const int32_t* __restrict__ words, int ld, const unsigned char* __restrict__ keep, int n, const unsigned char* __restrict__ tab,
    int ntab, const int32_t* __restrict__ ov, const unsigned char* __restrict__ keep_out, const unsigned char* __restrict__ disp,
    const int32_t* __restrict__ doff, long dbytes, int W, int32_t* __restrict__ records) {
    const long r = (long)blockIdx.x * GOM_TV_BLOCK + threadIdx.x;
    if (r >= n) return;
    const int i = ov[r];
    long at = 0;
    const int len = i >= 0 ? lr_display(doff, W, dbytes, i, 4 * GOM_TV_TEXT_WORDS, at) : 0;
    tv_record_ov(words + r * (long)ld, keep[r] != 0 && keep_out[r] != 0, tab, ntab, i >= 0 ? disp + at : nullptr, len,
                 records + r * GOM_TV_RECORD_WORDS);
}

__device__ __forceinline__ long clamp_idx(long v, long n) { return v < 0 ? 0 : (v > n ? n : v); }

__global__ __launch_bounds__(GOM_TV_BLOCK) void track_vote_count_kernel(const int32_t* __restrict__ records, long m,
                                                                        const int32_t* __restrict__ order, long nv,
                                                                        const int32_t* __restrict__ seg, int T,
                                                                        int32_t* __restrict__ winner) {
    __shared__ unsigned long long wbest[TV_WAVES];
    __shared__ int wbad[TV_WAVES];
    const int t = blockIdx.x, tid = threadIdx.x;
    if (t >= T) return;                                    // (the whole block leaves)
    const long s_raw = seg[t], e_raw = seg[t + 1];
    const long s = clamp_idx(s_raw, nv);
    long e = clamp_idx(e_raw, nv);
    if (e < s) e = s;
    const long L = e - s;
    int bad = (s != s_raw || e != e_raw || L < 1) ? GOM_TV_BAD_ORDER : 0;
    unsigned long long best = 0;
    for (long base = 0; base < L; base += GOM_TV_BLOCK) {
        const long i = base + tid;
        const long mine = i < L ? (long)order[s + i] : -1;
        const bool have = mine >= 0 && mine < m;
        if (i < L && !have) bad |= GOM_TV_BAD_ORDER;
        const int32_t* rec = records + (have ? mine : 0) * GOM_TV_RECORD_WORDS;
        const GomTvKey key = tv_key_load(rec);
        if (have && key.w[0] == GOM_TV_LEN_BAD) bad |= GOM_TV_BAD_ID;
        if (have && key.w[0] >= 0) {
            uint32_t count = 0;
            long pj = order[s];                            // (L >= 1 here) the same address in every lane: one broadcast load
            for (long j = 0; j < L; ++j) {
                const long pn = order[s + (j + 1 < L ? j + 1 : j)];   // read a step ahead: not behind record j's loads
                if (pj >= 0 && pj < m)                     // (a position outside the log is flagged by the lane that owns j)
                    count += tv_same(key, records + pj * GOM_TV_RECORD_WORDS) ? 1u : 0u;
                pj = pn;
            }
            const unsigned long long k = tv_vote_key(count, (uint32_t)i);
            best = k > best ? k : best;
        }
    }
    wb_block_stage<WbMax>(best, wbest);
    wb_block_stage<WbOr>(bad, wbad);
    __syncthreads();
    if (tid == 0) {
        best = wb_block_fold<GOM_TV_BLOCK, WbMax>(wbest);
        bad = wb_block_fold<GOM_TV_BLOCK, WbOr>(wbad);
        int pos = -1, count = 0, bytes = 0;
        if (best != 0) {
            const long place = (long)(0xFFFFFFFFu - (uint32_t)(best & 0xFFFFFFFFull));
            const long p = place < L ? (long)order[s + place] : -1;
            if (p >= 0 && p < m) {
                pos = (int)p;
                count = (int)(best >> 32);
                bytes = tv_line_len(records + p * GOM_TV_RECORD_WORDS);
            }
        }
        if (pos < 0 && !bad) bad = GOM_TV_BAD_ORDER;         // a track without a voting row: not what the caller's cut gives
        int32_t* w = winner + (long)t * GOM_TV_WINNER_WORDS;
        w[0] = pos;
        w[1] = count;
        w[2] = bytes;
        w[3] = bad;
    }
}

__global__ __launch_bounds__(GOM_TV_BLOCK) void track_vote_scan_kernel(const int32_t* __restrict__ winner, int T,
                                                                       int64_t* __restrict__ line_off,
                                                                       int64_t* __restrict__ totals) {
    __shared__ long long wsum[TV_WAVES];
    __shared__ int wbad[TV_WAVES];
    const int tid = threadIdx.x;
    long long carry = 0;
    int bad = 0;
    for (long base = 0; base < T; base += GOM_TV_BLOCK) {
        const long t = base + tid;
        long long v = 0;
        if (t < T) {
            v = winner[t * GOM_TV_WINNER_WORDS + 2];
            bad |= winner[t * GOM_TV_WINNER_WORDS + 3];
            if (v < 0) v = 0;
        }
        const long long at = wb_block_excl_scan_carry<GOM_TV_BLOCK>(v, wsum, carry);
        if (t < T) line_off[t] = at;
    }
    bad = wb_block_reduce<GOM_TV_BLOCK, WbOr>(bad, wbad);
    if (tid == 0) {
        line_off[T] = carry;
        totals[0] = carry;
        totals[GOM_TV_STATUS] = bad;
    }
}

__global__ __launch_bounds__(GOM_TV_BLOCK) void track_vote_emit_kernel(const int32_t* __restrict__ records, long m,
                                                                       const int32_t* __restrict__ winner,
                                                                       const int64_t* __restrict__ line_off, int T,
                                                                       unsigned char* __restrict__ out, long cap) {
    const int lane = threadIdx.x & 63;
    const long t = (long)blockIdx.x * TV_WAVES + (threadIdx.x >> 6);
    if (t >= T) return;
    const long p = winner[t * GOM_TV_WINNER_WORDS];
    if (p < 0 || p >= m || winner[t * GOM_TV_WINNER_WORDS + 3]) return;
    const int32_t* rec = records + p * GOM_TV_RECORD_WORDS;
    const long begin = line_off[t], end = line_off[t + 1];
    const int n = tv_line_len(rec);
    if (begin < 0 || end - begin != n || end > cap) return;  // not the arrays the scan left: nothing is written
    for (int k = lane; k < n; k += 64) {
        const long at = begin + k;
        if (at >= 0 && at < cap) out[at] = tv_line_byte(rec, k);
    }
}

}  // namespace

extern "C" int gom_track_vote_records_i32(const int32_t* words, int ld, const uint8_t* keep, int n, const uint8_t* txt_tab,
                                          int ntab, int32_t* records, void* stream) {
    GOM_CHECK_ARG(n >= 1 && ld >= GOM_RESULT_ROWS_WORDS && ntab >= 1 && words && keep && txt_tab && records);
    hipLaunchKernelGGL(track_vote_records_kernel, dim3((unsigned)cdiv((long)n, (long)GOM_TV_BLOCK)), dim3(GOM_TV_BLOCK), 0,
                       (hipStream_t)stream, words, ld, keep, n, txt_tab, ntab, records);
    return gom_launch_status();
}

extern "C" int gom_track_vote_records_ov_i32(const int32_t* words, int ld, const uint8_t* keep, int n, const uint8_t* txt_tab,
                                             int ntab, const int32_t* ov, const uint8_t* keep_out, const uint8_t* txt_disp,
                                             const int32_t* txt_doff, long txt_dbytes, int W, int32_t* records, void* stream) {
    GOM_CHECK_ARG(n >= 1 && ld >= GOM_RESULT_ROWS_WORDS && ntab >= 1 && words && keep && txt_tab && records);
    GOM_CHECK_ARG(ov && keep_out && txt_disp && txt_doff && txt_dbytes >= 0 && W >= 0);
    hipLaunchKernelGGL(track_vote_records_ov_kernel, dim3((unsigned)cdiv((long)n, (long)GOM_TV_BLOCK)), dim3(GOM_TV_BLOCK), 0,
                       (hipStream_t)stream, words, ld, keep, n, txt_tab, ntab, ov, keep_out, txt_disp, txt_doff, txt_dbytes, W,
                       records);
    return gom_launch_status();
}

extern "C" int gom_track_vote_count_scan(const int32_t* records, long m, const int32_t* order, long nv, const int32_t* seg, int T,
                                         int32_t* winner, int64_t* line_off, int64_t* totals, void* stream) {
    GOM_CHECK_ARG(m >= 1 && m <= 2147483647L && nv >= 1 && nv <= m && T >= 1 && (long)T <= nv);
    GOM_CHECK_ARG(records && order && seg && winner && line_off && totals);
    hipLaunchKernelGGL(track_vote_count_kernel, dim3((unsigned)T), dim3(GOM_TV_BLOCK), 0, (hipStream_t)stream, records, m, order,
                       nv, seg, T, winner);
    hipLaunchKernelGGL(track_vote_scan_kernel, dim3(1), dim3(GOM_TV_BLOCK), 0, (hipStream_t)stream, (const int32_t*)winner, T,
                       line_off, totals);
    return gom_launch_status();
}

extern "C" int gom_track_vote_emit(const int32_t* records, long m, const int32_t* winner, const int64_t* line_off, int T,
                                   uint8_t* out, long cap, void* stream) {
    GOM_CHECK_ARG(m >= 1 && m <= 2147483647L && T >= 1 && cap >= 0 && records && winner && line_off && out);
    hipLaunchKernelGGL(track_vote_emit_kernel, dim3((unsigned)cdiv((long)T, (long)TV_WAVES)), dim3(GOM_TV_BLOCK), 0,
                       (hipStream_t)stream, records, m, winner, line_off, T, out, cap);
    return gom_launch_status();
}
