// Result text: the bytes of jsons/<video>.json and preds/res_<video>.xml, formatted from the rows where `result_rows` left them
// (THE RULE: include/gomatching_hip.h, `gom_result_text_*`; the formatting functions: result_text_core.h, shared with the host).
//
//   count : one wave64 per row, a lane per piece (63 JSON pieces, 8 XML pieces: a polygon point, a rectangle point, the id, the
//           transcription ...), a wave reduction -> the row's JSON and XML length; 0 for a dropped row, -1 for a row with an
//           emitted character id outside the table.
//   scan  : ONE block of GOM_RT_SCAN_BLOCK threads walks the rows in chunks of the block (exclusive int64 scans of both lengths
//           and of the kept flags, a carry between chunks), then the frames the same way (a frame's length = wrappers + its rows +
//           the separators between them) -> frame_off and the totals.  Latency-sized: 30 000 rows are 118 chunks.
//   emit  : one wave64 per row: the lanes format their pieces into the wave's LDS stage at the offsets a wave scan gives them,
//           shifted so that stage and destination share their 16-byte phase; then the wave stores the row: bytes up to the first
//           16-byte boundary, uint4 words, bytes after the last.  One wave64 per frame writes that frame's wrappers, a lane each.
//
// No atomics, no scratch (no local arrays), one writer per output byte.  Stores: a staged byte is checked against the length the
// count pass left for the row (and the stage size), a global byte or word against the row's extent clipped to the cap.
#include "common.h"
#include "result_text_core.h"
#include "lexicon_rows_core.h"
#include "wave_block.h"

#define RT_WAVES 4

namespace {

// the operands of the `_ov` entries (THE RULE: include/gomatching_hip.h, `gom_lexicon_rows_*`): the per-row override, the keep
// flags the apply step left, and the display tables of the two streams over the lexicon's W words
struct RtOv {
    const int32_t* ov;
    const unsigned char* keep_out;
    const unsigned char* json_disp;
    const int32_t* json_doff;
    long json_dbytes;
    const unsigned char* xml_disp;
    const int32_t* xml_doff;
    long xml_dbytes;
    int W;
};

// OV = false: the row of the tables alone (the override pointers are null constants: the branch on them folds away)
template <bool OV>
__device__ __forceinline__ GomRtRow rt_row(const int32_t* words, int ld, const int64_t* pts, const unsigned char* jt,
                                           const unsigned char* xt, int ntab, long r, const RtOv& v) {
    GomRtRow row;
    row.words = words + r * (long)ld;
    row.pts = pts + r * 8;
    row.json_tab = jt;
    row.xml_tab = xt;
    row.ntab = ntab;
    row.json_ov = row.xml_ov = nullptr;
    row.json_ov_len = row.xml_ov_len = 0;
    if (OV) {
        const int i = v.ov[r];
        if (i >= 0) {                                      // (an index outside [0, W) reads nothing: the empty form)
            long at;
            row.json_ov_len = lr_display(v.json_doff, v.W, v.json_dbytes, i, 25 * (GOM_RT_ENTRY_BYTES - 1), at);
            row.json_ov = v.json_disp + at;
            row.xml_ov_len = lr_display(v.xml_doff, v.W, v.xml_dbytes, i, 25 * (GOM_RT_ENTRY_BYTES - 1), at);
            row.xml_ov = v.xml_disp + at;
        }
    }
    return row;
}

template <bool OV>
__device__ __forceinline__ bool rt_keeps(const unsigned char* keep, const RtOv& v, long r) {
    return keep[r] && (!OV || v.keep_out[r]);
}

__device__ __forceinline__ int clamp_row(int v, int n) { return v < 0 ? 0 : (v > n ? n : v); }

template <bool OV>
__device__ __forceinline__ void result_text_count_body(const int32_t* __restrict__ words, int ld, const int64_t* __restrict__ pts,
                                                       const unsigned char* __restrict__ keep, int n,
                                                       const unsigned char* __restrict__ jt, const unsigned char* __restrict__ xt,
                                                       int ntab, int32_t* __restrict__ row_len, const RtOv& v) {
    const int lane = threadIdx.x & 63;
    const long r = (long)blockIdx.x * RT_WAVES + (threadIdx.x >> 6);
    if (r >= n) return;                                   // (whole waves leave; nothing below needs the block)
    int lj = 0, lx = 0;
    if (rt_keeps<OV>(keep, v, r)) {
        const GomRtRow row = rt_row<OV>(words, ld, pts, jt, xt, ntab, r, v);
        GomRtOut o = {nullptr, 0, 0};
        if (lane < GOM_RT_JSON_PIECES) rt_json_piece(o, row, lane, false);
        const int pj = (int)o.pos;
        o.pos = 0;
        if (lane < GOM_RT_XML_PIECES) rt_xml_piece(o, row, lane);
        const int px = (int)o.pos;
        const int bad = wb_wave_reduce<WbSum>(lane < 25 && rt_char_bad(row, lane) ? 1 : 0);
        lj = wb_wave_reduce<WbSum>(pj);
        lx = wb_wave_reduce<WbSum>(px);
        if (bad) lj = lx = -1;
    }
    if (lane == 0) {
        row_len[r] = lj;
        row_len[(long)n + r] = lx;
    }
}

__global__ __launch_bounds__(64 * RT_WAVES) void result_text_count_kernel(const int32_t* __restrict__ words, int ld,
                                                                          const int64_t* __restrict__ pts,
                                                                          const unsigned char* __restrict__ keep, int n,
                                                                          const unsigned char* __restrict__ jt,
                                                                          const unsigned char* __restrict__ xt, int ntab,
                                                                          int32_t* __restrict__ row_len) {
    result_text_count_body<false>(words, ld, pts, keep, n, jt, xt, ntab, row_len, RtOv{});
}

__global__ __launch_bounds__(64 * RT_WAVES) void result_text_count_ov_kernel(const int32_t* __restrict__ words, int ld,
                                                                             const int64_t* __restrict__ pts,
                                                                             const unsigned char* __restrict__ keep, int n,
                                                                             const unsigned char* __restrict__ jt,
                                                                             const unsigned char* __restrict__ xt, int ntab,
                                                                             int32_t* __restrict__ row_len, RtOv v) {
    result_text_count_body<true>(words, ld, pts, keep, n, jt, xt, ntab, row_len, v);
}

// (the scans of one chunk of the block: wb_block_excl_scan_carry of wave_block.h -> this thread's exclusive prefix, carry included)
__global__ __launch_bounds__(GOM_RT_SCAN_BLOCK) void result_text_scan_kernel(const int32_t* __restrict__ row_len, int n,
                                                                             const int32_t* __restrict__ frame_rows, int F,
                                                                             long first_frame, int64_t* __restrict__ row_off,
                                                                             int32_t* __restrict__ row_kept,
                                                                             int64_t* __restrict__ frame_off,
                                                                             int64_t* __restrict__ totals) {
    __shared__ long long wj[GOM_RT_SCAN_BLOCK / 64], wx[GOM_RT_SCAN_BLOCK / 64];
    __shared__ int wk[GOM_RT_SCAN_BLOCK / 64];
    __shared__ int bad_any[GOM_RT_SCAN_BLOCK / 64];
    const int t = threadIdx.x;
    // ---- rows
    long long cj = 0, cx = 0;
    int ck = 0, bad = 0;
    for (long base = 0; base < n; base += GOM_RT_SCAN_BLOCK) {
        const long r = base + t;
        int lj = 0, lx = 0;
        if (r < n) {
            lj = row_len[r];
            lx = row_len[(long)n + r];
            if (lj < 0 || lx < 0) {
                bad = 1;
                lj = lx = 0;
            }
        }
        const long long oj = wb_block_excl_scan_carry<GOM_RT_SCAN_BLOCK, long long>(lj, wj, cj);
        const long long ox = wb_block_excl_scan_carry<GOM_RT_SCAN_BLOCK, long long>(lx, wx, cx);
        const int ok = wb_block_excl_scan_carry<GOM_RT_SCAN_BLOCK, int>(lj > 0 ? 1 : 0, wk, ck);
        if (r < n) {
            row_off[r] = oj;
            row_off[(long)n + 1 + r] = ox;
            row_kept[r] = ok;
        }
    }
    if (t == 0) {
        row_off[n] = cj;
        row_off[(long)n + 1 + n] = cx;
        row_kept[n] = ck;
    }
    wb_block_stage<WbOr>(bad, bad_any);
    __syncthreads();                                      // the block's own stores to row_off / row_kept are visible to it from here
    // ---- frames
    long long fj = 0, fx = 0;
    for (long base = 0; base < F; base += GOM_RT_SCAN_BLOCK) {
        const long f = base + t;
        long long lj = 0, lx = 0;
        if (f < F) {
            const int s = clamp_row(frame_rows[f], n), e = clamp_row(frame_rows[f + 1], n);
            const int kept = e > s ? row_kept[e] - row_kept[s] : 0;
            const long long bj = e > s ? row_off[e] - row_off[s] : 0;
            const long long bx = e > s ? row_off[(long)n + 1 + e] - row_off[(long)n + 1 + s] : 0;
            lj = rt_json_frame_len(first_frame + f, kept, bj);
            lx = rt_xml_frame_len(first_frame + f, kept, bx);
        }
        const long long oj = wb_block_excl_scan_carry<GOM_RT_SCAN_BLOCK, long long>(lj, wj, fj);
        const long long ox = wb_block_excl_scan_carry<GOM_RT_SCAN_BLOCK, long long>(lx, wx, fx);
        if (f < F) {
            frame_off[f] = oj;
            frame_off[(long)F + 1 + f] = ox;
        }
    }
    if (t == 0) {
        frame_off[F] = fj;
        frame_off[(long)F + 1 + F] = fx;
        const int any = wb_block_fold<GOM_RT_SCAN_BLOCK, WbOr>(bad_any);
        totals[0] = fj;
        totals[1] = fx;
        totals[GOM_RT_STATUS] = any ? GOM_RT_BAD_ID : 0;
        totals[3] = 0;
    }
}

// the wave stores stage[shift .. shift + len) to out[dst .. dst + len): [dst, dst + len) lies inside the buffer (the caller clipped
// it), stage is 16-byte aligned and shift = the destination ADDRESS mod 16, so the uint4 words in the middle are aligned on both sides
__device__ __forceinline__ void wave_store(unsigned char* __restrict__ out, long dst, long len, const unsigned char* stage,
                                           int shift, int lane) {
    const long end = dst + len;
    long a0 = dst + ((16 - shift) & 15);
    if (a0 > end) a0 = end;
    long a1 = a0 + ((end - a0) & ~15L);
    for (long i = dst + lane; i < a0; i += 64) out[i] = stage[i - dst + shift];
    for (long i = a0 + 16L * lane; i < a1; i += 16L * 64)
        *reinterpret_cast<uint4*>(out + i) = *reinterpret_cast<const uint4*>(stage + (i - dst + shift));
    for (long i = a1 + lane; i < end; i += 64) out[i] = stage[i - dst + shift];
}

template <bool OV>
__device__ __forceinline__ void result_text_emit_body(
    const int32_t* __restrict__ words, int ld, const int64_t* __restrict__ pts, const unsigned char* __restrict__ keep, int n,
    const int32_t* __restrict__ frame_rows, int F, long first_frame, const unsigned char* __restrict__ jt, const unsigned char* __restrict__ xt, int ntab,
    const int32_t* __restrict__ row_len, const int64_t* __restrict__ row_off, const int32_t* __restrict__ row_kept,
    const int64_t* __restrict__ frame_off, unsigned char* __restrict__ json, long json_cap, unsigned char* __restrict__ xml,
    long xml_cap, const RtOv& v) {
    __shared__ __attribute__((aligned(16))) unsigned char stage_all[RT_WAVES][GOM_RT_STAGE_BYTES];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    unsigned char* stage = stage_all[w];
    const long unit = (long)blockIdx.x * RT_WAVES + w;     // rows first, then frames; a tail wave has nothing to do but the barriers
    const bool is_row = unit < n, is_frame = !is_row && unit < (long)n + F;

    // ---- a frame's wrappers: head and tail of both streams, a lane each, straight to memory (a few dozen bytes)
    if (is_frame && lane < 4) {
        const long f = unit - n;
        const int s = clamp_row(frame_rows[f], n), e = clamp_row(frame_rows[f + 1], n);
        const int kept = e > s ? row_kept[e] - row_kept[s] : 0;
        const bool is_xml = lane >= 2, tail = lane & 1;
        const long begin = frame_off[(is_xml ? (long)F + 1 : 0) + f], next = frame_off[(is_xml ? (long)F + 1 : 0) + f + 1];
        const long cap = is_xml ? xml_cap : json_cap;
        GomRtOut len = {nullptr, 0, 0};
        if (is_xml) {
            if (tail) rt_xml_frame_tail(len, kept);
            else rt_xml_frame_head(len, first_frame + f, kept);
        } else {
            if (tail) rt_json_frame_tail(len, kept);
            else rt_json_frame_head(len, first_frame + f, kept);
        }
        const long at = tail ? next - len.pos : begin;
        if (begin >= 0 && at >= begin && at + len.pos <= next && next <= cap) {
            GomRtOut o = {(is_xml ? xml : json) + at, len.pos, 0};
            if (is_xml) {
                if (tail) rt_xml_frame_tail(o, kept);
                else rt_xml_frame_head(o, first_frame + f, kept);
            } else {
                if (tail) rt_json_frame_tail(o, kept);
                else rt_json_frame_head(o, first_frame + f, kept);
            }
        }
    }

    // ---- a row: where it goes
    long r = is_row ? unit : 0;
    int lj = 0, lx = 0;
    long dj = 0, dx = 0;
    bool sep = false;
    GomRtRow row = rt_row<false>(words, ld, pts, jt, xt, ntab, r, v);
    if (is_row) {
        if (OV) row = rt_row<true>(words, ld, pts, jt, xt, ntab, r, v);
        lj = row_len[r];
        lx = row_len[(long)n + r];
        if (lj <= 0 || lx <= 0 || !rt_keeps<OV>(keep, v, r)) lj = lx = 0;    // dropped, or flagged for an id outside the table
    }
    if (lj > 0) {
        int lo = 0, hi = F - 1;                            // the frame that owns row r: the last f with frame_rows[f] <= r
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (clamp_row(frame_rows[mid], n) <= r) lo = mid;
            else hi = mid - 1;
        }
        const int f = lo, s = clamp_row(frame_rows[f], n), e = clamp_row(frame_rows[f + 1], n);
        const int before = row_kept[r] - row_kept[s];
        sep = before > 0;
        GomRtOut hj = {nullptr, 0, 0}, hx = {nullptr, 0, 0};
        rt_json_frame_head(hj, first_frame + f, 1);
        rt_xml_frame_head(hx, first_frame + f, 1);
        // the `before` kept rows in front have before - 1 separators between them; this row's own separator is its first two bytes
        dj = frame_off[f] + hj.pos + (row_off[r] - row_off[s]) + (sep ? 2L * (before - 1) : 0L);
        dx = frame_off[(long)F + 1 + f] + hx.pos + (row_off[(long)n + 1 + r] - row_off[(long)n + 1 + s]);
        if (sep) lj += 2;
        // a row outside its frame's extent or outside the buffer is not written (arrays that are not the count pass's)
        const long j0 = frame_off[f], j1 = frame_off[f + 1], x0 = frame_off[(long)F + 1 + f], x1 = frame_off[(long)F + 1 + f + 1];
        if (r < s || r >= e || j0 < 0 || dj < j0 || dj + lj > j1 || j1 > json_cap) lj = 0;
        if (r < s || r >= e || x0 < 0 || dx < x0 || dx + lx > x1 || x1 > xml_cap) lx = 0;
    }

    // ---- JSON: a lane per piece into the stage, then the wave stores the row
    {
        const int shift = (int)((reinterpret_cast<uintptr_t>(json) + (uintptr_t)dj) & 15);
        if (shift + lj > GOM_RT_STAGE_BYTES) lj = 0;
        GomRtOut cnt = {nullptr, 0, 0};
        if (lj > 0 && lane < GOM_RT_JSON_PIECES) rt_json_piece(cnt, row, lane, sep);
        const long mine = cnt.pos;
        const long at = wb_wave_incl_scan<long>(mine) - mine;
        if (lj > 0 && lane < GOM_RT_JSON_PIECES) {
            GomRtOut o = {stage, (long)shift + lj, shift + at};
            rt_json_piece(o, row, lane, sep);
        }
        __syncthreads();
        if (lj > 0) wave_store(json, dj, lj, stage, shift, lane);
        __syncthreads();
    }
    // ---- XML
    {
        const int shift = (int)((reinterpret_cast<uintptr_t>(xml) + (uintptr_t)dx) & 15);
        if (shift + lx > GOM_RT_STAGE_BYTES) lx = 0;
        GomRtOut cnt = {nullptr, 0, 0};
        if (lx > 0 && lane < GOM_RT_XML_PIECES) rt_xml_piece(cnt, row, lane);
        const long mine = cnt.pos;
        const long at = wb_wave_incl_scan<long>(mine) - mine;
        if (lx > 0 && lane < GOM_RT_XML_PIECES) {
            GomRtOut o = {stage, (long)shift + lx, shift + at};
            rt_xml_piece(o, row, lane);
        }
        __syncthreads();
        if (lx > 0) wave_store(xml, dx, lx, stage, shift, lane);
    }
}

__global__ __launch_bounds__(64 * RT_WAVES) void result_text_emit_kernel(
    const int32_t* __restrict__ words, int ld, const int64_t* __restrict__ pts, const unsigned char* __restrict__ keep, int n,
    const int32_t* __restrict__ frame_rows, int F, long first_frame, const unsigned char* __restrict__ jt, const unsigned char* __restrict__ xt, int ntab,
    const int32_t* __restrict__ row_len, const int64_t* __restrict__ row_off, const int32_t* __restrict__ row_kept,
    const int64_t* __restrict__ frame_off, unsigned char* __restrict__ json, long json_cap, unsigned char* __restrict__ xml,
    long xml_cap) {
    result_text_emit_body<false>(words, ld, pts, keep, n, frame_rows, F, first_frame, jt, xt, ntab, row_len, row_off, row_kept,
                                 frame_off, json, json_cap, xml, xml_cap, RtOv{});
}

__global__ __launch_bounds__(64 * RT_WAVES) void result_text_emit_ov_kernel(
    const int32_t* __restrict__ words, int ld, const int64_t* __restrict__ pts, const unsigned char* __restrict__ keep, int n,
    const int32_t* __restrict__ frame_rows, int F, long first_frame, const unsigned char* __restrict__ jt, const unsigned char* __restrict__ xt, int ntab,
    const int32_t* __restrict__ row_len, const int64_t* __restrict__ row_off, const int32_t* __restrict__ row_kept,
    const int64_t* __restrict__ frame_off, unsigned char* __restrict__ json, long json_cap, unsigned char* __restrict__ xml,
    long xml_cap, RtOv v) {
    result_text_emit_body<true>(words, ld, pts, keep, n, frame_rows, F, first_frame, jt, xt, ntab, row_len, row_off, row_kept,
                                frame_off, json, json_cap, xml, xml_cap, v);
}

bool rt_args_ok(const void* words, int ld, const void* pts, const void* keep, int n, const void* frame_rows, int F,
                long first_frame, const void* jt, const void* xt, int ntab) {
    return n >= 1 && F >= 1 && ld >= GOM_RESULT_ROWS_WORDS && ntab >= 1 && first_frame >= 0 &&
           first_frame + F <= 2147483646L && words && pts && keep && frame_rows && jt && xt;
}

bool rt_ov_ok(const RtOv& v) {
    return v.ov && v.keep_out && v.json_disp && v.json_doff && v.xml_disp && v.xml_doff && v.W >= 0 && v.json_dbytes >= 0 &&
           v.xml_dbytes >= 0;
}

}  // namespace

extern "C" int gom_result_text_count_scan(const int32_t* words, int ld, const int64_t* pts, const uint8_t* keep, int n,
                                          const int32_t* frame_rows, int F, long first_frame, const uint8_t* json_tab,
                                          const uint8_t* xml_tab, int ntab, int32_t* row_len, int64_t* row_off,
                                          int32_t* row_kept, int64_t* frame_off, int64_t* totals, void* stream) {
    GOM_CHECK_ARG(rt_args_ok(words, ld, pts, keep, n, frame_rows, F, first_frame, json_tab, xml_tab, ntab));
    GOM_CHECK_ARG(row_len && row_off && row_kept && frame_off && totals);
    hipLaunchKernelGGL(result_text_count_kernel, dim3((unsigned)cdiv((long)n, (long)RT_WAVES)), dim3(64 * RT_WAVES), 0,
                       (hipStream_t)stream, words, ld, pts, keep, n, json_tab, xml_tab, ntab, row_len);
    hipLaunchKernelGGL(result_text_scan_kernel, dim3(1), dim3(GOM_RT_SCAN_BLOCK), 0, (hipStream_t)stream,
                       (const int32_t*)row_len, n, frame_rows, F, first_frame, row_off, row_kept, frame_off, totals);
    return gom_launch_status();
}

extern "C" int gom_result_text_emit(const int32_t* words, int ld, const int64_t* pts, const uint8_t* keep, int n,
                                    const int32_t* frame_rows, int F, long first_frame, const uint8_t* json_tab,
                                    const uint8_t* xml_tab, int ntab, const int32_t* row_len, const int64_t* row_off,
                                    const int32_t* row_kept, const int64_t* frame_off, uint8_t* json, long json_cap,
                                    uint8_t* xml, long xml_cap, void* stream) {
    GOM_CHECK_ARG(rt_args_ok(words, ld, pts, keep, n, frame_rows, F, first_frame, json_tab, xml_tab, ntab));
    GOM_CHECK_ARG(row_len && row_off && row_kept && frame_off && json && xml && json_cap >= 0 && xml_cap >= 0);
    hipLaunchKernelGGL(result_text_emit_kernel, dim3((unsigned)cdiv((long)n + F, (long)RT_WAVES)), dim3(64 * RT_WAVES), 0,
                       (hipStream_t)stream, words, ld, pts, keep, n, frame_rows, F, first_frame, json_tab, xml_tab, ntab, row_len,
                       row_off, row_kept, frame_off, json, json_cap, xml, xml_cap);
    return gom_launch_status();
}

// ---- the `_ov` forms (lexicon correction of rows): the same launches with the override operands
extern "C" int gom_result_text_count_scan_ov(const int32_t* words, int ld, const int64_t* pts, const uint8_t* keep, int n,
                                             const int32_t* frame_rows, int F, long first_frame, const uint8_t* json_tab,
                                             const uint8_t* xml_tab, int ntab, const int32_t* ov, const uint8_t* keep_out,
                                             const uint8_t* json_disp, const int32_t* json_doff, long json_dbytes,
                                             const uint8_t* xml_disp, const int32_t* xml_doff, long xml_dbytes, int W,
                                             int32_t* row_len, int64_t* row_off, int32_t* row_kept, int64_t* frame_off,
                                             int64_t* totals, void* stream) {
    const RtOv v = {ov, keep_out, json_disp, json_doff, json_dbytes, xml_disp, xml_doff, xml_dbytes, W};
    GOM_CHECK_ARG(rt_args_ok(words, ld, pts, keep, n, frame_rows, F, first_frame, json_tab, xml_tab, ntab) && rt_ov_ok(v));
    GOM_CHECK_ARG(row_len && row_off && row_kept && frame_off && totals);
    hipLaunchKernelGGL(result_text_count_ov_kernel, dim3((unsigned)cdiv((long)n, (long)RT_WAVES)), dim3(64 * RT_WAVES), 0,
                       (hipStream_t)stream, words, ld, pts, keep, n, json_tab, xml_tab, ntab, row_len, v);
    hipLaunchKernelGGL(result_text_scan_kernel, dim3(1), dim3(GOM_RT_SCAN_BLOCK), 0, (hipStream_t)stream,
                       (const int32_t*)row_len, n, frame_rows, F, first_frame, row_off, row_kept, frame_off, totals);
    return gom_launch_status();
}

extern "C" int gom_result_text_emit_ov(const int32_t* words, int ld, const int64_t* pts, const uint8_t* keep, int n,
                                       const int32_t* frame_rows, int F, long first_frame, const uint8_t* json_tab,
                                       const uint8_t* xml_tab, int ntab, const int32_t* ov, const uint8_t* keep_out,
                                       const uint8_t* json_disp, const int32_t* json_doff, long json_dbytes,
                                       const uint8_t* xml_disp, const int32_t* xml_doff, long xml_dbytes, int W,
                                       const int32_t* row_len, const int64_t* row_off, const int32_t* row_kept,
                                       const int64_t* frame_off, uint8_t* json, long json_cap, uint8_t* xml, long xml_cap,
                                       void* stream) {
    const RtOv v = {ov, keep_out, json_disp, json_doff, json_dbytes, xml_disp, xml_doff, xml_dbytes, W};
    GOM_CHECK_ARG(rt_args_ok(words, ld, pts, keep, n, frame_rows, F, first_frame, json_tab, xml_tab, ntab) && rt_ov_ok(v));
    GOM_CHECK_ARG(row_len && row_off && row_kept && frame_off && json && xml && json_cap >= 0 && xml_cap >= 0);
    hipLaunchKernelGGL(result_text_emit_ov_kernel, dim3((unsigned)cdiv((long)n + F, (long)RT_WAVES)), dim3(64 * RT_WAVES), 0,
                       (hipStream_t)stream, words, ld, pts, keep, n, frame_rows, F, first_frame, json_tab, xml_tab, ntab, row_len,
                       row_off, row_kept, frame_off, json, json_cap, xml, xml_cap, v);
    return gom_launch_status();
}
