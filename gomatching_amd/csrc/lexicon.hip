// Lexicon correction: the nearest word of a vocabulary by edit distance, for every distinct transcription of a
// result set in one launch -- what the reference's find_match_word does in a Python loop over the lexicon per detection.
// Contract and THE RULE: include/gomatching_hip.h; the statement the kernel is held to word for word: tests/lexicon_statement.py.
//
// lexicon_match_kernel: one 256-thread workgroup per query.  The query's code points go to LDS once, and with them the table
// of equality masks peq[c] = { j : q[j] == c } for the code points c < 256 (thread c OWNS entry c: no atomics).  Lanes then
// stride over the words of the query's segment in ascending index; per pair the Levenshtein distance comes from Hyyro's
// bit-vector form of the recurrence with the query as the pattern: the column of vertical differences lives in two machine
// words (vp, vn), one step per word character, ~16 integer operations whatever the query's length -- 32-bit words for queries
// of up to 32 code points (a workgroup-uniform choice), 64-bit above; the 64-point limit exists so that this fits.  The
// mask of a code point >= 256 is built by comparing it against the query's code points (m compares, LDS broadcast reads).
// A lane skips a word whose length differs from the query's by at least its own running best: the distance is never below
// that difference and the lane's later indices never win a tie, so the result is the true (lowest index, minimum) -- nothing
// depends on an acceptance bound.  (dist << 32 | index) is minimised with shuffles within the wave and through four LDS
// words across the waves; thread 0 writes.  Offsets, segment numbers and lengths are device data: every index is clamped.
#include "common.h"
#include "wave_block.h"

#define LX_THREADS 256
#define LX_TABLE 256                                                   // == LX_THREADS: thread c builds entry c
#define LX_MAX GOM_LEXICON_MAX_LEN

namespace {

__device__ __forceinline__ int lx_clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// Levenshtein distance of the query (m >= 1 code points qc[], masks peq[]) and a word w[0..n): Hyyro 2003.  Bits above m - 1
// only ever receive carries; they never reach the bits below.
template <typename T>
__device__ __forceinline__ int lx_distance(const unsigned long long* peq, const unsigned* qc, int m,
                                           const unsigned* __restrict__ w, int n) {
    T vp = ~(T)0, vn = 0;
    const T top = (T)1 << (m - 1);
    int d = m;
    for (int k = 0; k < n; ++k) {
        const unsigned c = w[k];
        T eq = 0;
        if (c < LX_TABLE) {
            eq = (T)peq[c];
        } else {
            for (int j = 0; j < m; ++j) eq |= (T)(qc[j] == c) << j;
        }
        const T d0 = (((eq & vp) + vp) ^ vp) | eq | vn;
        T hp = vn | ~(d0 | vp);
        T hn = d0 & vp;
        d += (hp & top) != 0;
        d -= (hn & top) != 0;
        hp = (hp << 1) | (T)1;
        hn <<= 1;
        vp = hn | ~(d0 | hp);
        vn = hp & d0;
    }
    return d;
}

__global__ __launch_bounds__(LX_THREADS) void lexicon_match_kernel(
    const unsigned* __restrict__ q_chars, int q_nchars, const int* __restrict__ q_off, const int* __restrict__ q_seg,
    const unsigned* __restrict__ w_chars, int w_nchars, const int* __restrict__ w_off, int W, const int* __restrict__ seg_off,
    int n_seg, int* __restrict__ best_index, int* __restrict__ best_dist) {
    __shared__ unsigned long long peq[LX_TABLE];
    __shared__ unsigned qc[LX_MAX];
    __shared__ unsigned long long red[LX_THREADS / 64];
    const int s = blockIdx.x, tid = threadIdx.x;

    const int qa = lx_clamp(q_off[s], 0, q_nchars), qb = lx_clamp(q_off[s + 1], qa, q_nchars);
    const int m = min(qb - qa, LX_MAX);
    if (tid < m) qc[tid] = q_chars[qa + tid];
    __syncthreads();
    {
        unsigned long long e = 0ull;
        for (int j = 0; j < m; ++j) e |= (unsigned long long)(qc[j] == (unsigned)tid) << j;
        peq[tid] = e;
    }
    __syncthreads();

    const int g = lx_clamp(q_seg[s], 0, n_seg - 1);
    const int s0 = lx_clamp(seg_off[g], 0, W), s1 = lx_clamp(seg_off[g + 1], s0, W);
    int bd = GOM_LEXICON_NO_MATCH_DIST, bi = -1;
    for (long long i = (long long)s0 + tid; i < s1; i += LX_THREADS) {
        const int wa = lx_clamp(w_off[i], 0, w_nchars), wb = lx_clamp(w_off[i + 1], wa, w_nchars);
        const int n = min(wb - wa, LX_MAX);
        if (abs(n - m) >= bd) continue;                               // exact: d >= |n - m|, and only a smaller d replaces bd
        int d;
        if (m == 0) d = n;
        else if (m <= 32) d = lx_distance<unsigned>(peq, qc, m, w_chars + wa, n);
        else d = lx_distance<unsigned long long>(peq, qc, m, w_chars + wa, n);
        if (d < bd) {
            bd = d;
            bi = (int)(i - s0);
        }
    }

    // the smallest (dist, index): nothing found is (100, 0xffffffff), above every real key
    const unsigned long long mine = ((unsigned long long)(unsigned)bd << 32) | (unsigned)bi;
    const unsigned long long key = wb_block_reduce<LX_THREADS, WbMin>(mine, red);
    if (tid == 0) {
        best_index[s] = (int)(unsigned)key;
        best_dist[s] = (int)(key >> 32);
    }
}

}  // namespace

extern "C" int gom_lexicon_match_u32(const uint32_t* q_chars, long q_nchars, const int32_t* q_off, const int32_t* q_seg, int S,
                                     const uint32_t* w_chars, long w_nchars, const int32_t* w_off, int W, const int32_t* seg_off,
                                     int n_seg, int max_len, int32_t* best_index, int32_t* best_dist, void* stream) {
    GOM_CHECK_ARG(S >= 0 && W >= 0 && n_seg >= 0 && q_nchars >= 0 && w_nchars >= 0);
    GOM_CHECK_ARG(q_nchars <= 2147483647L && w_nchars <= 2147483647L);
    GOM_CHECK_ARG(max_len >= 0 && max_len <= GOM_LEXICON_MAX_LEN);
    if (q_nchars > 0) GOM_CHECK_ARG(q_chars);
    if (w_nchars > 0) GOM_CHECK_ARG(w_chars);
    if (W > 0) GOM_CHECK_ARG(w_off);
    if (n_seg > 0) GOM_CHECK_ARG(seg_off);
    if (S > 0) GOM_CHECK_ARG(n_seg > 0 && q_off && q_seg && best_index && best_dist);
    if (S == 0) return GOM_OK;
    hipLaunchKernelGGL(lexicon_match_kernel, dim3((unsigned)S), dim3(LX_THREADS), 0, (hipStream_t)stream,
                       (const unsigned*)q_chars, (int)q_nchars, q_off, q_seg, (const unsigned*)w_chars, (int)w_nchars, w_off, W,
                       seg_off, n_seg, (int*)best_index, (int*)best_dist);
    return gom_launch_status();
}
