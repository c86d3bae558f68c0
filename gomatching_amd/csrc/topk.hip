// Top-k proposal selection over the S encoder tokens (deformable_transformer.py:188-190):
//   topk_proposals = torch.topk(enc_outputs_class[..., 0], nq, dim=1)[1]
// Two LDS bitonic-sort stages: per-chunk top-k, then a merge of the chunk winners.  Keys are
// (order-preserving float bits, ~index) packed in 64 bits, so the result is sorted by value
// descending with ties resolved towards the LOWER token index (deterministic; the reference's tie
// order is unspecified).  The order is that of the bit patterns: +0.0 ranks above -0.0 (torch.topk holds
// them equal), NaN logits are not ordered.  Invalid-proposal tokens get the constant logit the reference
// produces for a zeroed memory row (see DESIGN.md "proposal masking").  A last chunk with fewer than k
// tokens hands its zero padding keys to the merge as candidates; k <= S real keys, each above zero, are
// always among the candidates, so a padding key is never among the k winners.
//
// The lean forms (gom_topk_set_lean, on by default) give the same winners in the same order -- the keys are distinct, so the order
// is the keys' and not the method's -- with less sorting:
//   * a wave owns the 128 keys its 64 threads touch at strides <= 64, so those stages need no workgroup barrier (the lanes of a
//     wave share one instruction stream and their LDS operations retire in order);
//   * chunk stage, k <= 128: the wave-local sort leaves 32 runs of 128 keys in alternating directions; five rounds keep, of two
//     neighbouring runs, the upper 128 (max(A[i], B[i]) of a descending and an ascending run is the bitonic upper half) and merge
//     them at strides 64 .. 1: 7 workgroup barriers instead of 78;
//   * merge stage: the network is the next power of two >= the candidates (1024 .. 8192), not always 8192.
#include "common.h"

namespace {

constexpr int CHUNK = 4096;
constexpr int MERGE_MAX = 8192;

__device__ __forceinline__ unsigned long long make_key(float v, unsigned idx) {
    unsigned u = __float_as_uint(v);
    u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);        // ascending-orderable
    return ((unsigned long long)u << 32) | (unsigned long long)(0xFFFFFFFFu - idx);
}

template <int N>
__device__ void bitonic_sort_desc(unsigned long long* keys) {   // N power of two, blockDim = 1024
    for (int size = 2; size <= N; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            __syncthreads();
            for (int t = threadIdx.x; t < N / 2; t += blockDim.x) {
                const int lo = 2 * t - (t & (stride - 1));
                const int hi = lo + stride;
                const bool desc = ((lo & size) == 0);
                const unsigned long long a = keys[lo], b = keys[hi];
                if ((a < b) == desc) { keys[lo] = b; keys[hi] = a; }
            }
        }
    }
    __syncthreads();
}

// ---- lean forms --------------------------------------------------------------------------------------------------------------
constexpr int THREADS = 1024;                                // every launch of this file

__device__ __forceinline__ void wave_lds_sync() {            // orders this wave's LDS writes before its later LDS reads
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ void cmpx(unsigned long long* keys, int lo, int hi, bool desc) {
    const unsigned long long a = keys[lo], b = keys[hi];
    if ((a < b) == desc) { keys[lo] = b; keys[hi] = a; }
}

// the stages of merge size `size` at strides first .. 1 (first <= 64) on the 128-key segments the waves own: thread t of pass j
// touches keys [128 (t / 64), 128 (t / 64) + 128) only.  No workgroup barrier inside; the caller's barriers stand around it.
template <int N>
__device__ __forceinline__ void bitonic_wave_stages(unsigned long long* keys, int size, int first) {
    constexpr int PASSES = (N / 2 + THREADS - 1) / THREADS;
    if (N / 2 < THREADS && (int)threadIdx.x >= N / 2) return;   // (N / 2 and THREADS are multiples of 64: uniform per wave)
    for (int stride = first; stride > 0; stride >>= 1) {
        // a wave's segments of the passes are independent: all reads of a stage are issued in front of its writes
        unsigned long long a[PASSES], b[PASSES];
        int lo[PASSES];
#pragma unroll
        for (int j = 0; j < PASSES; ++j) {
            const int t = threadIdx.x + j * THREADS;
            lo[j] = 2 * t - (t & (stride - 1));
            a[j] = keys[lo[j]];
            b[j] = keys[lo[j] + stride];
        }
#pragma unroll
        for (int j = 0; j < PASSES; ++j)
            if ((a[j] < b[j]) == ((lo[j] & size) == 0)) { keys[lo[j]] = b[j]; keys[lo[j] + stride] = a[j]; }
        wave_lds_sync();
    }
}

// every 128-key segment sorted, segment j descending for even j and ascending for odd j (the network of sizes 2 .. 128)
template <int N>
__device__ __forceinline__ void sort_runs128(unsigned long long* keys) {
    for (int size = 2; size <= 128; size <<= 1) bitonic_wave_stages<N>(keys, size, size >> 1);
}

template <int N>
__device__ void bitonic_sort_desc_lean(unsigned long long* keys) {   // N power of two >= 128, blockDim a multiple of 64
    __syncthreads();
    sort_runs128<N>(keys);
    for (int size = 256; size <= N; size <<= 1) {
        for (int stride = size >> 1; stride > 64; stride >>= 1) {
            __syncthreads();
            for (int t = threadIdx.x; t < N / 2; t += blockDim.x) {
                const int lo = 2 * t - (t & (stride - 1));
                cmpx(keys, lo, lo + stride, (lo & size) == 0);
            }
        }
        __syncthreads();
        bitonic_wave_stages<N>(keys, size, 64);
    }
    __syncthreads();
}

// the upper 128 of N keys, descending, in keys[0, 128)
template <int N>
__device__ void top128_desc(unsigned long long* keys) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, waves = blockDim.x >> 6;
    __syncthreads();
    sort_runs128<N>(keys);
    for (int D = 128; D < N; D <<= 1) {                      // live runs at multiples of D: even ones descending, odd ones ascending
        __syncthreads();
        for (int m = wave; m < N / (2 * D); m += waves) {    // one wave per pair; the winner replaces the even run
            unsigned long long* A = keys + (size_t)2 * m * D;
            const unsigned long long* Bk = A + D;
            const bool desc = (m & 1) == 0;                  // ... as run m of the next round
            const unsigned long long a0 = A[lane], a1 = A[lane + 64], b0 = Bk[lane], b1 = Bk[lane + 64];
            const unsigned long long u = a0 > b0 ? a0 : b0, v = a1 > b1 ? a1 : b1;       // bitonic upper half; stride 64 in registers
            const bool sw = (u < v) == desc;
            A[lane] = sw ? v : u;
            A[lane + 64] = sw ? u : v;
            wave_lds_sync();
            for (int stride = 32; stride > 0; stride >>= 1) {
                const int lo = 2 * lane - (lane & (stride - 1));
                cmpx(A, lo, lo + stride, desc);
                wave_lds_sync();
            }
        }
    }
    __syncthreads();
}

template <int FORM>                                          // 0: the full network; 1: its wave-local stages; 2: the upper 128 only
__global__ __launch_bounds__(1024) void topk_chunk_kernel(const float* __restrict__ logits, int ld,
                                                          const unsigned char* __restrict__ valid, long valid_bs,
                                                          const float* __restrict__ invalid_logit, long S, int k,
                                                          unsigned long long* __restrict__ cand, int chunks) {
    __shared__ unsigned long long keys[CHUNK];
    const int b = blockIdx.y, ch = blockIdx.x;
    const long s0 = (long)ch * CHUNK;
    const float c0 = invalid_logit ? invalid_logit[0] : 0.f;
    for (int t = threadIdx.x; t < CHUNK; t += blockDim.x) {
        const long s = s0 + t;
        unsigned long long key = 0ull;                       // below every real key
        if (s < S) {
            float v = logits[((size_t)b * S + s) * ld];
            if (valid && !valid[b * valid_bs + s]) v = c0;          // valid_bs = S: a flag row per frame (0: one for the batch)
            key = make_key(v, (unsigned)s);
        }
        keys[t] = key;
    }
    if (FORM == 2) top128_desc<CHUNK>(keys);                 // (k <= 128)
    else if (FORM == 1) bitonic_sort_desc_lean<CHUNK>(keys);
    else bitonic_sort_desc<CHUNK>(keys);
    unsigned long long* out = cand + ((size_t)b * chunks + ch) * k;
    for (int t = threadIdx.x; t < k; t += blockDim.x) out[t] = keys[t];
}

template <int N, bool LEAN>
__global__ __launch_bounds__(1024) void topk_merge_kernel(const unsigned long long* __restrict__ cand, int ncand, int k,
                                                          long S, int* __restrict__ idx_out,
                                                          int* __restrict__ rows_out) {
    extern __shared__ unsigned long long mkeys[];
    const int b = blockIdx.x;
    for (int t = threadIdx.x; t < N; t += blockDim.x) mkeys[t] = t < ncand ? cand[(size_t)b * ncand + t] : 0ull;
    if (LEAN) bitonic_sort_desc_lean<N>(mkeys);
    else bitonic_sort_desc<N>(mkeys);
    for (int t = threadIdx.x; t < k; t += blockDim.x) {
        const int s = (int)(0xFFFFFFFFu - (unsigned)(mkeys[t] & 0xFFFFFFFFull));
        idx_out[(size_t)b * k + t] = s;
        if (rows_out) rows_out[(size_t)b * k + t] = (int)(b * S + s);   // row into the [B*S, .] token buffers
    }
}

}  // namespace

extern "C" long gom_topk_workspace_bytes(int B, long S, int k) {
    return (long)sizeof(unsigned long long) * B * cdiv(S, CHUNK) * k;
}

static int g_topk_lean = 1;

extern "C" int gom_topk_set_lean(int on) {
    g_topk_lean = on ? 1 : 0;
    return GOM_OK;
}

template <int N, bool LEAN>
static int merge_launch(const unsigned long long* cand, int B, int ncand, int k, long S, int* idx_out, int* rows_out, hipStream_t s) {
    auto kern = topk_merge_kernel<N, LEAN>;
    const int lds = N * sizeof(unsigned long long);
    if (lds > 48 * 1024) {
        // (the attribute is per DEVICE: set on every launch -- a process-wide flag would miss a second GPU; it costs ~1 us)
        hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
        if (e != hipSuccess) return GOM_ERR_HIP_BASE + (int)e;
    }
    hipLaunchKernelGGL(kern, dim3((unsigned)B), dim3(1024), lds, s, cand, ncand, k, S, idx_out, rows_out);
    return gom_launch_status();
}

static int topk_launch(const float* logits, int ld, const unsigned char* valid, long valid_bs, const float* invalid_logit,
                       int B, long S, int k, void* workspace, int* idx_out, int* rows_out, void* stream) {
    GOM_CHECK_ARG(logits && workspace && idx_out && B > 0 && S > 0 && k > 0 && ld >= 1);
    const int chunks = cdiv(S, CHUNK);
    GOM_CHECK_ARG(k <= CHUNK && k <= S && (long)chunks * k <= MERGE_MAX && (long)B * S < (1L << 31));
    hipStream_t s = (hipStream_t)stream;
    unsigned long long* cand = (unsigned long long*)workspace;
    const dim3 grid((unsigned)chunks, (unsigned)B);
    const int ncand = chunks * k;
    if (!g_topk_lean) {
        hipLaunchKernelGGL(topk_chunk_kernel<0>, grid, dim3(1024), 0, s, logits, ld, valid, valid_bs, invalid_logit, S, k, cand,
                           chunks);
        return merge_launch<MERGE_MAX, false>(cand, B, ncand, k, S, idx_out, rows_out, s);
    }
    if (k <= 128)
        hipLaunchKernelGGL(topk_chunk_kernel<2>, grid, dim3(1024), 0, s, logits, ld, valid, valid_bs, invalid_logit, S, k, cand,
                           chunks);
    else
        hipLaunchKernelGGL(topk_chunk_kernel<1>, grid, dim3(1024), 0, s, logits, ld, valid, valid_bs, invalid_logit, S, k, cand,
                           chunks);
    if (ncand <= 1024) return merge_launch<1024, true>(cand, B, ncand, k, S, idx_out, rows_out, s);
    if (ncand <= 2048) return merge_launch<2048, true>(cand, B, ncand, k, S, idx_out, rows_out, s);
    if (ncand <= 4096) return merge_launch<4096, true>(cand, B, ncand, k, S, idx_out, rows_out, s);
    return merge_launch<MERGE_MAX, true>(cand, B, ncand, k, S, idx_out, rows_out, s);
}

extern "C" int gom_topk_tokens(const float* logits, int ld, const unsigned char* valid, const float* invalid_logit,
                               int B, long S, int k, void* workspace, int* idx_out, int* rows_out, void* stream) {
    return topk_launch(logits, ld, valid, 0, invalid_logit, B, S, k, workspace, idx_out, rows_out, stream);
}

/* ... with a validity row per frame: valid [B][S] (a padded batch whose frames have their own valid extents) */
extern "C" int gom_topk_tokens_frames(const float* logits, int ld, const unsigned char* valid, const float* invalid_logit,
                                      int B, long S, int k, void* workspace, int* idx_out, int* rows_out, void* stream) {
    GOM_CHECK_ARG(valid);
    return topk_launch(logits, ld, valid, S, invalid_logit, B, S, k, workspace, idx_out, rows_out, stream);
}
