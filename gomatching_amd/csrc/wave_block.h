// The integer scan and reduce of the byte-pipeline kernels (result text / parse, scene polygons, lexicon rows, track vote, JPEG,
// mask pairs, lexicon match): ONE wave64 inclusive scan, ONE block exclusive scan, ONE wave / block reduce.  Device only; every
// operation is exact on integers, so which copy a kernel calls is not part of its results.  (The float and double reductions of
// the hot path are not here: their order IS part of their results.)
//
// Blocks are one-dimensional and a multiple of 64 threads: lane = threadIdx.x & 63, wave = threadIdx.x >> 6.
#pragma once
#include <hip/hip_runtime.h>

// ---- wave64 inclusive scan: lane l gets v[0] + .. + v[l].  T: int, unsigned, long, long long (what __shfl_up moves)
template <typename T>
__device__ __forceinline__ T wb_wave_incl_scan(T v) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const T o = __shfl_up(v, d, 64);
        if (lane >= d) v += o;
    }
    return v;
}

// ---- block exclusive scan over the BLOCK threads -> this thread's prefix; total = the block's sum, in every thread.
// EVERY thread of the block must call it (two barriers), with the same wsum[BLOCK / 64].  It ENDS with a barrier: when it
// returns, every thread has read wsum, so the next call (or any other use) may write the same wsum at once.
template <int BLOCK, typename T>
__device__ __forceinline__ T wb_block_excl_scan(T v, T* wsum, T& total) {
    static_assert(BLOCK % 64 == 0, "a block is whole waves");
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const T incl = wb_wave_incl_scan(v);
    if (lane == 63) wsum[w] = incl;
    __syncthreads();
    T base = 0, tot = 0;
#pragma unroll
    for (int i = 0; i < BLOCK / 64; ++i) {
        const T s = wsum[i];
        if (i < w) base += s;
        tot += s;
    }
    __syncthreads();
    total = tot;
    return base + incl - v;
}

// the carry form of the tiled loops: the prefix includes the carry of the tiles before, and the carry moves on by this tile's
// total.  The same rules: every thread calls it, and it ends with the barrier that frees wsum.
template <int BLOCK, typename T>
__device__ __forceinline__ T wb_block_excl_scan_carry(T v, T* wsum, T& carry) {
    T total;
    const T excl = carry + wb_block_excl_scan<BLOCK, T>(v, wsum, total);
    carry += total;
    return excl;
}

// ---- reduce: sum, OR, min, max of integers (64-bit unsigned keys included)
struct WbSum {
    template <typename T>
    static __device__ __forceinline__ T of(T a, T b) { return a + b; }
};
struct WbOr {
    template <typename T>
    static __device__ __forceinline__ T of(T a, T b) { return a | b; }
};
struct WbMin {
    template <typename T>
    static __device__ __forceinline__ T of(T a, T b) { return b < a ? b : a; }
};
struct WbMax {
    template <typename T>
    static __device__ __forceinline__ T of(T a, T b) { return b > a ? b : a; }
};

// over the wave: every lane gets the result
template <typename Op, typename T>
__device__ __forceinline__ T wb_wave_reduce(T v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = Op::of(v, (T)__shfl_xor(v, d, 64));
    return v;
}

// over the block, in two steps around the CALLER's barrier, so that several values go through one barrier:
//     wb_block_stage<Op>(a, slot_a); wb_block_stage<Op>(b, slot_b); __syncthreads();
//     if (threadIdx.x == 0) { a = wb_block_fold<BLOCK, Op>(slot_a); b = wb_block_fold<BLOCK, Op>(slot_b); ... }
// stage: the wave's result to slot[wave] (every thread calls it; slot: BLOCK / 64 values).  fold: the waves' results, for the one
// thread that wants them.  Nothing is broadcast and no barrier follows: a slot is not free for another use before the block's
// next barrier.
template <typename Op, typename T>
__device__ __forceinline__ void wb_block_stage(T v, T* slot) {
    v = wb_wave_reduce<Op>(v);
    if ((threadIdx.x & 63) == 0) slot[threadIdx.x >> 6] = v;
}

template <int BLOCK, typename Op, typename T>
__device__ __forceinline__ T wb_block_fold(const T* slot) {
    static_assert(BLOCK % 64 == 0, "a block is whole waves");
    T r = slot[0];
#pragma unroll
    for (int i = 1; i < BLOCK / 64; ++i) r = Op::of(r, slot[i]);
    return r;
}

// one value: stage, the barrier, fold -> the result in thread 0 ALONE (what another thread gets means nothing).  Every thread
// calls it.
template <int BLOCK, typename Op, typename T>
__device__ __forceinline__ T wb_block_reduce(T v, T* slot) {
    wb_block_stage<Op>(v, slot);
    __syncthreads();
    return threadIdx.x == 0 ? wb_block_fold<BLOCK, Op>(slot) : v;
}
