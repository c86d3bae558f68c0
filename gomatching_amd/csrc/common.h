// Shared helpers for the gfx950 kernels of the GoMatching hot path.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/gomatching_hip.h"

#define GOM_CHECK_ARG(cond)                      \
    do {                                         \
        if (!(cond)) return GOM_ERR_INVALID_ARG; \
    } while (0)

// Launch-error reporting: unlike the reference (which only printf()s cudaGetLastError,
// ms_deform_im2col_cuda.cuh:948-952) every entry point returns the HIP error to the caller.
static inline int gom_launch_status() {
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? GOM_OK : (GOM_ERR_HIP_BASE + (int)e);
}

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 half2_t __attribute__((ext_vector_type(2)));
typedef _Float16 half8 __attribute__((ext_vector_type(8)));

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

static inline int cdiv(long a, long b) { return (int)((a + b - 1) / b); }

// The f16x3 split of two fp32 values, x = h0 + h1 with h0 = fp16(x), h1 = fp16(x - h0) (gemm_f16x3.hip): `hi` / `lo` = the packed
// (x, y) halves of the two planes.  The residual x - float(h0) is ONE v_fma_mix_f32 per value (the fp16 operand is widened
// inside the instruction, times -1.0, plus x: exact product, one rounding) instead of v_cvt_f32_f16 + v_sub_f32: the same bits
// (tests/test_ops_gpu.py compares the planes with a numpy statement of the split), a third fewer VALU instructions -- which is
// what every kernel that splits activations in its loop pays with (4 cycles per wave-instruction, matrix pipe idle meanwhile).
__device__ __forceinline__ void gom_split2_f16(float x, float y, unsigned int& hi, unsigned int& lo) {
    const f32x2 v = {x, y};
    hi = __builtin_bit_cast(unsigned int, __builtin_convertvector(v, half2_t));
    float rx, ry;
    asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel_hi:[1,0,0]" : "=v"(rx) : "v"(hi), "v"(x));
    asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "=v"(ry) : "v"(hi), "v"(y));
    const f32x2 r = {rx, ry};
    lo = __builtin_bit_cast(unsigned int, __builtin_convertvector(r, half2_t));
}

// A launch's weight image towards this XCD's L2, once, at the start.  Between two launches that use it the image (0.3 - 3.4 MB, last
// read a layer or a step ago) is in HBM; every workgroup of a round then streams the same stage at the same time, and a ring's one or
// two stages of lookahead do not cover a miss per stage (dec_attn2.hip: inter + raw 76 us warm, 100 us behind a 768 MB fill, 88 us with
// this).  Workgroups go to the XCDs round-robin (1-D grids): the first-round workgroups of an XCD (at most 32) touch one line in 128
// bytes of the image each, a slice per workgroup.  The loads' results are never used; they are the oldest vector-memory operations of
// the wave, so the first counted wait of the kernel covers them.  Decoder launches only (one round of one-per-CU workgroups, 200-250 of
// them): in the encoder's and the backbone's row-resident kernels -- nine or more rounds, the image cold for the first only -- the
// same call measured -0.5 % frames/s (same box, three alternating pairs) and is not made.
// K loads per lane, unconditional (addresses clamped), unrolled and ORDINARY: the compiler then counts them like any other load.  (A
// loop of unknown length or a branch makes it wait for every outstanding load at the next use of any loaded value; a `volatile` load is
// followed by a wait for ALL of them on the spot -- either way the prologue's rows wait for the image's lines, +7k cycles.)  The
// values land in pf[]; gom_prefetch_done(pf) -- a use that generates no code -- goes where the kernel has to wait for its first
// loads anyway.  K x nthreads lines per workgroup are covered; a launch of few workgroups covers less.
template <int K>
__device__ __forceinline__ void gom_prefetch_image(const void* img, unsigned bytes, unsigned tid, unsigned nthreads, unsigned (&pf)[K]) {
    const unsigned first = gridDim.x < 256u ? gridDim.x : 256u;
    const unsigned nsl = (first + 7) / 8, sl = (blockIdx.x < first ? blockIdx.x : 0u) / 8;
    const unsigned lines = bytes / 128;
    const unsigned per = (lines + nsl - 1) / nsl;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        unsigned l = tid + k * nthreads;
        l = l < per ? l : per - 1;
        unsigned line = sl * per + l;
        line = line < lines ? line : lines - 1;
        pf[k] = *reinterpret_cast<const unsigned*>(reinterpret_cast<const unsigned char*>(img) + (size_t)line * 128);
    }
}
template <int K>
__device__ __forceinline__ void gom_prefetch_done(const unsigned (&pf)[K]) {
#pragma unroll
    for (int k = 0; k < K; ++k) asm volatile("" ::"v"(pf[k]));
}

// eight fp32 values -> one MFMA operand fragment piece per plane (hi, lo)
__device__ __forceinline__ void gom_split8_f16(const f32x4 a, const f32x4 b, half8& p0, half8& p1) {
    unsigned int l0, l1, l2, l3, h0, h1, h2, h3;
    gom_split2_f16(a[0], a[1], l0, h0);
    gom_split2_f16(a[2], a[3], l1, h1);
    gom_split2_f16(b[0], b[1], l2, h2);
    gom_split2_f16(b[2], b[3], l3, h3);
    p0 = __builtin_bit_cast(half8, (u32x4{l0, l1, l2, l3}));
    p1 = __builtin_bit_cast(half8, (u32x4{h0, h1, h2, h3}));
}

// four fp32 values -> their two fp16 planes of 4 x 16 bits each: {hi01, hi23} and {lo01, lo23}
__device__ __forceinline__ void gom_split4_f16(const f32x4 v, u32x2& hi, u32x2& lo) {
    unsigned int h0, l0, h1, l1;
    gom_split2_f16(v[0], v[1], h0, l0);
    gom_split2_f16(v[2], v[3], h1, l1);
    hi = u32x2{h0, h1};
    lo = u32x2{l0, l1};
}

__device__ __forceinline__ f32x4 gom_mfma16(const half8 a, const half8 b, const f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
}

// C (+)= A . B on the f16x3 planes with the 32x32x16 MFMA, smallest products first (hi x lo, lo x hi, hi x hi)
__device__ __forceinline__ f32x16 gom_mfma_x3(const half8 a_hi, const half8 a_lo, const half8 b_hi, const half8 b_lo, f32x16 c) {
    c = __builtin_amdgcn_mfma_f32_32x32x16_f16(a_hi, b_lo, c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_32x32x16_f16(a_lo, b_hi, c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_32x32x16_f16(a_hi, b_hi, c, 0, 0, 0);
    return c;
}

// registers 8 s .. 8 s + 7 of a 32x32 accumulator -> the two planes of k-step s of an operand fragment: f[s][plane hi, lo]
__device__ __forceinline__ void gom_acc_to_frags(const f32x16& a, half8 (&f)[2][2]) {
#pragma unroll
    for (int s = 0; s < 2; ++s)
        gom_split8_f16(f32x4{a[8 * s], a[8 * s + 1], a[8 * s + 2], a[8 * s + 3]},
                       f32x4{a[8 * s + 4], a[8 * s + 5], a[8 * s + 6], a[8 * s + 7]}, f[s][0], f[s][1]);
}

// A raw buffer descriptor over `bytes` bytes from `base` (stride 0: the accesses' byte offsets address it; beyond `bytes` a load
// reads zeros and a store is dropped).  Word 3 = 0x00020000: DATA_FORMAT (bits 18:15) = 4, i.e. 32-bit, every other field 0
// (no swizzle, no add-tid); a raw access takes its width from the instruction.
__device__ __forceinline__ __amdgpu_buffer_rsrc_t gom_buffer_rsrc(const void* base, int bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, bytes, 0x00020000);
}

// One KB MFMA operand fragment of a weight stream straight into LDS: each lane moves 16 bytes (buffer_load_dwordx4 ... lds) from
// descriptor `rs` at `voff` (vector) + `soff` (scalar, 0 if left out) to `lds` (the lane's own offset is implied: 16 x lane).  The
// MUBUF form, not global_load_lds: hipcc books a FLAT-segment LDS-DMA as "may return out of order" and from then on turns every
// counted s_waitcnt lgkmcnt(N) of the loop into lgkmcnt(0), which serialises the fragment prefetch of a ring.  An LDS-DMA
// instruction costs its wave 100-140 cycles of issue (s_memtime stamps, gemm_k256.hip: 1250 of the 4200 cycles of a chunk when all
// nine were issued in front of the MFMAs): a ring requests the next stage one piece per few MFMAs, beside which that time is hidden.
// (The destination is the last argument in both forms: the arguments are evaluated in the order the kernels always used.)
__device__ __forceinline__ void gom_dma_fragment(__amdgpu_buffer_rsrc_t rs, unsigned voff, unsigned soff, unsigned char* lds) {
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (__attribute__((address_space(3))) void*)lds, 16, (int)voff, (int)soff, 0, 0);
}
__device__ __forceinline__ void gom_dma_fragment(__amdgpu_buffer_rsrc_t rs, unsigned voff, unsigned char* lds) {
    gom_dma_fragment(rs, voff, 0, lds);
}

constexpr int GOM_FRAG_BYTES = 1024;                     // one MFMA operand fragment: 64 lanes x 8 fp16

// fragments N g .. N g + N - 1 of an LDS stage (`base` = the stage plus this lane's 16 bytes) -> dst[N].  A macro: as a function
// call the same reads moved the kernels' accumulator initialisation in the schedule (ffn_fused.hip, dec_tail.hip, dec_attn.hip).
#define GOM_READ_FRAGS(dst, base, g)                                                                                  \
    _Pragma("unroll") for (int i_ = 0; i_ < (int)(sizeof(dst) / sizeof((dst)[0])); ++i_)                              \
        (dst)[i_] = *reinterpret_cast<const half8*>((base) + ((g) * (int)(sizeof(dst) / sizeof((dst)[0])) + i_) * GOM_FRAG_BYTES);

// sched_group_barrier masks (LLVM's instruction classes)
constexpr int GOM_SG_MFMA = 0x008, GOM_SG_VMEM = 0x010, GOM_SG_VMEM_READ = 0x020, GOM_SG_DS_READ = 0x100;

// Schedule pin of one step of a ring's fragment pipeline: DS_READS fragment reads (the next group's), then DMAS pairs of
// (MFMAS_PER_DMA MFMAs, one LDS-DMA), then TAIL_MFMAS MFMAs.  A zero count emits no group.
template <int DS_READS, int DMAS, int MFMAS_PER_DMA, int TAIL_MFMAS>
__device__ __forceinline__ void gom_pin() {
    if constexpr (DS_READS > 0) __builtin_amdgcn_sched_group_barrier(GOM_SG_DS_READ, DS_READS, 0);
    if constexpr (DMAS > 0) {
        __builtin_amdgcn_sched_group_barrier(GOM_SG_MFMA, MFMAS_PER_DMA, 0);
        __builtin_amdgcn_sched_group_barrier(GOM_SG_VMEM, 1, 0);
        gom_pin<0, DMAS - 1, MFMAS_PER_DMA, TAIL_MFMAS>();
    } else if constexpr (TAIL_MFMAS > 0) {
        __builtin_amdgcn_sched_group_barrier(GOM_SG_MFMA, TAIL_MFMAS, 0);
    }
}

__device__ __forceinline__ float gom_sigmoid(float x) { return 1.f / (1.f + expf(-x)); }

__device__ __forceinline__ float gom_inv_sigmoid(float x) {   // adet/utils/misc.py:115-119, eps 1e-5
    x = fminf(fmaxf(x, 0.f), 1.f);
    const float x1 = fmaxf(x, 1e-5f), x2 = fmaxf(1.f - x, 1e-5f);
    return logf(x1 / x2);
}

// sin and cos of an angle in [0, 2 pi] (the sine embedding's range: a reference point in [0, 1] times 2 pi over dim_t >= 1):
// quadrant by a two-term Cody-Waite reduction (exact with fma for q <= 4), then the cephes single-precision kernels on
// [-pi/4, pi/4] -- within 1 ulp of 1 of the correctly rounded values.  Not ocml's sinf / cosf: their large-argument path keeps
// the compiler from unrolling the embedding loop, and a dynamically indexed operand array goes to scratch.
__device__ __forceinline__ void gom_sincos_0_2pi(float a, float& sn, float& cs) {
    const float q = rintf(a * 0.63661977236758134f);
    float r = fmaf(q, -1.57079637050628662109375f, a);
    r = fmaf(q, 4.37113900018624283e-8f, r);
    const float z = r * r;
    const float ps = fmaf(fmaf(fmaf(-1.9515295891e-4f, z, 8.3321608736e-3f), z, -1.6666654611e-1f) * z, r, r);
    const float pc = fmaf(fmaf(fmaf(2.443315711809948e-5f, z, -1.388731625493765e-3f), z, 4.166664568298827e-2f) * z, z, fmaf(-0.5f, z, 1.f));
    const int qi = (int)q;
    const float s0 = (qi & 1) ? pc : ps, c0 = (qi & 1) ? ps : pc;
    sn = (qi & 2) ? -s0 : s0;
    cs = ((qi + 1) & 2) ? -c0 : c0;
}

// sum over the four lane groups (lanes n, n + 16, n + 32, n + 48), result in all of them
__device__ __forceinline__ float gom_groups_sum(float v) {
    v += __shfl_xor(v, 16, 64);
    v += __shfl_xor(v, 32, 64);
    return v;
}

// sum over the 16 lanes of a DPP row, result in every lane: quad swaps (xor 1, xor 2), then the two mirrors
__device__ __forceinline__ float gom_row16_sum(float v) {
    auto dpp = [](float x, int ctrl_tag) {
        const int xi = __builtin_bit_cast(int, x);
        int r;
        if (ctrl_tag == 0) r = __builtin_amdgcn_update_dpp(0, xi, 0xB1, 0xF, 0xF, true);        // quad_perm [1,0,3,2]
        else if (ctrl_tag == 1) r = __builtin_amdgcn_update_dpp(0, xi, 0x4E, 0xF, 0xF, true);   // quad_perm [2,3,0,1]
        else if (ctrl_tag == 2) r = __builtin_amdgcn_update_dpp(0, xi, 0x141, 0xF, 0xF, true);  // row_half_mirror
        else r = __builtin_amdgcn_update_dpp(0, xi, 0x140, 0xF, 0xF, true);                     // row_mirror
        return __builtin_bit_cast(float, r);
    };
    v += dpp(v, 0);
    v += dpp(v, 1);
    v += dpp(v, 2);
    v += dpp(v, 3);
    return v;
}

// A wave's 32 rows x 256 fp32 -> the two fp16 planes of its MFMA operand fragments: lane (r = lane & 31, h = lane >> 5) ends up
// with floats 16 s + 8 h .. + 7 of row r for every k-step s, xf[plane][s].  Loading that layout straight from memory makes every
// wave-instruction touch 32 lines (16-byte pieces of 32 rows), and the texture-address unit pays per LINE (~3.6 cycles,
// profiles/r03_msda_ta_counters.txt): the 128 such instructions of a 128-row tile cost it ~14 000 cycles -- which is what the
// prologue of every row-resident kernel measured (ffn_fused.hip: 14.2k).  Here the rows are loaded as WHOLE lines (a wave-
// instruction = W floats of 256 / W rows: 8 lines) and change layout in a wave-private LDS scratch of 32 x W fp32 (16-byte
// pieces XOR-swizzled by the row: conflict-free both ways), W of a row's 256 floats at a time.  `row_a(r)` / `row_b(r)` return
// the address of row r (0..31) of the wave; ADD: the fragments are those of row_a + row_b.  `amax` = running largest magnitude
// (the f16x3 range check).  The wave barriers keep the compiler from moving the exchange into divergent code.
// `after_first_loads()` runs once, behind the first part's loads (where a kernel requests its first weight stage: the rows are
// then ahead of it in the memory queue and the first split runs while the weights are still on their way).
// K32 = true: the fragments of the 16x16x32 MFMA shape instead -- lane (n = lane & 15, kg = lane >> 4) ends up with floats
// 32 s + 8 kg .. + 7 of row 16 R + n for every 32-wide k-step s and row group R, xf[plane][8 R + s].
template <int W, bool ADD, bool K32, typename FA, typename FB, typename FH>
__device__ __forceinline__ void gom_rows_to_fragments_t(FA row_a, FB row_b, float* scratch, int lane, half8 (&xf)[2][16], float& amax,
                                                        FH after_first_loads) {
    constexpr int PC = W / 4;                                // 16-byte pieces of a row part
    constexpr int RPI = 64 / PC;                             // rows per wave-instruction
    constexpr int NI = 32 / RPI;                             // wave-instructions per part
    const int pc = lane % PC, r0 = lane / PC;
    const int fr = lane & 31, fh = lane >> 5;
#pragma unroll
    for (int part = 0; part < 256 / W; ++part) {
        f32x4 v[NI];
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            const int r = r0 + RPI * i;
            v[i] = *reinterpret_cast<const f32x4*>(row_a(r) + part * W + pc * 4);
            if constexpr (ADD) v[i] += *reinterpret_cast<const f32x4*>(row_b(r) + part * W + pc * 4);
        }
        if (part == 0) {
            __builtin_amdgcn_sched_barrier(0);
            after_first_loads();
            __builtin_amdgcn_sched_barrier(0);
        }
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            const int r = r0 + RPI * i;
            *reinterpret_cast<f32x4*>(scratch + r * W + ((pc ^ (r & (PC - 1))) << 2)) = v[i];
        }
        __builtin_amdgcn_wave_barrier();
        if constexpr (K32) {
            const int n = lane & 15, kg = lane >> 4;
#pragma unroll
            for (int s = 0; s < W / 32; ++s)
#pragma unroll
                for (int R = 0; R < 2; ++R) {
                    const int row = 16 * R + n, p0 = 8 * s + 2 * kg;
                    const f32x4 a = *reinterpret_cast<const f32x4*>(scratch + row * W + ((p0 ^ (row & (PC - 1))) << 2));
                    const f32x4 b = *reinterpret_cast<const f32x4*>(scratch + row * W + (((p0 + 1) ^ (row & (PC - 1))) << 2));
#pragma unroll
                    for (int e = 0; e < 4; ++e) amax = fmaxf(amax, fmaxf(fabsf(a[e]), fabsf(b[e])));
                    gom_split8_f16(a, b, xf[0][8 * R + part * (W / 32) + s], xf[1][8 * R + part * (W / 32) + s]);
                }
        } else {
#pragma unroll
            for (int s = 0; s < W / 16; ++s) {
                const int p0 = 4 * s + 2 * fh;
                const f32x4 a = *reinterpret_cast<const f32x4*>(scratch + fr * W + ((p0 ^ (fr & (PC - 1))) << 2));
                const f32x4 b = *reinterpret_cast<const f32x4*>(scratch + fr * W + (((p0 + 1) ^ (fr & (PC - 1))) << 2));
#pragma unroll
                for (int e = 0; e < 4; ++e) amax = fmaxf(amax, fmaxf(fabsf(a[e]), fabsf(b[e])));
                gom_split8_f16(a, b, xf[0][part * (W / 16) + s], xf[1][part * (W / 16) + s]);
            }
        }
        __builtin_amdgcn_wave_barrier();
    }
    asm volatile("" : "+v"(amax));                           // decided here (dec_attn.hip: deferred compares spill)
}

template <int W, bool ADD, typename FA, typename FB, typename FH>
__device__ __forceinline__ void gom_rows_to_fragments(FA row_a, FB row_b, float* scratch, int lane, half8 (&xf)[2][16], float& amax,
                                                      FH after_first_loads) {
    gom_rows_to_fragments_t<W, ADD, false>(row_a, row_b, scratch, lane, xf, amax, after_first_loads);
}
