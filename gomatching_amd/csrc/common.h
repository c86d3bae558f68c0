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

// Workgroups are dealt round-robin over the 8 XCDs (blocks b and b + 8 share one, MI355X_MICROARCH.md), so with the plain
// blockIdx -> work map every XCD's private L2 sees every 8th tile (or group of queries): neighbours, which read the same cache
// lines, sit on eight different L2s and every such line is fetched up to eight times.  This remap, bijective for any grid size,
// hands each XCD one contiguous eighth of the grid instead.  Speed only.
__device__ __forceinline__ int gom_xcd_contiguous_block(int bid, int nwg) {
    const int q = nwg >> 3, r = nwg & 7, xcd = bid & 7;
    return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (bid >> 3);
}

// ---- The tile GEMM / implicit-GEMM convolution on pre-split weight planes: the frame of gemm_f16x3.hip and gemm_bf16x6.hip ----
//
//   C[M,N] = epilogue( A[M,K] . W[N,K]^T ),  fp32 in, fp32 out
//
// Weights are constants: they are split ONCE into P::PLANES 16-bit planes [PLANES][N][Kpad] and stream global -> LDS with no VALU
// work.  Activations are split in registers on their way to LDS.  Tile 128 x (64 | 128) x 32, 4 waves (2 x 2, MFMA 32x32x16 tiles
// each), one LDS buffer + register prefetch (two barriers per k-tile; the CU's other workgroups' MFMAs cover this one's split/store
// phase), LDS rows padded to 80 B so ds_read_b128 fragment reads are conflict-free, XCD-aware tile order, implicit-im2col
// addressing (KH > 0) and split-K.  A back-end is a policy P -- the kernel has no run-time branch on it:
//   PLANES                 planes per operand
//   OCC                    workgroups per CU: >= 3 keeps ONE k-tile of A in flight, 2 keeps two (HBM latency > one MFMA phase)
//   frag                   the MFMA operand fragment type (8 x 16 bits)
//   split4(v, pl)          four activations -> their PLANES planes of 4 x 16 bits each
//   mma(a, b, c)           c += the plane products of one 32x32x16 block, smallest terms first
//   kernel<BM,BN,KH,KW>()  host: the back-end's __global__ wrapper of gom_tile_gemm
constexpr int GOM_TILE_BK = 32;
constexpr int GOM_TILE_ROW_BYTES = 80;           // 32 x 16 bits + 16 B pad: 5 sixteen-byte slots (odd) per row

struct GomTileArgs {
    const float* A;
    const unsigned short* Wp;                    // [PLANES][N][ldw] planes
    const float* wscale;                         // [N] or nullptr: applied to the accumulator before scale/shift (f16x3: 2^-e_n)
    int* flag;                                   // device word or nullptr, set non-zero when a result is not finite
    long w_plane_stride;                         // elements between planes
    float* C;
    const float* scale;
    const float* shift;
    const float* R;
    const int* a_rows;
    int M, N, K;
    int lda, ldw, ldc, ldr;
    int relu;                                    // 0 none, 1 ReLU, 2 GELU
    int r_cols;                                  // residual applies to columns < r_cols
    int r_period;                                // > 0: row m reads residual row m % r_period (a table shared by the frames)
    int H, Wd, cin_log2, OH, OW, stride, pad;
    // split-K (few output tiles, long K): blockIdx.y owns k-tiles [y*kt_per_split, ...) and stores raw partial sums
    int kt_per_split;
    float* partial;                              // [splits][M][N] or nullptr
};

template <class P, int BM, int BN, int KH, int KW>
__device__ __forceinline__ void gom_tile_gemm(const GomTileArgs p) {
    constexpr int BK = GOM_TILE_BK, ROW_BYTES = GOM_TILE_ROW_BYTES, PLANES = P::PLANES;
    constexpr int WM = BM / 2, WN = BN / 2;                  // 2 x 2 waves
    constexpr int MT = WM / 32, NT = WN / 32;
    constexpr int A_UNITS = BM * 8 / 256;                    // float4 units per thread per k-tile (8 per row)
    constexpr int W_UNITS = BN * 4 / 256;                    // 16-byte units per thread per plane (4 per row)
    constexpr bool CONV = KH > 0;
    constexpr int A_PLANE = BM * ROW_BYTES, W_PLANE = BN * ROW_BYTES;
    typedef typename P::frag frag;

    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned char* As = smem;                                // [PLANES][BM][80 B]
    unsigned char* Ws = smem + PLANES * A_PLANE;             // [PLANES][BN][80 B]

    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int wr = wave >> 1, wc = wave & 1;

    const int tiles_n = (p.N + BN - 1) / BN;
    const int bid = gom_xcd_contiguous_block(blockIdx.x, gridDim.x);
    const int tm = bid / tiles_n, tn = bid % tiles_n;
    const int m0 = tm * BM, n0 = tn * BN;

    // ---- buffer descriptors: 32-bit byte offsets, out-of-range lanes read zeros (no select instructions) ----
    constexpr unsigned RANGE = 0x80000000u, INVALID = 0xC0000000u;       // offsets stay OOB after adding < 1 GiB
    const __amdgpu_buffer_rsrc_t rsA = gom_buffer_rsrc(p.A, (int)RANGE);
    const __amdgpu_buffer_rsrc_t rsW = gom_buffer_rsrc(p.Wp, (int)RANGE);

    // A: unit u = tid + i*256 -> row u>>3, k-quad u&7.  a_off = byte offset of (row, k = kq*4) or of the tap origin
    const int kq = tid & 7;
    unsigned a_off[A_UNITS];
    int a_ih0[A_UNITS], a_iw0[A_UNITS];
#pragma unroll
    for (int i = 0; i < A_UNITS; ++i) {
        const int row = (tid >> 3) + i * 32;
        const int m = m0 + row;
        const bool ok = m < p.M;
        const int mm = ok ? m : 0;
        if (CONV) {
            const int ow = mm % p.OW;
            const int t = mm / p.OW;
            const int oh = t % p.OH;
            const int b = t / p.OH;
            a_ih0[i] = ok ? oh * p.stride - p.pad : -(1 << 28);            // invalid row: every tap fails the bounds test
            a_iw0[i] = ow * p.stride - p.pad;
            a_off[i] = (unsigned)((((b * p.H + oh * p.stride - p.pad) * p.Wd + a_iw0[i]) << p.cin_log2) * 4);
        } else {
            const int src = p.a_rows ? p.a_rows[mm] : mm;
            a_off[i] = ok ? (unsigned)(src * p.lda + kq * 4) * 4u : INVALID;
            a_ih0[i] = a_iw0[i] = 0;
        }
    }
    // W: unit u = tid + i*256 -> row u>>2, 16-byte chunk u&3 (8 x 16 bits); byte offsets into plane 0
    const int wq = tid & 3;
    unsigned w_off[W_UNITS];
#pragma unroll
    for (int i = 0; i < W_UNITS; ++i) {
        const int n = n0 + (tid >> 2) + i * 64;
        w_off[i] = n < p.N ? (unsigned)(n * p.ldw + wq * 8) * 2u : INVALID;
    }
    const unsigned w_plane_bytes = (unsigned)(p.w_plane_stride * 2);

    f32x4 a_even[A_UNITS], a_odd[A_UNITS];                 // a_odd: the second k-tile in flight of the two-deep form
    u32x4 w_reg[PLANES][W_UNITS];

    const int nk_all = (p.K + BK - 1) / BK;
    const int ktb = p.partial ? (int)blockIdx.y * p.kt_per_split : 0;   // first k-tile of this workgroup
    const int nk = p.partial ? max(0, min(nk_all - ktb, p.kt_per_split)) : nk_all;

    auto load_A = [&](int kt_rel, f32x4 (&a_reg)[A_UNITS]) {
        const int kt = kt_rel + ktb;
        unsigned koff = (unsigned)(kt * BK) * 4u;            // plain GEMM: columns kt*BK..
        const bool k_ok = kt * BK + kq * 4 < p.K;            // K tail reads nothing (weights are zero there anyway)
        int kh = 0, kw = 0;
        if (CONV) {
            const int k = kt * BK + kq * 4;
            const int c = k & ((1 << p.cin_log2) - 1);
            const int khw = k >> p.cin_log2;
            kh = khw / KW;
            kw = khw - kh * KW;
            koff = (unsigned)((((kh * p.Wd + kw) << p.cin_log2) + c) * 4);
            if (k >= p.K) kh = 1 << 28;                      // K tail: force out of range
        }
#pragma unroll
        for (int i = 0; i < A_UNITS; ++i) {
            unsigned off = a_off[i] + koff;
            if (!CONV && !k_ok) off = INVALID;
            if (CONV) {
                const int ih = a_ih0[i] + kh, iw = a_iw0[i] + kw;
                if (!(((unsigned)ih < (unsigned)p.H) && ((unsigned)iw < (unsigned)p.Wd))) off = INVALID;
            }
            a_reg[i] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsA, (int)off, 0, 0));
        }
    };
    auto load_W = [&](int kt_rel) {
        const unsigned koff = (unsigned)((kt_rel + ktb) * BK) * 2u;      // planes are zero-padded to ldw (multiple of 32)
#pragma unroll
        for (int pl = 0; pl < PLANES; ++pl)
#pragma unroll
            for (int i = 0; i < W_UNITS; ++i)
                w_reg[pl][i] = __builtin_amdgcn_raw_buffer_load_b128(rsW, (int)(w_off[i] + koff + pl * w_plane_bytes), 0, 0);
    };
    auto store_tile = [&](const f32x4 (&a_reg)[A_UNITS]) {  // split A in registers, then A planes + W planes -> LDS
#pragma unroll
        for (int i = 0; i < A_UNITS; ++i) {
            const int row = (tid >> 3) + i * 32;
            u32x2 pv[PLANES];
            P::split4(a_reg[i], pv);
            unsigned char* d = As + row * ROW_BYTES + kq * 8;
#pragma unroll
            for (int pl = 0; pl < PLANES; ++pl) *reinterpret_cast<u32x2*>(d + pl * A_PLANE) = pv[pl];
        }
#pragma unroll
        for (int pl = 0; pl < PLANES; ++pl)
#pragma unroll
            for (int i = 0; i < W_UNITS; ++i) {
                const int row = (tid >> 2) + i * 64;
                *reinterpret_cast<u32x4*>(Ws + pl * W_PLANE + row * ROW_BYTES + wq * 16) = w_reg[pl][i];
            }
    };

    f32x16 acc[MT][NT];
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    const int fr = lane & 31, fh = lane >> 5;
    const unsigned char* a_base = As + (wr * WM + fr) * ROW_BYTES + fh * 16;
    const unsigned char* w_base = Ws + (wc * WN + fr) * ROW_BYTES + fh * 16;

    auto compute = [&]() {
#pragma unroll
        for (int ks = 0; ks < BK / 16; ++ks) {
            frag af[MT][PLANES];
#pragma unroll
            for (int pl = 0; pl < PLANES; ++pl)
#pragma unroll
                for (int i = 0; i < MT; ++i)
                    af[i][pl] = *reinterpret_cast<const frag*>(a_base + pl * A_PLANE + i * 32 * ROW_BYTES + ks * 32);
#pragma unroll
            for (int j = 0; j < NT; ++j) {
                frag bf[PLANES];
#pragma unroll
                for (int pl = 0; pl < PLANES; ++pl)
                    bf[pl] = *reinterpret_cast<const frag*>(w_base + pl * W_PLANE + j * 32 * ROW_BYTES + ks * 32);
#pragma unroll
                for (int i = 0; i < MT; ++i) acc[i][j] = P::mma(af[i], bf, acc[i][j]);
            }
        }
    };

    if constexpr (P::OCC >= 3) {
        // one k-tile of A in flight; the CU's other workgroups cover the latency
        if (nk > 0) {
            load_A(0, a_even);
            load_W(0);
            store_tile(a_even);
        }
        __syncthreads();
        for (int kt = 0; kt < nk; ++kt) {
            if (kt + 1 < nk) {
                load_W(kt + 1);
                load_A(kt + 1, a_even);
            }
            compute();
            __syncthreads();
            if (kt + 1 < nk) {
                store_tile(a_even);
                __syncthreads();
            }
        }
    } else {
        if (nk > 0) {
            load_A(0, a_even);
            load_W(0);
            if (nk > 1) load_A(1, a_odd);
            store_tile(a_even);
        }
        __syncthreads();

        for (int kt = 0; kt < nk; kt += 2) {
            // tile kt is in LDS, a_odd holds tile kt+1 (issued a whole iteration ago)
            if (kt + 1 < nk) load_W(kt + 1);
            if (kt + 2 < nk) load_A(kt + 2, a_even);
            compute();
            __syncthreads();
            if (kt + 1 >= nk) break;
            store_tile(a_odd);
            __syncthreads();
            // tile kt+1 is in LDS, a_even holds tile kt+2
            if (kt + 2 < nk) load_W(kt + 2);
            if (kt + 3 < nk) load_A(kt + 3, a_odd);
            compute();
            __syncthreads();
            if (kt + 2 < nk) {
                store_tile(a_even);
                __syncthreads();
            }
        }
    }

    // ---- epilogue: y = acc*scale + shift (+ residual) (ReLU) --------------------------------------
    const float relu_lo = p.relu == 1 ? 0.f : -INFINITY;
    int bad = 0;
    if (p.partial) {                                         // split-K: raw sums, the reducer applies the epilogue
        float* dst = p.partial + (size_t)blockIdx.y * p.M * p.N;
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            const int n = n0 + wc * WN + j * 32 + fr;
#pragma unroll
            for (int i = 0; i < MT; ++i)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int m = m0 + wr * WM + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * fh;
                    if (n < p.N && m < p.M) dst[(size_t)m * p.N + n] = acc[i][j][r];
                }
        }
        return;
    }
    const bool vec_ok = ((p.N | p.ldc) & 3) == 0 && (!p.R || (p.ldr & 3) == 0);
    if (vec_ok) {
        // stage each 32-row slab of the wave's patch through (now free) LDS so that global traffic is whole
        // 16-byte pieces of contiguous rows: 4x fewer store/load instructions than the per-register pattern
        constexpr int ES = WN + 4;                           // padded row (floats)
        float* stage = reinterpret_cast<float*>(smem) + wave * (32 * ES);
        constexpr int C4 = WN / 4;                           // float4 per row
        constexpr int RPI = 64 / C4;                         // rows covered per wave-instruction
#pragma unroll
        for (int i = 0; i < MT; ++i) {
#pragma unroll
            for (int j = 0; j < NT; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    stage[((r & 3) + 8 * (r >> 2) + 4 * fh) * ES + j * 32 + fr] = acc[i][j][r];
            __builtin_amdgcn_s_waitcnt(0xC07F);              // lgkmcnt(0): the slab is wave-private
            const int c4 = (lane % C4) * 4;
            const int n = n0 + wc * WN + c4;
            const bool n_ok = n < p.N;
            f32x4 sc = {1.f, 1.f, 1.f, 1.f}, sh = {0.f, 0.f, 0.f, 0.f};
            if (n_ok && p.scale) sc = *reinterpret_cast<const f32x4*>(p.scale + n);
            if (n_ok && p.wscale) sc = sc * *reinterpret_cast<const f32x4*>(p.wscale + n);   // exact: a power of two
            if (n_ok && p.shift) sh = *reinterpret_cast<const f32x4*>(p.shift + n);
            const bool use_r = p.R && n < p.r_cols;
            f32x4 rv[32 / RPI];
#pragma unroll
            for (int t = 0; t < 32 / RPI; ++t) {
                const int m = m0 + wr * WM + i * 32 + t * RPI + lane / C4;
                rv[t] = f32x4{0.f, 0.f, 0.f, 0.f};
                if (use_r && n_ok && m < p.M)
                    rv[t] = *reinterpret_cast<const f32x4*>(p.R + (size_t)(p.r_period > 0 ? m % p.r_period : m) * p.ldr + n);
            }
#pragma unroll
            for (int t = 0; t < 32 / RPI; ++t) {
                const int row = t * RPI + lane / C4;
                const int m = m0 + wr * WM + i * 32 + row;
                f32x4 v = *reinterpret_cast<const f32x4*>(stage + row * ES + c4);
                v = v * sc + sh + rv[t];
                // range check on the PRE-activation value: fmaxf(NaN, 0) = 0 would hide the Inf - Inf of an operand beyond fp16
                const bool bad_v = !(fabsf(v[0]) <= 3.4e38f) | !(fabsf(v[1]) <= 3.4e38f) | !(fabsf(v[2]) <= 3.4e38f) |
                                   !(fabsf(v[3]) <= 3.4e38f);
                if (p.relu == 2) {                           // exact GELU (Swin MLP, swin_transformer.py:36-38)
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = 0.5f * v[e] * (1.f + erff(v[e] * 0.70710678118654752440f));
                } else {
                    v[0] = fmaxf(v[0], relu_lo); v[1] = fmaxf(v[1], relu_lo);
                    v[2] = fmaxf(v[2], relu_lo); v[3] = fmaxf(v[3], relu_lo);
                }
                if (n_ok && m < p.M) {
                    bad |= bad_v;
                    *reinterpret_cast<f32x4*>(p.C + (size_t)m * p.ldc + n) = v;
                }
            }
            __builtin_amdgcn_s_waitcnt(0xC07F);              // reads done before the next slab overwrites
        }
        if (bad && p.flag) atomicOr(p.flag, 1);              // Inf / NaN: an operand left fp16's range (or came in bad)
        return;
    }
#pragma unroll
    for (int j = 0; j < NT; ++j) {
        const int n = n0 + wc * WN + j * 32 + fr;
        const bool n_ok = n < p.N;
        const float sc = ((n_ok && p.scale) ? p.scale[n] : 1.f) * ((n_ok && p.wscale) ? p.wscale[n] : 1.f);
        const float sh = (n_ok && p.shift) ? p.shift[n] : 0.f;
        const bool use_r = p.R && n < p.r_cols;
#pragma unroll
        for (int i = 0; i < MT; ++i) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int m = m0 + wr * WM + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * fh;
                if (n_ok && m < p.M) {
                    float v = acc[i][j][r] * sc + sh;
                    if (use_r) v += p.R[(size_t)(p.r_period > 0 ? m % p.r_period : m) * p.ldr + n];
                    bad |= !(fabsf(v) <= 3.4e38f);             // before the activation (see above)
                    v = p.relu == 2 ? 0.5f * v * (1.f + erff(v * 0.70710678118654752440f)) : fmaxf(v, relu_lo);
                    p.C[(size_t)m * p.ldc + n] = v;
                }
            }
        }
    }
    if (bad && p.flag) atomicOr(p.flag, 1);
}

// sums the split-K partials in split order (deterministic) and applies the epilogue
__device__ __forceinline__ void gom_tile_splitk_reduce(const GomTileArgs p, int splits) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)p.M * p.N) return;
    const int m = (int)(i / p.N), n = (int)(i % p.N);
    float v = 0.f;
    for (int s = 0; s < splits; ++s) v += p.partial[(size_t)s * p.M * p.N + i];
    v = v * ((p.scale ? p.scale[n] : 1.f) * (p.wscale ? p.wscale[n] : 1.f)) + (p.shift ? p.shift[n] : 0.f);
    if (p.R && n < p.r_cols) v += p.R[(size_t)(p.r_period > 0 ? m % p.r_period : m) * p.ldr + n];
    if (!(fabsf(v) <= 3.4e38f) && p.flag) atomicOr(p.flag, 1);   // before the activation: fmaxf(NaN, 0) = 0
    if (p.relu == 1) v = fmaxf(v, 0.f);
    if (p.relu == 2) v = 0.5f * v * (1.f + erff(v * 0.70710678118654752440f));
    p.C[(size_t)m * p.ldc + n] = v;
}

template <class P, int BM, int BN, int KH, int KW>
int gom_tile_launch(const GomTileArgs& a, hipStream_t s, int splits) {
    const long tiles = (long)cdiv(a.M, BM) * cdiv(a.N, BN);
    if (tiles <= 0) return GOM_OK;
    constexpr int lds_loop = P::PLANES * (BM + BN) * GOM_TILE_ROW_BYTES, lds_epi = 4 * 32 * (BN / 2 + 4) * 4;   // k-loop planes | epilogue slabs
    const int lds = lds_loop > lds_epi ? lds_loop : lds_epi;
    hipLaunchKernelGGL((P::template kernel<BM, BN, KH, KW>()), dim3((unsigned)tiles, (unsigned)splits), dim3(256), lds, s, a);
    if (a.partial)
        hipLaunchKernelGGL(P::reduce_kernel(), dim3((unsigned)cdiv((long)a.M * a.N, 256)), dim3(256), 0, s, a, splits);
    return gom_launch_status();
}

template <class P, int KH, int KW>
int gom_tile_dispatch(const GomTileArgs& a, hipStream_t s, int splits = 1) {
    if (a.N <= 64) return gom_tile_launch<P, 128, 64, KH, KW>(a, s, splits);
    return gom_tile_launch<P, 128, 128, KH, KW>(a, s, splits);
}

// Number of K slices for a problem with few output tiles and a long K (0 = do not split): e.g. input_proj[3], a 3x3 s2
// conv 2048 -> 256 on res5 (M = 3584 pixels, K = 18432): 56 tiles of 576 k-tiles each leave 200 of the 256 CUs idle.
// (The tile count is gom_tile_dispatch's; exported as gom_conv_bf16x6_splits for both back-ends.)
static inline int gom_tile_splits(int M, int N, int K) {
    const long tiles = (long)cdiv(M, 128) * cdiv(N, N <= 64 ? 64 : 128);
    const int nk = cdiv(K, GOM_TILE_BK);
    if (tiles <= 0 || tiles >= 128 || nk < 64) return 0;
    int s = (int)(512 / tiles);
    if (s > 16) s = 16;
    if (s > nk / 16) s = nk / 16;
    return s < 2 ? 0 : s;
}

// The plain GEMM entry of a back-end: `a` carries the operands and epilogue terms, this checks them and the shape
template <class P>
int gom_tile_gemm_entry(GomTileArgs a, void* stream) {
    GOM_CHECK_ARG(a.A && a.Wp && a.C && a.r_period >= 0);
    GOM_CHECK_ARG(a.M >= 0 && a.N > 0 && a.K > 0 && (a.K % 4) == 0);
    GOM_CHECK_ARG((a.lda % 4) == 0 && a.lda >= a.K && (a.ldw % 32) == 0 && a.ldw >= a.K && a.ldc >= a.N && (a.w_plane_stride % 8) == 0);
    GOM_CHECK_ARG(!a.R || (a.r_cols > 0 && a.r_cols <= a.N && a.ldr >= a.r_cols));
    GOM_CHECK_ARG(((uintptr_t)a.A % 16) == 0 && ((uintptr_t)a.Wp % 16) == 0 && ((uintptr_t)a.C % 16) == 0);
    GOM_CHECK_ARG((long)a.M * a.lda < (1L << 29) || a.a_rows);        // 32-bit byte offsets with a 2 GiB range check
    if (a.M == 0) return GOM_OK;
    if (!a.R) a.r_period = 0;
    return gom_tile_dispatch<P, 0, 0>(a, (hipStream_t)stream);
}

// The NHWC convolution entry of a back-end: `a` carries A = X, Wp, w_plane_stride, ldw, C = Y, wscale, flag, scale, shift, R
// and relu; this checks the geometry, fills the rest and launches (K sliced `splits` ways through `workspace` when splits > 1)
template <class P>
int gom_tile_conv_entry(GomTileArgs a, int B, int H, int Wd, int Cin, int Cout, int KH, int KW, int stride, int pad,
                        void* workspace, long workspace_bytes, int splits, void* stream) {
    GOM_CHECK_ARG(a.A && a.Wp && a.C);
    GOM_CHECK_ARG(B > 0 && H > 0 && Wd > 0 && Cin >= 4 && Cout > 0 && stride > 0 && pad >= 0);
    GOM_CHECK_ARG((Cin & (Cin - 1)) == 0);
    GOM_CHECK_ARG(KH == KW && (KH == 1 || KH == 3 || KH == 7));
    GOM_CHECK_ARG((long)B * H * Wd * Cin < (1L << 29));
    const int OH = (H + 2 * pad - KH) / stride + 1, OW = (Wd + 2 * pad - KW) / stride + 1;
    GOM_CHECK_ARG(OH > 0 && OW > 0);
    int lg = 0;
    while ((1 << lg) < Cin) ++lg;
    a.r_cols = Cout;
    a.M = B * OH * OW; a.N = Cout; a.K = KH * KW * Cin;
    a.lda = Cin; a.ldc = Cout; a.ldr = Cout;
    a.H = H; a.Wd = Wd; a.cin_log2 = lg; a.OH = OH; a.OW = OW; a.stride = stride; a.pad = pad;
    GOM_CHECK_ARG(a.ldw >= a.K && (a.ldw % 32) == 0 && (long)a.M * Cout < (1L << 31));
    hipStream_t s = (hipStream_t)stream;
    if (splits > 1) {
        GOM_CHECK_ARG(workspace && workspace_bytes >= (long)sizeof(float) * splits * a.M * a.N);
        a.partial = (float*)workspace;
        a.kt_per_split = cdiv(cdiv(a.K, GOM_TILE_BK), splits);
    } else {
        splits = 1;
    }
    if (KH == 1 && stride == 1 && pad == 0) {
        a.H = a.Wd = a.OH = a.OW = 0;
        return gom_tile_dispatch<P, 0, 0>(a, s, splits);
    }
    if (KH == 1) return gom_tile_dispatch<P, 1, 1>(a, s, splits);
    if (KH == 3) return gom_tile_dispatch<P, 3, 3>(a, s, splits);
    return gom_tile_dispatch<P, 7, 7>(a, s, splits);
}
