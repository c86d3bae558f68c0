// Tail of a ResNet bottleneck block fused with the head of the next one (f16x3 split, fp32-class accuracy):
//
//   X  = relu( bn3(conv3_1x1(A)) + R )            A [M, K1] = the block's conv2 output, R [M, 4 K1] = its input / shortcut
//   Y1 = relu( bn1'(conv1'_1x1(X)) )              the NEXT block's first convolution, MP output channels
//
// (Detectron2 BottleneckBlock, STRIDE_IN_1X1 = False, FrozenBN folded into scale / shift: gom_lstmatcher.py:42-61 builds it through
// build_resnet_backbone)  As two launches the pair moves A + R + X (write) and then X AGAIN (read) + Y1: at res2
// (K1 = 64, 890 000 pixels per 8 frames) 2.05 + 1.14 GB, the two launches together 0.6 ms -- both HBM streams.  Fused, the block's
// output X is written once for the next residual and never read back: 2.28 GB.
//
// Structure = the fused FFN kernel's (ffn_fused.hip) with the hidden activation also leaving the chip: a workgroup = 4 waves =
// 128 pixels, a wave's 32 pixels of A stay in registers as MFMA operand fragments; per chunk of 32 X-channels
//     H^T[32 x 32 px]  = W3c . A^T                      (A operand = weight fragment from LDS, B = the pixels' fragments)
//     v = H^T * scale + shift + R^T, relu  ->  stored to X (the lane is the pixel: four 16-byte pieces = its half of the 128-byte
//                                               line of the chunk; the other half-wave writes the other half)
//     Y1^T[MP x 32 px] += W1'[:, chunk] . v^T           (B operand = v straight from the accumulator registers after the fp16
//                                               split; the k order that implies is baked into the weight image)
// and the weights stream through a two-stage LDS ring by LDS-DMA from a fragment-linear image.  The channel counts are template
// parameters; the small ones leave room for several workgroups per CU, which is what hides the HBM latency of the R / X streams.
// Plane products in the tile kernel's order; range contract and *flag of gemm_f16x3.hip (A, and X as conv1's operand, within
// fp16's range; checked in front of the ReLU of Y1).
//
// Shortcut form (KS > 0: the FIRST block of a stage, whose residual is a 1x1 projection of the block's input): R is not read but
// computed here,
//     r = fl32( (Wsc . S^T) * scaleS + shiftS ),   X = relu( (acc3 * scale3 + shift3) + r )
// from the block's INPUT rows S [B, Hs, Ws, KS] at pixel (b, STRIDE y, STRIDE x): the wave keeps its 32 pixels of S as fragments
// beside A's, every chunk streams KS / 16 x 2 more weight fragments and runs 3 KS / 16 more MFMAs.  The [M, 4 K1] shortcut tensor
// -- written by one launch only to be read by this one -- never exists, and neither does the residual's way in through the
// transpose tile.  r is rounded on its own and then added: the two launches' arithmetic (the tile kernel's epilogue, then this one's).
#include "common.h"

namespace {

constexpr int CH = 32;                                   // X channels per chunk = one 128-byte line per pixel
constexpr int FRAG = 1024;
constexpr int BM = 128;
constexpr int XT_ROW = 36;                               // floats per pixel row of a wave's transpose tile (32 + 4: conflict-free b128)
// a wave's transpose tile holds XTR = 32 or 16 of its pixels x 32 channels; with 16 the pixels pass in two halves (half the LDS:
// one more workgroup per CU at the wider shapes; slower where the whole tile fits anyway -- 64 -> 256 -> 64: 422 vs 678 us)

struct BnArgs {
    const float* A;
    const unsigned char* img;
    const float* R;
    const float* sc1;                                        // [MP] folded scale (BN scale x 1 / weight row scale), shift of conv1'
    const float* sh1;
    float* X;
    float* Y1;
    int* flag;
    int lda, ldr, ldx, ldy, M, chunks;
    const float* S;                                          // shortcut form: the block's input, NHWC [B, Hs, Ws, >= KS] with pixel stride lds
    int lds, Hs, Ws, OH, OW;
};

template <int K1, int MP, int KS>
struct Cfg {
    static constexpr int W3_FRAGS = (K1 / 16) * 2;           // k-steps x planes
    static constexpr int W1_FRAGS = (MP / 32) * 2 * 2;       // output tiles x k-steps x planes
    static constexpr int WS_FRAGS = (KS / 16) * 2;           // shortcut form: k-steps x planes of Wsc, behind the aux fragment
    static constexpr int STAGE_FRAGS = W3_FRAGS + W1_FRAGS + 1 + WS_FRAGS;
    static constexpr int STAGE_BYTES = STAGE_FRAGS * FRAG;
    static constexpr int XTR = (K1 == 64 && MP == 64) ? 32 : 16;
    static constexpr int XT_BYTES = XTR * XT_ROW * 4;
    static constexpr int LDS_BYTES = 2 * STAGE_BYTES + 4 * XT_BYTES;
};

template <int K1, int MP, int OCC, int KS, int STRIDE>
__global__ __launch_bounds__(256, OCC) void bneck_kernel(const BnArgs p) {
    using C = Cfg<K1, MP, KS>;
    constexpr bool SC = KS > 0;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int fr = lane & 31, fh = lane >> 5;
    const long m = (long)blockIdx.x * BM + wave * 32 + fr;
    const long row = m < p.M ? m : p.M - 1;                  // tail pixels recompute (and re-store) the last one: same bits
    const unsigned lane16 = lane * 16;

    const __amdgpu_buffer_rsrc_t rs_img = gom_buffer_rsrc(p.img, p.chunks * C::STAGE_BYTES);
    auto dma_stage = [&](int c, int slot) {
        for (int f = wave; f < C::STAGE_FRAGS; f += 4)
            gom_dma_fragment(rs_img, lane16, (unsigned)c * C::STAGE_BYTES + f * FRAG, smem + slot * C::STAGE_BYTES + f * FRAG);
    };

    // ---- this wave's 32 pixels of A as B-operand fragments (whole K1), the first chunk's residual piece ----
    float amax = 0.f, chk = 0.f;                             // running |value| of everything split into fp16 planes; NaN / Inf
                                                             // detector (v * 0 accumulates to NaN): see dec_attn.hip
    half8 xf[2][K1 / 16];
    // R in and X out move as WHOLE 128-byte lines: lane l handles 16-byte piece (l & 7) of pixels (l >> 3) + 8 i of the wave's 32
    // (i = 0..3), i.e. a wave-instruction touches 8 lines -- the accumulator layout (lane = pixel, 16 bytes of its half of the
    // line) touches 32 lines of 32 bytes, and the texture-address unit pays per line (profiles/r03_msda_ta_counters.txt: ~3.6 cycles):
    // measured 538 -> see tools/bneck_bench.py.  The two layouts meet in a wave-private LDS tile (no barrier: one wave).
    long crow[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const long mm = (long)blockIdx.x * BM + wave * 32 + (lane >> 3) + 8 * i;
        crow[i] = mm < p.M ? mm : p.M - 1;
    }
    const int cpc = (lane & 7) * 4;
    float* xt = reinterpret_cast<float*>(smem + 2 * C::STAGE_BYTES + wave * C::XT_BYTES);
    constexpr int XTR = C::XTR, PASSES = 32 / XTR, RPP = XTR / 8;     // pixels per pass, passes, row-layout instructions per pass
    f32x4 rv[4];                                             // the chunk's residual piece in the coalesced layout
    half8 sf[2][SC ? KS / 16 : 1];                           // shortcut form: the pixels' rows of S, fragments like xf
    {
        const float* xr = p.A + (size_t)row * p.lda + fh * 8;
        f32x4 ra[K1 / 8];
#pragma unroll
        for (int s = 0; s < K1 / 16; ++s) {
            ra[2 * s] = *reinterpret_cast<const f32x4*>(xr + 16 * s);
            ra[2 * s + 1] = *reinterpret_cast<const f32x4*>(xr + 16 * s + 4);
        }
        f32x4 rs[SC ? KS / 8 : 1];
        if constexpr (SC) {
            long srow = row;                                 // 1x1, pad 0: output pixel (b, y, x) reads input pixel (b, STRIDE y, STRIDE x)
            if constexpr (STRIDE != 1) {
                const int ohw = p.OH * p.OW;
                const int b = (int)(row / ohw), rem = (int)(row - (long)b * ohw);
                const int y = rem / p.OW, x = rem - y * p.OW;
                srow = ((long)b * p.Hs + STRIDE * y) * p.Ws + STRIDE * x;
            }
            const float* sr = p.S + (size_t)srow * p.lds + fh * 8;
#pragma unroll
            for (int s = 0; s < KS / 16; ++s) {
                rs[2 * s] = *reinterpret_cast<const f32x4*>(sr + 16 * s);
                rs[2 * s + 1] = *reinterpret_cast<const f32x4*>(sr + 16 * s + 4);
            }
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) rv[i] = *reinterpret_cast<const f32x4*>(p.R + (size_t)crow[i] * p.ldr + cpc);
        }
        __builtin_amdgcn_sched_barrier(0);
        dma_stage(0, 0);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int s = 0; s < K1 / 16; ++s) {
#pragma unroll
            for (int e = 0; e < 4; ++e) amax = fmaxf(amax, fmaxf(fabsf(ra[2 * s][e]), fabsf(ra[2 * s + 1][e])));
            gom_split8_f16(ra[2 * s], ra[2 * s + 1], xf[0][s], xf[1][s]);
        }
        if constexpr (SC) {
#pragma unroll
            for (int s = 0; s < KS / 16; ++s) {
#pragma unroll
                for (int e = 0; e < 4; ++e) amax = fmaxf(amax, fmaxf(fabsf(rs[2 * s][e]), fabsf(rs[2 * s + 1][e])));
                gom_split8_f16(rs[2 * s], rs[2 * s + 1], sf[0][s], sf[1][s]);
            }
        }
        asm volatile("" : "+v"(amax));
    }

    f32x16 acc2[MP / 32];
#pragma unroll
    for (int t = 0; t < MP / 32; ++t)
#pragma unroll
        for (int g = 0; g < 16; ++g) acc2[t][g] = 0.f;

    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();

    for (int c = 0; c < p.chunks; ++c) {
        const int st = c & 1;
        const unsigned char* base = smem + st * C::STAGE_BYTES + lane16;
        const float* aux = reinterpret_cast<const float*>(smem + st * C::STAGE_BYTES + (C::W3_FRAGS + C::W1_FRAGS) * FRAG);
        // the next stage's fragments and the next chunk's residual piece are requested first (they are the OLDEST vector-memory
        // operations of the chunk: the counted wait at its end lets only this chunk's four X stores stay in flight)
        if (c + 1 < p.chunks) dma_stage(c + 1, st ^ 1);
        f32x4 rn[4];
        if constexpr (!SC) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                rn[q] = f32x4{0.f, 0.f, 0.f, 0.f};
                if (c + 1 < p.chunks) rn[q] = *reinterpret_cast<const f32x4*>(p.R + (size_t)crow[q] * p.ldr + CH * (c + 1) + cpc);
            }
        }
        // this chunk's residual piece: coalesced layout -> the wave's LDS tile -> accumulator layout, XTR pixels at a time
        f32x4 ra4[4];
#pragma unroll
        for (int hp = 0; hp < (SC ? 0 : PASSES); ++hp) {
#pragma unroll
            for (int i = 0; i < RPP; ++i) *reinterpret_cast<f32x4*>(xt + ((lane >> 3) + 8 * i) * XT_ROW + cpc) = rv[RPP * hp + i];
            // lanes exchange data through the tile: the wave barriers are CONVERGENT points the compiler may not move into the
            // divergent halves -- without them it threaded `if (A) read; write; if (!A) read` into `if (A) {read; write} else
            // {write; read}`, whose halves run one after the other: the second half's readers saw stale rows
            __builtin_amdgcn_wave_barrier();
            if (PASSES == 1 || (fr >> 4) == hp) {
#pragma unroll
                for (int q = 0; q < 4; ++q) ra4[q] = *reinterpret_cast<const f32x4*>(xt + (fr & (XTR - 1)) * XT_ROW + 8 * q + 4 * fh);
            }
            __builtin_amdgcn_wave_barrier();
        }
        // ---- H^T chunk = W3c . A^T ----
        f32x16 acc1;
#pragma unroll
        for (int g = 0; g < 16; ++g) acc1[g] = 0.f;
#pragma unroll
        for (int s = 0; s < K1 / 16; ++s) {
            const half8 w_hi = *reinterpret_cast<const half8*>(base + (2 * s) * FRAG);
            const half8 w_lo = *reinterpret_cast<const half8*>(base + (2 * s + 1) * FRAG);
            acc1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(w_hi, xf[1][s], acc1, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(w_lo, xf[0][s], acc1, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(w_hi, xf[0][s], acc1, 0, 0, 0);
        }
        // ---- shortcut form: R^T chunk = Wsc_c . S^T, the same plane order ----
        f32x16 accs;
        if constexpr (SC) {
#pragma unroll
            for (int g = 0; g < 16; ++g) accs[g] = 0.f;
#pragma unroll
            for (int s = 0; s < KS / 16; ++s) {
                const half8 w_hi = *reinterpret_cast<const half8*>(base + (C::W3_FRAGS + C::W1_FRAGS + 1 + 2 * s) * FRAG);
                const half8 w_lo = *reinterpret_cast<const half8*>(base + (C::W3_FRAGS + C::W1_FRAGS + 1 + 2 * s + 1) * FRAG);
                accs = __builtin_amdgcn_mfma_f32_32x32x16_f16(w_hi, sf[1][s], accs, 0, 0, 0);
                accs = __builtin_amdgcn_mfma_f32_32x32x16_f16(w_lo, sf[0][s], accs, 0, 0, 0);
                accs = __builtin_amdgcn_mfma_f32_32x32x16_f16(w_hi, sf[0][s], accs, 0, 0, 0);
            }
        }
        // ---- X chunk = relu(acc * scale + shift + R): stored, and split into the B fragments of the second product ----
        half8 hf[2][2];
        f32x4 vx[4];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            f32x4 v[2];
#pragma unroll
            for (int qq = 0; qq < 2; ++qq) {
                const int q = 2 * u + qq;
                const f32x4 sc = *reinterpret_cast<const f32x4*>(aux + 8 * q + 4 * fh);
                const f32x4 sh = *reinterpret_cast<const f32x4*>(aux + CH + 8 * q + 4 * fh);
                if constexpr (SC) {
                    // the shortcut launch's epilogue: its own fp32 value.  (A shortcut beyond fp32 makes t Inf or NaN: chk sees it.)
                    const f32x4 scs = *reinterpret_cast<const f32x4*>(aux + 2 * CH + 8 * q + 4 * fh);
                    const f32x4 shs = *reinterpret_cast<const f32x4*>(aux + 3 * CH + 8 * q + 4 * fh);
#pragma unroll
                    for (int e = 0; e < 4; ++e) ra4[q][e] = accs[4 * q + e] * scs[e] + shs[e];
                }
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    // the tile kernel's epilogue arithmetic: acc * scale + shift + residual, then the ReLU; the finiteness
                    // check sits in FRONT of the ReLU (fmaxf(NaN, 0) = 0 would hide an operand beyond fp16)
                    const float t = acc1[4 * q + e] * sc[e] + sh[e] + ra4[q][e];
                    chk = fmaf(t, 0.f, chk);
                    v[qq][e] = fmaxf(t, 0.f);
                    amax = fmaxf(amax, v[qq][e]);
                }
                vx[q] = v[qq];
            }
            gom_split8_f16(v[0], v[1], hf[0][u], hf[1][u]);
        }
        // the X chunk leaves as whole lines, XTR pixels at a time through the tile (tail pixels re-store the last pixel's bits: the
        // four stores are ALWAYS issued, the counted wait below relies on it)
#pragma unroll
        for (int hp = 0; hp < PASSES; ++hp) {
            if (PASSES == 1 || (fr >> 4) == hp) {
#pragma unroll
                for (int q = 0; q < 4; ++q) *reinterpret_cast<f32x4*>(xt + (fr & (XTR - 1)) * XT_ROW + 8 * q + 4 * fh) = vx[q];
            }
            __builtin_amdgcn_wave_barrier();
#pragma unroll
            for (int i = 0; i < RPP; ++i) {
                const f32x4 o = *reinterpret_cast<const f32x4*>(xt + ((lane >> 3) + 8 * i) * XT_ROW + cpc);
                *reinterpret_cast<f32x4*>(p.X + (size_t)crow[RPP * hp + i] * p.ldx + CH * c + cpc) = o;
            }
            __builtin_amdgcn_wave_barrier();
        }
        // ---- Y1^T += W1'[:, chunk] . X^T ----
#pragma unroll
        for (int t = 0; t < MP / 32; ++t)
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const half8 w_hi = *reinterpret_cast<const half8*>(base + (C::W3_FRAGS + (t * 2 + u) * 2) * FRAG);
                const half8 w_lo = *reinterpret_cast<const half8*>(base + (C::W3_FRAGS + (t * 2 + u) * 2 + 1) * FRAG);
                acc2[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(w_hi, hf[1][u], acc2[t], 0, 0, 0);
                acc2[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(w_lo, hf[0][u], acc2[t], 0, 0, 0);
                acc2[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(w_hi, hf[0][u], acc2[t], 0, 0, 0);
            }
        if constexpr (!SC) {
#pragma unroll
            for (int q = 0; q < 4; ++q) rv[q] = rn[q];
        }
        asm volatile("s_waitcnt vmcnt(4)" ::: "memory");     // everything but this chunk's four stores has landed
        __syncthreads();
    }

    // ---- Y1 = relu(acc2 * scale + shift): lane = pixel, registers = channels 32 t + 8 q + 4 fh .. + 3 ----
    float* yrow = p.Y1 + (size_t)row * p.ldy + 4 * fh;
#pragma unroll
    for (int t = 0; t < MP / 32; ++t)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int col = 32 * t + 8 * q + 4 * fh;
            const f32x4 sc = *reinterpret_cast<const f32x4*>(p.sc1 + col);
            const f32x4 sh = *reinterpret_cast<const f32x4*>(p.sh1 + col);
            f32x4 o;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float tv = acc2[t][4 * q + e] * sc[e] + sh[e];
                chk = fmaf(tv, 0.f, chk);                      // in front of the ReLU: NaN / Inf -> NaN
                o[e] = fmaxf(tv, 0.f);
            }
            *reinterpret_cast<f32x4*>(yrow + 32 * t + 8 * q) = o;
        }
    if ((!(amax <= 65504.f) || !(chk == 0.f)) && p.flag) atomicOr(p.flag, 1);
}

// Fragment-linear weight image, per chunk c of 32 X-channels; element j of lane l = (r, h):
//   f = 2 s + p                       (s < K1 / 16)          : plane p of W3s[32 c + r][16 s + 8 h + j]
//   f = W3_FRAGS + 4 t + 2 u + p      (t < MP / 32, u < 2)   : plane p of W1s[32 t + r][32 c + 16 u + 8 (j >> 2) + 4 h + (j & 3)]
//   f = W3_FRAGS + W1_FRAGS                                   : floats 0..31 = scale (BN scale x 1 / row scale of W3s), 32..63 = shift;
//                                                               shortcut form: 64..95 / 96..127 = the same of the shortcut
//   f = W3_FRAGS + W1_FRAGS + 1 + 2 s + p   (s < KS / 16)     : plane p of Wscs[32 c + r][16 s + 8 h + j]   (shortcut form)
struct ImgSc {                                               // the shortcut's operands (ks = 0: none)
    const unsigned short* p;
    long ps;
    int ld, ks;
    const float *inv, *scale, *shift;
};

__global__ __launch_bounds__(256) void bneck_image_kernel(const unsigned short* __restrict__ p3, long ps3, int ld3,
                                                          const float* __restrict__ inv3, const float* __restrict__ scale3,
                                                          const float* __restrict__ shift3, const unsigned short* __restrict__ p1,
                                                          long ps1, int ld1, int k1, int c4, int mp, const ImgSc sc,
                                                          unsigned short* __restrict__ img) {
    const int w3f = (k1 / 16) * 2, w1f = (mp / 32) * 4, sf = w3f + w1f + 1 + (sc.ks / 16) * 2;
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    const long total = (long)(c4 / CH) * sf * 512;
    if (i >= total) return;
    const int e = (int)(i % 512), f = (int)((i / 512) % sf), c = (int)(i / (512L * sf));
    const int l = e >> 3, j = e & 7, r = l & 31, h = l >> 5;
    if (f < w3f) {
        const int s = f >> 1, pl = f & 1;
        img[i] = p3[pl * ps3 + (size_t)(CH * c + r) * ld3 + 16 * s + 8 * h + j];
    } else if (f < w3f + w1f) {
        const int id = f - w3f, t = id >> 2, u = (id >> 1) & 1, pl = id & 1;
        img[i] = p1[pl * ps1 + (size_t)(32 * t + r) * ld1 + CH * c + 16 * u + 8 * (j >> 2) + 4 * h + (j & 3)];
    } else if (f == w3f + w1f) {
        const int fi = e >> 1;
        float v = 0.f;
        if (fi < CH) v = inv3[CH * c + fi] * (scale3 ? scale3[CH * c + fi] : 1.f);   // exact: the row scale is a power of two
        else if (fi < 2 * CH) v = shift3 ? shift3[CH * c + fi - CH] : 0.f;
        else if (sc.ks > 0 && fi < 3 * CH) v = sc.inv[CH * c + fi - 2 * CH] * (sc.scale ? sc.scale[CH * c + fi - 2 * CH] : 1.f);
        else if (sc.ks > 0 && fi < 4 * CH) v = sc.shift ? sc.shift[CH * c + fi - 3 * CH] : 0.f;
        const unsigned bits = __builtin_bit_cast(unsigned, v);
        img[i] = (unsigned short)((e & 1) ? (bits >> 16) : (bits & 0xffffu));
    } else {
        const int id = f - (w3f + w1f + 1), s = id >> 1, pl = id & 1;
        img[i] = sc.p[pl * sc.ps + (size_t)(CH * c + r) * sc.ld + 16 * s + 8 * h + j];
    }
}

template <int K1, int MP, int OCC, int KS = 0, int STRIDE = 1>
int launch(const BnArgs& a, hipStream_t s) {
    using C = Cfg<K1, MP, KS>;
    auto kern = bneck_kernel<K1, MP, OCC, KS, STRIDE>;
    if (C::LDS_BYTES > 65536) {
        hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, C::LDS_BYTES);
        if (e != hipSuccess) return GOM_ERR_HIP_BASE + (int)e;
    }
    hipLaunchKernelGGL(kern, dim3((unsigned)cdiv(a.M, BM)), dim3(256), C::LDS_BYTES, s, a);
    return gom_launch_status();
}

bool served(int k1, int c4, int mp) {
    if (c4 != 4 * k1) return false;
    // (256 -> 1024 -> 256, res4: measured on this kernel AND on the fused FFN kernel's pipeline with the extra residual / store --
    // 328 resp. 285 us against 285 us for the two launches at 56 448 pixels: 441 one-per-CU workgroups are 1.7 rounds.  Not served.)
    return (k1 == 64 && (mp == 64 || mp == 128)) || (k1 == 128 && (mp == 128 || mp == 256));
}

// shortcut form: res2.0 (64 -> 256 -> 64 with the 64 -> 256 projection of the stem's output, stride 1): 405-420 us against 290 + 410
// for the shortcut launch + the fused launch at 890 000 pixels.  More waves per CU on the same ring (one workgroup of 8 or 12 waves)
// measured 445 / 438 us: the launch is 72 % writes and sits at what they reach, 3.8-3.9 TB/s.
// (res3.0 = <128, 128, 1, 256, 2>, 139 KB of LDS, one workgroup per CU: measured 513 us against 535 for its two launches at 223 000
// pixels -- within what two runs of either differ by.  Not built; docs/LAB_NOTES.md.)
bool served_sc(int k1, int c4, int mp, int ks, int stride) {
    return k1 == 64 && c4 == 256 && mp == 64 && ks == 64 && stride == 1;
}

long image_bytes(int k1, int c4, int mp, int ks) {
    return (long)(c4 / CH) * ((k1 / 16) * 2 + (mp / 32) * 4 + 1 + (ks / 16) * 2) * FRAG;
}

int make_image(const void* w3_planes, long w3_plane_stride, int ld3, const float* w3_inv_scale, const float* scale3,
               const float* shift3, const void* w1_planes, long w1_plane_stride, int ld1, int k1, int c4, int mp, const ImgSc& sc,
               void* image, void* stream) {
    const long total = image_bytes(k1, c4, mp, sc.ks) / 2;
    hipLaunchKernelGGL(bneck_image_kernel, dim3((unsigned)cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream,
                       (const unsigned short*)w3_planes, w3_plane_stride, ld3, w3_inv_scale, scale3, shift3,
                       (const unsigned short*)w1_planes, w1_plane_stride, ld1, k1, c4, mp, sc, (unsigned short*)image);
    return gom_launch_status();
}

}  // namespace

extern "C" long gom_bneck_image_bytes(int k1, int c4, int mp) {
    if (!served(k1, c4, mp)) return -1;
    return image_bytes(k1, c4, mp, 0);
}

extern "C" int gom_bneck_image(const void* w3_planes, long w3_plane_stride, int ld3, const float* w3_inv_scale, const float* scale3,
                               const float* shift3, const void* w1_planes, long w1_plane_stride, int ld1, int k1, int c4, int mp,
                               void* image, long image_bytes, void* stream) {
    GOM_CHECK_ARG(w3_planes && w3_inv_scale && w1_planes && image && served(k1, c4, mp) && ld3 >= k1 && ld1 >= c4);
    GOM_CHECK_ARG(image_bytes >= gom_bneck_image_bytes(k1, c4, mp));
    return make_image(w3_planes, w3_plane_stride, ld3, w3_inv_scale, scale3, shift3, w1_planes, w1_plane_stride, ld1, k1, c4, mp,
                      ImgSc{}, image, stream);
}

extern "C" int gom_bneck_f32(const float* A, int lda, const void* image, const float* R, int ldr, const float* scale1,
                             const float* shift1, float* X, int ldx, float* Y1, int ldy, int M, int k1, int c4, int mp, int* flag,
                             void* stream) {
    GOM_CHECK_ARG(A && image && R && scale1 && shift1 && X && Y1 && M >= 0 && served(k1, c4, mp));
    GOM_CHECK_ARG(lda >= k1 && ldr >= c4 && ldx >= c4 && ldy >= mp && (lda % 4) == 0 && (ldr % 4) == 0 && (ldx % 4) == 0 && (ldy % 4) == 0);
    GOM_CHECK_ARG(((uintptr_t)A % 16) == 0 && ((uintptr_t)R % 16) == 0 && ((uintptr_t)X % 16) == 0 && ((uintptr_t)Y1 % 16) == 0 &&
                  ((uintptr_t)image % 16) == 0 && ((uintptr_t)scale1 % 16) == 0 && ((uintptr_t)shift1 % 16) == 0);
    if (M == 0) return GOM_OK;
    BnArgs a{};
    a.A = A; a.img = (const unsigned char*)image; a.R = R; a.sc1 = scale1; a.sh1 = shift1; a.X = X; a.Y1 = Y1; a.flag = flag;
    a.lda = lda; a.ldr = ldr; a.ldx = ldx; a.ldy = ldy; a.M = M; a.chunks = c4 / CH;
    hipStream_t s = (hipStream_t)stream;
    if (k1 == 64 && mp == 64) return launch<64, 64, 3>(a, s);
    if (k1 == 64 && mp == 128) return launch<64, 128, 2>(a, s);        // 59 KB of LDS: two workgroups per CU
    if (k1 == 128 && mp == 128) return launch<128, 128, 2>(a, s);
    return launch<128, 256, 1>(a, s);                        // 98 KB of ring: one workgroup per CU
}

// ---- shortcut form ----
extern "C" long gom_bneck_sc_image_bytes(int k1, int c4, int mp, int ks, int stride) {
    if (!served_sc(k1, c4, mp, ks, stride)) return -1;
    return image_bytes(k1, c4, mp, ks);
}

extern "C" int gom_bneck_sc_image(const void* w3_planes, long w3_plane_stride, int ld3, const float* w3_inv_scale, const float* scale3,
                                  const float* shift3, const void* w1_planes, long w1_plane_stride, int ld1,
                                  const void* ws_planes, long ws_plane_stride, int lds, const float* ws_inv_scale, const float* scale_s,
                                  const float* shift_s, int k1, int c4, int mp, int ks, int stride, void* image, long image_bytes,
                                  void* stream) {
    GOM_CHECK_ARG(w3_planes && w3_inv_scale && w1_planes && ws_planes && ws_inv_scale && image && served_sc(k1, c4, mp, ks, stride));
    GOM_CHECK_ARG(ld3 >= k1 && ld1 >= c4 && lds >= ks && image_bytes >= gom_bneck_sc_image_bytes(k1, c4, mp, ks, stride));
    const ImgSc sc{(const unsigned short*)ws_planes, ws_plane_stride, lds, ks, ws_inv_scale, scale_s, shift_s};
    return make_image(w3_planes, w3_plane_stride, ld3, w3_inv_scale, scale3, shift3, w1_planes, w1_plane_stride, ld1, k1, c4, mp, sc,
                      image, stream);
}

extern "C" int gom_bneck_sc_f32(const float* A, int lda, const void* image, const float* S, int lds, int B, int Hs, int Ws, int stride,
                                const float* scale1, const float* shift1, float* X, int ldx, float* Y1, int ldy, int k1, int c4, int mp,
                                int ks, int* flag, void* stream) {
    GOM_CHECK_ARG(A && image && S && scale1 && shift1 && X && Y1 && B >= 0 && Hs > 0 && Ws > 0 && served_sc(k1, c4, mp, ks, stride));
    GOM_CHECK_ARG(lda >= k1 && lds >= ks && ldx >= c4 && ldy >= mp && (lda % 4) == 0 && (lds % 4) == 0 && (ldx % 4) == 0 && (ldy % 4) == 0);
    GOM_CHECK_ARG(((uintptr_t)A % 16) == 0 && ((uintptr_t)S % 16) == 0 && ((uintptr_t)X % 16) == 0 && ((uintptr_t)Y1 % 16) == 0 &&
                  ((uintptr_t)image % 16) == 0 && ((uintptr_t)scale1 % 16) == 0 && ((uintptr_t)shift1 % 16) == 0);
    const int OH = (Hs - 1) / stride + 1, OW = (Ws - 1) / stride + 1;
    const long M = (long)B * OH * OW;
    GOM_CHECK_ARG(M <= 0x7fffffffL);
    if (M == 0) return GOM_OK;
    BnArgs a{};
    a.A = A; a.img = (const unsigned char*)image; a.S = S; a.sc1 = scale1; a.sh1 = shift1; a.X = X; a.Y1 = Y1; a.flag = flag;
    a.lda = lda; a.lds = lds; a.ldx = ldx; a.ldy = ldy; a.M = (int)M; a.chunks = c4 / CH;
    a.Hs = Hs; a.Ws = Ws; a.OH = OH; a.OW = OW;
    return launch<64, 64, 2, 64, 1>(a, (hipStream_t)stream);   // 68 KB of LDS (25 KB stages): two workgroups per CU
}
