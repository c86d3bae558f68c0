// fp32-accurate GEMM / implicit-GEMM convolution on the bf16 matrix cores ("bf16x6" split emulation).
//
//   C[M,N] = epilogue( A[M,K] . W[N,K]^T ),  fp32 in, fp32 out
//
// gfx950 has no TF32-class fast path and its fp32 MFMA runs at 1/16 of the bf16 rate
// (MI355X_MICROARCH.md "Matrix cores").  Each fp32 operand is therefore split into three bf16 planes
//   x = x0 + x1 + x2,  x0 = bf16(x), x1 = bf16(x - x0), x2 = bf16(x - x0 - x1)      (24 mantissa bits)
// and the product is rebuilt from the six plane products of weight <= 2,
//   a.b ~= a0b0 + (a0b1 + a1b0) + (a0b2 + a1b1 + a2b0),
// each an exact bf16 x bf16 product accumulated in fp32 by v_mfma_f32_32x32x16_bf16.  The dropped terms are
// <= 3 * 2^-24 |a||b| -- the size of one fp32 rounding -- so results match the exact-fp32 kernel
// (gemm_conv.hip) to accumulation-order noise; tests hold both to the same tolerances.  Six bf16 MFMAs
// per 32x32x16 block cost 192 cycles against 512 for eight v_mfma_f32_32x32x2_f32: 2.67x the fp32 matrix rate.
//
// Weights are split ONCE into [3][N][Kpad] bf16 planes (gom_split_bf16x3).  bf16 has fp32's exponent: no weight
// scale and no range flag (the entry points pass neither), any finite input is served.
// The kernel is the shared tile frame (gom_tile_gemm, common.h) with the policy below.
#include "common.h"

namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ unsigned int f2bf_bits(float x) {      // round-to-nearest-even
    return (unsigned int)__builtin_bit_cast(unsigned short, (__bf16)x);
}
__device__ __forceinline__ float bf_bits2f(unsigned int b) { return __uint_as_float(b << 16); }

// two floats -> packed bf16 pair (v_cvt_pk_bf16_f32) and the exact residuals
__device__ __forceinline__ unsigned int cvt_pk(float lo, float hi) {
    f32x2 v = {lo, hi};
    return __builtin_bit_cast(unsigned int, __builtin_convertvector(v, bf16x2));
}
__device__ __forceinline__ void split2(float x, float y, unsigned int& q0, unsigned int& q1, unsigned int& q2) {
    q0 = cvt_pk(x, y);
    const float rx = x - __uint_as_float(q0 << 16), ry = y - __uint_as_float(q0 & 0xFFFF0000u);
    q1 = cvt_pk(rx, ry);
    const float sx = rx - __uint_as_float(q1 << 16), sy = ry - __uint_as_float(q1 & 0xFFFF0000u);
    q2 = cvt_pk(sx, sy);
}

struct Bf16x6 {
    static constexpr int PLANES = 3;
    // two workgroups per CU (three planes -> 60 KB of LDS, 250 VGPRs): two k-tiles of A in flight, HBM latency > one MFMA phase
    static constexpr int OCC = 2;
    typedef bf16x8 frag;
    // split 4 floats into 3 planes of 4 bf16 (8 bytes each)
    static __device__ __forceinline__ void split4(const f32x4 v, u32x2 (&pl)[PLANES]) {
        unsigned int a0, a1, a2, b0, b1, b2;
        split2(v[0], v[1], a0, a1, a2);
        split2(v[2], v[3], b0, b1, b2);
        pl[0] = u32x2{a0, b0};
        pl[1] = u32x2{a1, b1};
        pl[2] = u32x2{a2, b2};
    }
    static __device__ __forceinline__ f32x16 mma(const frag (&a)[PLANES], const frag (&b)[PLANES], f32x16 c) {
        c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[2], b[0], c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[1], b[1], c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0], b[2], c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[1], b[0], c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0], b[1], c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0], b[0], c, 0, 0, 0);
        return c;
    }
    template <int BM, int BN, int KH, int KW> static auto kernel();      // the __global__ wrappers below
    static auto reduce_kernel();
};

template <int BM, int BN, int KH, int KW>
__global__ __launch_bounds__(256, Bf16x6::OCC) void gemm_bf16x6_kernel(const GomTileArgs p) {
    gom_tile_gemm<Bf16x6, BM, BN, KH, KW>(p);
}
__global__ __launch_bounds__(256) void splitk_reduce_kernel(const GomTileArgs p, int splits) { gom_tile_splitk_reduce(p, splits); }

template <int BM, int BN, int KH, int KW> auto Bf16x6::kernel() { return gemm_bf16x6_kernel<BM, BN, KH, KW>; }
auto Bf16x6::reduce_kernel() { return splitk_reduce_kernel; }

// fp32 [N, ldw_in] -> three bf16 planes [3][N][Kpad] (zero padded in K)
__global__ __launch_bounds__(256) void split_planes_kernel(const float* __restrict__ W, int ldw, int N, int K,
                                                           unsigned short* __restrict__ out, int Kpad) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)N * Kpad) return;
    const int n = (int)(i / Kpad), k = (int)(i % Kpad);
    const float x = k < K ? W[(size_t)n * ldw + k] : 0.f;
    const unsigned int b0 = f2bf_bits(x);
    const float r1 = x - bf_bits2f(b0);
    const unsigned int b1 = f2bf_bits(r1);
    const float r2 = r1 - bf_bits2f(b1);
    const unsigned int b2 = f2bf_bits(r2);
    const long plane = (long)N * Kpad;
    out[i] = (unsigned short)b0;
    out[plane + i] = (unsigned short)b1;
    out[2 * plane + i] = (unsigned short)b2;
}

}  // namespace

extern "C" int gom_split_bf16x3(const float* W, int ldw, int N, int K, void* planes_out, int Kpad, void* stream) {
    GOM_CHECK_ARG(W && planes_out && N > 0 && K > 0 && ldw >= K && Kpad >= K && (Kpad % 32) == 0);
    hipLaunchKernelGGL(split_planes_kernel, dim3((unsigned)cdiv((long)N * Kpad, 256)), dim3(256), 0,
                       (hipStream_t)stream, W, ldw, N, K, (unsigned short*)planes_out, Kpad);
    return gom_launch_status();
}

extern "C" int gom_gemm_f32_bf16x6(const float* A, const int* a_rows, int lda, const void* Wplanes,
                                   long w_plane_stride, int ldw, const float* scale, const float* shift,
                                   const float* R, int ldr, int r_cols, int relu, float* C, int ldc, int M, int N,
                                   int K, void* stream) {
    GomTileArgs a{};
    a.A = A; a.r_cols = r_cols; a.Wp = (const unsigned short*)Wplanes; a.w_plane_stride = w_plane_stride; a.C = C;
    a.scale = scale; a.shift = shift; a.R = R; a.a_rows = a_rows;
    a.M = M; a.N = N; a.K = K; a.lda = lda; a.ldw = ldw; a.ldc = ldc; a.ldr = ldr; a.relu = relu != 0;
    return gom_tile_gemm_entry<Bf16x6>(a, stream);
}

extern "C" int gom_conv_bf16x6_splits(int M, int N, int K) { return gom_tile_splits(M, N, K); }

extern "C" int gom_conv2d_nhwc_f32_bf16x6(const float* X, const void* Wplanes, long w_plane_stride, int ldw,
                                          const float* scale, const float* shift, const float* R, int relu, float* Y,
                                          int B, int H, int Wd, int Cin, int Cout, int KH, int KW, int stride, int pad,
                                          void* stream) {
    return gom_conv2d_nhwc_f32_bf16x6_splitk(X, Wplanes, w_plane_stride, ldw, scale, shift, R, relu, Y, B, H, Wd, Cin,
                                             Cout, KH, KW, stride, pad, nullptr, 0, 0, stream);
}

extern "C" int gom_conv2d_nhwc_f32_bf16x6_splitk(const float* X, const void* Wplanes, long w_plane_stride, int ldw,
                                                 const float* scale, const float* shift, const float* R, int relu,
                                                 float* Y, int B, int H, int Wd, int Cin, int Cout, int KH, int KW,
                                                 int stride, int pad, void* workspace, long workspace_bytes, int splits,
                                                 void* stream) {
    GomTileArgs a{};
    a.A = X; a.Wp = (const unsigned short*)Wplanes; a.w_plane_stride = w_plane_stride; a.ldw = ldw; a.C = Y;
    a.scale = scale; a.shift = shift; a.R = R; a.relu = relu != 0;
    return gom_tile_conv_entry<Bf16x6>(a, B, H, Wd, Cin, Cout, KH, KW, stride, pad, workspace, workspace_bytes, splits, stream);
}
