// fp32-class GEMM / implicit-GEMM convolution on the fp16 matrix cores ("f16x3" split emulation).
//
//   C[M,N] = epilogue( A[M,K] . W[N,K]^T ),  fp32 in, fp32 out
//
// Each fp32 operand is split into TWO fp16 planes,  x0 = fp16(x), x1 = fp16(x - x0)  (x - x0 is exact in fp32), i.e.
// 22 significand bits, and the product is rebuilt from three plane products
//   a.b ~= a0b0 + a0b1 + a1b0            (the dropped a1b1 is <= 2^-22 |a||b|)
// accumulated in fp32 by v_mfma_f32_32x32x16_f16: HALF the MFMA passes, 2/3 of the LDS traffic and half the split
// VALU of the bf16x6 kernel (gemm_bf16x6.hip), for a relative error of ~3 * 2^-22 = 7e-7 per product against ~2e-7
// there -- both far inside what an fp32 GEMM's own accumulation order moves a K >= 64 dot product by (sqrt(K) * 2^-24).
// fp16 has a 5-bit exponent, which the split has to respect:
//   * weights are constants: each row is scaled by an exact power of two into fp16's upper normal range before the
//     split (gom_split_f16x2; the inverse scale is applied in the epilogue through `wscale`), so both planes are
//     normal numbers and the 2^-22 bound holds whatever the weight magnitude;
//   * activations are split as they are: magnitudes up to 65504 are representable; below ~0.25 the second plane
//     becomes subnormal and the element keeps an ABSOLUTE accuracy of 2^-25 = 3e-8 (fp32's spacing at 0.5) instead
//     of a relative one.  An activation beyond fp16's range would become Inf: every tile checks its results and raises
//     a device flag (`flag`), which the host turns into an error at the step's sync point -- never a silent wrong
//     result.  Badly scaled data (the 12-decade rows of tests/test_ops_gpu.py) belongs on the bf16x6 kernel.
// The kernel is the shared tile frame (gom_tile_gemm, common.h) with the policy below.
#include "common.h"

namespace {

struct F16x3 {
    static constexpr int PLANES = 2;
    // three workgroups per CU (40 KB LDS, <= 168 VGPRs, one k-tile of A in flight) measured 9 % faster end to end than
    // two with a two-deep A prefetch (251 VGPRs): 224-299 vs 187-265 TFLOP/s on the encoder shapes
    static constexpr int OCC = 3;
    typedef half8 frag;
    static __device__ __forceinline__ void split4(const f32x4 v, u32x2 (&pl)[PLANES]) { gom_split4_f16(v, pl[0], pl[1]); }
    static __device__ __forceinline__ f32x16 mma(const frag (&a)[PLANES], const frag (&b)[PLANES], f32x16 c) {
        c = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[1], b[0], c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[0], b[1], c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[0], b[0], c, 0, 0, 0);
        return c;
    }
    template <int BM, int BN, int KH, int KW> static auto kernel();      // the __global__ wrappers below
    static auto reduce_kernel();
};

template <int BM, int BN, int KH, int KW, int OCC>
__global__ __launch_bounds__(256, OCC) void gemm_f16x3_kernel(const GomTileArgs p) {
    static_assert(OCC == F16x3::OCC, "the frame takes its pipeline form from the policy");
    gom_tile_gemm<F16x3, BM, BN, KH, KW>(p);
}
__global__ __launch_bounds__(256) void splitk_reduce_kernel(const GomTileArgs p, int splits) { gom_tile_splitk_reduce(p, splits); }

template <int BM, int BN, int KH, int KW> auto F16x3::kernel() { return gemm_f16x3_kernel<BM, BN, KH, KW, OCC>; }
auto F16x3::reduce_kernel() { return splitk_reduce_kernel; }

// fp32 [N, ldw_in] -> two fp16 planes [2][N][Kpad] (zero padded in K) of the row scaled by 2^e_n, e_n chosen so that the
// row's largest magnitude lands in [2^13, 2^14); inv_scale[n] = 2^-e_n.  One workgroup per row.
__global__ __launch_bounds__(256) void split_rows_f16_kernel(const float* __restrict__ W, int ldw, int N, int K,
                                                             unsigned short* __restrict__ out, int Kpad,
                                                             float* __restrict__ inv_scale) {
    __shared__ float red[4];
    const int n = blockIdx.x;
    const float* row = W + (size_t)n * ldw;
    float mx = 0.f;
    for (int k = threadIdx.x; k < K; k += 256) mx = fmaxf(mx, fabsf(row[k]));
    mx = wave_max(mx);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = mx;
    __syncthreads();
    mx = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    int e = 0;
    if (mx > 0.f && mx <= 3.4e38f) {
        int ex;
        frexpf(mx, &ex);                                     // mx = f * 2^ex, f in [0.5, 1)
        e = 14 - ex;                                         // mx * 2^e in [2^13, 2^14)
        e = e > 100 ? 100 : (e < -100 ? -100 : e);
    }
    const float sc = ldexpf(1.f, e);
    if (threadIdx.x == 0) inv_scale[n] = ldexpf(1.f, -e);
    const long plane = (long)N * Kpad;
    for (int k = threadIdx.x; k < Kpad; k += 256) {
        const float x = k < K ? row[k] * sc : 0.f;           // exact: power-of-two scaling
        const _Float16 h0 = (_Float16)x;
        const _Float16 h1 = (_Float16)(x - (float)h0);
        out[(size_t)n * Kpad + k] = __builtin_bit_cast(unsigned short, h0);
        out[plane + (size_t)n * Kpad + k] = __builtin_bit_cast(unsigned short, h1);
    }
}

}  // namespace

extern "C" int gom_split_f16x2(const float* W, int ldw, int N, int K, void* planes_out, int Kpad, float* inv_scale,
                               void* stream) {
    GOM_CHECK_ARG(W && planes_out && inv_scale && N > 0 && K > 0 && ldw >= K && Kpad >= K && (Kpad % 32) == 0);
    hipLaunchKernelGGL(split_rows_f16_kernel, dim3((unsigned)N), dim3(256), 0, (hipStream_t)stream, W, ldw, N, K,
                       (unsigned short*)planes_out, Kpad, inv_scale);
    return gom_launch_status();
}

extern "C" int gom_gemm_f32_f16x3(const float* A, const int* a_rows, int lda, const void* Wplanes, long w_plane_stride,
                                  int ldw, const float* wscale, const float* scale, const float* shift, const float* R,
                                  int ldr, int r_cols, int relu, float* C, int ldc, int M, int N, int K, int* flag,
                                  void* stream) {
    return gom_gemm_f32_f16x3_rp(A, a_rows, lda, Wplanes, w_plane_stride, ldw, wscale, scale, shift, R, ldr, r_cols, 0, relu, C,
                                 ldc, M, N, K, flag, stream);
}

extern "C" int gom_gemm_f32_f16x3_rp(const float* A, const int* a_rows, int lda, const void* Wplanes, long w_plane_stride,
                                     int ldw, const float* wscale, const float* scale, const float* shift, const float* R,
                                     int ldr, int r_cols, int r_period, int relu, float* C, int ldc, int M, int N, int K,
                                     int* flag, void* stream) {
    GomTileArgs a{};
    a.A = A; a.r_cols = r_cols; a.r_period = r_period; a.Wp = (const unsigned short*)Wplanes; a.w_plane_stride = w_plane_stride; a.C = C;
    a.wscale = wscale; a.flag = flag;
    a.scale = scale; a.shift = shift; a.R = R; a.a_rows = a_rows;
    a.M = M; a.N = N; a.K = K; a.lda = lda; a.ldw = ldw; a.ldc = ldc; a.ldr = ldr; a.relu = relu;
    return gom_tile_gemm_entry<F16x3>(a, stream);
}

extern "C" int gom_conv2d_nhwc_f32_f16x3(const float* X, const void* Wplanes, long w_plane_stride, int ldw,
                                         const float* wscale, const float* scale, const float* shift, const float* R,
                                         int relu, float* Y, int B, int H, int Wd, int Cin, int Cout, int KH, int KW,
                                         int stride, int pad, void* workspace, long workspace_bytes, int splits,
                                         int* flag, void* stream) {
    GomTileArgs a{};
    a.A = X; a.Wp = (const unsigned short*)Wplanes; a.w_plane_stride = w_plane_stride; a.ldw = ldw; a.C = Y;
    a.wscale = wscale; a.flag = flag;
    a.scale = scale; a.shift = shift; a.R = R; a.relu = relu;
    return gom_tile_conv_entry<F16x3>(a, B, H, Wd, Cin, Cout, KH, KW, stride, pad, workspace, workspace_bytes, splits, stream);
}
