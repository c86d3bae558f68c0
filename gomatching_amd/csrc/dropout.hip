// Training-mode dropout of the association head (MODEL.ASSO_HEAD.DROPOUT; roi_heads/transformer.py:191-207, 264-287 of the
// reference): y = [r +] mask * scale * x, the row softmax of `Attention` with dropout on its weights, that softmax's backward,
// and the ReLU backward behind the FFN's inner dropout.  torch's semantics (keep with probability 1 - p, kept values times
// 1 / (1 - p), the backward uses the forward's mask) on a mask stream of OUR OWN: torch's generator cannot be matched, so
// the mask comes from a counter-based generator -- nothing is stored, the backward regenerates it, a resumed run reproduces an
// uninterrupted one, ranks draw different masks.
//
// The stream ("Dropout"; restated on the host by tests/dropout_statement.py):
//   Philox4x32-10, key (seed & 0xffffffff, seed >> 32), counter (e >> 2, site, iteration, rank) for LOGICAL element e;
//   element e uses output word e & 3 and is kept iff word >= threshold = floor(p 2^32);  scale = float(1 / (1 - p)).
//   e = row * cols + col of the logical [rows, cols] tensor ([heads Lq, Lk] for attention weights): it does not depend on the
//   leading dimension, on padding columns or on the alignment of the pointers.
// One Philox call serves four consecutive elements.  Accesses are 16 bytes wide where every base and leading dimension is a
// multiple of 16 bytes (and rows are whole groups of four), 4 bytes wide otherwise; the arithmetic is written once, with explicit
// roundings (no contraction), so both forms give the same bits.  No atomics, no host synchronisation.  Bandwidth kernels on
// small tensors.
#include <cmath>

#include "common.h"

namespace {

struct Stream {
    unsigned k0, k1, site, iteration, rank, threshold;
    float scale;
};

__device__ __forceinline__ u32x4 philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const unsigned hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        const unsigned n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
        c0 = n0;
        c1 = lo1;
        c2 = n2;
        c3 = lo0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return u32x4{c0, c1, c2, c3};
}

// the four words of group g (elements 4 g .. 4 g + 3)
__device__ __forceinline__ u32x4 group_words(const Stream& s, long g) {
    return philox4x32_10((unsigned)g, s.site, s.iteration, s.rank, s.k0, s.k1);
}

// mask * scale * x [+ r] with the roundings spelled out: one multiplication, one addition
__device__ __forceinline__ float dropped(float x, unsigned word, const Stream& s) {
    return word >= s.threshold ? __fmul_rn(x, s.scale) : 0.f;
}

// y = [r +] mask * scale * x over a logical [rows, cols] tensor, one group of four elements per thread.
// VEC: cols % 4 == 0, every leading dimension % 4 == 0, every base 16-byte aligned (a group lies inside one row).
// FLAT: every leading dimension == cols (the view is one run of rows * cols elements: no division).
template <bool VEC, bool FLAT>
__global__ __launch_bounds__(256) void dropout_kernel(const float* x, long ldx, const float* r, long ldr, float* y, long ldy,
                                                      long cols, long total, long groups, Stream s) {
    const long g = (long)blockIdx.x * 256 + threadIdx.x;
    if (g >= groups) return;
    const u32x4 w = group_words(s, g);
    const long e = g * 4;
    if constexpr (VEC) {
        long ox = e, orr = e, oy = e;
        if constexpr (!FLAT) {
            const long row = e / cols, col = e - row * cols;
            ox = row * ldx + col;
            orr = row * ldr + col;
            oy = row * ldy + col;
        }
        const f32x4 xv = *reinterpret_cast<const f32x4*>(x + ox);
        f32x4 o;
#pragma unroll
        for (int i = 0; i < 4; ++i) o[i] = dropped(xv[i], w[i], s);
        if (r) {
            const f32x4 rv = *reinterpret_cast<const f32x4*>(r + orr);
#pragma unroll
            for (int i = 0; i < 4; ++i) o[i] = __fadd_rn(rv[i], o[i]);
        }
        *reinterpret_cast<f32x4*>(y + oy) = o;
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const long ei = e + i;
            if (ei >= total) break;
            long ox = ei, orr = ei, oy = ei;
            if constexpr (!FLAT) {
                const long row = ei / cols, col = ei - row * cols;
                ox = row * ldx + col;
                orr = row * ldr + col;
                oy = row * ldy + col;
            }
            float o = dropped(x[ox], w[i], s);
            if (r) o = __fadd_rn(r[orr], o);
            y[oy] = o;
        }
    }
}

// dx = y > 0 ? dy * scale : 0: the backward of ReLU seen through the dropout behind it -- the saved tensor is
// y = dropout(relu(.)), which is positive exactly where the unit was active AND kept, so no mask is regenerated
__global__ __launch_bounds__(256) void relu_backward_scaled_kernel(const float* __restrict__ dy, const float* __restrict__ y,
                                                                   float* __restrict__ dx, long n, float scale) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) dx[i] = y[i] > 0.f ? __fmul_rn(dy[i], scale) : 0.f;
}

constexpr int SOFTMAX_MAX_COLS = 8192;

// Row r of x [rows, ld]: P = softmax(scale_qk * x[r, :cols]) written over x (the arithmetic of softmax_rows_kernel, vitae.hip,
// statement for statement: the undropped P has that kernel's bits), and pd[r, :cols] = mask * scale * P.  One workgroup per
// row; P goes through LDS so that the dropout pass can hand each thread four CONSECUTIVE logical elements (one Philox call)
// whatever thread computed them.  Row r covers logical elements elem0 + r cols .. + cols - 1; a group of four that straddles
// two rows is generated by both.  Columns cols .. ld of pd are left as they are (the caller zeroes the padding once).
__global__ __launch_bounds__(256) void softmax_dropout_kernel(float* __restrict__ x, float* __restrict__ pd, int cols, long ld,
                                                              float scale_qk, long elem0, Stream s, int vec) {
    __shared__ float red[4];
    __shared__ __attribute__((aligned(16))) float prow[SOFTMAX_MAX_COLS];
    float* row = x + (long)blockIdx.x * ld;
    float v[32];
    float mx = -INFINITY;
#pragma unroll
    for (int k = 0; k < 32; ++k) {
        const int c = threadIdx.x + 256 * k;
        v[k] = c < cols ? row[c] * scale_qk : -INFINITY;
        mx = fmaxf(mx, v[k]);
    }
    mx = wave_max(mx);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = mx;
    __syncthreads();
    mx = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    __syncthreads();
    float sum = 0.f;
#pragma unroll
    for (int k = 0; k < 32; ++k) {
        v[k] = expf(v[k] - mx);                              // exp(-inf) = 0 beyond the row
        sum += v[k];
    }
    sum = wave_sum(sum);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = sum;
    __syncthreads();
    const float inv = 1.f / (red[0] + red[1] + red[2] + red[3]);
#pragma unroll
    for (int k = 0; k < 32; ++k) {
        const int c = threadIdx.x + 256 * k;
        if (c < cols) {
            const float p = v[k] * inv;
            row[c] = p;
            prow[c] = p;
        }
    }
    __syncthreads();
    const long e0 = elem0 + (long)blockIdx.x * cols, e1 = e0 + cols;
    const long g0 = e0 >> 2, g1 = (e1 - 1) >> 2;
    float* out = pd + (long)blockIdx.x * ld;
    for (long g = g0 + threadIdx.x; g <= g1; g += 256) {
        const u32x4 w = group_words(s, g);
        if (vec) {                                           // e0 % 4 == 0 and cols % 4 == 0: the group is columns c .. c + 3
            const int c = (int)(g - g0) * 4;
            const f32x4 p = *reinterpret_cast<const f32x4*>(prow + c);
            f32x4 o;
#pragma unroll
            for (int i = 0; i < 4; ++i) o[i] = dropped(p[i], w[i], s);
            *reinterpret_cast<f32x4*>(out + c) = o;
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const long e = g * 4 + i;
                if (e >= e0 && e < e1) out[e - e0] = dropped(prow[e - e0], w[i], s);
            }
        }
    }
}

// dS[r, j] = scale_qk * P[r, j] * (G[r, j] - sum_k G[r, k] P[r, k]) with G = mask * scale * dPd (the incoming gradient of the
// DROPPED weights; the mask is applied here).  One wave per row, a lane per group of four consecutive logical elements; the
// mask is generated in both passes (a row has up to 8192 columns: not kept in registers).
__global__ __launch_bounds__(256) void softmax_dropout_backward_kernel(const float* __restrict__ P, const float* __restrict__ dPd,
                                                                       float* __restrict__ dS, long rows, int cols, long ld,
                                                                       float scale_qk, long elem0, Stream s, int vec) {
    const long r = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;
    const int lane = threadIdx.x & 63;
    const float* p = P + r * ld;
    const float* gin = dPd + r * ld;
    float* out = dS + r * ld;
    const long e0 = elem0 + r * cols, e1 = e0 + cols;
    const long g0 = e0 >> 2, g1 = (e1 - 1) >> 2;
    // G = mask * scale * dPd is formed in double, where the product is exact, and so is the row's dot product: G - dot then
    // rounds once (a one-key row gives exactly 0, as in the kernel without dropout) and the mask costs no accuracy
    double dot = 0.0;
    for (int pass = 0; pass < 2; ++pass) {
        for (long g = g0 + lane; g <= g1; g += 64) {
            const u32x4 w = group_words(s, g);
            float pv[4], gv[4];
            bool ok[4];
            if (vec) {
                const int c = (int)(g - g0) * 4;
                const f32x4 a = *reinterpret_cast<const f32x4*>(p + c), b = *reinterpret_cast<const f32x4*>(gin + c);
#pragma unroll
                for (int i = 0; i < 4; ++i) pv[i] = a[i], gv[i] = b[i], ok[i] = true;
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const long e = g * 4 + i;
                    ok[i] = e >= e0 && e < e1;
                    pv[i] = ok[i] ? p[e - e0] : 0.f;
                    gv[i] = ok[i] ? gin[e - e0] : 0.f;
                }
            }
            double G[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) G[i] = w[i] >= s.threshold ? (double)gv[i] * (double)s.scale : 0.0;
            if (pass == 0) {
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (ok[i]) dot = fma(G[i], (double)pv[i], dot);
            } else {
                float o[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) o[i] = __fmul_rn(__fmul_rn(scale_qk, pv[i]), (float)(G[i] - dot));
                if (vec) {
                    *reinterpret_cast<f32x4*>(out + (int)(g - g0) * 4) = f32x4{o[0], o[1], o[2], o[3]};
                } else {
#pragma unroll
                    for (int i = 0; i < 4; ++i)
                        if (ok[i]) out[g * 4 + i - e0] = o[i];
                }
            }
        }
        if (pass == 0) {
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) dot += __shfl_xor(dot, o, 64);
        }
    }
}

// threshold = floor(p 2^32) and scale = float(1 / (1 - p)) of ONE p in [0, 1): anything else is refused before any HIP call
bool stream_of(unsigned long long seed, unsigned site, unsigned iteration, unsigned rank, long threshold, float scale, Stream& s) {
    if (threshold < 0 || threshold >= (1L << 32) || !(scale >= 1.f) || !std::isfinite(scale)) return false;
    const double p = (double)threshold / 4294967296.0;
    if (std::fabs((1.0 - 1.0 / (double)scale) - p) > 1e-6) return false;
    s = Stream{(unsigned)(seed & 0xffffffffull), (unsigned)(seed >> 32), site, iteration, rank, (unsigned)threshold, scale};
    return true;
}

bool aligned16(const void* p) { return ((uintptr_t)p % 16) == 0; }

}  // namespace

extern "C" int gom_dropout_f32(const float* x, long ldx, const float* r, long ldr, float* y, long ldy, long rows, long cols,
                               unsigned long long seed, unsigned site, unsigned iteration, unsigned rank, long threshold,
                               float scale, void* stream) {
    Stream s;
    GOM_CHECK_ARG(stream_of(seed, site, iteration, rank, threshold, scale, s));
    GOM_CHECK_ARG(rows >= 0 && cols >= 0 && ldx >= cols && ldy >= cols && (!r || ldr >= cols));
    if (rows == 0 || cols == 0) return GOM_OK;
    GOM_CHECK_ARG(x && y && rows <= (1L << 34) / cols);       // the counter's first word is e >> 2 < 2^32
    const long total = rows * cols, groups = (total + 3) / 4;
    const bool flat = rows == 1 || (ldx == cols && ldy == cols && (!r || ldr == cols));
    const bool vec = (flat || (cols % 4 == 0 && ldx % 4 == 0 && ldy % 4 == 0 && (!r || ldr % 4 == 0))) && total % 4 == 0 &&
                     aligned16(x) && aligned16(y) && aligned16(r);
    const dim3 grid((unsigned)cdiv(groups, 256)), block(256);
    hipStream_t st = (hipStream_t)stream;
    if (vec && flat)
        hipLaunchKernelGGL((dropout_kernel<true, true>), grid, block, 0, st, x, ldx, r, ldr, y, ldy, cols, total, groups, s);
    else if (vec)
        hipLaunchKernelGGL((dropout_kernel<true, false>), grid, block, 0, st, x, ldx, r, ldr, y, ldy, cols, total, groups, s);
    else if (flat)
        hipLaunchKernelGGL((dropout_kernel<false, true>), grid, block, 0, st, x, ldx, r, ldr, y, ldy, cols, total, groups, s);
    else
        hipLaunchKernelGGL((dropout_kernel<false, false>), grid, block, 0, st, x, ldx, r, ldr, y, ldy, cols, total, groups, s);
    return gom_launch_status();
}

extern "C" int gom_relu_backward_scaled_f32(const float* dy, const float* y, float* dx, long n, float scale, void* stream) {
    GOM_CHECK_ARG(n >= 0 && (n == 0 || (dy && y && dx)) && scale >= 1.f && std::isfinite(scale));
    if (n == 0) return GOM_OK;
    hipLaunchKernelGGL(relu_backward_scaled_kernel, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, dy, y, dx, n,
                       scale);
    return gom_launch_status();
}

extern "C" int gom_softmax_dropout_rows_f32(float* x, float* pd, long rows, int cols, long ld, float scale_qk, long elem0,
                                            unsigned long long seed, unsigned site, unsigned iteration, unsigned rank,
                                            long threshold, float scale, void* stream) {
    Stream s;
    GOM_CHECK_ARG(stream_of(seed, site, iteration, rank, threshold, scale, s));
    GOM_CHECK_ARG(x && pd && x != pd && rows >= 0 && cols > 0 && cols <= SOFTMAX_MAX_COLS && ld >= cols && rows < (1L << 31));
    GOM_CHECK_ARG(elem0 >= 0 && elem0 <= (1L << 34) - rows * cols);
    if (rows == 0) return GOM_OK;
    const int vec = elem0 % 4 == 0 && cols % 4 == 0 && ld % 4 == 0 && aligned16(pd);
    hipLaunchKernelGGL(softmax_dropout_kernel, dim3((unsigned)rows), dim3(256), 0, (hipStream_t)stream, x, pd, cols, ld, scale_qk,
                       elem0, s, vec);
    return gom_launch_status();
}

extern "C" int gom_softmax_dropout_rows_backward_f32(const float* P, const float* dPd, float* dS, long rows, int cols, long ld,
                                                     float scale_qk, long elem0, unsigned long long seed, unsigned site,
                                                     unsigned iteration, unsigned rank, long threshold, float scale,
                                                     void* stream) {
    Stream s;
    GOM_CHECK_ARG(stream_of(seed, site, iteration, rank, threshold, scale, s));
    GOM_CHECK_ARG(rows >= 0 && cols >= 0 && cols <= SOFTMAX_MAX_COLS && ld >= cols && rows < (1L << 31));
    GOM_CHECK_ARG(elem0 >= 0 && elem0 <= (1L << 34) - rows * (long)cols);
    if (rows == 0 || cols == 0) return GOM_OK;
    GOM_CHECK_ARG(P && dPd && dS);
    const int vec = elem0 % 4 == 0 && cols % 4 == 0 && ld % 4 == 0 && aligned16(P) && aligned16(dPd) && aligned16(dS);
    hipLaunchKernelGGL(softmax_dropout_backward_kernel, dim3((unsigned)cdiv(rows, 4)), dim3(256), 0, (hipStream_t)stream, P, dPd,
                       dS, rows, cols, ld, scale_qk, elem0, s, vec);
    return gom_launch_status();
}
