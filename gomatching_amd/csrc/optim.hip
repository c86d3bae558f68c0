// The optimizer step of training the association head: AdamW with full-model gradient clipping over a
// table of tensors, what `FullModelGradientClippingOptimizer(torch.optim.AdamW)` of the reference's costom_solver.py:55-73 does
// in fp32 (clip_grad_norm_ with max_norm = CLIP_VALUE, norm_type 2, then AdamW with one param group per tensor).
//
// The head has 12-33 M fp32 parameters in about forty tensors.  The step is memory-bound and needs the gradients once for the
// norm and one pass that reads g, p, m, v and writes p, m, v (36 bytes per parameter).  Three kinds of launches, no host
// synchronisation, no atomics:
//   (a) sumsq_kernel    one partial sum of g^2 per CHUNK (4096 elements) of every tensor, written to partials[chunk];
//   (b) coef_kernel     one workgroup adds the partials in fp64 in a fixed order and writes {total norm, clip coefficient};
//   (c) update_kernel   the AdamW update with g' = coef * g, one chunk at a time.
// The gradients are NOT modified: g' exists in registers only (the reference scales `p.grad` in place, but nothing reads it
// between the step and the next zero_grad()).
//
// Reproducibility.  A partial belongs to a chunk, not to a workgroup, and a chunk's sum is formed in an order that depends on
// the element's INDEX in its tensor only: thread t of 256 takes elements 4 (t + 256 j) .. + 3, j = 0..3, whether it fetched them
// with one 16-byte load (gradient 16-byte aligned) or with four 4-byte loads (a view that starts off the 16-byte grid), and
// adds their squares with 16 fused multiply-adds; 6 shuffle steps add the 64 lanes; lane 0 of wave 0 adds the 4 wave sums.  The
// longest chain of fp32 additions in the reduction is therefore 16 + 6 + 3 = 25; everything after it (the sum over chunks, the
// square root) is fp64.  Grid size, alignment and the number of launches the table is split into change no bit.
//
// The update pass is element-wise, so its mapping is by ADDRESS: a tensor whose four arrays share one offset from the 16-byte
// grid gets a scalar head (up to 3 elements), 16-byte loads and stores on the aligned body, and a scalar tail; a tensor whose
// arrays disagree (a misaligned view beside freshly allocated moments) takes 4-byte accesses throughout.  One function holds the
// arithmetic for both, with the contractions written out, so the two forms give the same bits.
//
// The table travels in the kernel arguments (48 tensors per launch, the multi-tensor-apply form): no device-side table to keep
// in step with the host's, nothing to upload, capture-safe.  A workgroup finds its chunk's tensor by a binary search over the
// slots' first-chunk numbers (wave-uniform loads from the argument segment).
#include <math.h>

#include "common.h"

namespace {

constexpr int CHUNK = 4096;          // elements per partial sum / per unit of work: 16 KB per array, 16 per thread
constexpr int SLOTS = 48;            // tensors per launch: 48 x 56 B + 16 B < the 4 KB argument segment
constexpr int MAX_GRID = 2048;       // 256 CUs x 8 workgroups; chunks beyond it are taken by a grid stride

struct Slot {
    float* p;
    const float* g;
    float* m;
    float* v;
    long n;
    int chunk0;                      // number of this tensor's first chunk in the flattened table
    float decay;                     // 1 - lr * weight_decay
    float step_size;                 // lr / (1 - beta1^t)
    float bc2_sqrt;                  // sqrt(1 - beta2^t)
};

struct Batch {
    Slot s[SLOTS];
    int n;                           // slots in use
    int chunk_lo, chunk_hi;          // this launch's chunks: [chunk_lo, chunk_hi)
};

__device__ __forceinline__ int find_slot(const Batch& b, int c) {
    int lo = 0, hi = b.n;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (b.s[mid].chunk0 <= c) lo = mid; else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(256) void sumsq_kernel(const Batch b, float* __restrict__ partials) {
    __shared__ float wave_part[4];
    const int tid = threadIdx.x;
    for (int c = b.chunk_lo + (int)blockIdx.x; c < b.chunk_hi; c += (int)gridDim.x) {
        const int si = find_slot(b, c);
        const float* __restrict__ g = b.s[si].g;
        const long n = b.s[si].n;
        const long lo = (long)(c - b.s[si].chunk0) * CHUNK;
        const bool aligned = ((uintptr_t)g & 15) == 0;
        float acc = 0.f;
#pragma unroll
        for (int j = 0; j < CHUNK / 1024; ++j) {
            const long e = lo + 4L * (tid + 256 * j);
            float x[4] = {0.f, 0.f, 0.f, 0.f};
            if (aligned && e + 3 < n) {
                const f32x4 q = *reinterpret_cast<const f32x4*>(g + e);
                x[0] = q[0]; x[1] = q[1]; x[2] = q[2]; x[3] = q[3];
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (e + k < n) x[k] = g[e + k];
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) acc = fmaf(x[k], x[k], acc);
        }
        acc = wave_sum(acc);
        if ((tid & 63) == 0) wave_part[tid >> 6] = acc;
        __syncthreads();
        if (tid == 0) partials[c] = ((wave_part[0] + wave_part[1]) + wave_part[2]) + wave_part[3];
        __syncthreads();
    }
}

// total = sqrt(sum of the partials), coef = min(1, clip / (total + 1e-6)) as clip_grad_norm_ forms it in fp32 (clip <= 0: no
// clipping, coef = 1).  Thread t adds partials t, t + 256, ... in fp64; a fixed tree adds the 256 sums.
__global__ __launch_bounds__(256) void coef_kernel(const float* __restrict__ partials, long n_partials, float clip,
                                                   float* __restrict__ norm_out) {
    __shared__ double part[256];
    const int tid = threadIdx.x;
    double a = 0.0;
    for (long i = tid; i < n_partials; i += 256) a += (double)partials[i];
    part[tid] = a;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (tid < w) part[tid] += part[tid + w];
        __syncthreads();
    }
    if (tid == 0) {
        const float total = (float)sqrt(part[0]);
        norm_out[0] = total;
        norm_out[1] = clip > 0.f ? fminf(1.f, clip / (total + 1e-6f)) : 1.f;
    }
}

struct Hyper {
    float coef, w1, beta2, w2, eps, decay, neg_step, bc2_sqrt;
};

// torch.optim.AdamW's fp32 arithmetic, one element:  g' = coef g;  p *= 1 - lr wd;  m = lerp(m, g', 1 - b1);
// v = b2 v + (1 - b2) g' g';  p -= step_size * m / (sqrt(v) / sqrt(1 - b2^t) + eps).  Division and square root are the
// correctly rounded ones.
__device__ __forceinline__ void adamw_element(const Hyper& h, float g, float& p, float& m, float& v) {
#pragma clang fp contract(off)                               // the only fused operations are the three written out
    const float gs = h.coef * g;
    m = fmaf(h.w1, gs - m, m);
    v = fmaf(h.w2 * gs, gs, h.beta2 * v);
    const float denom = sqrtf(v) / h.bc2_sqrt + h.eps;
    p = fmaf(h.neg_step, m / denom, p * h.decay);
}

__device__ __forceinline__ void adamw_scalar(const Hyper& h, const Slot& s, long i) {
    float p = s.p[i], m = s.m[i], v = s.v[i];
    adamw_element(h, s.g[i], p, m, v);
    s.p[i] = p;
    s.m[i] = m;
    s.v[i] = v;
}

__global__ __launch_bounds__(256) void update_kernel(const Batch b, const float* __restrict__ norm, float beta1_w, float beta2,
                                                     float beta2_w, float eps) {
    const int tid = threadIdx.x;
    const float coef = norm[1];
    for (int c = b.chunk_lo + (int)blockIdx.x; c < b.chunk_hi; c += (int)gridDim.x) {
        const int si = find_slot(b, c);
        const Slot s = b.s[si];
        const Hyper h = {coef, beta1_w, beta2, beta2_w, eps, s.decay, -s.step_size, s.bc2_sqrt};
        const long n = s.n;
        const int ci = c - s.chunk0;
        // elements from here to the 16-byte grid, if the four arrays agree on it
        const unsigned op = (unsigned)((uintptr_t)s.p >> 2) & 3u, og = (unsigned)((uintptr_t)s.g >> 2) & 3u;
        const unsigned om = (unsigned)((uintptr_t)s.m >> 2) & 3u, ov = (unsigned)((uintptr_t)s.v >> 2) & 3u;
        const bool vec = op == og && op == om && op == ov;
        if (!vec) {
            const long lo = (long)ci * CHUNK, hi = lo + CHUNK < n ? lo + CHUNK : n;
            for (long i = lo + tid; i < hi; i += 256) adamw_scalar(h, s, i);
            continue;
        }
        long head = (4 - op) & 3;
        head = head < n ? head : n;
        if (ci == 0 && tid < head) adamw_scalar(h, s, tid);
        // chunk ci of the body: [head + ci CHUNK, head + (ci + 1) CHUNK) cut at n; the tensor has ceil(n / CHUNK) chunks, which
        // covers the body's ceil((n - head) / CHUNK)
        const long lo = head + (long)ci * CHUNK;
        if (lo >= n) continue;
        const long hi = lo + CHUNK < n ? lo + CHUNK : n;
        const int nvec = (int)((hi - lo) >> 2);
        for (int q = tid; q < nvec; q += 256) {
            const long e = lo + 4L * q;
            const f32x4 g4 = *reinterpret_cast<const f32x4*>(s.g + e);
            f32x4 p4 = *reinterpret_cast<const f32x4*>(s.p + e);
            f32x4 m4 = *reinterpret_cast<const f32x4*>(s.m + e);
            f32x4 v4 = *reinterpret_cast<const f32x4*>(s.v + e);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                float p = p4[k], m = m4[k], v = v4[k];
                adamw_element(h, g4[k], p, m, v);
                p4[k] = p; m4[k] = m; v4[k] = v;
            }
            *reinterpret_cast<f32x4*>(s.p + e) = p4;
            *reinterpret_cast<f32x4*>(s.m + e) = m4;
            *reinterpret_cast<f32x4*>(s.v + e) = v4;
        }
        const long tail = lo + 4L * nvec;                      // < 4 elements, the tensor's last
        if (tail + tid < hi) adamw_scalar(h, s, tail + tid);
    }
}

inline long chunks_of(long n) { return (n + CHUNK - 1) / CHUNK; }

bool table_ok(const gom_optim_tensor* t, int n_tensors) {
    if (!t || n_tensors < 1) return false;
    for (int i = 0; i < n_tensors; ++i) {
        if (t[i].n < 0) return false;
        if (t[i].n > 0 && !(t[i].param && t[i].grad && t[i].exp_avg && t[i].exp_avg_sq)) return false;
        if (t[i].n > 0 && (((uintptr_t)t[i].param | (uintptr_t)t[i].grad | (uintptr_t)t[i].exp_avg | (uintptr_t)t[i].exp_avg_sq) & 3))
            return false;
        if (t[i].step < 1 || !(t[i].lr == t[i].lr) || !(t[i].weight_decay == t[i].weight_decay)) return false;
    }
    return true;
}

}  // namespace

extern "C" long gom_clipped_adamw_partials(const gom_optim_tensor* tensors, int n_tensors) {
    if (!table_ok(tensors, n_tensors)) return -1;
    long total = 0;
    for (int i = 0; i < n_tensors; ++i) {
        total += chunks_of(tensors[i].n);
        if (total > 0x7fffffffL) return -1;
    }
    return total;
}

extern "C" int gom_clipped_adamw_step(const gom_optim_tensor* tensors, int n_tensors, double beta1, double beta2, double eps,
                                      double clip_value, float* partials, long n_partials, float* norm_out, void* stream) {
    GOM_CHECK_ARG(table_ok(tensors, n_tensors));
    GOM_CHECK_ARG(beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0 && eps >= 0.0 && clip_value == clip_value);
    const long need = gom_clipped_adamw_partials(tensors, n_tensors);
    GOM_CHECK_ARG(need >= 0 && norm_out && n_partials >= need && (need == 0 || partials));
    hipStream_t s = (hipStream_t)stream;

    // the table in launches of up to SLOTS tensors; empty tensors take no slot
    const int n_batches_max = (n_tensors + SLOTS - 1) / SLOTS;
    Batch* batches = new Batch[n_batches_max];
    int nb = 0, chunk = 0;
    Batch* cur = nullptr;
    for (int i = 0; i < n_tensors; ++i) {
        const gom_optim_tensor& t = tensors[i];
        if (t.n == 0) continue;
        if (!cur || cur->n == SLOTS) {
            cur = &batches[nb++];
            cur->n = 0;
            cur->chunk_lo = chunk;
        }
        Slot& sl = cur->s[cur->n++];
        sl.p = t.param; sl.g = t.grad; sl.m = t.exp_avg; sl.v = t.exp_avg_sq;
        sl.n = t.n;
        sl.chunk0 = chunk;
        // the scalars as torch.optim.AdamW forms them: in double on the host, rounded to fp32 once
        sl.decay = (float)(1.0 - t.lr * t.weight_decay);
        sl.step_size = (float)(t.lr / (1.0 - pow(beta1, (double)t.step)));
        sl.bc2_sqrt = (float)sqrt(1.0 - pow(beta2, (double)t.step));
        chunk += (int)chunks_of(t.n);
        cur->chunk_hi = chunk;
    }
    int rc = GOM_OK;
    for (int k = 0; k < nb && rc == GOM_OK; ++k) {
        const int nc = batches[k].chunk_hi - batches[k].chunk_lo;
        hipLaunchKernelGGL(sumsq_kernel, dim3((unsigned)(nc < MAX_GRID ? nc : MAX_GRID)), dim3(256), 0, s, batches[k], partials);
        rc = gom_launch_status();
    }
    if (rc == GOM_OK) {
        hipLaunchKernelGGL(coef_kernel, dim3(1), dim3(256), 0, s, (const float*)partials, (long)chunk, (float)clip_value, norm_out);
        rc = gom_launch_status();
    }
    for (int k = 0; k < nb && rc == GOM_OK; ++k) {
        const int nc = batches[k].chunk_hi - batches[k].chunk_lo;
        hipLaunchKernelGGL(update_kernel, dim3((unsigned)(nc < MAX_GRID ? nc : MAX_GRID)), dim3(256), 0, s, batches[k],
                           (const float*)norm_out, (float)(1.0 - beta1), (float)beta2, (float)(1.0 - beta2), (float)eps);
        rc = gom_launch_status();
    }
    delete[] batches;
    return rc;
}
