// Frame ingest: what the reference does on the host between cv2.imread and the model --
// BGR->RGB flip, Detectron2 ResizeShortestEdge = Pillow `Image.resize(..., BILINEAR)` on uint8, astype(float32),
// HWC->CHW (text_track_visualizer.py:315-324) -- followed by the model's own (x - mean) / std
// (gom_lstmatcher.py:159-170), as ONE kernel over uint8 frames resident in HBM.
//
// Pillow's resize is a separable fixed-point convolution (third-party, absent from /root/reference: Pillow
// src/libImaging/Resample.c, restated from its published algorithm and pinned against the installed Pillow
// in tests/): per axis, coefficient rows are built in double, normalised, rounded to 22-bit fixed point;
// the horizontal pass accumulates int32 from 1<<21, shifts by 22 and clamps to uint8; the vertical pass
// repeats that on the uint8 intermediate.  The kernel recomputes the (<= ksize_y) horizontally-filtered
// uint8 values of one output pixel in registers instead of materialising the intermediate image: the source
// frame (2.8 MB at 1280x720) is L2-resident, the 28 MB fp32 NHWC4 output write is the HBM traffic.
#include <math.h>

#include "common.h"

#define GOM_RESAMPLE_BITS 22   // Pillow: PRECISION_BITS = 32 - 8 - 2

// ---------------------------------------------------------------------------------------------- host
extern "C" int gom_resample_ksize_bilinear(int in_size, int out_size) {
    if (in_size <= 0 || out_size <= 0) return -1;
    double filterscale = (double)((float)in_size - 0.0f) / out_size;
    if (filterscale < 1.0) filterscale = 1.0;
    const double support = 1.0 * filterscale;
    return (int)ceil(support) * 2 + 1;
}

extern "C" int gom_resample_coeffs_bilinear(int in_size, int out_size, int* bounds, int* kk, int ksize) {
    GOM_CHECK_ARG(bounds && kk && in_size > 0 && out_size > 0);
    GOM_CHECK_ARG(ksize == gom_resample_ksize_bilinear(in_size, out_size));
    const float in0 = 0.0f, in1 = (float)in_size;
    double filterscale, scale;
    filterscale = scale = (double)(in1 - in0) / out_size;
    if (filterscale < 1.0) filterscale = 1.0;
    const double support = 1.0 * filterscale;
    double* k = new double[ksize];
    for (int xx = 0; xx < out_size; ++xx) {
        const double center = in0 + (xx + 0.5) * scale;
        double ww = 0.0;
        const double ss = 1.0 / filterscale;
        int xmin = (int)(center - support + 0.5);
        if (xmin < 0) xmin = 0;
        int xmax = (int)(center + support + 0.5);
        if (xmax > in_size) xmax = in_size;
        xmax -= xmin;
        int x;
        for (x = 0; x < xmax; ++x) {
            double t = (x + xmin - center + 0.5) * ss;
            if (t < 0.0) t = -t;
            const double w = t < 1.0 ? 1.0 - t : 0.0;
            k[x] = w;
            ww += w;
        }
        for (x = 0; x < xmax; ++x)
            if (ww != 0.0) k[x] /= ww;
        for (; x < ksize; ++x) k[x] = 0;
        for (x = 0; x < ksize; ++x)
            kk[(long)xx * ksize + x] = k[x] < 0 ? (int)(-0.5 + k[x] * (1 << GOM_RESAMPLE_BITS))
                                                : (int)(0.5 + k[x] * (1 << GOM_RESAMPLE_BITS));
        bounds[xx * 2 + 0] = xmin;
        bounds[xx * 2 + 1] = xmax;
    }
    delete[] k;
    return GOM_OK;
}

// -------------------------------------------------------------------------------------------- device
namespace {

__device__ __forceinline__ int clip8(int v) {
    v >>= GOM_RESAMPLE_BITS;
    return v < 0 ? 0 : (v > 255 ? 255 : v);
}

// The three 8-bit channels of pixel (ry, rx) of the resized image the tables describe: Pillow's horizontal pass on the
// (<= yks) source rows of the vertical pass, in registers.  Every resample kernel of this file calls it, so they agree bit
// for bit.
__device__ __forceinline__ void resample_pixel(const uint8_t* __restrict__ frame, int W, const int* __restrict__ xb,
                                               const int* __restrict__ xk, int xks, const int* __restrict__ yb,
                                               const int* __restrict__ yk, int yks, int ry, int rx, int& c0, int& c1,
                                               int& c2) {
    const int xmin = xb[2 * rx], xn = xb[2 * rx + 1];
    const int ymin = yb[2 * ry], yn = yb[2 * ry + 1];
    const int* kx = xk + (long)rx * xks;
    const int* ky = yk + (long)ry * yks;
    const int half = 1 << (GOM_RESAMPLE_BITS - 1);
    int v0 = half, v1 = half, v2 = half;
    for (int r = 0; r < yn; ++r) {
        const uint8_t* row = frame + ((long)(ymin + r) * W + xmin) * 3;
        int h0 = half, h1 = half, h2 = half;
        for (int x = 0; x < xn; ++x) {
            const int k = kx[x];
            h0 += (int)row[3 * x + 0] * k;
            h1 += (int)row[3 * x + 1] * k;
            h2 += (int)row[3 * x + 2] * k;
        }
        const int k = ky[r];
        v0 += clip8(h0) * k;
        v1 += clip8(h1) * k;
        v2 += clip8(h2) * k;
    }
    c0 = clip8(v0);
    c1 = clip8(v1);
    c2 = clip8(v2);
}

// One thread per output pixel (3 channels).  F32OUT: write (v[perm] - mean) / std as NHWC4; else uint8 HWC.
// The OH x OW output is the window at (y0, x0) of the resized image the tables describe (the whole of it for
// x0 = y0 = 0): pixel (oy, ox) reads table rows oy + y0 and ox + x0, nothing outside the window is computed.
template <bool F32OUT>
__global__ __launch_bounds__(256) void resample_kernel(const uint8_t* __restrict__ src, int H, int W,
                                                       const int* __restrict__ xb, const int* __restrict__ xk, int xks,
                                                       const int* __restrict__ yb, const int* __restrict__ yk, int yks,
                                                       void* __restrict__ dst, int OH, int OW, int y0, int x0, long total,
                                                       int flip, float m0, float m1, float m2, float s0, float s1, float s2) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int ox = (int)(i % OW);
    const long t = i / OW;
    const int oy = (int)(t % OH);
    const long b = t / OH;
    int c0, c1, c2;
    resample_pixel(src + b * (long)H * W * 3, W, xb, xk, xks, yb, yk, yks, oy + y0, ox + x0, c0, c1, c2);
    if (flip) {
        const int tmp = c0;
        c0 = c2;
        c2 = tmp;
    }
    if (F32OUT) {
        f32x4 o;
        o[0] = ((float)c0 - m0) / s0;
        o[1] = ((float)c1 - m1) / s1;
        o[2] = ((float)c2 - m2) / s2;
        o[3] = 0.f;
        *reinterpret_cast<f32x4*>(reinterpret_cast<float*>(dst) + i * 4) = o;
    } else {
        uint8_t* o = reinterpret_cast<uint8_t*>(dst) + i * 3;
        o[0] = (uint8_t)c0;
        o[1] = (uint8_t)c1;
        o[2] = (uint8_t)c2;
    }
}

// A motion clip: T windows of T resizes of ONE source image, padded to PH x PW.  The frame is blockIdx.y, so its descriptor
// -- passed by value, read from the kernel arguments -- is wave-uniform and costs scalar loads only; table offsets are in
// int32 words from `tab`.  One thread per pixel of the PADDED frame: inside the window the arithmetic of `resample_kernel`,
// outside it zeros (the padding is written here: dst needs no memset).
struct MotionFrame {
    int y0, x0, OH, OW, xks, yks, xb, xk, yb, yk;
};
struct MotionFrames {
    MotionFrame f[GOM_INGEST_MOTION_MAX_FRAMES];
};

__global__ __launch_bounds__(256) void motion_kernel(const uint8_t* __restrict__ src, int W, const int* __restrict__ tab,
                                                     MotionFrames frames, float* __restrict__ dst, int PH, int PW, int flip,
                                                     float m0, float m1, float m2, float s0, float s1, float s2) {
    const int i = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (i >= PH * PW) return;
    const MotionFrame f = frames.f[blockIdx.y];
    const int ox = i % PW, oy = i / PW;
    f32x4 o = {0.f, 0.f, 0.f, 0.f};
    if (ox < f.OW && oy < f.OH) {
        int c0, c1, c2;
        resample_pixel(src, W, tab + f.xb, tab + f.xk, f.xks, tab + f.yb, tab + f.yk, f.yks, oy + f.y0, ox + f.x0, c0, c1, c2);
        if (flip) {
            const int tmp = c0;
            c0 = c2;
            c2 = tmp;
        }
        o[0] = ((float)c0 - m0) / s0;
        o[1] = ((float)c1 - m1) / s1;
        o[2] = ((float)c2 - m2) / s2;
    }
    *reinterpret_cast<f32x4*>(dst + ((long)blockIdx.y * PH * PW + i) * 4) = o;
}

}  // namespace

#define GOM_RESAMPLE_ARGS_OK                                                                                       \
    (src && xbounds && xkk && ybounds && ykk && dst && B > 0 && H > 0 && W > 0 && OH > 0 && OW > 0 && xksize > 0 && \
     yksize > 0)

extern "C" int gom_resize_bilinear_u8_hwc3(const uint8_t* src, int B, int H, int W, const int* xbounds, const int* xkk,
                                           int xksize, const int* ybounds, const int* ykk, int yksize, uint8_t* dst,
                                           int OH, int OW, int flip_channels, void* stream) {
    GOM_CHECK_ARG(GOM_RESAMPLE_ARGS_OK);
    const long total = (long)B * OH * OW;
    hipLaunchKernelGGL(resample_kernel<false>, dim3((unsigned)cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream, src,
                       H, W, xbounds, xkk, xksize, ybounds, ykk, yksize, (void*)dst, OH, OW, 0, 0, total, flip_channels, 0.f,
                       0.f, 0.f, 1.f, 1.f, 1.f);
    return gom_launch_status();
}

extern "C" int gom_ingest_u8_hwc3_to_nhwc4(const uint8_t* src, int B, int H, int W, const int* xbounds, const int* xkk,
                                           int xksize, const int* ybounds, const int* ykk, int yksize,
                                           const float* mean3, const float* std3, float* dst, int OH, int OW,
                                           int flip_channels, void* stream) {
    GOM_CHECK_ARG(GOM_RESAMPLE_ARGS_OK && mean3 && std3);
    const long total = (long)B * OH * OW;
    hipLaunchKernelGGL(resample_kernel<true>, dim3((unsigned)cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream, src,
                       H, W, xbounds, xkk, xksize, ybounds, ykk, yksize, (void*)dst, OH, OW, 0, 0, total, flip_channels,
                       mean3[0], mean3[1], mean3[2], std3[0], std3[1], std3[2]);
    return gom_launch_status();
}

// Resize to SH x SW, then keep the OH x OW window at (y0, x0): EfficientDetResizeCropTransform.apply_image
// (custom_transform.py:46-59) without the SH x SW intermediate.  Tables are those of H -> SH and W -> SW.
#define GOM_RESAMPLE_WINDOW_OK \
    (SH > 0 && SW > 0 && y0 >= 0 && x0 >= 0 && OH <= SH - y0 && OW <= SW - x0)

extern "C" int gom_resize_crop_bilinear_u8_hwc3(const uint8_t* src, int B, int H, int W, const int* xbounds,
                                                const int* xkk, int xksize, const int* ybounds, const int* ykk,
                                                int yksize, uint8_t* dst, int SH, int SW, int y0, int x0, int OH, int OW,
                                                int flip_channels, void* stream) {
    GOM_CHECK_ARG(GOM_RESAMPLE_ARGS_OK && GOM_RESAMPLE_WINDOW_OK);
    const long total = (long)B * OH * OW;
    hipLaunchKernelGGL(resample_kernel<false>, dim3((unsigned)cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream, src,
                       H, W, xbounds, xkk, xksize, ybounds, ykk, yksize, (void*)dst, OH, OW, y0, x0, total,
                       flip_channels, 0.f, 0.f, 0.f, 1.f, 1.f, 1.f);
    return gom_launch_status();
}

extern "C" int gom_ingest_crop_u8_hwc3_to_nhwc4(const uint8_t* src, int B, int H, int W, const int* xbounds,
                                                const int* xkk, int xksize, const int* ybounds, const int* ykk,
                                                int yksize, const float* mean3, const float* std3, float* dst, int SH,
                                                int SW, int y0, int x0, int OH, int OW, int flip_channels,
                                                void* stream) {
    GOM_CHECK_ARG(GOM_RESAMPLE_ARGS_OK && GOM_RESAMPLE_WINDOW_OK && mean3 && std3);
    const long total = (long)B * OH * OW;
    hipLaunchKernelGGL(resample_kernel<true>, dim3((unsigned)cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream, src,
                       H, W, xbounds, xkk, xksize, ybounds, ykk, yksize, (void*)dst, OH, OW, y0, x0, total,
                       flip_channels, mean3[0], mean3[1], mean3[2], std3[0], std3[1], std3[2]);
    return gom_launch_status();
}

// One source image, T frames of a GEN_IMAGE_MOTION clip (rule in include/gomatching_hip.h).  Every descriptor is checked on
// the host before any HIP call: the kernel indexes the tables and the source by them.
extern "C" int gom_ingest_motion_u8_hwc3_to_nhwc4(const uint8_t* src, int H, int W, const int* tables, long table_words,
                                                  const int* frames, int T, const float* mean3, const float* std3,
                                                  float* dst, int PH, int PW, int flip_channels, void* stream) {
    GOM_CHECK_ARG(src && tables && frames && mean3 && std3 && dst && H > 0 && W > 0 && table_words > 0);
    GOM_CHECK_ARG(T >= 1 && T <= GOM_INGEST_MOTION_MAX_FRAMES && PH > 0 && PW > 0 && (long)PH * PW <= 0x7fffffffL - 256);
    MotionFrames fr = {};
    for (int t = 0; t < T; ++t) {
        const int* d = frames + (long)t * GOM_INGEST_MOTION_DESC_WORDS;
        const int SH = d[0], SW = d[1], y0 = d[2], x0 = d[3], OH = d[4], OW = d[5], xks = d[6], yks = d[7];
        const long xb = d[8], xk = d[9], yb = d[10], yk = d[11];
        GOM_CHECK_ARG(GOM_RESAMPLE_WINDOW_OK && OH > 0 && OW > 0 && OH <= PH && OW <= PW);
        GOM_CHECK_ARG(xks == gom_resample_ksize_bilinear(W, SW) && yks == gom_resample_ksize_bilinear(H, SH));
        GOM_CHECK_ARG(xb >= 0 && xk >= 0 && yb >= 0 && yk >= 0 && xb + 2L * SW <= table_words &&
                      xk + (long)SW * xks <= table_words && yb + 2L * SH <= table_words &&
                      yk + (long)SH * yks <= table_words);
        fr.f[t] = MotionFrame{y0, x0, OH, OW, xks, yks, (int)xb, (int)xk, (int)yb, (int)yk};
    }
    hipLaunchKernelGGL(motion_kernel, dim3((unsigned)cdiv((long)PH * PW, 256), (unsigned)T), dim3(256), 0,
                       (hipStream_t)stream, src, W, tables, fr, dst, PH, PW, flip_channels, mean3[0], mean3[1], mean3[2],
                       std3[0], std3[1], std3[2]);
    return gom_launch_status();
}
