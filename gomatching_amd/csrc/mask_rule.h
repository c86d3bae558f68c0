// Device helpers of the bit-row masks (representation and rasterisation rule: include/gomatching_hip.h), shared by
// csrc/mask_pairs.hip (scoring) and csrc/overlay.hip (drawing): index clamps, a mask's box, bit ranges of a 32-pixel word and the
// closed form of Boundary for one edge on one row.
#pragma once
#include "common.h"

namespace {

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
__device__ __forceinline__ long long clampl(long long v, long long lo, long long hi) { return v < lo ? lo : (v > hi ? hi : v); }

// bits [lo, hi] of a word (pixel offsets relative to the word's first pixel; any range)
__device__ __forceinline__ unsigned bit_range(long long lo, long long hi) {
    if (hi < 0 || lo > 31 || lo > hi) return 0u;
    const int l = lo < 0 ? 0 : (int)lo, h = hi > 31 ? 31 : (int)hi;
    return (0xffffffffu >> (31 - h)) & (0xffffffffu << l);
}

// floor(a / b), b > 0
__device__ __forceinline__ long long floor_div(long long a, long long b) {
    long long q = a / b;
    if ((a % b) < 0) --q;
    return q;
}

struct Box {
    int y0, y1, wx0, wx1;
};

// a mask's box, made consistent with the image and with the words the caller allotted to it
__device__ __forceinline__ Box load_box(const int* __restrict__ boxes, int k, int H, int W) {
    const int4 b = *reinterpret_cast<const int4*>(boxes + 4 * (long long)k);
    Box r;
    const int NWI = (W + 31) >> 5;
    r.y0 = clampi(b.x, 0, H);
    r.y1 = clampi(b.y, r.y0, H);
    r.wx0 = clampi(b.z, 0, NWI);
    r.wx1 = clampi(b.w, r.wx0, NWI);
    return r;
}

// Boundary of the edge (xa, ya) - (xb, yb) on row y, as bits of the word whose first pixel is px0: the line from the left end
// point to the right one.  Step k of the error-stepped line sits at the minor offset (2 m k + M - 1) / (2 M), so an x-major
// edge covers on its row j the steps ceil((2 M j - M + 1) / (2 m)) .. floor((2 M j + M) / (2 m)) -- a bit range -- and a
// y-major edge one pixel per row.
__device__ __forceinline__ unsigned boundary_bits(long long xa, long long ya, long long xb, long long yb, long long y,
                                                  long long px0) {
    const bool sw = xb < xa;
    const long long x0 = sw ? xb : xa, y0 = sw ? yb : ya, x1 = sw ? xa : xb, y1 = sw ? ya : yb;
    const long long dx = x1 - x0, dy = y1 - y0, ady = dy < 0 ? -dy : dy;
    const long long M = dx > ady ? dx : ady, m = dx > ady ? ady : dx;
    const long long j = dy < 0 ? y0 - y : y - y0;                                // the row's step along y
    if (ady > dx) {                                                              // y-major: one pixel per row
        if (j >= 0 && j <= M) {
            const long long x = x0 + (2 * m * j + M - 1) / (2 * M);
            return bit_range(x - px0, x - px0);
        }
    } else if (j >= 0 && j <= m) {                                               // x-major: a run of steps
        long long klo = 0, khi = M;
        if (m > 0) {
            klo = -floor_div(-(2 * M * j - M + 1), 2 * m);                       // ceil
            khi = floor_div(2 * M * j + M, 2 * m);
            if (klo < 0) klo = 0;
            if (khi > M) khi = M;
        }
        return bit_range(x0 + klo - px0, x0 + khi - px0);
    }
    return 0u;
}

}  // namespace
