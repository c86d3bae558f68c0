// The geometry of one (ground truth, detection) pair of convex quadrilaterals, shared by the scoring kernels (score.hip: the
// pair compaction; score_det.hip: the detection protocol's matching).  The rule is stated in score.hip's header and, in
// numpy float64, in tests/score_statement.py; both kernels include the SAME device functions so that a pair has the same bits
// in either.  fp64, the statement's operations in its order, each rounded once: the pragma below keeps hipcc from
// contracting, and it covers the including file from here on.
#pragma once
#include "common.h"

#pragma clang fp contract(off)

namespace {

struct ClipLds {
    double x[2][8][64];
    double y[2][8][64];
};

struct Hull {
    int x[4], y[4];      // counter-clockwise from the first sorted point; a dropped point's slot repeats a neighbour
    long long area2;     // twice the area (>= 0)
};

__device__ __forceinline__ long long cross_i(int ox, int oy, int ax, int ay, int bx, int by) {
    return (long long)(ax - (long long)ox) * (by - (long long)oy) - (long long)(ay - (long long)oy) * (bx - (long long)ox);
}

__device__ __forceinline__ void sort2(long long& a, long long& b) {
    const long long lo = a < b ? a : b, hi = a < b ? b : a;
    a = lo;
    b = hi;
}

__device__ __forceinline__ Hull quad_hull(const int* __restrict__ q) {
    const int4 a = *reinterpret_cast<const int4*>(q), b = *reinterpret_cast<const int4*>(q + 4);
    // (x, y) as one ordered 64-bit key: x in the high word, y with its sign bit flipped in the low word
    auto key = [](int x, int y) { return (long long)(((unsigned long long)(unsigned)x << 32) | ((unsigned)y ^ 0x80000000u)); };
    long long k0 = key(a.x, a.y), k1 = key(a.z, a.w), k2 = key(b.x, b.y), k3 = key(b.z, b.w);
    sort2(k0, k1);
    sort2(k2, k3);
    sort2(k0, k2);
    sort2(k1, k3);
    sort2(k1, k2);
    auto kx = [](long long k) { return (int)(k >> 32); };
    auto ky = [](long long k) { return (int)((unsigned)(unsigned long long)k ^ 0x80000000u); };
    const int x0 = kx(k0), y0 = ky(k0), x1 = kx(k1), y1 = ky(k1), x2 = kx(k2), y2 = ky(k2), x3 = kx(k3), y3 = ky(k3);
    const long long c1 = cross_i(x0, y0, x3, y3, x1, y1), c2 = cross_i(x0, y0, x3, y3, x2, y2);
    bool l1 = c1 < 0, l2 = c2 < 0, u1 = c1 > 0, u2 = c2 > 0;          // below (lower chain) / above (upper chain) the line p0 -> p3
    if (l1 && l2) {
        if (cross_i(x0, y0, x1, y1, x2, y2) <= 0) l1 = false;
        else if (cross_i(x1, y1, x2, y2, x3, y3) <= 0) l2 = false;
    }
    if (u1 && u2) {
        if (cross_i(x3, y3, x2, y2, x1, y1) <= 0) u2 = false;
        else if (cross_i(x2, y2, x1, y1, x0, y0) <= 0) u1 = false;
    }
    Hull h;                                                            // p0, [p1], [p2], p3, [p2], [p1] in four slots
    h.x[0] = x0;
    h.y[0] = y0;
    h.x[1] = l1 ? x1 : (l2 ? x2 : x3);
    h.y[1] = l1 ? y1 : (l2 ? y2 : y3);
    h.x[2] = l1 ? (l2 ? x2 : x3) : (l2 ? x3 : (u2 ? x2 : (u1 ? x1 : x3)));
    h.y[2] = l1 ? (l2 ? y2 : y3) : (l2 ? y3 : (u2 ? y2 : (u1 ? y1 : y3)));
    h.x[3] = u1 ? x1 : (u2 ? x2 : x3);
    h.y[3] = u1 ? y1 : (u2 ? y2 : y3);
    long long s = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int j = (i + 1) & 3;
        s += (long long)h.x[i] * h.y[j] - (long long)h.x[j] * h.y[i];
    }
    h.area2 = s;
    return h;
}

// value of one pair: `g` the ground-truth hull (wave-uniform), `d` this lane's detection hull
__device__ __forceinline__ double pair_value(const Hull& g, const Hull& d, int measure, ClipLds& L, int lane) {
    if (g.area2 <= 0 || d.area2 <= 0) return 0.0;
    int n = 4, cur_buf = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        L.x[0][i][lane] = (double)d.x[i];
        L.y[0][i][lane] = (double)d.y[i];
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int e1 = (e + 1) & 3;
        if (g.x[e] == g.x[e1] && g.y[e] == g.y[e1]) continue;         // a repeated vertex: no edge
        if (n == 0) break;
        const double ax = (double)g.x[e], ay = (double)g.y[e];
        const double ex = (double)g.x[e1] - ax, ey = (double)g.y[e1] - ay;
        const int nb = cur_buf ^ 1;
        double px = L.x[cur_buf][n - 1][lane], py = L.y[cur_buf][n - 1][lane];
        double dp = ex * (py - ay) - ey * (px - ax);
        int m = 0;
        for (int i = 0; i < n; ++i) {
            const double cx = L.x[cur_buf][i][lane], cy = L.y[cur_buf][i][lane];
            const double dc = ex * (cy - ay) - ey * (cx - ax);
            if ((dc >= 0) != (dp >= 0)) {
                const double t = dp / (dp - dc);
                if (m < 8) {
                    L.x[nb][m][lane] = px + t * (cx - px);
                    L.y[nb][m][lane] = py + t * (cy - py);
                }
                ++m;
            }
            if (dc >= 0) {
                if (m < 8) {
                    L.x[nb][m][lane] = cx;
                    L.y[nb][m][lane] = cy;
                }
                ++m;
            }
            px = cx;
            py = cy;
            dp = dc;
        }
        n = m < 8 ? m : 8;
        cur_buf = nb;
    }
    if (n < 3) return 0.0;
    double s = 0.0;
    double px = L.x[cur_buf][n - 1][lane], py = L.y[cur_buf][n - 1][lane];
    for (int i = 0; i < n; ++i) {
        const double cx = L.x[cur_buf][i][lane], cy = L.y[cur_buf][i][lane];
        s += px * cy - cx * py;
        px = cx;
        py = cy;
    }
    const double inter = fabs(s) * 0.5;
    const double ag = (double)g.area2 * 0.5, ad = (double)d.area2 * 0.5;
    if (measure == 1) return inter / ad;
    const double uni = ag + ad - inter;
    return uni == 0 ? 0.0 : inter / uni;
}

// the hull's bounding box (the four slots hold every hull point)
struct HullBox {
    int x0, x1, y0, y1;
};

__device__ __forceinline__ HullBox hull_box(const Hull& h) {
    HullBox b = {h.x[0], h.x[0], h.y[0], h.y[0]};
#pragma unroll
    for (int i = 1; i < 4; ++i) {
        b.x0 = min(b.x0, h.x[i]);
        b.x1 = max(b.x1, h.x[i]);
        b.y0 = min(b.y0, h.y[i]);
        b.y1 = max(b.y1, h.y[i]);
    }
    return b;
}

}  // namespace
