// Scoring: the pairwise measure between the ground-truth and the detected quadrilaterals of a whole video -- what
// the DSText protocol's `distance_fn` (IoU) and `overlapping_fn` (intersection over the detection's area) compute per pair in a
// Python double loop -- as the count pass and the emit pass of a stream compaction, so that only the pairs above the threshold
// (a few per ground-truth object) travel back to the host's CLEAR-MOT bookkeeping (gomatching_amd/score.py).
//
// Geometry per pair, as tests/score_statement.py states it in numpy float64:
//   * convex hull of each 4-gon: the four points sorted by (x, y), then Andrew's monotone chain with 64-bit integer cross
//     products, popping on cross <= 0 -- any point order is accepted (bow-ties included), duplicate and collinear points
//     collapse.  For four points the chain reduces to: the first and the last sorted point are hull points, each of the two
//     middle points is one when it lies strictly off the line through them, and two on the same side keep the turn convex.
//     The hull lives in FOUR slots, counter-clockwise from the first sorted point, a dropped point's slot repeating a
//     neighbour: a repeated vertex adds nothing to a shoelace sum and is a clip edge that every point is inside of.
//   * either hull without area (twice the area, exact in int64) -> 0.
//   * the detection hull clipped by each edge of the ground-truth hull (Sutherland-Hodgman; inside = cross >= 0; a crossing at
//     prev + t (cur - prev), t = dp / (dp - dc)); at most 4 + 4 = 8 vertices; the shoelace area of the result.
// Arithmetic: fp64, the statement's operations in its order, each rounded once (the pragma keeps hipcc from contracting).
// Side tests are fp64 cross products: exact -- equal to the int64 value -- while the vertex is an integer one below 2^25.
//
// One wave64 per ground-truth object; its lanes stride over the detections of the object's frame.  The clip polygon (up to 8
// vertices, written at a running index) ping-pongs between two per-lane LDS slots [vertex][lane] -- as a private array it
// would be runtime-indexed and go to scratch; hulls and the four clip edges are unrolled over registers.  Counts and write
// positions come from a ballot and a popcount prefix: no atomics, so the output is bitwise reproducible and does not depend
// on the launch geometry.  Offsets, scan and total are device data the host cannot see: every index made from them is clamped.
#include "common.h"

#pragma clang fp contract(off)

#define SC_WAVES 2

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

template <bool EMIT>
__global__ __launch_bounds__(64 * SC_WAVES) void quad_pairs_kernel(
    const int* __restrict__ gt_quads, const int* __restrict__ det_quads, const int* __restrict__ gt_off,
    const int* __restrict__ det_off, const int* __restrict__ gt_key, const int* __restrict__ det_key, int G, int D, int F,
    int measure, double threshold, int* __restrict__ counts, const long long* __restrict__ scan, long long total,
    int* __restrict__ out_det, double* __restrict__ out_val) {
    __shared__ ClipLds lds[SC_WAVES];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const long long gl = (long long)blockIdx.x * SC_WAVES + w;
    if (gl >= G) return;                                               // no barrier below: the LDS slots are per lane
    const int g = (int)gl;
    ClipLds& L = lds[w];

    // the object's frame: the largest f with gt_off[f] <= g
    int lo = 0, hi = F - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (gt_off[mid] <= g) lo = mid;
        else hi = mid - 1;
    }
    int d0 = det_off[lo], d1 = det_off[lo + 1];
    d0 = d0 < 0 ? 0 : (d0 > D ? D : d0);
    d1 = d1 < d0 ? d0 : (d1 > D ? D : d1);
    const int nd = d1 - d0;

    const Hull hg = quad_hull(gt_quads + (long long)g * 8);
    const int kg = gt_key[g];
    int gx0 = hg.x[0], gx1 = hg.x[0], gy0 = hg.y[0], gy1 = hg.y[0];
#pragma unroll
    for (int i = 1; i < 4; ++i) {
        gx0 = min(gx0, hg.x[i]);
        gx1 = max(gx1, hg.x[i]);
        gy0 = min(gy0, hg.y[i]);
        gy1 = max(gy1, hg.y[i]);
    }

    long long pos = EMIT ? scan[g] : 0;
    int kept = 0;
    for (int base = 0; base < nd; base += 64) {
        const int j = base + lane;
        bool keep = false;
        double v = 0.0;
        if (j < nd && det_key[d0 + j] == kg) {
            const Hull hd = quad_hull(det_quads + (long long)(d0 + j) * 8);
            int dx0 = hd.x[0], dx1 = hd.x[0], dy0 = hd.y[0], dy1 = hd.y[0];
#pragma unroll
            for (int i = 1; i < 4; ++i) {
                dx0 = min(dx0, hd.x[i]);
                dx1 = max(dx1, hd.x[i]);
                dy0 = min(dy0, hd.y[i]);
                dy1 = max(dy1, hd.y[i]);
            }
            // bounding boxes that do not meet: the intersection is empty, the value 0 (never above a positive threshold)
            if (dx0 <= gx1 && gx0 <= dx1 && dy0 <= gy1 && gy0 <= dy1) v = pair_value(hg, hd, measure, L, lane);
            keep = v > threshold;
        }
        const unsigned long long b = __ballot(keep);
        if (EMIT) {
            const long long p = pos + __popcll(b & ((1ull << lane) - 1ull));
            if (keep && p >= 0 && p < total) {
                out_det[p] = j;
                out_val[p] = v;
            }
            pos += __popcll(b);
        } else {
            kept += __popcll(b);
        }
    }
    if (!EMIT && lane == 0) counts[g] = kept;
}

int check_args(const void* gt_quads, const void* det_quads, const void* gt_off, const void* det_off, const void* gt_key,
               const void* det_key, int G, int D, int F, long pairs, int measure, double threshold) {
    GOM_CHECK_ARG(G >= 0 && D >= 0 && F >= 0);
    GOM_CHECK_ARG(F > 0 || (G == 0 && D == 0));
    GOM_CHECK_ARG(measure == 0 || measure == 1);
    GOM_CHECK_ARG(threshold > 0.0 && threshold < 1.0);                 // (a NaN fails both)
    GOM_CHECK_ARG(pairs >= 0 && pairs <= 2147483647L && pairs <= (long)G * (long)D);
    if (F > 0) GOM_CHECK_ARG(gt_off && det_off);
    if (G > 0) GOM_CHECK_ARG(gt_quads && gt_key);
    if (D > 0) GOM_CHECK_ARG(det_quads && det_key);
    return GOM_OK;
}

}  // namespace

extern "C" int gom_quad_pairs_count_f64(const int32_t* gt_quads, const int32_t* det_quads, const int32_t* gt_off,
                                        const int32_t* det_off, const int32_t* gt_key, const int32_t* det_key, int G, int D,
                                        int F, long pairs, int measure, double threshold, int32_t* counts, void* stream) {
    const int rc = check_args(gt_quads, det_quads, gt_off, det_off, gt_key, det_key, G, D, F, pairs, measure, threshold);
    if (rc != GOM_OK) return rc;
    if (G == 0) return GOM_OK;
    GOM_CHECK_ARG(counts);
    hipLaunchKernelGGL(quad_pairs_kernel<false>, dim3((unsigned)cdiv((long)G, (long)SC_WAVES)), dim3(64 * SC_WAVES), 0,
                       (hipStream_t)stream, gt_quads, det_quads, gt_off, det_off, gt_key, det_key, G, D, F, measure, threshold,
                       (int*)counts, (const long long*)nullptr, 0LL, (int*)nullptr, (double*)nullptr);
    return gom_launch_status();
}

extern "C" int gom_quad_pairs_emit_f64(const int32_t* gt_quads, const int32_t* det_quads, const int32_t* gt_off,
                                       const int32_t* det_off, const int32_t* gt_key, const int32_t* det_key, int G, int D,
                                       int F, long pairs, int measure, double threshold, const int64_t* scan, long total,
                                       int32_t* out_det, double* out_val, void* stream) {
    const int rc = check_args(gt_quads, det_quads, gt_off, det_off, gt_key, det_key, G, D, F, pairs, measure, threshold);
    if (rc != GOM_OK) return rc;
    GOM_CHECK_ARG(total >= 0 && total <= pairs);
    if (G == 0 || total == 0) return GOM_OK;
    GOM_CHECK_ARG(scan && out_det && out_val);
    hipLaunchKernelGGL(quad_pairs_kernel<true>, dim3((unsigned)cdiv((long)G, (long)SC_WAVES)), dim3(64 * SC_WAVES), 0,
                       (hipStream_t)stream, gt_quads, det_quads, gt_off, det_off, gt_key, det_key, G, D, F, measure, threshold,
                       (int*)nullptr, (const long long*)scan, (long long)total, (int*)out_det, (double*)out_val);
    return gom_launch_status();
}
